"""Times ops.region_overlap_counts (csrc/detect_eval.hip) on seeded synthetic region sets: 8 photos of 2400 x 1600 with about 100
detected and 60 ground-truth quads each, and 48 photos of 640 x 480 whose ground truth is 14-point polygons.  Per set, medians of
--repeat calls in one run: the whole op (host plan, one upload, two launches, one copy back; a host clock around the call, which ends
with the synchronous copy), its host plan alone, its two launches alone between events, a brute-force torch formulation on the same
device (per region and per pair a sample grid and boolean masks from the definition's cross products, one copy back at the end), and
the NumPy restatement on the host (3 calls; for scale).  The three results are compared with == before anything is timed.  Writes one JSON object
(default profiles/detect_eval_bench.json).

    python tools/bench_detect_eval.py [--out FILE] [--repeat N]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _turned(cx, cy, w, h, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    p = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]], np.float64)
    return np.stack([cx + c * p[:, 0] - s * p[:, 1], cy + s * p[:, 0] + c * p[:, 1]], axis=1)


def _arc(cx, cy, r, h, a0, a1):
    ang = np.radians(np.linspace(a0, a1, 7))
    top = np.stack([cx + (r + h) * np.cos(ang), cy + (r + h) * np.sin(ang)], axis=1)
    bot = np.stack([cx + r * np.cos(ang[::-1]), cy + r * np.sin(ang[::-1])], axis=1)
    return np.concatenate([top, bot])


def region_set(photos, H, W, n_gt, n_extra, polygons, seed):
    """Per photo n_gt ground-truth regions (quads, or 14-point arcs) and, as detections, a jittered quad over most of them plus n_extra
    quads elsewhere -> (detections, ground truth), lists per photo of (n, 2) arrays."""
    rng = np.random.RandomState(seed)
    scale = W / 640.0
    dets, gts = [], []
    for _ in range(photos):
        gt, det = [], []
        for _ in range(n_gt):
            cx, cy, w, h, deg = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(30, 120) * scale, rng.uniform(8, 24) * scale, rng.uniform(-25, 25)
            gt.append(_arc(cx, cy + w, w, h, 250, 290) if polygons else _turned(cx, cy, w, h, deg))
            if rng.rand() < 0.8:
                det.append(_turned(cx + rng.uniform(-3, 3), cy + rng.uniform(-3, 3), w * rng.uniform(0.8, 1.2), h * rng.uniform(0.8, 1.3),
                                   0.0 if polygons else deg + rng.uniform(-4, 4)))
        for _ in range(n_extra):
            det.append(_turned(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(30, 120) * scale, rng.uniform(8, 24) * scale, rng.uniform(-25, 25)))
        dets.append(det)
        gts.append(gt)
    return dets, gts


SETS = (dict(name="quads", photos=8, H=1600, W=2400, n_gt=60, n_extra=52, polygons=False, seed=1),
        dict(name="polygons", photos=48, H=480, W=640, n_gt=10, n_extra=6, polygons=True, seed=2))


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4))


def torch_counts(plan, dev):
    """The brute force on the device: the plan's tables uploaded once, then per region and per pair the samples of the box as a grid,
    the definition's cross product per sample and edge, a boolean mask per region and its sum -> int64 (R + P) on the host."""
    import torch
    from dpmn_amd.utils import detect_eval as de
    o_v, o_r, o_p = plan["offsets"][:3]
    host = plan["host"]
    verts = torch.from_numpy(host[o_v:].view(np.int32)[:2 * plan["n_verts"]].astype(np.int64).reshape(-1, 2)).to(dev)
    table = host[o_r:].view(np.int32)[:8 * plan["R"]].reshape(-1, 8)
    pairs = host[o_p:].view(np.int32)[:2 * plan["P"]].reshape(-1, 2)

    def inside(r, box):
        u = verts[table[r, 0]:table[r, 0] + table[r, 1]]
        x0, y0 = u[:, 0], u[:, 1]
        x1, y1 = torch.roll(x0, -1), torch.roll(y0, -1)
        ys = de.STEP * torch.arange(de.SUB * box[1], de.SUB * box[3], device=dev) + de.STEP // 2
        xs = de.STEP * torch.arange(de.SUB * box[0], de.SUB * box[2], device=dev) + de.STEP // 2
        cr = (y0[:, None] > ys[None, :]) != (y1[:, None] > ys[None, :])
        dy = (y1 - y0)[:, None, None]
        cross = ((x1 - x0)[:, None] * (ys[None, :] - y0[:, None]))[:, :, None] - (xs[None, None, :] - x0[:, None, None]) * dy
        right = torch.where(dy > 0, cross > 0, cross < 0)
        return ((cr[:, :, None] & right).sum(0) & 1).bool()

    out = torch.zeros(plan["R"] + plan["P"], dtype=torch.int64, device=dev)
    for r in range(plan["R"]):
        if table[r, 2] < table[r, 4] and table[r, 3] < table[r, 5]:
            out[r] = inside(r, table[r, 2:6]).sum()
    for p, (a, b) in enumerate(pairs.tolist()):
        box = (max(table[a, 2], table[b, 2]), max(table[a, 3], table[b, 3]), min(table[a, 4], table[b, 4]), min(table[a, 5], table[b, 5]))
        out[plan["R"] + p] = (inside(a, box) & inside(b, box)).sum()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_eval_bench.json"))
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from dpmn_amd import ops
    from dpmn_amd.utils import detect_eval as de
    assert torch.cuda.is_available(), "bench_detect_eval needs a GPU"
    dev = torch.device("cuda:0")
    sets = []
    for cfg in SETS:
        dets, gts = region_set(**{k: v for k, v in cfg.items() if k != "name"})
        plan = ops._region_plan(dets, gts)
        op = lambda: ops.region_overlap_counts(dets, gts, dev)
        brute = lambda: torch_counts(ops._region_plan(dets, gts), dev)
        got = op()
        flat = np.concatenate([np.concatenate([g[0], g[1]]) for g in got] + [g[3] for g in got]).astype(np.int64)
        t0 = time.perf_counter()
        want = de.region_counts_batch_np(dets, gts)
        t_np = [(time.perf_counter() - t0) * 1e3]
        for g, w in zip(got, want):
            assert all(np.array_equal(x, y) for x, y in zip(g, w)), "the op and the restatement disagree"
        assert np.array_equal(brute(), flat), "the torch brute force and the op disagree"
        for _ in range(2):
            t0 = time.perf_counter()
            de.region_counts_batch_np(dets, gts)
            t_np.append((time.perf_counter() - t0) * 1e3)
        for _ in range(args.warmup):
            op()
        t_op, t_brute, t_plan = [], [], []
        for _ in range(args.repeat):      # in turn: drift of the clocks or of the host touches both alike
            for fn, ts in ((op, t_op), (brute, t_brute)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ops._region_plan(dets, gts)
            t_plan.append((time.perf_counter() - t0) * 1e3)
        # the two launches alone, between events
        d = torch.from_numpy(plan["host"]).to(dev)
        out = torch.empty(plan["R"] + plan["P"], dtype=torch.int64, device=dev)
        t_k = []
        for i in range(args.warmup + args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops._region_launch(plan, d, out)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                t_k.append(e0.elapsed_time(e1))
        sets.append(dict(name=cfg["name"], photos=cfg["photos"], shape=[cfg["H"], cfg["W"]], detections=sum(len(x) for x in dets),
                         ground_truth=sum(len(x) for x in gts), pairs=plan["P"], area_blocks=plan["n_area_units"],
                         pair_blocks=plan["n_pair_units"], upload_bytes=int(plan["host"].nbytes), op_ms=stats(t_op), host_plan_ms=stats(t_plan),
                         two_launches_ms=stats(t_k), torch_brute_force_ms=stats(t_brute), numpy_restatement_ms=round(statistics.median(t_np), 2),
                         brute_force_over_op=round(statistics.median(t_brute) / statistics.median(t_op), 2)))
    res = dict(bench="region_overlap_counts against a torch brute force and the NumPy restatement", sets=sets, repeat=args.repeat,
               warmup=args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
