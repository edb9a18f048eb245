"""Times ops.detect_curved_u8 against the plain ops.detect_text_u8 (csrc/detect.hip) in the same process on the same photos: B = 8 of
2400 x 1600 and B = 48 of 640 x 480, seeded, with rows of word-sized blocks of letter-sized strokes, every second row bowed.  Warm-up,
then repeated timed calls of the two ops in turn (each ends with a synchronous copy to the host); median, minimum and the quartiles of
each, and the ratio of the medians.  Also timed: the curved op without its host tail (ribbons, filters, sort), and the profile kernel
alone, between events, on the maps of the row pass with the bins that the op uploads.  Writes one JSON object (default
profiles/detect_curved_bench.json).

    python tools/bench_detect_curved.py [--out FILE] [--repeat N]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETS = ((8, 1600, 2400), (48, 480, 640))      # (photos, height, width)


def photos(n, h, w, seed=0):
    """Seeded photos with text-like content, as tools/bench_detect.py draws them; the words of every second row rise and fall with a
    parabola of up to 20 pixels over the word."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        a = np.full((h, w), 200, np.int64)
        for j, y in enumerate(range(30, h - 60, 64)):
            x = 20 + rng.randint(0, 30)
            while x < w - 260:
                wd = rng.randint(40, 240)
                sag = rng.randint(8, 21) * (1 if rng.rand() < 0.5 else -1) if j % 2 else 0
                for sx in range(x, x + wd, 9):
                    t = 2.0 * (sx - x) / wd - 1.0
                    dy = int(round(sag * (1.0 - t * t)))
                    a[y + dy + rng.randint(0, 6):y + dy + 24, sx:sx + 5] = 40 + rng.randint(0, 40)
                x += wd + rng.randint(18, 40)
        a = a[:, :, None] + rng.randint(-4, 5, (h, w, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_curved_bench.json"))
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dpmn_amd import _abi, ops
    from dpmn_amd.utils import detect, resize
    assert torch.cuda.is_available(), "bench_detect_curved needs a GPU"
    dev = torch.device("cuda:0")
    sets = []
    for n, h, w in SETS:
        packed, meta = resize.pack_ragged(photos(n, h, w))
        packed = packed.to(dev)
        off, sizes = meta[:, 0], meta[:, 1:]
        plain = lambda: ops.detect_text_u8(packed, off, sizes)
        curved = lambda: ops.detect_curved_u8(packed, off, sizes)
        boxes, regions = plain(), curved()
        for _ in range(args.warmup):
            plain()
            curved()
        torch.cuda.synchronize()
        t_pl, t_cu = [], []
        for _ in range(args.repeat):      # in turn: drift of the clocks or of the host touches both alike
            for fn, ts in ((plain, t_pl), (curved, t_cu)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        # where the curved time goes: the launches, copies and bins (_detect_curved_run) against the host's ribbons, filters and sort
        t_run = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            ops._detect_curved_run(packed, off, sizes, 12, 2, 24, "bench")
            t_run.append((time.perf_counter() - t0) * 1e3)
        # the host's bins alone (utils.detect.curve_candidates over the component tables)
        host = ops._detect_plan(packed, off, sizes)
        d, d_items, d_tiles, g, hist, thr = ops._detect_thresholds(packed, host, 24)
        p = ops._detect_pass(host, d_items, d_tiles, g, thr, 12, 2)
        comps = ops._detect_comps(p)
        t_bins = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            cands = [detect.curve_candidates(c) for c in comps]
            t_bins.append((time.perf_counter() - t0) * 1e3)
        # the new kernel alone (with the initialisation of its table), between events, on the row pass's maps
        a, slices, d_slices, rows = ops._detect_oriented_args(host, d_items, d_tiles, p)
        bins = np.ascontiguousarray(np.concatenate(cands).astype(np.int32))
        d_bins = torch.from_numpy(bins).to(dev)
        prof = torch.empty(rows, 16, 4, dtype=torch.int32, device=dev)
        ts = []
        for i in range(args.warmup + args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _abi.check(_abi.lib.dpmn_detect_profile_i32(*a, d_bins.data_ptr(), prof.data_ptr(), rows, _abi.stream()))
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        sets.append(dict(photos=n, shape=[h, w], plain_boxes=int(sum(len(b) for b in boxes)), curved_regions=int(sum(len(r) for r in regions)),
                         curved_polygons=int(sum(len(q) > 4 for r in regions for q in r)), components=int(p["counts"].sum()),
                         candidates=int((bins[:, 2] > 0).sum()), profile_table_bytes=int(rows) * 16 * 4 * 4,
                         plain_ms=stats(t_pl), curved_ms=stats(t_cu), ratio_of_medians=round(statistics.median(t_cu) / statistics.median(t_pl), 3),
                         extra_ms_of_medians=round(statistics.median(t_cu) - statistics.median(t_pl), 4),
                         launches_copies_bins_ms=stats(t_run), host_bins_ms=stats(t_bins), profile_kernel_and_init_ms=stats(ts)))
    res = dict(bench="detect_curved_u8 against detect_text_u8", sets=sets, repeat=args.repeat, warmup=args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
