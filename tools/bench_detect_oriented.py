"""Times ops.detect_oriented_u8 against the upright ops.detect_text_u8 (csrc/detect.hip) in the same process on the same photos: B = 8
of 2400 x 1600 and B = 48 of 640 x 480, seeded, with rows of word-sized blocks of letter-sized strokes, every second photo slanted.
Warm-up, then repeated timed calls of the two ops in turn (each ends with a synchronous copy to the host); median, minimum and the
quartiles of each, and the ratio of the medians.  Also timed: the oriented op without its host tail (filters, cross-pass rule, corners,
sort), and the two oriented kernels alone, between events, on the maps of the row pass with the directions that the op uploads.  Writes one JSON object (default profiles/detect_oriented_bench.json).

    python tools/bench_detect_oriented.py [--out FILE] [--repeat N]
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
    """Seeded photos with text-like content, as tools/bench_detect.py draws them; every second photo is turned by 5 .. 35 degrees."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        a = np.full((h, w), 200, np.int64)
        for y in range(20, h - 40, 48):
            x = 20 + rng.randint(0, 30)
            while x < w - 160:
                wd = rng.randint(40, 150)
                for sx in range(x, x + wd, 9):
                    a[y + rng.randint(0, 6):y + 24, sx:sx + 5] = 40 + rng.randint(0, 40)
                x += wd + rng.randint(18, 40)
        if i % 2:
            a = np.asarray(Image.fromarray(a.astype(np.uint8)).rotate(int(rng.randint(5, 36)), resample=Image.BICUBIC, fillcolor=200), np.int64)
        a = a[:, :, None] + rng.randint(-4, 5, (h, w, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_oriented_bench.json"))
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dpmn_amd import _abi, ops
    from dpmn_amd.utils import resize
    assert torch.cuda.is_available(), "bench_detect_oriented needs a GPU"
    dev = torch.device("cuda:0")
    sets = []
    for n, h, w in SETS:
        packed, meta = resize.pack_ragged(photos(n, h, w))
        packed = packed.to(dev)
        off, sizes = meta[:, 0], meta[:, 1:]
        upright = lambda: ops.detect_text_u8(packed, off, sizes)
        oriented = lambda: ops.detect_oriented_u8(packed, off, sizes)
        boxes, quads = upright(), oriented()
        for _ in range(args.warmup):
            upright()
            oriented()
        torch.cuda.synchronize()
        t_up, t_or = [], []
        for _ in range(args.repeat):      # in turn: drift of the clocks or of the host touches both alike
            for fn, ts in ((upright, t_up), (oriented, t_or)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        # where the oriented time goes: the launches, copies and directions (_detect_oriented_run) against the host's filters, cross-pass
        # rule, corners and sort (the rest of detect_oriented_u8)
        t_run = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            ops._detect_oriented_run(packed, off, sizes, 12, 2, 24, "bench")
            t_run.append((time.perf_counter() - t0) * 1e3)
        # the two new kernels alone, between events, on the row pass's maps, the extents with the directions that the op uploads
        host = ops._detect_plan(packed, off, sizes)
        d, d_items, d_tiles, g, hist, thr = ops._detect_thresholds(packed, host, 24)
        p = ops._detect_pass(host, d_items, d_tiles, g, thr, 12, 2)
        a, slices, d_slices, rows = ops._detect_oriented_args(host, d_items, d_tiles, p)
        tables, dirs = ops._detect_dirs(ops._detect_comps(p), ops._detect_moments(a, rows, dev), slices)
        mom = torch.empty(rows, 5, dtype=torch.int64, device=dev)
        ext = torch.empty(rows, 4, dtype=torch.int32, device=dev)
        d_dirs = torch.from_numpy(dirs).to(dev)
        kernels, lib = {}, _abi.lib
        for name, call in (("moments", lambda: lib.dpmn_detect_moments_i64(*a, mom.data_ptr(), rows, _abi.stream())),
                           ("extents", lambda: lib.dpmn_detect_extents_i32(*a, d_dirs.data_ptr(), ext.data_ptr(), rows, _abi.stream()))):
            ts = []
            for i in range(args.warmup + args.repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _abi.check(call())
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ts.append(e0.elapsed_time(e1))
            kernels[name + "_ms"] = stats(ts)
        kernels.update(launches_copies_directions_ms=stats(t_run), components_with_a_direction=int((dirs != 0).any(axis=1).sum()))
        sets.append(dict(photos=n, shape=[h, w], upright_boxes=int(sum(len(b) for b in boxes)), oriented_quads=int(sum(len(q) for q in quads)),
                         components_row_pass=int(p["counts"].sum()), upright_ms=stats(t_up), oriented_ms=stats(t_or),
                         ratio_of_medians=round(statistics.median(t_or) / statistics.median(t_up), 3), **kernels))
    res = dict(bench="detect_oriented_u8 against detect_text_u8", sets=sets, repeat=args.repeat, warmup=args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
