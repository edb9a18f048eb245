"""Times ops.detect_text_u8 (csrc/detect.hip) on a batch of 8 seeded 768 x 1024 photos against the host restatement (numpy plus
scipy.ndimage.label) in the same process, and the gradient launch alone against its HBM floor (photo bytes read once plus map bytes
written).  Warm-up, then the median of repeated timed calls; one process.  Writes one JSON object (default profiles/detect_bench.json).

    python tools/bench_detect.py [--out FILE] [--repeat N]
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

HBM_GBS = 8000.0      # MI355X peak HBM3E bandwidth, GB/s


def photos(n=8, h=768, w=1024, seed=0):
    """Seeded photos with text-like content: a grainy light ground and rows of dark word-sized blocks of letter-sized strokes."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        a = np.full((h, w), 200, np.int64)
        for y in range(20, h - 40, 48):
            x = 20 + rng.randint(0, 30)
            while x < w - 160:
                wd = rng.randint(40, 150)
                for sx in range(x, x + wd, 9):
                    a[y + rng.randint(0, 6):y + 24, sx:sx + 5] = 40 + rng.randint(0, 40)
                x += wd + rng.randint(18, 40)
        a = a[:, :, None] + rng.randint(-4, 5, (h, w, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def host_detect(photo):
    """The restatement with scipy's labelling in the place of its own union-find: the fastest honest host version."""
    from scipy import ndimage
    from dpmn_amd.utils import detect
    g, hist = detect.gradient(detect.luma_map(photo))
    s = detect.smooth(g >= detect.threshold(hist), detect.GAP, detect.VGAP)
    lab, n = ndimage.label(s, structure=np.ones((3, 3)))
    comps = [[sl[1].start, sl[0].start, sl[1].stop, sl[0].stop, int((lab[sl] == k).sum())] for k, sl in enumerate(ndimage.find_objects(lab), 1)]
    return detect.boxes_from_components(np.array(comps, np.int64).reshape(-1, 5), photo.shape[0], photo.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dpmn_amd import ops
    from dpmn_amd.utils import resize
    assert torch.cuda.is_available(), "bench_detect needs a GPU"
    dev = torch.device("cuda:0")
    imgs = photos()
    packed, meta = resize.pack_ragged(imgs)
    packed = packed.to(dev)
    off, sizes = meta[:, 0], meta[:, 1:]

    def run():
        return ops.detect_text_u8(packed, off, sizes)

    boxes = run()
    ref = [host_detect(p) for p in imgs]
    same = all(np.array_equal(a, b) for a, b in zip(boxes, ref))
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        run()      # (ends with the copy of the component tables: synchronous)
        times.append((time.perf_counter() - t0) * 1e3)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for p in imgs:
            host_detect(p)
        host.append((time.perf_counter() - t0) * 1e3)
    # the gradient launch alone, between events
    plan = ops._detect_plan(packed, off, sizes)
    d, d_items, d_tiles = ops._upload(dev, plan["items"], plan["tiles"])
    for _ in range(args.warmup):
        ops._detect_gradient(packed, plan, d_items, d_tiles)
    grad = []
    for _ in range(args.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops._detect_gradient(packed, plan, d_items, d_tiles)
        e1.record()
        e1.synchronize()
        grad.append(e0.elapsed_time(e1))
    nbytes = packed.numel() + plan["map_px"]
    grad_ms = statistics.median(grad)
    floor_ms = nbytes / (HBM_GBS * 1e9) * 1e3
    res = dict(bench="detect_text_u8", photos=len(imgs), shape=[768, 1024], boxes=[int(len(b)) for b in boxes], boxes_equal_host=bool(same),
               gpu_ms_median=round(statistics.median(times), 4), gpu_ms_min=round(min(times), 4), host_ms_median=round(statistics.median(host), 2),
               speedup=round(statistics.median(host) / statistics.median(times), 1), gradient_ms_median=round(grad_ms, 5),
               gradient_bytes=int(nbytes), gradient_hbm_floor_ms=round(floor_ms, 5), gradient_fraction_of_floor=round(floor_ms / grad_ms, 4),
               hbm_gbs_assumed=HBM_GBS, repeat=args.repeat, warmup=args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
