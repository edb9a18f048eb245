#!/usr/bin/env python3
"""What the JPEG stage of the synthesised LR images costs on one MI355X and on the host: prints ONE JSON line.

Per shape (B x h x w: 48 and 64 of 16 x 64, the training shapes, and 96 of 64 x 256), glyph-like images, qualities 30 .. 95:
  kernel_us   -- csrc/jpeg.hip alone: dpmn_jpeg_roundtrip_u8 with the qualities and the workspace already on the device, HIP events
                 around --kernel-reps back-to-back calls (both launches of a call; three windows, the median)
  op_call_us  -- ops.jpeg_roundtrip_u8 with a host list of qualities (its B-int32 upload, the workspace and output allocations, both
                 launches), the same way
  pil_1t_ms   -- PIL's save + open of the same batch, one image after the other on one thread (median of --host-reps)
  pil_16t_ms  -- the same over a pool of 16 threads (PIL releases the GIL in the codec)
and for the loader, B = 48 HR images in the sizes of tools/bench_resize.py:
  loader_off_ms / loader_on_ms -- degrade_on_gpu from the packed host batch to the two float batches, jpeg=None against
                 jpeg=(30, 95, 0.5), alternating in the same run, wall clock ending in a device synchronise, medians
The GPU bytes are compared with PIL's before anything is timed.  The measurement runs in a child process under a time limit of its
own (--timeout seconds); the parent never opens the GPU."""
import argparse
import io
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = ((48, 16, 64), (64, 16, 64), (96, 64, 256))


def glyph_batch(B, h, w, seed=0):
    import numpy as np
    rng = np.random.RandomState(seed)
    out = np.empty((B, h, w, 3), np.uint8)
    for b in range(B):
        a = np.full((h, w, 3), rng.randint(150, 256, 3), np.int32) + rng.randint(-6, 7, (h, w, 3))
        x = 1
        while x < w:
            sw = int(rng.randint(1, max(h // 5, 2)))
            a[int(rng.randint(0, h // 3 + 1)):h - int(rng.randint(0, h // 4 + 1)), x:x + sw] = rng.randint(0, 90, 3)
            x += sw + int(rng.randint(2, max(h // 2, 3)))
        out[b] = np.clip(a, 0, 255)
    return out


def pil_batch(images, qualities):
    from PIL import Image
    import numpy as np

    def one(args):
        im, q = args
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, 'JPEG', quality=int(q))
        buf.seek(0)
        return np.asarray(Image.open(buf))
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_jpeg: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    import torch
    from bench_resize import make_batch
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_jpeg: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    res = {"kernel_reps": a.kernel_reps, "reps": a.reps, "shapes": []}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def windows(fn):
        """us per call: three windows of --kernel-reps back-to-back calls between two events, the median and the spread"""
        for _ in range(20):
            fn()
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(a.kernel_reps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            t.append(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps)
        return round(statistics.median(t), 2), round((max(t) - min(t)) / statistics.median(t), 3)

    pool = ThreadPoolExecutor(16)
    for B, h, w in SHAPES:
        imgs = glyph_batch(B, h, w)
        q = np.random.RandomState(1).randint(30, 96, B).astype(np.int32)
        one = pil_batch(imgs, q)
        want = np.stack(list(map(one, zip(imgs, q))))
        x, qd = torch.from_numpy(imgs).to(dev), torch.from_numpy(q).to(dev)
        got = ops.jpeg_roundtrip_u8(x, qd)
        row = {"B": B, "h": h, "w": w, "mcus": B * (-(-h // 16)) * (-(-w // 16)), "bytes_differing_from_pil": int((got.cpu().numpy() != want).sum())}
        out = torch.empty_like(x)
        ws = torch.empty(lib.dpmn_jpeg_roundtrip_workspace_bytes(B, h, w), dtype=torch.uint8, device=dev)
        st = stream()
        row["kernel_us"], row["kernel_spread"] = windows(lambda: check(lib.dpmn_jpeg_roundtrip_u8(
            x.data_ptr(), out.data_ptr(), qd.data_ptr(), B, h, w, ws.data_ptr(), ws.numel(), st)))
        ql = q.tolist()
        row["op_call_us"], row["op_call_spread"] = windows(lambda: ops.jpeg_roundtrip_u8(x, ql))
        t1, t16 = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            list(map(one, zip(imgs, q)))
            t1.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            list(pool.map(one, zip(imgs, q)))
            t16.append((time.perf_counter() - t0) * 1e3)
        row["pil_1t_ms"], row["pil_16t_ms"] = round(statistics.median(t1), 3), round(statistics.median(t16), 3)
        res["shapes"].append(row)

    pair = pack_ragged([np.asarray(hr, dtype=np.uint8) for hr, _, _, _, _ in make_batch(48)], pin=False)
    t = {None: [], (30, 95, 0.5): []}
    for r in range(a.warmup + a.reps):
        for jpeg in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tz.degrade_on_gpu(pair, (32, 128), 2, True, dev, rng=random.Random(r), jpeg=jpeg)
            torch.cuda.synchronize()
            if r >= a.warmup:
                t[jpeg].append((time.perf_counter() - t0) * 1e3)
    for name, v in (("loader_off", t[None]), ("loader_on", t[(30, 95, 0.5)])):
        med = statistics.median(v)
        res[name + "_ms"], res[name + "_best_ms"], res[name + "_spread"] = round(med, 3), round(min(v), 3), round((max(v) - min(v)) / med, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
