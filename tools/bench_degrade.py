#!/usr/bin/env python3
"""What synthesising the LR images of a TextZoom-sized batch costs on one MI355X and on the host: prints ONE JSON line.

A batch of --batch decoded HR images in the sizes of tools/bench_resize.py (43 x 157 .. 55 x 185), alternating in the same run,
  gpu_ms   -- alignCollate_realWTLAMask(degrade=True, cutblur=True) + sr_batches: pack the HR pixels, one upload, the parameter draws,
              ops.degrade_ragged_u8, the two ragged resizes, the collate kernel;  gpu_collate_ms = its host collate alone
  host_ms  -- the NumPy restatement utils.degrade.degrade_u8 (float32) over the same images with the same parameters, one image after
              the other on one core (what a loader worker would run), noise field drawn with NumPy; NOT followed by resize or collate
  op_call_us -- ops.degrade_ragged_u8 alone (its small upload of the items / params / tile table and both launches), HIP events around
              --kernel-reps back-to-back calls
Wall-clock times end in a device synchronise; median of --reps batches after --warmup, spread = (max - min) / median.  The measurement
runs in a child process under a time limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_degrade: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from bench_resize import make_batch
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import degrade as dg
    if not torch.cuda.is_available():
        print("bench_degrade: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    H, W, scale = 32, 128, 2
    batch = [(hr, hr, None, None, word) for hr, _, _, _, word in make_batch(a.batch)]
    col = tz.alignCollate_realWTLAMask(imgH=H, imgW=W, down_sample_scale=scale, mask=True, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True)
    loader = type("Loader", (), {"collate_fn": col})()
    random.seed(1)
    tot, colt = [], []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = col(batch)
        t1 = time.perf_counter()
        loader.__class__.__iter__ = lambda self, out=out: iter([out])
        (hr, lr, _, _), = list(tz.sr_batches(loader, dev, True))
        torch.cuda.synchronize()
        if r >= a.warmup:
            tot.append((time.perf_counter() - t0) * 1e3)
            colt.append((t1 - t0) * 1e3)
    med = statistics.median(tot)
    res = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "out_hw": [H, W], "scale": scale, "gpu_ms": round(med, 3),
           "gpu_best_ms": round(min(tot), 3), "gpu_spread": round((max(tot) - min(tot)) / med, 3),
           "gpu_collate_ms": round(statistics.median(colt), 3)}

    images = [np.asarray(im[0], dtype=np.uint8) for im in batch]
    params = dg.draw_params(len(images), cutblur=True, hr_widths=[im.shape[1] for im in images], rng=random.Random(2))
    host = []
    for r in range(a.host_reps):
        rng = np.random.RandomState(r)
        t0 = time.perf_counter()
        for im, p in zip(images, params):
            dg.degrade_u8(im, p, rng.standard_normal(im.shape).astype(np.float32), np.float32)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_ms"], res["host_best_ms"] = round(statistics.median(host), 1), round(min(host), 1)

    packed, meta = out[0]
    packed = packed.to(dev)
    for _ in range(10):
        ops.degrade_ragged_u8(packed, meta, params, seed=3)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(a.kernel_reps):
        ops.degrade_ragged_u8(packed, meta, params, seed=3)
    ev1.record()
    torch.cuda.synchronize()
    res["op_call_us"] = round(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps, 2)
    res["input_bytes"] = int(packed.numel())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
