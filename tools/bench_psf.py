#!/usr/bin/env python3
"""What the point-spread-function stage of the synthesised LR images (--psf_blur) costs on one MI355X: prints ONE JSON line.

B = 48 HR crops in the sizes of tools/bench_degrade.py (tools/bench_resize.py make_batch), PSFs of utils.psf.draw_psf with
kinds = motion, disk, aniso and the radius fraction 0.12 -- once every image blurred (prob 1) and once at the default prob 0.5:
  kernel_us    -- csrc/psf.hip alone: dpmn_psf_blur_ragged_u8 with the tables already on the device, HIP events around --kernel-reps
                  back-to-back calls (three windows, the median and the spread)
  cutblur_us   -- dpmn_cutblur_ragged_u8 the same way, every image with a cut
  op_call_us   -- ops.psf_blur_ragged_u8 with the host tap lists (its checks, the one upload, the output allocation, the launch)
  loader_off_ms / loader_on_ms -- degrade_on_gpu with cutblur from the packed host batch to the two float batches, psf=None against
                  psf=(kinds, 0.5, 0.12), alternating in the same run, wall clock ending in a device synchronise, medians
The GPU bytes are compared with utils.psf.psf_blur_u8 before anything is timed.  The measurement runs in a child process under a time
limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS, FRAC = ("motion", "disk", "aniso"), 0.12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
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
            print("bench_psf: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from bench_resize import make_batch
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import degrade as dg
    from dpmn_amd.utils import psf
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_psf: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    B = a.batch
    images = [np.asarray(hr, dtype=np.uint8) for hr, _, _, _, _ in make_batch(B)]
    pair = pack_ragged(images, pin=False)
    packed, meta = pair[0].to(dev), pair[1].numpy()
    heights = [int(h) for h in meta[:, 1]]
    res = {"B": B, "packed_bytes": int(packed.numel()), "kernel_reps": a.kernel_reps, "reps": a.reps, "cases": []}
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

    st = stream()
    m, items, tiles = ops._degrade_plan(packed, meta, "bench_psf")
    out = torch.zeros_like(packed)
    for prob in (1.0, 0.5):
        taps = psf.draw_psf(B, KINDS, prob, FRAC, heights, rng=random.Random(1))
        got = ops.psf_blur_ragged_u8(packed, meta, taps).cpu().numpy()
        bad = sum(int((got[o:o + h * w * 3].reshape(h, w, 3) != psf.psf_blur_u8(im, t)).sum())
                  for (o, h, w), im, t in zip(meta.tolist(), images, taps))
        table, flat = ops._psf_tables(taps, B)
        row = {"prob": prob, "tiles": int(tiles.shape[0]), "taps": int(flat.shape[0]), "largest_R": int(table[:, 2].max()),
               "blurred_images": int(sum(not psf.is_identity(t) for t in taps)), "bytes_differing_from_the_restatement": bad}
        d, d_items, d_tiles, d_psf, d_taps = ops._upload(dev, items, tiles, table, flat)
        row["kernel_us"], row["kernel_spread"] = windows(lambda: check(lib.dpmn_psf_blur_ragged_u8(
            packed.data_ptr(), packed.numel(), d_items, d_tiles, tiles.shape[0], d_psf, d_taps, flat.shape[0], B, out.data_ptr(), st)))
        row["op_call_us"], row["op_call_spread"] = windows(lambda: ops.psf_blur_ragged_u8(packed, meta, taps))
        res["cases"].append(row)

    cuts = np.concatenate((m, np.stack((m[:, 2] // 2, 1 + np.arange(B) % 2), axis=1)), axis=1).astype(np.int64)
    d, d_cuts = ops._upload(dev, np.ascontiguousarray(cuts))
    res["cutblur_us"], res["cutblur_spread"] = windows(lambda: check(lib.dpmn_cutblur_ragged_u8(
        packed.data_ptr(), packed.numel(), d_cuts, B, int((m[:, 1] * m[:, 2]).max()), out.data_ptr(), st)))

    setting = (KINDS, 0.5, FRAC)
    t = {None: [], setting: []}
    for r in range(a.warmup + a.reps):
        for s in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tz.degrade_on_gpu(pair, (32, 128), 2, True, dev, cutblur=True, rng=random.Random(r), psf=s)
            torch.cuda.synchronize()
            if r >= a.warmup:
                t[s].append((time.perf_counter() - t0) * 1e3)
    for name, v in (("loader_off", t[None]), ("loader_on", t[setting])):
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
