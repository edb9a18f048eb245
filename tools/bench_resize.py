#!/usr/bin/env python3
"""What the bicubic resize of a TextZoom batch costs on the host and on one MI355X: prints ONE JSON line.

Batches of --batch (HR, LR) pairs of decoded PIL images in the sizes of the test suite's stand-in data set (HR 43 x 157 .. 55 x 185,
LR 19 x 73 .. 23 x 85) go to 32 x 128 / 16 x 64 through, alternating in the same run,
  host_resize_ms -- (a) the default path: alignCollate_realWTLAMask(gpu_finish=True) = PIL resize per image on the host, then
                    sr_batches = upload of the resized pixels + k_collate_u8;                   collate_ms = its host collate alone
  gpu_resize_ms  -- (b) gpu_resize=True: the collate only packs the decoded pixels, sr_batches uploads them, resizes them on the GPU
                    (ops.resize_ragged_u8) and finishes them;                                   collate_ms = its host collate alone
  kernel_us      -- (c) dpmn_resize_ragged_u8 alone (both launches), HR and LR batch, HIP events around --kernel-reps back-to-back calls
Wall-clock times end in a device synchronise; median of --reps batches after --warmup, spread = (max - min) / median.  Both paths run
in this process, single-threaded (no loader workers): the per-batch cost, not the throughput of a loader whose workers hide it.
The measurement runs in a child process under a time limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_batch(n, seed=7):
    """n (HR image, LR image, None, None, label) items as lmdbDataset_real yields them, five size pairs in turn."""
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    batch = []
    for j in range(n):
        i = j % 5 + 1
        hr = rng.randint(0, 256, (40 + 3 * i, 150 + 7 * i, 3)).astype(np.uint8)
        lr = rng.randint(0, 256, (18 + i, 70 + 3 * i, 3)).astype(np.uint8)
        batch.append((Image.fromarray(hr), Image.fromarray(lr), None, None, "word%d" % j))
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
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
            print("bench_resize: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import torch
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.dataset import textzoom as tz
    if not torch.cuda.is_available():
        print("bench_resize: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    H, W, scale = 32, 128, 2
    batch = make_batch(a.batch)
    cols = {"host_resize": tz.alignCollate_realWTLAMask(imgH=H, imgW=W, down_sample_scale=scale, mask=True, gpu_finish=True),
            "gpu_resize": tz.alignCollate_realWTLAMask(imgH=H, imgW=W, down_sample_scale=scale, mask=True, gpu_finish=True, gpu_resize=True)}

    def one(col):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = col(batch)
        t1 = time.perf_counter()
        (hr, lr, _, _), = list(tz.sr_batches([out], dev, True, size=(H, W, scale)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, hr, lr

    times = {k: ([], []) for k in cols}
    last = {}
    for r in range(a.warmup + a.reps):
        for k, col in cols.items():      # alternating: both paths see the same machine state
            total, collate, hr, lr = one(col)
            last[k] = (hr, lr)
            if r >= a.warmup:
                times[k][0].append(total)
                times[k][1].append(collate)
    res = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "out_hw": [H, W], "scale": scale,
           "same_batches": bool(torch.equal(last["host_resize"][0], last["gpu_resize"][0]) and torch.equal(last["host_resize"][1], last["gpu_resize"][1]))}
    for k, (tot, colt) in times.items():
        med = statistics.median(tot)
        res[k + "_ms"], res[k + "_best_ms"], res[k + "_spread"] = round(med, 3), round(min(tot), 3), round((max(tot) - min(tot)) / med, 3)
        res[k + "_collate_ms"] = round(statistics.median(colt), 3)
    res["gpu_over_host"] = round(res["gpu_resize_ms"] / res["host_resize_ms"], 3)

    # (c) the two launches alone, with everything they read already on the device
    out = cols["gpu_resize"](batch)
    res["kernel_us"] = {}
    for tag, pair, (h, w) in (("hr", out[0], (H, W)), ("lr", out[2], (H // scale, W // scale))):
        packed = pair[0].to(dev)
        B, max_h, items, mid = ops._resize_ragged_plan(packed, pair[1], h, w)
        dst = torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
        call = lambda: check(lib.dpmn_resize_ragged_u8(packed.data_ptr(), packed.numel(), items.data_ptr(), B, max_h, dst.data_ptr(), h, w,
                                                       mid.data_ptr(), mid.numel(), stream()))
        for _ in range(10):
            call()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(a.kernel_reps):
            call()
        ev1.record()
        torch.cuda.synchronize()
        res["kernel_us"][tag] = round(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps, 2)
        res["kernel_us"][tag + "_input_bytes"] = int(packed.numel())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
