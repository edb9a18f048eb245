#!/usr/bin/env python3
"""Recogniser confidence (csrc/confidence.hip, main.py --demo_conf) on one MI355X: writes ONE JSON document (--out, default
profiles/confidence_bench.json) and prints it.

Per native recogniser with seeded synthetic weights, on B = 48 seeded images of 32 x 128:
  read_ms / read_conf_ms   wall time of the whole call (forward, decode, the ONE device-to-host copy, the host decoding), median of
                           --reps calls each; the two are called in turn, in the same process and run, after --warmup calls of each
For the CRNN, on the logits of that batch:
  conf_kernel_ms           dpmn_ctc_conf_f32 alone, between HIP events
  torch_ms                 the torch formulation on the same logits and the same greedy strings: F.log_softmax +
                           F.ctc_loss(reduction='none'), targets and lengths on the device before the clock starts
For MORAN: attn_kernel_ms, dpmn_attn_conf_f32 alone on the decoder's logits."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def event_median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def wall_pair(f, g, reps, warmup):
    """medians (ms) of f and g, called in turn"""
    for _ in range(warmup):
        f()
        g()
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(tf), statistics.median(tg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "confidence_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_confidence: needs the GPU"
    from dpmn_amd import ops
    from dpmn_amd.model.aster import ASTER, NativeASTER
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    from dpmn_amd.model.moran import MAX_ITER, MORAN, NativeMORAN
    from dpmn_amd.utils import aster_synth, moran_synth, synth
    dev = torch.device("cuda:0")
    B = args.batch
    x = synth.uniform("bench_confidence", (B, 3, 32, 128), 0, 1, 1).to(dev)
    out = {"metric": "read_conf against read, B = %d images of 32 x 128" % B, "unit": "ms", "batch": B, "reps": args.reps, "warmup": args.warmup}

    def pair(nat):
        r, c = wall_pair(lambda: nat.read(x), lambda: nat.read_conf(x), args.reps, args.warmup)
        return {"read_ms": round(r, 4), "read_conf_ms": round(c, 4), "difference_ms": round(c - r, 4)}

    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    crnn = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    crnn.load_state_dict(sd)
    res = pair(crnn)
    rows, b, t = crnn.logits_rows(crnn.prep(x))
    buf, cls, length = ops.ctc_greedy(rows, b, t, 37, extra=b)
    res["conf_kernel_ms"] = round(event_median(lambda: ops.ctc_confidence(rows, b, t, 37, buf), args.reps, args.warmup), 4)
    n = length.cpu().numpy()
    targets = torch.cat([cls[i, :int(n[i])] for i in range(b)]).long()
    lengths, in_len = length.long(), torch.full((b,), t, dtype=torch.long, device=dev)

    def stock():
        lp = F.log_softmax(rows[:, :37], -1).view(b, t, 37).permute(1, 0, 2)
        return -F.ctc_loss(lp, targets, in_len, lengths, blank=0, reduction="none")
    res["torch_ms"] = round(event_median(stock, args.reps, args.warmup), 4)
    res["max_abs_difference_to_torch"] = float((stock() - ops.ctc_confidence(rows, b, t, 37, buf)).abs().max())
    res["frames"], res["greedy_lengths_min_max"] = t, [int(n.min()), int(n.max())]
    out["crnn"] = res

    sd = MORAN().state_dict()
    moran_synth.moran_fill_(sd, 91)
    moran = NativeMORAN().to(dev).eval()
    moran.load_state_dict(sd)
    res = pair(moran)
    logits, ids = moran._run(*moran.prep(x), MAX_ITER)
    res["attn_kernel_ms"] = round(event_median(lambda: ops.attn_confidence(logits, ids, 36), args.reps, args.warmup), 4)
    out["moran"] = res

    sd = ASTER().state_dict()
    aster_synth.aster_fill_(sd, 81)
    aster = NativeASTER().to(dev).eval()
    aster.load_state_dict(sd)
    out["aster"] = pair(aster)

    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
