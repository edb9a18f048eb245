#!/usr/bin/env python3
"""CTC beam search with a character model (csrc/beam.hip, main.py --rec_beam / --rec_lm) on one MI355X: writes ONE JSON document
(--out, default profiles/beam_bench.json) and prints it.

The native CRNN with seeded synthetic weights on B = 48 seeded images of 32 x 128, medians of --reps calls in one run:
  read_ms / read_beam_ms   wall time of the whole call (forward, decode, the ONE device-to-host copy, the host decoding); read and
                           read_beam are called in turn, at width 1, 16 and 32, without a model and with an order-3 model
  kernel_ms                dpmn_ctc_beam_f64 alone on the logits of that batch, between HIP events
  beam_np_ms               utils.beam.beam_np on the host over the same rows (one call over the batch, median of 3)
There is no speed bar: the feature stands on agreement with the definition; this records what it costs."""
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


def corpus(n=2000, seed=7):
    """seeded words over the CRNN's symbols, as classes, with a skewed symbol distribution"""
    rng = np.random.RandomState(seed)
    p = rng.dirichlet(np.full(36, 0.3))
    return [tuple(int(c) + 1 for c in rng.choice(36, rng.randint(1, 11), p=p)) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam: needs the GPU"
    from dpmn_amd import ops
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    from dpmn_amd.utils import beam as bm
    from dpmn_amd.utils import synth
    dev = torch.device("cuda:0")
    B = args.batch
    x = synth.uniform("bench_beam", (B, 3, 32, 128), 0, 1, 1).to(dev)
    out = {"metric": "read_beam against read, B = %d images of 32 x 128" % B, "unit": "ms", "batch": B, "reps": args.reps, "warmup": args.warmup}
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    for k, v in sd.items():             # (as the tests: without the biases the readings depend on the image)
        if (k.startswith("rnn.") and "bias" in k) or (k.startswith("cnn.conv") and k.endswith(".bias")):
            v.zero_()
    crnn = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    crnn.load_state_dict(sd)
    lm = ops.CharLM(bm.build_char_lm(corpus(), 3), 3)
    rows, b, t = crnn.logits_rows(crnn.prep(x))
    host = rows.cpu().numpy()
    out["frames"] = t
    runs = []
    for width in (1, 16, 32):
        for model in (None, lm):
            r, g = wall_pair(lambda: crnn.read(x), lambda: crnn.read_beam(x, model, width), args.reps, args.warmup)
            k = event_median(lambda: ops.ctc_beam(rows, b, t, 37, model, width), args.reps, args.warmup)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                for i in range(b):
                    bm.beam_np(host[i * t:(i + 1) * t], model.table if model is not None else None, width, 0.5, 0.0, n_class=37)
                ts.append((time.perf_counter() - t0) * 1e3)
            runs.append({"width": width, "model_order": 3 if model is not None else 0, "read_ms": round(r, 4), "read_beam_ms": round(g, 4),
                         "difference_ms": round(g - r, 4), "kernel_ms": round(k, 4), "beam_np_ms": round(statistics.median(ts), 2)})
    out["runs"] = runs
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
