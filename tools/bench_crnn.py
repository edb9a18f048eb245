#!/usr/bin/env python3
"""Native CRNN recogniser (model/crnn.py NativeCRNN, --rec crnn) on one MI355X: prints ONE JSON line.

  native_ms  -- NativeCRNN prep -> CNN -> BiLSTMs -> greedy CTC classes (no host copy), B = 48, median of --reps runs, each
                bracketed by HIP events on the current stream after --warmup runs; in mode f32 and mode x3
                (dpmn_set_compute_dtype(2): the convs and GEMMs as bf16x3, the LSTM recurrence and pools stay fp32)
  mirror_ms  -- the stock-operator mirror (model/crnn.py CRNN: F.interpolate, MIOpen convs / LSTM, argmax) on the same GPU and
                inputs, same timing; the mode does not apply to it
  recurrence_ms -- the 2 x 26 dpmn_bilstm_f32 step launches alone (same timing), and their share of native_ms
  eval       -- TextSR.eval images/s on cfg1 (B = 48, synthetic priors) over --eval-batches labelled batches, without and with
                rec = NativeCRNN (host clock around a call that ends in a device synchronise; best of 3 after one warm-up call)
Inputs: 16x64 (LR) and 32x128 (SR) images.  Weights: name-seeded synthetic (tests/test_gpu_crnn.py).
--trace: only run read() --reps times (for `rocprofv3 --kernel-trace --stats -- python tools/bench_crnn.py --trace`)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def crnn_flops():
    """Multiply-adds x 2 of one 32x100 image: 7 convs + 2 BiLSTMs (input projection + recurrence) + 2 embeddings."""
    convs = [(1, 64, 3, 32, 100), (64, 128, 3, 16, 50), (128, 256, 3, 8, 25), (256, 256, 3, 8, 25), (256, 512, 3, 4, 26),
             (512, 512, 3, 4, 26), (512, 512, 2, 1, 26)]
    f = sum(2.0 * ci * co * k * k * h * w for ci, co, k, h, w in convs)
    T = 26
    for n_in, n_out in ((512, 256), (256, 37)):
        f += 2.0 * T * 2 * (4 * 256) * (n_in + 256) + 2.0 * T * 512 * n_out
    return f


def weights():
    from dpmn_amd.model.crnn import CRNN
    from dpmn_amd.utils import synth
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    return sd


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
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eval-batches", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crnn: needs the GPU"
    from dpmn_amd import _abi, ops
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    from dpmn_amd.utils import synth
    dev = torch.device("cuda:0")
    sd = weights()
    nat = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    nat.load_state_dict(sd)
    B = args.batch
    if args.trace:
        x = synth.uniform("bench_crnn", (B, 3, 32, 128), 0, 1, 1).to(dev)
        for _ in range(args.reps):
            nat.read(x)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "read", "batch": B, "calls": args.reps}))
        return
    mir = CRNN(32, 1, 37, 256).to(dev).eval()
    mir.load_state_dict(sd)
    out = {"metric": "CRNN recogniser forward, B = %d (prep -> decoded classes)" % B, "unit": "ms", "batch": B,
           "flop_per_image": crnn_flops(), "reps": args.reps, "warmup": args.warmup, "shapes": {}}

    def native(x):
        rows, b, t = nat.logits_rows(nat.prep(x))
        ops.ctc_greedy(rows, b, t, 37)

    def mirror(x):
        with torch.no_grad():
            mir(CRNN.parse_crnn_data(x[:, :3])).max(2)

    for hw in ((16, 64), (32, 128)):
        x = synth.uniform("bench_crnn", (B, 3) + hw, 0, 1, 1).to(dev)
        row = {}
        m_ms = event_median(lambda: mirror(x), args.reps, args.warmup)
        row["mirror_ms"] = round(m_ms[0], 4)
        row["mirror_ms_min_max"] = [round(m_ms[1], 4), round(m_ms[2], 4)]
        for mode, code in (("f32", 0), ("x3", 2)):
            _abi.check(_abi.lib.dpmn_set_compute_dtype(code))
            try:
                n_ms = event_median(lambda: native(x), args.reps, args.warmup)
                P = nat._packs()
                gx = [torch.zeros(B * 26, 2048, device=dev) for _ in range(2)]
                r_ms = event_median(lambda: [ops.bilstm(gx[i], P["rnn"][i][2], B, 26) for i in range(2)], args.reps, args.warmup)
            finally:
                _abi.lib.dpmn_set_compute_dtype(0)
            row[mode] = {"native_ms": round(n_ms[0], 4), "native_ms_min_max": [round(n_ms[1], 4), round(n_ms[2], 4)],
                         "mirror_over_native": round(m_ms[0] / n_ms[0], 3), "recurrence_ms": round(r_ms[0], 4),
                         "recurrence_share": round(r_ms[0] / n_ms[0], 3),
                         "achieved_tflops": round(crnn_flops() * B / (n_ms[0] * 1e-3) / 1e12, 2)}
        out["shapes"]["%dx%d" % hw] = row

    # eval images/s, cfg1, with and without the recogniser
    from dpmn_amd import workload
    sr, models, psn, inp = workload.build("cfg1")
    Be = inp["images_lr"].shape[0]
    labels = ["word%d" % i for i in range(Be)]
    loader = [(inp["images_hr"], inp["images_lr"], inp["label_vecs"], labels)] * args.eval_batches
    ev = {}
    for name, rec in (("without_rec", None), ("with_rec", nat)):
        sr.eval(models, loader, 0, rec=rec, model_psn=psn)
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sr.eval(models, loader, 0, rec=rec, model_psn=psn)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        ev[name] = {"images_per_s": round(Be * args.eval_batches / best, 2), "accuracy": res["accuracy"]}
    ev["batch"], ev["batches"] = Be, args.eval_batches
    out["eval_cfg1"] = ev
    print(json.dumps(out))


if __name__ == "__main__":
    main()
