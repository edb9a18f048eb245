#!/usr/bin/env python3
"""Lexicon-constrained reading (csrc/lexicon.hip, main.py --rec_lexicon) on one MI355X: writes ONE JSON document (--out, default
profiles/lexicon_bench.json) and prints it.

Inputs: seeded N(0, 3^2) logits (B = 48, T = 26, 37 classes in rows of 40) and a seeded synthetic lexicon of distinct words whose
lengths follow a rough English profile (2 .. 14, mode 7), L in --sizes (default 1000 and 90000).
  native_ms   dpmn_ctc_lexicon_f32 (both launches), median of --reps calls, each between HIP events after --warmup calls
  stock_ms    the same answer from stock operators on the same GPU in the same run: torch.nn.functional.ctc_loss(reduction='none')
              over every (image, word) pair -- the (T, 37) log-probabilities replicated once per word, in chunks of --chunk words so
              that they fit, every pair with the full T as its input length -- then argmax; the targets and lengths of every chunk
              are built and uploaded before the clock starts.  Median of --stock-reps calls
  index_mismatches  images on which the two disagree (the float32 top-2 gap can be below their rounding)
  edit_ms     dpmn_edit_lexicon_i32 for B strings against the same lexicon
  read_lexicon  at the largest L: NativeCRNN prep -> logits -> greedy classes -> lexicon kernel (no host copy), the kernel's share"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def synthetic_lexicon(L, seed=5):
    from dpmn_amd.model.crnn import ALPHABET
    rng = np.random.RandomState(seed)
    lengths = np.arange(2, 15)
    p = np.exp(-0.5 * ((lengths - 7) / 2.5) ** 2)
    p /= p.sum()
    letters = list(ALPHABET[10:]) * 4 + list(ALPHABET[:10])      # mostly letters
    words, seen = [], set()
    while len(words) < L:
        w = "".join(rng.choice(letters, rng.choice(lengths, p=p)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words


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
    ap.add_argument("--sizes", type=str, default="1000,90000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stock-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lexicon_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lexicon: needs the GPU"
    from dpmn_amd import ops
    from dpmn_amd.utils import lexicon as lx
    dev = torch.device("cuda:0")
    B, T, C, LD = args.batch, 26, 37, 40
    rng = np.random.RandomState(11)
    logits = np.zeros((B * T, LD), np.float32)
    logits[:, :C] = (rng.randn(B * T, C) * 3).astype(np.float32)
    rows = torch.from_numpy(logits).to(dev)
    out = {"metric": "lexicon-constrained reading, B = %d, T = %d, %d classes" % (B, T, C), "unit": "ms", "batch": B, "reps": args.reps,
           "stock_reps": args.stock_reps, "warmup": args.warmup, "stock_chunk_words": args.chunk, "sizes": {}}
    lex = None
    for L in [int(v) for v in args.sizes.split(",")]:
        lex = ops.Lexicon(synthetic_lexicon(L))
        n_ms = event_median(lambda: ops.ctc_lexicon(rows, B, T, C, lex), args.reps, args.warmup)
        h = ops.ctc_lexicon(rows, B, T, C, lex).cpu().numpy()
        # the stock path: targets / lengths of every chunk on the device before the clock starts
        chunks = []
        for lo in range(0, L, args.chunk):
            rec = lex.packed[lo:lo + args.chunk]
            n = rec.shape[0]
            chunks.append((n, torch.from_numpy(rec[:, 1:].astype(np.int64)).repeat(B, 1).to(dev),
                           torch.from_numpy(rec[:, 0].astype(np.int64)).repeat(B).to(dev), torch.full((B * n,), T, dtype=torch.long, device=dev)))

        def stock():
            lp = torch.log_softmax(rows[:, :C], -1).view(B, T, C).permute(1, 0, 2)                 # (T, B, C)
            scores = []
            for n, targets, lengths, in_len in chunks:
                rep = lp[:, :, None, :].expand(T, B, n, C).reshape(T, B * n, C)                    # entry b * n + w
                scores.append(-F.ctc_loss(rep, targets, in_len, lengths, blank=0, reduction="none").view(B, n))
            s = torch.cat(scores, 1)
            return s.argmax(1), s
        s_ms = event_median(stock, args.stock_reps, 1)
        s_idx, s_all = stock()
        s_idx = s_idx.cpu().numpy()
        idx, logp = h[:B].astype(np.int64), h[B:].view(np.float32)
        s_at = s_all.cpu().numpy()[np.arange(B), idx]
        strings = torch.from_numpy(lx.pack_strings([lex.words[i][:-1] + "x" for i in idx])).to(dev)
        e_ms = event_median(lambda: ops.edit_lexicon(strings, lex), args.reps, args.warmup)
        states = float((2 * lex.packed[:, 0].astype(np.int64) + 1).mean())
        out["sizes"][str(L)] = {
            "native_ms": round(n_ms[0], 4), "native_ms_min_max": [round(n_ms[1], 4), round(n_ms[2], 4)],
            "stock_ms": round(s_ms[0], 3), "stock_ms_min_max": [round(s_ms[1], 3), round(s_ms[2], 3)],
            "stock_over_native": round(s_ms[0] / n_ms[0], 2), "index_mismatches": int((idx != s_idx).sum()),
            "max_abs_logp_difference_at_the_native_index": float(np.abs(logp - s_at).max()),
            "recursions": B * L, "mean_states_per_word": round(states, 2),
            "native_ns_per_recursion": round(n_ms[0] * 1e6 / (B * L), 3),
            "edit_ms": round(e_ms[0], 4), "edit_ms_min_max": [round(e_ms[1], 4), round(e_ms[2], 4)]}
    # the kernel's share of read_lexicon's device work at the largest lexicon
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    from dpmn_amd.utils import synth
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    nat = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    nat.load_state_dict(sd)
    x = synth.uniform("bench_lexicon", (B, 3, 32, 128), 0, 1, 1).to(dev)

    def forward(with_lexicon):
        r, b, t = nat.logits_rows(nat.prep(x))
        buf, _, _ = ops.ctc_greedy(r, b, t, 37, extra=2 * b)
        if with_lexicon:
            ops.ctc_lexicon(r, b, t, 37, lex, out=buf[b * t + b:])
    f_ms = event_median(lambda: forward(False), args.reps, args.warmup)
    fl_ms = event_median(lambda: forward(True), args.reps, args.warmup)
    r_nat, b_, t_ = nat.logits_rows(nat.prep(x))
    k_ms = event_median(lambda: ops.ctc_lexicon(r_nat, b_, t_, 37, lex), args.reps, args.warmup)
    out["read_lexicon"] = {"L": len(lex), "forward_and_greedy_ms": round(f_ms[0], 4), "with_lexicon_kernel_ms": round(fl_ms[0], 4),
                           "lexicon_kernel_ms": round(k_ms[0], 4), "lexicon_kernel_share": round(k_ms[0] / fl_ms[0], 3)}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
