#!/usr/bin/env python3
"""A tiled line read as lexicon words (csrc/line_words.hip, main.py --rec_lexicon with --demo_tile --demo_line_read) on one MI355X:
writes ONE JSON document (--out, default profiles/line_words_bench.json) and prints it.  All in one process and run, medians of
--reps after --warmup calls.

Eight lines of 16 x 1024 LR columns (21 windows each, 168 windows, 401 frames per line) with seeded pixels, the cfg0 stack and a
NativeCRNN with seeded weights, as tools/bench_line_read.py; lexicons of --sizes words built as tools/bench_lexicon.py builds its own.
Per lexicon size:
  nodes / arm                         the prefix trie's nodes and the arm ops.line_words_arm dispatches
  windows_line_read_ms / _lexicon_ms  wall time of TextSR._demo_windows with line_read, without a lexicon (the path before --rec_lexicon
                                      combined with --demo_tile: the same kernels) and with it; called in turn
  step_ms / lds_ms                    each arm alone on the stitched rows of the 168 LR windows, between HIP events (lds_ms: null where
                                      the trie does not fit the LDS)
  step_hbm_fraction                   the frame-per-launch arm's state bytes per frame (per node and line: 24 read of its own state,
                                      24 of its parent's, 24 written, 16 of the trie) over its time per frame, as a fraction of the
                                      8.0 TB/s HBM peak"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_confidence import event_median, wall_pair  # noqa: E402
from bench_lexicon import synthetic_lexicon  # noqa: E402

HBM_PEAK = 8.0e12            # bytes per second
NODE_BYTES = 24 + 24 + 24 + 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 300, 650, 1000, 90000])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "line_words_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_line_words: needs the GPU"
    from dpmn_amd import ops, workload
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    from dpmn_amd.utils import synth, tile
    dev = torch.device("cuda:0")
    sr, models, psn = workload.build("cfg0", batch=args.chunk)[:3]
    fn = sr.synthetic_text_prior()
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    crnn = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    crnn.load_state_dict(sd)
    starts = tile.window_plan(args.width)
    plan = [(b, x0) for b in range(args.lines) for x0 in starts]
    x = synth.uniform("bench_line_read", (len(plan), 4, 16, 64), 0, 1, 1).to(dev)
    names = ["line%d.png" % b for b in range(args.lines)]
    run = lambda kw: list(sr._demo_windows(models, psn, [(names, plan, x)], fn, crnn.read, args.chunk, kw))
    rows = torch.cat([crnn.window_rows(x[lo:lo + args.chunk, :3])[0] for lo in range(0, len(plan), args.chunk)], 0)
    line_lp, table = ops.line_stitch(rows, rows.shape[0] // len(plan), 37, plan, 64)
    lds_nodes = ops.line_words_lds_nodes(dev)
    out = {"metric": "TextSR._demo_windows over %d lines of 16 x %d (%d windows each) with line_read, without and with a lexicon; each arm "
                     "of dpmn_line_words_f64 alone" % (args.lines, args.width, len(starts)),
           "unit": "ms", "lines": args.lines, "windows": len(plan), "frames_per_line": table.max_L, "chunk": args.chunk, "reps": args.reps,
           "warmup": args.warmup, "lds_arm_max_nodes": lds_nodes, "block_nodes": ops.LINE_WORDS_BLOCK, "hbm_peak_bytes_per_s": HBM_PEAK,
           "sizes": {}}
    for size in args.sizes:
        lex = ops.Lexicon(synthetic_lexicon(size))
        nodes = len(lex.trie)
        plain, lexed = wall_pair(lambda: run({"rec": crnn, "gap": 0}), lambda: run({"rec": crnn, "gap": 0, "lexicon": lex, "penalty": 0.0}),
                                 args.reps, args.warmup)
        step = event_median(lambda: ops.line_words_records(line_lp, table, lex, arm="step"), args.reps, args.warmup)
        lds = event_median(lambda: ops.line_words_records(line_lp, table, lex, arm="lds"), args.reps, args.warmup) if nodes <= lds_nodes else None
        same = None
        if lds is not None:
            same = bool(torch.equal(ops.line_words_records(line_lp, table, lex, arm="step"), ops.line_words_records(line_lp, table, lex, arm="lds")))
        reads = ops.line_words(line_lp, table, lex)
        out["sizes"][str(size)] = {
            "nodes": nodes, "arm": ops.line_words_arm(nodes, dev), "windows_line_read_ms": round(plain, 4),
            "windows_line_read_lexicon_ms": round(lexed, 4), "difference_ms": round(lexed - plain, 4), "step_ms": round(step, 4),
            "lds_ms": None if lds is None else round(lds, 4), "arms_write_equal_records": same,
            "step_us_per_frame": round(step * 1e3 / (table.max_L + 1), 4),
            "step_hbm_fraction": round(NODE_BYTES * nodes * len(table) / (step * 1e-3 / (table.max_L + 1)) / HBM_PEAK, 5),
            "words_per_line_min_max": [min(len(r[0]) for r in reads), max(len(r[0]) for r in reads)]}
        print(size, json.dumps(out["sizes"][str(size)]), flush=True)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
