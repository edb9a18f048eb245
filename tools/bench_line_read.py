#!/usr/bin/env python3
"""One read per tiled line (csrc/line_read.hip, main.py --demo_line_read) on one MI355X: writes ONE JSON document (--out, default
profiles/line_read_bench.json) and prints it.  All in one process and run, medians of --reps after --warmup calls.

Eight lines of 16 x 1024 LR columns (21 windows each, 168 windows) with seeded pixels, the cfg0 stack and a NativeCRNN with seeded weights:
  windows_ms / windows_line_read_ms   wall time of TextSR._demo_windows over the batch, without the flag (every window read on its own,
                                      the reads joined with '|': the behaviour before the flag existed) and with line_read; called in turn
On the frame logits of those 168 LR windows:
  stitch_ms / greedy_ms / ctc_ms      the three kernels alone, between HIP events
  torch_ms                            torch's formulation on the same stitched rows and the same strings: F.log_softmax + F.ctc_loss
                                      (reduction='none', lines padded to the longest), targets and lengths on the device beforehand
  max_abs_difference_to_torch         the largest |score - torch's|"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_confidence import event_median, wall_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "line_read_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_line_read: needs the GPU"
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
    plain, lines = wall_pair(lambda: run(None), lambda: run({"rec": crnn, "gap": 0}), args.reps, args.warmup)
    out = {"metric": "TextSR._demo_windows over %d lines of 16 x %d (%d windows each), without and with line_read" % (args.lines, args.width, len(starts)),
           "unit": "ms", "lines": args.lines, "windows": len(plan), "chunk": args.chunk, "reps": args.reps, "warmup": args.warmup,
           "windows_ms": round(plain, 4), "windows_line_read_ms": round(lines, 4), "difference_ms": round(lines - plain, 4)}
    rows = torch.cat([crnn.window_rows(x[lo:lo + args.chunk, :3])[0] for lo in range(0, len(plan), args.chunk)], 0)
    T = rows.shape[0] // len(plan)
    line_lp, table = ops.line_stitch(rows, T, 37, plan, 64)
    buf = ops.line_greedy(line_lp, table, extra=len(table))[0]
    out["stitch_ms"] = round(event_median(lambda: ops.line_stitch(rows, T, 37, plan, 64), args.reps, args.warmup), 4)
    out["greedy_ms"] = round(event_median(lambda: ops.line_greedy(line_lp, table, extra=len(table)), args.reps, args.warmup), 4)
    out["ctc_ms"] = round(event_median(lambda: ops.line_ctc_confidence(line_lp, table, buf), args.reps, args.warmup), 4)
    N, B = table.frames, len(table)
    h = buf.cpu().numpy()
    n = h[3 * N:3 * N + B]
    targets = torch.cat([torch.from_numpy(h[f0:f0 + k].copy()) for (f0, _), k in zip(table, n.tolist())]).long().to(dev)
    lengths, in_len = torch.from_numpy(n.copy()).long().to(dev), torch.tensor([L for _, L in table], device=dev)
    Lmax = table.max_L
    idx = torch.tensor([[min(f0 + j, f0 + L - 1) for f0, L in table] for j in range(Lmax)], device=dev)      # (Lmax, B) rows, padded

    def stock():
        return -F.ctc_loss(F.log_softmax(line_lp, -1)[idx], targets, in_len, lengths, blank=0, reduction="none")
    out["torch_ms"] = round(event_median(stock, args.reps, args.warmup), 4)
    out["max_abs_difference_to_torch"] = float((stock() - ops.line_ctc_confidence(line_lp, table, buf)).abs().max())
    out["frames_per_line"], out["greedy_lengths_min_max"] = Lmax, [int(n.min()), int(n.max())]
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
