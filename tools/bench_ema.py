#!/usr/bin/env python3
"""What the averaged weights (Trainer(ema_decay=...), main.py --ema) cost per training step on one MI355X: prints ONE JSON line.

The default training workload of bench.py (cfg1, B = 48, Dropout = attn_drop = DropPath = 0.1, PSN prefetch) is built twice in the
same process -- one trainer without the average, one with ema_decay = 0.999 -- and the two steps are timed ALTERNATING, one step of
each per round, HIP events around every step, the median of --rounds (default 30) rounds after --warmup steps of each.  Also
reports the bytes the average adds (one fp32 vector the size of the parameter arena) and the derived extra traffic per step (one
read and one write of it)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(workload, torch, name, batch, drop, ema_decay):
    from dpmn_amd.loss.image_loss import ImageLoss
    from dpmn_amd.model.distill_module import DistillModule
    from dpmn_amd.train.optim import Trainer
    sr, models, psn, inp = workload.build(name, batch=batch, drop=drop)
    spec = workload.describe(name)
    torch.manual_seed(2)
    distill = [DistillModule().to(sr.device) for _ in range(spec["b1"] + spec["b2"] - 2)]
    crit = ImageLoss(gradient=True, loss_weight=[1, 1])
    for m in models + distill:
        m.train()
        for p in m.parameters():
            p.requires_grad = True
    trainer = Trainer(models + distill, lr=1e-3, beta1=0.5, max_norm=0.25, ema_decay=ema_decay)
    state = {"h": None}

    def step():
        loss = sr.train_step(models, psn, distill, crit, trainer, inp["images_lr"], inp["images_hr"], inp.get("label_vecs"),
                             text_priors=inp["text_priors"], psn_out=state["h"], prefetch=(inp["images_lr"], inp.get("label_vecs")))
        state["h"] = sr.psn_prefetched
        return loss
    return step, trainer, inp["images_lr"].shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg1")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import gc
    import torch
    from dpmn_amd import workload
    torch.cuda.set_device(0)
    before = torch.cuda.memory_allocated()
    step_off, tr_off, B = build(workload, torch, args.workload, args.batch, args.drop, None)
    mem_off = torch.cuda.memory_allocated() - before
    step_on, tr_on, _ = build(workload, torch, args.workload, args.batch, args.drop, args.decay)
    mem_on = torch.cuda.memory_allocated() - before - mem_off
    gc.collect()
    gc.freeze()
    for _ in range(args.warmup):
        step_off()
        step_on()
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for key, step in (("off", step_off), ("on", step_on)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in times.items()}
    n = tr_on.flat_p.numel()
    line = {
        "what": "training step with and without the averaged weights (ema_decay = %g), alternating in one process" % args.decay,
        "workload": args.workload, "per_gpu_batch": B, "drop": args.drop, "rounds": args.rounds, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "step_ms_off_median": round(med["off"], 4), "step_ms_on_median": round(med["on"], 4),
        "delta_ms": round(med["on"] - med["off"], 4), "delta_pct": round(100.0 * (med["on"] - med["off"]) / med["off"], 3),
        "step_ms_off_min_max": [round(min(times["off"]), 4), round(max(times["off"]), 4)],
        "step_ms_on_min_max": [round(min(times["on"]), 4), round(max(times["on"]), 4)],
        "paired_delta_ms_median": round(statistics.median(b_ - a_ for a_, b_ in zip(times["off"], times["on"])), 4),
        "arena_floats": n, "ema_bytes": 4 * sum(g.e.numel() for g in tr_on.groups),
        "extra_traffic_bytes_per_step_derived": 8 * n,
        "allocated_bytes_after_build_off": mem_off, "allocated_bytes_after_build_on": mem_on,
        "timing": "HIP events around each step on the step's stream, synchronised after every step",
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
