#!/usr/bin/env python3
"""Native ASTER recogniser (model/aster.py NativeASTER, --rec aster) on one MI355X: prints ONE JSON line.

  native_ms / mirror_ms -- read() of B = 48 images of 32 x 128 (device work + the one host copy + host backtracking), median of
                           --reps runs after --warmup runs, native first then the stock-operator mirror (reference loop structure)
                           in the same process; per compute mode (f32, x3; the mirror has no modes)
  stage_ms              -- native stages timed with HIP events around each (prep + STN + TPS, ResNet, BiLSTM, decoder incl. xEmbed)
  launches_per_step     -- kernel launches of one decoder step (the library's launch sequence: sproj, attend, gru, topk)
Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_aster.py` for the per-kernel table (no counters in that run)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dpmn_amd import _abi
    from dpmn_amd.model.aster import ASTER, NativeASTER
    from dpmn_amd.utils import aster_synth
    from dpmn_amd.utils.labelmaps import AsterInfo
    dev = torch.device("cuda:0")
    sd = ASTER().state_dict()
    aster_synth.aster_fill_(sd, 81)
    nat, mir = NativeASTER().to(dev).eval(), ASTER().to(dev).eval()
    nat.load_state_dict(sd)
    mir.load_state_dict(sd)
    pool = aster_synth.aster_images(aster_synth.POOL)
    img = torch.cat([pool] * (a.batch // aster_synth.POOL + 1), 0)[:a.batch].to(dev)
    info = AsterInfo('all')

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts)

    def stages():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        norm, stn_in = nat.prep(img)
        rect = nat.rectify(norm, stn_in)[1]
        ev[1].record()
        f = nat.resnet(rect)[-1]
        ev[2].record()
        feats = nat.encode(rect)
        ev[3].record()
        nat.beam_search(feats)
        ev[4].record()
        torch.cuda.synchronize()
        e = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
        return {"prep_stn_tps": e[0], "resnet": e[1], "resnet_plus_bilstm_again": e[2], "decoder": e[3]}

    res = {"batch": a.batch, "reps": a.reps, "launches_per_step": 4}
    for mode, code in (("f32", 0), ("x3", 2)):
        _abi.check(_abi.lib.dpmn_set_compute_dtype(code))
        med, best = timed(lambda: nat.read(img))
        res["native_ms_" + mode], res["native_best_ms_" + mode] = round(med, 3), round(best, 3)
        stages()
        res["stage_ms_" + mode] = {k: round(v, 3) for k, v in stages().items()}
    _abi.check(_abi.lib.dpmn_set_compute_dtype(0))
    med, best = timed(lambda: mir.read(img, info))
    res["mirror_ms"], res["mirror_best_ms"] = round(med, 3), round(best, 3)
    res["speedup_f32"], res["speedup_x3"] = round(med / res["native_ms_f32"], 2), round(med / res["native_ms_x3"], 2)
    res["same_strings"] = nat.read(img) == mir.read(img, info)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
