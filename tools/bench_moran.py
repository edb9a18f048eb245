#!/usr/bin/env python3
"""Native MORAN recogniser (model/moran.py NativeMORAN, --rec moran) on one MI355X: prints ONE JSON line.

  native_ms / mirror_ms -- read() of B = 48 images of 32 x 128 and of 16 x 64 (device work + the one host copy + the cut at '$'),
                           median of --reps runs after --warmup runs, native first then the stock-operator mirror in the same
                           process; per compute mode (f32, x3; the mirror has no modes); spread = (max - min) / median of the runs
  stage_ms              -- native and mirror stages timed with HIP events around each (prep + MORN, ResNet, BiLSTM, decoder incl. i2h)
The measurement runs in a child process under a time limit of its own (--timeout seconds); the parent never opens the GPU.
Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_moran.py` for the per-kernel table (no counters in that run)."""
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
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_moran: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import torch
    from dpmn_amd import _abi
    from dpmn_amd.model.moran import MORAN, NativeMORAN
    from dpmn_amd.utils import moran_synth
    dev = torch.device("cuda:0")
    sd = MORAN().state_dict()
    moran_synth.moran_fill_(sd, 91)
    nat, mir = NativeMORAN().to(dev).eval(), MORAN().to(dev).eval()
    nat.load_state_dict(sd)
    mir.load_state_dict(sd)

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
        med = statistics.median(ts)
        return round(med, 3), round(min(ts), 3), round((max(ts) - min(ts)) / med, 3)

    def events(fns):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record()
        x = None
        for i, fn in enumerate(fns):
            x = fn(x)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [round(ev[i].elapsed_time(ev[i + 1]), 3) for i in range(len(fns))]

    names = ("prep_morn", "resnet", "bilstm", "decoder")

    def native_stages(img):
        P = nat._packs()
        fns = [lambda _: nat.rectify(*nat.prep(img), 1, P)[2], lambda x: nat.resnet(x, P), lambda f: nat.bilstm(f, P),
               lambda f: nat.decode(f, 20, P)]
        events(fns)
        return dict(zip(names, events(fns)))

    def mirror_stages(img):
        att = mir.ASRN.l2r
        fns = [lambda _: mir.MORN.stages(mir.parse_moran_data(img))[1], mir.ASRN.cnn,
               lambda c: mir.ASRN.rnn(c.squeeze(2).permute(2, 0, 1).contiguous()), lambda r: att.greedy(r, 20)]
        with torch.no_grad():
            events(fns)
            return dict(zip(names, events(fns)))

    res = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup}
    for tag, (h, w) in (("32x128", (32, 128)), ("16x64", (16, 64))):
        pool = moran_synth.moran_images(moran_synth.POOL, h=h, w=w)
        img = torch.cat([pool] * (a.batch // moran_synth.POOL + 1), 0)[:a.batch].to(dev)
        r = {}
        for mode, code in (("f32", 0), ("x3", 2)):
            _abi.check(_abi.lib.dpmn_set_compute_dtype(code))
            r["native_ms_" + mode], r["native_best_ms_" + mode], r["native_spread_" + mode] = timed(lambda: nat.read(img))
            r["stage_ms_" + mode] = native_stages(img)
        _abi.check(_abi.lib.dpmn_set_compute_dtype(0))
        r["mirror_ms"], r["mirror_best_ms"], r["mirror_spread"] = timed(lambda: mir.read(img))
        r["mirror_stage_ms"] = mirror_stages(img)
        r["speedup_f32"], r["speedup_x3"] = round(r["mirror_ms"] / r["native_ms_f32"], 2), round(r["mirror_ms"] / r["native_ms_x3"], 2)
        r["same_strings"] = nat.read(img) == mir.read(img)
        res[tag] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
