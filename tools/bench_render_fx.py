#!/usr/bin/env python3
"""What the outline, the drop shadow and the photo background cost on top of the plain word renderer on one MI355X (main.py
--train_words_fx): prints ONE JSON line.

One seeded batch of --batch words (utils.render.draw_render_fx from random.Random(2), PIL's built-in font, one atlas; a pool of 16
seeded noise photos of 256 x 512), the SAME words and render parameters for both calls, in one process:
  plain_kernel_us -- dpmn_render_words_u8 on buffers prepared once: the entry point's host checks and ONE launch, launch after launch
  fx_kernel_us    -- dpmn_render_words_fx_u8 likewise, all three kinds on for every sample
  kernel_ratio    -- fx_kernel_us / plain_kernel_us: the number to look at
  plain_call_us, fx_call_us, call_ratio -- the whole Python ops (sizes and tile table on the host, one small upload, the launch)
HIP events around --kernel-reps back-to-back calls after a warm-up, the four alternating over --rounds rounds; the median round is
reported, spread = (max - min) / median.  The measurement runs in a child process under a time limit of its own (--timeout seconds);
the parent never opens the GPU."""
import argparse
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORDS = ["the", "of", "scene", "text", "super", "resolution", "Instinct", "42", "a", "recognition", "wavefront", "x" * 25]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
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
            print("bench_render_fx: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from dpmn_amd import ops
    from dpmn_amd.utils import render as rd
    if not torch.cuda.is_available():
        print("bench_render_fx: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    at = rd.build_atlases(None)
    rng = np.random.RandomState(3)
    pool = rd.Backgrounds([rng.randint(0, 256, (256, 512, 3)).astype(np.uint8) for _ in range(16)])
    _, cls, lens, params, rows = rd.draw_render_fx(WORDS, at.n_fonts, random.Random(2), a.batch, rd.RenderFx(rd.FX_KINDS, 1.0, pool, at))
    assert (rows[:, rd.FX_FLAGS] == 7).all()
    # the two entry points on buffers prepared once: launch after launch, nothing of the Python ops between them
    from dpmn_amd._abi import check, lib, stream
    m = np.ascontiguousarray(np.concatenate((rd.render_meta(cls, lens, params, at), np.zeros((a.batch, 1), np.int64)), axis=1))
    tiles, _ = ops._tile_table(m[:, 1], m[:, 2], *ops.RENDER_TILE)
    host = [cls, lens, params, rows, m, pool.table]
    d_cls, d_lens, d_par, d_fx, d_m, d_tab, d_til, d_alpha, d_adv, d_hts, d_pix = (
        torch.from_numpy(x).to(dev) for x in host + [tiles, at.alpha, at.advance, at.height, pool.pixels])
    out = torch.empty(int(m[-1, 0] + m[-1, 1] * m[-1, 2] * 3), dtype=torch.uint8, device=dev)
    h_cls, h_lens, h_par, h_fx, h_m, h_tab = (x.ctypes.data for x in host)
    GH, GW = at.alpha.shape[3], at.alpha.shape[4]

    def plain_kernel():
        check(lib.dpmn_render_words_u8(d_cls.data_ptr(), d_lens.data_ptr(), d_par.data_ptr(), d_alpha.data_ptr(), d_adv.data_ptr(),
                                       d_hts.data_ptr(), d_m.data_ptr(), d_til.data_ptr(), tiles.shape[0], out.data_ptr(), out.numel(),
                                       a.batch, at.n_fonts, GH, GW, h_cls, h_lens, h_par, h_m, stream()))

    def fx_kernel():
        check(lib.dpmn_render_words_fx_u8(d_cls.data_ptr(), d_lens.data_ptr(), d_par.data_ptr(), d_fx.data_ptr(), d_alpha.data_ptr(),
                                          d_adv.data_ptr(), d_hts.data_ptr(), d_m.data_ptr(), d_til.data_ptr(), tiles.shape[0],
                                          d_pix.data_ptr(), d_pix.numel(), d_tab.data_ptr(), pool.n_photos, out.data_ptr(), out.numel(),
                                          a.batch, at.n_fonts, GH, GW, h_cls, h_lens, h_par, h_fx, h_m, h_tab, stream()))

    calls = {"plain_kernel": plain_kernel, "fx_kernel": fx_kernel,
             "plain_call": lambda: ops.render_words_u8(cls, lens, params, at, device=dev),
             "fx_call": lambda: ops.render_words_fx_u8(cls, lens, params, rows, at, pool, device=dev)}
    for f in calls.values():
        for _ in range(20):
            f()
    times = {k: [] for k in calls}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(a.kernel_reps):
                f()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps)
    res = {"batch": a.batch, "rounds": a.rounds, "kernel_reps": a.kernel_reps, "output_bytes": int(out.numel()), "tiles": int(tiles.shape[0]),
           "pool_bytes": int(pool.pixels.size)}
    for k, t in times.items():
        med = statistics.median(t)
        res[k + "_us"], res[k + "_best_us"], res[k + "_spread"] = round(med, 2), round(min(t), 2), round((max(t) - min(t)) / med, 3)
    res["kernel_ratio"] = round(res["fx_kernel_us"] / res["plain_kernel_us"], 3)
    res["call_ratio"] = round(res["fx_call_us"] / res["plain_call_us"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
