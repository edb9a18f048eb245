#!/usr/bin/env python3
"""What the projective map, the rotation and the curved baseline cost on top of the fx word renderer on one MI355X (main.py
--train_words_warp): prints ONE JSON line and writes it to --out (default profiles/render_warp_bench.json).

One seeded batch of --batch words (utils.render.draw_render_warp from random.Random(2), PIL's built-in font, one atlas; a pool of 16
seeded noise photos of 256 x 512; all three fx kinds and all three warp kinds on for every sample), the SAME draws for both launches,
in one process:
  fx_kernel_us    -- dpmn_render_words_fx_u8 on buffers prepared once (the flat canvases): the entry point's host checks and ONE launch
  warp_kernel_us  -- dpmn_render_words_warp_u8 likewise (the warped canvases, which are larger: their bounding boxes)
  kernel_ratio    -- warp_kernel_us / fx_kernel_us;  per_byte_ratio -- the same per output byte
  fx_call_us, warp_call_us, call_ratio -- the whole Python ops (sizes and tile table on the host, one small upload, the launch)
HIP events around --kernel-reps back-to-back calls after a warm-up, the four alternating over --rounds rounds (30); the median round is
reported, spread = (max - min) / median.  The measurement runs in a child process under a time limit of its own (--timeout seconds);
the parent never opens the GPU."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ["the", "of", "scene", "text", "super", "resolution", "Instinct", "42", "a", "recognition", "wavefront", "x" * 25]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_warp_bench.json"))
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_render_warp: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from dpmn_amd import ops
    from dpmn_amd.utils import render as rd
    if not torch.cuda.is_available():
        print("bench_render_warp: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    at = rd.build_atlases(None)
    rng = np.random.RandomState(3)
    pool = rd.Backgrounds([rng.randint(0, 256, (256, 512, 3)).astype(np.uint8) for _ in range(16)])
    _, cls, lens, params, rows, wrows = rd.draw_render_warp(WORDS, at.n_fonts, random.Random(2), a.batch, rd.RenderFx(rd.FX_KINDS, 1.0, pool, at),
                                                            rd.RenderWarp(rd.WARP_KINDS, 1.0, atlases=at))
    assert (rows[:, rd.FX_FLAGS] == 7).all() and (wrows[:, rd.WP_FLAGS] == 7).all()
    # the two entry points on buffers prepared once: launch after launch, nothing of the Python ops between them
    from dpmn_amd._abi import check, lib, stream
    pad = lambda m: np.ascontiguousarray(np.concatenate((m, np.zeros((a.batch, 1), np.int64)), axis=1))
    m_fx, m_wp = pad(rd.render_meta(cls, lens, params, at)), pad(rd.render_warp_meta(cls, lens, params, wrows, at))
    t_fx, t_wp = ops._tile_table(m_fx[:, 1], m_fx[:, 2], *ops.RENDER_TILE)[0], ops._tile_table(m_wp[:, 1], m_wp[:, 2], *ops.RENDER_TILE)[0]
    host = [cls, lens, params, rows, wrows, m_fx, m_wp, pool.table]
    d_cls, d_lens, d_par, d_fx, d_wp, d_mfx, d_mwp, d_tab, d_tfx, d_twp, d_alpha, d_adv, d_hts, d_pix = (
        torch.from_numpy(x).to(dev) for x in host + [t_fx, t_wp, at.alpha, at.advance, at.height, pool.pixels])
    nbytes = lambda m: int(m[-1, 0] + m[-1, 1] * m[-1, 2] * 3)
    out = torch.empty(max(nbytes(m_fx), nbytes(m_wp)), dtype=torch.uint8, device=dev)
    h_cls, h_lens, h_par, h_fx, h_wp, h_mfx, h_mwp, h_tab = (x.ctypes.data for x in host)
    GH, GW = at.alpha.shape[3], at.alpha.shape[4]

    def fx_kernel():
        check(lib.dpmn_render_words_fx_u8(d_cls.data_ptr(), d_lens.data_ptr(), d_par.data_ptr(), d_fx.data_ptr(), d_alpha.data_ptr(),
                                          d_adv.data_ptr(), d_hts.data_ptr(), d_mfx.data_ptr(), d_tfx.data_ptr(), t_fx.shape[0],
                                          d_pix.data_ptr(), d_pix.numel(), d_tab.data_ptr(), pool.n_photos, out.data_ptr(), out.numel(),
                                          a.batch, at.n_fonts, GH, GW, h_cls, h_lens, h_par, h_fx, h_mfx, h_tab, stream()))

    def warp_kernel():
        check(lib.dpmn_render_words_warp_u8(d_cls.data_ptr(), d_lens.data_ptr(), d_par.data_ptr(), d_fx.data_ptr(), d_wp.data_ptr(),
                                            d_alpha.data_ptr(), d_adv.data_ptr(), d_hts.data_ptr(), d_mwp.data_ptr(), d_twp.data_ptr(),
                                            t_wp.shape[0], d_pix.data_ptr(), d_pix.numel(), d_tab.data_ptr(), pool.n_photos, out.data_ptr(),
                                            out.numel(), a.batch, at.n_fonts, GH, GW, h_cls, h_lens, h_par, h_fx, h_wp, h_mwp, h_tab, stream()))

    calls = {"fx_kernel": fx_kernel, "warp_kernel": warp_kernel,
             "fx_call": lambda: ops.render_words_fx_u8(cls, lens, params, rows, at, pool, device=dev),
             "warp_call": lambda: ops.render_words_warp_u8(cls, lens, params, rows, wrows, at, pool, device=dev)}
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
    res = {"batch": a.batch, "rounds": a.rounds, "kernel_reps": a.kernel_reps, "fx_output_bytes": nbytes(m_fx), "warp_output_bytes": nbytes(m_wp),
           "fx_tiles": int(t_fx.shape[0]), "warp_tiles": int(t_wp.shape[0])}
    for k, t in times.items():
        med = statistics.median(t)
        res[k + "_us"], res[k + "_best_us"], res[k + "_spread"] = round(med, 2), round(min(t), 2), round((max(t) - min(t)) / med, 3)
    res["kernel_ratio"] = round(res["warp_kernel_us"] / res["fx_kernel_us"], 3)
    res["per_byte_ratio"] = round(res["kernel_ratio"] * nbytes(m_fx) / nbytes(m_wp), 3)
    res["call_ratio"] = round(res["warp_call_us"] / res["fx_call_us"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
