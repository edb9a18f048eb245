#!/usr/bin/env python3
"""What rendering the HR images of a batch from a word list costs on one MI355X (main.py --train_words): prints ONE JSON line.

A batch of --batch words drawn with utils.render.draw_render (PIL's built-in font, one atlas), in the same run:
  render_call_us  -- ops.render_words_u8 alone (the size computation and tile table on the host, one small upload, ONE launch), HIP
                     events around --kernel-reps back-to-back calls
  words_ms        -- one whole sr_batches batch of a render collate: the draws, the render, then the degrade / resize / collate chain
  folder_ms       -- the same chain fed like --train_hr_dir: the SAME images, rendered beforehand, handed over as decoded PIL images
                     (alignCollate_realWTLAMask(degrade=True) packs them on the host, one upload); file decoding is not counted
Wall-clock times end in a device synchronise; median of --reps batches after --warmup, spread = (max - min) / median.  The measurement
runs in a child process under a time limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORDS = ["the", "of", "scene", "text", "super", "resolution", "Instinct", "42", "a", "recognition", "wavefront", "x" * 25]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
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
            print("bench_render: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import torch
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import render as rd
    if not torch.cuda.is_available():
        print("bench_render: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    H, W, scale = 32, 128, 2
    at = rd.build_atlases(None)
    kw = dict(imgH=H, imgW=W, down_sample_scale=scale, mask=True, gpu_finish=True, gpu_resize=True, degrade=True, cutblur=True)

    def timed(col, item):
        loader = type("Loader", (), {"collate_fn": col})()
        random.seed(1)
        tot = []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = col(item)
            loader.__class__.__iter__ = lambda self, out=out: iter([out])
            list(tz.sr_batches(loader, dev, True))
            torch.cuda.synchronize()
            if r >= a.warmup:
                tot.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(tot)
        return round(med, 3), round(min(tot), 3), round((max(tot) - min(tot)) / med, 3)

    labels, cls, lens, params = rd.draw_render(WORDS, at.n_fonts, random.Random(2), n=a.batch)
    res = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "out_hw": [H, W], "scale": scale}
    res["words_ms"], res["words_best_ms"], res["words_spread"] = timed(tz.alignCollate_realWTLAMask(render=(WORDS, at), **kw),
                                                                       [(None, None, None, None, w) for w in labels])
    packed, meta = ops.render_words_u8(cls, lens, params, at, device=dev)
    flat = packed.cpu().numpy()
    images = [Image.fromarray(flat[o:o + h * w * 3].reshape(h, w, 3)) for o, h, w in meta.tolist()]
    res["folder_ms"], res["folder_best_ms"], res["folder_spread"] = timed(tz.alignCollate_realWTLAMask(**kw),
                                                                          [(im, im, None, None, w) for im, w in zip(images, labels)])
    for _ in range(10):
        ops.render_words_u8(cls, lens, params, at, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(a.kernel_reps):
        ops.render_words_u8(cls, lens, params, at, device=dev)
    ev1.record()
    torch.cuda.synchronize()
    res["render_call_us"] = round(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps, 2)
    res["output_bytes"] = int(packed.numel())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
