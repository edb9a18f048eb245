"""Synthetic weights and inputs for the ASTER recogniser's fixtures and tests (host code, no reference import).

The plain name rule of utils/synth.py leaves the attention decoder degenerate (every image decodes to nearly the same string, no
EOS in 100 steps, beams whose states collapse onto each other and tie exactly), and its stn_fc2 puts all control points near the
image corner.  `aster_fill_` applies the name rule and then overrides, by name-seeded uniform draws as well:
  * tps.*: the constructed buffers are kept (they are derived constants, not weights);
  * stn_head.stn_fc2: the identity control points of STNHead.init_stn (margin 0.01) plus a small image-dependent part;
  * decoder: wider ranges for wEmbed (sharp attention), tgt_embedding (the previous symbol matters), fc (decisive log-softmax
    margins), xEmbed and the GRU's input weights (the image matters), and an EOS bias in fc (sequences end).
`aster_images` draws soft bar images (vertical strokes of image-specific position, width and brightness, low-pass filtered)."""
import math

import numpy as np
import torch

from . import synth

D = "decoder.decoder."
EOS = 94


def aster_fill_(sd, seed=81):
    tps = {k: v.clone() for k, v in sd.items() if k.startswith("tps.")}      # derived constants (kernel inverse, zero padding rows)
    synth.synth_fill_(sd, seed)
    for k, v in tps.items():
        sd[k].copy_(v)
    u = lambda name, a: synth.uniform("aster::" + name, sd[name].shape, -a, a, seed)
    half = 10
    xs = np.linspace(0.01, 0.99, half)
    pts = np.concatenate([np.stack([xs, np.full(half, 0.01)], 1), np.stack([xs, np.full(half, 0.99)], 1)], 0).astype(np.float32)
    sd["stn_head.stn_fc2.weight"].copy_(u("stn_head.stn_fc2.weight", 0.02))
    sd["stn_head.stn_fc2.bias"].copy_(torch.from_numpy(pts).reshape(-1) + u("stn_head.stn_fc2.bias", 0.02))
    a = math.sqrt(3.0 / 512)
    sd[D + "attention_unit.wEmbed.weight"].copy_(u(D + "attention_unit.wEmbed.weight", 6 * a))
    sd[D + "attention_unit.xEmbed.weight"].copy_(u(D + "attention_unit.xEmbed.weight", 8 * a))
    sd[D + "attention_unit.sEmbed.weight"].copy_(u(D + "attention_unit.sEmbed.weight", 3 * a))
    sd[D + "tgt_embedding.weight"].copy_(u(D + "tgt_embedding.weight", 1.0))
    sd[D + "gru.weight_ih_l0"].copy_(u(D + "gru.weight_ih_l0", 4 * math.sqrt(3.0 / 1024)))
    sd[D + "gru.weight_hh_l0"].copy_(u(D + "gru.weight_hh_l0", 2 * a))
    sd[D + "fc.weight"].copy_(u(D + "fc.weight", 30 * a))
    sd[D + "fc.bias"].copy_(u(D + "fc.bias", 0.5))
    sd[D + "fc.bias"][EOS] += 5.0
    return sd


POOL = 32


def _box_blur(x, k, dim):
    """one pass of a length-k box filter along `dim` with replicated borders"""
    pad = [k // 2, k // 2, 0, 0] if dim == 3 else [0, 0, k // 2, k // 2]
    x = torch.nn.functional.pad(x, pad, mode="replicate")
    return x.unfold(dim, k, 1).mean(-1)


def aster_images(ids, h=32, w=128, seed=82):
    """(len(ids), 3, h, w) images in [0, 1]: members `ids` of a fixed pool of POOL images of soft bars (an int n: the first n).
    The bars are band-limited on purpose: three box passes of 11 pixels along x and of 7 along y (about a Gaussian of sigma 5.5 / 3.5
    pixels), a contrast of 0.3 and a fade to mid-grey at the borders keep the steepest slope near 0.05 per pixel in the normalised
    [-1, 1] range, border ramp of the zero padding included.  The TPS sums leave
    about 1e-3 pixel of fp32 rounding in a source coordinate (two summation orders differ by that much), so a sampled value moves by
    slope x 1e-3: only images this smooth can be compared at 1e-4 after the rectification.  (A recogniser's inputs here are
    super-resolved 16 x 64 images, which are smooth as well.)"""
    ids = list(range(ids)) if isinstance(ids, int) else [int(i) for i in ids]
    assert all(0 <= i < POOL for i in ids)
    out = 0.45 + 0.1 * synth.uniform("aster_img_noise", (POOL, 3, h, w), 0, 1, seed)
    for i in range(POOL):
        p = synth.uniform("aster_img_bars%d" % i, (12, 6), 0, 1, seed)
        for k in range(3 + int(p[0, 5] * 9)):
            x0, wd = int(p[k, 0] * (w - 16)), 6 + int(p[k, 1] * 14)
            y0, y1 = int(p[k, 2] * h * 0.4), h - int(p[k, 3] * h * 0.4)
            out[i, :, y0:y1, x0:x0 + wd] += (0.15 + 0.15 * p[k, 4]) * torch.tensor([1.0, 0.9 - 0.5 * p[k, 5], 0.6 + 0.4 * p[k, 1]]).view(3, 1, 1)
    out = out.clamp_(0, 0.85)
    for _ in range(3):
        out = _box_blur(_box_blur(out, 11, 3), 7, 2)
    # fade to mid-grey (0 in the normalised range) at the borders: grid_sample pads with zeros, so a border pixel of value v is a
    # ramp of height v over one pixel for every sample that lands within half a pixel of the edge
    wx = torch.sin(torch.clamp(torch.minimum(torch.arange(w) + 0.5, w - 0.5 - torch.arange(w)) / 20.0, 0, 1) * (math.pi / 2)) ** 2
    wy = torch.sin(torch.clamp(torch.minimum(torch.arange(h) + 0.5, h - 0.5 - torch.arange(h)) / 8.0, 0, 1) * (math.pi / 2)) ** 2
    out = 0.5 + (out - 0.5) * (wy.view(1, 1, h, 1) * wx.view(1, 1, 1, w))
    return out[ids].contiguous()
