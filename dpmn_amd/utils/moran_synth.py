"""Synthetic weights and inputs for the MORAN recogniser's fixtures and tests (host code, no reference import).

The plain name rule of utils/synth.py (like PyTorch's default init) leaves the attention decoder degenerate: every image decodes to
nearly the same 20 ids.  `moran_fill_` applies the name rule and then overrides, by name-seeded uniform draws as well:
  * MORN.cnn.15 / 16 (the last conv and its BatchNorm): scaled so that the accumulated offsets are a few percent of the image height
    -- not trivially zero, and small enough that no pixel samples wholly outside the image;
  * ASRN.cnn conv2 BatchNorm scales x 0.5: the features stay of order 1 .. 10 through the 24 residual blocks;
  * ASRN.attentionL2R / R2L: wider ranges for score (sharp attention), i2h and the GRU's input weights (the image matters),
    char_embeddings (the previous symbol matters), generator (decisive margins), and a '$' bias in generator (strings end).
`moran_images` draws soft bar images like utils/aster_synth.py aster_images from a seeded pool of any size."""
import math

import torch

from . import synth
from .aster_synth import _box_blur

EOS = 36          # '$', the last class of digits + lowercase + '$'


def moran_fill_(sd, seed=91):
    synth.synth_fill_(sd, seed)
    u = lambda name, a: synth.uniform("moran::" + name, sd[name].shape, -a, a, seed)
    sd["MORN.cnn.15.weight"].copy_(u("MORN.cnn.15.weight", 2.0 * math.sqrt(3.0 / 144)))
    sd["MORN.cnn.16.weight"].fill_(0.05)
    sd["MORN.cnn.16.bias"].fill_(0.0)
    sd["MORN.cnn.16.running_mean"].fill_(0.0)
    sd["MORN.cnn.16.running_var"].fill_(1.0)
    for k in sd:      # damp the residual branches: 24 blocks without a ReLU inside would otherwise grow the features past 100, where one
        if k.startswith("ASRN.cnn.block") and k.endswith("conv2.1.weight"):      # fp32 rounding alone exceeds the 1e-4 absolute bar
            sd[k].mul_(0.5)
    for k in ("ASRN.rnn.0.rnn.weight_ih_l0", "ASRN.rnn.0.rnn.weight_ih_l0_reverse"):      # ... and the first BiLSTM still sees the image
        sd[k].mul_(12.0)
    a = math.sqrt(3.0 / 256)
    for side in ("L2R", "R2L"):
        p = "ASRN.attention%s." % side
        sd[p + "attention_cell.score.weight"].copy_(u(p + "attention_cell.score.weight", 6 * a))
        sd[p + "attention_cell.i2h.weight"].copy_(u(p + "attention_cell.i2h.weight", 8 * a))
        sd[p + "attention_cell.h2h.weight"].copy_(u(p + "attention_cell.h2h.weight", 3 * a))
        sd[p + "char_embeddings"].copy_(u(p + "char_embeddings", 1.0))
        sd[p + "attention_cell.rnn.weight_ih"].copy_(u(p + "attention_cell.rnn.weight_ih", 4 * math.sqrt(3.0 / 512)))
        sd[p + "attention_cell.rnn.weight_hh"].copy_(u(p + "attention_cell.rnn.weight_hh", 2 * a))
        sd[p + "generator.weight"].copy_(u(p + "generator.weight", 12 * a))
        sd[p + "generator.bias"].copy_(u(p + "generator.bias", 0.5))
        sd[p + "generator.bias"][EOS] += 2.5
    return sd


POOL = 64


def moran_images(ids, h=32, w=128, seed=92, pool=POOL):
    """(len(ids), 3, h, w) images in [0, 1]: members `ids` of a seeded pool of `pool` images of soft bars (an int n: the first n).
    Band-limited (three box passes along x and y), contrast 0.3, faded to mid-grey at the borders: grid_sample pads with zeros, so a
    bright border pixel is a ramp of its height over one pixel for every sample within half a pixel of the edge, and a hard edge turns
    1e-3 pixel of coordinate rounding into 1e-3 of image error (measured for ASTER, utils/aster_synth.py)."""
    ids = list(range(ids)) if isinstance(ids, int) else [int(i) for i in ids]
    assert all(0 <= i < pool for i in ids)
    kx, ky = (11, 7) if h >= 32 else (5, 3)
    out = 0.45 + 0.1 * synth.uniform("moran_img_noise", (pool, 3, h, w), 0, 1, seed)
    for i in range(pool):
        p = synth.uniform("moran_img_bars%d" % i, (12, 6), 0, 1, seed)
        for k in range(3 + int(p[0, 5] * 9)):
            x0, wd = int(p[k, 0] * (w - w // 8)), w // 21 + int(p[k, 1] * (w // 9))
            y0, y1 = int(p[k, 2] * h * 0.4), h - int(p[k, 3] * h * 0.4)
            out[i, :, y0:y1, x0:x0 + wd] += (0.15 + 0.15 * p[k, 4]) * torch.tensor([1.0, 0.9 - 0.5 * p[k, 5], 0.6 + 0.4 * p[k, 1]]).view(3, 1, 1)
    out = out.clamp_(0, 0.85)
    for _ in range(3):
        out = _box_blur(_box_blur(out, kx, 3), ky, 2)
    wx = torch.sin(torch.clamp(torch.minimum(torch.arange(w) + 0.5, w - 0.5 - torch.arange(w)) / (w / 6.4), 0, 1) * (math.pi / 2)) ** 2
    wy = torch.sin(torch.clamp(torch.minimum(torch.arange(h) + 0.5, h - 0.5 - torch.arange(h)) / (h / 4.0), 0, 1) * (math.pi / 2)) ** 2
    out = 0.5 + (out - 0.5) * (wy.view(1, 1, h, 1) * wx.view(1, 1, 1, w))
    return out[ids].half().float().contiguous()      # fp16-representable: the fixture stores them losslessly in half the bytes
