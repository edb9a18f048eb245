"""Host side of the LR / SR / HR comparison images (``tripple_display`` / ``test_display``, interfaces/base.py:275-326 of the
reference): the coefficient tables of PIL's fixed-point bicubic resample, a numpy restatement of the whole triple (the CPU
reference of ``ops.display_triple``, csrc/display.hip) and the file-name rule.  No torch, no GPU: importable on any machine.

PIL's ``Image.resize((W, H), BICUBIC)`` on uint8 (libImaging/Resample.c) is two passes, horizontal first, the intermediate rounded
to uint8.  Per output index: a window [xmin, xmin + n) of input pixels and n weights of the a = -0.5 cubic over a support of
2 * max(scale, 1), normalised in double and converted to int with 22 fraction bits; a pixel is clip8((2^21 + sum in * k) >> 22).
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Resample.c: 8 bits of pixel, 2 bits of head room for the overshoot of the cubic


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def pil_bicubic_tables(insz, outsz):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for one axis -> int32 (outsz, 2 + ksize), read-only: per output
    index [xmin, n, k_0 .. k_{ksize-1}] (k_j = 0 for j >= n).  Built in float64 like PIL; cached per size pair.  Enlarging and equal
    sizes only (ksize = 5; int32 accumulation in the kernel holds for scale <= 1)."""
    insz, outsz = int(insz), int(outsz)
    if insz < 1 or outsz < 1:
        raise ValueError("pil_bicubic_tables: sizes must be positive, got %d -> %d" % (insz, outsz))
    if insz > outsz:
        raise NotImplementedError("pil_bicubic_tables: shrinking (%d -> %d) is not built: the comparison image only enlarges the LR "
                                  "input" % (insz, outsz))
    scale = filterscale = float(insz) / outsz
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    tab = np.zeros((outsz, 2 + ksize), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        tab[xx, 0], tab[xx, 1] = xmin, xmax
        for x, w in enumerate(k):
            tab[xx, 2 + x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
    tab.setflags(write=False)
    return tab


def _resample_axis0(img, tab):
    """One pass along axis 0 of a uint8 array with a table of pil_bicubic_tables (int64 accumulation: no assumption on the sums)."""
    src = img.astype(np.int64)
    out = np.empty((tab.shape[0],) + img.shape[1:], np.uint8)
    for xx in range(tab.shape[0]):
        xmin, n = int(tab[xx, 0]), int(tab[xx, 1])
        k = tab[xx, 2:2 + n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + n] * k).sum(0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_bicubic_resize_u8(img, out_h, out_w):
    """img (h, w[, C]) uint8 -> (out_h, out_w[, C]) uint8 = np.asarray(Image.fromarray(img).resize((out_w, out_h), BICUBIC)), bit for
    bit (tests/test_display.py): horizontal pass, uint8 intermediate, vertical pass."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    hor = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), pil_bicubic_tables(w, out_w)), 0, 1)
    return _resample_axis0(hor, pil_bicubic_tables(h, out_h))


def quantize_lr(x):
    """ToPILImage on a float tensor: x.mul(255).byte() -- one float32 multiply, then truncation.  Values outside [0, 1] (undefined in
    the reference: a float -> uint8 cast out of range) are clamped to [0, 255] first; NaN gives 0."""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    return np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8)


def quantize_sr(x):
    """torchvision save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two separately rounded float32 operations (no FMA),
    then truncation.  NaN gives 0."""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    v = v + np.float32(0.5)
    return np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8)


def triple_reference(image_in, image_out, image_target, sel):
    """The CPU restatement of ops.display_triple on numpy arrays: (B, >=3, h, w), (B, >=3, H, W) x 2, indices -> (n, 3 H, W, 3)
    uint8.  The enlarged LR passes ToTensor (/ 255) and save_image's quantisation again in the reference: the identity on 0..255."""
    image_in, image_out, image_target = (np.asarray(a, np.float32) for a in (image_in, image_out, image_target))
    H, W = image_target.shape[-2:]
    out = np.empty((len(sel), 3 * H, W, 3), np.uint8)
    for j, b in enumerate(sel):
        out[j, :H] = pil_bicubic_resize_u8(quantize_lr(image_in[b, :3]).transpose(1, 2, 0), H, W)
        out[j, H:2 * H] = quantize_sr(image_out[b, :3]).transpose(1, 2, 0)
        out[j, 2 * H:] = quantize_sr(image_target[b, :3]).transpose(1, 2, 0)
    return out


def image_name(pred_lr, pred_sr, label):
    """base.py:296-297 / 323-324: '<LR string>_<SR string>_<label>_.png' with every '/' removed (the strings come from a
    recogniser and from the data set: a '/' would name a directory)."""
    return (str(pred_lr) + '_' + str(pred_sr) + '_' + str(label) + '_.png').replace('/', '')
