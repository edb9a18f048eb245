"""Host side of the ragged-batch resize (``ops.resize_ragged_u8``, csrc/resize.hip): PIL's fixed-point bicubic resample for ANY pair
of sizes -- the coefficient tables, a numpy restatement of the two passes (the CPU reference of the kernel) and the packing of a
batch of images of different sizes into one buffer.  The one owner of the resample core: the comparison images (``utils/display.py``,
enlarging only: 5 taps) and the window cutter (``utils/tile.py``) take it from here.

PIL's ``Image.resize((W, H), BICUBIC)`` on uint8 (libImaging/Resample.c) is two passes, horizontal first, the intermediate rounded
to uint8.  Per output index: a window [xmin, xmin + n) of input pixels and n weights of the a = -0.5 cubic over a support of
2 * max(scale, 1), normalised in double and converted to int with 22 fraction bits; a pixel is clip8((2^21 + sum in * k) >> 22).
Shrinking widens the support by the scale factor: ksize = 2 * ceil(2 * scale) + 1 taps.  No GPU needed: importable on any machine.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Resample.c: 8 bits of pixel, 2 bits of head room for the overshoot of the cubic
MAX_SIDE = 8192               # per image side; 255 * sum |k| + 2^21 stays far below 2^31 for every pair up to here (tests/test_resize.py)
MAX_PACKED_BYTES = 2 ** 31 - 1


def _bicubic(x, a=-0.5):
    """Resample.c's bicubic_filter on an array, the same operations in the same order per branch."""
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=4096)
def pil_resample_tables(insz, outsz):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for one axis and any positive sizes -> int32 (outsz, 2 + ksize),
    read-only: per output index [xmin, n, k_0 .. k_{ksize-1}] (k_j = 0 for j >= n), 22 fraction bits.  Float64 in PIL's operation
    order: the weight sum grows tap by tap, each tap is divided by it, then rounded with +-0.5.  Vectorised over the output index
    (a loop over the taps only); tests/helpers.py restates it per index.  Cached per size pair."""
    insz, outsz = int(insz), int(outsz)
    if insz < 1 or outsz < 1:
        raise ValueError("pil_resample_tables: sizes must be positive, got %d -> %d" % (insz, outsz))
    scale = filterscale = float(insz) / outsz
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(outsz, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int): truncation
    n = np.minimum((center + support + 0.5).astype(np.int64), insz) - xmin
    k = np.zeros((outsz, ksize), np.float64)
    ww = np.zeros(outsz, np.float64)
    for x in range(ksize):
        live = x < n
        w = np.where(live, _bicubic((x + xmin - center + 0.5) * ss), 0.0)
        k[:, x] = w
        ww = np.where(live, ww + w, ww)
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    fixed = k * (1 << PRECISION_BITS)
    tab = np.empty((outsz, 2 + ksize), np.int32)
    tab[:, 0], tab[:, 1] = xmin, n
    tab[:, 2:] = np.where(k < 0, -0.5 + fixed, 0.5 + fixed).astype(np.int64)   # (int): truncation
    tab.setflags(write=False)
    return tab


def resample_axis0(img, tab):
    """One pass along axis 0 of a uint8 array with a table of pil_resample_tables (int64 accumulation: no assumption on the sums)."""
    src = img.astype(np.int64)
    out = np.empty((tab.shape[0],) + img.shape[1:], np.uint8)
    for xx in range(tab.shape[0]):
        xmin, n = int(tab[xx, 0]), int(tab[xx, 1])
        k = tab[xx, 2:2 + n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + n] * k).sum(0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_resize_u8(img, out_h, out_w):
    """img (h, w[, C]) uint8 -> (out_h, out_w[, C]) uint8 = np.asarray(Image.fromarray(img).resize((out_w, out_h), BICUBIC)) for any
    sizes, bit for bit (tests/test_resize.py): horizontal pass, uint8 intermediate, vertical pass; an axis whose sizes are equal goes
    through its (identity) table like any other.  The CPU reference of ops.resize_ragged_u8 and of the LR rows of
    ops.display_triple."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    hor = np.swapaxes(resample_axis0(np.swapaxes(img, 0, 1), pil_resample_tables(w, out_w)), 0, 1)
    return resample_axis0(hor, pil_resample_tables(h, out_h))


def check_image(im, what="image"):
    """(h, w) of an (h, w, 3) uint8 array with sides 1 .. MAX_SIDE; ValueError otherwise."""
    shape = tuple(getattr(im, "shape", ()))
    if len(shape) != 3 or shape[2] != 3 or getattr(im, "dtype", None) != np.uint8:
        raise ValueError("pack_ragged: %s is not an (h, w, 3) uint8 array (shape %s, dtype %s)" % (what, shape, getattr(im, "dtype", None)))
    h, w = shape[:2]
    if h < 1 or w < 1:
        raise ValueError("pack_ragged: %s has an empty side (%d x %d)" % (what, h, w))
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError("pack_ragged: %s is %d x %d, sides above %d are not resized" % (what, h, w, MAX_SIDE))
    return h, w


def pack_ragged(images, pin=None):
    """A list of (h, w, 3) uint8 arrays -> (packed, meta): one 1-D uint8 tensor holding the images back to back (HWC) and an int64
    tensor (B, 3) of (byte offset, h, w) per image.  pin=None: the packed tensor is pinned when CUDA is available (one asynchronous
    upload per batch); pin=False inside data-loader workers, whose batches the loader pins itself.  ValueError for an empty list, an
    image that is not (h, w, 3) uint8, a side of 0 or above MAX_SIDE, or more than 2^31 - 1 bytes in all -- checked before anything is
    copied."""
    import torch
    if len(images) == 0:
        raise ValueError("pack_ragged: an empty batch")
    meta = np.empty((len(images), 3), np.int64)
    total = 0
    for i, im in enumerate(images):
        h, w = check_image(im, "image %d" % i)
        meta[i] = total, h, w
        total += h * w * 3
        if total > MAX_PACKED_BYTES:
            raise ValueError("pack_ragged: the batch holds more than 2^31 - 1 bytes")
    if pin is None:
        pin = torch.cuda.is_available()
    packed = torch.empty(total, dtype=torch.uint8, pin_memory=bool(pin))
    flat = packed.numpy()
    for (off, h, w), im in zip(meta, images):
        flat[off:off + h * w * 3] = np.asarray(im).reshape(-1)
    return packed, torch.from_numpy(meta)
