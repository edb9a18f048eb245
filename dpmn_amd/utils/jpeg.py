"""JPEG artefacts for the synthesised LR training images (dataset/dataset.py:559 `JPEG_compress`; the call on the resized image at
:1298-1300 is commented out there because a cv2 round trip per image was too slow for its loader): the bytes an RGB image has after
it was written as a baseline JPEG and read back, without the file in between.  `jpeg_roundtrip_u8` is the NORMATIVE restatement of

    buf = io.BytesIO(); Image.fromarray(img).save(buf, 'JPEG', quality=q); np.asarray(Image.open(buf))

with PIL's defaults on libjpeg / libjpeg-turbo (baseline, 4:2:0, the standard tables, the islow DCT, fancy upsampling), byte for byte
(tests/test_jpeg.py), and the CPU reference of the kernel (csrc/jpeg.hip through ops.jpeg_roundtrip_u8).  Huffman coding is lossless,
so no entropy coding is involved; the stages, all in int32:

  jccolor.c   RGB -> YCbCr, 16-bit fixed-point tables
  jcprepct.c / jcsample.c   edge replication to whole 16 x 16 MCUs (columns, and rows up to an even count, before the downsample;
              the remaining rows after it, so below an image of even height the last CHROMA row repeats); h2v2 chroma downsample,
              bias 1, 2, 1, 2 .. along a row
  jcdctmgr.c / jfdctint.c   level shift, forward islow DCT (output scaled by 8)
  jcparam.c   the tables of `quality` (jpeg_quality_scaling, force_baseline: 1 .. 255); quantise = divide by 8 q, half away from zero
  jdcoefct.c / jidctint.c   dequantise, inverse islow DCT, + 128, clamp
  jdsample.c  h2v2 fancy (triangle) upsampling: 3 : 1 vertically with the nearer neighbour row (the image's first / last chroma row
              stands in above / below it), then 3 : 1 horizontally with rounding 8 / 7, first and last column 4 : 0; a chroma plane of
              at most 2 columns (image width <= 4) is replicated 2 x 2 instead, as jinit_upsampler chooses
  jdcolor.c   YCbCr -> RGB, the decoder's tables

Pure NumPy: importable on any machine.
"""
import random

import numpy as np

MAX_SIDE = 1024
MCU = 16

STD_LUMINANCE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int32)
STD_CHROMINANCE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int32)

# jfdctint.c / jidctint.c: CONST_BITS = 13, PASS1_BITS = 2, FIX(x) = round(x * 2^13)
CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172

SCALEBITS = 16


def _fix16(x):
    return int(x * (1 << SCALEBITS) + 0.5)


def draw_jpeg(n, lo, hi, prob, rng=random):
    """The (n,) int32 qualities of n images, drawn from `rng` (Python's `random` module or a random.Random) image by image in this
    order: first `rng.random()`; when that draw is below `prob`, `rng.randint(lo, hi)` follows and is the image's quality; otherwise
    no second draw is made and the entry is 0 (the image is left alone).  --train_state depends on this order."""
    q = np.zeros((n,), np.int32)
    for i in range(n):
        if rng.random() < prob:
            q[i] = rng.randint(lo, hi)
    return q


def jpeg_setting(args):
    """(lo, hi, prob) of main.py's --jpeg_degrade LO,HI and --jpeg_prob P, or None when the flag is off.  ValueError with one clear line
    for a malformed value, LO > HI, a quality outside 1 .. 100 or P outside 0 .. 1."""
    spec = getattr(args, "jpeg_degrade", None)
    if spec is None or spec is False or spec == "":
        return None
    try:
        lo, hi = (int(v) for v in (spec.split(",") if isinstance(spec, str) else spec))
    except (TypeError, ValueError):
        raise ValueError("--jpeg_degrade takes two integers LO,HI (for example 30,95), got %r" % (spec,)) from None
    prob = getattr(args, "jpeg_prob", None)
    prob = 0.5 if prob is None else float(prob)
    if not (1 <= lo <= hi <= 100):
        raise ValueError("--jpeg_degrade LO,HI needs 1 <= LO <= HI <= 100, got %d,%d" % (lo, hi))
    if not (0.0 <= prob <= 1.0):
        raise ValueError("--jpeg_prob needs a probability in 0 .. 1, got %r" % (prob,))
    return lo, hi, prob


def quant_tables(quality):
    """(luminance, chrominance) int32 (64,) tables in natural order: jpeg_set_quality(quality, force_baseline = TRUE)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int32) for t in (STD_LUMINANCE, STD_CHROMINANCE))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jpeg_fdct_islow on the 8 arrays d[0..7]."""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        o[0], o[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, sh)
    o[6] = _descale(z1 + t12 * (-F_1_847), sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961) + z5, z4 * (-F_0_390) + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh), _descale(t6 + z2 + z3, sh), _descale(t7 + z1 + z4, sh)
    return o


def _idct_pass(d, first):
    """One pass of jpeg_idct_islow on the 8 arrays d[0..7] (dequantised coefficients, then the workspace)."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * F_0_541
    t2, t3 = z1 + z3 * (-F_1_847), z1 + z2 * F_0_765
    t0, t1 = (d[0] + d[4]) << CONST_BITS, (d[0] - d[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961) + z5, z4 * (-F_0_390) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS + 3
    return [_descale(t10 + t3, sh), _descale(t11 + t2, sh), _descale(t12 + t1, sh), _descale(t13 + t0, sh),
            _descale(t13 - t0, sh), _descale(t12 - t1, sh), _descale(t11 - t2, sh), _descale(t10 - t3, sh)]


def _codec_plane(plane, table):
    """(H, W) int32 samples 0 .. 255, H and W multiples of 8 -> the samples after DCT, quantisation with `table` and back."""
    H, W = plane.shape
    x = (plane - 128).reshape(H // 8, 8, W // 8, 8)                                       # (block row, r, block column, c)
    x = np.stack(_fdct_pass([x[:, :, :, c] for c in range(8)], True), axis=3)           # rows
    x = np.stack(_fdct_pass([x[:, r] for r in range(8)], False), axis=1)                # columns
    q8 = (table.reshape(8, 8) << 3)[None, :, None, :]
    x = np.where(x < 0, -((-x + (q8 >> 1)) // q8), (x + (q8 >> 1)) // q8)               # half away from zero
    x = x * table.reshape(8, 8)[None, :, None, :]
    x = np.stack(_idct_pass([x[:, r] for r in range(8)], True), axis=1)                 # columns
    x = np.stack(_idct_pass([x[:, :, :, c] for c in range(8)], False), axis=3)          # rows
    return np.clip(x + 128, 0, 255).reshape(H, W).astype(np.int32)


def _upsample_h2v2(c, ch, cw):
    """The ch x cw real samples of a decoded chroma plane -> (2 ch, 2 cw) int32."""
    c = c[:ch, :cw]
    if cw <= 2:                                         # jinit_upsampler: fancy upsampling needs downsampled_width > 2
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    up, down = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for v, other in ((0, up), (1, down)):
        s = 3 * c + other                                                               # colsum
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[v::2, 0::2] = (3 * s + left + 8) >> 4                                        # column 0: (4 s + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4                                       # last column: (4 s + 7) >> 4
    return out


def jpeg_roundtrip_u8(img, quality):
    """(h, w, 3) uint8 RGB -> (h, w, 3) uint8: the image after PIL wrote it as a JPEG of `quality` (1 .. 100) and read it back.
    quality 0: the image is left alone (a copy).  Sides 1 .. 1024."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("jpeg_roundtrip_u8: expected (h, w, 3) uint8, got %s %s" % (img.shape, img.dtype))
    h, w = img.shape[:2]
    quality = int(quality)
    if not (0 <= quality <= 100) or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("jpeg_roundtrip_u8: quality 0 .. 100 and sides 1 .. %d, got quality %d, %d x %d" % (MAX_SIDE, quality, h, w))
    if quality == 0:
        return img.copy()
    Hp, Wp = -(-h // MCU) * MCU, -(-w // MCU) * MCU
    # the image's rows are replicated to an even count only: below that the DOWNSAMPLED rows are replicated (jcprepct.c)
    x = np.pad(img.astype(np.int32), ((0, h & 1), (0, Wp - w), (0, 0)), mode='edge')
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    half, off = 1 << (SCALEBITS - 1), 128 << SCALEBITS
    y = (_fix16(0.29900) * r + _fix16(0.58700) * g + _fix16(0.11400) * b + half) >> SCALEBITS
    cb = (-_fix16(0.16874) * r - _fix16(0.33126) * g + _fix16(0.50000) * b + off + half - 1) >> SCALEBITS
    cr = (_fix16(0.50000) * r - _fix16(0.41869) * g - _fix16(0.08131) * b + off + half - 1) >> SCALEBITS
    bias = (1 + (np.arange(Wp // 2, dtype=np.int32) & 1))[None, :]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    bottom = lambda p, rows: np.pad(p, ((0, rows - p.shape[0]), (0, 0)), mode='edge')
    down = lambda p: bottom((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2, Hp // 2)
    lum, chrom = quant_tables(quality)
    y = _codec_plane(bottom(y, Hp), lum)[:h, :w]
    cb = _upsample_h2v2(_codec_plane(down(cb), chrom), ch, cw)[:h, :w] - 128
    cr = _upsample_h2v2(_codec_plane(down(cr), chrom), ch, cw)[:h, :w] - 128
    out = np.empty((h, w, 3), np.int32)
    out[..., 0] = y + ((_fix16(1.40200) * cr + half) >> SCALEBITS)
    out[..., 1] = y + ((-_fix16(0.34414) * cb + half - _fix16(0.71414) * cr) >> SCALEBITS)
    out[..., 2] = y + ((_fix16(1.77200) * cb + half) >> SCALEBITS)
    return np.clip(out, 0, 255).astype(np.uint8)
