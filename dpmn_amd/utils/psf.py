"""Random point-spread functions for the synthesised LR images (main.py --psf_blur): camera shake (`motion`, a line at an angle), a lens
out of focus (`disk`) and astigmatism or a rolling shutter (`aniso`, an elongated Gaussian), the per-image PSF every blind-SR recipe
draws (KAIR's utils_sisr.py, which the reference vendors but never wires in; Real-ESRGAN; BSRGAN).  The HR pack is blurred BEFORE
utils.degrade's stages; the reference's own pre-blur (an isotropic Gaussian of 3 or 5 taps) stays part of those.

This module is the NORMATIVE restatement: `psf_taps` builds a PSF in float64 and quantises it ONCE to 16-bit integer taps; from there
on everything is integer arithmetic on the image side, so `psf_blur_u8` and the kernel (csrc/psf.hip through ops.psf_blur_ragged_u8)
give the same bytes whatever the compute mode.  Pure NumPy: importable on any machine.

A PSF is an int32 (n, 3) array of its non-zero taps (dy, dx, q) in row-major order, |dy|, |dx| <= R = ceil(r) <= 10, q > 0 and
sum q = 2^16 exactly, so a flat region and the identity PSF come out unchanged and no clip is needed.
"""
import math
import random

import numpy as np

from .degrade import reflect101

KINDS = ("motion", "disk", "aniso")
MAX_RADIUS = 10                                  # R = ceil(r) <= 10: K = 2 R + 1 <= 21
MAX_TAPS = (2 * MAX_RADIUS + 1) ** 2             # 441
ONE = 1 << 16                                    # the sum of a PSF's taps
IDENTITY = np.array([[0, 0, ONE]], np.int32)
DEFAULT_PROB, DEFAULT_FRAC = 0.5, 0.12


def _weights(kind, r, theta, ratio):
    """The real (K, K) float64 weights of a PSF, not normalised; row = dy + R, column = dx + R."""
    R = int(math.ceil(r))
    K = 2 * R + 1
    if kind == "motion":
        # a centred segment from -r to +r at angle theta: S = 8 K samples, each deposited bilinearly
        w = np.zeros((K, K), np.float64)
        S = 8 * K
        t = ((np.arange(S, dtype=np.float64) + 0.5) / S * 2 - 1) * r
        y, x = R + t * math.sin(theta), R + t * math.cos(theta)
        y0, x0 = np.floor(y), np.floor(x)
        fy, fx = y - y0, x - x0
        for oy, wy in ((0, 1 - fy), (1, fy)):
            for ox, wx in ((0, 1 - fx), (1, fx)):
                yy, xx = y0.astype(np.int64) + oy, x0.astype(np.int64) + ox
                ok = (yy >= 0) & (yy < K) & (xx >= 0) & (xx < K)      # (|t| < r <= R: only a weight of 0 ever falls outside)
                np.add.at(w, (yy[ok], xx[ok]), (wy * wx)[ok])
        return w
    d = np.arange(-R, R + 1, dtype=np.float64)
    dy, dx = d[:, None], d[None, :]
    if kind == "aniso":
        s1 = r / 2.0
        s2 = s1 * ratio
        c, s = math.cos(theta), math.sin(theta)
        u, v = dx * c + dy * s, -dx * s + dy * c
        return np.exp(-0.5 * (u * u / (s1 * s1) + v * v / (s2 * s2)))
    if kind == "disk":
        return np.clip(r + 0.5 - np.hypot(dx, dy), 0.0, 1.0)
    raise ValueError("psf_taps: unknown kind %r (one of %s)" % (kind, ", ".join(KINDS)))


def quantise(w):
    """(K, K) non-negative float64 weights -> the int32 (n, 3) taps: q = floor(w / sum(w) * 2^16 + 0.5); 2^16 - sum(q) goes to the
    largest tap (the first one in row-major order on a tie), which makes the sum exact; zero taps are dropped.  ValueError when that
    fix-up would not leave the largest tap positive."""
    w = np.asarray(w, np.float64)
    R = w.shape[0] // 2
    q = np.floor(w / w.sum() * ONE + 0.5).astype(np.int64)
    top = int(np.argmax(q))                      # (argmax: the first of equal values in row-major order)
    flat = q.reshape(-1)
    fix = ONE - int(flat.sum())
    if flat[top] + fix <= 0:
        raise ValueError("psf quantise: the fix-up %d does not fit the largest tap %d" % (fix, flat[top]))
    flat[top] += fix
    ys, xs = np.nonzero(q)
    return np.stack((ys - R, xs - R, q[ys, xs]), axis=1).astype(np.int32)


def psf_taps(kind, r=1.0, theta=0.0, ratio=1.0):
    """The taps of one PSF: kind 'motion' (a segment of half length r at angle theta), 'aniso' (a Gaussian of sigma r / 2 along theta
    and r / 2 * ratio across it), 'disk' (radius r, one pixel of soft edge) or 'identity'; 1 <= r <= 10.  theta turns from +x towards
    +y (down the image); 0 .. pi covers every line."""
    if kind == "identity":
        return IDENTITY.copy()
    if kind not in KINDS:
        raise ValueError("psf_taps: unknown kind %r (one of %s)" % (kind, ", ".join(KINDS)))
    r = float(r)
    if not (1.0 <= r <= MAX_RADIUS):
        raise ValueError("psf_taps: the radius must be in 1 .. %d, got %r" % (MAX_RADIUS, r))
    return quantise(_weights(kind, r, float(theta), float(ratio)))


def is_identity(taps):
    return taps.shape[0] == 1 and tuple(int(v) for v in taps[0]) == (0, 0, ONE)


def psf_blur_u8(img, taps):
    """(h, w, 3) uint8 image, (n, 3) taps -> the blurred (h, w, 3) uint8 image: per byte (2^15 + sum q * img[reflect101(y + dy),
    reflect101(x + dx)]) >> 16 in int64, the border folded as often as needed (a side of 1 -> index 0)."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("psf_blur_u8: expected (h, w, 3) uint8, got %s" % (img.shape,))
    h, w = img.shape[:2]
    x = img.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    acc = np.full(x.shape, ONE >> 1, np.int64)
    for dy, dx, q in np.asarray(taps, np.int64):
        acc += q * x[reflect101(ys + dy, h)][:, reflect101(xs + dx, w)]
    return (acc >> 16).astype(np.uint8)


def draw_psf(n, kinds, prob, frac, heights, rng=random):
    """The PSFs of n images (a list of tap arrays), drawn from `rng` (Python's `random` module or a random.Random) image by image in
    this order: first u = rng.random(); ONLY when u < prob four more draws follow, always all four: the kind's index rng.randint(0,
    len(kinds) - 1), r = rng.uniform(1, rmax) with rmax = min(10, max(1, frac * height)), theta = rng.uniform(0, pi), ratio =
    rng.uniform(0.25, 1); otherwise the image keeps the identity.  --train_state depends on this order."""
    if len(heights) != n:
        raise ValueError("draw_psf: needs the %d image heights" % n)
    out = []
    for i in range(n):
        if rng.random() < prob:
            kind = kinds[rng.randint(0, len(kinds) - 1)]
            r = rng.uniform(1.0, min(float(MAX_RADIUS), max(1.0, frac * int(heights[i]))))
            theta = rng.uniform(0.0, math.pi)
            ratio = rng.uniform(0.25, 1.0)
            out.append(psf_taps(kind, r, theta, ratio))
        else:
            out.append(IDENTITY.copy())
    return out


def psf_setting(args):
    """(kinds tuple in the given order, prob, frac) of main.py's --psf_blur KINDS, --psf_prob P and --psf_radius F, or None when the flag
    is off.  ValueError with one clear line for an unknown or repeated kind, P outside 0 .. 1 or F outside (0, 1]."""
    spec = getattr(args, "psf_blur", None)
    if spec is None or spec is False or spec == "":
        return None
    kinds = tuple(k.strip() for k in spec.split(",")) if isinstance(spec, str) else tuple(spec)
    if not kinds or any(k not in KINDS for k in kinds):
        raise ValueError("--psf_blur takes a comma list of %s, got %r" % (", ".join(KINDS), spec))
    if len(set(kinds)) != len(kinds):
        raise ValueError("--psf_blur names a kind twice: %r" % (spec,))
    prob, frac = getattr(args, "psf_prob", None), getattr(args, "psf_radius", None)
    prob = DEFAULT_PROB if prob is None else float(prob)
    frac = DEFAULT_FRAC if frac is None else float(frac)
    if not (0.0 <= prob <= 1.0):
        raise ValueError("--psf_prob needs a probability in 0 .. 1, got %r" % (prob,))
    if not (0.0 < frac <= 1.0):
        raise ValueError("--psf_radius needs a fraction of the image height in (0, 1], got %r" % (frac,))
    return kinds, prob, frac


def cutblur_u8(lr, hr, cut_x, side):
    """The last step of utils.degrade.degrade_u8 as a function of its own: a copy of the (h, w, 3) LR image whose columns >= cut_x
    (side 1) or < cut_x (side 2) are the HR image's; side 0 changes nothing."""
    lr, hr = np.asarray(lr, np.uint8), np.asarray(hr, np.uint8)
    if lr.shape != hr.shape:
        raise ValueError("cutblur_u8: the LR and HR images must have one size, got %s and %s" % (lr.shape, hr.shape))
    out = lr.copy()
    cut_x, side = int(cut_x), int(side)
    if side == 1:
        out[:, cut_x:] = hr[:, cut_x:]
    elif side == 2:
        out[:, :cut_x] = hr[:, :cut_x]
    return out
