"""Synthetic LR images from HR images (dataset/dataset.py:422-489 `degradation`, :622-637 `cutblur`): the random draws of the
reference in its order (`draw_params`) and a NumPy restatement of the image operations (`degrade_u8`), the CPU reference of the
kernel (csrc/degrade.hip through ops.degrade_ragged_u8).  The reference calls cv2, which is not available here, so the semantics
are FIXED HERE; the one known point where cv2 may differ is its 8-bit GaussianBlur (a fixed-point kernel there, a
rounded float result here).  Pure NumPy: importable on any machine.

Columns of a params row (float32, 16 per image):
   0 pre_k         pre-blur kernel size, 3 or 5
   1 pre_sigma     its sigma (5 .. 6)
   2 noise_on      1 when rand_p > 0.2: shot / read noise is added (unless the image is nearly white, see degrade_u8)
   3 shot          shot-noise factor (0 .. 0.005), 0 when noise_on is 0
   4 read          read-noise variance (0 .. 0.015), 0 when noise_on is 0
   5 nr_mode       noise reduction: 0 Gaussian, 1 bilateral
   6 nr_k          Gaussian NR kernel size, 3 or 5 (0 for mode 1)
   7 nr_sigma      its sigma (2 .. 3; 0 for mode 1)
   8 sigma_color   bilateral value sigma (70 .. 80; 0 for mode 0)
   9 sigma_space   bilateral space sigma (70 .. 80; 0 for mode 0)
  10 shp_k         unsharp-mask kernel size, 3 or 5
  11 shp_sigma     its sigma (2 .. 3)
  12 shp_gain      its gain (3 .. 4)
  13 cut_x         cutblur column
  14 cut_side      0 no cutblur, 1 the columns >= cut_x are the HR image's, 2 the columns < cut_x are
  15 (spare, 0)
"""
import random

import numpy as np

N_PARAMS = 16
(PRE_K, PRE_SIGMA, NOISE_ON, SHOT, READ, NR_MODE, NR_K, NR_SIGMA, SIGMA_COLOR, SIGMA_SPACE, SHP_K, SHP_SIGMA, SHP_GAIN, CUT_X,
 CUT_SIDE) = range(15)
KERNEL_SET = (3, 5)          # pre_blur_kernel_set = NR_kernel_set = sharp_kernel_set of the reference
BILATERAL_RADIUS = 3         # cv2.bilateralFilter(d = 7)
WHITE_MEAN = 252.0           # add_shot_gauss_noise: an image whose mean is above this gets no noise


def draw_params(n, cutblur=False, test=False, hr_widths=None, rng=random):
    """The (n, 16) float32 table of n images (columns: module docstring), drawn from `rng` (Python's `random` module or a
    random.Random) image by image in exactly the reference's order: pre-blur kernel index, blur_sigma, rand_p, [shot_noise,
    read_noise when rand_p > 0.2], choice, then NR kernel index and NR_sigma (choice < 0.7) or value_sigma and space_sigma, sharpen
    kernel index, shp_sigma, shp_gain; with cutblur and not test it goes on with p, the draw of randx = int(w * (0.2 + 0.8 * r)) and,
    when p > 0.7, left_mix (<= 0.5: side 1, else side 2).  hr_widths: the n image widths, needed for randx."""
    if cutblur and not test and (hr_widths is None or len(hr_widths) != n):
        raise ValueError("draw_params: cutblur needs the %d image widths (hr_widths)" % n)
    tab = np.zeros((n, N_PARAMS), np.float32)
    for i in range(n):
        row = tab[i]
        row[PRE_K] = KERNEL_SET[rng.randint(0, len(KERNEL_SET) - 1)]
        row[PRE_SIGMA] = rng.uniform(5., 6.)
        rand_p = rng.random()
        if rand_p > 0.2:
            row[NOISE_ON] = 1
            row[SHOT] = rng.uniform(0, 0.005)
            row[READ] = rng.uniform(0, 0.015)
        choice = rng.uniform(0, 1.0)
        if choice < 0.7:
            row[NR_K] = KERNEL_SET[rng.randint(0, len(KERNEL_SET) - 1)]
            row[NR_SIGMA] = rng.uniform(2., 3.)
        else:
            row[NR_MODE] = 1
            row[SIGMA_COLOR] = rng.uniform(70, 80)
            row[SIGMA_SPACE] = rng.uniform(70, 80)
        row[SHP_K] = KERNEL_SET[rng.randint(0, len(KERNEL_SET) - 1)]
        row[SHP_SIGMA] = rng.uniform(2., 3.)
        row[SHP_GAIN] = rng.uniform(3., 4.)
        if cutblur and not test:
            p = rng.random()
            row[CUT_X] = int(int(hr_widths[i]) * (0.2 + 0.8 * rng.random()))
            if p > 0.7:
                row[CUT_SIDE] = 1 if rng.random() <= 0.5 else 2
    return tab


def reflect101(i, n):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) of the indices i into a side of n, folded as often as needed; n = 1 -> 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def gauss_weights(k, sigma, dtype=np.float64):
    """w[i] = exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)), normalised to sum 1 (cv2.getGaussianKernel for sigma > 0)."""
    k, sigma = int(k), dtype(sigma)
    d = np.arange(k, dtype=dtype) - dtype((k - 1) * 0.5)
    e = np.exp(-(d * d) / (dtype(2) * sigma * sigma))
    s = dtype(0)
    for v in e:
        s = s + v
    return (e / s).astype(dtype)


def _blur_axis(x, w, axis):
    n, r = x.shape[axis], len(w) // 2
    base = np.arange(n)
    acc = np.zeros_like(x)
    for k in range(len(w)):
        if k != r:
            acc = acc + w[k] * (np.take(x, reflect101(base + k - r, n), axis=axis) - x)
    return x + acc


def gauss_blur(x, k, sigma, dtype=np.float64):
    """Separable Gaussian of an (h, w, C) array of `dtype`: rows first (along x), then columns.  A pass is evaluated as
    x_i + sum over the taps k != centre, in index order, of w[k] * (x_(i+k-centre) - x_i): the same value as sum w[k] x_(i+k-centre) for
    weights of sum 1, but a flat region comes out exactly, whatever the rounding of the normalised weights -- the unsharp mask's
    truncating cast would otherwise turn v into v - 1 wherever the rounded sum falls below v."""
    w = gauss_weights(k, sigma, dtype)
    return _blur_axis(_blur_axis(x, w, 1), w, 0)


def _round_u8(x):
    return np.clip(np.round(x), 0, 255).astype(np.uint8)      # np.round: half to even


def bilateral_u8(img, sigma_color, sigma_space, dtype=np.float64):
    """cv2's 8-bit bilateralFilter with d = 7 on an (h, w, 3) uint8 image: the neighbours (dy, dx) with sqrt(dx^2 + dy^2) <= 3 in
    row-major order, weight exp(-r^2 / (2 sigma_space^2)) * exp(-(|dR| + |dG| + |dB|)^2 / (2 sigma_color^2)) shared by the three
    channels, normalised, rounded half to even."""
    h, w = img.shape[:2]
    R = BILATERAL_RADIUS
    sc, ss = dtype(sigma_color), dtype(sigma_space)
    x = img.astype(dtype)
    ys, xs = np.arange(h), np.arange(w)
    num = np.zeros_like(x)
    den = np.zeros((h, w, 1), dtype)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            r2 = dx * dx + dy * dy
            if r2 > R * R:
                continue
            sw = np.exp(-dtype(r2) / (dtype(2) * ss * ss))
            nb = x[reflect101(ys + dy, h)][:, reflect101(xs + dx, w)]
            d = np.abs(nb - x).sum(axis=2, keepdims=True)          # integers: exact in either dtype
            wgt = (sw * np.exp(-(d * d) / (dtype(2) * sc * sc))).astype(dtype)
            num = num + nb * wgt
            den = den + wgt
    return _round_u8(num / den)


def degrade_u8(img, params_row, z, dtype=np.float64):
    """img (h, w, 3) uint8, one params row, z (h, w, 3) standard-normal field -> the degraded (h, w, 3) uint8 image, every step in
    `dtype` (float64: the reference of the kernel; float32: the same steps, to measure how many bytes the precision alone moves).
      borders     every filter uses BORDER_REFLECT_101, folded repeatedly (a side shorter than the radius works; a side of 1 -> 0)
      Gaussian    separable, rows then columns, w[i] = exp(-(i - (k-1)/2)^2 / (2 sigma^2)) normalised, one sigma for both axes,
                  evaluated around the centre tap (gauss_blur): a flat region is reproduced exactly
      pre-blur    on the float image
      noise       when noise_on and mean(pre-blurred) <= 252: + z * sqrt(shot * x + read); then clip(0, 255), np.round (half to
                  even), uint8
      NR          mode 0: Gaussian on the uint8 values, rounded half to even and saturated; mode 1: bilateral_u8
      unsharp     x + (x - G(x)) * gain, clip(0, 255), truncated to uint8
      cutblur     columns >= cut_x (side 1) or < cut_x (side 2) are the HR image's"""
    p = np.asarray(params_row, np.float32)
    img = np.ascontiguousarray(img, np.uint8)
    x = gauss_blur(img.astype(dtype), p[PRE_K], p[PRE_SIGMA], dtype)
    if p[NOISE_ON] != 0 and x.mean(dtype=dtype) <= WHITE_MEAN:
        x = x + np.asarray(z, dtype) * np.sqrt(dtype(p[SHOT]) * x + dtype(p[READ]))
    noisy = _round_u8(np.clip(x, 0, 255))
    if p[NR_MODE] == 0:
        nr = _round_u8(gauss_blur(noisy.astype(dtype), p[NR_K], p[NR_SIGMA], dtype))
    else:
        nr = bilateral_u8(noisy, p[SIGMA_COLOR], p[SIGMA_SPACE], dtype)
    x = nr.astype(dtype)
    out = np.clip(x + (x - gauss_blur(x, p[SHP_K], p[SHP_SIGMA], dtype)) * dtype(p[SHP_GAIN]), 0, 255).astype(np.uint8)
    cut_x, side = int(p[CUT_X]), int(p[CUT_SIDE])
    if side == 1:
        out[:, cut_x:] = img[:, cut_x:]
    elif side == 2:
        out[:, :cut_x] = img[:, :cut_x]
    return out
