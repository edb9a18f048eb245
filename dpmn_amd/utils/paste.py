"""The super-resolved text regions pasted back into their photo (main.py --demo_paste, TextSR.demo(boxes=True, paste=True)): the photo is
enlarged by the model's scale factor (PIL's bicubic resize, utils/resize.py), and every SR region is warped back into its quadrilateral
of the enlarged photo -- the inverse of the rectification of utils/quad.py -- and blended in with PIL's integer blend.  This module fixes
the semantics: the 8 coefficients of the inverse mapping, the feathered mask, the blend and a numpy restatement in float64 whose bytes
the kernel reproduces exactly (ops.paste_regions_u8, csrc/paste.hip).  With feather 0 the restatement is, byte for byte,
    warped = Image.fromarray(S).transform((W2, H2), Image.PERSPECTIVE, coeffs, Image.BICUBIC)
    mask = Image.new("L", (w_s, h_s), 255).transform((W2, H2), Image.PERSPECTIVE, coeffs, Image.BICUBIC)
    photo2.paste(warped, mask=mask)
per region (tests/test_paste.py).  No GPU needed: importable on any machine.

A region is (sr index, coeffs, feather): the SR image's index in the list, the 8 float64 coefficients a0 .. a7 that take the centre of
pixel (X, Y) of the ENLARGED photo to the SR image (sx = (a0 xin + a1 yin + a2) / (a6 xin + a7 yin + 1), sy likewise from a3, a4, a5:
utils/quad.py's form, the roles of photo and rectangle swapped) and the width of the feathered edge in SR pixels.  The regions are
applied in list order, each onto the result of the one before: a later region lies over an earlier one.

Visiting only a bounding box is exact.  A pixel is touched only where its source position lies in the SR rectangle.  A projective map
that is regular on the quadrilateral (the inverse mapping takes the four corners of the SR rectangle to finite points with denominators
of one sign) maps nothing else into that rectangle: the pre-image of the rectangle is the convex hull of the four mapped corners, the
scaled quadrilateral itself.  So the pixels of that quadrilateral's bounding box, grown by one pixel for the rounding of the corners and
clipped to the photo, are all that a region can touch, and `region_box` gives that box (the whole photo when the mapping is not
regular).  paste_regions_np visits the box; paste_regions_np(full=True) visits every pixel, and tests/test_paste.py shows the two equal.
"""
import math

import numpy as np

from .quad import _quad, perspective_sample
from .resize import MAX_SIDE, check_image, pil_resize_u8


def paste_coeffs(quad, scale, w_s, h_s):
    """The 8 float64 coefficients that take the quadrilateral of a region in the ENLARGED photo to its SR image: the four corners of
    quad (tl, tr, br, bl in photo coordinates) times scale (pixel i spans i .. i + 1, so continuous coordinates scale exactly) go to
    (0, 0), (w_s, 0), (w_s, h_s), (0, h_s).  np.linalg.solve of the 8 x 8 system: utils.quad.quad_coeffs with the roles swapped.
    ValueError when the coefficients are not finite or the denominator a6 X + a7 Y + 1 does not have one sign, and no zero, at the
    four scaled corners (it is linear: one sign at the corners, that sign inside).  Unlike quad_coeffs' rectangle the quadrilateral
    does not hold the origin, where the denominator is 1: a region in perspective whose vanishing line passes between the photo's
    origin and the region has a NEGATIVE denominator all over it, with the numerators negated -- the same regular mapping, which PIL,
    the restatement and the kernel evaluate as sx = num / den like any other."""
    q = _quad(quad) * float(scale)
    w_s, h_s = int(w_s), int(h_s)
    if not (1 <= w_s <= MAX_SIDE and 1 <= h_s <= MAX_SIDE):
        raise ValueError("paste_coeffs: SR size %d x %d outside 1 .. %d" % (h_s, w_s, MAX_SIDE))
    corners = ((0.0, 0.0), (float(w_s), 0.0), (float(w_s), float(h_s)), (0.0, float(h_s)))
    A, b = np.zeros((8, 8), np.float64), np.zeros(8, np.float64)
    try:
        with np.errstate(all="ignore"):
            for i, ((X, Y), (u, v)) in enumerate(zip(q, corners)):
                A[2 * i] = X, Y, 1, 0, 0, 0, -X * u, -Y * u
                A[2 * i + 1] = 0, 0, 0, X, Y, 1, -X * v, -Y * v
                b[2 * i], b[2 * i + 1] = u, v
            a = np.linalg.solve(A, b)
    except np.linalg.LinAlgError as e:
        raise ValueError("paste_coeffs: %s" % e) from e
    if not np.isfinite(a).all():
        raise ValueError("paste_coeffs: the coefficients are not finite")
    den = [a[6] * X + a[7] * Y + 1 for X, Y in q]
    if not (all(d > 0 for d in den) or all(d < 0 for d in den)):
        raise ValueError("paste_coeffs: the denominator changes sign over the quadrilateral")
    return a


def _coeffs(coeffs, what):
    a = np.asarray(coeffs, np.float64).reshape(-1)
    if a.size != 8:
        raise ValueError("%s: 8 coefficients expected, got %d" % (what, a.size))
    return a


def _feather(feather, what):
    f = float(feather)
    if not math.isfinite(f):
        raise ValueError("%s: the feather is not finite" % what)
    return f


def region_box(coeffs, w_s, h_s, H2, W2):
    """(x0, y0, x1, y1), x1 and y1 exclusive: the pixels of the enlarged photo that a region can touch -- the bounding box of the
    pre-image of the SR rectangle's corners, grown by one pixel and clipped to the photo (empty: x1 <= x0 or y1 <= y0).  The whole
    photo when the inverse of the mapping is not finite or its denominator changes sign over the rectangle (see the module's head)."""
    a = _coeffs(coeffs, "region_box")
    full = (0, 0, int(W2), int(H2))
    M = np.array([[a[0], a[1], a[2]], [a[3], a[4], a[5]], [a[6], a[7], 1.0]], np.float64)
    try:
        with np.errstate(all="ignore"):
            P = np.linalg.solve(M, np.array([[0.0, w_s, w_s, 0.0], [0.0, 0.0, h_s, h_s], [1.0, 1.0, 1.0, 1.0]], np.float64))
            xy = P[:2] / P[2]
    except np.linalg.LinAlgError:
        return full
    if not (np.isfinite(P).all() and np.isfinite(xy).all() and ((P[2] > 0).all() or (P[2] < 0).all())):
        return full
    # (clamped before the floats become integers: a corner far outside the photo stays a finite integer)
    lo = np.clip(np.floor(xy.min(axis=1)) - 1, -1.0, float(MAX_SIDE))
    hi = np.clip(np.ceil(xy.max(axis=1)) + 1, -1.0, float(MAX_SIDE))
    return max(int(lo[0]), 0), max(int(lo[1]), 0), min(int(hi[0]), int(W2)), min(int(hi[1]), int(H2))


def feather_mask(sx, sy, inside, w_s, h_s, feather):
    """The mask of a region, uint8 of the shape of sx: 0 where the pixel is not inside; 255 when feather <= 0; otherwise d = min(sx, w_s - sx, sy,
    h_s - sy) in float64 (sx, sy before the -0.5 shift: the distance of the source position to the nearest edge of the SR rectangle),
    t = d / feather, and m = 255 if t >= 1 else int(floor(t * 255 + 0.5))."""
    feather = _feather(feather, "feather_mask")
    if not feather > 0:
        return np.where(inside, 255, 0).astype(np.uint8)
    with np.errstate(all="ignore"):
        d = np.minimum(np.minimum(sx, w_s - sx), np.minimum(sy, h_s - sy))
        t = np.where(inside, d, 0.0) / feather
        m = np.where(t >= 1, 255.0, np.floor(t * 255 + 0.5))
    return np.where(inside, m, 0.0).astype(np.uint8)


def blend_u8(dst, src, m):
    """PIL's Image.paste(src, mask=L) on uint8 (libImaging/Paste.c): t = dst * (255 - m) + src * m + 128, out = ((t >> 8) + t) >> 8."""
    dst, src, m = (np.asarray(v).astype(np.int64) for v in (dst, src, m))
    t = dst * (255 - m) + src * m + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def region_patch(sr, coeffs, feather, box):
    """One region over the pixels x0 <= X < x1, y0 <= Y < y1 of the enlarged photo -> (warped (h, w, 3) uint8, mask (h, w) uint8):
    xin = X + 0.5, yin = Y + 0.5 through the coefficients as utils.quad.quad_crop_one does it, its bicubic sample of the SR image where
    0 <= sx < w_s and 0 <= sy < h_s (a non-finite value is outside), and feather_mask."""
    h_s, w_s = check_image(sr, "SR image")
    x0, y0, x1, y1 = box
    xin = (np.arange(x0, x1, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(y0, y1, dtype=np.float64) + 0.5)[:, None]
    warped, inside, sx, sy = perspective_sample(np.asarray(sr).astype(np.float64), xin, yin, _coeffs(coeffs, "region_patch"))
    return warped, feather_mask(sx, sy, inside, w_s, h_s, feather)


def paste_regions_np(photo2, sr_images, regions, full=False):
    """photo2 (H2, W2, 3) uint8, the enlarged photo; sr_images a list of (h_s, w_s, 3) uint8 arrays (the sizes may differ); regions a
    list of (sr index, coeffs, feather) -> a new (H2, W2, 3) uint8 array with the regions pasted in list order.  Per region and pixel
    (X, Y): region_patch's source byte and mask, then blend_u8 per channel where the pixel is inside (the mask is 0 elsewhere, and the
    blend with 0 leaves the byte).  full=False visits region_box's pixels, full=True all of them: the same bytes.  The CPU reference
    of ops.paste_regions_u8."""
    H2, W2 = check_image(photo2, "photo")
    out = np.array(photo2, dtype=np.uint8, copy=True)
    for r, reg in enumerate(regions):
        k, coeffs, feather = reg
        k = int(k)
        if not 0 <= k < len(sr_images):
            raise ValueError("paste_regions_np: region %d names SR image %d of %d" % (r, k, len(sr_images)))
        h_s, w_s = check_image(sr_images[k], "SR image %d" % k)
        x0, y0, x1, y1 = box = (0, 0, W2, H2) if full else region_box(coeffs, w_s, h_s, H2, W2)
        if x1 <= x0 or y1 <= y0:
            continue
        warped, mask = region_patch(sr_images[k], coeffs, feather, box)
        out[y0:y1, x0:x1] = blend_u8(out[y0:y1, x0:x1], warped, mask[..., None])
    return out


def enlarge_np(photo, scale):
    """The photo enlarged by an integer scale: utils.resize.pil_resize_u8(photo, scale * H, scale * W) = np.asarray(Image.fromarray(
    photo).resize((scale * W, scale * H), BICUBIC)).  ValueError when a side would exceed utils.resize.MAX_SIDE."""
    H, W = check_image(photo, "photo")
    scale = int(scale)
    if scale < 1 or scale * H > MAX_SIDE or scale * W > MAX_SIDE:
        raise ValueError("enlarge_np: a %d x %d photo times %d has a side outside 1 .. %d" % (H, W, scale, MAX_SIDE))
    return pil_resize_u8(photo, scale * H, scale * W)
