"""The super-resolved regions of curved text pasted back into their photo (main.py --demo_paste_polygons, TextSR.demo(paste=True,
paste_polygons=True)): utils/poly.py straightens a polygon strip by strip with PIL's bilinear QUAD map, and every strip of the SR region
goes back into its four-cornered piece of the enlarged photo by the INVERSE of that map.  PIL has no such transform, so this module
fixes the semantics itself: the strip table of a region, the inverse of one strip, the bounding boxes and a numpy restatement in float64
whose bytes the kernel reproduces exactly (ops.paste_mixed_u8, csrc/paste_poly.hip).  Quadrilaterals (utils/paste.py) and polygons go
through one list, so box-file order holds where they overlap.  No GPU needed: importable on any machine.

A polygon region is (sr index, strips, feather).  strips is a float64 (n, 10) array, one row per strip of the polygon (utils/poly.py:
strip i is t[i], t[i+1], b[i+1], b[i]): the corners NW, NE, SE, SW as (x, y) in the ENLARGED photo and the SR columns c0, c1 that the
strip covers.  `strip_table` builds it: the corners are the polygon's times the scale, and with (h, w, xs) = poly.polygon_plan(points)
c0 = xs[i] * w_s / w, c1 = xs[i+1] * w_s / w -- the region was resized from its rectified width w to the SR width w_s, which is in
general not scale * w.

The inverse of one strip.  The forward map is P = NW + u E + v F + u v G with E = NE - NW, F = SW - NW, G = SE - SW - NE + NW.  For
pixel (X, Y), P = (X + 0.5, Y + 0.5), Hv = P - NW and cross(a, b) = ax by - ay bx:
    A = cross(G, F), B = cross(Hv, G) + cross(E, F), C = cross(Hv, E)            (A v^2 + B v + C = 0)
    disc = B * B - 4 * A * C, r = sqrt(disc)
    v = (-2 * C) / (B + r) if B >= 0 else (-B + r) / (2 * A)
    D = E + v * G, N = Hv - v * F
    u = N.x / D.x if |D.x| >= |D.y| else N.y / D.y
in float64, plain * + - / and sqrt in exactly this order.  The derivative of the quadratic at the wanted root is the Jacobian of the
bilinear map, which is positive inside a strictly convex clockwise strip: that is the root with + r.  Its two forms avoid cancellation,
and the first gives -C / B without a branch when the strip is a parallelogram (A = 0).
A pixel belongs to the FIRST strip, in ascending order, with 0 <= u < 1 and 0 <= v < 1 (a NaN compares false: disc < 0 is outside).
Its source position is sx = c0 + u * (c1 - c0), sy = v * h_s; from there on it is a pixel of utils/paste.py: touched where 0 <= sx < w_s
and 0 <= sy < h_s, utils.quad.perspective_sample's bicubic sample, paste.feather_mask and paste.blend_u8.  sx is continuous across the
seams of the strips, so only the outline of the whole region is feathered.
One limit: a pixel whose centre lies within rounding of a seam between two strips may be claimed by neither (u just not below 1 in the
one, just below 0 in the other); it then keeps its byte.

Visiting only bounding boxes is exact, as in utils/paste.py: the image of the unit square under the bilinear map of a convex strip is
that strip, so the bounding box of its four corners, grown by one pixel and clipped to the photo (`strip_box`), holds every pixel the
strip can claim.  The region's box is the union of its strips' boxes.  paste_mixed_np visits the boxes, paste_mixed_np(full=True) every
pixel with every strip; tests/test_paste_poly.py shows the two equal.
"""
import numpy as np

from . import poly
from .paste import _coeffs, _feather, blend_u8, feather_mask, region_box, region_patch
from .quad import bicubic_at
from .resize import MAX_SIDE, check_image

STRIP_WORDS = 10      # NW, NE, SE, SW as (x, y), then c0, c1


def strip_table(points, scale, w_s, h_s):
    """The strips of a polygon region: points as utils/poly.py takes them (2k points, the photo's coordinates), the scale of the
    enlargement and the size of the region's SR image -> float64 (k - 1, 10), see the module's head.  ValueError for what
    poly.check_polygon or poly.polygon_plan refuses, for a value that is not finite and for an SR side outside 1 .. MAX_SIDE."""
    scale, w_s, h_s = float(scale), int(w_s), int(h_s)
    if not (1 <= w_s <= MAX_SIDE and 1 <= h_s <= MAX_SIDE):
        raise ValueError("strip_table: SR size %d x %d outside 1 .. %d" % (h_s, w_s, MAX_SIDE))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("strip_table: the scale %g is not a finite positive number" % scale)
    poly.check_polygon(points)
    _, w, xs = poly.polygon_plan(points)
    t, b = poly._edges(points)
    out = np.empty((t.shape[0] - 1, STRIP_WORDS), np.float64)
    with np.errstate(all="ignore"):
        for i in range(t.shape[0] - 1):
            out[i, :8] = np.concatenate([t[i] * scale, t[i + 1] * scale, b[i + 1] * scale, b[i] * scale])
            out[i, 8:] = float(xs[i] * w_s) / float(w), float(xs[i + 1] * w_s) / float(w)
    if not np.isfinite(out).all():
        raise ValueError("strip_table: a scaled corner is not finite")
    return out


def _strips(strips, what):
    s = np.asarray(strips, np.float64)
    if s.ndim != 2 or s.shape[1] != STRIP_WORDS or not 1 <= s.shape[0] <= poly.MAX_POLY_SIDE - 1:
        raise ValueError("%s: 1 .. %d strips of %d numbers expected, got shape %s" % (what, poly.MAX_POLY_SIDE - 1, STRIP_WORDS, s.shape))
    if not np.isfinite(s).all():
        raise ValueError("%s: a strip holds a value that is not finite" % what)
    return s


def is_polygon_region(region):
    """Whether an item of paste_mixed_np's list carries a strip table (a 2-D array) and not paste.py's 8 coefficients."""
    return len(region) == 3 and np.ndim(region[1]) == 2


def strip_uv(strip, xin, yin):
    """The inverse of one strip at the points (xin, yin) of the enlarged photo (arrays that broadcast; pixel centres are X + 0.5,
    Y + 0.5) -> (u, v) in float64, NaN or infinite where the quadratic has no root.  The operation order of the module's head."""
    nwx, nwy, nex, ney, sex, sey, swx, swy = (float(c) for c in np.asarray(strip, np.float64).reshape(-1)[:8])
    with np.errstate(all="ignore"):
        ex, ey = nex - nwx, ney - nwy
        fx, fy = swx - nwx, swy - nwy
        gx, gy = sex - swx - nex + nwx, sey - swy - ney + nwy
        hx, hy = xin - nwx, yin - nwy
        A = gx * fy - gy * fx
        B = (hx * gy - hy * gx) + (ex * fy - ey * fx)
        C = hx * ey - hy * ex
        disc = B * B - 4 * A * C
        r = np.sqrt(disc)
        v = np.where(B >= 0, (-2 * C) / (B + r), (-B + r) / (2 * A))
        dx, dy = ex + v * gx, ey + v * gy
        nx, ny = hx - v * fx, hy - v * fy
        u = np.where(np.abs(dx) >= np.abs(dy), nx / dx, ny / dy)
    return u, v


def strip_box(strip, H2, W2):
    """(x0, y0, x1, y1), x1 and y1 exclusive: the pixels of the enlarged photo that a strip can claim -- the bounding box of its four
    corners, grown by one pixel and clipped to the photo (empty: x1 <= x0 or y1 <= y0)."""
    c = np.asarray(strip, np.float64).reshape(-1)[:8].reshape(4, 2)
    # (clamped before the floats become integers: a corner far outside the photo stays a finite integer)
    lo = np.clip(np.floor(c.min(axis=0)) - 1, -1.0, float(MAX_SIDE))
    hi = np.clip(np.ceil(c.max(axis=0)) + 1, -1.0, float(MAX_SIDE))
    return max(int(lo[0]), 0), max(int(lo[1]), 0), min(int(hi[0]), int(W2)), min(int(hi[1]), int(H2))


def polygon_box(strips, H2, W2):
    """The union of the strips' boxes that are not empty, (0, 0, 0, 0) when all are."""
    boxes = [b for b in (strip_box(s, H2, W2) for s in _strips(strips, "polygon_box")) if b[2] > b[0] and b[3] > b[1]]
    if not boxes:
        return 0, 0, 0, 0
    return min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes)


def polygon_source(strips, w_s, h_s, box, H2, W2, full=False):
    """The source positions of a polygon region over the pixels x0 <= X < x1, y0 <= Y < y1 of the enlarged photo -> (sx, sy, inside):
    float64 (h, w) each (NaN where no strip claims the pixel) and whether the pixel is claimed and 0 <= sx < w_s, 0 <= sy < h_s.  A
    strip is evaluated over the pixels of its own strip_box, with full=True over all of them."""
    strips = _strips(strips, "polygon_source")
    x0, y0, x1, y1 = box
    sx = np.full((y1 - y0, x1 - x0), np.nan, np.float64)
    sy = sx.copy()
    claimed = np.zeros(sx.shape, bool)
    for s in strips:
        bx0, by0, bx1, by1 = box if full else strip_box(s, H2, W2)
        bx0, by0, bx1, by1 = max(bx0, x0), max(by0, y0), min(bx1, x1), min(by1, y1)
        if bx1 <= bx0 or by1 <= by0:
            continue
        sub = (slice(by0 - y0, by1 - y0), slice(bx0 - x0, bx1 - x0))
        xin = (np.arange(bx0, bx1, dtype=np.float64) + 0.5)[None, :]
        yin = (np.arange(by0, by1, dtype=np.float64) + 0.5)[:, None]
        u, v = strip_uv(s, xin, yin)
        with np.errstate(all="ignore"):
            hit = (u >= 0) & (u < 1) & (v >= 0) & (v < 1) & ~claimed[sub]      # (a NaN compares false: outside)
            sx[sub] = np.where(hit, s[8] + u * (s[9] - s[8]), sx[sub])
            sy[sub] = np.where(hit, v * float(h_s), sy[sub])
        claimed[sub] |= hit
    with np.errstate(all="ignore"):
        inside = claimed & (sx >= 0) & (sx < w_s) & (sy >= 0) & (sy < h_s)
    return sx, sy, inside


def polygon_patch(sr, strips, feather, box, H2, W2, full=False):
    """One polygon region over the pixels of box -> (warped (h, w, 3) uint8, mask (h, w) uint8): paste.region_patch with
    polygon_source's positions in place of the perspective map's."""
    h_s, w_s = check_image(sr, "SR image")
    sx, sy, inside = polygon_source(strips, w_s, h_s, box, H2, W2, full)
    return bicubic_at(np.asarray(sr).astype(np.float64), sx, sy, inside), feather_mask(sx, sy, inside, w_s, h_s, feather)


def paste_mixed_np(photo2, sr_images, regions, full=False):
    """photo2 (H2, W2, 3) uint8, the enlarged photo; sr_images a list of (h_s, w_s, 3) uint8 arrays; regions ONE list in paste order
    whose items are paste.py's (sr index, 8 coefficients, feather) or (sr index, strips, feather) -> a new (H2, W2, 3) uint8 array with
    the regions pasted in list order, each onto the result of the one before.  A quadrilateral is paste.paste_regions_np's region (a
    list of quadrilaterals alone gives its bytes), a polygon polygon_patch's source byte and mask, then paste.blend_u8.  full=False
    visits the boxes, full=True every pixel: the same bytes.  The CPU reference of ops.paste_mixed_u8."""
    H2, W2 = check_image(photo2, "photo")
    out = np.array(photo2, dtype=np.uint8, copy=True)
    for r, reg in enumerate(regions):
        if len(reg) != 3:
            raise ValueError("paste_mixed_np: region %d is not (sr index, coefficients or strips, feather)" % r)
        k, shape, feather = reg
        k = int(k)
        if not 0 <= k < len(sr_images):
            raise ValueError("paste_mixed_np: region %d names SR image %d of %d" % (r, k, len(sr_images)))
        h_s, w_s = check_image(sr_images[k], "SR image %d" % k)
        feather = _feather(feather, "paste_mixed_np")
        curved = is_polygon_region(reg)
        if full:
            box = (0, 0, W2, H2)
        else:
            box = polygon_box(shape, H2, W2) if curved else region_box(_coeffs(shape, "paste_mixed_np"), w_s, h_s, H2, W2)
        x0, y0, x1, y1 = box
        if x1 <= x0 or y1 <= y0:
            continue
        if curved:
            warped, mask = polygon_patch(sr_images[k], _strips(shape, "paste_mixed_np"), feather, box, H2, W2, full)
        else:
            warped, mask = region_patch(sr_images[k], shape, feather, box)
        out[y0:y1, x0:x1] = blend_u8(out[y0:y1, x0:x1], warped, mask[..., None])
    return out
