"""The text regions of whole photos, rectified (main.py --demo_boxes, TextSR.demo(boxes=True)): a detector's output or an ICDAR-style
ground-truth file names one quadrilateral per word -- often slanted or in perspective -- and every quadrilateral is mapped onto an
upright rectangle of its own size with PIL's perspective transform and bicubic filter.  This module fixes the semantics: the reader of
the box files, the size and the 8 coefficients of a region, and a numpy restatement in float64 of
Image.transform((w, h), Image.PERSPECTIVE, coeffs, Image.BICUBIC) (libImaging/Geometry.c: perspective_transform and the bicubic
filter, the same operations in the same order), whose bytes the kernel reproduces exactly (ops.quad_crop_u8, csrc/quad.hip).  No GPU
needed: importable on any machine.

A quad is 4 corners (x, y) clockwise from top-left in image coordinates (y down), as ICDAR 2015 writes them: tl, tr, br, bl.  A region
is (photo, h, w, coeffs): the photo's index in the batch, the size of the rectified rectangle and the 8 coefficients a0 .. a7 that take
the centre of output pixel (x, y) to the photo: sx = (a0 xin + a1 yin + a2) / (a6 xin + a7 yin + 1), sy likewise from a3, a4, a5.
"""
import math

import numpy as np

from .resize import MAX_SIDE, check_image

DONT_CARE = "###"      # ICDAR's transcription of a region that is not to be read


def numbered_boxes(path):
    """The usable lines of a box file -> [(k, line number, quad, label)]: k counts the file's non-empty lines from 0 (a line that is
    skipped keeps its number), line numbers count from 1.  See read_boxes."""
    out, k = [], -1
    with open(path, encoding="utf-8-sig") as fh:      # (utf-8-sig: a BOM is dropped)
        for lineno, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            k += 1
            parts = line.split(",", 8)
            try:
                if len(parts) < 8:
                    raise ValueError("%d numbers" % len(parts))
                quad = np.array([float(p) for p in parts[:8]], np.float64).reshape(4, 2)
            except ValueError as e:
                print("quad: %s line %d does not parse (%s), skipped" % (path, lineno, e))
                continue
            label = parts[8] if len(parts) == 9 and parts[8] != "" else " "
            if label.strip() == DONT_CARE:
                continue
            out.append((k, lineno, quad, label))
    return out


def read_boxes(path):
    """One text file of regions -> [(quad, label)], quad a float64 (4, 2) array of (x, y).  UTF-8, a BOM is dropped; a line is
    x1,y1,x2,y2,x3,y3,x4,y4[,transcription]: 8 ints or floats separated by commas with optional blanks, the corners clockwise from
    top-left; the transcription is everything after the 8th comma (it may hold commas), " " when it is missing (what the LMDB reader
    gives a missing label).  Empty lines are ignored, a line whose transcription is ### is skipped silently, a line that does not
    parse is skipped with one printed line naming the file and the line number."""
    return [(quad, label) for _, _, quad, label in numbered_boxes(path)]


def _quad(quad):
    q = np.asarray(quad, np.float64)
    if q.size != 8:
        raise ValueError("quad: 4 corners (x, y) expected, got shape %s" % (q.shape,))
    return q.reshape(4, 2)


def quad_size(quad):
    """(h_q, w_q) of the rectangle a quad is rectified to: the mean length of its top and bottom edges and of its left and right edges,
    rounded half up, each clamped to 1 .. MAX_SIDE.  The region is rectified at its own size and the antialiased resize
    (utils/resize.py) takes it to the LR size from there: a large word is not point-sampled down."""
    tl, tr, br, bl = _quad(quad)
    side = lambda a, b, c, d: (math.hypot(*(b - a)) + math.hypot(*(d - c))) / 2
    w, h = side(tl, tr, bl, br), side(tl, bl, tr, br)
    clamp = lambda v: int(min(max(math.floor(v + 0.5), 1), MAX_SIDE)) if math.isfinite(v) else MAX_SIDE
    return clamp(h), clamp(w)


def check_quad(quad):
    """ValueError unless the 8 coordinates are finite, the quad is strictly convex and clockwise in image coordinates (y down: the
    cross product of every two consecutive edges is > 0; an anticlockwise, self-crossing, concave or collinear quad has one that is
    not) and its area is at least 1.  A quad may extend outside its photo."""
    q = _quad(quad)
    if not np.isfinite(q).all():
        raise ValueError("quad: a coordinate is not finite")
    e = np.roll(q, -1, axis=0) - q                         # tl -> tr, tr -> br, br -> bl, bl -> tl
    n = np.roll(e, -1, axis=0)
    cross = e[:, 0] * n[:, 1] - e[:, 1] * n[:, 0]
    if not (cross > 0).all():
        raise ValueError("quad: the corners are not strictly convex and clockwise from top-left (%s)" % q.reshape(-1).tolist())
    nxt = np.roll(q, -1, axis=0)
    area = 0.5 * float((q[:, 0] * nxt[:, 1] - nxt[:, 0] * q[:, 1]).sum())
    if not area >= 1.0:
        raise ValueError("quad: area %.3g below 1" % area)


def quad_coeffs(quad, w, h):
    """The 8 float64 coefficients that PIL's Image.transform((w, h), Image.PERSPECTIVE, coeffs) takes for a quad: np.linalg.solve of
    the 8 x 8 system that maps the corners (0, 0), (w, 0), (w, h), (0, h) of the output rectangle to tl, tr, br, bl (pixel i spans
    i .. i + 1, as PIL has it).  ValueError when the denominator a6 u + a7 v + 1 is not positive at a corner of the rectangle (it is
    linear: positive at the corners, positive inside) or the system has no finite solution."""
    q = _quad(quad)
    w, h = int(w), int(h)
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError("quad_coeffs: output size %d x %d outside 1 .. %d" % (h, w, MAX_SIDE))
    corners = ((0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h)))
    A, b = np.zeros((8, 8), np.float64), np.zeros(8, np.float64)
    for i, ((u, v), (X, Y)) in enumerate(zip(corners, q)):
        A[2 * i] = u, v, 1, 0, 0, 0, -u * X, -v * X
        A[2 * i + 1] = 0, 0, 0, u, v, 1, -u * Y, -v * Y
        b[2 * i], b[2 * i + 1] = X, Y
    try:
        a = np.linalg.solve(A, b)
    except np.linalg.LinAlgError as e:
        raise ValueError("quad_coeffs: %s" % e) from e
    if not np.isfinite(a).all():
        raise ValueError("quad_coeffs: the coefficients are not finite")
    if not all(a[6] * u + a[7] * v + 1 > 0 for u, v in corners):
        raise ValueError("quad_coeffs: the denominator is not positive over the output rectangle")
    return a


def _cubic(v1, v2, v3, v4, d):
    """Geometry.c BICUBIC: the cubic through four values at the fraction d, in its operation order."""
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def bicubic_at(src, sx0, sy0, inside):
    """The sampling of perspective_sample for source positions found elsewhere (utils/paste_poly.py): src (H, W, 3) float64, sx0 / sy0
    (h, w) the source positions BEFORE the -0.5 shift, inside (h, w) bool -> the truncated bicubic sample (h, w, 3) uint8, black where
    the pixel is not inside (sx0 / sy0 are not read there)."""
    H, W = src.shape[:2]
    with np.errstate(all="ignore"):
        sx = np.where(inside, sx0, 0.5) - 0.5
        sy = np.where(inside, sy0, 0.5) - 0.5
    ix, iy = np.floor(sx), np.floor(sy)
    dx, dy = (sx - ix)[..., None], (sy - iy)[..., None]
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    xs = [np.clip(ix + k, 0, W - 1) for k in (-1, 0, 1, 2)]
    rows = []
    for k in (-1, 0, 1, 2):
        r = iy + k
        val = _cubic(*(src[np.clip(r, 0, H - 1), x] for x in xs), dx)
        if k >= 0:      # the first row is clipped; a later row outside the photo repeats the value of the row before it
            val = np.where(((r >= 0) & (r < H))[..., None], val, rows[-1])
        rows.append(val)
    v = _cubic(*rows, dy)
    out = np.where(v <= 0, 0.0, np.where(v >= 255, 255.0, v)).astype(np.uint8)      # (truncation, as Geometry.c casts)
    out[~inside] = 0
    return out


def perspective_sample(src, xin, yin, coeffs):
    """The sampling core of quad_crop_one, shared with utils/paste.py: src (H, W, 3) float64, xin (1, w) and yin (h, 1) the centres of
    the output pixels, coeffs the 8 coefficients -> (bytes (h, w, 3) uint8, inside (h, w) bool, sx, sy): the source position of every
    pixel BEFORE the -0.5 shift, whether it lies in 0 <= sx < W, 0 <= sy < H, and the truncated bicubic sample there (black outside)."""
    H, W = src.shape[:2]
    a = coeffs
    with np.errstate(all="ignore"):
        den = a[6] * xin + a[7] * yin + 1
        sx0 = (a[0] * xin + a[1] * yin + a[2]) / den
        sy0 = (a[3] * xin + a[4] * yin + a[5]) / den
        inside = (sx0 >= 0) & (sx0 < W) & (sy0 >= 0) & (sy0 < H)      # (a NaN compares false: outside)
    return bicubic_at(src, sx0, sy0, inside), inside, sx0, sy0


def quad_crop_one(photo, h, w, coeffs):
    """One region of quad_crop_np: photo (H, W, 3) uint8 -> (h, w, 3) uint8."""
    check_image(photo, "photo")
    h, w = int(h), int(w)
    a = np.asarray(coeffs, np.float64).reshape(-1)
    if a.size != 8 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("quad_crop: 8 coefficients and sides 1 .. %d expected, got %d and %d x %d" % (MAX_SIDE, a.size, h, w))
    xin = (np.arange(w, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    return perspective_sample(np.asarray(photo).astype(np.float64), xin, yin, a)[0]


def quad_crop_np(images, regions):
    """A list of (H, W, 3) uint8 photos and a list of regions (photo index, h, w, coeffs) -> one (h, w, 3) uint8 array per region,
    byte for byte np.asarray(Image.fromarray(photo).transform((w, h), Image.PERSPECTIVE, coeffs, Image.BICUBIC)), all in float64.
    Per output pixel (x, y): xin = x + 0.5, yin = y + 0.5, (sx, sy) as in the module's head; outside 0 <= sx < W, 0 <= sy < H (a
    non-finite value counts as outside) the pixel is black.  Otherwise sx -= 0.5, sy -= 0.5, (ix, iy) their floors, (dx, dy) the
    fractions; the taps are the columns ix - 1 .. ix + 2, each clipped to the photo, and the rows iy - 1 .. iy + 2, of which only the
    first is clipped -- a later row outside the photo repeats the value of the row before it; the cubic runs over each row with dx,
    then over the four row values with dy; the byte is 0 for v <= 0, 255 for v >= 255, else v truncated.  The CPU reference of
    ops.quad_crop_u8."""
    out = []
    for r, (b, h, w, coeffs) in enumerate(regions):
        b = int(b)
        if not 0 <= b < len(images):
            raise ValueError("quad_crop_np: region %d names photo %d of %d" % (r, b, len(images)))
        out.append(quad_crop_one(images[b], h, w, coeffs))
    return out
