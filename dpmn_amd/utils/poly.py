"""Curved text from polygon box files, rectified (main.py --demo_polygons, dataset/folder.py box_batches(polygons=True)): the curved-text
sets (CTW1500: 14 points per line, Total-Text, ArT) and the detectors trained on them name a word or a line by a polygon with k points
along its top edge and k along its bottom edge.  The polygon is cut into its k - 1 strips and every strip is straightened onto a
rectangle of its own width: PIL's Image.transform((w, h), Image.MESH, cells, Image.BICUBIC), every cell a rectangle of the output that
PIL's bilinear QUAD transform maps from a four-cornered piece of the photo.  This module fixes the semantics: the reader of the box
files, the checks, the size and the cells of a polygon, and a numpy restatement in float64 of the MESH transform (Image.__transformer's
QUAD coefficients, libImaging/Geometry.c: quad_transform and the bicubic filter, the same operations in the same order), whose bytes the
kernel reproduces exactly (ops.poly_crop_u8, csrc/poly.hip).  No GPU needed: importable on any machine.

A polygon is 2k points (x, y) clockwise from top-left in image coordinates (y down), as CTW1500 writes them: t[0] .. t[k-1] along the
top edge from left to right, then the bottom edge from right to left; b[i] is the bottom point under t[i].  2 <= k <= MAX_POLY_SIDE (a
stated limit: CTW1500 has k = 7, Total-Text stays below 16).  Strip i is (t[i], t[i+1], b[i+1], b[i]).  A region is (photo, h, w,
cells): the photo's index in the batch, the size of the rectified rectangle and per strip a cell (x0, x1, a): the columns x0 <= x < x1
of the output and the 8 coefficients a0 .. a7 that take the centre of output pixel (x, y) to the photo: with xin = (x - x0) + 0.5 and
yin = y + 0.5, sx = a0 + a1 xin + a2 yin + a3 xin yin, sy likewise from a4 .. a7.
"""
import math

import numpy as np

from .quad import DONT_CARE, _cubic
from .resize import MAX_SIDE, check_image

MAX_POLY_SIDE = 32          # points along one edge of a polygon, so at most 31 strips / cells per region
CTW_MARK = "####"           # CTW1500 writes the transcription as ####text


def _leading_floats(parts):
    out = []
    for p in parts:
        try:
            out.append(float(p))
        except ValueError:
            break
    return out


def numbered_polygons(path):
    """The usable lines of a box file -> [(k, line number, points, label)], points a float64 (n, 2) array of (x, y), n even and >= 4.
    The conventions of utils.quad.numbered_boxes: UTF-8, a BOM is dropped, empty lines are ignored, k counts the file's non-empty lines
    from 0 (a line that is skipped keeps its number), line numbers count from 1, a line whose transcription is ### is skipped
    silently, a line that does not parse is skipped with one printed line naming the file and the line number.
    A line is split at EVERY comma.  With n the number of leading fields that parse as a float, the coordinates are the first
    4 * (n // 4) of them -- a line holds an even number of points and at least four -- and everything after them, joined back with
    commas, is the transcription: " " when it is missing, a leading #### (CTW1500's marker) stripped.  Fewer than 8 leading numbers
    do not parse, nor does a polygon of more than 2 * MAX_POLY_SIDE points.
    So a quad with the label 2015 or 1,000 still reads as that quad and that label (one or two numbers too many for another pair of
    points), while a quad whose label is FOUR or more comma-separated numbers would be read as a polygon: #### in front of the
    transcription removes the doubt."""
    out, k = [], -1
    with open(path, encoding="utf-8-sig") as fh:      # (utf-8-sig: a BOM is dropped)
        for lineno, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            k += 1
            parts = line.split(",")
            nums = _leading_floats(parts)
            n = 4 * (len(nums) // 4)
            if n < 8 or n > 4 * MAX_POLY_SIDE:
                why = "%d leading numbers" % len(nums) if n < 8 else "%d points, more than %d" % (n // 2, 2 * MAX_POLY_SIDE)
                print("poly: %s line %d does not parse (%s), skipped" % (path, lineno, why))
                continue
            label = ",".join(parts[n:])
            if label.strip() == DONT_CARE:
                continue
            if label.startswith(CTW_MARK):
                label = label[len(CTW_MARK):]
                if label.strip() == DONT_CARE:
                    continue
            out.append((k, lineno, np.array(nums[:n], np.float64).reshape(-1, 2), label if label != "" else " "))
    return out


def _edges(points):
    """points -> (t, b), float64 (k, 2) each: the top edge from left to right and the bottom point under every top point."""
    p = np.asarray(points, np.float64)
    if p.size < 8 or p.size % 4 or p.size > 4 * MAX_POLY_SIDE:
        raise ValueError("polygon: 2k points (x, y) with 2 <= k <= %d expected, got shape %s" % (MAX_POLY_SIDE, p.shape))
    p = p.reshape(-1, 2)
    k = p.shape[0] // 2
    return p[:k], p[k:][::-1]


def check_polygon(points):
    """ValueError unless the polygon has 2k points, 2 <= k <= MAX_POLY_SIDE, every coordinate is finite, every strip
    (t[i], t[i+1], b[i+1], b[i]) is strictly convex and clockwise in image coordinates (utils.quad.check_quad's test: the cross product
    of every two consecutive edges is > 0 -- the bilinear map of a strip is one-to-one only then) and the polygon's area is at least 1.
    Points may lie outside the photo."""
    t, b = _edges(points)
    p = np.concatenate([t, b[::-1]])
    if not np.isfinite(p).all():
        raise ValueError("polygon: a coordinate is not finite")
    for i in range(t.shape[0] - 1):
        q = np.stack([t[i], t[i + 1], b[i + 1], b[i]])
        e = np.roll(q, -1, axis=0) - q
        n = np.roll(e, -1, axis=0)
        cross = e[:, 0] * n[:, 1] - e[:, 1] * n[:, 0]
        if not (cross > 0).all():
            raise ValueError("polygon: strip %d is not strictly convex and clockwise from top-left (%s)" % (i, q.reshape(-1).tolist()))
    nxt = np.roll(p, -1, axis=0)
    area = 0.5 * float((p[:, 0] * nxt[:, 1] - nxt[:, 0] * p[:, 1]).sum())
    if not area >= 1.0:
        raise ValueError("polygon: area %.3g below 1" % area)


def polygon_plan(points):
    """(h, w, xs) of the rectangle a polygon is rectified to.  h: the mean of the k lengths |t[i] - b[i]|, rounded half up and clamped
    to 1 .. MAX_SIDE.  xs: the k column bounds of the strips -- with c_i the running sum of the strips' widths (a strip's width is the
    mean of its top and bottom segment lengths), xs[0] = 0 and xs[i] = max(xs[i-1] + 1, floor(c_i + 0.5)), so every strip is at least
    one column wide; w = xs[k-1].  ValueError when w > MAX_SIDE (or a length is not finite).  For k = 2 this is
    utils.quad.quad_size (which clamps a width above MAX_SIDE where this refuses it)."""
    t, b = _edges(points)
    k = t.shape[0]
    length = lambda v: math.hypot(float(v[0]), float(v[1]))
    height = sum(length(b[i] - t[i]) for i in range(k)) / k
    if not math.isfinite(height):
        raise ValueError("polygon: the height is not finite")
    h = int(min(max(math.floor(height + 0.5), 1), MAX_SIDE))
    xs, c = [0], 0.0
    for i in range(1, k):
        c += (length(t[i] - t[i - 1]) + length(b[i] - b[i - 1])) / 2
        if not math.isfinite(c):
            raise ValueError("polygon: the width is not finite")
        xs.append(max(xs[-1] + 1, int(math.floor(c + 0.5))))
        if xs[-1] > MAX_SIDE:
            raise ValueError("polygon: the rectified line is more than %d columns wide" % MAX_SIDE)
    return h, xs[-1], xs


def polygon_cells(points, h, xs):
    """The cells of a polygon's region: per strip (x0, x1, a), a the 8 float64 QUAD coefficients exactly as PIL's Image.__transformer
    computes them for the box (x0, 0, x1, h) and the quad (NW, SW, SE, NE) = (t[i], b[i], b[i+1], t[i+1]): with As = 1.0 / (x1 - x0)
    and At = 1.0 / h, a0 = NWx, a1 = (NEx - NWx) * As, a2 = (SWx - NWx) * At, a3 = (SEx - SWx - NEx + NWx) * As * At, and a4 .. a7
    likewise from y."""
    t, b = _edges(points)
    h, xs = int(h), [int(x) for x in xs]
    if len(xs) != t.shape[0] or xs[0] != 0 or any(x1 <= x0 for x0, x1 in zip(xs, xs[1:])) or not 1 <= h <= MAX_SIDE or xs[-1] > MAX_SIDE:
        raise ValueError("polygon_cells: %d ascending column bounds from 0 and a height 1 .. %d expected, got %s and %d"
                         % (t.shape[0], MAX_SIDE, xs, h))
    cells = []
    for i, (x0, x1) in enumerate(zip(xs, xs[1:])):
        nw, sw, se, ne = (tuple(float(v) for v in p) for p in (t[i], b[i], b[i + 1], t[i + 1]))
        As, At = 1.0 / (x1 - x0), 1.0 / h
        a = []
        for c in (0, 1):
            a += [nw[c], (ne[c] - nw[c]) * As, (sw[c] - nw[c]) * At, (se[c] - sw[c] - ne[c] + nw[c]) * As * At]
        cells.append((x0, x1, np.array(a, np.float64)))
    return cells


def check_cells(h, w, cells):
    """(bounds, coeffs) of a region's cells as arrays -- int64 (n, 2) and float64 (n, 8) -- or ValueError: 1 .. MAX_POLY_SIDE - 1
    cells (x0, x1, 8 coefficients) whose bounds ascend from 0 to w without a gap, sides 1 .. MAX_SIDE."""
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("poly_crop: sides 1 .. %d expected, got %d x %d" % (MAX_SIDE, h, w))
    cells = list(cells)
    if not 1 <= len(cells) <= MAX_POLY_SIDE - 1:
        raise ValueError("poly_crop: 1 .. %d cells expected, got %d" % (MAX_POLY_SIDE - 1, len(cells)))
    bounds, coeffs = np.empty((len(cells), 2), np.int64), np.empty((len(cells), 8), np.float64)
    for i, cell in enumerate(cells):
        x0, x1, a = cell
        a = np.asarray(a, np.float64).reshape(-1)
        if a.size != 8:
            raise ValueError("poly_crop: cell %d carries %d coefficients, not 8" % (i, a.size))
        bounds[i], coeffs[i] = (int(x0), int(x1)), a
    if bounds[0, 0] != 0 or bounds[-1, 1] != w or (bounds[:, 1] <= bounds[:, 0]).any() or (bounds[1:, 0] != bounds[:-1, 1]).any():
        raise ValueError("poly_crop: the cell bounds %s do not ascend from 0 to %d without a gap" % (bounds.tolist(), w))
    return bounds, coeffs


def poly_crop_one(photo, h, w, cells):
    """One region of poly_crop_np: photo (H, W, 3) uint8 -> (h, w, 3) uint8."""
    check_image(photo, "photo")
    h, w = int(h), int(w)
    bounds, coeffs = check_cells(h, w, cells)
    src = np.asarray(photo).astype(np.float64)
    H, W = src.shape[:2]
    x = np.arange(w, dtype=np.int64)
    cell = np.searchsorted(bounds[:, 1], x, side="right")                       # the cell with x0 <= x < x1
    xin = ((x - bounds[cell, 0]).astype(np.float64) + 0.5)[None, :]
    yin = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    a = [coeffs[cell, j][None, :] for j in range(8)]
    with np.errstate(all="ignore"):
        sx0 = a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin
        sy0 = a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin
        inside = (sx0 >= 0) & (sx0 < W) & (sy0 >= 0) & (sy0 < H)      # (a NaN compares false: outside)
        sx = np.where(inside, sx0, 0.5) - 0.5
        sy = np.where(inside, sy0, 0.5) - 0.5
    # from here on utils.quad.perspective_sample's sampling, operation for operation
    ix, iy = np.floor(sx), np.floor(sy)
    dx, dy = (sx - ix)[..., None], (sy - iy)[..., None]
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    cols = [np.clip(ix + k, 0, W - 1) for k in (-1, 0, 1, 2)]
    rows = []
    for k in (-1, 0, 1, 2):
        r = iy + k
        val = _cubic(*(src[np.clip(r, 0, H - 1), c] for c in cols), dx)
        if k >= 0:      # the first row is clipped; a later row outside the photo repeats the value of the row before it
            val = np.where(((r >= 0) & (r < H))[..., None], val, rows[-1])
        rows.append(val)
    v = _cubic(*rows, dy)
    out = np.where(v <= 0, 0.0, np.where(v >= 255, 255.0, v)).astype(np.uint8)      # (truncation, as Geometry.c casts)
    out[~inside] = 0
    return out


def poly_crop_np(images, regions):
    """A list of (H, W, 3) uint8 photos and a list of regions (photo index, h, w, cells) -> one (h, w, 3) uint8 array per region, byte
    for byte np.asarray(Image.fromarray(photo).transform((w, h), Image.MESH, [((x0, 0, x1, h), NW + SW + SE + NE), ...],
    Image.BICUBIC)) with polygon_cells' coefficients, all in float64.  Per output pixel (x, y) in the cell with x0 <= x < x1:
    xin = (x - x0) + 0.5, yin = y + 0.5, sx = a0 + a1 * xin + a2 * yin + a3 * xin * yin and sy likewise from a4 .. a7, in that
    operation order; outside 0 <= sx < W, 0 <= sy < H (a NaN counts as outside) the pixel is black; otherwise the sample is that of
    utils.quad.quad_crop_np: the -0.5 shift, the 4 x 4 taps with clipped columns, the row rule, the cubic and the truncation.  The CPU
    reference of ops.poly_crop_u8."""
    out = []
    for r, (b, h, w, cells) in enumerate(regions):
        b = int(b)
        if not 0 <= b < len(images):
            raise ValueError("poly_crop_np: region %d names photo %d of %d" % (r, b, len(images)))
        out.append(poly_crop_one(images[b], h, w, cells))
    return out
