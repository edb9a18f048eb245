"""The text regions of a photo without a box file (main.py --demo_detect): the classical recipe -- morphological gradient of the luma,
Otsu threshold, run-length smoothing that joins letters into words, connected components, geometric filters -- in integers only.  This
module fixes the semantics as a numpy restatement whose maps the kernels reproduce byte for byte (ops.detect_maps_u8 /
ops.detect_text_u8, csrc/detect.hip) and holds everything the host does with the kernels' output: the threshold from the histogram,
the filters, the padding and the order of the boxes, and the writer of the box files that utils/quad.numbered_boxes reads.  No GPU
needed: importable on any machine.

Per photo (RGB uint8, H x W, sides 1 .. utils.resize.MAX_SIDE):
  1. working map: r = ceil(max(H, W) / 1024); r x r box means per channel, rounded half up, onto hm x wm = H // r x W // r (the remainder
     rows and columns are dropped; a photo thinner than r has an empty map and no box); Y = (77 R + 150 G + 29 B + 128) >> 8.
  2. gradient g = max3x3(Y) - min3x3(Y), edges replicated, and its 256-bin histogram.
  3. threshold: Otsu's t maximises (S0 N - S N0)^2 / (N0 N1) over the histogram (class 0: the bins <= t), compared exactly, the
     earliest t winning ties, t = 0 when no t leaves both classes non-empty; T = max(t + 1, floor); b = g >= T.
  4. run-length smoothing: in every row a run of background of length 1 .. gap between two foreground pixels is filled; then the same
     down every column of the result with vgap.
  5. components of the smoothed map under 8-connectivity; the label of a component is its least linear index y * wm + x, -1 on the
     background; per component the bounding box x0, y0, x1, y1 (exclusive ends) and the pixel count.
  6. filter: with h = y1 - y0, w = x1 - x0 a component stays if h >= 6, 2 h <= hm, 5 w >= 6 h and 100 area >= 35 w h.
  7. boxes: padded by (h + 5) // 10 on every side, multiplied by r, clamped to the photo, sorted by (top, left, bottom, right); more
     than MAX_BOXES: the MAX_BOXES of largest area stay (ties: the earlier in that order) and one line is printed.
What it finds: well-contrasted, roughly horizontal words and lines.  What it misses: under the one threshold per photo, text fainter
than the photo's strongest edges -- in a plain photo text less than about 50 luma levels from its background, and one high-contrast
sign anywhere lifts the threshold for every word (with local = C, below, only text under `floor` levels of gradient is lost to the
threshold); vertical or strongly rotated text (5 w >= 6 h), glyphs taller than half the working map, and very large glyphs whose
word spaces exceed `gap` at the working resolution (the word splits).  It is no learned detector.

Locally adaptive threshold (main.py --demo_detect_local; local = C on every function below, 0 = off = the recipe above): stage 3 with
a threshold per pixel, still in integers only.  C, MIN_LOCAL .. MAP_SIDE, is the cell side on the working map.
  3a. cells: per axis of length `size`, n = ceil(size / C) cells with the edges e_i = i * size // n (cell_edges): balanced, never empty,
      never wider than C.  A map with hm <= C and wm <= C is one cell.
  3b. cell thresholds: t[i][j] = max(otsu(histogram of g over the cell) + 1, floor) (cell_thresholds), the same otsu, exactly.
  3c. threshold map (threshold_map): bilinear between the cell centres.  Per axis the doubled centres c_i = e_i + e_{i+1}; a pixel's
      doubled centre p = 2x + 1, clamped to [c_0, c_{n-1}]; k the greatest index with c_k <= p, capped at n - 2; weights (c_{k+1} - p,
      p - c_k), D = c_{k+1} - c_k.  T(y, x) = (2 * sum of the four w_y w_x t + Dy Dx) // (2 Dy Dx): rounded half up.  An axis with one
      cell contributes weight 1 and D = 1.  b = g >= T(y, x).  Stages 4 to 7 and the oriented recipe are unchanged.
Consequences: with one cell T is threshold(hist, floor) everywhere, so local = 1024 gives byte for byte the maps and boxes of local = 0
for every photo; T >= floor; T lies within [min t, max t]; D = e_{k+2} - e_k <= size <= 1024 per axis and t <= 255, so
2 * 255 * Dy * Dx + Dy * Dx < 2^31 (csrc/detect.hip computes T in 32 bits).  Limits: the floor still rules; a textured cell (foliage,
brickwork) gets a threshold inside its own texture, so more clutter reaches the filters than under a high global threshold; a word
that straddles a faint cell and a cell with a strong edge sees a ramp of thresholds and can lose its faint end; C is untuned.

Oriented regions (main.py --demo_detect_oriented; detect_oriented_np, ops.detect_oriented_u8): stages 1 to 3 as above, then TWO passes
over the one gradient map and the one threshold -- the row pass smooth(b, gap, vgap) and the column pass smooth(b, vgap, gap) -- and per
component of a pass, still in integers only:
  a. moments: area A and the sums of x, y, x^2, x y, y^2 over its pixels; mxx = A Sxx - Sx^2, mxy = A Sxy - Sx Sy, myy = A Syy - Sy^2.
  b. axis: the k of the 64 directions DIRS (c_k, s_k) = round(16384 (cos, sin) of (k - 32) * 2.8125 degrees), c_k >= 0, that maximises
     c^2 mxx + 2 c s mxy + s^2 myy, compared exactly in Python integers; ties go to the k nearest 32, then to the lower k.  Components
     whose upright box is lower than MIN_H get no axis and are passed over (k = -1): a FURTHER filter of this recipe, not a shortcut
     (a thin slanted component may reach H2 >= 6 S from an upright box 5 high), the same in the restatement and on the GPU.
  c. extents: the least and greatest U2 = c (2x + 1) + s (2y + 1) and V2 = -s (2x + 1) + c (2y + 1) over its pixels (the pixel centres
     along and across the axis, doubled and scaled by 16384); with e2 = |c| + |s| and S = 32768 the rectangle that covers the pixel
     squares measures W2 = U2max - U2min + 2 e2 by H2 = V2max - V2min + 2 e2 (at k = 32: S w and S h of the upright box).
  d. filter: H2 >= 6 S, 2 H2 <= S X (X = hm in the row pass, wm in the column pass), 5 W2 >= 6 H2, 100 A S^2 >= 35 W2 H2; the row pass
     keeps |k - 32| <= 16 (at most 45 degrees), the column pass |k - 32| > 16.  Cross-pass rule: a rectangle is COVERED when its
     centre lies inside a rectangle of the other pass that passed the filter (padding included, borders included, tested exactly in
     that rectangle's frame) and whose W2 H2 is greater -- or, for a column-pass rectangle, not smaller.  A covered column-pass
     rectangle is dropped: a word that both passes find is written once, and the letters that the column pass splits off a
     horizontal word go.  A covered row-pass rectangle is dropped only when it is SQUAT, 2 W2 < 3 H2: such a piece of a larger steep
     rectangle is a turned letter (most glyphs are at most 1.5 times as high as wide), while a piece 1.5 times as long as high may be a
     line of a narrow block of horizontal text, which the column pass joins into one tall blob, and stays.  Nothing that one pass
     finds is lost to the other; what the shape cannot tell is written twice: stacked short lines come with the blob around them
     (steep, to be deleted by hand), and a steep word of unusually narrow glyphs (a turned l) comes with those letters beside it.
     (Dropping column-pass rectangles only, whatever their size, loses a steep word whose centre falls on one of its own letters;
     dropping by area alone loses the lines of the block.  The two cases are the same shape up to scale, hence the squatness.)
  e. quads: padded by p S, p = (H2 // S + 5) // 10, on all four sides; the corners (U2, V2) go back by x = (c U2 - s V2) / (2 n),
     y = (s U2 + c V2) / (2 n), n = c^2 + s^2, times r, in HUNDREDTHS of a photo pixel rounded half up, not clamped; tl, tr, br, bl with
     u to the right and v down (clockwise in image coordinates); sorted by the top-left corner's (y, x), then the other corners; more
     than MAX_BOXES: those of largest W2 H2 stay (ties: the earlier) and the same line is printed.
Text steeper than 45 degrees is read along +u: whether a vertical sign reads upward or downward cannot be told from its shape, and at
exactly 90 degrees the tie rule gives k = 0, -90 degrees, reading upward.

Bowed lines as polygons (main.py --demo_detect_curved; detect_curved_np, ops.detect_curved_u8): stages 1 to 5 as above (local
included), then per component of the ordinary row pass smooth(b, gap, vgap), with w = x1 - x0 and h = y1 - y0, in integers only:
  a. candidates (curve_candidates): h >= MIN_H and w >= CURVE_MIN_W = 16.  A candidate is cut by vertical lines into
     n = min(CURVE_BINS, w // 8) bins, 2 <= n <= 16, with the edges e_i = x0 + i * w // n.  The bin of column x is
     ((x - x0 + 1) * n - 1) // w: the greatest i with e_i <= x, because i * w // n <= x - x0 <=> i * w < (x - x0 + 1) * n <=>
     i <= ((x - x0 + 1) * n - 1) // w.  An 8-connected component has a pixel in every column of its box, so no bin is empty.
  b. profile (curve_profile): per bin over the component's pixels top_i = min y, bot_i = max y + 1, cnt_i and sy_i = sum y.
  c. ribbon (curve_ribbons): the stations in doubled x, X2_0 = 2 x0, X2_{n-1} = 2 x1, X2_i = e_i + e_{i+1} between (the bins'
     centres; the outermost stations are moved to the ends of the box); the doubled centre C_i = (2 sy_i + cnt_i) // cnt_i, the mean
     of the doubled pixel centres 2y + 1, floored; ONE doubled half-height R = max_i max(2 bot_i - C_i, C_i - 2 top_i) for the whole
     region, so that the rectification stretches every strip alike; the line height hc = R in map pixels (half of a doubled height).
  d. curved or straight: a candidate is curved when for an interior station, with D = X2_{n-1} - X2_0,
     2 |C_i D - (C_0 (X2_{n-1} - X2_i) + C_{n-1} (X2_i - X2_0))| > hc D -- the centre line leaves its chord by more than a quarter of the
     line height, compared exactly.  Everything else (non-candidates and n = 2 included) is straight.
  e. filter of a curved component: hc >= MIN_H, 2 hc <= hm, 5 w >= 6 hc and 100 area >= 35 hc w (the fill against the ribbon, whose
     strips are e_{i+1} - e_i wide and hc high, not against the upright box).  One that fails is dropped, not boxed.
  f. output (regions_from_profiles): the straight components give the boxes of stages 6 and 7, unchanged.  A curved component gives
     a polygon of 2n points, clockwise from top-left as utils/poly.py reads them: the top edge (X2_i / 2, (C_i - R) / 2 - p) from left
     to right, the bottom edge (X2_i / 2, (C_i + R) / 2 + p) from right to left, p = (hc + 5) // 10, times r, in HUNDREDTHS of a photo
     pixel (exact: 50 r X2_i and 50 r (C_i -+ R) -+ 100 r p), not clamped.  Every strip is a trapezoid with vertical sides of length
     R + 2p > 0 between strictly increasing stations, hence strictly convex and clockwise: utils.poly.check_polygon accepts it.
     Boxes and polygons are sorted together by the (top, left, bottom, right) of their bounding boxes (on a tie the box first); more
     than MAX_BOXES: those of largest bounding-box area stay (ties: the earlier) and the same line is printed.  A photo without a
     curved component gets byte for byte the box file of the plain recipe.
Limits: this inverts what --train_words_warp curve does -- columns displaced by a smooth curve -- and nothing more; it is no
arbitrary-shape detector.  The cuts are vertical, so the glyphs of a steep arc are sheared, not turned: fine up to a slope of about
0.5, wrong for a half circle.  Only the row pass is used (no vertical or steeply slanted lines).  An S-curve inside one bin is
invisible.  Two lines that the smoothing merges become one ribbon.  The bin count, the quarter-height rule and the 35 % are untuned.
"""
import numpy as np

from .resize import check_image

MAP_SIDE = 1024      # the longer side of the working map is at most this
FLOOR, GAP, VGAP = 24, 12, 2
MAX_GAP = 64         # of gap and vgap: a fill decision looks at most this far (csrc/detect.hip DETECT_MAX_GAP)
MAX_BOXES = 256
MIN_H = 6
MIN_LOCAL = 32       # the least cell side of the locally adaptive threshold (the greatest is MAP_SIDE: one cell)


def check_params(gap=GAP, vgap=VGAP, floor=FLOOR):
    """(gap, vgap, floor) as ints; ValueError unless gap and vgap are 1 .. MAX_GAP and floor is 1 .. 255."""
    gap, vgap, floor = int(gap), int(vgap), int(floor)
    if not (1 <= gap <= MAX_GAP and 1 <= vgap <= MAX_GAP):
        raise ValueError("detect: gap %d and vgap %d must be 1 .. %d" % (gap, vgap, MAX_GAP))
    if not 1 <= floor <= 255:
        raise ValueError("detect: floor %d must be 1 .. 255" % floor)
    return gap, vgap, floor


def working_size(H, W):
    """(r, hm, wm) of an H x W photo: the reduction factor and the size of the working map (either side may be 0)."""
    H, W = int(H), int(W)
    r = -(-max(H, W) // MAP_SIDE)
    return r, H // r, W // r


def luma_map(photo):
    """Stage 1: (H, W, 3) uint8 -> Y (hm, wm) uint8."""
    check_image(photo, "photo")
    a = np.asarray(photo)
    r, hm, wm = working_size(*a.shape[:2])
    s = a[:hm * r, :wm * r].astype(np.int64).reshape(hm, r, wm, r, 3).sum(axis=(1, 3))
    m = (s + (r * r) // 2) // (r * r)
    return ((77 * m[..., 0] + 150 * m[..., 1] + 29 * m[..., 2] + 128) >> 8).astype(np.uint8)


def gradient(Y):
    """Stage 2: Y (hm, wm) uint8 -> (g (hm, wm) uint8, its histogram (256,) int64)."""
    Y = np.asarray(Y, np.uint8)
    if Y.size == 0:
        return Y.copy(), np.zeros(256, np.int64)
    hm, wm = Y.shape
    p = np.pad(Y, 1, mode="edge")
    views = [p[dy:dy + hm, dx:dx + wm] for dy in range(3) for dx in range(3)]
    g = np.maximum.reduce(views) - np.minimum.reduce(views)
    return g, np.bincount(g.reshape(-1), minlength=256).astype(np.int64)


def otsu(hist):
    """Stage 3: the t of 0 .. 255 that maximises (S0 N - S N0)^2 / (N0 N1) over a 256-bin histogram, class 0 the bins <= t; exact
    (Python integers, cross-multiplied), the earliest t on a tie, 0 when no t has both classes non-empty."""
    h = [int(v) for v in np.asarray(hist).reshape(-1)]
    if len(h) != 256 or min(h) < 0:
        raise ValueError("otsu: 256 non-negative counts expected")
    N, S = sum(h), sum(i * v for i, v in enumerate(h))
    best, num, den, N0, S0 = 0, 0, 1, 0, 0
    for t in range(256):
        N0 += h[t]
        S0 += t * h[t]
        N1 = N - N0
        if N0 == 0 or N1 == 0:
            continue
        a, b = (S0 * N - S * N0) ** 2, N0 * N1
        if a * den > num * b:
            best, num, den = t, a, b
    return best


def threshold(hist, floor=FLOOR):
    """T = max(otsu + 1, floor): a pixel is foreground where g >= T."""
    return max(otsu(hist) + 1, int(floor))


def check_local(local=0):
    """local as an int; ValueError unless it is 0 (one threshold per photo) or a cell side MIN_LOCAL .. MAP_SIDE."""
    local = int(local)
    if local != 0 and not MIN_LOCAL <= local <= MAP_SIDE:
        raise ValueError("detect: local %d must be 0 (one threshold per photo) or a cell side %d .. %d" % (local, MIN_LOCAL, MAP_SIDE))
    return local


def cell_edges(size, C):
    """The edges e_0 .. e_n of the n = ceil(size / C) balanced cells of an axis of `size` pixels: e_i = i * size // n (a list of
    n + 1 ints; [0] for size 0).  No cell is empty, none is wider than C, and their widths differ by at most 1."""
    size, C = int(size), int(C)
    n = -(-size // C)
    return [i * size // n for i in range(n + 1)] if n else [0]


def cell_thresholds(g, C, floor=FLOOR):
    """The gradient map g (hm, wm) -> int32 (ny, nx): per cell max(otsu(histogram of g over the cell) + 1, floor)."""
    g = np.asarray(g, np.uint8)
    ey, ex = cell_edges(g.shape[0], C), cell_edges(g.shape[1], C)
    t = np.empty((len(ey) - 1, len(ex) - 1), np.int32)      # (an empty map has no cell along its empty axis)
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            t[i, j] = threshold(np.bincount(g[ey[i]:ey[i + 1], ex[j]:ex[j + 1]].reshape(-1), minlength=256), floor)
    return t


def _axis_weights(size, C):
    """Per pixel of an axis (k, k1, w0, w1, D): the two cells k and k1 whose centres lie around it, their integer weights and the
    weights' sum D (stage 3 of the local recipe).  One cell: (0, 0, 1, 0, 1)."""
    e = np.array(cell_edges(size, C), np.int64)
    n = len(e) - 1
    if n <= 1:
        z = np.zeros(size, np.int64)
        return z, z, z + 1, z, z + 1
    c = e[:-1] + e[1:]
    p = np.clip(2 * np.arange(size, dtype=np.int64) + 1, c[0], c[-1])
    k = np.minimum(np.searchsorted(c, p, side="right") - 1, n - 2)
    return k, k + 1, c[k + 1] - p, p - c[k], c[k + 1] - c[k]


def threshold_map(t, hm, wm, C):
    """The cell table of cell_thresholds -> T int32 (hm, wm): bilinear between the cell centres in integers, rounded half up, constant
    outside the outermost centres.  Every term is below 2^31 (D <= 1024 per axis, t <= 255)."""
    t = np.asarray(t, np.int64)
    ny, nx = len(cell_edges(hm, C)) - 1, len(cell_edges(wm, C)) - 1
    if hm == 0 or wm == 0:
        return np.zeros((hm, wm), np.int32)
    if t.shape != (ny, nx):
        raise ValueError("threshold_map: a table of %s cells for a %d x %d map with cells of %d (%d x %d expected)" % (t.shape, hm, wm, C, ny, nx))
    ky, ky1, wy0, wy1, Dy = (a[:, None] for a in _axis_weights(hm, C))
    kx, kx1, wx0, wx1, Dx = (a[None, :] for a in _axis_weights(wm, C))
    s = wy0 * (wx0 * t[ky, kx] + wx1 * t[ky, kx1]) + wy1 * (wx0 * t[ky1, kx] + wx1 * t[ky1, kx1])
    return ((2 * s + Dy * Dx) // (2 * Dy * Dx)).astype(np.int32)


def foreground(g, hist, floor=FLOOR, local=0):
    """Stage 3: b = g >= T, T the photo's one threshold (local = 0) or the threshold map of its cells of side `local`."""
    if not local:
        return g >= threshold(hist, floor)
    return g >= threshold_map(cell_thresholds(g, local, floor), g.shape[0], g.shape[1], local)


def smooth_rows(b, gap):
    """Stage 4 along the rows: b (h, w) bool -> bool; a background run of length 1 .. gap between two foreground pixels is filled."""
    b = np.asarray(b, bool)
    h, w = b.shape
    if w == 0:
        return b.copy()
    x = np.arange(w)[None, :]
    prev = np.maximum.accumulate(np.where(b, x, -1), axis=1)                             # the last foreground at or before x, -1: none
    nxt = np.minimum.accumulate(np.where(b, x, 2 * w)[:, ::-1], axis=1)[:, ::-1]         # the first at or after x, 2 w: none
    return b | ((prev >= 0) & (nxt < w) & (nxt - prev - 1 <= int(gap)))


def smooth(b, gap=GAP, vgap=VGAP):
    """Stage 4: the rows with gap, then the columns of the result with vgap."""
    return smooth_rows(smooth_rows(b, gap).T, vgap).T


def label(s):
    """Stage 5: s (h, w) bool -> int32 (h, w): per foreground pixel the least linear index y * w + x of its 8-connected component, -1 on
    the background.  Union-find over the runs of the rows: a run [a, b) touches a run [c, d) of the row above when a <= d and c <= b."""
    s = np.asarray(s, bool)
    h, w = s.shape
    out = np.full((h, w), -1, np.int32)
    if s.size == 0:
        return out
    d = np.diff(np.pad(s.astype(np.int8), ((0, 0), (1, 1))), axis=1)
    ys, starts = np.nonzero(d == 1)
    ends = np.nonzero(d == -1)[1]
    n = len(ys)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(ys, np.arange(h + 1))      # the runs of row y are first[y] .. first[y + 1], in raster order
    st, en = starts.tolist(), ends.tolist()
    for y in range(1, h):
        i, i1, j, j1 = first[y], first[y + 1], first[y - 1], first[y]
        while i < i1 and j < j1:
            if st[i] <= en[j] and st[j] <= en[i]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)      # (the runs are numbered in raster order: the least run holds the least index)
            if en[j] < en[i]:
                j += 1
            else:
                i += 1
    roots = np.array([find(i) for i in range(n)], np.int64)
    lab = (ys * w + starts)[roots] if n else roots
    for i in range(n):
        out[ys[i], st[i]:en[i]] = lab[i]
    return out


def components(labels):
    """Stage 5's table: the labels of label() -> int64 (n, 5) [x0, y0, x1, y1, area] per component, ends exclusive, in label order."""
    labels = np.asarray(labels)
    ys, xs = np.nonzero(labels >= 0)
    if len(ys) == 0:
        return np.zeros((0, 5), np.int64)
    _, inv, area = np.unique(labels[ys, xs], return_inverse=True, return_counts=True)
    n = len(area)
    out = np.empty((n, 5), np.int64)
    for col, v, fn, init in ((0, xs, np.minimum, labels.shape[1]), (1, ys, np.minimum, labels.shape[0]), (2, xs + 1, np.maximum, 0),
                             (3, ys + 1, np.maximum, 0)):
        acc = np.full(n, init, np.int64)
        fn.at(acc, inv, v)
        out[:, col] = acc
    out[:, 4] = area
    return out


def _sorted_boxes(comps, H, W):
    """Stages 6 and 7 before MAX_BOXES: the boxes of the components that pass the filter, int64 (n, 4), padded, clamped and sorted."""
    r, hm, wm = working_size(H, W)
    c = np.asarray(comps, np.int64).reshape(-1, 5)
    x0, y0, x1, y1, area = c.T
    h, w = y1 - y0, x1 - x0
    keep = (h >= MIN_H) & (2 * h <= hm) & (5 * w >= 6 * h) & (100 * area >= 35 * w * h)
    x0, y0, x1, y1, h = x0[keep], y0[keep], x1[keep], y1[keep], h[keep]
    p = (h + 5) // 10
    b = np.stack([np.clip((x0 - p) * r, 0, W), np.clip((y0 - p) * r, 0, H), np.clip((x1 + p) * r, 0, W), np.clip((y1 + p) * r, 0, H)], axis=1)
    return b[np.lexsort((b[:, 2], b[:, 3], b[:, 0], b[:, 1]))]


def boxes_from_components(comps, H, W, name=None):
    """Stages 6 and 7: the table of components() (in any order) of an H x W photo -> int32 (n, 4) boxes x0, y0, x1, y1 in photo pixels,
    ends exclusive, sorted by (top, left, bottom, right), at most MAX_BOXES (one printed line when some are dropped; name: the photo)."""
    b = _sorted_boxes(comps, H, W)
    if len(b) > MAX_BOXES:
        print("detect: %s%d regions found, the %d of largest area kept" % (name + ": " if name else "", len(b), MAX_BOXES))
        big = np.argsort(-(b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), kind="stable")[:MAX_BOXES]
        b = b[np.sort(big)]
    return b.astype(np.int32)


def detect_maps_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR, local=0):
    """One photo -> (g uint8, histogram int64 (256,), smoothed map uint8 of 0 / 1, labels int32), each map hm x wm: stages 1 to 5.
    The CPU reference of ops.detect_maps_u8.  local: 0, or the cell side of the locally adaptive threshold (the histogram stays that
    of the whole map)."""
    gap, vgap, floor = check_params(gap, vgap, floor)
    local = check_local(local)
    g, hist = gradient(luma_map(photo))
    s = smooth(foreground(g, hist, floor, local), gap, vgap)
    return g, hist, s.astype(np.uint8), label(s)


def detect_text_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR, name=None, local=0):
    """One photo -> its boxes, int32 (n, 4).  The CPU reference of ops.detect_text_u8."""
    labels = detect_maps_np(photo, gap, vgap, floor, local)[3]
    return boxes_from_components(components(labels), photo.shape[0], photo.shape[1], name)


def box_lines(boxes):
    """Boxes (n, 4) -> the text of a box file: one line x0,y0,x1,y0,x1,y1,x0,y1 per box (clockwise from top-left, no transcription)."""
    return "".join("%d,%d,%d,%d,%d,%d,%d,%d\n" % (x0, y0, x1, y0, x1, y1, x0, y1) for x0, y0, x1, y1 in np.asarray(boxes).reshape(-1, 4).tolist())


def write_boxes(path, boxes):
    """The boxes of one photo as a box file that utils.quad.numbered_boxes reads (empty for no box)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(box_lines(boxes))


# ---- oriented regions: everything below is integers only (Python ints where 64 bits do not suffice) ----

UNIT = 16384         # the scale of DIRS
S2 = 2 * UNIT        # one map pixel in the doubled, scaled units of U2 and V2
AXIS_ROW = 16        # the row pass keeps |k - 32| <= AXIS_ROW, the column pass the rest
# (c_k, s_k) = round(16384 cos, 16384 sin) of (k - 32) * 180 / 64 degrees: literal, so that no libm decides a byte
DIRS = (
    (0, -16384), (804, -16364), (1606, -16305), (2404, -16207), (3196, -16069), (3981, -15893), (4756, -15679), (5520, -15426),
    (6270, -15137), (7005, -14811), (7723, -14449), (8423, -14053), (9102, -13623), (9760, -13160), (10394, -12665), (11003, -12140),
    (11585, -11585), (12140, -11003), (12665, -10394), (13160, -9760), (13623, -9102), (14053, -8423), (14449, -7723), (14811, -7005),
    (15137, -6270), (15426, -5520), (15679, -4756), (15893, -3981), (16069, -3196), (16207, -2404), (16305, -1606), (16364, -804),
    (16384, 0), (16364, 804), (16305, 1606), (16207, 2404), (16069, 3196), (15893, 3981), (15679, 4756), (15426, 5520), (15137, 6270),
    (14811, 7005), (14449, 7723), (14053, 8423), (13623, 9102), (13160, 9760), (12665, 10394), (12140, 11003), (11585, 11585),
    (11003, 12140), (10394, 12665), (9760, 13160), (9102, 13623), (8423, 14053), (7723, 14449), (7005, 14811), (6270, 15137),
    (5520, 15426), (4756, 15679), (3981, 15893), (3196, 16069), (2404, 16207), (1606, 16305), (804, 16364),
)
_TIE_ORDER = sorted(range(64), key=lambda k: (abs(k - 32), k))      # a later k of this order wins only when strictly greater


def moments(labels):
    """The labels of label() -> int64 (n, 6) [area, sum x, sum y, sum x^2, sum x y, sum y^2] per component, in label order."""
    labels = np.asarray(labels)
    ys, xs = np.nonzero(labels >= 0)
    if len(ys) == 0:
        return np.zeros((0, 6), np.int64)
    _, inv = np.unique(labels[ys, xs], return_inverse=True)
    n = int(inv.max()) + 1
    out = np.zeros((n, 6), np.int64)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    for col, v in enumerate((np.ones_like(xs), xs, ys, xs * xs, xs * ys, ys * ys)):
        np.add.at(out[:, col], inv, v)
    return out


def axis_index(moments):
    """The table of moments() -> int64 (n): per component the k of DIRS that maximises c^2 mxx + 2 c s mxy + s^2 myy (the second moment
    along the direction, times A^2), compared exactly; ties go to the k nearest 32, then to the lower k.  float64 only SELECTS: a k
    whose rounded value (relative error below 1e-14) is more than 1e-9 of the greatest below it cannot be the exact maximum, and the
    k that remain are compared in Python ints."""
    m = np.asarray(moments, np.int64).reshape(-1, 6).astype(object)      # Python ints: the terms pass 2^64
    n = m.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    A, sx, sy, sxx, sxy, syy = m.T
    mxx, mxy, myy = A * sxx - sx * sx, A * sxy - sx * sy, A * syy - sy * sy
    d = np.array(DIRS, np.float64)
    V = (np.outer(mxx.astype(np.float64), d[:, 0] * d[:, 0]) + np.outer(mxy.astype(np.float64), 2 * d[:, 0] * d[:, 1])
         + np.outer(myy.astype(np.float64), d[:, 1] * d[:, 1]))
    scale = np.abs(mxx.astype(np.float64)) + np.abs(mxy.astype(np.float64)) + np.abs(myy.astype(np.float64))
    cand = V >= V.max(axis=1, keepdims=True) - 1e-9 * UNIT * UNIT * scale[:, None]
    arg = np.argmax(cand, axis=1).astype(np.int64)      # (exact where one k remains)
    for i in np.nonzero(cand.sum(axis=1) > 1)[0].tolist():
        best = None
        for k in _TIE_ORDER:
            if cand[i, k]:
                c, s = DIRS[k]
                v = (c * c) * mxx[i] + (2 * c * s) * mxy[i] + (s * s) * myy[i]
                if best is None or v > best:      # (a later k of the order wins only when strictly greater)
                    best, arg[i] = v, k
    return arg


def prefilter(comps):
    """The table of components() -> bool (n): the components that get an axis at all, those whose upright box is at least MIN_H high.
    A filter of its own (stage b), not only a shortcut: the oriented filter alone would let a few thin slanted components through."""
    c = np.asarray(comps, np.int64).reshape(-1, 5)
    return c[:, 3] - c[:, 1] >= MIN_H


def extents(labels, k_of_component):
    """The labels of label() and per component (in label order) its k of DIRS, or -1 for a component that is passed over -> int64
    (n, 4) [U2min, U2max, V2min, V2max] over the component's pixels, U2 = c (2x + 1) + s (2y + 1), V2 = -s (2x + 1) + c (2y + 1); a
    row of zeros where k is -1."""
    labels = np.asarray(labels)
    ks = np.asarray(k_of_component, np.int64).reshape(-1)
    out = np.zeros((len(ks), 4), np.int64)
    ys, xs = np.nonzero(labels >= 0)
    if len(ys) == 0:
        return out
    _, inv = np.unique(labels[ys, xs], return_inverse=True)
    if int(inv.max()) + 1 != len(ks):
        raise ValueError("extents: %d components, %d directions" % (int(inv.max()) + 1, len(ks)))
    d = np.array(DIRS + ((0, 0),), np.int64)[ks]      # (k = -1 takes the last row)
    c, s = d[inv, 0], d[inv, 1]
    X, Y = 2 * xs.astype(np.int64) + 1, 2 * ys.astype(np.int64) + 1
    U, V = c * X + s * Y, c * Y - s * X
    big = np.int64(1) << 40
    for col, v, fn, init in ((0, U, np.minimum, big), (1, U, np.maximum, -big), (2, V, np.minimum, big), (3, V, np.maximum, -big)):
        acc = np.full(len(ks), init, np.int64)
        fn.at(acc, inv, v)
        out[:, col] = acc
    out[ks < 0] = 0
    return out


def oriented_rects(comps, ks, ext, H, W, column=False):
    """Stage d without the cross-pass rule: the tables of one pass over an H x W photo (components(), the k per component with -1 for
    none, extents(); rows in any common order) -> int64 (m, 8) [k, U2 of the left side, U2 of the right side, V2 of the top, V2 of the
    bottom (padding included), W2, H2, 0] of the components that pass the filter and lie on the pass's side of 45 degrees."""
    r, hm, wm = working_size(H, W)
    comps = np.asarray(comps, np.int64).reshape(-1, 5)
    ks, ext = np.asarray(ks, np.int64).reshape(-1), np.asarray(ext, np.int64).reshape(-1, 4)
    d = np.array(DIRS + ((0, 0),), np.int64)[ks]
    e2 = np.abs(d[:, 0]) + np.abs(d[:, 1])
    W2, H2 = ext[:, 1] - ext[:, 0] + 2 * e2, ext[:, 3] - ext[:, 2] + 2 * e2
    side = (np.abs(ks - 32) > AXIS_ROW) if column else (np.abs(ks - 32) <= AXIS_ROW)
    keep = ((ks >= 0) & side & (H2 >= MIN_H * S2) & (2 * H2 <= S2 * (wm if column else hm)) & (5 * W2 >= 6 * H2)
            & (100 * comps[:, 4] * S2 * S2 >= 35 * W2 * H2))
    pad = ((H2 // S2 + 5) // 10) * S2 + e2
    out = np.stack([ks, ext[:, 0] - pad, ext[:, 1] + pad, ext[:, 2] - pad, ext[:, 3] + pad, W2, H2, np.zeros_like(ks)], axis=1)
    return out[keep]


def covered(rects, others, ties):
    """Stage d's cross-pass rule for one side: rows of oriented_rects() and those of the other pass -> bool (n): the centre lies inside
    one of `others` whose W2 H2 is greater (ties: or equal).  The centre (Xc, Yc), times 4 n' in the rectangle's own direction
    (c', s'), is projected onto the other's (c, s): U2 = 2 (c Xc + s Yc), so U2 * 2 n' = c PX + s PY is compared with the sides times
    2 n' (all below 2^59)."""
    rects, others = np.asarray(rects, np.int64).reshape(-1, 8), np.asarray(others, np.int64).reshape(-1, 8)
    out = np.zeros(len(rects), bool)
    if len(rects) == 0 or len(others) == 0:
        return out
    d = np.array(DIRS, np.int64)[others[:, 0]]
    c, s, area = d[:, 0], d[:, 1], others[:, 5] * others[:, 6]
    for i, (k, u0, u1, v0, v1, W2, H2, _) in enumerate(rects.tolist()):
        c1, s1 = DIRS[k]
        n2 = 2 * (c1 * c1 + s1 * s1)
        PX, PY = c1 * (u0 + u1) - s1 * (v0 + v1), s1 * (u0 + u1) + c1 * (v0 + v1)
        U, V = c * PX + s * PY, c * PY - s * PX
        larger = (area >= W2 * H2) if ties else (area > W2 * H2)
        out[i] = (larger & (others[:, 1] * n2 <= U) & (U <= others[:, 2] * n2) & (others[:, 3] * n2 <= V) & (V <= others[:, 4] * n2)).any()
    return out


def cross_pass(row_rects, col_rects):
    """Stage d's cross-pass rule: the rows of oriented_rects() of the two passes -> those that stay, the row pass first.  A column-pass
    rectangle goes when covered by a row-pass rectangle that is not smaller; a row-pass rectangle goes when covered by a larger
    column-pass rectangle AND squat (2 W2 < 3 H2: a turned letter, not a line)."""
    row_rects, col_rects = np.asarray(row_rects, np.int64).reshape(-1, 8), np.asarray(col_rects, np.int64).reshape(-1, 8)
    squat = 2 * row_rects[:, 5] < 3 * row_rects[:, 6]
    return np.concatenate([row_rects[~(squat & covered(row_rects, col_rects, False))], col_rects[~covered(col_rects, row_rects, True)]])


def quads_from_rects(rects, H, W, name=None):
    """Stage e: rows of oriented_rects() of an H x W photo -> int64 (n, 8) quads tl, tr, br, bl as x, y in hundredths of a photo pixel,
    sorted, at most MAX_BOXES (one printed line when some are dropped; name: the photo)."""
    r = working_size(H, W)[0]
    quads = []
    for k, u0, u1, v0, v1, W2, H2, _ in np.asarray(rects, np.int64).reshape(-1, 8).tolist():
        c, s = DIRS[k]
        n = c * c + s * s
        q = []
        for u, v in ((u0, v0), (u1, v0), (u1, v1), (u0, v1)):
            q += [(100 * r * (c * u - s * v) + n) // (2 * n), (100 * r * (s * u + c * v) + n) // (2 * n)]      # half up
        quads.append((q, W2 * H2))
    quads.sort(key=lambda t: (t[0][1], t[0][0], t[0][2:]))
    if len(quads) > MAX_BOXES:
        print("detect: %s%d regions found, the %d of largest area kept" % (name + ": " if name else "", len(quads), MAX_BOXES))
        big = sorted(sorted(range(len(quads)), key=lambda i: -quads[i][1])[:MAX_BOXES])      # (sorted() is stable: ties keep the earlier)
        quads = [quads[i] for i in big]
    return np.array([q for q, _ in quads], np.int64).reshape(-1, 8)


def oriented_pass_np(labels, H, W, column=False):
    """One pass of the restatement: the labels of a smoothed map -> (moments (n, 6), k (n) with -1 for a component that is passed
    over, extents (n, 4), the rows of oriented_rects()), the tables in label order: what ops.detect_oriented_tables_u8 returns."""
    comps, m = components(labels), moments(labels)
    ks = np.where(prefilter(comps), axis_index(m), -1)
    ext = extents(labels, ks)
    return m, ks, ext, oriented_rects(comps, ks, ext, H, W, column)


def detect_oriented_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR, name=None, local=0):
    """One photo -> its oriented regions, int64 (n, 8): quads tl, tr, br, bl in hundredths of a photo pixel.  The CPU reference of
    ops.detect_oriented_u8.  local: as detect_maps_np takes it; both passes share the one threshold map."""
    gap, vgap, floor = check_params(gap, vgap, floor)
    local = check_local(local)
    g, hist = gradient(luma_map(photo))
    b = foreground(g, hist, floor, local)
    H, W = photo.shape[:2]
    rows = oriented_pass_np(label(smooth(b, gap, vgap)), H, W)[3]
    cols = oriented_pass_np(label(smooth(b, vgap, gap)), H, W, True)[3]
    return quads_from_rects(cross_pass(rows, cols), H, W, name)


def _hundredths(v):
    v = int(v)
    return "%s%d.%02d" % ("-" if v < 0 else "", abs(v) // 100, abs(v) % 100)


def quad_lines(quads):
    """Quads (n, 8) in hundredths of a pixel -> the text of a box file: one line x1,y1,x2,y2,x3,y3,x4,y4 per quad in decimals."""
    return "".join(",".join(_hundredths(v) for v in q) + "\n" for q in np.asarray(quads, np.int64).reshape(-1, 8).tolist())


def write_quads(path, quads):
    """The oriented regions of one photo as a box file that utils.quad.numbered_boxes reads (empty for none)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(quad_lines(quads))


# ---- bowed lines as polygons: integers only ----

CURVE_MIN_W = 16     # a narrower component is never cut into bins
CURVE_BINS = 16      # the most bins of a component (csrc/detect.hip DETECT_BINS); a bin is at least 8 columns wide


def curve_bin(x, x0, w, n):
    """The bin of column x of a component [x0, x0 + w) cut into n bins: ((x - x0 + 1) * n - 1) // w, the greatest i with
    x0 + i * w // n <= x (arrays or ints)."""
    return ((x - x0 + 1) * n - 1) // w


def curve_candidates(comps):
    """The table of components() -> int64 (n, 3) [x0, w, bins] per component; bins = 0: no candidate (lower than MIN_H or narrower than
    CURVE_MIN_W), else min(CURVE_BINS, w // 8).  The table that the profile launch reads."""
    c = np.asarray(comps, np.int64).reshape(-1, 5)
    w, h = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    ok = (h >= MIN_H) & (w >= CURVE_MIN_W)
    out = np.zeros((len(c), 3), np.int64)
    out[ok] = np.stack([c[ok, 0], w[ok], np.minimum(CURVE_BINS, w[ok] // 8)], axis=1)
    return out


def curve_profile(labels, candidates):
    """The labels of label() and the rows of curve_candidates() (in label order) -> int64 (n, CURVE_BINS, 4) [top, bot, cnt, sy] per
    component and bin over the component's pixels: the least y, the greatest y + 1, their number and the sum of y.  Zeros for a
    component that is no candidate and for the bins past its last."""
    labels = np.asarray(labels)
    cand = np.asarray(candidates, np.int64).reshape(-1, 3)
    out = np.zeros((len(cand), CURVE_BINS, 4), np.int64)
    ys, xs = np.nonzero(labels >= 0)
    if len(ys) == 0:
        return out
    _, inv = np.unique(labels[ys, xs], return_inverse=True)
    if int(inv.max()) + 1 != len(cand):
        raise ValueError("curve_profile: %d components, %d candidate rows" % (int(inv.max()) + 1, len(cand)))
    on = cand[inv, 2] > 0
    ys, xs, inv = ys[on].astype(np.int64), xs[on].astype(np.int64), inv[on]
    if len(ys) == 0:
        return out
    x0, w, n = cand[inv].T
    b = curve_bin(xs, x0, w, n)
    assert (b >= 0).all() and (b < n).all()
    out[:, :, 0] = labels.shape[0]
    np.minimum.at(out[:, :, 0], (inv, b), ys)
    np.maximum.at(out[:, :, 1], (inv, b), ys + 1)
    np.add.at(out[:, :, 2], (inv, b), 1)
    np.add.at(out[:, :, 3], (inv, b), ys)
    used = np.arange(CURVE_BINS)[None, :] < cand[:, 2:3]
    assert (out[:, :, 2][used] > 0).all()      # (a pixel in every column of the box: no bin of a candidate is empty)
    out[~used] = 0
    return out


def curve_ribbons(comps, candidates, profiles, H, W):
    """Stages c to e: the tables of components(), curve_candidates() and curve_profile() of an H x W photo (rows in any common order)
    -> (straight bool (n): the components that go the way of the plain recipe, ribbons: per curved component that passes the
    filter (row, X2 (bins), C (bins), R, p), Python ints, in row order).  A curved component that fails the filter is in neither."""
    r, hm, wm = working_size(H, W)
    comps = np.asarray(comps, np.int64).reshape(-1, 5)
    cand = np.asarray(candidates, np.int64).reshape(-1, 3)
    prof = np.asarray(profiles, np.int64).reshape(-1, CURVE_BINS, 4)
    straight, ribbons = np.ones(len(comps), bool), []
    for j in np.nonzero(cand[:, 2] > 2)[0].tolist():      # (two bins have no interior station: straight)
        x0, w, n = cand[j].tolist()
        top, bot, cnt, sy = (prof[j, :n, k].tolist() for k in range(4))
        assert min(cnt) > 0
        e = [x0 + i * w // n for i in range(n + 1)]
        X2 = [2 * x0] + [e[i] + e[i + 1] for i in range(1, n - 1)] + [2 * (x0 + w)]
        C = [(2 * sy[i] + cnt[i]) // cnt[i] for i in range(n)]
        R = max(max(2 * bot[i] - C[i], C[i] - 2 * top[i]) for i in range(n))
        hc, D = R, X2[-1] - X2[0]
        if not any(2 * abs(C[i] * D - (C[0] * (X2[-1] - X2[i]) + C[-1] * (X2[i] - X2[0]))) > hc * D for i in range(1, n - 1)):
            continue
        straight[j] = False
        if hc >= MIN_H and 2 * hc <= hm and 5 * w >= 6 * hc and 100 * int(comps[j, 4]) >= 35 * sum(hc * (e[i + 1] - e[i]) for i in range(n)):
            ribbons.append((j, X2, C, R, (hc + 5) // 10))
    return straight, ribbons


def ribbon_points(X2, C, R, p, r):
    """Stage f: one ribbon -> its polygon, int64 (2 bins, 2) points (x, y) in hundredths of a photo pixel, clockwise from top-left."""
    top = [(50 * r * x, 50 * r * (c - R) - 100 * r * p) for x, c in zip(X2, C)]
    bottom = [(50 * r * x, 50 * r * (c + R) + 100 * r * p) for x, c in zip(X2, C)]
    return np.array(top + bottom[::-1], np.int64)


def regions_from_profiles(comps, candidates, profiles, H, W, name=None):
    """Stage f: the tables of one photo (rows in any common order) -> its regions, a list of int64 (m, 2) arrays of points (x, y) in
    hundredths of a photo pixel: m = 4 for a box (x0, y0), (x1, y0), (x1, y1), (x0, y1), m = 2 bins for a polygon; sorted by the
    bounding boxes' (top, left, bottom, right), at most MAX_BOXES (one printed line when some are dropped; name: the photo)."""
    comps = np.asarray(comps, np.int64).reshape(-1, 5)
    straight, ribbons = curve_ribbons(comps, candidates, profiles, H, W)
    r = working_size(H, W)[0]
    regions = [100 * np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], np.int64) for x0, y0, x1, y1 in _sorted_boxes(comps[straight], H, W).tolist()]
    if ribbons:
        regions += [ribbon_points(X2, C, R, p, r) for _, X2, C, R, p in ribbons]
        bounds = lambda q: (int(q[:, 1].min()), int(q[:, 0].min()), int(q[:, 1].max()), int(q[:, 0].max()))
        regions.sort(key=bounds)      # (stable: on a tie the box stays in front of the polygon)
    if len(regions) > MAX_BOXES:
        print("detect: %s%d regions found, the %d of largest area kept" % (name + ": " if name else "", len(regions), MAX_BOXES))
        area = [int((q[:, 0].max() - q[:, 0].min()) * (q[:, 1].max() - q[:, 1].min())) for q in regions]
        big = sorted(sorted(range(len(regions)), key=lambda i: -area[i])[:MAX_BOXES])      # (sorted() is stable: ties keep the earlier)
        regions = [regions[i] for i in big]
    return regions


def detect_curved_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR, name=None, local=0):
    """One photo -> its regions, boxes and polygons in one list (regions_from_profiles).  The CPU reference of ops.detect_curved_u8."""
    labels = detect_maps_np(photo, gap, vgap, floor, local)[3]
    comps = components(labels)
    cand = curve_candidates(comps)
    return regions_from_profiles(comps, cand, curve_profile(labels, cand), photo.shape[0], photo.shape[1], name)


def region_lines(regions):
    """The regions of regions_from_profiles -> the text of a box file.  A box is the line of box_lines, x0,y0,x1,y0,x1,y1,x0,y1 in whole
    pixels; a polygon is one line of its 2 bins points in decimals, which utils.poly.numbered_polygons reads."""
    out = []
    for q in regions:
        q = np.asarray(q, np.int64).reshape(-1, 2)
        if len(q) == 4:
            out.append(",".join("%d" % (v // 100) for v in q.reshape(-1).tolist()) + "\n")
        else:
            out.append(",".join(_hundredths(v) for v in q.reshape(-1).tolist()) + "\n")
    return "".join(out)


def write_regions(path, regions):
    """The regions of one photo as a box file that utils.poly.numbered_polygons reads (main.py --demo_polygons; empty for none)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(region_lines(regions))
