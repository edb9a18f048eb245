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
What it finds: well-contrasted, roughly horizontal words and lines.  What it misses: text less than about 50 luma levels from its
background (below the Otsu threshold), vertical or strongly rotated text (5 w >= 6 h), glyphs taller than half the working map, and
very large glyphs whose word spaces exceed `gap` at the working resolution (the word splits).  It is no learned detector.
"""
import numpy as np

from .resize import check_image

MAP_SIDE = 1024      # the longer side of the working map is at most this
FLOOR, GAP, VGAP = 24, 12, 2
MAX_GAP = 64         # of gap and vgap: a fill decision looks at most this far (csrc/detect.hip DETECT_MAX_GAP)
MAX_BOXES = 256
MIN_H = 6


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


def boxes_from_components(comps, H, W, name=None):
    """Stages 6 and 7: the table of components() (in any order) of an H x W photo -> int32 (n, 4) boxes x0, y0, x1, y1 in photo pixels,
    ends exclusive, sorted by (top, left, bottom, right), at most MAX_BOXES (one printed line when some are dropped; name: the photo)."""
    r, hm, wm = working_size(H, W)
    c = np.asarray(comps, np.int64).reshape(-1, 5)
    x0, y0, x1, y1, area = c.T
    h, w = y1 - y0, x1 - x0
    keep = (h >= MIN_H) & (2 * h <= hm) & (5 * w >= 6 * h) & (100 * area >= 35 * w * h)
    x0, y0, x1, y1, h = x0[keep], y0[keep], x1[keep], y1[keep], h[keep]
    p = (h + 5) // 10
    b = np.stack([np.clip((x0 - p) * r, 0, W), np.clip((y0 - p) * r, 0, H), np.clip((x1 + p) * r, 0, W), np.clip((y1 + p) * r, 0, H)], axis=1)
    b = b[np.lexsort((b[:, 2], b[:, 3], b[:, 0], b[:, 1]))]
    if len(b) > MAX_BOXES:
        print("detect: %s%d regions found, the %d of largest area kept" % (name + ": " if name else "", len(b), MAX_BOXES))
        big = np.argsort(-(b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), kind="stable")[:MAX_BOXES]
        b = b[np.sort(big)]
    return b.astype(np.int32)


def detect_maps_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR):
    """One photo -> (g uint8, histogram int64 (256,), smoothed map uint8 of 0 / 1, labels int32), each map hm x wm: stages 1 to 5.
    The CPU reference of ops.detect_maps_u8."""
    gap, vgap, floor = check_params(gap, vgap, floor)
    g, hist = gradient(luma_map(photo))
    s = smooth(g >= threshold(hist, floor), gap, vgap)
    return g, hist, s.astype(np.uint8), label(s)


def detect_text_np(photo, gap=GAP, vgap=VGAP, floor=FLOOR, name=None):
    """One photo -> its boxes, int32 (n, 4).  The CPU reference of ops.detect_text_u8."""
    labels = detect_maps_np(photo, gap, vgap, floor)[3]
    return boxes_from_components(components(labels), photo.shape[0], photo.shape[1], name)


def box_lines(boxes):
    """Boxes (n, 4) -> the text of a box file: one line x0,y0,x1,y0,x1,y1,x0,y1 per box (clockwise from top-left, no transcription)."""
    return "".join("%d,%d,%d,%d,%d,%d,%d,%d\n" % (x0, y0, x1, y0, x1, y1, x0, y1) for x0, y0, x1, y1 in np.asarray(boxes).reshape(-1, 4).tolist())


def write_boxes(path, boxes):
    """The boxes of one photo as a box file that utils.quad.numbered_boxes reads (empty for no box)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(box_lines(boxes))
