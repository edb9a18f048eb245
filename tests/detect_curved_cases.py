"""Photos that tests/test_detect_curved.py (CPU) and tests/test_gpu_detect_curved.py share: rows of dark LETTER_W x LETTER_H blocks,
LETTER_GAP apart, on a flat light ground, every block displaced vertically by a parabola that is 0 at both ends of the row and `sag` in
its middle (down for sag > 0, up for sag < 0), and the small photos that reach every branch of the profile kernel.  No font file needed."""
import numpy as np

import detect_cases as cases
from detect_oriented_cases import INK, LETTER_GAP, LETTER_H, LETTER_W, MARGIN, PAPER

ARC_LETTERS = 20
# 1.2 block heights, chosen on the CPU from 30, 36, 40, 45 and 60 so that tests/test_detect_curved.py's two statements hold for the
# restatements alone, for the arc up and down: the polygon's IoU with the ground-truth ribbon is 0.585 / 0.597 and the plain recipe's one
# upright box reaches 0.35.  The polygon is R + 2 p high around glyphs LETTER_H high, and in the steep end bins R exceeds the ring's
# LETTER_H + 2 by about sag / 4 (a bin is w / 16 wide, the slope there 4 sag / w), so its IoU falls with sag roughly as
# 30 / (32 + sag / 4 + 2 p): 0.61 at sag = 30, 0.53 at 45, 0.50 at 60.  The box's is near LETTER_H / (LETTER_H + sag + 2 p).
ARC_SAG = 36


def offsets(letters, sag):
    """The vertical displacement of every block: round(sag * (1 - t^2)), t = -1 .. 1 over the blocks' centres."""
    if letters < 2:
        return [0] * letters
    t = np.linspace(-1.0, 1.0, letters)
    return [int(v) for v in np.rint(sag * (1.0 - t * t))]


def bowed(letters=ARC_LETTERS, sag=ARC_SAG, margin=MARGIN, letter_w=LETTER_W, left=None, margin_y=None):
    """A bowed row -> (photo (H, W, 3) uint8, ground-truth ribbon float64 (2 letters, 2) in pixels: the top edge through the middle of
    every block's top side from left to right, its two ends at the row's ends, then the bottom edge, LETTER_H below, from right to
    left).  margin_y: the paper above and below, by default enough that the row's upright box is no higher than half the photo."""
    left = margin if left is None else left
    margin_y = max(margin, (LETTER_H + abs(sag)) // 2 + 4) if margin_y is None else margin_y
    dy = offsets(letters, sag)
    w = letters * letter_w + (letters - 1) * LETTER_GAP
    a = np.full((LETTER_H + abs(sag) + 2 * margin_y, w + left + margin), PAPER, np.uint8)
    base = margin_y - min(min(dy), 0)
    top = []
    for i in range(letters):
        x, y = left + i * (letter_w + LETTER_GAP), base + dy[i]
        a[y:y + LETTER_H, x:x + letter_w] = INK
        cx = x if i == 0 else x + letter_w if i == letters - 1 else x + letter_w / 2.0
        top.append((cx, float(y)))
    ribbon = np.array(top + [(x, y + LETTER_H) for x, y in reversed(top)], np.float64)
    return cases.gray(a), ribbon


def photo(*args, **kw):
    return bowed(*args, **kw)[0]


def narrow(w):
    """One dark block whose component (its 1-pixel ring included) is exactly w columns wide and 22 rows high, from x = 5."""
    a = np.full((40, w + 12), PAPER, np.uint8)
    a[10:30, 6:4 + w] = INK
    return cases.gray(a)


def two_rows_in_a_word():
    """Two bowed rows of 3 narrow blocks side by side, 20 columns apart (gap = 6 keeps them two components), both inside the first
    64 columns: their rows share lane words, so the profile kernel takes the per-lane branch."""
    a = np.full((60, 70), PAPER, np.uint8)
    for x0, up in ((3, 0), (38, 4)):
        for i, dy in enumerate((0, 6, 0)):
            a[10 + up + dy:30 + up + dy, x0 + 8 * i:x0 + 8 * i + 5] = INK
    return cases.gray(a)


def sparse_arc():
    """A bowed row of one-pixel-high hairlines with tall end posts: curved, and far too empty for the ribbon (the fill filter)."""
    a = np.full((120, 300), PAPER, np.uint8)
    xs = np.arange(20, 280)
    ys = 20 + np.rint(60 * (1 - ((xs - 150) / 130.0) ** 2)).astype(int)
    a[ys, xs] = INK
    a[10:80, 20:22] = INK
    a[10:80, 278:280] = INK
    return cases.gray(a)


def tall_arc():
    """A bowed row whose ribbon is higher than half the working map (2 hc <= hm fails)."""
    return photo(letters=8, sag=20, margin=4, margin_y=4)


def wide_strip():
    """2400 x 40 (r = 3): a gently bowed row of wide blocks along the strip."""
    a = np.full((40, 2400), PAPER, np.uint8)
    for i in range(20):
        t = (i - 9.5) / 9.5
        y = 4 + int(round(8 * (1 - t * t)))
        a[y:y + 24, 300 + i * 90:300 + i * 90 + 60] = INK
    return cases.gray(a)


# name -> (photo, parameters)
CASES = {
    "arc_down": (lambda: photo(), {}),
    "arc_up": (lambda: photo(sag=-ARC_SAG), {}),
    "straight_row": (lambda: photo(sag=0), {}),
    "w16": (lambda: narrow(16), {}),
    "w17": (lambda: narrow(17), {}),
    "crossing_a_word": (lambda: photo(letters=5, sag=16, left=37), {}),      # x0 = 36 .. 121: it crosses x = 64 and a bin edge falls inside a word
    "alone_130": (lambda: photo(letters=7, sag=20, letter_w=13), {}),       # 127 + 2 ring columns: 16 bins, one component per wave row
    "two_in_a_word": (two_rows_in_a_word, dict(gap=6, vgap=1)),
    "flat": (cases.flat, {}),
    "speckle_small": (lambda: cases.speckle(40, 70, 5, 0.02), dict(gap=1, vgap=1)),      # components, none a candidate
    "sparse_arc": (sparse_arc, {}),
    "tall_arc": (tall_arc, {}),
    "wide_strip": (wide_strip, {}),
    "local": (lambda: photo(letters=10, sag=30), dict(local=128)),
    "many": (lambda: cases.bricks(720, 720), dict(gap=1)),      # more components than ops.DETECT_TABLE rows, none 16 wide
    "many_wide": (lambda: many_wide(), dict(gap=1, vgap=1)),
}


def many_wide(h=720, w=720):
    """More components than ops.DETECT_TABLE rows (speckle, gap = vgap = 1), and among them three bowed rows that ARE candidates."""
    a = cases.speckle(h, w, 12, 0.03)
    row = photo(letters=8, sag=14, margin=6, margin_y=6)[:, :, 0]
    for y, x in ((10, 20), (300, 300), (600, 500)):
        a[y:y + row.shape[0], x:x + row.shape[1]] = np.where(row < 128, 230, 4)[:, :, None]      # bright blocks on the dark ground
    return a
