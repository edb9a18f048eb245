"""Photos that tests/test_detect_oriented.py (CPU) and tests/test_gpu_detect_oriented.py share: "words" of filled dark rectangles on a
light ground, rotated with PIL, and the small synthetic photos that reach every branch of the oriented kernels.  No font file needed."""
import numpy as np

import detect_cases as cases

ANGLES = (0, 10, 20, 30, 45, 60, 80, 90, -30)      # of the reading direction, degrees, clockwise on the screen (y down)
LETTER_W, LETTER_H, LETTER_GAP, LETTERS, MARGIN = 12, 30, 6, 8, 24
INK, PAPER = 60, 215


def word_image(letters=LETTERS, scale=1, letter_w=LETTER_W):
    """An upright word: `letters` filled rectangles letter_w x LETTER_H, LETTER_GAP apart, MARGIN of paper around -> PIL image (L)."""
    from PIL import Image
    w = letters * letter_w + (letters - 1) * LETTER_GAP
    a = np.full((LETTER_H + 2 * MARGIN, w + 2 * MARGIN), PAPER, np.uint8)
    for i in range(letters):
        x = MARGIN + i * (letter_w + LETTER_GAP)
        a[MARGIN:MARGIN + LETTER_H, x:x + letter_w] = INK
    im = Image.fromarray(a)
    return im.resize((im.width * scale, im.height * scale), Image.NEAREST) if scale > 1 else im


def rotated_word(angle, letters=LETTERS, scale=1, letter_w=LETTER_W):
    """The word read along `angle` degrees (clockwise on the screen: PIL's rotate turns the other way) -> (H, W, 3) uint8."""
    from PIL import Image
    im = word_image(letters, scale, letter_w).rotate(-angle, resample=Image.BICUBIC, expand=True, fillcolor=PAPER)
    return cases.gray(np.asarray(im))


def bar(h=100, w=150, angle=20):
    """A 150 x 100 photo with one slanted bar of 5 letters: it crosses the borders of the 64 x 16 tiles in both directions."""
    from PIL import Image
    im = word_image(5).rotate(-angle, resample=Image.BICUBIC, expand=True, fillcolor=PAPER)
    a = np.full((h, w), PAPER, np.uint8)
    src = np.asarray(im)
    y0, x0 = max((src.shape[0] - h) // 2, 0), max((src.shape[1] - w) // 2, 0)
    cut = src[y0:y0 + h, x0:x0 + w]
    oy, ox = (h - cut.shape[0]) // 2, (w - cut.shape[1]) // 2
    a[oy:oy + cut.shape[0], ox:ox + cut.shape[1]] = cut
    return cases.gray(a)


def large(h=300, w=1100, angle=10):
    """1100 x 300 (r = 2): a word at twice the size, slanted, in the middle of the photo."""
    src = rotated_word(angle, scale=2)[:, :, 0]
    a = np.full((h, w), PAPER, np.uint8)
    y0, x0 = max((src.shape[0] - h) // 2, 0), max((src.shape[1] - w) // 2, 0)
    cut = src[y0:y0 + h, x0:x0 + w]
    oy, ox = (h - cut.shape[0]) // 2, (w - cut.shape[1]) // 2
    a[oy:oy + cut.shape[0], ox:ox + cut.shape[1]] = cut
    return cases.gray(a)


def block(lines=6, letters=5, letter_gap=3, line_gap=8, margin=(24, 70)):
    """A narrow block of horizontal text: `lines` lines of `letters` upright LETTER_W x LETTER_H rectangles, 3 apart, the lines 8
    apart -- the column pass joins the lines into one tall blob."""
    my, mx = margin
    w = letters * LETTER_W + (letters - 1) * letter_gap
    a = np.full((lines * LETTER_H + (lines - 1) * line_gap + 2 * my, w + 2 * mx), PAPER, np.uint8)
    for j in range(lines):
        for i in range(letters):
            y, x = my + j * (LETTER_H + line_gap), mx + i * (LETTER_W + letter_gap)
            a[y:y + LETTER_H, x:x + LETTER_W] = INK
    return cases.gray(a)


def two_in_a_word(h=40, w=60):
    """Two dark blocks 20 x 12 whose rings share rows of ONE 64-pixel word and stay two components (3 pixels of paper between the
    rings, gap = 2): the wave's word holds two roots, the branch of per-pixel atomics."""
    a = np.full((h, w), PAPER, np.uint8)
    a[10:30, 8:20] = INK
    a[14:34, 25:37] = INK
    return cases.gray(a)


def many(h=720, w=720, seed=12):
    """Speckle that leaves more components than a table of ops.DETECT_TABLE rows in both passes (gap = vgap = 1)."""
    return cases.speckle(h, w, seed, 0.03)


# name -> (photo, parameters)
CASES = {"angle_%d" % a: ((lambda a=a: rotated_word(a)), {}) for a in ANGLES}
CASES.update({
    "bar": (bar, {}),
    "block": (block, {}),
    "large": (large, {}),
    "flat": (cases.flat, {}),
    "1x1": (lambda: cases.noise(1, 1, 1), {}),
    "two_in_a_word": (two_in_a_word, dict(gap=2, vgap=1)),
    "many": (many, dict(gap=1, vgap=1)),
})
