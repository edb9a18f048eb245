"""Photos for the tests of the locally adaptive threshold (utils/detect.py, local=C): the scene with one strong and one faint word, the
ragged batch of the GPU tests and the photos whose gradient histogram is known by construction."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont

import detect_cases as cases

FAINT_AT, FAINT_INK = (360, 330), (168, 168, 168)


def _font(size=40):
    return ImageFont.load_default(size=size)


def scene(noise=True):
    """640 x 480: "street" in black on a white panel (the top-left quarter) and "market" 40 levels from the grey ground; uniform
    noise of -3 .. 3.  The panel's edge and the black word lift the one Otsu threshold of the photo above the faint word's gradient."""
    im = Image.new("RGB", (640, 480), (128, 128, 128))
    d = ImageDraw.Draw(im)
    d.rectangle((0, 0, 320, 240), fill=(250, 250, 250))
    d.text((30, 80), "street", fill=(0, 0, 0), font=_font())
    d.text(FAINT_AT, "market", fill=FAINT_INK, font=_font())
    a = np.asarray(im, np.uint8).astype(np.int16)
    if noise:
        a = a + np.random.default_rng(0).integers(-3, 4, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def faint_ink_box():
    """x0, y0, x1, y1 (ends exclusive) of the pixels that the faint word's ink changes."""
    ys, xs = np.nonzero((scene(False)[250:, 330:] != 128).any(axis=2))      # (clear of the panel, which ends at 320, 240)
    return int(xs.min()) + 330, int(ys.min()) + 250, int(xs.max()) + 331, int(ys.max()) + 251


def ragged_batch():
    """The photos of the GPU tests: 130 x 257 puts the borders of 32-pixel cells off the 64 x 16 tile grid with ragged last tiles;
    1025 x 40 has r = 2 and one column of cells; 1 x 1 and 5 x 300 are a single cell and a single row of them.  Speckle gives every
    cell gradients of its own strengths, so the cell thresholds differ."""
    words = cases.word_photo(seed=11, size=(300, 300), words=(("quay 7", (20, 40)), ("exit", (150, 120)), ("north", (60, 220))))[0]
    return [cases.noise(1, 1, 1), cases.speckle(5, 300, 2), cases.speckle(130, 257, 3), cases.speckle(1025, 40, 4, 0.01), words, scene()]


def gray(y):
    """A luma map as a photo (r = 1): R = G = B = y gives Y = y exactly ((77 + 150 + 29) y + 128) >> 8."""
    y = np.asarray(y, np.uint8)
    return np.repeat(y[:, :, None], 3, axis=2)


def stripes(h, w, period, a, b):
    """Rows of luma a with every `period`-th row b: the 3 x 3 gradient is |a - b| on the rows b - 1 .. b + 1 and 0 elsewhere."""
    y = np.full((h, w), a, np.uint8)
    y[period // 2::period] = b
    return gray(y)
