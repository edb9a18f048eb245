"""Photos that tests/test_detect.py (CPU) and tests/test_gpu_detect.py share: the rendered words of the end-to-end check and the
synthetic photos whose gradient, smoothed map or components are known by construction."""
import numpy as np

WORDS = (("harbour", (24, 30)), ("street 42", (210, 140)), ("open", (60, 250)))
WORD_LUMA, PAPER_LUMA, GRAIN, FONT_SIZE = 60, 215, 4, 28


def word_photo(seed=7, size=(480, 320), words=WORDS):
    """A flat light 480 x 320 photo with three dark words in PIL's default font at size 28 and +-4 levels of seeded grain ->
    (photo (H, W, 3) uint8, [textbbox (x0, y0, x1, y1) per word])."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=FONT_SIZE)
    im = Image.new("RGB", size, (PAPER_LUMA,) * 3)
    draw = ImageDraw.Draw(im)
    boxes = []
    for text, at in words:
        draw.text(at, text, fill=(WORD_LUMA,) * 3, font=font)
        boxes.append(draw.textbbox(at, text, font=font))
    grain = np.random.RandomState(seed).randint(-GRAIN, GRAIN + 1, (size[1], size[0], 1))
    return np.clip(np.asarray(im).astype(np.int64) + grain, 0, 255).astype(np.uint8), boxes


def gray(a):
    """A (h, w) array of levels -> the (h, w, 3) uint8 photo whose luma it is ((77 + 150 + 29) v + 128 >> 8 = v)."""
    return np.repeat(np.asarray(a, np.uint8)[:, :, None], 3, axis=2)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def speckle(h, w, seed, density=0.03):
    """Seeded bright pixels of random level and colour on a dark, slightly grainy ground: gradient blobs of many strengths that the
    smoothing joins here and there -- a threshold inside the histogram, runs of every length, components of every shape."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 12, (h, w, 3))
    on = rng.rand(h, w) < density
    a[on] = rng.randint(40, 256, (int(on.sum()), 3))
    return a.astype(np.uint8)


def flat(h=40, w=70):
    """All background: the gradient is 0 everywhere and nothing reaches the floor."""
    return gray(np.full((h, w), 128))


def all_foreground(h=48, w=150):
    """One-pixel cells of 0 and 255: the gradient is 255 at every pixel -- an all-foreground map, one component whose every pixel is
    united with the pixel before it (the longest chain of unions)."""
    y, x = np.mgrid[:h, :w]
    return gray(((x + y) & 1) * 255)


def checkerboard(h=64, w=136):
    """Bright 2 x 2 dots in the middle of every other 4 x 4 cell: their gradient blobs are the 4 x 4 cells of a checkerboard, which
    touch only at their corners.  With gap = vgap = 1 nothing is filled, and 8-connectivity joins all of them into ONE component
    (4-connectivity would leave every cell alone)."""
    a = np.zeros((h, w), np.uint8)
    for i in range(h // 4):
        for j in range(w // 4):
            if (i + j) % 2 == 0:
                a[4 * i + 1:4 * i + 3, 4 * j + 1:4 * j + 3] = 255
    return gray(a)


def serpentine(n=64):
    """A one-pixel-wide bright line that runs to and fro over an n x n photo, three dark rows between its runs: with gap = vgap = 1 the
    smoothed map is one 3-pixel-wide snake, the longest path a component of this size can have."""
    a = np.zeros((n, n), np.uint8)
    for k, y in enumerate(range(2, n - 2, 6)):
        a[y, 2:n - 2] = 255
        if y + 6 < n - 2:
            a[y:y + 7, n - 3 if k % 2 == 0 else 2] = 255
    return gray(a)


def bricks(h, w, seed=3):
    """Bright bricks 4 high and a seeded 6 .. 8 wide at a pitch of 12 x 9 on a dark ground: with gap = 1 every brick is a component of
    its own, a ring 6 high and 8 .. 10 wide that passes the geometric filters (at least 2 background pixels between two rings of a row, 3
    between two of a column).  A photo that is large enough holds more components than a table of 4096 rows or a list of 256 boxes."""
    a = np.zeros((h, w), np.uint8)
    rng = np.random.RandomState(seed)
    for y in range(2, h - 6, 9):
        for x in range(2, w - 10, 12):
            a[y:y + 4, x:x + 6 + rng.randint(0, 3)] = 255
    return gray(a)
