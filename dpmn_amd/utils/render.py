"""HR text crops from a word list (main.py --train_words): the random draws of one sample (`draw_render`), the size that follows from
them (`render_meta`) and a NumPy restatement of the image (`render_u8`), the CPU reference of the kernel (csrc/render.hip through
ops.render_words_u8).  The semantics are FIXED HERE; integers only, so the kernel reproduces every byte.  The glyphs
come from the PIL / FreeType atlas of utils/glyphs.py (`build_atlases`: one uint8 alpha atlas per font).  The one deliberate difference
from PIL's own draw.text of the whole string: there is NO KERNING AND NO LIGATURE -- every glyph is placed by its own advance, as
k_text_prior (csrc/visionlan.hip) lays its strings out.  A character without a glyph in the atlas (punctuation under voc_type 'all') is
drawn as the blank of class 0; the label keeps it.  Pure NumPy: importable on any machine (PIL only inside build_atlases).

Columns of a params row (int64, 24 per sample):
   0 font        index of the atlas
   1 case        0 lower, 1 upper, 2 capitalised (the first letter upper); the label is the word as filtered, whatever the case
   2 gh          glyph height in pixels, even, 24 .. 64
   3 spacing     extra pixels between two glyphs, -1 .. 4
   4 .. 7        left, right, top, bottom margin, 0 .. gh / 4
   8 shear       s in Q16 (s * 65536), |s| <= 0.3: row y is moved right by (s * (baseline - y)) >> 16 pixels (floor)
   9 .. 11       foreground R, G, B
  12 .. 14       background R, G, B (integer BT.601 luma at least 64 away from the foreground's)
  15 style       background: 0 flat, 1 a horizontal linear gradient to the second colour, 2 a vertical one
  16 .. 18       second background colour R, G, B
  19 seed        63-bit seed of the background grain (+-4 levels per pixel, the counter hash of csrc/degrade.hip)
  20 word        index of the word in the list (not read by the renderer)
  21 .. 23       spare, 0

The image of one sample, h x w = (top + gh + bottom) x (left + text width + ceil(|s| gh) + right), both clamped to MAX_SIDE:
  advance     glyph k of the string has the scaled advance a_k = max(1, (adv * gh + A / 2) // A) (A: the atlas' base height, adv its
              advance there) and starts at pen_k = sum over j < k of (a_j + spacing); text width = pen_n - spacing, at least 1
  shear       u = x - ((s * (baseline - y)) >> 16) - x0, baseline = top + gh - 1, x0 = left (+ ceil(|s| gh) for s < 0); v = y - top
  glyph       the LAST k with pen_k <= u (a later glyph lies over an earlier one where a negative spacing makes them overlap); alpha 0
              outside the text box, and in the gap behind a glyph (u - pen_k >= a_k)
  alpha       the atlas cell sampled at ((2 i + 1) * (A << 16) // gh >> 1) - 32768 (pixel centres; Q16, clamped to the cell) along
              both axes, integer bilinear, (top * (65536 - fy) + bottom * fy + 2^31) >> 32 with top / bottom the two row blends:
              round half up; gh = A reads the atlas byte itself
  background  flat, or (bg * (n - t) + bg2 * t + n / 2) // n with t = x, n = max(w - 1, 1) (style 1) or t = y, n = max(h - 1, 1)
              (style 2); then + grain in -4 .. 4, the same for the three channels, clipped to 0 .. 255
  blend       (fg * a + bg * (255 - a) + 127) // 255 per channel
"""
import os
import zlib

import numpy as np

from .resize import MAX_SIDE

N_PARAMS = 24
(FONT, CASE, GH, SPACING, M_LEFT, M_RIGHT, M_TOP, M_BOTTOM, SHEAR, FG, BG, STYLE, BG2, SEED, WORD) = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 19, 20)
MAX_LEN = 25                 # longest word (characters); longer lines of a word file are dropped
BASE_H = 64                  # base height of an atlas
GH_MIN, GH_MAX = 24, 64
SHEAR_MAX = int(0.3 * 65536)
MIN_CONTRAST = 64            # |luma(fg) - luma(bg)|, integer BT.601
FIXED_DRAWS = 14             # random() calls per sample beside the colour pairs (6 per attempt) and the one getrandbits(63)
N_GLYPH = 37                 # class 0: the blank; class c: DICT36[c - 1]
DICT36 = "abcdefghijklmnopqrstuvwxyz1234567890"      # model/visionlan.py DICT36 (not imported: this module needs no torch)
PHI = 0x9E3779B97F4A7C15     # csrc/common.h DROP_PHI
M64 = (1 << 64) - 1
DEFAULT_EPOCH = 10000


# ---------------------------------------------------------------------------------------------------------------- word list, atlases
def read_words(path, voc_type):
    """The usable words of a word file (one per line, UTF-8): each line filtered with str_filt(line, voc_type); a line that is empty
    after filtering or longer than MAX_LEN characters is dropped.  Prints one line with the count; a file without a usable word is a
    SystemExit."""
    from .util import str_filt
    words, lines = [], 0
    with open(path, encoding="utf-8") as fh:
        for line in fh:
            lines += 1
            w = str_filt(line.strip(), voc_type)
            if 1 <= len(w) <= MAX_LEN:
                words.append(w)
    if not words:
        raise SystemExit("main.py: --train_words %s holds no usable word (%d lines; a word has 1 .. %d characters of voc_type %r)"
                         % (path, lines, MAX_LEN, voc_type))
    print("train_words: %d of %d lines of %s are usable words" % (len(words), lines, path))
    return words


def font_files(dir_):
    """The *.ttf / *.otf files of a directory in sorted name order (full paths)."""
    return [os.path.join(dir_, f) for f in sorted(os.listdir(dir_))
            if f.lower().endswith((".ttf", ".otf")) and os.path.isfile(os.path.join(dir_, f))]


class Atlases(object):
    """alpha (F, 2, 37, GHmax, GWmax) uint8 (case 0 lower, 1 upper; a cell's columns beyond its advance and an atlas' rows beyond its
    height are 0), advance (F, 2, 37) int32 at the base height, height (F,) int32: the base height of every atlas; names: one per
    font (the file's base name, or 'default')."""

    def __init__(self, alpha, advance, height, names):
        self.alpha = np.ascontiguousarray(alpha, np.uint8)
        self.advance = np.ascontiguousarray(advance, np.int32)
        self.height = np.ascontiguousarray(height, np.int32)
        self.names = list(names)
        self.n_fonts = int(self.alpha.shape[0])
        self._device = {}          # ops.render_words_u8: the device copies, per device

    def __getstate__(self):        # (loader workers get the host arrays only)
        d = dict(self.__dict__)
        d["_device"] = {}
        return d


def build_atlases(font_paths=None, heights=BASE_H):
    """One atlas per font on top of glyphs.build_atlas: font_paths a list of font files (None or an empty list: PIL's built-in
    ImageFont.load_default, one atlas per given height; a None entry is the built-in font too), heights the base height of every atlas (one int for
    all, or one per font).  A font PIL cannot open is skipped with one printed line; no usable font at all raises ValueError."""
    from .glyphs import build_atlas
    paths = list(font_paths) if font_paths else [None] * (1 if np.isscalar(heights) else len(heights))
    hs = [int(heights)] * len(paths) if np.isscalar(heights) else [int(h) for h in heights]
    if len(hs) != len(paths) or any(h < 1 or h > 256 for h in hs):
        raise ValueError("build_atlases: one base height in 1 .. 256 per font, got %r for %d fonts" % (heights, len(paths)))
    cells = []
    for p, h in zip(paths, hs):
        try:
            atlas, adv = build_atlas(p, h)
        except Exception as e:      # whatever FreeType raises on a file that is not a font
            print("train_words: skipping font %s (%s: %s)" % (p, type(e).__name__, e))
            continue
        cells.append((atlas.numpy().astype(np.uint8), adv.numpy().astype(np.int32), h, os.path.basename(p) if p else "default"))
    if not cells:
        raise ValueError("build_atlases: no usable font among %r" % (paths,))
    gh, gw = max(c[0].shape[2] for c in cells), max(c[0].shape[3] for c in cells)
    alpha = np.zeros((len(cells), 2, N_GLYPH, gh, gw), np.uint8)
    for f, c in enumerate(cells):
        alpha[f, :, :, :c[0].shape[2], :c[0].shape[3]] = c[0]
    return Atlases(alpha, np.stack([c[1] for c in cells]), [c[2] for c in cells], [c[3] for c in cells])


def words_setting(words, atlases, epoch):
    """The value of the `train_words` field of the --train_state fingerprint (interfaces/base.py): the crc32 of the filtered word
    list, the sorted font names and the epoch size."""
    return {"crc32": zlib.crc32("\n".join(words).encode("utf-8")) & 0xFFFFFFFF, "fonts": sorted(atlases.names), "epoch": int(epoch)}


# -------------------------------------------------------------------------------------------------------------------------- draws
def luma(rgb):
    """integer BT.601"""
    return (299 * int(rgb[0]) + 587 * int(rgb[1]) + 114 * int(rgb[2]) + 500) // 1000


def word_classes(word):
    """A filtered word -> its glyph classes (at most MAX_LEN): DICT36's index + 1 of the lower-cased character, 0 (the blank) for a
    character the atlas does not hold."""
    return [DICT36.find(ch.lower()) + 1 for ch in word[:MAX_LEN]]


def draw_render(words, n_fonts, rng, n=1):
    """The draws of n samples from `rng` (a random.Random, or Python's `random` module) -> (labels: the n drawn words, classes (n, 25)
    int32, lengths (n,) int32, params (n, 24) int64; columns: module docstring).  Only rng.random() and one rng.getrandbits(63) per
    sample are called, sample by sample in this order: word, font, case, gh, spacing, the four margins, shear, style (11 x random());
    foreground and background colour (6 x random()), drawn AGAIN as a pair until their lumas are MIN_CONTRAST apart -- the one part
    whose number of draws is not fixed; the second background colour (3 x random()); the grain seed (getrandbits(63)).  A bounded
    integer is int(random() * k)."""
    def below(k):
        return min(int(rng.random() * k), k - 1)

    n = int(n)
    if not words or n_fonts < 1 or n < 1:
        raise ValueError("draw_render: needs a word, a font and a sample at least")
    labels = []
    classes, lengths = np.zeros((n, MAX_LEN), np.int32), np.zeros(n, np.int32)
    params = np.zeros((n, N_PARAMS), np.int64)
    for i in range(n):
        row = params[i]
        row[WORD] = below(len(words))
        row[FONT] = below(n_fonts)
        row[CASE] = below(3)
        gh = GH_MIN + 2 * below((GH_MAX - GH_MIN) // 2 + 1)
        row[GH] = gh
        row[SPACING] = below(6) - 1
        for c in (M_LEFT, M_RIGHT, M_TOP, M_BOTTOM):
            row[c] = below(gh // 4 + 1)
        row[SHEAR] = below(2 * SHEAR_MAX + 1) - SHEAR_MAX
        row[STYLE] = below(3)
        while True:
            fg = [below(256) for _ in range(3)]
            bg = [below(256) for _ in range(3)]
            if abs(luma(fg) - luma(bg)) >= MIN_CONTRAST:
                break
        row[FG:FG + 3], row[BG:BG + 3] = fg, bg
        row[BG2:BG2 + 3] = [below(256) for _ in range(3)]
        row[SEED] = rng.getrandbits(63)
        word = words[int(row[WORD])]
        cls = word_classes(word)
        labels.append(word)
        classes[i, :len(cls)] = cls
        lengths[i] = len(cls)
    return labels, classes, lengths, params


# ------------------------------------------------------------------------------------------------------------------ layout, image
def check_render(classes, lengths, params, atlases):
    """ValueError for a row outside its domain (what the kernel's entry point rejects too); -> the three arrays in their dtypes."""
    classes = np.ascontiguousarray(classes, np.int32)
    lengths = np.ascontiguousarray(lengths, np.int32).reshape(-1)
    params = np.ascontiguousarray(params, np.int64)
    n = lengths.shape[0]
    if n < 1 or classes.shape != (n, MAX_LEN) or params.shape != (n, N_PARAMS):
        raise ValueError("render: classes (n, %d), lengths (n,), params (n, %d) with n >= 1 expected, got %s %s %s"
                         % (MAX_LEN, N_PARAMS, classes.shape, lengths.shape, params.shape))
    if lengths.min() < 1 or lengths.max() > MAX_LEN:
        raise ValueError("render: a word has a length outside 1 .. %d" % MAX_LEN)
    if classes.min() < 0 or classes.max() >= N_GLYPH:
        raise ValueError("render: a class outside the atlas (0 .. %d)" % (N_GLYPH - 1))
    p = params
    if p[:, FONT].min() < 0 or p[:, FONT].max() >= atlases.n_fonts:
        raise ValueError("render: a font index outside 0 .. %d" % (atlases.n_fonts - 1))
    ok = (np.isin(p[:, CASE], (0, 1, 2)).all() and p[:, GH].min() >= 1 and p[:, GH].max() <= 256 and p[:, SPACING].min() >= -1
          and p[:, SPACING].max() <= 64 and p[:, M_LEFT:M_BOTTOM + 1].min() >= 0 and p[:, M_LEFT:M_BOTTOM + 1].max() <= MAX_SIDE
          and np.abs(p[:, SHEAR]).max() <= 65536 and p[:, FG:FG + 6].min() >= 0 and p[:, FG:FG + 6].max() <= 255
          and p[:, BG2:BG2 + 3].min() >= 0 and p[:, BG2:BG2 + 3].max() <= 255 and np.isin(p[:, STYLE], (0, 1, 2)).all()
          and p[:, SEED].min() >= 0)
    if not ok:
        raise ValueError("render: a params row is outside its domain (case and style 0 / 1 / 2, gh 1 .. 256, spacing -1 .. 64, margins "
                         ">= 0, |shear| <= 65536, colours 0 .. 255, seed >= 0)")
    return classes, lengths, params


def layout(cls, row, atlases):
    """One sample -> (h, w, pens (n + 1,), advs (n,), planes (n,), shear room, x0): the scaled advances and pen positions of the
    string's glyphs (pens[n] = the text width + spacing), the case plane of every glyph, ceil(|s| gh) and the text's left edge."""
    f, gh, sp, s = int(row[FONT]), int(row[GH]), int(row[SPACING]), int(row[SHEAR])
    A = int(atlases.height[f])
    n = len(cls)
    case = int(row[CASE])
    planes = [1 if (case == 1 or (case == 2 and k == 0)) else 0 for k in range(n)]
    advs = [max(1, (int(atlases.advance[f, planes[k], cls[k]]) * gh + A // 2) // A) for k in range(n)]
    pens = [0]
    for a in advs:
        pens.append(pens[-1] + a + sp)
    tw = max(pens[-1] - sp, 1)
    room = (abs(s) * gh + 65535) >> 16
    w = min(int(row[M_LEFT]) + tw + room + int(row[M_RIGHT]), MAX_SIDE)
    h = min(int(row[M_TOP]) + gh + int(row[M_BOTTOM]), MAX_SIDE)
    return h, w, pens, advs, planes, room, int(row[M_LEFT]) + (room if s < 0 else 0)


def render_meta(classes, lengths, params, atlases):
    """(n, 3) int64 of (byte offset, h, w): the images back to back, the layout utils.resize.pack_ragged gives the same images."""
    classes, lengths, params = check_render(classes, lengths, params, atlases)
    meta = np.zeros((lengths.shape[0], 3), np.int64)
    total = 0
    for i in range(lengths.shape[0]):
        h, w = layout(classes[i, :lengths[i]].tolist(), params[i], atlases)[:2]
        meta[i] = total, h, w
        total += h * w * 3
    return meta


def grain(seed, n_pixels):
    """The grain of pixels 0 .. n_pixels - 1 (row-major) in -4 .. 4: splitmix64 of (4 * pixel) * PHI + seed, its top 24 bits mod 9."""
    z = (np.arange(n_pixels, dtype=np.uint64) * np.uint64(4)) * np.uint64(PHI) + np.uint64(int(seed) & M64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return ((z >> np.uint64(40)) % np.uint64(9)).astype(np.int64) - 4


def _axis_sample(idx, A, gh, limit):
    """Atlas coordinates of the scaled indices idx along one axis: (i0, i1, frac) with the cell's last index `limit`."""
    sc = (A << 16) // gh
    q = np.maximum((((2 * idx + 1) * sc) >> 1) - 32768, 0)
    i0 = np.minimum(q >> 16, limit)
    return i0, np.minimum(i0 + 1, limit), q & 0xFFFF


def render_u8(word_classes_, params_row, atlases):
    """One sample -> its (h, w, 3) uint8 image (module docstring): word_classes_ the glyph classes of the word (its length counts),
    params_row one row of draw_render, atlases of build_atlases."""
    cls = [int(c) for c in word_classes_]
    row = np.asarray(params_row, np.int64)
    if not 1 <= len(cls) <= MAX_LEN:
        raise ValueError("render: a word has a length outside 1 .. %d" % MAX_LEN)
    check_render(np.pad(np.asarray(cls, np.int32), (0, MAX_LEN - len(cls)))[None], [len(cls)], row[None], atlases)
    f, gh, s = int(row[FONT]), int(row[GH]), int(row[SHEAR])
    A = int(atlases.height[f])
    h, w, pens, advs, planes, room, x0 = layout(cls, row, atlases)
    n = len(cls)
    tw = max(pens[n] - int(row[SPACING]), 1)
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    v = np.broadcast_to(ys - int(row[M_TOP]), (h, w))
    u = xs - ((s * (int(row[M_TOP]) + gh - 1 - ys)) >> 16) - x0
    pens_a = np.asarray(pens[:n], np.int64)
    k = np.clip(np.searchsorted(pens_a, u, side="right") - 1, 0, n - 1)          # the last k with pen_k <= u
    ug = u - pens_a[k]
    adv_k = np.asarray(advs, np.int64)[k]
    inside = (v >= 0) & (v < gh) & (u >= 0) & (u < tw) & (ug >= 0) & (ug < adv_k)
    cell_w = atlases.advance[f][np.asarray(planes)[k], np.asarray(cls)[k]].astype(np.int64)      # the cell's width at the base height
    ugc, vc = np.where(inside, ug, 0), np.where(inside, v, 0)
    x_0, x_1, fx = _axis_sample(ugc, A, gh, np.maximum(cell_w - 1, 0))
    y_0, y_1, fy = _axis_sample(vc, A, gh, A - 1)
    at, pk, ck = atlases.alpha[f].astype(np.int64), np.asarray(planes)[k], np.asarray(cls)[k]
    a00, a01, a10, a11 = at[pk, ck, y_0, x_0], at[pk, ck, y_0, x_1], at[pk, ck, y_1, x_0], at[pk, ck, y_1, x_1]
    top, bot = a00 * (65536 - fx) + a01 * fx, a10 * (65536 - fx) + a11 * fx
    alpha = np.where(inside, (top * (65536 - fy) + bot * fy + (1 << 31)) >> 32, 0)
    bg, bg2 = row[BG:BG + 3][None, None, :], row[BG2:BG2 + 3][None, None, :]
    style = int(row[STYLE])
    if style == 0:
        back = np.broadcast_to(bg, (h, w, 3))
    else:
        t, m = (xs, max(w - 1, 1)) if style == 1 else (ys, max(h - 1, 1))
        back = np.broadcast_to((bg * (m - t[:, :, None]) + bg2 * t[:, :, None] + m // 2) // m, (h, w, 3))
    back = np.clip(back + grain(row[SEED], h * w).reshape(h, w, 1), 0, 255)
    a = alpha[:, :, None]
    return ((row[FG:FG + 3][None, None, :] * a + back * (255 - a) + 127) // 255).astype(np.uint8)
