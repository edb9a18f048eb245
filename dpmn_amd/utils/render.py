"""HR text crops from a word list (main.py --train_words): the random draws of one sample (`draw_render`), the size that follows from
them (`render_meta`) and a NumPy restatement of the image (`render_u8`), the CPU reference of the kernel (csrc/render.hip through
ops.render_words_u8).  The semantics are FIXED HERE; integers only, so the kernel reproduces every byte.  The glyphs
come from the PIL / FreeType atlas of utils/glyphs.py (`build_atlases`: one uint8 alpha atlas per font).  The one deliberate difference
from PIL's own draw.text of the whole string: there is NO KERNING AND NO LIGATURE -- every glyph is placed by its own advance, as
k_text_prior (csrc/visionlan.hip) lays its strings out.  A character without a glyph in the atlas (punctuation under voc_type 'all') is
drawn as the blank of class 0; the label keeps it.  Pure NumPy: importable on any machine (PIL only inside build_atlases and
load_backgrounds).  Outline, drop shadow and photo backgrounds (main.py --train_words_fx) stand beside all this at the end of the module:
draw_render_fx, check_render_fx, render_fx_u8; behind them projective distortion, rotation and a curved baseline (main.py
--train_words_warp): draw_render_warp, warp_row, check_render_warp, render_warp_meta, render_warp_u8 (the columns of a warp row and every
formula: the comment above N_WARP).

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


def words_setting(words, atlases, epoch, fx=None, warp=None):
    """The value of the `train_words` field of the --train_state fingerprint (interfaces/base.py): the crc32 of the filtered word
    list, the sorted font names and the epoch size; with a RenderFx (main.py --train_words_fx), and only then, also its kinds, its
    probability and the crc32 of its background pool (None without one); with a RenderWarp (main.py --train_words_warp), and only
    then, also its kinds, its probability and its three magnitudes."""
    s = {"crc32": zlib.crc32("\n".join(words).encode("utf-8")) & 0xFFFFFFFF, "fonts": sorted(atlases.names), "epoch": int(epoch)}
    if fx:
        s.update(fx_kinds=list(fx.kinds), fx_prob=float(fx.prob), fx_pool=None if fx.pool is None else int(fx.pool.crc32))
    if warp:
        s.update(warp_setting(warp))
    return s


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


# ------------------------------------------------------------------------------- outline, drop shadow, photo background (the fx path)
# main.py --train_words_fx: three more stages of the MJSynth recipe BESIDE the plain renderer above, which stays as it is -- the draws
# of a sample (`draw_render_fx`: draw_render's, then the fx draws), the domain of an fx row (`check_render_fx`) and the NumPy
# restatement of the image (`render_fx_u8`), the CPU reference of k_render_words_fx (csrc/render.hip through ops.render_words_fx_u8).
# The canvas is layout's, so render_meta serves both paths; with flags 0 the image is render_u8's byte for byte.
#
# Columns of an fx row (int64, 20 per sample); the columns of a kind whose flag bit is 0 are not read:
#    0 flags      bit 0 outline, bit 1 shadow, bit 2 texture
#    1 r          outline radius, 1 .. 3
#    2 .. 4       outline R, G, B (drawn with an integer BT.601 luma at least MIN_CONTRAST away from the foreground's)
#    5, 6         shadow offset dx, dy, each -3 .. 3, not both 0
#    7 q          shadow opacity, 96 .. 255
#    8 .. 10      shadow R, G, B
#   11 photo      index of the photo in the pool
#   12 .. 15      crop x0, y0, cw, ch inside that photo
#   16 m          blend weight of the texture, 64 .. 224 (of 256)
#   17 .. 19      spare, 0
#
# The image, with alpha(x, y) the plane of render_u8 and 0 outside the canvas:
#   background  style 0 / 1 / 2 as render_u8 gives bg; with the texture bit the crop is sampled at the canvas pixel's centre --
#               _axis_sample(x, cw, w, cw - 1) along x, _axis_sample(y, ch, h, ch - 1) along y, the integer bilinear blend of alpha
#               per channel -> tex; bg = (tex * m + bg * (256 - m) + 128) >> 8; then + grain, clipped, as render_u8 -> c
#   shadow      a_s = (alpha(x - dx, y - dy) * q + 127) // 255;  c = (shadow * a_s + c * (255 - a_s) + 127) // 255
#   outline     a_o = the largest alpha(x + i, y + j) over the disk i * i + j * j <= r * r (5, 13, 29 points);  c blended the same way
#   fill        (fg * alpha + c * (255 - alpha) + 127) // 255
N_FX = 20
(FX_FLAGS, FX_R, FX_OUTLINE, FX_DX, FX_DY, FX_Q, FX_SHADOW, FX_PHOTO, FX_X0, FX_Y0, FX_CW, FX_CH, FX_M) = (0, 1, 2, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16)
FX_KINDS = ("outline", "shadow", "texture")      # bit k of the flags: kind k
R_MAX = 3                    # largest outline radius and shadow offset: the halo of the kernel's alpha tile
Q_MIN, Q_MAX = 96, 255
M_MIN, M_MAX = 64, 224
POOL_SIDE = 512              # load_backgrounds: a photo's long side after the reduction
POOL_MAX_PHOTOS, POOL_MAX_BYTES = 4096, 512 << 20


class Backgrounds(object):
    """The pool of background photos: pixels, 1-D uint8, the photos back to back (HWC, the layout of utils.resize.pack_ragged); table
    (n, 3) int64 of (byte offset, h, w); crc32 of the pixels (the --train_state fingerprint).  images: (h, w, 3) uint8 arrays."""

    def __init__(self, images):
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        if not images or any(im.ndim != 3 or im.shape[2] != 3 or min(im.shape[:2]) < 1 or max(im.shape[:2]) > MAX_SIDE for im in images):
            raise ValueError("Backgrounds: one (h, w, 3) uint8 photo at least, sides 1 .. %d" % MAX_SIDE)
        sizes = np.asarray([im.size for im in images], np.int64)
        self.table = np.stack([np.cumsum(sizes) - sizes, [im.shape[0] for im in images], [im.shape[1] for im in images]], axis=1).astype(np.int64)
        self.pixels = np.concatenate([im.reshape(-1) for im in images])
        self.n_photos = len(images)
        self.crc32 = zlib.crc32(self.pixels.tobytes()) & 0xFFFFFFFF
        self._device = {}          # ops.render_words_fx_u8: the device copies, per device

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_device"] = {}
        return d

    def photo(self, i):
        off, h, w = (int(v) for v in self.table[i])
        return self.pixels[off:off + h * w * 3].reshape(h, w, 3)


def load_backgrounds(dir_):
    """The pool of --train_words_backgrounds: every file of the folder that PIL opens, in sorted name order, converted to RGB; a photo
    whose long side passes POOL_SIDE is reduced with Image.thumbnail((512, 512), BICUBIC).  At most 4096 photos and 512 MB are kept;
    what is left over is dropped with one printed line.  ValueError for a folder without a usable photo."""
    from PIL import Image
    images, total, dropped = [], 0, 0
    names = [f for f in sorted(os.listdir(dir_)) if os.path.isfile(os.path.join(dir_, f))]
    for k, f in enumerate(names):
        try:
            with Image.open(os.path.join(dir_, f)) as im:
                im = im.convert("RGB")
                if max(im.size) > POOL_SIDE:
                    im.thumbnail((POOL_SIDE, POOL_SIDE), Image.BICUBIC)
                a = np.asarray(im, np.uint8)
        except Exception:          # whatever PIL raises on a file that is no image
            continue
        if len(images) >= POOL_MAX_PHOTOS or total + a.size > POOL_MAX_BYTES:
            dropped = len(names) - k
            break
        images.append(a)
        total += a.size
    if not images:
        raise ValueError("%s holds no image that PIL can open" % dir_)
    if dropped:
        print("train_words: the background pool is full (%d photos, %d bytes); the last %d files of %s are not read"
              % (len(images), total, dropped, dir_))
    print("train_words: %d background photos of %s, %d bytes" % (len(images), dir_, total))
    return Backgrounds(images)


class RenderFx(object):
    """The fx setting of a run: kinds (of FX_KINDS, kept in that order), prob (each listed kind is on per sample with this probability,
    independently), pool (a Backgrounds; texture needs it, and only texture takes it) and atlases (texture needs them: the crop is
    drawn against the sample's canvas size)."""

    def __init__(self, kinds, prob=0.5, pool=None, atlases=None):
        self.kinds = fx_kinds(kinds, prob, pool is not None)
        if pool is not None and atlases is None:
            raise ValueError("RenderFx: texture needs the atlases (the crop is drawn against the canvas size)")
        self.prob, self.pool, self.atlases = float(prob), pool, atlases


def fx_kinds(kinds, prob, has_pool):
    """The checks of --train_words_fx / --train_words_fx_prob / --train_words_backgrounds on the values alone -> the kinds in FX_KINDS'
    order; ValueError with the one line main.py prints."""
    kinds = [str(k) for k in kinds]
    if not kinds or len(set(kinds)) != len(kinds) or any(k not in FX_KINDS for k in kinds):
        raise ValueError("--train_words_fx takes a comma list of distinct kinds of %s, got %r" % (", ".join(FX_KINDS), ",".join(kinds)))
    if not 0.0 <= float(prob) <= 1.0:          # (NaN fails both comparisons)
        raise ValueError("--train_words_fx_prob must be a probability in 0 .. 1, got %r" % (prob,))
    if ("texture" in kinds) != bool(has_pool):
        raise ValueError("--train_words_fx texture and --train_words_backgrounds DIR go together: the texture is a crop of a photo of "
                         "that folder")
    return tuple(k for k in FX_KINDS if k in kinds)


def draw_render_fx(words, n_fonts, rng, n=1, fx=()):
    """draw_render plus the fx rows: -> (labels, classes, lengths, params, fx (n, 20) int64).  fx: a RenderFx, or () / None: no fx
    draw at all and rows of zeros.  Sample by sample: exactly the draws of draw_render for ONE sample, then for every LISTED kind in
    the order outline, shadow, texture one random() -- the kind is on where it is below prob -- followed at once, where the kind is
    on, by its parameters, every one of them below(k) = int(random() * k):
      outline   r - 1 (3); R, G, B (256 each), the triple drawn AGAIN until its luma is MIN_CONTRAST away from the foreground's
      shadow    dx + 3, dy + 3 (7 each), the pair drawn AGAIN while both are 0; q - 96 (160); R, G, B (256 each)
      texture   photo (the pool's size); cw - max(1, w // 2) (2 w - max(1, w // 2) + 1), then clipped to the photo's width pw;
                ch = max(1, cw * h // w) clipped to the photo's height ph, no draw; x0 (pw - cw + 1); y0 (ph - ch + 1); m - 64 (161)
                -- h, w: the sample's canvas size from layout
    A kind that is not listed makes no draw; one that is listed and off makes the one."""
    def below(k):
        return min(int(rng.random() * k), k - 1)

    n = int(n)
    labels, classes, lengths, params = [], [], [], []
    rows = np.zeros((max(n, 0), N_FX), np.int64)
    if n < 1:
        draw_render(words, n_fonts, rng, n)          # (its ValueError)
    for i in range(n):
        l, c, ln, p = draw_render(words, n_fonts, rng, 1)
        labels += l
        classes.append(c)
        lengths.append(ln)
        params.append(p)
        if not fx:
            continue
        row, fg = rows[i], p[0, FG:FG + 3]
        if "outline" in fx.kinds and rng.random() < fx.prob:
            row[FX_FLAGS] |= 1
            row[FX_R] = 1 + below(R_MAX)
            while True:
                col = [below(256) for _ in range(3)]
                if abs(luma(col) - luma(fg)) >= MIN_CONTRAST:
                    break
            row[FX_OUTLINE:FX_OUTLINE + 3] = col
        if "shadow" in fx.kinds and rng.random() < fx.prob:
            row[FX_FLAGS] |= 2
            while True:
                dx, dy = below(2 * R_MAX + 1) - R_MAX, below(2 * R_MAX + 1) - R_MAX
                if dx or dy:
                    break
            row[FX_DX], row[FX_DY] = dx, dy
            row[FX_Q] = Q_MIN + below(Q_MAX - Q_MIN + 1)
            row[FX_SHADOW:FX_SHADOW + 3] = [below(256) for _ in range(3)]
        if "texture" in fx.kinds and rng.random() < fx.prob:
            row[FX_FLAGS] |= 4
            h, w = layout(c[0, :ln[0]].tolist(), p[0], fx.atlases)[:2]
            k = below(fx.pool.n_photos)
            ph, pw = int(fx.pool.table[k, 1]), int(fx.pool.table[k, 2])
            lo = max(1, w // 2)
            cw = min(lo + below(2 * w - lo + 1), pw)
            ch = min(max(1, cw * h // w), ph)
            row[FX_PHOTO], row[FX_CW], row[FX_CH] = k, cw, ch
            row[FX_X0] = below(pw - cw + 1)
            row[FX_Y0] = below(ph - ch + 1)
            row[FX_M] = M_MIN + below(M_MAX - M_MIN + 1)
    return labels, np.concatenate(classes), np.concatenate(lengths), np.concatenate(params), rows


def check_render_fx(fx, pool=None, n=None):
    """ValueError for an fx row outside its domain or a crop that leaves its photo (what the kernel's entry point rejects too); only
    the columns of the kinds whose flag bit is set are read, the spare columns are 0 -> the rows as (n, 20) int64."""
    fx = np.ascontiguousarray(fx, np.int64)
    if fx.ndim != 2 or fx.shape[1] != N_FX or fx.shape[0] < 1 or (n is not None and fx.shape[0] != n):
        raise ValueError("render_fx: fx (n, %d) with one row per sample expected, got %s" % (N_FX, fx.shape))
    fl = fx[:, FX_FLAGS]
    if fl.min() < 0 or fl.max() > 7 or fx[:, FX_M + 1:].any():
        raise ValueError("render_fx: flags outside 0 .. 7, or a spare column that is not 0")
    o, s, t = fx[(fl & 1) != 0], fx[(fl & 2) != 0], fx[(fl & 4) != 0]
    if o.size and not (o[:, FX_R].min() >= 1 and o[:, FX_R].max() <= R_MAX and o[:, FX_OUTLINE:FX_OUTLINE + 3].min() >= 0
                       and o[:, FX_OUTLINE:FX_OUTLINE + 3].max() <= 255):
        raise ValueError("render_fx: an outline outside its domain (radius 1 .. %d, colour 0 .. 255)" % R_MAX)
    if s.size and not (np.abs(s[:, FX_DX:FX_DY + 1]).max() <= R_MAX and (s[:, FX_DX:FX_DY + 1] != 0).any(axis=1).all()
                       and s[:, FX_Q].min() >= Q_MIN and s[:, FX_Q].max() <= Q_MAX and s[:, FX_SHADOW:FX_SHADOW + 3].min() >= 0
                       and s[:, FX_SHADOW:FX_SHADOW + 3].max() <= 255):
        raise ValueError("render_fx: a shadow outside its domain (dx, dy in -%d .. %d and not both 0, q %d .. %d, colour 0 .. 255)"
                         % (R_MAX, R_MAX, Q_MIN, Q_MAX))
    if t.size:
        if pool is None:
            raise ValueError("render_fx: a row has the texture bit and there is no pool of photos")
        k = t[:, FX_PHOTO]
        if k.min() < 0 or k.max() >= pool.n_photos:
            raise ValueError("render_fx: a photo index outside the pool (0 .. %d)" % (pool.n_photos - 1))
        ph, pw = pool.table[k, 1], pool.table[k, 2]
        if not ((t[:, FX_X0:FX_Y0 + 1] >= 0).all() and (t[:, FX_CW:FX_CH + 1] >= 1).all() and (t[:, FX_X0] + t[:, FX_CW] <= pw).all()
                and (t[:, FX_Y0] + t[:, FX_CH] <= ph).all()):
            raise ValueError("render_fx: a crop leaves its photo (x0, y0 >= 0, cw, ch >= 1, x0 + cw <= the photo's width, y0 + ch <= its height)")
        if t[:, FX_M].min() < M_MIN or t[:, FX_M].max() > M_MAX:
            raise ValueError("render_fx: a blend weight outside %d .. %d" % (M_MIN, M_MAX))
    return fx


def _alpha_plane(cls, row, atlases):
    """The alpha plane (h, w) int64 of render_u8 -- the same statements, up to the plane."""
    f, gh, s = int(row[FONT]), int(row[GH]), int(row[SHEAR])
    A = int(atlases.height[f])
    h, w, pens, advs, planes, room, x0 = layout(cls, row, atlases)
    n = len(cls)
    tw = max(pens[n] - int(row[SPACING]), 1)
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    v = np.broadcast_to(ys - int(row[M_TOP]), (h, w))
    u = xs - ((s * (int(row[M_TOP]) + gh - 1 - ys)) >> 16) - x0
    pens_a = np.asarray(pens[:n], np.int64)
    k = np.clip(np.searchsorted(pens_a, u, side="right") - 1, 0, n - 1)
    ug = u - pens_a[k]
    inside = (v >= 0) & (v < gh) & (u >= 0) & (u < tw) & (ug >= 0) & (ug < np.asarray(advs, np.int64)[k])
    pk, ck = np.asarray(planes)[k], np.asarray(cls)[k]
    cell_w = atlases.advance[f][pk, ck].astype(np.int64)
    x_0, x_1, fx = _axis_sample(np.where(inside, ug, 0), A, gh, np.maximum(cell_w - 1, 0))
    y_0, y_1, fy = _axis_sample(np.where(inside, v, 0), A, gh, A - 1)
    at = atlases.alpha[f].astype(np.int64)
    top = at[pk, ck, y_0, x_0] * (65536 - fx) + at[pk, ck, y_0, x_1] * fx
    bot = at[pk, ck, y_1, x_0] * (65536 - fx) + at[pk, ck, y_1, x_1] * fx
    return np.where(inside, (top * (65536 - fy) + bot * fy + (1 << 31)) >> 32, 0)


def _shifted(alpha, dx, dy):
    """alpha(x + dx, y + dy) as a plane, 0 where that leaves the canvas."""
    h, w = alpha.shape
    out = np.zeros_like(alpha)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = alpha[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def _fx_planes(alpha, fxr):
    """(a_s, a_o): the shadow's and the outline's alpha planes of one sample, zeros for a kind whose flag bit is 0."""
    flags = int(fxr[FX_FLAGS])
    a_s = a_o = np.zeros_like(alpha)
    if flags & 2:
        a_s = (_shifted(alpha, -int(fxr[FX_DX]), -int(fxr[FX_DY])) * int(fxr[FX_Q]) + 127) // 255
    if flags & 1:
        r = int(fxr[FX_R])
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                if i * i + j * j <= r * r:
                    a_o = np.maximum(a_o, _shifted(alpha, i, j))
    return a_s, a_o


def _render_fx(cls, row, fxr, atlases, pool, grain_plane=None, alpha=None):
    """render_fx_u8 behind its checks: the fx row is taken as it is (a test may pass m = 256, the crop's own bytes), grain_plane
    (h, w) replaces the grain of the row's seed, alpha (h, w) the plane of _alpha_plane (render_warp_u8: the warped plane, whose
    shape is then the canvas)."""
    if alpha is None:
        alpha = _alpha_plane(cls, row, atlases)
    h, w = alpha.shape
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    bg, bg2 = row[BG:BG + 3][None, None, :], row[BG2:BG2 + 3][None, None, :]
    style, flags = int(row[STYLE]), int(fxr[FX_FLAGS])
    if style == 0:
        back = np.broadcast_to(bg, (h, w, 3))
    else:
        t, m = (xs, max(w - 1, 1)) if style == 1 else (ys, max(h - 1, 1))
        back = np.broadcast_to((bg * (m - t[:, :, None]) + bg2 * t[:, :, None] + m // 2) // m, (h, w, 3))
    if flags & 4:
        x0, y0, cw, ch, m = (int(fxr[c]) for c in (FX_X0, FX_Y0, FX_CW, FX_CH, FX_M))
        crop = pool.photo(int(fxr[FX_PHOTO]))[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
        x_0, x_1, fx = _axis_sample(xs, cw, w, cw - 1)
        y_0, y_1, fy = _axis_sample(ys, ch, h, ch - 1)
        fx, fy = fx[:, :, None], fy[:, :, None]
        top = crop[y_0, x_0] * (65536 - fx) + crop[y_0, x_1] * fx
        bot = crop[y_1, x_0] * (65536 - fx) + crop[y_1, x_1] * fx
        tex = (top * (65536 - fy) + bot * fy + (1 << 31)) >> 32
        back = (tex * m + back * (256 - m) + 128) >> 8
    g = grain(row[SEED], h * w).reshape(h, w) if grain_plane is None else np.asarray(grain_plane, np.int64).reshape(h, w)
    c = np.clip(back + g[:, :, None], 0, 255)

    def over(colour, a):
        a = a[:, :, None]
        return (np.asarray(colour, np.int64)[None, None, :] * a + c * (255 - a) + 127) // 255

    a_s, a_o = _fx_planes(alpha, fxr)
    c = over(fxr[FX_SHADOW:FX_SHADOW + 3], a_s)
    c = over(fxr[FX_OUTLINE:FX_OUTLINE + 3], a_o)
    return over(row[FG:FG + 3], alpha).astype(np.uint8)


def render_fx_u8(word_classes_, params_row, fx_row, atlases, pool=None):
    """One sample -> its (h, w, 3) uint8 image with outline, shadow and photo background (the comment above states every formula):
    word_classes_ and params_row as render_u8 takes them, fx_row one row of draw_render_fx, pool the Backgrounds (None: no row may
    have the texture bit).  The canvas is render_u8's; an outline or a shadow that reaches past a margin is clipped at its edge."""
    cls = [int(c) for c in word_classes_]
    row = np.asarray(params_row, np.int64)
    if not 1 <= len(cls) <= MAX_LEN:
        raise ValueError("render: a word has a length outside 1 .. %d" % MAX_LEN)
    check_render(np.pad(np.asarray(cls, np.int32), (0, MAX_LEN - len(cls)))[None], [len(cls)], row[None], atlases)
    fxr = check_render_fx(np.asarray(fx_row, np.int64)[None], pool)[0]
    return _render_fx(cls, row, fxr, atlases, pool)


# ----------------------------------------------------------------------- projective distortion, rotation, curved baseline (the warp path)
# main.py --train_words_warp: two more stages of the synthetic-text recipes (MJSynth's projective distortion, SynthText's curved
# baseline) BESIDE the two renderers above, which stay as they are -- the draws of a sample (`draw_render_warp`: draw_render_fx's, then
# the warp draws), the host's one computation of a warp row (`warp_row`, Python floats), the domain of a row (`check_render_warp`), the
# canvas sizes (`render_warp_meta`, the sibling of render_meta) and the NumPy restatement of the image (`render_warp_u8`), the CPU
# reference of k_render_words_warp (csrc/render.hip through ops.render_words_warp_u8).  Only the TEXT is warped (the fill alpha and
# what the outline and the shadow take from it, on the warped plane, in output pixels); the background stays a function of the output
# pixel.  A row whose flags are 0 is not read: the sample takes the integer path above, canvas and bytes are render_fx_u8's.
#
# Columns of a warp row (int64, 16 per sample):
#    0 flags      bit 0 perspective, bit 1 rotate, bit 2 curve
#    1 amp        the parabola's height in the middle of the canvas, Q16 pixels, signed (negative: the word arches upward);
#                 |amp| <= CURVE_MAX * gh; 0 without the curve bit
#    2 room       ceil(|amp|) in whole pixels: the bent flat canvas is layout's w0 x (h0 + room)
#    3 .. 11      c0 .. c8, the INVERSE projective map, output pixel -> bent flat canvas, normalised so that the largest magnitude
#                 is COEF_MAX = 2^30 and rounded to integers; THESE INTEGERS ARE THE DEFINITION, nothing is solved later
#   12, 13        H, W: the output canvas, the bounding box of the forward-mapped corners of the bent flat canvas moved to the origin,
#                 1 .. MAX_SIDE
#   14, 15        spare, 0
#
# The alpha of output pixel (x, y), integers only, every division a FLOOR division (the flat coordinates go negative left of and
# above the text), positions in Q16 with a pixel's centre at i + 1/2:
#   map       X = 2 x + 1, Y = 2 y + 1 (twice the pixel centre);  den = c6 X + c7 Y + 2 c8 (> 0 on the whole canvas: checked at its
#             four corners);  px = ((c0 X + c1 Y + 2 c2) * 65536) // den,  py = ((c3 X + c4 Y + 2 c5) * 65536) // den
#             bound: |c| <= 2^30, X, Y <= 2^14 - 1, so |numerator| < 2^30 * 2^15 and |numerator * 65536| < 2^61.0001 < 2^62
#   column    alpha 0 unless 0 <= px < w0 * 65536
#   parabola  xq = px >> 12, Wq = w0 << 4 (sixteenths of a pixel);  p = (amp * 4 * xq * (Wq - xq)) // (Wq * Wq) -- 0 at both ends,
#             amp in the middle; |amp| < 2^23 and 4 xq (Wq - xq) <= Wq^2 <= 2^34, so the product stays below 2^57;
#             vq = py - (room << 16 if amp < 0 else 0) - p - (top << 16);  alpha 0 unless 0 <= vq < gh * 65536
#   shear     uq = px - ((s * (((gh - 1) << 16) + 32768 - vq)) >> 16) - (x0 << 16): the shear of render_u8 at the fractional row (not
#             floored to whole pixels);  alpha 0 unless 0 <= uq < tw * 65536
#   glyph     the LAST k with pen_k <= uq >> 16, as render_u8;  ugq = uq - (pen_k << 16);  alpha 0 in the gap (ugq >= a_k * 65536)
#   sample    the atlas cell at ((pos * sc) >> 16) - 32768 with sc = (A << 16) // gh, pos = ugq along x (clamped to the cell's width)
#             and vq along y -- at a pixel's centre, pos = (2 i + 1) << 15, this is render_u8's coordinate exactly; the same integer
#             bilinear blend, round half up
# Then the stages of render_fx_u8 on the H x W canvas with this plane: background, texture (the crop stretched over H x W), grain,
# shadow, outline, fill.  The columns are displaced, the glyphs are not turned along the curve; nothing is prefiltered.
N_WARP = 16
(WP_FLAGS, WP_AMP, WP_ROOM, WP_COEF, WP_H, WP_W) = (0, 1, 2, 3, 12, 13)
WARP_KINDS = ("perspective", "rotate", "curve")      # bit k of the flags: kind k
COEF_MAX = 1 << 30           # the largest magnitude of a coefficient: what keeps numerator * 65536 below 2^62 on canvases up to MAX_SIDE
PERSP_MAX, ANGLE_MAX, CURVE_MAX = 0.3, 20.0, 0.4      # the upper ends of --train_words_warp_persp / _angle / _curve


def warp_kinds(kinds, prob=0.5, persp=0.15, angle=10.0, curve=0.2):
    """The checks of --train_words_warp / _prob / _persp / _angle / _curve on the values alone -> the kinds in WARP_KINDS' order;
    ValueError with the one line main.py prints."""
    kinds = [str(k) for k in kinds]
    if not kinds or len(set(kinds)) != len(kinds) or any(k not in WARP_KINDS for k in kinds):
        raise ValueError("--train_words_warp takes a comma list of distinct kinds of %s, got %r" % (", ".join(WARP_KINDS), ",".join(kinds)))
    if not 0.0 <= float(prob) <= 1.0:          # (NaN fails both comparisons)
        raise ValueError("--train_words_warp_prob must be a probability in 0 .. 1, got %r" % (prob,))
    if not 0.0 < float(persp) <= PERSP_MAX:
        raise ValueError("--train_words_warp_persp must be a fraction of the glyph height in 0 < F <= %g, got %r" % (PERSP_MAX, persp))
    if not 0.0 < float(angle) <= ANGLE_MAX:
        raise ValueError("--train_words_warp_angle must be an angle in degrees in 0 < DEG <= %g, got %r" % (ANGLE_MAX, angle))
    if not 0.0 < float(curve) <= CURVE_MAX:
        raise ValueError("--train_words_warp_curve must be a fraction of the glyph height in 0 < F <= %g, got %r" % (CURVE_MAX, curve))
    return tuple(k for k in WARP_KINDS if k in kinds)


class RenderWarp(object):
    """The warp setting of a run: kinds (of WARP_KINDS, kept in that order), prob (each listed kind is on per sample with this
    probability, independently), persp / angle / curve (the three magnitudes) and atlases (the warp is drawn against the sample's flat
    canvas, which layout computes from them)."""

    def __init__(self, kinds, prob=0.5, persp=0.15, angle=10.0, curve=0.2, atlases=None):
        self.kinds = warp_kinds(kinds, prob, persp, angle, curve)
        if atlases is None:
            raise ValueError("RenderWarp: the warp needs the atlases (it is drawn against the flat canvas)")
        self.prob, self.persp, self.angle, self.curve, self.atlases = float(prob), float(persp), float(angle), float(curve), atlases


def warp_setting(warp):
    """The fields a RenderWarp adds to words_setting."""
    return dict(warp_kinds=list(warp.kinds), warp_prob=float(warp.prob), warp_persp=float(warp.persp), warp_angle=float(warp.angle),
                warp_curve=float(warp.curve))


def warp_quad(h0, w0, room=0, angle=0.0, jitter=None):
    """The forward image of the corners of the bent flat canvas (w0 x (h0 + room); top left, top right, bottom right, bottom left)
    before it is moved to the origin, in Python floats: turned about the canvas' centre by `angle` degrees (positive: clockwise on the
    screen, y pointing down), then every corner moved by its own jitter[k] = (dx, dy) pixels."""
    import math
    hb = h0 + room
    cx, cy = w0 / 2.0, hb / 2.0
    co, si = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    quad = []
    for k, (x, y) in enumerate(((0, 0), (w0, 0), (w0, hb), (0, hb))):
        qx, qy = cx + co * (x - cx) - si * (y - cy), cy + si * (x - cx) + co * (y - cy)
        if jitter is not None:
            qx, qy = qx + float(jitter[k][0]), qy + float(jitter[k][1])
        quad.append((qx, qy))
    return quad


def warp_row(h0, w0, flags, amp=0, angle=0.0, jitter=None):
    """One warp row from the flat canvas h0 x w0 of layout and the drawn magnitudes: amp (Q16 pixels; read with the curve bit), angle
    (degrees; with the rotate bit), jitter (four (dx, dy) in pixels; with the perspective bit).  ONE projective map takes the corners
    of the bent flat canvas to warp_quad's; its inverse (the adjugate), scaled so that the largest magnitude is COEF_MAX and rounded
    half up, is the row.  flags 0 -> a row of zeros.  ValueError where the quadrilateral is not convex enough for den > 0."""
    import math
    row = np.zeros(N_WARP, np.int64)
    flags = int(flags)
    if not flags:
        return row
    amp = int(amp) if flags & 4 else 0
    room = (abs(amp) + 65535) >> 16
    hb = h0 + room
    quad = warp_quad(h0, w0, room, angle if flags & 2 else 0.0, jitter if flags & 1 else None)
    x_min, y_min = min(q[0] for q in quad), min(q[1] for q in quad)
    W = min(max(int(math.ceil(max(q[0] for q in quad) - x_min)), 1), MAX_SIDE)
    H = min(max(int(math.ceil(max(q[1] for q in quad) - y_min)), 1), MAX_SIDE)
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(q[0] - x_min, q[1] - y_min) for q in quad]
    # the unit square -> the quadrilateral (Heckbert), then the flat canvas -> the unit square
    dx1, dx2, sx, dy1, dy2, sy = x1 - x2, x3 - x2, x0 - x1 + x2 - x3, y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    det = dx1 * dy2 - dy1 * dx2
    if det == 0.0:
        raise ValueError("render_warp: a degenerate quadrilateral")
    g, h = (sx * dy2 - dx2 * sy) / det, (dx1 * sy - sx * dy1) / det
    F = [[(x1 - x0 + g * x1) / w0, (x3 - x0 + h * x3) / hb, x0], [(y1 - y0 + g * y1) / w0, (y3 - y0 + h * y3) / hb, y0], [g / w0, h / hb, 1.0]]
    (a, b, c), (d, e, f), (g, h, i) = F
    inv = [e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d]
    if inv[6] * W / 2.0 + inv[7] * H / 2.0 + inv[8] < 0.0:
        inv = [-v for v in inv]
    scale = COEF_MAX / max(abs(v) for v in inv)
    row[WP_FLAGS], row[WP_AMP], row[WP_ROOM], row[WP_H], row[WP_W] = flags, amp, room, H, W
    row[WP_COEF:WP_COEF + 9] = [int(math.floor(v * scale + 0.5)) for v in inv]
    c = [int(v) for v in row[WP_COEF:WP_COEF + 9]]
    if min(c[6] * X + c[7] * Y + c[8] for X in (0, W) for Y in (0, H)) <= 0:
        raise ValueError("render_warp: the quadrilateral is not convex enough (den <= 0 at a corner of the canvas)")
    return row


def draw_render_warp(words, n_fonts, rng, n=1, fx=(), warp=()):
    """draw_render_fx plus the warp rows: -> (labels, classes, lengths, params, fx (n, 20), warp (n, 16) int64).  warp: a RenderWarp,
    or () / None: no warp draw at all and rows of zeros -- the stream is then draw_render_fx's exactly.  Sample by sample: exactly
    the draws of draw_render_fx for ONE sample, then for every LISTED kind in the order perspective, rotate, curve one random() -- the
    kind is on where it is below prob -- followed at once, where the kind is on, by its parameters, every one (2 * random() - 1) * limit:
      perspective   dx, dy of the top left, top right, bottom right, bottom left corner (8 draws); limit = persp * gh, and never more
                    than a quarter of the bent flat canvas' side along that axis (the quadrilateral stays convex)
      rotate        the angle in degrees; limit = angle
      curve         amp = int(. * 65536) in Q16 pixels (truncated toward 0); limit = curve * gh
    A kind that is not listed makes no draw; one that is listed and off makes the one.  Only rng.random() is called here.  The row is
    warp_row's of the sample's flat canvas (layout) and these magnitudes; where warp_row refuses them (den <= 0 at a corner of the
    bounding box: a narrow word, strongly keystoned and turned) the jitter is halved, up to five times, and then dropped -- no draw
    is added."""
    n = int(n)
    out = ([], [], [], [], [])
    rows = np.zeros((max(n, 0), N_WARP), np.int64)
    if n < 1:
        draw_render_fx(words, n_fonts, rng, n, fx)          # (its ValueError)
    for i in range(n):
        one = draw_render_fx(words, n_fonts, rng, 1, fx)
        out[0].extend(one[0])
        for dst, src in zip(out[1:], one[1:]):
            dst.append(src)
        if not warp:
            continue
        p = one[3][0]
        gh, flags, units, turn, amp = int(p[GH]), 0, None, 0.0, 0
        if "perspective" in warp.kinds and rng.random() < warp.prob:
            flags |= 1
            units = [2.0 * rng.random() - 1.0 for _ in range(8)]
        if "rotate" in warp.kinds and rng.random() < warp.prob:
            flags |= 2
            turn = (2.0 * rng.random() - 1.0) * warp.angle
        if "curve" in warp.kinds and rng.random() < warp.prob:
            flags |= 4
            amp = int((2.0 * rng.random() - 1.0) * warp.curve * gh * 65536.0)
        if flags:
            h0, w0 = layout(one[1][0, :one[2][0]].tolist(), p, warp.atlases)[:2]
            jitter = None
            if units:
                lx, ly = min(warp.persp * gh, w0 / 4.0), min(warp.persp * gh, (h0 + ((abs(amp) + 65535) >> 16)) / 4.0)
                jitter = [(units[2 * k] * lx, units[2 * k + 1] * ly) for k in range(4)]
            for _ in range(6):          # den > 0 is asked on the whole bounding box, which a turned narrow word can push past the horizon
                try:
                    rows[i] = warp_row(h0, w0, flags, amp, turn, jitter)
                    break
                except ValueError:
                    jitter = [(dx / 2.0, dy / 2.0) for dx, dy in jitter]
            else:
                rows[i] = warp_row(h0, w0, flags & 6, amp, turn) if flags & 6 else 0
    return (out[0],) + tuple(np.concatenate(a) for a in out[1:]) + (rows,)


def check_render_warp(warp, params, n=None):
    """ValueError for a warp row outside its domain (what the kernel's entry point rejects too); params: the samples' params rows (the
    range of amp follows gh).  A row with flags 0 is not read; of the others: the spare columns are 0, no coefficient passes COEF_MAX
    (the bound that keeps every intermediate below 2^62), the canvas is 1 .. MAX_SIDE a side, den > 0 at its four corners, |amp| <=
    CURVE_MAX * gh and room = ceil(|amp|) with the curve bit, both 0 without it -> the rows as (n, 16) int64."""
    warp = np.ascontiguousarray(warp, np.int64)
    params = np.ascontiguousarray(params, np.int64)
    if (warp.ndim != 2 or warp.shape[1] != N_WARP or warp.shape[0] < 1 or (n is not None and warp.shape[0] != n)
            or params.shape != (warp.shape[0], N_PARAMS)):
        raise ValueError("render_warp: warp (n, %d) with one row per sample and params (n, %d) expected, got %s %s"
                         % (N_WARP, N_PARAMS, warp.shape, params.shape))
    fl = warp[:, WP_FLAGS]
    if fl.min() < 0 or fl.max() > 7:
        raise ValueError("render_warp: flags outside 0 .. 7")
    on = fl != 0
    r, gh = warp[on], params[on, GH]
    if not r.size:
        return warp
    if r[:, WP_W + 1:].any():
        raise ValueError("render_warp: a spare column that is not 0")
    c = r[:, WP_COEF:WP_COEF + 9]
    if np.abs(c).max() > COEF_MAX:
        raise ValueError("render_warp: a coefficient of the map passes 2^30 (an intermediate could pass 2^62)")
    H, W = r[:, WP_H], r[:, WP_W]
    if min(H.min(), W.min()) < 1 or max(H.max(), W.max()) > MAX_SIDE:
        raise ValueError("render_warp: a canvas side outside 1 .. %d" % MAX_SIDE)
    for X in (0, W):
        for Y in (0, H):
            if (c[:, 6] * X + c[:, 7] * Y + c[:, 8] <= 0).any():
                raise ValueError("render_warp: den <= 0 at a corner of the output canvas (the map folds the canvas over)")
    amp, room, curve = r[:, WP_AMP], r[:, WP_ROOM], (r[:, WP_FLAGS] & 4) != 0
    if (np.abs(amp) * 10 > int(CURVE_MAX * 10) * 65536 * gh).any() or (room != ((np.abs(amp) + 65535) >> 16)).any() or amp[~curve].any():
        raise ValueError("render_warp: amp outside its range (|amp| <= %g gh in Q16 with the curve bit, 0 without it), or room is not "
                         "ceil(|amp|)" % CURVE_MAX)
    return warp


def render_warp_meta(classes, lengths, params, warp, atlases):
    """render_meta for warped samples: (n, 3) int64 of (byte offset, h, w) -- a sample with flags 0 has layout's canvas, any other
    the H x W of its row."""
    meta = render_meta(classes, lengths, params, atlases)
    warp = check_render_warp(warp, params, n=meta.shape[0])
    on = warp[:, WP_FLAGS] != 0
    meta[on, 1], meta[on, 2] = warp[on, WP_H], warp[on, WP_W]
    sizes = meta[:, 1] * meta[:, 2] * 3
    meta[:, 0] = np.cumsum(sizes) - sizes
    return meta


def _warp_sample(pos, A, gh, limit):
    """Atlas coordinates of the Q16 positions pos along one axis: _axis_sample at a fractional index."""
    q = np.maximum(((pos * ((A << 16) // gh)) >> 16) - 32768, 0)
    i0 = np.minimum(q >> 16, limit)
    return i0, np.minimum(i0 + 1, limit), q & 0xFFFF


def _alpha_plane_warp(cls, row, wr, atlases):
    """The alpha plane (H, W) int64 of a warped sample (the comment above states every formula); flags 0: _alpha_plane."""
    if not int(wr[WP_FLAGS]):
        return _alpha_plane(cls, row, atlases)
    f, gh, s, top = int(row[FONT]), int(row[GH]), int(row[SHEAR]), int(row[M_TOP])
    A = int(atlases.height[f])
    h0, w0, pens, advs, planes, room_s, x0 = layout(cls, row, atlases)
    n = len(cls)
    tw = max(pens[n] - int(row[SPACING]), 1)
    H, W, amp, room = int(wr[WP_H]), int(wr[WP_W]), int(wr[WP_AMP]), int(wr[WP_ROOM])
    c = [int(v) for v in wr[WP_COEF:WP_COEF + 9]]
    Y, X = 2 * np.arange(H, dtype=np.int64)[:, None] + 1, 2 * np.arange(W, dtype=np.int64)[None, :] + 1
    den = c[6] * X + c[7] * Y + 2 * c[8]
    px, py = ((c[0] * X + c[1] * Y + 2 * c[2]) * 65536) // den, ((c[3] * X + c[4] * Y + 2 * c[5]) * 65536) // den
    ok = (px >= 0) & (px < (w0 << 16))
    px = np.where(ok, px, 0)
    xq, Wq = px >> 12, w0 << 4
    vq = py - ((room << 16) if amp < 0 else 0) - (amp * 4 * xq * (Wq - xq)) // (Wq * Wq) - (top << 16)
    ok &= (vq >= 0) & (vq < (gh << 16))
    vq = np.where(ok, vq, 0)
    uq = px - ((s * (((gh - 1) << 16) + 32768 - vq)) >> 16) - (x0 << 16)
    ok &= (uq >= 0) & (uq < (tw << 16))
    uq = np.where(ok, uq, 0)
    pens_a = np.asarray(pens[:n], np.int64)
    k = np.clip(np.searchsorted(pens_a, uq >> 16, side="right") - 1, 0, n - 1)
    ugq = uq - (pens_a[k] << 16)
    ok &= ugq < (np.asarray(advs, np.int64)[k] << 16)
    ugq = np.where(ok, ugq, 0)
    pk, ck = np.asarray(planes)[k], np.asarray(cls)[k]
    cell_w = atlases.advance[f][pk, ck].astype(np.int64)
    x_0, x_1, fx = _warp_sample(ugq, A, gh, np.maximum(cell_w - 1, 0))
    y_0, y_1, fy = _warp_sample(vq, A, gh, A - 1)
    at = atlases.alpha[f].astype(np.int64)
    t = at[pk, ck, y_0, x_0] * (65536 - fx) + at[pk, ck, y_0, x_1] * fx
    b = at[pk, ck, y_1, x_0] * (65536 - fx) + at[pk, ck, y_1, x_1] * fx
    return np.where(ok, (t * (65536 - fy) + b * fy + (1 << 31)) >> 32, 0)


def render_warp_u8(word_classes_, params_row, fx_row, warp_row_, atlases, pool=None):
    """One sample -> its (H, W, 3) uint8 image with the warped text (the comment above) under the stages of render_fx_u8:
    word_classes_, params_row, fx_row and pool as render_fx_u8 takes them, warp_row_ one row of draw_render_warp.  A warp row with
    flags 0 gives render_fx_u8's image byte for byte, with an fx row of zeros also render_u8's."""
    cls = [int(c) for c in word_classes_]
    row = np.asarray(params_row, np.int64)
    if not 1 <= len(cls) <= MAX_LEN:
        raise ValueError("render: a word has a length outside 1 .. %d" % MAX_LEN)
    check_render(np.pad(np.asarray(cls, np.int32), (0, MAX_LEN - len(cls)))[None], [len(cls)], row[None], atlases)
    fxr = check_render_fx(np.asarray(fx_row, np.int64)[None], pool)[0]
    wr = check_render_warp(np.asarray(warp_row_, np.int64)[None], row[None])[0]
    return _render_fx(cls, row, fxr, atlases, pool, alpha=_alpha_plane_warp(cls, row, wr, atlases))
