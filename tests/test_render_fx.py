"""Outline, drop shadow and photo backgrounds of the word renderer on the CPU (utils/render.py draw_render_fx / check_render_fx /
render_fx_u8, main.py --train_words_fx): flags 0 against render_u8, the outline against scipy's grey dilation, the shadow against a
shifted plane, the texture against the crop's own bytes, the draws against a replay of their documented order, the flag checks and the
--train_state fingerprint."""
import importlib.util
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

from dpmn_amd.utils import render as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ["hello", "World", "a", "x" * 25, "it's", "42nd"]
_MADE = {}


def _atlases():
    """PIL's built-in font at the base heights 64 and 40 as two atlases: made once, never changed"""
    if "at" not in _MADE:
        _MADE["at"] = rd.build_atlases(None, [64, 40])
    return _MADE["at"]


def _pool():
    """three photos: noise 40 x 300, noise 9 x 13 and one single pixel; made once, never changed"""
    if "pool" not in _MADE:
        rng = np.random.RandomState(5)
        _MADE["pool"] = rd.Backgrounds([rng.randint(0, 256, (40, 300, 3)).astype(np.uint8), rng.randint(0, 256, (9, 13, 3)).astype(np.uint8),
                                        np.full((1, 1, 3), (7, 200, 90), np.uint8)])
    return _MADE["pool"]


def _row(font, gh, fg=(200, 30, 90), bg=(10, 220, 130), **kw):
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.FONT], row[rd.GH] = font, gh
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3] = fg, bg
    for k, v in kw.items():
        row[getattr(rd, k)] = v
    return row


def _fx(**kw):
    row = np.zeros(rd.N_FX, np.int64)
    for k, v in kw.items():
        c = getattr(rd, "FX_" + k)
        row[c:c + np.size(v)] = v
    return row


# ------------------------------------------------------------------------------------------------------------------------- flags 0
def test_flags_zero_is_render_u8_byte_for_byte():
    """the rows of tests/test_render.py, and a few drawn ones"""
    at = _atlases()
    cases = []
    for font, gh in ((0, 64), (1, 40)):
        for ch, case in (("g", 0), ("Q", 1), ("7", 0)):
            for seed in (0, 2 ** 63 - 1):
                cases.append(([rd.DICT36.index(ch.lower()) + 1], _row(font, gh, CASE=case, SEED=seed)))
    for word, case in (("hello42", 0), ("WAVE", 1), ("Type", 2)):
        cases.append((rd.word_classes(word), _row(1, 40, CASE=case, SEED=9)))
    row = _row(0, 32, M_LEFT=3, M_RIGHT=5, M_TOP=4, M_BOTTOM=2, SPACING=4, SHEAR=-19660, STYLE=2, SEED=1)
    row[rd.BG2:rd.BG2 + 3] = (250, 0, 40)
    cases.append((rd.word_classes("ab"), row))
    _, cls, lens, params = rd.draw_render(WORDS, 2, random.Random(4), n=6)
    cases += [(cls[i, :lens[i]].tolist(), params[i]) for i in range(6)]
    zero = np.zeros(rd.N_FX, np.int64)
    for c, r in cases:
        assert np.array_equal(rd.render_fx_u8(c, r, zero, at), rd.render_u8(c, r, at))
        # the columns of a kind whose bit is 0 are not read
        assert np.array_equal(rd.render_fx_u8(c, r, _fx(R=3, OUTLINE=(1, 2, 3), DX=2, Q=200, PHOTO=1, M=100), at), rd.render_u8(c, r, at))
        assert np.array_equal(rd._alpha_plane(c, r, at).shape, rd.layout(c, r, at)[:2])


def _alpha_from_image(cls, row, at):
    """The alpha plane out of render_u8 itself: white on black, at the pixels where the grain is removed exactly -- a black
    background with a grain <= 0 clips to 0, and white over 0 is the alpha; the other pixels are -1."""
    row = row.copy()
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3], row[rd.STYLE] = 255, 0, 0
    img = rd.render_u8(cls, row, at).astype(np.int64)
    h, w = img.shape[:2]
    return np.where(rd.grain(row[rd.SEED], h * w).reshape(h, w) <= 0, img[:, :, 0], -1)


def test_alpha_plane_is_the_plane_render_u8_blends():
    at = _atlases()
    for c, r in ((rd.word_classes("Wave"), _row(0, 48, CASE=2, M_LEFT=2, M_TOP=1, M_BOTTOM=3, SHEAR=15000, SPACING=-1, SEED=3)),
                 (rd.word_classes("q7"), _row(1, 30, SEED=8))):
        want, got = _alpha_from_image(c, r, at), rd._alpha_plane(c, r, at)
        assert (want >= 0).mean() > 0.4 and np.array_equal(got[want >= 0], want[want >= 0]) and got.max() == 255 and got.min() == 0


# ------------------------------------------------------------------------------------------------------------------------- outline
def _disk(r):
    j, i = np.mgrid[-r:r + 1, -r:r + 1]
    return i * i + j * j <= r * r


@pytest.mark.parametrize("r", [1, 2, 3])
def test_outline_is_the_grey_dilation_by_a_disk(r):
    """White fill and white outline on a black flat background, zero grain.  The outline's plane a_o is scipy's grey dilation of the
    alpha plane by the disk, zero outside the canvas; the fill is blended over it, so the image's plane is
    (255 alpha + a_o (255 - alpha) + 127) // 255 -- the dilation itself wherever alpha is 0 or 255 or the dilation is 255, and not on
    an anti-aliased glyph edge, where the fill's own blend comes on top (the formulas of the fill in utils/render.py)."""
    from scipy import ndimage
    at = _atlases()
    assert int(_disk(r).sum()) == {1: 5, 2: 13, 3: 29}[r]
    for cls, row in ((rd.word_classes("Wave"), _row(0, 48, (255,) * 3, (0,) * 3, CASE=2, M_LEFT=2, M_TOP=1, M_BOTTOM=3, SHEAR=15000, SPACING=-1)),
                     (rd.word_classes("i"), _row(0, 24, (255,) * 3, (0,) * 3)),                     # no margin: clipped on every side
                     (rd.word_classes("q7"), _row(1, 30, (255,) * 3, (0,) * 3, M_RIGHT=7, M_BOTTOM=1, SHEAR=-rd.SHEAR_MAX))):
        alpha = rd._alpha_plane(cls, row, at)
        want = ndimage.grey_dilation(alpha, footprint=_disk(r), mode="constant", cval=0)
        fxr = _fx(FLAGS=1, R=r, OUTLINE=(255,) * 3)
        assert np.array_equal(rd._fx_planes(alpha, fxr)[1], want)
        img = rd._render_fx(cls, row, fxr, at, None, grain_plane=np.zeros(alpha.shape, np.int64)).astype(np.int64)
        assert np.array_equal(img[:, :, 0], img[:, :, 1]) and np.array_equal(img[:, :, 0], img[:, :, 2])
        assert np.array_equal(img[:, :, 0], (255 * alpha + want * (255 - alpha) + 127) // 255)
        exact = (alpha == 0) | (alpha == 255) | (want == 255)
        assert exact.mean() > 0.5 and np.array_equal(img[:, :, 0][exact], want[exact]) and (want > alpha).any()
        # through the checked entry, with the row's own grain: the same image at the pixels where the grain is removed exactly
        pub = rd.render_fx_u8(cls, row, fxr, at).astype(np.int64)
        calm = rd.grain(row[rd.SEED], alpha.size).reshape(alpha.shape) <= 0
        assert np.array_equal(pub[calm], img[calm])


# -------------------------------------------------------------------------------------------------------------------------- shadow
@pytest.mark.parametrize("dx,dy", [(3, 2), (-3, 2), (3, -2), (-3, -2), (0, 1), (-1, 0)])
def test_shadow_is_the_shifted_plane_scaled_by_q(dx, dy):
    """black background, white shadow, zero grain: the shadow's plane is the alpha plane moved by (dx, dy) with zero fill, times q;
    the image shows it wherever the fill's alpha is 0, and the fill over it elsewhere"""
    at = _atlases()
    cls, row = rd.word_classes("Type"), _row(0, 40, (200, 30, 90), (0,) * 3, CASE=2, M_LEFT=1, M_BOTTOM=2, SHEAR=9000)
    alpha = rd._alpha_plane(cls, row, at)
    h, w = alpha.shape
    for q in (96, 255):
        moved = np.pad(alpha, 3)[3 - dy:3 - dy + h, 3 - dx:3 - dx + w]          # moved[y, x] = alpha[y - dy, x - dx], 0 from outside
        want = (moved * q + 127) // 255
        fxr = _fx(FLAGS=2, DX=dx, DY=dy, Q=q, SHADOW=(255,) * 3)
        assert np.array_equal(rd._fx_planes(alpha, fxr)[0], want) and want.max() == q
        img = rd._render_fx(cls, row, fxr, at, None, grain_plane=np.zeros((h, w), np.int64)).astype(np.int64)
        assert np.array_equal(img[alpha == 0], np.repeat(want[alpha == 0][:, None], 3, axis=1)) and (want[alpha == 0] > 0).any()
        fg = row[rd.FG:rd.FG + 3][None, None, :]
        assert np.array_equal(img, (fg * alpha[:, :, None] + want[:, :, None] * (255 - alpha[:, :, None]) + 127) // 255)


def test_shadow_lies_under_the_outline_and_the_outline_under_the_fill():
    at = _atlases()
    cls, row = rd.word_classes("o"), _row(0, 64, (255, 0, 0), (0, 0, 0), M_LEFT=6, M_RIGHT=6, M_TOP=6, M_BOTTOM=6)
    alpha = rd._alpha_plane(cls, row, at)

    def over(colour, a, c):
        return (np.asarray(colour)[None, None, :] * a[:, :, None] + c * (255 - a[:, :, None]) + 127) // 255

    seen = set()
    for r in (1, 3):
        fxr = _fx(FLAGS=3, R=r, OUTLINE=(0, 255, 0), DX=3, DY=3, Q=255, SHADOW=(0, 0, 255))
        a_s, a_o = rd._fx_planes(alpha, fxr)
        img = rd._render_fx(cls, row, fxr, at, None, grain_plane=np.zeros(alpha.shape, np.int64))
        want = over((255, 0, 0), alpha, over((0, 255, 0), a_o, over((0, 0, 255), a_s, np.zeros(alpha.shape + (3,), np.int64))))
        assert np.array_equal(img, want) and (img[alpha == 255] == (255, 0, 0)).all()
        assert (img[(alpha == 0) & (a_o == 255)] == (0, 255, 0)).all()
        assert (img[(alpha == 0) & (a_o == 0) & (a_s == 255)] == (0, 0, 255)).all()
        seen |= {tuple(p) for p in img.reshape(-1, 3)}
    assert {(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0)} <= seen


# ------------------------------------------------------------------------------------------------------------------------- texture
def test_texture_reproduces_the_crop_and_a_single_pixel_is_flat():
    at, pool = _atlases(), _pool()
    cls = [0, 0, 0]                                                   # three blanks: the canvas is background alone
    row = _row(0, 24, M_LEFT=1, M_TOP=2, STYLE=1, SEED=77)
    h, w = rd.layout(cls, row, at)[:2]
    assert rd._alpha_plane(cls, row, at).max() == 0 and h <= 40 - 3 and w <= 300 - 5
    zero = np.zeros((h, w), np.int64)
    # cw = w, ch = h: every pixel centre falls on a photo pixel; m = 256 (outside the drawn range, through the internal call only)
    for x0, y0 in ((0, 0), (5, 3), (300 - w, 40 - h)):
        fxr = _fx(FLAGS=4, PHOTO=0, X0=x0, Y0=y0, CW=w, CH=h, M=256)
        assert np.array_equal(rd._render_fx(cls, row, fxr, at, pool, grain_plane=zero), pool.photo(0)[y0:y0 + h, x0:x0 + w])
        with pytest.raises(ValueError, match="blend weight"):
            rd.render_fx_u8(cls, row, fxr, at, pool)
    # the single pixel: flat at m = 256, and at a drawn weight the documented pull toward the gradient, then the row's grain
    flat = rd._render_fx(cls, row, _fx(FLAGS=4, PHOTO=2, CW=1, CH=1, M=256), at, pool, grain_plane=zero)
    assert (flat == (7, 200, 90)).all()
    for m in (rd.M_MIN, 150, rd.M_MAX):
        fxr = _fx(FLAGS=4, PHOTO=2, CW=1, CH=1, M=m)
        plain = rd._render_fx(cls, row, np.zeros(rd.N_FX, np.int64), at, None, grain_plane=zero).astype(np.int64)
        want = (np.asarray((7, 200, 90)) * m + plain * (256 - m) + 128) >> 8
        assert np.array_equal(rd._render_fx(cls, row, fxr, at, pool, grain_plane=zero), want)
        g = rd.grain(77, h * w).reshape(h, w, 1)
        assert np.array_equal(rd.render_fx_u8(cls, row, fxr, at, pool), np.clip(want + g, 0, 255))
    # a crop half and twice the canvas: the bilinear sample stays between the crop's extremes and inside it
    for cw, ch in ((w // 2, h // 2), (min(2 * w, 300), 40)):
        fxr = _fx(FLAGS=4, PHOTO=0, X0=1, Y0=0, CW=cw, CH=ch, M=256)
        img = rd._render_fx(cls, row, fxr, at, pool, grain_plane=zero)
        crop = pool.photo(0)[0:ch, 1:1 + cw]
        assert img.min() >= crop.min() and img.max() <= crop.max() and np.array_equal(img[0, 0], crop[0, 0]) == (cw <= w)


# --------------------------------------------------------------------------------------------------------------------------- draws
def _replay(rng, kinds, prob, fg, h, w, pool):
    """The fx draws of one sample in their documented order, written down a second time -> the row."""
    def below(k):
        return min(int(rng.random() * k), k - 1)

    row = np.zeros(rd.N_FX, np.int64)
    if "outline" in kinds and rng.random() < prob:
        row[0] |= 1
        row[1] = 1 + below(3)
        while True:
            col = [below(256), below(256), below(256)]
            if abs(rd.luma(col) - rd.luma(fg)) >= rd.MIN_CONTRAST:
                break
        row[2:5] = col
    if "shadow" in kinds and rng.random() < prob:
        row[0] |= 2
        while True:
            dx, dy = below(7) - 3, below(7) - 3
            if (dx, dy) != (0, 0):
                break
        row[5], row[6], row[7] = dx, dy, 96 + below(160)
        row[8:11] = [below(256), below(256), below(256)]
    if "texture" in kinds and rng.random() < prob:
        row[0] |= 4
        row[11] = below(pool.n_photos)
        ph, pw = pool.table[row[11], 1:]
        lo = max(1, w // 2)
        row[14] = min(lo + below(2 * w - lo + 1), pw)
        row[15] = min(max(1, row[14] * h // w), ph)
        row[12], row[13] = below(pw - row[14] + 1), below(ph - row[15] + 1)
        row[16] = 64 + below(161)
    return row


def test_without_fx_the_stream_moves_as_draw_render_moves_it():
    for n in (1, 7):
        a, b = random.Random(12), random.Random(12)
        want = rd.draw_render(WORDS, 2, a, n=n)
        got = rd.draw_render_fx(WORDS, 2, b, n, ())
        assert a.getstate() == b.getstate() and got[0] == want[0] and all(np.array_equal(x, y) for x, y in zip(got[1:4], want[1:]))
        assert got[4].shape == (n, rd.N_FX) and got[4].dtype == np.int64 and not got[4].any()
        c = random.Random(12)
        assert not rd.draw_render_fx(WORDS, 2, c, n, None)[4].any() and c.getstate() == a.getstate()
    with pytest.raises(ValueError):
        rd.draw_render_fx([], 2, random.Random(1), 1, ())
    with pytest.raises(ValueError):
        rd.draw_render_fx(WORDS, 2, random.Random(1), 0, ())


@pytest.mark.parametrize("kinds,prob", [(("outline",), 1.0), (("shadow",), 1.0), (("texture",), 1.0), (("shadow", "outline"), 0.5),
                                        (("texture", "shadow", "outline"), 0.5), (("outline", "shadow", "texture"), 0.0)])
def test_draws_follow_the_documented_order_and_unlisted_kinds_draw_nothing(kinds, prob):
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(kinds, prob, pool if "texture" in kinds else None, at)
    assert fx.kinds == tuple(k for k in rd.FX_KINDS if k in kinds)
    a, b = random.Random(31), random.Random(31)
    state = a.getstate()
    labels, cls, lens, params, rows = rd.draw_render_fx(WORDS, 2, a, 40, fx)
    for i in range(40):
        l, c, n, p = rd.draw_render(WORDS, 2, b, 1)              # exactly draw_render's draws of one sample, then the fx draws
        assert l[0] == labels[i] and np.array_equal(c[0], cls[i]) and n[0] == lens[i] and np.array_equal(p[0], params[i])
        h, w = rd.layout(c[0, :n[0]].tolist(), p[0], at)[:2]
        assert np.array_equal(rows[i], _replay(b, kinds, prob, p[0, rd.FG:rd.FG + 3], h, w, pool)), i
    assert a.getstate() == b.getstate()
    bits = sum(1 << rd.FX_KINDS.index(k) for k in kinds)
    assert not (rows[:, 0] & ~bits).any() and (prob > 0 or not rows.any()) and (prob < 1 or (rows[:, 0] == bits).all())
    rd.check_render_fx(rows, pool)
    # the restored stream gives the rows again
    a.setstate(state)
    again = rd.draw_render_fx(WORDS, 2, a, 40, fx)
    assert again[0] == labels and np.array_equal(again[4], rows) and np.array_equal(again[3], params)


def test_drawn_rows_reach_their_ranges_and_stay_inside_them():
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(rd.FX_KINDS, 1.0, pool, at)
    _, cls, lens, params, rows = rd.draw_render_fx(WORDS, 2, random.Random(2), 400, fx)
    assert (rows[:, rd.FX_FLAGS] == 7).all() and not rows[:, 17:].any()
    assert set(rows[:, rd.FX_R]) == {1, 2, 3} and set(rows[:, rd.FX_DX]) == set(range(-3, 4)) == set(rows[:, rd.FX_DY])
    assert (rows[:, rd.FX_DX:rd.FX_DY + 1] != 0).any(axis=1).all()
    assert rows[:, rd.FX_Q].min() >= 96 and rows[:, rd.FX_Q].max() <= 255 and rows[:, rd.FX_Q].min() < 100 and rows[:, rd.FX_Q].max() > 250
    assert rows[:, rd.FX_M].min() >= 64 and rows[:, rd.FX_M].max() <= 224 and rows[:, rd.FX_M].min() < 68 and rows[:, rd.FX_M].max() > 220
    assert all(abs(rd.luma(r[rd.FX_OUTLINE:rd.FX_OUTLINE + 3]) - rd.luma(p[rd.FG:rd.FG + 3])) >= rd.MIN_CONTRAST for r, p in zip(rows, params))
    assert set(rows[:, rd.FX_PHOTO]) == {0, 1, 2}
    meta = rd.render_meta(cls, lens, params, at)
    ph, pw = pool.table[rows[:, rd.FX_PHOTO], 1], pool.table[rows[:, rd.FX_PHOTO], 2]
    cw, ch, h, w = rows[:, rd.FX_CW], rows[:, rd.FX_CH], meta[:, 1], meta[:, 2]
    assert (cw >= 1).all() and (cw <= np.minimum(2 * w, pw)).all() and ((cw >= np.maximum(1, w // 2)) | (cw == pw)).all()
    assert np.array_equal(ch, np.minimum(np.maximum(1, cw * h // w), ph))
    assert (rows[:, rd.FX_X0] >= 0).all() and (rows[:, rd.FX_X0] + cw <= pw).all() and (rows[:, rd.FX_Y0] >= 0).all() and (rows[:, rd.FX_Y0] + ch <= ph).all()
    assert (rows[:, rd.FX_X0] + cw == pw).any() and (rows[:, rd.FX_X0] > 0).any()
    # every drawn sample renders, at render_meta's size
    for i in range(0, 400, 50):
        assert rd.render_fx_u8(cls[i, :lens[i]], params[i], rows[i], at, pool).shape == (h[i], w[i], 3)


def test_rows_outside_their_domain_are_refused():
    pool = _pool()
    good = _fx(FLAGS=7, R=2, OUTLINE=(1, 2, 3), DX=-3, DY=0, Q=96, SHADOW=(255, 0, 9), PHOTO=1, X0=3, Y0=2, CW=10, CH=7, M=64)
    assert np.array_equal(rd.check_render_fx(good[None], pool), good[None])
    for col, val, msg in ((rd.FX_FLAGS, 8, "flags"), (rd.FX_FLAGS, -1, "flags"), (17, 1, "spare"), (rd.FX_R, 0, "outline"), (rd.FX_R, 4, "outline"),
                          (rd.FX_OUTLINE + 1, 256, "outline"), (rd.FX_DX, 4, "shadow"), (rd.FX_DX, 0, "shadow"), (rd.FX_DY, -4, "shadow"),
                          (rd.FX_Q, 95, "shadow"), (rd.FX_Q, 256, "shadow"), (rd.FX_SHADOW, -1, "shadow"), (rd.FX_PHOTO, 3, "photo"),
                          (rd.FX_PHOTO, -1, "photo"), (rd.FX_X0, 4, "crop"), (rd.FX_Y0, 3, "crop"), (rd.FX_X0, -1, "crop"), (rd.FX_CW, 0, "crop"),
                          (rd.FX_CH, 8, "crop"), (rd.FX_M, 63, "blend"), (rd.FX_M, 225, "blend")):
        bad = good.copy()
        bad[col] = val
        with pytest.raises(ValueError, match=msg):
            rd.check_render_fx(bad[None], pool)
    with pytest.raises(ValueError, match="no pool"):
        rd.check_render_fx(good[None], None)
    with pytest.raises(ValueError, match="one row per sample"):
        rd.check_render_fx(good[None], pool, n=2)
    with pytest.raises(ValueError):
        rd.check_render_fx(np.zeros((1, 19), np.int64))
    with pytest.raises(ValueError, match="distinct kinds"):
        rd.RenderFx(["outline", "glow"])
    with pytest.raises(ValueError, match="distinct kinds"):
        rd.RenderFx(["outline", "outline"])
    with pytest.raises(ValueError, match="go together"):
        rd.RenderFx(["texture"])
    with pytest.raises(ValueError, match="go together"):
        rd.RenderFx(["shadow"], 0.5, pool, _atlases())
    with pytest.raises(ValueError, match="probability"):
        rd.RenderFx(["shadow"], float("nan"))


# ------------------------------------------------------------------------------------------------------------ pool, flags, fingerprint
def _photo_dir(tmp_path):
    from PIL import Image
    d = tmp_path / "photos"
    d.mkdir()
    rng = np.random.RandomState(1)
    Image.fromarray(rng.randint(0, 256, (300, 600, 3)).astype(np.uint8)).save(str(d / "b_wide.png"))
    Image.fromarray(rng.randint(0, 256, (20, 30)).astype(np.uint8)).save(str(d / "a_grey.png"))
    (d / "c_notes.txt").write_text("not an image")
    (d / "sub").mkdir()
    return d


def test_load_backgrounds(tmp_path, capsys):
    from PIL import Image
    d = _photo_dir(tmp_path)
    pool = rd.load_backgrounds(str(d))
    assert "2 background photos" in capsys.readouterr().out
    assert pool.n_photos == 2 and pool.table.dtype == np.int64 and pool.table.tolist() == [[0, 20, 30], [20 * 30 * 3, 256, 512]]
    assert pool.pixels.dtype == np.uint8 and pool.pixels.shape == (20 * 30 * 3 + 256 * 512 * 3,)
    grey = np.asarray(Image.open(str(d / "a_grey.png")).convert("RGB"))
    assert np.array_equal(pool.photo(0), grey)
    big = Image.open(str(d / "b_wide.png")).convert("RGB")
    big.thumbnail((512, 512), Image.BICUBIC)
    assert np.array_equal(pool.photo(1), np.asarray(big))
    import zlib
    assert pool.crc32 == zlib.crc32(pool.pixels.tobytes()) & 0xFFFFFFFF
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "x.txt").write_text("nothing")
    with pytest.raises(ValueError, match="holds no image"):
        rd.load_backgrounds(str(empty))


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_render_fx", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_flag_checks_exit_with_one_clear_line(tmp_path):
    m = _main()
    f = tmp_path / "words.txt"
    f.write_text("word\n")
    d = _photo_dir(tmp_path)
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "x.txt").write_text("nothing")
    w = str(f)
    for args, msg in ((dict(train_words_fx="outline"), "need --train_words"),
                      (dict(train_words_backgrounds=str(d)), "need --train_words"),
                      (dict(train_words=w, train_words_fx="outline,glow"), "distinct kinds of outline, shadow, texture"),
                      (dict(train_words=w, train_words_fx="texture"), "go together"),
                      (dict(train_words=w, train_words_fx="outline", train_words_backgrounds=str(d)), "go together"),
                      (dict(train_words=w, train_words_backgrounds=str(d)), "needs --train_words_fx texture"),
                      (dict(train_words=w, train_words_fx="shadow", train_words_fx_prob=1.5), "probability in 0 .. 1"),
                      (dict(train_words=w, train_words_fx="shadow", train_words_fx_prob=-0.1), "probability in 0 .. 1"),
                      (dict(train_words=w, train_words_fx="texture", train_words_backgrounds=str(tmp_path / "nodir")), "is not a directory"),
                      (dict(train_words=w, train_words_fx="texture", train_words_backgrounds=str(empty)), "holds no image that PIL can open")):
        with pytest.raises(SystemExit, match=msg) as e:
            m.main(SimpleNamespace(), SimpleNamespace(**args))
        assert str(e.value).startswith("main.py: ") and "\n" not in str(e.value)
    src = m.train_words_source(SimpleNamespace(train_words=w, train_words_fx="texture, outline", train_words_fx_prob=0.25,
                                               train_words_backgrounds=str(d)), "upper")
    assert src[0] == ["word"] and src[2] == rd.DEFAULT_EPOCH
    fx = src[3]
    assert fx.kinds == ("outline", "texture") and fx.prob == 0.25 and fx.pool.n_photos == 2 and fx.atlases is src[1]
    assert m.train_words_source(SimpleNamespace(train_words=w), "upper")[3] is None
    assert m.train_words_source(SimpleNamespace(train_words=w, train_words_fx="shadow"), "upper")[3].prob == 0.5
    assert m.train_words_fx(SimpleNamespace()) is None


def test_fingerprint_carries_the_fx_setting(tmp_path):
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))
    args = SimpleNamespace(arch="tatt", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="4,", embed_dim="96,",
                           depths="1,", num_heads="6,", window_size="2,4,8,", mlp_ratio="4,", train_words="words.txt")
    at, pool = _atlases(), _pool()
    plain = rd.words_setting(WORDS, at, 100)
    assert plain == rd.words_setting(WORDS, at, 100, None) == rd.words_setting(WORDS, at, 100, ()) and sorted(plain) == ["crc32", "epoch", "fonts"]
    fx = rd.RenderFx(("shadow", "texture"), 0.5, pool, at)
    setting = rd.words_setting(WORDS, at, 100, fx)
    assert {k: setting[k] for k in plain} == plain
    assert setting["fx_kinds"] == ["shadow", "texture"] and setting["fx_prob"] == 0.5 and setting["fx_pool"] == pool.crc32
    assert rd.words_setting(WORDS, at, 100, rd.RenderFx(("outline",)))["fx_pool"] is None
    off, on = base.state_fingerprint(args, cfg, train_words=plain), base.state_fingerprint(args, cfg, train_words=setting)
    base.check_fingerprint(off, off)                      # a state written without fx keeps loading without it
    base.check_fingerprint(on, base.state_fingerprint(args, cfg, train_words=rd.words_setting(list(WORDS), at, 100, fx)))
    path = str(tmp_path / "state.pt")
    base.write_train_state(path, {"version": base.TRAIN_STATE_VERSION, "fingerprint": on})
    assert base.read_train_state(path, on)["fingerprint"]["train_words"] == setting          # (survives the weights_only round trip)
    other_pool = rd.Backgrounds([np.zeros((2, 2, 3), np.uint8)])
    for other in (plain, rd.words_setting(WORDS, at, 100, rd.RenderFx(("shadow", "texture"), 0.25, pool, at)),
                  rd.words_setting(WORDS, at, 100, rd.RenderFx(("outline", "shadow", "texture"), 0.5, pool, at)),
                  rd.words_setting(WORDS, at, 100, rd.RenderFx(("shadow", "texture"), 0.5, other_pool, at))):
        with pytest.raises(ValueError, match="train_words"):
            base.read_train_state(path, base.state_fingerprint(args, cfg, train_words=other))
    with pytest.raises(ValueError, match="train_words"):
        base.check_fingerprint(off, on)


# ------------------------------------------------------------------------------------------------- sr_batches with stubbed device ops
def test_sr_batches_draws_and_renders_through_the_fx_path(monkeypatch):
    """a WordsHR loader whose collate carries a RenderFx: per batch the draws are draw_render_fx's from random.Random(pass key + j),
    before the degradation's, and the render goes to ops.render_words_fx_u8 with the pool; without render_fx the plain op is called"""
    import torch
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.words import WordsHR
    from dpmn_amd.utils.degrade import draw_params
    from dpmn_amd.utils.resize import pack_ragged, pil_resize_u8
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(rd.FX_KINDS, 0.5, pool, at)
    calls = {"fx": [], "plain": 0, "degrade": []}

    def render_fx(cls, lens, params, rows, atlases, pool_, device=None, out=None):
        calls["fx"].append((np.array(cls), np.array(lens), np.array(params), np.array(rows), pool_))
        return pack_ragged([rd.render_fx_u8(c[:n], p, r, atlases, pool_) for c, n, p, r in zip(cls, lens, params, rows)], pin=False)

    def render(cls, lens, params, atlases, device=None, out=None):
        calls["plain"] += 1
        return pack_ragged([rd.render_u8(c[:n], p, atlases) for c, n, p in zip(cls, lens, params)], pin=False)

    def degrade(packed, meta, params, z=None, seed=0):
        calls["degrade"].append((np.array(params), int(seed)))
        return packed.clone()

    def resize(packed, meta, H, W):
        flat = packed.numpy()
        return torch.from_numpy(np.stack([pil_resize_u8(flat[o:o + h * w * 3].reshape(h, w, 3), H, W) for o, h, w in np.asarray(meta).tolist()]))

    monkeypatch.setattr(ops, "render_words_fx_u8", render_fx)
    monkeypatch.setattr(ops, "render_words_u8", render)
    monkeypatch.setattr(ops, "degrade_ragged_u8", degrade)
    monkeypatch.setattr(ops, "resize_ragged_u8", resize)
    monkeypatch.setattr(ops, "collate_u8", lambda img, mask: img.permute(0, 3, 1, 2).float() / 255.0)
    kw = dict(imgH=32, imgW=128, down_sample_scale=2, mask=False, gpu_finish=True, gpu_resize=True, degrade=True, cutblur=True)
    with pytest.raises(ValueError, match="render_fx needs render"):
        tz.alignCollate_realWTLAMask(render_fx=fx, **kw)
    col = tz.alignCollate_realWTLAMask(render=(WORDS, at), render_fx=fx, **kw)
    loader = torch.utils.data.DataLoader(WordsHR(WORDS, 6), batch_size=4, shuffle=False, collate_fn=col, num_workers=0)
    random.seed(3)
    state = random.getstate()
    got = list(tz.sr_batches(loader, torch.device("cpu")))
    assert [len(b[3]) for b in got] == [4, 2] and calls["plain"] == 0 and got[0][0].shape == (4, 3, 32, 128)
    random.setstate(state)
    key = random.getrandbits(63)
    for j, n in enumerate((4, 2)):
        rng = random.Random(key + j)
        want = rd.draw_render_fx(WORDS, 2, rng, n, fx)
        assert got[j][3] == want[0] and all(np.array_equal(x, y) for x, y in zip(calls["fx"][j][:4], want[1:])) and calls["fx"][j][4] is pool
        widths = rd.render_meta(*want[1:4], at)[:, 2]
        assert np.array_equal(calls["degrade"][j][0], draw_params(n, cutblur=True, hr_widths=widths.tolist(), rng=rng))
        assert calls["degrade"][j][1] == rng.getrandbits(63)
    assert any(c[3].any() for c in calls["fx"])
    plain = tz.alignCollate_realWTLAMask(render=(WORDS, at), **kw)
    assert plain.render_fx is None
    list(tz.sr_batches(torch.utils.data.DataLoader(WordsHR(WORDS, 4), batch_size=4, collate_fn=plain, num_workers=0), torch.device("cpu")))
    assert calls["plain"] == 1 and len(calls["fx"]) == 2
