"""Projective distortion, rotation and the curved baseline of the word renderer on the CPU (utils/render.py draw_render_warp / warp_row /
check_render_warp / render_warp_meta / render_warp_u8, main.py --train_words_warp): flags 0 against render_fx_u8 and render_u8, the
geometry of a solid text box against the forward-mapped quadrilateral in exact fractions and against the parabola, the draws against
draw_render_fx's stream, the domain checks, the --train_state fingerprint and the flag checks."""
import importlib.util
import math
import os
import random
from fractions import Fraction
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
    if "pool" not in _MADE:
        rng = np.random.RandomState(5)
        _MADE["pool"] = rd.Backgrounds([rng.randint(0, 256, (40, 300, 3)).astype(np.uint8), rng.randint(0, 256, (9, 13, 3)).astype(np.uint8)])
    return _MADE["pool"]


def _solid():
    """an atlas whose cells are all 255, base height 32, every advance 16: with zero spacing, margins and shear the text box of an
    n-letter word at gh 32 is the solid rectangle 32 x 16 n, the whole flat canvas"""
    if "solid" not in _MADE:
        _MADE["solid"] = rd.Atlases(np.full((1, 2, rd.N_GLYPH, 32, 16), 255, np.uint8), np.full((1, 2, rd.N_GLYPH), 16, np.int32), [32], ["solid"])
    return _MADE["solid"]


def _solid_row():
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.GH] = 32
    row[rd.FG:rd.FG + 3] = 255          # background 0 (+ grain up to 4): a byte is 255 exactly where alpha is 255
    return row


# ------------------------------------------------------------------------------------------------------------------------- flags 0
def test_flags_zero_is_render_fx_u8_and_render_u8_byte_for_byte():
    """sixteen samples in the style of tests/test_gpu_render_fx.py: drawn rows with all three fx kinds, then the same rows without fx"""
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(rd.FX_KINDS, 0.7, pool, at)
    _, cls, lens, params, rows = rd.draw_render_fx(WORDS, 2, random.Random(11), 16, fx)
    assert rows[:, 0].any()
    zero = np.zeros((16, rd.N_WARP), np.int64)
    assert np.array_equal(rd.render_warp_meta(cls, lens, params, zero, at), rd.render_meta(cls, lens, params, at))
    for i in range(16):
        c = cls[i, :lens[i]]
        assert np.array_equal(rd.render_warp_u8(c, params[i], rows[i], zero[i], at, pool), rd.render_fx_u8(c, params[i], rows[i], at, pool))
        assert np.array_equal(rd.render_warp_u8(c, params[i], np.zeros(rd.N_FX, np.int64), zero[i], at), rd.render_u8(c, params[i], at))


def test_the_fractional_path_lands_on_the_integer_path_under_the_identity():
    """a curve bit with amp 0 is the identity map through the FRACTIONAL path: without shear (whose fractional form is not floored to
    whole pixels) every byte is render_u8's"""
    at = _atlases()
    _, cls, lens, params = rd.draw_render(WORDS, 2, random.Random(4), n=8)
    for i in range(8):
        row, c = params[i].copy(), cls[i, :lens[i]].tolist()
        row[rd.SHEAR] = 0
        h0, w0 = rd.layout(c, row, at)[:2]
        wr = rd.warp_row(h0, w0, 4, 0)
        assert wr[rd.WP_H] == h0 and wr[rd.WP_W] == w0 and wr[rd.WP_COEF] == wr[rd.WP_COEF + 4] == wr[rd.WP_COEF + 8] == rd.COEF_MAX
        assert np.array_equal(rd.render_warp_u8(c, row, np.zeros(rd.N_FX, np.int64), wr, at), rd.render_u8(c, row, at))


# ------------------------------------------------------------------------------------------------------------------------ geometry
def _quad_exact(h0, w0, angle, jitter):
    """the forward-mapped corners in exact fractions (cos and sin: the floats' exact values), moved to the origin"""
    cx, cy = Fraction(w0, 2), Fraction(h0, 2)
    co, si = Fraction(math.cos(math.radians(angle))), Fraction(math.sin(math.radians(angle)))
    quad = []
    for k, (x, y) in enumerate(((0, 0), (w0, 0), (w0, h0), (0, h0))):
        qx, qy = cx + co * (x - cx) - si * (y - cy), cy + si * (x - cx) + co * (y - cy)
        if jitter is not None:
            qx, qy = qx + Fraction(jitter[k][0]), qy + Fraction(jitter[k][1])
        quad.append((qx, qy))
    x_min, y_min = min(q[0] for q in quad), min(q[1] for q in quad)
    return [(x - x_min, y - y_min) for x, y in quad]


def _dist2_to_segment(p, a, b):
    ab, ap = (b[0] - a[0], b[1] - a[1]), (p[0] - a[0], p[1] - a[1])
    t = max(Fraction(0), min(Fraction(1), (ap[0] * ab[0] + ap[1] * ab[1]) / (ab[0] * ab[0] + ab[1] * ab[1])))
    dx, dy = ap[0] - t * ab[0], ap[1] - t * ab[1]
    return dx * dx + dy * dy


JITTER = [(3.5, -2.25), (-4.0, 3.0), (2.0, 4.5), (-3.0, -4.0)]


@pytest.mark.parametrize("flags, angle, jitter", [(1, 0.0, JITTER), (2, 20.0, None), (2, -7.5, None), (3, 12.0, JITTER), (3, -20.0, JITTER)])
def test_a_solid_text_box_fills_the_forward_mapped_quadrilateral(flags, angle, jitter):
    at, row, cls = _solid(), _solid_row(), [1, 2, 3, 4, 5]
    h0, w0 = rd.layout(cls, row, at)[:2]
    assert (h0, w0) == (32, 80)
    wr = rd.warp_row(h0, w0, flags, 0, angle, jitter)
    img = rd.render_warp_u8(cls, row, np.zeros(rd.N_FX, np.int64), wr, at)
    quad = _quad_exact(h0, w0, angle, jitter)
    H, W = img.shape[:2]
    assert W == min(math.ceil(max(q[0] for q in quad)), rd.MAX_SIDE) and H == math.ceil(max(q[1] for q in quad))
    assert rd.render_warp_meta(np.pad(cls, (0, 20))[None], [5], row[None], wr[None], at).tolist() == [[0, H, W]]
    got = (img == 255).all(axis=2)
    assert set(np.unique(img[got ^ True])) <= set(range(5))          # alpha is 0 or 255: the box is solid and nothing is prefiltered
    half = Fraction(1, 2)
    mismatch = near = inside_n = 0
    for y in range(H):
        for x in range(W):
            p = (x + half, y + half)
            cross = [(b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) for a, b in zip(quad, quad[1:] + quad[:1])]
            inside = all(c >= 0 for c in cross)          # (clockwise on the screen, y pointing down)
            inside_n += inside
            close = any(_dist2_to_segment(p, a, b) <= 1 for a, b in zip(quad, quad[1:] + quad[:1]))
            near += close
            if inside != bool(got[y, x]):
                mismatch += 1
                assert close, "pixel (%d, %d) is %s the quadrilateral and more than a pixel from its edges" % (x, y, "inside" if inside else "outside")
    print("flags %d angle %g: %d x %d, %d pixels inside, %d within a pixel of an edge, %d of those mismatch" % (flags, angle, H, W, inside_n, near, mismatch))
    assert inside_n > 2000 and H * W - inside_n > 100 and mismatch <= near


@pytest.mark.parametrize("sign", [1, -1])
def test_the_top_edge_of_a_curved_box_follows_the_parabola(sign):
    at, row, cls = _solid(), _solid_row(), [1, 2, 3, 4, 5]
    h0, w0 = rd.layout(cls, row, at)[:2]
    amp = sign * int(rd.CURVE_MAX * 32 * 65536)
    wr = rd.warp_row(h0, w0, 4, amp)
    room = int(wr[rd.WP_ROOM])
    assert room == 13 and wr[rd.WP_H] == h0 + room and wr[rd.WP_W] == w0
    got = (rd.render_warp_u8(cls, row, np.zeros(rd.N_FX, np.int64), wr, at) == 255).all(axis=2)
    worst = Fraction(0)
    for x in range(w0):
        t = Fraction(2 * x + 1, 2 * w0)
        top = Fraction(amp, 65536) * 4 * t * (1 - t) + (room if sign < 0 else 0)          # the column's top edge on the bent canvas
        ys = np.flatnonzero(got[:, x])
        assert len(ys) and (np.diff(ys) == 1).all() and abs(len(ys) - h0) <= 1
        worst = max(worst, abs(int(ys[0]) - top))
    print("curve sign %+d: the top edge is at most %.3f pixels from the parabola" % (sign, float(worst)))
    assert worst <= 1
    assert got[:, 0].argmax() == got[:, w0 - 1].argmax() and abs(int(got[:, w0 // 2].argmax()) - int(got[:, 0].argmax())) >= room - 1


# --------------------------------------------------------------------------------------------------------------------------- draws
class _Counting(random.Random):
    def random(self):
        self.calls = getattr(self, "calls", 0) + 1
        return super().random()


def test_an_empty_setting_consumes_exactly_the_fx_stream():
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(rd.FX_KINDS, 0.5, pool, at)
    for setting in ((), None):
        a, b = random.Random(9), random.Random(9)
        want = rd.draw_render_fx(WORDS, 2, a, 7, fx)
        got = rd.draw_render_warp(WORDS, 2, b, 7, fx, setting)
        assert got[0] == want[0] and all(np.array_equal(x, y) for x, y in zip(got[1:5], want[1:]))
        assert got[5].shape == (7, rd.N_WARP) and not got[5].any() and a.random() == b.random()
    with pytest.raises(ValueError):
        rd.draw_render_warp(WORDS, 2, random.Random(1), 0, (), ())


@pytest.mark.parametrize("kinds", [("perspective",), ("rotate",), ("curve",), ("perspective", "curve"), rd.WARP_KINDS])
def test_a_listed_kind_draws_after_the_fx_draws_only(kinds):
    at, pool = _atlases(), _pool()
    fx = rd.RenderFx(("outline", "texture"), 0.5, pool, at)
    warp = rd.RenderWarp(kinds, 0.6, 0.3, 20.0, 0.4, at)
    # one sample: the params and fx rows are those of draw_render_fx from the same seed, and what follows in the stream are the warp's
    # random() calls alone: 1 per listed kind, + 8 / 1 / 1 where perspective / rotate / curve is on
    flags_seen = set()
    for seed in range(40):
        a, b = _Counting(seed), _Counting(seed)
        want = rd.draw_render_fx(WORDS, 2, a, 1, fx)
        got = rd.draw_render_warp(WORDS, 2, b, 1, fx, warp)
        assert all(np.array_equal(x, y) for x, y in zip(got[1:5], want[1:]))
        fl = int(got[5][0, 0])
        flags_seen.add(fl)
        assert fl & ~sum(1 << rd.WARP_KINDS.index(k) for k in kinds) == 0
        assert b.calls - a.calls == len(kinds) + 8 * (fl & 1) + (fl >> 1 & 1) + (fl >> 2 & 1)
        [a.random() for _ in range(b.calls - a.calls)]
        assert a.getstate() == b.getstate()          # (no getrandbits, no other call)
    assert len(flags_seen) == 2 ** len(kinds)
    # the same seed gives the same rows, and they are inside their domain
    one, two = rd.draw_render_warp(WORDS, 2, random.Random(3), 30, fx, warp), rd.draw_render_warp(WORDS, 2, random.Random(3), 30, fx, warp)
    assert one[0] == two[0] and all(np.array_equal(x, y) for x, y in zip(one[1:], two[1:]))
    rows = rd.check_render_warp(one[5], one[3], n=30)
    on = rows[:, 0] != 0
    gh = one[3][:, rd.GH]
    assert on.any() and (np.abs(rows[:, rd.WP_AMP]) <= 0.4 * gh * 65536).all() and np.abs(rows[on, rd.WP_COEF:rd.WP_COEF + 9]).max(axis=1).tolist() == [rd.COEF_MAX] * int(on.sum())
    meta = rd.render_warp_meta(one[1], one[2], one[3], rows, at)
    for i in range(0, 30, 5):
        assert rd.render_warp_u8(one[1][i, :one[2][i]], one[3][i], one[4][i], rows[i], at, pool).shape == (meta[i, 1], meta[i, 2], 3)


# -------------------------------------------------------------------------------------------------------------------------- checks
def test_check_render_warp_refuses_rows_outside_their_domain():
    at = _atlases()
    cls = rd.word_classes("hello")
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.GH] = 40
    row[rd.FG:rd.FG + 3] = 200
    h0, w0 = rd.layout(cls, row, at)[:2]
    good = rd.warp_row(h0, w0, 7, int(0.4 * 40 * 65536), 10.0, JITTER)
    assert np.array_equal(rd.check_render_warp(good[None], row[None]), good[None])
    bad_rows = []
    for col, val in ((rd.WP_COEF + 2, rd.COEF_MAX + 1), (rd.WP_COEF, -rd.COEF_MAX - 1),          # a coefficient over the bound
                     (rd.WP_COEF + 8, 0), (rd.WP_COEF + 8, -good[rd.WP_COEF + 8]),                # den <= 0 at the origin
                     (rd.WP_COEF + 6, -rd.COEF_MAX),                                              # den <= 0 at the right corners
                     (rd.WP_AMP, int(0.4 * 40 * 65536) + 1), (rd.WP_AMP, -int(0.4 * 40 * 65536) - 1), (rd.WP_ROOM, 15),
                     (rd.WP_FLAGS, 8), (rd.WP_FLAGS, -1), (rd.WP_H, 0), (rd.WP_W, rd.MAX_SIDE + 1), (14, 1), (15, 1)):
        bad = good.copy()
        bad[col] = val
        bad_rows.append(bad)
    no_curve = good.copy()
    no_curve[rd.WP_FLAGS] = 3          # amp without the curve bit
    for bad in bad_rows + [no_curve]:
        with pytest.raises(ValueError, match="render_warp"):
            rd.check_render_warp(bad[None], row[None])
        with pytest.raises(ValueError, match="render_warp"):
            rd.render_warp_u8(cls, row, np.zeros(rd.N_FX, np.int64), bad, at)
    for shape in ((1, 15), (2, 16), (16,)):
        with pytest.raises(ValueError, match="one row per sample"):
            rd.check_render_warp(np.zeros(shape, np.int64), row[None])
    with pytest.raises(ValueError, match="one row per sample"):
        rd.check_render_warp(good[None], row[None], n=2)
    # a row whose flags are 0 is not read
    idle = good.copy()
    idle[rd.WP_FLAGS] = 0
    rd.check_render_warp(idle[None], row[None])
    with pytest.raises(ValueError, match="not convex enough|degenerate"):
        rd.warp_row(h0, w0, 1, 0, 0.0, [(w0, 0), (-w0, 0), (0, 0), (0, 0)])
    for bad in (dict(kinds=["bend"]), dict(kinds=["curve", "curve"]), dict(kinds=[]), dict(kinds=["curve"], prob=1.5),
                dict(kinds=["curve"], prob=float("nan")), dict(kinds=["curve"], persp=0.0), dict(kinds=["curve"], persp=0.31),
                dict(kinds=["curve"], angle=0.0), dict(kinds=["curve"], angle=20.5), dict(kinds=["curve"], curve=-0.1),
                dict(kinds=["curve"], curve=0.41)):
        with pytest.raises(ValueError, match="--train_words_warp"):
            rd.RenderWarp(atlases=at, **bad)
    with pytest.raises(ValueError, match="needs the atlases"):
        rd.RenderWarp(["curve"])
    assert rd.RenderWarp(["curve", "perspective"], atlases=at).kinds == ("perspective", "curve")


def test_fingerprint_carries_the_warp_setting(tmp_path):
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))
    args = SimpleNamespace(arch="tatt", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="4,", embed_dim="96,",
                           depths="1,", num_heads="6,", window_size="2,4,8,", mlp_ratio="4,", train_words="words.txt")
    at = _atlases()
    plain = rd.words_setting(WORDS, at, 100)
    assert plain == rd.words_setting(WORDS, at, 100, None, None) == rd.words_setting(WORDS, at, 100, (), ()) and sorted(plain) == ["crc32", "epoch", "fonts"]
    fx = rd.RenderFx(("shadow",))
    assert rd.words_setting(WORDS, at, 100, fx) == rd.words_setting(WORDS, at, 100, fx, None)
    warp = rd.RenderWarp(("rotate", "curve"), 0.5, 0.15, 10.0, 0.2, at)
    setting = rd.words_setting(WORDS, at, 100, None, warp)
    assert {k: setting[k] for k in plain} == plain and setting["warp_kinds"] == ["rotate", "curve"]
    assert (setting["warp_prob"], setting["warp_persp"], setting["warp_angle"], setting["warp_curve"]) == (0.5, 0.15, 10.0, 0.2)
    off, on = base.state_fingerprint(args, cfg, train_words=plain), base.state_fingerprint(args, cfg, train_words=setting)
    base.check_fingerprint(off, off)                      # a state written without the flag keeps loading without it
    path = str(tmp_path / "state.pt")
    base.write_train_state(path, {"version": base.TRAIN_STATE_VERSION, "fingerprint": on})
    assert base.read_train_state(path, on)["fingerprint"]["train_words"] == setting
    others = [plain] + [rd.words_setting(WORDS, at, 100, None, rd.RenderWarp(*a, atlases=at)) for a in (
        (("rotate",), 0.5, 0.15, 10.0, 0.2), (("perspective", "rotate", "curve"), 0.5, 0.15, 10.0, 0.2), (("rotate", "curve"), 0.25, 0.15, 10.0, 0.2),
        (("rotate", "curve"), 0.5, 0.2, 10.0, 0.2), (("rotate", "curve"), 0.5, 0.15, 12.0, 0.2), (("rotate", "curve"), 0.5, 0.15, 10.0, 0.3))]
    for other in others:
        with pytest.raises(ValueError, match="train_words"):
            base.read_train_state(path, base.state_fingerprint(args, cfg, train_words=other))


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_render_warp", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_flag_checks_exit_with_one_clear_line(tmp_path):
    m = _main()
    f = tmp_path / "words.txt"
    f.write_text("word\n")
    w = str(f)
    for args, msg in ((dict(train_words_warp="curve"), "needs --train_words"),
                      (dict(train_words=w, train_words_warp="curve,bend"), "distinct kinds of perspective, rotate, curve"),
                      (dict(train_words=w, train_words_warp="curve,curve"), "distinct kinds"),
                      (dict(train_words=w, train_words_warp="rotate", train_words_warp_prob=1.5), "probability in 0 .. 1"),
                      (dict(train_words=w, train_words_warp="rotate", train_words_warp_persp=0.0), "0 < F <= 0.3"),
                      (dict(train_words=w, train_words_warp="rotate", train_words_warp_persp=0.35), "0 < F <= 0.3"),
                      (dict(train_words=w, train_words_warp="rotate", train_words_warp_angle=25.0), "0 < DEG <= 20"),
                      (dict(train_words=w, train_words_warp="rotate", train_words_warp_angle=-1.0), "0 < DEG <= 20"),
                      (dict(train_words=w, train_words_warp="curve", train_words_warp_curve=0.5), "0 < F <= 0.4"),
                      (dict(train_words=w, train_words_warp="curve", train_words_warp_curve=0.0), "0 < F <= 0.4")):
        with pytest.raises(SystemExit, match=msg) as e:
            m.main(SimpleNamespace(), SimpleNamespace(**args))
        assert str(e.value).startswith("main.py: ") and "\n" not in str(e.value)
    src = m.train_words_source(SimpleNamespace(train_words=w, train_words_warp="curve, perspective", train_words_warp_prob=0.25,
                                               train_words_warp_curve=0.4), "upper")
    assert len(src) == 5 and src[3] is None
    warp = src[4]
    assert warp.kinds == ("perspective", "curve") and (warp.prob, warp.persp, warp.angle, warp.curve) == (0.25, 0.15, 10.0, 0.4) and warp.atlases is src[1]
    assert rd.words_setting(*src)["warp_kinds"] == ["perspective", "curve"]
    assert len(m.train_words_source(SimpleNamespace(train_words=w), "upper")) == 4          # without the flag the tuple is what it was
    assert m.train_words_warp(SimpleNamespace()) is None


# ------------------------------------------------------------------------------------------------- sr_batches with stubbed device ops
def test_sr_batches_draws_and_renders_through_the_warp_path(monkeypatch):
    """a WordsHR loader whose collate carries a RenderWarp: per batch the draws are draw_render_warp's from random.Random(pass key + j),
    before the degradation's, and the render goes to ops.render_words_warp_u8; the degradation sees the warped canvases' widths"""
    import torch
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.words import WordsHR
    from dpmn_amd.utils.degrade import draw_params
    from dpmn_amd.utils.resize import pack_ragged, pil_resize_u8
    at = _atlases()
    warp = rd.RenderWarp(rd.WARP_KINDS, 0.7, atlases=at)
    calls = {"warp": [], "degrade": []}

    def render_warp(cls, lens, params, rows, wrows, atlases, pool_, device=None, out=None):
        calls["warp"].append((np.array(cls), np.array(lens), np.array(params), np.array(rows), np.array(wrows), pool_))
        return pack_ragged([rd.render_warp_u8(c[:n], p, r, wr, atlases, pool_) for c, n, p, r, wr in zip(cls, lens, params, rows, wrows)], pin=False)

    def degrade(packed, meta, params, z=None, seed=0):
        calls["degrade"].append((np.array(params), int(seed)))
        return packed.clone()

    def resize(packed, meta, H, W):
        flat = packed.numpy()
        return torch.from_numpy(np.stack([pil_resize_u8(flat[o:o + h * w * 3].reshape(h, w, 3), H, W) for o, h, w in np.asarray(meta).tolist()]))

    def never(*a, **k):
        raise AssertionError("the warp path renders with ops.render_words_warp_u8 alone")

    monkeypatch.setattr(ops, "render_words_warp_u8", render_warp, raising=False)
    monkeypatch.setattr(ops, "render_words_fx_u8", never)
    monkeypatch.setattr(ops, "render_words_u8", never)
    monkeypatch.setattr(ops, "degrade_ragged_u8", degrade)
    monkeypatch.setattr(ops, "resize_ragged_u8", resize)
    monkeypatch.setattr(ops, "collate_u8", lambda img, mask: img.permute(0, 3, 1, 2).float() / 255.0)
    kw = dict(imgH=32, imgW=128, down_sample_scale=2, mask=False, gpu_finish=True, gpu_resize=True, degrade=True, cutblur=True)
    with pytest.raises(ValueError, match="render_warp needs render"):
        tz.alignCollate_realWTLAMask(render_warp=warp, **kw)
    col = tz.alignCollate_realWTLAMask(render=(WORDS, at), render_warp=warp, **kw)
    assert col.render_fx is None and col.render_warp is warp
    loader = torch.utils.data.DataLoader(WordsHR(WORDS, 6), batch_size=4, shuffle=False, collate_fn=col, num_workers=0)
    random.seed(3)
    state = random.getstate()
    got = list(tz.sr_batches(loader, torch.device("cpu")))
    assert [len(b[3]) for b in got] == [4, 2] and got[0][0].shape == (4, 3, 32, 128)
    random.setstate(state)
    key = random.getrandbits(63)
    for j, n in enumerate((4, 2)):
        rng = random.Random(key + j)
        want = rd.draw_render_warp(WORDS, 2, rng, n, None, warp)
        assert got[j][3] == want[0] and all(np.array_equal(x, y) for x, y in zip(calls["warp"][j][:5], want[1:])) and calls["warp"][j][5] is None
        widths = rd.render_warp_meta(want[1], want[2], want[3], want[5], at)[:, 2]
        assert np.array_equal(calls["degrade"][j][0], draw_params(n, cutblur=True, hr_widths=widths.tolist(), rng=rng))
        assert calls["degrade"][j][1] == rng.getrandbits(63)
    assert any(c[4].any() for c in calls["warp"])
    assert tz.alignCollate_realWTLAMask(render=(WORDS, at), **kw).render_warp is None
