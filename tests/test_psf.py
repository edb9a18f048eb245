"""Random point-spread functions on the CPU (utils/psf.py, main.py --psf_blur): the properties of the quantised taps, the integer blur
against an independent dense float64 evaluation, the documented draw sequence and where it sits among degrade_on_gpu's draws, the
settings, the flag errors and the --train_state fingerprint."""
import importlib.util
import math
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dpmn_amd.utils import degrade as dg
from dpmn_amd.utils import psf
from dpmn_amd.utils.resize import pack_ragged

HERE = os.path.dirname(os.path.abspath(__file__))


def _dense(taps, R=None):
    """(K, K) int64 table of a tap list, R = the largest offset unless given"""
    t = np.asarray(taps, np.int64)
    R = int(np.abs(t[:, :2]).max()) if R is None else R
    k = np.zeros((2 * R + 1, 2 * R + 1), np.int64)
    k[t[:, 0] + R, t[:, 1] + R] = t[:, 2]
    return k


# ------------------------------------------------------------------------------------------------------------------------ psf_taps
def test_taps_properties_over_6000_draws():
    """sum exactly 2^16, q > 0, offsets within R, n <= 441, centroid within 0.05 px of the centre (the blur must not shift the LR image
    against the HR one), and the fix-up leaves the largest tap positive."""
    rng = random.Random(7)
    worst_c = worst_fix = 0.0
    least_top = psf.ONE
    seen_R = set()
    for i in range(6000):
        kind = psf.KINDS[i % 3]
        r, theta, ratio = rng.uniform(1, 10), rng.uniform(0, math.pi), rng.uniform(0.25, 1)
        t = psf.psf_taps(kind, r, theta, ratio)
        assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 3 and 1 <= t.shape[0] <= psf.MAX_TAPS == 441
        R = math.ceil(r)
        seen_R.add(R)
        q = t[:, 2].astype(np.int64)
        assert int(q.sum()) == 65536 and q.min() > 0
        assert np.abs(t[:, :2]).max() <= R
        order = t[:, 0].astype(np.int64) * 100 + t[:, 1]
        assert (np.diff(order) > 0).all(), "row-major order, no tap twice"
        c = max(abs(float((t[:, 0] * q).sum())), abs(float((t[:, 1] * q).sum()))) / 65536
        worst_c = max(worst_c, c)
        # the fix-up: recomputed from the real weights
        w = psf._weights(kind, r, theta, ratio)
        q0 = np.floor(w / w.sum() * 65536 + 0.5).astype(np.int64)
        fix = 65536 - int(q0.sum())
        assert q0.max() + fix > 0, (kind, r, theta, ratio, fix, int(q0.max()))
        worst_fix, least_top = max(worst_fix, abs(fix)), min(least_top, int(q0.max()))
        top = np.unravel_index(int(np.argmax(q0)), q0.shape)
        q0[top] += fix
        assert np.array_equal(_dense(t, R), q0)
    print("psf taps: largest centroid offset %.4f px, largest |fix-up| %d, smallest largest tap %d" % (worst_c, worst_fix, least_top))
    assert worst_c <= 0.05
    assert seen_R == set(range(2, 11))                   # (R = 1 is r = 1 exactly: test_taps_shapes)


def test_taps_shapes():
    for r in (1.0, 2.5, 7.3, 10.0):
        m = psf.psf_taps("motion", r, 0.0)
        assert (m[:, 0] == 0).all() and m.shape[0] > 1, "theta = 0: all the mass in the centre row"
        v = psf.psf_taps("motion", r, math.pi / 2)
        assert (v[:, 1] == 0).all() and v.shape[0] > 1, "theta = pi / 2: the centre column (cos(pi / 2) = 6e-17 quantises to nothing)"
        for kind, theta in (("disk", 0.0), ("aniso", 0.7)):
            # the real weights and the rounded taps are symmetric; the fix-up of the sum then goes to ONE tap, the first of the largest
            # in row-major order -- the centre for the Gaussian, but the first tap of the plateau for a disk, where it is the only
            # asymmetry (a few units of 65536; the centroid bound of the test above covers it)
            w = psf._weights(kind, r, theta, 1.0)
            assert all(np.allclose(w, v, rtol=1e-12, atol=0) for v in (w.T, w[::-1], w[:, ::-1]))      # (the rotation rounds)
            k = _dense(psf.psf_taps(kind, r, theta, 1.0), math.ceil(r))
            top = np.unravel_index(int(np.argmax(w)), w.shape)
            k[top] -= 65536 - int(np.floor(w / w.sum() * 65536 + 0.5).sum())
            assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])
            if kind == "aniso":
                k = _dense(psf.psf_taps(kind, r, theta, 1.0))
                assert top == (math.ceil(r),) * 2 and np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])
    a = _dense(psf.psf_taps("aniso", 8.0, 0.0, 0.25))
    assert (a > 0).sum(axis=1).max() > (a > 0).sum(axis=0).max(), "theta = 0, ratio < 1: long along x"
    assert psf.psf_taps("identity").tolist() == [[0, 0, 65536]] and psf.is_identity(psf.psf_taps("identity"))
    assert psf.psf_taps("disk", 1.0).shape[0] == 9 and psf.psf_taps("disk", 10.0).shape[0] <= 441
    for bad in (0.5, 10.5):
        with pytest.raises(ValueError, match="radius"):
            psf.psf_taps("disk", bad)
    with pytest.raises(ValueError, match="unknown kind"):
        psf.psf_taps("box", 2.0)


# --------------------------------------------------------------------------------------------------------------------- psf_blur_u8
def _image(rng, h, w):
    a = rng.randint(0, 256, (h, w, 3)).astype(np.int32)
    a[:, w // 3:] = np.clip(a[:, w // 3:] // 4 + 150, 0, 255)
    a[h // 2:, : w // 2] //= 3
    return a.astype(np.uint8)


def _dense_blur(img, taps, R):
    """independent: np.pad(mode='reflect') by R, the full K x K loop in float64 (every sum is an integer below 2^53: exact)"""
    h, w = img.shape[:2]
    k = np.zeros((2 * R + 1, 2 * R + 1), np.float64)
    for dy, dx, q in np.asarray(taps).tolist():
        k[dy + R, dx + R] = q
    p = np.pad(img.astype(np.float64), ((R, R), (R, R), (0, 0)), mode="reflect")
    v = np.zeros(img.shape, np.float64)
    for i in range(2 * R + 1):
        for j in range(2 * R + 1):
            v += k[i, j] * p[i:i + h, j:j + w]
    return np.floor(v / 65536 + 0.5).astype(np.uint8)


def _fold(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def test_blur_equals_the_dense_float64_evaluation():
    rng = np.random.RandomState(3)
    cases = [("motion", 10.0, 0.3, 1.0), ("motion", 1.0, 2.0, 1.0), ("disk", 10.0, 0, 1), ("disk", 1.0, 0, 1), ("aniso", 10.0, 1.1, 0.3),
             ("aniso", 1.7, 2.5, 0.9), ("motion", 4.2, math.pi / 2, 1.0)]
    for (h, w) in ((11, 11), (16, 64), (33, 45)):
        img = _image(rng, h, w)
        for kind, r, theta, ratio in cases:
            t = psf.psf_taps(kind, r, theta, ratio)
            got = psf.psf_blur_u8(img, t)
            assert got.dtype == np.uint8 and got.shape == img.shape
            assert np.array_equal(got, _dense_blur(img, t, math.ceil(r))), (h, w, kind, r)
            assert not np.array_equal(got, img)


def test_blur_of_sides_below_the_radius_folds_repeatedly():
    rng = np.random.RandomState(4)
    for kind in psf.KINDS:
        t = psf.psf_taps(kind, 10.0, 0.9, 0.5)
        assert np.abs(t[:, :2]).max() >= 8               # (R = 10; the segment at 0.9 rad reaches 10 sin 0.9 = 7.8)
        for h, w in ((1, 1), (1, 7), (2, 3), (3, 2), (3, 3), (2, 1)):
            img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            want = np.zeros_like(img)
            for y in range(h):
                for x in range(w):
                    acc = np.full(3, 32768, np.int64)
                    for dy, dx, q in t.tolist():
                        acc += q * img[_fold(y + dy, h), _fold(x + dx, w)].astype(np.int64)
                    want[y, x] = acc >> 16
            assert np.array_equal(psf.psf_blur_u8(img, t), want), (kind, h, w)


def test_identity_and_flat_images_come_out_unchanged():
    rng = np.random.RandomState(5)
    img = _image(rng, 13, 29)
    assert np.array_equal(psf.psf_blur_u8(img, psf.IDENTITY), img)
    for v in (0, 1, 127, 254, 255):
        flat = np.full((9, 14, 3), v, np.uint8)
        flat[..., 1] = 255 - v
        for kind in psf.KINDS:
            assert np.array_equal(psf.psf_blur_u8(flat, psf.psf_taps(kind, 6.5, 1.0, 0.4)), flat)
    with pytest.raises(ValueError):
        psf.psf_blur_u8(np.zeros((4, 4), np.uint8), psf.IDENTITY)


def test_cutblur_u8_is_degrade_u8s_last_step():
    rng = np.random.RandomState(6)
    lr, hr = rng.randint(0, 256, (5, 9, 3)).astype(np.uint8), rng.randint(0, 256, (5, 9, 3)).astype(np.uint8)
    assert np.array_equal(psf.cutblur_u8(lr, hr, 4, 0), lr)
    one, two = psf.cutblur_u8(lr, hr, 4, 1), psf.cutblur_u8(lr, hr, 4, 2)
    assert np.array_equal(one[:, 4:], hr[:, 4:]) and np.array_equal(one[:, :4], lr[:, :4])
    assert np.array_equal(two[:, :4], hr[:, :4]) and np.array_equal(two[:, 4:], lr[:, 4:])
    assert np.array_equal(psf.cutblur_u8(lr, hr, 0, 1), hr) and np.array_equal(psf.cutblur_u8(lr, hr, 9, 1), lr)
    assert np.array_equal(psf.cutblur_u8(lr, hr, 0, 2), lr) and np.array_equal(psf.cutblur_u8(lr, hr, 9, 2), hr)
    # the same bytes as degrade_u8 with the cut in its row
    row = np.array([3, 5.1, 0, 0, 0, 0, 3, 2.1, 0, 0, 3, 2.2, 3.1, 0, 0, 0], np.float32)
    cut = row.copy()
    cut[dg.CUT_X], cut[dg.CUT_SIDE] = 3, 2
    z = np.zeros(hr.shape, np.float32)
    assert np.array_equal(psf.cutblur_u8(dg.degrade_u8(hr, row, z), hr, 3, 2), dg.degrade_u8(hr, cut, z))
    with pytest.raises(ValueError):
        psf.cutblur_u8(lr, hr[:4], 1, 1)


# ------------------------------------------------------------------------------------------------------------------------- draws
class _Spy(random.Random):
    """records the calls of the public draw methods, in order (a method built on another one of the class is recorded once)"""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def _rec(self, name, args, fn):
        n = len(self.calls)
        v = fn(*args)
        del self.calls[n:]
        self.calls.append((name,) + tuple(args) + (v,))
        return v

    def random(self):
        return self._rec("random", (), super().random)

    def uniform(self, a, b):
        return self._rec("uniform", (a, b), super().uniform)

    def randint(self, a, b):
        return self._rec("randint", (a, b), super().randint)

    def getrandbits(self, k):
        return self._rec("getrandbits", (k,), super().getrandbits)


def test_draw_psf_replays_the_documented_sequence():
    kinds, prob, frac = ("disk", "motion", "aniso"), 0.6, 0.3
    heights = [5, 12, 20, 33, 64, 200] * 20
    spy = _Spy(7)
    taps = psf.draw_psf(len(heights), kinds, prob, frac, heights, rng=spy)
    it = iter(spy.calls)
    n_id = 0
    for h, t in zip(heights, taps):
        c = next(it)
        assert c[0] == "random"
        if c[1] < prob:
            k, r, th, ra = next(it), next(it), next(it), next(it)
            rmax = min(10.0, max(1.0, frac * h))
            assert k[:3] == ("randint", 0, 2) and r[:3] == ("uniform", 1.0, rmax) and th[:3] == ("uniform", 0.0, math.pi)
            assert ra[:3] == ("uniform", 0.25, 1.0) and 1.0 <= r[3] <= rmax
            assert np.array_equal(t, psf.psf_taps(kinds[k[3]], r[3], th[3], ra[3]))
            assert np.abs(t[:, :2]).max() <= math.ceil(rmax)
        else:
            assert psf.is_identity(t)
            n_id += 1
    assert next(it, None) is None and 0 < n_id < len(heights)
    ref = random.Random(7)                               # the same stream by hand
    for h, t in zip(heights, taps):
        if ref.random() < prob:
            kind = kinds[ref.randint(0, 2)]
            want = psf.psf_taps(kind, ref.uniform(1, min(10, max(1, frac * h))), ref.uniform(0, math.pi), ref.uniform(0.25, 1))
        else:
            want = psf.IDENTITY
        assert np.array_equal(t, want)
    spy = _Spy(1)
    off = psf.draw_psf(50, kinds, 0.0, frac, [32] * 50, rng=spy)
    assert all(psf.is_identity(t) for t in off) and [c[0] for c in spy.calls] == ["random"] * 50, "prob = 0: one draw per image"
    assert not any(psf.is_identity(t) for t in psf.draw_psf(50, ("disk",), 1.0, frac, [32] * 50, rng=random.Random(2)))
    small = psf.draw_psf(30, ("disk",), 1.0, 0.12, [4] * 30, rng=random.Random(3))      # rmax = 1: r = 1 exactly
    assert all(np.array_equal(t, psf.psf_taps("disk", 1.0)) for t in small)
    random.seed(5)
    a = psf.draw_psf(8, kinds, 0.5, frac, [40] * 8)     # Python's `random` module by default
    random.seed(5)
    assert all(np.array_equal(x, y) for x, y in zip(a, psf.draw_psf(8, kinds, 0.5, frac, [40] * 8)))
    with pytest.raises(ValueError):
        psf.draw_psf(3, kinds, 0.5, frac, [40, 40])


@pytest.fixture
def stub_ops(monkeypatch):
    """the device ops of degrade_on_gpu -> host stand-ins that record what they were given, in call order"""
    from dpmn_amd import ops
    calls = []

    def degrade(packed, meta, params, z=None, seed=0):
        calls.append(("degrade", np.array(params), int(seed)))
        return packed.clone()

    def blur(packed, meta, taps):
        calls.append(("psf", [np.array(t) for t in taps]))
        return packed.clone()

    def cut(low, packed, meta, params):
        calls.append(("cutblur", np.array(params)))
        return low

    def jpeg(images, quality, out=None):
        calls.append(("jpeg", np.array(quality)))
        return images

    monkeypatch.setattr(ops, "degrade_ragged_u8", degrade)
    monkeypatch.setattr(ops, "psf_blur_ragged_u8", blur)
    monkeypatch.setattr(ops, "cutblur_ragged_u8", cut)
    monkeypatch.setattr(ops, "jpeg_roundtrip_u8", jpeg)
    monkeypatch.setattr(ops, "resize_ragged_u8", lambda packed, meta, H, W: torch.zeros(len(meta), H, W, 3, dtype=torch.uint8))
    monkeypatch.setattr(ops, "collate_u8", lambda img, mask: img.permute(0, 3, 1, 2).float())
    return calls


def test_degrade_on_gpu_draws_params_then_seed_then_psf_then_jpeg(stub_ops):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils.jpeg import draw_jpeg
    rs = np.random.RandomState(8)
    pair = pack_ragged([rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((12, 40), (33, 90), (64, 200), (7, 9))], pin=False)
    meta = pair[1].numpy()
    widths, heights = [int(w) for w in meta[:, 2]], [int(h) for h in meta[:, 1]]
    setting = (("motion", "disk", "aniso"), 0.7, 0.3)

    # ---- with the stage: the recorded stream is params, seed, PSF, JPEG, in that order
    spy = _Spy(21)
    tz.degrade_on_gpu(pair, (32, 128), 2, True, "cpu", cutblur=True, rng=spy, jpeg=(30, 95, 0.5), psf=setting)
    ref = _Spy(21)
    params = dg.draw_params(4, cutblur=True, hr_widths=widths, rng=ref)
    seed = ref.getrandbits(63)
    taps = psf.draw_psf(4, setting[0], setting[1], setting[2], heights, rng=ref)
    q = draw_jpeg(4, 30, 95, 0.5, rng=ref)
    assert spy.calls == ref.calls
    assert [c[0] for c in stub_ops] == ["psf", "degrade", "cutblur", "jpeg"]
    assert all(np.array_equal(a, b) for a, b in zip(stub_ops[0][1], taps)) and len(stub_ops[0][1]) == 4
    uncut = params.copy()
    uncut[:, [dg.CUT_X, dg.CUT_SIDE]] = 0
    assert params[:, dg.CUT_X].any(), "the cut columns are drawn"
    assert np.array_equal(stub_ops[1][1], uncut) and stub_ops[1][2] == seed, "the blurred pack is degraded with the cut zeroed"
    assert np.array_equal(stub_ops[2][1], params), "cutblur gets the drawn rows"
    assert np.array_equal(stub_ops[3][1], q)

    # ---- without it: the sequence and the launches of before
    del stub_ops[:]
    spy = _Spy(21)
    tz.degrade_on_gpu(pair, (32, 128), 2, True, "cpu", cutblur=True, rng=spy, jpeg=(30, 95, 0.5))
    ref = _Spy(21)
    params = dg.draw_params(4, cutblur=True, hr_widths=widths, rng=ref)
    seed = ref.getrandbits(63)
    q = draw_jpeg(4, 30, 95, 0.5, rng=ref)
    assert spy.calls == ref.calls
    assert [c[0] for c in stub_ops] == ["degrade", "jpeg"]
    assert np.array_equal(stub_ops[0][1], params) and stub_ops[0][2] == seed and np.array_equal(stub_ops[1][1], q)


# ------------------------------------------------------------------------------------------------------------- settings and flags
def test_psf_setting():
    ns = SimpleNamespace
    assert psf.psf_setting(ns()) is None and psf.psf_setting(ns(psf_blur=None, psf_prob=7)) is None and psf.psf_setting(ns(psf_blur="")) is None
    assert psf.psf_setting(ns(psf_blur="motion")) == (("motion",), 0.5, 0.12)
    assert psf.psf_setting(ns(psf_blur="disk, motion", psf_prob=None, psf_radius=None)) == (("disk", "motion"), 0.5, 0.12), "the given order"
    assert psf.psf_setting(ns(psf_blur="aniso,disk,motion", psf_prob=1, psf_radius=1)) == (("aniso", "disk", "motion"), 1.0, 1.0)
    assert psf.psf_setting(ns(psf_blur=("disk",), psf_prob=0, psf_radius=0.3)) == (("disk",), 0.0, 0.3)
    for kw, word in ((dict(psf_blur="box"), "comma list"), (dict(psf_blur="motion,,disk"), "comma list"), (dict(psf_blur=","), "comma list"),
                     (dict(psf_blur="motion,motion"), "twice"), (dict(psf_blur="disk", psf_prob=1.5), "--psf_prob"),
                     (dict(psf_blur="disk", psf_prob=-0.1), "--psf_prob"), (dict(psf_blur="disk", psf_radius=0), "--psf_radius"),
                     (dict(psf_blur="disk", psf_radius=1.01), "--psf_radius"), (dict(psf_blur="disk", psf_radius=-1), "--psf_radius")):
        with pytest.raises(ValueError, match=word) as e:
            psf.psf_setting(ns(**kw))
        assert "\n" not in str(e.value)


def test_collate_needs_degrade_for_psf():
    from dpmn_amd.dataset import textzoom as tz
    with pytest.raises(ValueError, match="psf=.* needs degrade=True"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, psf=(("disk",), 0.5, 0.12))
    with pytest.raises(ValueError, match="distinct kinds"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True, psf=(("box",), 0.5, 0.12))
    with pytest.raises(ValueError, match="frac"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True, psf=(("disk",), 0.5, 0.0))
    col = tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True, psf=(["disk", "motion"], 1, 0.25))
    assert col.psf == (("disk", "motion"), 1.0, 0.25)
    assert tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True).psf is None
    assert tz.alignCollate_realWTLAMask().psf is None


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_psf", os.path.join(os.path.dirname(HERE), "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_exits_with_one_clear_line():
    m = _main()

    def run(**kw):
        a = dict(cutblur=False, manmade_degrade=True, train_hr_dir=None, psf_blur=None, psf_prob=0.5, psf_radius=0.12)
        a.update(kw)
        with pytest.raises(SystemExit) as e:
            m.main(SimpleNamespace(), SimpleNamespace(**a))
        assert "\n" not in str(e.value)
        return str(e.value)

    assert run(psf_blur="motion", manmade_degrade=False).startswith("main.py: --psf_blur needs --manmade_degrade")
    assert run(psf_blur="box").startswith("main.py: --psf_blur takes a comma list")
    assert "twice" in run(psf_blur="disk,disk")
    assert "--psf_prob" in run(psf_blur="disk", psf_prob=2)
    assert "--psf_radius" in run(psf_blur="disk", psf_radius=0)
    # with a source of synthesised LR images the flag passes this check (the run then ends at the next one: no such folder)
    assert "--train_hr_dir" in run(psf_blur="disk", manmade_degrade=False, train_hr_dir="/nonexistent/hr")


def test_fingerprint_with_and_without_the_field():
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))

    def args(**kw):
        a = dict(arch="tsrn", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="2,", embed_dim="96,", depths="1,",
                 num_heads="6,", window_size="2,4,8,", mlp_ratio="4,", manmade_degrade=True)
        a.update(kw)
        return SimpleNamespace(**a)

    off = base.state_fingerprint(args(), cfg)
    assert off["psf_blur"] is None and "psf_blur" in base.FINGERPRINT_FIELDS and "psf_blur" in base.DATA_FIELDS
    on = base.state_fingerprint(args(psf_blur="motion,disk", psf_prob=0.5, psf_radius=0.12), cfg)
    assert on["psf_blur"] == [["motion", "disk"], 0.5, 0.12]
    old = {k: v for k, v in off.items() if k != "psf_blur"}      # a state written before the field existed
    base.check_fingerprint(old, off)
    base.check_fingerprint(off, off)
    base.check_fingerprint(on, base.state_fingerprint(args(psf_blur="motion,disk"), cfg))      # the defaults of the other two flags
    base.check_fingerprint({**on, "psf_blur": (("motion", "disk"), 0.5, 0.12)}, on)            # tuples after a reload are the same setting
    for saved, current in ((old, on), (off, on), (on, off), (on, base.state_fingerprint(args(psf_blur="disk,motion"), cfg)),
                           (on, base.state_fingerprint(args(psf_blur="motion,disk", psf_prob=0.25), cfg)),
                           (on, base.state_fingerprint(args(psf_blur="motion,disk", psf_radius=0.2), cfg))):
        with pytest.raises(ValueError, match="psf_blur"):
            base.check_fingerprint(saved, current)
    # the file survives the weights-only reload of a training state
    import io
    buf = io.BytesIO()
    torch.save({"fingerprint": on}, buf)
    buf.seek(0)
    base.check_fingerprint(torch.load(buf, weights_only=True)["fingerprint"], on)
