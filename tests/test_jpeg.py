"""JPEG artefacts on the CPU side: utils.jpeg.jpeg_roundtrip_u8 (the normative NumPy restatement) against PIL's save + open byte for
byte -- live where PIL has JPEG support, and against tests/golden/jpeg_roundtrip.npz (PIL's bytes recorded by `write_fixture`, run once
by hand: `PYTHONPATH=. python tests/test_jpeg.py`) everywhere -- draw_jpeg's draw order, and the plumbing: the collate's ValueError, main.py's
exits, the --train_state fingerprint."""
import importlib.util
import io
import os
import random
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from dpmn_amd.utils import jpeg as jp

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "jpeg_roundtrip.npz")
SIZES = [(1, 1), (8, 8), (16, 16), (16, 64), (17, 33), (15, 130), (32, 128), (7, 500)]
QUALITIES = [1, 5, 24, 25, 40, 50, 75, 95, 100]      # <= 24: force_baseline clamps; 50: the unscaled table; 100: all ones
KINDS = ["noise", "flat", "step", "glyph"]
SEED = 20261019


def make_input(kind, h, w, seed=SEED):
    """The (h, w, 3) uint8 test image of `kind`: a pure function of (kind, h, w, seed) -- the fixture stores the seed and a CRC of every
    input instead of the pixels."""
    rng = np.random.RandomState((seed + 1000 * h + w) % (2 ** 32))
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (201, 77, 18), np.uint8)
    if kind == "step":                                   # black / white column step
        a = np.zeros((h, w, 3), np.uint8)
        a[:, w // 2:] = 255
        return a
    assert kind == "glyph"                               # dark strokes of a few pixels on tinted paper, a coloured underline
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([210 - xx // 8, 200 - yy * 2, 170 + (xx + yy) % 7], -1).astype(np.int32)
    x = 1
    while x < w:
        sw = int(rng.randint(1, 4))
        top, bot = int(rng.randint(0, max(h // 3, 1))), h - int(rng.randint(0, max(h // 4, 1)))
        a[top:bot, x:x + sw] = (20 + int(rng.randint(0, 30)), 25, 40)
        if rng.rand() < 0.5:
            a[top:top + 2, x:x + sw + 4] = (35, 30, 30)
        x += sw + int(rng.randint(2, 7))
    a[h - 2:h - 1, :] = (190, 40, 60)
    return np.clip(a, 0, 255).astype(np.uint8)


def cases():
    return [(kind, h, w, q) for (h, w) in SIZES for kind in KINDS for q in QUALITIES]


def pil_jpeg():
    try:
        from PIL import Image, features
        return Image if features.check("jpg") else None
    except ImportError:
        return None


def pil_roundtrip(Image, img, q):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=q)
    buf.seek(0)
    return np.asarray(Image.open(buf))


def write_fixture(path=FIXTURE):
    """Run once by hand on a machine whose PIL has JPEG support: PIL's bytes of every case, concatenated in cases() order."""
    Image = pil_jpeg()
    assert Image is not None, "PIL with JPEG support is needed to write the fixture"
    out = np.concatenate([pil_roundtrip(Image, make_input(kind, h, w), q).reshape(-1) for kind, h, w, q in cases()])
    crc = np.array([zlib.crc32(make_input(kind, h, w).tobytes()) for (h, w) in SIZES for kind in KINDS], np.int64)
    np.savez_compressed(path, seed=np.int64(SEED), sizes=np.array(SIZES, np.int32), qualities=np.array(QUALITIES, np.int32),
                        kinds=np.array(KINDS), input_crc=crc, out=out)
    return path


_FIX = {}


def fixture_cases():
    """[(kind, h, w, q, input, PIL's bytes)] of the committed fixture: loaded once, never changed."""
    if not _FIX:
        z = np.load(FIXTURE)
        assert int(z["seed"]) == SEED and z["sizes"].tolist() == [list(s) for s in SIZES] and z["qualities"].tolist() == QUALITIES
        assert z["kinds"].tolist() == KINDS
        crc = iter(z["input_crc"].tolist())
        inputs = {}
        for (h, w) in SIZES:
            for kind in KINDS:
                inputs[kind, h, w] = make_input(kind, h, w)
                assert zlib.crc32(inputs[kind, h, w].tobytes()) == next(crc), "the generated input differs from the one PIL saw"
        out, pos, rows = z["out"], 0, []
        for kind, h, w, q in cases():
            n = h * w * 3
            rows.append((kind, h, w, q, inputs[kind, h, w], out[pos:pos + n].reshape(h, w, 3)))
            pos += n
        assert pos == out.size
        _FIX["rows"] = rows
    return _FIX["rows"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_is_what_pil_writes_and_reads_back(size):
    Image = pil_jpeg()
    if Image is None:
        pytest.skip("PIL without JPEG support")
    h, w = size
    for kind in KINDS:
        img = make_input(kind, h, w)
        for q in QUALITIES:
            want, got = pil_roundtrip(Image, img, q), jp.jpeg_roundtrip_u8(img, q)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), "%s %dx%d quality %d: %d bytes differ" % (kind, h, w, q, int((got != want).sum()))


def test_restatement_against_the_recorded_pil_bytes():
    rows = fixture_cases()
    assert len(rows) == len(SIZES) * len(KINDS) * len(QUALITIES)
    for kind, h, w, q, img, want in rows:
        got = jp.jpeg_roundtrip_u8(img, q)
        assert np.array_equal(got, want), "%s %dx%d quality %d: %d bytes differ" % (kind, h, w, q, int((got != want).sum()))
    assert any(not np.array_equal(img, want) for _, _, _, _, img, want in rows)


def test_quality_zero_returns_the_input_and_bad_arguments_raise():
    img = make_input("noise", 17, 33)
    out = jp.jpeg_roundtrip_u8(img, 0)
    assert np.array_equal(out, img) and out is not img
    for bad in (-1, 101):
        with pytest.raises(ValueError):
            jp.jpeg_roundtrip_u8(img, bad)
    with pytest.raises(ValueError):
        jp.jpeg_roundtrip_u8(img[..., :2], 50)
    with pytest.raises(ValueError):
        jp.jpeg_roundtrip_u8(np.zeros((1, 1025, 3), np.uint8), 50)
    with pytest.raises(ValueError):
        jp.jpeg_roundtrip_u8(img.astype(np.int32), 50)


def test_quant_tables():
    lum, chrom = jp.quant_tables(50)
    assert np.array_equal(lum, jp.STD_LUMINANCE) and np.array_equal(chrom, jp.STD_CHROMINANCE)
    lum, chrom = jp.quant_tables(100)
    assert (lum == 1).all() and (chrom == 1).all()
    lum, chrom = jp.quant_tables(1)
    assert (lum == 255).all() and (chrom == 255).all()
    lum, chrom = jp.quant_tables(24)                     # scale 208
    assert lum.max() == 252 and lum[2] == 21 and chrom[0] == 35 and chrom.max() == 206
    lum, chrom = jp.quant_tables(5)                      # scale 1000: force_baseline clamps every entry above 25 (45 of luminance, 58 of chrominance)
    assert lum[:4].tolist() == [160, 110, 100, 160] and lum[8:12].tolist() == [120, 120, 140, 190] and lum.max() == 255
    assert int((lum == 255).sum()) == 45 and chrom[:3].tolist() == [170, 180, 240] and int((chrom == 255).sum()) == 58
    lum, _ = jp.quant_tables(75)
    assert lum[:4].tolist() == [8, 6, 5, 8]


class _Spy(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def getrandbits(self, k):                            # (defined here so that randint keeps drawing bits, as random.Random does)
        return super().getrandbits(k)

    def random(self):
        v = super().random()
        self.calls.append(("random", v))
        return v

    def randint(self, a, b):
        n = len(self.calls)
        v = super().randint(a, b)
        del self.calls[n:]                               # (randint may be built on other methods of the class)
        self.calls.append(("randint", a, b, v))
        return v


def test_draw_jpeg_order_and_ranges():
    spy = _Spy(7)
    q = jp.draw_jpeg(200, 30, 95, 0.5, rng=spy)
    assert q.dtype == np.int32 and q.shape == (200,)
    it = iter(spy.calls)
    for v in q.tolist():
        c = next(it)
        assert c[0] == "random"
        if c[1] < 0.5:
            r = next(it)
            assert r[:3] == ("randint", 30, 95) and r[3] == v and 30 <= v <= 95
        else:
            assert v == 0
    assert next(it, None) is None
    assert 0 < int((q == 0).sum()) < 200 and q.max() > 80 and q[q > 0].min() < 45
    ref = random.Random(7)                               # the same stream by hand
    want = [ref.randint(30, 95) if ref.random() < 0.5 else 0 for _ in range(200)]
    assert q.tolist() == want
    assert (jp.draw_jpeg(50, 30, 95, 0.0, rng=random.Random(1)) == 0).all()
    one = jp.draw_jpeg(50, 40, 40, 1.0, rng=random.Random(1))
    assert (one == 40).all()
    assert (jp.draw_jpeg(50, 1, 100, 1.0, rng=random.Random(2)) > 0).all()
    random.seed(5)
    a = jp.draw_jpeg(8, 10, 20, 0.5)                     # Python's `random` module by default
    random.seed(5)
    assert a.tolist() == jp.draw_jpeg(8, 10, 20, 0.5).tolist()


def test_collate_needs_degrade_for_jpeg():
    from dpmn_amd.dataset import textzoom as tz
    with pytest.raises(ValueError, match="jpeg=.* needs degrade=True"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, jpeg=(30, 95, 0.5))
    with pytest.raises(ValueError, match="lo <= hi"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True, jpeg=(95, 30, 0.5))
    col = tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True, jpeg=(30, 95, 0.25))
    assert col.jpeg == (30, 95, 0.25)
    assert tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, degrade=True).jpeg is None
    assert tz.alignCollate_realWTLAMask().jpeg is None


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_jpeg", os.path.join(os.path.dirname(HERE), "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_exits_with_one_clear_line():
    m = _main()

    def run(**kw):
        a = dict(cutblur=False, manmade_degrade=True, train_hr_dir=None, jpeg_degrade=None, jpeg_prob=0.5)
        a.update(kw)
        with pytest.raises(SystemExit) as e:
            m.main(SimpleNamespace(), SimpleNamespace(**a))
        assert "\n" not in str(e.value)
        return str(e.value)

    assert run(jpeg_degrade="30,95", manmade_degrade=False).startswith("main.py: --jpeg_degrade needs --manmade_degrade")
    assert "LO <= HI" in run(jpeg_degrade="95,30")
    assert "1 <= LO" in run(jpeg_degrade="0,50")
    assert "<= 100" in run(jpeg_degrade="50,101")
    assert "two integers" in run(jpeg_degrade="50")
    assert "two integers" in run(jpeg_degrade="a,b")
    assert "--jpeg_prob" in run(jpeg_degrade="30,95", jpeg_prob=1.5)
    assert "--jpeg_prob" in run(jpeg_degrade="30,95", jpeg_prob=-0.1)
    assert jp.jpeg_setting(SimpleNamespace(jpeg_degrade="40,40", jpeg_prob=None)) == (40, 40, 0.5)
    assert jp.jpeg_setting(SimpleNamespace(jpeg_degrade=None, jpeg_prob=7)) is None and jp.jpeg_setting(SimpleNamespace()) is None


def test_fingerprint_with_and_without_the_field():
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))

    def args(**kw):
        a = dict(arch="tsrn", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="2,", embed_dim="96,", depths="1,",
                 num_heads="6,", window_size="2,4,8,", mlp_ratio="4,", manmade_degrade=True)
        a.update(kw)
        return SimpleNamespace(**a)

    off = base.state_fingerprint(args(), cfg)
    assert off["jpeg_degrade"] is None and "jpeg_degrade" in base.FINGERPRINT_FIELDS and "jpeg_degrade" in base.DATA_FIELDS
    on = base.state_fingerprint(args(jpeg_degrade="30,95", jpeg_prob=0.5), cfg)
    assert on["jpeg_degrade"] == [30, 95, 0.5]
    old = {k: v for k, v in off.items() if k != "jpeg_degrade"}      # a state written before the field existed
    base.check_fingerprint(old, off)
    base.check_fingerprint(off, off)
    base.check_fingerprint(on, base.state_fingerprint(args(jpeg_degrade="30,95"), cfg))      # --jpeg_prob's default
    base.check_fingerprint({**on, "jpeg_degrade": (30, 95, 0.5)}, on)                       # a tuple after a reload is the same setting
    for saved, current in ((old, on), (off, on), (on, off), (on, base.state_fingerprint(args(jpeg_degrade="30,90"), cfg)),
                           (on, base.state_fingerprint(args(jpeg_degrade="30,95", jpeg_prob=0.25), cfg))):
        with pytest.raises(ValueError, match="jpeg_degrade"):
            base.check_fingerprint(saved, current)


if __name__ == "__main__":
    print(write_fixture(), os.path.getsize(FIXTURE), "bytes")
