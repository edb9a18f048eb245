"""Outline, drop shadow and photo backgrounds rendered on the GPU (csrc/render.hip k_render_words_fx through ops.render_words_fx_u8)
against the NumPy restatement utils.render.render_fx_u8, byte for byte, in one batch on every edge and in both compute modes; a batch
of one; what the entry point refuses; a --train_words batch with all three kinds through get_train_data and sr_batches."""
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import render as rd
from dpmn_amd.utils.resize import pack_ragged, pil_resize_u8

pytestmark = pytest.mark.gpu

WORDS = ["hello", "World", "a", "x" * 25, "it's", "42nd"]
_REF = {}


def _row(at, word, font, case, gh, spacing, margins, shear, style, seed, width=None, fg=(200, 30, 90), bg=(10, 220, 130), bg2=(250, 120, 0)):
    """-> (classes, params row); width: the left margin is chosen so that the canvas has exactly this width"""
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.FONT], row[rd.CASE], row[rd.GH], row[rd.SPACING], row[rd.SHEAR], row[rd.STYLE], row[rd.SEED] = font, case, gh, spacing, shear, style, seed
    row[rd.M_LEFT:rd.M_BOTTOM + 1] = margins
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3], row[rd.BG2:rd.BG2 + 3] = fg, bg, bg2
    cls = rd.word_classes(word)
    if width is not None:
        row[rd.M_LEFT] += width - rd.layout(cls, row, at)[1]
        assert row[rd.M_LEFT] >= 0 and rd.layout(cls, row, at)[1] == width
    return cls, row


def _fx(**kw):
    row = np.zeros(rd.N_FX, np.int64)
    for k, v in kw.items():
        c = getattr(rd, "FX_" + k)
        row[c:c + np.size(v)] = v
    return row


def _batch():
    """Sixteen samples on every edge of the fx kernel, their restatement images and pack_ragged pair: made once, never changed.  Two
    atlases (PIL's built-in font at the base heights 64 and 40); a pool of three photos: noise 40 x 300, noise 9 x 13, one pixel."""
    if not _REF:
        at = rd.build_atlases(None, [64, 40])
        rng = np.random.RandomState(5)
        pool = rd.Backgrounds([rng.randint(0, 256, (40, 300, 3)).astype(np.uint8), rng.randint(0, 256, (9, 13, 3)).astype(np.uint8),
                               np.full((1, 1, 3), (7, 200, 90), np.uint8)])
        S = rd.SHEAR_MAX
        out, sh = dict(R=3, OUTLINE=(255, 255, 40)), dict(Q=200, SHADOW=(20, 0, 60))
        #         word      font case gh spacing margins (l, r, t, b) shear style seed [width]      the fx row
        rows = [(("Word", 0, 2, 40, 2, (1, 0, 0, 0), 0, 1, 5), _fx()),                                             # flags 0
                (("i", 0, 0, 24, 0, (0, 0, 0, 0), 0, 0, 1), _fx(FLAGS=1, **out)),                                  # r = 3, clipped on every side
                (("wm" * 12, 1, 2, 64, -1, (3, 0, 7, 1), -S, 2, 3), _fx(FLAGS=1, R=2, OUTLINE=(0, 0, 0))),         # overlapping glyphs under an outline
                (("gpu", 0, 0, 30, 1, (2, 1, 0, 3), S, 0, 7), _fx(FLAGS=2, DX=3, DY=3, **sh)),                     # shear at both ends, the four corners
                (("gpu", 0, 0, 30, 1, (2, 1, 0, 3), -S, 0, 8), _fx(FLAGS=2, DX=-3, DY=-3, **sh)),
                (("a1", 1, 0, 24, -1, (0, 5, 0, 6), S, 2, 4), _fx(FLAGS=3, DX=-3, DY=3, Q=255, SHADOW=(0, 0, 0), R=1, OUTLINE=(9, 9, 9))),
                (("q", 0, 1, 64, 4, (0, 1, 16, 0), -S, 2, 9), _fx(FLAGS=2, DX=3, DY=-3, Q=96, SHADOW=(255, 255, 255))),
                # the tile edges: widths 127 / 128 / 129, heights 7 / 8 / 9 (hand-made rows: gh below 24), then 16 / 17 rows
                (("tile", 0, 0, 7, 0, (0, 0, 0, 0), 0, 1, 10, 127), _fx(FLAGS=7, PHOTO=0, X0=0, Y0=0, CW=300, CH=16, M=64, DX=1, DY=0, **out, **sh)),
                (("tile", 1, 1, 8, 0, (0, 2, 0, 0), 0, 2, 11, 128), _fx(FLAGS=5, PHOTO=1, X0=0, Y0=0, CW=13, CH=9, M=224, **out)),
                (("tile", 0, 0, 9, 1, (0, 0, 0, 0), 3000, 0, 12, 129), _fx(FLAGS=6, PHOTO=0, X0=171, Y0=31, CW=129, CH=9, M=150, DX=0, DY=-2, **sh)),
                (("edge", 0, 0, 14, 0, (0, 0, 1, 1), 0, 0, 13, 256), _fx(FLAGS=7, PHOTO=0, X0=44, Y0=24, CW=256, CH=16, M=100, DX=-2, DY=1, **out, **sh)),
                (("edge", 1, 2, 13, 0, (0, 0, 2, 2), -2000, 1, 14, 257), _fx(FLAGS=4, PHOTO=0, X0=0, Y0=3, CW=128, CH=8, M=224)),
                (("x" * 25, 0, 1, 64, 4, (16, 16, 16, 16), S, 1, 2 ** 63 - 1), _fx(FLAGS=7, PHOTO=0, X0=10, Y0=5, CW=290, CH=35, M=64, DX=2, DY=2,
                                                                                  R=2, OUTLINE=(0, 80, 255), **sh)),   # 25 letters, many tiles, the crop reaches the photo's right and bottom edge and is smaller than the canvas
                (("it's", 1, 1, 40, 0, (0, 0, 2, 2), 0, 0, 6), _fx(FLAGS=5, PHOTO=2, X0=0, Y0=0, CW=1, CH=1, M=224, R=1, OUTLINE=(255, 0, 0))),      # the single pixel
                (("i", 0, 0, 24, 0, (0, 0, 0, 0), 0, 2, 15), _fx(FLAGS=4, PHOTO=1, X0=3, Y0=1, CW=10, CH=8, M=64)),                                 # a crop larger than the canvas
                (("0123456789", 1, 0, 26, 3, (6, 6, 6, 6), 12345, 1, 8), _fx())]                                    # flags 0 behind fx samples
        n = len(rows)
        cls, lens = np.zeros((n, 25), np.int32), np.zeros(n, np.int32)
        params, fx = np.zeros((n, rd.N_PARAMS), np.int64), np.stack([r[1] for r in rows])
        for i, (r, _) in enumerate(rows):
            c, params[i] = _row(at, *r)
            cls[i, :len(c)], lens[i] = c, len(c)
        rd.check_render_fx(fx, pool)
        images = [rd.render_fx_u8(cls[i, :lens[i]], params[i], fx[i], at, pool) for i in range(n)]
        packed, meta = pack_ragged(images, pin=False)
        _REF.update(at=at, pool=pool, cls=cls, lens=lens, params=params, fx=fx, images=images, packed=packed, meta=meta)
    return _REF


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def test_the_batch_sits_on_every_edge():
    r = _batch()
    p, fx, sizes = r["params"], r["fx"], [im.shape[:2] for im in r["images"]]
    assert {(7, 127), (8, 128), (9, 129)} <= set(sizes) and {256, 257} <= {w for _, w in sizes} and {16, 17} <= {h for h, _ in sizes}
    assert set(fx[:, rd.FX_FLAGS]) == set(range(8)) and {1, 2, 3} <= set(fx[fx[:, 0] & 1 > 0, rd.FX_R])
    shadows = fx[fx[:, 0] & 2 > 0]
    assert {(3, 3), (-3, -3), (-3, 3), (3, -3)} <= {(int(a), int(b)) for a, b in shadows[:, rd.FX_DX:rd.FX_DY + 1]}
    assert {rd.SHEAR_MAX, -rd.SHEAR_MAX} <= set(p[fx[:, 0] & 2 > 0, rd.SHEAR]) and {96, 255} <= set(shadows[:, rd.FX_Q])
    tex = fx[:, 0] & 4 > 0
    assert {rd.M_MIN, rd.M_MAX} <= set(fx[tex, rd.FX_M]) and set(fx[tex, rd.FX_PHOTO]) == {0, 1, 2}
    ws = np.asarray([w for _, w in sizes])
    assert (fx[tex, rd.FX_CW] < ws[tex]).any() and (fx[tex, rd.FX_CW] > ws[tex]).any() and (fx[tex, rd.FX_CW] == ws[tex]).any()
    tab = r["pool"].table[fx[:, rd.FX_PHOTO]]
    assert (tex & (fx[:, rd.FX_X0] + fx[:, rd.FX_CW] == tab[:, 2]) & (fx[:, rd.FX_Y0] + fx[:, rd.FX_CH] == tab[:, 1])).any()
    assert 25 in r["lens"] and 1 in r["lens"] and -1 in p[fx[:, 0] & 1 > 0, rd.SPACING] and max(ws) > 3 * 128
    i = int(np.argmax((r["lens"] == 1) & (fx[:, rd.FX_R] == 3)))
    assert p[i, rd.GH] == 24 and not p[i, rd.M_LEFT:rd.M_BOTTOM + 1].any()
    # the fx stages change bytes wherever they are on
    for k in range(len(sizes)):
        plain = rd.render_u8(r["cls"][k, :r["lens"][k]], p[k], r["at"])
        assert np.array_equal(plain, r["images"][k]) == (fx[k, 0] == 0)


def test_bytes_equal_the_restatement_in_both_compute_modes(dev):
    from dpmn_amd import _abi, ops
    from helpers import record
    r = _batch()
    packed, meta = ops.render_words_fx_u8(r["cls"], r["lens"], r["params"], r["fx"], r["at"], r["pool"], device=dev)
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1 and meta.dtype == torch.int64
    assert torch.equal(meta, r["meta"]) and packed.numel() == r["packed"].numel()
    got = packed.cpu().numpy()
    bad = [int((got[o:o + h * w * 3].reshape(h, w, 3) != im).sum()) for (o, h, w), im in zip(meta.tolist(), r["images"])]
    print("render fx parity: %d bytes, mismatching per image %s" % (got.size, bad))
    record("render_words_fx", "bytes differing from the NumPy restatement (of %d)" % got.size, sum(bad), 0)
    assert sum(bad) == 0, bad
    # the samples with flags 0 are the plain kernel's images
    plain, pmeta = ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device=dev)
    assert torch.equal(pmeta, meta)
    plain = plain.cpu().numpy()
    zero = [k for k in range(len(r["images"])) if r["fx"][k, 0] == 0]
    assert len(zero) >= 2
    for k in zero:
        o, h, w = meta[k].tolist()
        assert np.array_equal(got[o:o + h * w * 3], plain[o:o + h * w * 3])
    # rows of zeros and no pool at all: the plain kernel's bytes for the whole batch
    none = ops.render_words_fx_u8(r["cls"], r["lens"], r["params"], np.zeros_like(r["fx"]), r["at"], None, device=dev)[0]
    assert np.array_equal(none.cpu().numpy(), plain)
    # the other compute mode (this test runs in both passes of the suite): integer arithmetic, the same bytes
    old = _abi.lib.dpmn_get_compute_dtype()
    _abi.check(_abi.lib.dpmn_set_compute_dtype(0 if old == 2 else 2))
    try:
        other = ops.render_words_fx_u8(torch.from_numpy(r["cls"]), torch.from_numpy(r["lens"]), torch.from_numpy(r["params"]),
                                       torch.from_numpy(r["fx"]), r["at"], r["pool"], device=dev)[0]
    finally:
        _abi.check(_abi.lib.dpmn_set_compute_dtype(old))
    assert torch.equal(other, packed)


def test_a_batch_of_one_and_the_bytes_around_it(dev):
    from dpmn_amd import ops
    r = _batch()
    for k in (7, 12):          # all three kinds: the 7 x 127 canvas, and the 25 letters
        im = r["images"][k]
        one = torch.full((im.size + 512,), 0x5A, dtype=torch.uint8, device=dev)
        got, meta = ops.render_words_fx_u8(r["cls"][k:k + 1], r["lens"][k:k + 1], r["params"][k:k + 1], r["fx"][k:k + 1], r["at"], r["pool"],
                                           device=dev, out=one)
        assert got is one and meta.tolist() == [[0, im.shape[0], im.shape[1]]]
        host = one.cpu().numpy()
        assert np.array_equal(host[:im.size].reshape(im.shape), im) and (host[im.size:] == 0x5A).all()


def test_bad_rows_are_rejected(dev):
    from dpmn_amd import _abi, ops
    r = _batch()
    call = lambda fx, pool=r["pool"], **kw: ops.render_words_fx_u8(r["cls"], r["lens"], r["params"], fx, r["at"], pool, **dict(dict(device=dev), **kw))
    for row, col, val in ((1, rd.FX_R, 4), (1, rd.FX_FLAGS, 8), (3, rd.FX_DX, 4), (6, rd.FX_Q, 95), (7, rd.FX_X0, 1), (7, rd.FX_PHOTO, 3),
                          (8, rd.FX_M, 225), (8, rd.FX_CH, 10), (0, 19, 1)):
        fx = r["fx"].copy()
        fx[row, col] = val
        with pytest.raises(_abi.DpmnError):
            call(fx)
    with pytest.raises(_abi.DpmnError, match="no pool"):
        call(r["fx"], None)
    with pytest.raises(_abi.DpmnError, match="one row per sample"):
        call(r["fx"][:-1])
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        call(r["fx"], device="cpu")
    with pytest.raises(_abi.DpmnError, match="out must be"):
        call(r["fx"], out=torch.zeros(16, dtype=torch.uint8, device=dev))
    # the entry point refuses the same rows by itself: a crop that leaves its photo, handed over behind the Python checks
    import ctypes
    k = 8
    m = np.concatenate((rd.render_meta(r["cls"][k:k + 1], r["lens"][k:k + 1], r["params"][k:k + 1], r["at"]), [[0]]), axis=1)
    fx = r["fx"][k:k + 1].copy()
    fx[0, rd.FX_CW] = 14
    tiles, _ = ops._tile_table(m[:, 1], m[:, 2], *ops.RENDER_TILE)
    cls, lens, par, tab = r["cls"][k:k + 1].copy(), r["lens"][k:k + 1].copy(), r["params"][k:k + 1].copy(), r["pool"].table
    d_ = lambda a: torch.from_numpy(a).to(dev)
    dv = [d_(a) for a in (cls, lens, par, fx, r["at"].alpha, r["at"].advance, r["at"].height, m, tiles, r["pool"].pixels, tab)]
    out = torch.zeros(int(m[0, 1] * m[0, 2] * 3), dtype=torch.uint8, device=dev)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = _abi.lib.dpmn_render_words_fx_u8(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), dv[5].data_ptr(),
                                          dv[6].data_ptr(), dv[7].data_ptr(), dv[8].data_ptr(), tiles.shape[0], dv[9].data_ptr(), dv[9].numel(),
                                          dv[10].data_ptr(), tab.shape[0], out.data_ptr(), out.numel(), 1, r["at"].n_fonts,
                                          r["at"].alpha.shape[3], r["at"].alpha.shape[4], hp(cls), hp(lens), hp(par), hp(fx), hp(m), hp(tab),
                                          _abi.stream())
    assert rc != 0
    with pytest.raises(_abi.DpmnError, match="crop leaves its photo"):
        _abi.check(rc)
    torch.cuda.synchronize()
    assert not out.any()


# ------------------------------------------------------------------------------------------------------------------- end to end
def _u8(x):
    """the bytes before the / 255 of a collated batch (channels 0 .. 2) as (B, h, w, 3)"""
    return (x[:, :3] * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def test_train_words_batch_with_all_three_kinds_equals_the_restatement(dev):
    """get_train_data(train_words=(words, atlases, epoch, fx)) with every kind on for every sample, one batch through sr_batches: the
    labels are the drawn words and the HR bytes are the restatement of the drawn rows, resized by PIL's bicubic"""
    from dpmn_amd import workload
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.interfaces.super_resolution import TextSR
    from helpers import record
    r = _batch()
    at, pool = r["at"], r["pool"]
    fx = rd.RenderFx(rd.FX_KINDS, 1.0, pool, at)
    B = 4
    args = workload.make_args("tatt", 2, 2, B)
    args.train_words, args.cutblur = "words.txt", True
    sr = TextSR(workload.make_config(B), args)
    dl = sr.get_train_data(train_words=(WORDS, at, 6, fx))[1]
    assert dl.collate_fn.render and dl.collate_fn.render_fx is fx and len(dl.dataset) == 6
    random.seed(21)
    state = random.getstate()
    (hr, lr, _, labels), = list(tz.sr_batches(dl, sr.device, sr.mask))
    assert hr.shape == (B, 4, 32, 128) and lr.shape == (B, 4, 16, 64) and hr.is_cuda
    random.setstate(state)
    rng = random.Random(random.getrandbits(63))
    want, cls, lens, params, rows = rd.draw_render_fx(WORDS, at.n_fonts, rng, B, fx)
    assert labels == want and (rows[:, rd.FX_FLAGS] == 7).all()
    high = np.stack([pil_resize_u8(rd.render_fx_u8(cls[i, :lens[i]], params[i], rows[i], at, pool), 32, 128) for i in range(B)])
    d_hr = int((_u8(hr) != high).sum())
    print("words fx end to end: HR bytes differing %d of %d" % (d_hr, high.size))
    record("render_words_fx", "HR bytes of sr_batches differing from the restatement (of %d)" % high.size, d_hr, 0)
    assert d_hr == 0
    # a loader without the fourth item renders the plain images from the same stream position
    plain = sr.get_train_data(train_words=(WORDS, at, 6))[1]
    assert plain.collate_fn.render_fx is None
