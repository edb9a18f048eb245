"""Projective distortion, rotation and the curved baseline rendered on the GPU (csrc/render.hip k_render_words_warp through
ops.render_words_warp_u8) against the NumPy restatement utils.render.render_warp_u8, byte for byte, in one batch on every edge and in
both compute modes; a batch of one; what the entry point refuses; a --train_words batch with all kinds through get_train_data and
sr_batches."""
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import render as rd
from dpmn_amd.utils.resize import pack_ragged, pil_resize_u8

pytestmark = pytest.mark.gpu

WORDS = ["hello", "World", "a", "x" * 25, "it's", "42nd"]
_REF = {}


def _row(at, word, font, case, gh, spacing, margins, shear, style, seed, fg=(200, 30, 90), bg=(10, 220, 130), bg2=(250, 120, 0)):
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.FONT], row[rd.CASE], row[rd.GH], row[rd.SPACING], row[rd.SHEAR], row[rd.STYLE], row[rd.SEED] = font, case, gh, spacing, shear, style, seed
    row[rd.M_LEFT:rd.M_BOTTOM + 1] = margins
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3], row[rd.BG2:rd.BG2 + 3] = fg, bg, bg2
    return rd.word_classes(word), row


def _fx(**kw):
    row = np.zeros(rd.N_FX, np.int64)
    for k, v in kw.items():
        c = getattr(rd, "FX_" + k)
        row[c:c + np.size(v)] = v
    return row


def _warp(at, cls, row, flags, amp=0.0, angle=0.0, jit=0.0, size=None):
    """-> (params row, warp row): amp and jit in glyph heights (every corner moves by jit * gh in x and y, clipped to a quarter of the
    canvas side as draw_render_warp clips it), angle in degrees; size = (H, W): the left and the bottom margin are chosen so that
    render_warp_meta gives exactly this canvas"""
    def make(r):
        gh = int(r[rd.GH])
        h0, w0 = rd.layout(cls, r, at)[:2]
        a = int(amp * gh * 65536)
        hb = h0 + ((abs(a) + 65535) >> 16)
        lx, ly = min(abs(jit) * gh, w0 / 4.0), min(abs(jit) * gh, hb / 4.0)
        sg = 1.0 if jit >= 0 else -1.0
        return rd.warp_row(h0, w0, flags, a, angle, [(sg * lx, sg * ly), (-sg * lx, sg * ly), (sg * lx, -sg * ly), (sg * lx, sg * ly)])
    if size is None:
        return row, make(row)
    for left in range(0, 300):
        for bottom in range(0, 12):
            r = row.copy()
            r[rd.M_LEFT], r[rd.M_BOTTOM] = left, bottom
            wr = make(r)
            if (int(wr[rd.WP_H]), int(wr[rd.WP_W])) == tuple(size):
                return r, wr
    raise AssertionError("no margins give the canvas %r" % (size,))


def _batch():
    """Seventeen samples on every edge of the warp kernel, their restatement images and pack_ragged pair: made once, never changed.
    Two atlases (PIL's built-in font at the base heights 64 and 40); a pool of two photos."""
    if not _REF:
        at = rd.build_atlases(None, [64, 40])
        rng = np.random.RandomState(5)
        pool = rd.Backgrounds([rng.randint(0, 256, (40, 300, 3)).astype(np.uint8), rng.randint(0, 256, (9, 13, 3)).astype(np.uint8)])
        S = rd.SHEAR_MAX
        P, A, C = rd.PERSP_MAX, rd.ANGLE_MAX, rd.CURVE_MAX
        full = dict(FLAGS=7, R=3, OUTLINE=(255, 255, 40), DX=-3, DY=3, Q=200, SHADOW=(20, 0, 60), PHOTO=0, X0=10, Y0=5, CW=290, CH=35, M=150)
        #        word      font case gh spacing margins (l, r, t, b) shear style seed     fx row     flags amp angle jitter [canvas]
        rows = [(("i", 0, 0, 24, 0, (0, 0, 0, 0), 0, 0, 1), _fx(FLAGS=1, R=3, OUTLINE=(255, 255, 40)), dict(flags=7, amp=C, angle=A, jit=0.05)),   # one letter, zero margins
                (("x" * 25, 0, 1, 64, 4, (16, 16, 16, 16), S, 1, 2 ** 63 - 1), _fx(**full), dict(flags=7, amp=-C, angle=-A, jit=-P)),               # 25 letters, many tiles, everything on
                (("Word", 0, 2, 40, 2, (1, 0, 0, 0), 0, 1, 5), _fx(), dict(flags=0)),                                                              # flags 0 between warped ones
                (("gpu", 0, 0, 30, 1, (2, 1, 0, 3), S, 0, 7), _fx(), dict(flags=1, jit=P)),                                                        # each kind alone, both signs, shear at both limits
                (("gpu", 0, 0, 30, 1, (2, 1, 0, 3), -S, 0, 8), _fx(FLAGS=2, DX=3, DY=3, Q=96, SHADOW=(255, 255, 255)), dict(flags=1, jit=-P)),
                (("a1", 1, 0, 24, -1, (0, 5, 0, 6), S, 2, 4), _fx(), dict(flags=2, angle=A)),
                (("a1", 1, 0, 24, -1, (0, 5, 0, 6), -S, 2, 4), _fx(FLAGS=1, R=2, OUTLINE=(0, 0, 0)), dict(flags=2, angle=-A)),
                (("q0", 0, 1, 64, 4, (0, 1, 16, 0), S, 2, 9), _fx(), dict(flags=4, amp=C)),
                (("q0", 0, 1, 64, 4, (0, 1, 16, 0), -S, 2, 9), _fx(FLAGS=4, PHOTO=1, X0=0, Y0=0, CW=13, CH=9, M=224), dict(flags=4, amp=-C)),
                (("wm" * 12, 1, 2, 48, -1, (3, 0, 7, 1), -S, 2, 3), _fx(FLAGS=1, R=1, OUTLINE=(9, 9, 9)), dict(flags=7, amp=C, angle=5.0, jit=0.1)),  # overlapping glyphs
                # the tile edges (hand-made rows: gh below 24); an odd width behind an odd width: the row starts are not dword-aligned
                (("tile", 0, 0, 6, 0, (0, 0, 0, 0), 0, 1, 10), _fx(), dict(flags=4, amp=0.1, size=(7, 127))),
                (("tile", 0, 0, 7, 1, (0, 0, 0, 0), 3000, 0, 12), _fx(FLAGS=2, DX=0, DY=-2, Q=200, SHADOW=(20, 0, 60)), dict(flags=5, amp=-0.1, jit=0.05, size=(9, 129))),
                (("tile", 1, 1, 6, 0, (0, 2, 0, 0), 0, 2, 11), _fx(), dict(flags=2, angle=0.3, size=(8, 128))),
                (("edge", 0, 0, 13, 0, (0, 0, 1, 0), 0, 0, 13), _fx(FLAGS=1, R=3, OUTLINE=(0, 80, 255)), dict(flags=4, amp=-0.1, size=(16, 255))),
                (("edge", 1, 2, 13, 0, (0, 0, 1, 0), -2000, 1, 14), _fx(), dict(flags=6, amp=0.05, angle=-0.2, size=(17, 257))),
                (("it's", 1, 1, 40, 0, (0, 0, 2, 2), 0, 0, 6), _fx(), dict(flags=3, angle=-12.0, jit=0.2)),
                (("0123456789", 1, 0, 26, 3, (6, 6, 6, 6), 12345, 1, 8), _fx(FLAGS=1, R=1, OUTLINE=(1, 2, 3)), dict(flags=0))]                      # flags 0 behind warped samples
        n = len(rows)
        cls, lens = np.zeros((n, 25), np.int32), np.zeros(n, np.int32)
        params, fx, warp = np.zeros((n, rd.N_PARAMS), np.int64), np.stack([r[1] for r in rows]), np.zeros((n, rd.N_WARP), np.int64)
        for i, (r, _, w) in enumerate(rows):
            c, row = _row(at, *r)
            params[i], warp[i] = _warp(at, c, row, **w)
            cls[i, :len(c)], lens[i] = c, len(c)
        rd.check_render_fx(fx, pool)
        rd.check_render_warp(warp, params)
        images = [rd.render_warp_u8(cls[i, :lens[i]], params[i], fx[i], warp[i], at, pool) for i in range(n)]
        packed, meta = pack_ragged(images, pin=False)
        _REF.update(at=at, pool=pool, cls=cls, lens=lens, params=params, fx=fx, warp=warp, images=images, packed=packed, meta=meta)
    return _REF


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def test_the_batch_sits_on_every_edge():
    r = _batch()
    p, fx, wp, sizes = r["params"], r["fx"], r["warp"], [im.shape[:2] for im in r["images"]]
    assert np.array_equal(rd.render_warp_meta(r["cls"], r["lens"], p, wp, r["at"]), r["meta"].numpy())
    assert {(7, 127), (9, 129), (8, 128), (16, 255), (17, 257)} <= set(sizes)
    ws = [w for _, w in sizes]
    assert any(a % 2 and b % 2 for a, b in zip(ws, ws[1:])) and max(ws) > 3 * 128
    fl = wp[:, rd.WP_FLAGS]
    assert {0, 1, 2, 4, 7} <= set(fl) and fl[0] != 0 and fl[2] == 0 and fl[1] != 0 and fl[3] != 0 and fl[-1] == 0
    for bit in (1, 2, 4):          # each kind alone under the shear at both limits
        assert {rd.SHEAR_MAX, -rd.SHEAR_MAX} <= set(p[fl == bit, rd.SHEAR])
    amp = wp[fl == 4, rd.WP_AMP]
    assert (amp > 0).any() and (amp < 0).any() and (np.abs(wp[:, rd.WP_AMP]) == 4 * 65536 * p[:, rd.GH] // 10).sum() >= 4
    assert 25 in r["lens"] and -1 in p[fl != 0, rd.SPACING]
    i = int(np.argmax(r["lens"] == 1))
    assert p[i, rd.GH] == 24 and not p[i, rd.M_LEFT:rd.M_BOTTOM + 1].any() and fl[i] == 7
    k = int(np.argmax(r["lens"] == 25))
    assert p[k, rd.GH] == 64 and fl[k] == 7 and fx[k, rd.FX_FLAGS] == 7 and fx[k, rd.FX_R] == 3
    # flat coordinates that are negative on the left AND the top (the kernel must floor, C++ truncates), with a remainder
    neg = 0
    for j in np.flatnonzero(fl & 2):
        c = [int(v) for v in wp[j, rd.WP_COEF:rd.WP_COEF + 9]]
        den = c[6] + c[7] + 2 * c[8]
        nx, ny = (c[0] + c[1] + 2 * c[2]) * 65536, (c[3] + c[4] + 2 * c[5]) * 65536          # the first pixel's centre
        for num in (nx, ny):
            neg += num < 0 and num % den != 0
    assert neg >= 2
    # the warp changes bytes wherever it is on; a row of zeros gives render_fx_u8's image
    for j in range(len(sizes)):
        flat = rd.render_fx_u8(r["cls"][j, :r["lens"][j]], p[j], fx[j], r["at"], r["pool"])
        assert (flat.shape == r["images"][j].shape and np.array_equal(flat, r["images"][j])) == (fl[j] == 0)


def test_bytes_equal_the_restatement_in_both_compute_modes(dev):
    from dpmn_amd import _abi, ops
    from helpers import record
    r = _batch()
    packed, meta = ops.render_words_warp_u8(r["cls"], r["lens"], r["params"], r["fx"], r["warp"], r["at"], r["pool"], device=dev)
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1 and meta.dtype == torch.int64
    assert torch.equal(meta, r["meta"]) and packed.numel() == r["packed"].numel()
    got = packed.cpu().numpy()
    bad = [int((got[o:o + h * w * 3].reshape(h, w, 3) != im).sum()) for (o, h, w), im in zip(meta.tolist(), r["images"])]
    print("render warp parity: %d bytes, mismatching per image %s" % (got.size, bad))
    record("render_words_warp", "bytes differing from the NumPy restatement (of %d)" % got.size, sum(bad), 0)
    assert sum(bad) == 0, bad
    # warp rows of zeros: the fx kernel's bytes for the whole batch, and with fx rows of zeros too the plain kernel's
    zero = np.zeros_like(r["warp"])
    flat = ops.render_words_warp_u8(r["cls"], r["lens"], r["params"], r["fx"], zero, r["at"], r["pool"], device=dev)
    want = ops.render_words_fx_u8(r["cls"], r["lens"], r["params"], r["fx"], r["at"], r["pool"], device=dev)
    assert torch.equal(flat[1], want[1]) and torch.equal(flat[0], want[0])
    plain = ops.render_words_warp_u8(r["cls"], r["lens"], r["params"], np.zeros_like(r["fx"]), zero, r["at"], None, device=dev)[0]
    assert torch.equal(plain, ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device=dev)[0])
    # the other compute mode (this test runs in both passes of the suite): integer arithmetic, the same bytes
    old = _abi.lib.dpmn_get_compute_dtype()
    _abi.check(_abi.lib.dpmn_set_compute_dtype(0 if old == 2 else 2))
    try:
        other = ops.render_words_warp_u8(torch.from_numpy(r["cls"]), torch.from_numpy(r["lens"]), torch.from_numpy(r["params"]),
                                         torch.from_numpy(r["fx"]), torch.from_numpy(r["warp"]), r["at"], r["pool"], device=dev)[0]
    finally:
        _abi.check(_abi.lib.dpmn_set_compute_dtype(old))
    assert torch.equal(other, packed)


def test_a_batch_of_one_and_the_bytes_around_it(dev):
    from dpmn_amd import ops
    r = _batch()
    for k in (1, 11):          # everything on over many tiles, and the 9 x 129 canvas
        im = r["images"][k]
        one = torch.full((im.size + 512,), 0x5A, dtype=torch.uint8, device=dev)
        got, meta = ops.render_words_warp_u8(r["cls"][k:k + 1], r["lens"][k:k + 1], r["params"][k:k + 1], r["fx"][k:k + 1], r["warp"][k:k + 1],
                                             r["at"], r["pool"], device=dev, out=one)
        assert got is one and meta.tolist() == [[0, im.shape[0], im.shape[1]]]
        host = one.cpu().numpy()
        assert np.array_equal(host[:im.size].reshape(im.shape), im) and (host[im.size:] == 0x5A).all()


def test_bad_rows_are_rejected(dev):
    from dpmn_amd import _abi, ops
    r = _batch()
    call = lambda warp, **kw: ops.render_words_warp_u8(r["cls"], r["lens"], r["params"], r["fx"], warp, r["at"], r["pool"], **dict(dict(device=dev), **kw))
    for row, col, val in ((0, rd.WP_FLAGS, 8), (0, rd.WP_COEF + 2, rd.COEF_MAX + 1), (1, rd.WP_COEF + 8, 0), (7, rd.WP_AMP, 2 ** 23),
                          (7, rd.WP_ROOM, 0), (3, rd.WP_AMP, 5), (5, rd.WP_H, 0), (5, 15, 1)):
        warp = r["warp"].copy()
        warp[row, col] = val
        with pytest.raises(_abi.DpmnError, match="render_warp"):
            call(warp)
    with pytest.raises(_abi.DpmnError, match="one row per sample"):
        call(r["warp"][:-1])
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        call(r["warp"], device="cpu")
    with pytest.raises(_abi.DpmnError, match="out must be"):
        call(r["warp"], out=torch.zeros(16, dtype=torch.uint8, device=dev))
    # the entry point refuses the same rows by itself: den <= 0 at a corner, handed over behind the Python checks
    import ctypes
    k = 5
    sl = slice(k, k + 1)
    cls, lens, par, fx = r["cls"][sl].copy(), r["lens"][sl].copy(), r["params"][sl].copy(), r["fx"][sl].copy()
    for col, val, msg in ((rd.WP_COEF + 8, 0, "den <= 0"), (rd.WP_COEF + 1, rd.COEF_MAX + 1, "passes 2\\^30"), (rd.WP_AMP, 9, "amp outside")):
        warp = r["warp"][sl].copy()
        m = np.concatenate((rd.render_warp_meta(cls, lens, par, warp, r["at"]), [[0]]), axis=1)
        warp[0, col] = val
        tiles, _ = ops._tile_table(m[:, 1], m[:, 2], *ops.RENDER_TILE)
        tab = r["pool"].table
        d_ = lambda a: torch.from_numpy(a).to(dev)
        dv = [d_(a) for a in (cls, lens, par, fx, warp, r["at"].alpha, r["at"].advance, r["at"].height, m, tiles, r["pool"].pixels, tab)]
        out = torch.zeros(int(m[0, 1] * m[0, 2] * 3), dtype=torch.uint8, device=dev)
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = _abi.lib.dpmn_render_words_warp_u8(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(),
                                                dv[5].data_ptr(), dv[6].data_ptr(), dv[7].data_ptr(), dv[8].data_ptr(), dv[9].data_ptr(),
                                                tiles.shape[0], dv[10].data_ptr(), dv[10].numel(), dv[11].data_ptr(), tab.shape[0],
                                                out.data_ptr(), out.numel(), 1, r["at"].n_fonts, r["at"].alpha.shape[3], r["at"].alpha.shape[4],
                                                hp(cls), hp(lens), hp(par), hp(fx), hp(warp), hp(m), hp(tab), _abi.stream())
        assert rc != 0
        with pytest.raises(_abi.DpmnError, match=msg):
            _abi.check(rc)
        torch.cuda.synchronize()
        assert not out.any()


# ------------------------------------------------------------------------------------------------------------------- end to end
def _u8(x):
    """the bytes before the / 255 of a collated batch (channels 0 .. 2) as (B, h, w, 3)"""
    return (x[:, :3] * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def test_train_words_batch_with_all_kinds_equals_the_restatement(dev):
    """get_train_data(train_words=(words, atlases, epoch, fx, warp)) with every fx and warp kind on for every sample, one batch through
    sr_batches: the labels are the drawn words and the HR bytes are the restatement of the drawn rows, resized by PIL's bicubic"""
    from dpmn_amd import workload
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.interfaces.super_resolution import TextSR
    from helpers import record
    r = _batch()
    at, pool = r["at"], r["pool"]
    fx = rd.RenderFx(rd.FX_KINDS, 1.0, pool, at)
    warp = rd.RenderWarp(rd.WARP_KINDS, 1.0, atlases=at)
    B = 4
    args = workload.make_args("tatt", 2, 2, B)
    args.train_words, args.cutblur = "words.txt", True
    sr = TextSR(workload.make_config(B), args)
    dl = sr.get_train_data(train_words=(WORDS, at, 6, fx, warp))[1]
    assert dl.collate_fn.render and dl.collate_fn.render_fx is fx and dl.collate_fn.render_warp is warp and len(dl.dataset) == 6
    random.seed(21)
    state = random.getstate()
    (hr, lr, _, labels), = list(tz.sr_batches(dl, sr.device, sr.mask))
    assert hr.shape == (B, 4, 32, 128) and lr.shape == (B, 4, 16, 64) and hr.is_cuda
    random.setstate(state)
    rng = random.Random(random.getrandbits(63))
    want, cls, lens, params, rows, wrows = rd.draw_render_warp(WORDS, at.n_fonts, rng, B, fx, warp)
    assert labels == want and (rows[:, rd.FX_FLAGS] == 7).all() and (wrows[:, rd.WP_FLAGS] == 7).all()
    high = np.stack([pil_resize_u8(rd.render_warp_u8(cls[i, :lens[i]], params[i], rows[i], wrows[i], at, pool), 32, 128) for i in range(B)])
    d_hr = int((_u8(hr) != high).sum())
    print("words warp end to end: HR bytes differing %d of %d" % (d_hr, high.size))
    record("render_words_warp", "HR bytes of sr_batches differing from the restatement (of %d)" % high.size, d_hr, 0)
    assert d_hr == 0
    # warp alone (no fx item), and a loader without the fifth item
    alone = sr.get_train_data(train_words=(WORDS, at, 6, None, warp))[1]
    assert alone.collate_fn.render_fx is None and alone.collate_fn.render_warp is warp
    assert sr.get_train_data(train_words=(WORDS, at, 6, fx))[1].collate_fn.render_warp is None
