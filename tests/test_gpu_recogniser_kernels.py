"""GPU parity of the recogniser kernels -- k_lstm_step, k_gray_prep, k_maxpool2d, k_ctc_greedy, k_crnn_label_vecs (csrc/crnn.hip),
k_aster_prep, k_subsample_nhwc, k_dec_sproj / k_dec_attend / k_dec_gru / k_dec_fc / k_dec_topk (aster.hip), k_moran_rectify,
k_moran_split, k_moran_decode (moran.hip), k_vl_tokens, k_vl_pp_pool, k_vl_decode (visionlan.hip) -- each entry point called alone on
caller-owned buffers against its float64 reference (tests/ref64.py, pinned to stock torch by tests/test_ref64.py) at the smallest shapes
that cross its hand-written boundaries: 16-row tiles with 1, 15, 16, 17 and 33 rows, 1 .. 64 attention positions, 1 .. 48 / 128 / 256
classes, beam 8 x 128 classes (two passes of the candidate walk), partial blocks, leading dimensions larger than the row.  The operands
and their references come from tests/recogniser_cases.py, which asserts on the float64 reference what each case is chosen for (gate
spread, PEAKED span, "some but not all beams end"); tests/test_recogniser_cases.py does so without a GPU.

Buffers (Buf of test_gpu_small_backward.py).  Every output a kernel overwrites -- the BiLSTM's cell state and the beam search's workspace
included -- starts NaN-filled and must come back NaN-free with its sentinel row intact; a rejected call must leave every output all-NaN.

Tolerances.  check_derived of test_gpu_small_kernels.py only: 8 x the max error of the same formula evaluated in fp32 torch on the CPU
against float64, floor 1e-6.  Decision margins take twice that bound.

The exponential.  Unlike the window-attention family (test_gpu_attn_family.py), none of these kernels calls the bare hardware exponential:
sigmoid_f of common.h is 1 / (1 + expf(-x)), the softmaxes and the log-sum-exp call expf / logf, the recurrences tanhf, and the library
is built without any fast-math flag, so these are the device math library's routines (argument reduction in extended precision, the
rounding class of the host's libm), not __expf / exp2 of a product rounded to fp32.  The term 2^-24 |x| of that family's docstring is
the error of the ROUNDED PRODUCT x log2 e, which does not exist here, so no exponential term is added to the floor.  The PEAKED cases
(attention rows and pooling scores spanning about 30, the maximum on the last position) are where such a term would show: a kernel that
did use the bare instruction would be off by 30 x 2^-24 relative there; the recorded errors of those arms stand next to the fp32 CPU
yardstick's.

Discrete decisions (k_moran_decode, k_dec_topk, k_ctc_greedy, k_vl_decode).  Ids are never compared with a free-running reference, and
no case is excluded.  The float64 reference REPLAYS the kernel's own decisions (the ids; for the beam the predecessor and symbol records)
as the fed-back inputs, and three things are checked: (1) every stored logit / score / state is within the derived bound of the replayed
float64 value; (2) every decision follows from the kernel's own stored numbers by the documented rule, bit for bit (first maximum; for
the beam: stored scores best first, equal stored scores in rising flat index beam_row * n_class + class, no candidate twice); (3) every
decision agrees with float64 wherever the float64 margin exceeds twice the bound -- for the beam: no unchosen candidate's float64 score
exceeds the smallest chosen one by more than that, and the chosen ones are ordered best first within the same slack.  k_ctc_greedy and
k_vl_decode decide on their INPUT, so their outputs are compared exactly on crafted rows."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import recogniser_cases as rc
import ref64
from helpers import record
from test_gpu_small_backward import Buf, SENT, abi, both, same_bits
from test_gpu_small_kernels import check_derived, err64

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ISENT = -777
u = rc.u


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sentinel(test, what, buf):
    assert bool((buf.flat[buf.n:] == SENT).all()), "%s %s: wrote past the end of the output" % (test, what)


def untouched(test, bufs):
    for what, buf in bufs.items():
        sentinel(test, what, buf)
        assert bool(torch.isnan(buf.t).all()), "%s %s: a rejected call wrote %d elements" % (test, what, int((~torch.isnan(buf.t)).sum()))


def exact(test, what, buf, ref):
    sentinel(test, what, buf)
    got = buf.t.cpu()
    assert not bool(torch.isnan(got).any()), "%s %s: %d outputs never written" % (test, what, int(torch.isnan(got).sum()))
    assert torch.equal(got, ref.reshape(got.shape).float()), "%s %s: %d of %d outputs differ" % (test, what, int((got != ref.reshape(got.shape).float()).sum()), got.numel())


def bound_of(ref, ref32, floor=1e-6):
    """check_derived's bound"""
    return max(8.0 * err64(ref32, ref), floor)


class IBuf:
    """int32 device output of `shape` with a sentinel row past its end, prefilled with the sentinel"""

    def __init__(self, dev, shape):
        self.n = 1
        for s in shape:
            self.n *= int(s)
        self.flat = torch.full((self.n + int(shape[-1]),), ISENT, dtype=torch.int32, device=dev)
        self.t = self.flat[:self.n].view(*shape)

    def get(self, test, what):
        assert bool((self.flat[self.n:] == ISENT).all()), "%s %s: wrote past the end of the output" % (test, what)
        return self.t.cpu()


def first_max_bits(x):
    """the first maximum of every row of the kernel's OWN stored numbers"""
    return ref64.first_argmax(x.cpu())


# ------------------------------------------------------------------------------------------------------------------ BiLSTM
def _bilstm_gpu(dev, B, T, H=256):
    lib, _, dptr, st = abi()
    gx, whh, _, _ = rc.bilstm_case(B, T)
    gxd, whd = gx.to(dev), whh.to(dev)
    out, cst = Buf(dev, (B * T, 512)), Buf(dev, (2, B, 256))      # both NaN: step 0 must read neither
    rc_ = lib.dpmn_bilstm_f32(dptr(gxd), dptr(whd), dptr(out.t), dptr(cst.t), B, T, H, st)
    torch.cuda.synchronize()
    return out, cst, rc_


@pytest.mark.parametrize("B", rc.BILSTM_B)
def test_bilstm(dev, B):
    for T in rc.BILSTM_T:
        test = "bilstm[B%d T%d]" % (B, T)
        _, _, (ref, cref), (ref32, cref32) = rc.bilstm_case(B, T)
        out, cst, code = _bilstm_gpu(dev, B, T)
        assert code == 0, test
        out.check(test, "out", ref, ref32)
        cst.check(test, "cell state after the last step", cref, cref32)


def test_bilstm_twice_and_reject(dev):
    a, ca, _ = _bilstm_gpu(dev, 33, 26)
    b, cb, _ = _bilstm_gpu(dev, 33, 26)
    same_bits("bilstm[B33 T26]", "out", a.t, b.t)
    same_bits("bilstm[B33 T26]", "cell state", ca.t, cb.t)
    out, cst, code = _bilstm_gpu(dev, 1, 1, H=128)
    assert code != 0
    untouched("bilstm[H128]", {"out": out, "cell state": cst})


# ------------------------------------------------------------------------------------------------------------------ ASTER decoder step
def _aster_struct(dev, w):
    from dpmn_amd import ops
    td = {k: v.to(dev).contiguous() for k, v in w.items()}
    return ops.aster_dec_weights(td), td


STEP_OUT = ("sproj", "ctx", "alpha", "state_out", "logits")


def _aster_step_gpu(dev, case, R, T, n_class):
    lib, _, dptr, st = abi()
    w, feats, xproj, row_img, state, y_prev = case[:6]
    ws, keep = _aster_struct(dev, w)
    fd, xd, rd, sd, yd = feats.to(dev), xproj.to(dev), row_img.to(dev), state.to(dev), y_prev.to(dev)
    Ra, Ta = state.shape[0], feats.shape[1]
    bufs = {"sproj": Buf(dev, (Ra, 512)), "ctx": Buf(dev, (Ra, 512)), "alpha": Buf(dev, (Ra, Ta)), "state_out": Buf(dev, (Ra, 512)),
            "logits": Buf(dev, (Ra, max(n_class, 1)))}
    code = lib.dpmn_aster_decode_step_f32(C.byref(ws), dptr(fd), dptr(xd), rd.data_ptr(), dptr(sd), yd.data_ptr(), *[dptr(bufs[k].t) for k in STEP_OUT],
                                          R, T, n_class, st)
    torch.cuda.synchronize()
    return bufs, code


def _aster_step_check(dev, R, T, n_class, peaked=False):
    test = "aster_decode_step[R%d T%d nc%d%s]" % (R, T, n_class, " peaked" if peaked else "")
    case = rc.aster_step_case(R, T, n_class, peaked)
    bufs, code = _aster_step_gpu(dev, case, R, T, n_class)
    assert code == 0, test
    for k in STEP_OUT:
        bufs[k].check(test, k, case[6][k], case[7][k])
    rows = float((bufs["alpha"].t.double().sum(-1) - 1.0).abs().max())
    record(test, "max |row sum of alpha - 1|", rows, 1e-5)
    assert rows <= 1e-5


@pytest.mark.parametrize("R", rc.ASTER_R)
def test_aster_decode_step(dev, R):
    for r, T, n_class in rc.aster_step_grid():
        if r == R:
            _aster_step_check(dev, R, T, n_class)


@pytest.mark.parametrize("T", [25, 64])
def test_aster_decode_step_peaked(dev, T):
    _aster_step_check(dev, 17, T, 97, True)


@pytest.mark.parametrize("what,R,T,n_class", [("T65", 17, 65, 97), ("nc129", 17, 25, 129), ("R0", 0, 25, 97)])
def test_aster_decode_step_rejects(dev, what, R, T, n_class):
    case = rc.aster_step_case(17, 25, 97)      # valid operands; the call's own R / T / n_class are out of range
    bufs, code = _aster_step_gpu(dev, case, R, T, n_class)
    assert code != 0
    untouched("aster_decode_step[%s]" % what, bufs)


# ------------------------------------------------------------------------------------------------------------------ ASTER beam search
def _beam_gpu(dev, w, feats, xproj, B, T, beam, n_class, eos, steps, short=0):
    lib, _, dptr, st = abi()
    ws_struct, keep = _aster_struct(dev, w)
    fd, xd = feats.to(dev), xproj.to(dev)
    R = max(B * beam, 1)
    nb = lib.dpmn_aster_beam_workspace_bytes(B, min(beam, 8))
    assert nb == (4 * B * min(beam, 8) * 512 + 2 * B * min(beam, 8)) * 4
    work = Buf(dev, (nb // 4,))
    sym, pred, score = IBuf(dev, (steps, R)), IBuf(dev, (steps, R)), Buf(dev, (steps, R))
    code = lib.dpmn_aster_beam_f32(C.byref(ws_struct), dptr(fd), dptr(xd), dptr(work.t), nb - short, sym.t.data_ptr(), pred.t.data_ptr(), dptr(score.t),
                                   B, T, beam, n_class, eos, steps, st)
    torch.cuda.synchronize()
    return work, sym, pred, score, code


def _finite_part(test, what, got, ref, ref32):
    """-inf (the children of an ended beam) must sit at the same places in all three and nothing may be NaN -> the three with the
    infinite entries zeroed"""
    got = got.cpu()
    assert not bool(torch.isnan(got).any()), "%s %s: NaN stored" % (test, what)
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(torch.isinf(ref32), inf), "%s %s: -inf entries differ from the replay's" % (test, what)
    assert bool((got[inf] < 0).all())
    z = lambda x: torch.where(inf, torch.zeros_like(x), x)
    return z(got), z(ref), z(ref32)


def _beam_check(dev, test, B, beam, n_class, T, steps, kind="cont"):
    w, feats, xproj, eos = rc.beam_case(B, beam, n_class, T, kind)
    R = B * beam
    work, sym_b, pred_b, score_b, code = _beam_gpu(dev, w, feats, xproj, B, T, beam, n_class, eos, steps)
    assert code == 0, test
    sentinel(test, "score", score_b)
    sentinel(test, "workspace", work)
    sym, pred, score = sym_b.get(test, "sym").long(), pred_b.get(test, "pred").long(), score_b.t.cpu()
    # the records are valid: a class, a row of the same image
    img = (torch.arange(R) // beam)[None].expand(steps, R)
    assert bool(((sym >= 0) & (sym < n_class)).all()) and bool((pred // beam == img).all()), "%s: sym / pred out of range" % test
    assert bool((pred[0] % beam == 0).all()), "%s: step 0 chose a child of a beam row that is not live" % test
    wk = work.t.cpu()
    assert not bool(torch.isnan(wk[:4 * R * 512 + R]).any()), "%s: workspace not fully written" % test
    gates = []
    ref = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=(sym, pred), gates=gates)
    ref32 = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=(sym, pred), dtype=F32)
    rc.gate_spread(test, gates)
    # (1) every stored score, the final state and the final sequence scores against the replay
    g, r, r32 = _finite_part(test, "score", score, ref["score"], ref32["score"])
    check_derived(test, "score", g, r, r32)
    bound = bound_of(r, r32)
    check_derived(test, "final state", wk[:R * 512].reshape(R, 512), ref["state"], ref32["state"])
    g, r, r32 = _finite_part(test, "final sequence scores", wk[4 * R * 512:4 * R * 512 + R], ref["seq"], ref32["seq"])
    check_derived(test, "final sequence scores", g, r, r32)
    flat = (pred % beam) * n_class + sym
    for s in range(steps):
        sc, fl, cand = score[s].reshape(B, beam), flat[s].reshape(B, beam), ref["cand"][s].reshape(B, beam * n_class)
        # (2) the kernel's own numbers: best first, equal scores in rising flat index, no candidate twice
        assert bool((sc[:, :-1] >= sc[:, 1:]).all()), "%s step %d: stored scores not best first" % (test, s)
        tied = sc[:, :-1] == sc[:, 1:]
        assert bool((fl[:, :-1] < fl[:, 1:])[tied].all()), "%s step %d: equal stored scores not in rising flat index" % (test, s)
        assert all(len(set(row)) == beam for row in fl.tolist()), "%s step %d: a candidate chosen twice" % (test, s)
        # (3) float64: nothing unchosen beats the smallest chosen one by more than the slack; the chosen ones best first within it
        chosen = torch.gather(cand, 1, fl)
        rest = cand.clone()
        rest.scatter_(1, fl, float("-inf"))
        worst = chosen.amin(1)
        assert bool((rest.amax(1) <= worst + 2.0 * bound).all()), "%s step %d: an unchosen candidate is %.3e above a chosen one (slack %.3e)" % (
            test, s, float((rest.amax(1) - worst).max()), 2.0 * bound)
        assert bool((chosen[:, :-1] >= chosen[:, 1:] - 2.0 * bound).all()), "%s step %d: chosen candidates out of order in float64" % (test, s)
        # no child of an ended beam while a finite candidate remains
        n_finite = torch.isfinite(cand).sum(1).clamp(max=beam)
        assert torch.equal(torch.isfinite(sc).sum(1), n_finite), "%s step %d: a child of an ended beam was chosen before a finite candidate" % (test, s)
    return ref, sym, pred, score


@pytest.mark.parametrize("B,beam", rc.BEAM_SHAPES)
def test_aster_beam(dev, B, beam):
    for b, bm, n_class, T, steps in rc.beam_grid():
        if (b, bm) == (B, beam):
            _beam_check(dev, "aster_beam[B%d beam%d nc%d T%d steps %d]" % (B, beam, n_class, T, steps), B, beam, n_class, T, steps)


@pytest.mark.parametrize("B,beam,n_class", [(3, 5, 97), (3, 8, 128), (4, 5, 5)])
def test_aster_beam_eos(dev, B, beam, n_class):
    test = "aster_beam[eos B%d beam%d nc%d]" % (B, beam, n_class)
    ref, sym, pred, score = _beam_check(dev, test, B, beam, n_class, 25, 6, "eos")
    assert rc.some_but_not_all_ended(ref, B, beam), "%s: no image with some but not all beams ended" % test
    ended = torch.stack(ref["ended"])
    child = ended[:-1].gather(1, pred[1:])          # step s chose a child of a beam that emitted EOS at step s - 1
    assert bool(torch.isinf(score[1:][child]).all()), "%s: a child of an ended beam carries a finite score" % test


@pytest.mark.parametrize("beam,n_class", [(5, 97), (8, 97), (8, 128)])
def test_aster_beam_ties(dev, beam, n_class):
    B = 2
    test = "aster_beam[ties beam%d nc%d]" % (beam, n_class)
    _, sym, pred, score = _beam_check(dev, test, B, beam, n_class, 25, 6, "tie")
    for s, exp in enumerate(rc.tie_expected(beam, n_class)):
        for b in range(B):
            got = [(int(p) - b * beam, int(c)) for p, c in zip(pred[s].reshape(B, beam)[b], sym[s].reshape(B, beam)[b])]
            assert got == exp, "%s step %d image %d: chose %s, the lower flat index gives %s" % (test, s, b, got, exp)
    n_top = sum(1 for _, c in rc.tie_expected(beam, n_class)[0] if c in (3, 70, n_class - 1))
    assert bool((score[0].reshape(B, beam)[:, :n_top] == score[0].reshape(B, beam)[:, :1]).all()), "%s: the tied maxima are not equal bits" % test


@pytest.mark.parametrize("what", ["beam9", "nc<beam", "eos=nc", "T65", "ws short"])
def test_aster_beam_rejects(dev, what):
    B, beam, n_class, T, eos, short = 2, 5, 97, 25, 1, 0
    w, feats, xproj, _ = rc.beam_case(2, 5, 97, 25)
    if what == "beam9":
        beam = 9
    elif what == "nc<beam":
        n_class = 4
    elif what == "eos=nc":
        eos = n_class
    elif what == "T65":
        T = 65
    else:
        short = 1
    work, sym, pred, score, code = _beam_gpu(dev, w, feats, xproj, B, T, beam, n_class, eos, 2, short)
    assert code != 0
    untouched("aster_beam[%s]" % what, {"score": score, "workspace": work})
    assert bool((sym.flat == ISENT).all()) and bool((pred.flat == ISENT).all())


# ------------------------------------------------------------------------------------------------------------------ MORAN decoder
def _moran_gpu(dev, feats, fproj, B, T, steps, n_class, w=None):
    from dpmn_amd import ops
    lib, _, dptr, st = abi()
    td = {k: v.to(dev).contiguous() for k, v in (w or rc.moran_weights_for(min(n_class, 48))).items()}
    ws = ops.moran_dec_weights(td)
    fd, pd = feats.to(dev), fproj.to(dev)
    logits, ids = Buf(dev, (feats.shape[0], steps, n_class)), IBuf(dev, (feats.shape[0], steps))
    code = lib.dpmn_moran_decode_f32(C.byref(ws), dptr(fd), dptr(pd), dptr(logits.t), ids.t.data_ptr(), B, T, steps, n_class, st)
    torch.cuda.synchronize()
    return logits, ids, code


def _moran_check(dev, B, T, n_class, steps):
    test = "moran_decode[B%d T%d nc%d steps %d]" % (B, T, n_class, steps)
    feats, fproj = rc.moran_case(B, T)
    rc.moran_free(B, T, n_class, steps)        # the case's gate spread
    lbuf, ibuf, code = _moran_gpu(dev, feats, fproj, B, T, steps, n_class)
    assert code == 0, test
    ids = ibuf.get(test, "ids").long()
    assert bool(((ids >= 0) & (ids < n_class)).all()), "%s: ids out of range" % test
    w = rc.moran_weights_for(n_class)
    (ref, _), (ref32, _) = both(ref64.moran_decode, w, feats, fproj, steps, n_class, ids=ids)
    lbuf.check(test, "logits", ref, ref32)                                                      # (1)
    assert torch.equal(first_max_bits(lbuf.t), ids), "%s: an id is not the first maximum of the stored logits" % test      # (2)
    if n_class > 1:                                                                             # (3)
        bound = bound_of(ref, ref32)
        top2 = ref.topk(2, -1)[0]
        clear = (top2[..., 0] - top2[..., 1]) > 2.0 * bound
        record(test, "share of decisions with a float64 margin above twice the bound", float(clear.double().mean()))
        assert torch.equal(ids[clear], ref64.first_argmax(ref)[clear]), "%s: %d ids differ from float64 at a clear margin" % (
            test, int((ids[clear] != ref64.first_argmax(ref)[clear]).sum()))
    return lbuf, ids


@pytest.mark.parametrize("B", rc.MORAN_B)
def test_moran_decode(dev, B):
    for b, T, n_class, steps in rc.moran_grid():
        if b == B:
            _moran_check(dev, B, T, n_class, steps)


def test_moran_decode_image_independence(dev):
    B, T, n_class, steps = 17, 25, 37, 20
    feats, fproj = rc.moran_case(B, T)
    whole, ids, _ = _moran_gpu(dev, feats, fproj, B, T, steps, n_class)
    alone, ida, code = _moran_gpu(dev, feats[16:].contiguous(), fproj[16:].contiguous(), 1, T, steps, n_class)
    assert code == 0
    same_bits("moran_decode[image 16 of 17]", "logits", whole.t[16:], alone.t)
    same_bits("moran_decode[image 16 of 17]", "ids", ids.t[16:], ida.t)


@pytest.mark.parametrize("what,T,n_class", [("T65", 65, 37), ("nc49", 25, 49)])
def test_moran_decode_rejects(dev, what, T, n_class):
    feats, fproj = rc.moran_case(3, 25)
    logits, ids, code = _moran_gpu(dev, feats, fproj, 3, T, 3, n_class)
    assert code != 0
    untouched("moran_decode[%s]" % what, {"logits": logits})
    assert bool((ids.flat == ISENT).all())


# ------------------------------------------------------------------------------------------------------------------ MORAN rectify / split
def _rectify_case(H, W, Hm, Wm, B=3):
    """image 0: offsets of a few tenths; image 1: offsets beyond +2.5, every row pushed into the zero padding; image 2: negative ones.
    The grids run past [-1, 1] at both ends."""
    omap = u("r_omap", (B, Hm, Wm), -0.6, 0.6)
    omap[1] = u("r_omap1", (Hm, Wm), 2.5, 4.0)
    omap[2] = u("r_omap2", (Hm, Wm), -1.5, 0.2)
    return omap, u("r_plane", (B, H, W)), torch.linspace(-1.15, 1.1, W), torch.linspace(-1.05, 1.2, H), u("r_acc", (B, H, W), -0.3, 0.3)


def _rectify_gpu(dev, omap, plane, gx, gy, acc, Hm=None):
    lib, _, dptr, st = abi()
    B, H, W = plane.shape
    od, pd, gxd, gyd = omap.to(dev), plane.to(dev), gx.to(dev), gy.to(dev)
    accd = None if acc is None else acc.to(dev)
    bufs = {"offsets": Buf(dev, (B, H, W)), "plane": Buf(dev, (B, H, W)), "nhwc4": Buf(dev, (B, H, W, 4))}
    code = lib.dpmn_moran_rectify_f32(dptr(od), dptr(pd), dptr(gxd), dptr(gyd), dptr(accd, True), dptr(bufs["offsets"].t), dptr(bufs["plane"].t),
                                      dptr(bufs["nhwc4"].t), B, H, W, omap.shape[1] if Hm is None else Hm, omap.shape[2], st)
    torch.cuda.synchronize()
    return bufs, code


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("H,W,Hm,Wm", [(3, 5, 2, 2), (7, 9, 2, 5), (32, 100, 16, 50)])
def test_moran_rectify(dev, H, W, Hm, Wm, with_acc):
    test = "moran_rectify[%dx%d map %dx%d%s]" % (H, W, Hm, Wm, " acc" if with_acc else "")
    omap, plane, gx, gy, acc = _rectify_case(H, W, Hm, Wm)
    acc = acc if with_acc else None
    (a, r), (a32, r32) = both(ref64.moran_rectify, omap, plane, gx, gy, acc)
    # whole rows of image 1 are pushed into the zero padding (not its outermost columns: there the offset map itself is sampled
    # outside and the offset falls back to 0) where the same rows of image 0 are not
    pushed = (r[1] == 0).all(-1) & ~(r[0] == 0).all(-1)
    assert int(pushed.sum()) >= 1, test
    bufs, code = _rectify_gpu(dev, omap, plane, gx, gy, acc)
    assert code == 0, test
    bufs["offsets"].check(test, "accumulated offsets", a, a32)
    bufs["plane"].check(test, "plane", r, r32)
    sentinel(test, "nhwc4", bufs["nhwc4"])
    assert torch.equal(bufs["nhwc4"].t[..., 0], bufs["plane"].t), "%s: channel 0 of the NHWC(4) copy differs from the plane" % test
    assert bool((bufs["nhwc4"].t[..., 1:] == 0).all()), "%s: channels 1..3 of the NHWC(4) copy are not zero" % test


def test_moran_rectify_rejects(dev):
    omap, plane, gx, gy, _ = _rectify_case(3, 5, 2, 2)
    bufs, code = _rectify_gpu(dev, omap, plane, gx, gy, None, Hm=1)
    assert code != 0
    untouched("moran_rectify[Hm1]", bufs)


@pytest.mark.parametrize("C_", [4, 12])
@pytest.mark.parametrize("sy,sx", [(1, 1), (2, 1), (3, 2)])
def test_moran_split(dev, sy, sx, C_):
    lib, check, dptr, st = abi()
    test = "moran_split[%dx%d C%d]" % (sy, sx, C_)
    B, H, W = 2, 5, 7
    x = u("split_x", (B, H, W, 2 * C_))
    Ho, Wo = (H - 1) // sy + 1, (W - 1) // sx + 1
    y1, y2 = Buf(dev, (B, Ho, Wo, C_)), Buf(dev, (B, Ho, Wo, C_))
    xd = x.to(dev)
    check(lib.dpmn_moran_split_nhwc_f32(dptr(xd), dptr(y1.t), dptr(y2.t), B, H, W, C_, sy, sx, st))
    exact(test, "y1", y1, x[:, ::sy, ::sx, :C_])
    exact(test, "y2", y2, x[:, ::sy, ::sx, C_:])


# ------------------------------------------------------------------------------------------------------------------ VisionLAN
def _pp_case(B, ld, peaked):
    scores = u("pp_scores", (B, 256, ld), -15.0, 12.0) if peaked else u("pp_scores", (B, 256, ld), -3.0, 3.0)
    if peaked:
        scores[:, 255] = 15.0
    return scores, u("pp_enc", (B, 256, 512)), u("pp_w", (256, 512), -0.2, 0.2), u("pp_b", (256,))


def _pp_gpu(dev, scores, enc, wv, bv, B, L, n_steps, n_class, ld):
    lib, _, dptr, st = abi()
    sd, ed, wd, bd = scores.to(dev), enc.to(dev), wv.to(dev), bv.to(dev)
    logits = Buf(dev, (B, min(n_steps, 26), n_class))
    code = lib.dpmn_vl_pp_pool_f32(dptr(sd), ld, dptr(ed), dptr(wd), dptr(bd), dptr(logits.t), B, L, 512, n_steps, n_class, st)
    torch.cuda.synchronize()
    return logits, code


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("B,n_steps,ld", [(1, 1, 1), (3, 26, 26), (3, 26, 29), (1, 1, 4)])
def test_vl_pp_pool(dev, B, n_steps, ld, peaked):
    scores, enc, wv, bv = _pp_case(B, ld, peaked)
    if peaked:
        col = scores[:, :, :n_steps].double()
        span = col.amax(1) - col.amin(1)
        assert bool((col.argmax(1) == 255).all()) and 25.0 <= float(span.min()) and float(span.max()) <= 30.0
    for n_class in (1, 37, 255, 256):
        test = "vl_pp_pool[B%d steps %d ld %d nc%d%s]" % (B, n_steps, ld, n_class, " peaked" if peaked else "")
        w_, b_ = wv[:n_class].contiguous(), bv[:n_class].contiguous()
        ref, ref32 = both(ref64.vl_pp_pool, scores, enc, w_, b_, n_steps)
        logits, code = _pp_gpu(dev, scores, enc, w_, b_, B, 256, n_steps, n_class, ld)
        assert code == 0, test
        logits.check(test, "logits", ref, ref32)


@pytest.mark.parametrize("what,L,n_steps,n_class,ld", [("nc257", 256, 26, 257, 26), ("L128", 128, 26, 37, 26), ("steps>ld", 256, 27, 37, 26)])
def test_vl_pp_pool_rejects(dev, what, L, n_steps, n_class, ld):
    scores, enc, wv, bv = _pp_case(1, 26, False)
    wv, bv = torch.cat([wv, wv[:1]]), torch.cat([bv, bv[:1]])
    logits, code = _pp_gpu(dev, scores, enc, wv, bv, 1, L, n_steps, n_class, ld)
    assert code != 0
    untouched("vl_pp_pool[%s]" % what, {"logits": logits})


@pytest.mark.parametrize("C_", [4, 512])
def test_vl_tokens(dev, C_):
    lib, check, dptr, st = abi()
    B, Hf, Wf = 2, 3, 5
    feat, pos = u("tok_feat", (B, Hf, Wf, C_)), u("tok_pos", (Hf * Wf, C_))
    tok = Buf(dev, (B, Hf * Wf, C_))
    fd, pd = feat.to(dev), pos.to(dev)
    check(lib.dpmn_vl_tokens_f32(dptr(fd), dptr(pd), dptr(tok.t), B, Hf, Wf, C_, st))
    exact("vl_tokens[3x5 C%d]" % C_, "tokens", tok, feat.permute(0, 2, 1, 3).reshape(B, Hf * Wf, C_) + pos)


def test_vl_decode(dev):
    """rows: EOS at step 0; EOS at the last step; no EOS (one only past max_len); a tie that includes class 0 (the first maximum is
    EOS); a tie among classes 2 and 3.  67 images: a second block of three threads.  max_len = 4 < n_steps = 6."""
    lib, check, dptr, st = abi()
    n_steps, n_class, max_len, B = 6, 5, 4, 67
    ids = torch.tensor([[0, 1, 2, 3, 4, 4], [1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 0, 0], [2, 2, 2, 2, 2, 2], [3, 3, 3, 3, 3, 3]])
    base = F.one_hot(ids, n_class).float() * 2.0 + u("vd_noise", (5, n_steps, n_class), 0.0, 0.5)
    base[3, 1] = torch.tensor([1.5, 0.2, 1.5, 0.1, 1.5])
    base[4, 2] = torch.tensor([0.3, 0.2, 1.5, 1.5, 0.1])
    logits = base[torch.arange(B) % 5].contiguous()
    cls_ref, len_ref = ref64.vl_decode(logits, max_len)
    assert cls_ref[:5].tolist() == [[0, 1, 2, 3], [1, 2, 3, 0], [1, 2, 3, 4], [2, 0, 2, 2], [3, 3, 2, 3]] and len_ref[:5].tolist() == [1, 4, 4, 2, 4]
    cls, length = IBuf(dev, (B, max_len)), IBuf(dev, (B,))
    ld_ = logits.to(dev)
    check(lib.dpmn_vl_decode_i32(dptr(ld_), cls.t.data_ptr(), length.t.data_ptr(), B, n_steps, n_class, max_len, st))
    torch.cuda.synchronize()
    assert torch.equal(cls.get("vl_decode", "cls"), cls_ref) and torch.equal(length.get("vl_decode", "length"), len_ref)


# ------------------------------------------------------------------------------------------------------------------ CRNN small kernels
@pytest.mark.parametrize("n_class", [1, 37])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 26), (65, 5)])
def test_crnn_label_vecs(dev, B, T, n_class):
    lib, check, dptr, st = abi()
    test = "crnn_label_vecs[B%d T%d nc%d]" % (B, T, n_class)
    ld = n_class + 3
    logits = u("lv_logits", (B * T, ld), -4.0, 4.0)
    logits[:, n_class:] = 50.0                      # past the row: would swamp the softmax if read
    logits[0, :n_class] = torch.linspace(-15.0, 15.0, n_class) if n_class > 1 else 7.0       # one row spanning 30, the maximum last
    ref, ref32 = both(ref64.crnn_label_vecs, logits, n_class, B, T)
    out = Buf(dev, (B, n_class, 1, T))
    lg = logits.to(dev)
    check(lib.dpmn_crnn_label_vecs_f32(dptr(lg), ld, n_class, dptr(out.t), B, T, st))
    out.check(test, "softmax", ref, ref32)


@pytest.mark.parametrize("n_class", [1, 37])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 26), (65, 5)])
def test_ctc_greedy(dev, B, T, n_class):
    """image 0: all blank; 1: all one class; 2: class and blank in turn; 3: a tie that includes class 0 at every step (the first maximum
    is the blank); the others: random classes, repeats among them"""
    lib, check, dptr, st = abi()
    ld = n_class + 2
    k = n_class - 1
    ids = (torch.rand(B, T, generator=torch.Generator().manual_seed(5)) * n_class * 0.6).long().clamp(max=k)
    ids[0] = 0
    if B > 2:
        ids[1] = k
        ids[2] = torch.arange(T) % 2 * k
    logits = F.one_hot(ids, ld).float() * 3.0 + u("cg_noise", (B, T, ld), 0.0, 0.5)
    logits[..., n_class:] = 9.0                     # past the row
    if B > 3 and n_class > 1:
        logits[3, :, :n_class] = 0.25
        logits[3, :, [0, k]] = 2.0
    logits = logits.reshape(B * T, ld).contiguous()
    cls_ref, len_ref = ref64.ctc_greedy(logits, n_class, B, T)
    if B > 3 and n_class > 1:
        assert len_ref[:4].tolist() == [0, 1, T // 2, 0]
    cls, length = IBuf(dev, (B, T)), IBuf(dev, (B,))
    lg = logits.to(dev)
    check(lib.dpmn_ctc_greedy_i32(dptr(lg), ld, n_class, cls.t.data_ptr(), length.t.data_ptr(), B, T, st))
    torch.cuda.synchronize()
    test = "ctc_greedy[B%d T%d nc%d]" % (B, T, n_class)
    got_cls, got_len = cls.get(test, "cls"), length.get(test, "length")
    assert torch.equal(got_len, len_ref) and torch.equal(got_cls, cls_ref), test
    assert all(bool((got_cls[b, int(got_len[b]):] == 0).all()) for b in range(B)), "%s: cls[b][length..T) is not zero" % test


PREP = [(1, 1, 2, 3), (3, 5, 32, 100), (37, 141, 32, 100)]


def _sliced(dev, B, H, W):
    """channels 1..3 of a five-channel image: img_stride = 5 H W > 3 H W -> (the view on the CPU, base pointer, stride, keep-alive)"""
    full = u("prep_img", (B, 5, H, W), 0.0, 1.0)
    fd = full.to(dev)
    return full[:, 1:4], fd.data_ptr() + 4 * H * W, 5 * H * W, fd


@pytest.mark.parametrize("H,W,Ho,Wo", PREP)
def test_gray_prep(dev, H, W, Ho, Wo):
    lib, check, dptr, st = abi()
    test = "gray_prep[%dx%d -> %dx%d]" % (H, W, Ho, Wo)
    B = 3
    img, ptr, stride, keep = _sliced(dev, B, H, W)
    ref, ref32 = both(ref64.gray_prep, img, Ho, Wo)
    plane, out4 = Buf(dev, (B, Ho, Wo)), Buf(dev, (B, Ho, Wo, 4))
    check(lib.dpmn_gray_prep_f32(ptr, stride, dptr(plane.t), dptr(out4.t), B, H, W, Ho, Wo, st))
    plane.check(test, "luma plane", ref, ref32)
    sentinel(test, "nhwc4", out4)
    assert torch.equal(out4.t[..., 0], plane.t) and bool((out4.t[..., 1:] == 0).all()), "%s: NHWC(4) copy" % test
    noplane = Buf(dev, (B, Ho, Wo, 4))
    check(lib.dpmn_gray_prep_f32(ptr, stride, None, dptr(noplane.t), B, H, W, Ho, Wo, st))
    same_bits(test, "without the plane output", noplane.t, out4.t)


@pytest.mark.parametrize("H,W,Hs,Ws", PREP + [(37, 141, 32, 64), (3, 5, 32, 64), (37, 141, 1, 1)])
def test_aster_prep(dev, H, W, Hs, Ws):
    lib, check, dptr, st = abi()
    test = "aster_prep[%dx%d -> %dx%d]" % (H, W, Hs, Ws)
    B = 3
    img, ptr, stride, keep = _sliced(dev, B, H, W)
    (norm, stn), (norm32, stn32) = both(ref64.aster_prep, img, Hs, Ws)
    nb, sb = Buf(dev, (B, 3, H, W)), Buf(dev, (B, Hs, Ws, 4))
    check(lib.dpmn_aster_prep_f32(ptr, stride, dptr(nb.t), dptr(sb.t), B, H, W, Hs, Ws, st))
    nb.check(test, "normalised image", norm, norm32)
    sentinel(test, "stn input", sb)
    assert not bool(torch.isnan(sb.t).any()) and bool((sb.t[..., 3] == 0).all()), "%s: channel 3 of the STN input" % test
    check_derived(test, "stn input", sb.t[..., :3].contiguous(), stn, stn32.contiguous())


def test_maxpool2d_and_subsample_partial_block(dev):
    """C = 4: one float4 per pixel; 2 x 5 x 7 pixels in, fewer than a block of 256 out"""
    lib, check, dptr, st = abi()
    B, H, W, C_ = 2, 5, 7, 4
    x = u("mp2_x", (B, H, W, C_), -2.0, 2.0)
    xd = x.to(dev)
    for k, s, p in (((2, 2), (2, 1), (0, 1)), ((2, 2), (2, 2), (0, 0)), ((3, 2), (1, 1), (1, 1))):
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
        y = Buf(dev, ref.shape)
        check(lib.dpmn_maxpool2d_f32(dptr(xd), dptr(y.t), B, H, W, C_, k[0], k[1], s[0], s[1], p[0], p[1], st))
        exact("maxpool2d[k%s s%s p%s]" % (k, s, p), "out", y, ref)
    for sy, sx in ((2, 1), (3, 2), (1, 1)):
        ref = x[:, ::sy, ::sx]
        y = Buf(dev, ref.shape)
        check(lib.dpmn_subsample_nhwc_f32(dptr(xd), dptr(y.t), B, H, W, C_, sy, sx, st))
        exact("subsample_nhwc[%dx%d]" % (sy, sx), "out", y, ref)
