"""GPU parity of the window-attention family -- k_window_attn, k_window_attn8_mfma, k_window_attn_mfma (csrc/pgrm.hip), k_window_attn_bwd,
k_window_attn8_bwd_mfma (backward_pgrm.hip), k_window_attn_bwd_mfma (wattn_bwd_mfma.hip) and the fused LayerNorm + q / kv + attention kernels
of attn_fused.hip, attn_fused_bwd.hip and attn_fused192.hip -- each entry point called alone on caller-owned buffers against its float64
reference (tests/ref64.py, pinned to the oracle and to torch.autograd by tests/test_ref64.py) at the smallest token grids that cross the
dispatch and scheduler predicates: H == W == ws, H < W and H > W, an odd slab count (the second half of a block inactive), every group
position, unsorted and repeated window sets, shifts 0, 1, ws / 2 and ws - 1, and for the fused kernels every arm of the persistent scheduler
(fa_plan() restates fa_prepare's formulas on the host and every batch size asserts the arm it was chosen for).

Buffers (Buf of test_gpu_small_backward.py).  Every output a kernel overwrites starts NaN-filled and must come back NaN-free with its
sentinel row intact; the dtables of the atomic backward start from a 2^-10-grid prefill; partial-row buffers and the folded-weight
workspaces start NaN-filled; every partial row below rows_out[g] (unfused) / dpmn_ln_qkv_window_attn_bwd_part_rows (fused) must have been
written, the unfused rows above rows_out[g] must still be NaN.  A rejected call must leave every output all-NaN.

Inputs.
(a) INDEXING: q = 0, tables 0, v on the 2^-5 grid, shift 0: every probability is exactly 1 / N (N a power of two), out is the window mean
of v -- at most 256 multiples of 2^-5 below 1, exact in fp32 in any order -- and the claim is bit equality with float64.  With shifts on
the masked keys carry exp(-100) (denormal or flushed): check_derived at its bare floor.
(b) CONTINUOUS: synth.uniform q / k in [-1.75, 1.75], v and tables in [-1, 1] (fused: tokens in [-1, 1], weights in [-0.15, 0.15]); the
reference's unmasked logits are asserted to stay within 8.  Bound: check_derived, 8 x the fp32 CPU evaluation's own error, floor 1e-6.
(c) PEAKED (forward only): q / k in [-0.5, 0.5], tables in [-15, 12] except row 0 = 15.  Row 0 is the offset (-(ws - 1), -(ws - 1)), used
by the single pair (query 0, key N - 1): for query 0 of every window the maximum sits on the LAST key, the spread within its row is about
30 (both asserted on the reference; a 2 x 2 window's query 0 meets four table rows only, so the other three are put at -15).  Only k_window_attn rescales online over 16-key chunks, and at its window sizes (N <= 16) the row
is one chunk, so the rescale factor is exp(-inf) = 0 on empty accumulators in every kernel of the family today; the kind stays as the
guard for a kernel that does split the row.

The exponential.  The kernels evaluate p = exp(x), x = logit - row maximum <= 0, as 2^(x log2 e) on the hardware exponential (__expf; the
fused kernels fold log2 e into the q weights and the table and call exp2), which the fp32 CPU yardstick (libm expf) does not share.  The
kernel guides do not state the accuracy of that instruction, so the term is NOT derived from them.  What follows from the fp32 format
alone: the rounded product x log2 e is off by 2^-24 |x| log2 e, which moves p by the relative amount 2^-24 |x| (ln 2 log2 e = 1); for the
instruction itself one unit in the last place (2^-23 relative) is ASSUMED.  So r = 2^-24 (|x| + 2) per probability, for the fused kernels
2^-24 (|x| + |logit| + 2) (the two parts of the logit are each rounded after the multiplication by log2 e).  The normalised P = p / sum p
then carries R_nm = r_nm + sum_k P_nk r_nk, i.e. |dP| <= P R, and every output is linear in P:
  out  = (P M) V                      sum_m P R M |v|
  dV   = (P M)^T dO                   sum_n P R M |dO|
  dS   = P (dP - sum P dP)            E = P R |dP - Delta| + P sum_k P R |dP|       (dP = dO V^T M carries no exponential)
  dQ   = scale dS K                   scale sum_m E |k|         dK = scale dS^T Q:  scale sum_n E |q|
  dtable = scatter of dS              the same scatter of E
every factor from the REFERENCE (exp_floors()), never from the kernel's output; the maximum over the tensor is added to the 1e-6 floor.
At these inputs the term is between 1e-7 and 1e-6 -- the bound stays dominated by the fp32 CPU yardstick.  Because the 2^-23 is an
assumption, every check records (helpers.record, through check_derived) the measured GPU error against float64 next to the fp32 CPU
evaluation's error against float64 and the bound, one line per arm and quantity.
The atomic dtable check runs on continuous values, so the order of its atomic additions, and with it the last bits, may change from run
to run (helpers.grid's warning).  A table entry adds at most B nW N terms, a few thousand here; its bound carries the exponential's
term of the same number of terms, and the errors recorded for it (the results file of helpers.record, "dtable g (atomic, on a prefill)")
stay below a quarter of the bound -- an order effect of a few ulps of the partial sums does not reach it.  The det form's float64 sum of
the partial rows has no such freedom.

Predicates.  dpmn_ln_qkv_window_attn{,_d32}_supported take no shifts: for the geometries they agree with the entry point's accept / reject;
shift == ws is a geometry they accept and the entry point must still reject."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import ref64
from dpmn_amd.utils import synth
from helpers import record
from test_gpu_small_backward import Buf, SENT, abi, both, grid, same_bits
from test_gpu_small_kernels import check_derived

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SEED = 0x5EEDA77E


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=130):
    return synth.uniform(name, shape, lo, hi, seed)


def arrs(tensors, windows, shifts):
    from dpmn_amd import _abi
    return _abi.ptr_array(tensors), _abi.int_array(windows), _abi.int_array(shifts)


def sentinel(test, what, buf):
    assert bool((buf.flat[buf.n:] == SENT).all()), "%s %s: wrote past the end of the output" % (test, what)


def untouched(test, what, buf):
    sentinel(test, what, buf)
    assert bool(torch.isnan(buf.t).all()), "%s %s: a rejected call wrote %d elements" % (test, what, int((~torch.isnan(buf.t)).sum()))


def judge(test, what, buf, ref, ref32, floor=1e-6):
    sentinel(test, what, buf)
    nan = int(torch.isnan(buf.t).sum())
    assert nan == 0, "%s %s: %d of %d outputs never written" % (test, what, nan, buf.n)
    check_derived(test, what, buf.t, ref.reshape(buf.t.shape), ref32.reshape(buf.t.shape), floor)


def exact(test, what, buf, ref):
    sentinel(test, what, buf)
    got = buf.t.cpu().double()
    assert not bool(torch.isnan(got).any()), "%s %s: %d outputs never written" % (test, what, int(torch.isnan(got).sum()))
    bad = int((got != ref).sum())
    record(test, what + ": GPU max abs err vs float64 (indexing kind)", float((got - ref).abs().max()), 0.0)
    assert bad == 0, "%s %s: %d of %d outputs differ from the exactly representable result (max %g)" % (test, what, bad, got.numel(), float((got - ref).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ the exponential's term
def exp_floors(parts, fused=False, bwd=False):
    """The module docstring's bounds from the float64 reference's own operands (parts: the per-group dicts of ref64.window_attn{,_bwd}).
    -> {"out"} or {"dq", "dkv", "dtable": [per group]}: the largest possible effect of the hardware exponential on any element"""
    res = {"out": 0.0, "dq": 0.0, "dkv": 0.0, "dtable": []}
    for r in parts:
        S, P, M = r["S"], r["P"], r["M"]
        x = S.amax(-1, keepdim=True) - S
        logit = torch.where(S < -50.0, S + 100.0, S).abs() if fused else 0.0
        rel = 2.0 ** -24 * (x + logit + 2.0)
        PR = P * (rel + (P * rel).sum(-1, keepdim=True))
        PRM = PR if M is None else PR * M
        if not bwd:
            res["out"] = max(res["out"], float((PRM @ r["V"].abs()).max()))
            continue
        dP, dO = r["dP"], r["dO"]
        E = PR * (dP - (P * dP).sum(-1, keepdim=True)).abs() + P * (PR * dP.abs()).sum(-1, keepdim=True)
        res["dq"] = max(res["dq"], float(r["scale"] * (E @ r["K"].abs()).max()))
        res["dkv"] = max(res["dkv"], float(r["scale"] * (E.transpose(-1, -2) @ r["Q"].abs()).max()), float((PRM.transpose(-1, -2) @ dO.abs()).max()))
        N = P.shape[-1]
        dt = torch.zeros(int(r["idx"].max()) + 1, 2, dtype=F64)
        dt.index_add_(0, r["idx"].reshape(-1), E.sum((0, 1)).permute(1, 2, 0).reshape(N * N, 2))
        res["dtable"].append(float(dt.max()))
    return res


def logits_within(test, parts, bound):
    """the continuous kind's premise, on the reference: every logit, its bias included and the -100 of the mask aside, within `bound`"""
    for r in parts:
        S = r["S"]
        m = float(torch.where(S < -50.0, S + 100.0, S).abs().max())
        assert m <= bound, "%s: a reference logit of magnitude %.2f (allowed %g)" % (test, m, bound)


# ------------------------------------------------------------------------------------------------------------------ unfused cases
@functools.lru_cache(maxsize=None)
def _inputs(kind, windows, D, B, H, W):
    G, L = len(windows), H * W
    Cd = 2 * D * G
    tag = "%s%s%d_%d_%d_%d" % (kind, windows, D, B, H, W)
    if kind == "index":
        q, k, v = torch.zeros(B, L, Cd), u("k" + tag, (B, L, Cd)), grid(u("v" + tag, (B, L, Cd)), 5)
        tables = [torch.zeros((2 * ws - 1) ** 2, 2) for ws in windows]
    elif kind == "peaked":
        q, k, v = u("q" + tag, (B, L, Cd), -0.5, 0.5), u("k" + tag, (B, L, Cd), -0.5, 0.5), u("v" + tag, (B, L, Cd))
        tables = [u("t%d" % g + tag, ((2 * ws - 1) ** 2, 2), -15.0, 12.0) for g, ws in enumerate(windows)]
        for t, ws in zip(tables, windows):
            t[0] = 15.0
            if ws == 2:      # query 0 of a 2 x 2 window meets rows 0, 1, 3, 4 only: the other three at the bottom of the range
                t[[1, 3, 4]] = -15.0
    else:
        q, k, v = u("q" + tag, (B, L, Cd), -1.75, 1.75), u("k" + tag, (B, L, Cd), -1.75, 1.75), u("v" + tag, (B, L, Cd))
        tables = [u("t%d" % g + tag, ((2 * ws - 1) ** 2, 2)) for g, ws in enumerate(windows)]
    return q, torch.cat([k, v], -1).contiguous(), tables, u("dout" + tag, (B, L, Cd))


@functools.lru_cache(maxsize=None)
def _fwd_ref(kind, windows, shifts, D, B, H, W, p):
    q, kv, tables, _ = _inputs(kind, windows, D, B, H, W)
    parts = []
    ref = ref64.window_attn(q, kv, tables, list(windows), list(shifts), H, W, p, SEED, parts=parts)
    ref32 = ref64.window_attn(q, kv, tables, list(windows), list(shifts), H, W, p, SEED, dtype=F32)
    test = "%s %s" % (kind, (windows, shifts, D, B, H, W))
    if kind == "cont":
        logits_within(test, parts, 8.0)
    if kind == "peaked":
        for r in parts:      # query 0 of every window: the maximum on the last key, a spread of about 30
            row = r["S"][:, :, :, 0]
            spread = row.amax(-1) - row.amin(-1)
            assert bool((row.argmax(-1) == row.shape[-1] - 1).all()) and float(spread.min()) >= 20.0, test
    return ref, ref32, 1e-6 + exp_floors(parts)["out"]


@functools.lru_cache(maxsize=None)
def _bwd_ref(windows, shifts, D, B, H, W, p):
    q, kv, tables, dout = _inputs("cont", windows, D, B, H, W)
    parts = []
    ref = ref64.window_attn_bwd(q, kv, tables, list(windows), list(shifts), H, W, dout, p, SEED, parts=parts)
    ref32 = ref64.window_attn_bwd(q, kv, tables, list(windows), list(shifts), H, W, dout, p, SEED, dtype=F32)
    logits_within("bwd %s" % ((windows, shifts, D, B, H, W),), parts, 8.0)
    return ref, ref32, exp_floors(parts, bwd=True)


def fwd_gpu(dev, kind, windows, shifts, D, B, H, W, p):
    """one dpmn_window_attn_drop_f32 launch into a NaN-filled caller-owned buffer -> (Buf, return code)"""
    lib, _, dptr, st = abi()
    q, kv, tables, _ = _inputs(kind, windows, D, B, H, W)
    qd, kvd, td = q.to(dev), kv.to(dev), [t.to(dev) for t in tables]
    out = Buf(dev, q.shape)
    tp, wp, sp = arrs(td, windows, shifts)
    rc = lib.dpmn_window_attn_drop_f32(dptr(qd), dptr(kvd), tp, wp, sp, len(windows), 2, dptr(out.t), B, H, W, q.shape[2], float(p), SEED, st)
    torch.cuda.synchronize()
    return out, rc


def shift_sets(ws, G):
    """every shift of {0, 1, ws / 2, ws - 1} at some group, in two launches"""
    a, b = [0, 1, ws - 1], [ws - 1, ws // 2, 1]
    return [tuple(a[:G]), tuple(b[:G])] if G == 3 else [(0,), (ws // 2,), (ws - 1,)]


def fwd_arm(dev, arm, ws, D, grids, batches, p):
    """Three groups that all carry the window under test, so it runs at g = 0, 1 and 2 (the g CG channel offset, the g term of the dropout
    index) in every launch, each group with its own shift; then one n_groups = 1 case."""
    for H, W in grids:
        for B in batches:
            for G in ((3, 1) if (H, W, B) == (grids[0][0], grids[0][1], batches[0]) else (3,)):
                windows = (ws,) * G
                for shifts in shift_sets(ws, G):
                    test = "%s[ws%d D%d G%d %dx%dx%d shifts %s p%g]" % (arm, ws, D, G, B, H, W, shifts, p)
                    ref, ref32, floor = _fwd_ref("cont", windows, shifts, D, B, H, W, p)
                    out, rc = fwd_gpu(dev, "cont", windows, shifts, D, B, H, W, p)
                    assert rc == 0, test
                    judge(test, "out", out, ref, ref32, floor)
                if p == 0.0:      # the indexing kind: shift 0 exact, shifts on at the bare floor
                    test = "%s[ws%d D%d G%d %dx%dx%d indexing]" % (arm, ws, D, G, B, H, W)
                    zero = (0,) * G
                    out, rc = fwd_gpu(dev, "index", windows, zero, D, B, H, W, 0.0)
                    assert rc == 0, test
                    exact(test, "out", out, _fwd_ref("index", windows, zero, D, B, H, W, 0.0)[0])
                    sh = shift_sets(ws, G)[-1]
                    ref, ref32, _ = _fwd_ref("index", windows, sh, D, B, H, W, 0.0)
                    out, rc = fwd_gpu(dev, "index", windows, sh, D, B, H, W, 0.0)
                    judge(test + " shifted", "out", out, ref, ref32)
    # the peaked kind, one case per kernel: the first grid, B = 3
    H, W = grids[0]
    windows, shifts = (ws,) * 3, (0, 0, 0)
    test = "%s[ws%d D%d peaked p%g]" % (arm, ws, D, p)
    ref, ref32, floor = _fwd_ref("peaked", windows, shifts, D, batches[-1], H, W, p)
    out, rc = fwd_gpu(dev, "peaked", windows, shifts, D, batches[-1], H, W, p)
    assert rc == 0, test
    judge(test, "out", out, ref, ref32, floor)


SMALL = ((8, 8), (8, 16), (16, 8))        # 8 x 8 at B = 1, 3: 1 / 3 slabs of 64 tokens -- the second half of the last block is inactive
LARGE = ((16, 16), (16, 32), (32, 16))    # one / two 16 x 16 windows per image


# (ws, D) -> kernel, dpmn_window_attn_drop_f32: (2, 16), (4, 16) -> k_window_attn<WS, 16>
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("ws,D", [(2, 16), (4, 16)])
def test_fwd_window_attn(dev, ws, D, p):
    fwd_arm(dev, "k_window_attn", ws, D, SMALL, (1, 3), p)


# (8, 16) -> k_window_attn8_mfma; 8 x 8: H == W == ws, one window per image
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_fwd_window_attn8_mfma(dev, p):
    fwd_arm(dev, "k_window_attn8_mfma", 8, 16, SMALL, (1, 3), p)


# (4, 32), (8, 32) -> k_window_attn_mfma<WS, 32>: two 64-token key sets per block
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("ws,D", [(4, 32), (8, 32)])
def test_fwd_window_attn_mfma(dev, ws, D, p):
    fwd_arm(dev, "k_window_attn_mfma", ws, D, SMALL, (1, 3), p)


# (16, 32) -> k_window_attn_mfma<16, 32>: one 16 x 16 window per 512-thread block; 16 x 16: H == W == ws
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_fwd_window_attn_mfma16(dev, p):
    fwd_arm(dev, "k_window_attn_mfma<16>", 16, 32, LARGE, (1, 2), p)


# ------------------------------------------------------------------------------------------------------------------ unfused backward
def rows_expected(ws, D, B, H, W):
    """rows_out[g] as window_attn_bwd_impl computes it: one row per 64-token slab (8, 16), per window (the matrix-core kernel), per block
    of two slabs (k_window_attn_bwd)"""
    slabs = B * (H * W // 64)
    if (ws, D) == (8, 16):
        return slabs
    if (ws, D) in ((8, 32), (16, 32), (16, 16)):
        return B * (H * W // (ws * ws))
    return (slabs + 1) // 2


def bwd_gpu(dev, windows, shifts, D, B, H, W, p, det):
    lib, check, dptr, st = abi()
    q, kv, tables, dout = _inputs("cont", windows, D, B, H, W)
    G, Cd = len(windows), q.shape[2]
    qd, kvd, td, dd = q.to(dev), kv.to(dev), [t.to(dev) for t in tables], dout.to(dev)
    dq, dkv = Buf(dev, (B, H * W, Cd)), Buf(dev, (B, H * W, 2 * Cd))
    tp, wp, sp = arrs(td, windows, shifts)
    if det:
        nrows = lib.dpmn_window_attn_bwd_part_rows(B, H, W)
        dt = [Buf(dev, (nrows, t.numel())) for t in tables]
        rows = (C.c_int * G)(*([-1] * G))
        check(lib.dpmn_window_attn_drop_bwd_det_f32(dptr(qd), dptr(kvd), tp, wp, sp, G, 2, dptr(dd), dptr(dq.t), dptr(dkv.t), arrs([b.t for b in dt], windows, shifts)[0],
                                                    rows, B, H, W, Cd, float(p), SEED, st))
        torch.cuda.synchronize()
        return dq, dkv, dt, list(rows)
    fills = [grid(u("dtfill%d" % g, tuple(t.shape)), 10) for g, t in enumerate(tables)]
    dt = [Buf(dev, tuple(f.shape), f) for f in fills]
    check(lib.dpmn_window_attn_drop_bwd_f32(dptr(qd), dptr(kvd), tp, wp, sp, G, 2, dptr(dd), dptr(dq.t), dptr(dkv.t), arrs([b.t for b in dt], windows, shifts)[0],
                                            B, H, W, Cd, float(p), SEED, st))
    torch.cuda.synchronize()
    return dq, dkv, dt, None


def bwd_arm(dev, arm, ws, D, grids, batches, p):
    for H, W in grids:
        for B in batches:
            for G in ((3, 1) if (H, W, B) == (grids[0][0], grids[0][1], batches[0]) else (3,)):
                windows = (ws,) * G
                for shifts in shift_sets(ws, G)[:2]:
                    test = "%s[ws%d D%d G%d %dx%dx%d shifts %s p%g]" % (arm, ws, D, G, B, H, W, shifts, p)
                    (rq, rkv, rt), (rq32, rkv32, rt32), fl = _bwd_ref(windows, shifts, D, B, H, W, p)
                    dq, dkv, dt, _ = bwd_gpu(dev, windows, shifts, D, B, H, W, p, False)
                    judge(test, "dq", dq, rq, rq32, 1e-6 + fl["dq"])
                    judge(test, "dkv", dkv, rkv, rkv32, 1e-6 + fl["dkv"])
                    for g in range(G):
                        dt[g].check(test, "dtable %d (atomic, on a prefill)" % g, rt[g], rt32[g], 1e-6 + fl["dtable"][g])
                    runs = [bwd_gpu(dev, windows, shifts, D, B, H, W, p, True) for _ in range(2)]
                    eq, ekv, parts, rows = runs[0]
                    same_bits(test, "det / atomic dq", eq.t, dq.t)
                    same_bits(test, "det / atomic dkv", ekv.t, dkv.t)
                    same_bits(test, "det dq, two launches", eq.t, runs[1][0].t)
                    same_bits(test, "det dkv, two launches", ekv.t, runs[1][1].t)
                    assert rows == [rows_expected(ws, D, B, H, W)] * G, "%s: rows_out %s, the dispatch computes %d" % (test, rows, rows_expected(ws, D, B, H, W))
                    for g in range(G):
                        sentinel(test, "partial rows %d" % g, parts[g])
                        wrote = parts[g].t[:rows[g]]
                        assert not bool(torch.isnan(wrote).any()), "%s: %d elements of the %d partial rows of group %d never written" % (test, int(torch.isnan(wrote).sum()), rows[g], g)
                        assert bool(torch.isnan(parts[g].t[rows[g]:]).all()), "%s: a row past rows_out[%d] = %d was written" % (test, g, rows[g])
                        assert torch.equal(wrote, runs[1][2][g].t[:rows[g]]), "%s: partial rows of group %d differ between two launches" % (test, g)
                        tot = wrote.double().sum(0).float().reshape(rt[g].shape)
                        check_derived(test, "dtable %d (float64 sum of the partial rows)" % g, tot, rt[g], rt32[g], 1e-6 + fl["dtable"][g])


# (2, 16), (4, 16), (4, 32) -> k_window_attn_bwd<WS, D>: two slabs per block, rows_out = ceil(slabs / 2)
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("ws,D", [(2, 16), (4, 16), (4, 32)])
def test_bwd_window_attn(dev, ws, D, p):
    bwd_arm(dev, "k_window_attn_bwd", ws, D, SMALL, (1, 3), p)


# (8, 16) -> k_window_attn8_bwd_mfma: one block per slab
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bwd_window_attn8_mfma(dev, p):
    bwd_arm(dev, "k_window_attn8_bwd_mfma", 8, 16, SMALL, (1, 3), p)


# (8, 32), (16, 32), (16, 16) -> k_window_attn_bwd_mfma<WS, D>: one block per (window, head), the two heads share a partial row
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("ws,D,grids,batches", [(8, 32, SMALL, (1, 3)), (16, 32, LARGE, (1, 2)), (16, 16, LARGE, (1, 2))])
def test_bwd_window_attn_mfma(dev, ws, D, grids, batches, p):
    bwd_arm(dev, "k_window_attn_bwd_mfma", ws, D, grids, batches, p)


# the forward has no (16, 16) arm: rejected at any group position, before any group has been launched
@pytest.mark.parametrize("windows", [(16, 16, 16), (4, 4, 16), (16,)])
def test_fwd_rejects_window16_dim16(dev, windows):
    out, rc = fwd_gpu(dev, "cont", windows, (0,) * len(windows), 16, 1, 16, 16, 0.0)
    assert rc != 0, "window 16 at head dim 16 accepted by the forward"
    untouched("fwd[%s D16]" % (windows,), "out", out)


# H % ws != 0 (12 x 16: 192 tokens), H W % 64 != 0 (8 x 12), shift == ws, shift < 0 -- in the LAST group, after two valid ones
@pytest.mark.parametrize("H,W,windows,shifts", [(12, 16, (4, 4, 8), (0, 0, 0)), (8, 12, (4, 4, 4), (0, 0, 0)), (8, 8, (4, 4, 4), (0, 1, 4)), (8, 8, (2, 4, 8), (0, 0, -1))])
def test_unfused_rejects(dev, H, W, windows, shifts):
    lib, _, dptr, st = abi()
    test = "unfused reject[%dx%d %s %s]" % (H, W, windows, shifts)
    out, rc = fwd_gpu(dev, "cont", windows, shifts, 16, 1, H, W, 0.0)
    assert rc != 0, test + ": forward accepted"
    untouched(test, "out", out)
    q, kv, tables, dout = _inputs("cont", windows, 16, 1, H, W)
    qd, kvd, td, dd = q.to(dev), kv.to(dev), [t.to(dev) for t in tables], dout.to(dev)
    dq, dkv, dt = Buf(dev, q.shape), Buf(dev, kv.shape), [Buf(dev, tuple(t.shape)) for t in tables]
    tp, wp, sp = arrs(td, windows, shifts)
    rc = lib.dpmn_window_attn_drop_bwd_f32(dptr(qd), dptr(kvd), tp, wp, sp, 3, 2, dptr(dd), dptr(dq.t), dptr(dkv.t), arrs([b.t for b in dt], windows, shifts)[0], 1, H, W, 96, 0.0, SEED, st)
    torch.cuda.synchronize()
    assert rc != 0, test + ": backward accepted"
    for what, b in [("dq", dq), ("dkv", dkv)] + [("dtable %d" % g, b) for g, b in enumerate(dt)]:
        untouched(test, what, b)


# ------------------------------------------------------------------------------------------------------------------ fused, dim 96
def two_cu(lib):
    """2 x the CU count rounded down to a multiple of 8 -- the block count of the persistent fused kernels once the work exceeds it,
    read through the library (dpmn_ln_qkv_window_attn_bwd_part_rows = the grid of both directions)"""
    return lib.dpmn_ln_qkv_window_attn_bwd_part_rows(1 << 16, 8, 8)


def fa_plan(lib, windows, B, H, W, cost_ws):
    """fa_prepare's scheduler restated: -> (arm, blocks, nblk, empty): arm 'walk' (nbx < 3: every block walks a cost-balanced range across
    the slots) or 'slot' (one slot per block, nblk[w][slot] blocks each; w = 1: the XCDs that hold one image fewer); empty: some block of
    the grid has no unit (an XCD without an image, or more blocks than units in a slot)"""
    S, cap = H * W // 64, two_cu(lib)
    blocks = min(cap, (3 * B * S + 7) // 8 * 8)
    assert blocks == lib.dpmn_ln_qkv_window_attn_bwd_part_rows(B, H, W)
    nbx = blocks // 8
    cost = [cost_ws[{8: 0, 4: 1, 2: 2}[ws]] for ws in sorted(windows, reverse=True)]
    nblk = [[0, 0, 0], [0, 0, 0]]
    for w in range(2):
        per = ((B + 7) // 8 if w == 0 else B // 8) * S
        if per == 0 or nbx < 3:
            continue
        best = -1
        for n0 in range(1, nbx - 1):
            for n1 in range(1, nbx - n0):
                n = (n0, n1, nbx - n0 - n1)
                t = [50 + (per + n[s] - 1) // n[s] * cost[s] for s in range(3)]
                key = max(t) * 1000000 + sum(t[s] * n[s] for s in range(3)) // nbx
                if best < 0 or key < best:
                    best, nblk[w] = key, list(n)
    empty = B < 8
    for xcd in range(min(B, 8)):
        ni = (B - xcd + 7) // 8
        nb = nblk[0 if ni == (B + 7) // 8 else 1]
        empty = empty or any(nb[s] > ni * S for s in range(3))
    return ("slot" if nblk[0][0] > 0 else "walk"), blocks, nblk, empty


FWD_COST, BWD_COST = (183, 151, 146), (330, 190, 190)
FUSED_WINDOWS = [(2, 4, 8), (8, 2, 4), (4, 8, 4), (8, 8, 8), (2, 2, 2)]


def fused_shifts(windows, on):
    return tuple([windows[0] - 1, 1, windows[2] // 2] if on else [0, 0, 0])


@functools.lru_cache(maxsize=None)
def _fused_case(Cd, windows, shifts, B, H, W, p, bwd):
    L = H * W
    tag = "f%d%s_%d_%d_%d" % (Cd, windows, B, H, W)
    wr = 0.15 if Cd == 96 else 0.1
    tq, tkv = u("tq" + tag, (B, L, Cd)), u("tkv" + tag, (B, L, Cd))
    ln = (u("g1", (Cd,), 0.5, 1.5), u("b1", (Cd,), -0.2, 0.2), u("g2", (Cd,), 0.5, 1.5), u("b2", (Cd,), -0.2, 0.2),
          u("wq%d" % Cd, (Cd, Cd), -wr, wr), u("bq%d" % Cd, (Cd,), -0.2, 0.2), u("wkv%d" % Cd, (2 * Cd, Cd), -wr, wr), u("bkv%d" % Cd, (2 * Cd,), -0.2, 0.2))
    tables = [u("ft%d" % g + tag, ((2 * ws - 1) ** 2, 2)) for g, ws in enumerate(windows)]
    dout = u("fdout" + tag, (B, L, Cd))
    parts = []
    ref = ref64.ln_qkv_window_attn(tq, tkv, ln, tables, list(windows), list(shifts), H, W, p, SEED, parts=parts)
    ref32 = ref64.ln_qkv_window_attn(tq, tkv, ln, tables, list(windows), list(shifts), H, W, p, SEED, dtype=F32)
    logits_within("fused %s" % tag, parts, 8.0)
    floor = 1e-6 + exp_floors(parts, fused=True)["out"]
    g = g32 = gfl = None
    if bwd:
        parts = []
        g = ref64.ln_qkv_window_attn_bwd(tq, tkv, ln, tables, list(windows), list(shifts), H, W, dout, p, SEED, parts=parts)
        g32 = ref64.ln_qkv_window_attn_bwd(tq, tkv, ln, tables, list(windows), list(shifts), H, W, dout, p, SEED, dtype=F32)
        gfl = exp_floors(parts, fused=True, bwd=True)
    return tq, tkv, ln, tables, dout, ref, ref32, floor, g, g32, gfl


def nan_ws(dev, nbytes):
    return torch.full((nbytes // 4,), float("nan"), device=dev)


def fused96(dev, test, windows, shifts, B, H, W):
    """forward, training forward (p = 0 and 0.3, with and without the saved q / kv) and backward of one dim-96 geometry"""
    lib, check, dptr, st = abi()
    wb = lib.dpmn_ln_qkv_window_attn_workspace_bytes()
    assert lib.dpmn_ln_qkv_window_attn_supported(96, 3, 2, arrs([], windows, shifts)[1], H, W) == 1, test
    for p in (0.0, 0.3):
        tq, tkv, ln, tables, dout, (ref, rq, rkv), (ref32, rq32, rkv32), floor, g, g32, gfl = _fused_case(96, windows, shifts, B, H, W, p, True)
        d = [t.to(dev) for t in (tq, tkv) + ln]
        td, dd = [t.to(dev) for t in tables], dout.to(dev)
        tp, wp, sp = arrs(td, windows, shifts)
        head = [dptr(t) for t in d[:6]] + [1e-5] + [dptr(t) for t in d[6:]] + [tp, wp, sp, 3, 2]
        if p == 0.0:      # the evaluation forward; then refold = 0 on the workspace that call left
            out, ws = Buf(dev, ref.shape), nan_ws(dev, wb)
            check(lib.dpmn_ln_qkv_window_attn_f32(*head, dptr(out.t), dptr(ws), 1, B, H, W, 96, st))
            judge(test, "forward cat", out, ref, ref32, floor)
            again = Buf(dev, ref.shape)
            check(lib.dpmn_ln_qkv_window_attn_f32(*head, dptr(again.t), dptr(ws), 0, B, H, W, 96, st))
            torch.cuda.synchronize()
            sentinel(test, "forward cat, refold = 0", again)
            same_bits(test, "forward refold 1 / 0", out.t, again.t)
        # training forward: the saved projections, cat under attn_drop, and the same cat without saving
        out, qo, kvo, fold = Buf(dev, ref.shape), Buf(dev, rq.shape), Buf(dev, rkv.shape), nan_ws(dev, wb)
        check(lib.dpmn_ln_qkv_window_attn_train_f32(*head, dptr(out.t), dptr(qo.t), dptr(kvo.t), p, SEED, dptr(fold), B, H, W, 96, st))
        judge(test + " p%g" % p, "train cat", out, ref, ref32, floor)
        judge(test + " p%g" % p, "train saved q", qo, rq, rq32)
        judge(test + " p%g" % p, "train saved kv", kvo, rkv, rkv32)
        nosave = Buf(dev, ref.shape)
        check(lib.dpmn_ln_qkv_window_attn_train_f32(*head, dptr(nosave.t), None, None, p, SEED, dptr(nan_ws(dev, wb)), B, H, W, 96, st))
        torch.cuda.synchronize()
        sentinel(test, "train cat, nothing saved", nosave)
        same_bits(test + " p%g" % p, "train cat with / without the saved q / kv", out.t, nosave.t)
        # backward: the forward's fold (refold = 0) and a fresh fold
        rows = lib.dpmn_ln_qkv_window_attn_bwd_part_rows(B, H, W)
        runs = []
        for workspace, refold in ((fold, 0), (nan_ws(dev, wb), 1)):
            dq, dkv = Buf(dev, (B * H * W, 96)), Buf(dev, (B * H * W, 192))
            parts = [Buf(dev, (rows, t.numel())) for t in tables]
            check(lib.dpmn_ln_qkv_window_attn_bwd_f32(*head, dptr(dd), dptr(dq.t), dptr(dkv.t), arrs([b.t for b in parts], windows, shifts)[0], p, SEED, dptr(workspace), refold,
                                                      B, H, W, 96, st))
            torch.cuda.synchronize()
            runs.append((dq, dkv, parts))
        dq, dkv, parts = runs[0]
        judge(test + " p%g" % p, "bwd dq", dq, g[0], g32[0], 1e-6 + gfl["dq"])
        judge(test + " p%g" % p, "bwd dkv", dkv, g[1], g32[1], 1e-6 + gfl["dkv"])
        same_bits(test, "bwd dq, the forward's fold / a fresh fold", dq.t, runs[1][0].t)
        same_bits(test, "bwd dkv, the forward's fold / a fresh fold", dkv.t, runs[1][1].t)
        for gi in range(3):
            sentinel(test, "bwd partial rows %d" % gi, parts[gi])
            nan = int(torch.isnan(parts[gi].t).sum())
            assert nan == 0, "%s: %d elements of the %d partial rows of group %d never written" % (test, nan, rows, gi)
            same_bits(test, "bwd partial rows %d, the forward's fold / a fresh fold" % gi, parts[gi].t, runs[1][2][gi].t)
            tot = parts[gi].t.double().sum(0).float().reshape(g[2][gi].shape)
            check_derived(test + " p%g" % p, "bwd dtable %d (float64 sum of the partial rows)" % gi, tot, g[2][gi], g32[2][gi], 1e-6 + gfl["dtable"][gi])


# (H, W, B, arm, what the batch size is there for).  S = H W / 64 units per image and slot; blocks = min(2 CUs, ceil8(3 B S)), nbx = blocks / 8
FUSED_GRID = [
    (8, 8, 1, "walk", "3 units -> 8 blocks, nbx = 1 < 3: XCD 0's one block walks all three slots, seven XCDs hold no image"),
    (8, 8, 2, "walk", "6 units -> 8 blocks, nbx = 1"),
    (8, 8, 5, "walk", "15 units -> 16 blocks, nbx = 2 < 3: two blocks per XCD share three units, cut by cost"),
    (8, 8, 7, "slot", "21 units -> 24 blocks, nbx = 3: one slot per block; XCD 7 holds no image (backward: zero-filled rows)"),
    (8, 8, 8, "slot", "24 units -> 24 blocks, nbx = 3: one unit per block"),
    (8, 8, 9, "slot", "27 units -> 32 blocks, nbx = 4; XCD 0 holds 2 images (nblk[0]), XCDs 1 .. 7 one (nblk[1]: 4 blocks, 3 units -- one empty)"),
    (8, 8, 13, "slot", "39 units -> 40 blocks, nbx = 5; XCDs 0 .. 4 hold 2 images, 5 .. 7 one (nblk[1])"),
    (16, 16, 9, "slot", "S = 4: 108 units -> 112 blocks, nbx = 14; nblk[1] for the XCDs with one image"),
    (16, 16, 13, "slot", "S = 4: 156 units -> 160 blocks, nbx = 20; nblk[1]"),
    (8, 32, 1, "walk", "S = 4: 12 units -> 16 blocks, nbx = 2; H < W"),
    (32, 8, 3, "slot", "S = 4: 36 units -> 40 blocks, nbx = 5; H > W"),
    (16, 16, 1, "walk", "S = 4: 12 units -> 16 blocks, nbx = 2"),
]


@pytest.mark.parametrize("i", range(len(FUSED_GRID)))
def test_fused96(dev, i):
    lib = abi()[0]
    H, W, B, arm, why = FUSED_GRID[i]
    # two of the five window sets per geometry (every set at four or five geometries), each with the zero shifts AND its matched
    # [ws - 1, 1, ws / 2]: every geometry -- the H < W and H > W grids among them -- runs rolled and unrolled
    for windows, on in [(FUSED_WINDOWS[(i + k) % 5], on) for k in (0, 2) for on in (False, True)]:
        shifts = fused_shifts(windows, on)
        test = "fused96[%s %s %dx%dx%d %s]" % (windows, shifts, B, H, W, arm)
        for cost in (FWD_COST, BWD_COST):
            got, blocks, nblk, empty = fa_plan(lib, windows, B, H, W, cost)
            assert got == arm, "%s: fa_prepare's formulas give the '%s' arm (%s)" % (test, got, why)
            if B > 8 and B % 8:
                assert nblk[1][0] > 0, "%s: nblk[1] is trivial" % test
            if (H, W, B) in ((8, 8, 7), (8, 8, 9), (8, 8, 1)):
                assert empty, "%s: no block with an empty unit range" % test
        fused96(dev, test, windows, shifts, B, H, W)


# 3 B units above 2 x the CU count: every block walks several units of its slot
def test_fused96_more_units_than_blocks(dev):
    lib = abi()[0]
    cap = two_cu(lib)
    B = cap // 3 + 8
    assert 3 * B > cap and B * 64 * 96 * 4 < 8 << 20
    for windows, on in (((8, 2, 4), True), ((4, 8, 4), False)):
        arm, blocks, nblk, _ = fa_plan(lib, windows, B, 8, 8, BWD_COST)
        assert arm == "slot" and blocks == cap and sum(nblk[0]) == cap // 8
        fused96(dev, "fused96[%s B%d 8x8 several units per block]" % (windows, B), windows, fused_shifts(windows, on), B, 8, 8)


# ------------------------------------------------------------------------------------------------------------------ fused, dim 192
D32_WINDOWS = [(4, 8, 16), (16, 4, 8), (8, 8, 16), (16, 16, 16)]


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("H,W", LARGE)
def test_fused192(dev, H, W, B):
    lib, check, dptr, st = abi()
    wb = lib.dpmn_ln_qkv_window_attn_d32_workspace_bytes()
    for windows, on in [(w, on) for w in D32_WINDOWS for on in (False, True)]:      # every window set unrolled and with its matched shifts
        shifts = fused_shifts(windows, on)
        test = "fused192[%s %s %dx%dx%d]" % (windows, shifts, B, H, W)
        assert lib.dpmn_ln_qkv_window_attn_d32_supported(192, 3, 2, arrs([], windows, shifts)[1], H, W) == 1, test
        tq, tkv, ln, tables, _, (ref, _, _), (ref32, _, _), floor, _, _, _ = _fused_case(192, windows, shifts, B, H, W, 0.0, False)
        d, td = [t.to(dev) for t in (tq, tkv) + ln], [t.to(dev) for t in tables]
        tp, wp, sp = arrs(td, windows, shifts)
        head = [dptr(t) for t in d[:6]] + [1e-5] + [dptr(t) for t in d[6:]] + [tp, wp, sp, 3, 2]
        out, ws = Buf(dev, ref.shape), nan_ws(dev, wb)
        check(lib.dpmn_ln_qkv_window_attn_d32_f32(*head, dptr(out.t), dptr(ws), 1, B, H, W, 192, st))
        judge(test, "cat", out, ref, ref32, floor)
        again = Buf(dev, ref.shape)
        check(lib.dpmn_ln_qkv_window_attn_d32_f32(*head, dptr(again.t), dptr(ws), 0, B, H, W, 192, st))
        torch.cuda.synchronize()
        sentinel(test, "cat, refold = 0", again)
        same_bits(test, "refold 1 / 0", out.t, again.t)


# ------------------------------------------------------------------------------------------------------------------ predicates
# (dim, windows, shifts, H, W, the entry point accepts).  _supported() sees no shifts: it must agree wherever the shifts are valid
PREDICATES = [
    (96, (2, 4, 8), (0, 0, 0), 8, 16, True),
    (96, (2, 4, 8), (0, 0, 0), 24, 8, False),        # divisible by every window, 192 tokens, not a power of two
    (96, (2, 4, 4), (0, 0, 0), 4, 16, False),        # H < 8
    (96, (4, 8, 16), (0, 0, 0), 16, 16, False),      # window 16 at dim 96
    (96, (2, 4, 8), (0, 4, 0), 8, 8, False),         # shift == ws
    (96, (2, 4, 8), (0, 0, 0), 12, 16, False),       # H % ws != 0
    (96, (2, 4, 4), (0, 0, 0), 8, 12, False),        # H W % 64 != 0
    (192, (4, 8, 16), (0, 0, 0), 16, 16, True),
    (192, (4, 8, 8), (0, 0, 0), 8, 8, False),        # 8 x 8 at dim 192
    (192, (4, 8, 16), (0, 0, 16), 16, 16, False),    # shift == ws
    (192, (4, 8, 16), (0, 0, 0), 24, 32, False),
    (192, (2, 4, 8), (0, 0, 0), 16, 16, False),      # window 2 at dim 192
    (192, (4, 8, 16), (0, 0, 0), 16, 8, False),      # 128 tokens: not a multiple of 256
]


@pytest.mark.parametrize("Cd,windows,shifts,H,W,ok", PREDICATES)
def test_predicates(dev, Cd, windows, shifts, H, W, ok):
    lib, _, dptr, st = abi()
    test = "predicate[dim %d %s %s %dx%d]" % (Cd, windows, shifts, H, W)
    B, L = 2, H * W
    sup = (lib.dpmn_ln_qkv_window_attn_supported if Cd == 96 else lib.dpmn_ln_qkv_window_attn_d32_supported)(Cd, 3, 2, arrs([], windows, shifts)[1], H, W)
    valid_shifts = all(0 <= s < w for s, w in zip(shifts, windows))
    assert sup == int(ok or not valid_shifts), "%s: _supported() says %d, the entry point %s" % (test, sup, "accepts" if ok else "rejects")
    wr = 0.15 if Cd == 96 else 0.1
    tq, tkv = u("ptq", (B, L, Cd)).to(dev), u("ptkv", (B, L, Cd)).to(dev)
    ln = [t.to(dev) for t in (u("g1", (Cd,), 0.5, 1.5), u("b1", (Cd,), -0.2, 0.2), u("g2", (Cd,), 0.5, 1.5), u("b2", (Cd,), -0.2, 0.2),
                              u("wq%d" % Cd, (Cd, Cd), -wr, wr), u("bq%d" % Cd, (Cd,), -0.2, 0.2), u("wkv%d" % Cd, (2 * Cd, Cd), -wr, wr), u("bkv%d" % Cd, (2 * Cd,), -0.2, 0.2))]
    td = [u("pt%d" % g, ((2 * ws - 1) ** 2, 2)).to(dev) for g, ws in enumerate(windows)]
    tp, wp, sp = arrs(td, windows, shifts)
    head = [dptr(tq), dptr(tkv)] + [dptr(t) for t in ln[:4]] + [1e-5] + [dptr(t) for t in ln[4:]] + [tp, wp, sp, 3, 2]
    out = Buf(dev, (B, L, Cd))
    if Cd == 192:
        ws = nan_ws(dev, lib.dpmn_ln_qkv_window_attn_d32_workspace_bytes())
        rc = lib.dpmn_ln_qkv_window_attn_d32_f32(*head, dptr(out.t), dptr(ws), 1, B, H, W, Cd, st)
        torch.cuda.synchronize()
        assert (rc == 0) == ok, "%s: entry point returned %d" % (test, rc)
        if not ok:
            untouched(test, "cat", out)
            assert bool(torch.isnan(ws).all()), test + ": the rejected call wrote its workspace"
        return
    ws = nan_ws(dev, lib.dpmn_ln_qkv_window_attn_workspace_bytes())
    rc = lib.dpmn_ln_qkv_window_attn_f32(*head, dptr(out.t), dptr(ws), 1, B, H, W, Cd, st)
    torch.cuda.synchronize()
    assert (rc == 0) == ok, "%s: forward returned %d" % (test, rc)
    qo, kvo, out2 = Buf(dev, (B, L, Cd)), Buf(dev, (B, L, 2 * Cd)), Buf(dev, (B, L, Cd))
    rc = lib.dpmn_ln_qkv_window_attn_train_f32(*head, dptr(out2.t), dptr(qo.t), dptr(kvo.t), 0.3, SEED, dptr(ws), B, H, W, Cd, st)
    torch.cuda.synchronize()
    assert (rc == 0) == ok, "%s: training forward returned %d" % (test, rc)
    dq, dkv, dout = Buf(dev, (B * L, Cd)), Buf(dev, (B * L, 2 * Cd)), u("pdout", (B, L, Cd)).to(dev)
    rows = max(lib.dpmn_ln_qkv_window_attn_bwd_part_rows(B, H, W), 1)
    parts = [Buf(dev, (rows, t.numel())) for t in td]
    rc = lib.dpmn_ln_qkv_window_attn_bwd_f32(*head, dptr(dout), dptr(dq.t), dptr(dkv.t), arrs([b.t for b in parts], windows, shifts)[0], 0.3, SEED, dptr(ws), 1, B, H, W, Cd, st)
    torch.cuda.synchronize()
    assert (rc == 0) == ok, "%s: backward returned %d" % (test, rc)
    if not ok:
        for what, b in [("cat", out), ("train cat", out2), ("saved q", qo), ("saved kv", kvo), ("dq", dq), ("dkv", dkv)] + [("partial rows %d" % g, b) for g, b in enumerate(parts)]:
            untouched(test, what, b)
        assert bool(torch.isnan(ws).all()), test + ": a rejected call wrote its workspace"


# ------------------------------------------------------------------------------------------------------------------ negative controls
# valid inputs, a deliberately wrong float64 variant: the comparison must raise -- the shapes and inputs above can tell the kernels'
# likely mistakes apart
@contextlib.contextmanager
def wrong(name, fn):
    old = getattr(ref64, name)
    setattr(ref64, name, fn)
    try:
        yield
    finally:
        setattr(ref64, name, old)


def _roll_other_way(H, W, ws, shift):
    plane = torch.roll(torch.arange(H * W).reshape(H, W), shifts=(shift, shift), dims=(0, 1))
    return plane.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1)


def _rel_index_swapped(ws):
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).reshape(2, -1)
    rel = coords[:, :, None] - coords[:, None, :] + (ws - 1)
    return rel[1] * (2 * ws - 1) + rel[0]


def _labels_ws_shift_exchanged(H, W, ws, shift):
    img = torch.zeros(H, W, dtype=torch.long)
    cnt = 0
    for hs in (slice(0, -shift), slice(-shift, -ws), slice(-ws, None)):
        for wsl in (slice(0, -shift), slice(-shift, -ws), slice(-ws, None)):
            img[hs, wsl] = cnt
            cnt += 1
    return img.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)


def _drop_index_head_group_exchanged(B, G, g, L, N):
    import numpy as np
    b, win, h, n, m = np.meshgrid(np.arange(B), np.arange(L // N), np.arange(2), np.arange(N), np.arange(N), indexing="ij")
    return (((b * 2 + h) * G + g) * L + win * N + n) * N + m


_good_src = ref64._wattn_src


def _gather_hw_exchanged(H, W, ws, shift):
    return _good_src(W, H, ws, shift)


CONTROLS = [("roll in the other direction", "_wattn_src", _roll_other_way, 0.0), ("bias index with (i, j) swapped", "_wattn_rel_index", _rel_index_swapped, 0.0),
            ("region thresholds with ws and shift exchanged", "_wattn_labels", _labels_ws_shift_exchanged, 0.0),
            ("dropout index with head and group exchanged", "_wattn_drop_index", _drop_index_head_group_exchanged, 0.3),
            ("H and W exchanged in the gather", "_wattn_src", _gather_hw_exchanged, 0.0)]


# (4, 16) on k_window_attn, (8, 16) on the matrix cores, (8, 32): 8 x 16 and 16 x 8 (non-square), shifts 1, ws / 2, ws - 1
@pytest.mark.parametrize("ws,D", [(4, 16), (8, 16), (8, 32)])
@pytest.mark.parametrize("c", range(len(CONTROLS)))
def test_negative_controls(dev, c, ws, D):
    what, name, fn, p = CONTROLS[c]
    windows, shifts = (ws,) * 3, (1, ws // 2, ws - 1)
    for H, W in ((8, 16), (16, 8)):
        q, kv, tables, dout = _inputs("cont", windows, D, 3, H, W)
        out, rc = fwd_gpu(dev, "cont", windows, shifts, D, 3, H, W, p)
        assert rc == 0
        ref, ref32, floor = _fwd_ref("cont", windows, shifts, D, 3, H, W, p)
        judge("control baseline", "out", out, ref, ref32, floor)
        with wrong(name, fn):
            bad, bad32 = both(ref64.window_attn, q, kv, tables, list(windows), list(shifts), H, W, p, SEED)
        with pytest.raises(AssertionError, match="GPU max err"):
            check_derived("control[%s]" % what, "out", out.t, bad, bad32, floor)
        dq, dkv, dt, _ = bwd_gpu(dev, windows, shifts, D, 3, H, W, p, False)
        with wrong(name, fn):
            (bq, bkv, _), (bq32, bkv32, _) = both(ref64.window_attn_bwd, q, kv, tables, list(windows), list(shifts), H, W, dout, p, SEED)
        with pytest.raises(AssertionError, match="GPU max err"):
            check_derived("control[%s]" % what, "dq", dq.t, bq, bq32, floor)
        with pytest.raises(AssertionError, match="GPU max err"):
            check_derived("control[%s]" % what, "dkv", dkv.t, bkv, bkv32, floor)
