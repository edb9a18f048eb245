"""GPU parity of the small hand-written BACKWARD kernels -- k_sk_select / k_sk_select_bwd / k_sk_gate_bwd / k_sk_feats_grad, k_dwconv_bwd
(banded and persistent KEEP form), k_act_fwd, k_axpby, k_rowsum_mod, k_tail_elem_fwd / _bwd (csrc/backward_pgrm.hip), k_tn_reduce behind
dpmn_rows_reduce_f32, k_colsum, k_act_bwd (backward.hip), the channel-gate backward and the L1 loss (tail of conv_bwd.hip) -- each called
alone through _abi.lib against its float64 reference (tests/ref64.py, pinned to torch.autograd by tests/test_ref64.py) at the smallest
shapes that cross its hand-written boundaries: unroll tails, partial blocks, thread-takes-two-columns, one band / several bands / the
persistent path, null optional pointers, overwrite / accumulate / partial-row modes.

Buffers.  An output the kernel OVERWRITES starts NaN-filled and must come back NaN-free; an output it ACCUMULATES into starts from a
non-zero prefill and is compared with prefill + reference; every output carries a sentinel row (or element) past its end that must be
unchanged; the atomics-free `det` entry points run twice and must be bitwise equal.

Tolerances.  No constant of this file's own: check_derived of tests/test_gpu_small_kernels.py.  The reference formula (the same
function of ref64.py, dtype=float32) is evaluated in fp32 torch on the CPU and the kernel is allowed 8 x that evaluation's max error
against float64 -- another summation order plus hardware exp / rcp -- with a floor of 1e-6.  A reduction's fp32 CPU evaluation adds the
same number of terms, so the bound follows the length of the sum by itself.  The pure sums (colsum, rowsum_mod, rows_reduce) take their
inputs on a 2^-10 grid, where every order of addition is exact in fp32 and the expected error is 0 (see grid()).
The floor is raised only where the kernel evaluates GELU / GELU' through erf_as (Abramowitz-Stegun 7.1.26, |error in erf| <= 1.5e-7),
which the fp32 CPU evaluation (libm erf) does not share: GELU(x) = x (1 + erf) / 2 and GELU'(x) = (1 + erf) / 2 + x phi(x) carry
0.5 * 1.5e-7 * |x| and 0.5 * 1.5e-7 of it, so an output o = sum_i f_i GELU'(.) (or f_i GELU(.)) is off by at most
0.5 * 1.5e-7 * sum_i |f_i| (|x_i|).  For the depthwise backward (_dw_floors) that is, per output, with E = 0.5 * 1.5e-7:
  dy = dg GELU'(gpre)                      E |dg| per pixel
  x  = GELU(P) mask                        E |P| mask per pixel
  db = sum dy                              E sum |dg|
  dw = sum dy x(shifted)                   E (sum |dg| |x| + sum |dy| |P| mask), shifted alike
  dP = (sum_k dy w_k) mask GELU'(P)        E (sum_k |dg| |w_k|) mask |GELU'(P)| + E |sum_k dy w_k| mask
every factor computed from the inputs and the float64 reference, never from the kernel's output.  In every other kernel here the
factor is below 1e-6 / E = 13 (the gate MLP's operands are below 1, sk_feats_grad multiplies GELU' by |dS| / L <= 1, the activation
kernels by |x| <= 6 or |dy| <= 1): the plain floor holds there."""
import functools
import itertools

import pytest
import torch

import ref64
from dpmn_amd.utils import synth
from helpers import record
from test_gpu_small_kernels import check_derived

pytestmark = pytest.mark.gpu
SENT = -12345.0
E_ERF = 0.5 * 1.5e-7
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=90):
    return synth.uniform(name, shape, lo, hi, seed)


def abi():
    from dpmn_amd import _abi
    return _abi.lib, _abi.check, _abi.dptr, _abi.stream()


class Buf:
    """A device output of `shape` with one sentinel row (last axis; one element for a vector) past its end.  fill=None: NaN (an
    output the kernel overwrites); a CPU tensor: the prefill of an output the kernel accumulates into."""

    def __init__(self, dev, shape, fill=None):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        self.n, self.fill = n, fill
        self.flat = torch.empty(n + (shape[-1] if len(shape) > 1 else 1), device=dev)
        self.flat[n:] = SENT
        self.t = self.flat[:n].view(shape)
        if fill is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill)

    def check(self, test, what, ref, ref32, floor=1e-6):
        """sentinel intact; NaN-free; prefill + reference within the derived bound"""
        assert bool((self.flat[self.n:] == SENT).all()), "%s %s: wrote past the end of the output" % (test, what)
        nan = int(torch.isnan(self.t).sum())
        assert nan == 0, "%s %s: %d of %d outputs %s" % (test, what, nan, self.n, "never written" if self.fill is None else "NaN")
        ref, ref32 = ref.reshape(self.t.shape), ref32.reshape(self.t.shape)
        if self.fill is not None:
            ref, ref32 = self.fill.double() + ref, self.fill + ref32
        check_derived(test, what, self.t, ref, ref32, floor)
        return self.t


def pre(name, shape):
    return u("prefill_" + name, shape, -1.0, 1.0)


def grid(t, bits=10):
    """rounded to multiples of 2^-bits.  The inputs (and prefills) of the pure sums -- colsum, rowsum_mod, rows_reduce: at most 5005 terms
    of magnitude <= 1 -- are taken on this grid: every partial sum then needs at most 13 + 10 bits, so it is exact in fp32 in ANY order
    of addition, the fp32 CPU evaluation's error is 0, the bound is the bare 1e-6 floor and the expected error is exactly 0.  With
    continuous inputs these checks measure the order of addition instead of the indexing they are here for: k_colsum at N = 4 adds
    its 256 row-lane partials one after the other (~sqrt(256) roundings against the CPU's pairwise sum; measured 0.94 of the bound at
    M = 1027), and in the atomic entry points the order -- so pass or fail -- would change from run to run."""
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


def both(fn, *a, **k):
    """the reference in float64 and the same formula in float32"""
    return fn(*a, **k), fn(*a, dtype=F32, **k)


def same_bits(test, what, a, b):
    assert torch.equal(a, b), "%s %s: two runs differ in %d elements" % (test, what, int((a != b).sum()))


# ------------------------------------------------------------------------------------------------------------------ SK select
@functools.lru_cache(maxsize=None)
def _sel_case(B, L, C, G):
    cg = C // G
    cat, A, dV = u("cat", (B * L, C)), u("A", (B, G, cg)), u("dV", (B * L, cg))
    return cat, A, dV, both(ref64.sk_select, cat, A, L), both(ref64.sk_select_bwd, cat, A, dV, L)


# 32 rows per block, 128 threads, a 4-row unroll: L = 1, 3 (tail only), 4 (unroll only), 33, 37 (a second block of 1 / 5 rows), 64 (two
# whole blocks), 95 (a block of 31 = 7 unrolls + 3); C = 192: a thread takes two columns; G = 1: cg = C
@pytest.mark.parametrize("C,G", [(96, 2), (96, 3), (192, 3), (64, 1)])
def test_sk_select(dev, C, G):
    lib, check, dptr, st = abi()
    cg = C // G
    for B, L in itertools.product((1, 3), (1, 3, 4, 33, 37, 64, 95)):
        test = "sk_select[B%d L%d C%d G%d]" % (B, L, C, G)
        cat, A, dV, (V, V32), ((dcat, dA, parts), (dcat32, dA32, parts32)) = _sel_case(B, L, C, G)
        M, nblk = B * L, (L + 31) // 32
        catd, Ad, dVd = cat.to(dev), A.to(dev), dV.to(dev)
        out = Buf(dev, (M, cg))
        check(lib.dpmn_sk_select_only_f32(dptr(catd), dptr(Ad), dptr(out.t), M, L, C, G, st))
        out.check(test, "V", V, V32)
        # atomic path: dcat and dA accumulated
        bc, bA = Buf(dev, (M, C), pre("dcat", (M, C))), Buf(dev, (B, G, cg), pre("dA", (B, G, cg)))
        check(lib.dpmn_sk_select_bwd_f32(dptr(catd), dptr(Ad), dptr(dVd), dptr(bc.t), dptr(bA.t), B, L, C, G, st))
        bc.check(test, "bwd dcat", dcat, dcat32)
        bA.check(test, "bwd dA", dA, dA32)
        # det: dcat accumulated, the blocks' partial rows of dA stored; det_set: dcat stored too, never read (NaN-poisoned)
        for name, fn, fill in (("det", lib.dpmn_sk_select_bwd_det_f32, pre("dcat", (M, C))), ("det_set", lib.dpmn_sk_select_bwd_det_set_f32, None)):
            runs = []
            for _ in range(2):
                bc, bp = Buf(dev, (M, C), fill), Buf(dev, (nblk, B, C))
                check(fn(dptr(catd), dptr(Ad), dptr(dVd), dptr(bc.t), dptr(bp.t), B, L, C, G, st))
                runs.append((bc.t, bp.t))
            same_bits(test, name + " dcat", runs[0][0], runs[1][0])
            same_bits(test, name + " dA_part", runs[0][1], runs[1][1])
            bc.check(test, name + " dcat", dcat, dcat32)
            got = bp.check(test, name + " dA_part", parts, parts32)
            tot = got[0].clone()
            for k in range(1, nblk):          # added in block order, as the gate backward adds them
                tot += got[k]
            check_derived(test, name + " dA_part rows added in block order", tot.reshape(B, G, cg), dA, dA32)


# ------------------------------------------------------------------------------------------------------------------ SK gate backward
PPI, NPARTS = (1, 7, 8, 9, 17), (1, 3, 8, 9)
GATE_CASES = [(i,) + c for i, c in enumerate(itertools.product((8, 16, 24, 48), (96, 192), (2, 3), (1, 3)))]      # 32 = every (dmid, C, G, B)


@functools.lru_cache(maxsize=None)
def _gate_case(i, dmid, C, G, B):
    """parts_per_image and nparts cycle with periods 5 and 4 over the 32 cases: every value of each, and every pair of the two"""
    ppi, nparts = PPI[i % 5], NPARTS[i % 4]
    L = 32 * ppi - 5 if ppi > 1 else 27
    partial = u("partial", (B * ppi, C), 0.0, 30.0)           # column sums of GELU(feats) over 32 token rows
    w1, b1, w2, b2 = u("fc1_w", (dmid, C), -0.2, 0.2), u("fc1_b", (dmid,), -0.3, 0.3), u("fc2_w", (C, dmid), -0.5, 0.5), u("fc2_b", (C,), -0.3, 0.3)
    A = ref64.sk_gate(ref64.sk_pool(partial, ppi, L), w1, b1, w2, b2, G).float()      # the float64 forward's A, as the kernel's input
    dA_part = u("dA_part", (nparts, B, C), -1.0, 1.0)
    dA = dA_part[0].reshape(B, G, C // G).contiguous()
    r_one = both(ref64.sk_gate_bwd, partial, ppi, L, w1, b1, w2, A, dA)
    r_sum = (ref64.sk_gate_bwd(partial, ppi, L, w1, b1, w2, A, dA_part.double().sum(0).reshape(B, G, -1)),
             ref64.sk_gate_bwd(partial, ppi, L, w1, b1, w2, A, dA_part.sum(0).reshape(B, G, -1), dtype=F32))
    return ppi, nparts, L, partial, w1, b1, w2, A, dA, dA_part, r_one, r_sum


# row_sum: 8 loads per pass + tail -- 1, 7 (tail only), 8 (one pass), 9, 17 (passes + 1) rows, for the pooled partials and (det) for
# dA's partial rows; 16 outputs of the gate MLP per pass of 128 threads: dmid = 8 (half a pass), 16, 24 (1.5), 48 (3)
@pytest.mark.parametrize("i,dmid,C,G,B", GATE_CASES)
def test_sk_gate_bwd(dev, i, dmid, C, G, B):
    lib, check, dptr, st = abi()
    ppi, nparts, L, partial, w1, b1, w2, A, dA, dA_part, (r, r32), (s, s32) = _gate_case(i, dmid, C, G, B)
    test = "sk_gate_bwd[ppi%d nparts%d dmid%d C%d G%d B%d]" % (ppi, nparts, dmid, C, G, B)
    pd, w1d, b1d, w2d, Ad, dAd = (t.to(dev) for t in (partial, w1, b1, w2, A, dA))
    names = ("dfc1_w", "dfc1_b", "dfc2_w", "dfc2_b")
    dS = Buf(dev, (B, C))
    g = {k: Buf(dev, r[k].shape, pre(k, r[k].shape)) for k in names}
    check(lib.dpmn_sk_gate_bwd_f32(dptr(pd), ppi, L, dptr(w1d), dptr(b1d), dptr(w2d), dptr(Ad), dptr(dAd), dptr(dS.t),
                                   dptr(g["dfc1_w"].t), dptr(g["dfc1_b"].t), dptr(g["dfc2_w"].t), dptr(g["dfc2_b"].t), B, C, G, dmid, st))
    dS.check(test, "dS", r["dS"], r32["dS"])
    for k in names:
        g[k].check(test, k, r[k], r32[k])
    # det: dA as nparts partial rows added in row order, the weight gradients as per-image rows for dpmn_rows_reduce_f32
    dpd, runs = dA_part.to(dev), []
    for _ in range(2):
        dS, p2, p1 = Buf(dev, (B, C)), Buf(dev, (B, C * dmid + C)), Buf(dev, (B, dmid * C + dmid))
        check(lib.dpmn_sk_gate_bwd_det_f32(dptr(pd), ppi, L, dptr(w1d), dptr(b1d), dptr(w2d), dptr(Ad), dptr(dpd), nparts, dptr(dS.t),
                                           dptr(p2.t), dptr(p1.t), B, C, G, dmid, st))
        f2, f1 = pre("w2row", (C * dmid + C,)), pre("w1row", (dmid * C + dmid,))
        g2, g1 = Buf(dev, (C * dmid + C,), f2), Buf(dev, (dmid * C + dmid,), f1)
        check(lib.dpmn_rows_reduce_f32(dptr(p2.t), dptr(g2.t), dptr(g2.t[C * dmid:]), C * dmid, C, B, st))
        check(lib.dpmn_rows_reduce_f32(dptr(p1.t), dptr(g1.t), dptr(g1.t[dmid * C:]), dmid * C, dmid, B, st))
        runs.append((dS.t, p2.t, p1.t, g2.t, g1.t))
    for k, what in enumerate(("dS", "wpart2", "wpart1", "reduced fc2", "reduced fc1")):
        same_bits(test, "det " + what, runs[0][k], runs[1][k])
    dS.check(test, "det dS", s["dS"], s32["dS"])
    p2.check(test, "det wpart2", s["wpart2"], s32["wpart2"])
    p1.check(test, "det wpart1", s["wpart1"], s32["wpart1"])
    g2.check(test, "det [dfc2_w | dfc2_b] by rows_reduce", torch.cat([s["dfc2_w"].reshape(-1), s["dfc2_b"]]), torch.cat([s32["dfc2_w"].reshape(-1), s32["dfc2_b"]]))
    g1.check(test, "det [dfc1_w | dfc1_b] by rows_reduce", torch.cat([s["dfc1_w"].reshape(-1), s["dfc1_b"]]), torch.cat([s32["dfc1_w"].reshape(-1), s32["dfc1_b"]]))


# ------------------------------------------------------------------------------------------------------------------ SK feats gradient
@functools.lru_cache(maxsize=None)
def _feats_case(B, L, C):
    feats, dout, dS = u("feats", (B * L, C), -6.0, 6.0), u("dout", (B * L, C)), u("dS", (B, C))
    feats.reshape(-1)[::11] = 6.0            # GELU' = 1 and 0 up to 1e-8
    feats.reshape(-1)[5::11] = -6.0
    feats.reshape(-1)[3::11] = 0.0
    return feats, dout, dS, both(ref64.sk_feats_grad, dout, feats, dS, L)


# M C = 96 ... 18624, none a multiple of the 256-thread block (C = 97 keeps L = 64 off it)
@pytest.mark.parametrize("C", [96, 97])
def test_sk_feats_grad(dev, C):
    lib, check, dptr, st = abi()
    for B, L in itertools.product((1, 3), (1, 5, 64)):
        if (B * L * C) % 256 == 0:
            continue                          # (C = 96, L = 64)
        test = "sk_feats_grad[B%d L%d C%d]" % (B, L, C)
        feats, dout, dS, (ref, ref32) = _feats_case(B, L, C)
        doutd, featsd, dSd, out = dout.to(dev), feats.to(dev), dS.to(dev), Buf(dev, (B * L, C))      # (every operand held until the check)
        check(lib.dpmn_sk_feats_grad_f32(dptr(doutd), dptr(featsd), dptr(dSd), dptr(out.t), B * L, L, C, st))
        out.check(test, "dfeats", ref, ref32, max(1e-6, E_ERF * float(dS.abs().max()) / L))


# ------------------------------------------------------------------------------------------------------------------ depthwise 3 x 3 backward
DW_SEED = 0x5DEECE66D
FLAGS = {"plain": (False, 0, 0), "gpre": (True, 0, 0), "in_gelu": (True, 1, 0), "all": (True, 1, 1)}


@functools.lru_cache(maxsize=None)
def _drop_mask(n, p):
    """the mask of dpmn_dropout_f32 (pinned to the oracle's hash by test_dropout_kernel_masks_equal_oracle_hash): ones through the kernel"""
    from dpmn_amd import ops
    return ops.dropout(torch.ones(n, device="cuda:0"), p, DW_SEED).cpu()


def _dw_floors(P, dg, w, gpre, in_gelu, out_gelu, mask):
    """the erf_as allowance of (dP, dw, db): see the module docstring"""
    P, dg, w = P.double(), dg.double(), w.double()
    m = torch.ones_like(P) if mask is None else mask.double().reshape(P.shape)
    dy = dg * ref64.gelu_grad(gpre) if gpre is not None else dg
    x = (ref64.gelu(P) if in_gelu else P) * m
    fP = torch.zeros_like(P)
    fw, fb = torch.zeros(w.shape[0], 9, dtype=torch.float64), 0.0
    if gpre is not None:
        fP = fP + ref64.dwconv3x3_bwd(P, dg.abs(), w.abs())[0] * m * (ref64.gelu_grad(P).abs() if out_gelu else 1.0)
        fw = fw + ref64.dwconv3x3_bwd(x.abs(), dg.abs(), w)[1]
        fb = float(dg.abs().sum((0, 2, 3)).max())
    if in_gelu:
        fw = fw + ref64.dwconv3x3_bwd(P.abs() * m, dy.abs(), w)[1]
    if out_gelu:
        fP = fP + ref64.dwconv3x3_bwd(P, dy, w)[0].abs() * m
    return tuple(max(1e-6, E_ERF * float(f)) for f in (fP.max(), fw.max(), fb))


@functools.lru_cache(maxsize=None)
def _dw_case(B, Ch, r, flags, p_drop):
    gp, in_gelu, out_gelu = FLAGS[flags]
    shape = (B, Ch, r, r)
    # |dg| <= 2 / (r sqrt(B)): db and dw are sums over B r^2 pixels, and db is a SINGLE number for Ch = 1 -- with dg of order 1 it would be
    # of order r (up to 64, one ulp = 3.8e-6), where the rule's 1e-6 floor is below one rounding of the output itself and the fp32 CPU
    # evaluation of one number can be exact by chance; this keeps |db| and |dw| below 8, where the floor is two ulp
    s = min(1.0, 2.0 / (r * B ** 0.5))
    P, dg, w = u("P", shape, -3.0, 3.0), u("dg", shape, -s, s), u("dw_w", (Ch, 3, 3), -0.5, 0.5)
    gpre = u("gpre", shape, -3.0, 3.0) if gp else None
    mask = _drop_mask(B * Ch * r * r, p_drop) if p_drop > 0 else None
    if mask is not None:          # 0 or 1 / (1 - p), some of each once there are enough elements
        assert bool(((mask == 0) | ((mask - 1.0 / (1.0 - p_drop)).abs() < 1e-6)).all()) and bool((mask != 0).any())
        assert mask.numel() < 256 or bool((mask == 0).any())
    ref, ref32 = both(ref64.dwconv3x3_bwd, P, dg, w, gpre, bool(in_gelu), bool(out_gelu), mask)
    return P, dg, w, gpre, ref, ref32, _dw_floors(P, dg, w, gpre, in_gelu, out_gelu, mask)


def _dw_run(dev, test, B, Ch, r, flags, p_drop, entries):
    lib, check, dptr, st = abi()
    gp, in_gelu, out_gelu = FLAGS[flags]
    P, dg, w, gpre, ref, ref32, floors = _dw_case(B, Ch, r, flags, p_drop)
    Pd, dgd, wd, gd = P.to(dev), dg.to(dev), w.to(dev), (gpre.to(dev) if gp else None)
    fw, fb = pre("dw", (Ch, 9)), pre("db", (Ch,))

    def outs():
        return Buf(dev, (B, Ch, r, r)), Buf(dev, (Ch, 9), fw), Buf(dev, (Ch,), fb)

    def verify(name, o):
        for buf, what, k in zip(o, ("dP", "dw", "db"), range(3)):
            buf.check(test, name + " " + what, ref[k], ref32[k], floors[k])

    if "plain" in entries:
        o = outs()
        check(lib.dpmn_dwconv3x3_bwd_f32(dptr(Pd), dptr(dgd), dptr(wd), dptr(o[0].t), dptr(o[1].t), dptr(o[2].t), B, Ch, r, st))
        verify("plain entry", o)
    if "atomic" in entries:
        o = outs()
        check(lib.dpmn_dwconv3x3_bwd_fused_f32(dptr(Pd), dptr(dgd), dptr(gd, True), dptr(wd), dptr(o[0].t), dptr(o[1].t), dptr(o[2].t),
                                               in_gelu, out_gelu, p_drop, DW_SEED, B, Ch, r, st))
        verify("fused", o)
    if "det" in entries:
        nws = lib.dpmn_dwconv3x3_bwd_det_bytes(B, Ch, r) // 4
        runs = []
        for _ in range(2):
            o, ws = outs(), Buf(dev, (nws,))
            check(lib.dpmn_dwconv3x3_bwd_fused_det_f32(dptr(Pd), dptr(dgd), dptr(gd, True), dptr(wd), dptr(o[0].t), dptr(o[1].t), dptr(o[2].t),
                                                       in_gelu, out_gelu, p_drop, DW_SEED, B, Ch, r, dptr(ws.t), nws * 4, st))
            runs.append([b.t for b in o] + [ws.t])
        for k, what in enumerate(("dP", "dw", "db", "partial rows")):
            same_bits(test, "det " + what, runs[0][k], runs[1][k])
        assert bool((ws.flat[ws.n:] == SENT).all()) and not torch.isnan(ws.t).any(), "%s det: partial-row workspace overrun or not fully written" % test
        verify("det", o)


# dwconv_band_rows: r > 32 and r % 16 == 0 -> bands of 16 rows, else the whole plane.  r = 4 (one float4 per row, a 6-row tile), 36 (ONE band
# of 36 rows: 9 float4 per row, 53.5 KB of LDS -- above the 48 KB default), 48 (3 bands), 32 (one band; the persistent KEEP kernel when all
# three GELUs are on), 64 (4 bands).  Planes 1, 4, 5, 9: a partial block of four waves, a whole one, one + 1, two + 1.
@pytest.mark.parametrize("r", [4, 36, 48, 32, 64])
def test_dwconv3x3_bwd(dev, r):
    from dpmn_amd._abi import lib
    rb = r if not (r > 32 and r % 16 == 0) else 16
    assert lib.dpmn_dwconv3x3_bwd_det_bytes(2, 3, r) == 2 * (r // rb) * 3 * 10 * 4      # the band split this test's choice of r relies on
    for (B, Ch), flags, p_drop in itertools.product(((1, 1), (2, 2), (1, 5), (3, 3)), FLAGS, (0.0, 0.1)):
        path = "" if flags != "all" else (" KEEP" if r == 32 else " banded")
        test = "dwconv3x3_bwd[r%d B%d Ch%d %s%s p%.1f]" % (r, B, Ch, flags, path, p_drop)
        _dw_run(dev, test, B, Ch, r, flags, p_drop, ("atomic", "det") + (("plain",) if flags == "plain" and p_drop == 0.0 else ()))


def test_dwconv3x3_bwd_keep_persistent(dev):
    """more planes than the persistent KEEP grid has waves (2 blocks x 4 waves per CU): waves take several planes each, and the last
    round's prefetch is clamped to the wave's current plane (plane + pstep < planes)"""
    B = 3
    Ch = 8 * torch.cuda.get_device_properties(dev).multi_processor_count // B + 1
    _dw_run(dev, "dwconv3x3_bwd[KEEP persistent B%d Ch%d p0.1]" % (B, Ch), B, Ch, 32, "all", 0.1, ("atomic", "det"))


# ------------------------------------------------------------------------------------------------------------------ activations
@functools.lru_cache(maxsize=None)
def _act_case(name, n):
    code, slope = ref64.ACT_CODES[name], 0.25
    x, dy = u("act_x", (n,), -6.0, 6.0), u("act_dy", (n,))
    x[::9] = 0.0                              # the kink: value 0, the negative side's slope
    return code, slope, x, dy, both(ref64.act, x, code, slope), both(ref64.act_grad, x, code, slope)


# n = 4: one float4; 1020, 1028: a last block of 255 / 1 float4
@pytest.mark.parametrize("name", sorted(ref64.ACT_CODES))
def test_act_fwd_bwd(dev, name):
    lib, check, dptr, st = abi()
    for n in (4, 1020, 1028):
        test = "act[%s n%d]" % (name, n)
        code, slope, x, dy, (y, y32), (g, g32) = _act_case(name, n)
        xd, dyd, out = x.to(dev), dy.to(dev), Buf(dev, (n,))
        check(lib.dpmn_act_fwd_f32(dptr(xd), dptr(out.t), code, slope, n, st))
        out.check(test, "fwd", y, y32)
        out = Buf(dev, (n,))
        check(lib.dpmn_act_bwd_f32(dptr(dyd), dptr(xd), dptr(out.t), code, slope, n, st))
        out.check(test, "bwd", dy.double() * g, dy * g32)


# ------------------------------------------------------------------------------------------------------------------ axpby
@pytest.mark.parametrize("n", [1, 255, 257])
def test_axpby(dev, n):
    lib, check, dptr, st = abi()
    x, z, y0 = u("ax_x", (n,)), u("ax_z", (n,)), pre("ax_y", (n,))
    xd, zd = x.to(dev), z.to(dev)
    for with_z, acc in itertools.product((False, True), (0, 1)):
        test = "axpby[n%d%s%s]" % (n, " z" if with_z else "", " accumulate" if acc else "")
        out = Buf(dev, (n,), y0 if acc else None)
        check(lib.dpmn_axpby_f32(dptr(xd), dptr(zd if with_z else None, True), dptr(out.t), 0.75, -1.5, acc, n, st))
        zz = z if with_z else None
        out.check(test, "y", ref64.axpby(x, zz, None, 0.75, -1.5, False), ref64.axpby(x, zz, None, 0.75, -1.5, False, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------ reductions
# cols & 3 == 0: float4 loads (64: a quarter of the lanes, 100: 25 lanes, 260: one pass + 1 lane); else scalar (5 lanes, 1001 = 15 passes
# + 41 lanes); four rows per block: 9, 4, 35 rows
@pytest.mark.parametrize("mod,k", [(3, 3), (4, 1), (7, 5)])
@pytest.mark.parametrize("cols", [5, 64, 100, 260, 1001])
def test_rowsum_mod(dev, cols, mod, k):
    lib, check, dptr, st = abi()
    rows = mod * k
    test = "rowsum_mod[cols%d mod%d rows%d]" % (cols, mod, rows)
    x = grid(u("rs_x", (rows, cols)))
    ref, ref32 = both(ref64.rowsum_mod, x, mod)
    xd, fill = x.to(dev), grid(pre("rs_out", (mod,)))
    out = Buf(dev, (mod,), fill)
    check(lib.dpmn_rowsum_mod_f32(dptr(xd), dptr(out.t), rows, cols, mod, st))
    out.check(test, "atomic", ref, ref32)
    runs = []
    for _ in range(2):
        out, ws = Buf(dev, (mod,), fill), Buf(dev, (rows,))
        check(lib.dpmn_rowsum_mod_det_f32(dptr(xd), dptr(out.t), rows, cols, mod, dptr(ws.t), rows * 4, st))
        runs.append((out.t, ws.t))
    same_bits(test, "det out", runs[0][0], runs[1][0])
    same_bits(test, "det row sums", runs[0][1], runs[1][1])
    ws.check(test, "det row sums", x.double().sum(1), x.sum(1))
    out.check(test, "det", ref, ref32)


# 64 columns per block, rows in four groups of every fourth: NK + N = 5 (db null), 64, 960 (15 blocks), 131 (2 blocks + 3); rows 1, 3
# (groups without a row), 4, 5, 9
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("NK,N", [(5, 0), (60, 4), (864, 96), (100, 31)])
def test_rows_reduce(dev, NK, N, rows):
    lib, check, dptr, st = abi()
    test = "rows_reduce[NK%d N%d rows%d]" % (NK, N, rows)
    part = grid(u("rr_part", (rows, NK + N)))
    (dw, db), (dw32, db32) = both(ref64.rows_reduce, part, NK, N)
    partd, runs = part.to(dev), []
    for _ in range(2):
        bw, bb = Buf(dev, (NK,), grid(pre("rr_dw", (NK,)))), (Buf(dev, (N,), grid(pre("rr_db", (N,)))) if N else None)
        check(lib.dpmn_rows_reduce_f32(dptr(partd), dptr(bw.t), dptr(bb.t if N else None, True), NK, N, rows, st))
        runs.append((bw.t, bb.t if N else bw.t))
    same_bits(test, "dw", runs[0][0], runs[1][0])
    same_bits(test, "db", runs[0][1], runs[1][1])
    bw.check(test, "dw", dw, dw32)
    if N:
        bb.check(test, "db", db, db32)


# cols4 = N / 4 = 1, 24, 25 (256 / 25 = 10 row lanes, 6 idle threads), 96 (2 row lanes, 64 idle), 256 (one row lane); 256 rows per block:
# M = 1, 255, 256, 257, 1027 (4 blocks + 3 rows; with one row lane the 4-rows-in-flight loop and its tail)
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1027])
@pytest.mark.parametrize("N", [4, 96, 100, 384, 1024])
def test_colsum(dev, N, M):
    lib, check, dptr, st = abi()
    test = "colsum[M%d N%d]" % (M, N)
    dy = grid(u("cs_dy", (M, N)))
    ref, ref32 = both(ref64.colsum, dy)
    dyd, fill = dy.to(dev), grid(pre("cs_db", (N,)))
    out = Buf(dev, (N,), fill)
    check(lib.dpmn_colsum_f32(dptr(dyd), dptr(out.t), M, N, st))
    out.check(test, "atomic", ref, ref32)
    nb, runs = (M + 255) // 256, []
    for _ in range(2):
        out, ws = Buf(dev, (N,), fill), Buf(dev, (nb, N))
        check(lib.dpmn_colsum_det_f32(dptr(dyd), dptr(out.t), M, N, dptr(ws.t), nb * N * 4, st))
        runs.append((out.t, ws.t))
    same_bits(test, "det db", runs[0][0], runs[1][0])
    same_bits(test, "det block rows", runs[0][1], runs[1][1])
    ws.check(test, "det block rows", torch.stack([dy[i:i + 256].double().sum(0) for i in range(0, M, 256)]), torch.stack([dy[i:i + 256].sum(0) for i in range(0, M, 256)]))
    out.check(test, "det", ref, ref32)


# ------------------------------------------------------------------------------------------------------------------ PGRM tail
@functools.lru_cache(maxsize=None)
def _tail_case(B, n, H, W):
    c1 = u("c1", (B, H, W, 12), -2.0, 2.0)
    c1.reshape(-1)[::5] = 0.0                 # exact zeros: value 0, slope 0.01 (c1 > 0 ? 1 : 0.01)
    assert bool((c1 < 0).any())
    wl = tuple(u("wl%d" % i, (3, 2 * H, 2 * W)) for i in range(max(n, 1)))
    res = tuple(u("res%d" % i, (B, 3, 2 * H, 2 * W)) for i in range(n))
    dout = u("tail_dout", (B, 3, 2 * H, 2 * W))
    return c1, wl, res, dout, both(ref64.tail_elem, c1, wl, res), both(ref64.tail_elem_bwd, dout, c1, wl, res)


# the backward runs four images per iteration + a tail: B = 1, 3 (tail only), 4 (one iteration), 5, 9; n_residuals 0 and 1 (no residual
# term: residual 0 is skipped), 2, 4, 8 (the limit: 7 terms); 3 * 2H * 2W = 72 (a partial block) and 3072 (12 blocks)
@pytest.mark.parametrize("H,W", [(2, 3), (8, 32)])
@pytest.mark.parametrize("n", [0, 1, 2, 4, 8])
def test_tail_elem(dev, n, H, W):
    from dpmn_amd import _abi
    lib, check, dptr, st = abi()

    def ptrs(tensors):
        arr = (_abi.fp * max(len(tensors), 1))()
        for i, t in enumerate(tensors):
            if t is not None:
                arr[i] = dptr(t)
        return arr

    for B in (1, 3, 4, 5, 9):
        test = "tail_elem[B%d n%d %dx%d]" % (B, n, H, W)
        c1, wl, res, dout, (out, out32), ((dc1, dwl, dres), (dc132, dwl32, dres32)) = _tail_case(B, n, H, W)
        c1d, wld, resd, doutd = c1.to(dev), [t.to(dev) for t in wl], [t.to(dev) for t in res], dout.to(dev)
        o = Buf(dev, out.shape)
        check(lib.dpmn_pgrm_tail_elem_f32(dptr(c1d), ptrs(wld), ptrs(resd), n, dptr(o.t), B, H, W, st))
        o.check(test, "fwd", out, out32)
        for mode in (("null", "all", "mix") if n >= 2 else ("null", "all")):
            bc = Buf(dev, c1.shape)
            bw = [Buf(dev, wl[i].shape, pre("dwl%d" % i, wl[i].shape)) for i in range(max(n, 1))]
            # residual 0 takes no part: its gradient buffer, when given, keeps its contents
            br = [None if mode == "null" or (mode == "mix" and i % 2 == 0 and i > 0) else
                  Buf(dev, res[i].shape, pre("dres%d" % i, res[i].shape)) for i in range(n)]
            check(lib.dpmn_pgrm_tail_elem_bwd_f32(dptr(doutd), dptr(c1d), ptrs(wld), ptrs(resd), None if mode == "null" else ptrs([b and b.t for b in br]),
                                                  ptrs([b.t for b in bw]), n, dptr(bc.t), B, H, W, st))
            bc.check(test, mode + " dc1", dc1, dc132)
            for i, b in enumerate(bw):
                b.check(test, mode + " dwl%d" % i, dwl[i], dwl32[i])
            for i, b in enumerate(br):
                if b is not None and i == 0:
                    assert torch.equal(b.flat[:b.n].cpu(), b.fill.reshape(-1)) and bool((b.flat[b.n:] == SENT).all()), "%s %s: dresiduals[0] was touched" % (test, mode)
                elif b is not None:
                    b.check(test, mode + " dres%d" % i, dres[i], dres32[i])


# ------------------------------------------------------------------------------------------------------------------ channel gate backward
@functools.lru_cache(maxsize=None)
def _se_case(C, Cmid, B, P):
    x, dg = u("se_x", (B, P, C), -2.0, 2.0), u("se_dg", (B, P, C))
    w = (u("se_w1", (Cmid, C), -0.3, 0.3), u("se_b1", (Cmid,)), u("se_w2", (C, Cmid), -0.3, 0.3), u("se_b2", (C,)))
    return x, dg, w, both(ref64.se_gate_bwd, x, dg, *w)


# C = 32 (half of the 64-column pooling block), 64, 128 (two); P = 1 (three of the four pooling row groups idle), 7, 100
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("C,Cmid", [(32, 32), (64, 32), (128, 64)])
def test_se_gate_bwd(dev, C, Cmid, B):
    lib, check, dptr, st = abi()
    for P in (1, 7, 100):
        test = "se_gate_bwd[C%d Cmid%d B%d P%d]" % (C, Cmid, B, P)
        x, dg, w, (ref, ref32) = _se_case(C, Cmid, B, P)
        wd, xd, dgd = [t.to(dev) for t in w], x.to(dev), dg.to(dev)
        dx = Buf(dev, (B, P, C))
        g = [Buf(dev, t.shape, pre("se_g%d" % i, t.shape)) for i, t in enumerate(w)]
        ws = Buf(dev, (B * (5 * C + 2 * Cmid) + 2 * C * Cmid,))      # "ws: B*(5C+2Cmid) + 2*C*Cmid floats", NaN-filled: never read before written
        check(lib.dpmn_se_gate_bwd_f32(dptr(xd), dptr(dgd), dptr(wd[0]), dptr(wd[1]), dptr(wd[2]), dptr(wd[3]), dptr(dx.t),
                                       dptr(g[0].t), dptr(g[1].t), dptr(g[2].t), dptr(g[3].t), dptr(ws.t), B, P, C, Cmid, st))
        assert bool((ws.flat[ws.n:] == SENT).all()), "%s: wrote past the workspace" % test
        dx.check(test, "dx", ref[0], ref32[0])
        for i, what in enumerate(("dfc1_w", "dfc1_b", "dfc2_w", "dfc2_b")):
            g[i].check(test, what, ref[i + 1], ref32[i + 1])


# ------------------------------------------------------------------------------------------------------------------ L1 loss
# 256 elements per partial: n = 1, 255, 257 (2 partials), 70001 (274 partials: more than four rounds of the 64-thread final sum)
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_l1_loss(dev, n, with_extra):
    lib, check, dptr, st = abi()
    test = "l1_loss[n%d%s]" % (n, " extra_a" if with_extra else "")
    a, b = u("l1_a", (n,)), u("l1_b", (n,))
    b[::3] = a[::3]                           # exact ties: |a - b| = 0 and sign 0
    extra, gs, inv = (u("l1_extra", (n,)) if with_extra else None), 0.7, 1.0 / n
    ad, bd, gsd, exd = a.to(dev), b.to(dev), torch.full((1,), gs, device=dev), (extra.to(dev) if with_extra else None)
    loss, part = Buf(dev, (1,)), Buf(dev, ((n + 255) // 256,))
    check(lib.dpmn_l1_loss_fwd_f32(dptr(ad), dptr(bd), inv, dptr(loss.t), dptr(part.t), n, st))
    part.check(test, "block partial sums", torch.stack([(a[i:i + 256].double() - b[i:i + 256].double()).abs().sum() for i in range(0, n, 256)]),
               torch.stack([(a[i:i + 256] - b[i:i + 256]).abs().sum() for i in range(0, n, 256)]))
    loss.check(test, "loss", *both(ref64.l1_loss, a, b, inv))
    (da, db), (da32, db32) = both(ref64.l1_loss_bwd, a, b, gs, inv, extra)
    bda, bdb = Buf(dev, (n,)), Buf(dev, (n,))
    check(lib.dpmn_l1_loss_bwd_f32(dptr(ad), dptr(bd), dptr(gsd), inv, dptr(exd, True),
                                   dptr(bda.t), dptr(bdb.t), n, st))
    got_a = bda.check(test, "da", da, da32)
    got_b = bdb.check(test, "db", db, db32)
    ties = torch.arange(0, n, 3)
    assert torch.equal(got_a.cpu()[ties], extra[ties] if with_extra else torch.zeros(len(ties))) and bool((got_b.cpu()[ties] == 0).all()), "%s: a tie a == b must give sign 0" % test
    record(test, "ties checked", len(ties))
