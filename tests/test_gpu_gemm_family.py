"""GPU parity of the GEMM family -- k_gemm_wstat (256- and 512-thread forms, FULL and straight-line epilogues), k_gemm_rowreg, k_gemm_kloop,
k_gemm_kloop128, k_gemm_pw (csrc/gemm.hip), their bf16x3 twins (gemm_x3.hip, gemm_rowreg_x3.hip, gemm_tn_x3.hip) and the Linear weight
gradient (k_gemm_tn / k_gemm_tn_reg, backward.hip) -- each entry point called alone through _abi.lib on caller-owned buffers against its
float64 reference (tests/ref64.py, pinned by tests/test_ref64.py) at the smallest shapes that cross the predicates of launch_wholeK,
try_rowreg and launch_rowreg: M >= 1024, M % 16, M % 32, M >= 4096, M % 64, N % 96, K in {32, 64, 96, 128, 192}, the residuals present,
the activation; more tiles than blocks (the register prefetch of tile + stride / tile + 3 stride, clamped and not); tile counts that the
waves do not divide; k-splits without chunks.

Buffers (Buf of test_gpu_small_backward.py).  An output the kernel overwrites starts NaN-filled and must come back NaN-free; dw / db,
which it accumulates into, start from a prefill; every output carries a sentinel row past its end; every workspace starts NaN-filled.

Inputs.  (a) EXACT: operands on a 2^-5 grid in [-1, 1], biases / residuals / prefills on a 2^-10 grid.  Every product is a multiple of
2^-10 and a sum of up to 2^13 of them needs at most 13 + 10 bits: every order of addition is exact in fp32, the three-term bf16 split
is exact (at most 7 significant bits per operand), the fp32 CPU evaluation has error 0 -- so check_derived asks for equality with the
float64 reference up to its bare 1e-6 floor, and the recorded error is 0.  Used wherever there is no activation and no LayerNorm:
forward K <= 384, weight gradients over at most 8192 terms.  (b) CONTINUOUS: synth.uniform inputs, weights scaled so that
|pre-activation| <= 6 (asserted on the reference); the bound is check_derived, 8 x the fp32 CPU evaluation's own error against
float64, floor 1e-6.  No constant of this file's own.  GELU runs through erf_as in the kernels (|error in erf| <= 1.5e-7): GELU(x) is
off by at most E |x| with E = 0.5 * 1.5e-7, below the floor for |x| <= 6; the column sums of sk_proj add 32 of them, so their floor is
E * max over the partial rows of sum |feats| -- from the reference, never from the kernel's output."""
import functools
import itertools

import numpy as np
import pytest
import torch

import ref64
from dpmn_amd.utils import synth
from helpers import record
from oracle.pgrm import drop_mask
from test_gpu_small_backward import Buf, SENT, E_ERF, abi, both, grid, same_bits
from test_gpu_small_kernels import check_derived

pytestmark = pytest.mark.gpu
ACT = ref64.ACT_CODES
SLOPE = 0.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=100):
    return synth.uniform(name, shape, lo, hi, seed)


def op(name, shape):
    """an operand of the exact kind: multiples of 2^-5 in [-1, 1]"""
    return grid(u(name, shape), 5)


def fine(name, shape):
    """a bias / residual / prefill of the exact kind: multiples of 2^-10 in [-1, 1]"""
    return grid(u(name, shape), 10)


def untouched(test, what, buf):
    assert bool(torch.isnan(buf.t).all()) and bool((buf.flat[buf.n:] == SENT).all()), "%s %s: a rejected call wrote its output" % (test, what)


def exact(test, what, got, ref):
    """the exact kind's claim, on top of check_derived's floor: not one bit of difference"""
    bad = int((got.detach().cpu().double() != ref.reshape(got.shape)).sum())
    assert bad == 0, "%s %s: %d of %d outputs differ from the exactly representable result" % (test, what, bad, got.numel())


# ------------------------------------------------------------------------------------------------------------------ Linear forward
# name -> (bias, res1, res2, activation); without activation: the exact kind, with: the continuous kind
EPIS = {"none": (0, 0, 0, "none"), "bias": (1, 0, 0, "none"), "bias_gelu": (1, 0, 0, "gelu"), "bias_res1": (1, 1, 0, "none"),
        "bias_res1_res2": (1, 1, 1, "none"), "res1": (0, 1, 0, "none"), "bias_gelu_res1": (1, 1, 0, "gelu"), "bias_prelu": (1, 0, 0, "prelu")}


@functools.lru_cache(maxsize=6)
def _lin_inputs(M, N, K, cont):
    if cont:        # |x w^T| <= 2, |bias| <= 4
        return u("x", (M, K)), u("w", (N, K), -2.0 / K, 2.0 / K), u("bias", (N,), -4.0, 4.0), u("res1", (M, N)), u("res2", (M, N))
    return op("x", (M, K)), op("w", (N, K)), fine("bias", (N,)), fine("res1", (M, N)), fine("res2", (M, N))


@functools.lru_cache(maxsize=6)
def _lin_dev(M, N, K, cont):
    return tuple(t.cuda() for t in _lin_inputs(M, N, K, cont))


def _lin_ref_raw(M, N, K, epi):
    hb, h1, h2, act = EPIS[epi]
    x, w, b, r1, r2 = _lin_inputs(M, N, K, act != "none")
    return both(ref64.linear, x, w, b if hb else None, r1 if h1 else None, r2 if h2 else None, ACT[act], SLOPE)


_lin_ref_small = functools.lru_cache(maxsize=None)(_lin_ref_raw)


def _lin_ref(M, N, K, epi):
    """references of the small shapes are kept for the second arithmetic pass; the large ones are computed again"""
    return (_lin_ref_small if M * N <= 1 << 18 else _lin_ref_raw)(M, N, K, epi)


def _linear_shape(dev, M, N, K, epis=tuple(EPIS)):
    lib, check, dptr, st = abi()
    for epi in epis:
        hb, h1, h2, act = EPIS[epi]
        cont = act != "none"
        test = "linear[M%d N%d K%d %s]" % (M, N, K, epi)
        x, w, b, r1, r2 = _lin_dev(M, N, K, cont)
        ref, ref32 = _lin_ref(M, N, K, epi)
        y = Buf(dev, (M, N))
        check(lib.dpmn_linear_f32(dptr(x), dptr(w), dptr(b if hb else None, True), dptr(r1 if h1 else None, True), dptr(r2 if h2 else None, True),
                                  dptr(y.t), M, N, K, ACT[act], SLOPE, st))
        got = y.check(test, "y", ref, ref32)
        if not cont:
            exact(test, "y", got, ref)


# rowreg: M % 16 == 0, N % 96 == 0, M >= 1024, K = 96 / 192 and one of the epilogues none / bias, GELU, res1, res1 + res2 -- M = 1008 (below
# the gate) and 1032 (M % 16) fall to the 256-thread wstat, as do GELU + res1 and PReLU at every M; 1040 / 1136: 65 / 71 tiles of 16 rows,
# which the 4 gx waves do not divide
@pytest.mark.parametrize("K", [96, 192])
@pytest.mark.parametrize("N", [96, 192, 384])
def test_linear_rowreg(dev, N, K):
    for M in (1008, 1024, 1040, 1032, 1136):
        _linear_shape(dev, M, N, K)


# 256-thread wstat: tiles of 32 rows x 96 columns; M = 1 .. 95 (a partial tile, one, one + 1 row, three less one row), N = 4 (one float4 of
# one column tile), 100 (a second column tile of one float4), 96 / 192 whole
@pytest.mark.parametrize("K", [32, 64, 96, 128, 192])
def test_linear_wstat256(dev, K):
    for M, N in itertools.product((1, 31, 32, 33, 95), (4, 96, 100, 192)):
        _linear_shape(dev, M, N, K)


# ny = 8 column tiles -> gx = 768 / 8 = 96 blocks per column tile; 2 * 96 + 1 = 193 tiles of 32 rows: block 0 walks three tiles, the others
# two (both register sets and the refill tile + 3 * stride past the end); + 5 rows: a ragged last tile.  (At M = 6176 rowreg takes the
# epilogues it has -- 386 tiles of 16 rows over 4 gx waves -- and GELU + res1 / PReLU walk the wstat tiles; at 6181 every epilogue does)
# 4 * 96 + 1 tiles: block 0 walks five -- only from 3 * gx + 1 tiles on does the refill tile + 3 * stride load a tile of its own
@pytest.mark.parametrize("M", [32 * (2 * 96 + 1), 32 * (2 * 96 + 1) + 5, 32 * (4 * 96 + 1) + 5])
def test_linear_wstat256_multi_tile(dev, M):
    _linear_shape(dev, M, 768, 192)


# 512-thread wstat (M >= 4096, K <= 128): ny = 4 -> gx = 128 blocks; FULL (M % 64 == 0, N % 96 == 0) with its straight-line epilogues 1 (none /
# bias), 2 (GELU), 3 (two residuals), 5 (one) and the generic one (GELU + res1, PReLU), else the predicated form.  64 * (2 * 128 + 1) rows:
# 257 tiles, block 0 takes three (the clamped prefetch min(tile + 3 * stride, tiles - 1)), the others two
@pytest.mark.parametrize("K", [32, 64, 128])
@pytest.mark.parametrize("M", [4096, 4097, 4128, 64 * (2 * 128 + 1), 64 * (2 * 128 + 1) + 37])
def test_linear_wstat512(dev, M, K):
    _linear_shape(dev, M, 384, K)


# ny = 8 -> gx = 64: the same 257 tiles are five for block 0, FULL (unpredicated refills at tile + 3 * stride = 192, 256) and predicated
@pytest.mark.parametrize("M", [64 * (4 * 64 + 1), 64 * (4 * 64 + 1) + 37])
def test_linear_wstat512_five_tiles(dev, M):
    _linear_shape(dev, M, 768, 32, ("bias", "bias_gelu", "bias_res1_res2", "bias_gelu_res1"))


@pytest.mark.parametrize("K", [32, 64, 128])
def test_linear_wstat512_n_edge(dev, K):
    _linear_shape(dev, 4096, 100, K)


# K = 96 above M = 4096: rowreg takes the whole-tile calls it has an epilogue for; GELU + res1 and PReLU reach the generic FULL 512-thread
# form, and with M % 16 != 0 every epilogue the predicated one
def test_linear_wstat512_k96(dev):
    _linear_shape(dev, 4096, 384, 96, ("bias_gelu_res1", "bias_prelu"))
    _linear_shape(dev, 4097, 384, 96)


# k-loop (K > 192): 64 x 96 tiles, 32-deep steps in two register sets -- K = 224: 7 steps (the odd-count break), 256: 8, 384: 12; M = 1, 64, 65,
# 130 and N = 96, 100, 192: bias + res1 takes the fast epilogue on interior tiles and the generic one on the ragged ones
@pytest.mark.parametrize("K", [224, 256, 384])
def test_linear_kloop(dev, K):
    for M, N in itertools.product((1, 64, 65, 130), (96, 100, 192)):
        _linear_shape(dev, M, N, K, ("bias_res1", "none", "bias_gelu"))


# ------------------------------------------------------------------------------------------------------------------ prologues
PRO_M = (33, 4096, 4160 + 3)      # the 256-thread form; FULL 512-thread; the predicated 512-thread form with a ragged 66th tile
PRO_N = 192


@functools.lru_cache(maxsize=None)
def _add_case(M, K, act):
    N = PRO_N
    if act == "none":
        x, addv, w, b = op("ax", (M, K)), op("addv", (M, K)), op("aw", (N, K)), fine("ab", (N,))
    else:           # |x + addv| <= 2
        x, addv, w, b = u("ax", (M, K)), u("addv", (M, K)), u("aw", (N, K), -1.0 / K, 1.0 / K), u("ab", (N,), -4.0, 4.0)
    return x, addv, w, b, both(ref64.linear, x, w, b, None, None, ACT[act], 0.0, ("add", addv))


# FULL straight-line epilogues 1 (none) and 2 (GELU), the generic FULL epilogue (LeakyReLU 0.2; the entry point takes no slope); at K = 192
# every M runs the 256-thread form
@pytest.mark.parametrize("K", [32, 64, 96, 128, 192])
def test_add_linear(dev, K):
    lib, check, dptr, st = abi()
    for M, act in itertools.product(PRO_M, ("none", "gelu", "leaky02")):
        test = "add_linear[M%d K%d %s]" % (M, K, act)
        x, addv, w, b, (ref, ref32) = _add_case(M, K, act)
        xd, ad, wd, bd, y = x.to(dev), addv.to(dev), w.to(dev), b.to(dev), Buf(dev, (M, PRO_N))
        check(lib.dpmn_add_linear_f32(dptr(xd), dptr(ad), dptr(wd), dptr(bd), dptr(y.t), M, PRO_N, K, ACT[act], st))
        got = y.check(test, "y", ref, ref32)
        if act == "none":
            exact(test, "y", got, ref)


@functools.lru_cache(maxsize=None)
def _cat2_case(M, k1, k2, act):
    N, K = PRO_N, k1 + k2
    if act == "none":
        x1, x2, w, b = op("c1", (M, k1)), op("c2", (M, k2)), op("cw", (N, K)), fine("cb", (N,))
    else:
        x1, x2, w, b = u("c1", (M, k1)), u("c2", (M, k2)), u("cw", (N, K), -2.0 / K, 2.0 / K), u("cb", (N,), -4.0, 4.0)
    return x1, x2, w, b, both(ref64.linear, x1, w, b, None, None, ACT[act], SLOPE, ("cat2", x2))


# a staging thread owns K / 8 consecutive columns and an MFMA chunk is 16 deep: k1 = 4 (K = 32), 36 (K = 96), 100 (K = 192) put the seam
# inside a thread's share and inside a chunk; 64 + 64 is aligned
@pytest.mark.parametrize("k1,k2", [(4, 28), (36, 60), (64, 64), (100, 92)])
def test_cat2_linear(dev, k1, k2):
    lib, check, dptr, st = abi()
    for M, act in itertools.product(PRO_M, ("none", "gelu")):
        test = "cat2_linear[M%d k1 %d k2 %d %s]" % (M, k1, k2, act)
        x1, x2, w, b, (ref, ref32) = _cat2_case(M, k1, k2, act)
        x1d, x2d, wd, bd, y = x1.to(dev), x2.to(dev), w.to(dev), b.to(dev), Buf(dev, (M, PRO_N))
        check(lib.dpmn_cat2_linear_f32(dptr(x1d), k1, dptr(x2d), k2, dptr(wd), dptr(bd), dptr(y.t), M, PRO_N, ACT[act], st))
        got = y.check(test, "y", ref, ref32)
        if act == "none":
            exact(test, "y", got, ref)


@functools.lru_cache(maxsize=None)
def _ln_case(M, K, act):
    """rows with a large common offset: x = u(-1, 1) + 3 u_row -- the two-pass statistics must not lose the deviations in it"""
    N = PRO_N
    x = u("lx", (M, K)) + 3.0 * u("lrow", (M, 1))
    gm, bt, w, b = u("lg", (K,), 0.5, 1.5), u("lbeta", (K,), -0.5, 0.5), u("lw", (N, K), -0.5 / K, 0.5 / K), u("lb", (N,), -4.0, 4.0)
    assert float(ref64.linear(x, w, b, pro=("ln", gm, bt, 1e-5)).abs().max()) <= 6.0
    return x, gm, bt, w, b, both(ref64.linear, x, w, b, None, None, ACT[act], SLOPE, ("ln", gm, bt, 1e-5))


# M = 1, 33: 256-thread wstat; 1024 / 1040: rowreg at K = 96 / 192 (64 / 65 tiles), wstat otherwise; 4096 / 4099: the 512-thread form FULL / not
# for K <= 128 (rowreg again at K = 96, 4096), the 256-thread form at K = 192
@pytest.mark.parametrize("K", [32, 64, 96, 128, 192])
def test_ln_linear(dev, K):
    lib, check, dptr, st = abi()
    for M, act in itertools.product((1, 33, 1024, 1040, 4096, 4099), ("none", "gelu")):
        test = "ln_linear[M%d K%d %s]" % (M, K, act)
        x, gm, bt, w, b, (ref, ref32) = _ln_case(M, K, act)
        xd, gd, btd, wd, bd, y = x.to(dev), gm.to(dev), bt.to(dev), w.to(dev), b.to(dev), Buf(dev, (M, PRO_N))
        check(lib.dpmn_ln_linear_f32(dptr(xd), dptr(gd), dptr(btd), 1e-5, dptr(wd), dptr(bd), dptr(y.t), M, PRO_N, K, ACT[act], st))
        y.check(test, "y", ref, ref32)


# ------------------------------------------------------------------------------------------------------------------ Linear + Dropout + DropPath
SEED_E = 0x5DEECE66D


@functools.lru_cache(maxsize=None)
def _seed_row(p):
    """the first seed under which DropPath keeps one of the samples 0, 1 and drops the other: both fates inside the first 64-row tile"""
    return next(s for s in range(1, 4096) if int((drop_mask(s, np.arange(2), p) == 0).sum()) == 1)


@functools.lru_cache(maxsize=None)
def _drop_case(M, N, K, pe, pr):
    row_len = 48 * N          # a sample boundary inside every 64-row tile
    x, w, b, res = u("dx", (M, K)), u("dw", (N, K), -2.0 / K, 2.0 / K), u("db", (N,), -4.0, 4.0), u("dres", (M, N))
    idx = np.arange(M * N)
    me = drop_mask(SEED_E, idx, pe).reshape(M, N) if pe > 0 else None
    seed_r = _seed_row(pr) if pr > 0 else 0
    mr = drop_mask(seed_r, idx // row_len, pr).reshape(M, N) if pr > 0 else None
    dead = torch.zeros(M, N, dtype=torch.bool)
    for m in (me, mr):
        if m is not None:
            dead |= m == 0
    assert bool(dead.any()) and not bool(dead.all())
    return row_len, seed_r, x, w, b, res, dead, both(ref64.linear_drop, x, w, b, res, me, mr)


@pytest.mark.parametrize("pe,pr", [(0.3, 0.0), (0.0, 0.25), (0.3, 0.25)])
@pytest.mark.parametrize("M,N,K", [(64, 96, 224), (192, 192, 256)])
def test_linear_drop(dev, M, N, K, pe, pr):
    lib, check, dptr, st = abi()
    test = "linear_drop[M%d N%d K%d p_elem %.2f p_row %.2f]" % (M, N, K, pe, pr)
    row_len, seed_r, x, w, b, res, dead, (ref, ref32) = _drop_case(M, N, K, pe, pr)
    xd, wd, bd, rd, y = x.to(dev), w.to(dev), b.to(dev), res.to(dev), Buf(dev, (M, N))
    check(lib.dpmn_linear_drop_f32(dptr(xd), dptr(wd), dptr(bd), dptr(rd), dptr(y.t), M, N, K, pe, SEED_E, pr, seed_r, row_len, st))
    got = y.check(test, "y", ref, ref32)
    # a zeroed output is the residual itself, bit for bit; a kept one differs from it (x w^T + b is not 0)
    assert torch.equal(got.cpu() == res, dead), "%s: the zeroed outputs are not the oracle mask's (%d vs %d)" % (test, int((got.cpu() == res).sum()), int(dead.sum()))
    record(test, "zeroed outputs", int(dead.sum()))


@pytest.mark.parametrize("M,N,K", [(65, 96, 224), (64, 100, 224), (64, 96, 192), (64, 96, 128)])
def test_linear_drop_rejects(dev, M, N, K):
    lib, check, dptr, st = abi()
    x, w, b, res = (torch.zeros(s, device=dev) for s in ((M, K), (N, K), (N,), (M, N)))
    y = Buf(dev, (M, N))
    assert lib.dpmn_linear_drop_f32(dptr(x), dptr(w), dptr(b), dptr(res), dptr(y.t), M, N, K, 0.3, SEED_E, 0.25, 7, 48 * N, st) != 0
    torch.cuda.synchronize()
    untouched("linear_drop[M%d N%d K%d]" % (M, N, K), "y", y)


# ------------------------------------------------------------------------------------------------------------------ SKConv projection
@functools.lru_cache(maxsize=None)
def _skp_case(M, C, cont):
    if cont:
        cat, w, b = u("scat", (M, C)), u("sw", (C, C), -2.0 / C, 2.0 / C), u("sb", (C,), -4.0, 4.0)
    else:
        cat, w, b = op("scat", (M, C)), op("sw", (C, C)), fine("sb", (C,))
    (feats, part), r32 = both(ref64.sk_proj, cat, w, b)
    assert not cont or float(feats.abs().max()) <= 6.0
    floor = max(1e-6, E_ERF * float(torch.stack([feats[r0:r0 + 32].abs().sum(0) for r0 in range(0, M, 32)]).max()))
    return cat, w, b, (feats, part), r32, floor


# C = 96: M = 32, 992 the straight-line 256-thread epilogue 4; 1024, 1056 rowreg epilogue 4 (33 pairs of 16-row tiles: waves with unequal
# counts); 1000: generic, the last partial over 8 rows; 1040: M % 32 != 0 above the rowreg gate.  C = 64 (N % 96 != 0: generic), 192 (rowreg
# at 1024): M = 33 (a last partial of one row), 1024
@pytest.mark.parametrize("C,M", [(96, m) for m in (32, 992, 1024, 1056, 1000, 1040)] + [(c, m) for c in (64, 192) for m in (33, 1024)])
def test_sk_proj(dev, C, M):
    lib, check, dptr, st = abi()
    nparts = (M + 31) // 32
    for cont in (False, True):
        test = "sk_proj[M%d C%d %s]" % (M, C, "continuous" if cont else "exact")
        cat, w, b, (feats, part), (feats32, part32), floor = _skp_case(M, C, cont)
        cd, wd, bd, bf, bp = cat.to(dev), w.to(dev), b.to(dev), Buf(dev, (M, C)), Buf(dev, (nparts, C))
        check(lib.dpmn_sk_proj_f32(dptr(cd), dptr(wd), dptr(bd), dptr(bf.t), dptr(bp.t), M, C, st))
        got = bf.check(test, "feats", feats, feats32)
        if cont:
            bp.check(test, "GELU column sums per 32 rows", part, part32, floor)
        else:       # (GELU of the grid values is not exact: the sums are judged on the continuous inputs)
            exact(test, "feats", got, feats)
            assert bool((bp.flat[bp.n:] == SENT).all()) and not bool(torch.isnan(bp.t).any()), "%s: partial rows overrun or not all written" % test


# ------------------------------------------------------------------------------------------------------------------ pointwise conv
@functools.lru_cache(maxsize=None)
def _pw_case(B, Ch, L, cont):
    if cont:
        g, w, b = u("pg", (B, Ch, L)), u("pw", (Ch, Ch), -2.0 / Ch, 2.0 / Ch), u("pb", (Ch,), -4.0, 4.0)
    else:
        g, w, b = op("pg", (B, Ch, L)), op("pw", (Ch, Ch)), fine("pb", (Ch,))
    return g, w, b, both(ref64.pointwise, g, w, b)


# tiles of 128 positions x 128 (Ch = 128, 256) or 192 (Ch = 384) channels, 16-deep steps: L = 128 / 384 one / three position tiles
@pytest.mark.parametrize("Ch", [128, 256, 384])
def test_pointwise(dev, Ch):
    lib, check, dptr, st = abi()
    for B, L, cont in [(b, l, False) for b in (1, 3) for l in (128, 384)] + [(3, 384, True)]:
        test = "pointwise[B%d Ch%d L%d %s]" % (B, Ch, L, "continuous" if cont else "exact")
        g, w, b, (ref, ref32) = _pw_case(B, Ch, L, cont)
        gd, wd, bd, z = g.to(dev), w.to(dev), b.to(dev), Buf(dev, (B, Ch, L))
        check(lib.dpmn_pointwise_f32(dptr(gd), dptr(wd), dptr(bd), dptr(z.t), B, Ch, L, st))
        got = z.check(test, "z", ref, ref32)
        if not cont:
            exact(test, "z", got, ref)


@functools.lru_cache(maxsize=None)
def _pwg_case(B, Ch, L):
    assert B * L <= 8192
    dz, g, fill = op("wdz", (B, Ch, L)), op("wg", (B, Ch, L)), fine("wdw", (Ch, Ch))
    return dz, g, fill, both(ref64.pointwise_wgrad, dz, g)


# 32 k-splits over nk_all = B L / 32 chunks, cps = ceil(nk_all / 32) each: (1, 32) one chunk, 31 splits without; (7, 160) 35 chunks, cps = 2,
# 18 splits at work, their ranges crossing image boundaries (5 chunks per image); (3, 1024) 96 chunks, cps = 3.  Ch = 100: ragged in both tile
# dimensions (64 rows, 96 columns).  The sums are exact, so the atomic result does not depend on the arrival order: two runs, the same bits
@pytest.mark.parametrize("B,L", [(1, 32), (7, 160), (3, 1024)])
@pytest.mark.parametrize("Ch", [96, 100, 192])
def test_pointwise_wgrad_atomic(dev, Ch, B, L):
    lib, check, dptr, st = abi()
    test = "pointwise_wgrad[Ch%d B%d L%d]" % (Ch, B, L)
    dz, g, fill, (ref, ref32) = _pwg_case(B, Ch, L)
    dzd, gd, runs = dz.to(dev), g.to(dev), []
    for _ in range(2):
        dw = Buf(dev, (Ch, Ch), fill)
        check(lib.dpmn_pointwise_wgrad_f32(dptr(dzd), dptr(gd), dptr(dw.t), B, Ch, L, st))
        runs.append(dw.t)
    same_bits(test, "dw", runs[0], runs[1])
    exact(test, "dw", dw.check(test, "dw", ref, ref32), fill.double() + ref)


def _pwg_det(dev, Ch, B, L, splits):
    lib, check, dptr, st = abi()
    test = "pointwise_wgrad_det[Ch%d B%d L%d]" % (Ch, B, L)
    dz, g, fill, (ref, ref32) = _pwg_case(B, Ch, L)
    nbytes = lib.dpmn_pointwise_wgrad_det_bytes(Ch, L)
    assert nbytes == splits * Ch * Ch * 4, "%s: %d bytes, not %d splits" % (test, nbytes, splits)
    dzd, gd, runs = dz.to(dev), g.to(dev), []
    dw, ws = Buf(dev, (Ch, Ch), fill), Buf(dev, (nbytes // 4,))
    assert lib.dpmn_pointwise_wgrad_det_f32(dptr(dzd), dptr(gd), dptr(dw.t), B, Ch, L, dptr(ws.t), nbytes - 1, st) != 0, "%s: a workspace one byte short was accepted" % test
    torch.cuda.synchronize()
    assert torch.equal(dw.t.cpu(), fill) and bool(torch.isnan(ws.t).all()), "%s: the rejected call wrote" % test
    for _ in range(2):
        dw, ws = Buf(dev, (Ch, Ch), fill), Buf(dev, (nbytes // 4,))
        check(lib.dpmn_pointwise_wgrad_det_f32(dptr(dzd), dptr(gd), dptr(dw.t), B, Ch, L, dptr(ws.t), nbytes, st))
        runs.append((dw.t, ws.t))
    assert bool((ws.flat[ws.n:] == SENT).all()), "%s: wrote past the workspace" % test
    holes = torch.isnan(ws.t.view(splits, Ch * Ch)).any(1).nonzero().flatten().tolist()
    assert not holes, "%s: the reduce adds %d slabs, the slabs of splits %s were never (fully) written" % (test, splits, holes)
    same_bits(test, "dw", runs[0][0], runs[1][0])
    same_bits(test, "split slabs", runs[0][1], runs[1][1])
    exact(test, "dw", dw.check(test, "dw", ref, ref32), fill.double() + ref)
    added = ws.t.view(splits, Ch, Ch).double().sum(0).float()
    check_derived(test, "split slabs added", added, ref, ref32)
    exact(test, "split slabs added", added, ref)


# fallback (Ch % 128 != 0): the 64 x 96 k-loop in store mode, 32 slabs added by dpmn_rows_reduce_f32.  (1, 32): one chunk, 31 splits without
# any; (5, 256): 40 chunks, cps = 2, splits 20 .. 31 without; (7, 160): 35 chunks, splits 18 .. 31 without; (2, 1024): 64 chunks, every
# split two.  A split without chunks still owns a slab the reduce reads: it has to store zeros
@pytest.mark.parametrize("B,L", [(1, 32), (5, 256), (7, 160), (2, 1024)])
@pytest.mark.parametrize("Ch", [96, 100, 192])
def test_pointwise_wgrad_det_fallback(dev, Ch, B, L):
    _pwg_det(dev, Ch, B, L, 32)


# 128 x 128 tiles: splits S = (504 / tiles) & ~7 -- split z takes the chunks [nchunks z / S, nchunks (z + 1) / S): (1, 32) one chunk, every
# split but the last without any; (3, 160) 15 chunks, 5 per image, each decoded to (image, offset) on its own; (5, 512) 80 chunks, 16 per
# image: at S = 56 ranges of one and two chunks, some across an image boundary
@pytest.mark.parametrize("B,L", [(1, 32), (3, 160), (5, 512)])
@pytest.mark.parametrize("Ch,S", [(128, 504), (256, 120), (384, 56)])
def test_pointwise_wgrad_det_128(dev, Ch, S, B, L):
    _pwg_det(dev, Ch, B, L, S)


# ------------------------------------------------------------------------------------------------------------------ Linear weight gradient
@functools.lru_cache(maxsize=None)
def _tn_case(M, N, K):
    dy, x = op("tdy", (M, N)), op("tx", (M, K))
    return dy, x, fine("tdw", (N, K)), fine("tdb", (N,)), both(ref64.gemm_tn, dy, x)


def _tn_plan(M, N, K):
    """the split plan of dpmn_gemm_tn_f32 (tn_plan, backward.hip): -> (splits, rows per split)"""
    cdiv = lambda a, b: (a + b - 1) // b
    s0 = cdiv(256, cdiv(N, 96) * cdiv(K, 96))
    rows = max(32, cdiv(cdiv(M, s0), 32) * 32)
    return cdiv(M, rows), rows


# 96 x 96 tiles, M split into ranges of a multiple of 32 rows: M = 1 .. 32 one split (atomics even with a workspace), 33 two (32 + 1), 100
# four (the last of 4 rows), 1001 32 (the last of 9).  (48, 48), (144, 48), (96, 96): N and K multiples of 48, the operands-in-registers
# kernel once there is a workspace and several splits; (96, 32), (16, 96): the LDS kernel with a ragged tile
@pytest.mark.parametrize("N,K", [(48, 48), (96, 32), (16, 96), (144, 48), (96, 96)])
@pytest.mark.parametrize("M", [1, 3, 31, 32, 33, 100, 1001])
def test_gemm_tn(dev, M, N, K):
    lib, check, dptr, st = abi()
    dy, x, fw, fb, ((dW, db), (dW32, db32)) = _tn_case(M, N, K)
    dyd, xd = dy.to(dev), x.to(dev)
    splits, rows = _tn_plan(M, N, K)
    nbytes = lib.dpmn_gemm_tn_partial_bytes(M, N, K)
    assert nbytes == (splits * (N * K + N) * 4 + 255) // 256 * 256
    for with_db, with_ws in itertools.product((True, False), (True, False)):
        test = "gemm_tn[M%d N%d K%d%s%s]" % (M, N, K, " db" if with_db else "", " ws" if with_ws else " atomics")
        runs = []
        for _ in range(2):
            bw, bb, ws = Buf(dev, (N, K), fw), Buf(dev, (N,), fb), Buf(dev, (nbytes // 4,))
            check(lib.dpmn_gemm_tn_f32(dptr(dyd), dptr(xd), dptr(bw.t), dptr(bb.t if with_db else None, True), M, N, K,
                                       dptr(ws.t if with_ws else None, True), nbytes if with_ws else 0, st))
            runs.append((bw.t, bb.t))
        same_bits(test, "dW", runs[0][0], runs[1][0])
        same_bits(test, "db", runs[0][1], runs[1][1])
        exact(test, "dW", bw.check(test, "dW", dW, dW32), fw.double() + dW)
        if with_db:
            exact(test, "db", bb.check(test, "db", db, db32), fb.double() + db)
        else:
            assert torch.equal(bb.flat.cpu(), torch.cat([fb, torch.full((1,), SENT)])), "%s: no db asked for, yet the buffer changed" % test
        assert bool((ws.flat[ws.n:] == SENT).all()), "%s: wrote past the workspace" % test
        if with_ws and splits > 1:      # the slabs the reduce reads: NK (+ N with db) floats per split
            slabs = ws.t[:splits * (N * K + N)].view(splits, N * K + N)[:, :N * K + (N if with_db else 0)]
            assert not bool(torch.isnan(slabs).any()), "%s: a split's partial slab was not fully written" % test
