"""GPU parity of the convolution family -- dpmn_conv2d_nhwc_f32 (csrc/conv.hip, conv_body.h: k_conv_direct, k_conv_halo_c4, k_conv_halo,
k_conv_igemm in its generic / UNI / SIMPLE / SIMPLE + AFF loaders, k_conv_igemm_sk, k_conv_splitk_reduce and the bf16x3 twins of conv_x3.hip),
the weight gradient (k_conv_wgrad of conv_bwd.hip in its P2 and generic forms, conv_wgrad_x3.hip, the pack / unpack kernels) and the
data-gradient constructions of train/cmm_train.py -- each entry point called alone on caller-owned buffers against its float64
reference (tests/ref64.py, pinned by tests/test_ref64.py) at the smallest shapes on either side of every predicate of the dispatch code.
Every case carries a comment naming the predicate and the arm it takes; where the profile tags tell the arms apart the kernel family
that ran is asserted (run(): the set of conv tags of the launch), elsewhere the comment carries the derivation.

Buffers (Buf of test_gpu_small_backward.py).  An overwritten output starts NaN-filled and must come back NaN-free; every output carries
a sentinel row; dW accumulators start from a 2^-10-grid prefill; the split-K workspace and the exclusive wgrad slots start NaN-filled;
with out_coff / out_ld the other channels of the wide buffer, with the odd-pixel scatter / a single transposed phase the other pixels of
the prefilled output must be bitwise unchanged.

Inputs.  No constant of this file's own.
(a) EXACT, wherever there is no transcendental: operands on the 2^-5 grid in [-1, 1], bias / residual / prefill on the 2^-10 grid, affine
scale in {0.5, 1, 2} with the shift on the 2^-5 grid, input activation none or ReLU.  A transformed input is then a multiple of 2^-6 below
3 in magnitude (8 significant bits), a product a multiple of 2^-11, and in_range() asserts from the INPUTS -- the reference evaluated on
|x| and |w| in float64 -- that 2^11 max sum |x| |w| < 2^24: every partial sum in every order is exact in fp32, the three-term bf16 split
is exact, and the claim is exact(): not one differing element, a recorded error of 0.  Split-K, stream-K, the in-L2 reduction on and off,
the atomic weight gradient and repeated runs therefore agree bit for bit with each other and with float64.
(b) CONTINUOUS (leaky slopes, mish / tanh / sigmoid / GELU, sums of squares): synth.uniform inputs, weights scaled by 1 / sqrt(K); the bound is
check_derived, 8 x the fp32 CPU evaluation's own error against float64, floor 1e-6 -- raised only for the GELU epilogue by the erf_as
rule of test_gpu_small_backward.py (E_ERF |pre-activation|, from the reference)."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import ref64
from dpmn_amd.utils import synth
from helpers import record
from test_gpu_small_backward import Buf, SENT, E_ERF, abi, both, grid, same_bits
from test_gpu_small_kernels import check_derived

pytestmark = pytest.mark.gpu
ACT = ref64.ACT_CODES
F32 = torch.float32
T128, T64, TN, RED, HALO, C4, SK, WG = ("k_conv_igemm<128,128>", "k_conv_igemm<64,64>", "k_conv_igemm<128,16|32>", "k_conv_splitk_reduce",
                                        "k_conv_halo", "k_conv_halo_c4", "k_conv_igemm_sk", "k_conv_wgrad")
CONV_TAGS = (T128, T64, TN, RED, HALO, C4, SK, WG)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=110):
    return synth.uniform(name, shape, lo, hi, seed)


def op(name, shape):
    """an operand of the exact kind: multiples of 2^-5 in [-1, 1]"""
    return grid(u(name, shape), 5)


def fine(name, shape):
    """a bias / residual / prefill of the exact kind: multiples of 2^-10 in [-1, 1]"""
    return grid(u(name, shape), 10)


def scale3(name, c):
    """an affine scale of the exact kind: 0.5, 1 or 2 per channel"""
    return 2.0 ** torch.round(u(name, (c,), -1.49, 1.49))


def in_range(test, absref):
    """the exact kind's premise, from the inputs: 2^11 max sum |x| |w| < 2^24"""
    assert 2.0 ** 11 * float(absref.max()) < 2.0 ** 24, "%s: the inputs do not keep every partial sum exact in fp32 (max sum |x||w| = %g)" % (test, float(absref.max()))


def exact(test, what, got, ref):
    """the exact kind's claim: NaN-free and not one bit of difference from the exactly representable float64 result"""
    got = got.detach().cpu().double()
    assert not bool(torch.isnan(got).any()), "%s %s: %d outputs never written" % (test, what, int(torch.isnan(got).sum()))
    ref = ref.reshape(got.shape)
    bad = int((got != ref).sum())
    record(test, what + ": GPU max abs err vs float64 (exact kind)", float((got - ref).abs().max()), 0.0)
    assert bad == 0, "%s %s: %d of %d outputs differ from the exactly representable result (max %g)" % (test, what, bad, got.numel(), float((got - ref).abs().max()))


def judge(test, what, got, ref, ref32=None, floor=1e-6):
    if ref32 is None:
        exact(test, what, got, ref)
    else:
        assert not bool(torch.isnan(got).any()), "%s %s: outputs never written" % (test, what)
        check_derived(test, what, got.contiguous(), ref.reshape(got.shape), ref32.reshape(got.shape), floor)


def sentinel(test, what, buf):
    assert bool((buf.flat[buf.n:] == SENT).all()), "%s %s: wrote past the end of the output" % (test, what)


def run(fn):
    """fn() under the launch profiler -> (result, the set of conv kernel families that ran)"""
    from dpmn_amd import _abi
    _abi.profile_begin(None)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        rows = _abi.profile_end()
    return out, {r["kernel"] for r in rows if r["kernel"] in CONV_TAGS}


@contextlib.contextmanager
def stream_k(on):
    """ops.STREAM_K (arrival counters attached: stream-K / in-L2 reduction possible) for one block, the old value put back afterwards"""
    from dpmn_amd import ops
    old = ops.STREAM_K
    ops.STREAM_K = on
    try:
        yield
    finally:
        ops.STREAM_K = old


@contextlib.contextmanager
def xred(on):
    """dpmn_xred_enable(on) for one block; -1 afterwards: the library's own default (the switch has no getter)"""
    lib, check, _, _ = abi()
    check(lib.dpmn_xred_enable(on))
    try:
        yield
    finally:
        check(lib.dpmn_xred_enable(-1))


def conv_out(n, k, stride, pad, dil):
    return ref64.conv_out_size(n, k, stride, pad, dil)


# ------------------------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=None)
def _fwd_case(segs, cout, k, B, H, W, stride, pad, dil, pro, epi, aff, res, bias, form, cont, stats):
    """inputs and references of one forward case, computed once and shared by both arithmetic passes.  aff: per segment 0 / 1"""
    cin, K = sum(segs), k * k * sum(segs)
    mk, mkf = (u, u) if cont else (op, fine)
    xs = [mk("x%d" % i, (B, H, W, c)) for i, c in enumerate(segs)]
    w = u("w", (cout, cin, k, k)) / K ** 0.5 if cont else op("w", (cout, cin, k, k))
    af = None
    if any(aff):
        af = [((u("sc%d" % i, (c,), 0.5, 1.5) if cont else scale3("sc%d" % i, c)), mk("sh%d" % i, (c,)) * (0.5 if cont else 1.0)) if a else None
              for i, (c, a) in enumerate(zip(segs, aff))]
    Ho, Wo = conv_out(H, k, stride, pad, dil), conv_out(W, k, stride, pad, dil)
    b = mkf("b", (cout,)) if bias else None
    r = mkf("res", (B, Ho, Wo, cout)) if res else None
    kw = dict(stride=stride, pad=pad, dil=dil, pro=ACT[pro], epi=ACT[epi], slope=0.25, affine=af, res=r, pixel_shuffle=form == "ps", out_nchw=form == "nchw")
    rawkw = dict(stride=stride, pad=pad, dil=dil, pro=ACT[pro], affine=af)
    ref32 = raw = raw32 = None
    floor = 1e-6
    if cont:      # the reference in float64 and the same formula in fp32: the yardstick of check_derived
        ref, ref32 = both(ref64.conv2d, xs, w, b, **kw)
        if stats:
            raw, raw32 = both(ref64.conv2d, xs, w, b, **rawkw)
        elif epi == "gelu":
            raw = ref64.conv2d(xs, w, b, **rawkw)
        if epi == "gelu":
            floor = max(floor, E_ERF * float(raw.abs().max()))
    else:
        ref = ref64.conv2d(xs, w, b, **kw)
        raw = ref64.conv2d(xs, w, b, **rawkw) if stats else None
        name = "conv[%s]" % (segs,)
        in_range(name, ref64.conv2d([ref64.conv_input(xs, af, ACT[pro]).abs()], w.abs(), stride=stride, pad=pad, dil=dil) + 2.0)
    return xs, w, b, af, r, ref, ref32, raw, raw32, floor


def fwd(dev, test, segs, cout, k, B, H, W, stride=1, pad=None, dil=1, pro="none", epi="none", aff=(0, 0, 0), res=False, bias=True, form="nhwc",
        cont=False, stats=False, wide=False, expect=None, mutate=None):
    """one dpmn_conv2d_nhwc_f32 launch through ops.conv2d into a caller-owned buffer, judged against float64.  wide: the output goes to
    channels [4, 4 + cout) of a prefilled buffer with 8 channels more.  Returns (output, kernel tags)."""
    from dpmn_amd import ops
    from dpmn_amd.model import packing
    segs = tuple(segs)
    pad = (k - 1) // 2 if pad is None else pad
    aff = tuple(aff[:len(segs)])
    cont = cont or pro not in ("none", "relu") or epi not in ("none", "relu")
    xs, w, b, af, r, ref, ref32, raw, raw32, floor = _fwd_case(segs, cout, k, B, H, W, stride, pad, dil, pro, epi, aff, res, bias, form, cont, stats)
    wp = packing.pack_conv(w.to(dev))[0]
    if mutate is not None:
        wp = mutate(wp)
    xd = [x.to(dev) for x in xs]
    afd = None if af is None else [None if a is None else (a[0].to(dev), a[1].to(dev)) for a in af]
    Ho, Wo = conv_out(H, k, stride, pad, dil), conv_out(W, k, stride, pad, dil)
    ld = (cout + 3) // 4 * 4 + 8
    shape = {"nhwc": (B, Ho, Wo, ld if wide else cout), "nchw": (B, cout, Ho, Wo), "ps": (B, 2 * Ho, 2 * Wo, cout // 4)}[form]
    fill = fine("widefill", shape) if wide else None
    out = Buf(dev, shape, fill)
    st = torch.zeros(32, 2, cout, dtype=torch.float64, device=dev) if stats else None
    rd = None if r is None else r.to(dev)
    if wide and r is not None:      # the residual is read in the output's layout: the same wide rows
        rd = torch.zeros(shape, device=dev)
        rd[..., 4:4 + cout] = r.to(dev)
    _, tags = run(lambda: ops.conv2d(xd, wp, None if b is None else b.to(dev), cout, k, stride, pad, dil, pro, epi, 0.25, rd,
                                     afd, out.t, form == "nchw", form == "ps", st, out_coff=4 if wide else None))
    sentinel(test, "out", out)
    got = out.t
    if wide:      # the neighbouring channels of the wide buffer: bitwise the prefill
        keep = torch.ones(ld, dtype=torch.bool)
        keep[4:4 + cout] = False
        assert torch.equal(out.t.cpu()[..., keep], fill[..., keep]), "%s: channels outside [out_coff, out_coff + Cout) changed" % test
        got = out.t[..., 4:4 + cout]
    judge(test, "out", got, ref, ref32, floor)
    if stats:     # slotted fp64 sums of the raw output: the sum is exact on the exact kind, the sum of squares is not (v^2 needs 2 x the bits)
        s = st.sum(0).cpu()
        (rs, rq) = ref64.conv_stats(raw)
        (rs32, rq32) = ref64.conv_stats(raw32 if cont else raw, dtype=F32)
        if not cont:
            exact(test, "stats sum", s[0], rs)
        else:
            check_derived(test, "stats sum / M", (s[0] / raw[..., 0].numel()).float(), rs / raw[..., 0].numel(), rs32 / raw[..., 0].numel())
        n = raw[..., 0].numel()
        check_derived(test, "stats sum of squares / M", (s[1] / n).float(), rq / n, rq32 / n)
    if expect is not None:      # (a reduce launch is asserted where the case names it; elsewhere the split is the plan's business)
        seen = tags if RED in expect else tags - {RED}
        assert seen == set(expect), "%s: kernel families %s ran, expected %s" % (test, sorted(tags), sorted(expect))
    return got, tags


# M >= 4096, cin <= 16, Cout <= 16, cin Cout <= 64 -> k_conv_direct<NG>, NG = ceil(Cout / 4): Cout 3 | 4 (NG 1), 5 | 8 (NG 2), 9 | 12 (NG 3),
# 13 | 16 (NG 4); (8, 8) and (16, 4) sit on cin Cout = 64.  M = 4096 exactly = 1 x 32 x 128: 16 whole 256-pixel blocks.  An NHWC row of
# Cout % 4 != 0 >= 4 channels is not a legal output (16-byte rows): those go to channels [4, 4 + Cout) of a wider buffer (out_ld / out_coff).
# k_conv_direct and k_conv_igemm<128,16|32> share ONE profile tag: expect={TN} here and in test_direct_forms rules out the halo / 64 / 128
# families only and does NOT tell the direct arm from the igemm one -- which of the two runs follows from M >= 4096 in the dispatch code
@pytest.mark.parametrize("cin,cout", [(4, 3), (4, 4), (4, 5), (4, 8), (4, 9), (4, 12), (4, 13), (4, 16), (8, 8), (16, 4)])
def test_direct(dev, cin, cout):
    wide = cout > 4 and cout % 4 != 0
    fwd(dev, "direct[cin%d cout%d M4096]" % (cin, cout), (cin,), cout, 3, 1, 32, 128, wide=wide, res=True, expect={TN})
    # 33 x 125 = 4125 = 16 x 256 + 29: a partial last block, odd row length
    fwd(dev, "direct[cin%d cout%d M4125]" % (cin, cout), (cin,), cout, 3, 1, 33, 125, wide=wide, pro="relu", expect={TN})
    # 31 x 132 = 4092 < 4096: k_conv_igemm<128,16> with the generic loader (the same tag, see above)
    fwd(dev, "direct[cin%d cout%d M4092 -> igemm]" % (cin, cout), (cin,), cout, 3, 1, 31, 132, wide=wide, expect={TN})


# direct kernel: 1 - 3 segments (4 + 4 + 4 channels x Cout 4: cin Cout = 48), per-segment and mixed affine, the BatchNorm statistics, NCHW
# store, 9 x 9 taps, a null bias, tanh / leaky epilogue (continuous)
def test_direct_forms(dev):
    fwd(dev, "direct[2 segs affine]", (4, 4), 4, 3, 1, 32, 128, aff=(1, 1), pro="relu", stats=True, expect={TN})
    fwd(dev, "direct[3 segs mixed affine]", (4, 4, 4), 4, 3, 1, 33, 125, aff=(0, 1, 0), stats=True, expect={TN})
    fwd(dev, "direct[9x9 nchw no bias]", (4,), 3, 9, 1, 32, 128, form="nchw", bias=False, expect={TN})
    fwd(dev, "direct[9x9 tanh]", (4,), 3, 9, 1, 33, 125, epi="tanh", expect={TN})
    fwd(dev, "direct[leaky001 on load, prelu, stats]", (4, 4), 8, 3, 1, 32, 128, pro="leaky001", epi="prelu", aff=(1, 0), stats=True, expect={TN})
    fwd(dev, "direct[stride 2]", (8,), 8, 4, 1, 128, 128, stride=2, pad=1, expect={TN})      # Hp x Wp = 64 x 64 = 4096


# halo_ok (stride 1, "same" 3 x 3 / 9 x 9, Hin % 8 == 0, Win % 16 == 0, 32-channel segments, M >= 1024) and Cout <= 4, no residual ->
# k_conv_halo_c4: tiles of 8 rows x 13 columns, so the last tile of Win = 16 / 32 / 48 has 3 / 6 / 9 columns.  M = 1024 exactly (2 x 32 x 16,
# 1 x 32 x 32) and 1152 (1 x 24 x 48)
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_halo_c4(dev, k, cout):
    for B, H, W in ((2, 32, 16), (1, 32, 32), (1, 24, 48)):
        fwd(dev, "halo_c4[k%d cout%d %dx%dx%d]" % (k, cout, B, H, W), (32,), cout, k, B, H, W, pro="relu", aff=(1,), expect={C4})


# the nearest shapes that do not qualify: Hin % 8 != 0 (36 x 32), Win % 16 != 0 (32 x 40), M = 896 < 1024 (8 x 112) -> k_conv_igemm<128,16>;
# a residual -> k_conv_halo<KS,16>; three 32-channel segments and the statistics stay on halo_c4
@pytest.mark.parametrize("k", [3, 9])
def test_halo_c4_leaves(dev, k):
    fwd(dev, "halo_c4[k%d Hin 36]" % k, (32,), 4, k, 1, 36, 32, expect={TN})
    fwd(dev, "halo_c4[k%d Win 40]" % k, (32,), 4, k, 1, 32, 40, expect={TN})
    fwd(dev, "halo_c4[k%d M 896]" % k, (32,), 4, k, 1, 8, 112, expect={TN})
    fwd(dev, "halo_c4[k%d residual]" % k, (32,), 4, k, 1, 32, 32, res=True, expect={HALO})
    fwd(dev, "halo_c4[k%d 3 segs stats]" % k, (32, 32, 32), 3, k, 1, 32, 32, aff=(1, 0, 1), stats=True, expect={C4})
    fwd(dev, "halo_c4[k%d sigmoid]" % k, (32,), 2, k, 1, 32, 32, epi="sigmoid", expect={C4})


# k_conv_halo<KS, BN, TH>: BN = 16 for Cout <= 16, else 64 -- Cout 5 (NCHW: an NHWC row of 5 is not a legal output), 16 | 17, 64 | 68 (a second
# column block of 4).  blocks8 = B (Hin / 8) (Win / 16) ceil(Cout / BN) < 768 -> TH = 4 for KS = 3 (every shape here); KS = 9: always TH = 8.
# bf16x3 pass, KS = 3, BN = 64: blocks8 >= 8 B takes the x3 halo kernel -- per image 32 x 32 has 4 x 2 = 8 tiles (x3 at Cout 17, 64, 68), 32 x 16 has
# 4: the fp32 kernel at Cout 17 and 64 (16 < 32), but two column blocks at Cout 68 make it 8 again (32 >= 32: x3).  Both sides at Cout 64
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("cout", [5, 16, 17, 64, 68])
def test_halo(dev, k, cout):
    form = "nchw" if cout % 4 else "nhwc"
    fwd(dev, "halo[k%d cout%d 2x32x32]" % (k, cout), (32,), cout, k, 2, 32, 32, form=form, pro="relu", aff=(1,), res=form == "nhwc", expect={HALO})
    fwd(dev, "halo[k%d cout%d 4x32x16]" % (k, cout), (32,), cout, k, 4, 32, 16, form=form, stats=True, expect={HALO})


# three segments with mixed affine; mish epilogue + leaky on load (continuous); pixel-shuffle store from the halo kernel
def test_halo_forms(dev):
    fwd(dev, "halo[3 segs]", (32, 32, 32), 64, 3, 1, 32, 32, aff=(1, 0, 1), pro="relu", expect={HALO})
    fwd(dev, "halo[leaky02 mish]", (32, 32), 36, 3, 2, 16, 32, pro="leaky02", epi="mish", aff=(1, 1), expect={HALO})
    fwd(dev, "halo[pixel shuffle]", (32,), 64, 3, 1, 32, 32, form="ps", expect={HALO})
    fwd(dev, "halo[gelu no bias]", (64,), 20, 3, 1, 32, 32, epi="gelu", bias=False, expect={HALO})


# KS = 3: blocks8 = 4 x 8 x 24 x 1 = 768 -> TH = 8; 4 x 8 x 23 = 736 -> TH = 4 (Cout = 16: one column block, 0.9 GFLOP for the reference)
@pytest.mark.parametrize("W,th", [(384, 8), (368, 4)])
def test_halo_th(dev, W, th):
    fwd(dev, "halo[TH%d 4x64x%d]" % (th, W), (32,), 16, 3, 4, 64, W, expect={HALO})


# halo_starved = (M / 128) ceil(Cout / 64) < 256 and Cout >= 128 (with a split-K workspace): M = 16384 -> 128 x 2 = 256: the halo kernel;
# M = 16256 does not tile (Hin % 8), M = 8192 -> 128 < 256: starved, the implicit GEMM on 128 x 128 tiles (K = 288: nk = 9 < 16, no split)
def test_halo_starved(dev):
    fwd(dev, "halo[starved off M16384]", (32,), 128, 3, 2, 64, 128, expect={HALO})
    fwd(dev, "halo[starved on M8192]", (32,), 128, 3, 1, 64, 128, expect={T128})


# tile choice of the implicit GEMM on a map the halo kernels do not take (M < 1024): Cout 16 | 20 -> <128,16> | <128,32> (one tag), 32 | 36 ->
# <128,32> | <64,64>, 124 | 128 -> <64,64> | <128,128>, and at Cout >= 128 M = 126 | 128 -> <64,64> | <128,128>
@pytest.mark.parametrize("cout,B,H,W,tag", [(16, 2, 9, 7, TN), (20, 2, 9, 7, TN), (32, 2, 9, 7, TN), (36, 2, 9, 7, T64), (124, 2, 8, 8, T64), (128, 2, 8, 8, T128),
                                            (128, 2, 9, 7, T64), (132, 2, 8, 8, T128), (132, 2, 9, 7, T64)])
def test_igemm_tiles(dev, cout, B, H, W, tag):
    fwd(dev, "igemm[cout%d M%d]" % (cout, B * H * W), (32,), cout, 3, B, H, W, res=True, expect={tag})
    fwd(dev, "igemm[cout%d M%d s2]" % (cout, B * H * W), (32,), cout, 3, B, 2 * H, 2 * W, stride=2, pad=1, pro="relu", aff=(1,), expect={tag})


# loaders.  generic: cin % 32 != 0 -- cin 4, 12 (K = 108: K % 32 != 0), 24, 36, and segments (12, 24) whose seam falls inside a 32-chunk
@pytest.mark.parametrize("segs", [(4,), (12,), (24,), (36,), (12, 24), (4, 8, 12)])
def test_loader_generic(dev, segs):
    fwd(dev, "loader generic[%s cout36]" % (segs,), segs, 36, 3, 3, 5, 7, aff=(0, 1, 1), pro="relu", expect={T64})
    fwd(dev, "loader generic[%s cout12 d2]" % (segs,), segs, 12, 3, 3, 10, 6, pad=2, dil=2, expect={TN})
    fwd(dev, "loader generic[%s cout128]" % (segs,), segs, 128, 3, 2, 8, 8, stats=True, expect={T128})


# UNI (32-channel segments, not SIMPLE): an input activation outside {none, relu, leaky02}; mixed affine segments; 9 x 9 = 81 > 31 taps on a
# map the halo kernel does not take.  SIMPLE: <= 31 taps, act(0) = 0, affine on none or (SIMPLE + AFF) all of the segments
@pytest.mark.parametrize("cout,tag", [(36, T64), (128, T128), (24, TN)])
def test_loader_uni_and_simple(dev, cout, tag):
    t = "loader[cout%d] " % cout
    fwd(dev, t + "UNI leaky001", (32, 64), cout, 3, 2, 8, 8, pro="leaky001", aff=(1, 1), expect={tag})
    fwd(dev, t + "UNI mish on load", (64,), cout, 3, 2, 8, 8, pro="mish", expect={tag})
    fwd(dev, t + "UNI mixed affine", (32, 32, 64), cout, 3, 2, 8, 8, aff=(1, 0, 1), pro="relu", expect={tag})
    fwd(dev, t + "UNI 81 taps", (32,), cout, 9, 2, 12, 20, aff=(1,), expect={tag})
    fwd(dev, t + "SIMPLE", (32, 64), cout, 3, 2, 8, 8, pro="relu", expect={tag})
    fwd(dev, t + "SIMPLE leaky02", (64,), cout, 3, 2, 8, 8, pro="leaky02", expect={tag})
    fwd(dev, t + "SIMPLE+AFF", (32, 32, 64), cout, 3, 2, 8, 8, aff=(1, 1, 1), pro="relu", expect={tag})
    fwd(dev, t + "SIMPLE+AFF d2 s2", (64,), cout, 4, 2, 16, 16, stride=2, pad=3, dil=2, aff=(1,), expect={tag})


# split-K: tiles < 384 and nk = Kp / 32 >= 16 -> S = min(ceil(768 / tiles), nk / 8, 64), then "no empty splits": cps = ceil(nk / S), S = ceil(nk / cps).
# 5 x 5 x 64: nk = 50 -> S = 6, cps = 9, S = 6: the last split has 5 chunks; 7 x 7 x 32: nk = 49 -> a last split of 4; 3 x 3 x 60: Kp = 544, nk = 17 -> 9 + 8
# (generic loader).  The reduce: cq_lanes 16 / 32 / 64 for Cout = 64 (and 100) / 128 / 256 (npad / 4 = 16 (25) / 32 / 64), so RL = 256 / cq_lanes = 16 / 8 / 4
# row lanes; at this M the plan's rows = 4 is raised to RL: rows per block = 16 / 8 / 4, ONE row per lane -- the single-row branch only.  The forms
# with several rows per lane: test_splitk_reduce_rows_per_lane below.
# The split-K workspace starts NaN-filled; XRED on / off and repeated runs: the same bits
@pytest.mark.parametrize("cout,tag", [(64, T64), (128, T128), (256, T128), (100, T64)])
@pytest.mark.parametrize("segs,k", [((64,), 5), ((32,), 7), ((60,), 3)])
def test_splitk(dev, cout, tag, segs, k):
    from dpmn_amd import ops
    lib = abi()[0]
    B, H, W = 3, 9, 10      # M = 270: 5 / 3 row tiles
    t = "splitk[%s k%d cout%d] " % (segs, k, cout)
    with stream_k(False):
        ops.splitk_workspace(dev).fill_(float("nan"))
        a, _ = fwd(dev, t + "reduce launch", segs, cout, k, B, H, W, aff=(1,), pro="relu", res=True, expect={tag, RED})
        b, _ = fwd(dev, t + "reduce launch, again", segs, cout, k, B, H, W, aff=(1,), pro="relu", res=True, expect={tag, RED})
        same_bits(t, "two runs", a, b)
        fwd(dev, t + "stats", segs, cout, k, B, H, W, stats=True, expect={tag, RED})
        fwd(dev, t + "nchw", segs, cout, k, B, H, W, form="nchw", bias=False, expect={tag, RED})
        fwd(dev, t + "mish", segs, cout, k, B, H, W, epi="mish", expect={tag, RED})
    with xred(1):      # the in-L2 reduction: SIMPLE loaders on 128 x 128 tiles only -- no reduce launch there
        # (7 x 7 = 49 taps: UNI, not SIMPLE; the bf16x3 pass has its own 128 x 128 kernel: both keep the reduce launch)
        xr = tag == T128 and segs[0] % 32 == 0 and k * k <= 31 and lib.dpmn_get_compute_dtype() != 2
        c, ran = fwd(dev, t + "xred on", segs, cout, k, B, H, W, aff=(1,), pro="relu", res=True, expect={tag} if xr else {tag, RED})
        assert not (xr and RED in ran), t + "the in-L2 reduction was asked for, yet the reduce kernel ran"
    same_bits(t, "xred on / off", a, c)


# the reduce with several rows per lane: rows = 16 once cb ceil(M / 16) >= 1024, i.e. M >= 16369 (cb = 1 column block of the reduce for every Cout
# here).  Cout 128: RL = 8, two rows per lane -- one pass of the two-rows-per-iteration loop (rows m, m + 8); Cout 256: RL = 4, four rows per lane --
# two passes.  M = 4 x 64 x 64 = 16384: whole blocks; M = 4 x 63 x 65 = 16380: the last block has 12 rows, so at RL = 8 lanes 0 .. 3 run the pair
# and lanes 4 .. 7 the single-row tail, at RL = 4 every lane runs one pair, then the tail.  With the statistics (their order: row m, then m + RL).
# 5 x 5 x 32: nk = 25; Cout 128: 128 tiles, S = min(6, 25 / 8) = 3, cps = 9: 9 + 9 + 7; Cout 256: 256 tiles, S = 3 cut to 2 by the 32 MB cap on the
# partial sums (2 x 16384 x 256 x 4 bytes = the cap exactly), cps = 13: 13 + 12.  (Cout 64 has RL = 16 = rows at every M: always one row per lane.
#  rows = 64 needs cb ceil(M / 64) >= 1024 with fewer than 384 tiles: no shape has both.)
@pytest.mark.parametrize("B,H,W", [(4, 64, 64), (4, 63, 65)])
@pytest.mark.parametrize("cout", [128, 256])
def test_splitk_reduce_rows_per_lane(dev, cout, B, H, W):
    with stream_k(False):
        fwd(dev, "splitk[cout%d M%d rows 16]" % (cout, B * H * W), (32,), cout, 5, B, H, W, stats=True, expect={T128, RED})
    fwd(dev, "splitk[cout%d M%d rows 16 nchw relu]" % (cout, B * H * W), (32,), cout, 5, B, H, W, form="nchw", epi="relu", aff=(1,), expect={T128, RED})


# stream-K on 64-row tiles: Cout >= 128, M % 128 != 0, M % 64 == 0, M <= 1024, a SIMPLE loader -- M = 192, 320.  Fallbacks to the fixed split on
# 128 x 128 tiles: mixed affine, an activation outside the SIMPLE set, no arrival counters.  Exact sums: every path the same bits
@pytest.mark.parametrize("B", [3, 5])
def test_streamk(dev, B):
    from dpmn_amd import ops
    t = "streamk[M%d] " % (B * 64)
    a, _ = fwd(dev, t + "sk", (64, 64), 128, 3, B, 8, 8, aff=(1, 1), pro="relu", res=True, expect={SK})
    b, _ = fwd(dev, t + "sk again", (64, 64), 128, 3, B, 8, 8, aff=(1, 1), pro="relu", res=True, expect={SK})
    same_bits(t, "two runs", a, b)
    fwd(dev, t + "sk stats 2 column tiles", (64,), 132, 4, B, 16, 16, stride=2, pad=1, stats=True, expect={SK})
    fwd(dev, t + "sk leaky02 nchw", (64,), 128, 3, B, 8, 8, pro="leaky02", form="nchw", expect={SK})
    fwd(dev, t + "mixed affine -> fixed split", (64, 64), 128, 3, B, 8, 8, aff=(1, 0), pro="relu", expect={T128, RED})
    fwd(dev, t + "mish on load -> fixed split", (64, 64), 128, 3, B, 8, 8, pro="mish", expect={T128, RED})
    with stream_k(False):
        c, _ = fwd(dev, t + "no counters -> fixed split", (64, 64), 128, 3, B, 8, 8, aff=(1, 1), pro="relu", res=True, expect={T128, RED})
    same_bits(t, "stream-K / fixed split", a, c)
    assert all(int(cnt.abs().max()) == 0 for cnt in ops._ARRIVE_CNT.values()), t + "arrival counters not left at zero"


def test_pixel_shuffle_and_null_bias(dev):
    fwd(dev, "igemm[pixel shuffle cout16]", (32,), 16, 3, 2, 6, 10, form="ps", epi="relu", expect={TN})
    fwd(dev, "igemm[pixel shuffle cout64 mish]", (36,), 64, 3, 2, 6, 10, form="ps", epi="mish", bias=False, expect={T64})
    fwd(dev, "igemm[null bias cout128]", (32,), 128, 3, 2, 8, 8, bias=False, expect={T128})
    fwd(dev, "igemm[wide out cout36]", (32,), 36, 3, 2, 9, 7, wide=True, res=True, expect={T64})
    fwd(dev, "igemm[wide out cout128 splitk]", (64,), 128, 5, 3, 9, 10, wide=True, expect={T128, RED})


# ------------------------------------------------------------------------------------------------------------------ transposed conv, phases, scatter
@functools.lru_cache(maxsize=None)
def _ct_case(segs, cout, B, H, W, pro, aff):
    xs = [op("tx%d" % i, (B, H, W, c)) for i, c in enumerate(segs)]
    wt, b = op("tw", (sum(segs), cout, 4, 4)), fine("tb", (cout,))
    af = [(scale3("tsc%d" % i, c), op("tsh%d" % i, (c,))) if a else None for i, (c, a) in enumerate(zip(segs, aff))] if any(aff) else None
    ref = ref64.conv_transpose2d(xs, wt, b, 2, 1, ACT[pro], affine=af)
    in_range("convT", ref64.conv_transpose2d([ref64.conv_input(xs, af, ACT[pro]).abs()], wt.abs(), None, 2, 1) + 2.0)
    return xs, wt, b, af, ref


def _ct_launch(dev, xd, wp4, b, cout, out, pro, afd, stats=None):
    """the phase-fused launch of ops.convT_s2k4 into a caller-owned output"""
    from dpmn_amd import ops, _abi
    d = ops.conv_desc(xd, 2, cout=cout, pro_act=pro, affine=afd, phase=(0, 0))
    d.nphase, d.w_phase_stride = 4, wp4.shape[1] * wp4.shape[2]
    d.w, d.bias, d.out, d.stats = _abi.dptr(wp4), _abi.dptr(b, True), _abi.dptr(out), ops._stats_ptr(stats, cout)
    ops._attach_workspace(d, out.device)
    _abi.check(_abi.lib.dpmn_conv2d_nhwc_f32(C.byref(d), _abi.stream()))


# nphase = 4 (ConvTranspose2d(4, 2, 1) as four 2 x 2 phase convs with dil -1 in one launch) against ref64.conv_transpose2d: Cout 36 -> <64,64>,
# 128 with M = 192 per phase -> stream-K on 64-row tiles, 128 with M = 120 -> <64,64>, 16 -> <128,16>; the GPU phase packs (tpack_convT_s2k4)
@pytest.mark.parametrize("segs,cout,B,H,W,tags", [((32,), 36, 2, 5, 7, {T64}), ((64, 64), 128, 3, 8, 8, {SK}), ((36,), 128, 3, 5, 8, {T64}), ((12, 4), 16, 3, 3, 5, {TN}),
                                                  ((32, 32), 128, 4, 8, 8, {T128})])
def test_conv_transpose_phase_fused(dev, segs, cout, B, H, W, tags):
    from dpmn_amd.model import packing
    t = "convT4[%s cout%d M%d] " % (segs, cout, B * H * W)
    for pro, aff in (("none", (0, 0)), ("relu", (1, 1))):
        xs, wt, b, af, ref = _ct_case(segs, cout, B, H, W, pro, aff[:len(segs)])
        xd, afd = [x.to(dev) for x in xs], None if af is None else [(a[0].to(dev), a[1].to(dev)) for a in af]
        wp4 = packing.tpack_convT_s2k4(wt.to(dev))
        out = Buf(dev, (B, 2 * H, 2 * W, cout))
        _, ran = run(lambda: _ct_launch(dev, xd, wp4, b.to(dev), cout, out.t, pro, afd))
        sentinel(t, "out", out)
        exact(t + pro, "out", out.t, ref)
        assert ran - {RED} == tags, "%s: kernel families %s ran, expected %s" % (t, sorted(ran), sorted(tags))


# a single phase (ops.conv2d(phase=(py, px)): k 2, dil -1, pad -phase, ostep 2): writes output pixels (2 y + py, 2 x + px) only -- the other
# three quarters of a prefilled output stay bitwise as they were
@pytest.mark.parametrize("py,px", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_conv_transpose_single_phase(dev, py, px):
    from dpmn_amd import ops
    from dpmn_amd.model import packing
    segs, cout, B, H, W = (32,), 36, 2, 5, 7
    xs, wt, b, af, ref = _ct_case(segs, cout, B, H, W, "relu", (1,))
    fill = fine("phasefill", (B, 2 * H, 2 * W, cout))
    out = Buf(dev, fill.shape, fill)
    wp = packing.tpack_convT_s2k4(wt.to(dev))[2 * py + px]
    ops.conv2d([xs[0].to(dev)], wp, b.to(dev), cout, 2, pro_act="relu", affine=[(af[0][0].to(dev), af[0][1].to(dev))], out=out.t, phase=(py, px))
    sentinel("phase", "out", out)
    want = fill.double().clone()
    want[:, py::2, px::2] = ref[:, py::2, px::2]
    exact("convT phase (%d, %d)" % (py, px), "out", out.t, want)


# ------------------------------------------------------------------------------------------------------------------ groups = 2
@functools.lru_cache(maxsize=None)
def _grp_case(cin, cout, k, B, H, W, stride, pad, dil):
    x = op("gx", (B, H, W, cin))
    ws, bs = [op("gw%d" % g, (cout, cin, k, k)) for g in range(2)], [fine("gb%d" % g, (cout,)) for g in range(2)]
    h = B // 2
    ref = torch.cat([ref64.conv2d([x[g * h:(g + 1) * h]], ws[g], bs[g], stride, pad, dil, ACT["relu"]) for g in range(2)], 0)
    in_range("groups", ref64.conv2d([x.abs()], torch.max(ws[0].abs(), ws[1].abs()), None, stride, pad, dil) + 2.0)
    return x, ws, bs, ref


# images [B / 2, B) take the second weight set.  (a) whole row tiles: m_per_group = 128 on <64,64>, 256 on <128,128> (split-K), 192 on the
# 64-row stream-K tiles; (b) split_groups inside the library: m_per_group = 192 at Cout 32 (<128,32> wants % 128; ops.conv2d asks % 64 up to
# 512 pixels) and at Cout 128 without arrival counters; (c) the Python-side split of ops.conv2d: m_per_group = 100
@pytest.mark.parametrize("cin,cout,B,H,W,counters,tags", [
    (32, 64, 4, 8, 8, True, {T64}), (64, 128, 8, 8, 8, True, {T128, RED}), (64, 128, 6, 8, 8, True, {SK}),
    (32, 32, 6, 8, 8, True, {TN}), (64, 128, 6, 8, 8, False, {T128, RED}), (32, 64, 4, 5, 10, True, {T64})])
def test_groups2(dev, cin, cout, B, H, W, counters, tags):
    from dpmn_amd import ops
    from dpmn_amd.model import packing
    t = "groups2[cin%d cout%d mpg%d%s]" % (cin, cout, B // 2 * H * W, "" if counters else " no counters")
    x, ws, bs, ref = _grp_case(cin, cout, 3, B, H, W, 1, 1, 1)
    wp = torch.stack([packing.pack_conv(w.to(dev))[0] for w in ws]).contiguous()
    bp = torch.stack(bs).to(dev)
    python_split = (B // 2 * H * W) % 64 != 0
    out = None if python_split else Buf(dev, (B, H, W, cout))
    with stream_k(counters):
        got, ran = run(lambda: ops.conv2d([x.to(dev)], wp, bp, cout, 3, pad=1, pro_act="relu", groups=2, out=None if out is None else out.t))
    if out is not None:
        sentinel(t, "out", out)
    exact(t, "out", got, ref)
    assert ran == tags, "%s: kernel families %s ran, expected %s" % (t, sorted(ran), sorted(tags))


# ------------------------------------------------------------------------------------------------------------------ bf16 mode
@pytest.fixture
def bf16_mode():
    """dpmn_set_compute_dtype(1) for one test, the mode of the surrounding pass put back afterwards"""
    lib, check, _, _ = abi()
    old = lib.dpmn_get_compute_dtype()
    check(lib.dpmn_set_compute_dtype(1))
    try:
        yield
    finally:
        check(lib.dpmn_set_compute_dtype(old))


# bf16 operands (8 significant bits): the exact kind's transformed inputs have at most 8, its weights 6 -- the bf16 igemm on 128 x 128 and
# 64 x 64 tiles (SIMPLE loaders only) and the 3 x 3 BN = 64 halo kernel must still reproduce float64 bit for bit
def test_bf16_mode(dev, bf16_mode):
    fwd(dev, "bf16[igemm 128]", (32, 32), 128, 3, 2, 8, 8, aff=(1, 1), pro="relu", res=True, expect={T128})
    fwd(dev, "bf16[igemm 128 splitk]", (64,), 128, 5, 3, 9, 10, aff=(1,), expect={T128, RED})
    fwd(dev, "bf16[igemm 64]", (32, 32), 36, 3, 2, 9, 7, aff=(1, 1), pro="relu", res=True, expect={T64})
    fwd(dev, "bf16[igemm 64 s2]", (64,), 64, 4, 2, 16, 16, stride=2, pad=1, expect={T64})
    fwd(dev, "bf16[halo 3x3]", (32, 32), 64, 3, 2, 32, 32, aff=(1, 1), pro="relu", res=True, expect={HALO})
    fwd(dev, "bf16[halo 3x3 cout68]", (32,), 68, 3, 4, 32, 16, expect={HALO})


# ------------------------------------------------------------------------------------------------------------------ weight gradient
def _layout(shape, layout, phase=None):
    """(co, ci, strides) of pgrm_train.conv_wgrad_into for a parameter-layout gradient tensor"""
    if layout == "conv":
        co, ci, kh, kw = shape
        return co, ci, (ci * kh * kw, kh * kw, kw, 1, 0)
    if layout == "convT_s1":
        ci, co, kh, kw = shape
        return co, ci, (kh * kw, co * kh * kw, -kw, -1, (kh - 1) * kw + (kw - 1))
    ci, co = shape[:2]
    return co, ci, (16, co * 16, 8, 2, (1 - phase[0]) * 4 + (1 - phase[1]))


def wgrad_gpu(dev, d, dyd, dw, layout, mode, phase=None, expect_slots=None):
    """one weight gradient accumulated into the prefilled parameter-layout Buf `dw`, on caller-owned workspaces.  mode: 'excl' (exclusive
    NaN-filled slots + unpack), 'atomic1' / 'atomic32' (packed copies from a 2^-10 prefill, unpack with clear), 'strided'.  Returns the slot
    count of the plan."""
    lib, check, dptr, st = abi()
    cin = sum(d.cseg[i] for i in range(3) if d.inp[i])
    kp = (d.KH * d.KW * cin + 31) // 32 * 32
    co, ci, strides = _layout(dw.t.shape, layout, phase)
    slots = C.c_int(-1)
    check(lib.dpmn_conv2d_wgrad_excl_slots(C.byref(d), C.cast(C.pointer(slots), C.c_void_p)))
    if mode == "excl":
        assert slots.value > 0
        ws = Buf(dev, (slots.value, d.Cout, kp))
        before = dw.flat.clone()
        assert lib.dpmn_conv2d_wgrad_excl_f32(C.byref(d), dptr(dyd), dptr(ws.t), slots.value + 1, st) != 0, "a wrong slot count was accepted"
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws.t).all()) and torch.equal(dw.flat, before), "the rejected call wrote"
        _, ran = run(lambda: check(lib.dpmn_conv2d_wgrad_excl_f32(C.byref(d), dptr(dyd), dptr(ws.t), slots.value, st)))
        assert ran == {WG}, ran
        sentinel("wgrad", "slots", ws)
        assert not bool(torch.isnan(ws.t).any()), "an exclusive slot was not fully written"
        check(lib.dpmn_conv2d_wgrad_unpack_f32(dptr(ws.t), dptr(dw.t), d.Cout, cin, d.KH, d.KW, co, ci, *strides, 0, slots.value, st))
    elif mode.startswith("atomic"):
        n = int(mode[6:])
        pre = fine("wsfill", (n, d.Cout, kp))
        ws = Buf(dev, (n, d.Cout, kp), pre)
        check(lib.dpmn_conv2d_wgrad_f32(C.byref(d), dptr(dyd), dptr(ws.t), n, st))
        check(lib.dpmn_conv2d_wgrad_unpack_f32(dptr(ws.t), dptr(dw.t), d.Cout, cin, d.KH, d.KW, co, ci, *strides, 1, n, st))
        torch.cuda.synchronize()
        sentinel("wgrad", "packed copies", ws)
        assert int((ws.t != 0).sum()) == 0, "unpack(clear = 1) left the packed copies non-zero"
        return slots.value, pre
    else:
        check(lib.dpmn_conv2d_wgrad_strided_f32(C.byref(d), dptr(dyd), dptr(dw.t), co, ci, *strides, st))
    torch.cuda.synchronize()
    return slots.value, None


def _unpack_ref(pre, shape, layout, cin_d, k, phase=None):
    """what the unpack adds for the prefilled packed copies: their sum, read back through the layout"""
    co, ci, st = _layout(shape, layout, phase)
    s = pre.double().sum(0)[:, :k * k * cin_d].reshape(-1, k, k, cin_d)[:co, :, :, :ci]      # (co, ky, kx, ci)
    if layout == "conv":
        return s.permute(0, 3, 1, 2)
    if layout == "convT_s1":
        return s.flip(1, 2).permute(3, 0, 1, 2)
    raise ValueError(layout)


@functools.lru_cache(maxsize=None)
def _wg_case(segs, cout, k, B, H, W, stride, pad, dil, pro, aff):
    xs = [op("wx%d" % i, (B, H, W, c)) for i, c in enumerate(segs)]
    af = [(scale3("wsc%d" % i, c), op("wsh%d" % i, (c,))) if a else None for i, (c, a) in enumerate(zip(segs, aff))] if any(aff) else None
    Ho, Wo = conv_out(H, k, stride, pad, dil), conv_out(W, k, stride, pad, dil)
    cont = pro not in ("none", "relu")
    dy = (u if cont else op)("wdy", (B, Ho, Wo, cout))
    if cont:
        xs = [u("wx%d" % i, (B, H, W, c)) for i, c in enumerate(segs)]
    if cont:
        ref, ref32 = both(ref64.conv2d_wgrad, xs, dy, k, stride, pad, dil, ACT[pro], af)
    else:
        ref, ref32 = ref64.conv2d_wgrad(xs, dy, k, stride, pad, dil, ACT[pro], af), None
    if not cont:
        in_range("wgrad", ref64.conv2d_wgrad([ref64.conv_input(xs, af, ACT[pro]).abs()], dy.abs(), k, stride, pad, dil) + 2.0 * 33)
    return xs, af, dy, ref, ref32


def wgrad(dev, test, segs, cout, k, B, H, W, stride=1, pad=None, dil=1, pro="none", aff=(0, 0, 0), modes=("excl", "atomic1", "strided"), mutate=None):
    from dpmn_amd import ops
    segs = tuple(segs)
    pad = (k - 1) // 2 if pad is None else pad
    xs, af, dy, ref, ref32 = _wg_case(segs, cout, k, B, H, W, stride, pad, dil, pro, tuple(aff[:len(segs)]))
    xd, dyd = [x.to(dev) for x in xs], dy.to(dev)
    if mutate is not None:
        dyd = mutate(dyd)
    afd = None if af is None else [None if a is None else (a[0].to(dev), a[1].to(dev)) for a in af]
    d = ops.conv_desc(xd, k, stride, pad, dil, cout=cout, pro_act=pro, affine=afd)
    fill = fine("dwfill", ref.shape)
    outs = []
    for mode in modes:
        dw = Buf(dev, ref.shape, fill)
        slots, pre = wgrad_gpu(dev, d, dyd, dw, "conv", mode)
        sentinel(test, "dW " + mode, dw)
        add = 0.0 if pre is None else _unpack_ref(pre, ref.shape, "conv", sum(segs), k)
        judge(test + " " + mode, "dW", dw.t, fill.double() + add + ref, None if ref32 is None else (fill + (add.float() if pre is not None else 0.0) + ref32))
        outs.append(dw.t)
    return outs


# the four tiles -- BN = 16 (Cout <= 16), 64 (<= 64), 128; BKT = 128 for BN = 128 and for BN = 64 when it pads K less (K = 288), else 256
# (K = 512) -- each in the P2 form (Hp, Wp powers of two, activation none / relu / leaky02) and the generic one (any other plane, or
# leaky001): <16,256> Cout 12, <64,128> Cout 36 K 288, <64,256> Cout 64 K 512, <128,128> Cout 68 (one partial 128-row
# co tile) and Cout 132 (a second co tile of 4 rows).  M = B Hp Wp: P2 8 x 16 x 4 = 512; generic 5 x 7 x 3 = 105
@pytest.mark.parametrize("cin,cout,k", [(32, 12, 3), (32, 36, 3), (32, 64, 4), (32, 68, 3), (64, 132, 3)])
def test_wgrad_tiles(dev, cin, cout, k):
    pad = 1 if k == 3 else 2
    for B, H, W, form in ((4, 8, 16, "P2"), (3, 5, 7, "generic")):
        t = "wgrad[cin%d cout%d k%d %s]" % (cin, cout, k, form)
        if k == 4:      # 4 x 4 pad 2 grows the plane by one: Hp x Wp = 8 x 16 needs a 7 x 15 input, the generic plane is 6 x 8
            H, W = H - 1, W - 1
        a = wgrad(dev, t, (cin,), cout, k, B, H, W, pad=pad, pro="relu")
        same_bits(t, "excl / strided", a[0], a[2])


# generic maps whose rows are shorter than the loaders' row strides (4, 8, 16 pixels between a thread's loads): several row and image wraps
# per step -- Hp x Wp = 1 x 3, 3 x 1, 2 x 5, 5 x 7, 9 x 12 with B = 3 .. 40
@pytest.mark.parametrize("B,H,W", [(40, 1, 3), (37, 3, 1), (13, 2, 5), (3, 5, 7), (3, 9, 12)])
@pytest.mark.parametrize("cout", [12, 36, 68])
def test_wgrad_small_planes(dev, cout, B, H, W):
    wgrad(dev, "wgrad[cout%d %dx%dx%d]" % (cout, B, H, W), (32,), cout, 3, B, H, W, aff=(1,), pro="relu")


# atomic mode with one copy: pix_per_block >= 512 -- M = 511 one split, 512 exactly one, 513 a second split of ONE pixel, 545 a second of 33
# (M % 32 != 0); 7 x 73, 27 x 19, 5 x 109 are generic planes, 8 x 64 is P2 (and generic under leaky001, continuous kind)
@pytest.mark.parametrize("B,H,W", [(1, 7, 73), (1, 8, 64), (1, 27, 19), (5, 1, 109)])
def test_wgrad_m_edges(dev, B, H, W):
    for cout in (12, 36, 132):
        wgrad(dev, "wgrad[cout%d M%d]" % (cout, B * H * W), (32,), cout, 3, B, H, W)
    wgrad(dev, "wgrad[leaky001 M%d]" % (B * H * W), (32,), 36, 3, B, H, W, pro="leaky001", aff=(1,))


# 1 - 3 segments with per-segment and mixed affine; the input activation none / relu / leaky02 (P2) and leaky001 (generic); the seam of
# (12, 24, 4) lies inside a thread's float4-aligned k columns only at multiples of 4 (segment channel counts are multiples of 4)
@pytest.mark.parametrize("pro", ["none", "relu", "leaky02", "leaky001"])
def test_wgrad_segments(dev, pro):
    for segs, aff in (((32,), (1,)), ((32, 32), (1, 0)), ((12, 24, 4), (0, 1, 1)), ((32, 64, 32), (1, 1, 1))):
        for B, H, W in ((2, 8, 8), (3, 5, 7)):
            wgrad(dev, "wgrad[%s aff%s %s %dx%d]" % (segs, aff, pro, H, W), segs, 36, 3, B, H, W, pro=pro, aff=aff)


# stride 2, dilation 2, pad 3 (the EncodeBlock conv): 10 x 14 -> 5 x 7 generic, 16 x 32 -> 8 x 16 P2; pad > radius: taps that never meet the image
def test_wgrad_strided_dilated(dev):
    for B, H, W in ((3, 10, 14), (2, 16, 32)):
        wgrad(dev, "wgrad[k4 s2 d2 p3 %dx%d]" % (H, W), (32,), 36, 4, B, H, W, stride=2, pad=3, dil=2, aff=(1,), pro="relu")
        wgrad(dev, "wgrad[k3 s2 p3 %dx%d]" % (H, W), (32,), 68, 3, B, H, W, stride=2, pad=3)


# excl_slots reports 0 for BN = 16 with K <= 128 (a tiny gradient over many pixels): the slotted-atomic path with 32 copies
def test_wgrad_excl_slots_zero(dev):
    from dpmn_amd import ops
    lib, check, _, _ = abi()
    x = op("zx", (2, 16, 16, 12)).to(dev)
    d = ops.conv_desc([x], 3, 1, 1, 1, cout=4)
    slots = C.c_int(-1)
    check(lib.dpmn_conv2d_wgrad_excl_slots(C.byref(d), C.cast(C.pointer(slots), C.c_void_p)))
    assert slots.value == 0
    for B, H, W in ((2, 16, 16), (3, 9, 12)):
        wgrad(dev, "wgrad[slots 0 %dx%d]" % (H, W), (12,), 4, 3, B, H, W, modes=("atomic32", "atomic1", "strided"))


# ci_lim = 3 of a 4-padded input and co_lim = 3 of a 4-padded dy: the gradient tensor is (3, 3, k, k); padding channels are dropped by the
# unpack (exclusive / atomic) and by the atomic epilogue itself (strided)
@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (3, 9, 12)])
def test_wgrad_channel_limits(dev, B, H, W):
    from dpmn_amd import ops
    x, dy = op("lx", (B, H, W, 4)), op("ldy", (B, H, W, 4))
    ref = ref64.conv2d_wgrad([x], dy, 3, 1, 1, 1)[:3, :3].contiguous()
    xd = x.to(dev)      # (the descriptor holds the bare pointer: the tensor has to outlive it)
    d = ops.conv_desc([xd], 3, 1, 1, 1, cout=4)
    fill = fine("lfill", ref.shape)
    for mode in ("atomic32", "strided"):
        dw = Buf(dev, ref.shape, fill)
        _, pre = wgrad_gpu(dev, d, dy.to(dev), dw, "conv", mode)
        sentinel("limits", "dW", dw)
        add = 0.0 if pre is None else _unpack_ref(pre, ref.shape, "conv", 4, 3)
        exact("wgrad[limits %dx%d %s]" % (H, W, mode), "dW", dw.t, fill.double() + add + ref)


# ConvTranspose2d(3, 1, 1): the conv with flipped taps, gradient in the (Cin, Cout, KH, KW) layout
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (3, 5, 7)])
def test_wgrad_convT_s1(dev, B, H, W):
    from dpmn_amd import ops
    cin, cout = 32, 36
    x, dy = op("sx", (B, H, W, cin)), op("sdy", (B, H, W, cout))
    ref = ref64.conv_transpose2d_wgrad([x], dy, 3, 1, 1, ACT["relu"])
    xd = x.to(dev)
    d = ops.conv_desc([xd], 3, 1, 1, 1, cout=cout, pro_act="relu")
    fill = fine("sfill", ref.shape)
    for mode in ("excl", "atomic1", "strided"):
        dw = Buf(dev, ref.shape, fill)
        _, pre = wgrad_gpu(dev, d, dy.to(dev), dw, "convT_s1", mode)
        sentinel("convT_s1", "dW", dw)
        add = 0.0 if pre is None else _unpack_ref(pre, ref.shape, "convT_s1", cin, 3)
        exact("wgrad[convT_s1 %dx%d %s]" % (H, W, mode), "dW", dw.t, fill.double() + add + ref)


# the four phases of ConvTranspose2d(4, 2, 1) (ostep 2, dil -1, pad -phase: dy read at pixels (2 y + py, 2 x + px)), each accumulated into its
# taps of the (Cin, Cout, 4, 4) gradient, assembled and compared with the transposed conv's weight gradient; 4 x 8 P2, 3 x 5 generic
@pytest.mark.parametrize("B,H,W", [(4, 4, 8), (3, 3, 5)])
@pytest.mark.parametrize("cout", [12, 36, 68])
def test_wgrad_convT_phases(dev, cout, B, H, W):
    from dpmn_amd import ops
    cin = 32
    x, dy = op("px", (B, H, W, cin)), op("pdy", (B, 2 * H, 2 * W, cout))
    sc, sh = scale3("psc", cin), op("psh", (cin,))
    ref = ref64.conv_transpose2d_wgrad([x], dy, 4, 2, 1, ACT["relu"], [(sc, sh)])
    xd, dyd, afd = x.to(dev), dy.to(dev), [(sc.to(dev), sh.to(dev))]
    fill = fine("pfill", ref.shape)
    for mode in (("excl", "strided") if cout > 16 else ("strided",)):      # (Cout 12, K = 128: excl_slots reports 0)
        dw = Buf(dev, ref.shape, fill)
        for py in range(2):
            for px in range(2):
                d = ops.conv_desc([xd], 2, cout=cout, pro_act="relu", affine=afd, phase=(py, px))
                wgrad_gpu(dev, d, dyd, dw, "convT_s2k4", mode, (py, px))
        sentinel("convT phases", "dW", dw)
        exact("wgrad[convT phases cout%d %dx%d %s]" % (cout, H, W, mode), "dW", dw.t, fill.double() + ref)


# the production path (pgrm_train.conv_wgrad_into on its own workspaces) in both reduction modes
def test_wgrad_into(dev, monkeypatch):
    from dpmn_amd import ops
    from dpmn_amd.train import pgrm_train
    xs, af, dy, ref, _ = _wg_case((32, 32), 36, 3, 3, 5, 7, 1, 1, 1, "relu", (1, 0))
    afd = [(af[0][0].to(dev), af[0][1].to(dev)), None]
    xd = [x.to(dev) for x in xs]
    d = ops.conv_desc(xd, 3, 1, 1, 1, cout=36, pro_act="relu", affine=afd)
    fill = fine("ifill", ref.shape)
    for mode in ("excl", "atomic"):
        monkeypatch.setattr(pgrm_train, "WGRAD_MODE", mode)
        dw = Buf(dev, ref.shape, fill)
        pgrm_train.conv_wgrad_into(d, dy.to(dev), dw.t, "conv")
        sentinel("into", "dW", dw)
        exact("wgrad[conv_wgrad_into %s]" % mode, "dW", dw.t, fill.double() + ref)


# ------------------------------------------------------------------------------------------------------------------ data gradients
@functools.lru_cache(maxsize=None)
def _dg_w(O, I, k, transposed):
    return op("dgw", (I, O, k, k) if transposed else (O, I, k, k))


# the five constructions of train/cmm_train.py Unit.bwd_inputs against the adjoint, for an input-channel slice [c0, c0 + cs) with c0 != 0 and
# cs < cin: small (O 8, I 12: <128,16> generic loader) and wide (O 64, I 96: 64 x 64 tiles / the halo kernel, SIMPLE loader)
@pytest.mark.parametrize("O,I,c0,cs,B,H,W", [(8, 12, 4, 4, 3, 5, 7), (64, 96, 32, 36, 2, 8, 16), (32, 96, 32, 64, 2, 32, 16)])
@pytest.mark.parametrize("kind", ["conv3", "convT3", "convT4s2", "conv4s2", "conv4s2d2"])
def test_data_gradients(dev, kind, O, I, c0, cs, B, H, W):
    """H x W: the plane of dy (the conv's output)"""
    from dpmn_amd import ops
    from dpmn_amd.model import packing
    t = "dgrad[%s O%d I%d c0 %d cs %d %dx%dx%d]" % (kind, O, I, c0, cs, B, H, W)
    if kind == "conv3":
        w, dy = _dg_w(O, I, 3, False), op("dgy", (B, H, W, O))
        ref = ref64.conv2d_dgrad(dy, w, (H, W), 1, 1, 1, c0, cs)
        absref = ref64.conv2d_dgrad(dy.abs(), w.abs(), (H, W), 1, 1, 1, c0, cs)
        out = Buf(dev, ref.shape)
        ops.conv2d([dy.to(dev)], packing.tpack_dgrad_conv_s1(w.to(dev), c0, cs), None, cs, 3, pad=1, out=out.t)
    elif kind == "convT3":      # cin_pad = cout: dy carries `O + 4` channels, the last four meet zero weights
        w, dy = _dg_w(O, I, 3, True), op("dgyp", (B, H, W, O + 4))
        ref = ref64.conv_transpose2d_dgrad(dy[..., :O], w, 1, 1, c0, cs)
        absref = ref64.conv_transpose2d_dgrad(dy[..., :O].abs(), w.abs(), 1, 1, c0, cs)
        out = Buf(dev, ref.shape)
        ops.conv2d([dy.to(dev)], packing.tpack_dgrad_convT(w.to(dev), c0, cs, cin_pad=O + 4), None, cs, 3, pad=1, out=out.t)
    elif kind == "convT4s2":    # dy (B, 2 h, 2 w): the transposed conv's output; dX on (h, w)
        w, dy = _dg_w(O, I, 4, True), op("dgy", (B, H, W, O))
        ref = ref64.conv_transpose2d_dgrad(dy, w, 2, 1, c0, cs)
        absref = ref64.conv_transpose2d_dgrad(dy.abs(), w.abs(), 2, 1, c0, cs)
        out = Buf(dev, ref.shape)
        ops.conv2d([dy.to(dev)], packing.tpack_dgrad_convT(w.to(dev), c0, cs), None, cs, 4, stride=2, pad=1, out=out.t)
    elif kind == "conv4s2":     # Conv2d(4, 2, 1): dX on (2 H, 2 W) as the four phases of the matching transposed conv
        w, dy = _dg_w(O, I, 4, False), op("dgy", (B, H, W, O))
        ref = ref64.conv2d_dgrad(dy, w, (2 * H, 2 * W), 2, 1, 1, c0, cs)
        absref = ref64.conv2d_dgrad(dy.abs(), w.abs(), (2 * H, 2 * W), 2, 1, 1, c0, cs)
        out = Buf(dev, ref.shape)
        _ct_launch(dev, [dy.to(dev)], packing.tpack_dgrad_conv_s2k4(w.to(dev), c0, cs), None, cs, out.t, "none", None)
    else:                       # Conv2d(4, stride 2, pad 3, dil 2): iy = 2 oy + 2 ky - 3 is odd -- a scatter to the odd pixels; the even ones keep the prefill
        w, dy = _dg_w(O, I, 4, False), op("dgy", (B, H, W, O))
        Hi, Wi = 2 * H, 2 * W
        ref = ref64.conv2d_dgrad(dy, w, (Hi, Wi), 2, 3, 2, c0, cs)
        absref = ref64.conv2d_dgrad(dy.abs(), w.abs(), (Hi, Wi), 2, 3, 2, c0, cs)
        assert float(ref[:, 0::2].abs().max()) == 0.0 and float(ref[:, :, 0::2].abs().max()) == 0.0
        fill = fine("dgfill", ref.shape)
        out = Buf(dev, ref.shape, fill)
        geom = dict(stride=1, dil_y=-1, dil_x=-1, pad_y=-2, pad_x=-2, Hp=Hi // 2, Wp=Wi // 2, Hout=Hi, Wout=Wi, ostep=2, ooy=1, oox=1)
        ops.conv2d([dy.to(dev)], packing.tpack_dgrad_generic(w.to(dev), c0, cs), None, cs, 4, out=out.t, geom=geom)
        want = fill.double().clone()
        want[:, 1::2, 1::2] = ref[:, 1::2, 1::2]
        ref = want
    in_range(t, absref + 2.0)
    torch.cuda.synchronize()
    sentinel(t, "dX", out)
    exact(t, "dX", out.t, ref)


# the grouped twin launch of backward_pair: both branches' packs in one (2, cs, Kp) buffer, images [B / 2, B) of dy meet the second
@pytest.mark.parametrize("O,I,B,H,W", [(64, 32, 4, 8, 8), (128, 64, 2, 16, 16)])
def test_data_gradient_grouped(dev, O, I, B, H, W):
    from dpmn_amd import ops
    from dpmn_amd.model import packing
    ws, dy, h = [op("tw%d" % g, (O, I, 3, 3)) for g in range(2)], op("tdy", (B, H, W, O)), B // 2
    ref = torch.cat([ref64.conv2d_dgrad(dy[g * h:(g + 1) * h], ws[g], (H, W), 1, 1, 1) for g in range(2)], 0)
    in_range("grouped dgrad", ref64.conv2d_dgrad(dy.abs(), torch.max(ws[0].abs(), ws[1].abs()), (H, W), 1, 1, 1) + 2.0)
    buf = torch.empty(2, I, 9 * O, device=dev)
    for g in range(2):
        packing.tpack_dgrad_conv_s1(ws[g].to(dev), 0, I, out=buf[g])
    out = Buf(dev, ref.shape)
    ops.conv2d([dy.to(dev)], buf, None, I, 3, pad=1, groups=2, out=out.t)
    torch.cuda.synchronize()
    sentinel("grouped dgrad", "dX", out)
    exact("dgrad[grouped O%d I%d]" % (O, I), "dX", out.t, ref)


# ------------------------------------------------------------------------------------------------------------------ packs
# the GPU pack kernels (one dpmn_conv_pack_f32 launch each) bitwise equal to the torch packs of model/packing.py at ragged (Cout, cin, k)
@pytest.mark.parametrize("O,I,k", [(5, 12, 3), (36, 36, 3), (17, 4, 9), (68, 33, 3), (128, 64, 4), (3, 7, 1)])
def test_tpack_equals_pack(dev, O, I, k):
    from dpmn_amd.model import packing as P
    w = u("pkw", (O, I, k, k)).to(dev)
    wt = u("pkwt", (I, O, k, k)).to(dev)
    ip = (I + 3) // 4 * 4
    c0, cs = I // 3, I - I // 3 - 1
    pairs = [("tpack_conv", P.tpack_conv(w), P.pack_conv(w)[0]), ("tpack_conv cin_pad", P.tpack_conv(w, cin_pad=ip), P.pack_conv(w, cin_pad=ip)[0]),
             ("tpack_convT_s1", P.tpack_convT_s1(wt), P.pack_convT_s1(wt)[0]),
             ("tpack_dgrad_conv_s1", P.tpack_dgrad_conv_s1(w, c0, cs), P.pack_convT_s1(w[:, c0:c0 + cs])[0]),
             ("tpack_dgrad_convT", P.tpack_dgrad_convT(wt, c0, cs), P.pack_conv(wt[c0:c0 + cs])[0]),
             ("tpack_dgrad_convT cin_pad", P.tpack_dgrad_convT(wt, c0, cs, cin_pad=O + 4), P.pack_conv(wt[c0:c0 + cs], cin_pad=O + 4)[0]),
             ("tpack_dgrad_generic", P.tpack_dgrad_generic(w, c0, cs), P.pack_bwd_data_generic(w[:, c0:c0 + cs])[0])]
    if k == 4:
        pairs += [("tpack_convT_s2k4", P.tpack_convT_s2k4(wt), torch.stack([p[0] for p in P.pack_convT_s2k4(wt)])),
                  ("tpack_dgrad_conv_s2k4", P.tpack_dgrad_conv_s2k4(w, c0, cs), torch.stack([p[0] for p in P.pack_convT_s2k4(w[:, c0:c0 + cs])]))]
    for name, got, want in pairs:
        assert got.shape == want.shape and torch.equal(got, want), "%s (O %d, I %d, k %d): %d elements differ" % (name, O, I, k, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------------------ negative controls
# valid inputs, wrong answers: the comparison must raise
def test_negative_control_swapped_taps(dev):
    def swap(wp):       # taps 0 and 1 of every output channel (cin = 32 columns each)
        wp = wp.clone()
        wp[:, :32], wp[:, 32:64] = wp[:, 32:64].clone(), wp[:, :32].clone()
        return wp
    with pytest.raises(AssertionError, match="differ from the exactly representable"):
        fwd(dev, "control[swapped taps]", (32,), 36, 3, 2, 9, 7, mutate=swap)


def test_negative_control_wgrad_last_pixel(dev):
    def bump(dy):
        dy = dy.clone()
        dy[-1, -1, -1] += 2.0 ** -5
        return dy
    with pytest.raises(AssertionError, match="differ from the exactly representable"):
        wgrad(dev, "control[dy last pixel]", (32,), 36, 3, 3, 5, 7, modes=("excl",), mutate=bump)


def test_negative_control_phase_order(dev):
    from dpmn_amd.model import packing
    xs, wt, b, af, ref = _ct_case((32,), 36, 2, 5, 7, "none", (0,))
    wp4 = packing.tpack_convT_s2k4(wt.to(dev))[[1, 0, 2, 3]].contiguous()
    out = Buf(dev, (2, 10, 14, 36))
    _ct_launch(dev, [xs[0].to(dev)], wp4, b.to(dev), 36, out.t, "none", None)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="differ from the exactly representable"):
        exact("control[phase order]", "out", out.t, ref)
