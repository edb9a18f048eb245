"""GPU parity of the three small forward kernels that were restructured for memory-level parallelism -- the streaming 32 x 32 form of the Mlp
depthwise 3 x 3 (k_dwconv_gelu_r32, csrc/pgrm.hip) next to the band kernel of every other plane size, the SK gate (k_sk_gate) and the patch
embedding with its token rows stored through a wave-private LDS tile (k_patch_embed_ln) -- each called on its own.

Reference: a float64 restatement in torch on the CPU, built here (F.conv2d, F.layer_norm, F.gelu(approximate='none'), softmax).
Criterion (the precedent of tests/test_gpu_x3.py): the kernel's max error against float64 may not exceed TWICE the error the kernel
of the parent commit had on the same inputs -- nothing but reordering noise.  The parent's figures are in
profiles/r16a_small_kernel_floors_parent.json, written once by tools/record_small_kernel_floors.py with the parent's library; a case
missing from that file fails.  All three kernels keep every output's chain of operations, so their outputs are also required to be bitwise
those of the parent (the SHA-256 of the output bytes, recorded in the same file): no r = 32 fallback is left to call side by side.

Shapes: B in {1, 3} x Ch in {1, 5, 384} (plane counts 1 ... 1152: one wave, a partial block, many blocks -- at r = 32 every wave of the
streaming kernel still has ONE plane there) x r in {4, 8, 32, 64} (one float4 per row, whole planes, the streaming kernel, 16-row bands),
with and without the input GELU, p_drop in {0, 0.1} with the mask of dpmn_dropout_f32, through every entry point (conv only, GELU,
conv + GELU of the training forward).  The streaming kernel's loop over SEVERAL planes per wave -- the register prefetch, the tile
overwritten by the next commit, the weights and the mask index of the later planes -- needs more planes than the grid has waves
(7 blocks per CU x 4): DW_STREAM_SHAPES, 7173 planes (two per wave, the last wave one) and 2 x 7175 (three per wave, the last two waves two; the
channel wraps inside a wave's walk), asserted against the device's CU count.  SK gate B in {1, 48} x L in {32, 1024} (1 and 32 partials per
image), C = 96, groups = 3.  Patch embed: images 4 x 6 and 32 x 128 x B in {1, 5} (6, 30, 1024 and 5120 tokens: part of a wave, part of a
block, whole blocks), cin = 2 with prior_fusion and cin = 3 without, C in {96, 192}, p_drop in {0, 0.1}."""
import functools
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from dpmn_amd.utils import synth
from helpers import record

pytestmark = pytest.mark.gpu
PARENT_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16a_small_kernel_floors_parent.json")
SEED = 0x5DEECE66D
DW_SHAPES = [(B, Ch, r) for B in (1, 3) for Ch in (1, 5, 384) for r in (4, 8, 32, 64)]
DW_STREAM_SHAPES = [(1, 7173, 32), (2, 7175, 32)]
SK_SHAPES = [(B, L) for B in (1, 48) for L in (32, 1024)]
PE_SHAPES = [(B, H, W, C) for (H, W) in ((4, 6), (32, 128)) for B in (1, 5) for C in (96, 192)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def parent():
    with open(PARENT_JSON) as f:
        return json.load(f)["cases"]


def u(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(name, shape, lo, hi, 81)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def measure(got, ref):
    """(max abs error against float64, SHA-256 of the bytes) of a kernel output"""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all()
    return {"err": float((got.double() - ref).abs().max()), "sha256": sha(got)}


def verify(case, m):
    """m: what measure() returned for `case`; twice the parent's error at most, and the parent's bits"""
    rec = parent().get(case)
    assert rec is not None, "%s: no parent figure in %s" % (case, os.path.basename(PARENT_JSON))
    record(case, "max abs err vs float64 (bound: 2 x parent kernel)", m["err"], 2.0 * rec["err"])
    print("%s: err %.3e, parent %.3e, bitwise %s" % (case, m["err"], rec["err"], m["sha256"] == rec["sha256"]))
    assert m["err"] <= 2.0 * rec["err"], "%s: max err %.3e > 2 x the parent kernel's %.3e" % (case, m["err"], rec["err"])
    assert m["sha256"] == rec["sha256"], "%s: output bits differ from the parent kernel's" % case


# ------------------------------------------------------------------------------------------------------------------ depthwise 3 x 3
@functools.lru_cache(maxsize=None)
def _drop_mask(n, p):
    """the mask of dpmn_dropout_f32: ones through the kernel"""
    from dpmn_amd import ops
    return ops.dropout(torch.ones(n, device="cuda:0"), p, SEED).cpu()


@functools.lru_cache(maxsize=None)
def _dw_inputs(B, Ch, r):
    return u("y", (B, Ch, r, r), -3.0, 3.0), u("dw_w", (Ch, 3, 3), -0.5, 0.5), u("dw_b", (Ch,), -0.5, 0.5)


def _dw_ref(y, w, b, in_gelu, mask):
    """(conv output, GELU of it) in float64; the planes are the raw (B Ch, r, r) view, channel = plane % Ch"""
    x = y.double()
    if in_gelu:
        x = F.gelu(x, approximate="none")
    if mask is not None:
        x = x * mask.double().reshape(x.shape)
    pre = F.conv2d(x, w.double()[:, None], b.double(), padding=1, groups=w.shape[0])
    return pre, F.gelu(pre, approximate="none")


def dw_measure(dev, B, Ch, r):
    """every entry point of the depthwise kernel at one shape -> {case: measure()}"""
    from dpmn_amd._abi import lib, check, dptr, stream
    y, w, b = _dw_inputs(B, Ch, r)
    yd, wd, bd = y.to(dev), w.to(dev), b.to(dev)
    out = {}

    def buf():
        return torch.full((B, Ch, r, r), float("nan"), device=dev)           # an unwritten element shows

    for in_gelu in (0, 1):
        for p in (0.0, 0.1):
            mask = _drop_mask(y.numel(), p) if p > 0 else None
            if mask is not None and y.numel() >= 256:
                assert bool((mask == 0).any()) and bool((mask != 0).any())
            pre_ref, g_ref = _dw_ref(y, w, b, in_gelu, mask)
            case = "dwconv[B%d Ch%d r%d gelu_in%d p%.1f]" % (B, Ch, r, in_gelu, p)
            gpre, g = buf(), buf()
            check(lib.dpmn_dwconv3x3_train_f32(dptr(yd), dptr(wd), dptr(bd), dptr(gpre), dptr(g), in_gelu, p, SEED, B, Ch, r, stream()))
            out[case + " train.pre"], out[case + " train.gelu"] = measure(gpre, pre_ref), measure(g, g_ref)
            if p == 0.0:                                                      # the evaluation entry points have no mask
                ge = buf()
                fn = lib.dpmn_dwconv3x3_gelu_in_f32 if in_gelu else lib.dpmn_dwconv3x3_gelu_f32
                check(fn(dptr(yd), dptr(wd), dptr(bd), dptr(ge), B, Ch, r, stream()))
                out[case + " eval"] = measure(ge, g_ref)
                assert torch.equal(ge, g), case + ": the evaluation and the training entry point disagree"
                if not in_gelu:
                    gc = buf()
                    check(lib.dpmn_dwconv3x3_f32(dptr(yd), dptr(wd), dptr(bd), dptr(gc), B, Ch, r, stream()))
                    out[case + " conv"] = measure(gc, pre_ref)
                    assert torch.equal(gc, gpre), case + ": the plain conv and the training entry point disagree"
    return out


@pytest.mark.parametrize("B,Ch,r", DW_SHAPES)
def test_dwconv3x3_forward(dev, B, Ch, r):
    for case, m in dw_measure(dev, B, Ch, r).items():
        verify(case, m)


@pytest.mark.parametrize("B,Ch,r", DW_STREAM_SHAPES)
def test_dwconv3x3_forward_several_planes_per_wave(dev, B, Ch, r):
    waves = 7 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    per = -(-B * Ch // waves)
    assert r == 32 and per >= 2 and (B * Ch) % per != 0, "%d planes on %d waves: the shape no longer reaches the uneven multi-plane walk" % (B * Ch, waves)
    for case, m in dw_measure(dev, B, Ch, r).items():
        verify(case, m)


# ------------------------------------------------------------------------------------------------------------------ SK gate
C_SK, G_SK = 96, 3
DMID = C_SK // G_SK // 2


@functools.lru_cache(maxsize=None)
def _sk_inputs(B, L):
    ppi = (L + 31) // 32
    return (u("partial", (B * ppi, C_SK), -8.0, 24.0), u("sk_fc1_w", (DMID, C_SK), -0.3, 0.3), u("sk_fc1_b", (DMID,), -0.2, 0.2),
            u("sk_fc2_w", (C_SK, DMID), -0.6, 0.6), u("sk_fc2_b", (C_SK,), -0.2, 0.2))


def sk_measure(dev, B, L):
    from dpmn_amd._abi import lib, check, dptr, stream
    ppi = (L + 31) // 32
    partial, w1, b1, w2, b2 = _sk_inputs(B, L)
    S = partial.double().reshape(B, ppi, C_SK).sum(1) / L
    z = F.gelu(S @ w1.double().t() + b1.double(), approximate="none")
    ref = torch.softmax((z @ w2.double().t() + b2.double()).reshape(B, G_SK, C_SK // G_SK), dim=1)
    d = [t.to(dev) for t in (partial, w1, b1, w2, b2)]
    avec = torch.full((B, G_SK, C_SK // G_SK), float("nan"), device=dev)
    check(lib.dpmn_sk_gate_f32(dptr(d[0]), ppi, L, dptr(d[1]), dptr(d[2]), dptr(d[3]), dptr(d[4]), dptr(avec), B, C_SK, G_SK, DMID, stream()))
    return {"sk_gate[B%d L%d]" % (B, L): measure(avec, ref)}


@pytest.mark.parametrize("B,L", SK_SHAPES)
def test_sk_gate(dev, B, L):
    for case, m in sk_measure(dev, B, L).items():
        verify(case, m)


# ------------------------------------------------------------------------------------------------------------------ patch embed
@functools.lru_cache(maxsize=None)
def _pe_weights(C):
    return (u("pe_w", (C, 3, 2, 2), -0.5, 0.5), u("pe_b", (C,), -0.2, 0.2), u("pe_ln_w", (C,), 0.5, 1.5), u("pe_ln_b", (C,), -0.5, 0.5),
            u("pf_w", (3, 2, 3, 3), -0.4, 0.4), u("pf_b", (3,), -0.2, 0.2))


def pe_measure(dev, B, H, W, C):
    """prior_fusion (2-channel prior) and plain (3-channel image) patch embedding + LayerNorm, without and with pos_drop -> {case: measure()}"""
    from dpmn_amd import ops
    pw, pb, nw, nb, fw, fb = _pe_weights(C)
    d = [t.to(dev) for t in (pw, pb, nw, nb, fw, fb)]
    out = {}
    for fuse in (0, 1):
        img = u("pe_img%d" % fuse, (B, 2 if fuse else 3, H, W), -1.0, 1.0)
        x = img.double()
        if fuse:
            x = F.conv2d(x, fw.double(), fb.double(), padding=1)
        t = F.conv2d(x, pw.double(), pb.double(), stride=2).flatten(2).transpose(1, 2)
        ref0 = F.layer_norm(t, (C,), nw.double(), nb.double(), 1e-5)
        for p in (0.0, 0.1):
            ref = ref0 * _drop_mask(ref0.numel(), p).double().reshape(ref0.shape) if p > 0 else ref0
            got = ops.patch_embed_ln(img.to(dev), d[0], d[1], d[2], d[3], 2, *((d[4], d[5]) if fuse else ()), p_drop=p, seed=SEED)
            out["patch_embed[B%d %dx%d C%d fuse%d p%.1f]" % (B, H, W, C, fuse, p)] = measure(got, ref)
    return out


@pytest.mark.parametrize("B,H,W,C", PE_SHAPES)
def test_patch_embed_ln(dev, B, H, W, C):
    for case, m in pe_measure(dev, B, H, W, C).items():
        verify(case, m)
