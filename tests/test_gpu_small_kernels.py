"""GPU parity of the small hand-written kernels around the PSN backbones, the CMM gate and the recogniser front ends -- k_bigru,
k_encoder_layer, k_cross_attn, k_add_layernorm64, k_gru_gate, k_tl_interp (csrc/tatt.hip), k_mha<32|64>, k_ln_std (tbsrn.hip),
dpmn_layernorm_f32, k_se_fc1 / k_se_fc2_apply (cmm.hip), k_maxpool_nhwc (stn.hip) -- each called on its own against its float64
reference (tests/ref64.py, pinned by tests/test_ref64.py) at the smallest shapes that cross its hand-written boundaries: leftover steps,
partial blocks and waves, null optional pointers, the LMAX / SMAX limits, one and several key tiles.

Tolerances.  tatt.hip / tbsrn.hip kernels: the project's ATOL = RTOL = 1e-4 (1e-5 / 1e-4 for attention weights) of tests/test_gpu_psn.py.
gru_gate, layernorm, se_gate, mha64: the same operation is also evaluated in fp32 torch on the CPU and the kernel is allowed 8 x that
result's max error against float64 (another summation order plus hardware exp / rcp), floor 1e-6.  tl_interp: 1e-4 / 1e-4 (its source
coordinate is one fp32 multiply).  The affine max-pool: 1e-6 absolute on values of magnitude <= 4 (it differs from fp32 torch by one
rounding, whether v * s + t is contracted to an fma).  Every achieved error goes through helpers.record."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import ref64
from dpmn_amd.utils import synth
from helpers import record

pytestmark = pytest.mark.gpu
ATOL, RTOL = 1e-4, 1e-4          # tests/test_gpu_psn.py
SENT = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=80):
    return synth.uniform(name, shape, lo, hi, seed)


def err64(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max()) if ref.numel() else 0.0


def check_fixed(test, what, got, ref, atol=ATOL, rtol=RTOL):
    """|got - ref| <= atol + rtol |ref| elementwise against the float64 reference; the achieved max error is recorded first"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, "%s %s: shape %s vs %s" % (test, what, tuple(got.shape), tuple(ref.shape))
    e = (got - ref).abs()
    record(test, what + ": max abs err vs float64", float(e.max()), atol)
    assert torch.isfinite(got).all(), "%s %s: non-finite output" % (test, what)
    bad = e > atol + rtol * ref.abs()
    assert not bad.any(), "%s %s: max err %.3e at %d / %d elements (atol %.0e rtol %.0e)" % (test, what, float(e.max()), int(bad.sum()), e.numel(), atol, rtol)


def check_derived(test, what, got, ref, cpu32, floor=1e-6):
    """max |got - ref| <= max(8 x max |fp32 CPU torch - ref|, floor)"""
    assert cpu32.dtype == torch.float32 and got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) == tuple(cpu32.shape)
    e32, e = err64(cpu32, ref), err64(got, ref)
    bound = max(8.0 * e32, floor)
    record(test, what + ": fp32 CPU max abs err vs float64", e32)
    record(test, what + ": GPU max abs err vs float64", e, bound)
    assert torch.isfinite(got).all(), "%s %s: non-finite output" % (test, what)
    assert e <= bound, "%s %s: GPU max err %.3e > %.3e = max(8 x fp32 CPU err %.3e, %.0e)" % (test, what, e, bound, e32, floor)


# ------------------------------------------------------------------------------------------------------------------ bigru
@functools.lru_cache(maxsize=None)
def _bigru_case(axis, B, H, W, gain):
    gi = u("gi", (B, H, W, 192), -2.0, 2.0) * gain
    whh, bhh, res = u("whh", (2, 96, 32), -0.4, 0.4), u("bhh", (2, 96), -0.2, 0.2), u("res", (B, H, W, 64))
    return gi, whh, bhh, res, ref64.bigru(gi, whh, bhh, None, axis)


def _bigru_raw(gi, whh, bhh, res, out, axis):
    """dpmn_bigru_f32 into a caller-owned `out` (the geometry of ops.bigru)"""
    from dpmn_amd._abi import lib, check, dptr, stream
    B, H, W, _ = gi.shape
    if axis == "w":
        nseq, T, inner, outer, inner_s, step = B * H, W, 1, W, 0, 1
    else:
        nseq, T, inner, outer, inner_s, step = B * W, H, W, H * W, 1, W
    check(lib.dpmn_bigru_f32(dptr(gi), dptr(whh), dptr(bhh), dptr(res, True), dptr(out), nseq, T, inner, outer, inner_s, step, 32, stream()))
    return out


def _bigru_run(dev, test, axis, B, H, W, gain=1.0):
    from dpmn_amd import ops
    gi, whh, bhh, res, ref = _bigru_case(axis, B, H, W, gain)
    gid, whd, bhd, resd = gi.to(dev), whh.to(dev), bhh.to(dev), res.to(dev)
    # an unwritten step shows even where stale memory would have held plausible values
    raw = _bigru_raw(gid, whd, bhd, None, torch.full((B, H, W, 64), float("nan"), device=dev), axis)
    assert not torch.isnan(raw).any(), "%s: %d outputs never written" % (test, int(torch.isnan(raw).sum()))
    check_fixed(test, "res=None into a NaN-filled out", raw, ref)
    check_fixed(test, "res=None", ops.bigru(gid, whd, bhd, B, H, W, axis), ref)
    check_fixed(test, "with residual", ops.bigru(gid, whd, bhd, B, H, W, axis, res=resd), ref + res.double())


# nseq = 1, 5, 7 (a partial block of four waves, with and without a whole one) x every T % 4, T < 4 (the prefetch ring re-reads the
# last step) and the workload's T = 64
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7, 9, 64])
@pytest.mark.parametrize("axis,B,R", [("w", 1, 1), ("w", 1, 5), ("w", 7, 1), ("h", 1, 5), ("h", 7, 1)])
def test_bigru(dev, axis, B, R, T):
    H, W = (R, T) if axis == "w" else (T, R)
    _bigru_run(dev, "bigru[%s B%d R%d T%d]" % (axis, B, R, T), axis, B, H, W)


def test_bigru_saturated_gates(dev):
    """gi x 40: most gate pre-activations beyond |30|, where exp(-x) overflows to inf / underflows to 0 inside sigmoid_fast / tanh_fast"""
    gi = _bigru_case("w", 1, 5, 9, 40.0)[0]
    assert 0.3 < float((gi.abs() > 30).float().mean()) < 0.9
    _bigru_run(dev, "bigru[saturated]", "w", 1, 5, 9, 40.0)


# ------------------------------------------------------------------------------------------------------------------ encoder layer
def _enc_weights():
    E = 64
    return [u("in_w", (3 * E, E), -0.2, 0.2), u("in_b", (3 * E,), -0.1, 0.1), u("out_w", (E, E), -0.2, 0.2), u("out_b", (E,), -0.1, 0.1),
            u("l1_w", (E, E), -0.2, 0.2), u("l1_b", (E,), -0.1, 0.1), u("l2_w", (E, E), -0.2, 0.2), u("l2_b", (E,), -0.1, 0.1),
            u("n1_w", (E,), 0.5, 1.5), u("n1_b", (E,), -0.5, 0.5), u("n2_w", (E,), 0.5, 1.5), u("n2_b", (E,), -0.5, 0.5)]


@pytest.mark.parametrize("N,L", [(1, 1), (3, 5), (2, 26), (2, 32)])
def test_tatt_encoder_layer(dev, N, L):
    from dpmn_amd import ops, _abi
    from dpmn_amd._abi import lib, check, dptr, stream
    test = "encoder_layer[N%d L%d]" % (N, L)
    w = _enc_weights()
    src, pos = u("src", (N, L, 64)), u("pos", (L, 64))
    ref = ref64.encoder_layer(src, pos, w)
    wd = [t.to(dev) for t in w]
    srcd, posd = src.to(dev), pos.to(dev)
    check_fixed(test, "ops", ops.tatt_encoder_layer(srcd, posd, wd), ref)
    mem = torch.full((N * L + 1, 64), SENT, device=dev)      # one row past the output: must stay untouched
    check(lib.dpmn_tatt_encoder_layer_f32(dptr(srcd), dptr(posd), _abi.ptr_array(wd), dptr(mem), N, L, 64, 4, stream()))
    assert bool((mem[-1] == SENT).all()), "%s: wrote past the N * L output rows" % test
    check_fixed(test, "into a sentinel-filled mem", mem[:-1].reshape(N, L, 64), ref)


# ------------------------------------------------------------------------------------------------------------------ cross attention
@pytest.mark.parametrize("need_weights", [False, True])
@pytest.mark.parametrize("N,L,S", [(1, 1, 1), (2, 63, 7), (2, 257, 26), (1, 300, 32), (1, 512, 32)])
def test_cross_attn(dev, N, L, S, need_weights):
    from dpmn_amd import ops
    test = "cross_attn[N%d L%d S%d%s]" % (N, L, S, " pw" if need_weights else "")
    q, k, v = u("q", (N, L, 64), -2, 2), u("k", (N, S, 64), -2, 2), u("v", (N, S, 64))
    ref_o, ref_w = ref64.cross_attn(q, k, v)
    o, pw = ops.cross_attn(q.to(dev), k.to(dev), v.to(dev), need_weights=need_weights)
    check_fixed(test, "out", o, ref_o)
    if not need_weights:
        assert pw is None
        return
    check_fixed(test, "weights", pw, ref_w, 1e-5, 1e-4)
    rows = float((pw.double().sum(-1) - 1.0).abs().max())
    record(test, "max |row sum of the weights - 1|", rows, 1e-5)
    assert rows <= 1e-5


@pytest.mark.parametrize("s0", [0, 25])
def test_cross_attn_dominant_key(dev, s0):
    """one key more than 50 above every other score in every head: the output is that key's value, the weights are one-hot"""
    from dpmn_amd import ops
    test = "cross_attn[dominant key %d]" % s0
    N, L, S = 2, 70, 26
    q_dir = torch.where(u("qdir", (64,)) > 0, 1.5, -1.5)
    q = q_dir + u("qn", (N, L, 64), -0.1, 0.1)
    k, v = u("k", (N, S, 64)), u("v", (N, S, 64))
    k[:, s0] = 8.0 * q_dir
    sc = (q.double().reshape(N, L, 4, 16).permute(0, 2, 1, 3) @ k.double().reshape(N, S, 4, 16).permute(0, 2, 3, 1)) / 4.0
    gap = sc[..., s0] - torch.cat([sc[..., :s0], sc[..., s0 + 1:]], -1).amax(-1)
    assert float(gap.min()) > 50.0
    ref_o, ref_w = ref64.cross_attn(q, k, v)
    o, pw = ops.cross_attn(q.to(dev), k.to(dev), v.to(dev), need_weights=True)
    check_fixed(test, "out", o, ref_o)
    check_fixed(test, "weights", pw, ref_w, 1e-5, 1e-4)
    check_fixed(test, "out vs the dominant key's value", o, v[:, s0:s0 + 1].expand(N, L, 64).double())
    onehot = torch.zeros(N, L, S, dtype=torch.float64)
    onehot[:, :, s0] = 1.0
    check_fixed(test, "weights vs one-hot", pw, onehot, 1e-5, 1e-4)


# ------------------------------------------------------------------------------------------------------------------ add + LayerNorm
def _aln_params():
    return u("g1", (64,), 0.5, 1.5), u("b1", (64,)), u("g2", (64,), 0.5, 1.5), u("b2", (64,))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 301])
def test_add_layernorm64(dev, M, with_res):
    from dpmn_amd import ops
    test = "add_layernorm64[M%d%s]" % (M, " res" if with_res else "")
    x, r, acc0 = u("x", (M, 64), -2, 2), (u("r", (M, 64), -2, 2) if with_res else None), u("acc", (M, 64))
    g1, b1, g2, b2 = _aln_params()
    xd, rd = x.to(dev), (r.to(dev) if with_res else None)
    pd = [t.to(dev) for t in (g1, b1, g2, b2)]
    ref_y, _ = ref64.add_layernorm64(x, r, g1, b1)
    check_fixed(test, "no acc_out", ops.add_layernorm64(xd, rd, pd[0], pd[1]), ref_y)
    _, ref_acc = ref64.add_layernorm64(x, r, g1, b1, g2, b2, acc0, 0.5, True)
    accd = acc0.to(dev)
    check_fixed(test, "accumulate: y", ops.add_layernorm64(xd, rd, *pd, accd, alpha=0.5, accumulate=True), ref_y)
    check_fixed(test, "accumulate: acc_out", accd, ref_acc)
    # accumulate=False overwrites whatever acc_out holds
    _, ref_set = ref64.add_layernorm64(x, r, g1, b1, g2, b2, None, 0.5, False)
    accd = torch.full((M, 64), float("nan"), device=dev)
    check_fixed(test, "overwrite: y", ops.add_layernorm64(xd, rd, *pd, accd, alpha=0.5, accumulate=False), ref_y)
    assert torch.isfinite(accd).all(), "%s: accumulate=False read the previous acc_out" % test
    check_fixed(test, "overwrite: NaN-filled acc_out", accd, ref_set)


@pytest.mark.parametrize("with_res", [False, True])
def test_add_layernorm64_constant_rows(dev, with_res):
    """rows of one repeated value: the butterfly sum of 64 equal floats is a chain of exact doublings, so the centred value is exactly 0
    (fp32 and float64 alike) and y is exactly b -- a well-conditioned edge"""
    from dpmn_amd import ops
    test = "add_layernorm64[constant rows%s]" % (" res" if with_res else "")
    M = 6
    x = torch.full((M, 64), 0.5 if with_res else 0.7)
    r = torch.full((M, 64), 0.2) if with_res else None
    g1, b1, g2, b2 = _aln_params()
    pd = [t.to(dev) for t in (g1, b1, g2, b2)]
    accd = torch.full((M, 64), float("nan"), device=dev)
    y = ops.add_layernorm64(x.to(dev), None if r is None else r.to(dev), *pd, accd, alpha=1.0, accumulate=False)
    assert torch.equal(y.cpu(), b1.expand(M, 64)), "%s: y differs from b by up to %.3e" % (test, float((y.cpu() - b1).abs().max()))
    ref_y, ref_acc = ref64.add_layernorm64(x, r, g1, b1, g2, b2, None, 1.0, False)
    check_fixed(test, "y", y, ref_y)
    check_fixed(test, "acc_out", accd, ref_acc)


# ------------------------------------------------------------------------------------------------------------------ GRU gate step
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("R,H", [(1, 1), (3, 64), (26, 64), (130, 32)])
def test_gru_gate(dev, R, H, wide):
    from dpmn_amd import ops
    stride = 2 * H + 3 if wide else H
    test = "gru_gate[R%d H%d stride %d]" % (R, H, stride)
    gi, gh, h = u("gi", (R, 3 * H), -3, 3), u("gh", (R, 3 * H), -3, 3), u("h", (R, H))
    ref = ref64.gru_gate(gi, gh, h)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    cpu32 = (1.0 - z) * torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]) + z * h
    hd = h.to(dev)
    hist = torch.full((R, stride), SENT, device=dev)
    ops.gru_gate(gi.to(dev), gh.to(dev), hd, hist, stride)
    check_derived(test, "h", hd, ref, cpu32)
    assert torch.equal(hist[:, :H], hd), "%s: hist differs from the updated h" % test
    assert bool((hist[:, H:] == SENT).all()), "%s: wrote outside columns [0, H) of hist" % test


# ------------------------------------------------------------------------------------------------------------------ tl_interp
@pytest.mark.parametrize("N,Win,C,H,W", [(1, 1, 4, 1, 1), (2, 1, 8, 2, 5), (2, 26, 32, 3, 1), (1, 26, 64, 2, 64), (2, 7, 4, 1, 7), (1, 5, 8, 2, 9)])
def test_tl_interp(dev, N, Win, C, H, W):
    from dpmn_amd._abi import lib, check, dptr, stream
    test = "tl_interp[N%d Win%d C%d H%d W%d]" % (N, Win, C, H, W)
    inp = u("tl", (N, Win, C))
    inpd, out = inp.to(dev), torch.full((N, H, W, C), float("nan"), device=dev)
    check(lib.dpmn_tl_interp_f32(dptr(inpd), dptr(out), N, Win, C, H, W, stream()))
    check_fixed(test, "out", out, ref64.tl_interp(inp, H, W), 1e-4, 1e-4)
    assert torch.equal(out, out[:, :1].expand(N, H, W, C)), "%s: an output row differs from row 0" % test


# ------------------------------------------------------------------------------------------------------------------ mha32 / mha64
def _mha_cpu32(qkv, B, L, heads, d):
    q, k, v = (qkv[:, i * heads * d:(i + 1) * heads * d].reshape(B, L, heads, d).transpose(1, 2) for i in range(3))
    return (torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(d), -1) @ v).transpose(1, 2).reshape(B * L, heads * d)


def _mha_check(dev, test, qkv, B, L, heads, d):
    from dpmn_amd import ops
    ref = ref64.mha(qkv, B, L, heads, d)
    got = (ops.mha32 if d == 32 else ops.mha64)(qkv.to(dev), B, L, heads, 1.0 / math.sqrt(d))
    if d == 32:
        check_fixed(test, "out", got, ref)
    else:
        check_derived(test, "out", got, ref, _mha_cpu32(qkv, B, L, heads, d))
    return got, ref


# L = 64: one key tile (the online-softmax correction must be a no-op); 128, 256, 320: 2, 4, 5 tiles; 1, 3, 4, 8 heads
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("B,L,heads", [(1, 64, 1), (2, 128, 3), (1, 320, 4), (1, 256, 8)])
def test_mha(dev, B, L, heads, d):
    _mha_check(dev, "mha%d[B%d L%d heads %d]" % (d, B, L, heads), u("qkv", (B * L, 3 * heads * d), -2.0, 2.0), B, L, heads, d)


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("pos", [3, 317])
def test_mha_planted_key(dev, pos, d):
    """a key more than 50 above every other score, in the first key tile (the running max is set early and never replaced) and in the
    last one (everything accumulated before it is rescaled away on the final tile): the output is that key's value"""
    B, L, heads = 1, 320, 2
    test = "mha%d[planted key %d]" % (d, pos)
    qkv = u("qkv", (B * L, 3, heads, d), -2.0, 2.0)
    q_dir = torch.where(u("qdir", (heads, d)) > 0, 1.5, -1.5)
    qkv[:, 0] = q_dir + u("qn", (B * L, heads, d), -0.1, 0.1)
    qkv[pos, 1] = 8.0 * q_dir
    qkv = qkv.reshape(B * L, 3 * heads * d)
    sc = torch.einsum("lhd,shd->hls", qkv[:, :heads * d].double().reshape(L, heads, d), qkv[:, heads * d:2 * heads * d].double().reshape(L, heads, d)) / math.sqrt(d)
    gap = sc[..., pos] - torch.cat([sc[..., :pos], sc[..., pos + 1:]], -1).amax(-1)
    assert float(gap.min()) > 50.0
    got, ref = _mha_check(dev, test, qkv, B, L, heads, d)
    vrow = qkv[pos, 2 * heads * d:].double().expand(B * L, heads * d)
    assert err64(ref, vrow) < 1e-12
    e = err64(got, vrow)
    record(test, "max abs err vs the planted key's value", e, 1e-6)
    assert e <= 1e-6      # (softmax weight 1 up to e^-50: what is left is the rounding of v / l_run, |v| <= 2)


# ------------------------------------------------------------------------------------------------------------------ LayerNorms
@pytest.mark.parametrize("M", [1, 5, 777])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_layernorm_std(dev, C, M):
    from dpmn_amd import ops
    x, a2, b2 = u("lns_x", (M, C), -3, 3), u("lns_a", (C,), 0.5, 1.5), u("lns_b", (C,))
    check_fixed("layernorm_std[C%d M%d]" % (C, M), "out", ops.layernorm_std(x.to(dev), a2.to(dev), b2.to(dev), 1e-6), ref64.layernorm_std(x, a2, b2, 1e-6))


@pytest.mark.parametrize("M", [1, 5, 301])
@pytest.mark.parametrize("C", [64, 96, 192, 512])
def test_layernorm(dev, C, M):
    from dpmn_amd import ops
    x, w, b = u("ln_x", (M, C), -3, 3), u("ln_w", (C,), 0.5, 1.5), u("ln_b", (C,))
    check_derived("layernorm[C%d M%d]" % (C, M), "out", ops.layernorm(x.to(dev), w.to(dev), b.to(dev), 1e-5), ref64.layernorm(x, w, b, 1e-5),
                  F.layer_norm(x, (C,), w, b, 1e-5))


@pytest.mark.parametrize("which", ["layernorm", "layernorm_std"])
def test_layernorm_unsupported_width_is_an_error(dev, which):
    """C = 80 has no kernel: DpmnError, and nothing is launched (a caller-owned output keeps its sentinel)"""
    from dpmn_amd import ops
    from dpmn_amd._abi import DpmnError, lib, dptr, stream
    x, w, b = u("x80", (5, 80)).to(dev), u("w80", (80,)).to(dev), u("b80", (80,)).to(dev)
    with pytest.raises(DpmnError):
        getattr(ops, which)(x, w, b, 1e-5)
    y = torch.full((5, 80), SENT, device=dev)
    rc = getattr(lib, "dpmn_%s_f32" % which)(dptr(x), dptr(w), dptr(b), 1e-5, dptr(y), 5, 80, stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((y == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ CMM channel gate
# Cmid % 16 != 0 and Cmid < 16 (the early exit of the four-units-per-wave loop), P = 1 and 64 (lane < P), C below / not a multiple of 64
@pytest.mark.parametrize("B,P,C,Cmid", [(1, 1, 16, 4), (3, 4, 128, 20), (2, 64, 96, 36), (2, 4, 1024, 256)])
def test_se_gate(dev, B, P, C, Cmid):
    from dpmn_amd import ops
    x = u("se_x", (B, 1, P, C), -2, 2)
    w1, b1, w2, b2 = u("se_w1", (Cmid, C), -0.3, 0.3), u("se_b1", (Cmid,)), u("se_w2", (C, Cmid), -0.3, 0.3), u("se_b2", (C,))
    gate = torch.sigmoid(F.linear(F.relu(F.linear(x.mean((1, 2)), w1, b1)), w2, b2))
    cpu32 = x * gate[:, None, None, :] + x
    got = ops.se_gate(x.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev))
    check_derived("se_gate[B%d P%d C%d Cmid%d]" % (B, P, C, Cmid), "out", got, ref64.se_gate(x, w1, b1, w2, b2), cpu32)


# ------------------------------------------------------------------------------------------------------------------ max-pool (+ affine + ReLU)
@pytest.mark.parametrize("B,H,W,C,kh,kw", [(1, 2, 2, 4, 2, 2), (2, 4, 6, 8, 2, 3), (2, 6, 4, 12, 1, 2)])
def test_maxpool_affine(dev, B, H, W, C, kh, kw):
    from dpmn_amd import ops
    test = "maxpool[B%d %dx%d C%d k%dx%d]" % (B, H, W, C, kh, kw)
    x = u("mp_x", (B, H, W, C), -2, 2)
    plain = ops.maxpool(x.to(dev), kh, kw)
    assert torch.equal(plain.cpu(), F.max_pool2d(x.permute(0, 3, 1, 2), (kh, kw)).permute(0, 2, 3, 1)), "%s: scale=None is not bit-equal to max_pool2d" % test
    # about half the scales negative: there "max, then affine" is not "affine + ReLU, then max"; |x s + t| <= 4
    s, t = u("mp_s", (C,), -1.5, 1.5), u("mp_t", (C,))
    s[::2] = -s[::2].abs()
    s[1::2] = s[1::2].abs()
    ref = ref64.maxpool_affine_relu(x, kh, kw, s, t)
    cpu32 = F.max_pool2d(F.relu(x * s + t).permute(0, 3, 1, 2), (kh, kw)).permute(0, 2, 3, 1)
    got = ops.maxpool(x.to(dev), kh, kw, s.to(dev), t.to(dev))
    e32, e = err64(cpu32, ref), err64(got, ref)
    record(test, "affine: fp32 CPU max abs err vs float64", e32)
    record(test, "affine: GPU max abs err vs float64", e, 1e-6)
    assert tuple(got.shape) == tuple(ref.shape) and e <= 1e-6, "%s: max err %.3e" % (test, e)
