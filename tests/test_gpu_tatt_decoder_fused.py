"""GPU parity of the two fused kernels of the TATT text-prior decoder (csrc/tatt.hip) and of the interpreter that calls them:

  * dpmn_tatt_dec_tail_f32 (k_tatt_dec_tail): out_proj + residual -> norm2 -> linear1 + ReLU -> linear2 + residual -> norm3 (-> decoder.norm,
    scaled into acc_out) in one launch, against the five launches it replaces, called through their own C ABI entry points
    (dpmn_linear_f32, dpmn_add_layernorm64_f32) on the same inputs;
  * dpmn_cross_attn_qproj_f32 (k_cross_attn_qproj): the q projection inside the attention launch, against dpmn_add_linear_f32 followed by
    dpmn_cross_attn_f32;
  * dpmn_tatt_interpreter_f32 at B = 2, against the unfused chain composed from the entry points (the host mirror's non-native path,
    dpmn_amd/model/tatt.py).

Reference: a float64 restatement written here in torch on the CPU (matmul, mean, sqrt, exp, clamp -- no torch.nn call).  Criterion (the
rule of tests/test_gpu_small_kernel_floors.py): the fused kernel's max error against float64 may not exceed TWICE the error the unfused chain
has against float64 on the same case and output.  The chain's error is measured in the test, never fixed in advance; both run in the
compute mode of the pass (the fused kernels are plain fp32 in every mode, the chain's K = 64 products take the bf16x3 form in mode 2).
Outputs are allocated as NaN, so an unwritten element fails the finiteness check.

Shapes of the tail (rows M of 64 floats; a wave owns a 16-row tile, four waves a block): 16 (one tile), 17 and 31 (ragged last tile, clamped
rows), 16 * 4 * 3 + 5 = 197 (several tiles, several blocks and a tail), 1024 (one image), and 16 * 1024 * 3 + 5 = 49157, the smallest class of
size at which the launcher gives a wave SEVERAL tiles (more tiles than two blocks per CU have waves: asserted against the device's CU
count), so that the prefetch of the next tile's rows, residual and acc_out rows is exercised.  Every output mode at every shape: without the
second norm, and with it for accumulate in {0, 1} x alpha in {1, 0.5}.  Attention: N in {1, 2} x L in {256, 300} (whole query blocks, a
ragged one whose last three waves have no row) x S in {26, 32, 1}, with and without the head-averaged weights.  Interpreter: B = 2, L = 300,
S = 26, three decoder layers (first write, accumulate, both ping-pong buffers) with the attention weights of the last layer; the f64
reference of the decoder starts from the encoder output `mem` that both paths compute with the same launches."""
import ctypes as C
import functools
import math

import pytest
import torch

from dpmn_amd.utils import synth
from helpers import record

pytestmark = pytest.mark.gpu
E = 64
TAIL_M = [16, 17, 31, 16 * 4 * 3 + 5, 1024, 16 * 1024 * 3 + 5]
TAIL_MODES = [(False, 0, 1.0), (True, 0, 1.0), (True, 0, 0.5), (True, 1, 1.0), (True, 1, 0.5)]      # (second norm, accumulate, alpha)
ATTN_SHAPES = [(N, L, S) for N in (1, 2) for L in (256, 300) for S in (26, 32, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(name, shape, lo, hi, 97)


def d64(t):
    return t.detach().cpu().double()


def ln64(x, g, b):
    c = x - x.mean(-1, keepdim=True)
    return c / torch.sqrt((c * c).mean(-1, keepdim=True) + 1e-5) * d64(g) + d64(b)


def lin64(x, w, b):
    return x @ d64(w).t() + d64(b)


def err(got, ref):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all()
    return float((got.double() - ref).abs().max())


def verify(case, e_fused, e_chain):
    record(case, "max abs err vs float64 (bound: 2 x unfused chain)", e_fused, 2.0 * e_chain)
    print("%s: fused %.3e, unfused chain %.3e" % (case, e_fused, e_chain))
    assert e_fused <= 2.0 * e_chain, "%s: max err %.3e > 2 x the unfused chain's %.3e" % (case, e_fused, e_chain)


def nan_like(t):
    return torch.full_like(t, float("nan"))


# ------------------------------------------------------------------------------------------------------------------ decoder layer weights
LAYER_NAMES = ("wq", "bq", "wk", "bk", "wv", "bv", "out_w", "out_b", "norm2_w", "norm2_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
               "norm3_w", "norm3_b")


@functools.lru_cache(maxsize=None)
def layer_params(tag):
    """one decoder layer's parameters on the CPU: weights at the 1 / sqrt(E) scale of nn.Linear's init, norm gains around 1"""
    p = {}
    for n in LAYER_NAMES:
        if n.startswith("norm"):
            p[n] = u(tag + n, (E,), 0.5, 1.5) if n.endswith("_w") else u(tag + n, (E,), -0.2, 0.2)
        elif n.startswith("b") or n.endswith("_b"):
            p[n] = u(tag + n, (E,), -0.125, 0.125)
        else:
            p[n] = u(tag + n, (E, E), -0.125, 0.125)
    return p


@functools.lru_cache(maxsize=None)
def dec_norm():
    return u("dn_w", (E,), 0.5, 1.5), u("dn_b", (E,), -0.2, 0.2)


def to_dev(p, dev):
    return {k: v.to(dev) for k, v in p.items()}


def tail_fused(o, res, p, g2, b2, acc, alpha, accumulate):
    """-> (y, acc_out or None); acc is overwritten when given"""
    from dpmn_amd import ops
    y = ops.tatt_dec_tail(o, res, p["out_w"], p["out_b"], p["norm2_w"], p["norm2_b"], p["lin1_w"], p["lin1_b"], p["lin2_w"], p["lin2_b"],
                          p["norm3_w"], p["norm3_b"], g2, b2, acc, alpha, accumulate)
    return y, acc


def tail_chain(o, res, p, g2, b2, acc, alpha, accumulate):
    from dpmn_amd import ops
    t1 = ops.linear(o, p["out_w"], p["out_b"], res1=res)
    o1 = ops.add_layernorm64(t1, None, p["norm2_w"], p["norm2_b"])
    f = ops.linear(o1, p["lin1_w"], p["lin1_b"], act="relu")
    t2 = ops.linear(f, p["lin2_w"], p["lin2_b"], res1=o1)
    y = ops.add_layernorm64(t2, None, p["norm3_w"], p["norm3_b"], g2, b2, acc, alpha, accumulate)
    return y, acc


def tail_ref(o, res, p, g2, b2, acc, alpha, accumulate):
    o1 = ln64(lin64(d64(o), p["out_w"], p["out_b"]) + d64(res), p["norm2_w"], p["norm2_b"])
    f = torch.clamp(lin64(o1, p["lin1_w"], p["lin1_b"]), min=0.0)
    y = ln64(lin64(f, p["lin2_w"], p["lin2_b"]) + o1, p["norm3_w"], p["norm3_b"])
    if g2 is None:
        return y, None
    a = alpha * ln64(y, g2, b2)
    return y, (d64(acc) + a if accumulate else a)


@functools.lru_cache(maxsize=None)
def tail_inputs(M):
    return u("o%d" % M, (M, E)), u("res%d" % M, (M, E)), u("acc%d" % M, (M, E))


@pytest.mark.parametrize("M", TAIL_M)
def test_dec_tail_vs_unfused_chain(dev, M):
    from dpmn_amd._abi import lib
    if M > 16 * 1024:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert (M + 15) // 16 > 2 * cus * 4, "M = %d gives no wave a second tile on %d CUs" % (M, cus)
    assert lib.dpmn_get_compute_dtype() in (0, 2)
    o, res, acc0 = tail_inputs(M)
    p = layer_params("t")
    g2, b2 = dec_norm()
    od, resd, pd, g2d, b2d = o.to(dev), res.to(dev), to_dev(p, dev), g2.to(dev), b2.to(dev)
    y_ref = None
    for second, accumulate, alpha in TAIL_MODES:
        case = "dec_tail[M%d norm2nd%d acc%d alpha%.1f]" % (M, second, accumulate, alpha)
        args = (g2, b2, acc0, alpha, accumulate) if second else (None, None, None, 1.0, 0)
        yr, ar = tail_ref(o, res, p, *args)
        y_ref = yr if y_ref is None else y_ref
        outs = []
        for fn in (tail_fused, tail_chain):
            acc = None
            if second:
                acc = acc0.to(dev) if accumulate else torch.full((M, E), float("nan"), device=dev)
            outs.append(fn(od, resd, pd, g2d if second else None, b2d if second else None, acc, alpha, accumulate))
        torch.cuda.synchronize()
        (yf, af), (yc, ac) = outs
        verify(case + " y", err(yf, yr), err(yc, yr))
        if second:
            verify(case + " acc_out", err(af, ar), err(ac, ar))
    # y in the residual's own buffer (every lane reads a row before any lane stores it)
    from dpmn_amd._abi import check, dptr, stream, TattDecLayer
    d = TattDecLayer()
    for n in LAYER_NAMES[6:]:
        setattr(d, n, dptr(pd[n]))
    buf = resd.clone()
    check(lib.dpmn_tatt_dec_tail_f32(dptr(od), dptr(buf), C.byref(d), dptr(buf), None, None, None, 1.0, 0, M, stream()))
    torch.cuda.synchronize()
    assert torch.equal(buf, outs[0][0]), "dec_tail[M%d]: in-place y differs from the out-of-place result" % M


# ------------------------------------------------------------------------------------------------------------------ q projection + attention
def attn_ref(x, qe, wq, bq, k, v, nhead=4):
    """-> (o (N, L, E), head-averaged weights (N, L, S)) in float64"""
    q = lin64(d64(x) + d64(qe), wq, bq)
    N, L, _ = q.shape
    S, dh = k.shape[1], E // nhead
    qh = q.reshape(N, L, nhead, dh).permute(0, 2, 1, 3)
    kh = d64(k).reshape(N, S, nhead, dh).permute(0, 2, 1, 3)
    vh = d64(v).reshape(N, S, nhead, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    pr = e / e.sum(-1, keepdim=True)
    return (pr @ vh).permute(0, 2, 1, 3).reshape(N, L, E), pr.mean(1)


@pytest.mark.parametrize("N,L,S", ATTN_SHAPES)
def test_cross_attn_qproj_vs_add_linear_then_cross_attn(dev, N, L, S):
    from dpmn_amd import ops
    x, qe = u("x%d_%d" % (N, L), (N, L, E)), u("qe%d_%d" % (N, L), (N, L, E))
    k, v = u("k%d_%d" % (N, S), (N, S, E)), u("v%d_%d" % (N, S), (N, S, E))
    p = layer_params("a")
    o_ref, pw_ref = attn_ref(x, qe, p["wq"], p["bq"], k, v)
    xd, qd, kd, vd, wq, bq = (t.to(dev) for t in (x, qe, k, v, p["wq"], p["bq"]))
    for need in (False, True):
        of, pf = ops.cross_attn_qproj(xd, qd, wq, bq, kd, vd, need_weights=need)
        q = ops.add_linear(xd.reshape(N * L, E), qd.reshape(N * L, E), wq, bq).reshape(N, L, E)
        oc, pc = ops.cross_attn(q, kd, vd, need_weights=need)
        torch.cuda.synchronize()
        case = "cross_attn_qproj[N%d L%d S%d pw%d]" % (N, L, S, need)
        verify(case + " o", err(of, o_ref), err(oc, o_ref))
        assert (pf is None) == (not need)
        if need:
            verify(case + " pw", err(pf, pw_ref), err(pc, pw_ref))


# ------------------------------------------------------------------------------------------------------------------ whole interpreter
def test_interpreter_vs_unfused_chain(dev):
    from dpmn_amd import ops, _abi
    from dpmn_amd._abi import lib, check, dptr, stream
    B, L, S, T, n_dec = 2, 300, 26, 37, 3
    x, b1, qe, pos = u("ix", (B * S, T)), u("ib1", (B * L, E)), u("iqe", (B * L, E)), u("ipos", (S, E))
    fc_w, fc_b, slope = u("ifc_w", (E, T), -0.16, 0.16), u("ifc_b", (E,), -0.125, 0.125), 0.25
    enc = [u("ienc%d" % i, s_, lo, hi) for i, (s_, lo, hi) in enumerate(
        [((3 * E, E), -0.125, 0.125), ((3 * E,), -0.125, 0.125)] + [((E, E), -0.125, 0.125), ((E,), -0.125, 0.125)] * 3
        + [((E,), 0.5, 1.5), ((E,), -0.2, 0.2)] * 2)]
    layers = [layer_params("i%d" % i) for i in range(n_dec)]
    g2, b2 = dec_norm()
    xd, b1d, qed, posd, fc_wd, fc_bd, g2d, b2d = (t.to(dev) for t in (x, b1, qe, pos, fc_w, fc_b, g2, b2))
    encd = [t.to(dev) for t in enc]
    ld = [to_dev(p, dev) for p in layers]

    # the unfused chain, launch by launch (the host mirror's non-native path)
    src = ops.small_linear(xd, fc_wd, fc_bd, act="prelu", slope=slope)
    mem = ops.tatt_encoder_layer(src.reshape(B, S, E), posd, encd).reshape(B * S, E)
    out, tpc, pwc = b1d, torch.full((B * L, E), float("nan"), device=dev), None
    for li, p in enumerate(ld):
        q = ops.add_linear(out, qed, p["wq"], p["bq"])
        k = ops.small_linear(mem, p["wk"], p["bk"], add=posd)
        v = ops.small_linear(mem, p["wv"], p["bv"])
        o, w_ = ops.cross_attn(q.reshape(B, L, E), k.reshape(B, S, E), v.reshape(B, S, E), need_weights=li == n_dec - 1)
        pwc = w_ if li == n_dec - 1 else pwc
        out, _ = tail_chain(o.reshape(B * L, E), out, p, g2d, b2d, tpc, 1.0 / n_dec, li > 0)

    # the interpreter
    w = _abi.TattInterpWeights()
    w.n_dec, w.nhead = n_dec, 4
    w.fc_in_w, w.fc_in_b, w.fc_in_slope = dptr(fc_wd), dptr(fc_bd), slope
    for i, t in enumerate(encd):
        w.enc[i] = dptr(t)
    for i, p in enumerate(ld):
        for n in LAYER_NAMES:
            setattr(w.dec[i], n, dptr(p[n]))
    w.dec_norm_w, w.dec_norm_b = dptr(g2d), dptr(b2d)
    tpf, pwf = torch.full((B * L, E), float("nan"), device=dev), torch.full((B, L, S), float("nan"), device=dev)
    ws = torch.empty(lib.dpmn_tatt_interpreter_workspace_bytes(B, L, S) // 4, device=dev)
    check(lib.dpmn_tatt_interpreter_f32(C.byref(w), dptr(xd), T, dptr(b1d), dptr(qed), dptr(posd), dptr(tpf), dptr(pwf), dptr(ws),
                                        ws.numel() * 4, B, L, S, stream()))
    torch.cuda.synchronize()

    # float64 decoder from the shared encoder output
    m64, out64, tp64, pw64 = d64(mem), d64(b1), None, None
    for li, p in enumerate(layers):
        k64 = lin64(m64 + d64(pos).repeat(B, 1), p["wk"], p["bk"]).reshape(B, S, E)
        v64 = lin64(m64, p["wv"], p["bv"]).reshape(B, S, E)
        o64, pw64 = attn_ref(out64.reshape(B, L, E), qe.reshape(B, L, E), p["wq"], p["bq"], k64, v64)
        out64, tp64 = tail_ref(o64.reshape(B * L, E), out64, p, g2, b2, tp64, 1.0 / n_dec, li > 0)
    verify("tatt_interpreter[B2 L300 S26] tp", err(tpf, tp64), err(tpc, tp64))
    verify("tatt_interpreter[B2 L300 S26] pw", err(pwf, pw64), err(pwc, pw64))
