"""tests/ref64.py (the float64 references of the small-kernel GPU tests) pinned, each, to an independent statement of the same
operation -- the torch.nn module / torch.nn.functional routine or the oracle -- evaluated in float64: a mistake shared by a reference
and the kernel it judges would otherwise go unseen.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

import ref64
from dpmn_amd.utils import synth

RTOL = 1e-12


def u(name, shape, lo=-1.0, hi=1.0, seed=70):
    return synth.uniform(name, shape, lo, hi, seed).double()


def close(got, ref, what):
    """Elementwise |got - ref| <= RTOL * |ref| + ATOL, both float64.  The absolute term is for the elements that are small by cancellation
    only: a sum of n terms of size s carries n * 2^-53 * s of rounding whatever its own size, so an element 10^-4 of its neighbours has
    lost four digits in both operands alike (measured: one element of 4480 of the attention output at 1.8e-12 relative).  ATOL =
    2^-43 * max|ref| is that rounding for the longest sums here (n = 512, the C = 512 LayerNorm, x 2 operands), a tenth of RTOL at the
    tensor's own scale -- elements of ordinary size are still held to RTOL."""
    assert got.dtype == torch.float64 and ref.dtype == torch.float64 and got.shape == ref.shape, what
    err = (got - ref).abs()
    bad = err > RTOL * ref.abs() + 2.0 ** -43 * ref.abs().max()
    worst = (err / ref.abs().clamp_min(1e-300)).max().item()
    assert not bad.any(), "%s: worst relative error %.3e at %d / %d elements" % (what, worst, int(bad.sum()), ref.numel())


@pytest.mark.parametrize("axis,B,H,W", [("w", 2, 3, 7), ("h", 2, 6, 3), ("w", 1, 1, 1)])
def test_bigru_vs_nn_gru(axis, B, H, W):
    hid, I = 32, 24
    gru = torch.nn.GRU(I, hid, bidirectional=True, batch_first=True).double()
    sd = gru.state_dict()
    for k in sd:
        sd[k] = u(k, sd[k].shape, -0.4, 0.4)
    gru.load_state_dict(sd)
    x, res = u("x", (B, H, W, I)), u("res", (B, H, W, 2 * hid))
    gi = F.linear(x, torch.cat([sd["weight_ih_l0"], sd["weight_ih_l0_reverse"]]), torch.cat([sd["bias_ih_l0"], sd["bias_ih_l0_reverse"]]))
    whh = torch.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]])
    bhh = torch.stack([sd["bias_hh_l0"], sd["bias_hh_l0_reverse"]])
    seqs = x.reshape(B * H, W, I) if axis == "w" else x.transpose(1, 2).reshape(B * W, H, I)
    with torch.no_grad():
        ref = gru(seqs)[0]
    ref = ref.reshape(B, H, W, 2 * hid) if axis == "w" else ref.reshape(B, W, H, 2 * hid).transpose(1, 2)
    close(ref64.bigru(gi, whh, bhh, None, axis), ref, "bigru")
    close(ref64.bigru(gi, whh, bhh, res, axis), ref + res, "bigru + res")


@pytest.mark.parametrize("N,L,S", [(2, 9, 5), (1, 1, 1), (1, 70, 32)])
def test_cross_attn_vs_sdpa_and_oracle_mha(N, L, S):
    from oracle import tsrn as ot
    E, nh = 64, 4
    q, k, v = u("q", (N, L, E), -2, 2), u("k", (N, S, E), -2, 2), u("v", (N, S, E))
    o, pw = ref64.cross_attn(q, k, v)
    heads = lambda x: x.reshape(N, -1, nh, E // nh).transpose(1, 2)
    sd = F.scaled_dot_product_attention(heads(q), heads(k), heads(v)).transpose(1, 2).reshape(N, L, E)
    close(o, sd, "cross_attn vs scaled_dot_product_attention")
    # the oracle's nn.MultiheadAttention restatement with identity projections (exact in any precision): output and averaged weights
    eye = torch.eye(E, dtype=torch.float64)
    ident = {"in_proj_weight": eye.repeat(3, 1), "in_proj_bias": torch.zeros(3 * E, dtype=torch.float64), "out_proj.weight": eye,
             "out_proj.bias": torch.zeros(E, dtype=torch.float64)}
    oo, ow = ot.mha(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), ident, "")
    close(o, oo.transpose(0, 1), "cross_attn vs oracle mha")
    close(pw, ow, "cross_attn weights vs oracle mha")


@pytest.mark.parametrize("B,L,heads,d", [(2, 64, 3, 32), (1, 128, 2, 64), (1, 5, 1, 32)])
def test_mha_vs_sdpa(B, L, heads, d):
    qkv = u("qkv", (B * L, 3 * heads * d), -2, 2)
    q, k, v = (qkv[:, i * heads * d:(i + 1) * heads * d].reshape(B, L, heads, d).transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * L, heads * d)
    close(ref64.mha(qkv, B, L, heads, d), ref, "mha")
    close(ref64.mha(qkv, B, L, heads, d, 1.0 / math.sqrt(d)), ref, "mha, explicit scale")


def enc_weights(seed=70):
    E = 64
    return [u("in_w", (3 * E, E), -0.2, 0.2, seed), u("in_b", (3 * E,), -0.1, 0.1, seed), u("out_w", (E, E), -0.2, 0.2, seed),
            u("out_b", (E,), -0.1, 0.1, seed), u("l1_w", (E, E), -0.2, 0.2, seed), u("l1_b", (E,), -0.1, 0.1, seed),
            u("l2_w", (E, E), -0.2, 0.2, seed), u("l2_b", (E,), -0.1, 0.1, seed), u("n1_w", (E,), 0.5, 1.5, seed), u("n1_b", (E,), -0.5, 0.5, seed),
            u("n2_w", (E,), 0.5, 1.5, seed), u("n2_b", (E,), -0.5, 0.5, seed)]


@pytest.mark.parametrize("N,L", [(2, 7), (1, 1), (1, 32)])
def test_encoder_layer_vs_functional_composition(N, L):
    E = 64
    w = enc_weights()
    src, pos = u("src", (N, L, E)), u("pos", (L, E))
    x = (2.0 * src).transpose(0, 1)                       # (L, N, E): the doubled source is the layer input
    qk = x + pos[:, None, :]
    a, _ = F.multi_head_attention_forward(qk, qk, x, E, 4, w[0], w[1], None, None, False, 0.0, w[2], w[3], training=False, need_weights=False)
    y = F.layer_norm(x + a, (E,), w[8], w[9], 1e-5)
    ff = F.linear(F.relu(F.linear(y, w[4], w[5])), w[6], w[7])
    ref = F.layer_norm(y + ff, (E,), w[10], w[11], 1e-5).transpose(0, 1)
    close(ref64.encoder_layer(src, pos, w), ref, "encoder_layer")


@pytest.mark.parametrize("C", [64, 128, 256])
def test_layernorm_std_vs_oracle(C):
    from oracle import tsrn as ot
    x, a2, b2 = u("x", (9, C), -3, 3), u("a2", (C,), 0.5, 1.5), u("b2", (C,))
    close(ref64.layernorm_std(x, a2, b2, 1e-6), ot.tbsrn_ln(x, {"a_2": a2, "b_2": b2}, "", 1e-6), "layernorm_std")


@pytest.mark.parametrize("N,Win,C,H,W", [(2, 26, 8, 3, 64), (1, 1, 4, 2, 5), (2, 7, 4, 1, 7), (1, 5, 8, 2, 9), (2, 26, 4, 3, 1), (1, 203, 4, 2, 64)])
def test_tl_interp_vs_f_interpolate(N, Win, C, H, W):
    inp = u("tl", (N, Win, C))
    ref = F.interpolate(inp.transpose(1, 2)[:, :, None, :], size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    close(ref64.tl_interp(inp, H, W), ref.contiguous(), "tl_interp")


@pytest.mark.parametrize("R,H", [(1, 1), (5, 32), (3, 64)])
def test_gru_gate_vs_gru_cell(R, H):
    I = 11
    cell = torch.nn.GRUCell(I, H).double()
    sd = {k: u(k, v.shape, -0.5, 0.5) for k, v in cell.state_dict().items()}
    cell.load_state_dict(sd)
    x, h = u("x", (R, I), -2, 2), u("h", (R, H))
    with torch.no_grad():
        ref = cell(x, h)
    gi, gh = F.linear(x, sd["weight_ih"], sd["bias_ih"]), F.linear(h, sd["weight_hh"], sd["bias_hh"])
    close(ref64.gru_gate(gi, gh, h), ref, "gru_gate")


@pytest.mark.parametrize("C", [64, 96, 192, 512])
def test_layernorm_vs_f_layer_norm(C):
    x, w, b = u("x", (7, C), -3, 3), u("w", (C,), 0.5, 1.5), u("b", (C,))
    close(ref64.layernorm(x, w, b, 1e-5), F.layer_norm(x, (C,), w, b, 1e-5), "layernorm")


def test_add_layernorm64_vs_f_layer_norm():
    x, r, acc = u("x", (5, 64), -2, 2), u("r", (5, 64), -2, 2), u("acc", (5, 64))
    g, b, g2, b2 = u("g", (64,), 0.5, 1.5), u("b", (64,)), u("g2", (64,), 0.5, 1.5), u("b2", (64,))
    y0, none = ref64.add_layernorm64(x, None, g, b)
    assert none is None
    close(y0, F.layer_norm(x, (64,), g, b, 1e-5), "add_layernorm64, no residual")
    yr = F.layer_norm(x + r, (64,), g, b, 1e-5)
    second = 0.5 * F.layer_norm(yr, (64,), g2, b2, 1e-5)
    y, a = ref64.add_layernorm64(x, r, g, b, g2, b2, acc, 0.5, True)
    close(y, yr, "add_layernorm64")
    close(a, acc + second, "add_layernorm64 accumulate")
    y, a = ref64.add_layernorm64(x, r, g, b, g2, b2, torch.full((5, 64), float("nan")), 0.5, False)
    close(a, second, "add_layernorm64 overwrite")
    _, a = ref64.add_layernorm64(x, r, g, b, g2, b2, None, 0.5, False)
    close(a, second, "add_layernorm64 overwrite, no previous value")


@pytest.mark.parametrize("B,P,C,Cm", [(2, 4, 32, 12), (1, 1, 16, 4)])
def test_se_gate_vs_functional_composition(B, P, C, Cm):
    x = u("x", (B, 1, P, C), -2, 2)
    w1, b1, w2, b2 = u("w1", (Cm, C), -0.3, 0.3), u("b1", (Cm,)), u("w2", (C, Cm), -0.5, 0.5), u("b2", (C,))
    pooled = F.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 1).flatten(1)
    gate = torch.sigmoid(F.linear(F.relu(F.linear(pooled, w1, b1)), w2, b2))
    close(ref64.se_gate(x, w1, b1, w2, b2), x * gate[:, None, None, :] + x, "se_gate")
    close(ref64.se_gate(x.reshape(B, P, C), w1, b1, w2, b2), (x * gate[:, None, None, :] + x).reshape(B, P, C), "se_gate (B, P, C)")


@pytest.mark.parametrize("B,H,W,C,kh,kw", [(2, 4, 6, 8, 2, 3), (1, 6, 4, 4, 1, 2)])
def test_maxpool_affine_relu_vs_f_max_pool2d(B, H, W, C, kh, kw):
    x = u("x", (B, H, W, C), -2, 2)
    s, t = u("s", (C,), -1.5, 1.5), u("t", (C,))
    assert (s < 0).any() and (s > 0).any()
    nchw = lambda v: v.permute(0, 3, 1, 2)
    ref = F.max_pool2d(nchw(x), (kh, kw)).permute(0, 2, 3, 1)
    got = ref64.maxpool_affine_relu(x, kh, kw)
    assert torch.equal(got, ref)
    ref = F.max_pool2d(F.relu(nchw(x * s + t)), (kh, kw)).permute(0, 2, 3, 1).contiguous()
    close(ref64.maxpool_affine_relu(x, kh, kw, s, t), ref, "maxpool_affine_relu")
