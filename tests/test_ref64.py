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


# ====================================================================================================================
# the hand-written gradients of the backward references against torch.autograd of an independent forward, in double
def leaf(name, shape, lo=-1.0, hi=1.0):
    return u(name, shape, lo, hi).requires_grad_(True)


def test_gelu_and_its_derivative_vs_f_gelu():
    x = leaf("gx", (501,), -6, 6)
    y = F.gelu(x)
    close(ref64.gelu(x), y.detach(), "gelu")
    close(ref64.gelu_grad(x), torch.autograd.grad(y.sum(), x)[0], "gelu_grad")


@pytest.mark.parametrize("B,L,C,G", [(2, 37, 96, 3), (1, 1, 64, 1), (3, 33, 192, 2)])
def test_sk_select_and_backward_vs_autograd(B, L, C, G):
    cg = C // G
    cat, A, dV = leaf("cat", (B * L, C)), leaf("A", (B, G, cg)), u("dV", (B * L, cg))
    V = torch.einsum("bgc,blgc->blc", A, cat.reshape(B, L, G, cg)).reshape(B * L, cg)
    gcat, gA = torch.autograd.grad(V, (cat, A), dV)
    close(ref64.sk_select(cat, A, L), V.detach(), "sk_select")
    dcat, dA, parts = ref64.sk_select_bwd(cat, A, dV, L)
    close(dcat, gcat, "sk_select_bwd dcat")
    close(dA, gA, "sk_select_bwd dA")
    assert parts.shape == ((L + 31) // 32, B, C)
    close(parts.sum(0).reshape(B, G, cg), gA, "sk_select_bwd partial rows")


@pytest.mark.parametrize("B,C,G,dmid,ppi,L", [(3, 96, 3, 24, 7, 200), (1, 192, 2, 48, 1, 9), (2, 96, 2, 8, 9, 64)])
def test_sk_gate_backward_vs_autograd(B, C, G, dmid, ppi, L):
    partial = leaf("part", (B * ppi, C), 0.0, 20.0)
    w1, b1 = leaf("w1", (dmid, C), -0.2, 0.2), leaf("b1", (dmid,), -0.3, 0.3)
    w2, b2 = leaf("w2", (C, dmid), -0.5, 0.5), leaf("b2", (C,), -0.3, 0.3)
    dA = u("dA", (B, G, C // G))
    S = partial.reshape(B, ppi, C).sum(1) / L
    S.retain_grad()
    A = torch.softmax(F.linear(F.gelu(F.linear(S, w1, b1)), w2, b2).reshape(B, G, C // G), 1)
    A.backward(dA)
    close(ref64.sk_pool(partial, ppi, L), S.detach(), "sk_pool")
    close(ref64.sk_gate(S, w1, b1, w2, b2, G), A.detach(), "sk_gate")
    r = ref64.sk_gate_bwd(partial, ppi, L, w1, b1, w2, A, dA)
    for key, g in (("dS", S.grad), ("dfc1_w", w1.grad), ("dfc1_b", b1.grad), ("dfc2_w", w2.grad), ("dfc2_b", b2.grad)):
        close(r[key], g, "sk_gate_bwd " + key)
    close(r["wpart2"].sum(0), torch.cat([w2.grad.reshape(-1), b2.grad]), "sk_gate_bwd wpart2")
    close(r["wpart1"].sum(0), torch.cat([w1.grad.reshape(-1), b1.grad]), "sk_gate_bwd wpart1")


@pytest.mark.parametrize("B,L,C", [(3, 5, 97), (1, 1, 96)])
def test_sk_feats_grad_vs_autograd(B, L, C):
    feats, dout, dS = leaf("feats", (B * L, C), -6, 6), u("dout", (B * L, C)), u("dS", (B, C))
    loss = (feats * dout).sum() + (F.gelu(feats).reshape(B, L, C).mean(1) * dS).sum()
    close(ref64.sk_feats_grad(dout, feats, dS, L), torch.autograd.grad(loss, feats)[0], "sk_feats_grad")


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("gp,in_gelu,out_gelu", [(False, False, False), (True, False, False), (True, True, False), (True, True, True)])
@pytest.mark.parametrize("B,Ch,r", [(2, 3, 4), (1, 5, 12)])
def test_dwconv3x3_backward_vs_autograd(B, Ch, r, gp, in_gelu, out_gelu, with_mask):
    P, w, bias = leaf("P", (B, Ch, r, r), -3, 3), leaf("w", (Ch, 3, 3)), leaf("bias", (Ch,))
    dg = u("dg", (B, Ch, r, r))
    mask = (u("m", (B, Ch, r, r), 0, 1) > 0.3).double() / 0.7 if with_mask else None
    a = F.gelu(P) if in_gelu else P
    if not out_gelu:
        a = a.detach().requires_grad_(True)      # the kernel then returns the gradient of the conv's (unmasked) input
    x = a * mask if with_mask else a
    y = F.conv2d(x, w[:, None], bias, padding=1, groups=Ch)
    out = F.gelu(y) if gp else y
    gin, gw, gb = torch.autograd.grad(out, (P if out_gelu else a, w, bias), dg)
    dP, dw, db = ref64.dwconv3x3_bwd(P, dg, w, y if gp else None, in_gelu, out_gelu, mask)
    close(dP, gin, "dwconv3x3_bwd dP")
    close(dw, gw.reshape(Ch, 9), "dwconv3x3_bwd dw")
    close(db, gb, "dwconv3x3_bwd db")


def _torch_act(x, name, slope):
    return {"none": lambda v: v * 1.0, "gelu": F.gelu, "relu": F.relu, "leaky02": lambda v: F.leaky_relu(v, 0.2),
            "leaky001": lambda v: F.leaky_relu(v, 0.01), "mish": F.mish, "prelu": lambda v: F.prelu(v, torch.tensor([slope], dtype=v.dtype)),
            "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name](x)


@pytest.mark.parametrize("name", sorted(ref64.ACT_CODES))
def test_act_and_its_derivative_vs_torch(name):
    code, slope = ref64.ACT_CODES[name], 0.25
    with torch.no_grad():
        x0 = u("ax", (400,), -6, 6)
        x0[::50] = 0.0                       # the kink: value 0, slope of the negative side
    x = x0.requires_grad_(True)
    y = _torch_act(x, name, slope)
    close(ref64.act(x, code, slope), y.detach(), "act " + name)
    close(ref64.act_grad(x, code, slope), torch.autograd.grad(y.sum(), x)[0], "act_grad " + name)


def test_elementwise_and_reduction_references():
    x, z, y = u("x", (257,)), u("z", (257,)), u("y", (257,))
    close(ref64.axpby(x, z, y, 0.5, -2.0, True), torch.add(torch.add(y, x, alpha=0.5), z, alpha=-2.0), "axpby accumulate")
    close(ref64.axpby(x, None, y, 0.5, -2.0, False), 0.5 * x, "axpby z = None, overwrite")
    m = u("m", (35, 13))
    want = torch.zeros(7, dtype=torch.float64).index_add_(0, torch.arange(35) % 7, m.sum(1))
    close(ref64.rowsum_mod(m, 7), want, "rowsum_mod")
    close(ref64.colsum(m), torch.ones(1, 35, dtype=torch.float64).mm(m)[0], "colsum")
    dw, db = ref64.rows_reduce(m, 9, 4)
    close(dw, sum(m[i, :9] for i in range(35)), "rows_reduce dw")
    close(db, sum(m[i, 9:] for i in range(35)), "rows_reduce db")
    assert ref64.rows_reduce(m, 13, 0)[1].numel() == 0


@pytest.mark.parametrize("B,H,W,n", [(3, 2, 3, 4), (1, 2, 3, 0), (2, 4, 2, 1)])
def test_tail_elem_and_backward_vs_autograd(B, H, W, n):
    with torch.no_grad():
        c0 = u("c1", (B, H, W, 12))
        c0.reshape(-1)[::7] = 0.0
    c1 = c0.requires_grad_(True)
    wl = [leaf("wl%d" % i, (3, 2 * H, 2 * W)) for i in range(max(n, 1))]
    res = [leaf("res%d" % i, (B, 3, 2 * H, 2 * W)) for i in range(n)]
    dout = u("dout", (B, 3, 2 * H, 2 * W))
    out = F.leaky_relu(F.pixel_shuffle(c1.permute(0, 3, 1, 2), 2), 0.01) * wl[0]
    for i in range(1, n):                    # residual 0 is skipped
        out = out + res[i] * wl[i]
    out.backward(dout)
    close(ref64.tail_elem(c1, wl, res), out.detach(), "tail_elem")
    dc1, dwl, dres = ref64.tail_elem_bwd(dout, c1, wl, res)
    close(dc1, c1.grad, "tail_elem_bwd dc1")
    assert len(dwl) == max(n, 1) and len(dres) == max(n, 1) and dres[0] is None and (n == 0 or res[0].grad is None)
    for i in range(max(n, 1)):
        close(dwl[i], wl[i].grad, "tail_elem_bwd dwl %d" % i)
    for i in range(1, n):
        close(dres[i], res[i].grad, "tail_elem_bwd dres %d" % i)


@pytest.mark.parametrize("B,P,C,Cm", [(3, 7, 32, 32), (1, 1, 64, 32)])
def test_se_gate_backward_vs_autograd(B, P, C, Cm):
    x, dg = leaf("x", (B, P, C), -2, 2), u("dg", (B, P, C))
    w1, b1, w2, b2 = leaf("w1", (Cm, C), -0.3, 0.3), leaf("b1", (Cm,)), leaf("w2", (C, Cm), -0.5, 0.5), leaf("b2", (C,))
    gate = torch.sigmoid(F.linear(F.relu(F.linear(x.mean(1), w1, b1)), w2, b2))
    g = x * (1.0 + gate[:, None])
    close(ref64.se_gate(x, w1, b1, w2, b2), g.detach(), "se_gate")
    g.backward(dg)
    for got, want, what in zip(ref64.se_gate_bwd(x, dg, w1, b1, w2, b2), (x.grad, w1.grad, b1.grad, w2.grad, b2.grad), ("dx", "dfc1_w", "dfc1_b", "dfc2_w", "dfc2_b")):
        close(got, want, "se_gate_bwd " + what)


@pytest.mark.parametrize("with_extra", [False, True])
def test_l1_loss_and_backward_vs_autograd(with_extra):
    n = 257
    with torch.no_grad():
        a0, b0 = u("a", (n,)), u("b", (n,))
        b0[::5] = a0[::5]                    # exact ties: sign(0) = 0
    a, b = a0.requires_grad_(True), b0.requires_grad_(True)
    extra = u("extra", (n,)) if with_extra else None
    loss = F.l1_loss(a, b, reduction="sum") / n
    close(ref64.l1_loss(a, b, 1.0 / n), loss.detach().reshape(1), "l1_loss")
    total = 0.7 * loss + ((a * extra).sum() if with_extra else 0.0)
    total.backward()
    da, db = ref64.l1_loss_bwd(a, b, 0.7, 1.0 / n, extra)
    assert bool((da[::5] == (extra[::5] if with_extra else 0.0)).all()) and bool((db[::5] == 0).all())
    close(da, a.grad, "l1_loss_bwd da")
    close(db, b.grad, "l1_loss_bwd db")


# ====================================================================================================================
# GEMM family references
@pytest.mark.parametrize("name", ["none", "gelu", "leaky02", "prelu"])
@pytest.mark.parametrize("M,N,K", [(5, 8, 32), (33, 100, 96)])
def test_linear_vs_f_linear(M, N, K, name):
    code, slope = ref64.ACT_CODES[name], 0.25
    x, w, b, r1, r2 = u("lx", (M, K)), u("lw", (N, K), -0.3, 0.3), u("lb", (N,)), u("lr1", (M, N)), u("lr2", (M, N))
    pre = F.linear(x, w, b)
    close(ref64.linear(x, w), F.linear(x, w), "linear")
    close(ref64.linear(x, w, b, None, None, code, slope), _torch_act(pre, name, slope), "linear bias " + name)
    close(ref64.linear(x, w, b, r1, None, code, slope), _torch_act(pre, name, slope) + r1, "linear res1 " + name)
    close(ref64.linear(x, w, b, r1, r2, code, slope), _torch_act(pre, name, slope) + r1 + r2, "linear res1 res2 " + name)
    close(ref64.linear(x, w, None, r1, None, code, slope), _torch_act(F.linear(x, w), name, slope) + r1, "linear no bias " + name)


@pytest.mark.parametrize("M,N,K", [(5, 8, 32), (33, 100, 96)])
def test_linear_prologues_vs_functional(M, N, K):
    x, w, b = u("px", (M, K)), u("pw", (N, K), -0.3, 0.3), u("pb", (N,))
    addv = u("padd", (M, K))
    close(ref64.linear(x, w, b, act_code=1, pro=("add", addv)), F.gelu(F.linear(x + addv, w, b)), "add prologue")
    k1 = K // 4 + 4
    close(ref64.linear(x[:, :k1].contiguous(), w, b, act_code=1, pro=("cat2", x[:, k1:].contiguous())), F.gelu(F.linear(x, w, b)), "cat2 prologue")
    xo = x + 3.0 * u("prow", (M, 1))
    gm, bt = u("pg", (K,), 0.5, 1.5), u("pbeta", (K,))
    close(ref64.linear(xo, w, b, act_code=1, pro=("ln", gm, bt, 1e-5)), F.gelu(F.linear(F.layer_norm(xo, (K,), gm, bt, 1e-5), w, b)), "ln prologue")


def test_linear_drop_and_sk_proj_vs_functional():
    M, N, K = 12, 8, 32
    x, w, b, res = u("dx", (M, K)), u("dw", (N, K), -0.3, 0.3), u("db", (N,)), u("dres", (M, N))
    me = (u("dme", (M, N), 0, 1) > 0.3).double() / 0.7
    mr = ((u("dmr", (M, 1), 0, 1) > 0.25).double() / 0.75).expand(M, N)
    close(ref64.linear_drop(x, w, b, res, me, mr), res + F.linear(x, w, b) * me * mr, "linear_drop")
    close(ref64.linear_drop(x, w, b, res, None, mr), res + F.linear(x, w, b) * mr, "linear_drop row mask only")
    M = 70
    cat = u("scat", (M, K), -3, 3)
    feats, part = ref64.sk_proj(cat, w, b)
    close(feats, F.linear(cat, w, b), "sk_proj feats")
    assert part.shape == (3, N)
    want = torch.zeros(3, N, dtype=torch.float64).index_add_(0, torch.arange(M) // 32, F.gelu(F.linear(cat, w, b)))
    close(part, want, "sk_proj partial column sums")


@pytest.mark.parametrize("B,Ch,L", [(3, 8, 32), (1, 12, 64)])
def test_pointwise_and_wgrad_vs_conv1d_autograd(B, Ch, L):
    g, w, bias, dz = leaf("pwg", (B, Ch, L)), leaf("pww", (Ch, Ch)), leaf("pwb", (Ch,)), u("pwdz", (B, Ch, L))
    z = F.conv1d(g, w[:, :, None], bias)
    close(ref64.pointwise(g, w, bias), z.detach(), "pointwise")
    close(ref64.pointwise_wgrad(dz, g), torch.autograd.grad(z, w, dz)[0], "pointwise_wgrad")


@pytest.mark.parametrize("M,N,K", [(1, 4, 8), (37, 12, 20)])
def test_gemm_tn_vs_autograd(M, N, K):
    x, w, b, dy = u("tx", (M, K)), leaf("tw", (N, K)), leaf("tb", (N,)), u("tdy", (M, N))
    gw, gb = torch.autograd.grad(F.linear(x, w, b), (w, b), dy)
    dW, db = ref64.gemm_tn(dy, x)
    close(dW, gw, "gemm_tn dW")
    close(db, gb, "gemm_tn db")


# ====================================================================================================================
# conv family references: tiny ragged planes, stride 2, dilation 2, a padding larger than the kernel's radius, 1 .. 3 segments
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


CODE = ref64.ACT_CODES
CONV_GEOM = [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (4, 2, 3, 2), (4, 2, 1, 1), (3, 1, 3, 1), (1, 1, 0, 1), (9, 1, 4, 1), (2, 2, 3, 2)]


def _conv_pin_case(k, segs_c, cout, B, H, W):
    segs = [u("cs%d" % i, (B, H, W, c), -2, 2) for i, c in enumerate(segs_c)]
    aff = [(u("csc%d" % i, (c,), 0.5, 1.5), u("csh%d" % i, (c,), -0.5, 0.5)) if i != 1 else None for i, c in enumerate(segs_c)]
    w, b = u("cw", (cout, sum(segs_c), k, k), -0.3, 0.3), u("cb", (cout,))
    return segs, aff, w, b


def _torch_conv_input(segs, aff, pro):
    xs = [s if a is None else s * a[0] + a[1] for s, a in zip(segs, aff)]
    return _nchw(_torch_act(torch.cat(xs, 3), pro, 0.0))


@pytest.mark.parametrize("k,stride,pad,dil", CONV_GEOM)
@pytest.mark.parametrize("segs_c", [(5,), (3, 4), (2, 1, 3)])
def test_conv2d_vs_f_conv2d(k, stride, pad, dil, segs_c):
    B, H, W, cout = 2, 7, 11, 8
    segs, aff, w, b = _conv_pin_case(k, segs_c, cout, B, H, W)
    for pro, epi in (("none", "none"), ("leaky02", "mish"), ("relu", "prelu")):
        raw = F.conv2d(_torch_conv_input(segs, aff, pro), w, b, stride, pad, dil)
        res = u("cres", tuple(_nhwc(raw).shape))
        want = _nhwc(_torch_act(raw, epi, 0.25)) + res
        got = ref64.conv2d(segs, w, b, stride, pad, dil, CODE[pro], CODE[epi], 0.25, aff, res)
        close(got, want, "conv2d %s %s" % (pro, epi))
    close(ref64.conv2d(segs, w, None, stride, pad, dil), _nhwc(F.conv2d(_nchw(torch.cat(segs, 3)), w, None, stride, pad, dil)), "conv2d plain")
    raw = F.conv2d(_nchw(torch.cat(segs, 3)), w, b, stride, pad, dil)
    close(ref64.conv2d(segs, w, b, stride, pad, dil, out_nchw=True), raw.contiguous(), "conv2d NCHW")
    close(ref64.conv2d(segs, w, b, stride, pad, dil, epi=CODE["relu"], pixel_shuffle=True), _nhwc(F.pixel_shuffle(F.relu(raw), 2)), "conv2d pixel shuffle")
    s, q = ref64.conv_stats(_nhwc(raw))
    close(s, raw.sum((0, 2, 3)), "stats sum")
    close(q, (raw * raw).sum((0, 2, 3)), "stats sum of squares")


def test_conv2d_zero_padding_stays_zero_under_the_affine():
    """a shift would otherwise leak into the border: the affine and the activation come BEFORE the padding"""
    x, w = torch.zeros(1, 3, 3, 1, dtype=torch.float64), torch.ones(1, 1, 3, 3, dtype=torch.float64)
    got = ref64.conv2d([x], w, None, 1, 1, 1, affine=[(torch.ones(1), torch.ones(1))])
    assert got.reshape(3, 3).tolist() == [[4.0, 6.0, 4.0], [6.0, 9.0, 6.0], [4.0, 6.0, 4.0]]


@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (4, 2, 1)])
@pytest.mark.parametrize("segs_c", [(5,), (2, 1, 3)])
def test_conv_transpose2d_and_its_gradients_vs_autograd(k, stride, pad, segs_c):
    B, H, W, cout = 2, 3, 5, 6
    segs, aff, _, b = _conv_pin_case(k, segs_c, cout, B, H, W)
    w = leaf("ctw", (sum(segs_c), cout, k, k), -0.3, 0.3)
    xin = _torch_conv_input(segs, aff, "relu").requires_grad_(True)
    raw = F.conv_transpose2d(xin, w, b, stride, pad)
    dy = u("ctdy", tuple(_nhwc(raw).shape))
    close(ref64.conv_transpose2d(segs, w, b, stride, pad, CODE["relu"], CODE["tanh"], affine=aff), _nhwc(torch.tanh(raw)).detach(), "conv_transpose2d")
    gx, gw = torch.autograd.grad(raw, (xin, w), _nchw(dy))
    close(ref64.conv_transpose2d_wgrad(segs, dy, k, stride, pad, CODE["relu"], aff), gw, "conv_transpose2d_wgrad")
    close(ref64.conv_transpose2d_dgrad(dy, w, stride, pad), _nhwc(gx), "conv_transpose2d_dgrad")
    c0, cs = 1, sum(segs_c) - 2
    close(ref64.conv_transpose2d_dgrad(dy, w, stride, pad, c0, cs), _nhwc(gx)[..., c0:c0 + cs].contiguous(), "conv_transpose2d_dgrad slice")


@pytest.mark.parametrize("k,stride,pad,dil", CONV_GEOM)
@pytest.mark.parametrize("segs_c", [(5,), (2, 1, 3)])
def test_conv2d_gradients_vs_autograd(k, stride, pad, dil, segs_c):
    B, H, W, cout = 2, 7, 11, 4
    segs, aff, _, b = _conv_pin_case(k, segs_c, cout, B, H, W)
    w = leaf("gw", (cout, sum(segs_c), k, k), -0.3, 0.3)
    xin = _torch_conv_input(segs, aff, "leaky001").requires_grad_(True)
    raw = F.conv2d(xin, w, b, stride, pad, dil)
    dy = u("gdy", tuple(_nhwc(raw).shape))
    gx, gw = torch.autograd.grad(raw, (xin, w), _nchw(dy))
    close(ref64.conv2d_wgrad(segs, dy, k, stride, pad, dil, CODE["leaky001"], aff), gw, "conv2d_wgrad")
    close(ref64.conv2d_dgrad(dy, w, (H, W), stride, pad, dil), _nhwc(gx), "conv2d_dgrad")
    c0, cs = 1, sum(segs_c) - 2
    close(ref64.conv2d_dgrad(dy, w, (H, W), stride, pad, dil, c0, cs), _nhwc(gx)[..., c0:c0 + cs].contiguous(), "conv2d_dgrad slice")


def test_conv_references_fp32_evaluation():
    """dtype=float32 evaluates the same formulas in fp32 (the yardstick of the continuous-kind tolerances)"""
    segs, aff, w, b = _conv_pin_case(3, (3, 4), 8, 2, 5, 6)
    pro, epi = CODE["leaky02"], CODE["mish"]
    y64, y32 = ref64.conv2d(segs, w, b, 1, 1, 1, pro, epi, affine=aff), ref64.conv2d(segs, w, b, 1, 1, 1, pro, epi, affine=aff, dtype=torch.float32)
    assert y32.dtype == torch.float32 and 0 < float((y32.double() - y64).abs().max()) < 1e-5
    dy = u("fdy", tuple(y64.shape))
    g32 = ref64.conv2d_wgrad(segs, dy, 3, 1, 1, 1, pro, aff, dtype=torch.float32)
    assert g32.dtype == torch.float32 and float((g32.double() - ref64.conv2d_wgrad(segs, dy, 3, 1, 1, 1, pro, aff)).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------ window attention
# forward against oracle.pgrm.window_attention_core in double, backward against torch.autograd through it; H == ws for the window of 8 /
# W > H, and H == W == ws for the window of 16; unsorted window sets, shifts 0, 1, ws / 2 (+ 1), ws - 1
WATTN_GEOM = [(8, 16, [8, 2, 4], [7, 1, 3]), (16, 16, [16, 4, 8], [5, 0, 1])]


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("H,W,windows,shifts", WATTN_GEOM)
def test_window_attn_vs_oracle_and_autograd(H, W, windows, shifts, p_drop):
    from oracle import pgrm as op
    B, C, L, seed = 2, 96, H * W, 0x1234ABCD
    q, k, v = leaf("waq", (B, L, C), -2, 2), leaf("wak", (B, L, C), -2, 2), leaf("wav", (B, L, C))
    sd = {"a.relative_position_bias_table_%d" % g: leaf("watbl%d" % g, ((2 * ws - 1) ** 2, 2)) for g, ws in enumerate(windows)}
    tables = [sd["a.relative_position_bias_table_%d" % g] for g in range(3)]
    dout = u("wadout", (B, L, C))
    ref = op.window_attention_core(q, k, v, sd, "a.", H, W, windows, shifts, 2, p_drop, seed)
    grads = torch.autograd.grad(ref, [q, k, v] + tables, dout)
    kv = torch.cat([k, v], -1).detach()
    close(ref64.window_attn(q, kv, tables, windows, shifts, H, W, p_drop, seed), ref.detach(), "window_attn")
    dq, dkv, dt = ref64.window_attn_bwd(q, kv, tables, windows, shifts, H, W, dout, p_drop, seed)
    close(dq, grads[0], "window_attn_bwd dq")
    close(dkv, torch.cat([grads[1], grads[2]], -1), "window_attn_bwd dkv")
    for g in range(3):
        close(dt[g], grads[3 + g], "window_attn_bwd dtable %d" % g)


def test_ln_qkv_window_attn_vs_oracle():
    """the fused operator = nn.LayerNorm + nn.Linear + the core; its backward twin returns the gradients of the PROJECTED q / kv"""
    from oracle import pgrm as op
    B, C, H, W, windows, shifts, p, seed = 2, 96, 8, 16, [8, 2, 4], [7, 1, 3], 0.3, 77
    L = H * W
    tq, tkv = u("ftq", (B, L, C)), u("ftkv", (B, L, C))
    ln = (u("g1", (C,), 0.5, 1.5), u("b1", (C,), -0.2, 0.2), u("g2", (C,), 0.5, 1.5), u("b2", (C,), -0.2, 0.2),
          u("fwq", (C, C), -0.3, 0.3), u("fbq", (C,)), u("fwkv", (2 * C, C), -0.3, 0.3), u("fbkv", (2 * C,)))
    sd = {"a.relative_position_bias_table_%d" % g: u("ftbl%d" % g, ((2 * ws - 1) ** 2, 2)) for g, ws in enumerate(windows)}
    tables = [sd["a.relative_position_bias_table_%d" % g] for g in range(3)]
    q = F.linear(F.layer_norm(tq, (C,), ln[0], ln[1]), ln[4], ln[5]).requires_grad_(True)
    kv = F.linear(F.layer_norm(tkv, (C,), ln[2], ln[3]), ln[6], ln[7]).requires_grad_(True)
    ref = op.window_attention_core(q, kv[..., :C], kv[..., C:], sd, "a.", H, W, windows, shifts, 2, p, seed)
    dout = u("fdout", (B, L, C))
    gq, gkv = torch.autograd.grad(ref, (q, kv), dout)
    cat, q64, kv64 = ref64.ln_qkv_window_attn(tq, tkv, ln, tables, windows, shifts, H, W, p, seed)
    close(q64, q.detach(), "ln_qkv q")
    close(kv64, kv.detach(), "ln_qkv kv")
    close(cat, ref.detach(), "ln_qkv_window_attn")
    dq, dkv, _ = ref64.ln_qkv_window_attn_bwd(tq, tkv, ln, tables, windows, shifts, H, W, dout, p, seed)
    close(dq, gq, "ln_qkv_window_attn_bwd dq")
    close(dkv, gkv, "ln_qkv_window_attn_bwd dkv")


def test_window_attn_fp32_evaluation():
    """dtype=float32 evaluates the same formulas in fp32 (the yardstick of the GPU suite's bounds)"""
    B, C, H, W, windows, shifts = 1, 96, 8, 8, [2, 4, 8], [1, 2, 7]
    q, kv = u("yq", (B, 64, C)), u("ykv", (B, 64, 2 * C))
    tables = [u("ytbl%d" % g, ((2 * ws - 1) ** 2, 2)) for g, ws in enumerate(windows)]
    o64, o32 = ref64.window_attn(q, kv, tables, windows, shifts, H, W, 0.3, 5), ref64.window_attn(q, kv, tables, windows, shifts, H, W, 0.3, 5, dtype=torch.float32)
    assert o32.dtype == torch.float32 and 0 < float((o32.double() - o64).abs().max()) < 1e-5
    g32 = ref64.window_attn_bwd(q, kv, tables, windows, shifts, H, W, o64, 0.3, 5, dtype=torch.float32)
    g64 = ref64.window_attn_bwd(q, kv, tables, windows, shifts, H, W, o64, 0.3, 5)
    assert all(a.dtype == torch.float32 and float((a.double() - b).abs().max()) < 1e-5 for a, b in zip((g32[0], g32[1], *g32[2]), (g64[0], g64[1], *g64[2])))


# ------------------------------------------------------------------------------------------------------------------ recogniser kernels
def _grucell(I, D, tag):
    cell = torch.nn.GRUCell(I, D).double()
    sd = {k: u(tag + k, v.shape, -0.5, 0.5) for k, v in cell.state_dict().items()}
    cell.load_state_dict(sd)
    return cell, sd


@pytest.mark.parametrize("B,T", [(1, 1), (3, 4), (2, 7)])
def test_bilstm_vs_nn_lstm(B, T):
    H, I = 8, 5
    lstm = torch.nn.LSTM(I, H, bidirectional=True, batch_first=True).double()
    sd = {k: u(k, v.shape, -0.5, 0.5) for k, v in lstm.state_dict().items()}
    lstm.load_state_dict(sd)
    x = u("lstm_x", (B, T, I), -2, 2)
    gx = torch.cat([F.linear(x, sd["weight_ih_l0" + s], sd["bias_ih_l0" + s] + sd["bias_hh_l0" + s]) for s in ("", "_reverse")], -1)
    with torch.no_grad():
        ref, (_, cn) = lstm(x)
    out, cst = ref64.bilstm(gx.reshape(B * T, 8 * H), torch.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]]), B, T)
    close(out, ref.reshape(B * T, 2 * H), "bilstm out")
    close(cst, cn, "bilstm cell state")


def test_gru_cell_table_vs_nn_grucell():
    D, Ie, n = 8, 6, 5
    cell, sd = _grucell(Ie + D, D, "gct")
    table, ctx, h = u("gct_tab", (n, Ie)), u("gct_ctx", (4, D)), u("gct_h", (4, D))
    y = torch.tensor([0, 4, 2, 4])
    E = F.linear(table, sd["weight_ih"][:, :Ie], sd["bias_ih"])
    with torch.no_grad():
        ref = cell(torch.cat([table[y], ctx], 1), h)
    close(ref64.gru_cell_table(E[y], ctx, sd["weight_ih"][:, Ie:], h, sd["weight_hh"], sd["bias_hh"]), ref, "gru_cell_table")


def _aster_small(D=8, n_class=6, B=3, T=4, tag="as"):
    cell, sd = _grucell(2 * D, D, tag)
    emb = u(tag + "emb", (n_class + 1, D))
    w = {"s_w": u(tag + "s_w", (D, D)), "s_b": u(tag + "s_b", (D,)), "w_w": u(tag + "w_w", (D,), -2, 2), "w_b": u(tag + "w_b", (1,)),
         "E": F.linear(emb, sd["weight_ih"][:, :D], sd["bias_ih"]), "wih_ctx": sd["weight_ih"][:, D:], "whh": sd["weight_hh"],
         "bhh": sd["bias_hh"], "fc_w": u(tag + "fc_w", (n_class, D), -3, 3), "fc_b": u(tag + "fc_b", (n_class,))}
    return cell, emb, w, u(tag + "feats", (B, T, D)), u(tag + "xproj", (B, T, D))


def _aster_stock_step(cell, emb, w, feats, xproj, row_img, state, y_prev):
    """the same step from nn.GRUCell, F.linear and F.softmax"""
    sproj = F.linear(state, w["s_w"], w["s_b"])
    e = F.linear(torch.tanh(sproj[:, None] + xproj[row_img]), w["w_w"][None], w["w_b"]).squeeze(-1)
    alpha = F.softmax(e, -1)
    ctx = torch.bmm(alpha[:, None], feats[row_img]).squeeze(1)
    with torch.no_grad():
        snew = cell(torch.cat([emb[y_prev], ctx], 1), state)
    return sproj, alpha, ctx, snew, F.linear(snew, w["fc_w"], w["fc_b"])


def test_aster_decode_step_vs_stock():
    cell, emb, w, feats, xproj = _aster_small()
    row_img, y_prev, state = torch.tensor([2, 0, 0, 1, 2]), torch.tensor([0, 6, 3, 5, 6]), u("as_state", (5, 8))
    got = ref64.aster_decode_step(w, feats, xproj, row_img, state, y_prev, 6)
    for name, ref in zip(("sproj", "alpha", "ctx", "state_out", "logits"), _aster_stock_step(cell, emb, w, feats, xproj, row_img, state, y_prev)):
        close(got[name], ref, "aster_decode_step " + name)


@pytest.mark.parametrize("beam,eos", [(1, 0), (3, 2)])
def test_aster_beam_vs_log_softmax_topk(beam, eos):
    n_class, steps = 6, 4
    cell, emb, w, feats, xproj = _aster_small()
    B, R = feats.shape[0], feats.shape[0] * beam
    got = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps)
    state, yprev = torch.zeros(R, 8, dtype=torch.float64), torch.full((R,), n_class)
    seq = torch.full((B, beam), float("-inf"), dtype=torch.float64)
    seq[:, 0] = 0.0
    for s in range(steps):
        snew, logits = _aster_stock_step(cell, emb, w, feats, xproj, torch.arange(R) // beam, state, yprev)[3:]
        cand = (seq[:, :, None] + F.log_softmax(logits, -1).reshape(B, beam, n_class)).reshape(B, beam * n_class)
        top, flat = cand.topk(beam, -1)
        finite = torch.isfinite(top)
        gap = (top[:, :-1] - top[:, 1:])[finite[:, 1:]]
        assert gap.numel() == 0 or float(gap.min()) > 1e-6      # no near-ties among the finite ones: topk's order is the documented one
        pred, sym = (flat // n_class + torch.arange(B)[:, None] * beam).reshape(R), (flat % n_class).reshape(R)
        ok = finite.reshape(R)      # among -inf candidates topk's order is unspecified: the values are still pinned
        assert torch.equal(got["sym"][s][ok], sym[ok]) and torch.equal(got["pred"][s][ok], pred[ok]), "beam step %d" % s
        assert torch.equal(torch.isfinite(got["score"][s]), ok)
        close(got["score"][s][ok], top.reshape(R)[ok], "beam score step %d" % s)
        sym, pred = got["sym"][s], got["pred"][s]
        seq = torch.where(sym == eos, torch.tensor(float("-inf"), dtype=torch.float64), got["score"][s]).reshape(B, beam)
        state, yprev = snew[pred], sym
    close(got["state"], state, "beam final state")
    # the replay of its own decisions is the same computation
    again = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=(got["sym"], got["pred"]))
    assert torch.equal(again["score"], got["score"]) and torch.equal(again["state"], got["state"])


def test_beam_select_ties_take_the_lower_flat_index():
    cand = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, float("-inf")], [float("-inf")] * 6], dtype=torch.float64)
    assert ref64.beam_select(cand, 4).tolist() == [[1, 2, 4, 3], [0, 1, 2, 3]]
    assert ref64.first_argmax(torch.tensor([[1.0, 5.0, 5.0], [2.0, 2.0, 2.0]])).tolist() == [1, 0]


def test_moran_decode_vs_stock():
    D, n_class, B, T, steps = 8, 5, 3, 4, 6
    cell, sd = _grucell(2 * D, D, "mo")          # MORAN's order: [context | embedding]
    emb = u("mo_emb", (n_class + 1, D))
    w = {"h2h_w": u("mo_h2h", (D, D)), "h2h_b": u("mo_h2hb", (D,)), "score_w": u("mo_sc", (D,), -2, 2),
         "E": F.linear(emb, sd["weight_ih"][:, D:], sd["bias_ih"]), "wih_ctx": sd["weight_ih"][:, :D], "whh": sd["weight_hh"],
         "bhh": sd["bias_hh"], "gen_w": u("mo_gen", (n_class, D), -3, 3), "gen_b": u("mo_genb", (n_class,))}
    feats, fproj = u("mo_feats", (B, T, D)), u("mo_fproj", (B, T, D))
    logits, ids = ref64.moran_decode(w, feats, fproj, steps, n_class)
    h, y = torch.zeros(B, D, dtype=torch.float64), torch.zeros(B, dtype=torch.long)
    for s in range(steps):
        alpha = F.softmax(F.linear(torch.tanh(fproj + F.linear(h, w["h2h_w"], w["h2h_b"])[:, None]), w["score_w"][None]).squeeze(-1), -1)
        with torch.no_grad():
            h = cell(torch.cat([torch.bmm(alpha[:, None], feats).squeeze(1), emb[y]], 1), h)
        lg = F.linear(h, w["gen_w"], w["gen_b"])
        top2 = lg.topk(2, -1)[0]
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-6
        close(logits[:, s], lg, "moran logits step %d" % s)
        assert torch.equal(ids[:, s], lg.argmax(-1))
        y = ids[:, s] + 1
    again, ids2 = ref64.moran_decode(w, feats, fproj, steps, n_class, ids=ids)
    assert torch.equal(again, logits) and torch.equal(ids2, ids)
    forced = (ids + 1) % n_class          # a replay follows the ids it is given, not its own arg-max
    assert torch.equal(ref64.moran_decode(w, feats, fproj, steps, n_class, ids=forced)[1], forced)


@pytest.mark.parametrize("H,W,Hm,Wm", [(3, 5, 2, 2), (7, 9, 2, 5), (6, 4, 5, 3)])
@pytest.mark.parametrize("with_acc", [False, True])
def test_moran_rectify_vs_grid_sample(H, W, Hm, Wm, with_acc):
    B = 2
    omap, plane = u("mr_o", (B, Hm, Wm), -1.5, 1.5), u("mr_p", (B, H, W))
    gx, gy = torch.linspace(-1.2, 1.1, W, dtype=torch.float64), torch.linspace(-1.0, 1.3, H, dtype=torch.float64)
    acc = u("mr_acc", (B, H, W), -0.6, 0.6) if with_acc else None
    o4 = omap[:, None]
    pooled = F.max_pool2d(F.relu(o4), 2, 1) - F.max_pool2d(F.relu(-o4), 2, 1)
    grid = torch.stack([gx[None, None, :].expand(B, H, W), gy[None, :, None].expand(B, H, W)], -1)
    off = F.grid_sample(pooled, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    a = off if acc is None else acc + off
    moved = torch.stack([grid[..., 0], grid[..., 1] + a], -1)
    rect = F.grid_sample(plane[:, None], moved, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    got_a, got_r = ref64.moran_rectify(omap, plane, gx, gy, acc)
    close(got_a, a, "moran_rectify offsets")
    close(got_r, rect, "moran_rectify plane")


@pytest.mark.parametrize("H,W,Ho,Wo", [(1, 1, 2, 3), (3, 5, 32, 100), (37, 141, 32, 100), (4, 6, 1, 1), (9, 7, 32, 64)])
def test_prep_vs_interpolate(H, W, Ho, Wo):
    img = u("prep_img", (2, 3, H, W), 0.0, 1.0)
    v = F.interpolate(img, (Ho, Wo), mode="bicubic", align_corners=False)
    close(ref64.gray_prep(img, Ho, Wo), 0.299 * v[:, 0] + 0.587 * v[:, 1] + 0.114 * v[:, 2], "gray_prep")
    norm, stn = ref64.aster_prep(img, Ho, Wo)
    close(norm, img * 2 - 1, "aster_prep norm")
    close(stn, F.interpolate(img * 2 - 1, (Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous(), "aster_prep stn")


def test_vl_pp_pool_and_label_vecs_vs_softmax():
    B, L, C, n_steps, ld, n_class = 2, 7, 6, 3, 5, 4
    scores, enc, wv, bv = u("pp_s", (B, L, ld), -3, 3), u("pp_e", (B, L, C)), u("pp_w", (n_class, C)), u("pp_b", (n_class,))
    p = F.softmax(scores[:, :, :n_steps], 1)
    close(ref64.vl_pp_pool(scores, enc, wv, bv, n_steps), F.linear(torch.einsum("bln,blc->bnc", p, enc), wv, bv), "vl_pp_pool")
    lg = u("lv", (B * L, ld), -3, 3)
    close(ref64.crnn_label_vecs(lg, n_class, B, L), F.softmax(lg[:, :n_class], -1).reshape(B, L, n_class).permute(0, 2, 1)[:, :, None].contiguous(), "label_vecs")


def test_ctc_greedy_and_vl_decode_rules():
    oh = lambda ids, n: F.one_hot(torch.tensor(ids), n).double()
    cls, length = ref64.ctc_greedy(oh([0, 2, 2, 0, 2, 3, 3, 0], 4), 4, 2, 4)
    assert cls.tolist() == [[2, 0, 0, 0], [2, 3, 0, 0]] and length.tolist() == [1, 2]
    cls, length = ref64.vl_decode(oh([[1, 0, 2, 0], [1, 2, 3, 0]], 4), 3)
    assert cls.tolist() == [[1, 0, 2], [1, 2, 3]] and length.tolist() == [2, 3]
