"""float64 references of the small hand-written kernels (csrc/tatt.hip, tbsrn.hip, cmm.hip, stn.hip, dpmn_layernorm_f32): plain torch on
the CPU, one function per operation, written from the operation's definition with elementwise arithmetic, matmul, exp / tanh / sqrt and
reductions only -- no torch.nn / torch.nn.functional call, so that a mistake in one of them cannot hide behind the library routine it
would share with the fp32 comparison.  tests/test_ref64.py pins each of them to an independent statement of the same operation.
Every function takes tensors of any float dtype and returns float64.

The second half holds the references of the small BACKWARD kernels (csrc/backward_pgrm.hip, backward.hip, the tail of conv_bwd.hip):
the gradient formulas written out by hand from the forward definition (plus torch.erf for the exact GELU), pinned in
tests/test_ref64.py to torch.autograd of an independent forward in double.  They take `dtype` (default float64): the same formula
evaluated with dtype=torch.float32 is the fp32 CPU evaluation that tests/test_gpu_small_backward.py derives its tolerances from.

The last part holds the references of the convolution family (tests/test_gpu_conv_family.py): forward, transposed forward, weight
gradient, data gradient and the BatchNorm statistics, as loops over the taps with one slice and one matmul / einsum per tap; then the
window-attention family (tests/test_gpu_attn_family.py): the multi-window shifted-window attention and its hand-written backward, alone
and behind the LayerNorm + q / kv projections -- roll as torch.roll on the token plane, window partition as a reshape, the region mask
from the Swin definition's nine labelled slices; from oracle.pgrm only drop_mask (the counter hash of the masks); and the recogniser
kernels (tests/test_gpu_recogniser_kernels.py): BiLSTM, the ASTER decoder step and beam search, the MORAN decoder and rectifier, the
prep resizes, the VisionLAN pooling -- the decoders either free running or replaying a kernel's own decisions."""
import math

import torch


def _d(x):
    return None if x is None else torch.as_tensor(x).detach().cpu().double()


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _softmax(s):
    """over the last axis"""
    e = torch.exp(s - s.amax(-1, keepdim=True))
    return e / e.sum(-1, keepdim=True)


def _ln(x, g, b, eps):
    """nn.LayerNorm over the last axis: biased variance, eps inside the root"""
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def bigru(gi, w_hh, b_hh, res=None, axis="w"):
    """Recurrence of a bidirectional one-layer nn.GRU on precomputed input projections.  gi NHWC (B, H, W, 2 * 3 * hid) = [forward: r z n
    | reverse: r z n] (b_ih folded); w_hh (2, 3 * hid, hid), b_hh (2, 3 * hid); sequences run along W (axis 'w', the B * H rows as batch)
    or along H (axis 'h', the B * W columns as batch).  Gate order r, z, n; n = tanh(gi_n + r * (W_hn h + b_hn)); h' = (1 - z) n + z h,
    h_0 = 0.  Returns NHWC (B, H, W, 2 * hid) = [forward | reverse] (+ res)."""
    gi, w_hh, b_hh, res = _d(gi), _d(w_hh), _d(b_hh), _d(res)
    hid = w_hh.shape[2]
    if axis == "h":
        gi = gi.transpose(1, 2)
    B, R, T, _ = gi.shape
    g = gi.reshape(B * R, T, 2, 3 * hid)
    out = gi.new_zeros(B * R, T, 2 * hid)
    for d in range(2):
        h = gi.new_zeros(B * R, hid)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gh = h @ w_hh[d].t() + b_hh[d]
            a = g[:, t, d]
            r = _sigmoid(a[:, :hid] + gh[:, :hid])
            z = _sigmoid(a[:, hid:2 * hid] + gh[:, hid:2 * hid])
            n = torch.tanh(a[:, 2 * hid:] + r * gh[:, 2 * hid:])
            h = (1.0 - z) * n + z * h
            out[:, t, d * hid:(d + 1) * hid] = h
    out = out.reshape(B, R, T, 2 * hid)
    if axis == "h":
        out = out.transpose(1, 2)
    return out if res is None else out + res


def _attention(q, k, v, nhead):
    """q (N, L, E), k / v (N, S, E), already projected -> (out (N, L, E), weights (N, nhead, L, S))"""
    N, L, E = q.shape
    S, d = k.shape[1], E // nhead
    qh = q.reshape(N, L, nhead, d).permute(0, 2, 1, 3)
    kh = k.reshape(N, S, nhead, d).permute(0, 2, 1, 3)
    vh = v.reshape(N, S, nhead, d).permute(0, 2, 1, 3)
    p = _softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d))
    return (p @ vh).permute(0, 2, 1, 3).reshape(N, L, E), p


def encoder_layer(src, pos, w12, nhead=4, eps=1e-5):
    """The one-layer TransformerEncoder of the TPInterpreter, post-norm: src (N, L, E), pos (L, E), w12 = [in_proj_weight (3E, E),
    in_proj_bias, out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight, norm1.bias,
    norm2.weight, norm2.bias].  The layer input is 2 * src; q = k = 2 * src + pos, v = 2 * src; ReLU feed-forward."""
    src, pos = _d(src), _d(pos)
    in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b = (_d(w) for w in w12)
    E = src.shape[-1]
    x = 2.0 * src
    qk = x + pos
    q = qk @ in_w[:E].t() + in_b[:E]
    k = qk @ in_w[E:2 * E].t() + in_b[E:2 * E]
    v = x @ in_w[2 * E:].t() + in_b[2 * E:]
    a, _ = _attention(q, k, v, nhead)
    y = _ln(x + a @ out_w.t() + out_b, n1_w, n1_b, eps)
    ff = torch.clamp(y @ l1_w.t() + l1_b, min=0.0) @ l2_w.t() + l2_b
    return _ln(y + ff, n2_w, n2_b, eps)


def cross_attn(q, k, v, nhead=4):
    """Softmax attention core of nn.MultiheadAttention on projected q (N, L, E), k / v (N, S, E): scores q . k / sqrt(E / nhead) per head
    -> (out (N, L, E), head-averaged weights (N, L, S))."""
    o, p = _attention(_d(q), _d(k), _d(v), nhead)
    return o, p.mean(1)


def add_layernorm64(x, res, g, b, g2=None, b2=None, acc=None, alpha=1.0, accumulate=False, eps=1e-5):
    """y = LN(x (+ res)) * g + b.  With g2 / b2: the second norm alpha * (LN(y) * g2 + b2), added to `acc` (accumulate) or replacing
    it.  Returns (y, acc_out or None)."""
    x, res, g, b, g2, b2, acc = _d(x), _d(res), _d(g), _d(b), _d(g2), _d(b2), _d(acc)
    y = _ln(x if res is None else x + res, g, b, eps)
    if g2 is None:
        return y, None
    o2 = alpha * _ln(y, g2, b2, eps)
    return y, (acc + o2 if accumulate else o2)


def gru_gate(gi, gh, h):
    """One GRU step from the two projections: gi, gh (R, 3H) = [r z n] (biases folded), h (R, H) -> h' (R, H)."""
    gi, gh, h = _d(gi), _d(gh), _d(h)
    H = h.shape[1]
    r = _sigmoid(gi[:, :H] + gh[:, :H])
    z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1.0 - z) * n + z * h


def tl_interp(inp, H, W):
    """Bilinear resize with align_corners=True of a one-row map: inp (N, Win, C) -> NHWC (N, H, W, C).  Output column x reads the source
    coordinate x (Win - 1) / (W - 1) (0 for W = 1); the single source row is repeated over H."""
    inp = _d(inp)
    N, Win, C = inp.shape
    out = inp.new_zeros(N, W, C)
    for x in range(W):
        sx = x * (Win - 1) / (W - 1) if W > 1 else 0.0
        x0 = min(int(math.floor(sx)), Win - 1)
        x1 = min(x0 + 1, Win - 1)
        f = sx - x0
        out[:, x] = (1.0 - f) * inp[:, x0] + f * inp[:, x1]
    return out[:, None].expand(N, H, W, C).contiguous()


def mha(qkv, B, L, heads, d, scale=None):
    """Self-attention core on packed rows: qkv (B * L, 3 * heads * d) = [q | k | v], head h at columns h * d of each third ->
    (B * L, heads * d).  scale defaults to 1 / sqrt(d)."""
    qkv = _d(qkv)
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    q, k, v = (qkv[:, i * heads * d:(i + 1) * heads * d].reshape(B, L, heads, d).permute(0, 2, 1, 3) for i in range(3))
    p = _softmax(q @ k.transpose(-1, -2) * scale)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * L, heads * d)


def layernorm_std(x, a2, b2, eps=1e-6):
    """a2 * (x - mean) / (std + eps) + b2 over the last axis: the UNBIASED standard deviation, eps added to the std."""
    x, a2, b2 = _d(x), _d(a2), _d(b2)
    C = x.shape[-1]
    d = x - x.sum(-1, keepdim=True) / C
    std = torch.sqrt((d * d).sum(-1, keepdim=True) / (C - 1))
    return a2 * d / (std + eps) + b2


def layernorm(x, w, b, eps=1e-5):
    """nn.LayerNorm over the last axis."""
    return _ln(_d(x), _d(w), _d(b), eps)


def se_gate(x, fc1_w, fc1_b, fc2_w, fc2_b):
    """Channel gate of the CMM: x (B, ..., C) channels-last; mean over the positions -> fc1 -> ReLU -> fc2 -> sigmoid -> x * gate + x."""
    x, fc1_w, fc1_b, fc2_w, fc2_b = _d(x), _d(fc1_w), _d(fc1_b), _d(fc2_w), _d(fc2_b)
    B, C = x.shape[0], x.shape[-1]
    pooled = x.reshape(B, -1, C).mean(1)
    hid = torch.clamp(pooled @ fc1_w.t() + fc1_b, min=0.0)
    gate = _sigmoid(hid @ fc2_w.t() + fc2_b).reshape((B,) + (1,) * (x.dim() - 2) + (C,))
    return x * gate + x


def maxpool_affine_relu(x, kh, kw, scale=None, shift=None):
    """MaxPool2d((kh, kw), stride (kh, kw)) over NHWC x (B, H, W, C); with scale / shift (C,) the per-channel affine and a ReLU are
    applied to every element BEFORE the maximum (a negative scale reverses the order of a window's elements)."""
    x, scale, shift = _d(x), _d(scale), _d(shift)
    if scale is not None:
        x = torch.clamp(x * scale + shift, min=0.0)
    B, H, W, C = x.shape
    return x.reshape(B, H // kh, kh, W // kw, kw, C).amax((2, 4))


# ====================================================================================================================
# backward kernels: every function below evaluates in `dtype` (float64: the reference; float32: the tolerance yardstick)
def _c(x, dtype):
    return None if x is None else torch.as_tensor(x).detach().cpu().to(dtype)


def _cdf(x):
    """standard normal CDF"""
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu(x, dtype=torch.float64):
    """exact (erf) GELU x Phi(x)"""
    x = _c(x, dtype)
    return x * _cdf(x)


def gelu_grad(x, dtype=torch.float64):
    """GELU'(x) = Phi(x) + x phi(x)"""
    x = _c(x, dtype)
    return _cdf(x) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def sk_select(cat, A, L, dtype=torch.float64):
    """V[m, c] = sum_g A[b, g, c] cat[m, g cg + c], b = m // L: cat (B L, G cg), A (B, G, cg) -> (B L, cg)"""
    cat, A = _c(cat, dtype), _c(A, dtype)
    B, G, cg = A.shape
    return (cat.reshape(B, L, G, cg) * A[:, None]).sum(2).reshape(B * L, cg)


def sk_select_bwd(cat, A, dV, L, rows_per_block=32, dtype=torch.float64):
    """Backward of sk_select for the cotangent dV (B L, cg): dcat[m, g cg + c] = A[b, g, c] dV[m, c]; dA[b, g, c] = sum over the image's
    tokens of cat[m, g cg + c] dV[m, c].  Returns (dcat (B L, G cg), dA (B, G, cg), parts (ceil(L / rows_per_block), B, G cg)): parts[k]
    is the share of dA of token rows [k rows_per_block, (k + 1) rows_per_block) of every image; they add up to dA."""
    cat, A, dV = _c(cat, dtype), _c(A, dtype), _c(dV, dtype)
    B, G, cg = A.shape
    dv = dV.reshape(B, L, 1, cg)
    prod = cat.reshape(B, L, G, cg) * dv
    dcat = (A[:, None] * dv).reshape(B * L, G * cg)
    parts = torch.stack([prod[:, r0:r0 + rows_per_block].sum(1).reshape(B, G * cg) for r0 in range(0, L, rows_per_block)])
    return dcat, prod.sum(1), parts


def sk_pool(partial, parts_per_image, L, dtype=torch.float64):
    """S[b] = sum of image b's partial column sums / L: partial (B parts_per_image, C) -> (B, C)"""
    partial = _c(partial, dtype)
    return partial.reshape(-1, parts_per_image, partial.shape[1]).sum(1) / L


def sk_gate(S, fc1_w, fc1_b, fc2_w, fc2_b, G, dtype=torch.float64):
    """A = softmax over g of (fc2 GELU(fc1 S + b1) + b2) viewed (B, G, C / G): S (B, C), fc1 (dmid, C), fc2 (C, dmid)"""
    S, fc1_w, fc1_b, fc2_w, fc2_b = (_c(t, dtype) for t in (S, fc1_w, fc1_b, fc2_w, fc2_b))
    z = gelu(S @ fc1_w.t() + fc1_b, dtype)
    logit = (z @ fc2_w.t() + fc2_b).reshape(S.shape[0], G, -1)
    return _softmax(logit.transpose(1, 2)).transpose(1, 2).contiguous()


def sk_gate_bwd(partial, parts_per_image, L, fc1_w, fc1_b, fc2_w, A, dA, dtype=torch.float64):
    """Backward of sk_gate(sk_pool(partial)) for the cotangent dA (B, G, cg), with the forward's A given.  Softmax over g:
    dlogit = A (dA - sum_g A dA); fc2: dfc2_w = dlogit^T Z, dfc2_b = sum_b dlogit, dZ = dlogit fc2_w; GELU: dzp = dZ GELU'(zp);
    fc1: dfc1_w = dzp^T S, dfc1_b = sum_b dzp, dS = dzp fc1_w.  Returns a dict with those five gradients (summed over the images) and
    the per-image rows wpart2 (B, C dmid + C) = [dfc2_w | dfc2_b], wpart1 (B, dmid C + dmid) = [dfc1_w | dfc1_b] they are the sums of."""
    fc1_w, fc1_b, fc2_w, A, dA = (_c(t, dtype) for t in (fc1_w, fc1_b, fc2_w, A, dA))
    S = sk_pool(partial, parts_per_image, L, dtype)
    B, C = S.shape
    zp = S @ fc1_w.t() + fc1_b
    Z = gelu(zp, dtype)
    dl = (A * (dA - (A * dA).sum(1, keepdim=True))).reshape(B, C)
    dzp = (dl @ fc2_w) * gelu_grad(zp, dtype)
    w2 = dl[:, :, None] * Z[:, None, :]            # (B, C, dmid)
    w1 = dzp[:, :, None] * S[:, None, :]           # (B, dmid, C)
    return {"dS": dzp @ fc1_w, "dfc2_w": w2.sum(0), "dfc2_b": dl.sum(0), "dfc1_w": w1.sum(0), "dfc1_b": dzp.sum(0),
            "wpart2": torch.cat([w2.reshape(B, -1), dl], 1), "wpart1": torch.cat([w1.reshape(B, -1), dzp], 1),
            "S": S, "zp": zp, "dl": dl, "dZ": dl @ fc2_w}


def sk_feats_grad(dout, feats, dS, L, dtype=torch.float64):
    """dfeats = dout + GELU'(feats) dS[b] / L: the gradient of feats (B L, C) when it feeds dout directly and S = mean_l GELU(feats)"""
    dout, feats, dS = _c(dout, dtype), _c(feats, dtype), _c(dS, dtype)
    B, C = dS.shape
    return dout + (gelu_grad(feats, dtype).reshape(B, L, C) * dS[:, None] / L).reshape(B * L, C)


def dwconv3x3_bwd(P, dg, w, gpre=None, in_gelu=False, out_gelu_bwd=False, mask=None, dtype=torch.float64):
    """Backward of the depthwise 3 x 3 cross-correlation with zero padding, y[b, c, i, j] = sum_k w[c, ky, kx] x[b, c, i + ky - 1, j + kx - 1]
    (+ bias), on planes P, dg (B, Ch, r, r), w (Ch, 3, 3).  The conv input is x = P, GELU(P) with in_gelu, times the dropout `mask`
    (0 or 1 / (1 - p)) when given.  With gpre (the conv output, whose GELU was the layer output) the incoming gradient is
    dy = dg GELU'(gpre), else dy = dg.  dw[c, k] = sum dy x shifted, db[c] = sum dy, dx[i, j] = sum_k dy[i - ky + 1, j - kx + 1] w[ky, kx];
    dP = dx (mask) (GELU'(P) with out_gelu_bwd: the gradient of the pre-activation).  Returns (dP, dw (Ch, 9), db (Ch))."""
    P, dg, w, gpre, mask = (_c(t, dtype) for t in (P, dg, w, gpre, mask))
    B, Ch, r, _ = P.shape
    w = w.reshape(Ch, 9)
    x = gelu(P, dtype) if in_gelu else P
    if mask is not None:
        x = x * mask.reshape(P.shape)
    dy = dg if gpre is None else dg * gelu_grad(gpre, dtype)
    xp, dyp = P.new_zeros(B, Ch, r + 2, r + 2), P.new_zeros(B, Ch, r + 2, r + 2)
    xp[:, :, 1:-1, 1:-1] = x
    dyp[:, :, 1:-1, 1:-1] = dy
    dw = torch.stack([(dy * xp[:, :, ky:ky + r, kx:kx + r]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)], 1)
    dx = torch.zeros_like(P)
    for ky in range(3):
        for kx in range(3):
            dx = dx + w[:, 3 * ky + kx].reshape(1, Ch, 1, 1) * dyp[:, :, 2 - ky:2 - ky + r, 2 - kx:2 - kx + r]
    if mask is not None:
        dx = dx * mask.reshape(P.shape)
    if out_gelu_bwd:
        dx = dx * gelu_grad(P, dtype)
    return dx, dw, dy.sum((0, 2, 3))


ACT_CODES = {"none": 0, "gelu": 1, "relu": 2, "leaky02": 3, "leaky001": 4, "mish": 5, "prelu": 6, "tanh": 7, "sigmoid": 8}


def act(x, code, slope=0.0, dtype=torch.float64):
    """The activation codes of the GEMM / conv epilogues: identity, exact GELU, ReLU, LeakyReLU(0.2), LeakyReLU(0.01),
    mish x tanh(softplus x), PReLU with one `slope`, tanh, sigmoid.  The leaky family is x for x > 0 and slope x otherwise."""
    x = _c(x, dtype)
    leaky = {2: 0.0, 3: 0.2, 4: 0.01, 6: slope}
    if code == 0:
        return x.clone()
    if code == 1:
        return gelu(x, dtype)
    if code in leaky:
        return torch.where(x > 0, x, leaky[code] * x)
    if code == 5:
        return x * torch.tanh(torch.log1p(torch.exp(x)))
    if code == 7:
        return torch.tanh(x)
    if code == 8:
        return _sigmoid(x)
    raise ValueError(code)


def act_grad(pre, code, slope=0.0, dtype=torch.float64):
    """d act(pre) / d pre.  At the kink pre == 0 the leaky family takes the NEGATIVE side's slope (the convention of torch.autograd for
    relu / leaky_relu / prelu).  mish' = tanh(sp) + pre (1 - tanh(sp)^2) sigmoid(pre), sp = softplus(pre)."""
    x = _c(pre, dtype)
    leaky = {2: 0.0, 3: 0.2, 4: 0.01, 6: slope}
    if code == 0:
        return torch.ones_like(x)
    if code == 1:
        return gelu_grad(x, dtype)
    if code in leaky:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, leaky[code]))
    if code == 5:
        th = torch.tanh(torch.log1p(torch.exp(x)))
        return th + x * (1.0 - th * th) * _sigmoid(x)
    if code == 7:
        return 1.0 - torch.tanh(x) ** 2
    if code == 8:
        s = _sigmoid(x)
        return s * (1.0 - s)
    raise ValueError(code)


def axpby(x, z, y, a, b, accumulate, dtype=torch.float64):
    """a x (+ b z) (+ y when accumulate)"""
    x, z, y = _c(x, dtype), _c(z, dtype), _c(y, dtype)
    v = a * x if z is None else a * x + b * z
    return y + v if accumulate else v


def rowsum_mod(x, mod, dtype=torch.float64):
    """out[j] = sum of the row sums of the rows r with r % mod == j: x (k mod, cols) -> (mod,)"""
    x = _c(x, dtype)
    return x.reshape(-1, mod, x.shape[1]).sum((0, 2))


def rows_reduce(part, NK, N, dtype=torch.float64):
    """rows of NK + N floats added over the rows: -> (dw (NK,), db (N,))"""
    part = _c(part, dtype)
    return part[:, :NK].sum(0), part[:, NK:NK + N].sum(0)


def colsum(dy, dtype=torch.float64):
    return _c(dy, dtype).sum(0)


def _shuffle2(c1):
    """NHWC (B, H, W, 12) -> NCHW (B, 3, 2 H, 2 W): out[b, c, Y, X] = c1[b, Y // 2, X // 2, 4 c + 2 (Y % 2) + X % 2] (PixelShuffle(2))"""
    B, H, W, _ = c1.shape
    return c1.reshape(B, H, W, 3, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 2 * H, 2 * W)


def _unshuffle2(g):
    B, _, Ho, Wo = g.shape
    return g.reshape(B, 3, Ho // 2, 2, Wo // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, Ho // 2, Wo // 2, 12)


def tail_elem(c1, wl, residuals, dtype=torch.float64):
    """PGRM tail: out = LeakyReLU_0.01(PixelShuffle2(c1)) wl[0] + sum_{i >= 1} residuals[i] wl[i] -- residuals[0] is SKIPPED (quirk Q11 of
    the source: the loop over the residuals starts at 1) and wl[0] weighs the shuffled branch.  c1 NHWC (B, H, W, 12), wl[i] (3, 2 H, 2 W),
    residuals[i] (B, 3, 2 H, 2 W)."""
    c1 = _c(c1, dtype)
    v = _shuffle2(c1)
    out = torch.where(v > 0, v, 0.01 * v) * _c(wl[0], dtype)
    for i in range(1, len(residuals)):
        out = out + _c(residuals[i], dtype) * _c(wl[i], dtype)
    return out


def tail_elem_bwd(dout, c1, wl, residuals, dtype=torch.float64):
    """Backward of tail_elem -> (dc1 NHWC, [dwl_i], [dres_i]); dres[0] is None (residual 0 takes no part).  The LeakyReLU slope at
    c1 == 0 is the negative side's 0.01."""
    dout, c1 = _c(dout, dtype), _c(c1, dtype)
    v = _shuffle2(c1)
    w0 = _c(wl[0], dtype)
    dc1 = _unshuffle2(dout * w0 * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, 0.01)))
    dwl = [(dout * torch.where(v > 0, v, 0.01 * v)).sum(0)]
    dres = [None]
    for i in range(1, len(residuals)):
        dwl.append((dout * _c(residuals[i], dtype)).sum(0))
        dres.append(dout * _c(wl[i], dtype))
    return dc1, dwl, dres


def se_gate_bwd(x, dg, fc1_w, fc1_b, fc2_w, fc2_b, dtype=torch.float64):
    """Backward of g = x (1 + w), w = sigmoid(fc2 relu(fc1 mean_p x + b1) + b2), x / dg (B, P, C): with D[b, c] = sum_p dg x,
    dlogit = D w (1 - w), dfc2 = dlogit^T h / sum_b dlogit, dh = (dlogit fc2_w) [h > 0], dfc1 = dh^T S / sum_b dh, dS = dh fc1_w,
    dx = dg (1 + w) + dS / P.  Returns (dx, dfc1_w, dfc1_b, dfc2_w, dfc2_b)."""
    x, dg, fc1_w, fc1_b, fc2_w, fc2_b = (_c(t, dtype) for t in (x, dg, fc1_w, fc1_b, fc2_w, fc2_b))
    B, P, C = x.shape
    S = x.sum(1) / P
    pre = S @ fc1_w.t() + fc1_b
    h = torch.clamp(pre, min=0.0)
    w = _sigmoid(h @ fc2_w.t() + fc2_b)
    dlog = (dg * x).sum(1) * w * (1.0 - w)
    dh = (dlog @ fc2_w) * (pre > 0).to(dtype)
    dx = dg * (1.0 + w)[:, None] + (dh @ fc1_w)[:, None] / P
    return dx, dh.t() @ S, dh.sum(0), dlog.t() @ h, dlog.sum(0)


def l1_loss(a, b, inv_count, dtype=torch.float64):
    """inv_count sum |a - b| -> (1,)"""
    return ((_c(a, dtype) - _c(b, dtype)).abs().sum() * inv_count).reshape(1)


def l1_loss_bwd(a, b, grad_scale, inv_count, extra_a=None, dtype=torch.float64):
    """da = grad_scale inv_count sign(a - b) (+ extra_a), db = -grad_scale inv_count sign(a - b).  At a tie a == b the subgradient
    taken is 0 -- sign(0) = 0, the convention of torch.sign and so of torch's own L1 loss backward."""
    a, b, extra_a = _c(a, dtype), _c(b, dtype), _c(extra_a, dtype)
    g = float(grad_scale) * inv_count * torch.sign(a - b)
    return (g if extra_a is None else g + extra_a), -g


# ====================================================================================================================
# GEMM family (csrc/gemm.hip and its bf16x3 twins, dpmn_gemm_tn_f32): written from each operation's definition; `dtype` as above
def linear(x, w, bias=None, res1=None, res2=None, act_code=0, slope=0.0, pro=None, dtype=torch.float64):
    """y = act(pro(x) w^T + bias) + res1 + res2 (the residuals AFTER the activation): x (M, K), w (N, K).  `pro`, the prologue on x:
    None; ("add", addv): x + addv; ("cat2", x2): the channel concatenation [x | x2]; ("ln", gamma, beta, eps): nn.LayerNorm over the
    row, two passes (mean, then the mean of the squared deviations)."""
    x, w, bias, res1, res2 = (_c(t, dtype) for t in (x, w, bias, res1, res2))
    if pro is not None and pro[0] == "add":
        x = x + _c(pro[1], dtype)
    elif pro is not None and pro[0] == "cat2":
        x = torch.cat([x, _c(pro[1], dtype)], 1)
    elif pro is not None and pro[0] == "ln":
        x = _ln(x, _c(pro[1], dtype), _c(pro[2], dtype), pro[3])
    elif pro is not None:
        raise ValueError(pro[0])
    y = x @ w.t()
    if bias is not None:
        y = y + bias
    y = act(y, act_code, slope, dtype)
    if res1 is not None:
        y = y + res1
    if res2 is not None:
        y = y + res2
    return y


def linear_drop(x, w, bias, res, mask_elem, mask_row, dtype=torch.float64):
    """y = res + ((x w^T + bias) mask_elem) mask_row: the Linear's output times the element mask, then the per-sample mask (each 0 or
    1 / (1 - p), already expanded to (M, N); None: that factor is off), the residual last -- the order of dpmn_dropout_f32."""
    y = linear(x, w, bias, dtype=dtype)
    if mask_elem is not None:
        y = y * _c(mask_elem, dtype)
    if mask_row is not None:
        y = y * _c(mask_row, dtype)
    return _c(res, dtype) + y


def sk_proj(cat, w, bias, rows=32, dtype=torch.float64):
    """feats = cat w^T + bias and partial[i] = sum of GELU(feats[m]) over the rows m in [rows i, rows i + rows) below M:
    -> (feats (M, C), partial (ceil(M / rows), C))"""
    feats = linear(cat, w, bias, dtype=dtype)
    g = gelu(feats, dtype)
    return feats, torch.stack([g[r0:r0 + rows].sum(0) for r0 in range(0, feats.shape[0], rows)])


def pointwise(g, w, bias, dtype=torch.float64):
    """z[b] = w g[b] + bias[:, None]: g (B, Ch, L), w (Ch, Ch)"""
    g, w, bias = _c(g, dtype), _c(w, dtype), _c(bias, dtype)
    return w @ g + bias[None, :, None]


def pointwise_wgrad(dz, g, dtype=torch.float64):
    """dw = sum_b dz[b] g[b]^T: the weight gradient of pointwise for the cotangent dz (B, Ch, L) -> (Ch, Ch)"""
    dz, g = _c(dz, dtype), _c(g, dtype)
    return (dz @ g.transpose(1, 2)).sum(0)


def gemm_tn(dy, x, dtype=torch.float64):
    """dW = dy^T x, db = column sums of dy: the nn.Linear weight / bias gradient for dy (M, N), x (M, K) -> ((N, K), (N,))"""
    dy, x = _c(dy, dtype), _c(x, dtype)
    return dy.t() @ x, dy.sum(0)


# ====================================================================================================================
# conv family (csrc/conv.hip, conv_body.h, conv_x3.hip, k_conv_wgrad of conv_bwd.hip, conv_wgrad_x3.hip): each written from the
# operation's definition -- a loop over the taps, a strided slice and one matmul / einsum per tap; `dtype` as above.  Activations are
# NHWC, weights in the nn.Conv2d (Cout, Cin, KH, KW) / nn.ConvTranspose2d (Cin, Cout, KH, KW) parameter layout.
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv_out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_input(segs, affine=None, pro=0, dtype=torch.float64):
    """What the conv multiplies: the channel concatenation of the NHWC segments, each through its own per-channel affine
    (affine[i] = (scale, shift) or None), then the input activation `pro` -- all BEFORE the zero padding, which so stays exactly 0."""
    xs = []
    for i, s in enumerate(segs):
        x = _c(s, dtype)
        if affine is not None and affine[i] is not None:
            x = x * _c(affine[i][0], dtype) + _c(affine[i][1], dtype)
        xs.append(x)
    return act(torch.cat(xs, 3), pro, dtype=dtype)


def _padded(x, ph, pw):
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + 2 * ph, W + 2 * pw, C)
    xp[:, ph:ph + H, pw:pw + W] = x
    return xp


def _tap(xp, ky, kx, Ho, Wo, stride, dil):
    """the padded input at the pixels tap (ky, kx) meets: rows ky dil + oy stride, oy < Ho"""
    return xp[:, ky * dil:ky * dil + (Ho - 1) * stride + 1:stride, kx * dil:kx * dil + (Wo - 1) * stride + 1:stride]


def _corr(x, w, stride, pad, dil):
    """y[b, oy, ox, co] = sum_{ky, kx, ci} x[b, oy stride + ky dil - pad_y, ox stride + kx dil - pad_x, ci] w[co, ci, ky, kx]"""
    (ph, pw), (KH, KW) = _pair(pad), w.shape[2:]
    Ho, Wo = conv_out_size(x.shape[1], KH, stride, ph, dil), conv_out_size(x.shape[2], KW, stride, pw, dil)
    xp = _padded(x, ph, pw)
    y = x.new_zeros(x.shape[0], Ho, Wo, w.shape[0])
    for ky in range(KH):
        for kx in range(KW):
            y = y + _tap(xp, ky, kx, Ho, Wo, stride, dil) @ w[:, :, ky, kx].t()
    return y


def _corr_t(x, w, stride, pad):
    """y[b, iy stride - pad + ky, ix stride - pad + kx, co] += x[b, iy, ix, ci] w[ci, co, ky, kx] (nn.ConvTranspose2d)"""
    (ph, pw), (KH, KW) = _pair(pad), w.shape[2:]
    B, H, W, _ = x.shape
    full = x.new_zeros(B, (H - 1) * stride + KH, (W - 1) * stride + KW, w.shape[1])
    for ky in range(KH):
        for kx in range(KW):
            full[:, ky:ky + (H - 1) * stride + 1:stride, kx:kx + (W - 1) * stride + 1:stride] += x @ w[:, :, ky, kx]
    return full[:, ph:full.shape[1] - ph, pw:full.shape[2] - pw]


def conv_epilogue(y, bias=None, epi=0, slope=0.0, res=None, pixel_shuffle=False, out_nchw=False, dtype=torch.float64):
    """bias, activation, residual -- in that order -- then the store form: PixelShuffle(2) as NHWC (B, 2 H, 2 W, C / 4), out[b, 2 y + i,
    2 x + j, c] = y[b, y, x, 4 c + 2 i + j], or NCHW."""
    if bias is not None:
        y = y + _c(bias, dtype)
    y = act(y, epi, slope, dtype)
    if res is not None:
        y = y + _c(res, dtype)
    if pixel_shuffle:
        B, H, W, C = y.shape
        y = y.reshape(B, H, W, C // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, C // 4)
    return y.permute(0, 3, 1, 2).contiguous() if out_nchw else y


def conv2d(segs, w, bias=None, stride=1, pad=0, dil=1, pro=0, epi=0, slope=0.0, affine=None, res=None, pixel_shuffle=False,
           out_nchw=False, dtype=torch.float64):
    """nn.Conv2d over conv_input(segs, affine, pro), then conv_epilogue.  w (Cout, Cin, KH, KW)."""
    y = _corr(conv_input(segs, affine, pro, dtype), _c(w, dtype), stride, pad, dil)
    return conv_epilogue(y, bias, epi, slope, res, pixel_shuffle, out_nchw, dtype)


def conv_transpose2d(segs, w, bias=None, stride=1, pad=0, pro=0, epi=0, slope=0.0, affine=None, res=None, dtype=torch.float64):
    """nn.ConvTranspose2d(k, stride, pad) -- (3, 1, 1) and (4, 2, 1) here -- over conv_input, then conv_epilogue.  w (Cin, Cout, KH, KW)."""
    y = _corr_t(conv_input(segs, affine, pro, dtype), _c(w, dtype), stride, pad)
    return conv_epilogue(y, bias, epi, slope, res, dtype=dtype)


def conv_stats(raw, dtype=torch.float64):
    """per-channel sum and sum of squares of the raw (pre-activation, bias included) NHWC output -> ((C,), (C,))"""
    raw = _c(raw, dtype)
    return raw.sum((0, 1, 2)), (raw * raw).sum((0, 1, 2))


def conv2d_wgrad(segs, dy, k, stride=1, pad=0, dil=1, pro=0, affine=None, dtype=torch.float64):
    """dW[co, ci, ky, kx] = sum_{b, oy, ox} dy[b, oy, ox, co] X[b, oy stride + ky dil - pad, ox stride + kx dil - pad, ci] with
    X = conv_input(segs, affine, pro): the weight gradient of conv2d for the cotangent dy (B, Ho, Wo, Cout) of the raw output."""
    x, dy = conv_input(segs, affine, pro, dtype), _c(dy, dtype)
    (KH, KW), (ph, pw) = _pair(k), _pair(pad)
    Ho, Wo = dy.shape[1], dy.shape[2]
    assert (Ho, Wo) == (conv_out_size(x.shape[1], KH, stride, ph, dil), conv_out_size(x.shape[2], KW, stride, pw, dil))
    xp = _padded(x, ph, pw)
    dw = x.new_zeros(dy.shape[3], x.shape[3], KH, KW)
    for ky in range(KH):
        for kx in range(KW):
            dw[:, :, ky, kx] = torch.einsum("bhwo,bhwi->oi", dy, _tap(xp, ky, kx, Ho, Wo, stride, dil))
    return dw


def conv_transpose2d_wgrad(segs, dy, k, stride=1, pad=0, pro=0, affine=None, dtype=torch.float64):
    """dW[ci, co, ky, kx] = sum_{b, iy, ix} X[b, iy, ix, ci] dy[b, iy stride - pad + ky, ix stride - pad + kx, co]: the weight gradient
    of conv_transpose2d (terms outside dy's plane do not exist)."""
    x, dy = conv_input(segs, affine, pro, dtype), _c(dy, dtype)
    (KH, KW), (ph, pw) = _pair(k), _pair(pad)
    B, H, W, _ = x.shape
    full = _padded(dy, ph, pw)
    assert full.shape[1] == (H - 1) * stride + KH and full.shape[2] == (W - 1) * stride + KW
    dw = x.new_zeros(x.shape[3], dy.shape[3], KH, KW)
    for ky in range(KH):
        for kx in range(KW):
            dw[:, :, ky, kx] = torch.einsum("bhwi,bhwo->io", x, full[:, ky:ky + (H - 1) * stride + 1:stride, kx:kx + (W - 1) * stride + 1:stride])
    return dw


def conv2d_dgrad(dy, w, in_hw, stride=1, pad=0, dil=1, c0=0, cs=None, dtype=torch.float64):
    """The adjoint of conv2d with respect to the conv's input, channels [c0, c0 + cs): dX[b, oy stride + ky dil - pad, ox stride + kx dil
    - pad, ci] += dy[b, oy, ox, co] w[co, c0 + ci, ky, kx] -> (B, Hin, Win, cs); input pixels no tap reaches keep 0."""
    dy, w = _c(dy, dtype), _c(w, dtype)
    cs = w.shape[1] - c0 if cs is None else cs
    (ph, pw), (KH, KW), (Hin, Win) = _pair(pad), w.shape[2:], in_hw
    Ho, Wo = dy.shape[1], dy.shape[2]
    assert (Ho, Wo) == (conv_out_size(Hin, KH, stride, ph, dil), conv_out_size(Win, KW, stride, pw, dil))
    dxp = dy.new_zeros(dy.shape[0], Hin + 2 * ph, Win + 2 * pw, cs)
    for ky in range(KH):
        for kx in range(KW):
            dxp[:, ky * dil:ky * dil + (Ho - 1) * stride + 1:stride, kx * dil:kx * dil + (Wo - 1) * stride + 1:stride] += dy @ w[:, c0:c0 + cs, ky, kx]
    return dxp[:, ph:ph + Hin, pw:pw + Win].contiguous()


def conv_transpose2d_dgrad(dy, w, stride=1, pad=0, c0=0, cs=None, dtype=torch.float64):
    """The adjoint of conv_transpose2d with respect to its input channels [c0, c0 + cs): dX[b, iy, ix, ci] = sum dy[b, iy stride - pad
    + ky, ix stride - pad + kx, co] w[c0 + ci, co, ky, kx] -- the correlation of dy with w read as (out = Cin, in = Cout)."""
    w = _c(w, dtype)
    cs = w.shape[0] - c0 if cs is None else cs
    return _corr(_c(dy, dtype), w[c0:c0 + cs], stride, pad, 1)


# ====================================================================================================================
# window-attention family (k_window_attn*, k_window_attn*_bwd* and the fused LayerNorm + q / kv + attention kernels): written from the
# definition of the shifted-window attention of one SwinTransformerBlock with several window sizes -- group g of n_groups takes channels
# [g cg, (g + 1) cg) of q (B, L, C) and of the k and v halves of kv (B, L, 2 C), two heads of D = cg / 2 channels each.  Per group: roll the
# (H, W) token plane by -shift along both axes, cut it into ws x ws windows (a reshape), attend within each window with
# logit = (q D^-0.5) . k + bias[head][n][m] + mask[window][n][m], softmax over the keys, attn_drop on the probabilities, P V.  The output
# stays in window-major order, the roll is NOT undone (quirk Q1): cat[b, win N + n, g cg + head D + d].  `dtype` as above.
def _wattn_src(H, W, ws, shift):
    """source raster token of every window-major slot: torch.roll of the token plane by -shift, then the window partition as a reshape"""
    plane = torch.roll(torch.arange(H * W).reshape(H, W), shifts=(-shift, -shift), dims=(0, 1))
    return plane.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1)


def _wattn_rel_index(ws):
    """(N, N): row of the (2 ws - 1)^2 bias table for query n and key m -- the pair's row and column offsets, each moved into
    [0, 2 ws - 2], the row offset counted in whole table rows"""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).reshape(2, -1)      # (2, N): i, j of a token
    rel = coords[:, :, None] - coords[:, None, :] + (ws - 1)
    return rel[0] * (2 * ws - 1) + rel[1]


def _wattn_labels(H, W, ws, shift):
    """(nW, N) region label of every token of the rolled frame: the frame is cut by the three row slices and the three column slices
    [0, -ws), [-ws, -shift), [-shift, end) and every one of the nine pieces gets its own label (the attention mask of the Swin
    transformer); only tokens with the same label attend to each other"""
    img = torch.zeros(H, W, dtype=torch.long)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    return img.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)


def _wattn_drop_index(B, G, g, L, N):
    """(B, nW, 2, N, N) element index of the attn_drop mask (include/dpmn_hip.h): ((((b G + g) 2 + head) L + window-major query token)
    N + key row in the window)"""
    import numpy as np
    b, win, h, n, m = np.meshgrid(np.arange(B), np.arange(L // N), np.arange(2), np.arange(N), np.arange(N), indexing="ij")
    return (((b * G + g) * 2 + h) * L + win * N + n) * N + m


def _wattn_group(q, kv, table, g, G, ws, shift, H, W, p_drop, seed, dtype):
    """one group's attention -> dict of the window-major operands Q, K, V (B, nW, 2, N, D), the logits S, the probabilities P, the
    dropout mask M (None: off), the output O (B, nW, 2, N, D), and src / idx / scale"""
    B, L, C = q.shape
    cg, N = C // G, ws * ws
    D, nW = cg // 2, L // N
    src = _wattn_src(H, W, ws, shift)

    def split(x, c0):
        return x[:, src, c0:c0 + cg].reshape(B, nW, N, 2, D).permute(0, 1, 3, 2, 4)
    Q, K, V = split(q, g * cg), split(kv, g * cg), split(kv, C + g * cg)
    scale = D ** -0.5
    idx = _wattn_rel_index(ws)
    bias = table.reshape(-1, 2)[idx.reshape(-1)].reshape(N, N, 2).permute(2, 0, 1)
    S = (Q * scale) @ K.transpose(-1, -2) + bias
    if shift > 0:      # the mask adds -100, not -inf: the operation's definition
        lab = _wattn_labels(H, W, ws, shift)
        S = S + torch.where(lab[:, :, None] == lab[:, None, :], 0.0, -100.0).to(dtype)[None, :, None]
    P = _softmax(S)                  # the denominator is over the undropped row
    M = None
    if p_drop > 0:
        from oracle.pgrm import drop_mask       # the counter hash of the masks, not attention arithmetic
        M = drop_mask(seed, _wattn_drop_index(B, G, g, L, N), p_drop).to(dtype)
    O = (P if M is None else P * M) @ V
    return {"Q": Q, "K": K, "V": V, "S": S, "P": P, "M": M, "O": O, "src": src, "idx": idx, "scale": scale}


def _wattn_merge(X, B, L):
    """(B, nW, 2, N, D) -> (B, L, 2 D) window-major"""
    return X.permute(0, 1, 3, 2, 4).reshape(B, L, -1)


def window_attn(q, kv, tables, windows, shifts, H, W, p_drop=0.0, seed=0, dtype=torch.float64, parts=None):
    """-> cat (B, L, C).  tables[g]: ((2 ws_g - 1)^2, 2).  parts: a list that receives every group's _wattn_group dict"""
    q, kv = _c(q, dtype), _c(kv, dtype)
    B, L, _ = q.shape
    G = len(windows)
    outs = []
    for g in range(G):
        r = _wattn_group(q, kv, _c(tables[g], dtype), g, G, windows[g], shifts[g], H, W, p_drop, seed, dtype)
        if parts is not None:
            parts.append(r)
        outs.append(_wattn_merge(r["O"], B, L))
    return torch.cat(outs, -1)


def window_attn_bwd(q, kv, tables, windows, shifts, H, W, dout, p_drop=0.0, seed=0, dtype=torch.float64, parts=None):
    """Backward of window_attn for the cotangent dout (B, L, C) of cat (window-major, as cat): with the dropout mask M,
    dP = dO V^T M, dS = P (dP - sum_m P dP), dQ = scale dS K, dK = scale dS^T Q, dV = (P M)^T dO; dq / dk / dv go back to the raster token
    the roll and the window partition took them from; dtable[idx[n, m], head] += dS[.., head, n, m] over images and windows.
    -> (dq (B, L, C), dkv (B, L, 2 C), [dtable_g ((2 ws_g - 1)^2, 2)]).  parts: receives every group's dict, with dP and dS added"""
    q, kv, dout = _c(q, dtype), _c(kv, dtype), _c(dout, dtype)
    B, L, C = q.shape
    G = len(windows)
    cg = C // G
    dq, dkv, dtables = torch.zeros_like(q), torch.zeros_like(kv), []
    for g in range(G):
        ws = windows[g]
        N = ws * ws
        r = _wattn_group(q, kv, _c(tables[g], dtype), g, G, ws, shifts[g], H, W, p_drop, seed, dtype)
        P, M = r["P"], r["M"]
        dO = dout[:, :, g * cg:(g + 1) * cg].reshape(B, L // N, N, 2, cg // 2).permute(0, 1, 3, 2, 4)
        dP = dO @ r["V"].transpose(-1, -2)
        if M is not None:
            dP = dP * M
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        dQ = r["scale"] * (dS @ r["K"])
        dK = r["scale"] * (dS.transpose(-1, -2) @ r["Q"])
        dV = (P if M is None else P * M).transpose(-1, -2) @ dO
        dq[:, r["src"], g * cg:(g + 1) * cg] = _wattn_merge(dQ, B, L)
        dkv[:, r["src"], g * cg:(g + 1) * cg] = _wattn_merge(dK, B, L)
        dkv[:, r["src"], C + g * cg:C + (g + 1) * cg] = _wattn_merge(dV, B, L)
        dt = torch.zeros((2 * ws - 1) ** 2, 2, dtype=dtype)
        dt.index_add_(0, r["idx"].reshape(-1), dS.sum((0, 1)).permute(1, 2, 0).reshape(N * N, 2))
        dtables.append(dt)
        if parts is not None:
            r.update(dP=dP, dS=dS, dO=dO)
            parts.append(r)
    return dq, dkv, dtables


def ln_qkv(tq, tkv, lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv, eps=1e-5, dtype=torch.float64):
    """q = Linear_q(LayerNorm_q(tq)) (B, L, C), kv = Linear_kv(LayerNorm_kv(tkv)) (B, L, 2 C): _ln and linear above"""
    B, L, C = tq.shape
    q = linear(_c(tq, dtype).reshape(B * L, C), wq, bq, pro=("ln", lnq_w, lnq_b, eps), dtype=dtype)
    kv = linear(_c(tkv, dtype).reshape(B * L, C), wkv, bkv, pro=("ln", lnkv_w, lnkv_b, eps), dtype=dtype)
    return q.reshape(B, L, C), kv.reshape(B, L, 2 * C)


def ln_qkv_window_attn(tq, tkv, ln, tables, windows, shifts, H, W, p_drop=0.0, seed=0, eps=1e-5, dtype=torch.float64, parts=None):
    """The fused operator: ln = (lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv) -> (cat, q, kv)"""
    q, kv = ln_qkv(tq, tkv, *ln, eps=eps, dtype=dtype)
    return window_attn(q, kv, tables, windows, shifts, H, W, p_drop, seed, dtype, parts), q, kv


def ln_qkv_window_attn_bwd(tq, tkv, ln, tables, windows, shifts, H, W, dout, p_drop=0.0, seed=0, eps=1e-5, dtype=torch.float64, parts=None):
    """Its backward twin: (dq, dkv, [dtable_g]) of the recomputed PROJECTED q / kv, not of the tokens"""
    q, kv = ln_qkv(tq, tkv, *ln, eps=eps, dtype=dtype)
    return window_attn_bwd(q, kv, tables, windows, shifts, H, W, dout, p_drop, seed, dtype, parts)


# ====================================================================================================================
# recogniser kernels (csrc/crnn.hip, aster.hip, moran.hip, visionlan.hip; tests/test_gpu_recogniser_kernels.py).  The widths (hidden
# size, attention width) are read from the operands, so tests/test_ref64.py pins these functions to nn.LSTM / nn.GRUCell / F.grid_sample
# / F.max_pool2d / F.interpolate / log_softmax + topk at small widths.  `gates`: a list that receives the sigmoid activations of the
# recurrences (the fixtures' gate-spread assertion).  The decoders that feed discrete decisions back take those decisions as an
# argument (the REPLAY of a kernel's own ids) or, without it, make them by the documented rule (free running).
def first_argmax(x):
    """index of the FIRST maximum along the last axis (the rule of k_moran_decode, k_ctc_greedy, k_vl_decode)"""
    n = x.shape[-1]
    at = torch.where(x == x.amax(-1, keepdim=True), torch.arange(n), torch.tensor(n))
    return at.amin(-1)


def bilstm(gx, w_hh, B, T, dtype=torch.float64, gates=None):
    """Recurrence of a bidirectional one-layer nn.LSTM on precomputed input projections: gx (B T, 8 H), row b T + t, columns [forward
    i f g o | backward i f g o] (both biases folded), w_hh (2, 4 H, H); h0 = c0 = 0, the backward direction starts at t = T - 1.
    -> (out (B T, 2 H) = [h_fwd | h_bwd], the cell state of both directions after their last step (2, B, H))"""
    gx, w_hh = _c(gx, dtype), _c(w_hh, dtype)
    H = w_hh.shape[2]
    g = gx.reshape(B, T, 2, 4 * H)
    out, cst = gx.new_zeros(B, T, 2 * H), gx.new_zeros(2, B, H)
    for d in range(2):
        h, c = gx.new_zeros(B, H), gx.new_zeros(B, H)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = g[:, t, d] + h @ w_hh[d].t()
            i, f, o = _sigmoid(a[:, :H]), _sigmoid(a[:, H:2 * H]), _sigmoid(a[:, 3 * H:])
            c = f * c + i * torch.tanh(a[:, 2 * H:3 * H])
            h = o * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
            if gates is not None:
                gates.append(torch.cat([i, f, o]).reshape(-1))
        cst[d] = c
    return out.reshape(B * T, 2 * H), cst


def gru_cell_table(e, ctx, wih_ctx, h, whh, bhh, gates=None):
    """nn.GRUCell whose input product is split: e = the embedding half (a row of the table E, b_ih folded) + ctx W_ih_ctx^T;
    r = sig(i_r + h_r), z = sig(i_z + h_z), n = tanh(i_n + r (W_hn h + b_hn)), h' = (1 - z) n + z h"""
    D = h.shape[1]
    gi = e + ctx @ wih_ctx.t()
    gh = h @ whh.t() + bhh
    r, z = _sigmoid(gi[:, :D] + gh[:, :D]), _sigmoid(gi[:, D:2 * D] + gh[:, D:2 * D])
    if gates is not None:
        gates.append(torch.cat([r, z]).reshape(-1))
    return (1.0 - z) * torch.tanh(gi[:, 2 * D:] + r * gh[:, 2 * D:]) + z * h


def additive_attention(sp, xp, feats, w, b):
    """e[r, t] = w . tanh(sp[r] + xp[r, t]) + b; alpha = softmax_t e; ctx = sum_t alpha feats[r, t] -> (e, alpha, ctx)"""
    e = (torch.tanh(xp + sp[:, None]) * w).sum(-1) + b
    alpha = _softmax(e)
    return e, alpha, (alpha[:, :, None] * feats).sum(1)


def aster_decode_step(w, feats, xproj, row_img, state, y_prev, n_class, dtype=torch.float64, gates=None):
    """One teacher-forced step of ASTER's attention decoder for R rows; row r attends to image row_img[r].  w: the fields of
    dpmn_aster_dec_weights (E has a row per class and the BOS row n_class).  -> dict sproj, e, alpha, ctx, state_out, logits"""
    w = {k: _c(v, dtype) for k, v in w.items()}
    feats, xproj, state = _c(feats, dtype), _c(xproj, dtype), _c(state, dtype)
    ri, yp = torch.as_tensor(row_img).long(), torch.as_tensor(y_prev).long()
    sproj = state @ w["s_w"].t() + w["s_b"]
    e, alpha, ctx = additive_attention(sproj, xproj[ri], feats[ri], w["w_w"], w["w_b"])
    snew = gru_cell_table(w["E"][yp], ctx, w["wih_ctx"], state, w["whh"], w["bhh"], gates)
    return {"sproj": sproj, "e": e, "alpha": alpha, "ctx": ctx, "state_out": snew, "logits": snew @ w["fc_w"][:n_class].t() + w["fc_b"][:n_class]}


def beam_select(cand, beam):
    """cand (B, beam n_class) -> the flat indices of the `beam` best of every image, best first; equal scores: the lower flat index"""
    return torch.sort(cand, dim=-1, descending=True, stable=True)[1][:, :beam]


def aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=None, dtype=torch.float64, gates=None):
    """ASTER's beam search (attention_recognition_head.py:187-268): per step the decoder step of every beam row, log-softmax, sequence
    score + log-probability, the `beam` best of an image's beam x n_class candidates, EOS erase (the sequence score of a beam that
    emitted EOS becomes -inf), state reorder.  At step 0 only beam row 0 of an image is live; the first input is the BOS row n_class of E.
    decisions = (sym, pred) (steps, R) as the kernel stores them (pred = the global predecessor row): the reference takes them instead of
    choosing.  -> dict sym, pred (steps, R), score (steps, R), cand [(R, n_class) per step], state (R, D), seq (R), ended [(R) bool per step]"""
    B, R = feats.shape[0], feats.shape[0] * beam
    row_img = torch.arange(R) // beam
    fd = _c(feats, dtype)
    state = fd.new_zeros(R, fd.shape[2])
    seq = fd.new_full((R,), float("-inf"))
    seq[::beam] = 0.0
    yprev = torch.full((R,), n_class, dtype=torch.long)
    res = {"sym": [], "pred": [], "score": [], "cand": [], "ended": []}
    for s in range(steps):
        st = aster_decode_step(w, feats, xproj, row_img, state, yprev, n_class, dtype, gates)
        x = st["logits"]
        m = x.amax(-1, keepdim=True)
        lse = m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))
        cand = seq[:, None] + (x - lse)
        if decisions is None:
            flat = beam_select(cand.reshape(B, beam * n_class), beam)
            k, c = flat // n_class, flat % n_class
            pred = (k + torch.arange(B)[:, None] * beam).reshape(R)
            sym = c.reshape(R)
        else:
            sym, pred = decisions[0][s].long(), decisions[1][s].long()
        score = cand[pred, sym]
        seq = torch.where(sym == eos, torch.full_like(score, float("-inf")), score)
        yprev, state = sym, st["state_out"][pred]
        for key, v in (("sym", sym), ("pred", pred), ("score", score), ("cand", cand), ("ended", sym == eos)):
            res[key].append(v)
    for key in ("sym", "pred", "score"):
        res[key] = torch.stack(res[key])
    res["state"], res["seq"] = state, seq
    return res


def moran_decode(w, feats, fproj, steps, n_class, ids=None, dtype=torch.float64, gates=None):
    """MORAN's greedy attention decoder (asrn_res.py:127-144): h0 = 0, first input row 0 of E; per step h2h(h), additive attention over
    fproj, GRU cell with the table row E[previous id + 1], generator, first-maximum arg-max fed back -- or `ids` (B, steps), the
    kernel's own decisions.  w: the fields of dpmn_moran_dec_weights.  -> (logits (B, steps, n_class), ids (B, steps))"""
    w = {k: _c(v, dtype) for k, v in w.items()}
    feats, fproj = _c(feats, dtype), _c(fproj, dtype)
    B = feats.shape[0]
    h = feats.new_zeros(B, feats.shape[2])
    y = torch.zeros(B, dtype=torch.long)
    logits, out_ids = [], []
    for s in range(steps):
        ps = h @ w["h2h_w"].t() + w["h2h_b"]
        _, _, ctx = additive_attention(ps, fproj, feats, w["score_w"], 0.0)
        h = gru_cell_table(w["E"][y], ctx, w["wih_ctx"], h, w["whh"], w["bhh"], gates)
        lg = h @ w["gen_w"][:n_class].t() + w["gen_b"][:n_class]
        best = first_argmax(lg) if ids is None else torch.as_tensor(ids)[:, s].long()
        y = best + 1
        logits.append(lg)
        out_ids.append(best)
    return torch.stack(logits, 1), torch.stack(out_ids, 1)


def _pool2x2s1(x):
    """MaxPool2d(2, 1) of (B, H, W)"""
    return torch.maximum(torch.maximum(x[:, :-1, :-1], x[:, :-1, 1:]), torch.maximum(x[:, 1:, :-1], x[:, 1:, 1:]))


def grid_sample_bilinear(img, cx, cy):
    """F.grid_sample(bilinear, zeros padding, align_corners=False) of planes img (B, h, w) at normalised coordinates cx, cy (B, H, W):
    pixel = ((coord + 1) size - 1) / 2, the four neighbours weighted, neighbours outside the plane count as zero"""
    B, h, w = img.shape
    fx, fy = ((cx + 1.0) * w - 1.0) / 2.0, ((cy + 1.0) * h - 1.0) / 2.0
    x0, y0 = torch.floor(fx), torch.floor(fy)
    out = torch.zeros_like(fx)
    bi = torch.arange(B)[:, None, None].expand(fx.shape)
    for dy in (0, 1):
        for dx in (0, 1):
            px, py = x0 + dx, y0 + dy
            wgt = (fx - x0 if dx else (x0 + 1.0) - fx) * (fy - y0 if dy else (y0 + 1.0) - fy)
            ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            v = img[bi, py.clamp(0, h - 1).long(), px.clamp(0, w - 1).long()]
            out = out + torch.where(ok, v * wgt, torch.zeros_like(v))
    return out


def moran_rectify(omap, plane, grid_x, grid_y, acc=None, dtype=torch.float64):
    """One pass of MORN behind its offset head (morn.py:63-82): offsets = pool(relu(o)) - pool(relu(-o)) with MaxPool2d(2, 1) of omap
    (B, Hm, Wm), sampled on the identity grid (grid_x (W), grid_y (H)), added to the running offsets `acc` (B, H, W); the plane
    (B, H, W) is then sampled at (grid_x, grid_y + offsets).  -> (accumulated offsets, rectified plane), both (B, H, W)"""
    o, p, gx, gy, acc = _c(omap, dtype), _c(plane, dtype), _c(grid_x, dtype), _c(grid_y, dtype), _c(acc, dtype)
    B, H, W = p.shape
    pooled = _pool2x2s1(o.clamp(min=0.0)) - _pool2x2s1((-o).clamp(min=0.0))
    cx, cy = gx[None, None, :].expand(B, H, W), gy[None, :, None].expand(B, H, W)
    off = grid_sample_bilinear(pooled, cx, cy)
    a = off if acc is None else acc + off
    return a, grid_sample_bilinear(p, cx, cy + a)


def _resize_matrix(n_in, n_out, mode, dtype):
    """(n_out, n_in) interpolation matrix of one axis.  'bicubic': torch's upsample_bicubic2d, align_corners=False, A = -0.75, source
    index (dst + 0.5) in / out - 0.5, taps clamped to the plane; 'linear_ac': bilinear with align_corners=True, source dst (in - 1) / (out - 1)"""
    dst = torch.arange(n_out, dtype=dtype)
    M = torch.zeros(n_out, n_in, dtype=dtype)
    rows = torch.arange(n_out)
    if mode == "bicubic":
        real = (torch.tensor(float(n_in), dtype=dtype) / n_out) * (dst + 0.5) - 0.5
        i0 = torch.floor(real)
        t = real - i0
        A = -0.75
        x1, x2 = t + 1.0, 1.0 - t
        x3 = x2 + 1.0
        wts = [((A * x1 - 5.0 * A) * x1 + 8.0 * A) * x1 - 4.0 * A, ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0,
               ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A]
        for k, wk in enumerate(wts):
            M.index_put_((rows, (i0.long() - 1 + k).clamp(0, n_in - 1)), wk, accumulate=True)
        return M
    scale = torch.tensor(float(n_in - 1), dtype=dtype) / (n_out - 1) if n_out > 1 else torch.tensor(0.0, dtype=dtype)
    real = scale * dst
    i0 = real.long().clamp(max=n_in - 1)
    l1 = real - i0.to(dtype)
    M.index_put_((rows, i0), 1.0 - l1, accumulate=True)
    M.index_put_((rows, (i0 + 1).clamp(max=n_in - 1)), l1, accumulate=True)
    return M


def gray_prep(img, Ho, Wo, dtype=torch.float64):
    """parse_crnn_data / parse_moran_data: bicubic resize of channels 0..2 of img (B, >= 3, H, W) to Ho x Wo, ITU-601 luma -> (B, Ho, Wo)"""
    x = _c(img, dtype)[:, :3]
    My, Mx = _resize_matrix(x.shape[2], Ho, "bicubic", dtype), _resize_matrix(x.shape[3], Wo, "bicubic", dtype)
    v = My @ x @ Mx.t()
    return (0.299 * v[:, 0] + 0.587 * v[:, 1]) + 0.114 * v[:, 2]


def aster_prep(img, Hs, Ws, dtype=torch.float64):
    """parse_aster_data (x 2 - 1) -> (normalised (B, 3, H, W), its bilinear align_corners=True resize to Hs x Ws as NHWC (B, Hs, Ws, 3))"""
    x = _c(img, dtype)[:, :3] * 2.0 - 1.0
    My, Mx = _resize_matrix(x.shape[2], Hs, "linear_ac", dtype), _resize_matrix(x.shape[3], Ws, "linear_ac", dtype)
    return x, (My @ x @ Mx.t()).permute(0, 2, 3, 1)


def vl_pp_pool(scores, enc, w_vrm, b_vrm, n_steps, dtype=torch.float64):
    """PP_layer + Prediction of VisionLAN: scores (B, L, ld >= n_steps), enc (B, L, C): p = softmax over the positions of scores[b, :, n],
    g = sum_l p_l enc[b, l], logits[b, n] = g W^T + bias -> (B, n_steps, n_class)"""
    s, enc, wv, bv = _c(scores, dtype), _c(enc, dtype), _c(w_vrm, dtype), _c(b_vrm, dtype)
    p = _softmax(s[:, :, :n_steps].transpose(1, 2))
    return (p @ enc) @ wv.t() + bv


def crnn_label_vecs(logits, n_class, B, T, dtype=torch.float64):
    """softmax over the first n_class columns of the rows b T + t of logits (B T, ld) -> (B, n_class, 1, T)"""
    p = _softmax(_c(logits, dtype)[:, :n_class])
    return p.reshape(B, T, n_class).permute(0, 2, 1).reshape(B, n_class, 1, T)


def ctc_greedy(logits, n_class, B, T):
    """strLabelConverter.decode(raw=False) after the first-maximum arg-max: repeats collapsed, blanks (class 0) dropped
    -> (cls (B, T) padded with 0, length (B))"""
    best = first_argmax(torch.as_tensor(logits)[:, :n_class]).reshape(B, T).tolist()
    cls, length = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n, prev = 0, -1
        for c in best[b]:
            if c != 0 and c != prev:
                cls[b, n] = c
                n += 1
            prev = c
        length[b] = n
    return cls, length


def vl_decode(logits, max_len):
    """MLM_VRM.forward 107-126: first-maximum arg-max of the first max_len steps of logits (B, n_steps, n_class); length = the first
    step that reads class 0, + 1, else max_len -> (cls (B, max_len), length (B))"""
    cls = first_argmax(torch.as_tensor(logits)[:, :max_len]).to(torch.int32)
    length = torch.full((cls.shape[0],), max_len, dtype=torch.int32)
    for b in range(cls.shape[0]):
        hit = (cls[b] == 0).nonzero()
        if hit.numel():
            length[b] = int(hit[0]) + 1
    return cls, length
