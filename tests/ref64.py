"""float64 references of the small hand-written kernels (csrc/tatt.hip, tbsrn.hip, cmm.hip, stn.hip, dpmn_layernorm_f32): plain torch on
the CPU, one function per operation, written from the operation's definition with elementwise arithmetic, matmul, exp / tanh / sqrt and
reductions only -- no torch.nn / torch.nn.functional call, so that a mistake in one of them cannot hide behind the library routine it
would share with the fp32 comparison.  tests/test_ref64.py pins each of them to an independent statement of the same operation.
Every function takes tensors of any float dtype and returns float64."""
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
