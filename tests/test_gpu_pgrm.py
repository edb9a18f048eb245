"""GPU parity: every PGRM kernel and the native PGRM forward vs the CPU oracle (oracle/pgrm.py),
called through the C ABI (dpmn_amd.ops / dpmn_amd.model.pgrm).  fp32, tolerance stated per test.
Run on the MI355X box:  python -m pytest tests -m gpu
"""
import pytest
import torch
import torch.nn.functional as F

from dpmn_amd.utils import synth
from helpers import load_golden, sd_from_manifest, t, assert_close

pytestmark = pytest.mark.gpu

ATOL = 1e-4   # fp32 MFMA (k-ordered fma chain) vs fp32 CPU; activations are O(1)
RTOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def cu(sd, dev):
    return {k: v.to(dev).contiguous() for k, v in sd.items()}


def u(name, shape, lo=-1.0, hi=1.0, seed=40):
    return synth.uniform(name, shape, lo, hi, seed)


# ------------------------------------------------------------------------------ GEMM family
@pytest.mark.parametrize("M,N,K", [(128, 96, 96), (1000, 192, 96), (256, 384, 96), (192, 96, 384), (64, 96, 32),
                                   (130, 64, 64), (64, 100, 128), (4096, 192, 192)])
def test_linear(dev, M, N, K):
    from dpmn_amd import ops
    x, w, b = u("x", (M, K)), u("w", (N, K), -0.2, 0.2), u("b", (N,))
    r1, r2 = u("r1", (M, N)), u("r2", (M, N))
    ref = F.gelu(F.linear(x, w, b)) + r1 + r2
    got = ops.linear(x.to(dev), w.to(dev), b.to(dev), r1.to(dev), r2.to(dev), act="gelu")
    assert_close(got, ref, ATOL, RTOL, "linear %s" % ((M, N, K),))
    got = ops.linear(x.to(dev), w.to(dev))
    assert_close(got, F.linear(x, w), ATOL, RTOL, "linear nobias")


@pytest.mark.parametrize("K,N", [(96, 96), (96, 192), (96, 384), (192, 384), (64, 64)])
def test_ln_linear(dev, K, N):
    from dpmn_amd import ops
    M = 320
    x = u("x", (M, K), -2, 3)
    g, be = u("g", (K,), 0.5, 1.5), u("be", (K,))
    w, b = u("w", (N, K), -0.2, 0.2), u("b", (N,))
    ref = F.linear(F.layer_norm(x, (K,), g, be), w, b)
    got = ops.ln_linear(x.to(dev), g.to(dev), be.to(dev), w.to(dev), b.to(dev))
    assert_close(got, ref, ATOL, RTOL, "ln_linear")
    got = ops.ln_linear(x.to(dev), g.to(dev), be.to(dev), w.to(dev), b.to(dev), act="gelu")
    assert_close(got, F.gelu(ref), ATOL, RTOL, "ln_linear gelu")


@pytest.mark.parametrize("M", [4096, 4160, 6144, 12288])
@pytest.mark.parametrize("K,N", [(96, 96), (96, 192), (96, 384), (32, 96), (64, 192), (128, 192), (96, 100)])
def test_whole_k_gemm_dispatch_interior_and_edge_tiles(dev, M, K, N):
    """Every epilogue instantiation of the whole-K GEMM (predicate-free interior tiles with straight-line bias / GELU / one or
    two residuals vs the generic edge path: M not a multiple of 64, N not a multiple of 96) against torch on the same data."""
    from dpmn_amd import ops
    x, w, b = u("x", (M, K)), u("w", (N, K), -0.2, 0.2), u("b", (N,))
    r1, r2 = u("r1", (M, N)), u("r2", (M, N))
    xd, wd, bd, r1d, r2d = (t_.to(dev) for t_ in (x, w, b, r1, r2))
    base = F.linear(x, w, b)
    assert_close(ops.linear(xd, wd, bd), base, ATOL, RTOL, "bias")
    assert_close(ops.linear(xd, wd), F.linear(x, w), ATOL, RTOL, "no bias")
    assert_close(ops.linear(xd, wd, bd, act="gelu"), F.gelu(base), ATOL, RTOL, "bias + gelu")
    assert_close(ops.linear(xd, wd, bd, r1d), base + r1, ATOL, RTOL, "bias + res1")
    assert_close(ops.linear(xd, wd, bd, r1d, r2d), base + r1 + r2, ATOL, RTOL, "bias + res1 + res2")
    assert_close(ops.linear(xd, wd, None, r1d), F.linear(x, w) + r1, ATOL, RTOL, "res1 only")
    if K == 96:
        g, be = u("g", (K,), 0.5, 1.5), u("be", (K,))
        ref = F.linear(F.layer_norm(x, (K,), g, be), w, b)
        assert_close(ops.ln_linear(xd, g.to(dev), be.to(dev), wd, bd), ref, ATOL, RTOL, "ln + linear")
        assert_close(ops.ln_linear(xd, g.to(dev), be.to(dev), wd, bd, act="gelu"), F.gelu(ref), ATOL, RTOL, "ln + linear + gelu")


@pytest.mark.parametrize("M,N,K", [(6144, 96, 384), (6200, 96, 384), (4096, 100, 192), (64, 96, 256)])
def test_k_loop_gemm_residual_epilogues(dev, M, N, K):
    from dpmn_amd import ops
    x, w, b, r1 = u("x", (M, K)), u("w", (N, K), -0.2, 0.2), u("b", (N,)), u("r1", (M, N))
    xd, wd, bd, r1d = (t_.to(dev) for t_ in (x, w, b, r1))
    assert_close(ops.linear(xd, wd, bd, r1d), F.linear(x, w, b) + r1, ATOL, RTOL, "k-loop bias + res1")
    assert_close(ops.linear(xd, wd, bd, act="gelu"), F.gelu(F.linear(x, w, b)), ATOL, RTOL, "k-loop bias + gelu")
    assert_close(ops.linear(xd, wd), F.linear(x, w), ATOL, RTOL, "k-loop plain")


def test_add_linear(dev):
    from dpmn_amd import ops
    x, a = u("x", (200, 64)), u("a", (200, 64))
    w, b = u("w", (64, 64), -0.2, 0.2), u("b", (64,))
    got = ops.add_linear(x.to(dev), a.to(dev), w.to(dev), b.to(dev))
    assert_close(got, F.linear(x + a, w, b), ATOL, RTOL, "add_linear")


def test_cat2_linear(dev):
    from dpmn_amd import ops
    x1, x2 = u("x1", (300, 64)), u("x2", (300, 64))
    w, b = u("w", (192, 128), -0.2, 0.2), u("b", (192,))
    got = ops.cat2_linear(x1.to(dev), x2.to(dev), w.to(dev), b.to(dev))
    assert_close(got, F.linear(torch.cat([x1, x2], 1), w, b), ATOL, RTOL, "cat2_linear")


def test_pointwise(dev):
    from dpmn_amd import ops
    B, L, Ch = 3, 1024, 384
    g = u("g", (B, L, Ch))
    w, b = u("w", (Ch, Ch), -0.1, 0.1), u("b", (Ch,))
    ref = (torch.einsum("oc,bcs->bos", w, g.reshape(B, Ch, L)) + b[None, :, None]).reshape(B, L, Ch)
    got = ops.pointwise(g.to(dev), w.to(dev), b.to(dev))
    assert_close(got, ref, ATOL, RTOL, "pointwise")


def test_kernel_profile_hooks_time_tagged_launches(dev):
    """bench.py's roofline timing (include/dpmn_hip.h dpmn_profile_*): while armed, the library brackets each launch of an
    armed kernel family with HIP events on its stream and reports launches, time and the algorithmic FLOPs / bytes."""
    from dpmn_amd import _abi, ops
    g, w, b = u("g", (2, 1024, 384)).to(dev), u("w", (384, 384), -0.1, 0.1).to(dev), u("b", (384,)).to(dev)
    x, wl = u("x", (2048, 96)).to(dev), u("wl", (96, 96), -0.1, 0.1).to(dev)
    ops.pointwise(g, w, b)
    assert "k_gemm_pw" in _abi.profile_tags() and "k_conv_igemm<128,128>" in _abi.profile_tags()
    _abi.profile_begin(["k_gemm_pw"], max_launches=3)
    for _ in range(5):                      # only the first 3 launches fit the record
        ops.pointwise(g, w, b)
    ops.linear(x, wl)                       # another family: not armed, not recorded
    torch.cuda.synchronize()
    rows = _abi.profile_end()
    assert len(rows) == 1 and rows[0]["kernel"] == "k_gemm_pw" and rows[0]["launches"] == 3
    assert 3e-3 < rows[0]["total_ms"] < 15.0
    assert rows[0]["flops"] == 3 * 2.0 * 384 * 384 * 1024 * 2
    assert rows[0]["bytes"] == 3 * 4.0 * (2 * 2 * 384 * 1024 + 384 * 384 + 384)
    ops.pointwise(g, w, b)                  # disarmed: nothing recorded
    torch.cuda.synchronize()
    assert _abi.profile_end() == []
    _abi.profile_begin(None)                # every family
    ops.pointwise(g, w, b)
    ops.linear(x, wl)
    torch.cuda.synchronize()
    assert {r["kernel"] for r in _abi.profile_end()} == {"k_gemm_pw", "k_gemm_wstat|rowreg"}
    assert _abi.lib.dpmn_profile_begin(1, 0) != 0        # rejected loudly


# ------------------------------------------------------------------------------ PGRM pieces
def test_patch_embed(dev):
    from dpmn_amd import ops
    from oracle import pgrm as o
    B = 3
    sd = {"patch_embed.proj.weight": u("pw", (96, 3, 2, 2)), "patch_embed.proj.bias": u("pb", (96,)),
          "patch_embed.norm.weight": u("nw", (96,), 0.5, 1.5), "patch_embed.norm.bias": u("nb", (96,))}
    img = u("img", (B, 3, 32, 128), 0, 1)
    ref = o.patch_embed(img, sd, 2)
    d = cu(sd, dev)
    got = ops.patch_embed_ln(img.to(dev), d["patch_embed.proj.weight"], d["patch_embed.proj.bias"],
                             d["patch_embed.norm.weight"], d["patch_embed.norm.bias"], 2)
    assert_close(got, ref, ATOL, RTOL, "patch_embed")
    # with fused prior_fusion on a uint8-valued 2-channel text prior (quirk Q6)
    pfw, pfb = u("pfw", (3, 2, 3, 3), -0.3, 0.3), u("pfb", (3,))
    prior = torch.floor(u("prior", (B, 2, 32, 128), 0, 256))
    ref = o.patch_embed(F.conv2d(prior, pfw, pfb, padding=1), sd, 2)
    got = ops.patch_embed_ln(prior.to(dev), d["patch_embed.proj.weight"], d["patch_embed.proj.bias"],
                             d["patch_embed.norm.weight"], d["patch_embed.norm.bias"], 2, pfw.to(dev), pfb.to(dev))
    assert_close(got, ref, 2e-4, RTOL, "patch_embed + prior_fusion")
    # pos_drop in the epilogue / on the backward's load == a dropout launch behind / in front of the plain kernel (bitwise)
    from dpmn_amd import _abi
    w4 = [d["patch_embed.proj.weight"], d["patch_embed.proj.bias"], d["patch_embed.norm.weight"], d["patch_embed.norm.bias"]]
    seed = 0x1234567890ABCDEF % (2 ** 62)
    for im, pf in ((img.to(dev), (None, None)), (prior.to(dev), (pfw.to(dev), pfb.to(dev)))):
        plain = ops.patch_embed_ln(im, *w4, 2, *pf)
        fused = ops.patch_embed_ln(im, *w4, 2, *pf, p_drop=0.1, seed=seed)
        two = ops.dropout(plain.clone(), 0.1, seed)
        assert torch.equal(fused, two) and not torch.equal(fused, plain)
        M = plain.shape[0] * plain.shape[1]
        dtok = u("dtok", (M, 96), -1, 1).to(dev)
        outs = []
        for fused_bwd in (True, False):
            dconv, patches = torch.empty(M, 96, device=dev), torch.empty(M, 16, device=dev)
            lnp = torch.empty((M + 63) // 64, 192, device=dev)
            dt = dtok if fused_bwd else ops.dropout(dtok.clone(), 0.1, seed)
            _abi.check(_abi.lib.dpmn_patch_embed_bwd_det_drop_f32(_abi.dptr(im), im.shape[1], _abi.dptr(pf[0], True), _abi.dptr(pf[1], True), _abi.dptr(w4[0]),
                                                                  _abi.dptr(w4[1]), _abi.dptr(w4[2]), _abi.dptr(dt), _abi.dptr(dconv), _abi.dptr(patches),
                                                                  lnp.data_ptr(), B, 32, 128, 96, 0.1 if fused_bwd else 0.0, seed, _abi.stream()))
            outs.append((dconv, patches, lnp))
        assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("tag,shifts", [("shift0", [0, 0, 0]), ("shifted", [1, 2, 4])])
def test_window_attention_vs_oracle_and_golden(dev, tag, shifts):
    from dpmn_amd import ops
    from oracle import pgrm as o
    g = load_golden("wattn_" + tag)
    sd = sd_from_manifest(g["manifest"], 21)
    B, H, W, C = 1, 16, 64, 96
    xq = synth.uniform("wa_xq", (B, H, W, C), -1, 1, 6).reshape(B, H * W, C)
    xkv = synth.uniform("wa_xkv", (B, H, W, C), -1, 1, 6).reshape(B, H * W, C)
    q = F.linear(xq, sd["q.weight"], sd["q.bias"])
    kv = F.linear(xkv, sd["kv.weight"], sd["kv.bias"])
    tables = [sd["relative_position_bias_table_%d" % i].to(dev) for i in range(3)]
    got = ops.window_attn(q.to(dev).contiguous(), kv.to(dev).contiguous(), tables, [2, 4, 8], shifts, 2, H, W)
    assert_close(got, t(g["cat"]), ATOL, RTOL, "window attention vs reference golden " + tag)
    ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sd, "", H, W, [2, 4, 8], shifts, 2)
    assert_close(got, ref, ATOL, RTOL, "window attention vs oracle " + tag)


@pytest.mark.parametrize("B,shifts", [(1, [0, 0, 0]), (3, [1, 2, 4]), (5, [0, 0, 0]), (48, [1, 2, 4])])
def test_fused_ln_qkv_window_attention_vs_oracle(dev, B, shifts):
    """The fused LayerNorm + q/kv projection + window attention kernel (attn_fused.hip: q and kv never reach HBM) against the
    oracle composed from the same pieces (torch LayerNorm / Linear restating pgrm.py:322-323, 188, 194 + the pinned
    window_attention_core), and -- at the golden's shapes -- through it against the reference's own `cat` tensor."""
    from dpmn_amd import ops
    from oracle import pgrm as o
    from helpers import record, max_abs_err
    H, W, C = 16, 64, 96
    g = load_golden("wattn_shift0" if shifts[0] == 0 else "wattn_shifted")
    sd = sd_from_manifest(g["manifest"], 21)
    lnq_w, lnq_b = u("lnq_w", (C,), 0.5, 1.5), u("lnq_b", (C,), -0.5, 0.5)
    lnk_w, lnk_b = u("lnk_w", (C,), 0.5, 1.5), u("lnk_b", (C,), -0.5, 0.5)
    tq, tkv = u("f_tq%d" % B, (B, H * W, C), -2, 3), u("f_tkv%d" % B, (B, H * W, C), -3, 2)
    assert ops.ln_qkv_window_attn_supported(C, [2, 4, 8], 2, H, W)
    q = F.linear(F.layer_norm(tq, (C,), lnq_w, lnq_b), sd["q.weight"], sd["q.bias"])
    kv = F.linear(F.layer_norm(tkv, (C,), lnk_w, lnk_b), sd["kv.weight"], sd["kv.bias"])
    ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sd, "", H, W, [2, 4, 8], shifts, 2)
    d = cu(sd, dev)
    tables = [d["relative_position_bias_table_%d" % i] for i in range(3)]
    got = ops.ln_qkv_window_attn(tq.to(dev), tkv.to(dev), lnq_w.to(dev), lnq_b.to(dev), lnk_w.to(dev), lnk_b.to(dev), d["q.weight"],
                                 d["q.bias"], d["kv.weight"], d["kv.bias"], tables, [2, 4, 8], shifts, 2, H, W)
    record("fused_ln_qkv_wattn_B%d_shift%d" % (B, shifts[0]), "max|err| vs oracle", max_abs_err(got, ref), 1.5e-5)
    assert_close(got, ref, 1.5e-5, 1.5e-5, "fused LN+QKV+window attention B=%d shifts=%s" % (B, shifts))
    # the unfused kernels on the same inputs agree too (they stay the path of the stress shapes and of training)
    q_d = ops.ln_linear(tq.to(dev).reshape(-1, C), lnq_w.to(dev), lnq_b.to(dev), d["q.weight"], d["q.bias"]).reshape(B, H * W, C)
    kv_d = ops.ln_linear(tkv.to(dev).reshape(-1, C), lnk_w.to(dev), lnk_b.to(dev), d["kv.weight"], d["kv.bias"]).reshape(B, H * W, 2 * C)
    assert_close(got, ops.window_attn(q_d, kv_d, tables, [2, 4, 8], shifts, 2, H, W), ATOL, RTOL, "fused vs unfused kernels")
    if B == 1:
        # the reference's own cat tensor: identity LayerNorms make the fused kernel's input the golden's (already normalised) x
        xq = synth.uniform("wa_xq", (1, H, W, C), -1, 1, 6).reshape(1, H * W, C)
        xkv = synth.uniform("wa_xkv", (1, H, W, C), -1, 1, 6).reshape(1, H * W, C)
        mu_q, sg_q = xq.mean(-1, keepdim=True), (xq.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        mu_k, sg_k = xkv.mean(-1, keepdim=True), (xkv.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        # LN(x) * sg + mu == x only per token; instead fold it: feed y = x (so LN(y) = (x - mu)/sg) and compare with the
        # reference's projection of (x - mu)/sg computed on the CPU -- the golden pins the attention core on the same q / kv
        one, zero = torch.ones(C), torch.zeros(C)
        q1 = F.linear((xq - mu_q) / sg_q, sd["q.weight"], sd["q.bias"])
        kv1 = F.linear((xkv - mu_k) / sg_k, sd["kv.weight"], sd["kv.bias"])
        ref1 = o.window_attention_core(q1, kv1[..., :C], kv1[..., C:], sd, "", H, W, [2, 4, 8], shifts, 2)
        got1 = ops.ln_qkv_window_attn(xq.to(dev), xkv.to(dev), one.to(dev), zero.to(dev), one.to(dev), zero.to(dev), d["q.weight"],
                                      d["q.bias"], d["kv.weight"], d["kv.bias"], tables, [2, 4, 8], shifts, 2, H, W)
        assert_close(got1, ref1, ATOL, RTOL, "fused kernel, identity affine")


def test_window_attention_batch_and_dim192(dev):
    from dpmn_amd import ops
    from oracle import pgrm as o
    for (B, H, W, C, wins) in ((5, 16, 64, 96, [2, 4, 8]), (2, 32, 128, 192, [4, 8, 8])):
        q, kv = u("q", (B, H * W, C)), u("kv", (B, H * W, 2 * C))
        sd = {"relative_position_bias_table_%d" % i: u("tb%d" % i, ((2 * w - 1) ** 2, 2)) for i, w in enumerate(wins)}
        for shifts in ([0, 0, 0], [w // 2 for w in wins]):
            ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sd, "", H, W, wins, shifts, 2)
            got = ops.window_attn(q.to(dev), kv.to(dev), [sd["relative_position_bias_table_%d" % i].to(dev) for i in range(3)],
                                  wins, shifts, 2, H, W)
            assert_close(got, ref, ATOL, RTOL, "window attention B=%d C=%d shifts=%s" % (B, C, shifts))


def test_sk_fuse(dev):
    from dpmn_amd import ops
    from oracle import pgrm as o
    B, L, C = 3, 1024, 96
    sd = {"proj.weight": u("a", (C, C), -0.2, 0.2), "proj.bias": u("b", (C,)),
          "fc1.weight": u("c", (16, C), -0.3, 0.3), "fc1.bias": u("d", (16,)),
          "fc2.weight": u("e", (C, 16), -0.5, 0.5), "fc2.bias": u("f", (C,)),
          "proj_head.weight": u("g", (C, 32), -0.3, 0.3), "proj_head.bias": u("h", (C,))}
    cat, sc = u("cat", (B, L, C)), u("sc", (B, L, C))
    ref = sc + o.sk_fuse(cat, sd, "", 3)
    d = cu(sd, dev)
    got, _ = ops.sk_fuse(cat.to(dev), sc.to(dev), d["proj.weight"], d["proj.bias"], d["fc1.weight"], d["fc1.bias"],
                         d["fc2.weight"], d["fc2.bias"], d["proj_head.weight"], d["proj_head.bias"], 3)
    assert_close(got, ref, ATOL, RTOL, "shortcut + SKConv")


@pytest.mark.parametrize("B", [1, 3, 48])
def test_sk_select_ln2_fc1_one_launch_equals_two_and_oracle(dev, B):
    """dpmn_sk_mlp_in_f32 (select + proj_head + residuals -> x1 -> LayerNorm2 -> fc1 in one launch) is bitwise equal to
    dpmn_sk_select_f32 + dpmn_ln_linear_f32, and both match the oracle (pgrm.py:79-96, 327-331, 31)."""
    from dpmn_amd import ops
    from oracle import pgrm as o
    L, C, N = 1024, 96, 384
    sd = {"proj.weight": u("a", (C, C), -0.2, 0.2), "proj.bias": u("b", (C,)),
          "fc1.weight": u("c", (16, C), -0.3, 0.3), "fc1.bias": u("d", (16,)),
          "fc2.weight": u("e", (C, 16), -0.5, 0.5), "fc2.bias": u("f", (C,)),
          "proj_head.weight": u("g", (C, 32), -0.3, 0.3), "proj_head.bias": u("h", (C,))}
    ln_w, ln_b = u("lnw", (C,), 0.5, 1.5), u("lnb", (C,), -0.3, 0.3)
    w1, b1 = u("w1", (N, C), -0.2, 0.2), u("b1", (N,))
    cat, sc = u("cat", (B, L, C)), u("sc", (B, L, C))
    d = cu(sd, dev)
    args = (d["proj.weight"], d["proj.bias"], d["fc1.weight"], d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], d["proj_head.weight"],
            d["proj_head.bias"], 3)
    x1_two, _ = ops.sk_fuse(cat.to(dev), sc.to(dev), *args)
    y_two = ops.ln_linear(x1_two.reshape(-1, C), ln_w.to(dev), ln_b.to(dev), w1.to(dev), b1.to(dev)).reshape(B, L, N)
    x1, y = ops.sk_fuse_mlp_in(cat.to(dev), sc.to(dev), *args, ln_w.to(dev), ln_b.to(dev), w1.to(dev), b1.to(dev))
    assert torch.equal(x1, x1_two) and torch.equal(y, y_two)
    if B <= 3:
        x1_ref = sc + o.sk_fuse(cat, sd, "", 3)
        y_ref = F.linear(F.layer_norm(x1_ref, (C,), ln_w, ln_b, 1e-5), w1, b1)
        assert_close(x1, x1_ref, ATOL, RTOL, "x1")
        assert_close(y, y_ref, 2e-4, 2e-4, "fc1(LayerNorm2(x1))")


def test_mlp_chain_vs_golden(dev):
    from dpmn_amd import ops
    g = load_golden("mlp")
    sd = cu(sd_from_manifest(g["manifest"], 22), dev)
    x = synth.uniform("mlp_x", (2, 1024, 96), -1, 1, 6).to(dev)
    y = ops.linear(x.reshape(-1, 96), sd["fc1.weight"], sd["fc1.bias"], act="gelu").reshape(2, 1024, 384)
    gg = ops.dwconv3x3_gelu(y, sd["depthwise_conv.weight"], sd["depthwise_conv.bias"], 32)
    z = ops.pointwise(gg, sd["pointwise_conv.weight"], sd["pointwise_conv.bias"])
    out = ops.linear(z.reshape(-1, 384), sd["fc2.weight"], sd["fc2.bias"]).reshape(2, 1024, 96)
    assert_close(out, t(g["out"]), ATOL, RTOL, "Mlp chain vs reference golden")


def test_tail(dev):
    from dpmn_amd import ops
    B, H, W, C = 2, 16, 64, 96
    tok = u("tok", (B, H * W, C))
    w0, b0 = u("w0", (12, C, 3, 3), -0.05, 0.05), u("b0", (12,))
    w1, b1 = u("w1", (12, 12, 3, 3), -0.2, 0.2), u("b1", (12,))
    wl = [u("wl%d" % i, (1, 3, 32, 128), 0.8, 1.2) for i in range(3)]
    res = [u("res%d" % i, (B, 3, 32, 128), 0, 1) for i in range(3)]
    x = tok.transpose(1, 2).reshape(B, C, H, W)
    x = F.leaky_relu(F.conv2d(F.conv2d(x, w0, b0, padding=1), w1, b1, padding=1), 0.01)
    ref = F.pixel_shuffle(x, 2) * wl[0] + res[1] * wl[1] + res[2] * wl[2]
    got = ops.pgrm_tail(tok.to(dev), w0.to(dev), b0.to(dev), w1.to(dev), b1.to(dev), [w.to(dev) for w in wl],
                        [r.to(dev) for r in res], H, W, 3, 2)
    assert_close(got, ref, ATOL, RTOL, "tail with residuals (Q11: residual 0 skipped)")
    ref0 = F.pixel_shuffle(x, 2) * wl[0]
    got0 = ops.pgrm_tail(tok.to(dev), w0.to(dev), b0.to(dev), w1.to(dev), b1.to(dev), [wl[0].to(dev)], [], H, W, 3, 2)
    assert_close(got0, ref0, ATOL, RTOL, "tail without residuals")


# ------------------------------------------------------------------------------ whole module
def _pgrm_args(n=6):
    return dict(patch_size=[2] * n, embed_dim=[96] * n, depths=[1] * n, num_heads=[[6]] * n, window_size=[[2, 4, 8]] * n,
                mlp_ratio=[4.] * n, drop_rate=[0.] * n, attn_drop_rate=[0.] * n, drop_path_rate=[0.] * n)


@pytest.mark.parametrize("tag,it,mode", [("mode0_iter0", 0, False), ("mode1_iter2", 2, True)])
def test_pgrm_module_vs_reference_golden(dev, tag, it, mode):
    from dpmn_amd.model.pgrm import PGRM
    g = load_golden("pgrm_" + tag)
    B, _, _, wseed, iseed = [int(v) for v in g["meta"]]
    m = PGRM(iter=it, mode=mode, hidden_size=3, **_pgrm_args()).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, wseed)
    m.load_state_dict(sd)
    m = m.to(dev)
    if mode:
        x_q = (synth.uniform("x_q", (B, 1, 32, 128), 0, 1, iseed) > 0.5).float().repeat(1, 3, 1, 1)
    else:
        x_q = torch.floor(synth.uniform("x_q", (B, 2, 32, 128), 0, 256, iseed))
    x_kv = synth.uniform("x_kv", (B, 3, 32, 128), 0, 1, iseed)
    res = [synth.uniform("res%d" % i, (B, 3, 32, 128), 0, 1, iseed).to(dev) for i in range(it)]
    with torch.no_grad():
        out = m(x_q.to(dev), x_kv.to(dev), res)
    assert_close(out, t(g["out"]), 2e-4, 2e-4, "PGRM module vs reference golden " + tag)


def test_pgrm_module_batch48_vs_oracle(dev):
    """config-1 per-GPU batch; checks batch indexing at full size against the oracle."""
    from dpmn_amd.model.pgrm import PGRM
    from oracle import pgrm as o
    B = 48
    m = PGRM(iter=1, mode=False, hidden_size=3, **_pgrm_args()).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, 77)
    m.load_state_dict(sd)
    x_q = torch.floor(u("xq", (B, 2, 32, 128), 0, 256))
    x_kv = u("xkv", (B, 3, 32, 128), 0, 1)
    res = [u("r0", (B, 3, 32, 128), 0, 1)]
    ref = o.pgrm_forward({k: v for k, v in sd.items()}, x_q, x_kv, res)
    m = m.to(dev)
    with torch.no_grad():
        out = m(x_q.to(dev), x_kv.to(dev), [r.to(dev) for r in res])
    assert_close(out, ref, 2e-4, 2e-4, "PGRM module B=48 vs oracle")


def test_basiclayer_stress_dims_vs_reference_golden_and_oracle(dev):
    """Stress configuration (config 4 dims: dim 192, windows 4/8/16 -> a 256-token window, 32x128 tokens, L = 4096) at the
    BasicLayer level, where the reference pins it (quirk Q7): reference golden at B=1, oracle at B=3."""
    from dpmn_amd.model.pgrm import BasicLayer
    from oracle import pgrm as opgrm
    g = load_golden("basiclayer_stress")
    m = BasicLayer(192, (32, 128), depth=2, num_heads=6, window_size=[4, 8, 16], mlp_ratio=4.).eval()
    sd = m.state_dict()
    assert sorted(sd.keys()) == sorted(str(r).split("|")[0] for r in g["manifest"])
    synth.synth_fill_(sd, 23)
    m.load_state_dict(sd)
    m = m.to(dev)
    xq = synth.uniform("bl_xq", (1, 4096, 192), -1, 1, 6)
    xkv = synth.uniform("bl_xkv", (1, 4096, 192), -1, 1, 6)
    with torch.no_grad():
        _, o = m(xq.to(dev), xkv.to(dev))
    assert_close(o[:, ::7], t(g["out"]), 3e-4, 3e-4, "BasicLayer stress vs reference golden")
    sdc = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    xq3, xkv3 = synth.uniform("bl_xq3", (3, 4096, 192), -1, 1, 7), synth.uniform("bl_xkv3", (3, 4096, 192), -1, 1, 7)
    ref = opgrm.basic_layer(xq3, xkv3, sdc, "", 32, 128, [4, 8, 16], 6)
    with torch.no_grad():
        _, o3 = m(xq3.to(dev), xkv3.to(dev))
    assert_close(o3, ref, 3e-4, 3e-4, "BasicLayer stress B=3 vs oracle")


@pytest.mark.parametrize("B,shifts,p", [(3, [1, 2, 4], 0.0), (5, [0, 0, 0], 0.1), (48, [1, 2, 4], 0.1)])
def test_fused_attention_training_variant_vs_oracle_and_unfused(dev, B, shifts, p):
    """Training forward of the fused kernel (dpmn_ln_qkv_window_attn_train_f32): the saved q / kv equal Linear(LayerNorm(x)) of
    pgrm.py:188,194, and `cat` under attn_drop equals the oracle with the SAME counter-based masks (and the unfused DROP kernels)."""
    from dpmn_amd import ops
    from oracle import pgrm as o
    from helpers import record, max_abs_err
    H, W, C = 16, 64, 96
    g = load_golden("wattn_shift0" if shifts[0] == 0 else "wattn_shifted")
    sd = sd_from_manifest(g["manifest"], 21)
    lnq_w, lnq_b = u("tlnq_w", (C,), 0.5, 1.5), u("tlnq_b", (C,), -0.5, 0.5)
    lnk_w, lnk_b = u("tlnk_w", (C,), 0.5, 1.5), u("tlnk_b", (C,), -0.5, 0.5)
    tq, tkv = u("t_tq%d" % B, (B, H * W, C), -2, 3), u("t_tkv%d" % B, (B, H * W, C), -3, 2)
    seed = 0x1234567 + B
    q = F.linear(F.layer_norm(tq, (C,), lnq_w, lnq_b), sd["q.weight"], sd["q.bias"])
    kv = F.linear(F.layer_norm(tkv, (C,), lnk_w, lnk_b), sd["kv.weight"], sd["kv.bias"])
    ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sd, "", H, W, [2, 4, 8], shifts, 2, p_attn=p, seed=seed)
    d = cu(sd, dev)
    tables = [d["relative_position_bias_table_%d" % i] for i in range(3)]
    cat, q_d, kv_d = ops.ln_qkv_window_attn_train(tq.to(dev), tkv.to(dev), lnq_w.to(dev), lnq_b.to(dev), lnk_w.to(dev), lnk_b.to(dev),
                                                  d["q.weight"], d["q.bias"], d["kv.weight"], d["kv.bias"], tables, [2, 4, 8], shifts, 2, H, W,
                                                  p_drop=p, seed=seed)
    tag = "fused_train_B%d_p%g" % (B, p)
    record(tag, "q max|err| vs oracle", max_abs_err(q_d, q), 1e-5)
    record(tag, "kv max|err| vs oracle", max_abs_err(kv_d, kv), 1e-5)
    record(tag, "cat max|err| vs oracle (same masks)", max_abs_err(cat, ref), 2e-5)
    assert_close(q_d, q, 1e-5, 1e-5, "saved q")
    assert_close(kv_d, kv, 1e-5, 1e-5, "saved kv")
    assert_close(cat, ref, 2e-5, 2e-5, "fused training forward, attn_drop %g" % p)
    unf = ops.window_attn(q_d, kv_d, tables, [2, 4, 8], shifts, 2, H, W, p_drop=p, seed=seed)
    assert_close(cat, unf, 2e-5, 2e-5, "fused vs unfused DROP kernels on the saved q / kv")


@pytest.mark.parametrize("B,H,W,shifts", [(1, 8, 8, [1, 2, 0]), (2, 8, 16, [0, 0, 0]), (9, 8, 8, [1, 2, 4]), (2, 32, 32, [1, 2, 4])])
def test_fused_attention_token_grids(dev, B, H, W, shifts):
    """Other token grids of the fused attention kernels (forward + recomputing backward): one slab per image (8 x 8: the block ranges
    span window sizes -- the contiguous schedule), fewer images than XCDs, a square 32 x 32 grid; against the oracle's attention core
    and torch autograd through it."""
    from dpmn_amd import ops
    from oracle import pgrm as o
    C = 96
    g = load_golden("wattn_shifted")
    sd = sd_from_manifest(g["manifest"], 21)
    ln = [u("g_lnq_w", (C,), 0.5, 1.5), u("g_lnq_b", (C,), -0.5, 0.5), u("g_lnk_w", (C,), 0.5, 1.5), u("g_lnk_b", (C,), -0.5, 0.5)]
    tq, tkv = u("g_tq%d%d" % (B, H), (B, H * W, C), -2, 3), u("g_tkv%d%d" % (B, H), (B, H * W, C), -3, 2)
    dout = u("g_dout%d%d" % (B, H), (B, H * W, C), -1, 1)
    assert ops.ln_qkv_window_attn_supported(C, [2, 4, 8], 2, H, W)
    q = F.linear(F.layer_norm(tq, (C,), ln[0], ln[1]), sd["q.weight"], sd["q.bias"]).requires_grad_(True)
    kv = F.linear(F.layer_norm(tkv, (C,), ln[2], ln[3]), sd["kv.weight"], sd["kv.bias"]).requires_grad_(True)
    sdg = dict(sd)
    for i in range(3):
        sdg["relative_position_bias_table_%d" % i] = sd["relative_position_bias_table_%d" % i].clone().requires_grad_(True)
    ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sdg, "", H, W, [2, 4, 8], shifts, 2)
    (ref * dout).sum().backward()
    d = cu(sd, dev)
    tables = [d["relative_position_bias_table_%d" % i] for i in range(3)]
    args = (tq.to(dev), tkv.to(dev), *[x.to(dev) for x in ln], d["q.weight"], d["q.bias"], d["kv.weight"], d["kv.bias"], tables, [2, 4, 8], shifts, 2, H, W)
    got = ops.ln_qkv_window_attn(*args)
    assert_close(got, ref.detach(), 1.5e-5, 1.5e-5, "fused attention forward on a %d x %d grid" % (H, W))
    dq, dkv, parts = ops.ln_qkv_window_attn_bwd(*args, dout.to(dev))
    assert_close(dq, q.grad.reshape(-1, C), 7e-6, 7e-6, "fused attention backward dq on a %d x %d grid" % (H, W))
    assert_close(dkv, kv.grad.reshape(-1, 2 * C), 7e-6, 7e-6, "fused attention backward dkv on a %d x %d grid" % (H, W))
    for i in range(3):
        want = sdg["relative_position_bias_table_%d" % i].grad
        got_t = parts[i].double().sum(0).float().reshape(want.shape)
        assert_close(got_t, want, 1.5e-6 * max(1.0, float(want.abs().max())), 1e-4, "fused attention backward table %d on a %d x %d grid" % (i, H, W))


@pytest.mark.parametrize("B,shifts", [(1, [0, 0, 0]), (3, [1, 2, 4]), (5, [0, 0, 0]), (48, [1, 2, 4])])
def test_fused_attention_backward_vs_oracle(dev, B, shifts):
    """The recomputing backward of the fused kernel (attn_fused_bwd.hip: one launch, q / k / v rebuilt from the token rows, all three
    window sizes on MFMA) against torch autograd through the oracle's window_attention_core (pgrm.py:184-271) on the same
    q = a.q(norm1_q(tq)), kv = a.kv(norm1_kv(tkv)): dq, dkv, the three bias-table gradients; and against the unfused backward
    kernels with attention dropout on (same counter-based masks)."""
    from dpmn_amd import ops, _abi
    from dpmn_amd._abi import lib, check, dptr
    from oracle import pgrm as o
    from helpers import record, max_abs_err
    H, W, C = 16, 64, 96
    g = load_golden("wattn_shift0" if shifts[0] == 0 else "wattn_shifted")
    sd = sd_from_manifest(g["manifest"], 21)
    lnq_w, lnq_b = u("lnq_w", (C,), 0.5, 1.5), u("lnq_b", (C,), -0.5, 0.5)
    lnk_w, lnk_b = u("lnk_w", (C,), 0.5, 1.5), u("lnk_b", (C,), -0.5, 0.5)
    tq, tkv = u("f_tq%d" % B, (B, H * W, C), -2, 3), u("f_tkv%d" % B, (B, H * W, C), -3, 2)
    dout = u("f_dout%d" % B, (B, H * W, C), -1, 1)
    q = F.linear(F.layer_norm(tq, (C,), lnq_w, lnq_b), sd["q.weight"], sd["q.bias"]).requires_grad_(True)
    kv = F.linear(F.layer_norm(tkv, (C,), lnk_w, lnk_b), sd["kv.weight"], sd["kv.bias"]).requires_grad_(True)
    sdg = dict(sd)
    for i in range(3):
        sdg["relative_position_bias_table_%d" % i] = sd["relative_position_bias_table_%d" % i].clone().requires_grad_(True)
    ref = o.window_attention_core(q, kv[..., :C], kv[..., C:], sdg, "", H, W, [2, 4, 8], shifts, 2)
    (ref * dout).sum().backward()
    d = cu(sd, dev)
    tables = [d["relative_position_bias_table_%d" % i] for i in range(3)]
    args = (tq.to(dev), tkv.to(dev), lnq_w.to(dev), lnq_b.to(dev), lnk_w.to(dev), lnk_b.to(dev), d["q.weight"], d["q.bias"], d["kv.weight"],
            d["kv.bias"], tables, [2, 4, 8], shifts, 2, H, W)
    dq, dkv, parts = ops.ln_qkv_window_attn_bwd(*args, dout.to(dev))
    tol = 7e-6       # measured 1.2e-6 .. 2.3e-6
    for name, got, want in (("dq", dq, q.grad.reshape(-1, C)), ("dkv", dkv, kv.grad.reshape(-1, 2 * C))):
        record("fused_attn_bwd_%s_B%d_shift%d" % (name, B, shifts[0]), "max|err| vs oracle autograd", max_abs_err(got, want), tol)
        assert_close(got, want, tol, tol, "fused attention backward %s B=%d" % (name, B))
    for i in range(3):
        want = sdg["relative_position_bias_table_%d" % i].grad
        got = parts[i].double().sum(0).float().reshape(want.shape)
        ttol = 1.5e-6 * max(1.0, float(want.abs().max()))      # measured <= 5.4e-7 of the largest entry
        record("fused_attn_bwd_table%d_B%d_shift%d" % (i, B, shifts[0]), "max|err| vs oracle autograd", max_abs_err(got, want), ttol)
        assert_close(got, want, ttol, 1e-4, "fused attention backward table %d B=%d" % (i, B))
    # twice the same launch: bitwise equal (no atomics reach HBM)
    dq2, dkv2, parts2 = ops.ln_qkv_window_attn_bwd(*args, dout.to(dev))
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2) and all(torch.equal(a_, b_) for a_, b_ in zip(parts, parts2))
    # attention dropout: the unfused backward kernels on the saved q / kv of the training forward, same seed
    pa, seed = 0.1, 1234
    cat_s, q_s, kv_s = ops.ln_qkv_window_attn_train(*args, p_drop=pa, seed=seed)
    cat_n, _, _ = ops.ln_qkv_window_attn_train(*args, p_drop=pa, seed=seed, save_qkv=False)
    assert torch.equal(cat_s, cat_n)
    dq_f, dkv_f, parts_f = ops.ln_qkv_window_attn_bwd(*args, dout.to(dev), p_drop=pa, seed=seed)
    dq_u, dkv_u = torch.empty_like(dq_f), torch.empty_like(dkv_f)
    dt_u = [torch.zeros_like(t_) for t_ in tables]
    check(lib.dpmn_window_attn_drop_bwd_f32(dptr(q_s), dptr(kv_s), _abi.ptr_array(tables), _abi.int_array([2, 4, 8]), _abi.int_array(shifts), 3, 2,
                                            dptr(dout.to(dev)), dptr(dq_u), dptr(dkv_u), _abi.ptr_array(dt_u), B, H, W, C, pa, seed, ops.stream()))
    assert_close(dq_f, dq_u, 3e-5, 3e-5, "fused vs unfused attention backward with dropout: dq")
    assert_close(dkv_f, dkv_u, 3e-5, 3e-5, "fused vs unfused attention backward with dropout: dkv")
    for i in range(3):
        got = parts_f[i].double().sum(0).float().reshape(dt_u[i].shape)
        assert_close(got, dt_u[i], 2e-5 * max(1.0, float(dt_u[i].abs().max())), 1e-4, "fused vs unfused attention backward with dropout: table %d" % i)
