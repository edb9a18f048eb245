"""A second GPU in one process: every launcher that opts a kernel in to more dynamic LDS than the default, or sizes a persistent grid
from the CU count, keeps that state per device (csrc/common.h dpmn_lds_optin, dpmn_cu_count).  hipFuncSetAttribute acts on the current
device's copy of a kernel, so an opt-in made once per process leaves the kernel unlaunchable on every other device: the call returns a
launch error.  Each family runs once on cuda:1 -- current device and stream switched to match -- after cuda:0 has been used, then on
cuda:0, and the two results must be equal bit for bit (same kernels, same grids: the devices of a node are alike).  Shapes: the smallest
at which the family's direct test (test_gpu_gemm_family, test_gpu_small_kernels, test_gpu_small_backward, test_gpu_pgrm, test_gpu_x3,
test_gpu_streamk) reaches the kernel.  Like every GPU test the file runs once in fp32 and once in mode 2 (conftest.py), which is how the
bf16x3 twins of the halo conv, rowreg, sk_mlp_in and pointwise kernels are reached."""
import functools

import pytest
import torch

from dpmn_amd.utils import synth

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs (found %d)" % torch.cuda.device_count())]
SEED = 0x5DEECE66D


@functools.lru_cache(maxsize=None)
def u(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(name, shape, lo, hi, 48)


@pytest.fixture(scope="module", autouse=True)
def device0_used_first():
    from dpmn_amd import ops
    with torch.cuda.device(0):
        ops.linear(u("x", (1024, 96)).cuda(), u("w", (96, 96)).cuda())
        torch.cuda.synchronize()


def on_device(index, fn):
    dev = torch.device("cuda", index)
    with torch.cuda.device(dev):
        outs = fn(dev)
        torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def same_on_both(what, fn):
    """fn(dev) -> the output tensors of one call with every operand on dev"""
    second, first = on_device(1, fn), on_device(0, fn)
    assert len(first) == len(second) > 0
    for k, (a, b) in enumerate(zip(first, second)):
        assert not torch.isnan(a).any(), "%s output %d: NaN on cuda:0" % (what, k)
        assert torch.equal(a, b), "%s output %d: cuda:1 differs from cuda:0 in %d elements" % (what, k, int((a != b).sum()))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv(segs, cout, k, stride, pad, B, H, W):
    def run(dev):
        from dpmn_amd import ops
        from dpmn_amd.model import packing
        cin = sum(segs)
        w = u("cw", (cout, cin, k, k)) * (1.0 / (cin * k * k) ** 0.5)
        wp, bp = packing.pack_conv(w.to(dev), u("cb", (cout,)).to(dev))
        xs = [nhwc(u("cx%d" % i, (B, c, H, W))).to(dev) for i, c in enumerate(segs)]
        return [ops.conv2d(xs, wp, bp, cout, k, stride=stride, pad=pad, pro_act="leaky02")]
    return run


def test_halo_conv_64_channels():
    # M = 1024 pixels, 8 tiles of 8 x 16: k_conv_halo<3, 64, 4> in fp32, k_conv_halo_x3 in mode 2 (8 row tiles per image)
    same_on_both("3x3 halo conv 64 -> 64", conv((64,), 64, 3, 1, 1, 1, 16, 64))


def test_halo_conv_c4():
    same_on_both("3x3 halo conv 32 -> 3", conv((32,), 3, 3, 1, 1, 1, 16, 64))


def test_streamk_conv():
    # M = 192 output pixels: 64-pixel row tiles, the stream-K launch by default; its grid is the device's CUs x blocks per CU
    from dpmn_amd import _abi
    run = conv((128,), 128, 4, 2, 1, 6, 8, 16)
    same_on_both("stream-K conv", run)
    with torch.cuda.device(0):
        _abi.profile_begin(None, 16)
        run(torch.device("cuda:0"))
        torch.cuda.synchronize()
        rows = _abi.profile_end()
    assert any(r["kernel"] == "k_conv_igemm_sk" for r in rows), "the stream-K launch did not run: %s" % [r["kernel"] for r in rows]


@pytest.mark.parametrize("M,what", [(1024, "rowreg"), (32, "wstat")])
def test_linear(M, what):
    def run(dev):
        from dpmn_amd import ops
        return [ops.linear(u("x", (M, 96)).to(dev), u("w", (96, 96)).to(dev), u("b", (96,)).to(dev), act="gelu")]
    same_on_both("linear " + what, run)


@pytest.mark.parametrize("save", [False, True])
def test_sk_mlp_in(save):
    def run(dev):
        from dpmn_amd import ops
        M, C, N = 1024, 96, 96
        d = lambda name, shape, *r: u(name, shape, *r).to(dev)
        assert ops.sk_mlp_in_supported(M, M, C, 3, N)
        return ops.sk_mlp_in(d("cat", (M, C)), d("avec", (1, 3, 32), 0.0, 1.0), d("hw", (C, 32), -0.3, 0.3), d("hb", (C,)), d("feats", (M, C)),
                             d("sc", (M, C)), d("lnw", (C,), 0.5, 1.5), d("lnb", (C,), -0.3, 0.3), d("w1", (N, C), -0.2, 0.2), d("b1", (N,)), M,
                             save=save)
    same_on_both("sk_mlp_in save=%s" % save, run)


@pytest.mark.parametrize("Ch", [128, 384])
def test_pointwise(Ch):      # k_gemm_pw_bf16x3<128> / <192> in the mode 2 pass
    def run(dev):
        from dpmn_amd import ops
        return [ops.pointwise(u("g", (1, 128, Ch), -2, 2).to(dev), u("pw", (Ch, Ch), -0.3, 0.3).to(dev), u("pb", (Ch,)).to(dev))]
    same_on_both("pointwise Ch=%d" % Ch, run)


def attn_args(dev, B, H, W, C, wins):
    d = lambda name, shape, *r: u(name, shape, *r).to(dev)
    tables = [d("tb%d" % w, ((2 * w - 1) ** 2, 2), -0.5, 0.5) for w in wins]
    return (d("tq", (B, H * W, C), -2, 3), d("tkv", (B, H * W, C), -3, 2), d("lnq_w", (C,), 0.5, 1.5), d("lnq_b", (C,), -0.5, 0.5),
            d("lnk_w", (C,), 0.5, 1.5), d("lnk_b", (C,), -0.5, 0.5), d("wq", (C, C), -0.2, 0.2), d("bq", (C,)), d("wkv", (2 * C, C), -0.2, 0.2),
            d("bkv", (2 * C,)), tables, wins, [w // 2 for w in wins], 2, H, W)


def test_fused_attention_forward_train_backward():
    B, H, W, C = 2, 8, 32, 96

    def run(dev):
        from dpmn_amd import ops
        args = attn_args(dev, B, H, W, C, [2, 4, 8])
        dout = u("dout", (B, H * W, C)).to(dev)
        outs = [ops.ln_qkv_window_attn(*args)]
        for p in (0.0, 0.1):
            outs += list(ops.ln_qkv_window_attn_train(*args, p_drop=p, seed=SEED))
            dq, dkv, parts = ops.ln_qkv_window_attn_bwd(*args, dout, p_drop=p, seed=SEED)
            outs += [dq, dkv] + parts
        return outs
    same_on_both("ln_qkv_window_attn", run)


def test_fused_attention_dim192():
    def run(dev):
        from dpmn_amd import ops
        assert ops.ln_qkv_window_attn_d32_supported(192, [4, 8, 16], 2, 16, 16)
        return [ops.ln_qkv_window_attn_d32(*attn_args(dev, 1, 16, 16, 192, [4, 8, 16]))]
    same_on_both("ln_qkv_window_attn_d32", run)


@pytest.mark.parametrize("B,H,W,C,wins", [(2, 8, 32, 96, [2, 4, 8]), (1, 16, 16, 192, [4, 8, 16])])
def test_window_attention_forward_backward(B, H, W, C, wins):
    def run(dev):
        from dpmn_amd import ops, _abi
        from dpmn_amd._abi import lib, check, dptr
        d = lambda name, shape, *r: u(name, shape, *r).to(dev)
        q, kv, dout = d("q", (B, H * W, C)), d("kv", (B, H * W, 2 * C)), d("dout", (B, H * W, C))
        tables = [d("tb%d" % w, ((2 * w - 1) ** 2, 2), -0.5, 0.5) for w in wins]
        shifts = [w // 2 for w in wins]
        outs = []
        for p in (0.0, 0.1):
            outs.append(ops.window_attn(q, kv, tables, wins, shifts, 2, H, W, p_drop=p, seed=SEED))
            dq, dkv = torch.empty_like(q), torch.empty_like(kv)
            nrows = lib.dpmn_window_attn_bwd_part_rows(B, H, W)
            parts = [torch.zeros(nrows, t.numel(), device=dev) for t in tables]
            rows = _abi.int_array([0] * 3)
            check(lib.dpmn_window_attn_drop_bwd_det_f32(dptr(q), dptr(kv), _abi.ptr_array(tables), _abi.int_array(wins), _abi.int_array(shifts), 3, 2,
                                                        dptr(dout), dptr(dq), dptr(dkv), _abi.ptr_array(parts), rows, B, H, W, C, p, SEED,
                                                        ops.stream()))
            outs += [dq, dkv] + [parts[g][:rows[g]] for g in range(3)]
        return outs
    same_on_both("window_attn C=%d" % C, run)


# r = 32: the streaming forward on at most 7 blocks per CU and the persistent KEEP backward on 2; r = 60 / 36: whole-plane tiles of 67 / 53.5 KB
@pytest.mark.parametrize("r,Ch", [(32, 8), (60, 2)])
def test_dwconv_forward(r, Ch):
    def run(dev):
        from dpmn_amd import ops
        return [ops.dwconv3x3_gelu(u("y", (1, r * r, Ch), -3, 3).to(dev), u("dww", (Ch, 1, 3, 3), -0.5, 0.5).to(dev), u("dwb", (Ch,)).to(dev), r)]
    same_on_both("dwconv3x3_gelu r=%d" % r, run)


@pytest.mark.parametrize("r,Ch", [(32, 8), (36, 2)])
def test_dwconv_backward(r, Ch):
    def run(dev):
        from dpmn_amd import ops
        from dpmn_amd._abi import lib, check, dptr
        shape = (1, Ch, r, r)
        P, dg, gpre = u("P", shape, -3, 3).to(dev), u("dg", shape).to(dev), u("gpre", shape, -3, 3).to(dev)
        w = u("dww", (Ch, 1, 3, 3), -0.5, 0.5).to(dev)
        dP, dw, db = torch.empty(shape, device=dev), torch.zeros(Ch, 9, device=dev), torch.zeros(Ch, device=dev)
        nws = lib.dpmn_dwconv3x3_bwd_det_bytes(1, Ch, r) // 4
        ws = torch.empty(nws, device=dev)
        check(lib.dpmn_dwconv3x3_bwd_fused_det_f32(dptr(P), dptr(dg), dptr(gpre), dptr(w), dptr(dP), dptr(dw), dptr(db), 1, 1, 0.1, SEED, 1, Ch, r,
                                                   dptr(ws), nws * 4, ops.stream()))
        return [dP, dw, db]
    same_on_both("dwconv3x3 backward r=%d" % r, run)


def test_sk_gate_above_default_lds():
    B, C, G, dmid, L = 2, 192, 3, 32, 64      # both weight matrices in LDS: 54.8 KB

    def run(dev):
        from dpmn_amd import ops
        from dpmn_amd._abi import lib, check, dptr
        d = lambda name, shape, *r: u(name, shape, *r).to(dev)
        avec = torch.empty(B, G, C // G, device=dev)
        check(lib.dpmn_sk_gate_f32(dptr(d("part", (B * 2, C), 0.0, 32.0)), 2, L, dptr(d("g1w", (dmid, C), -0.3, 0.3)), dptr(d("g1b", (dmid,))),
                                   dptr(d("g2w", (C, dmid), -0.5, 0.5)), dptr(d("g2b", (C,))), dptr(avec), B, C, G, dmid, ops.stream()))
        return [avec]
    same_on_both("sk_gate", run)
