"""GPU parity of the training path: HIP forward+backward (explicit backward kernels behind torch.autograd) vs
torch autograd through the CPU oracle on the same weights / inputs / cotangent.  fp32; tolerances per test."""
import os

import pytest
import torch

from dpmn_amd.utils import synth
from helpers import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def u(name, shape, lo=-1.0, hi=1.0, seed=80):
    return synth.uniform(name, shape, lo, hi, seed)


def _pgrm_args(n=6):
    return dict(patch_size=[2] * n, embed_dim=[96] * n, depths=[1] * n, num_heads=[[6]] * n, window_size=[[2, 4, 8]] * n,
                mlp_ratio=[4.] * n, drop_rate=[0.] * n, attn_drop_rate=[0.] * n, drop_path_rate=[0.] * n)


def l2_err(a, b):
    """relative L2 error: robust to the isolated ReLU / LeakyReLU derivative flips that fp32 round-off differences
    (atomics order in the BatchNorm statistics) cause at pre-activations within ~1e-6 of zero."""
    a, b = a.float().cpu().double(), b.float().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def test_image_loss_fwd_bwd(dev):
    from dpmn_amd.loss.image_loss import ImageLoss
    from oracle import cmm as ocmm
    o = u("o", (4, 3, 32, 128), 0, 1).requires_grad_(True)
    t = u("t", (4, 4, 32, 128), 0, 1)
    ref = ocmm.image_loss(o, t[:, :3], True) * 100
    ref.backward()
    od = o.detach().to(dev).requires_grad_(True)
    loss = ImageLoss(gradient=True, loss_weight=[1, 1])(od, t.to(dev)[:, :3, :]) * 100
    loss.backward()
    assert abs(float(loss) - float(ref)) < 1e-4 * abs(float(ref))
    assert rel_err(od.grad, o.grad) < 1e-4


@pytest.mark.parametrize("it,mode", [(0, False), (2, True)])
def test_pgrm_backward_vs_oracle_autograd(dev, it, mode):
    from dpmn_amd.model.pgrm import PGRM
    from oracle import pgrm as o
    B = 2
    m = PGRM(iter=it, mode=mode, hidden_size=3, **_pgrm_args())
    sd = m.state_dict()
    synth.synth_fill_(sd, 90 + it)
    m.load_state_dict(sd)
    x_q = torch.floor(u("xq", (B, 2, 32, 128), 0, 256)) if not mode else (u("xq", (B, 1, 32, 128), 0, 1) > 0.5).float().repeat(1, 3, 1, 1)
    x_kv = u("xkv", (B, 3, 32, 128), 0, 1)
    res = [u("r%d" % i, (B, 3, 32, 128), 0, 1) for i in range(it)]
    cot = u("cot", (B, 3, 32, 128), -1, 1)
    # oracle with autograd
    sd_ref = {k: v.clone().requires_grad_(torch.is_floating_point(v) and "index" not in k and "mask" not in k) for k, v in sd.items()}
    xkv_ref = x_kv.clone().requires_grad_(True)
    res_ref = [r.clone().requires_grad_(True) for r in res]
    out_ref = o.pgrm_forward(sd_ref, x_q, xkv_ref, res_ref)
    (out_ref * cot).sum().backward()
    # HIP
    m = m.to(dev).train()
    xkv_d = x_kv.to(dev).requires_grad_(True)
    res_d = [r.to(dev).requires_grad_(True) for r in res]
    out = m(x_q.to(dev), xkv_d, res_d)
    assert_close(out, out_ref.detach(), 3e-4, 3e-4, "train-mode forward")
    (out * cot.to(dev)).sum().backward()
    assert rel_err(xkv_d.grad, xkv_ref.grad) < 2e-3, "dx_kv"
    for i in range(1, it):
        assert rel_err(res_d[i].grad, res_ref[i].grad) < 1e-3, "dres %d" % i
    worst = ("", 0.0)
    for name, p in m.named_parameters():
        g_ref = sd_ref[name].grad
        assert p.grad is not None, name
        if g_ref is None:   # parameter unused by the reference forward (e.g. weight_list_iter, quirk Q11): zero gradient
            assert float(p.grad.abs().max()) == 0.0, name
            continue
        e = rel_err(p.grad, g_ref)
        if e > worst[1]:
            worst = (name, e)
        assert e < 3e-3, "grad %s rel err %.2e (|ref|max %.3e)" % (name, e, float(g_ref.abs().max()))
    print("worst param grad", worst)


@pytest.mark.parametrize("M", [49, 1000, 4096])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("det", [False, True])
def test_layernorm_backward_ragged_rows_vs_torch(dev, M, accumulate, det, monkeypatch):
    """dpmn_layernorm_bwd_f32 (vector kernel: 32 rows per block pass, rows past M clamped and masked) and its atomics-free form
    dpmn_layernorm_bwd_det_f32 (per-block dgamma / dbeta partials added in block order) vs torch autograd."""
    from dpmn_amd.train import pgrm_train
    monkeypatch.setattr(pgrm_train, "LNB_DET", det)
    C = 96
    x = u("lnx", (M, C), -2, 3).requires_grad_(True)
    g, b = u("lng", (C,), 0.5, 1.5).requires_grad_(True), u("lnb", (C,)).requires_grad_(True)
    dy, dx0 = u("lndy", (M, C)), u("lndx0", (M, C))
    torch.nn.functional.layer_norm(x, (C,), g, b).backward(dy)
    dx = dx0.clone().to(dev) if accumulate else torch.full((M, C), float("nan"), device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    pgrm_train.layernorm_bwd(x.detach().to(dev), dy.to(dev), g.detach().to(dev), dx, accumulate, dg, db)
    assert_close(dx, x.grad + (dx0 if accumulate else 0), 2e-4, 2e-4, "dx")
    assert_close(dg, g.grad, 2e-3, 2e-4, "dgamma")
    assert_close(db, b.grad, 2e-3, 2e-4, "dbeta")


@pytest.mark.parametrize("M,N,K", [(49152, 96, 96), (49152, 384, 96), (24576, 96, 384), (8190, 192, 96), (1001, 144, 48),
                                   (4099, 96, 32), (777, 32, 96), (515, 16, 96)])
@pytest.mark.parametrize("with_db", [False, True])
def test_linear_weight_gradient_vs_torch(dev, M, N, K, with_db):
    """dpmn_gemm_tn_f32: dW += dY^T X (+ db += column sums), every nn.Linear weight gradient of pgrm.py.  N, K multiples of 48
    take the operands-in-registers kernel (ragged row counts: the last 4-row step and the last block run past M; 144 = one and
    a half block tiles), the others the LDS kernel.  Reference: fp64 on the CPU; accumulation into a non-zero dW; two runs equal."""
    from dpmn_amd.train import pgrm_train
    dy, x = u("tndy", (M, N)), u("tnx", (M, K))
    dw0, db0 = u("tndw0", (N, K)), u("tndb0", (N,))
    ref_w = (dw0.double() + dy.double().t() @ x.double()).float()
    ref_b = (db0.double() + dy.double().sum(0)).float()
    outs = []
    for _ in range(2):
        dw, db = dw0.clone().to(dev), db0.clone().to(dev)
        pgrm_train.gemm_tn(dy.to(dev), x.to(dev), dw, db if with_db else None)
        outs.append((dw, db))
    tol = 2e-6 * M ** 0.5 + 1e-5             # fp32 sums of M products of magnitude <= 1
    assert_close(outs[0][0], ref_w, tol, 1e-5, "dW %s" % ((M, N, K),))
    if with_db:
        assert_close(outs[0][1], ref_b, tol, 1e-5, "db")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_grouped_linear_weight_gradients_equal_the_single_calls_bitwise(dev):
    """dpmn_gemm_tn_group_f32 (the Linear weight gradients of one Swin block in ONE partial-sum launch, csrc/backward.hip
    k_gemm_tn_reg_multi / gemm_tn_x3.hip in mode 2) == the same products as dpmn_gemm_tn_f32 calls, bit for bit: the shapes of a PGRM
    block at B = 48 and B = 3 (fc2, fc1, SKConv proj, q, kv; the SKConv head K = 32 and a ragged row count keep their own launches),
    with and without bias gradients, accumulating into non-zero gradients; two grouped runs equal.  The last item (one 32-row split:
    it cannot join the group) adds into the dW / db of an earlier grouped item: the sums stay in array order."""
    import ctypes as C
    from dpmn_amd._abi import lib, check, dptr, stream, TnItem
    shapes = [(49152, 96, 384, True), (49152, 384, 96, True), (49152, 96, 32, True), (49152, 96, 96, False), (49152, 96, 96, True),
              (49152, 192, 96, True), (3072, 96, 384, True), (1001, 144, 48, True), (515, 16, 96, False), (32, 96, 96, True)]
    shared = {len(shapes) - 1: 4}        # item -> the earlier item whose dW / db it accumulates into
    ops_ = []
    for i, (M, N, K, with_db) in enumerate(shapes):
        ops_.append((u("gdy%d" % i, (M, N)).to(dev), u("gx%d" % i, (M, K)).to(dev), u("gdw%d" % i, (N, K)).to(dev),
                     u("gdb%d" % i, (N,)).to(dev) if with_db else None))

    def single():
        out = []
        for i, (dy, x, dw0, db0) in enumerate(ops_):
            M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
            dw, db = out[shared[i]] if i in shared else (dw0.clone(), None if db0 is None else db0.clone())
            ws = torch.empty(lib.dpmn_gemm_tn_partial_bytes(M, N, K) // 4, device=dev)
            check(lib.dpmn_gemm_tn_f32(dptr(dy), dptr(x), dptr(dw), dptr(db, True), M, N, K, dptr(ws), ws.numel() * 4, stream()))
            out.append((dw, db))
        torch.cuda.synchronize()
        return out

    def grouped():
        items, keep, out = (TnItem * len(ops_))(), [], []
        for i, (dy, x, dw0, db0) in enumerate(ops_):
            M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
            dw, db = out[shared[i]] if i in shared else (dw0.clone(), None if db0 is None else db0.clone())
            ws = torch.empty(lib.dpmn_gemm_tn_partial_bytes(M, N, K) // 4, device=dev)
            items[i] = TnItem(dptr(dy), dptr(x), dptr(dw), dptr(db, True), M, N, K, dptr(ws), ws.numel() * 4)
            keep.append(ws)
            out.append((dw, db))
        check(lib.dpmn_gemm_tn_group_f32(items, len(ops_), stream()))
        torch.cuda.synchronize()
        return out
    a, b, c = single(), grouped(), grouped()
    for (M, N, K, _), (w1, b1), (w2, b2), (w3, b3) in zip(shapes, a, b, c):
        assert torch.equal(w1, w2) and torch.equal(w2, w3), "dW %s" % ((M, N, K),)
        assert (b1 is None) or (torch.equal(b1, b2) and torch.equal(b2, b3)), "db %s" % ((M, N, K),)


@pytest.mark.parametrize("pixels,C,act,accumulate", [(1000, 64, "leaky02", False), (4099, 128, "relu", True), (515, 512, "none", False),
                                                     (196608, 64, "relu", False)])
def test_batchnorm_backward_with_folded_reduction_vs_torch_autograd(dev, pixels, C, act, accumulate):
    """dpmn_affine_act_bwd_stats_f32 (activation backward of the last consumer + the producer's per-channel sums in fp64) followed
    by dpmn_bn_bwd_apply_f32 == autograd of act(nn.BatchNorm2d(r)) in batch-statistics mode (cmm.py:12, 48, 69); two runs equal."""
    from dpmn_amd import ops
    from dpmn_amd._abi import lib, check, dptr, stream
    r = u("bnr", (pixels, C), -2, 2).requires_grad_(True)
    gamma, beta = u("bng", (C,), 0.5, 1.5).requires_grad_(True), u("bnb", (C,), -0.5, 0.5).requires_grad_(True)
    dA, G0 = u("bndA", (pixels, C)), u("bnG0", (pixels, C))
    z = torch.nn.functional.batch_norm(r, None, None, gamma, beta, True, 0.0, 1e-5)
    fn = {"leaky02": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "relu": torch.relu, "none": lambda t: t}[act]
    (fn(z) * dA).sum().backward(retain_graph=True)
    if accumulate:          # a second consumer already left its gradient w.r.t. z in G
        z.backward(G0)
    with torch.no_grad():
        mean, var = r.mean(0), r.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        scale, shift = gamma * rstd, beta - mean * gamma * rstd
    outs = []
    for _ in range(2):
        G = G0.clone().to(dev) if accumulate else torch.full((pixels, C), float("nan"), device=dev)
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        ws, dr = torch.empty(2 * C, device=dev), torch.empty(pixels, C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        rd, md, sd = r.detach().to(dev), mean.to(dev), rstd.to(dev)      # (named: a temporary's memory is reused by the next upload)
        dAd, scd, shd, gad = dA.to(dev), scale.detach().to(dev), shift.detach().to(dev), gamma.detach().to(dev)
        check(lib.dpmn_affine_act_bwd_stats_f32(dptr(dAd), dptr(rd), dptr(scd), dptr(shd), ops.ACT[act],
                                                dptr(G), 1 if accumulate else 0, pixels, C, dptr(md), dptr(sd), sums.data_ptr(), stream()))
        check(lib.dpmn_bn_bwd_apply_f32(dptr(G), dptr(rd), dptr(gad), dptr(md), dptr(sd), sums.data_ptr(), dptr(ws), dptr(dr),
                                        dptr(dg), dptr(db), pixels, C, stream()))
        outs.append((dr, dg, db))
    tol = 3e-6 * pixels ** 0.5 + 2e-5
    assert_close(outs[0][0], r.grad, 1e-4, 1e-4, "d(raw conv output)")
    assert_close(outs[0][1], gamma.grad, tol * 4, 1e-4, "dgamma")
    assert_close(outs[0][2], beta.grad, tol * 4, 1e-4, "dbeta")
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_dropout_kernel_masks_equal_oracle_hash(dev):
    """dpmn_dropout_f32 (elementwise + per-sample DropPath + residual) vs the numpy restatement of the mask hash: the kept set
    is bit-identical, values equal to fp32 round-off of the single multiply."""
    from dpmn_amd import ops
    from oracle import pgrm as o
    x, r = u("dx", (4, 256, 96), -1, 1), u("dr", (4, 256, 96), -1, 1)
    seed_e, seed_r = 0x1234567890ABCDE, 0x0FEDCBA987654321
    y = ops.dropout(x.to(dev), 0.1, seed_e, 0.5, seed_r, row_len=256 * 96, res=r.to(dev), out=torch.empty_like(x, device=dev))
    ref = r + o.drop_path(o.dropout(x, 0.1, seed_e), 0.5, seed_r)
    assert_close(y, ref, 1e-6, 1e-6, "dropout + droppath + residual")
    kept = (ops.dropout(torch.ones(4, 256, 96, device=dev), 0.1, seed_e) != 0).cpu()
    assert torch.equal(kept, o.dropout(torch.ones(4, 256, 96), 0.1, seed_e) != 0)
    assert abs(float(kept.float().mean()) - 0.9) < 0.01


@pytest.mark.parametrize("rates", [(0.1, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, 0.0, 0.9), (0.1, 0.1, 0.6)])
def test_pgrm_train_dropout_vs_oracle_same_masks(dev, rates):
    """Train-mode Dropout / attn_drop / DropPath (the reference README's training flags use 0.1 for all three): forward and
    every gradient vs torch autograd through the oracle applying the SAME counter-based masks at the reference's sites."""
    from dpmn_amd.model.pgrm import PGRM
    from dpmn_amd.train import pgrm_train
    from oracle import pgrm as o
    B, it = 4, 2
    pd, pa, pp = rates
    args = _pgrm_args()
    args.update(drop_rate=[pd] * 6, attn_drop_rate=[pa] * 6, drop_path_rate=[pp] * 6)
    m = PGRM(iter=it, mode=True, hidden_size=3, **args)
    dpr = [x.item() for x in torch.linspace(0, pp, 12)]
    assert m.drop_probs == (pd, pa, (dpr[4], dpr[5]))            # pgrm.py:499,512
    sd = m.state_dict()
    synth.synth_fill_(sd, 95)
    m.load_state_dict(sd)
    x_q = (u("xq", (B, 1, 32, 128), 0, 1) > 0.5).float().repeat(1, 3, 1, 1)
    x_kv = u("xkv", (B, 3, 32, 128), 0, 1)
    res = [u("r%d" % i, (B, 3, 32, 128), 0, 1) for i in range(it)]
    cot = u("cot", (B, 3, 32, 128), -1, 1)
    torch.manual_seed(4242)
    seeds = pgrm_train.draw_seeds()
    drop = dict(p=pd, pa=pa, dp=(dpr[4], dpr[5]), seeds=seeds)
    sd_ref = {k: v.clone().requires_grad_(torch.is_floating_point(v) and "index" not in k and "mask" not in k) for k, v in sd.items()}
    xkv_ref = x_kv.clone().requires_grad_(True)
    out_ref = o.pgrm_forward(sd_ref, x_q, xkv_ref, res, drop=drop)
    (out_ref * cot).sum().backward()
    out_eval = o.pgrm_forward(sd, x_q, x_kv, res)
    assert float((out_ref.detach() - out_eval).abs().max()) > 1e-3, "the masks must actually change the output"
    m = m.to(dev).train()
    xkv_d = x_kv.to(dev).requires_grad_(True)
    torch.manual_seed(4242)                                       # the module draws the same seeds from the CPU generator
    out = m(x_q.to(dev), xkv_d, [r.to(dev) for r in res])
    assert_close(out, out_ref.detach(), 3e-4, 3e-4, "train-mode forward with dropout")
    (out * cot.to(dev)).sum().backward()
    assert rel_err(xkv_d.grad, xkv_ref.grad) < 2e-3, "dx_kv"
    for name, p in m.named_parameters():
        g_ref = sd_ref[name].grad
        if g_ref is None:
            assert float(p.grad.abs().max()) == 0.0, name
            continue
        e = rel_err(p.grad, g_ref)
        assert e < 3e-3, "grad %s rel err %.2e (|ref|max %.3e)" % (name, e, float(g_ref.abs().max()))
    # eval ignores every rate; a second training call draws new seeds
    m.eval()
    with torch.no_grad():
        assert_close(m(x_q.to(dev), x_kv.to(dev), [r.to(dev) for r in res]), out_eval, 3e-4, 3e-4, "eval forward")
        m.train()
        out2 = m(x_q.to(dev), x_kv.to(dev), [r.to(dev) for r in res])
    assert float((out2 - out.detach()).abs().max()) > 1e-4, "fresh masks per call"


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.6)])
@pytest.mark.parametrize("mode", [True, False])
def test_pgrm_native_training_forward_equals_per_op_forward(dev, rates, mode, monkeypatch):
    """dpmn_pgrm_forward_train_f32 (one native call per module) issues the same kernels in the same order as the per-op sequence of
    train/pgrm_train.py::forward: the output and every tensor saved for the backward are bitwise equal, with and without dropout,
    with the mask prior (mode=True, 3 channels) and the text prior through prior_fusion (mode=False, 2 channels)."""
    import ctypes as C
    from dpmn_amd.model.pgrm import PGRM
    from dpmn_amd.train import pgrm_train
    from dpmn_amd import _abi
    B, it = 4, 2
    pd, pa, pp = rates
    args = _pgrm_args()
    args.update(drop_rate=[pd] * 6, attn_drop_rate=[pa] * 6, drop_path_rate=[pp] * 6)
    m = PGRM(iter=it, mode=mode, hidden_size=3, **args)
    sd = m.state_dict()
    synth.synth_fill_(sd, 96)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x_q = (u("xq", (B, 1, 32, 128), 0, 1) > 0.5).float().repeat(1, 3 if mode else 2, 1, 1).to(dev)
    x_kv = u("xkv", (B, 3, 32, 128), 0, 1).to(dev)
    res = [u("r%d" % i, (B, 3, 32, 128), 0, 1).to(dev) for i in range(it)]
    assert _abi.lib.dpmn_pgrm_forward_train_supported(C.byref(m._weights()), B) == 1
    torch.manual_seed(77)
    drop = pgrm_train.drop_config(m)
    assert (drop is None) == (max(rates) == 0)
    outs = {}
    for native in (True, False):
        monkeypatch.setattr(pgrm_train, "NATIVE_FWD", native)
        out, sv = pgrm_train.forward(m, x_q, x_kv, res, drop)
        assert ("_slab" in sv) == native
        outs[native] = (out, sv)
    (o1, s1), (o0, s0) = outs[True], outs[False]
    assert torch.equal(o1, o0)
    for key in ("tq", "tkv_out", "c0", "c1"):
        assert torch.equal(s1[key].reshape(-1), s0[key].reshape(-1)), key
    for bi in range(2):
        for key, t0 in s0["blocks"][bi].items():
            t1 = s1["blocks"][bi][key]
            if torch.is_tensor(t0):
                assert torch.equal(t1.reshape(-1), t0.reshape(-1)[:t1.numel()]), "block %d %s" % (bi, key)
            elif key == "tables":
                assert all(a is b for a, b in zip(t0, t1))
            else:
                assert t1 == t0, "block %d %s" % (bi, key)
    # empty saved-tensor slots fail loudly before anything is launched
    with pytest.raises(_abi.DpmnError):
        w = m._weights()
        bad = _abi.PgrmSaved()
        _abi.check(_abi.lib.dpmn_pgrm_forward_train_f32(C.byref(w), _abi.dptr(x_q), x_q.shape[1], _abi.dptr(x_kv), _abi.ptr_array(res), len(res),
                                                        _abi.dptr(x_kv), _abi.dptr(x_kv), None, C.byref(bad), None, _abi.dptr(o1), B, _abi.stream()))


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.6)])
@pytest.mark.parametrize("mode", [True, False])
@pytest.mark.parametrize("native_fwd", [True, False])
def test_pgrm_native_block_backward_equals_per_op_backward(dev, rates, mode, native_fwd, monkeypatch):
    """dpmn_pgrm_blocks_backward_f32 (the Swin-block loop of the PGRM backward as one native call) issues the kernels of the per-op
    loop in the same order with the same arguments: every parameter gradient, dL/dx_kv and the residual gradients are bitwise
    equal -- with and without dropout, with the mask prior and the text prior (prior_fusion), behind the native and behind the per-op
    training forward (the saved tensors arrive as the forward's struct or are gathered from its dictionary)."""
    from dpmn_amd.model.pgrm import PGRM
    from dpmn_amd.train import pgrm_train
    B, it = 4, 2
    pd, pa, pp = rates
    args = _pgrm_args()
    args.update(drop_rate=[pd] * 6, attn_drop_rate=[pa] * 6, drop_path_rate=[pp] * 6)
    m = PGRM(iter=it, mode=mode, hidden_size=3, **args)
    sd = m.state_dict()
    synth.synth_fill_(sd, 94)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x_q = (u("xq", (B, 1, 32, 128), 0, 1) > 0.5).float().repeat(1, 3 if mode else 2, 1, 1).to(dev)
    x_kv = u("xkv", (B, 3, 32, 128), 0, 1).to(dev)
    res = [u("r%d" % i, (B, 3, 32, 128), 0, 1).to(dev) for i in range(it)]
    cot = u("cot", (B, 3, 32, 128), -1, 1).to(dev)
    monkeypatch.setattr(pgrm_train, "NATIVE_FWD", native_fwd)
    used = []
    orig = pgrm_train._blocks_backward_native
    monkeypatch.setattr(pgrm_train, "_blocks_backward_native", lambda *a, **k: (used.append(1), orig(*a, **k))[1])
    runs = {}
    for native in (True, False):
        monkeypatch.setattr(pgrm_train, "NATIVE_BWD", native)
        del used[:]
        for p in m.parameters():
            p.grad = None
        xk = x_kv.clone().requires_grad_(True)
        rs = [r.clone().requires_grad_(True) for r in res]
        torch.manual_seed(31)       # the same dropout seeds in both runs
        out = m(x_q, xk, rs)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        assert bool(used) == native
        runs[native] = [out.detach().clone(), xk.grad.clone()] + [None if r.grad is None else r.grad.clone() for r in rs] + \
                       [p.grad.clone() for p in m.parameters()]
    names = ["out", "dx_kv"] + ["dres%d" % i for i in range(it)] + [n for n, _ in m.named_parameters()]
    for n, a, b in zip(names, runs[True], runs[False]):
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(a, b), n


@pytest.mark.parametrize("cnum", [8, 16])
def test_cmm_train_forward_backward_vs_oracle_autograd(dev, cnum):
    """Train-mode CMM forward and every gradient vs torch autograd through the oracle.  The network is piecewise linear in its
    activations: an input whose pre-activation lies within round-off of zero gets the other branch of (Leaky)ReLU's derivative in one of
    the two implementations, and at these widths ONE such flip moves dx by ~1e-3 relative (4 of 12 (width, seed) pairs in a sweep show
    one; any change of a summation order moves it to other seeds).  So: up to three seeded weight / input sets; every one must agree
    to the flip level (2e-2: a wrong kernel is off by O(1) on all of them), and the first without a flip must agree to round-off."""
    from dpmn_amd.model.cmm import ComplementationModulationModule
    from oracle import cmm as ocmm
    from helpers import record
    B = 4
    tried = []
    for seed in (95, 96, 97):
        m = ComplementationModulationModule(cnum=cnum)
        sd = m.state_dict()
        synth.synth_fill_(sd, seed)
        m.load_state_dict(sd)
        x1, x2 = u("x1s%d" % seed, (B, 3, 32, 128), 0, 1), u("x2s%d" % seed, (B, 3, 32, 128), 0, 1)
        cot = u("cots%d" % seed, (B, 3, 32, 128), -1, 1)
        sd_ref = {k: v.clone().requires_grad_(torch.is_floating_point(v) and "running" not in k) for k, v in sd.items()}
        x1r, x2r = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        out_ref = ocmm.cmm_forward(sd_ref, x1r, x2r, True)
        (out_ref * cot).sum().backward()
        m = m.to(dev).train()
        x1d, x2d = x1.to(dev).requires_grad_(True), x2.to(dev).requires_grad_(True)
        out = m(x1d, x2d)
        assert_close(out, out_ref.detach(), 5e-4, 5e-4, "CMM train-mode forward (batch-statistics BatchNorm)")
        (out * cot.to(dev)).sum().backward()
        edx = max(l2_err(x1d.grad, x1r.grad), l2_err(x2d.grad, x2r.grad))
        tried.append((seed, edx))
        assert edx < 2e-2, "dx off by more than a derivative flip explains: %r" % (tried,)
        if edx < 1e-5:
            break
    assert tried[-1][1] < 1e-5, "no seed without a derivative flip among %r" % (tried,)
    record("cmm_train_cnum%d_B4" % cnum, "dx rel L2 (max of x1, x2; seed %d, flips on earlier seeds: %d)" % (tried[-1][0], len(tried) - 1), tried[-1][1], 1e-5)
    worst = ("", 0.0)
    for name, p in m.named_parameters():
        g_ref = sd_ref[name].grad
        if float(g_ref.abs().max()) < 2e-3:
            # conv biases in front of a train-mode BatchNorm have an exactly-zero true gradient (the batch mean removes
            # them); the reference only holds round-off there
            assert float(p.grad.abs().max()) < 5e-3, name
            continue
        e = l2_err(p.grad, g_ref)
        worst = max(worst, (name, e), key=lambda t: t[1])
        assert e < 1.5e-5, "grad %s L2 err %.2e (|ref|max %.2e)" % (name, e, float(g_ref.abs().max()))
    record("cmm_train_cnum%d_B4" % cnum, "worst parameter-gradient rel L2 (%s)" % worst[0], worst[1], 1.5e-5)
    # running statistics follow nn.BatchNorm2d (momentum 0.1, unbiased variance): compare one layer with torch's update
    import torch.nn.functional as F
    bn = m.en_2_1.encode[2]
    rm, rv = sd["en_2_1.encode.2.running_mean"].clone(), sd["en_2_1.encode.2.running_var"].clone()
    pre = F.conv2d(F.leaky_relu(F.conv2d(x1, sd["en_1_1.weight"], sd["en_1_1.bias"], padding=1), 0.2), sd["en_2_1.encode.1.weight"],
                   sd["en_2_1.encode.1.bias"], stride=2, padding=3, dilation=2)
    F.batch_norm(pre, rm, rv, None, None, True, 0.1, 1e-5)
    assert_close(bn.running_mean, rm, 1e-5, 1e-4, "running_mean")
    assert_close(bn.running_var, rv, 1e-5, 1e-4, "running_var")
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("B", [2, 48])
def test_cmm_grouped_twin_data_gradients_equal_per_branch_launches(dev, B, monkeypatch):
    """The data gradients of the twin encoder branches as one grouped launch per level (train/cmm_train.py backward_pair) against one
    launch per branch: same sums up to the order of the split-K partial sums (fewer splits over twice the pixels), every parameter and
    input gradient within 1e-5 relative L2 (measured: 2.1e-6 on the first conv's bias, a sum over 4.7 M pixels); with the switch off no level
    is paired."""
    from dpmn_amd.model.cmm import ComplementationModulationModule
    from dpmn_amd.train import cmm_train
    m = ComplementationModulationModule(cnum=64)
    sd = m.state_dict()
    synth.synth_fill_(sd, 98)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x1, x2 = u("gx1", (B, 3, 32, 128), 0, 1).to(dev), u("gx2", (B, 3, 32, 128), 0, 1).to(dev)
    cot = u("gcot", (B, 3, 32, 128), -1, 1).to(dev)
    calls = []
    orig = cmm_train.backward_pair
    monkeypatch.setattr(cmm_train, "backward_pair", lambda *a, **k: (calls.append(a[0].kind), orig(*a, **k))[1])
    res = {}
    for on in (True, False):
        monkeypatch.setattr(cmm_train, "GROUP_BWD", on)
        monkeypatch.setattr(cmm_train, "GROUP_BWD_MAXPIX", 1 << 30)
        del calls[:]
        for p in m.parameters():
            p.grad = None
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        (m(a, b) * cot).sum().backward()
        torch.cuda.synchronize()
        res[on] = ([a.grad.clone(), b.grad.clone()] + [p.grad.clone() for p in m.parameters()], list(calls))
    assert res[False][1] == []
    # B = 48: all four levels of (dilated stride-2 conv, 3 x 3 conv) fill whole row tiles; B = 2: the two launches of the deepest level
    # (2 x 16 = 32 pixels per branch) do not and fall back to per-branch launches
    assert len(res[True][1]) == (8 if B == 48 else 6), res[True][1]
    names = ["dx1", "dx2"] + [n for n, _ in m.named_parameters()]
    worst = 0.0
    # fp32: the grouped launch and the two per-branch launches run the SAME kernel on the same operands in another tile order (2e-6).
    # Mode 2: the grouped 3 x 3 of a level may take the implicit-GEMM kernel (bf16x3) where the per-branch launches take the halo kernel
    # (fp32 at these sizes): two fp32-class results of different arithmetic, 1.0e-5 at the worst tensor -- the bar is 3x that
    from dpmn_amd import _abi
    tol = 3e-5 if _abi.lib.dpmn_get_compute_dtype() == 2 else 1e-5
    for n, g1, g0 in zip(names, res[True][0], res[False][0]):
        if float(g0.abs().max()) < 2e-3:
            continue      # bias in front of a train-mode BatchNorm: zero fill
        e = l2_err(g1, g0)
        worst = max(worst, e)
        assert e < tol, (n, e)
    from helpers import record
    record("cmm_grouped_dgrad_B%d" % B, "worst gradient rel L2, grouped vs per-branch data gradients", worst, tol)


@pytest.mark.parametrize("cnum,B", [(64, 4), (64, 6)])
def test_cmm_backward_is_bitwise_reproducible(dev, cnum, B):
    """Every gradient of the CMM's training step -- conv weight gradients (exclusive slots), BatchNorm backward (fp64 per-channel
    sums folded into the last consumer), bias column sums (per-block partials in block order), the channel gate -- and both input
    gradients are independent of the order in which workgroups finish: three runs of forward + backward give identical bits.
    (cnum = 64, the only width the trainer builds, super_resolution.py:72: a 3 -> 16 channel first conv of a narrower CMM would
    take the slotted-atomic weight-gradient path of the tiny convs, which is not order-independent.)"""
    from dpmn_amd.model.cmm import ComplementationModulationModule
    m = ComplementationModulationModule(cnum=cnum)
    sd = m.state_dict()
    synth.synth_fill_(sd, 97)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x1, x2 = u("rx1", (B, 3, 32, 128), 0, 1).to(dev), u("rx2", (B, 3, 32, 128), 0, 1).to(dev)
    cot = u("rcot", (B, 3, 32, 128), -1, 1).to(dev)
    runs = []
    for _ in range(3):
        for p in m.parameters():
            p.grad = None
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        out = m(a, b)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        runs.append([out.detach().clone(), a.grad.clone(), b.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    names = ["out", "dx1", "dx2"] + [n for n, _ in m.named_parameters()]
    for r in runs[1:]:
        bad = [n for n, t0, t1 in zip(names, runs[0], r) if not torch.equal(t0, t1)]
        assert not bad, "not bitwise reproducible: %s" % bad[:8]


def test_distill_module_train_vs_oracle_autograd(dev):
    from dpmn_amd.model.distill_module import DistillModule
    from oracle import cmm as ocmm
    from helpers import load_golden
    B = 4
    m = DistillModule()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(r).split("|")[0] for r in load_golden("distill")["manifest"]]
    synth.synth_fill_(sd, 32)
    m.load_state_dict(sd)
    xd, xs = u("xd", (B, 3, 32, 128), 0, 1), u("xs", (B, 3, 32, 128), 0, 1)
    cot = u("cotf", (B, 3, 32, 128), -0.01, 0.01)
    sd_ref = {k: v.clone().requires_grad_(torch.is_floating_point(v) and "running" not in k) for k, v in sd.items()}
    xdr, xsr = xd.clone().requires_grad_(True), xs.clone().requires_grad_(True)
    loss_ref, feat_ref = ocmm.distill_forward(sd_ref, xdr, xsr, True)
    (loss_ref * 100 + (feat_ref * cot).sum()).backward()
    m = m.to(dev).train()
    xdd, xsd = xd.to(dev).requires_grad_(True), xs.to(dev).requires_grad_(True)
    loss, feat = m(xdd, xsd)
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    assert_close(feat, feat_ref.detach(), 1e-4, 1e-4, "distill feature")
    (loss * 100 + (feat * cot.to(dev)).sum()).backward()
    assert l2_err(xdd.grad, xdr.grad) < 2e-2 and l2_err(xsd.grad, xsr.grad) < 2e-2
    for name, p in m.named_parameters():
        g_ref = sd_ref[name].grad
        if float(g_ref.abs().max()) < 2e-3:
            assert float(p.grad.abs().max()) < 5e-3, name
        else:
            assert l2_err(p.grad, g_ref) < 2e-2, name


def test_clip_adam_matches_torch(dev):
    from dpmn_amd.train.optim import FlatBucket
    lin = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7))
    ref = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7))
    ref.load_state_dict(lin.state_dict())
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.5, 0.999))
    lin = lin.to(dev)
    b = FlatBucket(lin)
    for step in range(1, 4):
        gs = [u("g%d_%d" % (step, i), p.shape, -1, 1) for i, p in enumerate(ref.parameters())]
        for p, g in zip(ref.parameters(), gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.25)
        opt.step()
        b.zero_grad()
        for p, g in zip(lin.parameters(), gs):
            p.grad += g.to(dev)
        b.step(step, 1e-3, 0.5)
        for p, q in zip(lin.parameters(), ref.parameters()):
            assert_close(p.detach(), q.detach(), 1e-6, 1e-5, "adam step %d" % step)


def test_full_train_step_vs_oracle_autograd(dev):
    """TSRN PSN + 2+2 PGRM + 2 DistillModules + CMM, B=2: loss value and every parameter after ONE step
    (zero_grad -> forward -> loss -> backward -> per-model clip 0.25 -> Adam) vs torch autograd on the CPU oracle."""
    from types import SimpleNamespace
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from oracle import dpmn as odpmn, pgrm as opgrm, cmm as ocmm, tsrn as otsrn
    B, b1, b2 = 2, 2, 2
    sr_ = TextSR(workload.make_config(B), workload.make_args("tsrn", b1, b2, B))
    models, psn, distill, crit, trainer = sr_.build_training()
    for i, m in enumerate([psn] + models + distill):
        sd = m.state_dict()
        synth.synth_fill_(sd, 300 + i)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(sd[k])
    psn.eval()
    sd0 = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in [psn] + models + distill]
    batch = synth.synth_batch(B, seed=4)
    priors = [torch.floor(synth.uniform("tp%d" % k, (B, 2, 32, 128), 0, 256, 4)) for k in range(b1)]
    loss = sr_.train_step(models, psn, distill, crit, trainer, batch["images_lr"].to(dev), batch["images_hr"].to(dev), None,
                          text_priors=[p.to(dev) for p in priors])
    # ---- oracle step on the CPU
    ref = [{k: v.clone().requires_grad_(torch.is_floating_point(v) and "running" not in k and "index" not in k and "mask" not in k)
            for k, v in sd.items()} for sd in sd0]
    with torch.no_grad():
        lr_psn = otsrn.tsrn_forward(sd0[0], batch["images_lr"])
    hr3 = batch["images_hr"][:, :3]
    tot, casc, l1, l2 = 0, lr_psn, [], []
    for k in range(b1):
        o = opgrm.pgrm_forward(ref[1 + k], priors[k], casc[:, :3], l1[:k]); l1.append(o); casc = o
        tot = tot + ocmm.image_loss(o, hr3, True) * 100
    casc = lr_psn
    for k in range(b1, b1 + b2):
        o = opgrm.pgrm_forward(ref[1 + k], ocmm.to_mask(casc.detach()[:, :3]), casc[:, :3], l2[:k - b2]); l2.append(o); casc = o
        tot = tot + ocmm.image_loss(o, hr3, True) * 100
    nm = 1 + b1 + b2 + 1
    feat = l1[-1]
    for k in range(b1 - 1, 0, -1):
        ld, feat = ocmm.distill_forward(ref[nm + k - 1], feat, l1[k - 1], True); tot = tot + ld * 100
    feat = l2[-1]
    for k in range(b2 - 1, 0, -1):
        ld, feat = ocmm.distill_forward(ref[nm + k + b1 - 2], feat, l2[k - 1], True); tot = tot + ld * 100
    o = ocmm.cmm_forward(ref[1 + b1 + b2], l1[-1], l2[-1], True)
    tot = (tot + ocmm.image_loss(o, hr3, True) * 100) / (b1 + b2 + 1)
    tot.backward()
    assert abs(float(loss) - float(tot)) < 2e-6 * abs(float(tot)), (float(loss), float(tot))
    # gradients of every model vs oracle autograd (the fused clip+Adam kernel is pinned separately above; comparing
    # Adam's first, sign-like update would amplify round-off on near-zero gradients)
    mods = models + distill
    for i, m in enumerate(mods):
        rsd = ref[1 + i]
        num, den, worst = 0.0, 0.0, ("", 0.0)
        for n, p_ in m.named_parameters():
            g_ref = rsd[n].grad if rsd[n].grad is not None else torch.zeros_like(rsd[n])
            d = (p_.grad.detach().cpu().double() - g_ref.double())
            num += float((d * d).sum()); den += float((g_ref.double() ** 2).sum())
            if float(g_ref.abs().max()) > 1e-3:
                e = float(d.norm() / g_ref.double().norm())
                worst = max(worst, (n, e), key=lambda t_: t_[1])
        tot_err = (num / max(den, 1e-30)) ** 0.5
        from helpers import record
        # 3x the recorded errors (r03l: text-prior PGRMs 3.1e-5, mask-prior PGRMs 2.2e-4, CMM 3.6e-4, DistillModules 8e-7), floor 1e-5
        tol = 1e-4 if i < b1 else 7e-4 if i < b1 + b2 else 1.1e-3 if i == b1 + b2 else 1e-5
        record("full_train_step_tsrn2p2_B2", "model %d whole-gradient rel L2 (worst tensor %s %.2e)" % (i, worst[0], worst[1]), tot_err, tol)
        assert tot_err < tol, "model %d gradient differs from oracle autograd: %.3e (%s %.3e)" % (i, tot_err, worst[0], worst[1])


def test_checkpoint_roundtrip_reference_format(tmp_path):
    """base.py:328-358 / 163-197: files written from flat-bucket-backed models load back (reference dict keys) and the
    restored model reproduces the forward bit for bit."""
    from dpmn_amd import workload
    from dpmn_amd.train.optim import Trainer
    sr, models, psn, inp = workload.build("cfg0")
    for m in models:
        for p in m.parameters():
            p.requires_grad = True
    Trainer(models)                      # parameters become views into padded flat buffers
    sr.vis_dir = str(tmp_path)
    sr.save_checkpoint(models, epoch=3, iters=7, best_acc_dict={}, best_model_info={}, is_best=True, converge_list=[], metric="sum")
    x_q, x_kv = inp["text_priors"][0], inp["images_hr"][:, :3].contiguous()
    with torch.no_grad():
        ref = models[0](x_q, x_kv, [])
    ck = torch.load(os.path.join(str(tmp_path), "ckpt", "model_best_sum_3_0.pth"), map_location="cpu")
    assert set(ck.keys()) == {"state_dict_G", "info", "best_history_res", "best_model_info", "param_num", "converge"}
    assert ck["info"]["arch"] == "tsrn" and ck["param_num"] == sum(p.numel() for p in models[0].parameters())
    fresh = sr.generator_init(iter=0, mode=False, hidden_size=3)["model"].eval()
    fresh.load_state_dict(ck["state_dict_G"])
    with torch.no_grad():
        out = fresh(x_q, x_kv, [])
    assert torch.equal(out, ref)


def test_graphed_train_step_matches_eager(dev):
    """One hipGraph capture of the whole training step replays to the same losses / parameters as the eager step
    (Adam's step count is read from device memory so the bias corrections advance across replays)."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    B, b1, b2 = 2, 2, 2

    def fresh():
        sr_ = TextSR(workload.make_config(B), workload.make_args("tsrn", b1, b2, B))
        models, psn, distill, crit, trainer = sr_.build_training()
        for i, m in enumerate([psn] + models + distill):
            sd = m.state_dict()
            synth.synth_fill_(sd, 500 + i)
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(sd[k])
        psn.eval()
        return sr_, models, psn, distill, crit, trainer

    batches = [synth.synth_batch(B, seed=20 + i) for i in range(2)]
    priors = [[torch.floor(synth.uniform("gtp%d_%d" % (i, k), (B, 2, 32, 128), 0, 256, 4)).to(dev) for k in range(b1)] for i in range(2)]
    warm = 2
    # eager: one step on each batch from the fresh state (the capture's warm-up steps are undone: parameters, Adam state and
    # BatchNorm running statistics are snapshotted before and restored after the capture)
    sr_, models, psn, distill, crit, trainer = fresh()
    lr0, hr0 = batches[0]["images_lr"].to(dev), batches[0]["images_hr"].to(dev)
    eager_losses = [float(sr_.train_step(models, psn, distill, crit, trainer, b["images_lr"].to(dev), b["images_hr"].to(dev), None,
                                         text_priors=priors[i])) for i, b in enumerate(batches)]
    eager_params = [p.detach().clone() for m in models for p in m.parameters()]
    # graphed
    sr_, models, psn, distill, crit, trainer = fresh()
    run = sr_.graphed_train_step(models, psn, distill, crit, trainer, lr0, hr0, None, priors[0], warmup=warm)
    graph_losses = [float(run(b["images_lr"].to(dev), b["images_hr"].to(dev), None, priors[i])) for i, b in enumerate(batches)]
    # the eager step is itself not bit-reproducible (fp32 atomics in BatchNorm statistics / weight gradients feed Adam's
    # sign-like early updates: 0.1 % run-to-run spread on the first loss, ~1 % a step later -- tools/dbg_graph.py), so this
    # checks agreement within that spread; the device-side step counter is pinned exactly in the test below
    assert abs(eager_losses[0] - graph_losses[0]) < 5e-3 * abs(eager_losses[0]), (eager_losses, graph_losses)
    assert abs(eager_losses[1] - graph_losses[1]) < 3e-2 * abs(eager_losses[1]), (eager_losses, graph_losses)
    assert graph_losses[1] < graph_losses[0]


def test_graph_replay_invalidates_eval_packs(dev):
    """replay -> eval -> replay -> eval: the evals between graph replays must see the parameters the replayed optimizer
    kernels wrote (raw pointers: no torch version counter moves), not the CMM packs / LayerNorm-folded attention weights
    cached by the previous eval."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    B, b1, b2 = 2, 1, 1
    sr_ = TextSR(workload.make_config(B), workload.make_args("tsrn", b1, b2, B))
    models, psn, distill, crit, trainer = sr_.build_training()
    for i, m in enumerate([psn] + models + distill):
        sd = m.state_dict()
        synth.synth_fill_(sd, 520 + i)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(sd[k])
    psn.eval()
    b = synth.synth_batch(B, seed=23)
    lr, hr = b["images_lr"].to(dev), b["images_hr"].to(dev)
    priors = [torch.floor(synth.uniform("rtp%d" % k, (B, 2, 32, 128), 0, 256, 4)).to(dev) for k in range(b1)]
    run = sr_.graphed_train_step(models, psn, distill, crit, trainer, lr, hr, None, priors, warmup=2)

    def evaluate(drop_caches):
        for m in models:
            m.eval()
            if drop_caches:
                m._pack = None
                if hasattr(m, "_fold_key"):
                    m._fold_key = None
        with torch.no_grad():
            out = sr_.refine(models, psn, lr, None, text_priors=priors).clone()
        for m in models:
            m.train()
        return out
    outs = []
    for _ in range(2):
        run(lr, hr, None, priors)
        got = evaluate(False)
        want = evaluate(True)
        assert torch.equal(got, want), "eval after a graph replay used stale packs: max diff %g" % float((got - want).abs().max())
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])


def test_adam_device_step_counter_equals_host_step(dev):
    from dpmn_amd.train.optim import FlatBucket
    torch.manual_seed(3)
    a, b = torch.nn.Linear(33, 17).to(dev), torch.nn.Linear(33, 17).to(dev)
    b.load_state_dict(a.state_dict())
    ba, bb = FlatBucket(a), FlatBucket(b)
    t_dev = torch.zeros(1, device=dev)
    for step in range(1, 5):
        g = [torch.randn_like(p) * 0.1 for p in a.parameters()]
        for bk, m in ((ba, a), (bb, b)):
            bk.zero_grad()
            for p, gi in zip(m.parameters(), g):
                p.grad += gi
        t_dev.add_(1.0)
        ba.step(step, 1e-3, 0.5)
        bb.step(0, 1e-3, 0.5, step_dev=t_dev)
        for p, q in zip(a.parameters(), b.parameters()):
            assert_close(p.detach(), q.detach(), 1e-7, 1e-6, "adam device step %d" % step)


# ---------------------------------------------------------------------------------------------------------------------
# HIP backward vs gradients captured from the IMPORTED reference itself (tests/golden/grads_*.npz, step_tsrn_2p2.npz;
# tools/gen_golden.py gen_grads / gen_step) -- not only vs autograd through the oracle.
def _fixture_check(test, g, named, prefix="", tol=3e-3):
    from helpers import fixture_grad_names, grad_error_vs_fixture, record
    worst = ("", 0.0)
    for n in fixture_grad_names(g, prefix):
        err, amax = grad_error_vs_fixture(g, prefix + n, named[n])
        if amax < 2e-3:      # exactly-zero true gradients: both sides hold round-off
            assert float(torch.as_tensor(named[n]).abs().max()) < 5e-3, n
            continue
        worst = max(worst, (n, err), key=lambda x: x[1])
        assert err < tol, "gradient %s%s differs from the reference's own by %.2e" % (prefix, n, err)
    record(test, "worst gradient error vs reference fixture (%s%s)" % (prefix, worst[0]), worst[1], tol)


@pytest.mark.parametrize("tag,it,mode", [("mode0_iter0", 0, False), ("mode1_iter2", 2, True)])
def test_pgrm_backward_vs_reference_gradient_fixture(dev, tag, it, mode):
    from dpmn_amd.model.pgrm import PGRM
    from helpers import load_golden, t
    B = 2
    g = load_golden("grads_pgrm_" + tag)
    m = PGRM(iter=it, mode=mode, hidden_size=3, **_pgrm_args())
    sd = m.state_dict()
    synth.synth_fill_(sd, 11 + it)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    if mode:
        x_q = (synth.uniform("x_q", (B, 1, 32, 128), 0, 1, 5) > 0.5).float().repeat(1, 3, 1, 1)
    else:
        x_q = torch.floor(synth.uniform("x_q", (B, 2, 32, 128), 0, 256, 5))
    x_kv = synth.uniform("x_kv", (B, 3, 32, 128), 0, 1, 5).to(dev).requires_grad_(True)
    res = [synth.uniform("res%d" % i, (B, 3, 32, 128), 0, 1, 5).to(dev).requires_grad_(True) for i in range(it)]
    cot = synth.uniform("cot", (B, 3, 32, 128), -1, 1, 5).to(dev)
    out = m(x_q.to(dev), x_kv, res)
    assert_close(out, t(g["out"]), 3e-4, 3e-4, "train-mode forward vs the reference's")
    (out * cot).sum().backward()
    named = {"x_kv": x_kv.grad}
    named.update({"res%d" % i: r.grad for i, r in enumerate(res) if r.grad is not None})
    named.update({n: p.grad for n, p in m.named_parameters()})
    _fixture_check("pgrm_grads_" + tag, g, named, tol=1e-5)


@pytest.mark.parametrize("cnum", [8, 64])
def test_cmm_backward_vs_reference_gradient_fixture(dev, cnum):
    from dpmn_amd.model.cmm import ComplementationModulationModule
    from helpers import load_golden, t
    B = 2
    g = load_golden("grads_cmm_cnum%d" % cnum)
    m = ComplementationModulationModule(cnum=cnum)
    sd = m.state_dict()
    synth.synth_fill_(sd, 31)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x1 = synth.uniform("cmm_x1", (B, 3, 32, 128), 0, 1, 7).to(dev).requires_grad_(True)
    x2 = synth.uniform("cmm_x2", (B, 3, 32, 128), 0, 1, 7).to(dev).requires_grad_(True)
    cot = synth.uniform("cmm_cot", (B, 3, 32, 128), -1, 1, 7).to(dev)
    out = m(x1, x2)
    assert_close(out, t(g["out"]), 5e-4, 5e-4, "CMM train forward vs the reference's")
    (out * cot).sum().backward()
    named = {"x1": x1.grad, "x2": x2.grad}
    named.update({n: p.grad for n, p in m.named_parameters()})
    if cnum == 8:
        _fixture_check("cmm_grads_cnum8", g, named, tol=1e-5)
    else:
        # The reference's OWN fp32 gradients are up to 6.6e-3 away from a float64 run of the same modules -- not because of the
        # 8-sample BatchNorm statistics at the 1 x 4 bottleneck (the explanation of rounds 4-5) but because one of the 2 M LeakyReLU /
        # ReLU inputs that lie within fp32 round-off of the kink takes the other derivative branch in its fp32 run (en_2_1); this
        # library's run flips another one (en_4_1: tools/dbg_cnum64_f64.py).  float64 arbitrates AFTER taking the implementation's
        # own branch at those 15 listed elements (helpers "Kink-aware float64 adjudication"): both implementations are then within
        # ~2e-6 of float64 on every tensor, and the common bar applies (worst / RMS within 3x the reference's, every tensor within 10x).
        from dpmn_amd.train import cmm_train
        from helpers import cmm_grads_f64, check_adjudicated, rel_l2, record
        z = load_golden("grads_cmm_cnum64_f64")
        with torch.no_grad():
            _, graph = cmm_train.build(m, x1.detach(), x2.detach())
        names = {id(mod): n for n, mod in m.named_modules()}
        prod = {"gate": graph["gated"]}
        for u_ in graph["units"]:
            if u_.out is not None and u_.out.r is not None:
                prod[names[id(u_.bn if u_.bn is not None else u_.conv)]] = u_.out
        forced, flips = [], 0
        for site, i, y64 in zip(z["kink_site"], z["kink_index"], z["kink_y64"]):
            tns = prod[str(site).split(">")[0]]
            Bq, Hq, Wq, Cq = tns.r.shape
            i = int(i)
            c_, h_, w_ = (i // (Hq * Wq)) % Cq, (i // Wq) % Hq, i % Wq
            b_ = i // (Cq * Hq * Wq)
            y = tns.r[b_, h_, w_, c_]
            if tns.scale is not None:
                y = y * tns.scale[c_] + tns.shift[c_]          # mul, then add: the kernels' on-load affine (-ffp-contract=off)
            forced.append((str(site), i, bool(y > 0)))
            flips += int(bool(y > 0) != (float(y64) > 0))
        record("cmm_grads_cnum64_f64", "pre-activations within %g of a kink where this run takes the other branch than float64 (of %d)" % (2e-6, len(forced)), flips)
        sd_cpu = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        g64 = cmm_grads_f64(sd_cpu, x1.detach().cpu(), x2.detach().cpu(), cot.cpu(), forced)
        gmax = max(float(v.abs().max()) for v in g64.values())
        nm, e_ours, e_ref = [], [], []
        for n_, g_ in named.items():
            if float(g64[n_].abs().max()) < 1e-9:          # exactly zero by construction (conv biases in front of a batch-statistics BatchNorm)
                assert float(g_.abs().max()) <= 1e-5 * gmax, (n_, float(g_.abs().max()))
                continue
            nm.append(n_); e_ours.append(rel_l2(g_, g64[n_])); e_ref.append(float(z[n_ + "::ref32_err_adj"]))
        check_adjudicated("cmm_grads_cnum64_f64", nm, e_ours, e_ref, factor=3.0, per_tensor=10.0)


def test_training_step_vs_reference_step_fixture(dev):
    """The a19 'step' fixture: loss, cascade images and per-model clip norms / gradients of one step of
    super_resolution.py:140-278 run on the imported reference modules (same seeds as the oracle-autograd test above)."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from helpers import load_golden, t, record
    g = load_golden("step_tsrn_2p2")
    B, b1, b2 = 2, 2, 2
    sr_ = TextSR(workload.make_config(B), workload.make_args("tsrn", b1, b2, B))
    models, psn, distill, crit, trainer = sr_.build_training()
    for i, m in enumerate([psn] + models + distill):
        sd = m.state_dict()
        synth.synth_fill_(sd, 300 + i)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(sd[k])
    psn.eval()
    batch = synth.synth_batch(B, seed=4)
    priors = [torch.floor(synth.uniform("tp%d" % k, (B, 2, 32, 128), 0, 256, 4)).to(dev) for k in range(b1)]
    loss = sr_.train_step(models, psn, distill, crit, trainer, batch["images_lr"].to(dev), batch["images_hr"].to(dev), None,
                          text_priors=priors)
    le = abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))
    record("step_fixture", "loss rel err vs reference", le, 1e-5)
    assert le < 1e-5
    # gradients: adjudicated by the float64 run of the same step (tests/golden/step_tsrn_2p2_f64.npz): per model, our worst tensor /
    # RMS error against float64 within helpers.check_vs_f64's factor of the reference's own fp32 gradients' (which are up to 5.6e-3
    # off at this batch of 2); the clip norm likewise against the float64 norm
    from helpers import check_vs_f64
    z = load_golden("step_tsrn_2p2_f64")
    l64 = abs(float(loss) - float(z["loss"])) / abs(float(z["loss"]))
    record("step_fixture_f64", "loss rel err vs float64 (reference fp32: %.1e)" % float(z["loss_ref32_err"]), l64, 3.0 * float(z["loss_ref32_err"]) + 2e-7)
    assert l64 <= 3.0 * float(z["loss_ref32_err"]) + 2e-7
    for i, m in enumerate(models + distill):
        named = {n: p.grad for n, p in m.named_parameters()}
        norm = float(torch.sqrt(sum((v.double() ** 2).sum() for v in named.values())))
        ne = abs(norm - float(z["grad_norms"][i])) / float(z["grad_norms"][i])
        ntol = 3.0 * float(z["grad_norms_ref32_err"][i]) + 1e-5
        record("step_fixture_f64", "model %d clip-norm rel err vs float64 (reference fp32: %.1e)" % (i, float(z["grad_norms_ref32_err"][i])), ne, ntol)
        assert ne < ntol, "model %d: the norm clip_grad_norm_ sees is %.2e from the float64 norm (reference fp32: %.2e)" % (i, ne, float(z["grad_norms_ref32_err"][i]))
        check_vs_f64("step_fixture_f64", z, named, "m%d/" % i)


def test_test_mode_loads_every_checkpoint_including_cmm(dev, tmp_path):
    """TextSR.test() (super_resolution.py:515-775): PGRMs from model_best_{k}.pth, CMM from model_best_cmm.pth (570-582), PSN
    from model_{arch}.pth -- written by save_checkpoint's format, evaluated through test(), equal to refine() on the
    original models; a missing CMM file is an error, never a silently random CMM."""
    import types
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    sr, models, psn, inp = workload.build("cfg0")
    ref = sr.refine(models, psn, inp["images_lr"], None, text_priors=inp["text_priors"])
    d = str(tmp_path)
    pack = lambda m: {"state_dict_G": {k: v.detach().clone() for k, v in m.state_dict().items()}}
    torch.save(pack(psn), os.path.join(d, "model_tsrn.pth"))
    for k, m in enumerate(models[:-1]):
        torch.save(pack(m), os.path.join(d, "model_best_%d.pth" % k))
    args = workload.make_args("tsrn", 1, 1, 4)
    args.resume = d
    sr2 = TextSR(workload.make_config(4), args)
    loader = [(inp["images_hr"], inp["images_lr"], None)]
    with pytest.raises(FileNotFoundError, match="model_best_cmm.pth"):
        sr2.test(loader)
    torch.save({"state_dict_G": {"module." + k: v.detach().clone() for k, v in models[-1].state_dict().items()}},
               os.path.join(d, "model_best_cmm.pth"))           # the ngpu > 1 key style is accepted too
    got = {}
    orig = sr2.refine
    sr2.refine = types.MethodType(lambda self, *a, **kw: got.setdefault("out", orig(*a, **kw)), sr2)
    res = sr2.test(loader)
    assert res["accuracy"] is None and res["psnr_avg"] == res["psnr_avg"]      # not computed is None, never a fake 0.0
    fn = sr2.synthetic_text_prior()
    ref2 = sr.refine(models, psn, inp["images_lr"], None, text_prior_fn=fn)
    assert torch.equal(got["out"], ref2)


def test_training_step_is_bitwise_reproducible(dev):
    """Two runs of THREE optimisation steps of the configs[2] stack (TATT PSN + 3+3 PGRM + 4 DistillModules + CMM) from the same
    state: every loss, every gradient of the last step and every parameter after it are bitwise equal.  Nothing on the step ends
    in a floating-point atomic whose order could vary: BatchNorm statistics are fp64 sums (order-independent after the final
    rounding), every other reduction is a set of per-block / per-image / per-split partial rows added in a fixed order."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from helpers import record
    B, b1, b2 = 4, 3, 3
    runs = []
    for _ in range(2):
        sr_ = TextSR(workload.make_config(B), workload.make_args("tatt", b1, b2, B))
        models, psn, distill, crit, trainer = sr_.build_training()
        for i, m in enumerate([psn] + models + distill):
            sd = m.state_dict()
            synth.synth_fill_(sd, 300 + i)
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(sd[k])
        psn.eval()
        losses = []
        for step in range(3):
            batch = synth.synth_batch(B, seed=4 + step)
            priors = [torch.floor(synth.uniform("tp%d_%d" % (k, step), (B, 2, 32, 128), 0, 256, 4)).to(dev) for k in range(b1)]
            losses.append(sr_.train_step(models, psn, distill, crit, trainer, batch["images_lr"].to(dev), batch["images_hr"].to(dev),
                                         batch["label_vecs"].to(dev), text_priors=priors).clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), trainer.flat_g.clone(), trainer.flat_p.clone(),
                     torch.cat([b_.reshape(-1).float() for m in models + distill for b_ in m.buffers()])))
    assert torch.equal(runs[0][0], runs[1][0]), "losses differ between runs: %r vs %r" % (runs[0][0].tolist(), runs[1][0].tolist())
    ndiff_g = int((runs[0][1] != runs[1][1]).sum())
    ndiff_p = int((runs[0][2] != runs[1][2]).sum())
    record("train_step_reproducibility", "gradient words differing between two runs (of %d)" % runs[0][1].numel(), ndiff_g, 0)
    record("train_step_reproducibility", "parameter words differing after 3 steps (of %d)" % runs[0][2].numel(), ndiff_p, 0)
    assert ndiff_g == 0 and ndiff_p == 0, (ndiff_g, ndiff_p)
    assert torch.equal(runs[0][3], runs[1][3]), "BatchNorm running statistics differ between runs"
    assert float(runs[0][0][2]) != float(runs[0][0][0])


def test_psn_prefetch_equals_in_step_psn(dev):
    """train_step(psn_out=..., prefetch=...): the frozen PSN's image of the next batch computed on a lane stream during the current
    step gives bitwise the losses and parameters of the plain step over three different batches (TATT PSN, label vectors)."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    B, b1, b2 = 2, 1, 1
    res = []
    for use in (False, True):
        sr_ = TextSR(workload.make_config(B), workload.make_args("tatt", b1, b2, B))
        models, psn, distill, crit, trainer = sr_.build_training()
        for i, m in enumerate([psn] + models + distill):
            sd = m.state_dict()
            synth.synth_fill_(sd, 900 + i)
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(sd[k])
        psn.eval()
        bs = [synth.synth_batch(B, seed=70 + i) for i in range(3)]
        bs = [(b["images_lr"].to(dev), b["images_hr"].to(dev), b["label_vecs"].to(dev)) for b in bs]
        pri = [torch.floor(synth.uniform("pf_tp", (B, 2, 32, 128), 0, 256, 4)).to(dev)]
        losses, handle = [], None
        for i, (lr, hr, lv) in enumerate(bs):
            nxt = bs[i + 1] if use and i + 1 < len(bs) else None
            losses.append(sr_.train_step(models, psn, distill, crit, trainer, lr, hr, lv, text_priors=pri, psn_out=handle,
                                         prefetch=None if nxt is None else (nxt[0], nxt[2])).clone())
            handle = sr_.psn_prefetched
            assert (handle is not None) == (nxt is not None)
        torch.cuda.synchronize()
        res.append((torch.stack(losses), trainer.flat_p.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_step_that_never_reaches_the_optimizer_leaves_complete_gradients(dev):
    """train_step arms the lazy weight-gradient join (the CMM backward returns while its conv weight gradients are still on the side
    stream, Trainer.arm_early_step).  If step() is never reached -- here it raises -- the promise must end with the call: the
    gradient arena read on the current stream right afterwards is complete (bitwise the arena of a step that did reach the
    optimizer, read at the same point), the buckets are disarmed, and the NEXT step's zero fill does not race a late unpack (its
    losses and parameters equal those of an undisturbed run)."""
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    B, b1, b2 = 4, 1, 1
    out = []
    for fail in (False, True):
        sr_ = TextSR(workload.make_config(B), workload.make_args("tsrn", b1, b2, B))
        models, psn, distill, crit, trainer = sr_.build_training()
        for i, m in enumerate([psn] + models + distill):
            sd = m.state_dict()
            synth.synth_fill_(sd, 500 + i)
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(sd[k])
        psn.eval()
        batch = synth.synth_batch(B, seed=9)
        args = (batch["images_lr"].to(dev), batch["images_hr"].to(dev), None)
        pri = [torch.floor(synth.uniform("lz_tp", (B, 2, 32, 128), 0, 256, 4)).to(dev)]
        grads = {}
        real_step = trainer.step

        def step_hook():
            if fail:
                raise RuntimeError("injected: the optimizer is never reached")
            trainer.disarm()
            grads["g"] = trainer.flat_g.clone()
            real_step()
        trainer.step = step_hook
        if fail:
            with pytest.raises(RuntimeError, match="injected"):
                sr_.train_step(models, psn, distill, crit, trainer, *args, text_priors=pri)
            grads["g"] = trainer.flat_g.clone()         # read on the current stream, no synchronize: disarm() ordered it
            assert not any(getattr(b, "lazy_join", False) for b in trainer.buckets)
            assert all(getattr(b, "ready_event", None) is None for b in trainer.buckets)
            trainer.step = real_step
            trainer.step()                              # finish the interrupted step by hand
        else:
            sr_.train_step(models, psn, distill, crit, trainer, *args, text_priors=pri)
        trainer.step = real_step
        l2 = sr_.train_step(models, psn, distill, crit, trainer, *args, text_priors=pri).clone()
        torch.cuda.synchronize()
        out.append((grads["g"], l2, trainer.flat_p.clone()))
    assert torch.equal(out[0][0], out[1][0]), "gradients read after the interrupted step are incomplete"
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
