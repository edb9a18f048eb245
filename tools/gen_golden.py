#!/usr/bin/env python3
"""Generate tests/golden/*.npz by importing the READ-ONLY reference (/root/reference) on CPU.

Runs only in the build container (the reference never travels to the GPU box).  Weights and
inputs are NOT stored: both sides regenerate them from dpmn_amd.utils.synth (name-seeded
uniform draws), so a fixture holds only the reference's outputs, the state-dict manifest
(names + shapes) and a float64 checksum of the synthetic weights.

usage: python tools/gen_golden.py [pgrm|parts|cmm|distill|loss|metrics|tsrn|tatt|tbsrn|step|all]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()
from dpmn_amd.utils import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)
torch.set_num_threads(8)


def manifest(sd):
    return np.array(["%s|%s|%s" % (k, ",".join(map(str, v.shape)), str(v.dtype).replace("torch.", ""))
                     for k, v in sd.items()])


def checksum(sd):
    skip = ("relative_position_index", "attn_mask", "num_batches_tracked")
    return float(sum(v.double().sum().item() for k, v in sd.items()
                     if torch.is_floating_point(v) and not any(s in k for s in skip) and not k.endswith(".pe")))


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()})
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def pgrm_args(n=6, dim=96, windows=(2, 4, 8), heads=6):
    return dict(patch_size=[2] * n, embed_dim=[dim] * n, depths=[1] * n, num_heads=[[heads]] * n,
                window_size=[list(windows)] * n, mlp_ratio=[4.] * n, drop_rate=[0.] * n,
                attn_drop_rate=[0.] * n, drop_path_rate=[0.] * n)


# ------------------------------------------------------------------------------------ PGRM
def gen_pgrm():
    from model import pgrm
    B = 2
    for tag, it, mode in (("mode0_iter0", 0, False), ("mode1_iter2", 2, True)):
        m = pgrm.PGRM(iter=it, mode=mode, hidden_size=3, **pgrm_args()).eval()
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=11 + it)
        m.load_state_dict(sd)
        cq = 3 if mode else 2
        if mode:
            x_q = (synth.uniform("x_q", (B, 1, 32, 128), 0, 1, 5) > 0.5).float().repeat(1, 3, 1, 1)
        else:
            x_q = torch.floor(synth.uniform("x_q", (B, cq, 32, 128), 0, 256, 5))
        x_kv = synth.uniform("x_kv", (B, 3, 32, 128), 0, 1, 5)
        res = [synth.uniform("res%d" % i, (B, 3, 32, 128), 0, 1, 5) for i in range(it)]
        out = m(x_q, x_kv, res)
        save("pgrm_" + tag, out=out, manifest=manifest(sd), checksum=checksum(sd),
             meta=np.array([B, it, int(mode), 11 + it, 5]))


def gen_parts():
    """Sub-module pins: WindowAttention (cat tensor fed to SKConv, shift 0 and shifted), SKConv,
    Mlp at config-1 dims, and one BasicLayer at the stress dims."""
    from model import pgrm
    import torch.nn as nn
    B, H, W, C = 1, 16, 64, 96
    for tag, shift in (("shift0", [0, 0, 0]), ("shifted", [1, 2, 4])):
        wa = pgrm.WindowAttention(C, window_size=[2, 4, 8], shift_size=list(shift), num_heads=6,
                                  act_layer=nn.GELU, input_resolution=(H, W)).eval()
        sd = wa.state_dict()
        synth.synth_fill_(sd, seed=21)
        wa.load_state_dict(sd)
        grabbed = {}
        wa.sknet.register_forward_hook(lambda mod, inp, out: grabbed.__setitem__("cat", inp[0].clone()))
        xq = synth.uniform("wa_xq", (B, H, W, C), -1, 1, 6)
        xkv = synth.uniform("wa_xkv", (B, H, W, C), -1, 1, 6)
        out = wa(xq, xkv)
        save("wattn_" + tag, cat=grabbed["cat"].reshape(B, H * W, C), out=out.contiguous(),
             manifest=manifest(sd), checksum=checksum(sd))
    mlp = pgrm.Mlp(C, 4 * C).eval()
    sd = mlp.state_dict()
    synth.synth_fill_(sd, seed=22)
    mlp.load_state_dict(sd)
    x = synth.uniform("mlp_x", (2, H * W, C), -1, 1, 6)
    save("mlp", out=mlp(x), manifest=manifest(sd), checksum=checksum(sd))
    # stress dims: dim 192, windows 4/8/16, 32x128 tokens, B=1 (quirk Q7: only pinned at layer level)
    Hs, Ws, Cs = 32, 128, 192
    bl = pgrm.BasicLayer(Cs, (Hs, Ws), depth=2, num_heads=6, window_size=[4, 8, 16], mlp_ratio=4.,
                         drop=0., attn_drop=0., drop_path=0.).eval()
    sd = bl.state_dict()
    synth.synth_fill_(sd, seed=23)
    bl.load_state_dict(sd)
    xq = synth.uniform("bl_xq", (1, Hs * Ws, Cs), -1, 1, 6)
    xkv = synth.uniform("bl_xkv", (1, Hs * Ws, Cs), -1, 1, 6)
    _, o = bl(xq, xkv)
    save("basiclayer_stress", out=o[:, ::7].contiguous(), manifest=manifest(sd), checksum=checksum(sd))


# ------------------------------------------------------------------------------------ CMM etc.
def gen_cmm():
    from model import cmm
    B = 2
    x1 = synth.uniform("cmm_x1", (B, 3, 32, 128), 0, 1, 7)
    x2 = synth.uniform("cmm_x2", (B, 3, 32, 128), 0, 1, 7)
    for cnum in (8, 64):
        m = cmm.ComplementationModulationModule(cnum=cnum)
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=31)
        sd = {k: v.clone() for k, v in sd.items()}  # state_dict() aliases live buffers (BN stats mutate)
        m.load_state_dict(sd)
        outs = {}
        for training in (False, True):
            m.train(training)
            outs["out_train" if training else "out_eval"] = m(x1, x2)
        save("cmm_cnum%d" % cnum, manifest=manifest(sd), checksum=checksum(sd), **outs)


def gen_distill():
    from model import distill_module
    B = 2
    xd = synth.uniform("dist_deep", (B, 3, 32, 128), 0, 1, 8)
    xs = synth.uniform("dist_shallow", (B, 3, 32, 128), 0, 1, 8)
    m = distill_module.DistillModule()
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=32)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    m.train()
    loss, feat = m(xd, xs)
    m.load_state_dict(sd)
    m.eval()
    loss_e, feat_e = m(xd, xs)
    save("distill", loss_train=loss, feat_train=feat, loss_eval=loss_e, feat_eval=feat_e,
         manifest=manifest(sd), checksum=checksum(sd))


def gen_loss():
    from loss import image_loss
    sys.modules.setdefault("IPython", sys.modules["IPython"])
    from utils import ssim_psnr
    B = 4
    a = synth.uniform("loss_a", (B, 3, 32, 128), 0, 1, 9)
    b = synth.uniform("loss_b", (B, 4, 32, 128), 0, 1, 9)
    b3 = (0.7 * a + 0.3 * b[:, :3])
    crit = image_loss.ImageLoss(gradient=True, loss_weight=[1, 1])
    crit_ng = image_loss.ImageLoss(gradient=False, loss_weight=[1, 1])
    save("loss_metrics", loss_grad=crit(a, b3), loss_nograd=crit_ng(a, b3),
         psnr=ssim_psnr.calculate_psnr(a, torch.cat([b3, b[:, 3:]], 1)),
         ssim=ssim_psnr.SSIM()(a, torch.cat([b3, b[:, 3:]], 1)),
         gradmap=image_loss.GradientPriorLoss.gradient_map(a)[:1])


def gen_rotate():
    """torch_rotate_img (utils/util.py:37-58) through the reference function itself (rotate_train = 5 degrees)."""
    from utils import util
    N = 4
    img = synth.uniform("rot_img", (N, 4, 16, 64), 0, 1, 11)
    deg = synth.uniform("rot_deg", (N,), -5.0, 5.0, 11)
    arc = deg / 180.0 * float(np.pi)
    offs = synth.uniform("rot_off", (N,), 0, 1, 11)
    save("rotate", out_lr=util.torch_rotate_img(img, arc, offs),
         out_hr=util.torch_rotate_img(synth.uniform("rot_img_hr", (N, 4, 32, 128), 0, 1, 11), arc, offs))


def gen_tbsrn(x):
    """TBSRN in eval mode (config 3's PSN).  FeatureEnhancer hard-codes .cuda() (tbsrn.py:83): identity on this CPU box."""
    from model import tbsrn
    orig = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        m = tbsrn.TBSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=43)
        sd = {k: v.clone() for k, v in sd.items()}
        m.load_state_dict(sd)
        feats = {}
        m.block2.feature_enhancer.register_forward_hook(lambda mod, i, o: feats.setdefault("fe", o))
        out = m(x)
        save("tbsrn", out=out, fe_block2=feats["fe"][:, ::8].contiguous(), manifest=manifest(sd), checksum=checksum(sd))
    finally:
        torch.Tensor.cuda = orig


def gen_stn_layout():
    """state_dict layout + constructor values of the --STN front end (the README's train/test commands pass --STN)."""
    from model import tatt
    m = tatt.TSRN_TL_TRANS(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)
    sd = m.state_dict()
    save("stn_layout", manifest=manifest(sd), inverse_kernel=sd["tps.inverse_kernel"], target_control_points=sd["tps.target_control_points"],
         target_coordinate_repr=sd["tps.target_coordinate_repr"][::37].contiguous(), fc2_bias=sd["stn_head.stn_fc2.bias"],
         fc2_weight_absmax=sd["stn_head.stn_fc2.weight"].abs().max())


def gen_stn_fwd():
    """Row a15 forward: the imported STNHead (train and eval mode) and TPSSpatialTransformer on synthetic weights."""
    from model import stn_head, tps_spatial_transformer as tps
    B = 6
    x = synth.uniform("stn_x", (B, 4, 16, 64), 0, 1, 51)
    out = {}
    for mode in ("train", "eval"):
        m = stn_head.STNHead(in_planes=4, num_ctrlpoints=20, activation='none')
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=52)
        sd = {k: v.clone() for k, v in sd.items()}
        m.load_state_dict(sd)
        m.train(mode == "train")
        feat, ctrl = m(x)
        out[mode + "_feat"], out[mode + "_ctrl"] = feat, ctrl
        if mode == "train":
            sd2 = m.state_dict()
            for k in sd2:
                if "running" in k or "num_batches" in k:
                    out["after." + k] = sd2[k].clone()
    t = tps.TPSSpatialTransformer(output_image_size=(16, 64), num_control_points=20, margins=(0.05, 0.05))
    # control points around the identity layout, pushed far enough that some source coordinates leave [0, 1] (clamp path)
    ctrl = t.target_control_points[None] + synth.uniform("stn_ctrl", (B, 20, 2), -0.12, 0.12, 53)
    warped, src = t(x, ctrl)
    save("stn_fwd", manifest=manifest(sd), checksum=checksum(sd), tps_out=warped, tps_src=src[:, ::7].contiguous(),
         tps_src_minmax=np.array([float(src.min()), float(src.max())]), **out)


def gen_psn():
    """PSN backbones in eval mode (frozen in DPMN, super_resolution.py:56-59): TSRN and TATT."""
    from model import tsrn, tatt
    b = synth.synth_batch(2, seed=2)
    x, lv = b["images_lr"], b["label_vecs"]
    m = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=41)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    save("tsrn", out=m(x), manifest=manifest(sd), checksum=checksum(sd))
    m = tatt.TSRN_TL_TRANS(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=42)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    out, prw = m(x, lv)
    gen_tbsrn(x)
    save("tatt", out=out, pr_weights=prw[:, ::16].contiguous(), tp_map=m.block["1"][:1, :8].contiguous(),
         manifest=manifest(sd), checksum=checksum(sd))


def gen_tpgsr():
    """--arch tpgsr: TSRN_TL (tsrn.py:153-247) in eval mode on the same inputs as the TATT fixture + the InfoGen map."""
    from model import tsrn
    b = synth.synth_batch(2, seed=2)
    x, lv = b["images_lr"], b["label_vecs"]
    m = tsrn.TSRN_TL(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=44)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    save("tpgsr", out=m(x, lv), info=m.infoGen(lv)[:, :, 0, ::7].contiguous(), manifest=manifest(sd), checksum=checksum(sd))


def gen_stack():
    """config 0 (BASELINE.json): TSRN PSN + 1+1 PGRM + CMM, B=4, eval forward of
    interfaces/super_resolution.py:370-449 re-stated around the IMPORTED reference modules.  toMask needs
    torchvision (absent) -> the PIL-pinned restatement oracle.cmm.to_mask is used for the mask prior."""
    from model import tsrn, pgrm, cmm
    from oracle import cmm as ocmm
    B, b1, b2, alpha = 4, 1, 1, 0.5
    batch = synth.synth_batch(B, seed=2)
    psn = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
    mods = [pgrm.PGRM(iter=0, mode=False, hidden_size=3, **pgrm_args(2)).eval(),
            pgrm.PGRM(iter=1, mode=True, hidden_size=3, **pgrm_args(2)).eval()]
    fuse = cmm.ComplementationModulationModule().eval()
    for i, m in enumerate([psn] + mods + [fuse]):
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=100 + i)
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
    prior = torch.floor(synth.uniform("text_prior_0", (B, 2, 32, 128), 0.0, 256.0, 2))
    lr_psn = psn(batch["images_lr"])
    cascade, l1 = lr_psn, []
    for k in range(b1):
        sr = mods[k](prior, cascade[:, :3, :], l1[:k])
        l1.append(sr)
        cascade = sr
    cascade, l2 = lr_psn, []
    for k in range(b1, b1 + b2):
        sr = mods[k](ocmm.to_mask(cascade[:, :3]), cascade[:, :3, :], l2[:(k - b2)])
        l2.append(sr)
        cascade = sr
    out = alpha * fuse(l1[-1], l2[-1]) + (1 - alpha) * lr_psn[:, :3, :, :]
    sys.modules.setdefault("IPython", sys.modules["IPython"])
    from utils import ssim_psnr
    save("stack_cfg0", out=out, psn=lr_psn, branch1=l1[-1], branch2=l2[-1],
         psnr=ssim_psnr.calculate_psnr(out, batch["images_hr"]), ssim=ssim_psnr.SSIM()(out, batch["images_hr"]))


# ------------------------------------------------------------------------------------ gradients of the reference itself
def grad_arrays(prefix, named_grads):
    """npz entries for a set of gradients: helpers.grad_digest (full tensor up to 4096 elements, otherwise norm / sum /
    64 strided samples / one seeded projection) -- the reference's own autograd results, SURVEY.md section 8c."""
    from tests.helpers import grad_digest
    out = {}
    for name, g in named_grads:
        for k, v in grad_digest(name, g).items():
            out["%s%s::%s" % (prefix, name, k)] = v
    return out


def gen_grads():
    """d(out . r)/d(inputs, params) for a fixed seeded cotangent r through the IMPORTED reference modules (train mode,
    drop rates 0): PGRM (both fixture variants), CMM (cnum 8 and 64, batch-statistics BatchNorm), DistillModule."""
    from model import pgrm, cmm, distill_module
    with torch.enable_grad():
        B = 2
        for tag, it, mode in (("mode0_iter0", 0, False), ("mode1_iter2", 2, True)):
            m = pgrm.PGRM(iter=it, mode=mode, hidden_size=3, **pgrm_args()).train()
            sd = m.state_dict()
            synth.synth_fill_(sd, seed=11 + it)
            m.load_state_dict(sd)
            if mode:
                x_q = (synth.uniform("x_q", (B, 1, 32, 128), 0, 1, 5) > 0.5).float().repeat(1, 3, 1, 1)
            else:
                x_q = torch.floor(synth.uniform("x_q", (B, 2, 32, 128), 0, 256, 5))
            x_kv = synth.uniform("x_kv", (B, 3, 32, 128), 0, 1, 5).requires_grad_(True)
            res = [synth.uniform("res%d" % i, (B, 3, 32, 128), 0, 1, 5).requires_grad_(True) for i in range(it)]
            cot = synth.uniform("cot", (B, 3, 32, 128), -1, 1, 5)
            out = m(x_q, x_kv, res)
            (out * cot).sum().backward()
            named = [("x_kv", x_kv.grad)] + [("res%d" % i, r.grad) for i, r in enumerate(res) if r.grad is not None]
            named += [(n, p.grad) for n, p in m.named_parameters() if p.grad is not None]
            save("grads_pgrm_" + tag, out=out.detach(), **grad_arrays("", named))
        x1 = synth.uniform("cmm_x1", (B, 3, 32, 128), 0, 1, 7).requires_grad_(True)
        x2 = synth.uniform("cmm_x2", (B, 3, 32, 128), 0, 1, 7).requires_grad_(True)
        cot = synth.uniform("cmm_cot", (B, 3, 32, 128), -1, 1, 7)
        for cnum in (8, 64):
            m = cmm.ComplementationModulationModule(cnum=cnum).train()
            sd = m.state_dict()
            synth.synth_fill_(sd, seed=31)
            m.load_state_dict({k: v.clone() for k, v in sd.items()})
            x1.grad = x2.grad = None
            out = m(x1, x2)
            (out * cot).sum().backward()
            named = [("x1", x1.grad), ("x2", x2.grad)] + [(n, p.grad) for n, p in m.named_parameters()]
            save("grads_cmm_cnum%d" % cnum, out=out.detach(), **grad_arrays("", named))
        xd = synth.uniform("dist_deep", (B, 3, 32, 128), 0, 1, 8).requires_grad_(True)
        xs = synth.uniform("dist_shallow", (B, 3, 32, 128), 0, 1, 8).requires_grad_(True)
        cot = synth.uniform("dist_cot", (B, 3, 32, 128), -0.01, 0.01, 8)
        m = distill_module.DistillModule().train()
        sd = m.state_dict()
        synth.synth_fill_(sd, seed=32)
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        loss, feat = m(xd, xs)
        (loss.sum() * 100 + (feat * cot).sum()).backward()
        named = [("xd", xd.grad), ("xs", xs.grad)] + [(n, p.grad) for n, p in m.named_parameters()]
        save("grads_distill", loss=loss.detach(), **grad_arrays("", named))


def gen_step():
    """One optimisation step of interfaces/super_resolution.py:140-278 re-stated around the IMPORTED reference modules
    (TSRN PSN frozen in eval, 2+2 PGRM, 2 DistillModules, CMM, B=2, drop rates 0; text priors are inputs, toMask is the
    PIL-pinned restatement): the loss, every cascade image, and per model the gradient norm that clip_grad_norm_(0.25)
    sees plus digests of the pre-clip gradients.  Same seeds as tests/test_gpu_train.py::test_full_train_step_*."""
    from model import tsrn, pgrm, cmm, distill_module
    from loss import image_loss
    from oracle import cmm as ocmm
    B, b1, b2 = 2, 2, 2
    with torch.enable_grad():
        psn = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
        mods = [pgrm.PGRM(iter=k, mode=False, hidden_size=3, **pgrm_args(4)).train() for k in range(b1)]
        mods += [pgrm.PGRM(iter=k, mode=True, hidden_size=3, **pgrm_args(4)).train() for k in range(b1, b1 + b2)]
        mods.append(cmm.ComplementationModulationModule().train())
        distill = [distill_module.DistillModule().train() for _ in range(b1 + b2 - 2)]
        for i, m in enumerate([psn] + mods + distill):
            sd = m.state_dict()
            synth.synth_fill_(sd, seed=300 + i)
            m.load_state_dict({k: v.clone() for k, v in sd.items()})
        crit = image_loss.ImageLoss(gradient=True, loss_weight=[1, 1])
        batch = synth.synth_batch(B, seed=4)
        priors = [torch.floor(synth.uniform("tp%d" % k, (B, 2, 32, 128), 0, 256, 4)) for k in range(b1)]
        hr = batch["images_hr"]
        with torch.no_grad():
            lr_psn = psn(batch["images_lr"])
        loss = 0
        casc, l1 = lr_psn, []
        for k in range(b1):
            sr = mods[k](priors[k], casc[:, :3, :], l1[:k]); l1.append(sr); casc = sr
            loss = loss + crit(sr, hr[:, :3, :]).mean() * 100
        casc, l2 = lr_psn, []
        for k in range(b1, b1 + b2):
            sr = mods[k](ocmm.to_mask(casc.detach()[:, :3]), casc[:, :3, :], l2[:(k - b2)]); l2.append(sr); casc = sr
            loss = loss + crit(sr, hr[:, :3, :]).mean() * 100
        feat = l1[-1]
        for k in range(b1 - 1, 0, -1):
            ld, feat = distill[k - 1](feat, l1[k - 1]); loss = loss + ld.sum() * 100
        feat = l2[-1]
        for k in range(b2 - 1, 0, -1):
            ld, feat = distill[k + b1 - 2](feat, l2[k - 1]); loss = loss + ld.sum() * 100
        out = mods[-1](l1[-1], l2[-1])
        loss = (loss + crit(out, hr[:, :3, :]).mean() * 100) / (b1 + b2 + 1)
        loss.backward()
        arrs = dict(loss=loss.detach(), psn=lr_psn, cmm_out=out.detach())
        for k in range(b1):
            arrs["branch1_%d" % k] = l1[k].detach()
        for k in range(b2):
            arrs["branch2_%d" % k] = l2[k].detach()
        norms = []
        for i, m in enumerate(mods + distill):
            named = [(n, p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in m.named_parameters()]
            norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for _, g in named))))
            arrs.update(grad_arrays("m%d/" % i, named))
        arrs["grad_norms"] = np.array(norms)
        save("step_tsrn_2p2", **arrs)

# ------------------------------------------------------------------------------------ float64 adjudication of the gradient fixtures
def f64_arrays(prefix, named64, named32):
    """Digests of the float64 gradients plus, per tensor, `ref32_err`: how far the reference's OWN fp32 gradient is from that
    float64 result under the metric the tests use (helpers.grad_error_vs_fixture) -- the yardstick for the HIP path's error."""
    from tests.helpers import grad_digest, grad_error_vs_fixture
    out = {}
    for name, g in named64:
        for k, v in grad_digest(name, g, f64=True).items():
            out["%s%s::%s" % (prefix, name, k)] = v

    class _Npz(dict):
        files = property(lambda self: list(self.keys()))
    z = _Npz(out)
    for name, g32 in named32:
        err, _ = grad_error_vs_fixture(z, prefix + name, g32)
        out["%s%s::ref32_err" % (prefix, name)] = np.array(err)
    return out


def gen_f64():
    """The reference modules in float64 (`.double()`, the SAME fp32 synthetic weights and inputs, exactly representable) as the
    arbiter of the two loose gradient fixtures: grads_cmm_cnum64 (B = 2: 8-sample BatchNorm statistics at the 1 x 4 bottleneck
    make the fp32 gradients ill-conditioned) and step_tsrn_2p2.  A fixture holds float64 digests and, per tensor, the error of
    the reference's own fp32 gradient against them; the GPU tests require err(HIP, f64) <= 1.5 x err(reference fp32, f64)."""
    from model import tsrn, pgrm, cmm, distill_module
    from loss import image_loss
    from oracle import cmm as ocmm
    with torch.enable_grad():
        B = 2
        x1 = synth.uniform("cmm_x1", (B, 3, 32, 128), 0, 1, 7)
        x2 = synth.uniform("cmm_x2", (B, 3, 32, 128), 0, 1, 7)
        cot = synth.uniform("cmm_cot", (B, 3, 32, 128), -1, 1, 7)
        named = {}
        for dt in (torch.float32, torch.float64):
            m = cmm.ComplementationModulationModule(cnum=64).train()
            sd = m.state_dict()
            synth.synth_fill_(sd, seed=31)
            m.load_state_dict({k: v.clone() for k, v in sd.items()})
            m = m.to(dt)
            a, b = x1.detach().clone().to(dt).requires_grad_(True), x2.detach().clone().to(dt).requires_grad_(True)
            out = m(a, b)
            (out * cot.to(dt)).sum().backward()
            named[dt] = [("x1", a.grad), ("x2", b.grad)] + [(n, p.grad) for n, p in m.named_parameters()]
            if dt == torch.float64:
                out64 = out.detach()
        # kink-aware adjudication (tests/helpers.py "Kink-aware float64 adjudication"): the pre-activations within fp32 round-off of a
        # LeakyReLU / ReLU kink, the sign the REFERENCE's fp32 run has there, and the reference's fp32 gradient error against the
        # float64 gradients that differentiate the same branch at those elements (`ref32_err_adj`)
        from tests import helpers as th
        sd32 = {k: v.clone() for k, v in sd.items()}
        sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd32.items()}
        sites64 = th.cmm_sites(sd64, x1.double(), x2.double())
        kinks = th.ambiguous_kinks(sites64)
        # the reference's fp32 pre-activations: inputs of its activation modules (decoder inputs are channel concatenations of the
        # oracle's parts, in the oracle's order)
        m32 = cmm.ComplementationModulationModule(cnum=64).train()
        m32.load_state_dict({k: v.clone() for k, v in sd32.items()})
        ins = {}
        for n_, mod in m32.named_modules():
            if isinstance(mod, (torch.nn.LeakyReLU, torch.nn.ReLU)):
                mod.register_forward_pre_hook(lambda _m, a, n_=n_: ins.__setitem__(n_, a[0].detach()))
        with torch.no_grad():
            m32(x1, x2)
        parts32, off = {}, {}
        for site, x in sites64:
            cons = site.split(">")[1]
            o = off.get(cons, 0)
            parts32[site] = ins[cons][:, o:o + x.shape[1]]
            off[cons] = o + x.shape[1]
            assert parts32[site].shape == x.shape, (site, parts32[site].shape, x.shape)
        forced = [(site, i, float(parts32[site].reshape(-1)[i]) > 0) for site, i, _ in kinks]
        g64_adj = th.cmm_grads_f64(sd32, x1, x2, cot, forced)
        g64_plain = th.cmm_grads_f64(sd32, x1, x2, cot)
        extra = {"kink_site": np.array([k[0] for k in kinks]), "kink_index": np.array([k[1] for k in kinks], dtype=np.int64),
                 "kink_y64": np.array([k[2] for k in kinks]), "kink_ref32_positive": np.array([f[2] for f in forced])}
        for name, g32 in named[torch.float32]:
            extra[name + "::ref32_err_adj"] = np.array(th.rel_l2(g32, g64_adj[name]))
            # the oracle's float64 gradients ARE the reference's (same float64 math): recorded, and asserted by the tests
            extra[name + "::oracle64_vs_ref64"] = np.array(th.rel_l2(g64_plain[name], dict(named[torch.float64])[name]))
        print("cnum64 f64: %d ambiguous pre-activations (|y| < %g); reference fp32 takes the other branch at %d of them; oracle f64 vs reference f64 max %.1e" % (
            len(kinks), th.KINK_TOL, sum(1 for (s_, i, y), f in zip(kinks, forced) if (y > 0) != f[2]), max(float(v) for k, v in extra.items() if k.endswith("oracle64_vs_ref64"))))
        save("grads_cmm_cnum64_f64", out=out64.numpy(), **f64_arrays("", named[torch.float64], named[torch.float32]), **extra)

        b1 = b2 = 2
        batch = synth.synth_batch(B, seed=4)
        priors = [torch.floor(synth.uniform("tp%d" % k, (B, 2, 32, 128), 0, 256, 4)) for k in range(b1)]
        res, masks = {}, None
        for dt in (torch.float32, torch.float64):
            psn = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32).eval()
            mods = [pgrm.PGRM(iter=k, mode=False, hidden_size=3, **pgrm_args(4)).train() for k in range(b1)]
            mods += [pgrm.PGRM(iter=k, mode=True, hidden_size=3, **pgrm_args(4)).train() for k in range(b1, b1 + b2)]
            mods.append(cmm.ComplementationModulationModule().train())
            distill = [distill_module.DistillModule().train() for _ in range(b1 + b2 - 2)]
            for i, m in enumerate([psn] + mods + distill):
                sd = m.state_dict()
                synth.synth_fill_(sd, seed=300 + i)
                m.load_state_dict({k: v.clone() for k, v in sd.items()})
                m.to(dt)
            crit = image_loss.ImageLoss(gradient=True, loss_weight=[1, 1])
            hr = batch["images_hr"].to(dt)
            with torch.no_grad():
                lr_psn = psn(batch["images_lr"].to(dt))
            loss = 0
            casc, l1 = lr_psn, []
            for k in range(b1):
                sr = mods[k](priors[k].to(dt), casc[:, :3, :], l1[:k]); l1.append(sr); casc = sr
                loss = loss + crit(sr, hr[:, :3, :]).mean() * 100
            casc, l2 = lr_psn, []
            new_masks = []
            for k in range(b1, b1 + b2):
                # the mask prior is a threshold (discontinuous): the float64 run takes the fp32 run's masks, so that both
                # differentiate the same function
                mk = ocmm.to_mask(casc.detach()[:, :3].float()) if masks is None else masks[k - b1]
                new_masks.append(mk)
                sr = mods[k](mk.to(dt), casc[:, :3, :], l2[:(k - b2)]); l2.append(sr); casc = sr
                loss = loss + crit(sr, hr[:, :3, :]).mean() * 100
            masks = masks or new_masks
            feat = l1[-1]
            for k in range(b1 - 1, 0, -1):
                ld, feat = distill[k - 1](feat, l1[k - 1]); loss = loss + ld.sum() * 100
            feat = l2[-1]
            for k in range(b2 - 1, 0, -1):
                ld, feat = distill[k + b1 - 2](feat, l2[k - 1]); loss = loss + ld.sum() * 100
            out = mods[-1](l1[-1], l2[-1])
            loss = (loss + crit(out, hr[:, :3, :]).mean() * 100) / (b1 + b2 + 1)
            loss.backward()
            res[dt] = (float(loss.detach()), [[(n, p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in m.named_parameters()]
                                              for m in mods + distill])
        arrs = dict(loss=np.array(res[torch.float64][0]), loss_ref32_err=np.array(abs(res[torch.float32][0] - res[torch.float64][0]) / abs(res[torch.float64][0])))
        norms, norm_err = [], []
        for i, (n64, n32) in enumerate(zip(res[torch.float64][1], res[torch.float32][1])):
            arrs.update(f64_arrays("m%d/" % i, n64, n32))
            a = float(torch.sqrt(sum((g.double() ** 2).sum() for _, g in n64)))
            b_ = float(torch.sqrt(sum((g.double() ** 2).sum() for _, g in n32)))
            norms.append(a); norm_err.append(abs(a - b_) / a)
        arrs["grad_norms"] = np.array(norms)
        arrs["grad_norms_ref32_err"] = np.array(norm_err)
        save("step_tsrn_2p2_f64", **arrs)


def gen_visionlan():
    """VisionLAN (the branch-1 text-prior recogniser) in eval mode through the imported reference: per-step logits captured at
    Prediction, the flattened (output, out_length) pair MLM_VRM returns, a digest of the backbone feature map and the strings
    cha_encdec.decode (restated: the dict file is read there, utils.py:13-16) produces.  B = 3 images of 64x256."""
    from model.VisionLAN.VisionLAN import VisionLAN
    B = 3
    m = VisionLAN(strides=[(1, 1), (2, 2), (2, 2), (2, 2), (1, 1), (1, 1)], input_shape=[3, 64, 256]).eval()
    pos_tab = m.MLM_VRM.SequenceModeling.position_enc.pos_table[0, ::5, ::7].clone()      # the constructor's sinusoid table
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=61)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    x = synth.uniform("vl_img", (B, 3, 64, 256), 0, 1, 62)
    grab = {}
    m.MLM_VRM.Prediction.register_forward_hook(lambda mod, i, o: grab.__setitem__("logits", o.clone()))
    m.backbone.register_forward_hook(lambda mod, i, o: grab.__setitem__("feat", o[-1].clone()))
    m.MLM_VRM.SequenceModeling.register_forward_hook(lambda mod, i, o: grab.__setitem__("enc", o[0].clone()))
    output, out_length = m(x, None, '', False)
    dic = [l.replace("\n", "") for l in open(os.path.join(ref_shims.REF_ROOT, "dic_36.txt")).readlines()]
    prob = torch.softmax(output, 1)
    texts, start = [], 0
    for i in range(B):
        n = int(out_length[i])
        idx = prob[start:start + n].topk(1)[1][:, 0].tolist()
        texts.append("".join(dic[c - 1] if 0 < c <= len(dic) else "" for c in idx))
        start += n
    # the decode loop (VisionLAN.py:107-135) on logits with EOS in the middle / at step 0 / never: Prediction replaced by a stub
    # returning crafted logits, everything after it is the reference's own code
    grab = dict(grab)                                    # (the hooks fire again below)
    m.backbone._forward_hooks.clear(); m.MLM_VRM.SequenceModeling._forward_hooks.clear(); m.MLM_VRM.Prediction._forward_hooks.clear()
    crafted = synth.uniform("vl_crafted", (4, 26, 37), -1, 1, 64)
    crafted[:, :, 0] -= 3.0
    crafted[0, 6, 0] = 5.0; crafted[0, 9, 0] = 5.0      # first EOS at step 6 -> length 7
    crafted[1, 0, 0] = 5.0                               # EOS at step 0 -> length 1, empty string
    crafted[3, 24, 0] = 5.0                              # EOS at the last step -> length 25
    m.MLM_VRM.Prediction.forward = lambda *a, **k: crafted.clone()
    d_out, d_len = m(synth.uniform("vl_img4", (4, 3, 64, 256), 0, 1, 62), None, '', False)
    d_prob = torch.softmax(d_out, 1)
    d_texts, start = [], 0
    for i in range(4):
        n = int(d_len[i])
        idx = d_prob[start:start + n].topk(1)[1][:, 0].tolist()
        d_texts.append("".join(dic[c - 1] if 0 < c <= len(dic) else "" for c in idx))
        start += n
    save("visionlan", pos_table_sample=pos_tab, decode_output=d_out, decode_length=d_len, decode_texts=np.array(d_texts), logits=grab["logits"], output=output, out_length=out_length, feat_sample=grab["feat"][:, ::16, :, ::4].contiguous(),
         enc_sample=grab["enc"][:, ::8, ::8].contiguous(), texts=np.array(texts), dict36=np.array("".join(dic)),
         manifest=manifest(sd), checksum=checksum(sd))


GENS = {"f64": gen_f64, "tpgsr": gen_tpgsr, "visionlan": gen_visionlan, "grads": gen_grads, "step": gen_step, "stack": gen_stack, "psn": gen_psn, "pgrm": gen_pgrm, "parts": gen_parts, "cmm": gen_cmm, "distill": gen_distill, "loss": gen_loss, "rotate": gen_rotate, "stn": gen_stn_layout, "stn_fwd": gen_stn_fwd}



def gen_crnn():
    """The frozen CRNN that produces TATT's label_vecs on real data (model/crnn/crnn.py through the import; CRNN_init's
    CRNN(32, 1, 37, 256), base.py:411-417) + the reference lines around it: parse_crnn_data (base.py:419-425) and the softmax /
    permute of super_resolution.py:165-169, on name-seeded synthetic weights and LR images."""
    import torch.nn.functional as F
    from model.crnn import crnn
    m = crnn.CRNN(32, 1, 37, 256).eval()
    sd = m.state_dict()
    synth.synth_fill_(sd, seed=71)
    sd = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd)
    imgs = synth.uniform("crnn_lr", (3, 3, 16, 64), 0, 1, 72)
    x = F.interpolate(imgs, (32, 100), mode='bicubic')                                   # parse_crnn_data
    gray = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    logits = m(gray)
    lv = torch.nn.functional.softmax(logits, -1).permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2)
    save("crnn", logits=logits, label_vecs=lv.contiguous(), manifest=manifest(sd), checksum=checksum(sd))


def gen_crnn_ctc():
    """Greedy CTC decoding of the CRNN recogniser: the reference's own strLabelConverter.decode(raw=False) (utils/utils_crnn.py:54-90)
    with the converter of base.py:62 (digits + lowercase) on hand-made (B, 26) class sequences -- all blank, repeats with and without
    a blank between them, a full 26-character run, every class once, leading / trailing blanks -- exactly as eval() calls it
    (super_resolution.py:474-479: the (B*26) flattened arg-max classes with 26 per image)."""
    import string
    from utils import utils_crnn
    conv = utils_crnn.strLabelConverter(string.digits + string.ascii_lowercase)
    T = 26
    rows = [[0] * T,                                                          # all blank
            [5] * T,                                                          # one class repeated: one character
            [5, 5, 0, 5, 5] + [0] * (T - 5),                                  # a blank between repeats keeps both
            [11, 11, 12, 12, 12, 13] + [0] * (T - 6),                         # repeats collapse
            [(i % 36) + 1 for i in range(T)],                                 # 26 distinct characters, no blank
            [1 + ((2 * i) % 36) for i in range(T)],
            [0, 0, 0, 20, 21, 22] + [0] * (T - 6),                            # leading and trailing blanks
            [36, 0, 36, 36, 0, 0, 1, 1, 0, 1] + [0] * (T - 10),
            [0] + list(range(1, 26)),                                         # every class once (with the next row)
            list(range(26, 37)) + [0] * (T - 11),
            [7, 8] * (T // 2),                                                # alternation, no repeat to collapse
            [3, 0] * (T // 2)]
    rng = np.random.RandomState(11)
    for _ in range(8):                                                        # random sequences, blank-heavy
        r = rng.randint(0, 37, T)
        r[rng.rand(T) < 0.4] = 0
        rows.append(r.tolist())
    cls = torch.tensor(rows, dtype=torch.int64)
    preds = cls.reshape(-1)
    sizes = torch.IntTensor([T] * cls.shape[0])
    texts = conv.decode(preds, sizes, raw=False)
    save("crnn_ctc", classes=cls.to(torch.int32), texts=np.array(texts), alphabet=np.array(conv.alphabet[:-1]))


def _aster_reference():
    """The reference's RecognizerBuilder on the CPU: its decoder calls .cuda() on fresh tensors, so torch.Tensor.cuda is the identity
    while the returned `restore` has not been called."""
    import types
    for name in ("torchsnooper", "editdistance"):      # imported by the recogniser / utils.metrics, never called on this path
        sys.modules.setdefault(name, types.ModuleType(name))
    orig = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    from model.recognizer.recognizer_builder import RecognizerBuilder
    ref = RecognizerBuilder(arch='ResNet_ASTER', rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True).eval()

    def restore():
        torch.Tensor.cuda = orig
    return ref, restore


def _ref_aster_info(voc_type):
    """What interfaces/base.py AsterInfo holds (lines 480-492), from the reference's get_vocabulary (importing interfaces.base itself
    pulls in the LMDB data path)."""
    import types
    from utils.labelmaps import get_vocabulary
    voc = get_vocabulary(voc_type, EOS='EOS', PADDING='PADDING', UNKNOWN='UNKNOWN')
    return types.SimpleNamespace(voc_type=voc_type, EOS='EOS', PADDING='PADDING', UNKNOWN='UNKNOWN', max_len=100, voc=voc,
                                 char2id=dict(zip(voc, range(len(voc)))), id2char=dict(zip(range(len(voc)), voc)), rec_num_classes=len(voc))


ASTER_IDS = [3, 5, 18, 4, 7, 9, 0, 19]      # members of utils/aster_synth.py's image pool (chosen on the reference's own run, asserted below)
ASTER_STEPS = [0, 5, 20]


def _sample(t, n=256):
    f = t.reshape(-1)
    return f[::max(1, f.numel() // n)][:n].clone()


def gen_aster():
    """The ASTER recogniser (model/recognizer/) in eval mode on name-seeded weights (utils/aster_synth.py aster_fill_, seed 81) and
    bar images: every stage of RecognizerBuilder.forward, the beam search re-run step by step on the reference's own DecoderUnit (the
    candidate scores give the decision margins; its stored tensors backtrack to the reference's pred_rec), three teacher-forced
    steps, the strings of get_str_list."""
    import torch.nn.functional as F
    from dpmn_amd.utils import aster_synth
    ref, restore = _aster_reference()
    from utils.metrics import get_str_list
    AsterInfo = _ref_aster_info
    try:
        sd = ref.state_dict()
        assert len(sd) == 384
        aster_synth.aster_fill_(sd, 81)
        sd = {k: v.clone() for k, v in sd.items()}
        ref.load_state_dict(sd)
        img = aster_synth.aster_images(ASTER_IDS)
        n = img.shape[0]
        x = img * 2 - 1
        out = ref({'images': x, 'rec_targets': torch.IntTensor(n, 100).fill_(1), 'rec_lengths': [100] * n})
        pred_rec = out['output']['pred_rec']
        stn_in = F.interpolate(x, ref.tps_inputsize, mode='bilinear', align_corners=True)
        _, ctrl = ref.stn_head(stn_in)
        rect, _ = ref.tps(x, ctrl)
        enc = ref.encoder
        layers = [enc.layer0(rect)]
        for li in range(1, 6):
            layers.append(getattr(enc, "layer%d" % li)(layers[-1]))
        feats = enc(rect).contiguous()
        dec = ref.decoder.decoder
        xproj = dec.attention_unit.xEmbed(feats.view(-1, 512)).view(n, -1, 512)
        # the beam search step by step on the reference's DecoderUnit
        K, C, eos, L = 5, 97, 94, 100
        fi = feats.unsqueeze(1).expand(n, K, 25, 512).reshape(n * K, 25, 512).contiguous()
        state = torch.zeros(1, n * K, 512)
        pos = (torch.arange(n) * K).view(-1, 1)
        seq = torch.full((n * K, 1), -float('inf'))
        seq[::K] = 0.0
        y = torch.full((n * K,), C, dtype=torch.long)
        sym, pred, score, gaps, steps = [], [], [], [], {}
        for i in range(L):
            if i in ASTER_STEPS:
                rows = torch.arange(2 * K)       # all beams of images 0 and 1 (their encoder features are stored in full)
                s_in, y_in = state[0, rows].clone(), y[rows].clone()
                alpha = dec.attention_unit(fi[:2 * K], s_in.unsqueeze(0))
                lg, s_out = dec(fi[:2 * K], s_in.unsqueeze(0), y_in)
                steps[i] = (s_in, y_in, lg, s_out[0], alpha)
            o, state = dec(fi, state, y)
            cand = (seq + F.log_softmax(o, dim=1)).view(n, -1)
            top6 = cand.topk(6, 1)[0]
            g = top6[:, :-1] - top6[:, 1:]
            g[~torch.isfinite(g)] = float('inf')
            gaps.append(g.min(1)[0])
            top, idx = cand.topk(K, 1)
            y = (idx % C).view(-1)
            seq = top.view(-1, 1)
            p = (idx // C + pos).view(-1)
            state = state.index_select(1, p)
            score.append(seq.view(-1).clone())
            seq = seq.masked_fill(y.view(-1, 1).eq(eos), -float('inf'))
            pred.append(p)
            sym.append(y)
        sym, pred, score, gaps = torch.stack(sym), torch.stack(pred), torch.stack(score), torch.stack(gaps)
        from dpmn_amd.utils.labelmaps import beam_backtrack
        assert (torch.from_numpy(beam_backtrack(sym.numpy(), pred.numpy(), score.numpy(), n, K, eos)) == pred_rec).all(), \
            "the step-by-step run does not reproduce the reference's beam_search"
        info = AsterInfo('all')
        strings, _ = get_str_list(pred_rec, torch.ones_like(pred_rec), info)
        margin = gaps.min(0)[0]
        first_eos = [int((r == eos).nonzero()[0]) if (r == eos).any() else -1 for r in pred_rec]
        assert len(set(strings)) >= 3, strings
        assert sum(1 for e in first_eos if 1 <= e <= 30) * 2 >= n, first_eos
        assert int((margin < 1e-3).sum()) * 4 <= n, margin.tolist()
        # a beam other than the winner emits EOS before the last step (the winner accounts for at most one EOS of its image)
        ended = [int((sym[:L - 1, b * K:(b + 1) * K] == eos).sum()) - (1 if 0 <= first_eos[b] < L - 1 else 0) for b in range(n)]
        assert max(ended) >= 1, "no beam other than the winner ends early"
        arrs = dict(ids=np.array(ASTER_IDS), manifest=manifest(sd), checksum=checksum(sd), vocabulary=np.array(info.voc),
                    stn_input=stn_in[:, :, ::4, ::4].contiguous(), ctrl=ctrl, rectified=rect[:, :, ::4, ::5].contiguous(),
                    encoder=feats[:, :, ::8].contiguous(), feats01=feats[:2].contiguous(), xproj01=xproj[:2, :, ::4].contiguous(), symbols=sym.to(torch.int32),
                    predecessors=pred.to(torch.int32), scores=score, gaps=gaps, margin=margin, pred_rec=pred_rec.to(torch.int32),
                    strings=np.array(strings), steps=np.array(ASTER_STEPS))
        for li, t in enumerate(layers):
            arrs["layer%d_sample" % li] = _sample(t)
            arrs["layer%d_norm" % li] = np.array(float(t.double().norm()))
        for i, (s_in, y_in, lg, s_out, alpha) in steps.items():
            arrs.update({"step%d_state" % i: s_in, "step%d_y" % i: y_in.to(torch.int32), "step%d_logits" % i: lg, "step%d_new" % i: s_out,
                         "step%d_alpha" % i: alpha})
        save("aster", **arrs)
    finally:
        restore()


def gen_aster_beam():
    """Backtracking of the beam search (attention_recognition_head.py:124-184): the reference's own beam_search run on hand-made
    decoder outputs -- a stand-in DecoderUnit that returns a table of per-(step, row) log-probabilities, so the stored symbols,
    predecessors and scores are hand-made -- with EOS at step 0, mid-string and never, several beams ending at the same step and
    exactly equal final scores.  Plus get_str_list's strings and the four vocabularies."""
    ref, restore = _aster_reference()
    from utils.metrics import get_str_list
    from utils.labelmaps import get_vocabulary
    AsterInfo = _ref_aster_info
    try:
        head = ref.decoder
        B, K, C, eos, L = 6, 5, 97, 94, 100
        rng = np.random.RandomState(5)
        table = np.full((L, B * K, C), 1e-4)

        def put(t, b, probs, rows=range(K), same=False):
            for r in rows:       # rows of an image differ slightly unless `same`: exact score ties only where they are meant
                for c, pr in probs.items():
                    table[t, b * K + r, c] = pr if same else pr * (1.0 - 0.03 * r - 0.001 * (c % 7))
        put(0, 0, {eos: 0.5, 10: 0.2, 11: 0.1, 12: 0.05})                       # image 0: EOS wins at step 0
        for t in range(1, L):
            put(t, 0, {int(rng.randint(0, 94)): 0.4, eos: 0.3})
        for t in range(L):                                                      # image 1: EOS mid-string (step 4) on the best beam
            put(t, 1, {20 + t % 7: 0.6, 30 + t % 5: 0.2, eos: 0.7 if t == 4 else 0.01})
        for t in range(L):                                                      # image 2: never EOS
            put(t, 2, {40 + t % 11: 0.5, 50 + t % 3: 0.3, eos: 1e-6})
        put(0, 3, {10: 0.25, 11: 0.25, 12: 0.25, 13: 0.125, 14: 0.0625}, same=True)        # image 3: equal beams, all end at step 3 with equal scores
        for t in range(1, L):
            put(t, 3, {eos: 0.5, 15: 0.25} if t == 3 else {16 + t % 4: 0.5, 70: 0.25, eos: 1e-6}, same=t <= 3)      # (distinct scores at the last step)
        for t in range(L):                                                      # image 4: several beams end at the same steps
            put(t, 4, {eos: 0.3, 60: 0.3, 61: 0.2} if t in (2, 6) else {62 + t % 9: 0.45, 80: 0.35, eos: 1e-5})
        for t in range(L):                                                      # image 5: random rows
            for r in range(K):
                put(t, 5, {int(c): float(v) for c, v in zip(rng.choice(C, 6, replace=False), rng.rand(6))}, rows=[r])
        table = torch.from_numpy(np.log(table / table.sum(-1, keepdims=True))).float()
        calls = []

        class Stub(torch.nn.Module):
            def forward(self, x, state, y_prev):
                calls.append(1)
                return table[len(calls) - 1], state
        head.decoder = Stub()
        pred_rec, _ = head.beam_search(torch.zeros(B, 25, 512), K, eos)
        # the stored tensors of that run: the same loop on the table (no decoder state involved)
        import torch.nn.functional as F
        seq = torch.full((B * K, 1), -float('inf'))
        seq[::K] = 0.0
        pos = (torch.arange(B) * K).view(-1, 1)
        sym, pred, score = [], [], []
        for i in range(L):
            cand = (seq.repeat(1, C) + F.log_softmax(table[i], dim=1)).view(B, -1)
            top, idx = cand.topk(K, 1)
            y = (idx % C).view(-1)
            seq = top.view(-1, 1)
            score.append(seq.view(-1).clone())
            pred.append((idx // C + pos).view(-1))
            seq = seq.masked_fill(y.view(-1, 1).eq(eos), -float('inf'))
            sym.append(y)
        sym, pred, score = torch.stack(sym), torch.stack(pred), torch.stack(score)
        from dpmn_amd.utils.labelmaps import beam_backtrack
        mine = torch.from_numpy(beam_backtrack(sym.numpy(), pred.numpy(), score.numpy(), B, K, eos))
        assert (mine == pred_rec).all(), "numpy backtracking differs from the reference at images %s" % ((mine != pred_rec).any(1).nonzero().view(-1).tolist(),)
        last = score[-1].view(B, K)
        assert len(set(score[3, 3 * K:4 * K].tolist())) < K, "image 3 was built to end several beams with exactly equal scores"
        info = AsterInfo('all')
        strings, _ = get_str_list(pred_rec, torch.ones_like(pred_rec), info)
        ids = torch.tensor([[10, 36, 62, 95, 96, 70, 94, 5] + [1] * 92, [94] + [3] * 99, list(range(94)) + [94] * 6, [96] * 100], dtype=torch.int64)
        id_strings, _ = get_str_list(ids, torch.ones_like(ids), info)
        save("aster_beam", symbols=sym.to(torch.int32), predecessors=pred.to(torch.int32), scores=score, pred_rec=pred_rec.to(torch.int32),
             strings=np.array(strings), ids=ids.to(torch.int32), id_strings=np.array(id_strings),
             **{"voc_" + v: np.array(get_vocabulary(v)) for v in ('digit', 'lower', 'upper', 'all')},
             rec_num_classes=np.array([AsterInfo(v).rec_num_classes for v in ('digit', 'lower', 'upper', 'all')]))
    finally:
        restore()


MORAN_IDS = [0, 1, 10, 3, 5, 18, 31, 8]      # members of utils/moran_synth.py's image pool (chosen by gen_moran_pick on the reference's own run, asserted below)
MORAN_MARGIN = 1e-3


def _moran_reference():
    from model.moran.moran import MORAN
    from dpmn_amd.utils import moran_synth
    ref = MORAN(1, 37, 256, 32, 100, BidirDecoder=True, inputDataType='torch.FloatTensor', CUDA=False).eval()
    sd = ref.state_dict()
    assert len(sd) == 427 and abs(sum(p.numel() for p in ref.parameters()) / 1e6 - 20.34) < 0.01
    moran_synth.moran_fill_(sd, 91)
    sd = {k: v.clone() for k, v in sd.items()}
    ref.load_state_dict(sd)
    return ref, sd


def _moran_run(ref, img):
    """parse_moran_data (base.py:396-409, restated: importing interfaces.base pulls in the LMDB data path) and the reference's eval
    call (super_resolution.py:453-457) with debug=False, which gives the same predictions without the cv2 / colour drawing."""
    import torch.nn.functional as F
    n = img.shape[0]
    x = F.interpolate(img, (32, 100), mode='bicubic')
    gray = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    length = torch.IntTensor([20] * n)
    text = torch.zeros(n * 20, dtype=torch.long)
    preds, _ = ref(gray, length, text, text, test=True, debug=False)
    return gray, length, preds.view(n, 20, 37)


def gen_moran_pick():
    """Prints, for every member of the image pool, the reference's string and smallest decision margin: MORAN_IDS is chosen from
    this list (margin >= 1e-3, distinct strings, some cut by '$' and some not)."""
    from dpmn_amd.utils import moran_synth
    from dpmn_amd.utils.labelmaps import moran_strings
    ref, _ = _moran_reference()
    _, _, logits = _moran_run(ref, moran_synth.moran_images(moran_synth.POOL))
    top2 = logits.topk(2, 2)[0]
    margin = (top2[..., 0] - top2[..., 1]).min(1)[0]
    ids = logits.max(2)[1]
    for i, s in enumerate(moran_strings(ids.numpy())):
        print("%2d margin %.2e  %-22r first $ %s" % (i, float(margin[i]), s, (ids[i] == 36).nonzero()[:1].view(-1).tolist()))


def gen_moran():
    """The MORAN recogniser (model/moran/) in eval mode (test=True) on name-seeded weights (utils/moran_synth.py moran_fill_, seed 91)
    and 8 soft-bar images of 32 x 128: the prep output, the accumulated offsets after each of MORN's two passes and the rectified image
    (morn.py:58-82 re-run on the reference's own members and checked against its forward), the ResNet and BiLSTM outputs, i2h(feats),
    the 20 x 37 L2R logits with their ids and margins, the strings of the reference's converter."""
    import string
    import torch.nn.functional as F
    from dpmn_amd.utils import moran_synth
    from utils import utils_moran
    ref, sd = _moran_reference()
    img = moran_synth.moran_images(MORAN_IDS)
    n = img.shape[0]
    grab = {}
    ref.ASRN.cnn.register_forward_hook(lambda m, i, o: grab.__setitem__("resnet", o.clone()))
    ref.ASRN.rnn.register_forward_hook(lambda m, i, o: grab.__setitem__("rnn", o.clone()))
    gray, length, logits = _moran_run(ref, img)
    morn = ref.MORN
    grid, gx, gy = morn.grid[:n], morn.grid_x[:n], morn.grid_y[:n]

    def offs(x):
        o = morn.cnn(x)
        pool = morn.pool(F.relu(o)) - morn.pool(F.relu(-o))
        return F.grid_sample(pool, grid).permute(0, 2, 3, 1).contiguous()
    acc1 = offs(F.interpolate(gray, size=(32, 100), mode='bilinear'))
    rect1 = F.grid_sample(gray, torch.cat([gx, gy + acc1], 3))
    acc2 = acc1 + offs(rect1)
    rect = F.grid_sample(gray, torch.cat([gx, gy + acc2], 3))
    assert torch.equal(rect, morn(gray, True)), "the step-by-step MORN does not reproduce the reference's forward"
    ids = logits.max(2)[1]
    top2 = logits.topk(2, 2)[0]
    margin = top2[..., 0] - top2[..., 1]
    alphabet = ':'.join(string.digits + string.ascii_lowercase + '$')
    conv = utils_moran.strLabelConverterForAttention(alphabet, ':')
    sim = conv.decode(ids.reshape(-1), length)
    strings = [s.split('$')[0] for s in sim]
    # conditions on the fixture
    assert len(set(strings)) >= 4, strings
    assert any((r == 36).any() for r in ids) and any(not (r == 36).any() for r in ids), strings
    assert float(margin.min()) >= MORAN_MARGIN, "decision margin %.2e: choose other MORAN_IDS (gen_moran_pick)" % float(margin.min())
    amax = float(acc2.abs().max())
    iy = ((gy + acc2 + 1) * 32 - 1) / 2      # grid_sample's source row (align_corners=False): every pixel keeps a tap inside the image
    iy1 = ((gy + acc1 + 1) * 32 - 1) / 2
    assert amax >= 0.05, "offsets trivially small: %.3f" % amax
    assert float(min(iy.min(), iy1.min())) > -1.0 and float(max(iy.max(), iy1.max())) < 32.0, "a pixel samples wholly outside the image"
    rnn = grab["rnn"]
    i2h = ref.ASRN.attentionL2R.attention_cell.i2h(rnn)
    assert float((img - img.half().float()).abs().max()) == 0.0      # fp16-representable by construction: stored losslessly in half the bytes
    print("moran: strings %s, min margin %.2e, max |offset| %.3f, source rows %.2f .. %.2f" % (strings, float(margin.min()), amax, float(iy.min()), float(iy.max())))
    save("moran", ids=np.array(MORAN_IDS), manifest=manifest(sd), checksum=checksum(sd), images=img.half(), prep=gray,
         offsets1=acc1[..., 0].contiguous(), offsets2=acc2[..., 0].contiguous(), rectified=rect, resnet=grab["resnet"][:, ::4].contiguous(),
         rnn=rnn.permute(1, 0, 2)[:, :, ::2].contiguous(), i2h=i2h.permute(1, 0, 2)[:, :, ::2].contiguous(), logits=logits,
         pred_ids=ids.to(torch.int32), margin=margin, strings=np.array(strings), raw_strings=np.array(sim))


def gen_moran_labels():
    """The reference's own strLabelConverterForAttention.decode (utils/utils_moran.py:79-107) with the converter of base.py:60-61 on
    flat id sequences of 20 per image, exactly as eval() calls it (super_resolution.py:457-459): '$' at position 0, at position 19,
    nowhere, mid-string, every class once; plus a single sequence (the scalar-length branch)."""
    import string
    from utils import utils_moran
    alphabet = ':'.join(string.digits + string.ascii_lowercase + '$')
    conv = utils_moran.strLabelConverterForAttention(alphabet, ':')
    L = 20
    rows = [[36] + [5] * (L - 1),                              # '$' at position 0: empty string
            list(range(10, 29)) + [36],                         # '$' at position 19
            [(3 * i) % 36 for i in range(L)],                   # no '$' at all
            [17, 14, 21, 21, 24, 36, 36, 1, 2, 36] + [0] * 10,  # cut mid-string, more '$' behind
            list(range(0, 20)), list(range(17, 37))]            # every class once (two rows)
    rng = np.random.RandomState(13)
    for _ in range(6):
        rows.append(rng.randint(0, 37, L).tolist())
    ids = torch.tensor(rows, dtype=torch.int64)
    texts = conv.decode(ids.reshape(-1), torch.IntTensor([L] * len(rows)))
    single = conv.decode(ids[3], torch.IntTensor([L]))
    save("moran_labels", ids=ids.to(torch.int32), texts=np.array(texts), cut=np.array([s.split('$')[0] for s in texts]),
         single=np.array(single), alphabet=np.array(conv.alphabet))


def gen_collate():
    """Data path: the reference's own `resizeNormalize` and `alignCollate_realWTLAMask.__call__`
    (dataset/dataset.py:1266-1319, 1966-2076) and `str_filt` (utils/util.py) run on five synthetic RGB images of ragged sizes
    (the generator of tests/test_dataset.py::_fake_env, RandomState(7)) and labels that exercise every branch of the label
    spreading (1 char, empty, 2..25 chars, >= 26 chars, out-of-alphabet characters).
    Import-time shims beyond tools/ref_shims.py (none of them executed except ToTensor): lmdb, imgaug.augmenters (constructed by
    alignCollate_syn.__init__, never applied by this class), cv2, torchvision.utils.  torchvision.transforms.ToTensor IS executed
    and is stood in for by its definition for uint8 PIL images (HWC uint8 -> CHW float32 / 255): torchvision is absent."""
    import types
    from PIL import Image

    class _Any:
        def __getattr__(self, k):
            return _Any()

        def __call__(self, *a, **k):
            return _Any()

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img, dtype=np.uint8)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255)

    tvt = sys.modules["torchvision.transforms"]
    tvt.ToTensor = ToTensor
    tvt.ToPILImage = _Any
    sys.modules["torchvision"].utils = types.ModuleType("torchvision.utils")
    sys.modules["torchvision.utils"] = sys.modules["torchvision"].utils
    sys.modules["torchvision.utils"].make_grid = None
    sys.modules["torchvision"].transforms = tvt
    for name in ("lmdb", "imgaug"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["imgaug.augmenters"] = _Any()
    sys.modules["imgaug"].augmenters = sys.modules["imgaug.augmenters"]
    import scipy
    scipy.finfo = np.finfo      # version skew: dataset.py builds an (unused here) blur kernel at import through scipy.finfo (removed in scipy 1.x)
    from dataset import dataset as rds       # /root/reference/dataset/dataset.py
    from utils import str_filt as ref_str_filt

    rng = np.random.RandomState(7)
    words = ["Hello", "a", "", "SuperResolution-2023!", "abcdefghijklmnopqrstuvwxyz0123"]
    batch = []
    for i in range(1, 6):
        hr = rng.randint(0, 256, (40 + 3 * i, 150 + 7 * i, 3)).astype(np.uint8)
        lr = rng.randint(0, 256, (18 + i, 70 + 3 * i, 3)).astype(np.uint8)
        ph, pl = Image.fromarray(hr), Image.fromarray(lr)
        batch.append((ph, pl, ph, pl, ref_str_filt(words[i - 1], "all")))
    out = {}
    for mask in (True, False):
        col = rds.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=mask)
        r = col(batch)
        tag = "mask" if mask else "nomask"
        out["hr_" + tag] = r[0].numpy()
        out["lr_" + tag] = r[2].numpy()
        if mask:
            out["label_vecs"] = r[6].numpy()
            out["weighted_masks"] = r[7].numpy()
            out["weighted_tics"] = r[8].numpy()
            out["label_strs"] = np.array(list(r[5]))
    filt_in = ["Hello, World!", "abc DEF 123", "", "!!", "MiXed-Case_09"]
    for voc in ("lower", "upper", "all", "digit"):
        out["str_filt_" + voc] = np.array([ref_str_filt(w, voc) for w in filt_in])
    out["str_filt_in"] = np.array(filt_in)
    save("collate", **out)


def gen_display():
    """The LR / SR / HR comparison images of tripple_display (interfaces/base.py:275-298) for ops.display_triple.  torchvision is
    absent and the reference method cannot be imported, so the expected bytes come from PIL itself plus the two torchvision formulas
    restated on torch CPU tensors: ToPILImage = x.mul(255).byte(), Image.resize((W, H), BICUBIC), ToTensor = / 255, make_grid(nrow=1,
    padding=0) = vertical stack, save_image = x.mul(255).add_(0.5).clamp_(0, 255).to(uint8).  Inputs are stored (small or compressible):
      a  B = 3, 4 channels, 16x64 -> 32x128: image 0 random, image 1 binary 0 / 1 (overshoot clipping in both passes), image 2 the
         quantisation edges: SR / HR values k / 255 and (k + 0.5) / 255, LR values k / 255, each exact and one ulp up and down, all k
      b  6x10 -> 16x24 (non-integer ratio)      c  64x256 -> 128x512 (config 4), blocky content so that the file stays small"""
    from PIL import Image
    from dpmn_amd.utils import display as dsp, resize as rsz
    rng = np.random.RandomState(20240611)
    f32 = np.float32

    def expected(lr, sr, hr, sel):
        H, W = hr.shape[-2:]
        out = []
        for b in sel:
            u8 = torch.from_numpy(lr[b, :3]).mul(255).byte().numpy().transpose(1, 2, 0)
            big = np.asarray(Image.fromarray(np.ascontiguousarray(u8)).resize((W, H), Image.BICUBIC))
            t_in = torch.from_numpy(np.ascontiguousarray(big.transpose(2, 0, 1))).float().div(255)
            grid = torch.cat([t_in, torch.from_numpy(sr[b, :3]), torch.from_numpy(hr[b, :3])], 1)      # make_grid(nrow=1, padding=0)
            out.append(grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy())
        return np.stack(out)

    def ulps(v):
        v = np.asarray(v, f32)
        return np.concatenate([np.nextafter(v, f32(-1)), v, np.nextafter(v, f32(2))]).astype(f32)

    k = np.arange(256, dtype=np.float64)
    edge_lr = ulps((k / 255).astype(f32))                                                   # 768 values: the truncation boundary
    edge_sr = np.concatenate([ulps((k / 255).astype(f32)), ulps(((k + 0.5) / 255).astype(f32))])      # 1536: the rounding boundary
    lr = np.empty((3, 4, 16, 64), f32)
    sr = np.empty((3, 4, 32, 128), f32)
    hr = np.empty((3, 4, 32, 128), f32)
    lr[:, 3], sr[:, 3], hr[:, 3] = 0.6, 0.3, 0.9            # a 4th channel that would show if it were read
    lr[0, :3], sr[0, :3], hr[0, :3] = rng.rand(3, 16, 64), rng.rand(3, 32, 128), rng.rand(3, 32, 128)
    lr[1, :3], sr[1, :3], hr[1, :3] = rng.randint(0, 2, (3, 16, 64)), rng.randint(0, 2, (3, 32, 128)), rng.randint(0, 2, (3, 32, 128))
    for c in range(3):
        plane = np.resize(np.roll(edge_lr, 37 * c), 16 * 64)
        lr[2, c] = plane.reshape(16, 64)
        sr[2, c] = np.resize(np.roll(edge_sr, 101 * c), 32 * 128).reshape(32, 128)
        hr[2, c] = np.resize(np.roll(edge_sr[::-1], 53 * c), 32 * 128).reshape(32, 128)
    for c in range(3):
        assert np.isin(edge_lr, lr[2, c]).all() and np.isin(edge_sr, sr[2, c]).all() and np.isin(edge_sr, hr[2, c]).all()
    # x * 255 + 0.5 rounded once (a fused multiply-add: exact in float64, then to fp32) gives other floats than the two roundings
    # of save_image on some crafted values; recorded, not asserted on the bytes: next to (k + 0.5) / 255 both forms truncate to
    # the same byte on every value tried, so the fixture pins the two-step form without depending on that
    two = (edge_sr * f32(255) + f32(0.5))
    one = (edge_sr.astype(np.float64) * 255.0 + 0.5).astype(f32)
    n_fused_differs = int((two != one).sum())
    # overshoot: unclipped sums of either pass below 0 / above 255 on the binary image
    lo = hi = 0
    u8 = dsp.quantize_lr(lr[1, :3]).transpose(1, 2, 0).astype(np.int64)
    th, tv = rsz.pil_resample_tables(64, 128), rsz.pil_resample_tables(16, 32)
    hor = np.stack([(1 << 21) + sum(u8[:, th[x, 0] + j] * int(th[x, 2 + j]) for j in range(th[x, 1])) for x in range(128)], 1) >> 22
    lo, hi = lo + int((hor < 0).sum()), hi + int((hor > 255).sum())
    hor = np.clip(hor, 0, 255)
    ver = np.stack([(1 << 21) + sum(hor[tv[y, 0] + j] * int(tv[y, 2 + j]) for j in range(tv[y, 1])) for y in range(32)], 0) >> 22
    lo, hi = lo + int((ver < 0).sum()), hi + int((ver > 255).sum())
    assert lo >= 100 and hi >= 100, "the binary image clips too few overshoot pixels (%d below, %d above)" % (lo, hi)
    sel_a = [2, 0]
    exp_a = expected(lr, sr, hr, sel_a)
    exp_all = expected(lr, sr, hr, [0, 1, 2])
    assert not (exp_all[0] == exp_all[1]).all() and not (exp_all[1] == exp_all[2]).all() and not (exp_all[0] == exp_all[2]).all()
    assert (exp_a[0] == exp_all[2]).all() and (exp_a[1] == exp_all[0]).all() and not (exp_a[0] == exp_a[1]).all()

    lr_b, sr_b, hr_b = rng.rand(1, 3, 6, 10).astype(f32), rng.rand(1, 3, 16, 24).astype(f32), rng.rand(1, 3, 16, 24).astype(f32)
    exp_b = expected(lr_b, sr_b, hr_b, [0])

    def blocky(h, w, bs):      # uint8: random colours in bs x bs blocks (stored as uint8, the test divides by 255)
        return np.kron(rng.randint(0, 256, (3, h // bs, w // bs)), np.ones((bs, bs), np.int64)).astype(np.uint8)
    lr_c, sr_c, hr_c = blocky(64, 256, 4)[None], blocky(128, 512, 8)[None], blocky(128, 512, 8)[None]
    exp_c = expected(*((a.astype(f32) / f32(255)) for a in (lr_c, sr_c, hr_c)), [0])
    assert not (exp_c[0, :128] == exp_c[0, 128:256]).all()
    save("display", a_lr=lr, a_sr=sr, a_hr=hr, a_sel=np.array(sel_a, np.int32), a_expected=exp_a,
         b_lr=lr_b, b_sr=sr_b, b_hr=hr_b, b_expected=exp_b, c_lr_u8=lr_c, c_sr_u8=sr_c, c_hr_u8=hr_c, c_expected=exp_c,
         edge_lr=edge_lr, edge_sr=edge_sr, n_fused_differs=np.array(n_fused_differs), overshoot=np.array([lo, hi]))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["all"]
    GENS["crnn"] = gen_crnn
    GENS["crnn_ctc"] = gen_crnn_ctc
    GENS["aster"] = gen_aster
    GENS["aster_beam"] = gen_aster_beam
    GENS["moran"] = gen_moran
    GENS["moran_labels"] = gen_moran_labels
    GENS["display"] = gen_display
    GENS["collate"] = gen_collate     # last: it installs extra import shims (lmdb, imgaug, torchvision.utils)
    for name, fn in GENS.items():
        if "all" in which or name in which:
            fn()
    if "moran_pick" in which:
        gen_moran_pick()
