"""GPU parity of the native ASTER recogniser (model/aster.py NativeASTER, csrc/aster.hip) against the imported reference
(tests/golden/aster.npz, tools/gen_golden.py gen_aster) and against the stock-operator mirror on the same device: prep, STN head +
TPS, ResNet + BiLSTM encoder, xEmbed projection, one teacher-forced decoder step from the recorded state, the beam search id for id
where the recorded decision margin allows it, batch independence, the eval-only guard.

Tolerances: 1e-4 abs + rel per kernel, 3e-4 per module.  Beam search: ids equal for every image whose recorded
margin (smallest gap between consecutive entries of the top 6 candidate scores over all steps) is >= 1e-3; the other images (at
most one in four) by prefix up to the first step whose own gap is below 1e-3."""
import numpy as np
import pytest
import torch

from dpmn_amd.utils import aster_synth
from helpers import checksum, load_golden, record, t

pytestmark = pytest.mark.gpu
MARGIN = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env(dev):
    from dpmn_amd.model.aster import ASTER, NativeASTER
    z = load_golden("aster")
    cpu = ASTER().eval()
    sd = cpu.state_dict()
    assert [r.split("|")[0] for r in z["manifest"].tolist()] == list(sd.keys())
    aster_synth.aster_fill_(sd, 81)
    assert abs(checksum(sd) - float(z["checksum"])) < 1e-6 * max(1.0, abs(float(z["checksum"])))
    cpu.load_state_dict(sd)
    nat = NativeASTER().to(dev).eval()
    nat.load_state_dict(sd)
    mir = ASTER().to(dev).eval()
    mir.load_state_dict(sd)
    img = aster_synth.aster_images(z["ids"].tolist())
    return {"z": z, "cpu": cpu, "nat": nat, "mir": mir, "img": img, "cpu_stages": cpu.stages(img), "sd": sd}


def _close(name, what, got, ref, atol, rtol):
    got, ref = torch.as_tensor(got).float().cpu(), torch.as_tensor(ref).float().cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    ratio = float((err / (atol + rtol * ref.abs())).max())
    record(name, "%s: max abs err %.3e, worst err / (atol + rtol |ref|)" % (what, float(err.max())), ratio, 1.0)
    assert ratio <= 1.0, "%s: max abs err %.3e, %.2f x the tolerance (atol %.0e, rtol %.0e)" % (what, float(err.max()), ratio, atol, rtol)
    return float(err.max())


def test_prep_and_rectify(env, dev):
    z, nat, cs = env["z"], env["nat"], env["cpu_stages"]
    norm, stn_in = nat.prep(env["img"].to(dev))
    stn_nchw = stn_in[..., :3].permute(0, 3, 1, 2)
    assert float(stn_in[..., 3].abs().max()) == 0.0
    _close("aster_prep", "normalised image vs x * 2 - 1", norm, env["img"] * 2 - 1, 1e-6, 0.0)
    _close("aster_prep", "STN input vs reference", stn_nchw[:, :, ::4, ::4], t(z["stn_input"]), 1e-4, 1e-4)
    _close("aster_prep", "STN input vs mirror", stn_nchw, cs["stn_input"], 1e-4, 1e-4)
    ctrl, rect = nat.rectify(norm, stn_in)
    _close("aster_rectify", "control points vs reference", ctrl, t(z["ctrl"]), 1e-4, 1e-4)
    ms = env["mir"].stages(env["img"].to(dev))
    _close("aster_rectify", "control points vs mirror on the GPU", ctrl, ms["ctrl"], 1e-4, 1e-4)


def test_rectified_image(env, dev):
    """dpmn_tps_sample_f32 at 32 x 128 -> 32 x 100 on the reference's own control points (a control-point error of 1e-4 alone moves a
    sample by 0.013 pixel), 1e-4 abs + rel against the mirror on the same device and against the reference.
    The TPS sums (23 terms against an inverse kernel with large entries of both signs) leave ~1e-3 pixel of fp32 rounding in a source
    coordinate, so two summation orders differ by about that times the image slope: on images with unit steps between neighbouring
    pixels the stock-operator mirror on the GPU is itself 1.6e-3 from the CPU reference (measured; this kernel 7.7e-4 from the mirror).
    grid_sample's zero padding adds a ramp of the border pixel's height over one pixel.  The fixture images are therefore
    band-limited and fade to 0 (normalised) at the borders (utils/aster_synth.py aster_images); measured on them: 2.1e-5 from the
    mirror, 4.0e-5 from the reference."""
    from dpmn_amd import ops
    z, nat = env["z"], env["nat"]
    norm, _ = nat.prep(env["img"].to(dev))
    ref_ctrl = t(z["ctrl"]).to(dev)
    rect_k, src = ops.tps_sample(norm, ref_ctrl, nat.tps.inverse_kernel, nat.tps.target_coordinate_repr, (32, 100))
    mir = env["mir"].tps_torch(norm, ref_ctrl)
    record("aster_rectify", "stock-operator mirror on the GPU vs reference, rectified image max abs err",
           float((mir[:, :, ::4, ::5].cpu() - t(z["rectified"])).abs().max()))
    print("rectified: native vs mirror %.3e, native vs reference %.3e, mirror vs reference %.3e" % (
        float((rect_k - mir).abs().max()), float((rect_k[:, :, ::4, ::5].cpu() - t(z["rectified"])).abs().max()),
        float((mir[:, :, ::4, ::5].cpu() - t(z["rectified"])).abs().max())))
    _close("aster_rectify", "rectified image (reference control points) vs mirror on the GPU", rect_k, mir, 1e-4, 1e-4)
    _close("aster_rectify", "rectified image (reference control points) vs reference", rect_k[:, :, ::4, ::5], t(z["rectified"]), 1e-4, 1e-4)


def test_strided_pointwise_conv_gather(dev):
    """dpmn_subsample_nhwc_f32: the (2, 1) and (2, 2) gathers are exact copies."""
    from dpmn_amd import ops
    x = torch.randn(3, 8, 25, 64, device=dev)
    for sy, sx in ((2, 1), (2, 2), (1, 2), (3, 2)):
        assert torch.equal(ops.subsample_nhwc(x, sy, sx), x[:, ::sy, ::sx].contiguous())


def test_encoder(env, dev):
    """Module tolerance 3e-4; should the 45-conv stack not meet it, the bound is 3 x the error of the stock-operator mirror on the
    GPU against the same CPU-reference fixture -- both errors are recorded."""
    z, nat, cs = env["z"], env["nat"], env["cpu_stages"]
    rect = cs["rectified"].to(dev)
    layers = nat.resnet(rect)
    for li, f in enumerate(layers):
        nchw = f.permute(0, 3, 1, 2).contiguous().cpu()
        ref = cs["layers"][li]
        n = 256
        flat = nchw.reshape(-1)
        smp = flat[::max(1, flat.numel() // n)][:n]
        e = float((smp - t(z["layer%d_sample" % li])).abs().max())
        record("aster_encoder", "layer%d sample vs reference, max abs err (ref max %.2f)" % (li, float(ref.abs().max())), e)
        rel = float((nchw - ref).norm() / ref.norm())
        record("aster_encoder", "layer%d vs CPU mirror, relative L2" % li, rel, 1e-4)
        assert rel <= 1e-4, "layer%d: relative L2 %.2e" % (li, rel)
    enc = nat.encode(rect)
    ref = t(z["encoder"])
    mir = env["mir"].stages(env["img"].to(dev))["encoder"]
    e_mir = float((mir[:, :, ::8].cpu() - ref).abs().max())
    e_nat = float((enc[:, :, ::8].cpu() - ref).abs().max())
    tol = max(3e-4, 3.0 * e_mir)
    record("aster_encoder", "encoder output vs reference: stock-operator mirror on the GPU, max abs err", e_mir)
    record("aster_encoder", "encoder output vs reference: native, max abs err", e_nat, tol)
    assert e_nat <= tol, "encoder output: native %.3e, mirror %.3e, allowed %.3e" % (e_nat, e_mir, tol)
    _close("aster_encoder", "encoder output vs CPU mirror (all elements)", enc, cs["encoder"], tol, 0.0)


def test_xproj_and_decoder_step(env, dev):
    """On the reference's own encoder features of images 0 and 1 (stored in full): the xEmbed projection, and one teacher-forced
    step for all ten beam rows of the two images from the recorded (state, y_prev) of three steps."""
    z, nat = env["z"], env["nat"]
    feats = t(z["feats01"]).to(dev)
    _close("aster_xproj", "xEmbed(feats) vs reference", nat.xproj(feats)[:, :, ::4], t(z["xproj01"]), 1e-4, 1e-4)
    rows = torch.arange(10) // 5
    for i in z["steps"].tolist():
        logits, new, alpha = nat.decode_step(feats, rows, t(z["step%d_state" % i]).to(dev), t(z["step%d_y" % i]))
        _close("aster_decode_step", "step %d logits" % i, logits, t(z["step%d_logits" % i]), 1e-4, 1e-4)
        _close("aster_decode_step", "step %d new state" % i, new, t(z["step%d_new" % i]), 1e-4, 1e-4)
        _close("aster_decode_step", "step %d alpha" % i, alpha, t(z["step%d_alpha" % i]), 1e-4, 1e-4)


def _check_beam(name, z, rec, stored, ref_rec, ref_sym, ref_pred, ref_score, K=5):
    margin, gaps = z["margin"], z["gaps"]
    n = len(margin)
    below = [b for b in range(n) if margin[b] < MARGIN]
    assert 4 * len(below) <= n, "degenerate fixture: %d of %d images below the margin" % (len(below), n)
    worst = 0.0
    for b in range(n):
        cols = slice(b * K, (b + 1) * K)
        if margin[b] >= MARGIN:
            assert np.array_equal(stored["symbols"][:, cols], ref_sym[:, cols]), "image %d: stored symbols differ" % b
            assert np.array_equal(stored["predecessors"][:, cols], ref_pred[:, cols]), "image %d: stored predecessors differ" % b
            assert np.array_equal(np.asarray(rec[b]), ref_rec[b]), "image %d: pred_rec differs" % b
            fin = np.isfinite(ref_score[:, cols])
            worst = max(worst, float(np.abs(stored["scores"][:, cols][fin] - ref_score[:, cols][fin]).max()))
        else:
            t0 = int(np.argmax(gaps[:, b] < MARGIN))
            assert np.array_equal(stored["symbols"][:t0, cols], ref_sym[:t0, cols]), "image %d: symbols differ before step %d" % (b, t0)
            keep = 0      # prefix of pred_rec that the steps before t0 decide
            while keep < t0 and ref_rec[b][keep] != 94:
                keep += 1
            if keep == t0:      # the reference's winner is still open at t0: only the symbols of the best beam are pinned
                continue
            assert np.array_equal(np.asarray(rec[b])[:keep], ref_rec[b][:keep]), "image %d: prefix of %d differs" % (b, keep)
    record(name, "largest sequence-score difference over the images compared id for id (log-probability units)", worst, MARGIN)
    return worst


def test_beam_search_equals_reference(env, dev):
    z, nat = env["z"], env["nat"]
    assert int((z["margin"] < MARGIN).sum()) * 4 <= len(z["margin"])
    norm, stn_in = nat.prep(env["img"].to(dev))
    feats = nat.encode(nat.rectify(norm, stn_in)[1])
    rec, stored = nat.beam_search(feats, return_stored=True)
    _check_beam("aster_beam_vs_reference", z, rec.numpy(), stored, z["pred_rec"].astype(np.int64), z["symbols"].astype(np.int64),
                z["predecessors"].astype(np.int64), z["scores"])
    from dpmn_amd.utils.labelmaps import AsterInfo, ids_to_strings
    got = nat.read(env["img"].to(dev))
    for b in range(len(got)):
        if z["margin"][b] >= MARGIN:
            assert got[b] == str(z["strings"][b])
    assert got == ids_to_strings(rec.numpy(), AsterInfo('all'))


def test_beam_search_equals_mirror_on_gpu(env, dev):
    z, nat, mir = env["z"], env["nat"], env["mir"]
    feats = mir.stages(env["img"].to(dev))["encoder"]
    m_rec, m_st = mir.decoder.beam_search(feats, 5, 94, return_stored=True)
    rec, stored = nat.beam_search(feats, return_stored=True)
    _check_beam("aster_beam_vs_mirror", z, rec.numpy(), stored, m_rec.numpy(), m_st["symbols"], m_st["predecessors"], m_st["scores"])


def test_batch_independence(env, dev):
    """image i alone, in a batch of 5 and in a batch of 48 decodes to identical ids"""
    nat = env["nat"]
    pool = aster_synth.aster_images(aster_synth.POOL).to(dev)
    big = torch.cat([pool, pool.flip(0)[:16]], 0)
    assert big.shape[0] == 48
    r48 = nat.pred_rec(big)
    r5 = nat.pred_rec(big[7:12])
    for i in (7, 9, 11):
        r1 = nat.pred_rec(big[i:i + 1])
        assert torch.equal(r1[0], r48[i]) and torch.equal(r5[i - 7], r48[i]), "image %d depends on its batch" % i
    assert torch.equal(r48[16:32], r48[32:].flip(0)), "equal images in one batch decode differently"


def test_forward_dict_and_eval_guard(env, dev):
    nat = env["nat"]
    img = env["img"][:2].to(dev)
    out = nat({'images': img * 2 - 1, 'rec_targets': torch.IntTensor(2, 100).fill_(1), 'rec_lengths': [100, 100]})
    rec = out['output']['pred_rec']
    assert rec.shape == (2, 100) and rec.dtype == torch.int64 and torch.equal(out['output']['pred_rec_score'], torch.ones_like(rec))
    assert torch.equal(rec.cpu(), nat.pred_rec(img))
    from dpmn_amd.model.aster import NativeASTER
    m = NativeASTER().to(dev)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.read(img)
