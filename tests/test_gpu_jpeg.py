"""JPEG artefacts on the GPU (csrc/jpeg.hip through ops.jpeg_roundtrip_u8) against PIL's recorded bytes (tests/golden/jpeg_roundtrip.npz)
and the NumPy restatement utils.jpeg.jpeg_roundtrip_u8, byte for byte; per-image tables, the per-image skip and in-place operation in
one batch; run-to-run determinism; and the loader on top of it (degrade_on_gpu, sr_batches) with the flag off, on and at prob 0."""
import os
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import jpeg as jp
from dpmn_amd.utils.degrade import draw_params
from dpmn_amd.utils.resize import pack_ragged
from test_jpeg import SIZES, fixture_cases, make_input

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _by_size():
    """{(h, w): (inputs (n, h, w, 3), qualities (n,), PIL's bytes (n, h, w, 3), the restatement's bytes)}: made once, never changed."""
    if not _REF:
        for (h, w) in SIZES:
            rows = [r for r in fixture_cases() if (r[1], r[2]) == (h, w)]
            _REF[h, w] = (np.stack([r[4] for r in rows]), np.array([r[3] for r in rows], np.int32), np.stack([r[5] for r in rows]),
                          np.stack([jp.jpeg_roundtrip_u8(r[4], r[3]) for r in rows]))
    return _REF


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_fixture_case_is_pils_bytes(dev, size):
    from dpmn_amd import ops
    imgs, q, pil, ref = _by_size()[size]
    assert imgs.shape[0] == 36
    got = ops.jpeg_roundtrip_u8(torch.from_numpy(imgs).to(dev), q).cpu().numpy()
    for name, want in (("the restatement", ref), ("PIL", pil)):
        bad = [(i, int(q[i]), int((got[i] != want[i]).sum())) for i in range(len(q)) if not np.array_equal(got[i], want[i])]
        assert not bad, "%d x %d: (case, quality, differing bytes) against %s: %s" % (size + (name, bad))


def test_batch_with_per_image_tables_skip_and_in_place(dev):
    from dpmn_amd import ops
    q = [0, 1, 40, 95, 100]
    imgs = np.stack([make_input(k, 16, 64) for k in ("noise", "glyph", "glyph", "noise", "step")])
    want = np.stack([jp.jpeg_roundtrip_u8(im, v) for im, v in zip(imgs, q)])
    assert np.array_equal(want[0], imgs[0]) and not np.array_equal(want[1], want[2])
    x = torch.from_numpy(imgs).to(dev)
    out = ops.jpeg_roundtrip_u8(x, q)
    assert out.data_ptr() != x.data_ptr() and np.array_equal(x.cpu().numpy(), imgs), "a new tensor; the input is not written"
    assert np.array_equal(out.cpu().numpy(), want)
    back = ops.jpeg_roundtrip_u8(x, torch.tensor(q, dtype=torch.int32, device=dev), out=x)      # in place, qualities on the device
    assert back is x and np.array_equal(x.cpu().numpy(), want)


def test_odd_batch_with_mixed_qualities(dev):
    from dpmn_amd import ops
    q = [24, 0, 75]
    imgs = np.stack([make_input(k, 17, 33) for k in ("glyph", "noise", "noise")])
    want = np.stack([jp.jpeg_roundtrip_u8(im, v) for im, v in zip(imgs, q)])
    assert np.array_equal(ops.jpeg_roundtrip_u8(torch.from_numpy(imgs).to(dev), np.array(q)).cpu().numpy(), want)


def test_same_call_twice_gives_the_same_bytes(dev):
    from dpmn_amd import ops
    imgs, q, _, _ = _by_size()[(15, 130)]
    x = torch.from_numpy(imgs).to(dev)
    assert torch.equal(ops.jpeg_roundtrip_u8(x, q), ops.jpeg_roundtrip_u8(x, q))


def test_cpu_tensors_and_bad_arguments_are_rejected(dev):
    from dpmn_amd import _abi, ops
    cpu = torch.from_numpy(make_input("noise", 16, 16))[None]
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.jpeg_roundtrip_u8(cpu, [50])
    x = cpu.to(dev)
    for bad in ([101], [-1], [50, 50], [50.0], []):
        with pytest.raises(_abi.DpmnError):
            ops.jpeg_roundtrip_u8(x, bad)
    with pytest.raises(_abi.DpmnError):
        ops.jpeg_roundtrip_u8(x.float(), [50])
    with pytest.raises(_abi.DpmnError):
        ops.jpeg_roundtrip_u8(x.expand(2, 16, 16, 3), [50, 50])                 # not contiguous
    with pytest.raises(_abi.DpmnError):
        ops.jpeg_roundtrip_u8(torch.zeros(1, 1, 1025, 3, dtype=torch.uint8, device=dev), [50])
    with pytest.raises(_abi.DpmnError):
        ops.jpeg_roundtrip_u8(x, [50], out=cpu.clone())


# ---------------------------------------------------------------------------------------------------------------- the loader
LR_H, LR_W, SCALE = 16, 64, 2


def _hr_pair():
    rng = np.random.RandomState(31)
    images = []
    for h, w in ((40, 150), (23, 77), (12, 40)):
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        a[:, w // 2:] //= 3
        images.append(a)
    return pack_ragged(images, pin=False)


def _degrade(dev, jpeg, seed=5):
    from dpmn_amd.dataset import textzoom as tz
    rng = random.Random(seed)
    hr, lr = tz.degrade_on_gpu(_hr_pair(), (LR_H * SCALE, LR_W * SCALE), SCALE, True, dev, rng=rng, jpeg=jpeg)
    return hr, lr, rng


def _plain_lr_bytes(dev, seed=5):
    """The resized LR bytes of the flag-off path, replayed by hand from the same stream."""
    from dpmn_amd import ops
    packed, meta = _hr_pair()
    rng = random.Random(seed)
    params = draw_params(meta.shape[0], cutblur=False, hr_widths=[int(w) for w in meta[:, 2]], rng=rng)
    noise_seed = rng.getrandbits(63)
    packed = packed.to(dev)
    return ops.resize_ragged_u8(ops.degrade_ragged_u8(packed, meta, params, seed=noise_seed), meta, LR_H, LR_W), rng


def test_loader_flag_off_makes_no_draw(dev):
    from dpmn_amd import ops
    hr, lr, rng = _degrade(dev, None)
    lr_u8, ref_rng = _plain_lr_bytes(dev)
    assert rng.getstate() == ref_rng.getstate(), "jpeg=None: draw_params and the 63-bit noise seed, nothing more"
    assert torch.equal(lr, ops.collate_u8(lr_u8, True)) and hr.shape == (3, 4, 32, 128) and lr.shape == (3, 4, 16, 64)


def test_loader_flag_on_is_the_restatement_on_the_lr_bytes(dev):
    from dpmn_amd import ops
    hr0, lr0, _ = _degrade(dev, None)
    hr, lr, rng = _degrade(dev, (40, 40, 1.0))
    lr_u8, ref_rng = _plain_lr_bytes(dev)
    want = np.stack([jp.jpeg_roundtrip_u8(im, 40) for im in lr_u8.cpu().numpy()])
    assert torch.equal(lr, ops.collate_u8(torch.from_numpy(want).to(dev), True))
    assert torch.equal(hr, hr0) and not torch.equal(lr, lr0)
    assert jp.draw_jpeg(3, 40, 40, 1.0, rng=ref_rng).tolist() == [40, 40, 40] and rng.getstate() == ref_rng.getstate()


def test_loader_prob_zero_leaves_the_images_alone(dev):
    hr0, lr0, _ = _degrade(dev, None)
    hr, lr, _ = _degrade(dev, (30, 95, 0.0))
    assert torch.equal(hr, hr0) and torch.equal(lr, lr0)


def test_sr_batches_repeats_under_the_same_seed(dev, tmp_path):
    from PIL import Image
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.folder import FolderHR
    rng = np.random.RandomState(21)
    d = str(tmp_path / "hr")
    os.makedirs(d)
    for i in range(4):
        Image.fromarray(rng.randint(0, 256, (12 + 5 * i, 40 + 9 * i, 3)).astype(np.uint8)).save(os.path.join(d, "crop%d.png" % i))
    ds = FolderHR(d, voc_type="all")

    def passes(jpeg):
        col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=True, gpu_finish=True, gpu_resize=True,
                                           degrade=True, jpeg=jpeg)
        batches = [col([ds[0], ds[1]]), col([ds[2], ds[3]])]
        loader = type("Loader", (), {"collate_fn": col, "__iter__": lambda self: iter(batches)})()
        random.seed(3)
        return list(tz.sr_batches(loader, dev))

    a, b, off = passes((30, 95, 1.0)), passes((30, 95, 1.0)), passes(None)
    for x, y, z in zip(a, b, off):
        assert torch.equal(x[1], y[1]) and torch.equal(x[0], y[0])
        assert torch.equal(x[0], z[0]) and not torch.equal(x[1], z[1]), "the HR batch is untouched, the LR batch is not"
