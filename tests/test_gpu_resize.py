"""The ragged-batch bicubic resize on the GPU (csrc/resize.hip through ops.resize_ragged_u8) against PIL itself, the TextZoom loader's
gpu_resize path against the fixture of the imported reference classes (tests/golden/collate.npz), ops.quantize_sr_u8 against
display.quantize_sr, and the folder path on top of them: TextSR.demo and main.py --demo_dir."""
import csv
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import display, resize
from helpers import load_golden, record
from test_dataset import _fake_env
from test_resize import PAIRS, images, pil_resize

pytestmark = pytest.mark.gpu

OUT_SIZES = [(16, 64), (32, 128)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


@pytest.fixture(scope="module")
def ragged():
    """All twelve input sizes of test_resize.PAIRS at once, random and 0 / 255 content: {kind: (images, {out size: PIL's resizes})}."""
    out = {}
    for kind in (0, 1):
        imgs = [images(src, 40 + i)[kind] for i, (src, _) in enumerate(PAIRS)]
        out[kind] = (imgs, {hw: [pil_resize(a, *hw) for a in imgs] for hw in OUT_SIZES})
    return out


@pytest.mark.parametrize("kind", [0, 1], ids=["random", "binary"])
def test_ragged_batch_equals_pil(dev, ragged, kind):
    from dpmn_amd import ops
    imgs, refs = ragged[kind]
    packed, meta = resize.pack_ragged(imgs)
    assert packed.is_pinned()
    packed = packed.to(dev)
    for H, W in OUT_SIZES:
        first = ops.resize_ragged_u8(packed, meta, H, W)
        again = ops.resize_ragged_u8(packed, meta.numpy(), H, W)      # warm table caches; the meta as a numpy array
        assert first.is_cuda and first.dtype == torch.uint8 and tuple(first.shape) == (len(imgs), H, W, 3)
        got = first.cpu().numpy()
        for i, ref in enumerate(refs[(H, W)]):
            assert int((got[i] != ref).sum()) == 0, "image %d (%s -> %d x %d) differs from PIL" % (i, imgs[i].shape[:2], H, W)
        assert torch.equal(first, again)


def test_single_image_batch_and_rejections(dev, ragged):
    from dpmn_amd import _abi, ops
    img = ragged[0][0][2]
    packed, meta = resize.pack_ragged([img])
    got = ops.resize_ragged_u8(packed.to(dev), meta, 32, 128).cpu().numpy()
    assert got.shape == (1, 32, 128, 3) and np.array_equal(got[0], ragged[0][1][(32, 128)][2])
    with pytest.raises(ValueError):
        resize.pack_ragged([])
    with pytest.raises(_abi.DpmnError):
        ops.resize_ragged_u8(packed, meta, 32, 128)                         # a CPU tensor
    with pytest.raises(_abi.DpmnError):
        ops.resize_ragged_u8(packed.to(dev), meta[:0], 32, 128)             # no image
    with pytest.raises(_abi.DpmnError):
        ops.resize_ragged_u8(packed.to(dev)[:-1], meta, 32, 128)            # the meta points past the buffer
    with pytest.raises(_abi.DpmnError):
        ops.quantize_sr_u8(torch.zeros(1, 3, 4, 4))


def test_resize_windows_and_display_share_one_pass(dev):
    """One resample pass serves three ops: each image, random and 0 / 255 (overshoot clipped in both passes), -> 16 x 64 through
    ops.resize_ragged_u8, ops.resize_windows_u8 (line_width == 64: one window per image) and rows [0, 16) of ops.display_triple on
    (u8 + 0.25) / 255, which quantize_lr maps back to u8.  16 x 64 goes through the identity tables.  Every result equals
    utils.resize.pil_resize_u8, byte for byte."""
    from dpmn_amd import ops
    from dpmn_amd.utils.tile import line_width
    H, W = 16, 64
    shapes = [(9, 30), (3, 5), (16, 64)]
    assert [line_width(h, w, H, W) for h, w in shapes] == [W] * 3
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(display.quantize_lr((k.astype(np.float32) + np.float32(0.25)) / np.float32(255)), k)
    differing = 0
    for kind in (0, 1):
        imgs = [images(s, 70 + i)[kind] for i, s in enumerate(shapes)]
        refs = np.stack([resize.pil_resize_u8(a, H, W) for a in imgs])
        packed, meta = resize.pack_ragged(imgs)
        packed = packed.to(dev)
        ragged = ops.resize_ragged_u8(packed, meta, H, W).cpu().numpy()
        windows, plan = ops.resize_windows_u8(packed, meta, H, W)
        assert plan == [(b, 0) for b in range(len(imgs))]
        zeros = torch.zeros(1, 3, H, W, device=dev)
        triple = np.stack([ops.display_triple(((torch.from_numpy(a).to(dev).float() + 0.25) / 255).permute(2, 0, 1)[None], zeros, zeros,
                                              [0])[0, :H].cpu().numpy() for a in imgs])
        for got in (ragged, windows.cpu().numpy(), triple):
            assert got.shape == refs.shape and got.dtype == np.uint8
            differing += int((got != refs).sum())
    assert record("resize", "one pass: bytes differing from pil_resize_u8 (ragged, windows, display; 3 images x 2 kinds)", differing, 0) == 0


@pytest.mark.parametrize("mask", [True, False])
def test_gpu_resize_collate_equals_reference_fixture(dev, mask):
    """test_gpu_dataset.test_gpu_collate_equals_reference_fixture with the resize on the GPU too: the fixture holds the outputs of the
    imported reference classes."""
    from dpmn_amd.dataset import textzoom as tz
    g = load_golden("collate")
    env, _, _ = _fake_env()
    ds = tz.lmdbDataset_real(env=env, voc_type='all')
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=mask, gpu_finish=True, gpu_resize=True)
    out = col([ds[i] for i in range(5)])
    assert len(out) == 9 and out[0][0].dtype == torch.uint8 and out[0][0].dim() == 1 and tuple(out[2][1].shape) == (5, 3)
    (hr, lr, lv, strs), = list(tz.sr_batches([out], dev, mask, size=(32, 128, 2)))
    tag = "mask" if mask else "nomask"
    assert hr.is_cuda and hr.shape == ((5, 4, 32, 128) if mask else (5, 3, 32, 128))
    assert torch.equal(hr.cpu(), torch.from_numpy(g["hr_" + tag])), "HR batch differs from the reference collate"
    assert torch.equal(lr.cpu(), torch.from_numpy(g["lr_" + tag])), "LR batch differs from the reference collate"
    assert strs == [str(s) for s in g["label_strs"]] and lv is None
    assert torch.equal(out[6], torch.from_numpy(g["label_vecs"]))


def test_quantize_sr_u8_equals_the_host_formula(dev):
    from dpmn_amd import ops
    g = load_golden("display")
    vals = np.concatenate([g["edge_sr"].reshape(-1), np.array([-3, -1e-9, 1.5, 300, np.nan, np.inf, -np.inf], np.float32)]).astype(np.float32)
    B, h, w = 2, 8, 33
    x = np.full(B * 3 * h * w, 0.5, np.float32)
    x[:vals.size] = vals
    x = x.reshape(B, 3, h, w)
    ref = display.quantize_sr(x).transpose(0, 2, 3, 1)
    four = torch.full((B, 4, h, w), 7.0, device=dev)
    four[:, :3] = torch.from_numpy(x).to(dev)
    eight = torch.full((B, 8, h, w), 7.0, device=dev)
    eight[:, ::2][:, :3] = torch.from_numpy(x).to(dev)
    for t in (four, four[:, :3], eight[:, ::2], four[:1]):
        got = ops.quantize_sr_u8(t)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (t.shape[0], h, w, 3)
        assert np.array_equal(got.cpu().numpy(), ref[:t.shape[0]])


def _write_folder(d, n=5):
    rng = np.random.RandomState(9)
    names = []
    for i in range(n):
        a = rng.randint(0, 256, (14 + 9 * i, 50 + 31 * i, 3)).astype(np.uint8)
        names.append("im%d.png" % i)
        Image.fromarray(a).save(os.path.join(d, names[-1]))
    return names


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def test_demo_writes_one_sr_image_per_file(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import folder_batches
    src, out_dir = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    names = _write_folder(str(src))
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    batches = lambda: folder_batches(str(src), 2, (16, 64), True, dev)
    reader_calls = []

    def reader(x):
        reader_calls.append(tuple(x.shape))
        return ["ab"] * x.shape[0]
    rows = sr.demo(models, psn, batches(), str(out_dir), rec=reader, text_prior_fn=fn)
    assert rows == [[n, "ab", "ab"] for n in names]
    assert reader_calls == [(2, 3, 16, 64), (2, 3, 32, 128)] * 2 + [(1, 3, 16, 64), (1, 3, 32, 128)]
    assert sorted(os.listdir(out_dir)) == sorted(["demo_result.csv"] + [n[:-4] + "_sr.png" for n in names])
    with open(out_dir / "demo_result.csv", newline="") as f:
        assert list(csv.reader(f)) == [["file", "lr_string", "sr_string"]] + rows
    seen = []
    for bnames, images_lr in batches():
        assert images_lr.is_cuda and tuple(images_lr.shape) == (len(bnames), 4, 16, 64)
        x = torch.cat([images_lr, images_lr], 0) if len(bnames) == 1 else images_lr      # the padded single-image batch
        out = sr.refine(models, psn, x, None, fn)[:len(bnames)]
        expected = display.quantize_sr(out[:, :3].cpu().numpy()).transpose(0, 2, 3, 1)
        for name, e in zip(bnames, expected):
            got = _png(out_dir / (name[:-4] + "_sr.png"))
            assert got.shape == (32, 128, 3) and np.array_equal(got, e), name
            assert got.min() != got.max()
            seen.append(name)
    assert seen == names
    # without a recogniser the string columns are empty
    rows = sr.demo(models, psn, batches(), str(tmp_path / "out2"), text_prior_fn=fn)
    assert rows == [[n, "", ""] for n in names]


def test_demo_keeps_colliding_stems_apart(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import folder_batches
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.RandomState(2)
    for name, shape in (("a.png", (20, 70, 3)), ("a.bmp", (11, 90, 3))):
        Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8)).save(src / name)
    sr, models, psn = stack
    rows = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), str(tmp_path / "out"), text_prior_fn=sr.synthetic_text_prior())
    assert [r[0] for r in rows] == ["a.bmp", "a.png"]
    assert sorted(os.listdir(tmp_path / "out")) == ["a.png_sr.png", "a_sr.png", "demo_result.csv"]
    assert not np.array_equal(_png(tmp_path / "out" / "a_sr.png"), _png(tmp_path / "out" / "a.png_sr.png"))


def test_main_demo_dir_loads_the_checkpoints(dev, stack, tmp_path):
    """main.py --demo_dir DIR --resume CKPT [--demo_out OUT]: build_models(testing=True) on checkpoints written here, then demo."""
    import main as cli
    from dpmn_amd import workload
    from dpmn_amd.dataset.folder import folder_batches
    from test_gpu_display_eval import _checkpoints
    src = tmp_path / "in"
    src.mkdir()
    names = _write_folder(str(src), 3)
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    args = workload.make_args("tsrn", 1, 1, 2)
    args.resume, args.demo_dir, args.vis_dir, args.synthetic_steps = d, str(src), os.path.join(d, "vis"), 0
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "out"))})
    cli.main(config, args)
    out_dir = os.path.join(d, "vis", "demo")      # the default of --demo_out
    assert sorted(os.listdir(out_dir)) == sorted(["demo_result.csv"] + [n[:-4] + "_sr.png" for n in names])
    (bnames, images_lr), _ = list(folder_batches(str(src), 2, (16, 64), True, dev))
    expected = display.quantize_sr(sr.refine(models, psn, images_lr, None, sr.synthetic_text_prior())[:, :3].cpu().numpy())
    for name, e in zip(bnames, expected.transpose(0, 2, 3, 1)):
        assert np.array_equal(_png(os.path.join(out_dir, name[:-4] + "_sr.png")), e), name
    args.demo_out, args.resume = os.path.join(d, "elsewhere"), None
    with pytest.raises(SystemExit):
        cli.main(config, args)
    args.resume = d
    cli.main(config, args)
    assert len(os.listdir(args.demo_out)) == 4
