"""csrc/tile.hip against the numpy restatement of dpmn_amd/utils/tile.py, byte for byte: ops.resize_windows_u8 (a ragged batch ->
overlapping LR windows), ops.stitch_windows_u8 (SR windows -> one image per input), and the folder path on top of them:
dataset.folder.folder_window_batches and TextSR.demo(tile=True)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import display, resize, tile
from test_tile import SIZES, _plan_of, line_images

pytestmark = pytest.mark.gpu

KINDS = ["random", "zeros", "ones"]


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
def lines():
    """The five sizes of test_tile.SIZES as one ragged batch per kind: {kind: (images, windows, plan)} of resize_windows_np."""
    out = {}
    for k, kind in enumerate(KINDS):
        imgs = line_images(kind=k)
        out[kind] = (imgs,) + tile.resize_windows_np(imgs, (16, 64))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_resize_windows_equals_the_restatement(dev, lines, kind):
    from dpmn_amd import ops
    imgs, ref, ref_plan = lines[kind]
    packed, meta = resize.pack_ragged(imgs)
    got, plan = ops.resize_windows_u8(packed.to(dev), meta, 16, 64)
    assert plan == ref_plan
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
    diff = (got.cpu().numpy() != ref)
    print("resize_windows_u8 [%s]: %d of %d bytes differ" % (kind, int(diff.sum()), diff.size))
    assert int(diff.sum()) == 0
    again, _ = ops.resize_windows_u8(packed.to(dev), meta.numpy(), 16, 64)
    assert torch.equal(got, again)


def test_resize_windows_single_image_and_rejections(dev, lines):
    from dpmn_amd import _abi, ops
    imgs, ref, ref_plan = lines["random"]
    first = [t for t, (b, _) in enumerate(ref_plan) if b == 3]
    packed, meta = resize.pack_ragged([imgs[3]])
    got, plan = ops.resize_windows_u8(packed.to(dev), meta, 16, 64)
    assert plan == [(0, x0) for b, x0 in ref_plan if b == 3] and np.array_equal(got.cpu().numpy(), ref[first])
    # one window: the image of the plain resize
    one, plan = ops.resize_windows_u8(packed.to(dev)[:33 * 70 * 3], [[0, 33, 70]], 16, 64)
    assert plan == [(0, 0)] and torch.equal(one, ops.resize_ragged_u8(packed.to(dev), [[0, 33, 70]], 16, 64))
    with pytest.raises(_abi.DpmnError):
        ops.resize_windows_u8(packed, meta, 16, 64)                          # a CPU tensor
    with pytest.raises(_abi.DpmnError):
        ops.resize_windows_u8(packed.to(dev), meta[:0], 16, 64)              # no image
    with pytest.raises(_abi.DpmnError):
        ops.resize_windows_u8(packed.to(dev)[:-1], meta, 16, 64)             # the meta points past the buffer
    with pytest.raises(_abi.DpmnError):
        ops.resize_windows_u8(packed.to(dev), [[0, 1, 600]], 16, 64)         # a line wider than MAX_SIDE
    with pytest.raises(_abi.DpmnError):
        ops.stitch_windows_u8(torch.zeros(1, 3, 32, 128), [(0, 0)])
    with pytest.raises(_abi.DpmnError):
        ops.stitch_windows_u8(torch.zeros(2, 3, 32, 128, device=dev), [(0, 0), (0, 7), (0, 9)])      # 2 windows, a plan of 3
    with pytest.raises(_abi.DpmnError):
        ops.stitch_windows_u8(torch.zeros(3, 3, 32, 128, device=dev), [(0, 0), (0, 7), (0, 3)])                     # a start that decreases


def test_corrupted_items_give_black_windows_and_are_not_read(dev, lines):
    """Validation of the caller's numbers in the kernels (the host wrapper would have refused them): an image whose byte offset lies
    past the packed buffer, one whose table lies past the tables, and a window that starts outside its line come out black; every other
    window is untouched and the runtime reports nothing."""
    from dpmn_amd import ops
    imgs, ref, ref_plan = lines["random"]
    packed, meta = resize.pack_ragged(imgs)
    packed = packed.to(dev)
    plan, host = ops._resize_windows_plan(packed, meta, 16, 64)
    host["items"] = host["items"].copy()
    host["windows"] = host["windows"].copy()
    host["items"][2, 0] = packed.numel()                    # image 2 (2 windows): its byte offset is past the packed buffer
    host["items"][0, 6] = host["tables"].size - 3           # image 0 (1 window): its horizontal table ends past the tables
    bad_window = next(t for t, (b, _) in enumerate(plan) if b == 4) + 5
    host["windows"][bad_window, 1] = 1143 - 63              # one window of image 4: one column too far right
    got = ops._resize_windows_run(packed, host)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    black = [t for t, (b, _) in enumerate(plan) if b in (0, 2)] + [bad_window]
    assert len(black) == 4
    for t in range(len(plan)):
        if t in black:
            assert int(got[t].max()) == 0, "window %d is not black" % t
        else:
            assert np.array_equal(got[t], ref[t]), "window %d changed" % t


def test_stitch_equals_the_restatement(dev):
    from dpmn_amd import ops
    rng = np.random.RandomState(8)
    w_lines = [w_line for _, w_line, _ in SIZES] + [65, 113]
    plan = _plan_of(w_lines)
    T = len(plan)
    # random windows that do not agree where they overlap, with values outside [0, 1], infinities and a NaN
    x = (rng.rand(T, 4, 32, 128) * 1.4 - 0.2).astype(np.float32)
    x[1, 0, 0, :6] = [np.nan, np.inf, -np.inf, 300.0, -3.0, 0.5]
    x[3, 2, 31, 120:] = np.nan
    ref = tile.stitch_np(x, plan)
    four = torch.from_numpy(x).to(dev)
    eight = torch.full((T, 8, 32, 128), 7.0, device=dev)
    eight[:, ::2] = four
    for t in (four, four[:, :3], eight[:, ::2]):
        packed, meta = ops.stitch_windows_u8(t, plan)
        assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1
        assert meta.tolist() == [[sum(32 * 2 * w * 3 for w in w_lines[:b]), 32, 2 * w] for b, w in enumerate(w_lines)]
        flat = packed.cpu().numpy()
        assert flat.size == sum(r.size for r in ref)
        differ = sum(int((flat[off:off + h * w * 3].reshape(h, w, 3) != r).sum()) for (off, h, w), r in zip(meta, ref))
        print("stitch_windows_u8: %d of %d bytes differ" % (differ, flat.size))
        assert differ == 0


def test_stitch_of_the_windows_of_one_line_is_the_quantised_line(dev):
    from dpmn_amd import ops
    rng = np.random.RandomState(5)
    w_lines = [w_line for _, w_line, _ in SIZES] + [65, 112, 160]
    plan = _plan_of(w_lines)
    full = [rng.rand(3, 32, 2 * w_line).astype(np.float32) for w_line in w_lines]
    sr = torch.from_numpy(np.stack([full[b][:, :, 2 * x0:2 * x0 + 128] for b, x0 in plan])).to(dev)
    packed, meta = ops.stitch_windows_u8(sr, plan)
    flat = packed.cpu().numpy()
    for (off, h, w), line in zip(meta, full):
        assert (h, w) == line.shape[1:]
        assert int((flat[off:off + h * w * 3].reshape(h, w, 3) != display.quantize_sr(line).transpose(1, 2, 0)).sum()) == 0


def _write(d, shapes, seed=9):
    rng = np.random.RandomState(seed)
    names = []
    for i, hw in enumerate(shapes):
        names.append("im%d.png" % i)
        Image.fromarray(rng.randint(0, 256, hw + (3,)).astype(np.uint8)).save(os.path.join(d, names[-1]))
    return names


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _reader(calls):
    def reader(x):
        calls.append(tuple(x.shape))
        return ["ab"] * x.shape[0]
    return reader


def test_demo_tile_of_narrow_crops_writes_the_files_of_the_plain_demo(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import folder_batches, folder_window_batches
    src = tmp_path / "in"
    src.mkdir()
    names = _write(str(src), [(14, 50), (23, 81), (32, 112), (16, 64), (40, 90)])      # aspect 4 : 1 or less: one window each
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    calls = [[], []]
    rows_plain = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), str(tmp_path / "plain"), rec=_reader(calls[0]),
                         text_prior_fn=fn)
    rows_tile = sr.demo(models, psn, folder_window_batches(str(src), 2, (16, 64), True, dev), str(tmp_path / "tile"), rec=_reader(calls[1]),
                        text_prior_fn=fn, tile=True)
    assert rows_tile == rows_plain == [[n, "ab", "ab"] for n in names] and calls[0] == calls[1]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "tile")) == sorted(["demo_result.csv"] + [n[:-4] + "_sr.png" for n in names])
    for f in files:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "tile" / f).read_bytes(), f


def test_demo_tile_writes_the_stitched_lines(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import folder_window_batches
    src, out_dir = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    names = _write(str(src), [(20, 300), (9, 40)])
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    batches = lambda: folder_window_batches(str(src), 2, (16, 64), True, dev)
    calls = []
    rows = sr.demo(models, psn, batches(), str(out_dir), rec=_reader(calls), text_prior_fn=fn, tile=True, chunk=8)
    # the reads of an image's windows, joined
    assert rows == [[names[0], "|".join(["ab"] * 5), "|".join(["ab"] * 5)], [names[1], "ab|ab", "ab|ab"]]
    assert calls == [(7, 3, 16, 64), (7, 3, 32, 128)]
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "im0_sr.png", "im1_sr.png"]
    (bnames, plan, images_lr), = list(batches())
    assert bnames == names and plan == [(0, x0) for x0 in tile.window_plan(240)] + [(1, 0), (1, 7)]
    assert images_lr.is_cuda and tuple(images_lr.shape) == (7, 4, 16, 64)
    expected = tile.stitch_np(sr.refine(models, psn, images_lr, None, fn).cpu().numpy(), plan)
    for name, e, hw in zip(names, expected, ((32, 480), (32, 142))):
        got = _png(out_dir / (name[:-4] + "_sr.png"))
        assert got.shape == hw + (3,) and e.shape == got.shape
        assert int((got != e).sum()) == 0, name
        assert got.min() != got.max()


def test_demo_tile_runs_a_final_chunk_of_one_window(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import folder_window_batches
    src, out_dir = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    names = _write(str(src), [(20, 300), (9, 40), (16, 64)])      # 5 + 2 windows in the first batch, 1 in the second
    sr, models, psn = stack
    calls = []
    rows = sr.demo(models, psn, folder_window_batches(str(src), 2, (16, 64), True, dev), str(out_dir), rec=_reader(calls),
                   text_prior_fn=sr.synthetic_text_prior(), tile=True)      # chunks of the stack's batch size 2: 2, 2, 2, 1 and 1
    assert [r[0] for r in rows] == names and [r[1].count("|") for r in rows] == [4, 1, 0]
    assert calls == [(2, 3, 16, 64), (2, 3, 32, 128)] * 3 + [(1, 3, 16, 64), (1, 3, 32, 128)] * 2
    for name, hw in zip(names, ((32, 480), (32, 142), (32, 128))):
        got = _png(out_dir / (name[:-4] + "_sr.png"))
        assert got.shape == hw + (3,) and got.min() != got.max()


def test_main_demo_tile_writes_the_lines(dev, stack, tmp_path):
    """main.py --demo_dir DIR --demo_tile --resume CKPT: the tiled loader and demo(tile=True) behind the flag."""
    import main as cli
    from dpmn_amd import workload
    from test_gpu_display_eval import _checkpoints
    src = tmp_path / "in"
    src.mkdir()
    names = _write(str(src), [(20, 300), (16, 64)])
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    args = workload.make_args("tsrn", 1, 1, 2)
    args.resume, args.demo_dir, args.demo_tile, args.demo_out, args.synthetic_steps = d, str(src), True, os.path.join(d, "lines"), 0
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "out"))})
    cli.main(config, args)
    assert sorted(os.listdir(args.demo_out)) == ["demo_result.csv", "im0_sr.png", "im1_sr.png"]
    assert _png(os.path.join(args.demo_out, "im0_sr.png")).shape == (32, 480, 3)
    assert _png(os.path.join(args.demo_out, "im1_sr.png")).shape == (32, 128, 3)
