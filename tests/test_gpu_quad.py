"""csrc/quad.hip against the numpy restatement of dpmn_amd/utils/quad.py, byte for byte: ops.quad_crop_u8 (a ragged batch of photos and
a list of quadrilaterals -> the rectified regions in pack_ragged's layout), its output straight into the ragged resize and the window
cutter, and the box path on top of it: dataset.folder.box_region_batches / box_window_batches, TextSR.demo(boxes=True) and
main.py --demo_boxes."""
import csv
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import quad, resize, tile
from test_quad import CASES, photos

pytestmark = pytest.mark.gpu

# three photos (1 x 1, 7 x 31, 40 x 89) and nine regions (photo, quad, (h, w) or None for quad_size's) in one call: offsets, tiles and
# the photo index all matter -- one pixel, a slanted word, a 1 x 70 row and a 9 x 1 column, 16 x 64, one past the 8 x 32 tile in both
# directions, exactly one tile, a region half outside its photo and one wholly outside (all black)
_Q = {c[0]: c[2] for c in CASES}
REGIONS = [(0, _Q["one_pixel"], (1, 1)), (1, _Q["small_7x31_slanted"], None), (1, _Q["small_7x31_slanted"], (1, 70)),
           (1, _Q["small_7x31_column"], (9, 1)), (2, _Q["foreshortened"], (16, 64)), (2, _Q["past_one_tile_9x33"], (9, 33)),
           (2, _Q["one_tile_8x32"], (8, 32)), (2, _Q["half_outside"], None), (2, _Q["wholly_outside"], (5, 40))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def batch():
    """(photos, regions, the restatement's crops) of REGIONS, computed once."""
    p = photos()
    imgs = [p[0], p[3], p[4]]
    regions = []
    for b, q, hw in REGIONS:
        h, w = hw or quad.quad_size(q)
        regions.append((b, h, w, quad.quad_coeffs(q, w, h)))
    return imgs, regions, quad.quad_crop_np(imgs, regions)


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def _regions_of(flat, meta):
    return [flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in np.asarray(meta).tolist()]


def test_quad_crop_equals_the_restatement(dev, batch):
    from dpmn_amd import ops
    imgs, regions, ref = batch
    packed, meta = resize.pack_ragged(imgs)
    out, rmeta = ops.quad_crop_u8(packed.to(dev), meta, regions)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1
    sizes = [r.size for r in ref]
    assert np.asarray(rmeta).dtype == np.int64
    assert np.asarray(rmeta).tolist() == [[sum(sizes[:i]), r.shape[0], r.shape[1]] for i, r in enumerate(ref)]
    flat = out.cpu().numpy()
    assert flat.size == sum(sizes)
    differ = [int((g != r).sum()) for g, r in zip(_regions_of(flat, rmeta), ref)]
    print("quad_crop_u8: %d of %d bytes differ (per region %s)" % (sum(differ), flat.size, differ))
    assert sum(differ) == 0
    assert int(ref[-1].max()) == 0 and ref[4].min() != ref[4].max()
    again, ameta = ops.quad_crop_u8(packed.to(dev), meta.numpy(), list(reversed(regions)))      # other offsets, the same regions
    assert all(np.array_equal(g, r) for g, r in zip(_regions_of(again.cpu().numpy(), ameta), reversed(ref)))


def test_no_region_and_rejections(dev, batch):
    from dpmn_amd import _abi, ops
    imgs, regions, _ = batch
    packed, meta = resize.pack_ragged(imgs)
    out, rmeta = ops.quad_crop_u8(packed.to(dev), meta, [])
    assert out.is_cuda and out.dtype == torch.uint8 and out.numel() == 0 and np.asarray(rmeta).shape == (0, 3)
    a = regions[1][3]
    for bad in ([(3, 5, 20, a)], [(-1, 5, 20, a)], [(0, 0, 20, a)], [(0, 5, resize.MAX_SIDE + 1, a)], [(0, 5, 20, a[:7])],
                [(0, 5, 20, [np.nan] + list(a[1:]))], [(0, 5, 20)]):
        with pytest.raises(_abi.DpmnError):
            ops.quad_crop_u8(packed.to(dev), meta, bad)
    with pytest.raises(_abi.DpmnError):
        ops.quad_crop_u8(packed, meta, regions)                          # a CPU tensor
    with pytest.raises(_abi.DpmnError):
        ops.quad_crop_u8(packed.to(dev)[:-1], meta, regions)             # the meta points past the buffer


def test_a_region_past_the_packed_buffer_is_black_and_reported(dev, batch):
    """Validation of the caller's numbers in the library (the host wrapper would have refused them): a region whose table entry names
    a photo past the packed buffer is not read -- it comes out black, the call returns the library's error code, and every other
    region of the call is computed.  A tile that names no region or lies outside its region writes nothing and is not an error."""
    from dpmn_amd import _abi, ops
    imgs, regions, ref = batch
    packed, meta = resize.pack_ragged(imgs)
    packed = packed.to(dev)
    host = ops._quad_crop_plan(packed, meta, regions)
    good = host["table"].copy()
    host["table"][4, 0] = packed.numel() - 40 * 89 * 3 + 1      # region 4 (16 x 64): its photo ends one byte past the buffer
    out, code = ops._quad_crop_run(packed, host)
    torch.cuda.synchronize()
    assert code == -1
    with pytest.raises(_abi.DpmnError, match="quad_crop"):
        _abi.check(code)
    for r, (g, e) in enumerate(zip(_regions_of(out.cpu().numpy(), host["meta"]), ref)):
        if r == 4:
            assert int(g.max()) == 0 and int(e.max()) > 0, "region 4 is not black"
        else:
            assert np.array_equal(g, e), "region %d changed" % r
    host["table"] = good
    host["tiles"] = host["tiles"].copy()
    first = int(np.nonzero(host["tiles"][:, 0] == 4)[0][0])      # region 4: 2 x 2 tiles
    host["tiles"][first] = len(regions), 0, 0                   # its tile (0, 0) names a region past the table
    host["tiles"][first + 3] = 4, 1, 2                          # its tile (1, 1) a column past the region
    out, code = ops._quad_crop_run(packed, host)
    torch.cuda.synchronize()
    assert code == 0
    got = _regions_of(out.cpu().numpy(), host["meta"])
    expected = ref[4].copy()
    expected[:8, :32] = 0
    expected[8:, 32:] = 0
    assert np.array_equal(got[4], expected)
    assert all(np.array_equal(g, e) for r, (g, e) in enumerate(zip(got, ref)) if r != 4)


def test_the_regions_go_straight_into_the_resize_and_the_window_cut(dev, batch):
    from dpmn_amd import ops
    imgs, regions, ref = batch
    packed, meta = resize.pack_ragged(imgs)
    crops, cmeta = ops.quad_crop_u8(packed.to(dev), meta, regions)
    lr = ops.resize_ragged_u8(crops, cmeta, 16, 64).cpu().numpy()
    expected = np.stack([resize.pil_resize_u8(r, 16, 64) for r in ref])
    print("quad_crop_u8 -> resize_ragged_u8: %d of %d bytes differ" % (int((lr != expected).sum()), lr.size))
    assert lr.shape == expected.shape and int((lr != expected).sum()) == 0
    windows, plan = ops.resize_windows_u8(crops, cmeta, 16, 64)
    ref_windows, ref_plan = tile.resize_windows_np(ref, (16, 64))
    assert plan == ref_plan and len(plan) > len(ref)
    windows = windows.cpu().numpy()
    print("quad_crop_u8 -> resize_windows_u8: %d of %d bytes differ" % (int((windows != ref_windows).sum()), windows.size))
    assert windows.shape == ref_windows.shape and int((windows != ref_windows).sum()) == 0


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _reader(calls):
    def reader(x):
        calls.append(tuple(x.shape))
        return ["ab"] * x.shape[0]
    return reader


def _photo_folder(tmp_path, wide=False):
    """Two photos with three boxes and one ### line (wide: a third photo with a 12 x 200 region) -> (photo dir, box dir, photos)."""
    src, box = tmp_path / "photos", tmp_path / "boxes"
    src.mkdir()
    box.mkdir()
    rng = np.random.RandomState(21)
    imgs = {"p0": rng.randint(0, 256, (40, 100, 3)).astype(np.uint8), "p1": rng.randint(0, 256, (30, 120, 3)).astype(np.uint8)}
    (box / "p0.txt").write_text("3,5,67,5,67,21,3,21,axis\n10,10,30,10,30,20,10,20,###\n20.5,12,90,6.25,93,30,22,37.5,slant, ed\n")
    (box / "gt_p1.txt").write_text("4,3,110,8,108,27,2,22\n")
    if wide:
        imgs["p2"] = rng.randint(0, 256, (30, 260, 3)).astype(np.uint8)
        (box / "p2.txt").write_text("10,8,210,8,210,20,10,20,a long line\n")
    for name, a in imgs.items():
        Image.fromarray(a).save(str(src / (name + ".png")))
    return str(src), str(box), imgs


def test_demo_boxes_writes_one_file_per_region(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import box_batches, box_region_batches, folder_batches
    src, box, imgs = _photo_folder(tmp_path)
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    calls = [[], []]
    out_dir = tmp_path / "out"
    rows = sr.demo(models, psn, box_region_batches(src, box, 2, (16, 64), True, dev), str(out_dir), rec=_reader(calls[0]), text_prior_fn=fn,
                   boxes=True)
    names = ["p0_000", "p0_002", "p1_000"]
    assert rows == [["p0", "000", "axis", "ab", "ab"], ["p0", "002", "slant, ed", "ab", "ab"], ["p1", "000", " ", "ab", "ab"]]
    assert sorted(os.listdir(out_dir)) == sorted(["demo_result.csv"] + [n + "_sr.png" for n in names])
    with open(out_dir / "demo_result.csv", newline="") as f:
        assert list(csv.reader(f)) == [["file", "box", "label", "lr_string", "sr_string"]] + rows
    for n in names:
        got = _png(out_dir / (n + "_sr.png"))
        assert got.shape == (32, 128, 3) and got.min() != got.max()
    # the same crops saved as files of their own, through the plain demo: the old header and names, and the same bytes -- the
    # axis-aligned integer box is the photo's own pixels, the others are the restatement's
    crops_dir, plain = tmp_path / "crops", tmp_path / "plain"
    crops_dir.mkdir()
    crops = []
    for _, _, packed, meta, regions in box_batches(src, box, 8):
        flat = packed.numpy()
        crops = quad.quad_crop_np([flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in meta.tolist()], regions)
    assert len(crops) == 3 and np.array_equal(crops[0], imgs["p0"][5:21, 3:67])
    for n, c in zip(names, crops):
        Image.fromarray(c).save(str(crops_dir / (n + ".png")))
    rows_plain = sr.demo(models, psn, folder_batches(str(crops_dir), 2, (16, 64), True, dev), str(plain), rec=_reader(calls[1]), text_prior_fn=fn)
    assert rows_plain == [[n + ".png", "ab", "ab"] for n in names] and calls[0] == calls[1]
    assert sorted(os.listdir(plain)) == sorted(os.listdir(out_dir))
    with open(plain / "demo_result.csv", newline="") as f:
        assert list(csv.reader(f)) == [["file", "lr_string", "sr_string"]] + rows_plain
    for n in names:
        assert (plain / (n + "_sr.png")).read_bytes() == (out_dir / (n + "_sr.png")).read_bytes(), n


def test_demo_boxes_runs_a_photo_of_many_regions_in_chunks(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import box_region_batches
    src, box, _ = _photo_folder(tmp_path)
    sr, models, psn = stack
    calls = []
    # one batch of 3 regions (a photo is never split), chunks of the stack's batch size 2: 2 and 1 (the one is repeated)
    rows = sr.demo(models, psn, box_region_batches(src, box, 3, (16, 64), True, dev), str(tmp_path / "out"), rec=_reader(calls),
                   text_prior_fn=sr.synthetic_text_prior(), boxes=True)
    assert [r[:2] for r in rows] == [["p0", "000"], ["p0", "002"], ["p1", "000"]]
    assert calls == [(2, 3, 16, 64), (2, 3, 32, 128), (1, 3, 16, 64), (1, 3, 32, 128)]


def test_demo_boxes_tile_keeps_the_aspect_of_a_long_region(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import box_window_batches
    src, box, _ = _photo_folder(tmp_path, wide=True)
    sr, models, psn = stack
    out_dir = tmp_path / "out"
    rows = sr.demo(models, psn, box_window_batches(src, box, 2, (16, 64), True, dev), str(out_dir), rec=_reader([]),
                   text_prior_fn=sr.synthetic_text_prior(), tile=True, boxes=True, chunk=4)
    w_line = tile.line_width(12, 200)
    assert w_line == 267
    assert [r[:3] for r in rows] == [["p0", "000", "axis"], ["p0", "002", "slant, ed"], ["p1", "000", " "], ["p2", "000", "a long line"]]
    assert rows[3][3] == "|".join(["ab"] * len(tile.window_plan(w_line)))
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_002_sr.png", "p1_000_sr.png", "p2_000_sr.png"]
    got = _png(out_dir / "p2_000_sr.png")
    assert got.shape == (32, 2 * w_line, 3) and got.min() != got.max()
    assert _png(out_dir / "p0_000_sr.png").shape == (32, 128, 3)


def test_main_demo_boxes_writes_the_regions(dev, stack, tmp_path):
    """main.py --demo_dir DIR --demo_boxes BOXDIR --resume CKPT: the box loader and demo(boxes=True) behind the flag."""
    import main as cli
    from dpmn_amd import workload
    from test_gpu_display_eval import _checkpoints
    src, box, _ = _photo_folder(tmp_path)
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    args = workload.make_args("tsrn", 1, 1, 2)
    args.resume, args.demo_dir, args.demo_boxes, args.demo_out, args.synthetic_steps = d, src, box, os.path.join(d, "regions"), 0
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "out"))})
    cli.main(config, args)
    assert sorted(os.listdir(args.demo_out)) == ["demo_result.csv", "p0_000_sr.png", "p0_002_sr.png", "p1_000_sr.png"]
    assert _png(os.path.join(args.demo_out, "p1_000_sr.png")).shape == (32, 128, 3)
    with open(os.path.join(args.demo_out, "demo_result.csv"), newline="") as f:
        assert next(csv.reader(f)) == ["file", "box", "label", "lr_string", "sr_string"]
