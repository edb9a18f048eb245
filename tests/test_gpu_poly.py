"""csrc/poly.hip against the numpy restatement of dpmn_amd/utils/poly.py, byte for byte: ops.poly_crop_u8 (a ragged batch of photos and
a list of polygons cut into cells -> the rectified regions in pack_ragged's layout), quadrilaterals and polygons in one buffer
(ops.crop_regions_u8), the output straight into the ragged resize, and the polygon path on top of it:
dataset.folder.box_region_batches / box_window_batches(polygons=True), TextSR.demo(boxes=True) and main.py --demo_polygons."""
import csv
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import poly, quad, resize, tile
from test_poly import ARC_DOWN, arc, case_regions
from test_quad import photos

pytestmark = pytest.mark.gpu

PHOTO_OF = {0: 0, 3: 1, 4: 2}      # test_quad.photos() -> the three photos of the batch: 1 x 1, 7 x 31, 40 x 89


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def batch():
    """(photos, regions, the restatement's crops, names) of test_poly.CASES in one call, computed once."""
    p = photos()
    imgs = [p[0], p[3], p[4]]
    cases = case_regions()
    regions = [(PHOTO_OF[b], h, w, cells) for _, _, (b, h, w, cells), _ in cases]
    return imgs, regions, poly.poly_crop_np(imgs, regions), [c[0] for c in cases]


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def _regions_of(flat, meta):
    return [flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in np.asarray(meta).tolist()]


def test_poly_crop_equals_the_restatement(dev, batch):
    from dpmn_amd import ops
    imgs, regions, ref, names = batch
    packed, meta = resize.pack_ragged(imgs)
    out, rmeta = ops.poly_crop_u8(packed.to(dev), meta, regions)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1
    sizes = [r.size for r in ref]
    assert np.asarray(rmeta).dtype == np.int64
    assert np.asarray(rmeta).tolist() == [[sum(sizes[:i]), r.shape[0], r.shape[1]] for i, r in enumerate(ref)]
    flat = out.cpu().numpy()
    assert flat.size == sum(sizes)
    differ = [int((g != r).sum()) for g, r in zip(_regions_of(flat, rmeta), ref)]
    print("poly_crop_u8: %d of %d bytes differ (per region %s)" % (sum(differ), flat.size, dict(zip(names, differ))))
    assert sum(differ) == 0
    black, curved = ref[names.index("wholly_outside")], ref[names.index("arc_down_k7")]
    assert int(black.max()) == 0 and curved.min() != curved.max()
    again, ameta = ops.poly_crop_u8(packed.to(dev), meta.numpy(), list(reversed(regions)))      # other offsets, the same regions
    differ = [int((g != r).sum()) for g, r in zip(_regions_of(again.cpu().numpy(), ameta), reversed(ref))]
    print("poly_crop_u8, the regions reversed: %d bytes differ" % sum(differ))
    assert sum(differ) == 0 and np.asarray(ameta)[:, 1:].tolist() == [list(r.shape[:2]) for r in reversed(ref)]


def test_no_region_and_rejections(dev, batch):
    from dpmn_amd import _abi, ops
    imgs, regions, _, names = batch
    packed, meta = resize.pack_ragged(imgs)
    out, rmeta = ops.poly_crop_u8(packed.to(dev), meta, [])
    assert out.is_cuda and out.dtype == torch.uint8 and out.numel() == 0 and np.asarray(rmeta).shape == (0, 3)
    _, h, w, cells = regions[names.index("region_9x33")]      # two cells: 0 .. 16 .. 33
    a = cells[0][2]
    for bad in ([(3, h, w, cells)], [(-1, h, w, cells)], [(2, 0, w, cells)], [(2, h, resize.MAX_SIDE + 1, cells)], [(2, h, w)],
                [(2, h, w, [(0, 16, [np.nan] + list(a[1:])), cells[1]])], [(2, h, w, [(0, 16, [np.inf] + list(a[1:])), cells[1]])],
                [(2, h, w, [(0, 16, a[:7]), cells[1]])], [(2, h, w, [])], [(2, h, w, cells[:1])], [(2, h, w, cells[1:])],
                [(2, h, w, [(0, 16, a), (17, 33, a)])], [(2, h, w, [(0, 16, a), (16, 16, a), (16, 33, a)])], [(2, h, w, [cells[1], cells[0]])],
                [(2, h, w + 1, cells)], [(2, 4, 40, [(i, i + 1, a) for i in range(40)])], [(2, h, w, [(0, 16), cells[1]])]):
        with pytest.raises(_abi.DpmnError):
            ops.poly_crop_u8(packed.to(dev), meta, bad)
    with pytest.raises(_abi.DpmnError):
        ops.poly_crop_u8(packed, meta, regions)                          # a CPU tensor
    with pytest.raises(_abi.DpmnError):
        ops.poly_crop_u8(packed.to(dev)[:-1], meta, regions)             # the meta points past the buffer
    ops.poly_crop_u8(packed.to(dev), meta, [(2, 4, 31, [(i, i + 1, a) for i in range(31)])])      # MAX_POLY_SIDE - 1 cells: the most


def test_an_unsound_region_is_black_and_reported(dev, batch):
    """Validation of the caller's numbers in the library (the host wrapper would have refused them): a region whose table entry names
    a photo past the packed buffer, cells past the cell table, or whose cell bounds do not ascend from 0 to its width, is not read --
    it comes out black, the call returns the library's error code, and every other region of the call is computed."""
    from dpmn_amd import _abi, ops
    imgs, regions, ref, names = batch
    packed, meta = resize.pack_ragged(imgs)
    packed = packed.to(dev)
    r = names.index("arc_down_k7")
    plan = ops._poly_crop_plan(packed, meta, regions)
    first, n = (int(v) for v in plan["table"][r, 6:8])
    n_cells = plan["cells"].shape[0]

    def past_the_photo(table, cells):
        table[r, 0] = packed.numel() - 40 * 89 * 3 + 1

    def past_the_cell_table(table, cells):
        table[r, 6] = n_cells - n + 1

    def too_many_cells(table, cells):
        table[r, 7] = 32

    def a_gap(table, cells):
        cells[first + 2, 0] += 1

    def not_from_zero(table, cells):
        cells[first, 0] = 1

    def past_the_width(table, cells):
        cells[first + n - 1, 1] += 1

    for tamper in (past_the_photo, past_the_cell_table, too_many_cells, a_gap, not_from_zero, past_the_width):
        host = dict(plan, table=plan["table"].copy(), cells=plan["cells"].copy())
        tamper(host["table"], host["cells"])
        out, code = ops._poly_crop_run(packed, host)
        torch.cuda.synchronize()
        assert code == -1, tamper.__name__
        with pytest.raises(_abi.DpmnError, match="poly_crop"):
            _abi.check(code)
        for i, (g, e) in enumerate(zip(_regions_of(out.cpu().numpy(), host["meta"]), ref)):
            if i == r:
                assert int(g.max()) == 0 and int(e.max()) > 0, "%s: region %d is not black" % (tamper.__name__, r)
            else:
                assert np.array_equal(g, e), "%s: region %d changed" % (tamper.__name__, i)
    # a tile that names no region or lies outside its region writes nothing and is not an error
    host = dict(plan, tiles=plan["tiles"].copy())
    mine = np.nonzero(host["tiles"][:, 0] == r)[0]      # region r: 14 x 67, 2 x 3 tiles
    assert mine.size == 6
    host["tiles"][mine[0]] = len(regions), 0, 0
    host["tiles"][mine[5]] = r, 1, 3
    out, code = ops._poly_crop_run(packed, host)
    torch.cuda.synchronize()
    assert code == 0
    got = _regions_of(out.cpu().numpy(), host["meta"])
    expected = ref[r].copy()
    expected[:8, :32] = 0
    expected[8:, 64:] = 0
    assert np.array_equal(got[r], expected)
    assert all(np.array_equal(g, e) for i, (g, e) in enumerate(zip(got, ref)) if i != r)


def test_quads_and_polygons_share_one_buffer(dev, batch):
    from dpmn_amd import ops
    from test_quad import CASES as QUADS
    imgs, regions, ref, names = batch
    by_name = {c[0]: c[2] for c in QUADS}
    quads, quad_ref = [], []
    for b, name, hw in ((2, "foreshortened", (16, 64)), (1, "small_7x31_slanted", None), (2, "past_one_tile_9x33", (9, 33))):
        h, w = hw or quad.quad_size(by_name[name])
        quads.append((b, h, w, quad.quad_coeffs(by_name[name], w, h)))
    quad_ref = quad.quad_crop_np(imgs, quads)
    pick = [names.index(n) for n in ("arc_down_k7", "one_column_strip", "half_outside")]
    mixed = [regions[pick[0]], quads[0], quads[1], regions[pick[1]], regions[pick[2]], quads[2]]
    expected = [ref[pick[0]], quad_ref[0], quad_ref[1], ref[pick[1]], ref[pick[2]], quad_ref[2]]
    packed, meta = resize.pack_ragged(imgs)
    out, rmeta = ops.crop_regions_u8(packed.to(dev), meta, mixed)
    sizes = [e.size for e in expected]
    assert np.asarray(rmeta).tolist() == [[sum(sizes[:i]), e.shape[0], e.shape[1]] for i, e in enumerate(expected)]
    assert out.numel() == sum(sizes)
    differ = [int((g != e).sum()) for g, e in zip(_regions_of(out.cpu().numpy(), rmeta), expected)]
    print("crop_regions_u8: %d of %d bytes differ (per region %s)" % (sum(differ), out.numel(), differ))
    assert sum(differ) == 0
    # a list of one kind is that kind's op
    only, ometa = ops.crop_regions_u8(packed.to(dev), meta, quads)
    assert all(np.array_equal(g, e) for g, e in zip(_regions_of(only.cpu().numpy(), ometa), quad_ref))
    only, ometa = ops.crop_regions_u8(packed.to(dev), meta, regions[:3])
    assert all(np.array_equal(g, e) for g, e in zip(_regions_of(only.cpu().numpy(), ometa), ref[:3]))


def test_the_regions_go_straight_into_the_resize(dev, batch):
    from dpmn_amd import ops
    imgs, regions, ref, _ = batch
    packed, meta = resize.pack_ragged(imgs)
    crops, cmeta = ops.poly_crop_u8(packed.to(dev), meta, regions)
    lr = ops.resize_ragged_u8(crops, cmeta, 16, 64).cpu().numpy()
    expected = np.stack([resize.pil_resize_u8(r, 16, 64) for r in ref])
    print("poly_crop_u8 -> resize_ragged_u8: %d of %d bytes differ" % (int((lr != expected).sum()), lr.size))
    assert lr.shape == expected.shape and int((lr != expected).sum()) == 0


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _line(points, label=None):
    return ",".join("%g" % v for v in np.asarray(points).reshape(-1)) + ("" if label is None else "," + label) + "\n"


QUAD_LINE = "3,5,67,5,67,21,3,21,axis\n"
CURVE = np.round(ARC_DOWN, 2)                           # 14 points in a 40 x 100 photo
LONG_ARC = np.round(arc(130, 400, 380, 368, 0.27, 7), 2)      # about 202 x 12 in a 60 x 260 photo


def _photo_folder(tmp_path, name, first_lines, wide=False):
    """One photo p0 whose box file holds `first_lines`, a ### line and a malformed line (wide: a photo p1 with a long arc) ->
    (photo dir, box dir, photos)."""
    src, box = tmp_path / (name + "_photos"), tmp_path / (name + "_boxes")
    src.mkdir()
    box.mkdir()
    rng = np.random.RandomState(33)
    imgs = {"p0": rng.randint(0, 256, (40, 100, 3)).astype(np.uint8)}
    (box / "p0.txt").write_text(first_lines + "10,10,30,10,30,20,10,20,###\n1,2,3\n")
    if wide:
        imgs["p1"] = rng.randint(0, 256, (60, 260, 3)).astype(np.uint8)
        (box / "p1.txt").write_text(_line(LONG_ARC, "####a long arc"))
    for stem, a in imgs.items():
        Image.fromarray(a).save(str(src / (stem + ".png")))
    return str(src), str(box), imgs


def _reader(seen):
    def reader(x):
        seen.append(x.detach().clone())
        return ["ab"] * x.shape[0]
    return reader


def test_demo_polygons_writes_one_file_per_region(dev, stack, tmp_path, capsys):
    from dpmn_amd.dataset.folder import box_region_batches
    src, box, imgs = _photo_folder(tmp_path, "both", QUAD_LINE + _line(CURVE, "####curved"))
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    seen = []
    out_dir = tmp_path / "out"
    # chunk=1: every region goes through the models on its own (repeated), so its bytes do not depend on its neighbours in the batch
    rows = sr.demo(models, psn, box_region_batches(src, box, 2, (16, 64), True, dev, polygons=True), str(out_dir), rec=_reader(seen),
                   text_prior_fn=fn, boxes=True, chunk=1)
    assert rows == [["p0", "000", "axis", "ab", "ab"], ["p0", "001", "curved", "ab", "ab"]]      # the files are named by k
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png"]
    got = _png(out_dir / "p0_001_sr.png")
    assert got.shape == (32, 128, 3) and got.min() != got.max()
    # the polygon's LR input: the restatement's crop, resized (the reader saw LR, SR of region 0, then LR, SR of region 1)
    h, w, xs = poly.polygon_plan(CURVE)
    crop, = poly.poly_crop_np([imgs["p0"]], [(0, h, w, poly.polygon_cells(CURVE, h, xs))])
    assert [tuple(s.shape) for s in seen] == [(1, 3, 16, 64), (1, 3, 32, 128)] * 2
    lr = torch.round(seen[2][0] * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    expected = resize.pil_resize_u8(crop, 16, 64)
    print("the polygon's LR input: %d of %d bytes differ from poly_crop_np + pil_resize_u8" % (int((lr != expected).sum()), lr.size))
    assert int((lr != expected).sum()) == 0
    # the quadrilateral: byte for byte the file of a run WITHOUT the flag on a box file holding only that line at the same position
    src1, box1, _ = _photo_folder(tmp_path, "quad", QUAD_LINE)
    rows1 = sr.demo(models, psn, box_region_batches(src1, box1, 2, (16, 64), True, dev), str(tmp_path / "out1"), rec=_reader([]),
                    text_prior_fn=fn, boxes=True, chunk=1)
    assert rows1 == rows[:1]
    assert (tmp_path / "out1" / "p0_000_sr.png").read_bytes() == (out_dir / "p0_000_sr.png").read_bytes()
    # paste=True: the photo file exists, the polygon is not pasted (one printed line), the region files and the csv are unchanged
    capsys.readouterr()
    pasted = tmp_path / "pasted"
    rows2 = sr.demo(models, psn, box_region_batches(src, box, 2, (16, 64), True, dev, photos=True, polygons=True), str(pasted),
                    rec=_reader([]), text_prior_fn=fn, boxes=True, chunk=1, paste=True)
    said = [line for line in capsys.readouterr().out.splitlines() if "not pasted" in line]
    assert rows2 == rows and len(said) == 1 and "1 polygon region of p0" in said[0]
    assert sorted(os.listdir(pasted)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png", "p0_photo_sr.png"]
    for f in ("demo_result.csv", "p0_000_sr.png", "p0_001_sr.png"):
        assert (pasted / f).read_bytes() == (out_dir / f).read_bytes(), f
    photo = _png(pasted / "p0_photo_sr.png")
    assert photo.shape == (80, 200, 3)
    # only the quadrilateral was pasted: away from it (and its feathered edge) the photo is PIL's enlargement
    from dpmn_amd.utils import paste
    plain = paste.enlarge_np(imgs["p0"], 2)
    assert not np.array_equal(photo, plain) and np.array_equal(photo[46:], plain[46:]) and np.array_equal(photo[:, 138:], plain[:, 138:])


def test_demo_polygons_tile_keeps_the_aspect_of_a_long_arc(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import box_window_batches
    src, box, _ = _photo_folder(tmp_path, "wide", QUAD_LINE + _line(CURVE, "####curved"), wide=True)
    sr, models, psn = stack
    out_dir = tmp_path / "out"
    rows = sr.demo(models, psn, box_window_batches(src, box, 2, (16, 64), True, dev, polygons=True), str(out_dir), rec=_reader([]),
                   text_prior_fn=sr.synthetic_text_prior(), tile=True, boxes=True, chunk=4)
    h, w, _ = poly.polygon_plan(LONG_ARC)
    w_line = tile.line_width(h, w)
    assert h == 12 and 195 <= w <= 205 and len(tile.window_plan(w_line)) > 1
    assert [r[:3] for r in rows] == [["p0", "000", "axis"], ["p0", "001", "curved"], ["p1", "000", "a long arc"]]
    assert rows[2][3] == "|".join(["ab"] * len(tile.window_plan(w_line)))
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png", "p1_000_sr.png"]      # one stitched file
    got = _png(out_dir / "p1_000_sr.png")
    assert got.shape == (32, 2 * w_line, 3) and got.min() != got.max()


def test_main_demo_polygons_writes_the_regions(dev, stack, tmp_path):
    """main.py --demo_dir DIR --demo_boxes BOXDIR --demo_polygons --resume CKPT: the polygon reader behind the flag; without it the
    14-point line is a quadrilateral with a long label, which check_quad refuses here."""
    import main as cli
    from dpmn_amd import workload
    from test_gpu_display_eval import _checkpoints
    src, box, _ = _photo_folder(tmp_path, "main", QUAD_LINE + _line(CURVE, "####curved"))
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    args = workload.make_args("tsrn", 1, 1, 2)
    args.resume, args.demo_dir, args.demo_boxes, args.demo_out, args.synthetic_steps = d, src, box, os.path.join(d, "regions"), 0
    args.demo_polygons = True
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "out"))})
    cli.main(config, args)
    assert sorted(os.listdir(args.demo_out)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png"]
    with open(os.path.join(args.demo_out, "demo_result.csv"), newline="") as f:
        assert list(csv.reader(f))[:3:2] == [["file", "box", "label", "lr_string", "sr_string"], ["p0", "001", "curved", "", ""]]
