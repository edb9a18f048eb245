"""csrc/paste_poly.hip's perspective regions against the numpy restatement of dpmn_amd/utils/paste.py, byte for byte: ops.paste_regions_u8 (one enlarged photo,
the SR images in pack_ragged's layout and a list of regions -> the photo with the regions pasted, in place), its rejections, and the
paste path on top of it: TextSR.demo(boxes=True, paste=True) and main.py --demo_paste."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import paste, quad, resize, tile

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# a 23 x 41 photo enlarged to 46 x 82: no multiple of the 8 x 32 tile in either direction (6 tile rows, 3 tile columns, the last of each
# partial).  Seven regions (quad in photo coordinates, SR image) in one call: inside the single tile (0, 0); crossing tile borders in
# both directions; a sliver one enlarged pixel wide; a foreshortened quad; one that overlaps the last and the second (the order
# matters); one half outside the photo; one wholly outside.  The SR images are ragged -- 32 x 128, 32 x 200 and 1 x 1 -- behind an
# unused 3 x 5 image, so each lies at a non-zero offset.  No region's box meets tile (5, 2).
PHOTO_HW, SCALE = (23, 41), 2
SR_SIZES = [(3, 5), (32, 128), (32, 200), (1, 1)]
QUADS = [([(1.5, 0.75), (13.5, 1), (13.25, 3.25), (1.25, 3)], 3),
         ([(10, 5), (30, 4), (31, 12), (11, 13)], 1),
         ([(35, 2), (35.5, 2), (35.5, 12), (35, 12)], 2),
         ([(3, 12), (22, 10), (23, 21), (3.5, 15)], 1),
         ([(15, 8), (34, 9.5), (33, 17), (14, 15)], 2),
         ([(-8, 14), (9, 15), (8.5, 26), (-9, 24.5)], 2),
         ([(50, 30), (70, 31), (69, 38), (49, 37)], 1)]
FEATHERS = (0.0, 1.5)
TILE_H, TILE_W = 8, 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene():
    """(enlarged photo, SR images, {feather: regions}, {(feather, reversed): the restatement's result}), computed once."""
    rng = np.random.RandomState(31)
    photo2 = paste.enlarge_np(rng.randint(0, 256, PHOTO_HW + (3,)).astype(np.uint8), SCALE)
    srs = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in SR_SIZES]
    regions = {f: [(k, paste.paste_coeffs(q, SCALE, SR_SIZES[k][1], SR_SIZES[k][0]), f) for q, k in QUADS] for f in FEATHERS}
    ref = {(f, rev): paste.paste_regions_np(photo2, srs, regions[f][::-1] if rev else regions[f]) for f in FEATHERS for rev in (False, True)}
    return photo2, srs, regions, ref


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


@pytest.mark.parametrize("feather", FEATHERS)
def test_paste_regions_equals_the_restatement(dev, scene, feather):
    from dpmn_amd import ops
    photo2, srs, regions, ref = scene
    assert photo2.shape == (46, 82, 3)
    packed, meta = resize.pack_ragged(srs)
    assert meta[1:, 0].min() > 0
    packed = packed.to(dev)
    for rev in (False, True):
        regs = regions[feather][::-1] if rev else regions[feather]
        d = torch.from_numpy(photo2).to(dev)
        out = ops.paste_regions_u8(d, packed, meta, regs)
        assert out is d                                                   # in place
        got = out.cpu().numpy()
        expected = ref[(feather, rev)]
        print("paste_regions_u8 feather %g%s: %d of %d bytes differ, %d bytes pasted"
              % (feather, " reversed" if rev else "", int((got != expected).sum()), got.size, int((expected != photo2).sum())))
        assert np.array_equal(got, expected)
    assert not np.array_equal(ref[(feather, False)], ref[(feather, True)])      # the overlap: the order matters
    assert not np.array_equal(ref[(0.0, False)], ref[(1.5, False)])
    # only the tiles that a region's box meets are launched, and the pixels of the others are unchanged
    H2, W2 = photo2.shape[:2]
    met = set()
    for k, c, _ in regions[feather]:
        x0, y0, x1, y1 = paste.region_box(c, SR_SIZES[k][1], SR_SIZES[k][0], H2, W2)
        met |= {(r, col) for r in range(y0 // TILE_H, -(-y1 // TILE_H)) for col in range(x0 // TILE_W, -(-x1 // TILE_W)) if x1 > x0 and y1 > y0}
    host = ops._paste_mixed_plan(torch.from_numpy(photo2).to(dev), packed, meta, regions[feather], what="paste_regions_u8", polygons=False)
    assert {(int(t[0]), int(t[1])) for t in host["tiles"]} == met and host["tiles"].shape[0] == len(met)
    assert (0, 0) in met and (5, 2) not in met and len(met) < 18
    for r in range(6):
        for col in range(3):
            if (r, col) not in met:
                sl = (slice(r * TILE_H, (r + 1) * TILE_H), slice(col * TILE_W, (col + 1) * TILE_W))
                assert np.array_equal(got[sl], photo2[sl])
    # the first region lies in one tile; every tile's list is in the order of the regions
    assert [(int(t[0]), int(t[1])) for t in host["tiles"] if 0 in host["list"][t[2]:t[2] + t[3]]] == [(0, 0)]
    assert all(list(host["list"][t[2]:t[2] + t[3]]) == sorted(host["list"][t[2]:t[2] + t[3]]) for t in host["tiles"])


def test_stitched_lines_and_quantised_images_are_the_packed_layout(dev, scene):
    """What the demo passes: a contiguous (R, H, W, 3) uint8 batch viewed flat, with the meta of equal sizes."""
    from dpmn_amd import ops
    photo2, _, _, _ = scene
    rng = np.random.RandomState(4)
    batch = rng.randint(0, 256, (2, 32, 128, 3)).astype(np.uint8)
    regs = [(1, paste.paste_coeffs(QUADS[1][0], SCALE, 128, 32), 1.0), (0, paste.paste_coeffs(QUADS[3][0], SCALE, 128, 32), 1.0)]
    out = ops.paste_regions_u8(torch.from_numpy(photo2).to(dev), torch.from_numpy(batch).to(dev).reshape(-1),
                               [(r * 32 * 128 * 3, 32, 128) for r in range(2)], regs)
    assert np.array_equal(out.cpu().numpy(), paste.paste_regions_np(photo2, list(batch), regs))


def test_rejections_and_the_empty_list(dev, scene):
    from dpmn_amd import _abi, ops
    photo2, srs, regions, _ = scene
    packed, meta = resize.pack_ragged(srs)
    packed = packed.to(dev)
    regs = regions[0.0]
    fresh = lambda: torch.from_numpy(photo2).to(dev)
    d = fresh()
    assert ops.paste_regions_u8(d, packed, meta, []) is d and np.array_equal(d.cpu().numpy(), photo2)
    c = regs[1][1]
    flat = torch.zeros(46 * 82 * 3 + 64, dtype=torch.uint8, device=dev)
    bad_calls = [
        lambda: ops.paste_regions_u8(torch.from_numpy(photo2), packed, meta, regs),                       # a CPU photo
        lambda: ops.paste_regions_u8(fresh(), packed.cpu(), meta, regs),                                  # CPU SR images
        lambda: ops.paste_regions_u8(fresh().float(), packed, meta, regs),                                # a float photo
        lambda: ops.paste_regions_u8(fresh()[:, :, :2], packed, meta, regs),                              # a wrong shape
        lambda: ops.paste_regions_u8(fresh()[:, ::2], packed, meta, regs),                                # not contiguous
        lambda: ops.paste_regions_u8(fresh(), packed[:-1], meta, regs),                                   # the meta points past the buffer
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(len(srs), c, 0.0)]),                        # an SR index out of range
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(-1, c, 0.0)]),
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(1, [np.nan] + list(c[1:]), 0.0)]),          # NaN coefficients
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(1, c[:7], 0.0)]),
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(1, c, float("nan"))]),
        lambda: ops.paste_regions_u8(fresh(), packed, meta, [(1, c)]),
        lambda: ops.paste_regions_u8(flat[:46 * 82 * 3].view(46, 82, 3), flat, [(46 * 82 * 3 - 3, 1, 2)], [(0, c, 0.0)]),      # aliased
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(_abi.DpmnError, match="paste_regions_u8"):
            call()
            pytest.fail("call %d was accepted" % i)
    # the library refuses the same numbers when they reach it past the wrapper: nothing is launched, the photo stays
    d = fresh()
    host = ops._paste_mixed_plan(d, packed, meta, regs, what="paste_regions_u8", polygons=False)
    host["table"] = host["table"].copy()
    host["table"][2, 0] = packed.numel() - 32 * 200 * 3 + 1      # the SR image of region 2 ends one byte past the buffer
    code = ops._paste_mixed_run(d, packed, host)
    torch.cuda.synchronize()
    assert code == -1 and np.array_equal(d.cpu().numpy(), photo2)
    with pytest.raises(_abi.DpmnError, match="paste_mixed"):
        _abi.check(code)


def test_a_polygon_item_is_refused_under_the_name_paste_regions_u8(dev, scene):
    """paste_regions_u8 shares paste_mixed_u8's plan and kernel but takes quadrilaterals only: an item that carries a strip table is
    refused under its own name before anything is launched."""
    from dpmn_amd import _abi, ops
    from dpmn_amd.utils import paste_poly
    from test_poly import ARC_DOWN
    photo2, srs, regions, _ = scene
    packed, meta = resize.pack_ragged(srs)
    strips = paste_poly.strip_table(ARC_DOWN, SCALE, SR_SIZES[1][1], SR_SIZES[1][0])
    assert strips.ndim == 2 and strips.shape[1] == 10 and paste_poly.is_polygon_region((1, strips, 0.0))
    d = torch.from_numpy(photo2).to(dev)
    for regs in ([(1, strips, 0.0)], regions[0.0][:2] + [(1, strips, 0.0)]):
        with pytest.raises(_abi.DpmnError, match="paste_regions_u8"):
            ops.paste_regions_u8(d, packed.to(dev), meta, regs)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), photo2)


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


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


def _expected_photo(stem, photo, box_file, out_dir, feather):
    """The restatement on what the run wrote: the enlarged photo with the region PNGs of `stem`, read back, pasted in box-file order."""
    srs, regions = [], []
    for k, _, q, _ in quad.numbered_boxes(box_file):
        s = _png(os.path.join(out_dir, "%s_%03d_sr.png" % (stem, k)))
        regions.append((len(srs), paste.paste_coeffs(q, 2, s.shape[1], s.shape[0]), feather))
        srs.append(s)
    return paste.paste_regions_np(paste.enlarge_np(photo, 2), srs, regions)


@pytest.mark.parametrize("tiled", [False, True])
def test_demo_paste_writes_the_photos_with_their_regions_pasted(dev, stack, tmp_path, tiled):
    from dpmn_amd.dataset.folder import box_region_batches, box_window_batches
    src, box, imgs = _photo_folder(tmp_path, wide=tiled)
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    make = box_window_batches if tiled else box_region_batches
    kw = dict(text_prior_fn=fn, boxes=True, tile=tiled, chunk=4 if tiled else None)
    plain, out_dir = str(tmp_path / "plain"), str(tmp_path / "out")
    rows_plain = sr.demo(models, psn, make(src, box, 2, (16, 64), True, dev), plain, **kw)
    rows = sr.demo(models, psn, make(src, box, 2, (16, 64), True, dev, photos=True), out_dir, paste=True, feather=1.0, **kw)
    assert rows == rows_plain
    region_files = sorted(os.listdir(plain))
    assert sorted(os.listdir(out_dir)) == sorted(region_files + [stem + "_photo_sr.png" for stem in imgs])
    for f in region_files:      # the region files and the CSV: exactly as without paste
        with open(os.path.join(plain, f), "rb") as a, open(os.path.join(out_dir, f), "rb") as b:
            assert a.read() == b.read(), f
    box_files = {"p0": "p0.txt", "p1": "gt_p1.txt", "p2": "p2.txt"}
    for stem, photo in imgs.items():
        got = _png(os.path.join(out_dir, stem + "_photo_sr.png"))
        assert got.shape == (2 * photo.shape[0], 2 * photo.shape[1], 3)
        expected = _expected_photo(stem, photo, os.path.join(box, box_files[stem]), out_dir, 1.0)
        print("%s_photo_sr.png: %d of %d bytes differ from the restatement, %d bytes pasted"
              % (stem, int((got != expected).sum()), got.size, int((expected != paste.enlarge_np(photo, 2)).sum())))
        assert np.array_equal(got, expected)
        assert not np.array_equal(got, paste.enlarge_np(photo, 2))
    if tiled:
        assert _png(os.path.join(out_dir, "p2_000_sr.png")).shape == (32, 2 * tile.line_width(12, 200), 3)


def test_demo_paste_needs_boxes(dev, stack, tmp_path):
    sr, models, psn = stack
    with pytest.raises(ValueError, match="paste=True needs boxes=True"):
        sr.demo(models, psn, iter(()), str(tmp_path / "out"), text_prior_fn=sr.synthetic_text_prior(), paste=True)


def test_main_demo_paste_writes_the_photos(dev, stack, tmp_path):
    """python main.py --demo_dir DIR --demo_boxes BOXDIR --demo_paste --resume CKPT in a process of its own: the photo files appear
    beside the regions and hold the regions that this run wrote."""
    from test_gpu_display_eval import _checkpoints
    src, box, imgs = _photo_folder(tmp_path)
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    out_dir = os.path.join(d, "pasted")
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--arch", "tsrn", "--mask", "--gradient", "--synthetic_prior", "--batch_size", "2",
           "--stu_iter_b1", "1", "--stu_iter_b2", "1", "--patch_size", "2,2,", "--embed_dim", "96,96,", "--window_size", "2,4,8,2,4,8,",
           "--depths", "1,1,", "--num_heads", "6,6,", "--mlp_ratio", "4,4,", "--drop_rate", "0,0,", "--attn_drop_rate", "0,0,",
           "--drop_path_rate", "0,0,", "--resume", d, "--demo_dir", src, "--demo_boxes", box, "--demo_paste", "--demo_paste_feather", "2",
           "--demo_out", out_dir]
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=600)      # (cwd: the config's ./ckpt lands in the temp folder)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_002_sr.png", "p0_photo_sr.png", "p1_000_sr.png",
                                           "p1_photo_sr.png"]
    got = _png(os.path.join(out_dir, "p1_photo_sr.png"))
    assert got.shape == (60, 240, 3)
    assert np.array_equal(got, _expected_photo("p1", imgs["p1"], os.path.join(box, "gt_p1.txt"), out_dir, 2.0))
    assert np.array_equal(_png(os.path.join(out_dir, "p0_photo_sr.png")), _expected_photo("p0", imgs["p0"], os.path.join(box, "p0.txt"), out_dir, 2.0))
