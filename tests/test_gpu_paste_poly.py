"""csrc/paste_poly.hip against the numpy restatement of dpmn_amd/utils/paste_poly.py, byte for byte: ops.paste_mixed_u8 (one enlarged
photo, the SR images in pack_ragged's layout and ONE list of quadrilaterals and polygons -> the photo with the regions pasted, in
place), its rejections, and the path on top of it: TextSR.demo(paste=True, paste_polygons=True) and main.py --demo_paste_polygons."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dpmn_amd.utils import paste, paste_poly, poly, resize
from test_gpu_paste import PHOTO_HW, QUADS, SCALE, SR_SIZES, TILE_H, TILE_W
from test_gpu_poly import CURVE, QUAD_LINE, _line, _photo_folder, _png, _reader
from test_paste_poly import AXIS_POLY, arc
from test_poly import strips as edges

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# test_gpu_paste.py's geometry: a 23 x 41 photo enlarged to 46 x 82 (6 x 3 tiles of 8 x 32, the last of each partial), the SR images
# ragged behind an unused 3 x 5 one.  Three of its quadrilaterals (3: foreshortened, 4: overlapping it, 5: half outside) and seven
# polygons (points in photo coordinates, SR image): the k = 3 axis-aligned one of test_paste_poly.py (it leaves the photo on the right);
# a k = 7 arc that crosses tile borders in both directions and overlaps quadrilaterals 3 and 4; a k = 2 general convex quadrilateral; an
# arc whose middle strip is exactly one rectified column wide; an arc half outside the photo; one wholly outside; a small arc inside
# quadrilateral 4.  Nothing reaches the first tile row.
ARC = arc(20, 45, 38, 30, 0.45, 7)
NARROW = edges([(10, 10), (20, 10), (20.4, 10.1), (30, 11)], [(10, 16), (20, 16), (20.4, 16.1), (30, 17)])
POLYS = [(AXIS_POLY, 1),
         (ARC, 2),
         (np.array([(5.3, 6.2), (18.1, 5.4), (19.6, 10.9), (4.2, 12.3)]), 1),
         (NARROW, 1),
         (ARC + [-22.0, 5.0], 2),
         (ARC + [100.0, 60.0], 1),
         (arc(24, 40, 29, 25, 0.3, 4), 3)]
PICK = (3, 4, 5)
ORDER = ["q3", "p0", "p1", "q4", "p2", "p3", "q5", "p4", "p5", "p6"]      # quadrilaterals and polygons interleaved; p6 lies over q4
FEATHERS = (0.0, 1.5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene():
    """(enlarged photo, SR images, {feather: regions}, {(feather, reversed): the restatement's result}), computed once."""
    rng = np.random.RandomState(37)
    photo2 = paste.enlarge_np(rng.randint(0, 256, PHOTO_HW + (3,)).astype(np.uint8), SCALE)
    srs = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in SR_SIZES]
    regions = {}
    for f in FEATHERS:
        by = {"q%d" % i: (QUADS[i][1], paste.paste_coeffs(QUADS[i][0], SCALE, SR_SIZES[QUADS[i][1]][1], SR_SIZES[QUADS[i][1]][0]), f) for i in PICK}
        by.update({"p%d" % i: (k, paste_poly.strip_table(pts, SCALE, SR_SIZES[k][1], SR_SIZES[k][0]), f) for i, (pts, k) in enumerate(POLYS)})
        regions[f] = [by[name] for name in ORDER]
    ref = {(f, rev): paste_poly.paste_mixed_np(photo2, srs, regions[f][::-1] if rev else regions[f]) for f in FEATHERS for rev in (False, True)}
    return photo2, srs, regions, ref


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def test_the_scene_holds_what_it_names(scene):
    photo2, srs, regions, ref = scene
    assert photo2.shape == (46, 82, 3)
    xs = poly.polygon_plan(NARROW)[2]
    assert 1 in np.diff(xs).tolist() and len(xs) == 4                    # a strip exactly one rectified column wide
    assert regions[0.0][ORDER.index("p1")][1].shape == (6, 10) and regions[0.0][ORDER.index("p2")][1].shape == (1, 10)
    alone = lambda name: paste_poly.paste_mixed_np(photo2, srs, [regions[0.0][ORDER.index(name)]])
    assert np.array_equal(alone("p5"), photo2)                           # wholly outside
    assert all(not np.array_equal(alone("p%d" % i), photo2) for i in (0, 1, 2, 3, 4, 6))
    for f in FEATHERS:
        assert not np.array_equal(ref[(f, False)], ref[(f, True)])       # the overlaps: the order matters
    assert not np.array_equal(ref[(0.0, False)], ref[(1.5, False)])


@pytest.mark.parametrize("feather", FEATHERS)
def test_paste_mixed_equals_the_restatement(dev, scene, feather):
    from dpmn_amd import ops
    photo2, srs, regions, ref = scene
    packed, meta = resize.pack_ragged(srs)
    assert meta[1:, 0].min() > 0
    packed = packed.to(dev)
    for rev in (False, True):
        regs = regions[feather][::-1] if rev else regions[feather]
        d = torch.from_numpy(photo2).to(dev)
        out = ops.paste_mixed_u8(d, packed, meta, regs)
        assert out is d                                                   # in place
        got = out.cpu().numpy()
        expected = ref[(feather, rev)]
        print("paste_mixed_u8 feather %g%s: %d of %d bytes differ, %d bytes pasted"
              % (feather, " reversed" if rev else "", int((got != expected).sum()), got.size, int((expected != photo2).sum())))
        assert np.array_equal(got, expected)
    # only the tiles that a box meets are launched (a polygon: the boxes of its strips), and the pixels of the others are unchanged
    H2, W2 = photo2.shape[:2]
    tiles_of = lambda b: {(r, c) for r in range(b[1] // TILE_H, -(-b[3] // TILE_H)) for c in range(b[0] // TILE_W, -(-b[2] // TILE_W))
                          if b[2] > b[0] and b[3] > b[1]}
    met = set()
    for reg in regions[feather]:
        k, shape, _ = reg
        if paste_poly.is_polygon_region(reg):
            for s in shape:
                met |= tiles_of(paste_poly.strip_box(s, H2, W2))
        else:
            met |= tiles_of(paste.region_box(shape, SR_SIZES[k][1], SR_SIZES[k][0], H2, W2))
    host = ops._paste_mixed_plan(torch.from_numpy(photo2).to(dev), packed, meta, regions[feather])
    assert {(int(t[0]), int(t[1])) for t in host["tiles"]} == met and host["tiles"].shape[0] == len(met)
    assert not met & {(0, 0), (0, 1), (0, 2)} and (2, 1) in met and len(met) < 18
    got = ops.paste_mixed_u8(torch.from_numpy(photo2).to(dev), packed, meta, regions[feather]).cpu().numpy()
    for r in range(6):
        for col in range(3):
            if (r, col) not in met:
                sl = (slice(r * TILE_H, (r + 1) * TILE_H), slice(col * TILE_W, (col + 1) * TILE_W))
                assert np.array_equal(got[sl], photo2[sl])
    assert host["strips"].shape == (sum(r[1].shape[0] for r in regions[feather] if paste_poly.is_polygon_region(r)), 14)
    assert all(list(host["list"][t[2]:t[2] + t[3]]) == sorted(host["list"][t[2]:t[2] + t[3]]) for t in host["tiles"])
    # a list of quadrilaterals alone is paste_regions_u8's result
    quads = [r for r in regions[feather] if not paste_poly.is_polygon_region(r)]
    a = ops.paste_mixed_u8(torch.from_numpy(photo2).to(dev), packed, meta, quads).cpu().numpy()
    b = ops.paste_regions_u8(torch.from_numpy(photo2).to(dev), packed, meta, quads).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, paste.paste_regions_np(photo2, srs, quads))


def test_rejections_and_the_empty_list(dev, scene):
    from dpmn_amd import _abi, ops
    photo2, srs, regions, _ = scene
    packed, meta = resize.pack_ragged(srs)
    packed = packed.to(dev)
    regs = regions[0.0]
    fresh = lambda: torch.from_numpy(photo2).to(dev)
    d = fresh()
    assert ops.paste_mixed_u8(d, packed, meta, []) is d and np.array_equal(d.cpu().numpy(), photo2)
    strips = regs[ORDER.index("p1")][1]
    bad = strips.copy()
    bad[2, 5] = np.nan
    flat = torch.zeros(46 * 82 * 3 + 64, dtype=torch.uint8, device=dev)
    bad_calls = [
        lambda: ops.paste_mixed_u8(torch.from_numpy(photo2), packed, meta, regs),                          # a CPU photo
        lambda: ops.paste_mixed_u8(fresh(), packed[:-1], meta, regs),                                      # the meta points past the buffer
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(len(srs), strips, 0.0)]),                      # an SR index out of range
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(1, bad, 0.0)]),                                # a NaN in a strip
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(1, strips[:, :9], 0.0)]),
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(1, np.zeros((32, 10)), 0.0)]),                 # more strips than a polygon has
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(1, strips, float("nan"))]),
        lambda: ops.paste_mixed_u8(fresh(), packed, meta, [(1, strips)]),
        lambda: ops.paste_mixed_u8(flat[:46 * 82 * 3].view(46, 82, 3), flat, [(46 * 82 * 3 - 3, 1, 2)], [(0, strips, 0.0)]),      # aliased
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(_abi.DpmnError, match="paste_mixed_u8"):
            call()
            pytest.fail("call %d was accepted" % i)
    # the library refuses the same numbers when they reach it past the wrapper: nothing is launched, the photo stays
    plan = ops._paste_mixed_plan(fresh(), packed, meta, regs)
    r = ORDER.index("p1")
    first, n = (int(v) for v in plan["table"][r, 5:7])
    S = plan["strips"].shape[0]
    assert plan["table"][r, 4] == 1 and n == 6 and first + n < S

    def past_the_sr_buffer(table):
        table[r, 0] = packed.numel() - 32 * 200 * 3 + 1

    def strips_past_the_table(table):
        table[r, 5] = S - n + 1

    def a_negative_strip_offset(table):
        table[r, 5] = -1

    def too_many_strips(table):
        table[r, 6] = 32

    def no_strip(table):
        table[r, 6] = 0

    def an_unknown_kind(table):
        table[r, 4] = 2

    for tamper in (past_the_sr_buffer, strips_past_the_table, a_negative_strip_offset, too_many_strips, no_strip, an_unknown_kind):
        host = dict(plan, table=plan["table"].copy())
        tamper(host["table"])
        d = fresh()
        code = ops._paste_mixed_run(d, packed, host)
        torch.cuda.synchronize()
        assert code == -1 and np.array_equal(d.cpu().numpy(), photo2), tamper.__name__
        with pytest.raises(_abi.DpmnError, match="paste_mixed"):
            _abi.check(code)
    # overlapping buffers: the photo a view of the buffer that holds the SR images
    both = torch.cat([torch.from_numpy(photo2).to(dev).reshape(-1), packed])
    before = both.cpu().numpy()
    code = ops._paste_mixed_run(both[:46 * 82 * 3].view(46, 82, 3), both, plan)
    torch.cuda.synchronize()
    assert code == -1 and np.array_equal(both.cpu().numpy(), before)


def _expected_photo(photo, lines, out_dir, feather):
    """The restatement on what the run wrote: PIL's enlargement with the region PNGs of p0, read back, pasted in box-file order."""
    srs, regions = [], []
    for k, pts in enumerate(lines):
        s = _png(os.path.join(out_dir, "p0_%03d_sr.png" % k))
        shape = paste_poly.strip_table(pts, 2, s.shape[1], s.shape[0]) if len(pts) > 4 else paste.paste_coeffs(pts, 2, s.shape[1], s.shape[0])
        regions.append((len(srs), shape, feather))
        srs.append(s)
    return paste_poly.paste_mixed_np(paste.enlarge_np(photo, 2), srs, regions)


AXIS = np.array([3, 5, 67, 5, 67, 21, 3, 21], np.float64).reshape(4, 2)      # QUAD_LINE's corners


def test_demo_pastes_the_polygons(dev, stack, tmp_path, capsys):
    from dpmn_amd.dataset.folder import box_region_batches
    src, box, imgs = _photo_folder(tmp_path, "both", QUAD_LINE + _line(CURVE, "####curved"))
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    make = lambda: box_region_batches(src, box, 2, (16, 64), True, dev, photos=True, polygons=True)
    kw = dict(rec=_reader([]), text_prior_fn=fn, boxes=True, chunk=1, paste=True)
    plain, out_dir = tmp_path / "plain", tmp_path / "out"
    rows_plain = sr.demo(models, psn, make(), str(plain), **kw)
    capsys.readouterr()
    rows = sr.demo(models, psn, make(), str(out_dir), paste_polygons=True, **kw)
    assert "not pasted" not in capsys.readouterr().out
    assert rows == rows_plain
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png", "p0_photo_sr.png"]
    for f in ("demo_result.csv", "p0_000_sr.png", "p0_001_sr.png"):      # the region files and the csv: exactly as without the flag
        assert (plain / f).read_bytes() == (out_dir / f).read_bytes(), f
    got = _png(out_dir / "p0_photo_sr.png")
    expected = _expected_photo(imgs["p0"], [AXIS, CURVE], str(out_dir), 1.0)
    print("p0_photo_sr.png: %d of %d bytes differ from the restatement" % (int((got != expected).sum()), got.size))
    assert got.shape == (80, 200, 3) and np.array_equal(got, expected)
    # against the run without the flag: other bytes inside the polygon's box, the same bytes outside it
    before = _png(plain / "p0_photo_sr.png")
    x0, y0, x1, y1 = paste_poly.polygon_box(paste_poly.strip_table(CURVE, 2, 128, 32), 80, 200)
    differ = (got != before).any(axis=2)
    assert differ[y0:y1, x0:x1].sum() > 1000
    differ[y0:y1, x0:x1] = False
    assert not differ.any()
    with pytest.raises(ValueError, match="paste_polygons=True needs paste=True"):
        sr.demo(models, psn, iter(()), str(tmp_path / "no"), text_prior_fn=fn, boxes=True, paste_polygons=True)


def test_main_demo_paste_polygons_writes_the_photo(dev, stack, tmp_path):
    """python main.py ... --demo_paste --demo_polygons --demo_paste_polygons in a process of its own: the photo holds the regions that
    this run wrote, the polygon's too; without one of its companions the flag is a usage error."""
    from test_gpu_display_eval import _checkpoints
    src, box, imgs = _photo_folder(tmp_path, "main", QUAD_LINE + _line(CURVE, "####curved"))
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    out_dir = os.path.join(d, "pasted")
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--arch", "tsrn", "--mask", "--gradient", "--synthetic_prior", "--batch_size", "2",
            "--stu_iter_b1", "1", "--stu_iter_b2", "1", "--patch_size", "2,2,", "--embed_dim", "96,96,", "--window_size", "2,4,8,2,4,8,",
            "--depths", "1,1,", "--num_heads", "6,6,", "--mlp_ratio", "4,4,", "--drop_rate", "0,0,", "--attn_drop_rate", "0,0,",
            "--drop_path_rate", "0,0,", "--resume", d, "--demo_dir", src, "--demo_boxes", box, "--demo_out", out_dir, "--demo_paste_polygons"]
    for missing in (["--demo_paste"], ["--demo_polygons"]):
        r = subprocess.run(base + missing, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--demo_paste_polygons needs --demo_paste and --demo_polygons" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--demo_paste", "--demo_polygons", "--demo_paste_feather", "2"], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "not pasted" not in r.stdout
    assert sorted(os.listdir(out_dir)) == ["demo_result.csv", "p0_000_sr.png", "p0_001_sr.png", "p0_photo_sr.png"]
    got = _png(os.path.join(out_dir, "p0_photo_sr.png"))
    assert got.shape == (80, 200, 3) and np.array_equal(got, _expected_photo(imgs["p0"], [AXIS, CURVE], out_dir, 2.0))
