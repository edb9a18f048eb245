"""The semantics of the polygon path (dpmn_amd/utils/poly.py, dataset/folder.py box_batches(polygons=True)), no GPU: poly_crop_np
against PIL's own Image.transform(MESH, BICUBIC), byte for byte; the checks, the plan and the cells of a polygon; the reader of the box
files; the host half of the loader on a temp folder; and main.py's refusal of --demo_polygons without --demo_boxes."""
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from dpmn_amd.utils import poly, quad, resize
from test_quad import photos

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def arc(cx, cy, r_top, r_bottom, half_angle, k):
    """2k points of a ring segment around (cx, cy), clockwise from top-left: r_top > r_bottom is concave down (the centre lies below
    the text, a rainbow), r_top < r_bottom concave up (the centre above, a smile)."""
    a = np.linspace(-half_angle, half_angle, k)
    s = -1.0 if r_top > r_bottom else 1.0
    t = np.stack([cx + r_top * np.sin(a), cy + s * r_top * np.cos(a)], 1)
    b = np.stack([cx + r_bottom * np.sin(a), cy + s * r_bottom * np.cos(a)], 1)
    return np.concatenate([t, b[::-1]])


def strips(tops, bottoms):
    return np.concatenate([np.asarray(tops, np.float64), np.asarray(bottoms, np.float64)[::-1]])


ARC_DOWN = arc(44, 90, 74, 60, 0.5, 7)
ARC_UP = arc(44, -50, 60, 74, 0.5, 7)
NARROW = strips([(10, 10), (40, 10), (40.8, 10.2), (70, 12)], [(10, 22), (40, 22), (40.8, 22.2), (70, 24)])
BENT = strips([(20, 10), (40, 8), (60, 12)], [(19, 22), (40, 20), (59, 25)])
# (name, photo of test_quad.photos(), points, (h, xs) or None for polygon_plan's): the photos are 0: 1 x 1, 3: 7 x 31, 4: 40 x 89
CASES = [
    ("one_cell_k2", 4, [(10.3, 8.7), (75.2, 2.1), (78.9, 21.4), (13.6, 29.8)], None),
    ("arc_down_k7", 4, ARC_DOWN, None),
    ("arc_up_k7", 4, ARC_UP, None),
    ("one_column_strip", 4, NARROW, None),                       # xs = [0, 30, 31, 60]: a strip of one column, a bound at column 31
    ("height_one", 4, ARC_DOWN, (1, [0, 12, 24, 36, 48, 60, 70])),
    ("region_9x33", 4, BENT, (9, [0, 16, 33])),                  # one past the 8 x 32 tile in both directions
    ("bound_at_32", 4, BENT, (8, [0, 32, 50])),
    ("bound_at_31", 4, BENT, (12, [0, 31, 64])),
    ("half_outside", 4, ARC_UP + [-40.0, -12.0], None),
    ("wholly_outside", 4, ARC_DOWN + [200.0, 100.0], None),
    ("small_7x31_arc", 3, arc(15, 40, 38.5, 34, 0.35, 4), None),
    ("one_pixel_photo", 0, strips([(-1, -0.5), (0.5, -0.25), (2, -0.5)], [(-1, 1.5), (0.5, 1.25), (2, 1.5)]), (3, [0, 2, 5])),
]


def case_regions(names=None):
    """[(name, points, (photo, h, w, cells), xs)] of CASES (all, or the named ones in the order given)."""
    by_name = {c[0]: c for c in CASES}
    out = []
    for name, b, pts, plan in (CASES if names is None else [by_name[n] for n in names]):
        pts = np.asarray(pts, np.float64)
        poly.check_polygon(pts)
        h, xs = plan or (poly.polygon_plan(pts)[0], poly.polygon_plan(pts)[2])
        out.append((name, pts, (b, h, xs[-1], poly.polygon_cells(pts, h, xs)), xs))
    return out


def pil_crop(photo, pts, h, xs):
    """PIL's own answer: per strip the box (x0, 0, x1, h) of the output and the quad NW, SW, SE, NE = t[i], b[i], b[i+1], t[i+1]."""
    k = len(pts) // 2
    t, b = pts[:k], pts[k:][::-1]
    mesh = [((x0, 0, x1, h), tuple(float(v) for p in (t[i], b[i], b[i + 1], t[i + 1]) for v in p)) for i, (x0, x1) in enumerate(zip(xs, xs[1:]))]
    return np.asarray(Image.fromarray(photo).transform((xs[-1], h), Image.MESH, mesh, Image.BICUBIC))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_equals_pil_mesh(name):
    imgs = photos()
    (_, pts, (b, h, w, cells), xs), = case_regions([name])
    got, = poly.poly_crop_np(imgs, [(b, h, w, cells)])
    live = pil_crop(imgs[b], pts, h, xs)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) == live.shape
    differ = int((got != live).sum())
    print("%s %d x %d, bounds %s: %d of %d bytes differ from PIL" % (name, h, w, xs, differ, got.size))
    assert differ == 0


def test_what_the_cases_show():
    imgs = photos()
    by = {name: (pts, region, xs) for name, pts, region, xs in case_regions()}
    crop = lambda name: poly.poly_crop_np(imgs, [by[name][1]])[0]
    assert len(by["one_cell_k2"][1][3]) == 1 and len(by["arc_down_k7"][1][3]) == 6
    assert by["one_column_strip"][2] == [0, 30, 31, 60]
    assert by["height_one"][1][1] == 1 and by["region_9x33"][1][1:3] == (9, 33)
    assert int(crop("wholly_outside").max()) == 0
    half = crop("half_outside")
    assert int(half[:, :20].max()) == 0 and half[-1, -1].any()
    for name in ("arc_down_k7", "arc_up_k7", "small_7x31_arc"):
        c = crop(name)
        assert c.min() != c.max()
    # every tap of a 1 x 1 photo is its one pixel: its value where the polygon lies over the photo, black beyond
    assert {tuple(p) for p in crop("one_pixel_photo").reshape(-1, 3)} == {tuple(imgs[0][0, 0]), (0, 0, 0)}
    # one cell is PIL's QUAD transform of the quadrilateral
    pts, (b, h, w, cells), _ = by["one_cell_k2"]
    nw, ne, se, sw = pts
    quad_ = np.asarray(Image.fromarray(imgs[b]).transform((w, h), Image.QUAD, tuple(np.concatenate([nw, sw, se, ne])), Image.BICUBIC))
    assert np.array_equal(crop("one_cell_k2"), quad_)


def test_restatement_on_random_arcs_against_pil():
    rng = np.random.RandomState(7)
    total = differ = 0
    for _ in range(12):
        H, W = int(rng.randint(1, 90)), int(rng.randint(1, 200))
        ph = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        r, hh = rng.uniform(30, 200), rng.uniform(3, 25)
        down = rng.rand() < 0.5
        pts = arc(rng.uniform(-10, W + 10), rng.uniform(-10, H + 10) + (r if down else -r), r + hh if down else r, r if down else r + hh,
                  rng.uniform(0.15, 0.75), int(rng.randint(2, 8)))
        poly.check_polygon(pts)
        h, w, xs = poly.polygon_plan(pts)
        got, = poly.poly_crop_np([ph], [(0, h, w, poly.polygon_cells(pts, h, xs))])
        total += got.size
        differ += int((got != pil_crop(ph, pts, h, xs)).sum())
    print("random arcs: %d of %d bytes differ from PIL" % (differ, total))
    assert differ == 0 and total > 20000


def test_restatement_rejects_what_it_cannot_crop():
    ph = photos()[4]
    (_, _, (_, h, w, cells), _), = case_regions(["region_9x33"])
    a = cells[0][2]
    for bad in ([(1, h, w, cells)], [(-1, h, w, cells)], [(0, 0, w, cells)], [(0, h, w + 1, cells)], [(0, h, w, [])],
                [(0, h, w, cells[:1])], [(0, h, w, [(0, 16, a), (17, 33, a)])], [(0, h, w, [(0, 16, a[:7]), (16, 33, a)])],
                [(0, 40, 40, [(i, i + 1, a) for i in range(40)])], [(0, h, resize.MAX_SIDE + 1, [(0, resize.MAX_SIDE + 1, a)])]):
        with pytest.raises(ValueError):
            poly.poly_crop_np([ph], bad)
    # a non-finite source position counts as outside
    got, = poly.poly_crop_np([ph], [(0, 2, 2, [(0, 2, [np.nan, 0, 0, 0, 1, 0, 1, 0])])])
    assert int(got.max()) == 0


def test_polygon_plan():
    for q in ([(0, 0), (10, 0), (10, 4), (0, 4)], [(0, 0), (10, 0), (12, 5), (0, 4)], [(0, 0), (2.5, 0), (2.5, 1), (0, 1)],
              [(0, 0), (0.2, 0), (0.2, 0.3), (0, 0.3)], CASES[0][2]):
        h, w, xs = poly.polygon_plan(q)
        assert (h, w) == quad.quad_size(q) and xs == [0, w]
    assert poly.polygon_plan(ARC_DOWN)[:2] == (14, 67)              # arcs of radius 74 and 60 over 1 rad (mean length 67), 14 apart
    # a strip narrower than half a column still gets one
    h, w, xs = poly.polygon_plan(strips([(0, 0), (10, 0), (10.2, 0), (20, 0)], [(0, 5), (10, 5), (10.2, 5), (20, 5)]))
    assert (h, xs) == (5, [0, 10, 11, 20])
    with pytest.raises(ValueError):
        poly.polygon_plan([(0, 0), (resize.MAX_SIDE + 1, 0), (resize.MAX_SIDE + 1, 20), (0, 20)])
    assert poly.polygon_plan([(0, 0), (resize.MAX_SIDE, 0), (resize.MAX_SIDE, 20000), (0, 20000)])[:2] == (resize.MAX_SIDE, resize.MAX_SIDE)
    with pytest.raises(ValueError):
        poly.polygon_plan([(0, 0), (10, 0), (10, 4)])


def test_polygon_cells_are_pils_quad_coefficients():
    pts = np.asarray(BENT)
    cells = poly.polygon_cells(pts, 9, [0, 16, 33])
    assert [(x0, x1) for x0, x1, _ in cells] == [(0, 16), (16, 33)]
    x0, x1, a = cells[1]
    assert a.dtype == np.float64 and a.shape == (8,)
    # the bilinear map takes the corners of the cell's box to NW, NE, SE, SW of its strip
    for (u, v), (X, Y) in zip(((0, 0), (17, 0), (17, 9), (0, 9)), (pts[1], pts[2], pts[3], pts[4])):
        assert abs(a[0] + a[1] * u + a[2] * v + a[3] * u * v - X) <= 1e-12 and abs(a[4] + a[5] * u + a[6] * v + a[7] * u * v - Y) <= 1e-12
    for bad in ([0, 16], [1, 16, 33], [0, 16, 16], [0, 33, 16]):
        with pytest.raises(ValueError):
            poly.polygon_cells(pts, 9, bad)


def test_check_polygon():
    poly.check_polygon(ARC_DOWN)
    poly.check_polygon(ARC_UP + [-500.0, 300.0])                                # outside any photo: fine
    poly.check_polygon(np.asarray(NARROW).reshape(-1))                          # the flat form of a box file's line
    for name, bad in (("a concave strip", strips([(0, 0), (10, 0), (20, 0)], [(0, 8), (10, 8), (12, 1)])),
                      ("anticlockwise", np.asarray(ARC_DOWN)[::-1]),
                      ("area below 1", strips([(0, 0), (0.4, 0), (0.8, 0)], [(0, 0.9), (0.4, 0.9), (0.8, 0.9)])),
                      ("nan", strips([(0, 0), (10, np.nan), (20, 0)], [(0, 8), (10, 8), (20, 8)])),
                      ("inf", strips([(0, 0), (10, 0), (np.inf, 0)], [(0, 8), (10, 8), (20, 8)])),
                      ("a self-crossing strip", strips([(0, 0), (10, 0), (5, 0)], [(0, 8), (10, 8), (20, 8)])),
                      ("an odd number of points", [(0, 0), (10, 0), (20, 0), (20, 8), (0, 8)]),
                      ("2 points", [(0, 0), (10, 0)]),
                      ("too many points", arc(0, 500, 520, 500, 1.0, poly.MAX_POLY_SIDE + 1))):
        with pytest.raises(ValueError):
            poly.check_polygon(bad)
            pytest.fail("%s accepted" % name)
    poly.check_polygon(arc(0, 500, 520, 500, 1.0, poly.MAX_POLY_SIDE))


QUAD = "3,5,67,5,67,21,3,21"
CURVE = ",".join("%g" % v for v in np.round(ARC_DOWN, 2).reshape(-1))      # 14 points


def _read(tmp_path, text):
    p = tmp_path / "gt.txt"
    p.write_bytes(text.encode("utf-8"))
    return poly.numbered_polygons(str(p))


def test_reader_quad_with_a_year_as_label(tmp_path):
    (k, lineno, pts, label), = _read(tmp_path, QUAD + ",2015\n")
    assert (k, lineno, label) == (0, 1, "2015") and pts.dtype == np.float64 and pts.tolist() == [[3, 5], [67, 5], [67, 21], [3, 21]]


def test_reader_quad_with_a_number_with_a_comma_as_label(tmp_path):
    (_, _, pts, label), = _read(tmp_path, QUAD + ",1,000\n")
    assert label == "1,000" and pts.shape == (4, 2)


def test_reader_14_points_with_ctw_marker(tmp_path):
    (_, _, pts, label), = _read(tmp_path, CURVE + ",####curved\n")
    assert label == "curved" and np.array_equal(pts, np.round(ARC_DOWN, 2))


def test_reader_14_points_without_label(tmp_path):
    rows = _read(tmp_path, CURVE + "\n" + CURVE + ",\n")
    assert [r[3] for r in rows] == [" ", " "] and all(r[2].shape == (14, 2) for r in rows)


def test_reader_5_points_are_a_quad_and_a_label(tmp_path):
    (_, _, pts, label), = _read(tmp_path, QUAD + ",70,30\n")
    assert pts.tolist() == [[3, 5], [67, 5], [67, 21], [3, 21]] and label == "70,30"


def test_reader_skips_dont_care_silently(tmp_path, capsys):
    rows = _read(tmp_path, QUAD + ",###\n" + CURVE + ",###\n" + CURVE + ",#######\n" + QUAD + ",kept\n")
    assert [(r[0], r[3]) for r in rows] == [(3, "kept")] and capsys.readouterr().out == ""


def test_reader_malformed_line_keeps_k_counting(tmp_path, capsys):
    rows = _read(tmp_path, QUAD + ",a\n\n5,5,9,five,9,8,5,8,word\n1,2,3\n   \n" + QUAD + ", b,,c\n")
    out = capsys.readouterr().out.strip().splitlines()
    assert [(k, lineno, label) for k, lineno, _, label in rows] == [(0, 1, "a"), (3, 6, " b,,c")]
    assert len(out) == 2 and all("gt.txt" in line for line in out) and "line 3" in out[0] and "line 4" in out[1]


def test_reader_drops_a_bom(tmp_path):
    (k, _, pts, label), = _read(tmp_path, "\ufeff" + QUAD + ",café\r\n")
    assert (k, label) == (0, "café") and pts[0].tolist() == [3, 5]


def test_reader_more_than_64_points_do_not_parse(tmp_path, capsys):
    line = lambda n: ",".join(str(i) for i in range(2 * n))
    rows = _read(tmp_path, line(66) + ",too many\n" + line(64) + ",####the most\n")
    out = capsys.readouterr().out.strip().splitlines()
    assert [(r[0], r[2].shape, r[3]) for r in rows] == [(1, (64, 2), "the most")]
    assert len(out) == 1 and "line 1" in out[0]


def test_reader_agrees_with_numbered_boxes_on_quads(tmp_path):
    p = tmp_path / "q.txt"
    p.write_text(QUAD + ",hello\n" + " 1.5 , 2.25,30,4 ,31.0,14,2,1e1,a, b,,c\n" + QUAD + "\n" + QUAD + ",\n" + QUAD + ",###\n1,2\n" + QUAD + ",2015\n")
    old, new = quad.numbered_boxes(str(p)), poly.numbered_polygons(str(p))
    assert [(k, n, q.tolist(), lab) for k, n, q, lab in old] == [(k, n, q.tolist(), lab) for k, n, q, lab in new] and len(new) == 5


def test_box_batches_with_polygons(tmp_path, capsys):
    from dpmn_amd.dataset.folder import box_batches
    Image.fromarray(photos()[4]).save(str(tmp_path / "p.png"))
    concave = ",".join("%g" % v for v in strips([(0, 0), (10, 0), (20, 0)], [(0, 8), (10, 8), (12, 1)]).reshape(-1))
    (tmp_path / "p.txt").write_text(QUAD + ",word\n" + CURVE + ",####curved\n" + QUAD + ",###\n" + concave + ",bad\n1,2,3\n")
    (names, labels, packed, meta, regions, corners), = list(box_batches(str(tmp_path), str(tmp_path), 2, quads=True, polygons=True))
    out = capsys.readouterr().out.strip().splitlines()
    assert names == ["p_000", "p_001"] and labels == ["word", "curved"] and [len(c) for c in corners] == [4, 14]
    # the reader's line comes first (the file is read before its regions are checked), then the refused polygon's
    assert len(out) == 2 and "line 5" in out[0] and "p.txt line 4" in out[1] and "strip 1" in out[1]
    pts = np.round(ARC_DOWN, 2)
    h, w, xs = poly.polygon_plan(pts)
    assert regions[1][:3] == (0, h, w) and [c[:2] for c in regions[1][3]] == list(zip(xs, xs[1:]))
    assert all(np.array_equal(c[2], e[2]) for c, e in zip(regions[1][3], poly.polygon_cells(pts, h, xs)))
    # the quadrilateral is the region it is without the flag, which then sees the polygon's line as a quad with a long label
    plain = list(box_batches(str(tmp_path), str(tmp_path), 8))
    assert plain[0][0][0] == "p_000" and plain[0][4][0][1:3] == regions[0][1:3] and np.array_equal(plain[0][4][0][3], regions[0][3])
    # `check` sees a polygon's size like a quad's
    capsys.readouterr()

    def no_wide(rh, rw, name):
        if rw > 4.5 * rh:
            raise ValueError("%s is too wide" % name)
    (names, *_), = list(box_batches(str(tmp_path), str(tmp_path), 2, check=no_wide, polygons=True))
    assert names == ["p_000"] and "p_001 is too wide" in capsys.readouterr().out


def test_demo_polygons_without_demo_boxes_is_refused():
    spec = importlib.util.spec_from_file_location("dpmn_main_poly", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(demo_polygons=True, demo_boxes=None, demo_dir="photos"))
    assert str(e.value) == m.DEMO_POLYGONS_NEEDS_BOXES and str(e.value).startswith("main.py: --demo_polygons needs --demo_boxes")
    assert "\n" not in str(e.value)
    # the command line: the argument parser reports it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "photos", "--demo_polygons"], capture_output=True, text=True)
    assert r.returncode == 2 and "error: --demo_polygons needs --demo_boxes" in r.stderr
