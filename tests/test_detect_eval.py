"""utils/detect_eval.py without a GPU: the sampled overlap against exact geometry and against an independent brute force, the row form
against the sample form, the ICDAR protocol, the end-to-end counts, the reader and main.py's argument checks."""
import importlib.util
import math
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import detect_eval_cases as ec
from dpmn_amd.utils import detect_eval as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- exact geometry ----

def _shoelace(poly):
    return abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(poly, poly[1:] + poly[:1]))) / 2


def _clip(subject, clipper):
    """Sutherland-Hodgman in Fractions: both convex, the clipper clockwise in image coordinates (interior: cross >= 0)."""
    out = [(Fraction(x), Fraction(y)) for x, y in subject]
    for (ax, ay), (bx, by) in zip(clipper, clipper[1:] + clipper[:1]):
        side = lambda p: (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)
        src, out = out, []
        for p, q in zip(src, src[1:] + src[:1]):
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return []
    return out


def _units(p):
    return [tuple(int(v) for v in row) for row in de.region_units(p).tolist()]


def _perimeter(p):
    u = de.region_units(p).astype(np.float64) / de.UNIT
    return float(np.hypot(*(np.roll(u, -1, axis=0) - u).T).sum())


def _bound(perimeter, n):
    """The bound on |count / 16 - exact area| in pixels^2, from the geometry alone.  A sample stands for its cell, a square of side
    s = 1 / 4 pixel with the sample at its centre; a cell that the region's boundary does not enter lies wholly inside or wholly
    outside and is counted exactly, so the error is at most one cell area (1 / 16) per cell whose interior the boundary enters.  An edge
    of length l with direction angle a meets at most l |cos a| / s + 1 vertical and l |sin a| / s + 1 horizontal grid lines in its
    interior, and enters one cell more than it meets lines: at most (|cos a| + |sin a|) l / s + 3 <= sqrt(2) l / s + 3 = 4 sqrt(2) l + 3
    cells.  Summed over the n edges of perimeter P and divided by 16: sqrt(2) P / 4 + 3 n / 16.  (The boundary of an intersection is
    part of the two boundaries: P and n are then the sums over both regions.)"""
    return math.sqrt(2) * perimeter / 4 + 3 * n / 16


def _exact_check(a, b=None):
    ua = _units(a)
    if b is None:
        exact = Fraction(_shoelace(ua)) / de.UNIT ** 2
        got, P, n = de.area_np(de.region_units(a)), _perimeter(a), len(a)
    else:
        exact = Fraction(_shoelace(_clip(ua, _units(b)) or [(0, 0)])) / de.UNIT ** 2
        got, P, n = de.inter_np(de.region_units(a), de.region_units(b)), _perimeter(a) + _perimeter(b), len(a) + len(b)
    assert abs(got / 16 - float(exact)) <= _bound(P, n), (got / 16, float(exact), _bound(P, n))
    return got, exact


def test_pixel_aligned_rectangles_are_exact():
    for x0, y0, x1, y1 in ((0, 0, 10, 5), (3, 7, 4, 8), (-6, -2, 9, 1)):
        got, exact = _exact_check(ec.rect(x0, y0, x1, y1))
        assert got == 16 * (x1 - x0) * (y1 - y0) == 16 * exact
    got, exact = _exact_check(ec.rect(0, 0, 10, 10), ec.rect(4, 2, 20, 7))
    assert got == 16 * 6 * 5 == 16 * exact


@pytest.mark.parametrize("deg", [2.8125, 30, 45, 89])
def test_turned_quads_against_exact_area(deg):
    a, b = ec.turned(40.3, 30.7, 60, 14, deg), ec.turned(44.1, 33.2, 50, 18, deg / 2 + 5)
    _exact_check(a)
    _exact_check(b)
    got, exact = _exact_check(a, b)
    assert exact > 0 and got > 0


def test_nested_identical_and_disjoint_quads():
    outer, inner = ec.turned(50, 50, 80, 40, 20), ec.turned(50, 50, 30, 10, 20)
    uo, ui = de.region_units(outer), de.region_units(inner)
    _exact_check(inner, outer)
    assert de.inter_np(ui, uo) == de.area_np(ui)                     # a quad inside another
    assert de.inter_np(uo, uo) == de.area_np(uo) > 0                 # two identical quads
    a, b = ec.turned(20, 20, 40, 4, 45), ec.turned(32, 8, 10, 4, 45)      # disjoint, but the boxes meet
    ua, ub = de.region_units(a), de.region_units(b)
    assert len(de.meeting_pairs(de.boxes_of([ua]), de.boxes_of([ub]))) == 1
    assert not _clip(_units(a), _units(b)) and de.inter_np(ua, ub) == 0


# ---- the even-odd rule against an independent brute force ----

def _brute(points, box):
    """Every sample of the box by a float64 winding number along the UPWARD ray (the definition looks to the right): (inside under the
    even-odd rule, the winding numbers, the least distance of a sample to an edge in pixels)."""
    u = de.region_units(points).astype(np.float64) / de.UNIT
    x0b, y0b, x1b, y1b = box
    xs = (np.arange(4 * x0b, 4 * x1b) * 2 + 1) / 8.0
    ys = (np.arange(4 * y0b, 4 * y1b) * 2 + 1) / 8.0
    X, Y = np.meshgrid(xs, ys)
    wind, dist = np.zeros(X.shape, np.int64), np.full(X.shape, np.inf)
    for (ax, ay), (bx, by) in zip(u, np.roll(u, -1, axis=0)):
        ex, ey = bx - ax, by - ay
        if ex != 0:
            yc = ay + (X - ax) * ey / ex
            hit = ((ax > X) != (bx > X)) & (yc < Y)
            wind += np.where(hit, 1 if ex > 0 else -1, 0)
        L2 = ex * ex + ey * ey
        t = np.clip(((X - ax) * ex + (Y - ay) * ey) / L2, 0, 1) if L2 else np.zeros(X.shape)
        dist = np.minimum(dist, np.hypot(X - (ax + t * ex), Y - (ay + t * ey)))
    return wind % 2 != 0, wind, float(dist.min())


def _brute_check(a, b=None):
    ua = de.region_units(a)
    box = de.region_box(ua) if b is None else de._meet(de.region_box(ua), de.region_box(de.region_units(b)))
    ia, _, da = _brute(a, box)
    assert da > 1e-6, "a sample lies on an edge: move the case"
    assert np.array_equal(de.inside_np(ua, box), ia)
    if b is None:
        assert de.area_np(ua) == int(ia.sum()) == de.rows_count_np(ua)
        return int(ia.sum())
    ib, _, db = _brute(b, box)
    assert db > 1e-6
    n = int((ia & ib).sum())
    assert de.inter_np(ua, de.region_units(b)) == n == de.rows_count_np(ua, de.region_units(b))
    return n


def test_even_odd_against_brute_force():
    assert _brute_check(ec.arc14()) > 0
    assert _brute_check(ec.arc14(), ec.through_arc()) > 0
    assert _brute_check(ec.poly64()) > 0
    assert _brute_check(ec.poly64(), ec.turned(40, 30, 70, 9, 12)) > 0
    assert _brute_check(ec.comb()) > 0                                        # 12 crossings on one sample row
    q = ec.turned(30.3, 20.9, 40, 12, 17)
    assert _brute_check(q) == _brute_check(q[::-1].copy())                    # an anticlockwise quad counts as its clockwise twin
    tie = ec.bowtie()
    n = _brute_check(tie)
    assert 0 < n < de.area_np(de.region_units(ec.rect(3.3, 4.1, 43.7, 24.9)))       # its two lobes, about half the rectangle
    assert _brute_check(tie, ec.rect(3.3, 4.1, 43.7, 24.9)) == n


def test_row_form_equals_sample_form_on_random_regions():
    rng = np.random.RandomState(7)
    for it in range(60):
        a, b = rng.uniform(-6, 28, (int(rng.choice([4, 6, 14, 64])), 2)), rng.uniform(-6, 28, (int(rng.choice([4, 8])), 2))
        if it % 3 == 0:      # coordinates on the sample grid's lines: crossings that land exactly on a sample
            a, b = np.round(a * 4) / 4 + 0.125, np.round(b * 8) / 8
        ua, ub = de.region_units(a), de.region_units(b)
        assert de.area_np(ua) == de.rows_count_np(ua)
        assert de.inter_np(ua, ub) == de.rows_count_np(ua, ub)


def test_units_rounding_and_limits():
    u = de.region_units([[0.005, -0.005], [1.234, 2.0], [3, -2.375], [0, 1]])
    assert u.tolist() == [[8, -8], [984, 1600], [2400, -1904], [0, 800]]      # half away from zero (of 100 v in float64), times 8
    assert (u % 8 == 0).all()
    with pytest.raises(ValueError):
        de.region_units(ec.rect(0, 0, 16384.01, 5))
    de.region_units(ec.rect(-16384, 0, 16384, 5))
    with pytest.raises(ValueError):
        de.region_units(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        de.region_units(np.zeros((65, 2)))
    assert de.region_box(de.region_units(ec.rect(0.5, -0.5, 10, 3.01))) == (0, -1, 10, 4)


def test_regions_flat_equals_the_per_region_functions():
    regions = [ec.rect(0.5, -0.5, 10, 3.01), ec.arc14(), ec.poly64(), ec.bowtie(), ec.turned(-40.5, -30.25, 30, 8, -20), ec.rect(3.4, 4.4, 3.48, 4.48)]
    units, n, boxes = de.regions_flat(regions)
    assert n.tolist() == [4, 14, 64, 4, 4, 4]
    assert np.array_equal(units, np.concatenate([de.region_units(r) for r in regions]))
    assert np.array_equal(boxes, de.boxes_of([de.region_units(r) for r in regions]))
    assert [a.shape for a in de.regions_flat([])] == [(0, 2), (0,), (0, 4)]
    for bad in (np.zeros((3, 2)), ec.rect(0, 0, 20000, 4), np.full((4, 2), np.inf)):
        with pytest.raises(ValueError):
            de.regions_flat([regions[0], bad])


def test_region_counts_pairs_are_row_major_and_skip_far_boxes():
    a = [ec.rect(0, 0, 10, 10), ec.rect(100, 100, 110, 110), ec.rect(5, 5, 15, 15)]
    b = [ec.rect(8, 8, 12, 12), ec.rect(0, 0, 10, 10)]
    area_a, area_b, pairs, inter = de.region_counts_np(a, b)
    assert pairs.tolist() == [[0, 0], [0, 1], [2, 0], [2, 1]]
    assert area_a.tolist() == [1600] * 3 and area_b.tolist() == [256, 1600] and inter.tolist() == [64, 1600, 256, 400]
    assert area_a.dtype == area_b.dtype == inter.dtype == np.uint64 and pairs.dtype == np.int64


# ---- the protocol ----

def _record(dets, gts, dont_care=None):
    return de.match(*de.region_counts_np(dets, gts), dont_care or [False] * len(gts))


def test_detection_inside_a_dont_care_region_costs_nothing():
    rec = _record([ec.rect(0, 0, 10, 10), ec.rect(52, 52, 60, 58)], [ec.rect(0, 0, 10, 10), ec.rect(50, 50, 80, 80)], [False, True])
    assert rec["det_dont_care"] == [1] and rec["matches"] == [(0, 0)]
    assert (rec["gt_care"], rec["det_care"], rec["matched"], rec["precision"], rec["recall"]) == (1, 1, 1, 1.0, 1.0)


def test_greedy_order():
    rec = _record([ec.rect(0, 0, 10, 10), ec.rect(0, 0, 10, 9)], [ec.rect(0, 0, 10, 10)])
    assert rec["matches"] == [(0, 0)] and (rec["precision"], rec["recall"]) == (0.5, 1.0)      # the earlier detection
    rec = _record([ec.rect(0, 0, 10, 10)], [ec.rect(0, 0, 10, 9), ec.rect(0, 0, 10, 10)])
    assert rec["matches"] == [(0, 0)] and (rec["precision"], rec["recall"]) == (1.0, 0.5)      # the earlier ground truth


def test_iou_of_exactly_one_half_does_not_match():
    det, gt = ec.rect(0, 0, 20, 10), ec.rect(0, 0, 10, 10)      # inter 100, union 200
    area_d, area_g, pairs, inter = de.region_counts_np([det], [gt])
    assert 2 * int(inter[0]) == int(area_d[0]) + int(area_g[0]) - int(inter[0])
    assert de.match(area_d, area_g, pairs, inter, [False])["matched"] == 0
    assert _record([ec.rect(0, 0, 19, 10)], [gt])["matched"] == 1


def test_empty_set_conventions():
    assert de.prf(0, 0, 0) == (1.0, 1.0, 1.0)
    assert de.prf(0, 0, 3) == (0.0, 1.0, 0.0)
    assert de.prf(0, 2, 0) == (0.0, 0.0, 0.0)
    rec = _record([], [ec.rect(0, 0, 4, 4)], [True])
    assert (rec["precision"], rec["recall"], rec["hmean"]) == (1.0, 1.0, 1.0)
    rec = _record([ec.rect(20, 20, 30, 30)], [ec.rect(0, 0, 4, 4)], [True])
    assert (rec["precision"], rec["recall"], rec["hmean"]) == (0.0, 1.0, 0.0)
    rec = _record([ec.rect(0, 0, 0.001, 0.001)], [ec.rect(0, 0, 4, 4)])      # area 0: matches nothing
    assert rec["matched"] == 0 and rec["det_care"] == 1


def test_micro_average_differs_from_the_mean_of_the_photos():
    one = _record([ec.rect(0, 0, 10, 10)], [ec.rect(0, 0, 10, 10)])
    gts = [ec.rect(20 * i, 0, 20 * i + 10, 10) for i in range(4)]
    two = _record([gts[0], ec.rect(0, 50, 10, 60), ec.rect(30, 50, 40, 60), ec.rect(60, 50, 70, 60)], gts)
    tot = de.score([one, two])
    assert (tot["matched"], tot["gt_care"], tot["det_care"]) == (2, 5, 5)
    assert tot["recall"] == 2 / 5 and tot["recall"] != (one["recall"] + two["recall"]) / 2 == 0.625
    assert tot["hmean"] == pytest.approx(0.4)


def test_e2e_counts():
    gts = [ec.rect(0, 0, 10, 10), ec.rect(20, 0, 30, 10), ec.rect(40, 0, 50, 10), ec.rect(60, 0, 70, 10)]
    labels, dc = ["Hello!", " ", "New York", "###"], [False, False, False, True]
    dets = [gts[0], gts[1], gts[2], ec.rect(80, 0, 90, 10)]
    rec = de.match(*de.region_counts_np(dets, gts), dc)
    assert rec["matches"] == [(0, 0), (1, 1), (2, 2)] and rec["det_care"] == 4
    got = de.e2e(rec, labels, dc, ["hello", "x", "newyork", "zz"])
    assert (got["e2e_labelled"], got["e2e_correct"], got["e2e_det"]) == (2, 2, 3)      # the label-less GT and its detection are out
    assert got["e2e_recall"] == 1.0 and got["e2e_precision"] == 2 / 3
    got = de.e2e(rec, labels, dc, ["hello", "x", "new york", "zz"], spaces=False)      # a line read holding spaces
    assert got["e2e_correct"] == 2
    assert de.e2e(rec, labels, dc, ["hello", "x", "new york", "zz"])["e2e_correct"] == 1
    tot = de.score([dict(rec, **got)])
    assert (tot["e2e_correct"], tot["e2e_labelled"], tot["e2e_det"]) == (2, 2, 3)


# ---- the reader ----

def test_numbered_regions(tmp_path, capsys):
    path = tmp_path / "gt_a.txt"
    path.write_bytes("\ufeff0,0,10,0,10,10,0,10,###\r\n\r\n1,1,5,1,5,5,1,5,####text\n1,1,5,1,5,5,1,5,1,000\n1,2,3\n"
                     "0,0,1,0,2,0,3,0,3,1,2,1,1,1,0,1,####curve, two\n0,0,9,0,9,9,0,9,#######\n0,0,9,0,9,9,0,9\n".encode("utf-8"))
    rows = de.numbered_regions(str(path))
    assert "line 5 does not parse" in capsys.readouterr().out
    assert [(k, n, len(p), label, dc) for k, n, p, label, dc in rows] == [
        (0, 1, 4, "###", True), (1, 3, 4, "text", False), (2, 4, 4, "1,000", False), (4, 6, 8, "curve, two", False),
        (5, 7, 4, "###", True), (6, 8, 4, " ", False)]
    assert rows[0][2].tolist() == [[0, 0], [10, 0], [10, 10], [0, 10]]      # (the BOM is dropped: the first number parses)
    from dpmn_amd.utils.poly import numbered_polygons
    assert [r[0] for r in numbered_polygons(str(path))] == [1, 2, 4, 6]      # the same line counter; ### lines are skipped there


def test_load_photo_refuses_far_coordinates(tmp_path, capsys):
    (tmp_path / "gt").mkdir()
    (tmp_path / "box").mkdir()
    (tmp_path / "gt" / "p.txt").write_text("0,0,10,0,10,10,0,10,word\n0,0,20000,0,20000,10,0,10,far\n")
    (tmp_path / "box" / "p.txt").write_text("0,0,10,0,10,10,0,10\n0,0,99999,0,99999,10,0,10\n5,5,6,5,6,6,5,6\n")
    photo = de.load_photo("p", str(tmp_path / "box"), str(tmp_path / "gt"), {0: ("word", None), 1: ("x", None)})
    out = capsys.readouterr().out
    assert out.count("refused") == 2 and "line 2" in out
    assert photo["gt_dont_care"] == [False, True] and photo["det_absent"] == [1] and len(photo["det"]) == 2      # line 2 had no row
    recs, tot = de.evaluate([photo], de.region_counts_batch_np)
    assert (recs[0]["det"], recs[0]["det_care"], recs[0]["gt_care"], recs[0]["matched"], recs[0]["e2e_correct"]) == (1, 1, 1, 1, 1)
    assert de.load_photo("q", str(tmp_path / "box"), str(tmp_path / "gt"), {}) is None
    assert "q has no ground truth" in capsys.readouterr().out


def test_row_reads_columns():
    rows = [["p", "000", "a", "lr", "0.9", "sr", "0.8", "1", "lex", "-1.0", "1"], ["p", "002", "b", "lr", "0.9", "", "0.1", "0", "w", "-2.0", "0"]]
    assert de.row_reads(rows, conf=True, upright=True, lexicon=True, min_conf=True) == {"p": {0: ("sr", "lex")}}
    assert de.row_reads([["a_b", "001", "t", "lr", "sr"]]) == {"a_b": {1: ("sr", None)}}
    assert de.row_reads([["s", "003", "t", "lr", "sr", "word", "-3.5"]], lexicon=True) == {"s": {3: ("sr", "word")}}


# ---- main.py ----

def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_detect_eval", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_demo_eval_setting(tmp_path):
    m = _main()
    ns = types.SimpleNamespace
    assert m.demo_eval_setting(ns()) is None and m.demo_eval_setting(ns(demo_eval=None, demo_dir="d")) is None
    with pytest.raises(ValueError) as e:
        m.demo_eval_setting(ns(demo_eval=str(tmp_path), demo_detect=True))
    assert "main.py: " + str(e.value) == m.DEMO_EVAL_NEEDS_DIR
    with pytest.raises(ValueError) as e:
        m.demo_eval_setting(ns(demo_eval=str(tmp_path), demo_dir="d"))
    assert "main.py: " + str(e.value) == m.DEMO_EVAL_NEEDS_BOXES
    with pytest.raises(ValueError, match="is not a directory"):
        m.demo_eval_setting(ns(demo_eval=str(tmp_path / "missing"), demo_dir="d", demo_boxes="b"))
    assert m.demo_eval_setting(ns(demo_eval=str(tmp_path), demo_dir="d", demo_boxes="b")) == str(tmp_path)
    assert m.demo_eval_setting(ns(demo_eval=str(tmp_path), demo_dir="d", demo_detect=True)) == str(tmp_path)
    for flags, message in ((dict(demo_detect=True), m.DEMO_EVAL_NEEDS_DIR), (dict(demo_dir="d"), m.DEMO_EVAL_NEEDS_BOXES)):
        with pytest.raises(SystemExit) as e:      # main() ends with the one line before anything touches the GPU
            m.main(ns(), ns(demo_eval=str(tmp_path), **flags))
        assert str(e.value) in (message, m.DEMO_DETECT_NEEDS_DIR)


def test_csv_layout():
    rec = _record([ec.rect(0, 0, 10, 10)], [ec.rect(0, 0, 10, 10)])
    rec["file"] = "p"
    rows = de.csv_rows([rec], de.score([rec]), recogniser=False)
    assert rows[0] == de.CSV_HEAD and rows[-1][0] == "TOTAL" and rows[1][:9] == ["p", "1", "1", "1", "1", "1", "1.0000", "1.0000", "1.0000"]
    assert rows[1][9:] == [""] * 5
    rec.update(de.e2e(rec, ["a"], [False], ["a"]))
    rec.update({"e2e_lexicon_" + k[4:]: v for k, v in de.e2e(rec, ["a"], [False], ["b"]).items()})
    rows = de.csv_rows([rec], de.score([rec]), lexicon=True)
    assert rows[0] == de.CSV_HEAD + de.CSV_LEXICON and rows[2][9:] == ["1", "1", "1.0000", "1.0000", "1.0000", "0.0000", "0.0000", "0.0000"]
