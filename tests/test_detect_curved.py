"""utils/detect.py's curved recipe (main.py --demo_detect_curved) on the CPU: the bin identity, straight scenes byte for byte the plain
recipe, valid polygons that round-trip through the box-file reader, the arc scored with utils/detect_eval.py's NumPy overlap, the
filters, MAX_BOXES over the mixed list and the command line's two messages.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

import detect_cases as cases
import detect_curved_cases as cc
from dpmn_amd.utils import detect, detect_eval, poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_R = {}


def regions_of(name):
    """(photo, parameters, regions) of a case of detect_curved_cases, computed once."""
    if name not in _R:
        make, kw = cc.CASES[name]
        photo = make()
        _R[name] = (photo, kw, detect.detect_curved_np(photo, **kw))
    return _R[name]


def tables_of(photo, **kw):
    labels = detect.detect_maps_np(photo, **kw)[3]
    comps = detect.components(labels)
    cand = detect.curve_candidates(comps)
    return comps, cand, detect.curve_profile(labels, cand)


def iou(a, b):
    """IoU of two regions in pixels by the evaluator's sample counts."""
    area_a, area_b, pairs, inter = detect_eval.region_counts_np([a], [b])
    if len(pairs) == 0:
        return 0.0
    i = int(inter[0])
    return i / (int(area_a[0]) + int(area_b[0]) - i)


def box_points(b):
    x0, y0, x1, y1 = (float(v) for v in b)
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])


def test_the_bin_formula_is_the_search_over_the_edges():
    for w in range(16, 301):
        n = min(detect.CURVE_BINS, w // 8)
        assert 2 <= n <= 16
        for x0 in (0, 37):
            e = np.array([x0 + i * w // n for i in range(n + 1)])
            assert e[0] == x0 and e[-1] == x0 + w and (np.diff(e) >= 8).all()
            x = np.arange(x0, x0 + w)
            want = np.searchsorted(e, x, side="right") - 1      # the greatest i with e_i <= x
            assert np.array_equal(detect.curve_bin(x, x0, w, n), want), (w, n, x0)
    c = detect.curve_candidates(np.array([[0, 0, 15, 9, 1], [3, 0, 19, 5, 1], [3, 0, 19, 6, 1], [3, 0, 20, 6, 1], [0, 0, 300, 9, 1], [0, 0, 127, 9, 1]]))
    assert c.tolist() == [[0, 0, 0], [0, 0, 0], [3, 16, 2], [3, 17, 2], [0, 300, 16], [0, 127, 15]]


STRAIGHT = {
    "70x131": (lambda: cases.speckle(70, 131, 4), dict(gap=3)),
    "words": (lambda: cases.word_photo()[0], {}),
    "bricks": (lambda: cases.bricks(200, 260), dict(gap=1)),
    "all_foreground": (cases.all_foreground, {}),
    "checkerboard": (cases.checkerboard, dict(gap=1, vgap=1)),
    "serpentine": (cases.serpentine, dict(gap=1, vgap=1)),
    "flat": (cases.flat, {}),
    "1x2050": (lambda: cases.noise(1, 2050, 6), {}),
    "sag_0": (lambda: cc.photo(sag=0), {}),
    "sag_0_local": (lambda: cc.photo(sag=0), dict(local=128)),
}


@pytest.mark.parametrize("name", sorted(STRAIGHT))
def test_straight_scenes_keep_their_box_files_byte_for_byte(name):
    make, kw = STRAIGHT[name]
    photo = make()
    regions = detect.detect_curved_np(photo, **kw)
    assert all(len(q) == 4 for q in regions)
    assert detect.region_lines(regions) == detect.box_lines(detect.detect_text_np(photo, **kw))
    if name in ("words", "sag_0"):
        assert len(regions) >= 1


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_every_polygon_is_valid_and_the_file_round_trips(name, tmp_path):
    photo, kw, regions = regions_of(name)
    path = str(tmp_path / "a.txt")
    detect.write_regions(path, regions)
    back = poly.numbered_polygons(path)
    assert len(back) == len(regions)
    for (k, lineno, points, label), q in zip(back, regions):
        assert label == " " and points.shape == q.shape and np.array_equal(points, q / 100.0)
        if len(q) > 4:
            assert 6 <= len(q) <= 2 * detect.CURVE_BINS and len(q) % 2 == 0
            poly.check_polygon(points)
            poly.polygon_plan(points)
    bounds = [(q[:, 1].min(), q[:, 0].min(), q[:, 1].max(), q[:, 0].max()) for q in regions]
    assert bounds == sorted(bounds)


def test_the_cases_hold_what_they_are_for():
    n_poly = lambda name: sum(len(q) > 4 for q in regions_of(name)[2])
    for name in ("arc_down", "arc_up", "crossing_a_word", "alone_130", "local", "many_wide"):
        assert n_poly(name) >= 1, name
    for name in ("straight_row", "w16", "w17", "two_in_a_word", "flat", "speckle_small", "many", "wide_strip"):
        assert n_poly(name) == 0, name
    assert len(regions_of("straight_row")[2]) == 1


@pytest.mark.parametrize("sag", [cc.ARC_SAG, -cc.ARC_SAG])
def test_the_arc_is_found_as_a_polygon_and_not_by_the_plain_recipe(sag):
    """ICDAR's matching threshold, IoU > 0.5 with the ground-truth ribbon: the curved recipe's region passes it, no region of the plain
    recipe does (its box is there, and too high)."""
    assert cc.ARC_LETTERS >= 10
    photo, ribbon = cc.bowed(cc.ARC_LETTERS, sag)
    regions = detect.detect_curved_np(photo)
    assert len(regions) == 1 and len(regions[0]) == 2 * detect.CURVE_BINS
    got = iou(regions[0] / 100.0, ribbon)
    plain = [iou(box_points(b), ribbon) for b in detect.detect_text_np(photo)]
    print("sag %d: polygon IoU %.3f, plain boxes %s" % (sag, got, [round(v, 3) for v in plain]))
    assert got > 0.5
    assert len(plain) == 1 and all(v <= 0.5 for v in plain)


def _fabricated(area):
    """One component 160 x 60 whose 16 bins run 40 rows down from a parabola 20 deep, with the mass in their upper eighth: C_i =
    2 top_i + 10, so R = 70 -- a ribbon higher than the component's own box."""
    t = np.linspace(-1.0, 1.0, 16)
    top = np.rint(20 * (1 - t * t)).astype(np.int64)
    comps = np.array([[0, 0, 160, 60, area]], np.int64)
    cand = detect.curve_candidates(comps)
    assert cand.tolist() == [[0, 160, 16]]
    prof = np.zeros((1, 16, 4), np.int64)
    prof[0, :, 0], prof[0, :, 1], prof[0, :, 2] = top, top + 40, 200
    prof[0, :, 3] = 200 * top + 900      # C = (2 sy + cnt) // cnt = 2 top + 10
    return comps, cand, prof


@pytest.mark.parametrize("what,H,area", [("too tall for the map", 130, 6000), ("too sparse for its ribbon", 400, 3600)])
def test_a_curved_component_that_fails_its_filter_is_dropped_and_not_boxed(what, H, area):
    comps, cand, prof = _fabricated(area)
    assert len(detect.boxes_from_components(comps, H, 300)) == 1      # the plain recipe keeps it
    straight, ribbons = detect.curve_ribbons(comps, cand, prof, H, 300)
    assert not straight[0] and ribbons == []
    assert detect.regions_from_profiles(comps, cand, prof, H, 300) == []
    # and with room and ink enough the same profile is a ribbon 70 high
    straight, ribbons = detect.curve_ribbons(np.array([[0, 0, 160, 60, 6000]]), cand, prof, 400, 300)
    assert not straight[0] and len(ribbons) == 1 and ribbons[0][3] == 70 and ribbons[0][4] == 7


@pytest.mark.parametrize("name", ["sparse_arc", "tall_arc"])
def test_the_filter_scenes_are_curved_and_give_no_region(name):
    photo, kw, regions = regions_of(name)
    comps, cand, prof = tables_of(photo, **kw)
    straight, ribbons = detect.curve_ribbons(comps, cand, prof, *photo.shape[:2])
    assert len(comps) == 1 and not straight[0] and ribbons == [] and regions == []


def test_max_boxes_applies_to_the_mixed_list(capsys, monkeypatch):
    photo, kw, regions = regions_of("many_wide")
    comps, cand, prof = tables_of(photo, **kw)
    capsys.readouterr()
    capped = detect.regions_from_profiles(comps, cand, prof, *photo.shape[:2], name="p.png")
    out = capsys.readouterr().out
    monkeypatch.setattr(detect, "MAX_BOXES", 1 << 20)
    full = detect.regions_from_profiles(comps, cand, prof, *photo.shape[:2])
    assert len(full) > 256 and len(capped) == 256 and sum(len(q) > 4 for q in full) >= 1
    assert out == "detect: p.png: %d regions found, the 256 of largest area kept\n" % len(full)
    area = [int((q[:, 0].max() - q[:, 0].min()) * (q[:, 1].max() - q[:, 1].min())) for q in full]
    keep = sorted(sorted(range(len(full)), key=lambda i: -area[i])[:256])
    assert len(capped) == len(keep) and all(np.array_equal(a, full[i]) for a, i in zip(capped, keep))
    assert sum(len(q) > 4 for q in capped) >= 1      # (the polygon is among the largest)
    assert all(np.array_equal(a, b) for a, b in zip(capped, regions))


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_detect_curved", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_flag_needs_demo_detect_and_excludes_oriented():
    m = _main()
    for flags, msg in ((dict(demo_detect_curved=True), m.DEMO_DETECT_CURVED_NEEDS),
                       (dict(demo_detect_curved=True, demo_dir="d"), m.DEMO_DETECT_CURVED_NEEDS),
                       (dict(demo_detect_curved=True, demo_detect=True, demo_detect_oriented=True, demo_dir="d"), m.DEMO_DETECT_CURVED_OR_ORIENTED)):
        args = types.SimpleNamespace(**flags)
        with pytest.raises(ValueError) as e:
            m.demo_detect_curved_setting(args)
        assert "main.py: " + str(e.value) == msg
        with pytest.raises(SystemExit) as e:
            m.main(types.SimpleNamespace(), args)
        assert str(e.value) == msg and "\n" not in str(e.value)
    assert m.demo_detect_curved_setting(types.SimpleNamespace(demo_detect=True, demo_dir="d")) is False
    assert m.demo_detect_curved_setting(types.SimpleNamespace(demo_detect=True, demo_detect_curved=True, demo_dir="d")) is True


def test_the_command_line_knows_the_flag():
    import subprocess
    import sys
    m = _main()
    text = lambda s: " ".join(s.split())
    for extra, msg in ((["--demo_detect_curved"], m.DEMO_DETECT_CURVED_NEEDS),
                       (["--demo_detect", "--demo_detect_oriented", "--demo_detect_curved"], m.DEMO_DETECT_CURVED_OR_ORIENTED)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "d"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and text(r.stderr).endswith(msg[len("main.py: "):])


def test_detect_box_files_writes_the_regions(tmp_path, monkeypatch):
    """dataset.folder.detect_box_files(curved=True) asks ops.detect_curved_u8 (here: the restatement in its place, no GPU) and writes
    boxes and polygons into one file; without the flag it asks detect_text_u8 as before."""
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd.dataset import folder
    src = tmp_path / "photos"
    src.mkdir()
    photo = cc.photo()
    Image.fromarray(photo).save(str(src / "a.png"))
    asked = []

    def fake(find):
        def run(packed, offsets, sizes, gap=12, floor=24, names=None, **kw):
            asked.append((find.__name__, kw))
            a = packed.numpy()
            return [find(a[o:o + h * w * 3].reshape(h, w, 3), gap=gap, floor=floor)
                    for o, (h, w) in zip(np.asarray(offsets).tolist(), np.asarray(sizes).tolist())]
        return run

    monkeypatch.setattr(ops, "detect_curved_u8", fake(detect.detect_curved_np))
    monkeypatch.setattr(ops, "detect_text_u8", fake(detect.detect_text_np))
    n = folder.detect_box_files(str(src), str(tmp_path / "curved"), 4, "cpu", curved=True)
    assert n == 1 and asked == [("detect_curved_np", {})]
    with open(str(tmp_path / "curved" / "a.txt")) as f:
        assert f.read() == detect.region_lines(detect.detect_curved_np(photo))
    n = folder.detect_box_files(str(src), str(tmp_path / "plain"), 4, "cpu")
    assert asked[-1] == ("detect_text_np", {})
    with open(str(tmp_path / "plain" / "a.txt")) as f:
        assert f.read() == detect.box_lines(detect.detect_text_np(photo))
    with pytest.raises(ValueError):
        folder.detect_box_files(str(src), str(tmp_path / "x"), 4, "cpu", curved=True, oriented=True)
