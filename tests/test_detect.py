"""utils/detect.py, the integer restatement behind main.py --demo_detect, against independent references: scipy's grey morphology and
labelling, the textbook Otsu in float64, hand-written rows for the run-length smoothing, and a rendered photo end to end.  CPU only."""
import importlib.util
import os
import types

import numpy as np
import pytest
from scipy import ndimage

import detect_cases as cases
from dpmn_amd.utils import detect, quad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_working_map_is_the_box_mean_and_the_integer_luma():
    rng = np.random.RandomState(0)
    for H, W in ((5, 9), (1030, 1100), (1, 2050)):
        photo = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        r, hm, wm = detect.working_size(H, W)
        assert r == -(-max(H, W) // 1024) and (hm, wm) == (H // r, W // r)
        Y = detect.luma_map(photo)
        assert Y.shape == (hm, wm) and Y.dtype == np.uint8
        for y, x in ((0, 0), (hm - 1, wm - 1), (hm // 2, wm // 3)) if hm and wm else ():
            m = [int(np.floor(photo[y * r:(y + 1) * r, x * r:(x + 1) * r, c].astype(np.float64).mean() + 0.5)) for c in range(3)]
            assert Y[y, x] == (77 * m[0] + 150 * m[1] + 29 * m[2] + 128) >> 8
    assert detect.working_size(1, 2050) == (3, 0, 683)
    assert len(detect.detect_text_np(np.zeros((1, 2050, 3), np.uint8))) == 0


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 33), (70, 131)])
def test_gradient_equals_scipy_grey_morphology(shape):
    Y = np.random.RandomState(sum(shape)).randint(0, 256, shape).astype(np.uint8)
    g, hist = detect.gradient(Y)
    ref = ndimage.grey_dilation(Y, size=(3, 3), mode="nearest").astype(np.int64) - ndimage.grey_erosion(Y, size=(3, 3), mode="nearest")
    assert np.array_equal(g, ref)
    assert np.array_equal(hist, np.bincount(ref.reshape(-1), minlength=256))


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_labels_and_boxes_equal_scipy_label(density):
    s = np.random.RandomState(int(density * 10)).rand(61, 97) < density
    lab = detect.label(s)
    ref, n = ndimage.label(s, structure=np.ones((3, 3)))
    assert np.array_equal(lab >= 0, s)
    comps = detect.components(lab)
    assert len(comps) == n
    idx = np.arange(s.size).reshape(s.shape)
    for k, sl in enumerate(ndimage.find_objects(ref), 1):
        mine = lab[ref == k]
        least = idx[ref == k].min()
        assert (mine == least).all()      # one label per component, and it is the least linear index
        row = comps[np.searchsorted(np.unique(lab[lab >= 0]), least)]
        assert row.tolist() == [sl[1].start, sl[0].start, sl[1].stop, sl[0].stop, int((ref == k).sum())]


def _otsu_float(hist):
    p = hist.astype(np.float64) / hist.sum()
    i = np.arange(256, dtype=np.float64)
    var = np.full(256, -1.0)
    for t in range(256):
        w0, w1 = p[:t + 1].sum(), p[t + 1:].sum()
        if w0 > 0 and w1 > 0:
            var[t] = w0 * w1 * ((p[:t + 1] * i[:t + 1]).sum() / w0 - (p[t + 1:] * i[t + 1:]).sum() / w1) ** 2
    return var


def test_otsu_equals_the_textbook_between_class_variance():
    rng, checked = np.random.RandomState(5), 0
    for k in range(40):
        # (every bin is occupied: an empty bin gives its t the variance of the t before it, a tie that the reference cannot decide)
        hist = rng.randint(1, 1000, 256).astype(np.int64)
        hist[rng.randint(0, 256, 8)] += rng.randint(1, 50000, 8)
        var = _otsu_float(hist)
        top = np.sort(var)[-2:]
        if not top[1] - top[0] > 1e-9 * top[1]:      # (the float reference decides only where its maximum is unique)
            continue
        checked += 1
        assert detect.otsu(hist) == int(np.argmax(var))
    assert checked >= 30
    one = np.zeros(256, np.int64)
    one[200] = 7
    assert detect.otsu(one) == 0 and detect.threshold(one) == detect.FLOOR      # one bin: no t separates two classes
    two = np.zeros(256, np.int64)
    two[[0, 255]] = 5, 9
    assert detect.otsu(two) == 0 and detect.threshold(two, 24) == 24 and detect.threshold(two, 1) == 1      # the earliest t of a tie


def test_run_length_smoothing_on_hand_written_rows():
    def row(text):
        return np.array([[c == "#" for c in text]])
    gap = 3
    assert np.array_equal(detect.smooth_rows(row("#...#"), gap), row("#####"))            # a gap of exactly `gap` fills
    assert np.array_equal(detect.smooth_rows(row("#....#"), gap), row("#....#"))          # gap + 1 does not
    assert np.array_equal(detect.smooth_rows(row("..#.#.."), gap), row("..###.."))        # a gap at the row's edge is never filled
    assert np.array_equal(detect.smooth_rows(row(".#"), gap), row(".#"))
    assert np.array_equal(detect.smooth_rows(row("#.#....#..#"), gap), row("###....####"))
    assert np.array_equal(detect.smooth_rows(row("......"), gap), row("......"))
    # the columns after the rows, on the rows' result: the 1-gap of column 1 exists only once row 0 is filled
    b = np.array([[1, 0, 1], [0, 0, 0], [0, 1, 0]], bool)
    assert np.array_equal(detect.smooth(b, 1, 1), np.array([[1, 1, 1], [0, 1, 0], [0, 1, 0]], bool))
    assert np.array_equal(detect.smooth(b, 1, 1)[:, 0], [True, False, False])


def test_box_files_round_trip_through_the_reader(tmp_path):
    boxes = np.array([[0, 0, 7, 5], [12, 3, 480, 40], [5, 100, 6, 101]], np.int32)
    path = str(tmp_path / "p.txt")
    detect.write_boxes(path, boxes)
    got = quad.read_boxes(path)
    assert len(got) == 3
    for (q, label), (x0, y0, x1, y1) in zip(got, boxes.tolist()):
        quad.check_quad(q)
        assert label == " " and q.tolist() == [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    detect.write_boxes(path, np.zeros((0, 4), np.int32))
    assert open(path).read() == "" and quad.read_boxes(path) == []


def test_filters_padding_order_and_cap(capsys):
    # [x0, y0, x1, y1, area] in a 100 x 200 photo (r = 1): kept; too low; taller than half the map; too narrow; too sparse
    comps = [[10, 20, 50, 32, 300], [10, 40, 50, 45, 200], [60, 0, 199, 51, 7000], [0, 60, 11, 70, 110], [100, 60, 160, 80, 419]]
    got = detect.boxes_from_components(np.array(comps), 100, 200)
    assert got.tolist() == [[9, 19, 51, 33]] and got.dtype == np.int32            # padded by (12 + 5) // 10 = 1
    assert detect.boxes_from_components(np.array([[100, 60, 160, 80, 420]]), 100, 200).tolist() == [[98, 58, 162, 82]]
    # r = 2 and the clamp: a 2048-wide photo, a component at the map's corner
    assert detect.boxes_from_components(np.array([[0, 0, 40, 20, 800]]), 300, 2048).tolist() == [[0, 0, 84, 44]]
    many = np.array([[12 * k, 10 * (k % 7), 12 * k + 8 + k % 3, 10 * (k % 7) + 6, 48] for k in range(300)])
    got = detect.boxes_from_components(many, 200, 4000 // 4)      # (r = 1: W = 1000 clamps the boxes on the right)
    assert "300 regions found, the 256 of largest area kept" in capsys.readouterr().out
    assert len(got) == 256 and got.tolist() == sorted(got.tolist(), key=lambda b: (b[1], b[0], b[3], b[2]))


def test_three_rendered_words_come_back_as_three_boxes():
    photo, words = cases.word_photo()
    Y = detect.luma_map(photo).astype(int)
    assert Y.max() - Y.min() >= 100
    boxes = detect.detect_text_np(photo)
    print("boxes %s for textbboxes %s" % (boxes.tolist(), words))
    assert len(boxes) == 3
    for tb in words:
        holds = [b for b in boxes.tolist() if b[0] <= tb[0] and b[1] <= tb[1] and b[2] >= tb[2] and b[3] >= tb[3]]
        assert len(holds) == 1, tb
        b = holds[0]
        assert (b[2] - b[0]) * (b[3] - b[1]) <= 2 * (tb[2] - tb[0]) * (tb[3] - tb[1]), (b, tb)


def test_synthetic_cases_have_the_structure_they_are_named_for():
    assert len(detect.detect_text_np(cases.flat())) == 0
    for photo, kw in ((cases.all_foreground(), {}), (cases.checkerboard(), dict(gap=1, vgap=1)), (cases.serpentine(), dict(gap=1, vgap=1))):
        g, hist, s, lab = detect.detect_maps_np(photo, **kw)
        assert s.any() and len(np.unique(lab[lab >= 0])) == 1 and lab[lab >= 0][0] == np.flatnonzero(s)[0]
    assert detect.detect_maps_np(cases.all_foreground())[2].all()
    s = detect.detect_maps_np(cases.checkerboard(), gap=1, vgap=1)[2]
    assert ndimage.label(s)[1] > 100      # (4-connectivity leaves the cells alone)
    comps = detect.components(detect.detect_maps_np(cases.bricks(200, 300), gap=1)[3])
    assert len(comps) == len(range(2, 194, 9)) * len(range(2, 290, 12))


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_detect", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("flags, message", [
    (dict(demo_detect=True), "DEMO_DETECT_NEEDS_DIR"),
    (dict(demo_detect=True, demo_dir="d", demo_boxes="b"), "DEMO_DETECT_OR_BOXES"),
    (dict(demo_detect=True, demo_dir="d", demo_polygons=True), "DEMO_DETECT_OR_BOXES"),
    (dict(demo_detect=True, demo_dir="d", demo_detect_gap=0), "DEMO_DETECT_GAP"),
    (dict(demo_detect=True, demo_dir="d", demo_detect_gap=65), "DEMO_DETECT_GAP"),
    (dict(demo_detect=True, demo_dir="d", demo_detect_floor=0), "DEMO_DETECT_FLOOR"),
    (dict(demo_detect=True, demo_dir="d", demo_detect_floor=256), "DEMO_DETECT_FLOOR"),
    (dict(demo_dir="d", demo_detect_gap=5), "DEMO_DETECT_FLAGS_NEED"),
    (dict(demo_dir="d", demo_detect_floor=5), "DEMO_DETECT_FLAGS_NEED"),
])
def test_bad_flag_combinations_raise(flags, message):
    m = _main()
    args = types.SimpleNamespace(**flags)
    with pytest.raises(ValueError) as e:
        m.demo_detect_setting(args)
    assert "main.py: " + str(e.value) == getattr(m, message)
    with pytest.raises(SystemExit) as e:      # main() ends there, before it looks at anything else
        m.main(types.SimpleNamespace(), args)
    assert str(e.value) == getattr(m, message)


def test_good_flag_combinations_pass():
    m = _main()
    assert m.demo_detect_setting(types.SimpleNamespace(demo_dir="d")) is None
    assert m.demo_detect_setting(types.SimpleNamespace(demo_detect=True, demo_dir="d")) == (12, 24)
    assert m.demo_detect_setting(types.SimpleNamespace(demo_detect=True, demo_dir="d", demo_paste=True, demo_tile=True, demo_detect_gap=64,
                                                       demo_detect_floor=255)) == (64, 255)
    with pytest.raises(SystemExit) as e:      # --demo_paste still needs box files from somewhere
        m.main(types.SimpleNamespace(), types.SimpleNamespace(demo_dir="d", demo_paste=True))
    assert str(e.value) == m.DEMO_PASTE_NEEDS_BOXES
