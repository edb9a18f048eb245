"""The semantics of the box path (dpmn_amd/utils/quad.py, dataset/folder.py box_batches), no GPU: quad_crop_np against PIL's own
Image.transform(PERSPECTIVE, BICUBIC), byte for byte, live and against PIL's bytes recorded in tests/golden/quad_crop.npz (by
`write_fixture`, run once: `PYTHONPATH=. python tests/test_quad.py`), so a Pillow with another rounding shows as a disagreement between PIL and the
file; the box-file reader, the size / check / coefficients of a quad, the host half of the loader on a temp folder, and main.py's
refusal of --demo_boxes without --demo_dir."""
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from dpmn_amd.utils import quad, resize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "quad_crop.npz")

PHOTO_SIZES = [(1, 1), (2, 3), (3, 2), (7, 31), (40, 89)]      # (H, W); in the first three every tap is clipped

AXIS = (3, 5, 70, 30)      # x0, y0, x1, y1 of the axis-aligned integer quad in the 40 x 89 photo
# (name, photo, quad tl tr br bl, output (h, w) or None for quad_size's)
CASES = [
    ("one_pixel", 0, [(0, 0), (1, 0), (1, 1), (0, 1)], (1, 1)),
    ("one_pixel_enlarged", 0, [(-0.5, -0.25), (1.5, 0), (1.25, 1.5), (-0.25, 1.25)], (9, 1)),
    ("tiny_2x3_slanted", 1, [(0.2, 0.1), (2.9, 0.4), (2.7, 1.9), (0.1, 1.6)], (16, 64)),
    ("tiny_3x2_wide_row", 2, [(-1, -0.5), (3, 0.5), (2.5, 3.5), (-0.5, 2.75)], (1, 70)),
    ("small_7x31_slanted", 3, [(2.5, 1.25), (28.75, 0.5), (29.5, 5.5), (3.25, 6.5)], None),
    ("small_7x31_column", 3, [(10, -1), (14, 0), (13, 8), (9, 7)], (9, 1)),
    ("axis_aligned", 4, [(AXIS[0], AXIS[1]), (AXIS[2], AXIS[1]), (AXIS[2], AXIS[3]), (AXIS[0], AXIS[3])], None),
    ("slanted", 4, [(10.3, 8.7), (75.2, 2.1), (78.9, 21.4), (13.6, 29.8)], None),
    ("foreshortened", 4, [(5, 12), (80, 2), (84, 38), (6, 24)], (16, 64)),
    ("half_outside", 4, [(-30, -15), (50.5, -10), (48, 22.25), (-28, 20)], None),
    ("one_tile_8x32", 4, [(20, 10), (60, 12), (59, 25), (19, 22)], (8, 32)),
    ("past_one_tile_9x33", 4, [(20, 10), (60, 12), (59, 25), (19, 22)], (9, 33)),
    ("wholly_outside", 4, [(100, 50), (140, 52), (139, 65), (99, 62)], (5, 40)),
]


def photos(seed=11):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in PHOTO_SIZES]


def case_regions(names=None):
    """[(name, (photo, h, w, coeffs))] of CASES (all, or the named ones in the order given)."""
    by_name = {c[0]: c for c in CASES}
    out = []
    for name, b, q, hw in (CASES if names is None else [by_name[n] for n in names]):
        quad.check_quad(q)
        h, w = hw or quad.quad_size(q)
        out.append((name, (b, h, w, quad.quad_coeffs(q, w, h))))
    return out


def pil_crop(photo, h, w, coeffs):
    return np.asarray(Image.fromarray(photo).transform((w, h), Image.PERSPECTIVE, tuple(float(c) for c in coeffs), Image.BICUBIC))


def write_fixture():
    imgs = photos()
    arrays = {"photo_%d" % i: im for i, im in enumerate(imgs)}
    for name, (b, h, w, a) in case_regions():
        arrays["coeffs_" + name] = a
        arrays["expected_" + name] = pil_crop(imgs[b], h, w, a)
    np.savez_compressed(FIXTURE, **arrays)
    print("wrote %s (%d bytes)" % (FIXTURE, os.path.getsize(FIXTURE)))


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_the_fixture_holds_these_photos_and_coefficients(recorded):
    for i, im in enumerate(photos()):
        assert np.array_equal(recorded["photo_%d" % i], im)
    for name, (b, h, w, a) in case_regions():
        assert recorded["expected_" + name].shape == (h, w, 3), name
        assert np.array_equal(recorded["coeffs_" + name], a), name      # the same 8 doubles, bit for bit


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_equals_pil_and_the_recorded_bytes(recorded, name):
    imgs = photos()
    (_, (b, h, w, _)), = case_regions([name])
    a = recorded["coeffs_" + name]
    got, = quad.quad_crop_np(imgs, [(b, h, w, a)])
    live = pil_crop(imgs[b], h, w, a)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    d_live, d_file, d_pil = (int((x != y).sum()) for x, y in ((got, live), (got, recorded["expected_" + name]), (live, recorded["expected_" + name])))
    print("%s %d x %d: %d bytes differ from PIL, %d from the file, PIL and the file differ in %d" % (name, h, w, d_live, d_file, d_pil))
    assert d_pil == 0, "this Pillow does not write the recorded bytes"
    assert d_live == 0 and d_file == 0


def test_what_the_cases_show(recorded):
    imgs = photos()
    x0, y0, x1, y1 = AXIS
    assert np.array_equal(recorded["coeffs_axis_aligned"], [1, 0, x0, 0, 1, y0, 0, 0])
    assert np.array_equal(recorded["expected_axis_aligned"], imgs[4][y0:y1, x0:x1])      # the photo's own pixels
    assert int(recorded["expected_wholly_outside"].max()) == 0
    half = recorded["expected_half_outside"]
    assert int(half[:10].max()) == 0 and int(half[:, :25].max()) == 0 and half[-1, -1].any()      # black fill on two sides
    assert np.array_equal(recorded["expected_one_pixel"], imgs[0])
    # every tap is the one pixel: its value where the quad lies over the photo, black beyond
    assert {tuple(p) for p in recorded["expected_one_pixel_enlarged"].reshape(-1, 3)} == {tuple(imgs[0][0, 0]), (0, 0, 0)}


def test_restatement_on_random_quads_against_pil():
    rng = np.random.RandomState(5)
    total = differ = 0
    for _ in range(12):
        H, W = int(rng.randint(5, 60)), int(rng.randint(5, 120))
        ph = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        ww, hh, th = rng.uniform(4, W + 10), rng.uniform(3, H + 10), rng.uniform(-0.5, 0.5)
        base = np.array([[-ww / 2, -hh / 2], [ww / 2, -hh / 2], [ww / 2, hh / 2], [-ww / 2, hh / 2]])
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        q = base @ rot.T + [rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)] + rng.uniform(-0.1, 0.1, (4, 2)) * min(ww, hh)
        quad.check_quad(q)
        h, w = quad.quad_size(q)
        a = quad.quad_coeffs(q, w, h)
        got, = quad.quad_crop_np([ph], [(0, h, w, a)])
        total += got.size
        differ += int((got != pil_crop(ph, h, w, a)).sum())
    print("random quads: %d of %d bytes differ from PIL" % (differ, total))
    assert differ == 0 and total > 20000


def test_restatement_rejects_what_it_cannot_crop():
    ph = photos()[3]
    a = quad.quad_coeffs(CASES[4][2], 20, 5)
    for bad in ([(1, 5, 20, a)], [(-1, 5, 20, a)], [(0, 0, 20, a)], [(0, 5, resize.MAX_SIDE + 1, a)], [(0, 5, 20, a[:7])]):
        with pytest.raises(ValueError):
            quad.quad_crop_np([ph], bad)
    # a non-finite source position counts as outside
    got, = quad.quad_crop_np([ph], [(0, 2, 2, [np.nan, 0, 0, 0, 1, 0, 0, 0])])
    assert int(got.max()) == 0


def test_read_boxes(tmp_path, capsys):
    p = tmp_path / "gt.txt"
    p.write_bytes("\ufeff1,2,30,4,31,14,2,12,hello\r\n"
                  "\n"
                  " 1.5 , 2.25,30,4 ,31.0,14,2,1e1,a, b,,c\n"
                  "5,5,9,5,9,8,5,8\n"
                  "5,5,9,5,9,8,5,8,\n"
                  "5,5,9,5,9,8,5,8,###\n"
                  "   \n"
                  "5,5,9,five,9,8,5,8,word\n"
                  "5,5,9,5,9,8\n"
                  "7,7,11,7,11,10,7,10,café\n".encode("utf-8"))
    boxes = quad.read_boxes(str(p))
    out = capsys.readouterr().out.strip().splitlines()
    assert [label for _, label in boxes] == ["hello", "a, b,,c", " ", " ", "café"]
    assert boxes[0][0].dtype == np.float64 and boxes[0][0].tolist() == [[1, 2], [30, 4], [31, 14], [2, 12]]
    assert boxes[1][0].tolist() == [[1.5, 2.25], [30, 4], [31, 14], [2, 10]]
    # the two lines that do not parse: one printed line each, naming the file and the line; ### says nothing
    assert len(out) == 2 and all(str(p) in line for line in out) and "line 8" in out[0] and "line 9" in out[1]
    # the numbers of the kept lines among the non-empty ones: skipped lines keep theirs
    assert [(k, lineno) for k, lineno, _, _ in quad.numbered_boxes(str(p))] == [(0, 1), (1, 3), (2, 4), (3, 5), (7, 10)]
    capsys.readouterr()
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    assert quad.read_boxes(str(empty)) == [] and capsys.readouterr().out == ""


def test_quad_size():
    assert quad.quad_size([(0, 0), (10, 0), (10, 4), (0, 4)]) == (4, 10)
    assert quad.quad_size([(0, 0), (10, 0), (12, 5), (0, 4)]) == (5, 11)      # w: (10 + sqrt(145)) / 2 = 11.02, h: (4 + sqrt(29)) / 2 = 4.69
    assert quad.quad_size([(0, 0), (2.5, 0), (2.5, 1), (0, 1)]) == (1, 3)     # half up
    assert quad.quad_size([(0, 0), (0.2, 0), (0.2, 0.3), (0, 0.3)]) == (1, 1)
    assert quad.quad_size([(0, 0), (1e6, 0), (1e6, 20000), (0, 20000)]) == (resize.MAX_SIDE, resize.MAX_SIDE)


def test_check_quad():
    quad.check_quad([(0, 0), (10, 0), (10, 4), (0, 4)])
    quad.check_quad([(-50, -3), (10, 0), (12, 5), (-40, 9)])                  # partly outside any photo: fine
    quad.check_quad(np.array([0, 0, 10, 0, 10, 4, 0, 4]))                     # the flat form of a box file's line
    for name, bad in (("anticlockwise", [(0, 0), (0, 4), (10, 4), (10, 0)]),
                      ("self-crossing", [(0, 0), (10, 0), (0, 4), (10, 4)]),
                      ("concave", [(0, 0), (10, 0), (3, 1), (0, 4)]),
                      ("collinear", [(0, 0), (5, 0), (10, 0), (0, 4)]),
                      ("zero area", [(0, 0), (10, 0), (10, 0), (0, 0)]),
                      ("area below 1", [(0, 0), (0.9, 0), (0.9, 0.9), (0, 0.9)]),
                      ("nan", [(0, 0), (10, np.nan), (10, 4), (0, 4)]),
                      ("inf", [(0, 0), (np.inf, 0), (10, 4), (0, 4)])):
        with pytest.raises(ValueError):
            quad.check_quad(bad)
            pytest.fail("%s accepted" % name)
    with pytest.raises(ValueError):
        quad.check_quad([(0, 0), (10, 0), (10, 4)])


def test_quad_coeffs_map_the_corners():
    for _, _, q, hw in CASES:
        h, w = hw or quad.quad_size(q)
        a = quad.quad_coeffs(q, w, h)
        assert a.dtype == np.float64 and a.shape == (8,)
        for (u, v), (X, Y) in zip(((0, 0), (w, 0), (w, h), (0, h)), q):
            den = a[6] * u + a[7] * v + 1
            assert den > 0
            assert abs((a[0] * u + a[1] * v + a[2]) / den - X) <= 1e-9 and abs((a[3] * u + a[4] * v + a[5]) / den - Y) <= 1e-9
    with pytest.raises(ValueError):
        quad.quad_coeffs(CASES[0][2], 0, 4)
    with pytest.raises(ValueError):
        quad.quad_coeffs([(0, 0), (5, 0), (10, 0), (0, 4)], 10, 4)             # three corners on a line: no transform
    with pytest.raises(ValueError):
        quad.quad_coeffs([(0, 0), (10, 0), (3, 1), (0, 4)], 10, 4)             # concave: the denominator changes sign


def _folder(tmp_path):
    """Photos a (boxes in a.txt), b (gt_b.txt), c (no box file), d (only a ### line), e (not an image) and the box folder."""
    src, box = tmp_path / "photos", tmp_path / "boxes"
    src.mkdir()
    box.mkdir()
    rng = np.random.RandomState(2)
    shapes = {"a.png": (30, 50), "b.png": (24, 64), "c.png": (10, 10), "d.png": (10, 10)}
    imgs = {}
    for name, hw in shapes.items():
        imgs[name] = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
        Image.fromarray(imgs[name]).save(str(src / name))
    (src / "e.png").write_bytes(b"not an image")
    (box / "a.txt").write_text("2,3,40,3,40,15,2,15,first\n"
                               "0,0,9,0,9,9,0,9,###\n"
                               "1,2,3\n"
                               "2,3,2,15,40,15,40,3,anticlockwise\n"
                               "\n"
                               "5.5,4,45,8.5,44,20,4,16,second, with a comma\n")
    (box / "gt_b.txt").write_text("0,0,64,0,64,24,0,24\n1,1,20,2,19,12,0,10,x\n30,5,60,4,62,20,31,22,y\n")
    (box / "d.txt").write_text("0,0,9,0,9,9,0,9,###\n")
    (box / "e.txt").write_text("0,0,9,0,9,9,0,9,e\n")
    return str(src), str(box), imgs


def test_box_batches(tmp_path, capsys):
    from dpmn_amd.dataset.folder import box_batches
    src, box, imgs = _folder(tmp_path)
    batches = list(box_batches(src, box, 2))
    out = capsys.readouterr().out.strip().splitlines()
    # a photo is never split: a's 2 regions close the first batch, b's 3 are one batch
    assert [b[0] for b in batches] == [["a_000", "a_004"], ["b_000", "b_001", "b_002"]]
    assert [b[1] for b in batches] == [["first", "second, with a comma"], [" ", "x", "y"]]
    for (names, labels, packed, meta, regions), photo in zip(batches, ("a.png", "b.png")):
        assert packed.dtype.is_floating_point is False and meta.tolist() == [[0] + list(imgs[photo].shape[:2])]
        assert np.array_equal(packed.numpy().reshape(imgs[photo].shape), imgs[photo])
        assert [r[0] for r in regions] == [0] * len(names)
    (_, h, w, a), = batches[0][4][:1]
    assert (h, w) == (12, 38) and np.array_equal(a, [1, 0, 2, 0, 1, 3, 0, 0])
    assert batches[1][4][0][1:3] == (24, 64)
    # one printed line per skipped line, region and photo
    assert len(out) == 5
    assert "a.txt" in out[0] and "line 3" in out[0]                                        # does not parse (utils.quad)
    assert "a.png" in out[1] and "a.txt line 4" in out[1]                                  # refused by check_quad
    assert out[2].startswith("folder: skipping c.png") and "no box file" in out[2]
    assert out[3].startswith("folder: skipping d.png") and "no usable region" in out[3]
    assert out[4].startswith("folder: skipping e.png")
    # a larger batch size: both photos in one batch, the regions name their photo
    (names, labels, packed, meta, regions), = list(box_batches(src, box, 4))
    assert names == ["a_000", "a_004", "b_000", "b_001", "b_002"] and [r[0] for r in regions] == [0, 0, 1, 1, 1]
    assert meta.tolist() == [[0, 30, 50], [30 * 50 * 3, 24, 64]]
    # the restatement on what the loader yields: the axis-aligned regions are the photos' own pixels
    flat = packed.numpy()
    photos_ = [flat[off:off + ph * pw * 3].reshape(ph, pw, 3) for off, ph, pw in meta.tolist()]
    crops = quad.quad_crop_np(photos_, regions)
    assert np.array_equal(crops[0], imgs["a.png"][3:15, 2:40]) and np.array_equal(crops[2], imgs["b.png"])
    # `check` refuses a region by its size; the region's photo goes with its last region
    capsys.readouterr()

    def no_wide(h, w, name):
        if w > 3 * h:
            raise ValueError("%s is too wide" % name)
    assert [b[0] for b in box_batches(src, box, 8, check=no_wide)] == [["b_000", "b_001", "b_002"]]
    assert "too wide" in capsys.readouterr().out
    with pytest.raises(ValueError):
        list(box_batches(src, box, 0))
    (tmp_path / "none").mkdir()
    with pytest.raises(FileNotFoundError):
        list(box_batches(str(tmp_path / "none"), box, 2))


def test_box_files_may_lie_beside_the_photos(tmp_path, capsys):
    from dpmn_amd.dataset.folder import box_batches
    Image.fromarray(photos()[4]).save(str(tmp_path / "p.png"))
    (tmp_path / "p.txt").write_text("3,5,70,5,70,30,3,30,w\n")
    (names, labels, _, _, regions), = list(box_batches(str(tmp_path), str(tmp_path), 2))
    assert names == ["p_000"] and labels == ["w"] and regions[0][1:3] == (25, 67) and capsys.readouterr().out == ""


def test_demo_boxes_without_demo_dir_is_refused():
    spec = importlib.util.spec_from_file_location("dpmn_main_quad", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(demo_boxes="boxes", demo_dir=None))
    assert str(e.value).startswith("main.py: --demo_boxes needs --demo_dir") and "\n" not in str(e.value)
    # the command line: the argument parser reports it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_boxes", "boxes"], capture_output=True, text=True)
    assert r.returncode == 2 and "error: --demo_boxes needs --demo_dir" in r.stderr


if __name__ == "__main__":
    write_fixture()
