"""The locally adaptive threshold of the text detector (utils/detect.py, local = C; main.py --demo_detect_local) on the CPU: the cells,
the integer interpolation between their centres, the degenerate case of one cell (the shipped global recipe, byte for byte), the scene
that shows what the feature is for, and the argument checks."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import detect_cases as cases
import detect_local_cases as lc
from dpmn_amd.utils import detect

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _main():
    import importlib
    return importlib.import_module("main")


def _same_maps(a, b):
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype and np.array_equal(u, v)


@pytest.mark.parametrize("h,w,local", [(1, 1, 1024), (5, 300, 1024), (130, 257, 1024), (1025, 40, 1024), (300, 300, 1024), (20, 30, 32)])
def test_one_cell_is_the_global_recipe(h, w, local):
    photo = cases.speckle(h, w, 3)
    assert detect.working_size(h, w)[0] == (2 if h == 1025 else 1)
    _same_maps(detect.detect_maps_np(photo, local=local), detect.detect_maps_np(photo))
    assert np.array_equal(detect.detect_text_np(photo, local=local), detect.detect_text_np(photo))
    assert np.array_equal(detect.detect_oriented_np(photo, local=local), detect.detect_oriented_np(photo))
    g, hist = detect.gradient(detect.luma_map(photo))
    t = detect.cell_thresholds(g, local, 24)
    assert t.shape == (1, 1) and t[0, 0] == detect.threshold(hist, 24)
    assert (detect.threshold_map(t, g.shape[0], g.shape[1], local) == detect.threshold(hist, 24)).all()


@pytest.mark.parametrize("C", [32, 128])
def test_cell_edges_cover_the_axis_with_cells_that_are_not_empty(C):
    for size in range(1, 1101):
        e = detect.cell_edges(size, C)
        w = np.diff(e)
        assert e[0] == 0 and e[-1] == size and len(w) == -(-size // C) and w.min() >= 1 and w.max() <= C
        assert w.max() - w.min() <= 1 and (len(w) == 1 or 2 * w.min() >= C - 1)      # balanced: about C / 2 at the least
    assert detect.cell_edges(0, C) == [0]


def _threshold_map_slow(t, hm, wm, C):
    """The definition pixel by pixel, in Python integers."""
    def axis(x, size):
        e = detect.cell_edges(size, C)
        n = len(e) - 1
        if n == 1:
            return 0, 0, 1, 0, 1
        c = [e[i] + e[i + 1] for i in range(n)]
        p = min(max(2 * x + 1, c[0]), c[-1])
        k = min(max(i for i in range(n) if c[i] <= p), n - 2)
        return k, k + 1, c[k + 1] - p, p - c[k], c[k + 1] - c[k]

    out = np.empty((hm, wm), np.int32)
    ax = [axis(x, wm) for x in range(wm)]
    for y in range(hm):
        ky, ky1, wy0, wy1, Dy = axis(y, hm)
        for x in range(wm):
            kx, kx1, wx0, wx1, Dx = ax[x]
            s = (wy0 * wx0 * int(t[ky][kx]) + wy0 * wx1 * int(t[ky][kx1]) + wy1 * wx0 * int(t[ky1][kx]) + wy1 * wx1 * int(t[ky1][kx1]))
            out[y, x] = (2 * s + Dy * Dx) // (2 * Dy * Dx)
    return out


def test_threshold_map_is_the_definition_pixel_by_pixel():
    rng = np.random.default_rng(5)
    for hm, wm, C in ((130, 257, 32), (20, 257, 32), (130, 30, 32), (40, 70, 33)):
        ny, nx = -(-hm // C), -(-wm // C)
        for lo, hi in ((24, 256), (1, 256), (200, 203)):
            t = rng.integers(lo, hi, (ny, nx)).astype(np.int32)
            T = detect.threshold_map(t, hm, wm, C)
            assert T.dtype == np.int32 and np.array_equal(T, _threshold_map_slow(t, hm, wm, C)), (hm, wm, C)


def test_threshold_map_at_the_centres_between_them_and_outside():
    rng = np.random.default_rng(6)
    hm, wm, C, floor = 135, 261, 32, 24      # 5 cells of 27 by 9 cells of 29: odd widths, so every cell's centre is a pixel's centre
    ey, ex = detect.cell_edges(hm, C), detect.cell_edges(wm, C)
    t = rng.integers(floor, 256, (len(ey) - 1, len(ex) - 1)).astype(np.int32)
    T = detect.threshold_map(t, hm, wm, C)
    assert T.min() >= t.min() >= floor and T.max() <= t.max()
    # a cell whose doubled centre e_i + e_{i+1} is odd has a pixel whose centre is the cell's: there T is the cell's own threshold
    hit = 0
    for i in range(len(ey) - 1):
        for j in range(len(ex) - 1):
            cy, cx = ey[i] + ey[i + 1], ex[j] + ex[j + 1]
            if cy % 2 and cx % 2:
                assert T[cy // 2, cx // 2] == t[i, j]
                hit += 1
    assert hit == t.size
    # constant outside the outermost centres: rows above the first centre repeat the row of the first centre, and so on
    y_first, y_last = (ey[0] + ey[1]) // 2, (ey[-2] + ey[-1] + 1) // 2
    x_first, x_last = (ex[0] + ex[1]) // 2, (ex[-2] + ex[-1] + 1) // 2
    assert (T[:y_first] == T[y_first - 1]).all() and (T[y_last:] == T[y_last]).all()
    assert (T[:, :x_first] == T[:, x_first - 1:x_first]).all() and (T[:, x_last:] == T[:, x_last:x_last + 1]).all()
    assert T[0, 0] == t[0, 0] and T[-1, -1] == t[-1, -1] and T[0, -1] == t[0, -1] and T[-1, 0] == t[-1, 0]
    with pytest.raises(ValueError):
        detect.threshold_map(t[:-1], hm, wm, C)


def test_cell_thresholds_are_otsu_of_every_cell():
    g = detect.gradient(detect.luma_map(cases.speckle(130, 257, 3)))[0]
    t = detect.cell_thresholds(g, 32, 24)
    ey, ex = detect.cell_edges(130, 32), detect.cell_edges(257, 32)
    assert t.shape == (5, 9) and t.dtype == np.int32 and t.min() >= 24 and len(np.unique(t)) > 3
    for i, j in ((0, 0), (2, 4), (4, 8)):
        h = np.bincount(g[ey[i]:ey[i + 1], ex[j]:ex[j + 1]].reshape(-1), minlength=256)
        assert t[i, j] == max(detect.otsu(h) + 1, 24)
    assert detect.cell_thresholds(np.zeros((0, 683), np.uint8), 32, 24).shape == (0, 22)


def test_the_scene_one_threshold_loses_the_faint_word_and_cell_thresholds_find_it():
    photo = lc.scene()
    g, hist = detect.gradient(detect.luma_map(photo))
    assert detect.threshold(hist) == 92
    one = detect.detect_text_np(photo)
    assert one.tolist() == [[27, 89, 134, 124]]
    two = detect.detect_text_np(photo, local=128)
    assert len(two) == 2 and two[0].tolist() == one[0].tolist()
    x0, y0, x1, y1 = lc.faint_ink_box()
    assert two[1][0] <= x0 and two[1][1] <= y0 and two[1][2] >= x1 and two[1][3] >= y1      # the faint word's ink, whole
    assert two[1][2] - two[1][0] <= (x1 - x0) + 16 and two[1][3] - two[1][1] <= (y1 - y0) + 16      # and little else
    t = detect.cell_thresholds(g, 128, 24)
    assert t.shape == (4, 5) and t[0, 0] > 92 and (t[2:, 2:] <= 45).all() and (t == 24).sum() >= 12
    assert len(detect.detect_oriented_np(photo)) == 1 and len(detect.detect_oriented_np(photo, local=128)) == 2


@pytest.mark.parametrize("local", [31, 1025, -1, 1])
def test_a_cell_side_outside_its_range_is_refused(local):
    photo = cases.flat()
    for f in (detect.detect_maps_np, detect.detect_text_np, detect.detect_oriented_np):
        with pytest.raises(ValueError):
            f(photo, local=local)
    with pytest.raises(ValueError):
        detect.check_local(local)
    assert detect.check_params() == (12, 2, 24) and detect.check_local(0) == 0 and detect.check_local(32) == 32


def test_the_flag_needs_demo_detect_and_a_side_in_range():
    m = _main()
    assert m.demo_detect_local_setting(types.SimpleNamespace(demo_detect=True, demo_dir="d")) == 0
    assert m.demo_detect_local_setting(types.SimpleNamespace(demo_detect=True, demo_dir="d", demo_detect_local=128)) == 128
    for flags, message in ((dict(demo_detect_local=128), m.DEMO_DETECT_LOCAL_NEEDS), (dict(demo_detect_local=128, demo_dir="d"), m.DEMO_DETECT_LOCAL_NEEDS),
                           (dict(demo_detect=True, demo_dir="d", demo_detect_local=31), m.DEMO_DETECT_LOCAL_RANGE),
                           (dict(demo_detect=True, demo_dir="d", demo_detect_local=1025), m.DEMO_DETECT_LOCAL_RANGE)):
        args = types.SimpleNamespace(**flags)
        with pytest.raises(ValueError) as e:
            m.demo_detect_local_setting(args)
        assert "main.py: " + str(e.value) == message
        with pytest.raises(SystemExit) as e:
            m.main(types.SimpleNamespace(), args)
        assert str(e.value) == message and "\n" not in str(e.value)


def test_the_command_line_refuses_the_flag_without_demo_detect():
    m = _main()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "d", "--demo_detect_local"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and " ".join(r.stderr.split()).endswith(m.DEMO_DETECT_LOCAL_NEEDS[len("main.py: "):])


def test_detect_box_files_passes_the_cell_side_on(tmp_path, monkeypatch):
    """dataset.folder.detect_box_files(local=128) asks ops.detect_text_u8(local=128) (here: the restatement in its place, no GPU): two
    lines for the scene; without it the call is the one it was and writes one."""
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd.dataset import folder
    src = tmp_path / "photos"
    src.mkdir()
    Image.fromarray(lc.scene()).save(str(src / "scene.png"))
    seen = []

    def fake(packed, offsets, sizes, gap=12, vgap=2, floor=24, names=None, **kw):
        seen.append(kw)
        (off, h, w), = [(int(o), int(a), int(b)) for o, (a, b) in zip(offsets, sizes)]
        return [detect.detect_text_np(packed.numpy()[off:off + h * w * 3].reshape(h, w, 3), gap, vgap, floor, **kw)]

    monkeypatch.setattr(ops, "detect_text_u8", fake)
    assert folder.detect_box_files(str(src), str(tmp_path / "l"), 2, "cpu", local=128) == 2
    assert folder.detect_box_files(str(src), str(tmp_path / "g"), 2, "cpu") == 1
    assert seen == [{"local": 128}, {}]
    with open(str(tmp_path / "l" / "scene.txt")) as f:
        assert len(f.read().splitlines()) == 2
