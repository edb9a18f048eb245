"""The semantics of the tiled demo path (dpmn_amd/utils/tile.py), no GPU: the plan arithmetic, resize_windows_np against PIL itself,
stitch_np against the identity and against hand-computed blend bytes, and main.py's refusal of --demo_tile without --demo_dir."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from dpmn_amd.utils import display, resize, tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w) -> (w_line, windows): one window untouched, one window stretched, two windows that overlap almost fully, a text line, a sign
SIZES = [((16, 64), 64, 1), ((33, 70), 64, 1), ((9, 40), 71, 2), ((20, 300), 240, 5), ((7, 500), 1143, 24)]


def line_images(seed=3, kind=0):
    """One image per entry of SIZES: kind 0 random bytes, kind 1 all 0, kind 2 all 255."""
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, hw + (3,)).astype(np.uint8) if kind == 0 else np.full(hw + (3,), 255 * (kind - 1), np.uint8)
            for hw, _, _ in SIZES]


@pytest.mark.parametrize("hw,w_line,n", SIZES)
def test_line_width_and_window_plan(hw, w_line, n):
    assert tile.line_width(*hw) == w_line
    starts = tile.window_plan(w_line)
    assert len(starts) == n and starts[0] == 0 and starts[-1] == w_line - 64
    assert all(a <= b for a, b in zip(starts, starts[1:]))
    assert all(b - a <= tile.STRIDE for a, b in zip(starts, starts[1:]))
    covered = np.zeros(w_line, bool)
    for x0 in starts:
        assert 0 <= x0 and x0 + 64 <= w_line
        covered[x0:x0 + 64] = True
    assert covered.all()


def test_plan_of_every_width_up_to_three_windows_per_column():
    most = 0
    for w_line in list(range(64, 400)) + [1143, 4000, resize.MAX_SIDE]:
        starts = tile.window_plan(w_line)
        d = w_line - 64
        assert len(starts) == (1 if d == 0 else -(-d // 48) + 1) and starts[0] == 0 and starts[-1] == d
        assert all(0 <= b - a <= 48 for a, b in zip(starts, starts[1:]))
        cover = np.zeros(w_line, int)
        for x0 in starts:
            cover[x0:x0 + 64] += 1
        assert cover.min() >= 1
        most = max(most, cover.max())
    assert most == 3
    assert tile.window_plan(65) == [0, 1]


def test_line_width_limits():
    assert tile.line_width(1, 512) == resize.MAX_SIDE
    for h, w in ((1, 513), (0, 5), (5, 0), (resize.MAX_SIDE + 1, 5), (16, resize.MAX_SIDE + 1)):
        with pytest.raises(ValueError):
            tile.line_width(h, w)
    assert tile.line_width(32, 129) == 65 and tile.line_width(32, 130) == 65 and tile.line_width(32, 131) == 66      # half up
    with pytest.raises(ValueError):
        tile.window_plan(63)
    with pytest.raises(ValueError):
        tile.plan_lines([(0, 0), (0, 7), (0, 3)])           # a start that decreases
    with pytest.raises(ValueError):
        tile.plan_lines([(0, 0), (2, 0)])                   # an image left out
    assert tile.plan_lines([(0, 0), (1, 0), (1, 7), (2, 0)]) == [(0, 1, 64), (1, 2, 71), (3, 1, 64)]


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["random", "zeros", "ones"])
def test_resize_windows_np_equals_pil(kind):
    imgs = line_images(kind=kind)
    windows, plan = tile.resize_windows_np(imgs, (16, 64))
    assert windows.dtype == np.uint8 and windows.shape == (sum(n for _, _, n in SIZES), 16, 64, 3) and len(plan) == windows.shape[0]
    assert [b for b, _ in plan] == [b for b, (_, _, n) in enumerate(SIZES) for _ in range(n)]
    lines = [np.asarray(Image.fromarray(a).resize((w_line, 16), Image.BICUBIC)) for a, (_, w_line, _) in zip(imgs, SIZES)]
    for win, (b, x0) in zip(windows, plan):
        assert int((win != lines[b][:, x0:x0 + 64]).sum()) == 0, "window (%d, %d) differs from PIL" % (b, x0)
    # an image of one window is the image folder_batches resizes
    assert np.array_equal(windows[1], resize.pil_resize_u8(imgs[1], 16, 64))


def _plan_of(w_lines):
    return [(b, x0) for b, w_line in enumerate(w_lines) for x0 in tile.window_plan(w_line)]


def test_stitch_of_the_windows_of_one_line_is_the_quantised_line():
    rng = np.random.RandomState(5)
    w_lines = [w_line for _, w_line, _ in SIZES] + [65, 112, 160]
    plan = _plan_of(w_lines)
    lines = [rng.rand(3, 32, 2 * w_line).astype(np.float32) for w_line in w_lines]
    sr = np.stack([lines[b][:, :, 2 * x0:2 * x0 + 128] for b, x0 in plan])
    out = tile.stitch_np(sr, plan)
    assert len(out) == len(w_lines)
    for got, line in zip(out, lines):
        assert got.dtype == np.uint8 and got.shape == (32, line.shape[2], 3)
        assert int((got != display.quantize_sr(line).transpose(1, 2, 0)).sum()) == 0


def test_stitch_blends_differing_windows_with_the_integer_ramp():
    """The 9 x 40 case: a line of 71 columns, windows at 0 and 7, SR columns [0, 128) and [14, 142).  Window 0 is 0.0 (byte 0), window
    1 is 1.0 (byte 255): the bytes are round(255 * wgt1 / (wgt0 + wgt1)), wgt0 = min(64, 128 - X), wgt1 = min(X - 13, 64)."""
    assert tile.window_plan(tile.line_width(9, 40)) == [0, 7]
    sr = np.zeros((2, 4, 32, 128), np.float32)
    sr[1] = 1.0
    (got,) = tile.stitch_np(sr, [(0, 0), (0, 7)])
    assert got.shape == (32, 142, 3) and (got == got[:1, :, :1]).all()      # the same in every row and channel
    row = got[0, :, 0].astype(int)
    assert (row[:14] == 0).all() and (row[128:] == 255).all()
    # X: (wgt0, wgt1) -> (255 * wgt1 + W // 2) // W, by hand
    by_hand = {14: 4,        # (64, 1): 287 // 65
               64: 113,      # (64, 51): 13062 // 115
               71: 129,      # (57, 58): 14847 // 115
               77: 142,      # (51, 64): 16377 // 115
               127: 251}     # (1, 64): 16352 // 65
    assert {x: row[x] for x in by_hand} == by_hand
    for X in range(14, 128):
        w0, w1 = min(64, 128 - X), min(X - 13, 64)
        assert row[X] == (255 * w1 + (w0 + w1) // 2) // (w0 + w1)
    assert (np.diff(row) >= 0).all()
    # save_image's rule on the way: out-of-range values and a NaN
    sr[0, 0, 0, :3] = [-2.0, 7.0, np.nan]
    (got,) = tile.stitch_np(sr, [(0, 0), (0, 7)])
    assert got[0, :3, 0].tolist() == [0, 255, 0]


def test_demo_tile_without_demo_dir_exits_with_one_clear_line():
    spec = importlib.util.spec_from_file_location("dpmn_main_tile", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(demo_tile=True, demo_dir=None))
    assert str(e.value).startswith("main.py: --demo_tile needs --demo_dir") and "\n" not in str(e.value)
