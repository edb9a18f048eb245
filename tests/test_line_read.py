"""One read per tiled line on the CPU (utils/line_read.py, main.py --demo_line_read): the restatement against the cases where the answer
is known without it -- integral geometry, a single window, the cover and the weights of every plan the tiler makes, letters that two
windows both see -- insert_spaces, then the refusals of TextSR.demo and of main.py's flags.  No GPU."""
import argparse

import numpy as np
import pytest

from dpmn_amd.utils import confidence as cf
from dpmn_amd.utils import line_read as lr
from dpmn_amd.utils import tile


def _cut(line, starts, T, step):
    """the windows of a line's logits (L, C) whose first columns are `starts` (multiples of `step` columns per frame)"""
    return np.stack([line[x0 // step:x0 // step + T] for x0 in starts])


@pytest.mark.parametrize("ragged", [False, True])
def test_windows_cut_from_one_line_stitch_back_to_it(ragged):
    """T = 17, P = 64: a frame every 4 columns; window starts that are multiples of 4 put every window frame ON a line frame."""
    T, P, C = 17, 64, 37
    rng = np.random.RandomState(3)
    batch = [(108, [0, 44])] + ([(200, [0, 44, 92, 136]), (64, [0])] if ragged else [])
    lines, windows, plan = [], [], []
    for b, (w_line, starts) in enumerate(batch):
        L = lr.line_frames(w_line, T, P)
        assert L == w_line // 4 + 1
        lines.append(rng.randn(L, C) * 3.0)
        windows.append(_cut(lines[-1], starts, T, 4))
        plan += [(b, x0) for x0 in starts]
    got = lr.stitch_lp_np(np.concatenate(windows), plan, P)
    assert len(got) == len(batch)
    for g, line in zip(got, lines):
        assert g.shape == line.shape and g.dtype == np.float64
        assert np.abs(g - cf._log_softmax(line)).max() <= 1e-12


def test_a_single_window_is_the_word_read():
    T, P, C = 26, 64, 37
    x = np.random.RandomState(5).randn(1, T, C) * 2.0
    (line,) = lr.stitch_lp_np(x, [(0, 0)], P)
    assert lr.line_frames(64, T, P) == T and line.shape == (T, C)
    assert np.abs(line - cf._log_softmax(x[0])).max() <= 1e-12
    classes, spans = lr.greedy_np(line)
    cls, length = cf.ctc_greedy(x)
    assert classes == cls[0, :length[0]].tolist() and len(spans) == len(classes) > 0
    score, terms = lr.line_score_np(line, classes)
    ref, ref_terms = cf.ctc_score(x, cls, length)
    assert abs(score - ref[0]) <= 1e-9 and terms == ref_terms[0]


def test_every_line_frame_of_every_plan_is_covered():
    T, P = 26, 64
    D = T - 1
    for w_line in range(64, 401):
        starts = tile.window_plan(w_line)
        L = lr.line_frames(w_line, T, P)
        assert L == (w_line * 25) // 64 + 1
        for j in range(L):
            cover = [lr.frame_cover(j, x0, i == 0, i == len(starts) - 1, T, P) for i, x0 in enumerate(starts)]
            cover = [c for c in cover if c is not None]
            assert 1 <= len(cover) <= 3, (w_line, j)
            for f, r, g in cover:
                assert g >= 1 and isinstance(g, int) and 0 <= r < P
                assert f + (r > 0) <= D, (w_line, j)                   # no window frame beyond D is read
        f, r, _ = lr.frame_cover(L - 1, starts[-1], len(starts) == 1, True, T, P)
        assert f + (r > 0) <= D
    # the ramp: blend_weight's, in frame units -- the outer edges of a line at the cap, an inner edge from P
    assert lr.frame_cover(0, 0, True, False, T, P) == (0, 0, 800)
    assert lr.frame_cover(25, 0, True, False, T, P) == (25, 0, 64)
    assert lr.frame_cover(25, 64, False, True, T, P) == (0, 0, 64)
    assert lr.frame_cover(24, 64, False, True, T, P) is None and lr.frame_cover(51, 64, False, True, T, P) is None
    with pytest.raises(ValueError, match="leave columns of the line uncovered"):
        lr.stitch_lp_np(np.zeros((2, T, 3)), [(0, 0), (0, 65)], P)
    assert lr.covered_lines([(0, 0), (0, 64), (1, 0)], P) == [(0, 2, 128), (2, 1, 64)]
    for bad in ((64, 1, 64), (64, 26, 1), (63, 26, 64)):
        with pytest.raises(ValueError, match="line_frames"):
            lr.line_frames(*bad)


def test_letters_in_an_overlap_are_read_once():
    """Two windows of a 108-column line (T = 17: a frame every 4 columns) both see the letters a and b, one frame apart: the windows'
    reads joined with '|' hold each letter twice, the line read once."""
    T, P, C = 17, 64, 37
    x = np.random.RandomState(9).randn(2, T, C) * 0.1
    best = np.zeros((2, T), np.int64)
    best[0, 12], best[0, 15] = 1, 2              # columns 48 and 60
    best[1, 2], best[1, 5] = 1, 2                # columns 44 + 8 = 52 and 44 + 20 = 64
    for w in range(2):
        x[w, np.arange(T), best[w]] += 6.0
    cls, length = cf.ctc_greedy(x)
    joined = "|".join("".join("_ab"[c] for c in cls[w, :length[w]]) for w in range(2))
    assert joined == "ab|ab"
    (line,) = lr.stitch_lp_np(x, [(0, 0), (0, 44)], P)
    classes, spans = lr.greedy_np(line)
    assert classes == [1, 2]
    assert all(12 <= a <= b <= 16 for a, b in spans) and spans[0][1] < spans[1][0]
    assert np.abs(np.exp(line).sum(1) - 1.0).max() <= 1e-12                       # a posterior per line frame
    score, terms = lr.line_score_np(line, classes)
    assert terms == 2 and np.isfinite(score) and 0.0 < np.exp(score / terms) <= 1.0


def test_insert_spaces():
    classes = [3, 4, 5, 6]
    for gap in (1, 2, 5):
        # runs of two frames; gap - 1 blank frames, then gap, then gap + 1
        spans, at = [], 0
        for blank in (0, gap - 1, gap, gap + 1):
            at += blank
            spans.append((at, at + 1))
            at += 2
        assert all(a <= b for a, b in spans) and all(spans[i][1] < spans[i + 1][0] for i in range(3))      # ordered and disjoint
        assert lr.insert_spaces(classes, spans, gap) == [3, 4, lr.SPACE, 5, lr.SPACE, 6]
        assert lr.insert_spaces(classes, spans, 0) == classes
        assert lr.insert_spaces(classes, spans, gap + 2) == classes
    assert lr.insert_spaces([], [], 3) == [] and lr.insert_spaces([7], [(0, 0)], 1) == [7]
    with pytest.raises(ValueError, match="insert_spaces"):
        lr.insert_spaces([1, 2], [(0, 0)], 1)
    with pytest.raises(ValueError, match="insert_spaces"):
        lr.insert_spaces([1], [(0, 0)], -1)
    # the spans greedy_np gives are ordered and disjoint
    best = [0, 2, 2, 0, 0, 2, 3, 3, 0, 1]
    lp = np.full((len(best), 4), -5.0)
    lp[np.arange(len(best)), best] = -0.1
    classes, spans = lr.greedy_np(lp)
    assert classes == [2, 2, 3, 1] and spans == [(1, 2), (5, 5), (6, 7), (9, 9)]
    assert lr.insert_spaces(classes, spans, 2) == [2, lr.SPACE, 2, 3, 1]
    assert lr.insert_spaces(classes, spans, 1) == [2, lr.SPACE, 2, 3, lr.SPACE, 1]


class _Words:
    """a recogniser with a confidence but no frame posteriors"""

    def read_conf(self, images):
        return ["ab"], [np.log(0.25)], [2]

    def __call__(self, images):
        return ["ab"]


class _Lines(_Words):
    def window_rows(self, images):
        raise AssertionError("not reached")

    def read_lines(self, rows, plan, gap=0, lr_w=64):
        raise AssertionError("not reached")


def test_demo_refuses_what_a_line_read_cannot_be(tmp_path):
    """TextSR.demo checks its flags before it touches a model or the GPU: one ValueError line each."""
    from dpmn_amd.interfaces.super_resolution import TextSR
    sr = object.__new__(TextSR)
    demo = lambda **kw: TextSR.demo(sr, [], None, iter(()), str(tmp_path / "out"), **kw)
    for kw, text in ((dict(rec=_Lines(), line_read=True), "line_read needs tile=True"),
                     (dict(rec=_Words(), tile=True, line_read=True), "window_rows"),
                     (dict(rec=lambda x: [""], tile=True, line_read=True), "window_rows"),
                     (dict(rec=_Words(), tile=True, confidence=True), "tile=True"),
                     (dict(rec=_Lines(), tile=True, confidence=True), "tile=True"),
                     (dict(rec=_Lines(), tile=True, line_read=True, upright=True), "tile=True"),
                     (dict(rec=_Lines(), tile=True, line_read=True, boxes=True, min_conf=0.5), "tile=True"),
                     (dict(rec=_Lines(), tile=True, line_space=3), "line_space needs line_read"),
                     (dict(rec=_Lines(), tile=True, line_read=True, line_space=65), "line_space must be 0 .. 64"),
                     (dict(rec=_Lines(), tile=True, line_read=True, line_space=-1), "line_space must be 0 .. 64")):
        with pytest.raises(ValueError) as e:
            demo(**kw)
        assert text in str(e.value) and "\n" not in str(e.value), kw
    assert not (tmp_path / "out").exists()
    assert TextSR._line_reader(_Lines(), True, False, 0) is None
    kw = TextSR._line_reader(_Lines(), True, True, 4)
    assert kw["gap"] == 4 and isinstance(kw["rec"], _Lines)


def _args(**kw):
    base = dict(demo_dir=None, demo_tile=False, demo_boxes=None, demo_detect=False, demo_conf=False, demo_upright=False, demo_min_conf=None,
                demo_line_read=False, demo_line_space=0, rec="crnn")
    base.update(kw)
    return argparse.Namespace(**base)


def test_main_line_read_flags():
    import main
    s = main.demo_line_setting
    assert s(_args()) is None and s(_args(demo_dir="d", demo_tile=True)) is None
    assert s(argparse.Namespace()) is None                                           # (an args object from before the flags)
    assert s(_args(demo_dir="d", demo_tile=True, demo_line_read=True)) == {"line_read": True, "line_space": 0}
    assert s(_args(demo_dir="d", demo_tile=True, demo_line_read=True, demo_line_space=64)) == {"line_read": True, "line_space": 64}
    for kw, message in ((dict(demo_line_read=True), main.DEMO_LINE_READ_NEEDS_TILE),
                        (dict(demo_dir="d", demo_line_read=True), main.DEMO_LINE_READ_NEEDS_TILE),
                        (dict(demo_tile=True, demo_line_read=True), main.DEMO_LINE_READ_NEEDS_TILE),
                        (dict(demo_dir="d", demo_tile=True, demo_line_read=True, rec="aster"), main.DEMO_LINE_READ_NEEDS_CRNN),
                        (dict(demo_dir="d", demo_tile=True, demo_line_read=True, rec="moran"), main.DEMO_LINE_READ_NEEDS_CRNN),
                        (dict(demo_dir="d", demo_tile=True, demo_line_space=3), main.DEMO_LINE_SPACE_NEEDS),
                        (dict(demo_dir="d", demo_tile=True, demo_line_read=True, demo_line_space=65), main.DEMO_LINE_SPACE_RANGE),
                        (dict(demo_dir="d", demo_tile=True, demo_line_read=True, demo_line_space=-1), main.DEMO_LINE_SPACE_RANGE),
                        (dict(demo_dir="d", demo_tile=True, demo_line_read=True, demo_line_space=2.5), main.DEMO_LINE_SPACE_RANGE)):
        with pytest.raises(ValueError) as e:
            s(_args(**kw))
        assert "main.py: " + str(e.value) == message and "\n" not in message, kw
    # --demo_conf combines with --demo_tile under --demo_line_read only; the other two never do
    c = main.demo_conf_setting
    assert c(_args(demo_dir="d", demo_tile=True, demo_line_read=True, demo_conf=True)) == {"confidence": True, "upright": False, "min_conf": None}
    for kw in (dict(demo_conf=True), dict(demo_conf=True, demo_line_read=True, demo_upright=True),
               dict(demo_line_read=True, demo_boxes="b", demo_min_conf=0.5)):
        with pytest.raises(ValueError) as e:
            c(_args(demo_dir="d", demo_tile=True, **kw))
        assert "main.py: " + str(e.value) == main.DEMO_CONF_OR_TILE


def test_main_refuses_line_flags_on_the_command_line():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import main
    for flags, message in ((["--demo_dir", "d", "--demo_line_read"], main.DEMO_LINE_READ_NEEDS_TILE),
                           (["--demo_dir", "d", "--demo_tile", "--demo_line_read", "--rec", "aster"], main.DEMO_LINE_READ_NEEDS_CRNN),
                           (["--demo_dir", "d", "--demo_tile", "--rec", "crnn", "--demo_line_space", "2"], main.DEMO_LINE_SPACE_NEEDS)):
        r = subprocess.run([sys.executable, os.path.join(root, "main.py")] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and " ".join(r.stderr.split()).endswith(message[len("main.py: "):]), r.stderr
