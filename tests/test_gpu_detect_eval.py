"""ops.region_overlap_counts (csrc/detect_eval.hip) against the NumPy restatement utils.detect_eval.region_counts_np with ==, at the
smallest shapes where the kernel can go wrong, then main.py's evaluation function against the CSV made from the restatement."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import detect_eval_cases as ec
from dpmn_amd.utils import detect_eval as de

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_ROWS = 128      # csrc/detect_eval.hip DE_THREADS: the sample rows of one block, one per thread (32 pixel rows)
KEPT_BREAKS = 8       # csrc/detect_eval.hip DE_SLOTS: a row with more crossings of a region tests its samples one by one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (x, y)


def _check(dev, photos_a, photos_b):
    from dpmn_amd import ops
    want = de.region_counts_batch_np(photos_a, photos_b)
    _same(ops.region_overlap_counts(photos_a, photos_b, dev), want)
    return want


def test_block_constant_is_the_library_s():
    from dpmn_amd import _abi
    assert _abi.lib.dpmn_region_block() == BLOCK_ROWS


def test_smallest_shapes(dev):
    tiny = ec.rect(3.40, 4.40, 3.48, 4.48)                        # smaller than one sample cell, between samples: area 0
    sliver = ec.turned(30.2, 20.6, 40, 0.3, 30)                   # 0.3 px wide, 40 long
    negative = ec.turned(-40.5, -30.25, 30, 8, -20)               # wholly at negative coordinates
    corner = ec.turned(0.4, -0.3, 24, 10, 35)                     # straddles the photo's corner
    a, b = ec.turned(20, 20, 40, 4, 45), ec.turned(32, 8, 10, 4, 45)      # disjoint, the boxes meet
    want = _check(dev, [[tiny, sliver, negative, corner, a, corner]], [[tiny, ec.rect(0, 0, 64, 48), negative, corner, b]])[0]
    assert int(want[0][0]) == 0 and int(want[0][1]) > 0
    table = {tuple(p): int(v) for p, v in zip(want[2].tolist(), want[3].tolist())}
    assert table[(3, 3)] == int(want[0][3]) == table[(5, 3)] > 0      # identical regions
    assert table[(2, 2)] == int(want[0][2]) > 0
    assert table[(4, 4)] == 0


def test_polygons(dev):
    arc, star, tie = ec.arc14(), ec.poly64(), ec.bowtie()
    want = _check(dev, [[arc, star, star, tie, ec.comb(), ec.comb()]],
                  [[ec.through_arc(), star, ec.turned(40, 30, 70, 9, 12), ec.rect(3.3, 4.1, 43.7, 24.9), ec.comb(), ec.rect(0, 0, 40, 12.5)]])[0]
    table = {tuple(p): int(v) for p, v in zip(want[2].tolist(), want[3].tolist())}
    assert 0 < table[(0, 0)] < int(want[1][0])           # the arc against the quad through its concavity
    assert table[(1, 1)] == int(want[0][1])              # the 64-point polygon against itself
    assert 0 < table[(1, 2)] < int(want[1][2])           # ... and against a quad
    assert table[(3, 3)] == int(want[0][3])              # the bow-tie lies in its rectangle with its own (two-lobe) area
    # the comb has 2 * 6 > KEPT_BREAKS crossings on the rows through its teeth: the sample-by-sample arm, alone and in a pair
    assert table[(4, 4)] == int(want[0][4]) and 0 < table[(5, 5)] <= int(want[0][5])


def test_decomposition_boundaries(dev):
    one_row = (ec.rect(0, 0, 30, 10.25), ec.rect(5, 10, 25, 20))                # the boxes share one pixel row ...
    one_sample_row = (ec.rect(0, 0, 30, 10.2), ec.rect(5, 10.1, 25, 20))
    over = (ec.rect(1.5, 0, 9.5, BLOCK_ROWS / 4 + 0.25), ec.turned(5, 16, 6, 40, 10))      # one sample row more than a block's threads
    line = (ec.turned(400, 300, 700, 3, 60), ec.turned(401, 300, 700, 3, 60.2))   # several blocks' worth of rows
    long_ = (ec.turned(1100, 40, 2000, 6, 0.4), ec.rect(60, 20, 2090, 50))        # 2000 px long: a row's count passes 2^12
    pairs = [one_row, one_sample_row, over, line, long_]
    want = _check(dev, [[p[0]] for p in pairs], [[p[1]] for p in pairs])
    boxes = [de._meet(*(de.region_box(de.region_units(r)) for r in p)) for p in pairs]
    assert de.SUB * (boxes[0][3] - boxes[0][1]) == 4 and int(want[1][3][0]) > 0
    assert de.SUB * (boxes[2][3] - boxes[2][1]) > BLOCK_ROWS + 1 > de.SUB * (boxes[2][3] - boxes[2][1] - 1)
    assert de.SUB * (boxes[3][3] - boxes[3][1]) > 4 * BLOCK_ROWS and int(want[3][3][0]) > 0
    assert int(want[4][3][0]) > 4 * 2000 * 4 > 2 ** 12


def test_batch_of_photos(dev):
    rng = np.random.RandomState(11)
    n_det, n_gt = (0, 1, 3, 0, 40), (2, 0, 3, 0, 25)
    photos_a = [ec.random_quads(rng, n, 640, 480) for n in n_det]
    photos_b = [ec.random_quads(rng, n, 640, 480) for n in n_gt]
    photos_b[2][1] = ec.arc14(300, 200)
    want = _check(dev, photos_a, photos_b)
    assert [len(w[0]) for w in want] == list(n_det) and [len(w[1]) for w in want] == list(n_gt)
    assert all(len(w[2]) == 0 for w, a, b in zip(want, n_det, n_gt) if a == 0 or b == 0)      # pairs never cross photos
    assert len(want[4][2]) > 0 and int(want[4][3].max()) > 0


def test_empty_batch_launches_nothing(dev, monkeypatch):
    from dpmn_amd import ops

    def launched(*a):
        raise AssertionError("an entry point was called for a batch without regions")
    monkeypatch.setattr(ops.lib, "dpmn_region_area_u64", launched)
    monkeypatch.setattr(ops.lib, "dpmn_region_inter_u64", launched)
    got = ops.region_overlap_counts([[], []], [[], []], dev)
    _same(got, de.region_counts_batch_np([[], []], [[], []]))
    assert ops.region_overlap_counts([], [], dev) == []
    assert all(len(a) == 0 and a.dtype == np.uint64 for a in (got[0][0], got[0][1], got[0][3])) and got[0][2].shape == (0, 2)


def test_refusals(dev):
    from dpmn_amd import _abi, ops
    with pytest.raises(_abi.DpmnError):
        ops.region_overlap_counts([[ec.rect(0, 0, 4, 4)]], [[ec.rect(0, 0, 4, 4)]], torch.device("cpu"))
    with pytest.raises(_abi.DpmnError):
        ops.region_overlap_counts([[torch.zeros(4, 2)]], [[]], "cpu")
    with pytest.raises(_abi.DpmnError):
        ops.region_overlap_counts([[ec.rect(0, 0, 20000, 4)]], [[]], dev)
    with pytest.raises(_abi.DpmnError):
        ops.region_overlap_counts([[]], [], dev)


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_gpu_detect_eval", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_evaluation_function_writes_the_restatement_s_csv(dev, tmp_path):
    from dpmn_amd.utils.detect import write_quads
    photos, boxes, gt, out, ref = (tmp_path / n for n in ("photos", "boxes", "gt", "out", "ref"))
    for d in (photos, boxes, gt, out, ref):
        d.mkdir()
    hundredths = lambda q: np.round(np.asarray(q) * 100).astype(np.int64).reshape(-1)
    dets = {"a": [ec.turned(60, 40, 80, 20, 10), ec.turned(200, 90, 60, 16, -5), ec.turned(300, 200, 50, 14, 0)],
            "b": [ec.turned(100, 100, 90, 24, 30), ec.rect(10, 10, 50, 30)]}
    for stem, quads in dets.items():
        (photos / (stem + ".png")).write_bytes(b"")      # (only the names are read)
        write_quads(str(boxes / (stem + ".txt")), np.stack([hundredths(q) for q in quads]))
    (photos / "c.png").write_bytes(b"")                  # a photo without ground truth: one line, left out
    (gt / "a.txt").write_text("20,28,100,34,98,60,18,52,Hello\n168,80,232,84,230,100,166,96,###\n280,190,330,190,330,210,280,210,####World\n")
    (gt / "gt_b.txt").write_text("60,60,140,100,128,124,48,84,line\n0,0,5,0,5,5,0,5\n")
    rows = [["a", "000", " ", "", "hello"], ["a", "001", " ", "", "x"], ["a", "002", " ", "", "word"], ["b", "000", " ", "", "line"]]
    m = _main()
    records, totals = m.demo_eval(rows, str(photos), str(boxes), str(gt), str(out), dev)      # (b's second line has no row: left out)
    want = de.evaluate_dir(["a", "b", "c"], de.row_reads(rows), str(boxes), str(gt), str(ref / "detect_eval.csv"), de.region_counts_batch_np)
    assert (out / "detect_eval.csv").read_bytes() == (ref / "detect_eval.csv").read_bytes()
    assert (records, totals) == want
    assert [(r["file"], r["gt_care"], r["det"], r["det_care"], r["matched"], r["e2e_correct"]) for r in records] == [
        ("a", 2, 3, 2, 2, 1), ("b", 2, 1, 1, 1, 1)]
    assert (totals["matched"], totals["gt_care"], totals["det_care"], totals["e2e_labelled"], totals["e2e_correct"]) == (3, 4, 3, 3, 2)
