"""The locally adaptive threshold on the GPU (csrc/detect.hip: k_detect_cell_otsu, k_detect_hsmooth_local; ops.detect_*_u8(local=C))
against the numpy restatement (utils/detect.py), with ==: the cell tables, the threshold maps, the smoothed maps, labels, boxes and
quads of one ragged batch at two cell sides; the device's Otsu at the corners of its exact comparison; one cell against the global
path; and main.py --demo_detect_local on the scene that the feature is for."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import detect_cases as cases
import detect_local_cases as lc
from dpmn_amd.utils import detect, resize

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIDES = (32, 128)
_REF = {}


def batch():
    if "batch" not in _REF:
        _REF["batch"] = lc.ragged_batch()
        assert [p.shape[:2] for p in _REF["batch"]] == [(1, 1), (5, 300), (130, 257), (1025, 40), (300, 300), (480, 640)]
    return _REF["batch"]


def reference(C):
    """Per photo of the batch (cell table, T map, maps, boxes, quads) of the restatement at cell side C (0: the global recipe), once."""
    if C not in _REF:
        out = []
        for p in batch():
            maps = detect.detect_maps_np(p, local=C)
            t = detect.cell_thresholds(maps[0], C, detect.FLOOR) if C else None
            T = detect.threshold_map(t, maps[0].shape[0], maps[0].shape[1], C) if C else None
            out.append((t, T, maps, detect.boxes_from_components(detect.components(maps[3]), p.shape[0], p.shape[1]),
                        detect.detect_oriented_np(p, local=C)))
        _REF[C] = out
    return _REF[C]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pack(dev, photos):
    packed, meta = resize.pack_ragged(photos)
    return packed.to(dev), meta[:, 0], meta[:, 1:]


def _equal(what, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    print("%s: %d of %d elements differ" % (what, int((a != b).sum()), a.size))
    assert np.array_equal(a, b), what


def _thresholds_equal(dev, photos, C, floor):
    from dpmn_amd import ops
    got = ops.detect_thresholds_u8(*_pack(dev, photos), C, floor)
    assert len(got) == len(photos)
    tables = []
    for i, (p, (t, T)) in enumerate(zip(photos, got)):
        g = detect.gradient(detect.luma_map(p))[0]
        ref = detect.cell_thresholds(g, C, floor)
        _equal("photo %d cell table" % i, t, ref)
        _equal("photo %d threshold map" % i, T, detect.threshold_map(ref, g.shape[0], g.shape[1], C))
        tables.append(t)
    return tables


@pytest.mark.parametrize("C", SIDES)
def test_cell_tables_and_threshold_maps_equal_the_restatement(dev, C):
    from dpmn_amd import ops
    got = ops.detect_thresholds_u8(*_pack(dev, batch()), C, detect.FLOOR)
    for i, ((t, T), ref) in enumerate(zip(got, reference(C))):
        _equal("C %d photo %d cell table" % (C, i), t, ref[0])
        _equal("C %d photo %d threshold map" % (C, i), T, ref[1])
    if C == 32:      # the plans the batch is for: cell borders off the 64 x 16 tiles, and a single column of cells at r = 2
        assert got[2][0].shape == (5, 9) and got[3][0].shape == (16, 1) and got[0][0].shape == (1, 1) and len(np.unique(got[2][0])) > 3


@pytest.mark.parametrize("C", SIDES)
def test_maps_and_labels_equal_the_restatement(dev, C):
    from dpmn_amd import ops
    got = ops.detect_maps_u8(*_pack(dev, batch()), local=C)
    for i, (maps, ref) in enumerate(zip(got, reference(C))):
        for what, a, b in zip(("gradient", "histogram", "smoothed map", "labels"), maps, ref[2]):
            _equal("C %d photo %d %s" % (C, i, what), a, b)


@pytest.mark.parametrize("C", SIDES)
def test_boxes_and_quads_equal_the_restatement(dev, C):
    from dpmn_amd import ops
    args = _pack(dev, batch())
    boxes, quads = ops.detect_text_u8(*args, local=C), ops.detect_oriented_u8(*args, local=C)
    for i, (b, q, ref) in enumerate(zip(boxes, quads, reference(C))):
        _equal("C %d photo %d boxes" % (C, i), b, ref[3])
        _equal("C %d photo %d quads" % (C, i), q, ref[4])
    assert len(boxes[5]) == 2 and len(reference(0)[5][3]) == 1      # the scene: the faint word is found, and only with cells
    assert sum(len(b) for b in boxes) >= 10 and sum(len(q) for q in quads) >= 10


def test_one_cell_is_the_global_path_byte_for_byte(dev):
    from dpmn_amd import ops
    args = _pack(dev, batch())
    for i, (a, b, ref) in enumerate(zip(ops.detect_maps_u8(*args, local=1024), ops.detect_maps_u8(*args), reference(0))):
        for what, u, v, w in zip(("gradient", "histogram", "smoothed map", "labels"), a, b, ref[2]):
            _equal("photo %d %s, one cell against none" % (i, what), u, v)
            _equal("photo %d %s, against the restatement" % (i, what), u, w)
    for i, (a, b) in enumerate(zip(ops.detect_text_u8(*args, local=1024), ops.detect_text_u8(*args))):
        _equal("photo %d boxes" % i, a, b)
    for i, (a, b) in enumerate(zip(ops.detect_oriented_u8(*args, local=1024), ops.detect_oriented_u8(*args))):
        _equal("photo %d quads" % i, a, b)


def _tie_photo():
    """30 x 30, one bright pixel in the middle of every 3 x 3 block on a ground of 0: the gradient of a block is its pixel's level.
    40 blocks of 10, 20 of 130, 40 of 250: a symmetric histogram whose only two splits tie exactly -- Otsu's t is the earlier, 10."""
    levels = np.random.default_rng(8).permutation(np.repeat([10, 130, 250], [40, 20, 40])).reshape(10, 10)
    y = np.zeros((30, 30), np.uint8)
    y[1::3, 1::3] = levels
    return lc.gray(y)


def _half_photo():
    """128 x 128: one-pixel cells of 0 and 255 in the upper half (gradient 255 down to row 64), flat below (gradient 0): one full
    128 x 128 cell of the two extreme bins, the largest products of the comparison at that size."""
    yy, xx = np.mgrid[:128, :128]
    return lc.gray(np.where(yy < 64, ((yy + xx) & 1) * 255, 0))


def test_device_otsu_at_the_corners_of_its_comparison(dev):
    flat, two, tie, half = cases.flat(), lc.stripes(40, 70, 8, 60, 200), _tie_photo(), _half_photo()
    hists = [detect.gradient(detect.luma_map(p))[1] for p in (flat, two, tie, half)]
    assert (hists[0] > 0).sum() == 1 and (hists[1] > 0).sum() == 2 and detect.otsu(hists[0]) == 0      # no valid split: t = 0
    assert np.nonzero(hists[2])[0].tolist() == [10, 130, 250] and hists[2][10] == hists[2][250] and detect.otsu(hists[2]) == 10
    assert np.nonzero(hists[3])[0].tolist() == [0, 255] and hists[3].sum() == 1 << 14 and abs(int(hists[3][0]) - int(hists[3][255])) <= 256
    t = _thresholds_equal(dev, [flat, two, tie], 32, 1)      # (floor 1: the table shows t + 1 itself)
    assert t[0].max() == 1 and t[2].tolist() == [[11]]
    t = _thresholds_equal(dev, [flat, two, tie, half], 128, 24)
    assert t[0].tolist() == [[24]] and t[3].tolist() == [[max(detect.otsu(hists[3]) + 1, 24)]]


def test_device_otsu_over_the_largest_cell(dev):
    """C = 1024 on 1024 x 1024 random bytes: one cell of 2^20 pixels, where the products of the comparison pass 128 bits."""
    photo = lc.gray(np.random.default_rng(9).integers(0, 256, (1024, 1024), dtype=np.uint8))
    t = _thresholds_equal(dev, [photo], 1024, 24)
    assert t[0].shape == (1, 1) and t[0][0, 0] == detect.threshold(detect.gradient(detect.luma_map(photo))[1], 24)


def test_rejections(dev):
    from dpmn_amd import _abi, ops
    args = _pack(dev, [cases.flat()])
    for local in (31, 1025, -1):
        for f in (ops.detect_text_u8, ops.detect_maps_u8, ops.detect_oriented_u8, ops.detect_oriented_tables_u8):
            with pytest.raises(_abi.DpmnError):
                f(*args, local=local)
    with pytest.raises(_abi.DpmnError):
        ops.detect_thresholds_u8(*args, 0)
    # a cell offset that is not the running sum of the cell counts, or a table of another size: refused before any launch
    host = ops._detect_plan(*_pack(dev, [cases.flat(), cases.flat()]), "test", 32)
    items, n = host["items"], host["n_cells"]
    assert n == 2 * 2 * 3 and items[:, 7].tolist() == [0, 6]
    d_items = torch.from_numpy(items).to(dev)
    g = torch.zeros(host["map_px"], dtype=torch.uint8, device=dev)
    table = torch.full((n,), -7, dtype=torch.int32, device=dev)
    bad = items.copy()
    bad[1, 7] = 5
    for it, cells in ((items, n - 1), (items, n + 1), (bad, n)):
        rc = _abi.lib.dpmn_detect_cell_otsu_i32(g.data_ptr(), host["map_px"], d_items.data_ptr(), it.ctypes.data, 2, 32, 24, table.data_ptr(), cells,
                                                _abi.stream())
        assert rc != 0
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == -7).all()


def test_detect_box_files_writes_the_faint_word_only_with_cells(dev, tmp_path):
    from dpmn_amd.dataset import folder
    src = tmp_path / "photos"
    src.mkdir()
    Image.fromarray(lc.scene()).save(str(src / "scene.png"))
    ref = reference(128)[5]
    assert folder.detect_box_files(str(src), str(tmp_path / "l"), 2, dev, local=128) == 2
    assert folder.detect_box_files(str(src), str(tmp_path / "g"), 2, dev) == 1
    assert folder.detect_box_files(str(src), str(tmp_path / "o"), 2, dev, oriented=True, local=128) == 2
    with open(str(tmp_path / "l" / "scene.txt")) as f:
        assert f.read() == detect.box_lines(ref[3])
    with open(str(tmp_path / "g" / "scene.txt")) as f:
        assert f.read() == detect.box_lines(reference(0)[5][3])
    with open(str(tmp_path / "o" / "scene.txt")) as f:
        assert f.read() == detect.quad_lines(ref[4])


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def test_main_demo_detect_local_super_resolves_both_words(dev, stack, tmp_path):
    """python main.py --demo_dir DIR --demo_detect --demo_detect_local on the scene: two lines in boxes/scene.txt, the restatement's,
    and two region images."""
    from test_gpu_display_eval import _checkpoints
    src = tmp_path / "photos"
    src.mkdir()
    Image.fromarray(lc.scene()).save(str(src / "scene.png"))
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    out = os.path.join(d, "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--arch", "tsrn", "--mask", "--gradient", "--synthetic_prior", "--batch_size", "2",
                        "--stu_iter_b1", "1", "--stu_iter_b2", "1", "--patch_size", "2,2,", "--embed_dim", "96,96,", "--window_size", "2,4,8,2,4,8,",
                        "--depths", "1,1,", "--num_heads", "6,6,", "--mlp_ratio", "4,4,", "--drop_rate", "0,0,", "--attn_drop_rate", "0,0,",
                        "--drop_path_rate", "0,0,", "--resume", d, "--demo_dir", str(src), "--demo_detect", "--demo_detect_local", "--demo_out", out],
                       cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(out, "boxes", "scene.txt")) as f:
        assert f.read() == detect.box_lines(reference(128)[5][3])
    assert sorted(f for f in os.listdir(out) if f != "boxes") == ["demo_result.csv", "scene_000_sr.png", "scene_001_sr.png"]
