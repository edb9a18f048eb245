"""ops.detect_maps_u8 / ops.detect_text_u8 (csrc/detect.hip) against the numpy restatement (utils/detect.py), byte for byte and box
for box, at the smallest shapes where each stage can go wrong; then main.py --demo_detect against --demo_boxes on box files that the
restatement wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import detect_cases as cases
from dpmn_amd.utils import detect, resize

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# name -> (photo, parameters).  The tiles of the kernels are 64 x 16 pixels of the working map.
CASES = {
    "1x1": (lambda: cases.noise(1, 1, 1), {}),                                  # all halo
    "3x5": (lambda: cases.noise(3, 5, 2), {}),
    "17x33": (lambda: cases.speckle(17, 33, 3, 0.05), dict(gap=2, vgap=1)),     # one partial tile and one row of a second
    "70x131": (lambda: cases.speckle(70, 131, 4), dict(gap=3)),                 # r = 1, crosses tile borders in both directions
    "70x131_noise": (lambda: cases.noise(70, 131, 4), {}),
    "40x200": (lambda: cases.speckle(40, 200, 9, 0.01), {}),                    # the default parameters over four tile columns
    "70x131_vgap64": (lambda: cases.speckle(70, 131, 4, 0.004), dict(vgap=64)),      # the longest walk along a column
    "1030x1100": (lambda: cases.speckle(1030, 1100, 5, 0.004), dict(gap=3)),   # r = 2, both remainders non-zero
    "1x2050": (lambda: cases.noise(1, 2050, 6), {}),                            # r = 3: an empty working map
    "flat": (cases.flat, {}),                                                   # all background: no box
    "all_foreground": (cases.all_foreground, {}),                               # one component, the longest chain of unions
    "serpentine": (cases.serpentine, dict(gap=1, vgap=1)),                      # the longest path of a component
    "checkerboard": (cases.checkerboard, dict(gap=1, vgap=1)),                  # joined at corners only
    "bricks": (lambda: cases.bricks(720, 720), dict(gap=1)),                    # > 4096 components (a second table pass), > 256 boxes
    "words": (lambda: cases.word_photo()[0], {}),
    "words_gap1": (lambda: cases.word_photo()[0], dict(gap=1)),
    "words_gap64": (lambda: cases.word_photo()[0], dict(gap=64)),
    "words_floor": (lambda: cases.word_photo()[0], dict(floor=200)),
}
_REF = {}


def reference(name):
    """(photo, parameters, the restatement's maps, its boxes) of a case, computed once."""
    if name not in _REF:
        make, kw = CASES[name]
        photo = make()
        maps = detect.detect_maps_np(photo, **kw)
        _REF[name] = (photo, kw, maps, detect.boxes_from_components(detect.components(maps[3]), photo.shape[0], photo.shape[1]))
    return _REF[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, photos, **kw):
    from dpmn_amd import ops
    packed, meta = resize.pack_ragged(photos)
    packed = packed.to(dev)
    return ops.detect_maps_u8(packed, meta[:, 0], meta[:, 1:], **kw), ops.detect_text_u8(packed, meta[:, 0], meta[:, 1:], **kw)


def _same(name, got_maps, got_boxes, ref_maps, ref_boxes):
    for what, a, b in zip(("gradient", "histogram", "smoothed map", "labels"), got_maps, ref_maps):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, what, a.shape, b.shape, a.dtype, b.dtype)
        print("%s %s: %d of %d elements differ" % (name, what, int((a != b).sum()), a.size))
        assert np.array_equal(a, b), (name, what)
    assert got_boxes.dtype == np.int32 and got_boxes.shape == ref_boxes.shape and np.array_equal(got_boxes, ref_boxes), (name, "boxes")


@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_and_boxes_equal_the_restatement(dev, name):
    photo, kw, ref_maps, ref_boxes = reference(name)
    maps, boxes = _run(dev, [photo], **kw)
    assert len(maps) == len(boxes) == 1
    _same(name, maps[0], boxes[0], ref_maps, ref_boxes)


def test_the_cases_reach_what_they_are_for(dev):
    from dpmn_amd import ops
    assert len(reference("flat")[3]) == 0 and reference("1x2050")[2][0].shape == (0, 683)
    assert reference("all_foreground")[2][2].all()
    n = len(detect.components(reference("bricks")[2][3]))
    assert n > ops.DETECT_TABLE and len(reference("bricks")[3]) == detect.MAX_BOXES
    assert len(reference("words")[3]) == 3 and len(reference("words_floor")[3]) == 0


def test_a_ragged_batch_is_its_photos_one_by_one(dev):
    names = ["3x5", "1x2050", "words", "all_foreground", "40x200"]
    assert all(reference(n)[1] == {} for n in names)      # (one call, one set of parameters)
    maps, boxes = _run(dev, [reference(n)[0] for n in names])
    for n, m, b in zip(names, maps, boxes):
        _same(n, m, b, reference(n)[2], reference(n)[3])


def test_rejections(dev):
    from dpmn_amd import _abi, ops
    packed, meta = resize.pack_ragged([cases.flat()])
    d = packed.to(dev)
    for kw in (dict(gap=0), dict(gap=65), dict(vgap=0), dict(vgap=65), dict(floor=0), dict(floor=256)):
        with pytest.raises(_abi.DpmnError):
            ops.detect_text_u8(d, meta[:, 0], meta[:, 1:], **kw)
    with pytest.raises(_abi.DpmnError):
        ops.detect_text_u8(packed, meta[:, 0], meta[:, 1:])                        # a host tensor: there is no CPU fallback
    with pytest.raises(_abi.DpmnError):
        ops.detect_text_u8(d, meta[:, 0] + 1, meta[:, 1:])                         # the photo leaves the buffer
    with pytest.raises(_abi.DpmnError):
        ops.detect_maps_u8(d, meta[:, 0], meta[:, 1:2])


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def test_main_demo_detect_equals_demo_boxes_on_the_restatements_files(dev, stack, tmp_path):
    """python main.py --demo_dir DIR --demo_detect against --demo_boxes BOXDIR with the box files that utils.detect writes on the CPU:
    the same box files, the same region images and the same CSV, byte for byte."""
    from test_gpu_display_eval import _checkpoints
    src, box = tmp_path / "photos", tmp_path / "boxes_np"
    src.mkdir()
    box.mkdir()
    photos = {"a": cases.word_photo()[0], "b": cases.word_photo(seed=11, size=(300, 200), words=(("quay 7", (20, 40)), ("exit", (150, 120))))[0]}
    for stem, a in photos.items():
        Image.fromarray(a).save(str(src / (stem + ".png")))
        detect.write_boxes(str(box / (stem + ".txt")), detect.detect_text_np(a))
    assert [len(detect.detect_text_np(a)) for a in photos.values()] == [3, 2]
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--arch", "tsrn", "--mask", "--gradient", "--synthetic_prior", "--batch_size", "2",
            "--stu_iter_b1", "1", "--stu_iter_b2", "1", "--patch_size", "2,2,", "--embed_dim", "96,96,", "--window_size", "2,4,8,2,4,8,",
            "--depths", "1,1,", "--num_heads", "6,6,", "--mlp_ratio", "4,4,", "--drop_rate", "0,0,", "--attn_drop_rate", "0,0,",
            "--drop_path_rate", "0,0,", "--resume", d, "--demo_dir", str(src)]
    outs = {}
    for tag, extra in (("detect", ["--demo_detect"]), ("boxes", ["--demo_boxes", str(box)])):
        outs[tag] = os.path.join(d, "out_" + tag)
        r = subprocess.run(base + extra + ["--demo_out", outs[tag]], cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for stem in photos:
        with open(os.path.join(outs["detect"], "boxes", stem + ".txt")) as f, open(str(box / (stem + ".txt"))) as g:
            assert f.read() == g.read(), stem
    files = sorted(f for f in os.listdir(outs["boxes"]))
    assert files == ["a_000_sr.png", "a_001_sr.png", "a_002_sr.png", "b_000_sr.png", "b_001_sr.png", "demo_result.csv"]
    assert sorted(f for f in os.listdir(outs["detect"]) if f != "boxes") == files
    for f in files:
        with open(os.path.join(outs["detect"], f), "rb") as a, open(os.path.join(outs["boxes"], f), "rb") as b:
            assert a.read() == b.read(), f
