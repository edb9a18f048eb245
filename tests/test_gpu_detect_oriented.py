"""ops.detect_oriented_tables_u8 / ops.detect_oriented_u8 (csrc/detect.hip: k_detect_moments, k_detect_extents) against the numpy
restatement (utils/detect.py), table for table and quad for quad, at the smallest shapes where each branch can go wrong; the upright
ops on the cases they had before; then main.py --demo_detect --demo_detect_oriented against --demo_boxes on the restatement's file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import detect_cases as cases
import detect_oriented_cases as oc
from dpmn_amd.utils import detect, resize

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_REF = {}


def reference(name):
    """(photo, parameters, [row pass, column pass] as (moments, k, extents), quads) of a case by the restatement, computed once."""
    if name not in _REF:
        make, kw = oc.CASES[name]
        photo = make()
        gap, vgap, floor = detect.check_params(**kw)
        g, hist = detect.gradient(detect.luma_map(photo))
        b = g >= detect.threshold(hist, floor)
        tables = [detect.oriented_pass_np(detect.label(detect.smooth(b, *gaps)), photo.shape[0], photo.shape[1], column)[:3]
                  for column, gaps in ((False, (gap, vgap)), (True, (vgap, gap)))]
        _REF[name] = (photo, kw, tables, detect.detect_oriented_np(photo, **kw))
    return _REF[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, photos, **kw):
    from dpmn_amd import ops
    packed, meta = resize.pack_ragged(photos)
    packed = packed.to(dev)
    return (ops.detect_oriented_tables_u8(packed, meta[:, 0], meta[:, 1:], **kw),
            ops.detect_oriented_u8(packed, meta[:, 0], meta[:, 1:], **kw))


def _same(name, got_tables, got_quads, ref_tables, ref_quads):
    assert len(got_tables) == 2
    for which, got, ref in zip(("row pass", "column pass"), got_tables, ref_tables):
        for what, a, b in zip(("moments", "k", "extents"), got, ref):
            assert a.shape == b.shape and a.dtype == b.dtype == np.int64, (name, which, what, a.shape, b.shape, a.dtype, b.dtype)
            print("%s %s %s: %d of %d elements differ" % (name, which, what, int((a != b).sum()), a.size))
            assert np.array_equal(a, b), (name, which, what)
    assert got_quads.dtype == np.int64 and got_quads.shape == ref_quads.shape and np.array_equal(got_quads, ref_quads), (name, "quads")


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_tables_and_quads_equal_the_restatement(dev, name):
    photo, kw, ref_tables, ref_quads = reference(name)
    tables, quads = _run(dev, [photo], **kw)
    assert len(tables) == len(quads) == 1
    _same(name, tables[0], quads[0], ref_tables, ref_quads)


def test_the_cases_reach_what_they_are_for(dev):
    from dpmn_amd import ops
    assert all(len(t[0]) == 0 for n in ("flat", "1x1") for t in reference(n)[2]) and len(reference("flat")[3]) == 0
    assert all(len(t[0]) > ops.DETECT_TABLE for t in reference("many")[2]) and len(reference("many")[3]) == detect.MAX_BOXES
    assert [len(t[0]) for t in reference("two_in_a_word")[2]] == [2, 2]      # two roots in the one word of a row
    assert detect.working_size(*reference("large")[0].shape[:2])[0] == 2 and len(reference("large")[3]) == 1
    for angle in oc.ANGLES:
        assert len(reference("angle_%d" % angle)[3]) >= 1
    k = reference("bar")[2][0][1]
    assert len(k) == 1 and k[0] not in (-1, 32)      # a slanted component over several tiles in both directions
    assert reference("bar")[0].shape[:2] == (100, 150)


def test_a_ragged_batch_of_three_is_its_photos_one_by_one(dev):
    names = ["angle_30", "1x1", "bar"]
    assert all(reference(n)[1] == {} for n in names)      # (one call, one set of parameters)
    tables, quads = _run(dev, [reference(n)[0] for n in names])
    for n, t, q in zip(names, tables, quads):
        _same(n, t, q, reference(n)[2], reference(n)[3])


def test_rejections(dev):
    from dpmn_amd import _abi, ops
    packed, meta = resize.pack_ragged([cases.flat()])
    d = packed.to(dev)
    for kw in (dict(gap=0), dict(gap=65), dict(vgap=0), dict(vgap=65), dict(floor=0), dict(floor=256)):
        with pytest.raises(_abi.DpmnError):
            ops.detect_oriented_u8(d, meta[:, 0], meta[:, 1:], **kw)
    with pytest.raises(_abi.DpmnError):
        ops.detect_oriented_u8(packed, meta[:, 0], meta[:, 1:])                        # a host tensor: there is no CPU fallback
    with pytest.raises(_abi.DpmnError):
        ops.detect_oriented_u8(d, meta[:, 0] + 1, meta[:, 1:])                         # the photo leaves the buffer
    with pytest.raises(_abi.DpmnError):
        ops.detect_oriented_tables_u8(d, meta[:, 0], meta[:, 1:2])


def test_the_entry_points_refuse_bad_arguments_without_a_launch(dev):
    """Bad items, slices that leave the table and null pointers come back as errors, and the tables keep what they held."""
    from dpmn_amd import _abi
    lib, s = _abi.lib, _abi.stream()
    items = np.array([[0, 40, 70, 0, 40, 70, 1, 0]], np.int64)
    tiles = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [0, 2, 0], [0, 2, 1]], np.int32)
    slices = np.array([[0, 4]], np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_items, d_tiles, d_slices = t(items), t(tiles), t(slices)
    smooth = torch.zeros(2800, dtype=torch.uint8, device=dev)
    labels = torch.full((2800,), -1, dtype=torch.int32, device=dev)
    slots = torch.zeros(2800, dtype=torch.int32, device=dev)
    dirs = torch.zeros(4, 2, dtype=torch.int32, device=dev)
    mom = torch.full((4, 5), 7, dtype=torch.int64, device=dev)
    ext = torch.full((4, 4), 7, dtype=torch.int32, device=dev)

    def moments(items_h=items, slices_h=slices, table=mom.data_ptr(), sm=smooth.data_ptr(), n_tiles=6, rows=4, B=1):
        return lib.dpmn_detect_moments_i64(sm, labels.data_ptr(), 2800, d_items.data_ptr(), items_h.ctypes.data, B, d_tiles.data_ptr(), n_tiles,
                                           d_slices.data_ptr(), slices_h.ctypes.data, slots.data_ptr(), table, rows, s)

    def extents(items_h=items, slices_h=slices, table=ext.data_ptr(), d=dirs.data_ptr(), n_tiles=6, rows=4, B=1):
        return lib.dpmn_detect_extents_i32(smooth.data_ptr(), labels.data_ptr(), 2800, d_items.data_ptr(), items_h.ctypes.data, B,
                                           d_tiles.data_ptr(), n_tiles, d_slices.data_ptr(), slices_h.ctypes.data, slots.data_ptr(), d, table,
                                           rows, s)

    bad_item = items.copy()
    bad_item[0, 4] = 41      # a working map that is not its photo's
    far = items.copy()
    far[0, 3] = 1            # the map leaves the buffer
    bad_slice = np.array([[2, 4]], np.int64)
    for call in (moments, extents):
        for kw in (dict(items_h=bad_item), dict(items_h=far), dict(slices_h=bad_slice), dict(table=None), dict(B=0), dict(n_tiles=-1), dict(rows=-1)):
            assert call(**kw) != 0, (call.__name__, kw)
    assert moments(sm=None) != 0 and extents(d=None) != 0
    torch.cuda.synchronize()
    assert (mom == 7).all() and (ext == 7).all()      # nothing was launched, nothing was initialised
    # n_tiles == 0: the tables are initialised and nothing else happens; then a launch over a map without foreground leaves them so
    for n_tiles in (0, 6):
        assert moments(n_tiles=n_tiles) == 0 and extents(n_tiles=n_tiles) == 0
        torch.cuda.synchronize()
        assert (mom == 0).all() and (ext == -2139062144).all()      # (every byte 0x80: below every projection)
        mom.fill_(7)
        ext.fill_(7)


@pytest.mark.parametrize("name", ["70x131", "words", "bricks", "1x2050"])
def test_the_upright_ops_return_what_they_returned(dev, name):
    """detect_maps_u8 and detect_text_u8 on tests/detect_cases.py's photos, after an oriented call on the same device: the new path
    does not disturb the old."""
    from dpmn_amd import ops
    make, kw = {"70x131": (lambda: cases.speckle(70, 131, 4), dict(gap=3)), "words": (lambda: cases.word_photo()[0], {}),
                "bricks": (lambda: cases.bricks(720, 720), dict(gap=1)), "1x2050": (lambda: cases.noise(1, 2050, 6), {})}[name]
    photo = make()
    packed, meta = resize.pack_ragged([photo])
    packed = packed.to(dev)
    ops.detect_oriented_u8(packed, meta[:, 0], meta[:, 1:], **kw)
    maps, boxes = ops.detect_maps_u8(packed, meta[:, 0], meta[:, 1:], **kw), ops.detect_text_u8(packed, meta[:, 0], meta[:, 1:], **kw)
    ref = detect.detect_maps_np(photo, **kw)
    for a, b in zip(maps[0], ref):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), name
    want = detect.boxes_from_components(detect.components(ref[3]), photo.shape[0], photo.shape[1])
    assert boxes[0].dtype == np.int32 and np.array_equal(boxes[0], want), name


@pytest.fixture(scope="module")
def stack(dev):
    """(sr, models, psn) of config 0 (TSRN + 1 + 1 PGRM + CMM) with seeded synthetic weights, batch size 2."""
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def test_main_demo_detect_oriented_equals_demo_boxes_on_the_restatements_file(dev, stack, tmp_path):
    """python main.py --demo_dir DIR --demo_detect --demo_detect_oriented on the word at 30 degrees against --demo_boxes BOXDIR with the
    box file that utils.detect writes on the CPU: the same box file, the same region images byte for byte, each 32 x 128."""
    from test_gpu_display_eval import _checkpoints
    src, box = tmp_path / "photos", tmp_path / "boxes_np"
    src.mkdir()
    box.mkdir()
    photo = oc.rotated_word(30)
    Image.fromarray(photo).save(str(src / "a.png"))
    quads = detect.detect_oriented_np(photo)
    assert len(quads) == 1
    detect.write_quads(str(box / "a.txt"), quads)
    sr, models, psn = stack
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--arch", "tsrn", "--mask", "--gradient", "--synthetic_prior", "--batch_size", "2",
            "--stu_iter_b1", "1", "--stu_iter_b2", "1", "--patch_size", "2,2,", "--embed_dim", "96,96,", "--window_size", "2,4,8,2,4,8,",
            "--depths", "1,1,", "--num_heads", "6,6,", "--mlp_ratio", "4,4,", "--drop_rate", "0,0,", "--attn_drop_rate", "0,0,",
            "--drop_path_rate", "0,0,", "--resume", d, "--demo_dir", str(src)]
    outs = {}
    for tag, extra in (("detect", ["--demo_detect", "--demo_detect_oriented"]), ("boxes", ["--demo_boxes", str(box)])):
        outs[tag] = os.path.join(d, "out_" + tag)
        r = subprocess.run(base + extra + ["--demo_out", outs[tag]], cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(outs["detect"], "boxes", "a.txt")) as f, open(str(box / "a.txt")) as g:
        assert f.read() == g.read() == detect.quad_lines(quads)
    files = sorted(os.listdir(outs["boxes"]))
    assert files == ["a_000_sr.png", "demo_result.csv"]
    assert sorted(f for f in os.listdir(outs["detect"]) if f != "boxes") == files
    for f in files:
        with open(os.path.join(outs["detect"], f), "rb") as a, open(os.path.join(outs["boxes"], f), "rb") as b:
            assert a.read() == b.read(), f
    assert Image.open(os.path.join(outs["detect"], "a_000_sr.png")).size == (128, 32)
