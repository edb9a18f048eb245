"""ops.detect_curved_tables_u8 / ops.detect_curved_u8 (csrc/detect.hip: k_detect_profile) against the numpy restatement
(utils/detect.py) with ==, at the smallest shapes where each branch of the kernel can go wrong; then one bowed scene from the detector
through its box file into ops.poly_crop_u8."""
import numpy as np
import pytest
import torch

import detect_curved_cases as cc
from dpmn_amd.utils import detect, poly, resize

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """(photo, parameters, components, candidates, profiles, regions) of a case by the restatement, computed once."""
    if name not in _REF:
        make, kw = cc.CASES[name]
        photo = make()
        labels = detect.detect_maps_np(photo, **kw)[3]
        comps = detect.components(labels)
        cand = detect.curve_candidates(comps)
        prof = detect.curve_profile(labels, cand)
        _REF[name] = (photo, kw, comps, cand, prof, detect.regions_from_profiles(comps, cand, prof, photo.shape[0], photo.shape[1]))
    return _REF[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, photos, **kw):
    from dpmn_amd import ops
    packed, meta = resize.pack_ragged(photos)
    packed = packed.to(dev)
    return (ops.detect_curved_tables_u8(packed, meta[:, 0], meta[:, 1:], **kw), ops.detect_curved_u8(packed, meta[:, 0], meta[:, 1:], **kw))


def _same(name, tables, regions, launched=True):
    photo, kw, comps, cand, prof, ref = reference(name)
    got_cand, got_prof = tables
    assert got_cand.dtype == np.int64 and got_cand.shape == cand.shape and np.array_equal(got_cand, cand), (name, "candidates")
    if launched:
        assert got_prof.dtype == np.int64 and got_prof.shape == prof.shape, (name, got_prof.shape, prof.shape)
        print("%s profiles: %d of %d elements differ" % (name, int((got_prof != prof).sum()), prof.size))
        assert np.array_equal(got_prof, prof), (name, "profiles")
    else:
        assert got_prof is None and not (cand[:, 2] > 0).any(), (name, "no candidate: no table")
    assert len(regions) == len(ref), (name, len(regions), len(ref))
    for a, b in zip(regions, ref):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (name, "regions")


NO_CANDIDATE = ("flat", "speckle_small", "many")


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_tables_and_regions_equal_the_restatement(dev, name):
    tables, regions = _run(dev, [reference(name)[0]], **reference(name)[1])      # B = 1
    assert len(tables) == len(regions) == 1
    _same(name, tables[0], regions[0], launched=name not in NO_CANDIDATE)


def test_the_cases_reach_what_they_are_for():
    from dpmn_amd import ops
    comps, cand = (lambda name: reference(name)[2]), (lambda name: reference(name)[3])
    assert cand("w16").tolist() == [[5, 16, 2]] and cand("w17").tolist() == [[5, 17, 2]]      # two bins, the edge at 5 + 8
    x0, w, n = cand("crossing_a_word")[0].tolist()
    edges = [x0 + i * w // n for i in range(n + 1)]
    assert x0 % 64 != 0 and x0 < 64 < x0 + w and any(e % 64 for e in edges[1:-1])      # over a word boundary, bin edges inside the words
    assert len(comps("crossing_a_word")) == 1 and len(comps("alone_130")) == 1                   # alone: the reduced branch
    assert cand("alone_130")[0, 1] >= 128 and cand("alone_130")[0, 2] == 16
    c = comps("two_in_a_word")
    assert len(c) == 2 and (cand("two_in_a_word")[:, 2] == 2).all() and c[:, 2].max() <= 64      # two candidates in one lane word
    assert max(c[0, 1], c[1, 1]) < min(c[0, 3], c[1, 3])                                           # ... that share rows: the per-lane branch
    assert len(comps("flat")) == 0
    assert len(comps("speckle_small")) > 0 and not (cand("speckle_small")[:, 2] > 0).any()
    for name in ("many", "many_wide"):
        assert len(comps(name)) > ops.DETECT_TABLE      # the first pass over the tables meets slot >= cap
    assert not (cand("many")[:, 2] > 0).any() and (cand("many_wide")[:, 2] > 0).sum() >= 3
    assert detect.working_size(*reference("wide_strip")[0].shape[:2])[0] == 3 and reference("wide_strip")[0].shape[:2] == (40, 2400)
    assert (cand("wide_strip")[:, 2] > 0).any()
    assert reference("local")[1] == dict(local=128)
    for name in ("arc_down", "arc_up", "crossing_a_word", "alone_130", "local", "many_wide"):
        assert any(len(q) > 4 for q in reference(name)[5]), name


def test_a_ragged_batch_of_three_is_its_photos_one_by_one(dev):
    names = ["crossing_a_word", "wide_strip", "flat"]
    assert all(reference(n)[1] == {} for n in names)      # (one call, one set of parameters)
    tables, regions = _run(dev, [reference(n)[0] for n in names])
    for n, t, r in zip(names, tables, regions):
        _same(n, t, r)      # (the batch has candidates: the photo without a component gets an empty table)
    assert tables[2][1].shape == (0, 16, 4)


def test_a_batch_without_a_candidate_launches_nothing(dev, monkeypatch):
    from dpmn_amd import _abi, ops
    calls = []
    real = _abi.lib.dpmn_detect_profile_i32
    monkeypatch.setattr(ops.lib, "dpmn_detect_profile_i32", lambda *a: calls.append(1) or real(*a), raising=False)
    photos = [reference("flat")[0], cc.photo(sag=0, letters=1)]      # no component; one component 14 wide
    tables, regions = _run(dev, photos)
    assert calls == [] and all(t[1] is None for t in tables)
    assert [len(r) for r in regions] == [0, len(detect.detect_text_np(photos[1]))]
    _run(dev, [reference("w16")[0]])
    assert calls == [1, 1]      # (the tables op and the regions op, one launch each)


def test_rejections(dev):
    from dpmn_amd import _abi, ops
    packed, meta = resize.pack_ragged([reference("flat")[0]])
    d = packed.to(dev)
    for kw in (dict(gap=0), dict(gap=65), dict(vgap=0), dict(vgap=65), dict(floor=0), dict(floor=256), dict(local=5)):
        with pytest.raises(_abi.DpmnError):
            ops.detect_curved_u8(d, meta[:, 0], meta[:, 1:], **kw)
    with pytest.raises(_abi.DpmnError):
        ops.detect_curved_u8(packed, meta[:, 0], meta[:, 1:])      # a host tensor: there is no CPU fallback
    with pytest.raises(_abi.DpmnError):
        ops.detect_curved_tables_u8(d, meta[:, 0] + 1, meta[:, 1:])


def test_the_entry_point_refuses_bad_arguments_and_initialises_its_table(dev):
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
    bins = torch.zeros(4, 3, dtype=torch.int32, device=dev)
    prof = torch.full((4, 16, 4), 7, dtype=torch.int32, device=dev)

    def call(items_h=items, slices_h=slices, table=prof.data_ptr(), b=bins.data_ptr(), sm=smooth.data_ptr(), n_tiles=6, rows=4, B=1):
        return lib.dpmn_detect_profile_i32(sm, labels.data_ptr(), 2800, d_items.data_ptr(), items_h.ctypes.data, B, d_tiles.data_ptr(), n_tiles,
                                           d_slices.data_ptr(), slices_h.ctypes.data, slots.data_ptr(), b, table, rows, s)

    bad_item, far = items.copy(), items.copy()
    bad_item[0, 4], far[0, 3] = 41, 1
    for kw in (dict(items_h=bad_item), dict(items_h=far), dict(slices_h=np.array([[2, 4]], np.int64)), dict(table=None), dict(b=None), dict(sm=None),
               dict(B=0), dict(n_tiles=-1), dict(rows=-1)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert (prof == 7).all()      # nothing was launched, nothing was initialised
    for n_tiles in (0, 6):        # initialised, and a launch over a map without foreground leaves it so
        assert call(n_tiles=n_tiles) == 0
        torch.cuda.synchronize()
        assert (prof[:, :, :2] == -2139062144).all() and (prof[:, :, 2:] == 0).all()
        prof.fill_(7)


def test_a_bowed_scene_feeds_the_polygon_crop(dev, tmp_path):
    """detect_curved_u8 -> write_regions -> the box-file reader -> ops.poly_crop_u8: a crop as high as the ribbon."""
    from dpmn_amd import ops
    photo, kw, comps, cand, prof, ref = reference("arc_down")
    packed, meta = resize.pack_ragged([photo])
    packed = packed.to(dev)
    regions = ops.detect_curved_u8(packed, meta[:, 0], meta[:, 1:])[0]
    path = str(tmp_path / "a.txt")
    detect.write_regions(path, regions)
    (k, lineno, points, label), = poly.numbered_polygons(path)
    assert len(points) == 2 * detect.CURVE_BINS
    poly.check_polygon(points)
    h, w, xs = poly.polygon_plan(points)
    (_, X2, C, R, p), = detect.curve_ribbons(comps, cand, prof, *photo.shape[:2])[1]
    assert h == R + 2 * p and w >= cand[0, 1]
    region = (0, h, w, poly.polygon_cells(points, h, xs))
    out, out_meta = ops.poly_crop_u8(packed, meta, [region])
    assert np.asarray(out_meta)[0, 1:].tolist() == [h, w]
    crop = out.cpu().numpy()[:h * w * 3].reshape(h, w, 3)
    assert np.array_equal(crop, poly.poly_crop_np([photo], [region])[0])
    ink = crop[:, :, 0] < 128
    assert ink.any(axis=0).mean() > 0.6 and ink[h // 2].mean() > 0.6      # the blocks, straightened along the middle of the crop
