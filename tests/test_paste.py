"""The semantics of the paste path (dpmn_amd/utils/paste.py), no GPU: paste_coeffs, the restatement paste_regions_np against PIL's own
Image.transform(PERSPECTIVE, BICUBIC) + Image.paste(mask=L), byte for byte, the feathered mask and the integer blend against the
installed PIL, the bounding-box visit against the full visit, enlarge_np against Image.resize, and main.py's refusal of --demo_paste
without --demo_boxes."""
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from dpmn_amd.utils import paste, resize
from test_quad import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_Q = {c[0]: c[2] for c in CASES}
H, W, SCALE = 40, 89, 2      # the 40 x 89 photo that test_quad's quads of photo 4 lie in; enlarged to 80 x 178
# (quad, SR image): several regions -- 'slanted' and 'foreshortened' overlap, so their order matters; one partly outside the photo, one
# wholly outside; SR sizes 32 x 128 and 32 x 200
REGIONS = [("axis_aligned", 0), ("slanted", 1), ("foreshortened", 0), ("half_outside", 1), ("wholly_outside", 0), ("one_tile_8x32", 1)]
FEATHERS = (0.0, 0.5, 1.0, 3.0)


def _photo_and_sr(seed=5):
    rng = np.random.RandomState(seed)
    photo = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return photo, [rng.randint(0, 256, (32, 128, 3)).astype(np.uint8), rng.randint(0, 256, (32, 200, 3)).astype(np.uint8)]


@pytest.fixture(scope="module")
def scene():
    """(the enlarged photo, the SR images, {feather: regions})."""
    photo, srs = _photo_and_sr()
    photo2 = paste.enlarge_np(photo, SCALE)
    regions = {f: [(k, paste.paste_coeffs(_Q[name], SCALE, srs[k].shape[1], srs[k].shape[0]), f) for name, k in REGIONS] for f in FEATHERS}
    return photo2, srs, regions


@pytest.fixture(scope="module")
def pasted(scene):
    """The restatement's result per feather, computed once."""
    photo2, srs, regions = scene
    return {f: paste.paste_regions_np(photo2, srs, regions[f]) for f in FEATHERS}


def _pil_paste(photo2, srs, regions, pil_mask):
    """The regions through PIL: transform, mask, paste.  pil_mask: the mask comes from PIL's own transform of an all-255 L image,
    otherwise from the restatement's mask function over the whole photo."""
    H2, W2 = photo2.shape[:2]
    im = Image.fromarray(photo2)
    for k, c, f in regions:
        h_s, w_s = srs[k].shape[:2]
        ct = tuple(float(v) for v in c)
        warped = Image.fromarray(srs[k]).transform((W2, H2), Image.PERSPECTIVE, ct, Image.BICUBIC)
        if pil_mask:
            mask = Image.new("L", (w_s, h_s), 255).transform((W2, H2), Image.PERSPECTIVE, ct, Image.BICUBIC)
        else:
            mask = Image.fromarray(paste.region_patch(srs[k], c, f, (0, 0, W2, H2))[1])
        im.paste(warped, mask=mask)
    return np.asarray(im)


@pytest.mark.parametrize("scale", [2, 3])
@pytest.mark.parametrize("name", ["axis_aligned", "slanted", "foreshortened"])
def test_paste_coeffs_take_the_scaled_corners_to_the_sr_rectangle(name, scale):
    for w_s, h_s in ((128, 32), (200, 32)):
        a = paste.paste_coeffs(_Q[name], scale, w_s, h_s)
        assert a.dtype == np.float64 and a.shape == (8,)
        for (x, y), (u, v) in zip(_Q[name], ((0, 0), (w_s, 0), (w_s, h_s), (0, h_s))):
            X, Y = x * scale, y * scale
            den = a[6] * X + a[7] * Y + 1
            assert den > 0      # (these quads lie on the origin's side of their vanishing line)
            assert abs((a[0] * X + a[1] * Y + a[2]) / den - u) < 1e-9 and abs((a[3] * X + a[4] * Y + a[5]) / den - v) < 1e-9


def test_paste_coeffs_refuse_a_degenerate_mapping():
    for bad in ([(3, 3), (3, 3), (3, 3), (3, 3)],                      # one point
                [(0, 0), (10, 0), (20, 0), (30, 0)],                   # collinear
                [(0, 0), (10, 10), (10, 0), (0, 10)],                  # self-crossing: the denominator changes sign
                [(0, 0), (np.inf, 0), (10, 10), (0, 10)]):
        with pytest.raises(ValueError):
            paste.paste_coeffs(bad, 2, 128, 32)
    with pytest.raises(ValueError):
        paste.paste_coeffs(_Q["slanted"], 2, 0, 32)
    with pytest.raises(ValueError):
        paste.paste_coeffs(_Q["slanted"][:3], 2, 128, 32)


def test_a_hard_edge_equals_pil_transform_and_paste(scene, pasted):
    photo2, srs, regions = scene
    regs = regions[0.0]
    got = pasted[0.0]
    assert got.dtype == np.uint8 and got.shape == photo2.shape and got is not photo2
    expected = _pil_paste(photo2, srs, regs, pil_mask=True)
    print("feather 0: %d of %d bytes differ from PIL, %d bytes pasted" % (int((got != expected).sum()), got.size, int((got != photo2).sum())))
    assert np.array_equal(got, expected)
    assert (got != photo2).any()
    # 'slanted' and 'foreshortened' overlap: the later one lies over the earlier one
    swapped = list(regs)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    other = paste.paste_regions_np(photo2, srs, swapped)
    assert np.array_equal(other, _pil_paste(photo2, srs, swapped, pil_mask=True)) and not np.array_equal(other, got)
    # a region wholly outside leaves the photo as it is; one partly outside pastes the part inside
    assert np.array_equal(paste.paste_regions_np(photo2, srs, [regs[4]]), photo2)
    half = paste.paste_regions_np(photo2, srs, [regs[3]])
    assert (half[0, 0] != photo2[0, 0]).any() and np.array_equal(half[:, 110:], photo2[:, 110:])
    assert np.array_equal(paste.paste_regions_np(photo2, srs, []), photo2)
    with pytest.raises(ValueError):
        paste.paste_regions_np(photo2, srs, [(2, regs[0][1], 0.0)])


def test_a_region_behind_its_vanishing_line_equals_pil(scene):
    """The left edge of this quad is 8 high, the right one 36: its vanishing line lies at x of about 27, between the photo's origin and
    the quad.  With the constant of the denominator fixed to 1 (PIL's form) the denominator is then negative all over the quad -- the
    same regular mapping, which paste_coeffs accepts and PIL evaluates alike."""
    photo2, srs, _ = scene
    q = [(40, 14), (85, 2), (88, 38), (41, 22)]
    a = paste.paste_coeffs(q, SCALE, 128, 32)
    assert all(a[6] * x * SCALE + a[7] * y * SCALE + 1 < 0 for x, y in q)
    for (x, y), (u, v) in zip(q, ((0, 0), (128, 0), (128, 32), (0, 32))):
        den = a[6] * x * SCALE + a[7] * y * SCALE + 1
        assert abs((a[0] * x * SCALE + a[1] * y * SCALE + a[2]) / den - u) < 1e-9 and abs((a[3] * x * SCALE + a[4] * y * SCALE + a[5]) / den - v) < 1e-9
    for f in (0.0, 1.0):
        got = paste.paste_regions_np(photo2, srs, [(0, a, f)])
        assert np.array_equal(got, _pil_paste(photo2, srs, [(0, a, f)], pil_mask=f == 0.0)) and (got != photo2).any()
        assert np.array_equal(got, paste.paste_regions_np(photo2, srs, [(0, a, f)], full=True))


@pytest.mark.parametrize("feather", [0.5, 1.0, 3.0])
def test_a_feathered_edge_equals_pil_paste_with_the_restatements_mask(scene, pasted, feather):
    photo2, srs, regions = scene
    got = pasted[feather]
    expected = _pil_paste(photo2, srs, regions[feather], pil_mask=False)
    print("feather %g: %d of %d bytes differ from PIL" % (feather, int((got != expected).sum()), got.size))
    assert np.array_equal(got, expected)
    assert not np.array_equal(got, pasted[0.0])
    # the mask: 0 outside, a ramp of the stated rule at the edge, 255 from `feather` SR pixels inside
    k, c, _ = regions[feather][1]
    mask = paste.region_patch(srs[k], c, feather, (0, 0) + photo2.shape[1::-1])[1]
    hard = paste.region_patch(srs[k], c, 0.0, (0, 0) + photo2.shape[1::-1])[1]
    assert mask.dtype == np.uint8 and set(np.unique(hard).tolist()) == {0, 255}
    assert ((mask > 0) <= (hard == 255)).all() and mask.max() == 255 and len(np.unique(mask)) > 2


def test_feather_mask_follows_the_stated_rule():
    sx = np.array([[0.0, 0.25, 0.5, 1.0, 64.0, 127.75, 127.0, 5.0]])
    sy = np.array([[16.0, 16.0, 16.0, 16.0, 16.0, 16.0, 31.5, 40.0]])
    inside = (sx >= 0) & (sx < 128) & (sy >= 0) & (sy < 32)
    for f in (0.5, 1.0, 3.0):
        expected = []
        for x, y, i in zip(sx[0], sy[0], inside[0]):
            t = min(x, 128 - x, y, 32 - y) / f
            expected.append(0 if not i else 255 if t >= 1 else int(np.floor(t * 255 + 0.5)))
        assert paste.feather_mask(sx, sy, inside, 128, 32, f).tolist() == [expected]
    assert paste.feather_mask(sx, sy, inside, 128, 32, 0.0).tolist() == [[255] * 7 + [0]]
    assert paste.feather_mask(sx, sy, inside, 128, 32, -1.0).tolist() == [[255] * 7 + [0]]
    with pytest.raises(ValueError):
        paste.feather_mask(sx, sy, inside, 128, 32, float("nan"))


def test_the_blend_is_pils_for_every_dst_src_and_mask():
    dst, src = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    base, over = Image.fromarray(dst), Image.fromarray(src)
    for m in range(256):
        im = base.copy()
        im.paste(over, mask=Image.new("L", (256, 256), m))
        assert np.array_equal(np.asarray(im), paste.blend_u8(dst, src, m)), m
    assert np.array_equal(paste.blend_u8(dst, src, 0), dst) and np.array_equal(paste.blend_u8(dst, src, 255), src)
    # RGB goes through the same rule per channel
    rgb_d, rgb_s = np.stack([dst, src, dst[::-1]], -1), np.stack([src, dst, src[:, ::-1]], -1)
    im = Image.fromarray(rgb_d)
    im.paste(Image.fromarray(rgb_s), mask=Image.new("L", (256, 256), 77))
    assert np.array_equal(np.asarray(im), paste.blend_u8(rgb_d, rgb_s, 77))


@pytest.mark.parametrize("feather", FEATHERS)
def test_the_bounding_box_visit_equals_the_full_visit(scene, pasted, feather):
    photo2, srs, regions = scene
    assert np.array_equal(paste.paste_regions_np(photo2, srs, regions[feather], full=True), pasted[feather])
    H2, W2 = photo2.shape[:2]
    for (name, k), (_, c, _) in zip(REGIONS, regions[feather]):
        x0, y0, x1, y1 = paste.region_box(c, srs[k].shape[1], srs[k].shape[0], H2, W2)
        mask = paste.region_patch(srs[k], c, 0.0, (0, 0, W2, H2))[1]
        ys, xs = np.nonzero(mask)
        if name == "wholly_outside":
            assert ys.size == 0 and (x1 <= x0 or y1 <= y0)
        else:
            assert ys.size and x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1, name
            assert (x1 - x0) * (y1 - y0) < H2 * W2
    # a mapping that is not regular (sx = X / (1 + X / 50) < 50 for every X >= 0: the inverse's denominator changes sign over the SR
    # rectangle) is visited in full
    assert paste.region_box([1, 0, 0, 0, 1, 0, 1.0 / 50, 0], 128, 32, H2, W2) == (0, 0, W2, H2)
    assert paste.region_box([0, 0, 1, 0, 0, 1, 0, 0], 128, 32, H2, W2) == (0, 0, W2, H2)      # singular


@pytest.mark.parametrize("hw,scale", [((1, 1), 2), ((7, 31), 2), ((40, 89), 2), ((23, 41), 3)])
def test_enlarge_equals_pil_resize(hw, scale):
    a = np.random.RandomState(3).randint(0, 256, hw + (3,)).astype(np.uint8)
    expected = np.asarray(Image.fromarray(a).resize((scale * hw[1], scale * hw[0]), Image.BICUBIC))
    assert np.array_equal(paste.enlarge_np(a, scale), expected)


def test_enlarge_refuses_a_side_past_the_limit():
    with pytest.raises(ValueError):
        paste.enlarge_np(np.zeros((2, resize.MAX_SIDE // 2 + 1, 3), np.uint8), 2)
    with pytest.raises(ValueError):
        paste.enlarge_np(np.zeros((resize.MAX_SIDE // 2 + 1, 2, 3), np.uint8), 2)
    with pytest.raises(ValueError):
        paste.enlarge_np(np.zeros((2, 2, 3), np.uint8), 0)
    assert paste.enlarge_np(np.zeros((1, resize.MAX_SIDE // 2, 3), np.uint8), 2).shape == (2, resize.MAX_SIDE, 3)


def test_box_batches_hands_out_the_quads_on_request(tmp_path):
    from dpmn_amd.dataset.folder import box_batches
    Image.fromarray(_photo_and_sr()[0]).save(str(tmp_path / "p.png"))
    (tmp_path / "p.txt").write_text("3,5,70,5,70,30,3,30,w\n10.3,8.7,75.2,2.1,78.9,21.4,13.6,29.8,v\n")
    plain, = list(box_batches(str(tmp_path), str(tmp_path), 4))
    with_quads, = list(box_batches(str(tmp_path), str(tmp_path), 4, quads=True))
    assert len(plain) == 5 and len(with_quads) == 6 and plain[0] == with_quads[0] == ["p_000", "p_001"]
    assert [np.asarray(q).tolist() for q in with_quads[5]] == [[[3, 5], [70, 5], [70, 30], [3, 30]], [[10.3, 8.7], [75.2, 2.1], [78.9, 21.4], [13.6, 29.8]]]


def test_demo_paste_without_demo_boxes_is_refused():
    spec = importlib.util.spec_from_file_location("dpmn_main_paste", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(demo_paste=True, demo_boxes=None, demo_dir="photos"))
    assert str(e.value).startswith("main.py: --demo_paste needs --demo_boxes") and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(demo_paste=True, demo_boxes="boxes", demo_dir="photos", demo_paste_feather=-0.5))
    assert str(e.value).startswith("main.py: --demo_paste_feather must be")
    # the command line: the argument parser reports it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "photos", "--demo_paste"], capture_output=True, text=True)
    assert r.returncode == 2 and "error: --demo_paste needs --demo_boxes" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "photos", "--demo_boxes", "boxes", "--demo_paste",
                        "--demo_paste_feather", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "error: --demo_paste_feather must be" in r.stderr
