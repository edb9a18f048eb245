"""The semantics of pasting polygon regions back (dpmn_amd/utils/paste_poly.py), no GPU: an axis-aligned polygon against the PIL-verified
quadrilateral paste of utils/paste.py, byte for byte; the inverse of a strip against the forward map of utils/poly.py's cells; a slanted
parallelogram against paste_coeffs' perspective map; the bounding boxes, the order of a mixed list, and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dpmn_amd.utils import paste, paste_poly, poly, quad

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

AXIS_POLY = np.array([3, 5, 35, 5, 67, 5, 67, 21, 35, 21, 3, 21], np.float64).reshape(-1, 2)      # k = 3, integer corners
AXIS_QUAD = np.array([3, 5, 67, 5, 67, 21, 3, 21], np.float64).reshape(4, 2)
SLANTED = np.array([10, 8, 60, 14, 56, 30, 6, 24], np.float64).reshape(4, 2)                        # k = 2: a parallelogram


def arc(cx, cy, r_top, r_bottom, half_angle, k):
    """2k points of a ring segment around (cx, cy), clockwise from top-left, the centre below the text (r_top > r_bottom)."""
    a = np.linspace(-half_angle, half_angle, k)
    t = np.stack([cx + r_top * np.sin(a), cy - r_top * np.cos(a)], 1)
    b = np.stack([cx + r_bottom * np.sin(a), cy - r_bottom * np.cos(a)], 1)
    return np.concatenate([t, b[::-1]])


def scene(seed=5):
    """A 40 x 100 photo enlarged by 2 and one random 32 x 128 SR image."""
    rng = np.random.RandomState(seed)
    photo2 = paste.enlarge_np(rng.randint(0, 256, (40, 100, 3)).astype(np.uint8), 2)
    return photo2, rng.randint(0, 256, (32, 128, 3)).astype(np.uint8)


@pytest.mark.parametrize("feather", [0.0, 1.5])
def test_axis_aligned_polygon_is_the_quadrilateral_paste(feather):
    photo2, sr = scene()
    strips = paste_poly.strip_table(AXIS_POLY, 2, 128, 32)
    assert strips.shape == (2, 10)
    assert strips.tolist() == [[6, 10, 70, 10, 70, 42, 6, 42, 0, 64], [70, 10, 134, 10, 134, 42, 70, 42, 64, 128]]
    got = paste_poly.paste_mixed_np(photo2, [sr], [(0, strips, feather)])
    expected = paste.paste_regions_np(photo2, [sr], [(0, paste.paste_coeffs(AXIS_QUAD, 2, 128, 32), feather)])
    print("feather %g: %d of %d bytes differ, %d bytes pasted" % (feather, int((got != expected).sum()), got.size, int((expected != photo2).sum())))
    assert got.dtype == np.uint8 and np.array_equal(got, expected)
    assert int((expected != photo2).sum()) > 128 * 32


def random_strip(rng):
    """A random strictly convex clockwise quadrilateral (NW, NE, SE, SW), rejected with quad.check_quad."""
    while True:
        base = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64) * rng.uniform(4, 60, 2)
        q = base + rng.uniform(-0.35, 0.35, (4, 2)) * base.max(axis=0) + rng.uniform(-20, 80, 2)
        th = rng.uniform(-0.6, 0.6)
        q = (q - q.mean(0)) @ np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]]) + q.mean(0)
        try:
            quad.check_quad(q)
        except ValueError:
            continue
        return q


def test_inverse_round_trip_and_nothing_outside_is_claimed():
    rng = np.random.RandomState(11)
    worst, outside_points = 0.0, 0
    for _ in range(200):
        nw, ne, se, sw = q = random_strip(rng)
        # the forward map: poly.polygon_cells' coefficients for one cell of 1 x 1 (xin = u, yin = v), independent code
        (_, _, a), = poly.polygon_cells(np.stack([nw, ne, se, sw]), 1, [0, 1])
        u, v = rng.uniform(0, 1, 64), rng.uniform(0, 1, 64)
        px = a[0] + a[1] * u + a[2] * v + a[3] * u * v
        py = a[4] + a[5] * u + a[6] * v + a[7] * u * v
        strip = np.concatenate([q.reshape(-1), [0.0, 1.0]])
        gu, gv = paste_poly.strip_uv(strip, px, py)
        worst = max(worst, float(np.abs(gu - u).max()), float(np.abs(gv - v).max()))
        # the pixels of the grown bounding box whose centre lies outside the strip (by the sign of the four edge cross products)
        x0, y0, x1, y1 = paste_poly.strip_box(strip, 4096, 4096)
        X, Y = np.meshgrid(np.arange(x0, x1) + 0.5, np.arange(y0, y1) + 0.5)
        e = np.roll(q, -1, axis=0) - q
        side = [e[i, 0] * (Y - q[i, 1]) - e[i, 1] * (X - q[i, 0]) for i in range(4)]
        out = np.any([s < -1e-9 for s in side], axis=0)
        gu, gv = paste_poly.strip_uv(strip, X, Y)
        with np.errstate(invalid="ignore"):
            claimed = (gu >= 0) & (gu < 1) & (gv >= 0) & (gv < 1)
        outside_points += int(out.sum())
        assert not (claimed & out).any()
        assert claimed[~np.any([s < 1e-9 for s in side], axis=0)].all()      # and everything well inside is
    print("round trip over 200 strips: max |u - u'|, |v - v'| = %.3g; %d outside points, none claimed" % (worst, outside_points))
    assert worst <= 1e-12 and outside_points > 1000


def test_parallelogram_agrees_with_the_perspective_map():
    strips = paste_poly.strip_table(SLANTED, 2, 128, 32)
    assert strips.shape == (1, 10) and strips[0, 8:].tolist() == [0, 128]
    coeffs = paste.paste_coeffs(SLANTED, 2, 128, 32)
    H2, W2 = 80, 200
    box = paste_poly.polygon_box(strips, H2, W2)
    assert box == (11, 15, 121, 61)
    x0, y0, x1, y1 = box
    sx, sy, inside = paste_poly.polygon_source(strips, 128, 32, box, H2, W2)
    xin = (np.arange(x0, x1, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(y0, y1, dtype=np.float64) + 0.5)[:, None]
    _, p_inside, psx, psy = quad.perspective_sample(np.zeros((32, 128, 3)), xin, yin, coeffs)
    both = inside & p_inside
    err = max(float(np.abs(sx - psx)[both].max()), float(np.abs(sy - psy)[both].max()))
    near_edge = (np.minimum(np.minimum(np.abs(psx), np.abs(128 - psx)), np.minimum(np.abs(psy), np.abs(32 - psy))) <= 1e-9)
    print("parallelogram: %d inside pixels, max |sx - sx'|, |sy - sy'| = %.3g SR pixels, %d pixels differ in the inside set"
          % (int(both.sum()), err, int((inside != p_inside).sum())))
    assert both.sum() > 3000 and err <= 1e-9
    assert not ((inside != p_inside) & ~near_edge).any()


def mixed_scene():
    """An enlarged photo, three SR images and a list in which a quadrilateral, an arc and a second quadrilateral overlap."""
    rng = np.random.RandomState(23)
    photo2 = paste.enlarge_np(rng.randint(0, 256, (40, 100, 3)).astype(np.uint8), 2)
    srs = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in ((32, 128), (32, 200), (16, 90))]
    curve = arc(44, 90, 74, 60, 0.5, 7)
    quads = [(0, paste.paste_coeffs([(20.5, 12), (90, 6.25), (93, 30), (22, 37.5)], 2, 128, 32), 1.5),
             (2, paste.paste_coeffs([(-8, 14), (19, 15), (18.5, 26), (-9, 24.5)], 2, 90, 16), 0.0)]
    polys = [(1, paste_poly.strip_table(curve, 2, 200, 32), 1.5), (0, paste_poly.strip_table(AXIS_POLY, 2, 128, 32), 0.0),
             (2, paste_poly.strip_table(curve + [40.0, -10.0], 2, 90, 16), 1.0)]      # the last: half outside the photo
    return photo2, srs, quads, polys


def test_boxes_order_and_quadrilaterals_alone():
    photo2, srs, quads, polys = mixed_scene()
    mixed = [quads[0], polys[0], quads[1], polys[1], polys[2]]
    got = paste_poly.paste_mixed_np(photo2, srs, mixed)
    full = paste_poly.paste_mixed_np(photo2, srs, mixed, full=True)
    print("boxes against every pixel: %d of %d bytes differ; %d bytes pasted" % (int((got != full).sum()), got.size, int((got != photo2).sum())))
    assert np.array_equal(got, full)
    assert int((got != photo2).sum()) > 10000
    # a list of quadrilaterals alone is paste_regions_np
    assert np.array_equal(paste_poly.paste_mixed_np(photo2, srs, quads), paste.paste_regions_np(photo2, srs, quads))
    # the overlap of a quadrilateral and a polygon: the order matters
    pair = [quads[0], polys[0]]
    a, b = paste_poly.paste_mixed_np(photo2, srs, pair), paste_poly.paste_mixed_np(photo2, srs, pair[::-1])
    assert not np.array_equal(a, b)
    # every polygon pasted alone changes bytes inside its box and none outside
    H2, W2 = photo2.shape[:2]
    for p in polys:
        x0, y0, x1, y1 = paste_poly.polygon_box(p[1], H2, W2)
        one = paste_poly.paste_mixed_np(photo2, srs, [p])
        changed = (one != photo2).any(axis=2)
        assert changed[y0:y1, x0:x1].any()
        changed[y0:y1, x0:x1] = False
        assert not changed.any()
    # only the outline is feathered: across the seams of the arc the mask stays 255
    strips = polys[0][1]
    box = paste_poly.polygon_box(strips, H2, W2)
    _, mask = paste_poly.polygon_patch(srs[1], strips, 1.5, box, H2, W2)
    sx, sy, inside = paste_poly.polygon_source(strips, 200, 32, box, H2, W2)
    deep = inside & (sx > 2) & (sx < 198) & (sy > 2) & (sy < 30)
    assert deep.sum() > 2000 and (mask[deep] == 255).all() and (mask[inside] < 255).any()
    # (the seams leave no holes here: every pixel surrounded by claimed pixels is claimed)
    core = inside[1:-1, 1:-1]
    ring = inside[:-2, 1:-1] & inside[2:, 1:-1] & inside[1:-1, :-2] & inside[1:-1, 2:]
    assert not (ring & ~core).any()


def test_refusals():
    good = arc(44, 90, 74, 60, 0.5, 7)
    assert paste_poly.strip_table(good, 2, 128, 32).shape == (6, 10)
    dented = AXIS_POLY.copy()
    dented[1] = (35, 30)                      # the middle top point below the bottom edge: neither strip is convex
    nan = AXIS_POLY.copy()
    nan[2, 0] = np.nan
    for pts, w_s, h_s in ((dented, 128, 32), (nan, 128, 32), (AXIS_POLY[[0, 5]], 128, 32), (AXIS_POLY, 0, 32), (AXIS_POLY, 128, 0),
                          (AXIS_POLY, 8193, 32)):
        with pytest.raises(ValueError):
            paste_poly.strip_table(pts, 2, w_s, h_s)
    for scale in (np.nan, np.inf, 0):
        with pytest.raises(ValueError):
            paste_poly.strip_table(AXIS_POLY, scale, 128, 32)
    with pytest.raises(ValueError), np.errstate(all="ignore"):
        paste_poly.strip_table(AXIS_POLY * 1e300, 1e10, 128, 32)      # finite points, scaled corners that are not
    photo2, sr = scene()
    strips = paste_poly.strip_table(AXIS_POLY, 2, 128, 32)
    bad = strips.copy()
    bad[1, 3] = np.inf
    for regions in ([(1, strips, 0.0)], [(0, bad, 0.0)], [(0, strips[:, :9], 0.0)], [(0, strips, float("nan"))], [(0, strips)],
                    [(0, np.zeros((0, 10)), 0.0)], [(0, np.zeros((32, 10)), 0.0)]):
        with pytest.raises(ValueError):
            paste_poly.paste_mixed_np(photo2, [sr], regions)


def test_main_refuses_paste_polygons_without_its_companions(tmp_path):
    """--demo_paste_polygons needs --demo_paste and --demo_polygons: a usage error from the parser, before anything is built."""
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", str(tmp_path), "--demo_boxes", str(tmp_path), "--demo_paste_polygons"]
    for extra in ([], ["--demo_paste"], ["--demo_polygons"]):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--demo_paste_polygons needs --demo_paste and --demo_polygons" in r.stderr, r.stderr[-2000:]
