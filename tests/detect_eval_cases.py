"""Shapes shared by tests/test_detect_eval.py and tests/test_gpu_detect_eval.py: regions as (n, 2) float arrays in photo pixels."""
import math

import numpy as np


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def turned(cx, cy, w, h, deg):
    """A w x h rectangle about (cx, cy) turned by deg degrees, clockwise from top-left in image coordinates."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    p = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]], np.float64)
    return np.stack([cx + c * p[:, 0] - s * p[:, 1], cy + s * p[:, 0] + c * p[:, 1]], axis=1)


def arc14(cx=60.3, cy=80.7, r0=40.0, r1=52.0):
    """A 14-point arc as CTW1500 writes it: 7 points along the outer (top) edge from left to right, then 7 back along the inner edge."""
    ang = np.radians(np.linspace(200.0, 340.0, 7))
    top = np.stack([cx + r1 * np.cos(ang), cy + r1 * np.sin(ang)], axis=1)
    bot = np.stack([cx + r0 * np.cos(ang[::-1]), cy + r0 * np.sin(ang[::-1])], axis=1)
    return np.concatenate([top, bot])


def through_arc():
    """A quad laid through the concavity of arc14(): it meets both ends of the arc and the hollow between them."""
    return rect(10.2, 58.4, 110.6, 70.9)


def poly64(cx=40.13, cy=33.37, r=30.0):
    """A 64-point star-ish polygon: the radius alternates, so the outline is concave at every other vertex."""
    ang = np.radians(np.arange(64) * (360.0 / 64) + 1.7)
    rad = np.where(np.arange(64) % 2 == 0, r, 0.8 * r)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def bowtie(x0=3.3, y0=4.1, x1=43.7, y1=24.9):
    """A self-crossing quad: tl, br, tr, bl."""
    return np.array([[x0, y0], [x1, y1], [x1, y0], [x0, y1]], np.float64)


def comb(teeth=6, x0=2.1, y0=3.3, pitch=4.0, height=12.0):
    """A comb of `teeth` teeth: a sample row through the teeth crosses 2 * teeth edges (more than the 8 breaks a kernel thread keeps)."""
    pts = [[x0, y0 + height]]
    for t in range(teeth):
        x = x0 + t * pitch
        pts += [[x, y0], [x + pitch / 2, y0], [x + pitch / 2, y0 + height - 3.0], [x + pitch, y0 + height - 3.0]]
    pts += [[x0 + teeth * pitch, y0 + height]]
    return np.array(pts, np.float64)


def random_quads(rng, n, W, H):
    """n turned rectangles of word-like sizes inside a W x H photo."""
    return [turned(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(20, 160), rng.uniform(8, 40), rng.uniform(-30, 30)) for _ in range(n)]
