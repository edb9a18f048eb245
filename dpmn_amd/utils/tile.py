"""A wide text line as overlapping windows of the model's LR size (main.py --demo_tile, TextSR.demo(tile=True)): the line is resized
to the LR height with its aspect ratio kept (PIL's bicubic resize, utils/resize.py), cut into lr_h x lr_w windows that overlap, every
window is super-resolved on its own, and the SR windows are blended back into one image.  This module fixes the semantics in integer
arithmetic -- the plan of the windows and a numpy restatement of both device steps (ops.resize_windows_u8 / ops.stitch_windows_u8,
csrc/tile.hip), whose bytes the kernels reproduce exactly.  No GPU needed: importable on any machine.

A plan is a list of (image, x0) per window: the image's index in the batch and the window's first column in its resized line; the
windows of an image are consecutive, their starts do not decrease, the first is 0 and the last ends at the line's width.
"""
import numpy as np

from .display import quantize_sr
from .resize import MAX_SIDE, check_image, pil_resize_u8

LR_H, LR_W = 16, 64
STRIDE = 48               # the largest step between two windows: neighbours share at least lr_w - STRIDE = 16 LR columns


def line_width(h, w, lr_h=LR_H, lr_w=LR_W):
    """The width of an h x w image resized to the height lr_h with its aspect ratio kept: w * lr_h / h rounded half up, never below
    lr_w (a crop of aspect lr_w : lr_h or less is stretched to lr_h x lr_w, one window).  ValueError for a side outside 1 .. MAX_SIDE
    or a line wider than MAX_SIDE, which is not resized."""
    h, w, lr_h, lr_w = int(h), int(w), int(lr_h), int(lr_w)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and 1 <= lr_h <= MAX_SIDE and 1 <= lr_w <= MAX_SIDE):
        raise ValueError("line_width: %d x %d -> height %d, window width %d: sides outside 1 .. %d" % (h, w, lr_h, lr_w, MAX_SIDE))
    w_line = max(lr_w, (2 * w * lr_h + h) // (2 * h))
    if w_line > MAX_SIDE:
        raise ValueError("line_width: a %d x %d image is %d wide at height %d, lines above %d are not resized" % (h, w, w_line, lr_h, MAX_SIDE))
    return w_line


def window_plan(w_line, lr_w=LR_W, stride=STRIDE):
    """The first columns of the windows of a line w_line >= lr_w wide: n = ceil((w_line - lr_w) / stride) + 1 windows spread evenly,
    x0_t = t * (w_line - lr_w) / (n - 1) rounded half up.  The first starts at 0, the last ends at w_line, two neighbours are at most
    `stride` apart; no window reads outside the line."""
    w_line, lr_w, stride = int(w_line), int(lr_w), int(stride)
    if lr_w < 1 or not 1 <= stride <= lr_w or w_line < lr_w:
        raise ValueError("window_plan: line %d, window %d, stride %d (need line >= window >= stride >= 1)" % (w_line, lr_w, stride))
    d = w_line - lr_w
    if d == 0:
        return [0]
    n = -(-d // stride) + 1
    return [(t * d + (n - 1) // 2) // (n - 1) for t in range(n)]


def check_line(im, lr_size=(LR_H, LR_W), what="image"):
    """check_image plus the width of the image's line -> (h, w, w_line); ValueError for an image whose line is not resized."""
    h, w = check_image(im, what)
    return h, w, line_width(h, w, *lr_size)


def plan_lines(plan, lr_w=LR_W):
    """A plan -> [(first window, n windows, w_line)] per image, checked: the images 0, 1, .. in turn, every image's windows
    consecutive with starts that begin at 0 and do not decrease.  ValueError otherwise."""
    lines = []
    for t, (b, x0) in enumerate(plan):
        b, x0 = int(b), int(x0)
        if b == len(lines) and x0 == 0:
            lines.append([t, 1, lr_w])
        elif lines and b == len(lines) - 1 and lines[-1][2] - lr_w <= x0 <= MAX_SIDE - lr_w:
            lines[-1][1] += 1
            lines[-1][2] = x0 + lr_w
        else:
            raise ValueError("plan_lines: window %d = (image %d, x0 %d) does not continue the plan" % (t, b, x0))
    if not lines:
        raise ValueError("plan_lines: an empty plan")
    return [tuple(l) for l in lines]


def resize_windows_np(images, lr_size=(LR_H, LR_W)):
    """A list of (h, w, 3) uint8 images -> (windows (T, lr_h, lr_w, 3) uint8, plan): every image resized to (lr_h, line_width) =
    np.asarray(Image.fromarray(img).resize((w_line, lr_h), BICUBIC)) (resize.pil_resize_u8) and cut at window_plan's starts.  The CPU reference of ops.resize_windows_u8."""
    lr_h, lr_w = lr_size
    windows, plan = [], []
    for b, im in enumerate(images):
        h, w, w_line = check_line(im, lr_size, "image %d" % b)
        line = pil_resize_u8(im, lr_h, w_line)
        for x0 in window_plan(w_line, lr_w):
            windows.append(line[:, x0:x0 + lr_w])
            plan.append((b, x0))
    if not windows:
        raise ValueError("resize_windows_np: an empty batch")
    return np.stack(windows), plan


def blend_weight(j, first, last, sr_w):
    """The integer weight of SR column j (0 .. sr_w - 1) of a window: a ramp 1, 2, .. from an inner edge, capped at sr_w // 2; the
    outer edge of a line's first / last window carries the cap."""
    cap = sr_w // 2
    return min(cap if first else j + 1, cap if last else sr_w - j, cap)


def stitch_np(sr, plan, scale=2):
    """The SR windows sr (T, >= 3, H, sr_w) float (sr_w = scale * lr_w) and their plan -> one (H, scale * w_line, 3) uint8 image per
    input image: every window quantised with save_image's rule (display.quantize_sr), then per output byte the integer blend
    (sum wgt * q + W // 2) // W over the windows that cover its column, W = the sum of their weights (blend_weight).  Where one window
    covers a column the byte is that window's.  The CPU reference of ops.stitch_windows_u8."""
    sr = np.asarray(sr, np.float32)
    if sr.ndim != 4 or sr.shape[1] < 3 or sr.shape[0] != len(plan) or sr.shape[3] % scale:
        raise ValueError("stitch_np: (T, >= 3, H, scale * lr_w) windows and a plan of T entries expected, got %s and %d" % (sr.shape, len(plan)))
    H, sr_w = sr.shape[2:]
    q = quantize_sr(sr[:, :3]).transpose(0, 2, 3, 1).astype(np.int64)       # (T, H, sr_w, 3)
    out = []
    for first, n, w_line in plan_lines(plan, sr_w // scale):
        acc = np.zeros((H, scale * w_line, 3), np.int64)
        wsum = np.zeros(scale * w_line, np.int64)
        for t in range(first, first + n):
            wgt = np.array([blend_weight(j, t == first, t == first + n - 1, sr_w) for j in range(sr_w)], np.int64)
            X0 = scale * int(plan[t][1])
            acc[:, X0:X0 + sr_w] += q[t] * wgt[None, :, None]
            wsum[X0:X0 + sr_w] += wgt
        W = wsum[None, :, None]
        out.append(((acc + W // 2) // W).astype(np.uint8))
    return out
