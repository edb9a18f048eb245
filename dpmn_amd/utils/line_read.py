"""One read per tiled text line (ours, not the reference's; main.py --demo_line_read, TextSR.demo(tile=True, line_read=True)): the
definition, as a NumPy restatement in float64 with integer geometry of the kernels of csrc/line_read.hip.  No GPU needed.

--demo_tile cuts a line into overlapping windows (utils/tile.py) and the CRNN reads every window on its own: T frame posteriors per
window, the first and the last on the window's edges.  Here the posteriors of a line's windows are blended along the line with the
ramp of the pixel stitch, and the line is decoded and scored ONCE: one string, one CTC likelihood, one confidence per line.

Notation: T frames per window, D = T - 1, P = lr_w, x0 a window's first column (utils.tile.plan_lines checks the plan).
  line frames   frame j sits at column j * P / D (window frame t at x0 + t * P / D: the same grid whenever x0 * D is a multiple of
                P); a line w_line wide has L = (w_line * D) // P + 1 of them
  cover         num = j * P - x0 * D; a window covers frame j iff 0 <= num <= D * P; with f = num // P, r = num % P its value there
                is v = ((P - r) * lp[f] + r * lp[f + 1]) / P, lp the window's log-softmax over the first n_class columns; r == 0
                reads frame f alone (so f = D never reads past the window)
  weight        g = min(cap if first else num + P, cap if last else D * P - num + P, cap), cap = (D * P) // 2, first / last: the
                line's first / last window -- utils.tile.blend_weight's ramp in frame units, a positive integer
  posterior     line_lp[j] = log_softmax(sum_w g_w v_w / sum_w g_w) over the covering windows
  decode        arg-max per line frame (first maximum), repeats collapsed, blank (class 0) dropped; per kept symbol the first and
                the last frame of its arg-max run (spans)
  score         utils.confidence.ctc_word_score(line_lp, string); terms = max(n, 1), conf = exp(score / terms), as for a word
The blend is in the LOG domain -- a weighted geometric mean of the windows' posteriors -- because that is what keeps a confident
window's veto: a letter cut by a window edge is read with a flat posterior there and sharply by the neighbour that sees it whole, and
in the log domain the sharp one dominates, while an arithmetic mean would leave half the mass on the wrong read; a class one window
rules out (log-probability -40) stays ruled out.  A weighted geometric mean is not a distribution, hence the renormalisation.
What it cannot do: repair a glyph that BOTH windows see cut, and find spaces -- the CRNN has no space class (insert_spaces is a
heuristic on its blank runs).  The string is over the CRNN's 36 symbols."""
import numpy as np

from .confidence import _log_softmax, ctc_word_score
from .tile import plan_lines

MAX_T, MAX_CLASS, MAX_L = 64, 64, 3201      # csrc/line_read.hip's limits: frames per window, classes, frames per line
SPACE = -1                                   # insert_spaces' mark between two classes


def line_frames(w_line, T, lr_w):
    """The number of frames L of a line w_line columns wide: (w_line * D) // P + 1."""
    w_line, T, lr_w = int(w_line), int(T), int(lr_w)
    if T < 2 or lr_w < 2 or w_line < lr_w:
        raise ValueError("line_frames: line %d, %d frames per window of %d columns (need T >= 2, lr_w >= 2, line >= window)" % (w_line, T, lr_w))
    return (w_line * (T - 1)) // lr_w + 1


def frame_cover(j, x0, first, last, T, lr_w):
    """Line frame j under the window that starts at column x0 -> None when the window does not cover it, else (f, r, g): the window
    frames f and f + 1 it lies between (r == 0: on f), r of P the way, and its integer weight g."""
    D, P = T - 1, lr_w
    num = j * P - x0 * D
    if not 0 <= num <= D * P:
        return None
    cap = (D * P) // 2
    return num // P, num % P, min(cap if first else num + P, cap if last else D * P - num + P, cap)


def covered_lines(plan, lr_w):
    """utils.tile.plan_lines, and no columns between two windows of a line: every line frame then lies under a window.  ValueError
    otherwise."""
    lines = plan_lines(plan, lr_w)
    for first, n, _ in lines:
        for w in range(first + 1, first + n):
            if int(plan[w][1]) - int(plan[w - 1][1]) > int(lr_w):
                raise ValueError("covered_lines: windows %d and %d of image %d leave columns of the line uncovered" % (w - 1, w, int(plan[w][0])))
    return lines


def stitch_lp_np(logits, plan, lr_w):
    """logits (Twin, T, C) of the windows of a plan -> one (L_b, C) float64 array of line log-posteriors per image.  The CPU
    reference of ops.line_stitch."""
    x = np.asarray(logits, np.float64)
    if x.ndim != 3 or x.shape[0] != len(plan):
        raise ValueError("stitch_lp_np: (windows, T, C) logits and a plan of as many entries expected, got %s and %d" % (x.shape, len(plan)))
    T, P = x.shape[1], int(lr_w)
    lp = _log_softmax(x)
    out = []
    for first, n, w_line in covered_lines(plan, P):
        L = line_frames(w_line, T, P)
        line = np.empty((L, x.shape[2]), np.float64)
        for j in range(L):
            acc, gsum = 0.0, 0
            for w in range(first, first + n):
                c = frame_cover(j, int(plan[w][1]), w == first, w == first + n - 1, T, P)
                if c is None:
                    continue
                f, r, g = c
                v = lp[w, f] if r == 0 else ((P - r) * lp[w, f] + r * lp[w, f + 1]) / P
                acc = acc + g * v
                gsum += g
            line[j] = _log_softmax(acc / gsum)
        out.append(line)
    return out


def greedy_np(line_lp):
    """line_lp (L, C) -> (classes: the arg-max classes (first maximum) with repeats collapsed and blanks dropped, spans: per kept
    symbol the (first, last) frame of its arg-max run).  The CPU reference of ops.line_greedy."""
    best = np.asarray(line_lp).argmax(-1).tolist()
    classes, spans = [], []
    prev = -1
    for j, c in enumerate(best):
        if c != 0 and c != prev:
            classes.append(c)
            spans.append([j, j])
        elif c != 0:
            spans[-1][1] = j
        prev = c
    return classes, [tuple(s) for s in spans]


def line_score_np(line_lp, classes):
    """-> (score, terms): the CTC log-likelihood of the line's own string under its posteriors (utils.confidence.ctc_word_score) and
    max(n, 1).  The CPU reference of ops.line_ctc_confidence."""
    return ctc_word_score(line_lp, classes), max(len(classes), 1)


def insert_spaces(classes, spans, gap):
    """A heuristic on the CRNN's blank runs (it has no space class): with gap >= 1, SPACE goes between two symbols that have at least
    `gap` line frames between the end of one arg-max run and the start of the next; gap = 0 inserts none.  -> the list of classes."""
    gap = int(gap)
    if gap < 0 or len(classes) != len(spans):
        raise ValueError("insert_spaces: gap >= 0 and one span per class expected, got gap %d, %d classes, %d spans" % (gap, len(classes), len(spans)))
    out = []
    for i, c in enumerate(classes):
        if gap and i and spans[i][0] - spans[i - 1][1] - 1 >= gap:
            out.append(SPACE)
        out.append(int(c))
    return out
