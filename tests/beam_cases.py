"""Seeded inputs and float64 references that tests/test_beam.py (CPU) and tests/test_gpu_beam.py share: the same logits and models on
both sides, every reference (utils.beam.beam_np per image) computed once per process."""
import functools

import numpy as np

from dpmn_amd.utils import beam as bm

LD = 40             # the leading dimension of logits_rows; the columns at or beyond n_class hold 1e4 and must never be read

# name -> (B, T, n_class, width, order (0: no model), alpha, beta): a sample of
#   B {1, 3, 48} x T {1, 2, 26, 64} x n_class {3, 37} x width {1, 2, 8, 32} x order {none, 1, 2, 3} x (alpha, beta) {(0, 0), (.5, 0), (1, .3)}
# in which every value occurs, with the widths and orders spread over the frame counts
CASES = {
    "one_frame": (1, 1, 3, 1, 0, 0.0, 0.0),
    "one_frame_wide": (1, 1, 37, 32, 3, 0.5, 0.0),
    "two_frames_c3": (3, 2, 3, 2, 1, 1.0, 0.3),
    "two_frames": (3, 2, 37, 8, 2, 0.5, 0.0),
    "greedy_like": (1, 26, 37, 1, 0, 0.0, 0.0),
    "narrow_o1": (3, 26, 37, 2, 1, 0.5, 0.0),
    "flagship": (48, 26, 37, 8, 3, 0.5, 0.0),
    "default_width": (3, 26, 37, 16, 3, 0.5, 0.0),
    "full_width_bonus": (3, 26, 37, 32, 3, 1.0, 0.3),
    "full_width_plain": (3, 26, 37, 32, 0, 0.0, 0.0),
    "plain_bonus": (3, 26, 37, 8, 0, 1.0, 0.3),              # no model: alpha counts as 0, beta still pays per symbol
    "c3_o2": (3, 26, 3, 8, 2, 1.0, 0.3),
    "long_full": (1, 64, 37, 32, 3, 0.5, 0.0),
    "long_plain": (3, 64, 37, 8, 0, 0.0, 0.0),
    "long_c3": (3, 64, 3, 32, 1, 0.5, 0.0),
    "long_greedy_o2": (1, 64, 37, 1, 2, 1.0, 0.3),
    "batch_short": (48, 2, 37, 32, 2, 1.0, 0.3),
    "batch_c3": (48, 26, 3, 2, 0, 0.0, 0.0),
    "batch_one_frame": (48, 1, 37, 2, 1, 0.5, 0.0),
}


@functools.lru_cache(maxsize=None)
def corpus():
    """A seeded word list over the CRNN's 36 symbols with a skewed symbol distribution and repeated words (classes, not strings)."""
    rng = np.random.RandomState(4242)
    p = rng.dirichlet(np.full(36, 0.3))
    words = [tuple(int(c) + 1 for c in rng.choice(36, rng.randint(1, 9), p=p)) for _ in range(300)]
    return words + words[:40] * 3


@functools.lru_cache(maxsize=None)
def table(order):
    return bm.build_char_lm(corpus(), order) if order else None


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: B, T, n_class, width, order, alpha, beta; logits (B*T, LD) float32 = randn * 3 with the padding columns at 1e4; table
    (float32 or None); ref: per image (classes, score, margin) of the definition; tau: per image the tests' threshold
    (utils.beam.tolerance with |lm| bounded by (T + 1) |alpha| max|table| + T |beta|)."""
    B, T, n_class, width, order, alpha, beta = CASES[name]
    rng = np.random.RandomState(2000 + sorted(CASES).index(name))
    logits = np.full((B * T, LD), 1e4, np.float32)
    logits[:, :n_class] = (rng.randn(B * T, n_class) * 3).astype(np.float32)
    tab = table(order)
    lm_abs = (T + 1) * abs(alpha) * float(np.abs(tab).max()) + T * abs(beta) if tab is not None else T * abs(beta)
    ref, tau = [], []
    for b in range(B):
        trace = {}
        ref.append(bm.beam_np(logits[b * T:(b + 1) * T], tab, width, alpha, beta, n_class=n_class, trace=trace))
        tau.append(bm.tolerance(T, n_class, trace["lp"], lm_abs))
    return dict(B=B, T=T, n_class=n_class, width=width, order=order, alpha=alpha, beta=beta, logits=logits, table=tab, ref=ref, tau=tau)
