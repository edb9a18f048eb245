"""Seeded inputs and float64 references that tests/test_lexicon.py (CPU) and tests/test_gpu_lexicon.py share: the same logits and
lexicons on both sides, every reference computed once per process."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from dpmn_amd.utils import lexicon as lx

CTC_SLAB = 128      # words per block of k_ctc_lexicon (csrc/lexicon.hip): one lexicon size just below and one just above it

# name -> (B, T, L, n_class, ld, sigma of the logits, word lengths lo .. hi)
CTC_CASES = {
    "one_word": (1, 26, 1, 37, 40, 3.0, 25, 25),              # 51 states: its score is the answer
    "one_long_T64": (1, 64, 1, 64, 64, 3.0, 31, 31),          # 63 states
    "ragged_257": (3, 26, 257, 37, 40, 3.0, 1, 25),
    "short_T7_1000": (5, 7, 1000, 37, 40, 3.0, 1, 25),        # most words do not fit 7 frames
    "wide_T64_C64": (2, 64, 33, 64, 64, 3.0, 1, 31),
    "below_slab": (2, 26, CTC_SLAB - 1, 37, 40, 3.0, 1, 25),
    "above_slab": (2, 26, CTC_SLAB + 1, 37, 40, 3.0, 1, 25),
    "none_fits": (2, 7, 5, 37, 40, 3.0, 8, 25),               # wholly infeasible: index -1
}


def _words(rng, L, n_sym, lo, hi):
    """L distinct words (tuples of classes 1 .. n_sym) with lengths lo .. hi: the first ones are the edge cases -- the shortest, the
    longest, a doubled letter, a run of one letter -- the rest random."""
    seen, out = set(), []

    def add(w):
        w = tuple(int(c) for c in w)
        if w not in seen and len(out) < L:
            seen.add(w)
            out.append(w)
    add(rng.randint(1, n_sym + 1, lo))
    add(rng.randint(1, n_sym + 1, hi))
    if hi >= 4 and lo <= 4:
        add([3, 7, 7, 2])
    if hi >= 3 and lo <= 3:
        add([5, 5, 5])
    while len(out) < L:
        add(rng.randint(1, n_sym + 1, rng.randint(lo, hi + 1)))
    return out


@functools.lru_cache(maxsize=None)
def ctc_case(name):
    """-> dict: logits (B, T, ld) float32 with the padding columns at +1e4, packed (L, 32), alphabet, ref (B, L) float64 scores of the
    restatement, idx / best (its choice), margin (B; top-2 gap in nats, inf with fewer than two feasible words), e_ref (the error
    of torch's fp32 CPU ctc_loss against the restatement), bound (the score tolerance of the issue)."""
    B, T, L, n_class, ld, sigma, lo, hi = CTC_CASES[name]
    rng = np.random.RandomState(1000 + sorted(CTC_CASES).index(name))
    alphabet = list(range(1, n_class))
    words = _words(rng, L, n_class - 1, lo, hi)
    packed = lx.pack_lexicon(words, alphabet)
    logits = np.full((B, T, ld), 1e4, np.float32)
    logits[:, :, :n_class] = (rng.randn(B, T, n_class) * sigma).astype(np.float32)
    real = logits[:, :, :n_class]
    ref = lx.ctc_word_logp(real.astype(np.float64), packed)
    idx, best = lx.best_of_scores(ref)
    top = np.sort(ref, 1)[:, ::-1]
    with np.errstate(invalid="ignore"):
        margin = np.where(L > 1, top[:, 0] - top[:, min(1, L - 1)], np.inf)
    margin = np.where(np.isnan(margin), np.inf, margin)          # (-inf minus -inf: nothing to decide)
    # torch's own fp32 error on the same inputs: every (image, word) pair as one batch entry, the full T as the input length
    lp32 = torch.log_softmax(torch.from_numpy(real.copy()), -1)                                  # (B, T, C) fp32
    lp32 = lp32.permute(1, 0, 2).repeat_interleave(L, 1)                                         # (T, B * L, C), entry b * L + w
    lengths = torch.from_numpy(packed[:, 0].astype(np.int64)).repeat(B)
    targets = torch.from_numpy(packed[:, 1:].astype(np.int64)).repeat(B, 1)
    nll = F.ctc_loss(lp32, targets, torch.full((B * L,), T, dtype=torch.long), lengths, blank=0, reduction="none")
    got = -nll.double().numpy().reshape(B, L)
    finite = np.isfinite(ref)
    assert np.array_equal(finite, np.isfinite(got)), "torch and the restatement disagree on which words fit"
    e_ref = float(np.abs(got[finite] - ref[finite]).max()) if finite.any() else 0.0
    biggest = float(np.abs(ref[finite]).max()) if finite.any() else 0.0
    bound = 4.0 * max(e_ref, T * 2.0 ** -24 * biggest)
    return dict(B=B, T=T, L=L, n_class=n_class, ld=ld, logits=logits, words=words, packed=packed, alphabet=alphabet, ref=ref, idx=idx, best=best,
                margin=margin, e_ref=e_ref, bound=bound)


EDIT_ALPHABET = "abc"      # a small alphabet: near words and ties are common


@functools.lru_cache(maxsize=None)
def edit_case(B, L):
    """-> dict: strings / words (lists), sp (B, 32) / wp (L, 32) their records, idx / dist the restatement's answer.  The strings hold an empty one
    (B > 1) and one of 26 symbols; the words hold duplicates-by-distance, so ties are everywhere."""
    rng = np.random.RandomState(77 + 1000 * B + L)
    rand = lambda lo, hi: "".join(rng.choice(list(EDIT_ALPHABET), rng.randint(lo, hi + 1)))
    strings = [rand(26, 26)] + [rand(0, 31) for _ in range(B - 1)]
    if B > 1:
        strings[1] = ""
    if B > 2:
        strings[2] = rand(31, 31)
    # (every third word is short: they repeat and tie, which is what the lowest-index rule is tested on)
    words = [rand(1, 31) if k % 3 else rand(1, 4) for k in range(L)]
    sp, wp = lx.pack_lexicon(strings, EDIT_ALPHABET, allow_empty=True), lx.pack_lexicon(words, EDIT_ALPHABET)
    idx, dist = lx.edit_lexicon_best(sp, wp)
    return dict(strings=strings, words=words, sp=sp, wp=wp, idx=idx, dist=dist)
