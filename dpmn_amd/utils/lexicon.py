"""Lexicon-constrained reading (ours; main.py --rec_lexicon): the word list, its packed records and the NumPy restatement of the two
kernels of csrc/lexicon.hip.

A lexicon is a list of distinct words over the recognisers' alphabet.  A word travels as a 32-byte record: byte 0 its length n
(1 .. 31), bytes 1 .. n its classes (1-based, 0 is the CTC blank: model.crnn.ALPHABET's numbering), the rest 0.  Two protocols pick
a word for an image:
  score  (CTC recognisers)  the word with the highest CTC log-likelihood under the frame posteriors: ctc_word_logp / ctc_lexicon_best
  edit   (any recogniser)   the word with the smallest Levenshtein distance to the greedy string: edit_lexicon_best
Ties go to the lowest index in both.  Everything here is float64 / integer NumPy on the host: it fixes the semantics and is what
the GPU tests compare the kernels with."""
import numpy as np

MAX_WORDS = 1 << 20     # the kernels keep a word's index in 20 bits
MAX_LEN = 25            # load_lexicon's rule (utils.render.MAX_LEN, --train_words)
RECORD = 32             # bytes per packed word


def _alphabet():
    from ..model.crnn import ALPHABET
    return ALPHABET


def load_lexicon(path, voc_type='lower'):
    """The words of a word file (one per line, UTF-8): every line through str_filt(line, voc_type); empty results and words of more
    than 25 characters are dropped (the --train_words rule), then duplicates (the first occurrence stays, the order is kept).  No
    word left, or more than 2^20 of them: ValueError."""
    from .util import str_filt
    words, seen = [], set()
    with open(path, encoding="utf-8") as fh:
        for line in fh:
            w = str_filt(line.strip(), voc_type)
            if 1 <= len(w) <= MAX_LEN and w not in seen:
                seen.add(w)
                words.append(w)
    if not words:
        raise ValueError("lexicon %s holds no usable word (a word has 1 .. %d characters of voc_type %r)" % (path, MAX_LEN, voc_type))
    if len(words) > MAX_WORDS:
        raise ValueError("lexicon %s holds %d words; at most %d are supported" % (path, len(words), MAX_WORDS))
    return words


def pack_lexicon(words, alphabet=None, allow_empty=False):
    """words (strings, or sequences of symbols of `alphabet`) -> (L, 32) uint8 records.  alphabet: at most 255 symbols, class of
    alphabet[i] = i + 1 (default: the CRNN's).  allow_empty: a length of 0 is packed too (the strings of edit_lexicon_best)."""
    alphabet = _alphabet() if alphabet is None else alphabet
    if len(alphabet) > 255:
        raise ValueError("pack_lexicon: at most 255 classes fit a byte")
    cls = {ch: i + 1 for i, ch in enumerate(alphabet)}
    out = np.zeros((len(words), RECORD), np.uint8)
    for i, w in enumerate(words):
        n = len(w)
        if n > RECORD - 1 or (n == 0 and not allow_empty):
            raise ValueError("pack_lexicon: word %d has %d symbols; 1 .. %d are supported" % (i, n, RECORD - 1))
        out[i, 0] = n
        try:
            out[i, 1:1 + n] = [cls[ch] for ch in w]
        except KeyError as e:
            raise ValueError("pack_lexicon: word %d holds %r, which is not in the alphabet" % (i, e.args[0]))
    return out


def unpack_lexicon(packed, alphabet=None):
    """The inverse of pack_lexicon for a string alphabet: (L, 32) uint8 -> list of strings."""
    alphabet = _alphabet() if alphabet is None else alphabet
    return ["".join(alphabet[c - 1] for c in rec[1:1 + rec[0]]) for rec in np.asarray(packed, np.uint8).reshape(-1, RECORD)]


def pack_strings(strings, alphabet=None):
    """A recogniser's strings as records for the edit protocol: symbols outside the alphabet are dropped after lowering, a string
    of more than 31 symbols is cut at 31; the empty string is a record of length 0."""
    alphabet = _alphabet() if alphabet is None else alphabet
    return pack_lexicon(["".join(ch for ch in str(s).lower() if ch in alphabet)[:RECORD - 1] for s in strings], alphabet, allow_empty=True)


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def ctc_word_logp(logits, words_packed):
    """logits (B, T, n_class) float64, words (L, 32) -> (B, L) float64: log sum over all CTC alignments of the word (blank = class 0,
    2n + 1 states, a skip over a blank only between different labels) on the log-softmax of the logits; -inf for a word that does
    not fit (n + its adjacent equal pairs > T)."""
    lp = _log_softmax(logits)
    B, T, _ = lp.shape
    words = np.asarray(words_packed, np.uint8).reshape(-1, RECORD)
    L = words.shape[0]
    n = words[:, 0].astype(np.int64)
    S = 2 * RECORD - 1                                           # 63 states at the most; states >= 2n + 1 stay -inf
    ext = np.zeros((L, S), np.int64)
    ext[:, 1::2] = words[:, 1:]
    state = np.arange(S)[None, :]
    live = state < (2 * n + 1)[:, None]
    skip = np.zeros((L, S), bool)
    skip[:, 3::2] = ext[:, 3::2] != ext[:, 1:-2:2]
    skip &= live
    out = np.empty((B, L), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            emit = lp[b][:, ext]                                 # (T, L, S)
            a = np.full((L, S), -np.inf)
            a[:, 0] = emit[0, :, 0]
            a[:, 1] = emit[0, :, 1]
            a[~live] = -np.inf
            for t in range(1, T):
                p1 = np.full((L, S), -np.inf)
                p1[:, 1:] = a[:, :-1]
                p2 = np.full((L, S), -np.inf)
                p2[:, 2:] = a[:, :-2]
                p2[~skip] = -np.inf
                m = np.maximum(np.maximum(a, p1), p2)
                ms = np.where(np.isfinite(m), m, 0.0)
                a = ms + np.log(np.exp(a - ms) + np.exp(p1 - ms) + np.exp(p2 - ms)) + emit[t]
                a[~live] = -np.inf
            rows = np.arange(L)
            e1, e2 = a[rows, 2 * n], a[rows, 2 * n - 1]
            m = np.maximum(e1, e2)
            ms = np.where(np.isfinite(m), m, 0.0)
            out[b] = ms + np.log(np.exp(e1 - ms) + np.exp(e2 - ms))
    return out


def best_of_scores(scores):
    """(B, L) scores -> (index (B) int64, score (B)): the highest score, the lowest index among equals; -1 / -inf where every score
    is -inf."""
    scores = np.asarray(scores, np.float64)
    idx = scores.argmax(1)                                       # (the first maximum)
    best = scores[np.arange(scores.shape[0]), idx]
    idx = np.where(np.isneginf(best), -1, idx)
    return idx.astype(np.int64), best


def ctc_lexicon_best(logits, words_packed):
    return best_of_scores(ctc_word_logp(logits, words_packed))


def edit_distances(strings_packed, words_packed):
    """(B, 32) strings (length 0 allowed), (L, 32) words -> (B, L) int64 Levenshtein distances (insert, delete, substitute: 1 each)."""
    strings = np.asarray(strings_packed, np.uint8).reshape(-1, RECORD)
    words = np.asarray(words_packed, np.uint8).reshape(-1, RECORD)
    L = words.shape[0]
    n = words[:, 0].astype(np.int64)
    out = np.empty((strings.shape[0], L), np.int64)
    for b, rec in enumerate(strings):
        m = int(rec[0])
        s = rec[1:1 + m].astype(np.int64)
        # prev[:, i] = distance between the first i symbols of the string and the first j symbols of every word
        prev = np.tile(np.arange(m + 1), (L, 1))
        res = np.where(n == 0, m, 0)
        for j in range(1, RECORD):
            c = words[:, j].astype(np.int64)
            cur = np.empty_like(prev)
            cur[:, 0] = j
            sub = prev[:, :-1] + (s[None, :] != c[:, None])
            dele = prev[:, 1:] + 1
            best = np.minimum(sub, dele)
            for i in range(1, m + 1):                            # the insertion chain runs along the string
                cur[:, i] = np.minimum(best[:, i - 1], cur[:, i - 1] + 1)
            prev = cur
            res = np.where(n == j, prev[:, m], res)
        out[b] = res
    return out


def edit_lexicon_best(strings_packed, words_packed):
    """-> (index (B) int64, distance (B) int64) of the nearest word, the lowest index among equals."""
    d = edit_distances(strings_packed, words_packed)
    idx = d.argmin(1)
    return idx.astype(np.int64), d[np.arange(d.shape[0]), idx]
