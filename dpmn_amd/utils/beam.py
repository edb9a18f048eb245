"""CTC prefix beam search with a character n-gram model for the CRNN (ours; main.py --rec_beam / --rec_lm): the definition, float64
NumPy on the host, and what the GPU tests compare the kernel of csrc/beam.hip with.  No GPU needed.

The third way to turn the CRNN's frame posteriors into a string, between the greedy decode (arg-max per frame) and a lexicon (a closed
word list): the CTC prefix beam search of Hannun et al. 2014 ("First-pass large vocabulary continuous speech recognition using
bi-directional recurrent DNNs") sums over the alignments of every kept prefix and weighs each new symbol with a character model, so
the vocabulary stays open and an undecided picture falls to the likelier spelling.

  character model  build_char_lm(words, order): symbols are the CRNN's classes 1 .. 36; class 0 is the word boundary -- the padding
                   before a word's first symbol and the end-of-word event after its last.  Counts n(.) over the padded words (a word
                   that is listed five times counts five times); n(b) and n(ab) are the counts of b and ab AS A CONTEXT (the sum of
                   n(bc) over c, of n(abc) over c), N the number of symbols and end events.  Dirichlet-prior interpolation:
                     P1(c)      = (n(c) + 1) / (N + 37)
                     P2(c | b)  = (n(bc) + k P1(c)) / (n(b) + k)
                     P3(c | ab) = (n(abc) + k P2(c | b)) / (n(ab) + k)
                   so every probability is positive and every row sums to 1.  The table is float32, natural logs, shaped
                   (37 ** (order - 1), 37), the context index a * 37 + b (order 3), b (order 2), 0 (order 1).  k = 4 is untuned.
  search           beam_np(rows, table or None, width, alpha, beta) on ONE image's (T, >= n_class) float32 logits: widened to
                   float64, log-softmax over the first n_class columns (lp), then per frame t every prefix p of the beam (rank i, last
                   symbol e, pb / pnb the log-probabilities of its alignments that end in a blank / in e, tot = lse(pb, pnb), lm its
                   model score) offers
                     p itself   pb'  = tot + lp[t, 0]
                                pnb' = lse(pnb + lp[t, e]  [p not empty],  the offer of p[:-1] + e if p[:-1] is in the beam)
                     p + c      pnb' = (pb if c == e else tot) + lp[t, c], pb' = -inf,  for every class c = 1 .. n_class - 1
                                lm'  = lm + (alpha * LM(c | the last order - 1 symbols of p, boundary-padded) + beta)
                   An extension p + c that is itself a member of the beam is not a candidate of its own: its offer is the second
                   term of that member's pnb'.  A candidate ranks by lse(pb', pnb') + lm'; one whose rank score is -inf (no alignment
                   yet: a doubled letter before its blank) does not exist.  The `width` best survive.  TIES go to the lower parent rank i,
                   then to the lower class (p itself counts as class 0); the survivors' order is the next frame's rank.  Start: the
                   empty prefix with (pb, pnb, lm) = (0, -inf, 0).  After the last frame lm += alpha * LM(boundary | context); the best
                   prefix (ties: the lower rank) is the answer, its rank score the score.
                   lse(a, b) = m + log(exp(a - m) + exp(b - m)) with m = max(a, b), -inf when both are.  Without a table alpha counts
                   as 0 and LM as 0.
  margin           the smallest of: per frame, the gap between the last kept and the best dropped rank score (inf where nothing was
                   dropped); at the end, the gap between the best and the second-best prefix (inf with one prefix).  A kernel that
                   differs from this file by less than the margin in every rank score makes the same choices.
Limits (csrc/beam.hip's): T <= 64, n_class <= 64 (<= 37 with a model), 1 <= width <= 32, order <= 3."""
import numpy as np

MAX_T, MAX_CLASS, MAX_WIDTH, MAX_ORDER = 64, 64, 32, 3
LM_CLASSES = 37         # the CRNN's classes: the boundary (0) and 36 symbols
MAX_LEN = 25            # load_lm_words' rule (utils.lexicon.load_lexicon's)
NEG = -np.inf


def load_lm_words(path, voc_type='lower'):
    """The words of a word file (one per line, UTF-8) for the character model: utils.lexicon.load_lexicon's filter -- every line
    through str_filt(line, voc_type), results of 1 .. 25 characters kept -- but duplicates STAY: a word's count is its weight.  No
    word left: ValueError."""
    from .util import str_filt
    words = []
    with open(path, encoding="utf-8") as fh:
        for line in fh:
            w = str_filt(line.strip(), voc_type)
            if 1 <= len(w) <= MAX_LEN:
                words.append(w)
    if not words:
        raise ValueError("word file %s holds no usable word (a word has 1 .. %d characters of voc_type %r)" % (path, MAX_LEN, voc_type))
    return words


def _classes(word, cls):
    if isinstance(word, str):
        try:
            return [cls[ch] for ch in word]
        except KeyError as e:
            raise ValueError("build_char_lm: %r holds %r, which is not in the CRNN's alphabet" % (word, e.args[0]))
    out = [int(c) for c in word]
    if any(not 1 <= c < LM_CLASSES for c in out):
        raise ValueError("build_char_lm: classes 1 .. %d expected, got %r" % (LM_CLASSES - 1, word))
    return out


def build_char_lm(words, order=3, k=4.0):
    """words (strings over the CRNN's alphabet, or sequences of classes 1 .. 36; duplicates count) -> the float32 table of natural
    logs (37 ** (order - 1), 37) of the module docstring.  order 1 .. 3, k > 0 and finite."""
    from ..model.crnn import ALPHABET
    if order not in (1, 2, 3):
        raise ValueError("build_char_lm: order is 1, 2 or 3, got %r" % (order,))
    k = float(k)
    if not (np.isfinite(k) and k > 0):
        raise ValueError("build_char_lm: k must be a finite number > 0, got %r" % (k,))
    cls = {ch: i + 1 for i, ch in enumerate(ALPHABET)}
    C = LM_CLASSES
    n1, n2, n3 = np.zeros(C), np.zeros((C, C)), np.zeros((C, C, C))
    for word in words:
        seq = [0, 0] + _classes(word, cls) + [0]
        if len(seq) < 4:
            raise ValueError("build_char_lm: an empty word")
        for a, b, c in zip(seq, seq[1:], seq[2:]):
            n1[c] += 1
            n2[b, c] += 1
            n3[a, b, c] += 1
    if not n1.sum():
        raise ValueError("build_char_lm: no word")
    p1 = (n1 + 1.0) / (n1.sum() + C)
    if order == 1:
        return np.log(p1)[None, :].astype(np.float32)
    p2 = (n2 + k * p1[None, :]) / (n2.sum(1, keepdims=True) + k)
    if order == 2:
        return np.log(p2).astype(np.float32)
    p3 = (n3 + k * p2[None, :, :]) / (n3.sum(2, keepdims=True) + k)
    return np.log(p3).reshape(C * C, C).astype(np.float32)


def table_order(table):
    """The order of a table by its shape; ValueError for anything that is not (37 ** (order - 1), 37) float32."""
    t = np.asarray(table)
    for order in (1, 2, 3):
        if t.shape == (LM_CLASSES ** (order - 1), LM_CLASSES):
            if t.dtype != np.float32:
                raise ValueError("beam: the model's table must be float32, got %s" % t.dtype)
            return order
    raise ValueError("beam: a model table is (37 ** (order - 1), 37) with order 1 .. %d, got %s" % (MAX_ORDER, t.shape))


def lse(a, b):
    """log(e^a + e^b) as the kernel takes it: m + log(exp(a - m) + exp(b - m)), -inf when both are."""
    m = a if a > b else b
    if m == NEG:
        return NEG
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def log_softmax_rows(rows, n_class):
    """(T, >= n_class) logits -> (T, n_class) float64 log-softmax; the columns at or beyond n_class are not read."""
    x = np.asarray(rows)[:, :n_class].astype(np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def check_limits(T, n_class, width, alpha, beta, table=None):
    """ValueError outside the limits of the module docstring -> the model's order (0 without a table)."""
    if not 1 <= T <= MAX_T or not 2 <= n_class <= MAX_CLASS:
        raise ValueError("beam: 1 .. %d frames and 2 .. %d classes are supported, got T = %d, n_class = %d" % (MAX_T, MAX_CLASS, T, n_class))
    if isinstance(width, bool) or width != int(width) or not 1 <= int(width) <= MAX_WIDTH:
        raise ValueError("beam: the width is an integer 1 .. %d, got %r" % (MAX_WIDTH, width))
    if not (np.isfinite(alpha) and np.isfinite(beta)):
        raise ValueError("beam: alpha and beta must be finite, got %r, %r" % (alpha, beta))
    if table is None:
        return 0
    order = table_order(table)
    if n_class > LM_CLASSES:
        raise ValueError("beam: the model knows %d classes, the logits have %d" % (LM_CLASSES, n_class))
    return order


def beam_np(rows, table=None, width=16, alpha=0.5, beta=0.0, n_class=None, trace=None):
    """One image: rows (T, >= n_class) float32 logits (n_class: default all columns), table: build_char_lm's or None -> (classes (a
    list of ints), score, margin), as the module docstring defines them.  trace: a dict that receives 'dropped', whether any
    candidate was dropped on the way, and 'lp', the log-softmax."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError("beam: one image's (T, >= n_class) logits expected, got %s" % (rows.shape,))
    n_class = rows.shape[1] if n_class is None else int(n_class)
    if rows.shape[1] < n_class:
        raise ValueError("beam: %d columns hold no %d classes" % (rows.shape[1], n_class))
    T = rows.shape[0]
    order = check_limits(T, n_class, width, alpha, beta, table)
    width = int(width)
    if table is None:
        alpha, lm_of = 0.0, None
    else:
        lm_of = np.asarray(table).astype(np.float64)
    alpha, beta = np.float64(alpha), np.float64(beta)
    n_ctx = LM_CLASSES ** max(order - 1, 0)
    lp = log_softmax_rows(rows, n_class)
    # a member: (symbols, pb, pnb, lm, context index)
    beam = [((), np.float64(0.0), np.float64(NEG), np.float64(0.0), 0)]
    margin, dropped = np.inf, False
    for t in range(T):
        where = {p[0]: i for i, p in enumerate(beam)}
        tot = [lse(pb, pnb) for _, pb, pnb, _, _ in beam]
        cands = []                                               # (rank score, parent rank, class, member)
        for i, (sym, pb, pnb, lm, ctx) in enumerate(beam):
            e = sym[-1] if sym else 0
            own = pnb + lp[t, e] if sym else np.float64(NEG)
            j = where.get(sym[:-1]) if sym else None
            if j is not None:
                q = beam[j]
                qe = q[0][-1] if q[0] else 0
                ext = (q[1] if e == qe else tot[j]) + lp[t, e]
            else:
                ext = np.float64(NEG)
            spb, spnb = tot[i] + lp[t, 0], lse(own, ext)
            cands.append((lse(spb, spnb) + lm, i, 0, (sym, spb, spnb, lm, ctx)))
            for c in range(1, n_class):
                if sym + (c,) in where:
                    continue
                v = (pb if c == e else tot[i]) + lp[t, c]
                lmn = lm + (alpha * (lm_of[ctx, c] if lm_of is not None else 0.0) + beta)
                s = v + lmn
                if s == NEG:
                    continue
                cands.append((s, i, c, (sym + (c,), np.float64(NEG), v, lmn, (ctx * LM_CLASSES + c) % n_ctx)))
        cands.sort(key=lambda cand: (-cand[0], cand[1], cand[2]))
        if len(cands) > width:
            dropped = True
            margin = min(margin, cands[width - 1][0] - cands[width][0])
        beam = [cand[3] for cand in cands[:width]]
    final = []
    for i, (sym, pb, pnb, lm, ctx) in enumerate(beam):
        lmf = lm + alpha * (lm_of[ctx, 0] if lm_of is not None else 0.0)
        final.append((lse(pb, pnb) + lmf, i, sym))
    final.sort(key=lambda f: (-f[0], f[1]))
    if len(final) > 1:
        margin = min(margin, final[0][0] - final[1][0])
    if trace is not None:
        trace["dropped"], trace["lp"] = dropped, lp
    return [int(c) for c in final[0][2]], float(final[0][0]), float(margin)


def tolerance(T, n_class, lp, lm_abs=0.0):
    """The tests' threshold tau = 64 eps T (n_class + 2) S with S = max(1, T max|lp| + |lm|): a rank score is the end of a chain of at
    most T frames, each adding one lse over at most n_class + 2 terms (the row's log-sum-exp, and the two lse of a member) of
    magnitude up to S, every operation good to one eps of float64; the 64 is headroom for the device's exp and log, whose error in
    ulp nobody has measured here."""
    S = max(1.0, T * float(np.abs(lp).max()) + abs(float(lm_abs)))
    return 64.0 * np.finfo(np.float64).eps * T * (n_class + 2) * S
