"""Recogniser confidence (ours; main.py --demo_conf / --demo_upright / --demo_min_conf): the definitions, as a NumPy restatement in
float64 of the kernels of csrc/confidence.hip and of the host extraction for the beam search.  No GPU needed.

Every read has three values: `score`, a natural-log likelihood of the recogniser's own string; `terms`, the number of factors in it;
conf = exp(score / terms), the geometric mean of the per-symbol probabilities, in (0, 1] and comparable across string lengths.
  CTC (CRNN)        score = log P_CTC(greedy string | log_softmax(logits)): the forward recursion over the 2n + 1 extended states --
                    utils.lexicon.ctc_word_logp's quantity for each image's own word of any length 0 <= n <= T; terms = max(n, 1)
                    (CTC has no end symbol; n = 0 gives the sum of the blank log-probabilities)
  greedy attention  score = the sum of log_softmax(logits[t])[ids[t]] over the steps up to and with the first EOS; terms = those steps
  beam (ASTER)      score = the stored sequence score of the returned hypothesis at the step where it ends; terms = its length with EOS
The attention decoders count the EOS because they emit it: ending the word is one of their decisions and has a probability of its own."""
import numpy as np


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _lse(values):
    v = np.asarray(values, np.float64)
    m = v.max()
    if np.isneginf(m):
        return -np.inf
    return float(m + np.log(np.exp(v - m).sum()))


def ctc_greedy(logits):
    """logits (B, T, C) -> (cls (B, T) int64: the arg-max classes (first maximum) with repeats collapsed and blanks (class 0) dropped,
    zero-filled; length (B) int64): dpmn_ctc_greedy_i32's output."""
    best = np.asarray(logits).argmax(-1)
    B, T = best.shape
    cls, length = np.zeros((B, T), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        prev = -1
        for c in best[b].tolist():
            if c != 0 and c != prev:
                cls[b, length[b]] = c
                length[b] += 1
            prev = c
    return cls, length


def ctc_word_score(lp, word):
    """lp (T, C) log-probabilities, word a sequence of n classes (0 <= n; none is the blank 0) -> log of the sum over all CTC
    alignments of the word: alpha over the states blank, w0, blank, w1, ..., blank; a skip over a blank only between different
    labels.  -inf when the word does not fit the T frames."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    word = [int(c) for c in word]
    ext = [0]
    for c in word:
        ext += [c, 0]
    S = len(ext)
    a = np.full(S, -np.inf)
    a[0] = lp[0, 0]
    if S > 1:
        a[1] = lp[0, ext[1]]
    # every state of a frame at once (a tiled line has thousands of states): per state the terms a[s], a[s - 1] and, over a blank
    # between different labels, a[s - 2], summed in this order as _lse sums them; an absent term is -inf and adds exactly 0
    ext = np.array(ext, np.int64)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    for t in range(1, T):
        p1, p2 = np.full(S, -np.inf), np.full(S, -np.inf)
        p1[1:] = a[:-1]
        p2[2:] = np.where(skip[2:], a[:-2], -np.inf)
        m = np.maximum(np.maximum(a, p1), p2)
        live = ~np.isneginf(m)
        ms = np.where(live, m, 0.0)
        with np.errstate(divide="ignore"):      # (a dead state: log(0), replaced by -inf)
            new = np.where(live, ms + np.log((np.exp(a - ms) + np.exp(p1 - ms)) + np.exp(p2 - ms)), -np.inf)
        a = new + lp[t, ext]
    return _lse([a[S - 1]] + ([a[S - 2]] if S > 1 else []))


def ctc_score(logits, cls, length):
    """logits (B, T, C), the collapsed classes (B, T) and lengths (B) of ctc_greedy (or of the kernel: arg-max ties then never enter a
    comparison) -> (score (B) float64, terms (B) int64)."""
    lp = _log_softmax(logits)
    cls, length = np.asarray(cls), np.asarray(length).astype(np.int64)
    score = np.array([ctc_word_score(lp[b], cls[b, :length[b]]) for b in range(lp.shape[0])], np.float64)
    return score, np.maximum(length, 1)


def attn_score(logits, ids, eos):
    """logits (B, steps, C), ids (B, steps), the EOS class -> (score (B) float64, terms (B) int64): with m the first step whose id is
    EOS (or none), the sum of log_softmax(logits[b, t])[ids[b, t]] over t = 0 .. m (over every step without an EOS) and their count."""
    lp = _log_softmax(logits)
    ids = np.asarray(ids).astype(np.int64)
    B, steps = ids.shape
    score, terms = np.zeros(B, np.float64), np.zeros(B, np.int64)
    for b in range(B):
        hit = np.nonzero(ids[b] == eos)[0]
        n = int(hit[0]) + 1 if hit.size else steps
        score[b] = lp[b, np.arange(n), ids[b, :n]].sum()
        terms[b] = n
    return score, terms


def beam_score(symbols, predecessors, scores, batch_size, beam_width, eos):
    """The beam search's stored tables (L, B * K), as utils.labelmaps.beam_backtrack takes them -> (pred_rec (B, L) int64: that
    function's result, score (B) float64, terms (B) int64) of the returned hypothesis of every image: its stored sequence score at
    the step where it ends -- its EOS step, or the last step -- and its length counted with the EOS.  The same walk as
    beam_backtrack, which keeps per kept sequence the step at which it ended beside its score."""
    symbols, predecessors, scores = np.asarray(symbols), np.asarray(predecessors), np.asarray(scores)
    L, K, B = symbols.shape[0], beam_width, batch_size
    order_desc = lambda v: np.argsort(-v, axis=1, kind='stable')
    pos = (np.arange(B) * K)[:, None]
    last = scores[L - 1].reshape(B, K)
    order = order_desc(last)
    s = np.take_along_axis(last, order, 1).copy()
    end = np.full((B, K), L - 1, np.int64)
    found = [0] * B
    back = (order + pos).reshape(-1)
    steps = []
    for t in range(L - 1, -1, -1):
        cur = symbols[t][back].copy()
        back = predecessors[t][back].copy()
        for i in np.nonzero(symbols[t] == eos)[0][::-1].tolist():
            b = i // K
            k = K - (found[b] % K) - 1
            found[b] += 1
            back[b * K + k] = predecessors[t][i]
            cur[b * K + k] = symbols[t][i]
            s[b, k] = scores[t][i]
            end[b, k] = t
        steps.append(cur)
    first = order_desc(s)[:, 0]
    best = first + pos[:, 0]
    rows = np.arange(B)
    rec = np.stack([step[best] for step in reversed(steps)], 1).astype(np.int64)
    return rec, s[rows, first].astype(np.float64), end[rows, first] + 1


def confidence(scores, terms):
    """conf = exp(score / terms) per read, as a list of floats."""
    return [float(np.exp(float(s) / max(int(t), 1))) for s, t in zip(scores, terms)]


def choose_direction(conf_up, str_up, conf_turned, str_turned):
    """Read a region as it is or turned by 180 degrees?  True (turned) iff the turned read is non-empty and either the upright read
    is empty or conf_turned > conf_up.  Ties and two empty reads stay upright."""
    if not str_turned:
        return False
    return (not str_up) or conf_turned > conf_up


def rotate_corners(points):
    """The corner list of a region read from its opposite corner: a quadrilateral's 4 corners rotated by two, a polygon's 2k points
    by k (its bottom edge, walked backwards, becomes the top edge).  -> float64 (n, 2)."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return np.roll(p, -(len(p) // 2), axis=0)


def _number(v):
    v = float(v)
    return "%d" % v if v == int(v) and abs(v) < 1e15 else repr(v)


def box_line(points, text):
    """One line of a box file (utils.quad.read_boxes / utils.poly.numbered_polygons read it back): the coordinates -- an integer as
    an integer, anything else in the shortest form that parses to the same float -- then the transcription; a polygon's (more than 4
    points) behind CTW1500's #### so that a transcription of numbers is never taken for points."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return ",".join(_number(v) for v in p.reshape(-1)) + "," + ("####" if len(p) > 4 else "") + str(text)
