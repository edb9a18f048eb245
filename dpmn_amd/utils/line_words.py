"""A tiled text line read as lexicon words (ours; main.py --rec_lexicon with --demo_tile --demo_line_read): the definition, float64
NumPy on the host, and what the GPU tests compare the kernels of csrc/line_words.hip with.  No GPU needed.

The classical one-pass token-passing Viterbi over "blank gap, word, blank gap, word, ...".  Inputs: line_lp (L, C), a line's
log-posteriors (ops.line_stitch's rows) used AS GIVEN -- not renormalised, -inf entries allowed; words_packed (W, 32), the records
of utils.lexicon.pack_lexicon; penalty, a finite float added once per word (negative: fewer, longer words).  Only + and max occur,
so no NaN can arise and a kernel that does the same operations in float64 gives the same bits.

  model       a line is k >= 0 lexicon words; every frame emits the blank (class 0) or a symbol.  The gap state G is a blank state with
              a self-loop before the first word, between two words and after the last one: at least one G frame separates two words
              (the CRNN has no space class; this also makes `at` + `tea` unambiguous).  A word of n symbols has the states s = 0 ..
              2n - 2: even s is symbol s / 2, odd s an optional blank.  The predecessors of s are s, s - 1 and s - 2, the last only for
              even s whose two symbols differ (utils.lexicon.ctc_word_logp's skip rule).
  frame 0     G[0] = lp[0, 0]; a[w][0][0] = lp[0, c1(w)] + (0.0 + pen), start 0; every other state -inf
  frame t     E[t-1]     = max over w of a[w][2 n_w - 2][t-1]                                   ties: the lowest word index
              G[t]       = lp[t, 0] + max2(G[t-1], E[t-1])                                      tie: stay in G
              a[w][0][t] = lp[t, c1] + max2(a[w][0][t-1], G[t-1] + pen)                         the second choice sets start = t
              a[w][s][t] = lp[t, ext(s)] + max3(a[s][t-1], a[s-1][t-1], a[s-2][t-1] if allowed)  start follows the chosen predecessor
              max2 / max3 return the FIRST maximum in the order written: that is the tie rule.
  end         result = max2(G[L-1], E[L-1])                                                     tie: G
  backtrace   E[t] records its word and that state's start.  A line that ends in E at frame t emits (word, start, t) and goes on in G
              at start - 1 (it stops at start == 0); from G it walks back while the choice was "stay".
  output      (word indices, [(first, last)] spans, score) in reading order; k = 0 is a valid answer, its score the blank column's sum.

Three functions compute it: line_words_np, the per-word form above; build_trie + line_words_trie_np, the same recursion with one
symbol state and one blank-after state per node of the lexicon's prefix trie -- the per-word states of a shared prefix have identical
values and starts, so the trie form returns exactly the per-word form's answer (tests/test_line_words.py asserts it) -- which is the
form the kernels run.  What it cannot do: every frame must be explained by a lexicon word or a gap, so a word outside the list comes
back as its nearest-scoring neighbours, and two words need a blank frame between them."""
import numpy as np

from .lexicon import RECORD

MAX_L, MAX_CLASS = 3201, 64          # csrc/line_words.hip's limits: frames per line, classes
NEG = -np.inf


def _inputs(line_lp, penalty):
    lp = np.asarray(line_lp, np.float64)
    if lp.ndim != 2 or lp.shape[0] < 1 or lp.shape[1] < 1:
        raise ValueError("line_words: line_lp (L >= 1, C >= 1) expected, got %s" % (lp.shape,))
    pen = np.float64(penalty)
    if not np.isfinite(pen):
        raise ValueError("line_words: the penalty must be finite, got %r" % (penalty,))
    return lp, np.float64(0.0) + pen


def _backtrace(L, G_last, E_last, ew, es, gc):
    """ew / es: per frame the word of E[t] and its start; gc[t]: 1 where G[t] came from E[t-1] -> (words, spans, score)."""
    words, spans = [], []
    if E_last > G_last:
        score, t, in_e = E_last, L - 1, True
    else:
        score, t, in_e = G_last, L - 1, False
    enter = np.flatnonzero(np.asarray(gc[:L]))                 # the frames whose G was entered from E
    while True:
        if not in_e:
            k = np.searchsorted(enter, t, side="right") - 1    # the last entered frame <= t: the walk back over "stay"
            if k < 0:
                break
            t = int(enter[k]) - 1
        w, s = int(ew[t]), int(es[t])
        words.append(w)
        spans.append((s, t))
        if s == 0:
            break
        t, in_e = s - 1, False
    return words[::-1], spans[::-1], float(score)


def line_words_np(line_lp, words_packed, penalty=0.0):
    """The per-word form, vectorised over (W, S) -> (word indices, [(first, last)] spans, score)."""
    lp, pen = _inputs(line_lp, penalty)
    words = np.asarray(words_packed, np.uint8).reshape(-1, RECORD)
    W, L = words.shape[0], lp.shape[0]
    n = words[:, 0].astype(np.int64)
    if W < 1 or (n < 1).any() or int(words[:, 1:].max()) >= lp.shape[1]:
        raise ValueError("line_words: words of 1 .. 31 classes below %d expected" % lp.shape[1])
    S = 2 * (RECORD - 1) - 1                                     # 61 states at the most; states > 2n - 2 stay -inf
    ext = np.zeros((W, S), np.int64)
    ext[:, 0::2] = words[:, 1:]
    state = np.arange(S)[None, :]
    live = state <= (2 * n - 2)[:, None]
    skip = np.zeros((W, S), bool)
    skip[:, 2::2] = ext[:, 2::2] != ext[:, 0:-2:2]
    skip &= live
    rows, last = np.arange(W), 2 * n - 2
    a = np.full((W, S), NEG)
    start = np.zeros((W, S), np.int64)
    a[:, 0] = lp[0, ext[:, 0]] + pen
    G = lp[0, 0]
    ew, es, gc = np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64)
    for t in range(1, L + 1):
        ends = a[rows, last]
        w = int(ends.argmax())                                   # (the first maximum: the lowest word index)
        E, ew[t - 1], es[t - 1] = ends[w], w, start[w, last[w]]
        if t == L:
            break
        p1, s1 = np.full((W, S), NEG), np.zeros((W, S), np.int64)
        p1[:, 1:], s1[:, 1:] = a[:, :-1], start[:, :-1]
        p1[:, 0], s1[:, 0] = G + pen, t                          # state 0's second choice: enter from the gap
        p2, s2 = np.full((W, S), NEG), np.zeros((W, S), np.int64)
        p2[:, 2:], s2[:, 2:] = a[:, :-2], start[:, :-2]
        p2[~skip] = NEG
        pick = np.stack([a, p1, p2]).argmax(0)                   # (the first maximum in the order written)
        best = np.where(pick == 0, a, np.where(pick == 1, p1, p2))
        start = np.where(pick == 0, start, np.where(pick == 1, s1, s2))
        a = lp[t][ext] + best
        a[~live] = NEG
        gc[t] = int(E > G)
        G = lp[t, 0] + (E if E > G else G)
    return _backtrace(L, G, E, ew, es, gc)


def build_trie(words_packed):
    """The prefix trie of the records as one int32 table (N, 4): per node [parent (-1 for a first symbol), class, 1 if the class
    equals the parent's class else 0, word index or -1].  Node order: the words are walked in index order and every prefix not seen
    before takes the next number, so a parent always stands before its children and node 0 is the first symbol of word 0."""
    words = np.asarray(words_packed, np.uint8).reshape(-1, RECORD)
    if words.shape[0] < 1 or (words[:, 0] < 1).any() or (words[:, 0] > RECORD - 1).any():
        raise ValueError("build_trie: records of 1 .. 31 symbols expected")
    index, table = {}, []
    for w, rec in enumerate(words.tolist()):
        parent = -1
        for c in rec[1:1 + rec[0]]:
            key = (parent, c)
            v = index.get(key)
            if v is None:
                v = index[key] = len(table)
                table.append([parent, c, int(parent >= 0 and table[parent][1] == c), -1])
            parent = v
        if table[parent][3] < 0:                                 # (distinct words: a repeated one keeps the lower index)
            table[parent][3] = w
    return np.asarray(table, np.int32).reshape(-1, 4)


def line_words_trie_np(line_lp, trie, penalty=0.0):
    """The same recursion over the trie's nodes: per node v a symbol state and a blank-after state,
        sym[v][t] = lp[t, c_v] + max3(sym[v][t-1], blk[parent][t-1], sym[parent][t-1] if the classes differ)
                    (a first symbol: max2(sym[v][t-1], G[t-1] + pen), the second choice sets start = t)
        blk[v][t] = lp[t, 0] + max2(blk[v][t-1], sym[v][t-1])
    and E[t] the best sym of the nodes that end a word (score, then the lower word index).  The CPU reference of ops.line_words."""
    lp, pen = _inputs(line_lp, penalty)
    trie = np.asarray(trie, np.int64).reshape(-1, 4)
    L = lp.shape[0]
    parent, cls, same, word = trie.T
    if int(cls.max()) >= lp.shape[1]:
        raise ValueError("line_words: the trie holds class %d, the line has %d classes" % (int(cls.max()), lp.shape[1]))
    top = parent < 0
    par = np.where(top, 0, parent)
    ends = np.flatnonzero(word >= 0)
    ends = ends[np.argsort(word[ends], kind="stable")]           # by word index: argmax then gives the lowest one
    sym = np.where(top, lp[0, cls] + pen, NEG)
    blk = np.full(len(trie), NEG)
    s_sym, s_blk = np.zeros(len(trie), np.int64), np.zeros(len(trie), np.int64)
    G = lp[0, 0]
    ew, es, gc = np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64)
    for t in range(1, L + 1):
        v = int(ends[sym[ends].argmax()])
        E, ew[t - 1], es[t - 1] = sym[v], word[v], s_sym[v]
        if t == L:
            break
        p1 = np.where(top, G + pen, blk[par])
        s1 = np.where(top, t, s_blk[par])
        p2 = np.where(top | (same != 0), NEG, sym[par])
        pick = np.stack([sym, p1, p2]).argmax(0)
        new_blk = lp[t, 0] + np.where(sym > blk, sym, blk)
        s_blk = np.where(sym > blk, s_sym, s_blk)
        best = np.where(pick == 0, sym, np.where(pick == 1, p1, p2))
        s_sym = np.where(pick == 0, s_sym, np.where(pick == 1, s1, s_sym[par]))
        sym, blk = lp[t, cls] + best, new_blk
        gc[t] = int(E > G)
        G = lp[t, 0] + (E if E > G else G)
    return _backtrace(L, G, E, ew, es, gc)


def decode_records(L, fin, ew, es, gc):
    """The host half of ops.line_words: a line's per-frame records as the kernels write them (ew / es: the word of E[t] and its
    start, gc: 1 where G[t] came from E[t-1]) and fin = (G[L-1], E[L-1]) -> (words, spans, score)."""
    return _backtrace(int(L), np.float64(fin[0]), np.float64(fin[1]), ew, es, gc)
