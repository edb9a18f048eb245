"""A tiled line read as lexicon words (utils/line_words.py): the float64 NumPy definition against a hand-built alignment and a brute
force, its trie form against its per-word form, the tie rules, the edge cases, and the flags of main.py and TextSR.demo.  No GPU."""
import argparse
import types

import numpy as np
import pytest

from dpmn_amd.utils import lexicon as lx
from dpmn_amd.utils import line_words as lw

ABC = "abc"                                     # a 3-class alphabet for the brute force: classes 1 .. 3, blank 0
LETTERS = "aesto"                               # the seeded cases' alphabet: classes 1 .. 5


def _sharp(classes, C=37, p=0.9):
    lp = np.full((len(classes), C), np.log((1.0 - p) / (C - 1)))
    lp[np.arange(len(classes)), classes] = np.log(p)
    return lp


def test_hand_built_alignment():
    """cat, two blanks, dog: exactly those words and spans; the score is the alignment's sum in frame order, pen added per word."""
    packed = lx.pack_lexicon(["dog", "cat", "cot"])
    cat, dog = packed[1, 1:4].tolist(), packed[0, 1:4].tolist()
    lp = _sharp(cat + [0, 0] + dog)
    for pen in (0.0, -0.5):
        words, spans, score = lw.line_words_np(lp, packed, pen)
        assert words == [1, 0] and spans == [(0, 2), (5, 7)]
        acc = lp[0, cat[0]] + (0.0 + pen)
        acc = lp[1, cat[1]] + acc
        acc = lp[2, cat[2]] + acc
        acc = lp[3, 0] + acc
        acc = lp[4, 0] + acc
        acc = lp[5, dog[0]] + (acc + pen)
        acc = lp[6, dog[1]] + acc
        acc = lp[7, dog[2]] + acc
        assert score == acc
        assert lw.line_words_trie_np(lp, lw.build_trie(packed), pen) == (words, spans, score)


def _brute(lp, words, pen):
    """Every word sequence and every alignment, by walking the automaton forwards: -> (best score, the word lists that reach it).
    Two word lists can share one labelling of the frames (a b _ a _ b is `ab`, `ab` and `aba`, `b`): the same additions in the same
    order, an exact tie, which only the recursion's tie rules settle; so the best may be reached by more than one list."""
    L = len(lp)
    best = [-np.inf, []]

    def end(score, seq):
        if score > best[0]:
            best[0], best[1] = score, [seq]
        elif score == best[0] and seq not in best[1]:
            best[1].append(seq)

    def walk(t, state, score, seq):
        # state: None = the gap, else (word, s)
        if t == L:
            if state is None or state[1] == 2 * len(words[state[0]]) - 2:
                end(score, seq)
            return
        if state is None:
            walk(t + 1, None, lp[t, 0] + score, seq)
            for w, word in enumerate(words):
                walk(t + 1, (w, 0), lp[t, word[0]] + (score + pen), seq + [w])
            return
        w, s = state
        word = words[w]
        last = 2 * len(word) - 2
        walk(t + 1, (w, s), lp[t, word[s // 2] if s % 2 == 0 else 0] + score, seq)
        if s < last:
            walk(t + 1, (w, s + 1), lp[t, 0 if s % 2 == 0 else word[(s + 1) // 2]] + score, seq)
        if s % 2 == 0 and s + 2 <= last and word[s // 2] != word[s // 2 + 1]:
            walk(t + 1, (w, s + 2), lp[t, word[s // 2 + 1]] + score, seq)
        if s == last:
            walk(t + 1, None, lp[t, 0] + score, seq)

    # frame 0: the gap, or a word's first symbol
    walk(1, None, lp[0, 0], [])
    for w, word in enumerate(words):
        walk(1, (w, 0), lp[0, word[0]] + (0.0 + pen), [w])
    return best[0], best[1]


def test_brute_force():
    rng = np.random.RandomState(20)
    lexicons = [["a"], ["ab", "b"], ["aa", "a", "ba"], ["abc", "ca"], ["c", "cb", "bcc"], ["aba", "ab", "b"]]
    n = unique = 0
    for lex in lexicons:
        packed = lx.pack_lexicon(lex, ABC)
        classes = [[ABC.index(ch) + 1 for ch in w] for w in lex]
        for L in range(1, 8):
            for pen in (0.0, -1.5):
                lp = rng.randn(L, 4) * 2.0
                words, spans, score = lw.line_words_np(lp, packed, pen)
                ref_score, ref_words = _brute(lp, classes, pen)
                assert score == ref_score and words in ref_words, (lex, L, pen)
                unique += len(ref_words) == 1
                assert lw.line_words_trie_np(lp, lw.build_trie(packed), pen) == (words, spans, score)
                assert all(a <= b for a, b in spans) and all(spans[i][1] + 1 < spans[i + 1][0] for i in range(len(spans) - 1))
                n += 1
    assert n == len(lexicons) * 7 * 2 and unique >= n - 10          # (nearly every best is a single word list: there the words are the same)


SEEDED = [["a", "at", "ate"], ["see", "ee", "s"], ["at", "tea"], ["toast"], ["a", "at", "ate", "see", "ee", "at", "tea", "oat", "so"][:5] + ["tea", "oat", "so"],
          ["seat", "sea", "eat", "tee", "toe", "to", "too", "o"]]


def test_trie_form_equals_the_per_word_form():
    rng = np.random.RandomState(7)
    n = 0
    for lex in SEEDED:
        packed = lx.pack_lexicon(lex, LETTERS)
        trie = lw.build_trie(packed)
        for L in (1, 2, 3, 5, 9, 26, 27):
            for rep in range(5):
                pen = (0.0, -1.5, 0.75, -0.25, 2.0)[rep]
                lp = rng.randn(L, 6) * (3.0 if rep % 2 else 1.0)
                lp -= np.log(np.exp(lp).sum(1, keepdims=True))
                got = lw.line_words_trie_np(lp, trie, pen)
                assert got == lw.line_words_np(lp, packed, pen), (lex, L, pen)
                n += 1
    assert n >= 200


def test_build_trie_tables():
    trie = lw.build_trie(lx.pack_lexicon(["at", "a", "ate", "see"], LETTERS))
    a, e, s, t = (LETTERS.index(ch) + 1 for ch in "aest")
    assert trie.dtype == np.int32 and trie.tolist() == [[-1, a, 0, 1], [0, t, 0, 0], [1, e, 0, 2], [-1, s, 0, -1], [3, e, 0, -1], [4, e, 1, 3]]
    with pytest.raises(ValueError, match="1 .. 31"):
        lw.build_trie(np.zeros((1, 32), np.uint8))


def _dyadic(rows):
    return np.asarray(rows, np.float64)


def test_ties():
    """lp in multiples of 0.25, not normalised: every sum is exact, so the ties are real ties."""
    both = lambda lp, packed, pen=0.0: (lw.line_words_np(lp, packed, pen), lw.line_words_trie_np(lp, lw.build_trie(packed), pen))
    # stay beats enter: `a` may start at frame 0 or at frame 1 for the same score (blank and `a` cost the same)
    packed = lx.pack_lexicon(["a"], ABC)
    lp = _dyadic([[-1.0, -1.0, -8, -8], [-8, -0.5, -8, -8]])
    got, got_trie = both(lp, packed)
    assert got == got_trie == ([0], [(0, 1)], -1.5)
    # G beats E at the end: a line of equal blank and symbol columns reads no word
    lp = _dyadic([[-1.0, -1.0, -8, -8]])
    got, got_trie = both(lp, packed)
    assert got == got_trie == ([], [], -1.0)
    lp = _dyadic([[-1.0, -0.75, -8, -8]])
    assert both(lp, packed)[0] == ([0], [(0, 0)], -0.75)
    # ... and stay in G beats entering it from E: blank, then (blank | a) tie, then blank
    lp = _dyadic([[-1.0, -1.0, -8, -8], [-0.5, -8, -8, -8]])
    got, got_trie = both(lp, packed)
    assert got == got_trie == ([], [], -1.5)
    # equal word ends go to the lower index
    for order in (["b", "a"], ["a", "b"]):
        packed = lx.pack_lexicon(order, ABC)
        lp = _dyadic([[-4.0, -0.5, -0.5, -8]])
        got, got_trie = both(lp, packed)
        assert got == got_trie == ([0], [(0, 0)], -0.5)
    # predecessor order decides start: `ab` over three frames, a a b or a b b score the same, and so does entering late
    packed = lx.pack_lexicon(["ab"], ABC)
    lp = _dyadic([[-1.0, -1.0, -8, -8], [-8, -0.5, -0.5, -8], [-8, -8, -0.25, -8]])
    got, got_trie = both(lp, packed)
    assert got == got_trie == ([0], [(0, 2)], -1.75)
    # the same with a penalty that is itself dyadic
    got, got_trie = both(lp, packed, -0.25)
    assert got == got_trie == ([0], [(0, 2)], -2.0)


def test_edge_cases():
    packed = lx.pack_lexicon(["ee"], LETTERS)
    e = LETTERS.index("e") + 1
    # `ee` needs e, blank, e: it does not fit two frames
    lp = _sharp([e, e], C=6)
    for f in (lw.line_words_np, lambda a, b, c=0.0: lw.line_words_trie_np(a, lw.build_trie(b), c)):
        words, spans, score = f(lp, packed)
        assert words == [] and spans == [] and score == lp[0, 0] + lp[1, 0]
        assert f(_sharp([e, 0, e], C=6), packed)[:2] == ([0], [(0, 2)])
    # a line too short for every word: k = 0 and the blank column's sum
    packed = lx.pack_lexicon(["toast", "seat"], LETTERS)
    lp = np.random.RandomState(3).randn(3, 6)
    words, spans, score = lw.line_words_np(lp, packed)
    assert (words, spans) == ([], []) and score == lp[2, 0] + (lp[1, 0] + lp[0, 0])
    assert lw.line_words_trie_np(lp, lw.build_trie(packed)) == (words, spans, score)
    # -inf columns: no NaN, and a line whose blank column is -inf where no word fits scores -inf
    packed = lx.pack_lexicon(["at", "tea"], LETTERS)
    a, t = LETTERS.index("a") + 1, LETTERS.index("t") + 1
    lp = np.full((4, 6), -np.inf)
    lp[[0, 1, 2, 3], [a, t, 0, 0]] = [-0.5, -0.25, -1.0, -1.0]
    with np.errstate(all="raise"):
        got = lw.line_words_np(lp, packed)
        assert got == lw.line_words_trie_np(lp, lw.build_trie(packed)) == ([0], [(0, 1)], -2.75)
        lp[:, 0] = -np.inf
        got = lw.line_words_np(lp, packed)
        # (G[2] = -inf + max2(-inf, E[1]) is -inf, and its recorded choice is still E[1] > G[1]: the walk back finds `at`)
        assert got == lw.line_words_trie_np(lp, lw.build_trie(packed)) == ([0], [(0, 1)], -np.inf)
    with pytest.raises(ValueError, match="finite"):
        lw.line_words_np(lp, packed, np.inf)
    with pytest.raises(ValueError, match="classes"):
        lw.line_words_np(lp[:, :3], packed)


# ------------------------------------------------------------------------------------------------ settings
def _ns(path, **kw):
    base = dict(rec="crnn", test=False, demo_dir="d", demo_tile=True, demo_line_read=True, rec_lexicon=path, rec_lexicon_mode=None,
                rec_lexicon_penalty=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_main_settings(tmp_path):
    import main
    p = tmp_path / "words.txt"
    p.write_text("shop\nexit\n", encoding="utf-8")
    path = str(p)
    assert main.rec_lexicon_setting(_ns(path)) == (["shop", "exit"], "score")
    assert main.rec_lexicon_setting(_ns(path, rec_lexicon_mode="score"), load=False) == (None, "score")
    with pytest.raises(ValueError) as e:
        main.rec_lexicon_setting(_ns(path, rec_lexicon_mode="edit"))
    assert "--rec_lexicon_mode edit does not combine" in str(e.value) and "\n" not in str(e.value)
    # without --demo_line_read the present error stays, word for word
    with pytest.raises(ValueError) as e:
        main.rec_lexicon_setting(_ns(path, demo_line_read=False))
    assert str(e.value) == "--rec_lexicon does not combine with --demo_tile: a window of a line is not a word"
    # the penalty: finite, and only with its two flags
    assert main.rec_lexicon_penalty(_ns(path)) == 0.0 and main.rec_lexicon_penalty(argparse.Namespace()) == 0.0
    assert main.rec_lexicon_penalty(_ns(path, rec_lexicon_penalty=-1.5)) == -1.5
    assert main.rec_lexicon_setting(_ns(path, rec_lexicon_penalty=-1.5))[1] == "score"
    for kw in (dict(rec_lexicon=None), dict(demo_line_read=False, demo_tile=False), dict(rec_lexicon_penalty=float("nan")),
               dict(rec_lexicon_penalty=float("inf"))):
        with pytest.raises(ValueError) as e:
            main.rec_lexicon_penalty(_ns(path, **dict(dict(rec_lexicon_penalty=0.5), **kw)))
        assert "--rec_lexicon_penalty" in str(e.value) and "\n" not in str(e.value), kw
    with pytest.raises(ValueError, match="--rec_lexicon_penalty"):
        main.rec_lexicon_setting(_ns(path, rec_lexicon_penalty=float("nan")))
    # labels and reads are compared without their spaces in the line-read branch only
    rows = [["p", "0", "Fish & Chips", "", "fish chips", "fish chips", "-1"], ["p", "1", "exit", "", "ex it", "exit", "-2"]]
    assert main.lexicon_accuracies(rows, spaces=False) == (2, 1.0, 1.0)
    assert main.lexicon_accuracies(rows) == (2, 0.0, 0.5)


class _Lines:
    def read(self, images):
        return [""]

    def __call__(self, images):
        return [""]

    def window_rows(self, images):
        raise AssertionError("not reached")

    def read_lines(self, rows, plan, gap=0, lr_w=64, lexicon=None, penalty=0.0):
        raise AssertionError("not reached")


def test_demo_checks(tmp_path):
    from dpmn_amd.interfaces.super_resolution import TextSR
    sr = object.__new__(TextSR)
    lex = lambda mode=None: types.SimpleNamespace(mode=mode, words=["a"])
    demo = lambda **kw: TextSR.demo(sr, [], None, iter(()), str(tmp_path / "out"), **kw)
    for kw, text in ((dict(rec=_Lines(), tile=True, lexicon=lex()), "demo: a lexicon does not combine with tile=True (a window of a line is not a word)"),
                     (dict(rec=_Lines(), tile=True, line_read=True, lexicon=lex("edit")), "mode 'edit' does not combine"),
                     (dict(rec=lambda x: [""], tile=True, line_read=True, lexicon=lex()), "window_rows"),
                     (dict(rec=_Lines(), tile=True, line_read=True, lexicon=lex(), lexicon_penalty=float("inf")), "lexicon_penalty must be finite"),
                     (dict(rec=_Lines(), tile=True, line_read=True, lexicon_penalty=-1.0), "lexicon_penalty needs a lexicon"),
                     (dict(rec=_Lines(), lexicon_penalty=-1.0), "lexicon_penalty needs a lexicon")):
        with pytest.raises(ValueError) as e:
            demo(**kw)
        assert text in str(e.value) and "\n" not in str(e.value), kw
    assert not (tmp_path / "out").exists()
    # accepted: the checks pass and the (empty) run writes its header with the lexicon's two columns
    for mode in (None, "score"):
        out = tmp_path / ("ok_%s" % mode)
        rows = TextSR.demo(sr, [], None, iter(()), str(out), rec=_Lines(), text_prior_fn=lambda *a: None, tile=True, chunk=2, line_read=True,
                           lexicon=lex(mode), lexicon_penalty=-0.5)
        assert rows == [] and (out / "demo_result.csv").read_text().split() == ["file,lr_string,sr_string,sr_lexicon,sr_lexicon_score"]
