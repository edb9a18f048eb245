"""CPU tests of the definition of the CTC beam search with a character model (utils/beam.py): the model's table, the search against
a brute-force enumeration of every alignment, its relation to utils.confidence's CTC score, what the model changes, and the condition
on the shared inputs (tests/beam_cases.py) that the GPU tests rest on."""
import itertools

import numpy as np
import pytest

import beam_cases as bc
from dpmn_amd.utils import beam as bm
from dpmn_amd.utils import confidence as cf


def _cls(word):
    from dpmn_amd.model.crnn import ALPHABET
    return [ALPHABET.index(ch) + 1 for ch in word]


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("order", [1, 2, 3])
def test_every_row_of_the_table_is_a_distribution(order):
    t = bm.build_char_lm(["clock", "block", "lock", "lock", "7up"], order)
    assert t.dtype == np.float32 and t.shape == (37 ** (order - 1), 37) and np.isfinite(t).all()
    sums = np.exp(t.astype(np.float64)).sum(1)
    # 37 float32 roundings of logs of values <= 1: each shifts its term by at most 2^-24 |log p| p <= 2^-24 / e
    assert np.abs(sums - 1).max() <= 37 * 2.0 ** -24
    assert bm.table_order(t) == order


def test_a_corpus_of_ab_gives_b_after_a():
    a, b = _cls("ab")
    for order in (2, 3):
        t = bm.build_char_lm(["ab"] * 200, order)
        ctx = a if order == 2 else 0 * 37 + a                    # (order 3: the word's second symbol sees (boundary, a))
        assert np.exp(t[ctx, b]) > 0.97
        end = b if order == 2 else a * 37 + b
        assert np.exp(t[end, 0]) > 0.97                          # ... and the word ends after b
    # the counts are weights: a word listed five times counts five times
    once, five = bm.build_char_lm(["ab", "cd"], 2), bm.build_char_lm(["ab"] * 5 + ["cd"], 2)
    assert five[0, a] > once[0, a]


def test_order_1_ignores_the_context():
    t1 = bm.build_char_lm(bc.corpus(), 1)
    assert t1.shape == (1, 37)
    rows = (np.random.RandomState(3).randn(12, 37) * 3).astype(np.float32)
    # an order-2 table whose rows are all the unigram row must read exactly as the order-1 table
    t2 = np.repeat(t1, 37, 0)
    assert bm.beam_np(rows, t1, 8, 0.7, 0.1) == bm.beam_np(rows, t2, 8, 0.7, 0.1)


def test_the_filter_is_the_lexicon_loaders_but_duplicates_count(tmp_path):
    from dpmn_amd.utils.lexicon import load_lexicon
    path = tmp_path / "w.txt"
    path.write_text("Clock\nclock!\n\n  lock \n%s\n%s\nlock\n###\n" % ("a" * 25, "b" * 26), encoding="utf-8")
    words = bm.load_lm_words(str(path), "lower")
    assert words == ["clock", "clock", "lock", "a" * 25, "lock"]
    assert list(dict.fromkeys(words)) == load_lexicon(str(path), "lower")
    empty = tmp_path / "e.txt"
    empty.write_text("###\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no usable word"):
        bm.load_lm_words(str(empty))


def test_limits_raise():
    rows = np.zeros((4, 37), np.float32)
    t = bm.build_char_lm(["ab"], 2)
    for kw in (dict(width=0), dict(width=33), dict(alpha=float("nan")), dict(beta=float("inf"))):
        with pytest.raises(ValueError):
            bm.beam_np(rows, t, **kw)
    with pytest.raises(ValueError):
        bm.beam_np(np.zeros((65, 37), np.float32), None, 4)
    with pytest.raises(ValueError):
        bm.beam_np(np.zeros((4, 65), np.float32), None, 4)
    with pytest.raises(ValueError):
        bm.beam_np(np.zeros((4, 38), np.float32), t, 4)          # a model knows 37 classes
    with pytest.raises(ValueError):
        bm.build_char_lm(["ab"], 4)
    with pytest.raises(ValueError):
        bm.beam_np(rows, np.zeros((37 ** 3, 37), np.float32), 4)


# ------------------------------------------------------------------------------------------------ exhaustive truth
def _brute(lp, table, alpha, beta):
    """Every one of the 3 ** T alignments of a (T, 3) log-posterior, collapsed -> {string: log-likelihood + model score}."""
    T = lp.shape[0]
    order = bm.table_order(table) if table is not None else 0
    mass = {}
    for path in itertools.product(range(3), repeat=T):
        s, prev = [], 0
        for c in path:
            if c != 0 and c != prev:
                s.append(c)
            prev = c
        mass.setdefault(tuple(s), []).append(sum(lp[t, c] for t, c in enumerate(path)))
    out = {}
    for s, logs in mass.items():
        logs = np.array(logs)
        ll = logs.max() + np.log(np.exp(logs - logs.max()).sum())
        lm = beta * len(s)
        if table is not None:
            seq = [0, 0] + list(s) + [0]
            for k in range(2, len(seq)):
                ctx = {1: 0, 2: seq[k - 1], 3: seq[k - 2] * 37 + seq[k - 1]}[order]
                lm += alpha * float(table[ctx, seq[k]])
        out[s] = ll + lm
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("model", [None, 2, 3])
def test_full_width_equals_the_enumeration_of_every_alignment(T, model):
    """3 classes and T <= 4: at most 31 prefixes exist, so a beam of 32 never drops one and the search is exact."""
    table = bm.build_char_lm([(1, 2), (1, 2), (2,), (1, 1, 2)], model) if model else None
    alpha, beta = (0.8, 0.25) if model else (0.0, 0.0)
    for seed in range(6):
        rows = (np.random.RandomState(100 * T + seed).randn(T, 3) * 3).astype(np.float32)
        trace = {}
        got, score, margin = bm.beam_np(rows, table, 32, alpha, beta, trace=trace)
        assert not trace["dropped"]
        truth = _brute(trace["lp"], table, alpha, beta)
        best = max(truth, key=truth.get)
        assert tuple(got) == best and abs(score - truth[best]) <= 1e-12
        second = sorted(truth.values())[-2] if len(truth) > 1 else -np.inf
        assert margin == pytest.approx(truth[best] - second, abs=1e-12)


# ------------------------------------------------------------------------------------------------ against utils.confidence
def _rows(seed, T, n_class):
    return (np.random.RandomState(seed).randn(T, n_class) * 3).astype(np.float32)


def test_score_equals_the_ctc_score_of_the_string_when_nothing_was_dropped():
    """alpha = beta = 0: a prefix that was never dropped has collected every alignment, so its score is log P_CTC(string)."""
    checked = 0
    for T, n_class, width in ((3, 3, 16), (4, 3, 32), (5, 3, 32), (2, 37, 32), (6, 4, 32), (3, 5, 32), (26, 37, 8)):
        for seed in range(4):
            rows = _rows(7 * T + seed, T, n_class)
            trace = {}
            got, score, _ = bm.beam_np(rows, None, width, 0.0, 0.0, trace=trace)
            if trace["dropped"]:
                continue
            checked += 1
            assert abs(score - cf.ctc_word_score(trace["lp"], got)) <= bm.tolerance(T, n_class, trace["lp"])
    assert checked >= 12


@pytest.mark.parametrize("width", [1, 2, 8, 32])
def test_score_never_exceeds_the_ctc_score_of_the_string(width):
    """alpha = beta = 0: a dropped prefix loses alignments, it never gains one."""
    for seed in range(3):
        for T, n_class in ((26, 37), (12, 3)):
            rows = _rows(900 + seed, T, n_class)
            trace = {}
            got, score, _ = bm.beam_np(rows, None, width, 0.0, 0.0, trace=trace)
            assert score <= cf.ctc_word_score(trace["lp"], got) + bm.tolerance(T, n_class, trace["lp"])


def test_width_1_without_a_model_follows_one_prefix():
    """width 1: the result is a valid string of at most T symbols and the margin is finite (something was dropped)."""
    rows = _rows(5, 26, 37)
    got, score, margin = bm.beam_np(rows, None, 1, 0.0, 0.0)
    assert len(got) <= 26 and all(1 <= c < 37 for c in got) and np.isfinite(score) and 0 <= margin < np.inf


# ------------------------------------------------------------------------------------------------ what the model is for
def test_the_model_turns_c1ock_into_clock():
    """Posteriors in which the greedy decode reads c1ock, `1` just above `l` in that frame: without the model the beam search agrees,
    with a model built from clock / block / lock it answers clock."""
    T = 13
    prob = np.full((T, 37), 1e-4)
    word = _cls("c1ock")
    ell = _cls("l")[0]
    for k, c in enumerate(word):
        prob[2 * k + 1, c] = 0.9
        prob[2 * k + 2, 0] = 0.9
    prob[0, 0] = 0.9
    prob[11:, 0] = 0.9
    prob[3, word[1]], prob[3, ell] = 0.5, 0.45
    rows = np.log(prob / prob.sum(1, keepdims=True)).astype(np.float32)
    cls, length = cf.ctc_greedy(rows[None])
    assert cls[0, :length[0]].tolist() == word
    table = bm.build_char_lm(["clock", "block", "lock"], 3)
    assert bm.beam_np(rows, table, 8, 0.0, 0.0)[0] == word
    assert bm.beam_np(rows, None, 8, 1.0, 0.0)[0] == word            # (no model: alpha counts as 0)
    assert bm.beam_np(rows, table, 8, 1.0, 0.0)[0] == _cls("clock")


# ------------------------------------------------------------------------------------------------ --demo_eval counts sr_lm
def test_demo_eval_finds_and_scores_the_sr_lm_column():
    from dpmn_amd.utils import detect_eval as de
    # file, box, label, lr_string, lr_conf, sr_string, sr_conf, sr_lm, sr_lm_score, turned, kept
    rows = [["p", "0", "clock", "c1ock", "0.5", "c1ock", "0.6", "clock", "-3.5", "0", "1"],
            ["p", "1", "x", "y", "0.5", "y", "0.6", "z", "-1", "1", "0"]]
    assert de.row_reads(rows, True, True, False, True, lm=True) == {"p": {0: ("c1ock", None, "clock")}}
    assert de.row_reads(rows, True, True, False, True) == {"p": {0: ("c1ock", None)}}
    # with a lexicon: ..., sr_conf, turned, sr_lexicon, sr_lexicon_score, sr_lm, sr_lm_score
    rows = [["p", "0", "clock", "c1ock", "0.5", "c1ock", "0.6", "0", "block", "-9", "clock", "-3.5"]]
    assert de.row_reads(rows, True, True, True, False, lm=True) == {"p": {0: ("c1ock", "block", "clock")}}
    rows = [["p", "0", "clock", "c1ock", "c1ock", "clock", "-3.5"]]
    assert de.row_reads(rows, lm=True) == {"p": {0: ("c1ock", None, "clock")}}
    square = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)
    photo = {"stem": "p", "det": [square], "det_reads": [("c1ock", None, "clock")], "det_absent": [], "gt": [square], "gt_labels": ["clock"],
             "gt_dont_care": [False]}
    records, totals = de.evaluate([photo], de.region_counts_batch_np, lm=True)
    assert records[0]["e2e_correct"] == 0 and records[0]["e2e_lm_correct"] == 1 and totals["e2e_lm_hmean"] == 1.0
    table = de.csv_rows(records, totals, lm=True)
    assert table[0] == de.CSV_HEAD + de.CSV_LM and table[-1][-3:] == ["1.0000"] * 3
    assert "under the beam search 1 of 1" in de.totals_line(totals, 1)
    plain = de.evaluate([photo], de.region_counts_batch_np)
    assert "e2e_lm_correct" not in plain[0][0] and de.csv_rows(*plain)[0] == de.CSV_HEAD


# ------------------------------------------------------------------------------------------------ the shared cases
def test_at_most_5_percent_of_the_shared_cases_lie_below_the_threshold():
    """A condition on the inputs of tests/beam_cases.py, not a measurement: the GPU tests compare strings only where the definition's
    own margin exceeds tau, and that exclusion may cover at most 5 % of the images."""
    below = total = 0
    for name in bc.CASES:
        c = bc.case(name)
        assert len(c["ref"]) == c["B"]
        for (_, score, margin), tau in zip(c["ref"], c["tau"]):
            assert np.isfinite(score) and margin >= 0 and 0 < tau < 1e-6
            total += 1
            below += int(not margin > tau)
    print("beam cases: %d of %d images below their threshold" % (below, total))
    assert below <= 0.05 * total
