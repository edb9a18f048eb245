"""CPU checks of lexicon-constrained reading (utils/lexicon.py, main.py --rec_lexicon): the NumPy restatement against brute force
and against torch's float64 ctc_loss, the word-file rules, the argument checks, and that the inputs of tests/test_gpu_lexicon.py
leave the index decided."""
import importlib.util
import itertools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dpmn_amd.utils import lexicon as lx
import lexicon_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _collapse(path):
    out, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


def test_ctc_word_logp_equals_enumeration_of_every_alignment():
    T, C = 4, 3
    rng = np.random.RandomState(3)
    logits = rng.randn(2, T, C) * 2
    words = [w for n in (1, 2, 3) for w in itertools.product((1, 2), repeat=n)]
    assert (1, 1) in words and (1, 1, 1) in words            # a doubled letter; 3 + 2 repeats > 4 frames: infeasible
    got = lx.ctc_word_logp(logits, lx.pack_lexicon(words, [1, 2]))
    lp = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
    for b in range(2):
        total = {}
        for path in itertools.product(range(C), repeat=T):
            w = _collapse(path)
            total[w] = total.get(w, 0.0) + np.exp(sum(lp[b, t, c] for t, c in enumerate(path)))
        for j, w in enumerate(words):
            if w in total:
                assert abs(got[b, j] - np.log(total[w])) < 1e-12, w
            else:
                assert got[b, j] == -np.inf, w
    assert got[0, words.index((1, 1, 1))] == -np.inf
    idx, best = lx.ctc_lexicon_best(logits, lx.pack_lexicon([(1, 1, 1), (2, 2, 2)], [1, 2]))
    assert idx.tolist() == [-1, -1] and np.all(best == -np.inf)
    idx, _ = lx.ctc_lexicon_best(logits, lx.pack_lexicon([(1,), (2,), (1,)], [1, 2]))       # equal scores: the lowest index
    assert all(i in (0, 1) for i in idx)


def test_ctc_word_logp_equals_torch_float64_ctc_loss():
    c = cases.ctc_case("ragged_257")
    B, T, L, C = c["B"], c["T"], c["L"], c["n_class"]
    assert (B, T, L) == (3, 26, 257)
    real = torch.from_numpy(c["logits"][:, :, :C].astype(np.float64))
    lp = torch.log_softmax(real, -1).permute(1, 0, 2).repeat_interleave(L, 1)
    nll = F.ctc_loss(lp, torch.from_numpy(c["packed"][:, 1:].astype(np.int64)).repeat(B, 1), torch.full((B * L,), T, dtype=torch.long),
                     torch.from_numpy(c["packed"][:, 0].astype(np.int64)).repeat(B), blank=0, reduction="none")
    got = -nll.numpy().reshape(B, L)
    finite = np.isfinite(c["ref"])
    assert finite.any() and np.array_equal(finite, np.isfinite(got))
    assert np.abs(got[finite] - c["ref"][finite]).max() < 1e-9


def _dp(a, b):
    prev = list(range(len(a) + 1))
    for j, ch in enumerate(b, 1):
        cur = [j]
        for i, ca in enumerate(a, 1):
            cur.append(min(prev[i - 1] + (ca != ch), prev[i] + 1, cur[i - 1] + 1))
        prev = cur
    return prev[-1]


def test_edit_lexicon_best_equals_plain_dp():
    e = cases.edit_case(7, 257)
    assert "" in e["strings"] and any(len(s) == 26 for s in e["strings"])
    ties = 0
    for b, s in enumerate(e["strings"]):
        d = [_dp(s, w) for w in e["words"]]
        assert e["dist"][b] == min(d) and e["idx"][b] == d.index(min(d))
        ties += d.count(min(d)) > 1
    assert ties > 0, "no string with two nearest words: the tie rule is not exercised"
    idx, dist = lx.edit_lexicon_best(lx.pack_strings([""]), lx.pack_lexicon(["abc", "a", "b"]))
    assert idx.tolist() == [1] and dist.tolist() == [1]


def test_load_lexicon_rules_and_pack_round_trip(tmp_path):
    p = tmp_path / "words.txt"
    p.write_text("Hello\nhello\n  WORLD!  \n\n???\n" + "a" * 26 + "\n" + "b" * 25 + "\ncafé\nx9\n", encoding="utf-8")
    words = lx.load_lexicon(str(p))
    assert words == ["hello", "world", "b" * 25, "caf", "x9"]
    assert lx.load_lexicon(str(p), "upper")[:2] == ["Hello", "hello"]
    packed = lx.pack_lexicon(words)
    assert packed.shape == (5, 32) and packed.dtype == np.uint8
    assert packed[0].tolist()[:7] == [5, 18, 15, 22, 22, 25, 0] and not packed[0, 6:].any()       # h e l l o: ALPHABET's numbering, 1-based
    assert lx.unpack_lexicon(packed) == words
    empty = tmp_path / "empty.txt"
    empty.write_text("!!!\n\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no usable word"):
        lx.load_lexicon(str(empty))
    with pytest.raises(ValueError):
        lx.pack_lexicon(["a" * 32])
    with pytest.raises(ValueError):
        lx.pack_lexicon(["A"])
    assert lx.pack_lexicon([(1, 2)], [1, 2]).tolist()[0][:3] == [2, 1, 2]
    assert lx.pack_strings(["Ab-C", "", "z" * 40])[:, 0].tolist() == [3, 0, 31]


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_rec_lexicon_argument_checks(tmp_path):
    m = _main()
    p = tmp_path / "words.txt"
    p.write_text("shop\nSHOP\nexit\n", encoding="utf-8")
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(rec="crnn", test=True, demo_dir=None, demo_tile=False, rec_lexicon=str(p),
                                                        rec_lexicon_mode=None), **kw))
    assert m.rec_lexicon_setting(ns(rec_lexicon=None)) is None
    assert m.rec_lexicon_setting(ns()) == (["shop", "exit"], "score")
    assert m.rec_lexicon_setting(ns(rec="aster")) == (["shop", "exit"], "edit")
    assert m.rec_lexicon_setting(ns(rec="moran", rec_lexicon_mode="edit"))[1] == "edit"
    assert m.rec_lexicon_setting(ns(rec_lexicon_mode="edit"))[1] == "edit"
    with pytest.raises(ValueError, match="needs --rec crnn"):
        m.rec_lexicon_setting(ns(rec="aster", rec_lexicon_mode="score"))
    with pytest.raises(ValueError, match="--demo_tile"):
        m.rec_lexicon_setting(ns(test=False, demo_dir="d", demo_tile=True))
    with pytest.raises(ValueError, match="is not a file"):
        m.rec_lexicon_setting(ns(rec_lexicon=str(tmp_path / "missing.txt")))
    with pytest.raises(ValueError, match="needs --rec_lexicon"):
        m.rec_lexicon_setting(ns(rec_lexicon=None, rec_lexicon_mode="edit"))
    with pytest.raises(ValueError, match="--test or --demo_dir"):
        m.rec_lexicon_setting(ns(test=False))
    bad = tmp_path / "bad.txt"
    bad.write_text("...\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no usable word"):
        m.rec_lexicon_setting(ns(rec_lexicon=str(bad)))
    # main() turns each of them into one SystemExit line before anything touches the GPU
    with pytest.raises(SystemExit, match="main.py: --rec_lexicon_mode score needs --rec crnn"):
        m.main(None, ns(rec="aster", rec_lexicon_mode="score"))
    rows = [["p", "0", "Shop", "", "shop", "shop", "-1.5"], ["p", "1", "exit", "", "exat", "exit", "-2"], ["p", "2", "", "", "q", "shop", "-9"]]
    assert m.lexicon_accuracies(rows) == (2, 0.5, 1.0)


@pytest.mark.parametrize("name", sorted(cases.CTC_CASES))
def test_gpu_test_inputs_leave_the_index_decided(name):
    """The index check of tests/test_gpu_lexicon.py skips images whose float64 top-2 margin is within twice the score bound; at most
    10 % may be.  With these seeds none is."""
    c = cases.ctc_case(name)
    undecided = c["margin"] <= 2 * c["bound"]
    assert undecided.mean() <= 0.10, (c["margin"], c["bound"])
    assert c["e_ref"] < 1e-3
