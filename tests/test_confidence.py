"""Recogniser confidence, the definitions (utils/confidence.py): the CTC score of an image's own string against brute-force enumeration,
utils.lexicon.ctc_word_logp and torch's ctc_loss; the attention score against torch's log_softmax; the beam score on hand-made stored
tables; choose_direction; the corner rotation through the box-file readers; main.py's flag checks.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from dpmn_amd.utils import confidence as cf
from dpmn_amd.utils import lexicon as lx


def _collapse(path):
    out, prev = [], -1
    for c in path:
        if c != 0 and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_ctc_score_equals_brute_force_enumeration(T):
    """All C^T alignments, summed per string they collapse to."""
    C = 3
    rng = np.random.RandomState(10 + T)
    logits = rng.randn(T, C) * 2.0
    lp = cf._log_softmax(logits)
    total = {}
    for path in itertools.product(range(C), repeat=T):
        total.setdefault(_collapse(path), []).append(sum(lp[t, c] for t, c in enumerate(path)))
    assert len(total) > 1 and () in total
    worst = 0.0
    for word, terms in total.items():
        ref = cf._lse(terms)
        got = cf.ctc_word_score(lp, word)
        worst = max(worst, abs(got - ref))
        cls = np.zeros((1, T), np.int64)
        cls[0, :len(word)] = word
        score, n = cf.ctc_score(logits[None], cls, [len(word)])
        assert abs(score[0] - ref) <= 1e-12 and n[0] == max(len(word), 1)
    assert worst <= 1e-12
    # a string that no alignment gives (it needs more frames than T) scores -inf
    assert cf.ctc_word_score(lp, [1] * (T + 1)) == -np.inf


def _random_case():
    rng = np.random.RandomState(5)
    logits = rng.randn(4, 26, 37) * 3.0
    cls, length = cf.ctc_greedy(logits)
    assert length.min() >= 1 and length.max() <= 25
    return logits, cls, length


def test_ctc_score_equals_the_lexicon_restatement():
    logits, cls, length = _random_case()
    score, terms = cf.ctc_score(logits, cls, length)
    packed = np.zeros((4, lx.RECORD), np.uint8)
    for b in range(4):
        packed[b, 0] = length[b]
        packed[b, 1:1 + length[b]] = cls[b, :length[b]]
    ref = lx.ctc_word_logp(logits, packed)
    assert np.abs(score - ref[np.arange(4), np.arange(4)]).max() <= 1e-12
    assert terms.tolist() == length.tolist()


def _torch_ctc(logits, cls, length, dtype=torch.float64):
    B, T, _ = logits.shape
    lp = torch.log_softmax(torch.as_tensor(logits, dtype=dtype), -1).permute(1, 0, 2)
    targets = torch.as_tensor(np.concatenate([cls[b, :length[b]] for b in range(B)]).astype(np.int64))
    nll = torch.nn.functional.ctc_loss(lp, targets, torch.full((B,), T, dtype=torch.long), torch.as_tensor(np.asarray(length), dtype=torch.long),
                                       blank=0, reduction="none", zero_infinity=False)
    return -nll.double().numpy()


def test_ctc_score_equals_torch_ctc_loss_in_float64():
    logits, cls, length = _random_case()
    score, _ = cf.ctc_score(logits, cls, length)
    assert np.abs(score - _torch_ctc(logits, cls, length)).max() <= 1e-10


def crafted_ctc(T=6, C=5, big=6.0):
    """name -> (logits (T, C), the greedy string): all blank, one repeated class, "aa" (the blank between), n = T."""
    def rows(best):
        x = np.full((T, C), -1.0)
        x[np.arange(T), best] = big
        return x + np.linspace(0.0, 0.3, T * C).reshape(T, C)
    return {"all_blank": (rows([0] * T), []), "one_repeated": (rows([2] * T), [2]),
            "aa": (rows([1, 1, 0, 1, 0, 0][:T] if T == 6 else [1, 0, 1] + [0] * (T - 3)), [1, 1]),
            "n_equals_T": (rows([1 + t % (C - 1) for t in range(T)]), [1 + t % (C - 1) for t in range(T)])}


def test_crafted_ctc_cases():
    for name, (logits, word) in crafted_ctc().items():
        cls, length = cf.ctc_greedy(logits[None])
        assert cls[0, :length[0]].tolist() == word, name
        score, terms = cf.ctc_score(logits[None], cls, length)
        lp = cf._log_softmax(logits)
        assert terms[0] == max(len(word), 1)
        assert np.isfinite(score[0]) and score[0] < 0
        if name == "all_blank":
            assert abs(score[0] - lp[:, 0].sum()) <= 1e-12
        if name == "n_equals_T":      # one alignment only
            assert abs(score[0] - lp[np.arange(len(word)), word].sum()) <= 1e-12
        if name == "aa":              # every alignment keeps a blank between the two: the path without one is not counted
            T = logits.shape[0]
            paths = [p for p in itertools.product(range(logits.shape[1]), repeat=T) if _collapse(p) == (1, 1)]
            assert all(0 in p for p in paths)
            assert abs(score[0] - cf._lse([sum(lp[t, c] for t, c in enumerate(p)) for p in paths])) <= 1e-12
        assert abs(score[0] - _torch_ctc(logits[None], cls, length)[0]) <= 1e-10
        conf = cf.confidence(score, terms)[0]
        assert 0.0 < conf <= 1.0


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_attn_score_equals_torch_log_softmax_gather(where):
    B, steps, C, eos = 3, 7, 11, 10
    rng = np.random.RandomState(3)
    logits = rng.randn(B, steps, C) * 2.0
    logits[..., eos] -= 50.0                                   # no EOS by chance
    if where != "absent":
        logits[:, 0 if where == "first" else steps - 1, eos] += 100.0
    ids = logits.argmax(-1)
    score, terms = cf.attn_score(logits, ids, eos)
    n = {"first": 1, "last": steps, "absent": steps}[where]
    assert terms.tolist() == [n] * B
    assert (ids == eos).any() == (where != "absent")
    lp = torch.log_softmax(torch.as_tensor(logits, dtype=torch.float64), -1).gather(2, torch.as_tensor(ids)[..., None])[..., 0]
    assert np.abs(score - lp[:, :n].sum(1).numpy()).max() <= 1e-12
    assert all(0.0 < c <= 1.0 for c in cf.confidence(score, terms))


def beam_tables(early):
    """A hand-made stored table of B = 1, K = 2, L = 3 with EOS = 9.  early: the winner emits EOS at step 1 (score -0.5; the beams of
    the last step score -2 and -3); otherwise no EOS before the last step, where beam 0 emits it with the best score -1.25."""
    eos = 9
    if early:
        sym = np.array([[3, 4], [9, 5], [6, 7]])
        pred = np.array([[0, 0], [0, 1], [1, 1]])
        sc = np.array([[-0.1, -0.4], [-0.5, -0.9], [-2.0, -3.0]], np.float32)
        return sym, pred, sc, eos, [3, 9], -0.5, 2
    sym = np.array([[3, 4], [5, 2], [9, 7]])
    pred = np.array([[0, 0], [1, 0], [0, 1]])
    sc = np.array([[-0.1, -0.4], [-0.6, -0.9], [-1.25, -3.0]], np.float32)
    return sym, pred, sc, eos, [4, 5, 9], -1.25, 3


@pytest.mark.parametrize("early", [True, False])
def test_beam_score_on_a_hand_made_table(early):
    from dpmn_amd.utils.labelmaps import beam_backtrack
    sym, pred, sc, eos, want, score, terms = beam_tables(early)
    rec, s, n = cf.beam_score(sym, pred, sc, 1, 2, eos)
    assert np.array_equal(rec, beam_backtrack(sym, pred, sc, 1, 2, eos))
    assert rec[0, :len(want)].tolist() == want
    assert s.tolist() == [score] and n.tolist() == [terms]
    assert abs(cf.confidence(s, n)[0] - np.exp(score / terms)) <= 1e-15


def test_choose_direction_truth_table():
    ch = cf.choose_direction
    assert ch(0.2, "ab", 0.9, "cd") is True
    assert ch(0.9, "ab", 0.2, "cd") is False
    assert ch(0.5, "ab", 0.5, "cd") is False            # a tie stays upright
    assert ch(0.9, "", 0.1, "cd") is True               # an empty upright read loses to any turned read
    assert ch(0.1, "ab", 0.9, "") is False              # an empty turned read never wins
    assert ch(0.3, "", 0.9, "") is False                # two empty reads stay upright


def test_rotated_corners_parse_back_through_the_box_readers(tmp_path):
    from dpmn_amd.utils import poly, quad
    q = np.array([[3, 5], [67.5, 5], [67, 21.25], [3, 21]], np.float64)
    k = 7
    top = [(10.0 + 9 * i, 20.0 + (i - 3) ** 2 * 0.5) for i in range(k)]
    bottom = [(10.0 + 9 * i, 34.0 + (i - 3) ** 2 * 0.5) for i in range(k)][::-1]
    p = np.array(top + bottom, np.float64)
    rq, rp = cf.rotate_corners(q), cf.rotate_corners(p)
    assert np.array_equal(rq, q[[2, 3, 0, 1]])
    assert np.array_equal(rp, np.concatenate([p[k:], p[:k]])) and np.array_equal(cf.rotate_corners(rp), p)
    f = tmp_path / "b.txt"
    f.write_text(cf.box_line(rq, "word") + "\n" + cf.box_line(q, "2015") + "\n" + cf.box_line(rp, "1234") + "\n" + cf.box_line(q, "") + "\n")
    assert f.read_text().splitlines()[0] == "67,21.25,3,21,3,5,67.5,5,word"
    boxes = quad.numbered_boxes(str(f))
    assert np.array_equal(boxes[0][2], rq) and boxes[0][3] == "word" and boxes[1][3] == "2015"
    polys = poly.numbered_polygons(str(f))
    assert [len(x[2]) for x in polys] == [4, 4, 2 * k, 4]
    assert np.array_equal(polys[0][2], rq) and np.array_equal(polys[2][2], rp)
    assert [x[3] for x in polys] == ["word", "2015", "1234", " "]


def _args(**kw):
    import argparse
    base = dict(demo_dir=None, demo_tile=False, demo_boxes=None, demo_detect=False, demo_conf=False, demo_upright=False, demo_min_conf=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_demo_conf_setting_accepts_and_refuses():
    import main
    s = main.demo_conf_setting
    assert s(_args()) is None and s(_args(demo_dir="d", demo_tile=True)) is None
    assert s(_args(demo_dir="d", demo_conf=True)) == {"confidence": True, "upright": False, "min_conf": None}
    assert s(_args(demo_dir="d", demo_upright=True)) == {"confidence": True, "upright": True, "min_conf": None}
    assert s(_args(demo_dir="d", demo_boxes="b", demo_min_conf=0.25)) == {"confidence": True, "upright": False, "min_conf": 0.25}
    assert s(_args(demo_dir="d", demo_detect=True, demo_min_conf=0.5, demo_upright=True))["min_conf"] == 0.5
    for flag in (dict(demo_conf=True), dict(demo_upright=True), dict(demo_min_conf=0.5, demo_boxes="b")):
        with pytest.raises(ValueError) as e:
            s(_args(**flag))
        assert str(e.value) == main.DEMO_CONF_NEEDS_DIR[len("main.py: "):] and "\n" not in str(e.value)
        with pytest.raises(ValueError) as e:
            s(_args(demo_dir="d", demo_tile=True, **flag))
        assert str(e.value) == main.DEMO_CONF_OR_TILE[len("main.py: "):] and "\n" not in str(e.value)
    with pytest.raises(ValueError) as e:
        s(_args(demo_dir="d", demo_min_conf=0.5))
    assert str(e.value) == main.DEMO_MIN_CONF_NEEDS_BOXES[len("main.py: "):]
    for c in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError) as e:
            s(_args(demo_dir="d", demo_boxes="b", demo_min_conf=c))
        assert str(e.value) == main.DEMO_MIN_CONF_RANGE[len("main.py: "):]


def test_demo_refuses_a_plain_callable_and_bad_settings():
    """TextSR._conf_reader, which demo calls before anything else: one ValueError line each."""
    from dpmn_amd.interfaces.super_resolution import TextSR

    class Stub:
        def read_conf(self, images):
            return ["ab"], [np.log(0.25)], [2]
    r = TextSR._conf_reader
    assert r(lambda x: [""], False, False, False, False, None) is None
    with pytest.raises(ValueError, match="a plain callable returns no score"):
        r(lambda x: [""], False, False, True, False, None)
    with pytest.raises(ValueError, match="tile=True"):
        r(Stub(), True, False, False, True, None)
    with pytest.raises(ValueError, match="min_conf needs boxes=True"):
        r(Stub(), False, False, False, False, 0.5)
    with pytest.raises(ValueError, match=r"min_conf must lie in \(0, 1\)"):
        r(Stub(), False, True, False, False, 1.0)
    strings, conf = r(Stub(), False, True, False, False, 0.5)(None)
    assert strings == ["ab"] and abs(conf[0] - 0.5) <= 1e-15
