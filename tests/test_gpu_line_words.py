"""A tiled line read as lexicon words on the GPU (csrc/line_words.hip): dpmn_line_words_f64's two arms against the float64 NumPy
definition (utils/line_words.py) with ==, NativeCRNN.read_lines(lexicon=...), then main.py with --rec_lexicon --demo_tile
--demo_line_read."""
import csv
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import lexicon as lx
from dpmn_amd.utils import line_words as lw

pytestmark = pytest.mark.gpu

C, LD = 37, 40
SHORT = (1, 2, 27)                              # the lines of a batch, in frames
BATCH = SHORT + (401,)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _alphabet():
    from dpmn_amd.model.crnn import ALPHABET
    return ALPHABET


@functools.lru_cache(maxsize=None)
def words_with_nodes(n):
    """distinct words over the CRNN's alphabet whose prefix trie has exactly n nodes (seeded by n)"""
    rng = np.random.RandomState(n)
    abc = _alphabet()
    prefixes, words = set(), []
    while len(prefixes) < n:
        left = n - len(prefixes)
        if left > 8 or not words:
            w = "".join(abc[i] for i in rng.randint(0, 8, rng.randint(1, min(left, 6) + 1)))
        else:
            w = words[rng.randint(len(words))][:20] + abc[rng.randint(0, 36)]
        new = {w[:i] for i in range(1, len(w) + 1)} - prefixes
        if w in words or not 0 < len(new) <= left:
            continue
        words.append(w)
        prefixes |= new
    assert len(lw.build_trie(lx.pack_lexicon(words))) == n
    return tuple(words)


@functools.lru_cache(maxsize=None)
def lines_lp(Ls, seed, scale=3.0):
    """the float32 log-posteriors of a batch of lines inside rows of leading dimension LD, the padding columns at 1e4"""
    rng = np.random.RandomState(seed)
    x = rng.randn(sum(Ls), C) * scale
    x[:, 0] += 1.0
    x = x - np.log(np.exp(x).sum(1, keepdims=True))
    out = np.full((sum(Ls), LD), 1e4, np.float32)
    out[:, :C] = x
    return out, np.stack([np.concatenate(([0], np.cumsum(Ls[:-1]))), Ls], 1).astype(np.int64)


def _reference(lp, table, packed, pen):
    return [lw.line_words_np(lp[f0:f0 + L].astype(np.float64), packed, pen) for f0, L in table.tolist()]


def _bits(reads):
    return [(w, s, np.float64(x).view(np.int64).item()) for w, s, x in reads]


def _run(dev, lex, lp_ld, table, pen, arm=None, width=C):
    from dpmn_amd import ops
    d = torch.from_numpy(lp_ld).to(dev)
    return ops.line_words(d[:, :width], ops.LineTable(table), lex, pen, arm=arm)


@pytest.mark.parametrize("where", ["block-1", "block", "block+1", "lds-1", "lds", "lds+1", "one word"])
def test_line_words_equals_the_restatement_in_both_arms(dev, where):
    """The node counts sit on the edges of both arms: a block of the frame-per-launch arm, the LDS of the single-launch arm.  Each
    arm that can run gives the restatement's words, spans and score bits; `None` is the dispatch."""
    from dpmn_amd import _abi, ops
    block, lds = ops.LINE_WORDS_BLOCK, ops.line_words_lds_nodes(dev)
    assert block == 256 and lds > block + 1
    if where == "one word":
        words = ("tea",)
    else:
        base = where.rstrip("+-1")
        words = words_with_nodes({"block": block, "lds": lds}[base] + {"": 0, "-1": -1, "+1": 1}[where[len(base):]])
    lex = ops.Lexicon(list(words))
    nodes = len(lex.trie)
    Ls = BATCH if nodes <= block + 1 else SHORT                     # (the float64 reference of a large lexicon takes its time)
    lp, table = lines_lp(Ls, 11)
    pen = -0.75
    ref = _bits(_reference(lp[:, :C], table, lex.packed, pen))
    assert ops.line_words_arm(nodes, dev) == ("lds" if nodes <= lds else "step")
    for arm in (None, "step", "lds"):
        if arm == "lds" and nodes > lds:
            with pytest.raises(_abi.DpmnError, match="does not fit the single-launch arm"):
                _run(dev, lex, lp, table, pen, arm)
            continue
        got = _bits(_run(dev, lex, lp, table, pen, arm))
        assert got == ref, (where, arm)
    print("line_words %s: %d words, %d nodes, lines %s, words per line %s" % (where, len(words), nodes, Ls, [len(r[0]) for r in ref]))
    assert any(r[0] for r in ref)


def test_line_words_ties_and_the_longest_line(dev):
    from dpmn_amd import ops
    abc = "abc"
    cases = [(["a"], [[-1.0, -1.0, -8, -8], [-8, -0.5, -8, -8]], 0.0, ([0], [(0, 1)], -1.5)),                 # stay beats enter
             (["a"], [[-1.0, -1.0, -8, -8]], 0.0, ([], [], -1.0)),                                            # G beats E at the end
             (["a"], [[-1.0, -1.0, -8, -8], [-0.5, -8, -8, -8]], 0.0, ([], [], -1.5)),                        # stay in G beats E
             (["b", "a"], [[-4.0, -0.5, -0.5, -8]], 0.0, ([0], [(0, 0)], -0.5)),                              # the lower index
             (["a", "b"], [[-4.0, -0.5, -0.5, -8]], 0.0, ([0], [(0, 0)], -0.5)),
             (["ab"], [[-1.0, -1.0, -8, -8], [-8, -0.5, -0.5, -8], [-8, -8, -0.25, -8]], -0.25, ([0], [(0, 2)], -2.0))]
    for words, rows, pen, want in cases:
        lex = ops.Lexicon(words, alphabet=abc)
        lp = np.asarray(rows, np.float32)
        assert lw.line_words_np(lp, lex.packed, pen) == want
        for arm in ("step", "lds"):
            d = torch.from_numpy(lp).to(dev)
            assert ops.line_words(d, [[0, len(lp)]], lex, pen, arm=arm) == [want], (words, arm)
    # -inf columns: no NaN
    lex = ops.Lexicon(["at", "tea"])
    a, t = (_alphabet().index(ch) + 1 for ch in "at")
    lp = np.full((4, C), -np.inf, np.float32)
    lp[[0, 1, 2, 3], [a, t, 0, 0]] = [-0.5, -0.25, -1.0, -1.0]
    for arm in ("step", "lds"):
        assert ops.line_words(torch.from_numpy(lp).to(dev), [[0, 4]], lex, arm=arm) == [([0], [(0, 1)], -2.75)]
    # one line of 3201 frames, three words
    lex = ops.Lexicon(["at", "tea", "a"])
    lp, table = lines_lp((lw.MAX_L,), 5, scale=1.0)
    ref = _bits(_reference(lp[:, :C], table, lex.packed, 0.0))
    assert len(ref[0][0]) > 100
    for arm in ("step", "lds"):
        assert _bits(_run(dev, lex, lp, table, 0.0, arm)) == ref, arm


def test_line_words_refuses_what_it_cannot_hold(dev):
    from dpmn_amd import _abi, ops
    lex = ops.Lexicon(["at"])
    with pytest.raises(_abi.DpmnError, match="at most 64 classes and 3201 frames per line"):
        ops.line_words(torch.zeros(3202, C, device=dev), [[0, 3202]], lex)
    with pytest.raises(_abi.DpmnError, match="at most 64 classes and 3201 frames per line"):
        ops.line_words(torch.zeros(4, 65, device=dev), [[0, 4]], lex)
    with pytest.raises(_abi.DpmnError, match="the lexicon holds class"):
        ops.line_words(torch.zeros(4, 8, device=dev), [[0, 4]], lex)
    with pytest.raises(_abi.DpmnError, match="penalty must be finite"):
        ops.line_words(torch.zeros(4, C, device=dev), [[0, 4]], lex, float("nan"))
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.line_words(torch.zeros(4, C), [[0, 4]], lex)


# ------------------------------------------------------------------------------------------------ NativeCRNN
def test_crnn_read_lines_with_a_lexicon(dev):
    from dpmn_amd import ops
    from test_gpu_crnn import _images, _pair
    _, nat = _pair(dev)
    imgs = _images(3, 16, 64, 72).to(dev)
    rows, B, T = nat.window_rows(imgs)
    lex = ops.Lexicon(["at", "tea", "7", "x1", "q", "zz9"])
    plan = [(0, 0), (0, 48), (0, 96)]
    plain = nat.read_lines(rows, plan, gap=1)
    copies = []
    to_host = torch.Tensor.cpu
    try:
        torch.Tensor.cpu = lambda t, *a, **k: (copies.append(tuple(t.shape)), to_host(t, *a, **k))[1]
        got = nat.read_lines(rows, plan, gap=1, lexicon=lex, penalty=-0.5)
    finally:
        torch.Tensor.cpu = to_host
    line_lp, lines = ops.line_stitch(rows, T, nat.nclass, plan, 64)
    L = lines.frames
    assert copies == [(3 * L + 2 + 3 * L + 4,)]                                      # ONE device-to-host copy
    assert len(plain) == 4 and len(got) == 7 and got[:4] == plain
    ref = lw.line_words_np(line_lp.cpu().numpy().astype(np.float64), lex.packed, -0.5)
    assert got[4] == [" ".join(lex.words[w] for w in ref[0])] and got[6] == [ref[1]]
    assert np.float64(got[5][0]).view(np.int64) == np.float64(ref[2]).view(np.int64) and isinstance(got[5][0], float)
    print("crnn read_lines with a lexicon: %r, score %.6g, spans %s" % (got[4][0], got[5][0], got[6][0]))


# ------------------------------------------------------------------------------------------------ main.py
def _csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_main_reads_tiled_lines_under_a_lexicon(dev, tmp_path, monkeypatch):
    """test_gpu_line_read's fixture (synthetic weights; 16 x 64: one window, 16 x 200: four) with and without --rec_lexicon."""
    import main as cli
    from dpmn_amd import ops, workload
    from test_gpu_crnn_eval import _checkpoints, _crnn_sd
    sr, models, psn = workload.build("cfg0", batch=2)[:3]
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    torch.save(_crnn_sd(), os.path.join(d, "crnn.pth"))
    src = os.path.join(d, "in")
    os.makedirs(src)
    rng = np.random.RandomState(6)
    for name, w in (("a.png", 64), ("b.png", 200)):
        Image.fromarray(rng.randint(0, 256, (16, w, 3)).astype(np.uint8)).save(os.path.join(src, name))
    words = ["at", "tea", "7", "x1", "q", "zz9", "i", "l"]
    with open(os.path.join(d, "words.txt"), "w", encoding="utf-8") as fh:
        fh.write("\n".join(words) + "\n")
    seen = []
    records = ops.line_words_records

    def spy(line_lp, lines, lex, penalty=0.0, **kw):
        seen.append((line_lp.cpu().numpy().astype(np.float64), [tuple(x) for x in lines], lex, penalty))
        return records(line_lp, lines, lex, penalty, **kw)
    monkeypatch.setattr(ops, "line_words_records", spy)

    def run(tag, **kw):
        args = workload.make_args("tsrn", 1, 1, 2)
        args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, False, None, 0, "crnn"
        args.vis_dir, args.demo_dir, args.demo_tile, args.demo_out = os.path.join(d, "vis_" + tag), src, True, os.path.join(d, tag)
        args.demo_line_read = True
        for k, v in kw.items():
            setattr(args, k, v)
        config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "ckpt_" + tag),
                                             VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
        cli.main(config, args)
        return args.demo_out
    plain = run("plain")
    assert not seen
    lexed = run("lexed", rec_lexicon=os.path.join(d, "words.txt"), rec_lexicon_penalty=-0.25)
    old, new = _csv(os.path.join(plain, "demo_result.csv")), _csv(os.path.join(lexed, "demo_result.csv"))
    assert old[0] == ["file", "lr_string", "sr_string"] and new[0] == old[0] + ["sr_lexicon", "sr_lexicon_score"]
    assert [r[:3] for r in new] == old and len(new) == 3
    assert sorted(os.listdir(lexed)) == sorted(os.listdir(plain)) == ["a_sr.png", "b_sr.png", "demo_result.csv"]
    for f in ("a_sr.png", "b_sr.png"):
        with open(os.path.join(lexed, f), "rb") as g, open(os.path.join(plain, f), "rb") as p:
            assert g.read() == p.read(), f
    # the two columns are the restatement's on the posteriors the run stitched (both images are one batch: one call, the SR side's)
    assert len(seen) == 1 and seen[0][3] == -0.25 and seen[0][2].words == words
    lp, table, lex, pen = seen[0]
    for row, (f0, L) in zip(new[1:], table):
        ref = lw.line_words_np(lp[f0:f0 + L], lex.packed, pen)
        assert row[3] == " ".join(words[w] for w in ref[0]) and row[4] == "%.6g" % ref[2], row
    print("main.py --rec_lexicon with --demo_tile --demo_line_read: %s" % new[1:])
