"""One read per tiled line on the GPU (csrc/line_read.hip): dpmn_line_stitch_f32, dpmn_line_greedy_i32 and dpmn_line_ctc_f32 against the
NumPy restatement (utils/line_read.py) and torch, NativeCRNN.window_rows / read_lines, then TextSR.demo and main.py with
--demo_line_read."""
import csv
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import confidence as cf
from dpmn_amd.utils import line_read as lr
from dpmn_amd.utils import tile
from helpers import record

pytestmark = pytest.mark.gpu

T, C, LD, P = 26, 37, 40, 64
BATCHES = {"one": [64], "two": [65], "three": [160], "four": [161], "ragged": [64, 65, 200, 1000]}      # the lines' widths
KINDS = ["random", "scaled80", "padding"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _plan(widths):
    return [(b, x0) for b, w in enumerate(widths) for x0 in tile.window_plan(w)]


@functools.lru_cache(maxsize=None)
def window_logits(batch, kind):
    """(windows, T, LD) float32 logits of a batch's plan; the padding columns hold noise, in the kind "padding" 1e4."""
    n = len(_plan(BATCHES[batch]))
    rng = np.random.RandomState(100 * list(BATCHES).index(batch) + KINDS.index(kind))
    x = rng.uniform(-80.0, 80.0, (n, T, LD)) if kind == "scaled80" else rng.randn(n, T, LD) * 2.0
    if kind == "padding":
        x[:, :, C:] = 1e4
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def stitched_reference(batch, kind):
    return lr.stitch_lp_np(window_logits(batch, kind)[:, :, :C], _plan(BATCHES[batch]), P)


def _stitch(dev, batch, kind):
    from dpmn_amd import ops
    x = window_logits(batch, kind)
    return ops.line_stitch(torch.from_numpy(x).to(dev).view(-1, LD), T, C, _plan(BATCHES[batch]), P)


def test_the_plans_of_the_cases():
    assert [len(_plan(w)) for w in BATCHES.values()] == [1, 2, 3, 4, 1 + 2 + 4 + 21]
    assert _plan([65]) == [(0, 0), (0, 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_line_stitch_equals_the_restatement(dev, batch, kind):
    """One fp32 rounding of an fp64 result, plus one ulp for libm differences: |got - ref| <= 2^-23 max(1, |ref|) per element."""
    line_lp, lines = _stitch(dev, batch, kind)
    ref = stitched_reference(batch, kind)
    assert [L for _, L in lines] == [len(r) for r in ref] == [lr.line_frames(w, T, P) for w in BATCHES[batch]]
    assert [f for f, _ in lines] == np.concatenate(([0], np.cumsum([len(r) for r in ref])[:-1])).tolist()
    got = line_lp.cpu().numpy()
    assert got.shape == (lines.frames, C) and got.dtype == np.float32
    ref = np.concatenate(ref)
    excess = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    print("line_stitch %s %s: %d frames, max |got - ref| / max(1, |ref|) %.3e, bound %.3e, min log-posterior %.4g"
          % (batch, kind, len(ref), excess.max(), 2.0 ** -23, ref.min()))
    record("line_stitch", "%s %s max |lp - float64| / max(1, |lp|)" % (batch, kind), excess.max(), 2.0 ** -23)
    assert np.all(np.isfinite(got)) and excess.max() <= 2.0 ** -23
    again, _ = _stitch(dev, batch, kind)
    assert torch.equal(again, line_lp)                                                # the same call twice: equal bits


# ------------------------------------------------------------------------------------------------ crafted lines
def _crafted(best, seed):
    """a line's float32 log-posteriors whose arg-max classes are `best`, with a margin of 6"""
    x = np.random.RandomState(seed).randn(len(best), C) * 0.1
    x[np.arange(len(best)), best] += 6.0
    return cf._log_softmax(x).astype(np.float32)


def _symbols(n, L):
    """n symbols in L frames: neighbouring classes differ, so n = L fits"""
    return [1 + j % 36 for j in range(n)] + [0] * (L - n)


CRAFTED = {
    # 1201 states: two per thread of the recursion's block
    "words": [[0] * 30, [C - 1] * 30, [1, 0, 1]] + [_symbols(n, 600) for n in (0, 31, 32, 63, 64)],
    # n = L = 1100: 2201 states, several per thread, every state live
    "full": [[1 + j % 2 for j in range(1100)], [0] * 30],
    # 4201 states: the widest block, seven states per thread
    "long": [_symbols(100, 2100)],
}


@functools.lru_cache(maxsize=None)
def crafted_lines(name):
    rows = [_crafted(best, 10 * list(CRAFTED).index(name) + i) for i, best in enumerate(CRAFTED[name])]
    L = [len(r) for r in rows]
    return np.concatenate(rows), np.stack([np.concatenate(([0], np.cumsum(L[:-1]))), L], 1).astype(np.int64)


def _decode(dev, line_lp, lines):
    """ops.line_greedy + ops.line_ctc_confidence -> (host buffer, per line (classes, spans), scores)"""
    from dpmn_amd import ops
    buf, cls, start, end, length = ops.line_greedy(line_lp, lines, extra=len(lines))
    view = ops.line_ctc_confidence(line_lp, lines, buf)
    h = buf.cpu().numpy()
    N, B = line_lp.shape[0], len(lines)
    assert h.shape == (3 * N + 2 * B,)
    for v, lo in ((cls, 0), (start, N), (end, 2 * N), (length, 3 * N)):
        assert np.array_equal(v.cpu().numpy(), h[lo:lo + len(v)])
    assert np.array_equal(view.cpu().numpy().view(np.int32), h[3 * N + B:])
    reads = []
    for (f0, L), n in zip(lines, h[3 * N:3 * N + B].tolist()):
        reads.append((h[f0:f0 + n].tolist(), list(zip(h[N + f0:N + f0 + n].tolist(), h[2 * N + f0:2 * N + f0 + n].tolist()))))
        for lo in (0, N, 2 * N):
            assert not h[lo + f0 + n:lo + f0 + L].any()                              # zero behind the length
    return h, reads, h[3 * N + B:].view(np.float32).astype(np.float64)


def _torch_ctc32(lp, classes):
    """torch's fp32 CPU formulation on the same rows and string: -ctc_loss(log_softmax(rows))"""
    x = torch.log_softmax(torch.from_numpy(np.ascontiguousarray(lp, np.float32)), -1)[:, None]
    nll = torch.nn.functional.ctc_loss(x, torch.tensor([classes], dtype=torch.long).view(1, -1), torch.tensor([len(lp)]),
                                       torch.tensor([len(classes)]), blank=0, reduction="none")
    return -float(nll[0])


def _check_reads(what, lp, table, reads, scores):
    """greedy: exactly greedy_np.  score: err <= 4 max(e_ref, L 2^-24 max|score|), e_ref torch's fp32 CPU error, over the batch."""
    ref, t32 = [], []
    for (f0, L), (classes, spans) in zip(table, reads):
        rows = lp[f0:f0 + L].astype(np.float64)
        assert (classes, spans) == lr.greedy_np(lp[f0:f0 + L]), what
        ref.append(lr.line_score_np(rows, classes)[0])
        t32.append(_torch_ctc32(lp[f0:f0 + L], classes))
    ref = np.array(ref)
    e_ref = float(np.abs(np.array(t32) - ref).max())
    bound = 4.0 * max(e_ref, max(L for _, L in table) * 2.0 ** -24 * float(np.abs(ref).max()))
    err = float(np.abs(scores - ref).max())
    print("line_ctc %s: score error %.3e, bound %.3e (e_ref %.3e), max |score| %.4g, lengths %s"
          % (what, err, bound, e_ref, np.abs(ref).max(), [len(c) for c, _ in reads]))
    record("line_ctc", "%s max |score - float64|" % what, err, bound)
    assert np.all(np.isfinite(scores)) and err <= bound, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_line_greedy_and_score_on_the_stitched_lines(dev, batch, kind):
    line_lp, lines = _stitch(dev, batch, kind)
    h, reads, scores = _decode(dev, line_lp, lines)
    _check_reads("%s %s" % (batch, kind), line_lp.cpu().numpy(), list(lines), reads, scores)
    assert np.array_equal(_decode(dev, line_lp, lines)[0], h)                        # the same calls again: equal bits


@pytest.mark.parametrize("name", list(CRAFTED))
def test_line_greedy_and_score_on_crafted_lines(dev, name):
    from dpmn_amd import ops
    lp, table = crafted_lines(name)
    lines = ops.LineTable(table)
    h, reads, scores = _decode(dev, torch.from_numpy(lp).to(dev), lines)
    for best, (classes, spans) in zip(CRAFTED[name], reads):
        assert classes == [c for c, p in zip(best, [-1] + best) if c != 0 and c != p]
        assert all(best[a] == best[b] == c and a <= b for c, (a, b) in zip(classes, spans))
    if name == "words":
        assert [len(c) for c, _ in reads] == [0, 1, 2, 0, 31, 32, 63, 64] and reads[1][1] == [(0, 29)] and reads[2][1] == [(0, 0), (2, 2)]
    if name == "full":
        assert len(reads[0][0]) == 1100 and reads[0][1][-1] == (1099, 1099)
    _check_reads(name, lp, table.tolist(), reads, scores)
    assert np.array_equal(_decode(dev, torch.from_numpy(lp).to(dev), table)[0], h)   # a host table instead of a LineTable


def test_line_read_refuses_what_it_cannot_hold(dev):
    from dpmn_amd import _abi, ops
    text = "at most 64 .*3201 frames per line"
    # T = 65, n_class = 65, and a line of 3329 frames (T = 27: a frame every 64 / 26 columns of an 8192-column line)
    wide = [(0, x0) for x0 in tile.window_plan(8192)]
    for Tw, n_class, plan in ((65, 37, [(0, 0)]), (26, 65, [(0, 0)]), (27, 37, wide)):
        rows = torch.zeros(len(plan) * Tw, n_class + 3, device=dev)
        with pytest.raises(_abi.DpmnError, match=text):
            ops.line_stitch(rows, Tw, n_class, plan, P)
    assert lr.line_frames(8192, 26, P) == 3201 == lr.MAX_L and lr.line_frames(8192, 27, P) == 3329
    table = [[0, 3202]]
    for n_class, tab in ((37, table), (65, [[0, 8]])):
        lp = torch.zeros(tab[0][1], n_class, device=dev)
        with pytest.raises(_abi.DpmnError, match=text):
            ops.line_greedy(lp, tab)
        buf = torch.full((3 * tab[0][1] + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        with pytest.raises(_abi.DpmnError, match=text):
            ops.line_ctc_confidence(lp, tab, buf)
        torch.cuda.synchronize()
        assert bool((buf == 0x5A5A5A5A).all())                                        # nothing was launched
    lp = torch.zeros(8, 37, device=dev)
    with pytest.raises(_abi.DpmnError, match="extra >= B"):
        ops.line_ctc_confidence(lp, [[0, 8]], ops.line_greedy(lp, [[0, 8]])[0])
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.line_stitch(torch.zeros(26, 40), 26, 37, [(0, 0)], P)
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.line_greedy(torch.zeros(8, 37), [[0, 8]])
    with pytest.raises(_abi.DpmnError, match="back to back"):
        ops.line_greedy(lp, [[1, 7]])
    with pytest.raises(_abi.DpmnError, match="does not continue the plan"):
        ops.line_stitch(torch.zeros(2 * 26, 40, device=dev), 26, 37, [(0, 0), (1, 5)], P)
    with pytest.raises(_abi.DpmnError, match="leave columns of the line uncovered"):
        ops.line_stitch(torch.zeros(2 * 26, 40, device=dev), 26, 37, [(0, 0), (0, 70)], P)


# ------------------------------------------------------------------------------------------------ NativeCRNN
def test_crnn_read_lines(dev):
    from test_gpu_crnn import _images, _pair
    _, nat = _pair(dev)
    imgs = _images(3, 16, 64, 72).to(dev)
    rows, B, Tw = nat.window_rows(imgs)
    assert (B, Tw) == (3, T) and tuple(rows.shape) == (3 * T, nat.N_PAD) and rows.is_cuda
    assert torch.equal(rows, nat.logits_rows(nat.prep(imgs))[0])
    # single-window images: read's strings and read_conf's scores
    strings, scores, terms, spans = nat.read_lines(rows, [(b, 0) for b in range(3)])
    words, w_scores, w_terms = nat.read_conf(imgs)
    assert strings == words == nat.read(imgs) and any(strings) and terms == w_terms
    assert [len(s) for s in spans] == [len(s) for s in strings]
    x = rows.view(3, T, -1)[..., :nat.nclass].cpu().numpy()
    cls, length = cf.ctc_greedy(x)
    ref, _ = cf.ctc_score(x.astype(np.float64), cls, length)
    e_ref = float(np.abs(np.array([_torch_ctc32(x[b], cls[b, :length[b]].tolist()) for b in range(3)]) - ref).max())
    bound = 4.0 * max(e_ref, T * 2.0 ** -24 * float(np.abs(ref).max()))
    err = max(float(np.abs(np.asarray(scores) - ref).max()), float(np.abs(np.asarray(w_scores) - ref).max()))
    print("crnn read_lines, single windows: %s, score error %.3e, bound %.3e (e_ref %.3e)" % (strings, err, bound, e_ref))
    record("crnn_read_lines", "single windows max |score - float64|", err, bound)
    assert err <= bound
    # the three windows as ONE line of 160 columns: one string, one host copy
    plan = [(0, 0), (0, 48), (0, 96)]
    copies = []
    to_host = torch.Tensor.cpu
    try:
        torch.Tensor.cpu = lambda t, *a, **k: (copies.append(tuple(t.shape)), to_host(t, *a, **k))[1]
        (line,), (score,), (n,), (span,) = nat.read_lines(rows, plan)
        spaced = nat.read_lines(rows, plan, gap=1)[0][0]
    finally:
        torch.Tensor.cpu = to_host
    L = lr.line_frames(160, T, P)
    assert copies == [(3 * L + 2,)] * 2
    (ref_lp,) = lr.stitch_lp_np(x, plan, P)
    classes, ref_spans = lr.greedy_np(ref_lp)
    from dpmn_amd.model.crnn import ALPHABET
    assert line == "".join(ALPHABET[c - 1] for c in classes) and span == ref_spans and n == max(len(classes), 1)
    assert "|" not in line and spaced.replace(" ", "") == line
    assert abs(score - lr.line_score_np(ref_lp, classes)[0]) <= 4.0 * max(e_ref, L * 2.0 ** -24 * abs(score))
    with pytest.raises(ValueError, match="do not divide"):
        nat.read_lines(rows, [(0, 0), (0, 40), (0, 80), (0, 120)])


# ------------------------------------------------------------------------------------------------ TextSR.demo and main.py
def _csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_demo_and_main_read_every_line_once(dev, tmp_path):
    """Two images, 16 x 64 (one window) and 16 x 200 (four windows): with the stack's batch size 2 the five windows go through the
    model in chunks of 2, 2 and 1."""
    import main as cli
    from dpmn_amd import workload
    from dpmn_amd.dataset.folder import folder_window_batches
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

    def run(tag, **kw):
        args = workload.make_args("tsrn", 1, 1, 2)
        args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, False, None, 0, "crnn"
        args.vis_dir, args.demo_dir, args.demo_tile, args.demo_out = os.path.join(d, "vis_" + tag), src, True, os.path.join(d, tag)
        for k, v in kw.items():
            setattr(args, k, v)
        config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "ckpt_" + tag),
                                             VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
        cli.main(config, args)
        return args.demo_out

    plain = run("plain")
    lines = run("lines", demo_line_read=True, demo_conf=True)
    head = ["file", "lr_string", "lr_conf", "sr_string", "sr_conf"]
    table = _csv(os.path.join(lines, "demo_result.csv"))
    assert table[0] == head and [r[0] for r in table[1:]] == ["a.png", "b.png"]
    old = _csv(os.path.join(plain, "demo_result.csv"))
    assert old[0] == ["file", "lr_string", "sr_string"] and old[2][1].count("|") == 3 and old[2][2].count("|") == 3
    for r in table[1:]:
        # (seeded random weights read with a geometric-mean probability that may print as 0.0000)
        assert "|" not in r[1] + r[3] and all(len(v) == 6 and 0.0 <= float(v) <= 1.0 for v in (r[2], r[4]))
    assert table[1][1] == old[1][1] and table[1][3] == old[1][2]                     # one window: read's string
    assert sorted(os.listdir(lines)) == sorted(os.listdir(plain)) == ["a_sr.png", "b_sr.png", "demo_result.csv"]
    for f in ("a_sr.png", "b_sr.png"):
        with open(os.path.join(lines, f), "rb") as g, open(os.path.join(plain, f), "rb") as p:
            assert g.read() == p.read(), f
    # TextSR.demo itself, on the models main.py loaded from these checkpoints: the same rows
    from dpmn_amd.interfaces.super_resolution import TextSR
    args = workload.make_args("tsrn", 1, 1, 2)
    args.resume, args.rec = d, "crnn"
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "ckpt_direct"),
                                         VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
    direct = TextSR(config, args)
    rec = direct.CRNN_init()
    m2, p2 = direct.build_models(testing=True)
    out = os.path.join(d, "direct")
    rows = direct.demo(m2, p2, folder_window_batches(src, 2, (16, 64), direct.mask, direct.device), out, rec=rec, tile=True, chunk=2,
                       line_read=True, confidence=True)
    assert [head] + rows == table and _csv(os.path.join(out, "demo_result.csv")) == table
    spaced = direct.demo(m2, p2, folder_window_batches(src, 2, (16, 64), direct.mask, direct.device), os.path.join(d, "spaced"), rec=rec,
                         tile=True, chunk=2, line_read=True, line_space=1)
    assert [[r[0], r[1].replace(" ", ""), r[2].replace(" ", "")] for r in spaced] == [[r[0], r[1], r[3]] for r in rows]
