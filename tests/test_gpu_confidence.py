"""Recogniser confidence on the GPU (csrc/confidence.hip): dpmn_ctc_conf_f32, dpmn_attn_conf_f32 and dpmn_turn180_f32 against the NumPy
restatement (utils/confidence.py) and torch, read_conf of the three native recognisers, then TextSR.demo with confidence / upright /
min_conf and a stub recogniser."""
import csv
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import confidence as cf
from helpers import record

pytestmark = pytest.mark.gpu

CTC_SHAPES = [(1, 1, 2, 2), (3, 2, 37, 40), (65, 26, 37, 40), (2, 64, 64, 64)]      # (B, T, n_class, ld)
CTC_KINDS = ["random", "crafted", "crafted2", "scaled80", "padding"]      # crafted2: the crafted images from the third on
ATTN_SHAPES = [(1, 1, 2), (3, 20, 37), (65, 20, 97)]                                # (B, steps, n_class)
SCORE_TOL_ASTER = 1e-3      # tests/test_gpu_aster.py MARGIN: what it grants the stored sequence scores


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _crafted_best(kind, T, C):
    """the arg-max class per frame of a crafted image: all blank, one repeated class, "aa" (a blank between), n = T"""
    if kind == 0:
        return [0] * T
    if kind == 1:
        return [C - 1] * T
    if kind == 2:
        return ([1, 0, 1] + [0] * T)[:T] if T >= 3 else [1] * T
    return [1 + t % (C - 1) for t in range(T)] if C > 2 else [(t + 1) % 2 for t in range(T)]


CRAFTED_FROM = {"crafted": 0, "crafted2": 2}      # image b is crafted image (b + this) % 4: a batch of two sees all four


@functools.lru_cache(maxsize=None)
def ctc_logits(shape, kind):
    """(B, T, ld) float32 logits; the padding columns hold noise, in the kind "padding" 1e4."""
    B, T, C, ld = shape
    rng = np.random.RandomState(100 * CTC_SHAPES.index(shape) + CTC_KINDS.index(kind))
    if kind == "scaled80":
        x = rng.uniform(-80.0, 80.0, (B, T, ld))
    elif kind in CRAFTED_FROM:
        x = rng.randn(B, T, ld) * 0.1
        for b in range(B):
            x[b, np.arange(T), _crafted_best((b + CRAFTED_FROM[kind]) % 4, T, C)] += 6.0
    else:
        x = rng.randn(B, T, ld) * 2.0
    if kind == "padding":
        x[:, :, C:] = 1e4
    return x.astype(np.float32)


def _torch_ctc32(logits, cls, length):
    """torch's fp32 CPU formulation: -ctc_loss(log_softmax) of every image's own string"""
    B, T, _ = logits.shape
    lp = torch.log_softmax(torch.from_numpy(logits), -1).permute(1, 0, 2)
    targets = torch.from_numpy(np.concatenate([cls[b, :length[b]] for b in range(B)]).astype(np.int64))
    nll = torch.nn.functional.ctc_loss(lp, targets, torch.full((B,), T, dtype=torch.long), torch.from_numpy(length.astype(np.int64)), blank=0,
                                       reduction="none")
    return -nll.double().numpy()


def _ctc_bound(logits, cls, length, ref):
    """4 max(e_ref, T 2^-24 max|score|), e_ref = the error of torch's fp32 CPU ctc_loss on the same inputs (tests/lexicon_cases.py)"""
    e_ref = float(np.abs(_torch_ctc32(logits, cls, length) - ref).max())
    return 4.0 * max(e_ref, logits.shape[1] * 2.0 ** -24 * float(np.abs(ref).max())), e_ref


@pytest.mark.parametrize("kind", CTC_KINDS)
@pytest.mark.parametrize("shape", CTC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ctc_confidence_equals_the_restatement(dev, shape, kind):
    from dpmn_amd import ops
    B, T, C, ld = shape
    x = ctc_logits(shape, kind)
    rows = torch.from_numpy(x).to(dev).view(B * T, ld)
    plain = ops.ctc_greedy(rows, B, T, C)[0].cpu().numpy()
    buf, _, _ = ops.ctc_greedy(rows, B, T, C, extra=B)
    view = ops.ctc_confidence(rows, B, T, C, buf)
    h = buf.cpu().numpy()
    n = B * T + B
    assert np.array_equal(h[:n], plain)                                              # cls / len: a plain ctc_greedy call, bit for bit
    assert np.array_equal(view.cpu().numpy().view(np.int32), h[n:])
    cls, length = h[:B * T].reshape(B, T).astype(np.int64), h[B * T:n].astype(np.int64)
    if kind in CRAFTED_FROM:
        for b in range(B):
            best = _crafted_best((b + CRAFTED_FROM[kind]) % 4, T, C)
            assert cls[b, :length[b]].tolist() == [c for c, p in zip(best, [-1] + best) if c != 0 and c != p]
        if B >= 2 and kind == "crafted2":
            assert length[1] == T                                                    # n = T: every one of the 2 T + 1 states is live
    got = h[n:].view(np.float32).astype(np.float64)
    ref, terms = cf.ctc_score(x[:, :, :C].astype(np.float64), cls, length)
    bound, e_ref = _ctc_bound(np.ascontiguousarray(x[:, :, :C]), cls, length, ref)
    err = float(np.abs(got - ref).max())
    print("ctc_conf %s %s: score error %.3e, bound %.3e (e_ref %.3e), max |score| %.4g, lengths %d .. %d"
          % (shape, kind, err, bound, e_ref, np.abs(ref).max(), length.min(), length.max()))
    record("ctc_conf", "%s %s max |score - float64|" % ("x".join(map(str, shape)), kind), err, bound)
    assert np.all(np.isfinite(got)) and err <= bound
    assert terms.tolist() == np.maximum(length, 1).tolist()
    # the same call again: equal bits
    buf2, _, _ = ops.ctc_greedy(rows, B, T, C, extra=B)
    ops.ctc_confidence(rows, B, T, C, buf2)
    assert np.array_equal(buf2.cpu().numpy(), h)


@pytest.mark.parametrize("T,C", [(65, 37), (26, 65)])
def test_ctc_confidence_refuses_what_it_cannot_hold(dev, T, C):
    from dpmn_amd import _abi, ops
    B = 2
    rows = torch.zeros(B * T, C + 3, device=dev)
    buf, _, _ = ops.ctc_greedy(rows, B, T, C, extra=B)
    buf[B * T + B:] = 0x5A5A5A5A
    with pytest.raises(_abi.DpmnError, match="at most 64 frames and 64 classes"):
        ops.ctc_confidence(rows, B, T, C, buf)
    torch.cuda.synchronize()
    assert buf[B * T + B:].cpu().tolist() == [0x5A5A5A5A] * B                       # nothing was launched
    with pytest.raises(_abi.DpmnError, match="extra >= B"):
        ops.ctc_confidence(rows, B, T, C, ops.ctc_greedy(rows, B, T, C)[0])


@pytest.mark.parametrize("where", ["first", "absent", "last"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn_confidence_equals_the_restatement(dev, shape, where):
    from dpmn_amd import ops
    B, steps, C = shape
    eos = C - 1
    rng = np.random.RandomState(10 * ATTN_SHAPES.index(shape) + ["first", "absent", "last"].index(where))
    x = (rng.randn(B, steps, C) * 2.0).astype(np.float32)
    x[..., eos] -= 30.0
    if where != "absent":
        x[:, 0 if where == "first" else steps - 1, eos] += 60.0
    ids = x.argmax(-1).astype(np.int32)
    n = 1 if where == "first" else steps
    assert (ids == eos).any() == (where != "absent")
    buf = ops.attn_confidence(torch.from_numpy(x).to(dev), torch.from_numpy(ids).to(dev), eos)
    h = buf.cpu().numpy()
    got, terms = h[:B].view(np.float32).astype(np.float64), h[B:]
    ref, ref_terms = cf.attn_score(x.astype(np.float64), ids, eos)
    assert terms.tolist() == ref_terms.tolist() == [n] * B                           # exact
    lp32 = torch.log_softmax(torch.from_numpy(x), -1).gather(2, torch.from_numpy(ids.astype(np.int64))[..., None])[..., 0]
    e_ref = float(np.abs(lp32[:, :n].sum(1).double().numpy() - ref).max())
    bound = 4.0 * max(e_ref, steps * 2.0 ** -24 * float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print("attn_conf %s %s: score error %.3e, bound %.3e (e_ref %.3e), max |score| %.4g" % (shape, where, err, bound, e_ref, np.abs(ref).max()))
    record("attn_conf", "%s eos %s max |score - float64|" % ("x".join(map(str, shape)), where), err, bound)
    assert err <= bound
    assert np.array_equal(ops.attn_confidence(torch.from_numpy(x).to(dev), torch.from_numpy(ids).to(dev), eos).cpu().numpy(), h)


def test_attn_confidence_refuses_what_it_cannot_hold(dev):
    from dpmn_amd import _abi, ops
    for steps, C in ((129, 37), (20, 129)):
        with pytest.raises(_abi.DpmnError, match="at most 128 steps and 128 classes"):
            ops.attn_confidence(torch.zeros(2, steps, C, device=dev), torch.zeros(2, steps, dtype=torch.int32, device=dev), 0)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 4, 16, 64), (3, 3, 5, 67)])
def test_turn180_equals_flip(dev, shape):
    from dpmn_amd import ops
    x = torch.from_numpy(np.random.RandomState(7).randn(*shape).astype(np.float32)).to(dev)
    y = ops.turn180(x)
    assert y.is_contiguous() and torch.equal(y, x.flip(2, 3))
    assert torch.equal(ops.turn180(x[:, :1]), x[:, :1].flip(2, 3))                   # a channel slice (not contiguous for C > 1)


# ------------------------------------------------------------------------------------------------ read_conf of the native recognisers
def test_crnn_read_conf(dev):
    from dpmn_amd import ops
    from test_gpu_crnn import _images, _pair
    _, nat = _pair(dev)
    imgs = _images(3, 16, 64, 72).to(dev)
    strings, scores, terms = nat.read_conf(imgs)
    assert strings == nat.read(imgs) and any(strings)
    rows, B, T = nat.logits_rows(nat.prep(imgs))
    h = ops.ctc_greedy(rows, B, T, nat.nclass)[0].cpu().numpy()
    cls, length = h[:B * T].reshape(B, T).astype(np.int64), h[B * T:].astype(np.int64)
    x = np.ascontiguousarray(rows.view(B, T, -1)[..., :nat.nclass].cpu().numpy())
    ref, ref_terms = cf.ctc_score(x.astype(np.float64), cls, length)
    bound, e_ref = _ctc_bound(x, cls, length, ref)
    err = float(np.abs(np.asarray(scores) - ref).max())
    print("crnn read_conf: %s, score error %.3e, bound %.3e (e_ref %.3e), conf %s" % (strings, err, bound, e_ref, cf.confidence(scores, terms)))
    record("crnn_read_conf", "max |score - float64|", err, bound)
    assert terms == ref_terms.tolist() and all(isinstance(t, int) for t in terms) and all(isinstance(s, float) for s in scores)
    assert err <= bound
    assert all(0.0 < c <= 1.0 for c in cf.confidence(scores, terms))


def test_moran_read_conf(dev):
    from dpmn_amd.model.moran import MAX_ITER, MORAN, NativeMORAN
    from dpmn_amd.utils import moran_synth
    sd = MORAN().state_dict()
    moran_synth.moran_fill_(sd, 91)
    nat = NativeMORAN().to(dev).eval()
    nat.load_state_dict(sd)
    imgs = moran_synth.moran_images(3, seed=93, pool=48).to(dev)
    strings, scores, terms = nat.read_conf(imgs)
    assert strings == nat.read(imgs)
    logits, ids = nat._run(*nat.prep(imgs), MAX_ITER)
    x, ids = logits.cpu().numpy(), ids.cpu().numpy()
    ref, ref_terms = cf.attn_score(x.astype(np.float64), ids, 36)
    n = ref_terms.tolist()
    lp32 = torch.log_softmax(torch.from_numpy(x), -1).gather(2, torch.from_numpy(ids.astype(np.int64))[..., None])[..., 0]
    e_ref = float(np.abs(np.array([float(lp32[b, :n[b]].sum()) for b in range(3)]) - ref).max())
    bound = 4.0 * max(e_ref, MAX_ITER * 2.0 ** -24 * float(np.abs(ref).max()))
    err = float(np.abs(np.asarray(scores) - ref).max())
    print("moran read_conf: %s, terms %s, score error %.3e, bound %.3e (e_ref %.3e)" % (strings, terms, err, bound, e_ref))
    record("moran_read_conf", "max |score - float64|", err, bound)
    assert terms == n and err <= bound
    assert [len(s) for s in strings] == [t - 1 if (ids[b] == 36).any() else t for b, t in enumerate(terms)]


def test_aster_read_conf(dev):
    """Against the stock-op mirror's beam search on the GPU, its stored tables through the same extraction; images whose candidate
    margin is below the one tests/test_gpu_aster.py decides ids at are compared for their strings with `read` only."""
    from dpmn_amd.model.aster import ASTER, NativeASTER
    from dpmn_amd.utils import aster_synth
    from helpers import load_golden
    z = load_golden("aster")
    sd = ASTER().state_dict()
    aster_synth.aster_fill_(sd, 81)
    nat, mir = NativeASTER().to(dev).eval(), ASTER().to(dev).eval()
    nat.load_state_dict(sd)
    mir.load_state_dict(sd)
    imgs = aster_synth.aster_images(z["ids"].tolist()[:3]).to(dev)
    strings, scores, terms = nat.read_conf(imgs)
    assert strings == nat.read(imgs)
    m_rec, m_st = mir.decoder.beam_search(mir.stages(imgs)["encoder"], 5, 94, return_stored=True)
    _, ref, ref_terms = cf.beam_score(np.asarray(m_st["symbols"]), np.asarray(m_st["predecessors"]), np.asarray(m_st["scores"]), 3, 5, 94)
    decided = [b for b in range(3) if z["margin"][b] >= SCORE_TOL_ASTER]
    assert decided
    err = max(abs(scores[b] - float(ref[b])) for b in decided)
    print("aster read_conf: %s, terms %s, score error %.3e over images %s" % (strings, terms, err, decided))
    record("aster_read_conf", "max |score - mirror|", err, SCORE_TOL_ASTER)
    assert [terms[b] for b in decided] == [int(ref_terms[b]) for b in decided] and err <= SCORE_TOL_ASTER
    assert all(1 <= t <= 100 for t in terms) and all(0.0 < c <= 1.0 for c in cf.confidence(scores, terms))


# ------------------------------------------------------------------------------------------------ TextSR.demo with a stub recogniser
class BrightTop:
    """read_conf: a fixed string, confident (0.9) when the top half of the image is brighter than the bottom half, else 0.3."""

    def read_conf(self, images):
        x = images.float()
        h = x.shape[2] // 2
        top = (x[:, :, :h].mean((1, 2, 3)) > x[:, :, h:].mean((1, 2, 3))).cpu().tolist()
        return ["word"] * len(top), [4 * float(np.log(0.9 if t else 0.3)) for t in top], [4] * len(top)

    def __call__(self, images):
        return self.read_conf(images)[0]


class ByPosition(BrightTop):
    """read_conf: the confidence of image i of every call is conf[i]"""

    def __init__(self, conf):
        self.conf = conf

    def read_conf(self, images):
        n = images.shape[0]
        return ["word"] * n, [4 * float(np.log(c)) for c in self.conf[:n]], [4] * n


@pytest.fixture(scope="module")
def stack(dev):
    from dpmn_amd import workload
    return workload.build("cfg0", batch=2)[:3]


def _csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_demo_upright_turns_the_image_that_reads_better_turned(dev, stack, tmp_path):
    """A (bright on top) and its exact 180 degree turn A' in one batch: A' is turned back on the device, so the model sees [A, A].
    The two rows of one batch are not bitwise alike in `refine` (measured: the two files of [A, A] differ, the synthetic text prior
    is drawn per row), so A''s file is compared with that of a run without the flags over a folder that holds A twice."""
    from dpmn_amd.dataset.folder import folder_batches
    sr, models, psn = stack
    rng = np.random.RandomState(4)
    a = rng.randint(0, 90, (16, 64, 3)).astype(np.uint8)
    a[:8] += 150
    src = tmp_path / "src"
    src.mkdir()
    Image.fromarray(a).save(str(src / "a.png"))
    Image.fromarray(np.ascontiguousarray(a[::-1, ::-1])).save(str(src / "b.png"))
    fn = sr.synthetic_text_prior()
    out = str(tmp_path / "out")
    rows = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), out, rec=BrightTop(), text_prior_fn=fn, upright=True)
    table = _csv(os.path.join(out, "demo_result.csv"))
    assert table[0] == ["file", "lr_string", "lr_conf", "sr_string", "sr_conf", "turned"] and table[1:] == rows
    assert [r[5] for r in rows] == ["0", "1"]
    assert [r[1] for r in rows] == ["word", "word"] and [r[2] for r in rows] == ["0.9000", "0.9000"]
    assert all(r[4] in ("0.9000", "0.3000") for r in rows)
    same = tmp_path / "same"
    same.mkdir()
    for name in ("a.png", "b.png"):
        Image.fromarray(a).save(str(same / name))
    out_same = str(tmp_path / "out_same")
    sr.demo(models, psn, folder_batches(str(same), 2, (16, 64), True, dev), out_same, rec=BrightTop(), text_prior_fn=fn)
    for name in ("a_sr.png", "b_sr.png"):
        assert _bytes(os.path.join(out, name)) == _bytes(os.path.join(out_same, name)), name
    # confidence alone: the columns without `turned`, nothing turned, the first file as above
    out2 = str(tmp_path / "out2")
    rows2 = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), out2, rec=BrightTop(), text_prior_fn=fn, confidence=True)
    assert _csv(os.path.join(out2, "demo_result.csv"))[0] == ["file", "lr_string", "lr_conf", "sr_string", "sr_conf"]
    assert [r[2] for r in rows2] == ["0.9000", "0.3000"]
    assert _bytes(os.path.join(out2, "a_sr.png")) == _bytes(os.path.join(out, "a_sr.png"))
    assert _bytes(os.path.join(out2, "b_sr.png")) != _bytes(os.path.join(out, "b_sr.png"))
    # all three off: what a call without the keywords writes
    out3, out4 = str(tmp_path / "out3"), str(tmp_path / "out4")
    rows3 = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), out3, rec=BrightTop(), text_prior_fn=fn)
    rows4 = sr.demo(models, psn, folder_batches(str(src), 2, (16, 64), True, dev), out4, rec=BrightTop(), text_prior_fn=fn, confidence=False,
                    upright=False, min_conf=None)
    assert rows3 == rows4 == [["a.png", "word", "word"], ["b.png", "word", "word"]]
    assert sorted(os.listdir(out3)) == sorted(os.listdir(out4)) == ["a_sr.png", "b_sr.png", "demo_result.csv"]
    for f in os.listdir(out3):
        assert _bytes(os.path.join(out3, f)) == _bytes(os.path.join(out4, f))
    assert _bytes(os.path.join(out3, "b_sr.png")) == _bytes(os.path.join(out2, "b_sr.png"))
    with pytest.raises(ValueError, match="a plain callable returns no score"):
        sr.demo(models, psn, iter(()), str(tmp_path / "out5"), rec=lambda x: [""] * len(x), text_prior_fn=fn, confidence=True)


def test_demo_min_conf_drops_the_region_that_reads_badly(dev, stack, tmp_path):
    from dpmn_amd.dataset.folder import box_region_batches
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    src, box, box1 = tmp_path / "photos", tmp_path / "boxes", tmp_path / "boxes1"
    for d in (src, box, box1):
        d.mkdir()
    Image.fromarray(np.random.RandomState(21).randint(0, 256, (40, 100, 3)).astype(np.uint8)).save(str(src / "p0.png"))
    (box / "p0.txt").write_text("3,5,67,5,67,21,3,21,first\n20.5,12,90,6.25,93,30,22,37.5,second\n")
    (box1 / "p0.txt").write_text("3,5,67,5,67,21,3,21,first\n")
    out, ref = str(tmp_path / "out"), str(tmp_path / "ref")
    make = lambda b: box_region_batches(str(src), str(b), 2, (16, 64), True, dev, photos=True)
    kw = dict(text_prior_fn=fn, boxes=True, paste=True, feather=1.0)
    rows = sr.demo(models, psn, make(box), out, rec=ByPosition([0.9, 0.2]), min_conf=0.5, **kw)
    assert _csv(os.path.join(out, "demo_result.csv"))[0] == ["file", "box", "label", "lr_string", "lr_conf", "sr_string", "sr_conf", "kept"]
    assert rows == [["p0", "000", "first", "word", "0.9000", "word", "0.9000", "1"], ["p0", "001", "second", "word", "0.2000", "word", "0.2000", "0"]]
    assert sorted(os.listdir(out)) == ["boxes_read", "demo_result.csv", "p0_000_sr.png", "p0_photo_sr.png"]
    with open(os.path.join(out, "boxes_read", "p0.txt")) as fh:
        assert fh.read() == "3,5,67,5,67,21,3,21,word\n"
    # the flagless paste of a box file that holds only the kept region
    sr.demo(models, psn, make(box1), ref, rec=ByPosition([0.9, 0.2]), **kw)
    assert _bytes(os.path.join(out, "p0_000_sr.png")) == _bytes(os.path.join(ref, "p0_000_sr.png"))
    assert _bytes(os.path.join(out, "p0_photo_sr.png")) == _bytes(os.path.join(ref, "p0_photo_sr.png"))
    with pytest.raises(ValueError, match="photos=True"):
        sr.demo(models, psn, box_region_batches(str(src), str(box), 2, (16, 64), True, dev), str(tmp_path / "out2"), rec=ByPosition([0.9, 0.2]),
                text_prior_fn=fn, boxes=True, min_conf=0.5)


def test_demo_upright_pastes_a_turned_region_where_it_was_cut(dev, stack, tmp_path):
    """A box file whose only region starts at the wrong corner (br, bl, tl, tr): upright turns it back and boxes_read names the
    corners from the top-left again, as for the box file written the right way round.  (The two rectifications sample the photo
    through different coefficients, so the pixels of the two runs are not compared byte for byte.)"""
    from dpmn_amd.dataset.folder import box_region_batches
    sr, models, psn = stack
    fn = sr.synthetic_text_prior()
    src, wrong, right = tmp_path / "photos", tmp_path / "wrong", tmp_path / "right"
    for d in (src, wrong, right):
        d.mkdir()
    photo = np.random.RandomState(22).randint(0, 90, (40, 100, 3)).astype(np.uint8)
    photo[:13] += 150                                                                   # the region 3..67 x 5..21: bright on top
    Image.fromarray(photo).save(str(src / "p0.png"))
    (right / "p0.txt").write_text("3,5,67,5,67,21,3,21,first\n")
    (wrong / "p0.txt").write_text("67,21,3,21,3,5,67,5,first\n")
    make = lambda b: box_region_batches(str(src), str(b), 2, (16, 64), True, dev, photos=True)
    kw = dict(rec=BrightTop(), text_prior_fn=fn, boxes=True, paste=True, feather=1.0, upright=True)
    out_w, out_r = str(tmp_path / "out_w"), str(tmp_path / "out_r")
    rows_w = sr.demo(models, psn, make(wrong), out_w, **kw)
    rows_r = sr.demo(models, psn, make(right), out_r, **kw)
    assert [r[7] for r in rows_w] == ["1"] and [r[7] for r in rows_r] == ["0"]
    assert rows_w[0][:5] == rows_r[0][:5] == ["p0", "000", "first", "word", "0.9000"]
    for out in (out_w, out_r):
        assert sorted(os.listdir(out)) == ["boxes_read", "demo_result.csv", "p0_000_sr.png", "p0_photo_sr.png"]
    assert _bytes(os.path.join(out_w, "boxes_read", "p0.txt")) == _bytes(os.path.join(out_r, "boxes_read", "p0.txt"))
    turned = np.asarray(Image.open(os.path.join(out_w, "p0_photo_sr.png")), np.int64)
    plain = np.asarray(Image.open(os.path.join(out_r, "p0_photo_sr.png")), np.int64)
    print("photo pasted from the wrong-corner box vs the right one: mean |diff| %.3f" % np.abs(turned - plain).mean())
    assert np.abs(turned - plain).mean() < 2.0                                          # (pasted upside-down it is above 40)
    with open(os.path.join(out_w, "boxes_read", "p0.txt")) as fh:
        assert fh.read() == "3,5,67,5,67,21,3,21,word\n"
