"""HR text crops rendered on the GPU (csrc/render.hip through ops.render_words_u8) against the NumPy restatement utils.render.render_u8,
byte for byte; the packed layout; untouched bytes around the images; sr_batches over a WordsHR loader end to end against the NumPy
chain; TextSR.train from a word list (--train_words) stopped and continued from its state file."""
import os
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import render as rd
from dpmn_amd.utils.resize import pack_ragged, pil_resize_u8

pytestmark = pytest.mark.gpu

WORDS = ["hello", "World", "a", "x" * 25, "it's", "42nd"]
_REF = {}


def _row(font, case, gh, spacing, margins, shear, style, seed, fg=(200, 30, 90), bg=(10, 220, 130), bg2=(250, 120, 0)):
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.FONT], row[rd.CASE], row[rd.GH], row[rd.SPACING], row[rd.SHEAR], row[rd.STYLE], row[rd.SEED] = font, case, gh, spacing, shear, style, seed
    row[rd.M_LEFT:rd.M_BOTTOM + 1] = margins
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3], row[rd.BG2:rd.BG2 + 3] = fg, bg, bg2
    return row


def _batch():
    """Nine samples on every edge, their restatement images and pack_ragged pair: made once, never changed.  Two atlases: PIL's built-in
    font at the base heights 64 and 40."""
    if not _REF:
        at = rd.build_atlases(None, [64, 40])
        S = rd.SHEAR_MAX
        #        word                    font case gh spacing margins (l, r, t, b)  shear style seed
        rows = [("i",                    0, 0, 24, 0, (0, 0, 0, 0), 0, 0, 1),                     # one letter, smallest gh, no margin at all
                ("x" * 25,               0, 1, 64, 4, (16, 16, 16, 16), S, 1, 2 ** 63 - 1),       # 25 letters, largest gh, widest spacing, many tiles
                ("wm" * 12,              1, 2, 64, -1, (3, 0, 7, 1), -S, 2, 3),                   # negative spacing, shear the other way, enlarged atlas
                ("a1",                   1, 0, 24, -1, (0, 5, 0, 6), S, 2, 4),                    # shrunk atlas, two letters
                ("Word",                 0, 2, 40, 2, (1, 0, 0, 0), 0, 1, 5),
                ("it's",                 1, 1, 40, 0, (0, 0, 2, 2), 0, 0, 6),                     # atlas height = gh; a blank inside
                ("gpu",                  0, 0, 30, 1, (2, 1, 0, 3), -7000, 0, 7),
                ("0123456789",           1, 0, 26, 3, (6, 6, 6, 6), 12345, 1, 8),
                ("q",                    0, 1, 64, 4, (0, 1, 16, 0), -S, 2, 9)]
        words = [r[0] for r in rows]
        cls = np.zeros((len(rows), 25), np.int32)
        lens = np.zeros(len(rows), np.int32)
        for i, w in enumerate(words):
            c = rd.word_classes(w)
            cls[i, :len(c)], lens[i] = c, len(c)
        params = np.stack([_row(*r[1:]) for r in rows])
        images = [rd.render_u8(cls[i, :lens[i]], params[i], at) for i in range(len(rows))]
        packed, meta = pack_ragged(images, pin=False)
        _REF.update(at=at, cls=cls, lens=lens, params=params, images=images, packed=packed, meta=meta)
    return _REF


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def test_the_batch_sits_on_every_edge():
    r = _batch()
    p, ws = r["params"], [im.shape[1] for im in r["images"]]
    assert {1, 25} <= set(r["lens"].tolist()) and {24, 64} <= set(p[:, rd.GH]) and {-1, 4} <= set(p[:, rd.SPACING])
    assert {-rd.SHEAR_MAX, 0, rd.SHEAR_MAX} <= set(p[:, rd.SHEAR]) and set(p[:, rd.STYLE]) == {0, 1, 2} and set(p[:, rd.FONT]) == {0, 1}
    assert any(w % 4 for w in ws) and any(w % 4 == 0 for w in ws) and max(ws) > 3 * 128 and min(ws) < 128      # scalar tail; more than one tile
    assert max(im.shape[0] for im in r["images"]) > 8 * 8
    starts = {int((o + y * w * 3) % 4) for o, h, w in r["meta"].tolist() for y in range(h)}
    assert 0 in starts and len(starts) > 1      # rows that allow dword stores and rows that do not


def test_bytes_and_meta_equal_the_restatement(dev):
    from dpmn_amd import ops
    from helpers import record
    r = _batch()
    packed, meta = ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device=dev)
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1 and meta.dtype == torch.int64
    assert torch.equal(meta, r["meta"]) and packed.numel() == r["packed"].numel()
    got = packed.cpu().numpy()
    bad = [int((got[o:o + h * w * 3].reshape(h, w, 3) != im).sum()) for (o, h, w), im in zip(meta.tolist(), r["images"])]
    print("render parity: %d bytes, mismatching per image %s" % (got.size, bad))
    record("render_words", "bytes differing from the NumPy restatement (of %d)" % got.size, sum(bad), 0)
    assert sum(bad) == 0, bad
    # tensors as arguments; the same call twice gives the same bytes
    again = ops.render_words_u8(torch.from_numpy(r["cls"]), torch.from_numpy(r["lens"]), torch.from_numpy(r["params"]), r["at"], device=dev)[0]
    assert torch.equal(again, packed)


def test_bytes_outside_the_images_are_untouched(dev):
    from dpmn_amd import ops
    r = _batch()
    n = r["packed"].numel()
    out = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    got, meta = ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device=dev, out=out)
    assert got is out
    host = out.cpu()
    assert torch.equal(host[:n], r["packed"]) and bool((host[n:] == 0xA5).all())
    # one image alone at the front of a pre-filled buffer: what follows its extent stays, whatever the tile's overhang
    one = torch.full((r["images"][0].size + 512,), 0x5A, dtype=torch.uint8, device=dev)
    ops.render_words_u8(r["cls"][:1], r["lens"][:1], r["params"][:1], r["at"], device=dev, out=one)
    host = one.cpu().numpy()
    assert np.array_equal(host[:r["images"][0].size].reshape(r["images"][0].shape), r["images"][0]) and (host[r["images"][0].size:] == 0x5A).all()


def test_bad_arguments_are_rejected(dev):
    from dpmn_amd import _abi, ops
    r = _batch()
    for col, val in ((rd.FONT, 2), (rd.FONT, -1), (rd.STYLE, 3), (rd.GH, 0)):
        p = r["params"].copy()
        p[3, col] = val
        with pytest.raises(_abi.DpmnError):
            ops.render_words_u8(r["cls"], r["lens"], p, r["at"], device=dev)
    lens = r["lens"].copy()
    lens[0] = 26
    with pytest.raises(_abi.DpmnError, match="length"):
        ops.render_words_u8(r["cls"], lens, r["params"], r["at"], device=dev)
    cls = r["cls"].copy()
    cls[2, 1] = 37
    with pytest.raises(_abi.DpmnError, match="class"):
        ops.render_words_u8(cls, r["lens"], r["params"], r["at"], device=dev)
    with pytest.raises(_abi.DpmnError):
        ops.render_words_u8(r["cls"][:0], r["lens"][:0], r["params"][:0], r["at"], device=dev)
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device="cpu")
    with pytest.raises(_abi.DpmnError, match="out must be"):
        ops.render_words_u8(r["cls"], r["lens"], r["params"], r["at"], device=dev, out=torch.zeros(16, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------------------------- end to end
def _loader(at, jpeg=None):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.words import WordsHR
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=True, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True, jpeg=jpeg, render=(WORDS, at))
    return torch.utils.data.DataLoader(WordsHR(WORDS, 6), batch_size=4, shuffle=False, drop_last=True, collate_fn=col, num_workers=0)


def _u8(x):
    """the bytes before the / 255 of a collated batch (channels 0 .. 2) as (B, h, w, 3)"""
    return (x[:, :3] * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def test_sr_batches_over_words_equals_the_numpy_chain(dev):
    """B = 4 from a 6-word WordsHR loader: the model's shapes, the drawn words as labels, and both tensors equal to the restatement
    pushed through the NumPy degrade_u8 (float64, fed with the field the kernel generates from the batch's seed), pil_resize_u8 and the
    utils.jpeg round trip.  A second pass after random.setstate reproduces them; another pass key does not."""
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import degrade as dg
    from dpmn_amd.utils.jpeg import draw_jpeg, jpeg_roundtrip_u8
    from helpers import record
    at = _batch()["at"]
    jpeg = (30, 95, 0.5)
    loader = _loader(at, jpeg)
    random.seed(21)
    state = random.getstate()
    (hr, lr, lv, labels), = list(tz.sr_batches(loader, dev))
    assert hr.shape == (4, 4, 32, 128) and lr.shape == (4, 4, 16, 64) and lv is None and hr.is_cuda and hr.dtype == torch.float32
    random.setstate(state)
    rng = random.Random(random.getrandbits(63))
    want, cls, lens, params = rd.draw_render(WORDS, at.n_fonts, rng, n=4)
    assert labels == want
    images = [rd.render_u8(cls[i, :lens[i]], params[i], at) for i in range(4)]
    meta = pack_ragged(images, pin=False)[1]
    dparams = dg.draw_params(4, cutblur=True, hr_widths=[im.shape[1] for im in images], rng=rng)
    seed = rng.getrandbits(63)
    z = ops.degrade_noise(seed, meta).cpu().numpy()
    low = [dg.degrade_u8(im, p, z[o:o + im.size].reshape(im.shape)) for im, p, (o, _, _) in zip(images, dparams, meta.tolist())]
    low = np.stack([pil_resize_u8(im, 16, 64) for im in low])
    q = draw_jpeg(4, jpeg[0], jpeg[1], jpeg[2], rng=rng)
    low = np.stack([jpeg_roundtrip_u8(im, int(qi)) if qi > 0 else im for im, qi in zip(low, q)])
    high = np.stack([pil_resize_u8(im, 32, 128) for im in images])
    d_hr, d_lr = int((_u8(hr) != high).sum()), int((_u8(lr) != low).sum())
    worst = int(np.abs(_u8(lr).astype(int) - low.astype(int)).max())
    print("words end to end: HR bytes differing %d of %d, LR bytes differing %d of %d (max |diff| %d), jpeg qualities %s"
          % (d_hr, high.size, d_lr, low.size, worst, q.tolist()))
    record("render_words", "HR bytes of sr_batches differing from the NumPy chain (of %d)" % high.size, d_hr, 0)
    record("render_words", "LR bytes of sr_batches differing from the NumPy chain (of %d)" % low.size, d_lr, 0)
    assert d_hr == 0
    assert d_lr == 0
    random.setstate(state)
    (hr2, lr2, _, labels2), = list(tz.sr_batches(loader, dev))
    assert labels2 == labels and torch.equal(hr2, hr) and torch.equal(lr2, lr)
    random.seed(22)
    (hr3, lr3, _, _), = list(tz.sr_batches(loader, dev))
    assert not torch.equal(hr3, hr) and not torch.equal(lr3, lr)


# ------------------------------------------------------------------------------------------------------- training, stop and continue
B, B1, B2 = 4, 2, 2
_RUNS = {}
_LABEL_VECS = {}


def _mission(out_dir):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.utils import synth

    class Filled(TextSR):      # (as in tests/test_gpu_train_state.py: synthetic weights written through the trainer's arena)
        def build_training(self, world_size=1, group=None):
            out = super().build_training(world_size, group)
            models, psn, distill = out[0], out[1], out[2]
            for i, m in enumerate([psn] + models + distill):
                sd = m.state_dict()
                synth.synth_fill_(sd, 300 + i)
                with torch.no_grad():
                    for k, v in m.state_dict().items():
                        v.copy_(sd[k])
            psn.eval()
            return out

    cfg = workload.make_config(B)
    cfg.TRAIN.ckpt_dir = out_dir
    cfg.TRAIN.displayInterval = 1000
    args = workload.make_args("tatt", B1, B2, B)
    args.train_words, args.cutblur = "words.txt", True
    sr = Filled(cfg, args)
    sr.vis_dir = out_dir
    return sr


def _train(sr, steps, state_path=None, words=WORDS):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import synth
    at = _batch()["at"]
    dl = sr.get_train_data(train_words=(words, at, 6))[1]
    assert dl.collate_fn.render and dl.collate_fn.degrade and dl.collate_fn.cutblur and len(dl.dataset) == 6

    def batches(epoch):
        """TATT's label_vecs come with the batch, seeded per epoch and batch (tests/test_gpu_degrade.py says why)"""
        for j, (hr, lr, _, strs) in enumerate(tz.sr_batches(dl, sr.device, sr.mask)):
            assert len(strs) == B and set(strs) <= set(words)
            key = (epoch, j)
            if key not in _LABEL_VECS:
                _LABEL_VECS[key] = synth.synth_batch(B, seed=50 + 7 * epoch + j)["label_vecs"]
            yield hr, lr, _LABEL_VECS[key]

    models, distill = sr.train(batches, steps=steps, epochs=3, state_path=state_path, train_words=rd.words_setting(words, at, 6))
    torch.cuda.synchronize()
    return dict(sd=[{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in models + distill],
                loss=sr.last_loss.cpu().clone(), loop=sr.loop_state)


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def _runs(tmp_path_factory):
    """The uninterrupted run A (3 steps) and run B stopped after step 2, once per compute mode."""
    from dpmn_amd import _abi
    key = _abi.lib.dpmn_get_compute_dtype()
    if key not in _RUNS:
        d = tmp_path_factory.mktemp("words_train")
        _seed(1)
        a = _train(_mission(str(d / "a")), 3)
        _seed(1)
        state = str(d / "b" / "state.pt")
        b = _train(_mission(str(d / "b")), 2, state)
        assert b["loop"]["it"] == 2 and os.path.isfile(state)
        _RUNS[key] = dict(A=a, dir=d, state=state)
    return _RUNS[key]


def test_training_from_words_stops_and_continues_bitwise(tmp_path, tmp_path_factory):
    """six samples per epoch, B = 4 (one batch per epoch), three steps; stopped after step 2 and continued by a new object under other
    seeds: weights and loss equal the uninterrupted run's bit for bit -- the words, the render parameters and the LR images of step 3
    came from the captured streams.  A state of another word list is refused."""
    from dpmn_amd.interfaces import base
    ref = _runs(tmp_path_factory)
    assert base.read_train_state(ref["state"])["fingerprint"]["train_words"] == rd.words_setting(WORDS, _batch()["at"], 6)
    state = str(tmp_path / "state.pt")
    os.link(ref["state"], state)
    with pytest.raises(ValueError, match="train_words"):
        _train(_mission(str(tmp_path / "other")), 3, state, words=WORDS[:-1])
    _seed(99)
    got = _train(_mission(str(tmp_path)), 3, state)
    a = ref["A"]
    assert got["loop"]["it"] == a["loop"]["it"] == 3
    for i, (x, y) in enumerate(zip(a["sd"], got["sd"])):
        for k in x:
            assert torch.equal(x[k], y[k]), "model %d %s differs" % (i, k)
    assert torch.equal(a["loss"], got["loss"]), (float(a["loss"]), float(got["loss"]))
