"""Point-spread functions on the GPU (csrc/psf.hip through ops.psf_blur_ragged_u8 / ops.cutblur_ragged_u8) against the integer NumPy
restatements utils.psf.psf_blur_u8 / cutblur_u8, byte for byte; degrade_on_gpu with the stage against the ops composed by hand; and
TextSR.train from a folder with --psf_blur, --cutblur and --jpeg_degrade stopped and continued from its state file."""
import math
import os
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import degrade as dg
from dpmn_amd.utils import psf
from dpmn_amd.utils.jpeg import draw_jpeg
from dpmn_amd.utils.resize import pack_ragged

pytestmark = pytest.mark.gpu

# sides below the halo (the border is folded repeatedly), tile seams at 32, ragged last tiles
SIZES = [(1, 1), (1, 7), (2, 3), (5, 40), (16, 64), (33, 130), (47, 200), (8, 8)]
# each kind at R = 10 and at R = 1, a motion PSF along x and along y      kind, r, theta, ratio
PSFS = {"motion_R10": ("motion", 10.0, 0.6, 1.0), "motion_R1": ("motion", 1.0, 2.2, 1.0), "disk_R10": ("disk", 10.0, 0.0, 1.0),
        "disk_R1": ("disk", 1.0, 0.0, 1.0), "aniso_R10": ("aniso", 10.0, 1.9, 0.35), "aniso_R1": ("aniso", 1.0, 0.4, 0.8),
        "motion_x": ("motion", 9.3, 0.0, 1.0), "motion_y": ("motion", 9.3, math.pi / 2, 1.0)}
_REF = {}


def _inputs():
    """The batch (the eight sizes and a ninth image that keeps the identity), made once, never changed; the CPU results per PSF are
    added as they are first asked for."""
    if not _REF:
        rng = np.random.RandomState(12)
        images = []
        for h, w in SIZES + [(16, 64)]:
            a = rng.randint(0, 256, (h, w, 3)).astype(np.int32)
            a[:, w // 3:] = np.clip(a[:, w // 3:] // 4 + 150, 0, 255)          # step edges over the noise
            a[h // 2:, : w // 2] = a[h // 2:, : w // 2] // 3
            images.append(a.astype(np.uint8))
        packed, meta = pack_ragged(images, pin=False)
        _REF.update(images=images, packed=packed, meta=meta, want={})
    return _REF


def _want(name):
    r = _inputs()
    if name not in r["want"]:
        t = psf.psf_taps(*PSFS[name])
        r["want"][name] = (t, [psf.psf_blur_u8(im, t) for im in r["images"][:-1]] + [r["images"][-1]])
    return r["want"][name]


def _unpack(buf, meta):
    flat = buf.cpu().numpy()
    return [flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in np.asarray(meta).tolist()]


@pytest.fixture
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(PSFS))
def test_blur_equals_the_restatement_byte_for_byte(dev, name):
    """Tolerance zero, derived: both sides are integer arithmetic on the same tap table."""
    from dpmn_amd import ops
    r = _inputs()
    t, want = _want(name)
    R = math.ceil(PSFS[name][1])
    assert np.abs(t[:, :2]).max() <= R and (R == 1 or np.abs(t[:, :2]).max() >= 6)
    if name == "motion_x":
        assert (t[:, 0] == 0).all()
    if name == "motion_y":
        assert (t[:, 1] == 0).all()
    taps = [t] * len(SIZES) + [psf.IDENTITY]
    out = ops.psf_blur_ragged_u8(r["packed"].to(dev), r["meta"], taps)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == r["packed"].shape
    got = _unpack(out, r["meta"])
    for (h, w), g, wnt in zip(SIZES + [(16, 64)], got, want):
        bad = int((g != wnt).sum())
        assert bad == 0, "%s %d x %d: %d bytes differ, max |diff| %d" % (name, h, w, bad, int(np.abs(g.astype(int) - wnt.astype(int)).max()))
    assert np.array_equal(got[-1], r["images"][-1]), "the identity image is copied"
    assert not np.array_equal(got[6], r["images"][6])


def test_a_psf_per_image_twice_the_same_and_gaps_stay_zero(dev):
    """Image i of one call gets PSF i (a ragged tap list); the same call again gives the same bytes; in a packed buffer with bytes
    between and after the images, those bytes stay 0."""
    from dpmn_amd import ops
    r = _inputs()
    names = list(PSFS)
    taps = [_want(n)[0] for n in names] + [psf.IDENTITY]
    want = [_want(n)[1][i] for i, n in enumerate(names)] + [r["images"][-1]]
    packed = r["packed"].to(dev)
    a = ops.psf_blur_ragged_u8(packed, r["meta"], taps)
    b = ops.psf_blur_ragged_u8(packed, r["meta"].numpy(), [t.astype(np.int64) for t in taps])
    assert torch.equal(a, b)
    for g, wnt in zip(_unpack(a, r["meta"]), want):
        assert np.array_equal(g, wnt)
    # the same images 5 bytes apart, 11 bytes in front and 7 behind
    meta = r["meta"].numpy().copy()
    meta[:, 0] += 11 + 5 * np.arange(len(meta))
    total = int(meta[-1, 0] + meta[-1, 1] * meta[-1, 2] * 3) + 7
    loose = np.full(total, 255, np.uint8)
    own = np.zeros(total, bool)
    for (off, h, w), im in zip(meta.tolist(), r["images"]):
        loose[off:off + h * w * 3] = im.reshape(-1)
        own[off:off + h * w * 3] = True
    out = ops.psf_blur_ragged_u8(torch.from_numpy(loose).to(dev), meta, taps)
    for g, wnt in zip(_unpack(out, meta), want):
        assert np.array_equal(g, wnt)
    assert not out.cpu().numpy()[~own].any() and int((~own).sum()) == 11 + 5 * (len(meta) - 1) + 7


def test_cutblur_equals_the_restatement(dev):
    """sides 0, 1 and 2; cut_x of 0 and of w"""
    from dpmn_amd import ops
    r = _inputs()
    rng = np.random.RandomState(13)
    lows = [rng.randint(0, 256, im.shape).astype(np.uint8) for im in r["images"]]
    low_packed = pack_ragged(lows, pin=False)[0]
    #         (1,1)  (1,7)  (2,3)  (5,40)  (16,64)  (33,130)  (47,200)  (8,8)  (16,64)
    cuts = [(0, 1), (7, 1), (1, 2), (13, 0), (64, 2), (40, 1), (0, 2), (8, 1), (33, 2)]
    params = np.zeros((len(cuts), dg.N_PARAMS), np.float32)
    params[:, dg.PRE_K] = 3                              # (the other columns are not read)
    params[:, [dg.CUT_X, dg.CUT_SIDE]] = cuts
    assert {s for _, s in cuts} == {0, 1, 2} and cuts[0] == (0, 1) and cuts[6] == (0, 2), "cut_x = 0 on either side"
    assert cuts[1] == (SIZES[1][1], 1) and cuts[4] == (SIZES[4][1], 2), "cut_x = w on either side"
    packed = r["packed"].to(dev)
    low = low_packed.to(dev)
    out = ops.cutblur_ragged_u8(low, packed, r["meta"], params)
    assert out is low, "in place on the LR buffer"
    changed = 0
    for g, lo, hr, (cx, side) in zip(_unpack(out, r["meta"]), lows, r["images"], cuts):
        assert np.array_equal(g, psf.cutblur_u8(lo, hr, cx, side))
        changed += int(not np.array_equal(g, lo))
    assert changed >= 4
    assert torch.equal(packed.cpu(), r["packed"])
    # no image with a cut: nothing changes
    none = params.copy()
    none[:, dg.CUT_SIDE] = 0
    low = low_packed.to(dev)
    assert torch.equal(ops.cutblur_ragged_u8(low, packed, r["meta"], none).cpu(), low_packed)


def test_bad_arguments_raise_before_any_launch(dev, monkeypatch):
    from dpmn_amd import _abi, ops
    r = _inputs()
    launched = []
    monkeypatch.setattr(ops, "lib", type("NoLaunch", (), {"__getattr__": lambda self, n: lambda *a: launched.append(n) or 0})())
    packed, meta = r["packed"].to(dev), r["meta"]
    B = meta.shape[0]
    good = [psf.psf_taps("disk", 2.0)] * B
    E = _abi.DpmnError
    with pytest.raises(E, match="no CPU fallback"):
        ops.psf_blur_ragged_u8(r["packed"], meta, good)
    with pytest.raises(E):
        ops.psf_blur_ragged_u8(packed[:-1], meta, good)                         # the meta points past the buffer
    with pytest.raises(E, match="one per image"):
        ops.psf_blur_ragged_u8(packed, meta, good[:-1])

    def one(t):
        return good[:3] + [np.asarray(t)] + good[4:]

    far = psf.IDENTITY.copy()
    far[0, 1] = 11
    with pytest.raises(E, match="above 10"):
        ops.psf_blur_ragged_u8(packed, meta, one(far))
    with pytest.raises(E, match="q > 0"):
        ops.psf_blur_ragged_u8(packed, meta, one([[0, 0, 65537], [0, 1, -1]]))
    with pytest.raises(E, match="q > 0"):
        ops.psf_blur_ragged_u8(packed, meta, one([[0, 0, 65536], [0, 1, 0]]))
    with pytest.raises(E, match="65536 exactly"):
        ops.psf_blur_ragged_u8(packed, meta, one([[0, 0, 65535]]))
    many = np.array([[0, 0, 65536 - 441]] + [[dy, dx, 1] for dy in range(-10, 11) for dx in range(-10, 11)], np.int32)
    assert many.shape[0] == 442 and many[:, 2].sum() == 65536
    with pytest.raises(E, match="1 <= n <= 441"):
        ops.psf_blur_ragged_u8(packed, meta, one(many))
    with pytest.raises(E, match=r"\(n, 3\)"):
        ops.psf_blur_ragged_u8(packed, meta, one(np.zeros((0, 3), np.int32)))
    with pytest.raises(E, match=r"\(n, 3\)"):
        ops.psf_blur_ragged_u8(packed, meta, one(np.array([[0.0, 0.0, 65536.0]])))
    # cutblur
    params = np.zeros((B, dg.N_PARAMS), np.float32)
    params[:, dg.CUT_SIDE] = 1
    low = torch.zeros_like(packed)
    with pytest.raises(E, match="no CPU fallback"):
        ops.cutblur_ragged_u8(low.cpu(), r["packed"], meta, params)
    for bad_low in (low.cpu(), low[:-1], packed, low.to(torch.int8)):
        with pytest.raises(E, match="low must be"):
            ops.cutblur_ragged_u8(bad_low, packed, meta, params)
    with pytest.raises(E, match="params must be"):
        ops.cutblur_ragged_u8(low, packed, meta, params[:-1])
    for col, v in ((dg.CUT_SIDE, 3), (dg.CUT_X, -1), (dg.CUT_X, 2), (dg.CUT_X, 0.5), (dg.CUT_X, float("nan"))):      # (image 0 is 1 x 1)
        bad = params.copy()
        bad[0, col] = v
        with pytest.raises(E, match="domain"):
            ops.cutblur_ragged_u8(low, packed, meta, bad)
    assert launched == [], launched


# ------------------------------------------------------------------------------------------------- degrade_on_gpu, end to end
def _write_folder(d):
    """the six PNGs of tests/test_gpu_degrade.py"""
    from PIL import Image
    rng = np.random.RandomState(21)
    os.makedirs(d)
    for i in range(6):
        a = rng.randint(0, 256, (12 + 5 * i, 40 + 9 * i, 3)).astype(np.uint8)
        a[:, a.shape[1] // 2:] //= 3
        Image.fromarray(a).save(os.path.join(d, "crop%d.png" % i))
    with open(os.path.join(d, "labels.txt"), "w") as f:
        f.write("crop0.png\thello\ncrop3.png\tw0rld\n")


SETTING = (("motion", "disk", "aniso"), 1.0, 0.3)


def test_degrade_on_gpu_is_the_ops_composed_by_hand(dev, tmp_path):
    from dpmn_amd import ops
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.folder import FolderHR
    _write_folder(str(tmp_path / "hr"))
    ds = FolderHR(str(tmp_path / "hr"), voc_type="all")
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=True, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True, psf=SETTING)
    pair = col([ds[i] for i in range(6)])[0]
    packed_host, meta = pair
    B = meta.shape[0]
    widths, heights = [int(w) for w in meta[:, 2]], [int(h) for h in meta[:, 1]]
    packed = packed_host.to(dev)
    hr_want = ops.collate_u8(ops.resize_ragged_u8(packed, meta, 32, 128), True)

    # ---- the flag off: today's draws and launches
    seed = next(s for s in range(100) if (dg.draw_params(B, cutblur=True, hr_widths=widths, rng=random.Random(s))[:, dg.CUT_SIDE] != 0).sum() >= 2)
    hr0, lr0 = tz.degrade_on_gpu(pair, (32, 128), 2, True, dev, cutblur=True, rng=random.Random(seed), jpeg=(30, 95, 1.0))
    rng = random.Random(seed)
    params = dg.draw_params(B, cutblur=True, hr_widths=widths, rng=rng)
    nseed = rng.getrandbits(63)
    low = ops.resize_ragged_u8(ops.degrade_ragged_u8(packed, meta, params, seed=nseed), meta, 16, 64)
    low = ops.jpeg_roundtrip_u8(low, draw_jpeg(B, 30, 95, 1.0, rng=rng))
    assert torch.equal(hr0, hr_want) and torch.equal(lr0, ops.collate_u8(low, True))

    # ---- the flag on: blur, degrade with the cut zeroed, cutblur from the unblurred pack, resize, JPEG, collate
    hr1, lr1 = tz.degrade_on_gpu(pair, (32, 128), 2, True, dev, cutblur=True, rng=random.Random(seed), jpeg=(30, 95, 1.0), psf=SETTING)
    rng = random.Random(seed)
    params = dg.draw_params(B, cutblur=True, hr_widths=widths, rng=rng)
    nseed = rng.getrandbits(63)
    taps = psf.draw_psf(B, SETTING[0], SETTING[1], SETTING[2], heights, rng=rng)
    q = draw_jpeg(B, 30, 95, 1.0, rng=rng)
    assert not any(psf.is_identity(t) for t in taps)
    uncut = params.copy()
    uncut[:, [dg.CUT_X, dg.CUT_SIDE]] = 0
    blurred = ops.psf_blur_ragged_u8(packed, meta, taps)
    pre = ops.cutblur_ragged_u8(ops.degrade_ragged_u8(blurred, meta, uncut, seed=nseed), packed, meta, params)
    low = ops.jpeg_roundtrip_u8(ops.resize_ragged_u8(pre, meta, 16, 64), q)
    assert torch.equal(lr1, ops.collate_u8(low, True)), "the LR batch is the hand composition"
    assert torch.equal(hr1, hr0), "the HR batch is the unblurred one"
    assert not torch.equal(lr1, lr0)
    n_cut = 0
    for g, b, hr, row in zip(_unpack(pre, meta), _unpack(blurred, meta), _unpack(packed, meta), params):
        cx, side = int(row[dg.CUT_X]), int(row[dg.CUT_SIDE])
        if side:
            n_cut += 1
            cols = slice(cx, None) if side == 1 else slice(0, cx)
            assert np.array_equal(g[:, cols], hr[:, cols]) and not np.array_equal(b[:, cols], hr[:, cols])
    assert n_cut >= 2
    # sr_batches hands the collate's setting on
    loader = type("Loader", (), {"collate_fn": col, "__iter__": lambda self: iter([col([ds[i] for i in range(6)])])})()
    random.seed(3)
    key = random.Random(3).getrandbits(63)
    hr2, lr2 = next(iter(tz.sr_batches(loader, dev)))[:2]
    want = tz.degrade_on_gpu(pair, (32, 128), 2, True, dev, cutblur=True, rng=random.Random(key), psf=SETTING)
    assert torch.equal(hr2, want[0]) and torch.equal(lr2, want[1])


# --------------------------------------------------------------------------------------------------------- training continuation
B, B1, B2 = 4, 2, 2
_RUNS = {}
_LABEL_VECS = {}


def _mission(out_dir, hr_dir):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.utils import synth

    class Filled(TextSR):      # (as in tests/test_gpu_degrade.py: synthetic weights written through the trainer's arena)
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
    args.train_hr_dir, args.manmade_degrade, args.cutblur = hr_dir, True, True
    args.jpeg_degrade, args.jpeg_prob = "30,95", 0.5
    args.psf_blur, args.psf_prob, args.psf_radius = "motion,disk,aniso", 0.75, 0.3
    sr = Filled(cfg, args)
    sr.vis_dir = out_dir
    return sr


def _train(sr, steps, state_path=None):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import synth
    dl = sr.get_train_data()[1]
    col = dl.collate_fn
    assert col.degrade and col.cutblur and col.jpeg == (30, 95, 0.5) and col.psf == (("motion", "disk", "aniso"), 0.75, 0.3)

    def batches(epoch):      # (label vectors handed in, seeded per epoch and batch: tests/test_gpu_degrade.py says why)
        for j, (hr, lr, _, strs) in enumerate(tz.sr_batches(dl, sr.device, sr.mask)):
            key = (epoch, j)
            if key not in _LABEL_VECS:
                _LABEL_VECS[key] = synth.synth_batch(B, seed=50 + 7 * epoch + j)["label_vecs"]
            yield hr, lr, _LABEL_VECS[key]

    models, distill = sr.train(batches, steps=steps, epochs=3, state_path=state_path)
    torch.cuda.synchronize()
    return dict(sd=[{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in models + distill],
                loss=sr.last_loss.cpu().clone(), loop=sr.loop_state)


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def test_training_with_the_stage_stops_and_continues_bitwise(tmp_path_factory):
    """six PNGs, B = 4, three steps, --psf_blur with --cutblur and --jpeg_degrade; stopped after step 1 and continued by a new object
    under other seeds: weights and loss equal the uninterrupted run's bit for bit.  A state written with the flag off refuses a run
    with it on."""
    from dpmn_amd.interfaces import base
    d = tmp_path_factory.mktemp("psf_train")
    hr = str(d / "hr")
    _write_folder(hr)
    _seed(1)
    a = _train(_mission(str(d / "a"), hr), 3)
    _seed(1)
    state = str(d / "b" / "state.pt")
    b = _train(_mission(str(d / "b"), hr), 1, state)
    assert b["loop"]["it"] == 1 and os.path.isfile(state)
    saved = base.read_train_state(state)
    assert saved["fingerprint"]["psf_blur"] == [["motion", "disk", "aniso"], 0.75, 0.3]
    _seed(99)
    got = _train(_mission(str(d / "c"), hr), 3, state)
    assert got["loop"]["it"] == a["loop"]["it"] == 3
    for i, (x, y) in enumerate(zip(a["sd"], got["sd"])):
        for k in x:
            assert torch.equal(x[k], y[k]), "model %d %s differs" % (i, k)
    assert torch.equal(a["loss"], got["loss"]), (float(a["loss"]), float(got["loss"]))
    # the state of a run without the flag
    off = base.read_train_state(state)
    off["fingerprint"]["psf_blur"] = None
    path = str(d / "off.pt")
    base.write_train_state(path, off)
    with pytest.raises(ValueError, match="psf_blur"):
        _train(_mission(str(d / "d"), hr), 3, path)
