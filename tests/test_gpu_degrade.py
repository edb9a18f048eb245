"""Synthetic LR images on the GPU (csrc/degrade.hip through ops.degrade_ragged_u8 / ops.degrade_noise) against the float64 NumPy
restatement utils.degrade.degrade_u8, the generated noise field, run-to-run determinism, and the training path on top of it:
TextSR.train from a folder of HR images (--train_hr_dir, --manmade_degrade, --cutblur) stopped and continued from its state file."""
import os
import random

import numpy as np
import pytest
import torch

from dpmn_amd.utils import degrade as dg
from dpmn_amd.utils.resize import pack_ragged

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (2, 3), (5, 40), (16, 64), (33, 130), (47, 200), (8, 8)]      # the last one is all white
#         pre_k sig  noise shot   read   mode nr_k sig  s_col s_spc shp_k sig  gain cut_x side
ROWS = [[3, 5.1, 1, 0.004, 0.010, 0, 3, 2.1, 0, 0, 3, 2.2, 3.1, 0, 0, 0],
        [5, 5.9, 1, 0.002, 0.015, 1, 0, 0, 71, 79, 5, 2.9, 4.0, 3, 1, 0],
        [5, 5.5, 0, 0, 0, 0, 5, 2.9, 0, 0, 3, 2.5, 3.5, 1, 2, 0],
        [3, 5.3, 1, 0.005, 0.005, 1, 0, 0, 79, 70, 5, 2.0, 4.0, 13, 2, 0],
        [5, 6.0, 1, 0.001, 0.012, 0, 5, 2.4, 0, 0, 5, 2.7, 3.8, 40, 1, 0],
        [3, 5.0, 0, 0, 0, 1, 0, 0, 75, 75, 3, 3.0, 3.0, 0, 0, 0],
        [5, 5.7, 1, 0.005, 0.015, 0, 3, 3.0, 0, 0, 5, 2.3, 4.0, 77, 2, 0],
        [3, 5.4, 1, 0.005, 0.015, 1, 0, 0, 72, 78, 3, 2.6, 3.3, 0, 0, 0]]
_REF = {}


def _inputs():
    """The batch, its params, the noise field and the two CPU results (float64, float32): made once, never changed."""
    if not _REF:
        rng = np.random.RandomState(11)
        images = []
        for h, w in SIZES[:-1]:
            a = rng.randint(0, 256, (h, w, 3)).astype(np.int32)
            a[:, w // 3:] = np.clip(a[:, w // 3:] // 4 + 150, 0, 255)          # step edges over the noise
            a[h // 2:, : w // 2] = a[h // 2:, : w // 2] // 3
            a[:, (3 * w) // 4:] = 255 - a[:, (3 * w) // 4:] // 2
            images.append(a.astype(np.uint8))
        images.append(np.full(SIZES[-1] + (3,), 255, np.uint8))
        params = np.array(ROWS, np.float32)
        zs = [rng.randn(h, w, 3).astype(np.float32) for h, w in SIZES]
        ref64 = [dg.degrade_u8(im, p, z) for im, p, z in zip(images, params, zs)]
        ref32 = [dg.degrade_u8(im, p, z, np.float32) for im, p, z in zip(images, params, zs)]
        packed, meta = pack_ragged(images, pin=False)
        _REF.update(images=images, params=params, zs=zs, ref64=ref64, ref32=ref32, packed=packed, meta=meta,
                    z=torch.from_numpy(np.concatenate([z.reshape(-1) for z in zs])))
    return _REF


def _unpack(buf, meta):
    flat = buf.cpu().numpy()
    return [flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in meta.tolist()]


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def test_parity_with_the_float64_restatement(dev):
    """(a) derived: max |difference| <= 6 grey levels -- one flipped 8-bit intermediate through the unsharp mask at gain 4 (1 + 4) plus
    the final truncation; (b) measured on the CPU here: the share of differing bytes is at most 4 x the share by which the float32
    restatement differs from the float64 one; (c) a condition: no noisy image's pre-blur mean lies within 252 +- 0.5."""
    from dpmn_amd import ops
    from helpers import record
    r = _inputs()
    p = r["params"]
    assert set(p[:, 0]) == set(p[:, 10]) == set(p[p[:, 5] == 0][:, 6]) == {3, 5} and set(p[:, 5]) == {0, 1}
    assert set(p[:, 2]) == {0, 1} and set(p[:, 14]) == {0, 1, 2}
    for im, row in zip(r["images"], p):                                            # (c)
        if row[2]:
            mean = dg.gauss_blur(im.astype(np.float64), row[0], row[1]).mean()
            assert abs(mean - 252.0) > 0.5, mean
    assert dg.gauss_blur(r["images"][-1].astype(np.float64), p[-1][0], p[-1][1]).mean() > 252.5 and p[-1][2] == 1
    got = _unpack(ops.degrade_ragged_u8(r["packed"].to(dev), r["meta"], p, z=r["z"].to(dev)), r["meta"])
    n = sum(a.size for a in r["ref64"])
    d32 = sum(int((a != b).sum()) for a, b in zip(r["ref32"], r["ref64"]))
    dgpu = sum(int((a != b).sum()) for a, b in zip(got, r["ref64"]))
    worst = max(int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) for a, b in zip(got, r["ref64"]))
    per_image = [int((a != b).sum()) for a, b in zip(got, r["ref64"])]
    print("degrade parity: %d bytes, float32 vs float64 restatement %d differ (share %.3g), GPU vs float64 %d differ (share %.3g), "
          "max |diff| %d, per image %s" % (n, d32, d32 / n, dgpu, dgpu / n, worst, per_image))
    record("degrade", "bytes differing from the float64 restatement (of %d; float32 restatement: %d)" % (n, d32), dgpu, 4 * d32)
    record("degrade", "max |GPU - float64 restatement| in grey levels", worst, 6)
    assert np.array_equal(got[-1], r["images"][-1]), "the white image (mean > 252) must pass unchanged: no noise, flat"
    for g, im, row in zip(got, r["images"], p):                                    # cutblur columns are the HR image's, exactly
        cx = int(row[13])
        if row[14] == 1:
            assert np.array_equal(g[:, cx:], im[:, cx:])
        elif row[14] == 2:
            assert np.array_equal(g[:, :cx], im[:, :cx])
    assert worst <= 6, worst                                                        # (a)
    assert dgpu / n <= 4 * d32 / n, (dgpu, d32, n)                                  # (b)


def test_same_call_twice_gives_the_same_bytes(dev):
    from dpmn_amd import ops
    r = _inputs()
    packed, z = r["packed"].to(dev), r["z"].to(dev)
    a = ops.degrade_ragged_u8(packed, r["meta"], r["params"], z=z)
    b = ops.degrade_ragged_u8(packed, r["meta"].numpy(), torch.from_numpy(r["params"]), z=z)
    assert torch.equal(a, b)
    c, d = ops.degrade_ragged_u8(packed, r["meta"], r["params"], seed=5), ops.degrade_ragged_u8(packed, r["meta"], r["params"], seed=5)
    assert torch.equal(c, d) and not torch.equal(a, c)


def test_noise_field(dev):
    """~10^5 samples: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N) (five standard errors); other seed, other field; same seed,
    same bytes; the fused path with the seed equals the fused path fed with the field."""
    from dpmn_amd import ops
    from helpers import record
    meta = pack_ragged([np.zeros((h, w, 3), np.uint8) for h, w in ((47, 200), (64, 300), (33, 130), (1, 7))], pin=False)[1]
    f = ops.degrade_noise(1234, meta)
    N = f.numel()
    assert f.is_cuda and f.dtype == torch.float32 and N == 3 * (47 * 200 + 64 * 300 + 33 * 130 + 7) and N > 9e4
    x = f.double().cpu().numpy()
    mean, var = x.mean(), x.var()
    print("degrade noise: N %d mean %.3g (bound %.3g) var - 1 %.3g (bound %.3g)" % (N, mean, 5 / np.sqrt(N), var - 1, 5 * np.sqrt(2 / N)))
    record("degrade_noise", "|mean| of %d samples" % N, abs(mean), 5 / np.sqrt(N))
    record("degrade_noise", "|var - 1|", abs(var - 1), 5 * np.sqrt(2 / N))
    assert np.isfinite(x).all()
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert torch.equal(f, ops.degrade_noise(1234, meta.numpy()))
    g = ops.degrade_noise(1235, meta)
    assert not torch.equal(f, g) and float((f == g).double().mean()) < 1e-3
    r = _inputs()
    packed = r["packed"].to(dev)
    field = ops.degrade_noise(2 ** 63 - 5, r["meta"])
    assert field.numel() == packed.numel()
    assert torch.equal(ops.degrade_ragged_u8(packed, r["meta"], r["params"], seed=2 ** 63 - 5),
                       ops.degrade_ragged_u8(packed, r["meta"], r["params"], z=field))


def test_cpu_tensors_and_bad_arguments_are_rejected(dev):
    from dpmn_amd import _abi, ops
    r = _inputs()
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.degrade_ragged_u8(r["packed"], r["meta"], r["params"])
    packed = r["packed"].to(dev)
    with pytest.raises(_abi.DpmnError):
        ops.degrade_ragged_u8(packed, r["meta"], r["params"], z=r["z"])             # z on the CPU
    with pytest.raises(_abi.DpmnError):
        ops.degrade_ragged_u8(packed[:-1], r["meta"], r["params"])                  # the meta points past the buffer
    with pytest.raises(_abi.DpmnError):
        ops.degrade_ragged_u8(packed, r["meta"], r["params"][:-1])                  # a row is missing
    bad = r["params"].copy()
    bad[0, 0] = 7
    with pytest.raises(_abi.DpmnError, match="domain"):
        ops.degrade_ragged_u8(packed, r["meta"], bad)
    with pytest.raises(_abi.DpmnError):
        ops.degrade_noise(1, r["meta"], device="cpu")


def _write_folder(d):
    from PIL import Image
    rng = np.random.RandomState(21)
    os.makedirs(d)
    for i in range(6):
        a = rng.randint(0, 256, (12 + 5 * i, 40 + 9 * i, 3)).astype(np.uint8)
        a[:, a.shape[1] // 2:] //= 3
        Image.fromarray(a).save(os.path.join(d, "crop%d.png" % i))
    with open(os.path.join(d, "labels.txt"), "w") as f:
        f.write("crop0.png\thello\ncrop3.png\tw0rld\n")


def test_sr_batches_draws_per_pass_and_batch(dev, tmp_path):
    """A pass takes ONE draw from Python's `random` when it starts; what follows does not depend on where that stream stands (the
    training loop fetches a batch before it writes the state of the step before).  The LR batch is the degraded HR batch: same
    shapes as a paired batch, not the resized HR image."""
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.folder import FolderHR
    _write_folder(str(tmp_path / "hr"))
    ds = FolderHR(str(tmp_path / "hr"), voc_type="all")
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=True, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True)
    batches = [col([ds[i] for i in (0, 1, 2)]), col([ds[i] for i in (3, 4, 5)])]
    loader = type("Loader", (), {"collate_fn": col, "__iter__": lambda self: iter(batches)})()
    random.seed(3)
    a = list(tz.sr_batches(loader, dev))
    after = random.random()
    random.seed(3)
    it = tz.sr_batches(loader, dev)
    b0 = next(it)
    assert random.random() == after, "a pass draws once, when it starts"
    random.seed(999)
    b1 = next(it)
    assert torch.equal(a[0][1], b0[1]) and torch.equal(a[1][1], b1[1]) and torch.equal(a[1][0], b1[0])
    hr, lr, lv, strs = a[0]
    assert hr.shape == (3, 4, 32, 128) and lr.shape == (3, 4, 16, 64) and lv is None and strs == ["hello", "", ""]
    plain = tz.resize_on_gpu(batches[0][0], (16, 64), True, dev)
    assert torch.equal(hr, tz.resize_on_gpu(batches[0][0], (32, 128), True, dev)) and not torch.equal(lr, plain)
    random.seed(4)
    assert not torch.equal(next(tz.sr_batches(loader, dev))[1], lr)


B, B1, B2 = 4, 2, 2
_RUNS = {}
_LABEL_VECS = {}


def _mission(out_dir, hr_dir):
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
    args.train_hr_dir, args.manmade_degrade, args.cutblur = hr_dir, True, True
    sr = Filled(cfg, args)
    sr.vis_dir = out_dir
    return sr


def _train(sr, steps, state_path=None):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.utils import synth
    dl = sr.get_train_data()[1]
    assert dl.collate_fn.degrade and dl.collate_fn.cutblur and dl.collate_fn.gpu_resize

    def batches(epoch):
        """TATT's label_vecs come with the batch, as in tests/test_gpu_train_state.py (seeded, per epoch and batch): with the frozen
        CRNN computing them inside the loop (label_vecs_from_crnn), two uninterrupted runs of this very configuration on the SAME
        recorded CPU batches already end with different losses from step 2 on (measured: 1975.35 vs 1975.95 at step 2, step 1 equal;
        with label_vecs given, 1975.97461 both times) -- a property of the training step beside a recogniser, not of the data path
        under test here."""
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


def _runs(tmp_path_factory):
    """The uninterrupted run A (3 steps) and run B stopped after step 1, once per compute mode."""
    from dpmn_amd import _abi
    key = _abi.lib.dpmn_get_compute_dtype()
    if key not in _RUNS:
        d = tmp_path_factory.mktemp("degrade_train")
        _write_folder(str(d / "hr"))
        _seed(1)
        a = _train(_mission(str(d / "a"), str(d / "hr")), 3)
        _seed(1)
        state = str(d / "b" / "state.pt")
        b = _train(_mission(str(d / "b"), str(d / "hr")), 1, state)
        assert b["loop"]["it"] == 1 and os.path.isfile(state)
        _RUNS[key] = dict(A=a, dir=d, state=state)
    return _RUNS[key]


def test_training_from_a_folder_stops_and_continues_bitwise(tmp_path, tmp_path_factory):
    """six PNGs, B = 4 (one batch per epoch), three steps; stopped after step 1 and continued by a new object under other seeds:
    weights and losses equal the uninterrupted run's bit for bit -- the shuffled order and the LR images of steps 2 and 3 came from
    the captured streams."""
    ref = _runs(tmp_path_factory)
    state = str(tmp_path / "state.pt")
    os.link(ref["state"], state)
    _seed(99)
    got = _train(_mission(str(tmp_path), str(ref["dir"] / "hr")), 3, state)
    a = ref["A"]
    assert got["loop"]["it"] == a["loop"]["it"] == 3
    for i, (x, y) in enumerate(zip(a["sd"], got["sd"])):
        for k in x:
            assert torch.equal(x[k], y[k]), "model %d %s differs" % (i, k)
    assert torch.equal(a["loss"], got["loss"]), (float(a["loss"]), float(got["loss"]))


def test_state_without_the_flags_refuses_a_run_with_them(tmp_path, tmp_path_factory):
    from dpmn_amd.interfaces import base
    ref = _runs(tmp_path_factory)
    state = base.read_train_state(ref["state"])
    assert state["fingerprint"]["manmade_degrade"] and state["fingerprint"]["cutblur"] and state["fingerprint"]["train_hr_dir"]
    for k in base.DATA_FIELDS:
        state["fingerprint"][k] = False                 # the file a run without the flags writes
    path = str(tmp_path / "plain.pt")
    base.write_train_state(path, state)
    sr = _mission(str(tmp_path), str(ref["dir"] / "hr"))
    with pytest.raises(ValueError, match="manmade_degrade"):
        _train(sr, 3, path)
