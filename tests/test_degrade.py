"""The CPU half of the synthetic-LR path (main.py --manmade_degrade / --cutblur / --train_hr_dir): the draw order of
utils.degrade.draw_params against a literal replay of the reference's sequence (dataset.py:442-489, 622-637), the properties of
utils.degrade.degrade_u8 that can be verified by hand, the folder data set, the collate function's degrade mode and the argument
checks.  No GPU needed."""
import importlib.util
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dpmn_amd.utils import degrade as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay(n, cutblur, widths):
    """The reference's statements, in its order, on Python's global `random` -> (rows, the branches seen)."""
    rows, seen = [], set()
    for i in range(n):
        r = np.zeros(16, np.float32)
        r[0] = [3, 5][random.randint(0, 1)]
        r[1] = random.uniform(5., 6.)
        rand_p = random.random()
        if rand_p > 0.2:
            r[2], r[3], r[4] = 1, random.uniform(0, 0.005), random.uniform(0, 0.015)
        seen.add("noise" if rand_p > 0.2 else "clean")
        choice = random.uniform(0, 1.0)
        if choice < 0.7:
            r[6] = [3, 5][random.randint(0, 1)]
            r[7] = random.uniform(2., 3.)
            seen.add("gauss")
        else:
            r[5], r[8], r[9] = 1, random.uniform(70, 80), random.uniform(70, 80)
            seen.add("bilateral")
        r[10] = [3, 5][random.randint(0, 1)]
        r[11] = random.uniform(2., 3.)
        r[12] = random.uniform(3., 4.)
        if cutblur:
            p = random.random()
            r[13] = int(widths[i] * (0.2 + 0.8 * random.random()))
            if p > 0.7:
                left_mix = random.random()
                r[14] = 1 if left_mix <= 0.5 else 2
            seen.add("cut" if p > 0.7 else "nocut")
        rows.append(r)
    return np.stack(rows), seen


def test_draw_params_consumes_random_in_the_reference_order():
    widths = [17, 64, 130, 200]
    seen = set()
    for s in range(40):
        random.seed(s)
        got = dg.draw_params(4, cutblur=True, hr_widths=widths)
        after = random.random()
        random.seed(s)
        ref, branches = _replay(4, True, widths)
        assert got.dtype == np.float32 and got.shape == (4, 16)
        assert np.array_equal(got, ref), s
        assert random.random() == after, "the stream stands elsewhere after seed %d" % s
        seen |= branches
        if seen >= {"noise", "clean", "gauss", "bilateral", "cut", "nocut"} and s >= 3:
            break
    assert seen >= {"noise", "clean", "gauss", "bilateral", "cut", "nocut"}, seen
    # test=True and cutblur=False draw nothing for cutblur; an own generator is honoured
    for kw in (dict(cutblur=True, test=True), dict()):
        random.seed(7)
        got = dg.draw_params(3, **kw)
        random.seed(7)
        assert np.array_equal(got, _replay(3, False, None)[0]) and not got[:, 13:].any()
    assert np.array_equal(dg.draw_params(3, rng=random.Random(7)), got)
    with pytest.raises(ValueError):
        dg.draw_params(2, cutblur=True)


def _rows():
    """hand-set rows: gauss NR / bilateral NR"""
    g = np.array([5, 5.5, 0, 0, 0, 0, 3, 2.5, 0, 0, 5, 2.5, 3.5, 0, 0, 0], np.float32)
    b = np.array([3, 5.2, 0, 0, 0, 1, 0, 0, 75, 72, 3, 2.2, 3.9, 0, 0, 0], np.float32)
    return g, b


def test_reflect101_folds_repeatedly():
    assert dg.reflect101(np.arange(-7, 8), 1).tolist() == [0] * 15
    assert dg.reflect101(np.arange(-4, 7), 3).tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]
    assert dg.reflect101(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_images_and_the_white_branch(dtype):
    z = np.random.RandomState(0).randn(9, 11, 3)
    for row in _rows():
        for v in (0, 1, 100, 254, 255):
            out = dg.degrade_u8(np.full((9, 11, 3), v, np.uint8), row, z, dtype)
            assert out.dtype == np.uint8 and (out == v).all(), (v, out.min(), out.max())
        noisy = row.copy()
        noisy[2:5] = 1, 0.005, 0.015
        assert (dg.degrade_u8(np.full((9, 11, 3), 255, np.uint8), noisy, z, dtype) == 255).all()      # mean > 252: no noise
        noisy[3] = 0.5                              # (a standard deviation of 7 grey levels: visible behind the noise reduction)
        assert (dg.degrade_u8(np.full((9, 11, 3), 255, np.uint8), noisy, z, dtype) == 255).all()
        assert (dg.degrade_u8(np.full((9, 11, 3), 100, np.uint8), noisy, z, dtype) != 100).any()      # below 252 the noise is added


def test_tiny_images_run():
    rng = np.random.RandomState(1)
    for shape in ((1, 1, 3), (1, 7, 3), (2, 3, 3)):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        for row in _rows():
            row = row.copy()
            row[2:5] = 1, 0.004, 0.01
            out = dg.degrade_u8(img, row, rng.randn(*shape))
            assert out.shape == shape and out.dtype == np.uint8
    one = np.array([[[10, 200, 77]]], np.uint8)
    assert np.array_equal(dg.degrade_u8(one, _rows()[0], np.zeros((1, 1, 3))), one)      # every tap folds onto the one pixel


def test_cutblur_columns_are_the_hr_image():
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, (6, 20, 3)).astype(np.uint8)
    z = rng.randn(6, 20, 3)
    row = _rows()[0]
    plain = dg.degrade_u8(img, row, z)
    for side in (1, 2):
        r = row.copy()
        r[13], r[14] = 8, side
        out = dg.degrade_u8(img, r, z)
        hr = slice(8, None) if side == 1 else slice(0, 8)
        lr = slice(0, 8) if side == 1 else slice(8, None)
        assert np.array_equal(out[:, hr], img[:, hr]) and np.array_equal(out[:, lr], plain[:, lr])
        assert not np.array_equal(plain[:, hr], img[:, hr])
    r = row.copy()
    r[13] = 8                                   # a cut without a side: nothing is replaced
    assert np.array_equal(dg.degrade_u8(img, r, z), plain)


def _folder(tmp_path, n=4):
    from PIL import Image
    rng = np.random.RandomState(3)
    d = tmp_path / "hr"
    d.mkdir()
    imgs = {}
    for i in range(n):
        a = rng.randint(0, 256, (8 + i, 20 + 3 * i, 3)).astype(np.uint8)
        imgs["im%d.png" % i] = a
        Image.fromarray(a).save(str(d / ("im%d.png" % i)))
    (d / "notes.bin").write_bytes(b"not an image")
    return d, imgs


def test_folder_hr(tmp_path, capsys):
    from dpmn_amd.dataset.folder import FolderHR
    d, imgs = _folder(tmp_path)
    ds = FolderHR(str(d))
    assert "skipping notes.bin" in capsys.readouterr().out
    assert len(ds) == 4 and ds.files == sorted(imgs)
    hr, lr, a, b, label = ds[2]
    assert hr is lr and a is None and b is None and label == ""      # str_filt drops the blank, as for an LMDB without label
    assert hr.mode == "RGB" and np.array_equal(np.asarray(hr), imgs["im2.png"])
    (d / "labels.txt").write_text("im1.png\tHello!\nim3.png\tw0rd\nno tab here\n")
    ds = FolderHR(str(d))
    assert len(ds) == 4 and [ds[i][4] for i in range(4)] == ["", "Hello", "", "w0rd"]
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        FolderHR(str(empty))


def test_collate_degrade_packs_the_hr_pixels_once(tmp_path):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.folder import FolderHR
    d, imgs = _folder(tmp_path)
    ds = FolderHR(str(d))
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=True, gpu_finish=True, gpu_resize=True,
                                       degrade=True, cutblur=True)
    out = col([ds[i] for i in range(4)])
    assert out[2] is out[0] and len(out) == 9
    packed, meta = out[0]
    assert packed.dtype == torch.uint8 and meta.shape == (4, 3)
    for (off, h, w), name in zip(meta.tolist(), sorted(imgs)):
        assert np.array_equal(packed.numpy()[off:off + h * w * 3].reshape(h, w, 3), imgs[name])
    with pytest.raises(ValueError, match="gpu_resize"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, degrade=True)
    with pytest.raises(ValueError, match="cutblur"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, cutblur=True)
    # without the flags the collate is what it was: two separately packed pairs
    plain = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, gpu_finish=True, gpu_resize=True)([ds[i] for i in range(4)])
    assert plain[2] is not plain[0] and torch.equal(plain[2][0], plain[0][0])


class _Env:
    """the `begin().get(key)` protocol of an LMDB environment over a dict (as in tests/test_dataset.py)"""

    def __init__(self, d):
        self.d = d

    def begin(self, write=False):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def get(self, key):
        return self.d.get(key)


def test_lmdb_dataset_with_manmade_degrade_does_not_read_the_lr_image():
    import io
    from PIL import Image
    from dpmn_amd.dataset import textzoom as tz
    buf = io.BytesIO()
    Image.fromarray(np.random.RandomState(4).randint(0, 256, (16, 40, 3)).astype(np.uint8)).save(buf, format="PNG")
    env = _Env({b"num-samples": b"1", b"image_hr-000000001": buf.getvalue(), b"label-000000001": b"word"})      # no image_lr-* at all
    ds = tz.lmdbDataset_real(env=env, manmade_degrade=True, cutblur=True)
    hr, lr, _, _, label = ds[0]
    assert lr is hr and hr.size == (40, 16) and label == "word"
    with pytest.raises(ValueError, match="cutblur"):
        tz.lmdbDataset_real(env=env, cutblur=True)


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_degrade", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cutblur_without_manmade_degrade_exits_with_one_clear_line(tmp_path):
    m = _main()
    with pytest.raises(SystemExit) as e:
        m.main(SimpleNamespace(), SimpleNamespace(cutblur=True, manmade_degrade=False, train_hr_dir=None))
    assert str(e.value) .startswith("main.py: --cutblur needs --manmade_degrade") and "\n" not in str(e.value)
    with pytest.raises(SystemExit, match="--train_hr_dir .* is not a directory"):
        m.main(SimpleNamespace(), SimpleNamespace(cutblur=True, manmade_degrade=False, train_hr_dir=str(tmp_path / "missing")))


def test_fingerprint_carries_the_three_flags():
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))

    def args(**kw):
        a = dict(arch="tatt", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="4,", embed_dim="96,", depths="1,",
                 num_heads="6,", window_size="2,4,8,", mlp_ratio="4,")
        a.update(kw)
        return SimpleNamespace(**a)

    plain = base.state_fingerprint(args(), cfg)
    assert (plain["manmade_degrade"], plain["cutblur"], plain["train_hr_dir"]) == (False, False, False)
    old = {k: v for k, v in plain.items() if k not in base.DATA_FIELDS}      # a state written before the flags existed
    base.check_fingerprint(old, plain)
    for kw, field in ((dict(manmade_degrade=True), "manmade_degrade"), (dict(manmade_degrade=True, cutblur=True), "manmade_degrade"),
                      (dict(train_hr_dir="/some/dir"), "manmade_degrade")):
        with pytest.raises(ValueError, match=field):
            base.check_fingerprint(plain, base.state_fingerprint(args(**kw), cfg))
        with pytest.raises(ValueError, match=field):
            base.check_fingerprint(old, base.state_fingerprint(args(**kw), cfg))
    deg = base.state_fingerprint(args(manmade_degrade=True), cfg)
    with pytest.raises(ValueError, match="cutblur"):
        base.check_fingerprint(deg, base.state_fingerprint(args(manmade_degrade=True, cutblur=True), cfg))
    with pytest.raises(ValueError, match="train_hr_dir"):
        base.check_fingerprint(deg, base.state_fingerprint(args(train_hr_dir="/some/dir"), cfg))
