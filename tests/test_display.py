"""CPU checks of the comparison-image path (dpmn_amd/utils/display.py on the resample core of utils/resize.py; tripple_display /
test_display, interfaces/base.py:275-326 of the reference): the coefficient tables the kernel reads reproduce PIL's bicubic resize exactly, the / 255 round trip of the enlarged
LR image is the identity, the file-name rule, and the fixture tests/golden/display.npz against the numpy restatement."""
import numpy as np
import pytest
import torch

from dpmn_amd.utils import display as dsp, resize
from helpers import load_golden

CASES = [(16, 64, 32, 128),       # config 1
         (64, 256, 128, 512),     # config 4
         (6, 10, 16, 24),         # non-integer ratio: the edge bounds
         (16, 64, 16, 64)]        # equal size


@pytest.mark.parametrize("h,w,H,W", CASES)
def test_tables_through_numpy_two_pass_equal_pil_resize(h, w, H, W):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(h * 1000 + W)
    for img in (rng.randint(0, 256, (h, w, 3)).astype(np.uint8), (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)):
        ref = np.asarray(Image.fromarray(img).resize((W, H), Image.BICUBIC))
        got = resize.pil_resize_u8(img, H, W)
        assert got.shape == ref.shape and got.dtype == np.uint8
        assert int((got != ref).sum()) == 0


def test_tables_layout_bounds_and_cache():
    for insz, outsz in ((16, 32), (64, 128), (6, 16), (10, 24), (16, 16), (256, 512)):
        t = resize.pil_resample_tables(insz, outsz)
        assert t.dtype == np.int32 and t.shape == (outsz, 7) and not t.flags.writeable
        assert (t[:, 0] >= 0).all() and (t[:, 1] >= 1).all() and (t[:, 0] + t[:, 1] <= insz).all()
        assert (np.diff(t[:, 0]) >= 0).all() and (np.diff(t[:, 0] + t[:, 1]) >= 0).all()      # the kernel's row bands rely on it
        for row in t:
            assert (row[2 + row[1]:] == 0).all()
            assert abs(int(row[2:].sum()) - (1 << 22)) <= 4            # normalised weights, 22 fraction bits
            assert 255 * int(np.abs(row[2:].astype(np.int64)).sum()) + (1 << 21) < 2 ** 31      # int32 accumulation is enough
        assert resize.pil_resample_tables(insz, outsz) is t
    eq = resize.pil_resample_tables(16, 16)
    assert all(int(eq[i, 2 + i - eq[i, 0]]) == 1 << 22 for i in range(16))      # equal size: the identity


def test_div255_round_trip_is_the_identity():
    """The enlarged LR image passes ToTensor (/ 255) and save_image's quantisation again: no kernel work is spent on it."""
    k = torch.arange(256, dtype=torch.uint8)
    back = k.float().div(255).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    assert torch.equal(back, k)
    assert np.array_equal(dsp.quantize_sr(np.arange(256, dtype=np.float32) / np.float32(255)), np.arange(256, dtype=np.uint8))


def test_quantisation_restatements_equal_the_torch_formulas():
    g = load_golden("display")
    x = torch.from_numpy(np.concatenate([g["edge_sr"], g["edge_lr"], g["a_sr"].reshape(-1)[:4096]]))
    assert np.array_equal(dsp.quantize_sr(x.numpy()), x.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy())
    assert np.array_equal(dsp.quantize_lr(x.numpy()), x.clone().mul(255).clamp_(0, 255).to(torch.uint8).numpy())
    # outside [0, 1] (undefined in the reference) and NaN: clamped
    odd = np.array([-3.0, -1e-9, 1.5, 300.0, np.nan, np.inf, -np.inf], np.float32)
    assert dsp.quantize_lr(odd).tolist() == [0, 0, 255, 255, 0, 255, 0]
    assert dsp.quantize_sr(odd).tolist() == [0, 0, 255, 255, 0, 255, 0]


def test_image_name_rule():
    assert dsp.image_name("ab", "abc", "ABC") == "ab_abc_ABC_.png"
    assert dsp.image_name("a/b", "/", "x/y/") == "ab__xy_.png"
    assert dsp.image_name("", "", "") == "___.png"
    assert dsp.image_name("", "sr", "") == "_sr__.png"
    assert "/" not in dsp.image_name("../../etc", "..", "/root")


def test_fixture_is_self_consistent():
    g = load_golden("display")
    sel = g["a_sel"].tolist()
    assert sel == [2, 0] and g["a_lr"].shape == (3, 4, 16, 64) and g["a_sr"].shape == g["a_hr"].shape == (3, 4, 32, 128)
    exp = g["a_expected"]
    assert exp.shape == (2, 96, 128, 3) and exp.dtype == np.uint8
    assert np.array_equal(dsp.triple_reference(g["a_lr"], g["a_sr"], g["a_hr"], sel), exp)
    assert not np.array_equal(exp[0], exp[1])
    # the crafted edge values sit in image 2, every channel; image 1 is binary; the 4th channel is not 0
    for c in range(3):
        assert np.isin(g["edge_lr"], g["a_lr"][2, c]).all()
        assert np.isin(g["edge_sr"], g["a_sr"][2, c]).all() and np.isin(g["edge_sr"], g["a_hr"][2, c]).all()
    assert g["edge_lr"].size == 768 and g["edge_sr"].size == 1536
    assert set(np.unique(g["a_lr"][1, :3]).tolist()) == {0.0, 1.0}
    assert (g["a_lr"][:, 3] != 0).all() and (g["a_sr"][:, 3] != 0).all() and (g["a_hr"][:, 3] != 0).all()
    assert int(g["overshoot"][0]) >= 100 and int(g["overshoot"][1]) >= 100
    assert np.array_equal(dsp.triple_reference(g["b_lr"], g["b_sr"], g["b_hr"], [0]), g["b_expected"])
    assert g["b_expected"].shape == (1, 48, 24, 3)
    c = [g[k].astype(np.float32) / np.float32(255) for k in ("c_lr_u8", "c_sr_u8", "c_hr_u8")]
    assert g["c_expected"].shape == (1, 384, 512, 3)
    assert np.array_equal(dsp.triple_reference(c[0], c[1], c[2], [0]), g["c_expected"])


def test_display_triple_rejects_cpu_tensors():
    from dpmn_amd import _abi, ops
    with pytest.raises(_abi.DpmnError):
        ops.display_triple(torch.zeros(1, 3, 16, 64), torch.zeros(1, 3, 32, 128), torch.zeros(1, 3, 32, 128), [0])
