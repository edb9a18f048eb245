"""ops.display_triple (csrc/display.hip) against tests/golden/display.npz -- PIL's bicubic resize plus the two torchvision
quantisation formulas (tools/gen_golden.py gen_display) -- on every byte: no tolerance, every stage of the reference is integer
arithmetic or a single fp32 operation.  The kernel has no MFMA variant: both compute modes of the suite must give the same bytes."""
import numpy as np
import pytest
import torch

from helpers import load_golden, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return load_golden("display")


def _diff(got, expected):
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == expected.shape
    return int((got.cpu().numpy() != expected).sum())


def test_case_a_masked_batch_selection_and_quantisation_edges(dev, golden):
    """B = 3, sel = [2, 0], 4-channel inputs read in place: random, binary (overshoot clipping in both passes) and the crafted
    truncation / rounding boundaries of both quantisations."""
    from dpmn_amd import ops
    lr, sr, hr = (torch.from_numpy(golden[k]).to(dev) for k in ("a_lr", "a_sr", "a_hr"))
    sel = torch.from_numpy(golden["a_sel"]).to(dev)
    assert sel.dtype == torch.int32
    n_bad = _diff(ops.display_triple(lr, sr, hr, sel), golden["a_expected"])
    record("display", "case a: differing bytes (4-channel tensors)", n_bad)
    assert n_bad == 0
    # channel-sliced views (what the trainer passes) and a host list of indices: the same bytes, and no hidden copy is needed
    view = lr[:, :3]
    assert not view.is_contiguous()
    assert _diff(ops.display_triple(view, sr[:, :3], hr[:, :3], [2, 0]), golden["a_expected"]) == 0
    # every image on its own equals its rows of the selection
    one = ops.display_triple(lr, sr, hr, [0])
    assert _diff(one, golden["a_expected"][1:2]) == 0
    with pytest.raises(IndexError):
        ops.display_triple(lr, sr, hr, [3])


def test_case_b_non_integer_ratio(dev, golden):
    from dpmn_amd import ops
    lr, sr, hr = (torch.from_numpy(golden[k]).to(dev) for k in ("b_lr", "b_sr", "b_hr"))
    n_bad = _diff(ops.display_triple(lr, sr, hr, [0]), golden["b_expected"])
    record("display", "case b: differing bytes (6x10 -> 16x24)", n_bad)
    assert n_bad == 0


def test_case_c_config4_row_bands(dev, golden):
    """64x256 -> 128x512: the horizontal-pass intermediate of the whole image does not fit the LDS buffer, the rows go in bands."""
    from dpmn_amd import ops
    # (divided on the host, as the generator did: a device division by a scalar may multiply by the reciprocal)
    lr, sr, hr = (torch.from_numpy(golden[k].astype(np.float32) / np.float32(255)).to(dev) for k in ("c_lr_u8", "c_sr_u8", "c_hr_u8"))
    n_bad = _diff(ops.display_triple(lr, sr, hr, [0]), golden["c_expected"])
    record("display", "case c: differing bytes (64x256 -> 128x512)", n_bad)
    assert n_bad == 0


def test_shrinking_is_not_built(dev):
    from dpmn_amd import ops
    big, small = torch.zeros(1, 3, 32, 128, device=dev), torch.zeros(1, 3, 16, 128, device=dev)
    with pytest.raises(NotImplementedError):
        ops.display_triple(big, small, small, [0])          # h > H
    wide = torch.zeros(1, 3, 16, 256, device=dev)
    with pytest.raises(NotImplementedError):
        ops.display_triple(wide, small, small, [0])         # w > W
