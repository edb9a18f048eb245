"""GPU parity of the native CRNN recogniser (model/crnn.py NativeCRNN, csrc/crnn.hip): the prep (bicubic + luma), the padded
stride-(2,1) max-pool, one BiLSTM layer, the whole forward against the imported reference's outputs (tests/golden/crnn.npz) and
against the stock-operator mirror on the CPU, the greedy CTC strings, and batch independence."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dpmn_amd.utils import synth
from helpers import load_golden, t, assert_close, record, max_abs_err

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-6          # measured <= 2e-7 (fp32 and x3) on logits of magnitude 0.1-0.3 (the synthetic recognisers)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _weights(seed, zero_bias):
    """Name-seeded synthetic CRNN weights; zero_bias=True drops the conv and LSTM / Linear biases, which otherwise dominate the
    logits of random weights and make every image read the same string."""
    from dpmn_amd.model.crnn import CRNN
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=seed)
    if zero_bias:
        for k, v in sd.items():
            if (k.startswith("rnn.") and "bias" in k) or (k.startswith("cnn.conv") and k.endswith(".bias")):
                v.zero_()
    return sd


def _pair(dev, seed=71, zero_bias=True):
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    sd = _weights(seed, zero_bias)
    ref = CRNN(32, 1, 37, 256).eval()
    ref.load_state_dict(sd)
    nat = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    nat.load_state_dict(sd)
    return ref, nat


def _images(B, H, W, seed):
    """Column stripes of random grey levels plus noise: images whose readings differ from one another."""
    blocks = synth.uniform("crnn_blocks", (B, 1, 2, W // 8), 0, 1, seed)
    x = blocks.repeat_interleave(H // 2, 2).repeat_interleave(8, 3).expand(B, 3, H, W)
    return (0.8 * x + 0.2 * synth.uniform("crnn_noise", (B, 3, H, W), 0, 1, seed)).contiguous()


def _ref_decode(logits):
    """eval()'s CRNN branch (super_resolution.py:474-479) with strLabelConverter.decode(raw=False) restated: arg-max per step,
    collapse repeats, drop blank 0, class c -> ALPHABET[c - 1]."""
    from dpmn_amd.model.crnn import ALPHABET
    out = []
    for row in logits.argmax(2).t().tolist():
        s, prev = [], -1
        for c in row:
            if c != 0 and c != prev:
                s.append(ALPHABET[c - 1])
            prev = c
        out.append("".join(s))
    return out


@pytest.mark.parametrize("hw", [(16, 64), (32, 128)])
@pytest.mark.parametrize("channels", [3, 4])
def test_prep_matches_bicubic_and_luma(dev, hw, channels):
    from dpmn_amd import ops
    x = synth.uniform("crnn_prep", (5, channels) + hw, 0, 1, 3)
    got = ops.crnn_prep(x.to(dev), 32, 100).cpu()
    y = F.interpolate(x[:, :3], (32, 100), mode='bicubic')
    ref = 0.299 * y[:, 0:1] + 0.587 * y[:, 1:2] + 0.114 * y[:, 2:3]
    err = record("crnn_prep", "%dx%d %dch max|err|" % (hw + (channels,)), max_abs_err(got[..., 0:1].permute(0, 3, 1, 2), ref), 1e-6)
    assert err <= 1e-6
    assert torch.count_nonzero(got[..., 1:]) == 0
    # a channel-sliced view is read in place (the SR output's sr[:, :3])
    got_v = ops.crnn_prep(x.to(dev)[:, :3], 32, 100).cpu()
    assert torch.equal(got_v, got)


@pytest.mark.parametrize("shape", [(3, 8, 25, 256), (2, 4, 26, 512), (1, 4, 26, 64)])
def test_maxpool_stride21_pad01_exact(dev, shape):
    from dpmn_amd import ops
    x = synth.uniform("crnn_pool", shape, -2, 1, 5)
    got = ops.maxpool2d(x.to(dev), (2, 2), (2, 1), (0, 1)).cpu()
    ref = nn.MaxPool2d((2, 2), (2, 1), (0, 1))(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("B", [1, 50])
def test_bilstm_layer_vs_torch_lstm(dev, B):
    from dpmn_amd import ops
    torch.manual_seed(17)
    lstm = nn.LSTM(512, 256, bidirectional=True)
    T = 26
    x = synth.uniform("crnn_lstm_x", (T, B, 512), -1, 1, 7)
    with torch.no_grad():
        ref, _ = lstm(x)
    sd = {k: v.detach().to(dev) for k, v in lstm.state_dict().items()}
    w_ih = torch.cat([sd["weight_ih_l0"], sd["weight_ih_l0_reverse"]], 0).contiguous()
    b = torch.cat([sd["bias_ih_l0"] + sd["bias_hh_l0"], sd["bias_ih_l0_reverse"] + sd["bias_hh_l0_reverse"]], 0).contiguous()
    w_hh = torch.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]], 0).contiguous()
    rows = x.permute(1, 0, 2).reshape(B * T, 512).contiguous().to(dev)
    out = ops.bilstm(ops.linear(rows, w_ih, b), w_hh, B, T).view(B, T, 512).permute(1, 0, 2).cpu()
    err = record("crnn_bilstm", "B=%d max|err| vs nn.LSTM" % B, max_abs_err(out, ref), 2e-5)
    assert err < 2e-5


def test_native_logits_and_label_vecs_vs_reference_golden(dev):
    from dpmn_amd.model.crnn import NativeCRNN
    g = load_golden("crnn")
    m = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    m.load_state_dict({k: v.to(dev) for k, v in _weights(71, False).items()})
    imgs = synth.uniform("crnn_lr", (3, 3, 16, 64), 0, 1, 72).to(dev)
    logits = m(m.parse_crnn_data(imgs)).cpu()
    record("crnn_golden", "logits max|err| vs reference", max_abs_err(logits, t(g["logits"])), LOGIT_TOL)
    assert_close(logits, t(g["logits"]), LOGIT_TOL, 0.0, "native CRNN logits vs the reference")
    lv = m.label_vecs(imgs).cpu()
    assert lv.shape == (3, 37, 1, 26)
    record("crnn_golden", "label_vecs max|err| vs reference", max_abs_err(lv, t(g["label_vecs"])), 1e-6)
    assert_close(lv, t(g["label_vecs"]), 1e-6, 1e-5, "native label_vecs vs the reference")


@pytest.mark.parametrize("hw", [(16, 64), (32, 128)])
def test_native_vs_mirror_logits_and_strings_b48(dev, hw):
    ref, nat = _pair(dev)
    x = _images(48, hw[0], hw[1], 81)
    with torch.no_grad():
        lg_ref = ref(ref.parse_crnn_data(x))
    lg = nat(nat.parse_crnn_data(x.to(dev))).cpu()
    err = record("crnn_mirror", "%dx%d B=48 logits max|err|" % hw, max_abs_err(lg, lg_ref), LOGIT_TOL)
    assert err < LOGIT_TOL
    # strings: every image whose 26 arg-maxes all have a top-1 / top-2 margin far above the logits tolerance must read the same
    top = lg_ref.topk(2, -1).values
    safe = (top[..., 0] - top[..., 1] > 10 * LOGIT_TOL).all(0)          # (B,)
    assert safe.float().mean() >= 0.6, "too few images with decisive arg-maxes: %d / 48" % int(safe.sum())
    want = _ref_decode(lg_ref)
    got = nat.read(x.to(dev))
    assert len(set(want)) >= 5 and any(want), "the synthetic recogniser reads too few distinct strings"
    for i in range(48):
        if safe[i]:
            assert got[i] == want[i], "image %d: %r vs %r" % (i, got[i], want[i])
    agree = sum(g_ == w_ for g_, w_ in zip(got, want))
    record("crnn_mirror", "%dx%d strings equal to mirror + reference decode" % hw, agree / 48.0)
    # the decode of the native logits themselves: bitwise the same rule
    assert _ref_decode(lg) == got


def test_batch48_equals_three_batch16(dev):
    ref, nat = _pair(dev)
    x = _images(48, 32, 128, 83).to(dev)
    full_rows, B, T = nat.logits_rows(nat.prep(x))
    parts = [nat.logits_rows(nat.prep(x[i * 16:(i + 1) * 16]))[0] for i in range(3)]
    err = max_abs_err(full_rows, torch.cat(parts))
    record("crnn_batch", "B=48 vs 3 x B=16 logits max|err|", err, 1e-6)
    assert err <= 1e-6
    assert nat.read(x) == sum((nat.read(x[i * 16:(i + 1) * 16]) for i in range(3)), [])
