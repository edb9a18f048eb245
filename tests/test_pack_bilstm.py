"""packing.pack_bilstm against nn.LSTM on the CPU in float64: the gate order, the direction layout and the folded biases that
NativeCRNN, NativeASTER and NativeMORAN share, for both state-dict prefix forms and for the second layer of a stacked LSTM."""
import pytest
import torch
import torch.nn as nn

from dpmn_amd.model import packing

T, B, H = 3, 2, 4
TOL = 1e-12         # float64 (eps 2.2e-16), sums of at most 12 terms of order 1


def _recurrence(gx, w_hh):
    """What ops.bilstm documents, in plain torch: gx (B*T, 8H) with row b*T + t and columns [forward i f g o | backward i f g o],
    w_hh (2, 4H, H) -> (B*T, 2H) = [h_fwd | h_bwd]; the backward direction reads t = T-1..0."""
    gx = gx.view(B, T, 2, 4 * H)
    out = gx.new_zeros(B, T, 2, H)
    for d in range(2):
        h, c = gx.new_zeros(B, H), gx.new_zeros(B, H)
        for t in (range(T) if d == 0 else reversed(range(T))):
            i, f, g, o = (gx[:, t, d] + h @ w_hh[d].t()).split(H, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[:, t, d] = h
    return out.reshape(B * T, 2 * H)


def _lstm(n_in, layers, seed):
    torch.manual_seed(seed)
    m = nn.LSTM(n_in, H, num_layers=layers, bidirectional=True).double()
    for p in m.parameters():
        nn.init.uniform_(p, -1.0, 1.0)
    return m


def _through(sd, prefix, layer, x_rows):
    w_ih, b, w_hh = packing.pack_bilstm(sd, prefix, layer)
    n_in = x_rows.shape[1]
    assert w_ih.shape == (8 * H, n_in) and b.shape == (8 * H,) and w_hh.shape == (2, 4 * H, H)
    assert w_ih.is_contiguous() and b.is_contiguous() and w_hh.is_contiguous()
    return _recurrence(x_rows @ w_ih.t() + b, w_hh)


@pytest.mark.parametrize("prefix", ["rnn.0.rnn.", "ASRN.rnn.0.rnn."])
def test_one_layer_behind_a_module_prefix(prefix):
    m = _lstm(8, 1, 11)
    sd = {prefix + k: v.detach() for k, v in m.state_dict().items()}
    x = torch.randn(T, B, 8, dtype=torch.float64)
    ref = m(x)[0].detach().permute(1, 0, 2).reshape(B * T, 2 * H)
    err = (_through(sd, prefix, 0, x.permute(1, 0, 2).reshape(B * T, 8)) - ref).abs().max().item()
    print("pack_bilstm %s max|err| %.3e" % (prefix, err))
    assert err <= TOL


def test_both_layers_of_a_stacked_lstm():
    m = _lstm(8, 2, 12)
    sd = {"encoder.rnn." + k: v.detach() for k, v in m.state_dict().items()}
    x = torch.randn(T, B, 8, dtype=torch.float64)
    ref = m(x)[0].detach().permute(1, 0, 2).reshape(B * T, 2 * H)
    rows = x.permute(1, 0, 2).reshape(B * T, 8)
    for layer in range(2):
        rows = _through(sd, "encoder.rnn.", layer, rows)
    err = (rows - ref).abs().max().item()
    print("pack_bilstm encoder.rnn. layers 0, 1 max|err| %.3e" % err)
    assert err <= TOL
    # layer 0 alone, against the same weights as a one-layer module
    one = _lstm(8, 1, 0)
    one.load_state_dict({k: v for k, v in m.state_dict().items() if "_l0" in k})
    ref0 = one(x)[0].detach().permute(1, 0, 2).reshape(B * T, 2 * H)
    assert (_through(sd, "encoder.rnn.", 0, x.permute(1, 0, 2).reshape(B * T, 8)) - ref0).abs().max().item() <= TOL


def test_pad_rows4():
    w, b = torch.arange(37.0 * 6).view(37, 6), torch.arange(37.0)
    wp, bp = packing.pad_rows4(w, b)
    assert wp.shape == (40, 6) and bp.shape == (40,) and wp.is_contiguous() and bp.is_contiguous()
    assert torch.equal(wp[:37], w) and torch.equal(bp[:37], b) and not wp[37:].any() and not bp[37:].any()
    w4, b4 = packing.pad_rows4(w[:36], b[:36])
    assert torch.equal(w4, w[:36]) and torch.equal(b4, b[:36])
