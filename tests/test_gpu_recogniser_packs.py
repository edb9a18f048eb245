"""The weight packs of the native recognisers (model/native.py PackedEval): one read() fetches them once and hands them down to its
stages, and the cache behind them still follows the parameters."""
import pytest
import torch

from dpmn_amd.utils import aster_synth, moran_synth, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _crnn(dev):
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    nat = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    nat.load_state_dict(sd)
    return nat, synth.uniform("recogniser_packs", (2, 3, 32, 128), 0, 1, 1).to(dev)


def _aster(dev):
    from dpmn_amd.model.aster import ASTER, NativeASTER
    nat = NativeASTER().to(dev).eval()
    nat.load_state_dict(aster_synth.aster_fill_(ASTER().state_dict(), 81))
    return nat, aster_synth.aster_images(2).to(dev)


def _moran(dev):
    from dpmn_amd.model.moran import MORAN, NativeMORAN
    nat = NativeMORAN().to(dev).eval()
    nat.load_state_dict(moran_synth.moran_fill_(MORAN().state_dict(), 91))
    return nat, moran_synth.moran_images(2).to(dev)


@pytest.mark.parametrize("make", [_crnn, _aster, _moran], ids=["crnn", "aster", "moran"])
def test_read_fetches_the_packs_once(dev, make):
    nat, img = make(dev)
    fetch, calls = nat._packs, []

    def counted():
        calls.append(1)
        return fetch()

    nat._packs = counted
    strings = nat.read(img)
    assert len(strings) == 2 and all(isinstance(s, str) for s in strings)
    assert len(calls) == 1


def test_crnn_cache_follows_the_parameters(dev):
    nat, img = _crnn(dev)
    nat.read(img)
    P0 = nat._packs()
    assert nat._packs() is P0
    x4 = nat.prep(img)
    before = nat.logits_rows(x4)[0].clone()
    with torch.no_grad():
        nat.rnn[1].embedding.bias.add_(1.0)
    after = nat.logits_rows(x4)[0]
    # fp32 rounding of logits of order 10 is 1e-6; the step is 1.0
    err = (after[:, :37] - before[:, :37] - 1.0).abs().max().item()
    print("crnn logits step after bias += 1: max|diff - 1| %.3e" % err)
    assert err <= 1e-5
    P1 = nat._packs()
    assert P1 is not P0
    assert nat._packs() is P1
