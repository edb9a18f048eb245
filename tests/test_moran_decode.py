"""Host side of the MORAN recogniser (no GPU): the stock-operator mirror `MORAN` against the imported reference
(tests/golden/moran.npz, tools/gen_golden.py gen_moran) -- state_dict layout (427 keys), every stage within 1e-4, ids and strings
exactly -- the label converter against the reference's (tests/golden/moran_labels.npz), the trainer surface."""
import inspect
import types

import numpy as np
import pytest
import torch

from helpers import checksum, load_golden, t

MARGIN = 1e-3


@pytest.fixture(scope="module")
def env():
    from dpmn_amd.model.moran import MORAN
    from dpmn_amd.utils import moran_synth
    z = load_golden("moran")
    m = MORAN(1, 37, 256, 32, 100, BidirDecoder=True).eval()
    sd = m.state_dict()
    moran_synth.moran_fill_(sd, 91)
    m.load_state_dict(sd)
    img = moran_synth.moran_images(z["ids"].tolist())
    return {"z": z, "m": m, "sd": sd, "img": img, "st": m.stages(img)}


def test_mirror_loads_reference_layout(env):
    z, m, sd = env["z"], env["m"], env["sd"]
    rows = [r.split("|") for r in z["manifest"].tolist()]
    assert len(rows) == 427 and [r[0] for r in rows] == list(sd.keys())
    for name, shape, dtype in rows:
        assert tuple(sd[name].shape) == (tuple(int(s) for s in shape.split(",")) if shape else ()), name
        assert str(sd[name].dtype).replace("torch.", "") == dtype, name
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - 20.34) < 0.01
    assert abs(checksum(sd) - float(z["checksum"])) <= 1e-6 * abs(float(z["checksum"]))
    assert torch.equal(env["img"], t(z["images"]).float()), "the fixture's images are not the seeded pool's"
    assert "MORN.grid" not in sd and m.MORN.grid.shape == (1, 32, 100, 2)


def test_fixture_is_not_degenerate(env):
    z = env["z"]
    ids, strings = z["pred_ids"], z["strings"].tolist()
    assert ids.shape == (8, 20) and len(set(strings)) >= 4
    assert any((r == 36).any() for r in ids) and any(not (r == 36).any() for r in ids)
    assert float(z["margin"].min()) >= MARGIN
    assert float(np.abs(z["offsets2"]).max()) >= 0.05


@pytest.mark.parametrize("stage,sub", [("prep", None), ("offsets1", None), ("offsets2", None), ("rectified", None),
                                       ("resnet", (slice(None), slice(None, None, 4))), ("rnn", (slice(None), slice(None), slice(None, None, 2))),
                                       ("i2h", (slice(None), slice(None), slice(None, None, 2))), ("logits", None)])
def test_mirror_stage_equals_reference(env, stage, sub):
    got = env["st"][stage]
    got = got if sub is None else got[sub]
    ref = t(env["z"][stage])
    assert got.shape == ref.shape, "%s: %s vs %s" % (stage, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max())
    print("%s: max abs err %.3e (ref max %.3f)" % (stage, err, float(ref.abs().max())))
    assert err <= 1e-4, "%s: max abs err %.3e" % (stage, err)


def test_mirror_ids_and_strings_equal_reference(env):
    z, m = env["z"], env["m"]
    assert np.array_equal(env["st"]["ids"].numpy(), z["pred_ids"].astype(np.int64))
    assert m.read(env["img"]) == z["strings"].tolist()
    gray, length, text, _ = _fake_base().parse_moran_data(env["img"])
    (rows, r2l), demo = m(gray, length, text, text, test=True, debug=True)
    assert r2l is None and demo is None and rows.shape == (160, 37)
    assert float((rows.view(8, 20, 37) - t(z["logits"])).abs().max()) <= 1e-4
    with pytest.raises(RuntimeError, match="test=True"):
        m(gray, length, text, text, test=False)


def test_label_converter_equals_reference():
    from dpmn_amd.utils.labelmaps import MORAN_ALPHABET, MoranLabelConverter, moran_strings
    z = load_golden("moran_labels")
    conv = MoranLabelConverter()
    assert conv.alphabet == z["alphabet"].tolist() == list(MORAN_ALPHABET) and len(conv.alphabet) == 37
    ids = z["ids"].astype(np.int64)
    assert ids[0, 0] == 36 and ids[1, 19] == 36 and not (ids[2] == 36).any()
    assert conv.decode(torch.from_numpy(ids).reshape(-1), torch.IntTensor([20] * len(ids))) == z["texts"].tolist()
    assert conv.decode(ids[3], torch.IntTensor([20])) == str(z["single"])
    assert moran_strings(ids) == z["cut"].tolist() and moran_strings(ids)[0] == ""
    text, length = conv.encode(['0' * 20] * 3)
    assert text.dtype == torch.int64 and text.tolist() == [0] * 60 and length.tolist() == [20] * 3
    assert conv.encode("aZ$")[0].tolist() == [10, 35, 36]
    with pytest.raises(AssertionError):
        conv.decode(ids[0], torch.IntTensor([19]))


def _fake_base():
    from dpmn_amd.interfaces.base import TextBase
    from dpmn_amd.utils.labelmaps import MoranLabelConverter
    fake = types.SimpleNamespace(config=types.SimpleNamespace(TRAIN=types.SimpleNamespace(VAL=types.SimpleNamespace(moran_pretrained=''))),
                                 device=torch.device("cpu"), converter_moran=MoranLabelConverter())
    fake.parse_moran_data = types.MethodType(TextBase.parse_moran_data, fake)
    fake.MORAN_init = types.MethodType(TextBase.MORAN_init, fake)
    return fake


def test_trainer_surface(env):
    from dpmn_amd.interfaces.base import TextBase
    for name, params in (("MORAN_init", ["self", "path"]), ("parse_moran_data", ["self", "imgs_input"])):
        assert list(inspect.signature(getattr(TextBase, name)).parameters) == params
    assert inspect.signature(TextBase.MORAN_init).parameters["path"].default is None
    fake = _fake_base()
    for path in (None, "", "/nonexistent/moran.pth"):
        with pytest.raises(FileNotFoundError, match="MORAN"):
            fake.MORAN_init(path)
    tensor, length, text, text_rev = fake.parse_moran_data(env["img"][:3])
    assert tensor.shape == (3, 1, 32, 100) and float((tensor - t(env["z"]["prep"][:3])).abs().max()) <= 1e-4
    assert length.dtype == torch.int32 and length.tolist() == [20] * 3
    assert text.dtype == torch.int64 and text.tolist() == [0] * 60 and text_rev is text


def test_native_rejects_other_configurations():
    from dpmn_amd.model.moran import NativeMORAN
    for args in ((3, 37, 256, 32, 100, True), (1, 38, 256, 32, 100, True), (1, 37, 128, 32, 100, True), (1, 37, 256, 32, 100, False)):
        with pytest.raises(NotImplementedError, match=r"MORAN\(1, 37, 256, 32, 100, BidirDecoder=True\)"):
            NativeMORAN(*args)
    assert len(NativeMORAN().state_dict()) == 427
