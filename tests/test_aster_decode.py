"""Host side of the ASTER recogniser (no GPU): vocabulary and AsterInfo, ids -> strings (get_str_list's prediction half), the numpy
backtracking of the beam search against the reference's on hand-made stored tensors (tests/golden/aster_beam.npz), the mirror's
state_dict layout (tests/golden/aster.npz manifest, 384 keys), the trainer surface."""
import inspect
import types

import numpy as np
import pytest
import torch

from helpers import load_golden


def test_vocabulary_and_info_equal_reference():
    from dpmn_amd.utils.labelmaps import AsterInfo, get_vocabulary
    z = load_golden("aster_beam")
    for i, v in enumerate(('digit', 'lower', 'upper', 'all')):
        assert get_vocabulary(v) == z["voc_" + v].tolist()
        info = AsterInfo(v)
        assert info.rec_num_classes == int(z["rec_num_classes"][i]) == len(info.voc)
        assert info.char2id[info.EOS] == len(info.voc) - 3 and info.id2char[len(info.voc) - 1] == 'UNKNOWN' and info.max_len == 100
    assert AsterInfo('all').rec_num_classes == 97 and AsterInfo('all').char2id['EOS'] == 94
    assert load_golden("aster")["vocabulary"].tolist() == AsterInfo('all').voc
    with pytest.raises(AssertionError):
        AsterInfo('nope')


def test_ids_to_strings_equal_get_str_list():
    from dpmn_amd.utils.labelmaps import AsterInfo, ids_to_strings
    z, info = load_golden("aster_beam"), AsterInfo('all')
    assert ids_to_strings(z["ids"], info) == z["id_strings"].tolist()
    assert ids_to_strings(z["pred_rec"], info) == z["strings"].tolist()
    a = load_golden("aster")
    assert ids_to_strings(a["pred_rec"], info) == a["strings"].tolist()


def test_backtracking_equals_reference():
    from dpmn_amd.utils.labelmaps import beam_backtrack
    z = load_golden("aster_beam")
    sym, pred, score = z["symbols"], z["predecessors"], z["scores"]
    B = sym.shape[1] // 5
    assert (sym[0, :5] == 94).any() and not (sym[:, 10:15] == 94).any()            # EOS at step 0 / never
    assert len(set(score[3, 15:20].tolist())) < 5 and (sym[3, 15:20] == 94).sum() >= 2      # equal scores, several beams end together
    got = beam_backtrack(sym, pred, score, B, 5, 94)
    assert got.shape == (B, 100) and np.array_equal(got, z["pred_rec"].astype(np.int64))
    a = load_golden("aster")
    got = beam_backtrack(a["symbols"], a["predecessors"], a["scores"], len(a["margin"]), 5, 94)
    assert np.array_equal(got, a["pred_rec"].astype(np.int64))


def test_fixture_is_not_degenerate():
    a = load_golden("aster")
    n = len(a["margin"])
    assert int((a["margin"] < 1e-3).sum()) * 4 <= n and len(set(a["strings"].tolist())) >= 3
    first = [int(np.argmax(r == 94)) if (r == 94).any() else -1 for r in a["pred_rec"]]
    assert sum(1 for e in first if 1 <= e <= 30) * 2 >= n


def test_mirror_loads_reference_layout():
    from dpmn_amd.model.aster import ASTER
    from dpmn_amd.utils import aster_synth
    from helpers import checksum
    z = load_golden("aster")
    m = ASTER().eval()
    sd = m.state_dict()
    rows = [r.split("|") for r in z["manifest"].tolist()]
    assert len(rows) == 384 and [r[0] for r in rows] == list(sd.keys())
    for name, shape, dtype in rows:
        assert tuple(sd[name].shape) == (tuple(int(s) for s in shape.split(",")) if shape else ()), name
        assert str(sd[name].dtype).replace("torch.", "") == dtype, name
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - 20.99) < 0.01
    aster_synth.aster_fill_(sd, 81)
    assert abs(checksum(sd) - float(z["checksum"])) <= 1e-6 * abs(float(z["checksum"]))
    m.load_state_dict(sd)
    st = m.stages(aster_synth.aster_images(z["ids"].tolist()[:2]))
    assert st["encoder"].shape == (2, 25, 512) and st["rectified"].shape == (2, 3, 32, 100)
    assert float((st["ctrl"] - torch.from_numpy(z["ctrl"][:2])).abs().max()) < 1e-4


def test_trainer_surface():
    from dpmn_amd.interfaces.base import TextBase
    for name, params in (("Aster_init", ["self", "path"]), ("parse_aster_data", ["self", "imgs_input"])):
        assert list(inspect.signature(getattr(TextBase, name)).parameters) == params
    assert inspect.signature(TextBase.Aster_init).parameters["path"].default is None
    fake = types.SimpleNamespace(config=types.SimpleNamespace(TRAIN=types.SimpleNamespace(VAL=types.SimpleNamespace(rec_pretrained=''), voc_type='all')),
                                 device=torch.device("cpu"))
    for path in (None, "", "/nonexistent/aster.pth"):
        with pytest.raises(FileNotFoundError, match="ASTER"):
            TextBase.Aster_init(fake, path)
    d = TextBase.parse_aster_data(fake, torch.full((3, 3, 32, 128), 0.25))
    assert float(d['images'].min()) == float(d['images'].max()) == -0.5
    assert d['rec_targets'].shape == (3, 100) and d['rec_targets'].dtype == torch.int32 and int(d['rec_targets'].min()) == 1 and d['rec_lengths'] == [100] * 3
