"""Word accuracy of the SR images through TextSR.test(loader, rec=Aster_init(path)[0]) and main.py --test --rec aster with
TRAIN.VAL.rec_pretrained pointing at a saved synthetic checkpoint: the reported accuracy equals the one of the stock-operator
mirror on the same SR images (labels chosen so that it lies strictly between 0 and 1)."""
import csv
import os
import types

import pytest
import torch

from dpmn_amd.utils import aster_synth
from helpers import record
from test_gpu_crnn_eval import _checkpoints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _aster_ckpt(path):
    from dpmn_amd.model.aster import ASTER
    sd = ASTER().state_dict()
    aster_synth.aster_fill_(sd, 81)
    torch.save({"state_dict": sd}, path)
    return sd


def test_test_mode_aster_accuracy_equals_mirror(dev, tmp_path):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.model.aster import ASTER, NativeASTER
    sr, models, psn, inp = workload.build("cfg0", batch=8)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    path = os.path.join(d, "aster.pth")
    sd = _aster_ckpt(path)
    args = workload.make_args("tsrn", 1, 1, 8)
    args.resume = d
    sr2 = TextSR(workload.make_config(8), args)
    with pytest.raises(FileNotFoundError, match="ASTER"):
        sr2.Aster_init("")
    rec, info = sr2.Aster_init(path)
    assert isinstance(rec, NativeASTER) and not rec.training and not any(p.requires_grad for p in rec.parameters()) and info.rec_num_classes == 97
    got = {}
    orig = sr2.refine
    sr2.refine = types.MethodType(lambda self, *a, **kw: got.setdefault("out", orig(*a, **kw)), sr2)
    assert sr2.test([(inp["images_hr"], inp["images_lr"], None)], rec=rec)["accuracy"] is None
    mir = ASTER().to(dev).eval()
    mir.load_state_dict(sd)
    reads = mir.read(got["out"][:, :3], info)
    native = rec.read(got["out"][:, :3])
    labels = [reads[i].upper() if i % 2 == 0 else "zz9zz" + str(i) for i in range(len(reads))]
    expected = round(sum(1 for i in range(len(reads)) if native[i] == reads[i] and i % 2 == 0) / len(reads), 4)
    res = sr2.test([(inp["images_hr"], inp["images_lr"], None, labels)], rec=rec)
    record("aster_eval", "test() accuracy (mirror's readings as labels on even images: %.4f)" % (len(reads[::2]) / len(reads)), res["accuracy"])
    assert native == reads, "native and mirror readings differ: %s vs %s" % (native, reads)
    assert res["accuracy"] == expected == round(len(reads[::2]) / len(reads), 4) and 0 < res["accuracy"] < 1


def test_main_test_rec_aster_writes_numeric_accuracy(dev, tmp_path, capsys):
    import main as cli
    from dpmn_amd import workload
    sr, models, psn, inp = workload.build("cfg0", batch=4)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    _aster_ckpt(os.path.join(d, "aster.pth"))
    args = workload.make_args("tsrn", 1, 1, 4)
    args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, True, None, 2, "aster"
    ckpt = os.path.join(d, "out_aster")
    config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(4).TRAIN), ckpt_dir=ckpt, VAL={"rec_pretrained": os.path.join(d, "aster.pth")})})
    cli.main(config, args)
    rows = list(csv.reader(open(os.path.join(ckpt, "test_result.csv"))))
    assert rows[1][0] == "aster" and 0.0 <= float(rows[1][2]) <= 1.0
    assert "recogniser not built" not in capsys.readouterr().out
