"""Word accuracy of the SR images through TextSR.test(loader, rec=MORAN_init(path)) and main.py --test --rec moran with
TRAIN.VAL.moran_pretrained pointing at a saved synthetic checkpoint: the reported accuracy equals the one of the stock-operator
mirror on the same SR images (labels chosen so that it lies strictly between 0 and 1); without moran_pretrained no recogniser is
built and the accuracy stays empty."""
import csv
import os
import types

import pytest
import torch

from dpmn_amd.utils import moran_synth
from helpers import record
from test_gpu_crnn_eval import _checkpoints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _moran_ckpt(path, prefix=""):
    from dpmn_amd.model.moran import MORAN
    sd = MORAN().state_dict()
    moran_synth.moran_fill_(sd, 91)
    torch.save({prefix + k: v for k, v in sd.items()}, path)
    return sd


def test_test_mode_moran_accuracy_equals_mirror(dev, tmp_path):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.model.moran import MORAN, NativeMORAN
    sr, models, psn, inp = workload.build("cfg0", batch=8)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    path = os.path.join(d, "moran.pth")
    sd = _moran_ckpt(path, prefix="module.")            # a DataParallel checkpoint: MORAN_init strips the prefix
    args = workload.make_args("tsrn", 1, 1, 8)
    args.resume = d
    sr2 = TextSR(workload.make_config(8), args)
    with pytest.raises(FileNotFoundError, match="MORAN"):
        sr2.MORAN_init("")
    rec = sr2.MORAN_init(path)
    assert isinstance(rec, NativeMORAN) and not rec.training and not any(p.requires_grad for p in rec.parameters())
    got = {}
    orig = sr2.refine
    sr2.refine = types.MethodType(lambda self, *a, **kw: got.setdefault("out", orig(*a, **kw)), sr2)
    assert sr2.test([(inp["images_hr"], inp["images_lr"], None)], rec=rec)["accuracy"] is None
    mir = MORAN().to(dev).eval()
    mir.load_state_dict(sd)
    reads = mir.read(got["out"][:, :3])
    native = rec.read(got["out"][:, :3])
    tensor, length, text, _ = sr2.parse_moran_data(got["out"][:, :3])
    assert float((tensor - mir.parse_moran_data(got["out"][:, :3])).abs().max()) <= 1e-4 and length.tolist() == [20] * 8 and text.numel() == 160
    labels = [reads[i].upper() if i % 2 == 0 else "zz9zz" + str(i) for i in range(len(reads))]
    expected = round(sum(1 for i in range(len(reads)) if native[i] == reads[i] and i % 2 == 0) / len(reads), 4)
    res = sr2.test([(inp["images_hr"], inp["images_lr"], None, labels)], rec=rec)
    record("moran_eval", "test() accuracy (mirror's readings as labels on even images: %.4f)" % (len(reads[::2]) / len(reads)), res["accuracy"])
    assert native == reads, "native and mirror readings differ: %s vs %s" % (native, reads)
    assert res["accuracy"] == expected == round(len(reads[::2]) / len(reads), 4) and 0 < res["accuracy"] < 1


def _run_main(tmp_path, val):
    import main as cli
    from dpmn_amd import workload
    sr, models, psn, inp = workload.build("cfg0", batch=4)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    _moran_ckpt(os.path.join(d, "moran.pth"))
    args = workload.make_args("tsrn", 1, 1, 4)
    args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, True, None, 2, "moran"
    ckpt = os.path.join(d, "out_moran")
    cfg = dict(vars(workload.make_config(4).TRAIN), ckpt_dir=ckpt)
    if val:
        cfg["VAL"] = {"moran_pretrained": os.path.join(d, "moran.pth")}
    cli.main(cli.AttrDict({"TRAIN": cfg}), args)
    return list(csv.reader(open(os.path.join(ckpt, "test_result.csv"))))


def test_main_test_rec_moran_writes_numeric_accuracy(dev, tmp_path, capsys):
    rows = _run_main(tmp_path, True)
    assert rows[1][0] == "moran" and 0.0 <= float(rows[1][2]) <= 1.0
    assert "recogniser not built" not in capsys.readouterr().out


def test_main_test_rec_moran_without_weights_builds_no_recogniser(dev, tmp_path, capsys):
    rows = _run_main(tmp_path, False)
    assert rows[1][0] == "moran" and rows[1][2] == ""       # None: not computed
    assert "--rec moran: recogniser not built" in capsys.readouterr().out
