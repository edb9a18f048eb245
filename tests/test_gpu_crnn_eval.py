"""Word accuracy of the SR images through TextSR.test(loader, rec=CRNN_init(path)) (super_resolution.py:453-493, --rec crnn): the
reported accuracy equals the one of the CPU mirror + the reference's greedy decode on the same SR images; main.py --test --rec crnn
writes it to test_result.csv; without a CRNN checkpoint CRNN_init raises."""
import csv
import os
import types

import pytest
import torch

from dpmn_amd.utils import synth
from helpers import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _crnn_sd():
    from dpmn_amd.model.crnn import CRNN
    sd = CRNN(32, 1, 37, 256).state_dict()
    synth.synth_fill_(sd, seed=71)
    for k, v in sd.items():             # (as tests/test_gpu_crnn.py: without the biases the readings depend on the image)
        if (k.startswith("rnn.") and "bias" in k) or (k.startswith("cnn.conv") and k.endswith(".bias")):
            v.zero_()
    return sd


def _mirror_read(sd, images):
    from dpmn_amd.model.crnn import CRNN, ALPHABET
    m = CRNN(32, 1, 37, 256).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        lg = m(m.parse_crnn_data(images.float()))
    out = []
    for row in lg.argmax(2).t().tolist():
        s, prev = [], -1
        for c in row:
            if c != 0 and c != prev:
                s.append(ALPHABET[c - 1])
            prev = c
        out.append("".join(s))
    top = lg.topk(2, -1).values
    return out, (top[..., 0] - top[..., 1]).min(0).values


def _checkpoints(d, models, psn):
    pack = lambda m: {"state_dict_G": {k: v.detach().clone() for k, v in m.state_dict().items()}}
    torch.save(pack(psn), os.path.join(d, "model_tsrn.pth"))
    for k, m in enumerate(models[:-1]):
        torch.save(pack(m), os.path.join(d, "model_best_%d.pth" % k))
    torch.save(pack(models[-1]), os.path.join(d, "model_best_cmm.pth"))


def test_test_mode_crnn_accuracy_equals_mirror(dev, tmp_path):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.model.crnn import NativeCRNN
    sr, models, psn, inp = workload.build("cfg0", batch=8)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    crnn_path = os.path.join(d, "crnn.pth")
    sd = _crnn_sd()
    torch.save(sd, crnn_path)
    args = workload.make_args("tsrn", 1, 1, 8)
    args.resume = d
    sr2 = TextSR(workload.make_config(8), args)
    with pytest.raises(FileNotFoundError, match="CRNN"):
        sr2.CRNN_init("")
    with pytest.raises(FileNotFoundError, match="CRNN"):
        sr2.CRNN_init()                 # no TRAIN.VAL.crnn_pretrained in this config
    rec = sr2.CRNN_init(crnn_path)
    assert isinstance(rec, NativeCRNN) and not rec.training and not any(p.requires_grad for p in rec.parameters())
    # the SR images test() will produce (the same checkpoints, the same priors): read them with the mirror to build the labels
    got = {}
    orig = sr2.refine
    sr2.refine = types.MethodType(lambda self, *a, **kw: got.setdefault("out", orig(*a, **kw)), sr2)
    loader0 = [(inp["images_hr"], inp["images_lr"], None)]
    assert sr2.test(loader0, rec=rec)["accuracy"] is None        # no label strings: not computed
    sr_img = got["out"][:, :3].cpu()
    reads, margin = _mirror_read(sd, sr_img)
    # labels: the mirror's reading upper-cased (str_filt lowers it) for the images whose arg-maxes are all decisive, even indices
    # only; a string no image reads for the rest
    labels = [reads[i].upper() if (i % 2 == 0 and margin[i] > 1e-4) else "zz9zz" + str(i) for i in range(len(reads))]
    n_right = sum(1 for i in range(len(reads)) if labels[i] != "zz9zz" + str(i))
    assert 0 < n_right < len(reads), "no usable image: margins %s" % margin.tolist()
    expected = round(n_right / len(reads), 4)
    loader = [(inp["images_hr"], inp["images_lr"], None, labels)]
    res = sr2.test(loader, rec=rec)
    record("crnn_eval", "test() accuracy (expected %.4f)" % expected, res["accuracy"])
    assert res["accuracy"] == expected and 0 < res["accuracy"] < 1


def test_main_test_rec_crnn_writes_numeric_accuracy(dev, tmp_path, capsys):
    import main as cli
    from dpmn_amd import workload
    sr, models, psn, inp = workload.build("cfg0", batch=4)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    torch.save(_crnn_sd(), os.path.join(d, "crnn.pth"))
    for rec_name in ("crnn", "aster"):
        args = workload.make_args("tsrn", 1, 1, 4)
        args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, True, None, 2, rec_name
        ckpt = os.path.join(d, "out_" + rec_name)
        config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(4).TRAIN), ckpt_dir=ckpt,
                                             VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
        cli.main(config, args)
        rows = list(csv.reader(open(os.path.join(ckpt, "test_result.csv"))))
        assert rows[0] == ["recognizer", "subset", "accuracy", "psnr", "ssim"] and rows[1][0] == rec_name
        if rec_name == "crnn":
            assert 0.0 <= float(rows[1][2]) <= 1.0
        else:
            assert rows[1][2] == ""       # None: not computed
    assert "--rec aster: recogniser not built" in capsys.readouterr().out
