"""Lexicon-constrained reading on the GPU (csrc/lexicon.hip): dpmn_ctc_lexicon_f32 and dpmn_edit_lexicon_i32 against the NumPy
restatement (utils/lexicon.py; inputs and references from tests/lexicon_cases.py), then end to end: TextSR.test(lexicon=...),
NativeCRNN.read_lexicon, main.py --rec_lexicon with --test and --demo_dir."""
import csv
import os

import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import lexicon as lx
from helpers import record
import lexicon_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(cases.CTC_CASES))
def test_ctc_lexicon_equals_restatement(dev, name):
    """Score: within 4 max(e_ref, T 2^-24 max|score|) of the restatement's score of the word the kernel chose, e_ref = the error of
    torch's fp32 CPU ctc_loss on the same inputs (the factor 4: the kernel's softmax and log-sum-exp order differ from torch's).
    Index: the restatement's wherever its top-2 margin exceeds twice that bound; at most 10 % of the images may be undecided."""
    from dpmn_amd import ops
    c = cases.ctc_case(name)
    B, T, L, C, ld = c["B"], c["T"], c["L"], c["n_class"], c["ld"]
    lex = ops.Lexicon(c["words"], alphabet=c["alphabet"])
    assert np.array_equal(lex.packed, c["packed"])
    rows = torch.from_numpy(c["logits"].reshape(B * T, ld)).to(dev)
    if ld > C:
        assert float(rows[:, C:].min()) == 1e4                   # the padding columns: they must not matter
    buf = ops.ctc_lexicon(rows, B, T, C, lex)
    h = buf.cpu().numpy()
    idx, logp = h[:B].astype(np.int64), h[B:].view(np.float32).astype(np.float64)
    if not np.isfinite(c["ref"]).any():
        assert idx.tolist() == [-1] * B and np.all(logp == -np.inf)
        return
    assert np.all(idx >= 0) and np.all(idx < L)
    err = float(np.abs(logp - c["ref"][np.arange(B), idx]).max())
    print("ctc_lexicon %s: score error %.3e, bound %.3e (e_ref %.3e), least margin %.3g" % (name, err, c["bound"], c["e_ref"], c["margin"].min()))
    record("ctc_lexicon", "%s max |logp - float64|" % name, err, c["bound"])
    assert err <= c["bound"]
    decided = c["margin"] > 2 * c["bound"]
    assert (~decided).mean() <= 0.10
    assert np.array_equal(idx[decided], c["idx"][decided])
    # the same call again, and behind a larger batch's workspace: the same answer
    assert torch.equal(ops.ctc_lexicon(rows, B, T, C, lex), buf)


def test_ctc_lexicon_refuses_what_it_was_not_built_for(dev):
    from dpmn_amd import _abi, ops
    lex = ops.Lexicon(["ab", "c"])
    with pytest.raises(_abi.DpmnError, match="64"):
        ops.ctc_lexicon(torch.zeros(65, 40, device=dev), 1, 65, 37, lex)
    with pytest.raises(_abi.DpmnError, match="64"):
        ops.ctc_lexicon(torch.zeros(4, 72, device=dev), 1, 4, 65, lex)
    with pytest.raises(_abi.DpmnError, match="classes"):
        ops.ctc_lexicon(torch.zeros(4, 8, device=dev), 1, 4, 8, lex)          # 'c' is class 13
    with pytest.raises(_abi.DpmnError):
        ops.edit_lexicon(torch.zeros(2, 32, dtype=torch.uint8), lex)             # a CPU tensor
    with pytest.raises(ValueError):
        ops.Lexicon(["a" * 32])


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("L", [1, 257, 1000])
def test_edit_lexicon_equals_restatement(dev, B, L):
    from dpmn_amd import ops
    e = cases.edit_case(B, L)
    lex = ops.Lexicon(e["words"], alphabet=cases.EDIT_ALPHABET)
    h = ops.edit_lexicon(torch.from_numpy(e["sp"]).to(dev), lex).cpu().numpy()
    assert h[:B].tolist() == e["idx"].tolist() and h[B:].tolist() == e["dist"].tolist()
    words, dist = ops.edit_read(e["strings"], lex, dev)
    assert words == [e["words"][i] for i in e["idx"]] and dist == e["dist"].tolist()


# ------------------------------------------------------------------------------------------------------------------ end to end
def _mirror_logits(sd, images):
    from dpmn_amd.model.crnn import CRNN
    m = CRNN(32, 1, 37, 256).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        return m(m.parse_crnn_data(images.float())).permute(1, 0, 2).double().numpy()       # (B, T, 37)


# A word's score is a sum over T = 26 frames of log-softmax terms, and a log-softmax term moves by at most 2 d when the logits move by
# d: native and mirror logits within 1e-3 of each other (the class of the CRNN parity tests) move a top-2 margin by less than
# 2 * 26 * 2e-3 ~ 0.1 nats.  Images with a smaller margin carry no label.
MARGIN = 0.1
LEXICON = ["shop", "exit", "open", "a", "7", "zz", "street", "number42", "aa", "o0o", "mi355x", "text", "b", "77", "e"]


def test_test_mode_lexicon_accuracy_equals_restatement(dev, tmp_path):
    from dpmn_amd import ops, workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from test_gpu_crnn_eval import _checkpoints, _crnn_sd, _mirror_read
    import types
    sr, models, psn, inp = workload.build("cfg0", batch=8)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    sd = _crnn_sd()
    torch.save(sd, os.path.join(d, "crnn.pth"))
    args = workload.make_args("tsrn", 1, 1, 8)
    args.resume = d
    sr2 = TextSR(workload.make_config(8), args)
    rec = sr2.CRNN_init(os.path.join(d, "crnn.pth"))
    lex = ops.Lexicon(LEXICON)
    got = {}
    orig = sr2.refine
    sr2.refine = types.MethodType(lambda self, *a, **kw: got.setdefault("out", orig(*a, **kw)), sr2)
    res0 = sr2.test([(inp["images_hr"], inp["images_lr"], None)], rec=rec, lexicon=lex)
    assert res0["accuracy"] is None and res0["accuracy_lexicon"] is None          # no label strings: not computed
    sr_img = got["out"][:, :3]
    # the mirror's logits of those SR images -> the restatement's word per image; a label is that word where the choice is decisive
    scores = lx.ctc_word_logp(_mirror_logits(sd, sr_img.cpu()), lex.packed)
    idx, best = lx.best_of_scores(scores)
    top = np.sort(scores, 1)[:, ::-1]
    margin = top[:, 0] - top[:, 1]
    n = len(idx)
    labels = [LEXICON[idx[i]].upper() if (i % 2 == 0 and margin[i] > MARGIN) else "zz9zz%d" % i for i in range(n)]
    n_right = sum(1 for i in range(n) if not labels[i].startswith("zz9zz"))
    assert 0 < n_right < n, "no usable image: margins %s" % margin.tolist()
    loader = [(inp["images_hr"], inp["images_lr"], None, labels)]
    before = rec.read(sr_img)
    res = sr2.test(loader, rec=rec, lexicon=lex)
    plain = sr2.test(loader, rec=rec)
    record("lexicon_eval", "test() accuracy_lexicon (expected %.4f)" % round(n_right / n, 4), res["accuracy_lexicon"])
    assert res["accuracy_lexicon"] == round(n_right / n, 4)
    assert "accuracy_lexicon" not in plain and res["accuracy"] == plain["accuracy"]
    assert sorted(res) == sorted(list(plain) + ["accuracy_lexicon"])
    # read_lexicon: the greedy strings are read()'s, the words and scores the restatement's; read() is what it was afterwards
    greedy, words, logp = rec.read_lexicon(sr_img, lex)
    assert greedy == before == rec.read(sr_img)
    decided = margin > MARGIN
    assert [w for w, ok in zip(words, decided) if ok] == [LEXICON[i] for i, ok in zip(idx, decided) if ok]
    assert all(np.isfinite(logp)) and max(logp) < 0
    # the edit protocol through a plain callable and through the CRNN in mode 'edit'
    fixed = ["shap", "", "street5", "q", "numbr42", "77", "o00", "xit"][:n]
    exp_i, exp_d = lx.edit_lexicon_best(lx.pack_strings(fixed), lex.packed)
    lab = [LEXICON[i] for i in exp_i[:4]] + ["zz9zz"] * (n - 4)
    res_e = sr2.test([(inp["images_hr"], inp["images_lr"], None, lab)], rec=lambda x: fixed[:x.shape[0]], lexicon=ops.Lexicon(LEXICON, mode="edit"))
    assert res_e["accuracy_lexicon"] == round(4 / n, 4)
    g2, w2, d2 = rec.read_lexicon(sr_img, ops.Lexicon(LEXICON, mode="edit"))
    ei, ed = lx.edit_lexicon_best(lx.pack_strings(g2), lex.packed)
    assert g2 == before and w2 == [LEXICON[i] for i in ei] and d2 == ed.tolist()


def test_main_rec_lexicon_writes_the_extra_columns(dev, tmp_path, capsys):
    import main as cli
    from dpmn_amd import workload
    from test_gpu_crnn_eval import _checkpoints, _crnn_sd
    sr, models, psn, inp = workload.build("cfg0", batch=4)
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    torch.save(_crnn_sd(), os.path.join(d, "crnn.pth"))
    words = os.path.join(d, "words.txt")
    with open(words, "w", encoding="utf-8") as f:
        f.write("\n".join(LEXICON + ["SHOP"]) + "\n")
    src = os.path.join(d, "in")
    os.makedirs(src)
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (16 + 5 * i, 60 + 9 * i, 3)).astype(np.uint8)).save(os.path.join(src, "im%d.png" % i))

    def run(tag, **kw):
        args = workload.make_args("tsrn", 1, 1, 4)
        args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, False, None, 2, "crnn"
        args.vis_dir = os.path.join(d, "vis_" + tag)
        for k, v in kw.items():
            setattr(args, k, v)
        ckpt = os.path.join(d, "out_" + tag)
        config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(4).TRAIN), ckpt_dir=ckpt, VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
        cli.main(config, args)
        return ckpt

    ckpt = run("t_lex", test=True, rec_lexicon=words)
    rows = list(csv.reader(open(os.path.join(ckpt, "test_result.csv"))))
    assert rows[0] == ["recognizer", "subset", "accuracy", "psnr", "ssim", "accuracy_lexicon"]
    assert len(rows[1]) == 6 and 0.0 <= float(rows[1][5]) <= 1.0 and 0.0 <= float(rows[1][2]) <= 1.0
    assert "rec_lexicon: %d words, mode score" % len(LEXICON) in capsys.readouterr().out
    ckpt0 = run("t_plain", test=True)
    rows0 = list(csv.reader(open(os.path.join(ckpt0, "test_result.csv"))))
    assert rows0[0] == ["recognizer", "subset", "accuracy", "psnr", "ssim"] and rows0[1][:5] == rows[1][:5]
    for tag, mode in (("d_lex", None), ("d_edit", "edit")):
        out = os.path.join(d, "demo_" + tag)
        run(tag, demo_dir=src, demo_out=out, rec_lexicon=words, rec_lexicon_mode=mode)
        drows = list(csv.reader(open(os.path.join(out, "demo_result.csv"), newline="")))
        assert drows[0] == ["file", "lr_string", "sr_string", "sr_lexicon", "sr_lexicon_score"] and len(drows) == 4
        for r in drows[1:]:
            assert r[3] in LEXICON
            if mode == "edit":
                assert int(r[4]) == lx.edit_distances(lx.pack_strings([r[2]]), lx.pack_lexicon([r[3]]))[0, 0]
            else:
                assert float(r[4]) < 0
    out = os.path.join(d, "demo_plain")
    run("d_plain", demo_dir=src, demo_out=out)
    assert list(csv.reader(open(os.path.join(out, "demo_result.csv"), newline="")))[0] == ["file", "lr_string", "sr_string"]
    with pytest.raises(SystemExit, match="--demo_tile"):
        run("d_tile", demo_dir=src, demo_tile=True, rec_lexicon=words)
    with pytest.raises(SystemExit, match="needs a recogniser"):
        run("t_norec", test=True, rec="aster", rec_lexicon=words)
