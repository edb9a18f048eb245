"""GPU tests of the CTC beam search with a character model (ours; main.py --rec_beam / --rec_lm): dpmn_ctc_beam_f64 against the
definition (utils/beam.py) on the inputs of tests/beam_cases.py, NativeCRNN.read_beam, the refusals, the model's upload cache, then
main.py and TextSR.eval.

The comparison with the definition.  Kernel and definition do the same float64 operations in the same order, but the device's exp and
log are not the host's, so their rank scores differ by rounding and a choice between two candidates closer than that may fall either
way.  The definition reports its own `margin` (the smallest gap it ever decided on); the tests' threshold is
    tau = 64 eps T (n_class + 2) S,   S = max(1, T max|lp| + |lm|),   eps = 2^-52:
a rank score ends a chain of at most T frames; a frame adds the row's log-sum-exp over n_class terms and the two lse of a member, so
at most n_class + 2 rounded operations, each good to one eps relative to a magnitude of at most S (T log-probabilities and the model
score; |lm| is bounded by (T + 1) |alpha| max|table| + T |beta|); the 64 is headroom for the device's exp and log, whose error in ulp
nobody has measured here.  Where margin > tau the kernel must return the definition's string (==) and its score within tau; below,
only the score is checked, and only if the kernel returned that string.  tests/test_beam.py holds the share of such images <= 5 %."""
import csv
import os

import numpy as np
import pytest
import torch
from PIL import Image

import beam_cases as bc
from dpmn_amd.utils import beam as bm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lm(c):
    from dpmn_amd import ops
    return ops.CharLM(c["table"], c["order"]) if c["table"] is not None else None


def _run(dev, c, lm):
    """The kernel on a case: the logits go up with their padding columns and are passed as a column slice (not contiguous)."""
    from dpmn_amd import ops
    d = torch.from_numpy(c["logits"]).to(dev)
    view = d[:, :c["n_class"]]
    assert view.stride() == (bc.LD, 1) and view.shape[1] < bc.LD
    buf = ops.ctc_beam(view, c["B"], c["T"], c["n_class"], lm, c["width"], c["alpha"], c["beta"])
    return ops.ctc_beam_decode(buf.cpu().numpy(), c["B"], c["T"])


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_kernel_equals_the_definition(dev, name):
    c = bc.case(name)
    cls, length, score = _run(dev, c, _lm(c))
    below = 0
    worst = 0.0
    for b, ((ref_cls, ref_score, margin), tau) in enumerate(zip(c["ref"], c["tau"])):
        got = cls[b, :length[b]].tolist()
        assert (cls[b, length[b]:] == 0).all()
        if margin > tau:
            assert got == ref_cls, (name, b, got, ref_cls, margin)
        else:
            below += 1
        if got == ref_cls:
            worst = max(worst, abs(score[b] - ref_score) / tau)
            assert abs(score[b] - ref_score) <= tau, (name, b, score[b], ref_score, tau)
    print("%s: %d images, %d below the threshold, worst |score error| / tau = %.3g" % (name, c["B"], below, worst))
    assert below <= 0.05 * c["B"] or c["B"] < 20


def test_share_of_images_below_the_threshold():
    total = sum(bc.case(n)["B"] for n in bc.CASES)
    below = sum(int(not m > t) for n in bc.CASES for (_, _, m), t in zip(bc.case(n)["ref"], bc.case(n)["tau"]))
    assert below <= 0.05 * total


def test_out_buffer_and_contiguous_rows(dev):
    """`out` behind ctc_greedy's result (its `extra`), contiguous rows with the padding columns: the same answer as a buffer of its own."""
    from dpmn_amd import ops
    c = bc.case("default_width")
    B, T, C = c["B"], c["T"], c["n_class"]
    d = torch.from_numpy(c["logits"]).to(dev)
    lm = _lm(c)
    buf, _, _ = ops.ctc_greedy(d, B, T, C, extra=B * T + 3 * B)
    ops.ctc_beam(d, B, T, C, lm, c["width"], c["alpha"], c["beta"], out=buf[B * T + B:])
    own = ops.ctc_beam(d[:, :C], B, T, C, lm, c["width"], c["alpha"], c["beta"])
    assert torch.equal(buf[B * T + B:], own)
    greedy, _, _ = ops.ctc_greedy(d, B, T, C)
    assert torch.equal(buf[:B * T + B], greedy)


# ------------------------------------------------------------------------------------------------ NativeCRNN
def test_read_beam_keeps_the_greedy_strings_and_makes_one_copy(dev):
    from dpmn_amd import ops
    from test_gpu_crnn import _images, _pair
    _, nat = _pair(dev)
    imgs = _images(5, 32, 128, 73).to(dev)
    lm = ops.CharLM(bc.table(3), 3)
    plain = nat.read(imgs)
    copies = []
    to_host = torch.Tensor.cpu
    try:
        torch.Tensor.cpu = lambda t, *a, **k: (copies.append(tuple(t.shape)), to_host(t, *a, **k))[1]
        greedy, beam, scores = nat.read_beam(imgs, lm, width=8, alpha=0.5, beta=0.1)
    finally:
        torch.Tensor.cpu = to_host
    rows, B, T = nat.window_rows(imgs)
    assert copies == [(B * T + B + B * T + 3 * B,)]                                  # ONE device-to-host copy
    assert greedy == plain and len(beam) == len(scores) == B == 5 and all(isinstance(s, float) for s in scores)
    host = rows.cpu().numpy()
    for b in range(B):
        trace = {}
        ref_cls, ref_score, margin = bm.beam_np(host[b * T:(b + 1) * T], lm.table, 8, 0.5, 0.1, n_class=nat.nclass, trace=trace)
        tau = bm.tolerance(T, nat.nclass, trace["lp"], (T + 1) * 0.5 * float(np.abs(lm.table).max()) + T * 0.1)
        if margin > tau:
            from dpmn_amd.model.crnn import decode_classes
            assert beam[b] == decode_classes([ref_cls], [len(ref_cls)])[0]
            assert abs(scores[b] - ref_score) <= tau
    # without a model and with width 1 it is still a string over the alphabet
    g2, b2, _ = nat.read_beam(imgs, width=1)
    assert g2 == plain and len(b2) == B
    print("read_beam: greedy %s, beam %s" % (greedy, beam))


# ------------------------------------------------------------------------------------------------ refusals, the cache
def test_refusals(dev):
    from dpmn_amd import _abi, ops
    lm = ops.CharLM(bc.table(2), 2)
    ok = torch.zeros(2 * 4, 40, device=dev)
    with pytest.raises(_abi.DpmnError, match="no CPU fallback"):
        ops.ctc_beam(torch.zeros(8, 40), 2, 4, 37, lm)
    for width in (0, 33, True, 2.0):
        with pytest.raises(_abi.DpmnError, match="width"):
            ops.ctc_beam(ok, 2, 4, 37, lm, width=width)
    with pytest.raises(_abi.DpmnError, match="frames"):
        ops.ctc_beam(torch.zeros(65, 40, device=dev), 1, 65, 37, lm)
    with pytest.raises(_abi.DpmnError, match="classes"):
        ops.ctc_beam(torch.zeros(8, 80, device=dev), 2, 4, 65, None)
    with pytest.raises(_abi.DpmnError, match="37 classes"):
        ops.ctc_beam(torch.zeros(8, 40, device=dev), 2, 4, 38, lm)
    with pytest.raises(_abi.DpmnError, match="order"):
        ops.CharLM(np.zeros((37 ** 3, 37), np.float32), 4)
    with pytest.raises(_abi.DpmnError, match="order"):
        ops.CharLM(bc.table(2), 3)
    for alpha, beta in ((float("nan"), 0.0), (float("inf"), 0.0), (0.5, float("-inf"))):
        with pytest.raises(_abi.DpmnError, match="finite"):
            ops.ctc_beam(ok, 2, 4, 37, lm, alpha=alpha, beta=beta)
    with pytest.raises(_abi.DpmnError, match="CharLM"):
        ops.ctc_beam(ok, 2, 4, 37, bc.table(2))
    with pytest.raises(_abi.DpmnError, match="rows"):
        ops.ctc_beam(ok, 3, 4, 37, lm)
    with pytest.raises(_abi.DpmnError, match="out must be"):
        ops.ctc_beam(ok, 2, 4, 37, lm, out=torch.zeros(5, dtype=torch.int32, device=dev))
    # the C entry point keeps the same limits
    assert _abi.lib.dpmn_ctc_beam_f64(ok.data_ptr(), 40, 37, None, 0, 33, 0.0, 0.0, ok.data_ptr(), ok.data_ptr(), ok.data_ptr(), 2, 4, None) != 0


def test_main_refuses_wrong_combinations(tmp_path):
    import main as cli
    import argparse
    words = tmp_path / "w.txt"
    words.write_text("clock\n", encoding="utf-8")
    base = dict(rec="crnn", test=True, demo_dir=None, demo_tile=False, rec_lm=str(words))
    ns = lambda **kw: argparse.Namespace(**dict(base, **kw))
    assert cli.rec_beam_setting(argparse.Namespace(rec="crnn", test=True)) is None
    got = cli.rec_beam_setting(ns())
    assert got["width"] == 16 and got["order"] == 3 and got["alpha"] == 0.5 and got["beta"] == 0.0 and got["words"] == ["clock"]
    assert cli.rec_beam_setting(ns(rec_lm=None, rec_beam=4))["words"] is None
    for kw, msg in ((dict(demo_tile=True, demo_dir="x"), "--demo_tile"), (dict(rec="aster"), "--rec crnn"), (dict(rec_beam=0), "1 .. 32"),
                    (dict(rec_beam=33), "1 .. 32"), (dict(rec_lm_order=4), "1 .. 3"), (dict(rec_lm_weight=float("nan")), "finite"),
                    (dict(rec_lm_bonus=float("inf")), "finite"), (dict(test=False), "--test or --demo_dir"),
                    (dict(rec_lm=str(tmp_path / "none.txt")), "not a file"), (dict(rec_lm=None, rec_lm_order=2), "need --rec_lm FILE")):
        with pytest.raises(ValueError, match=msg):
            cli.rec_beam_setting(ns(**kw))


def test_one_upload_per_device(dev):
    from dpmn_amd import ops
    c = bc.case("two_frames")
    lm = _lm(c)
    assert lm.uploads == 0
    first = _run(dev, c, lm)
    second = _run(torch.device("cuda", 0), c, lm)
    assert lm.uploads == 1 and all(np.array_equal(a, b) for a, b in zip(first, second))
    assert lm.device_table("cuda:0") is lm.device_table(dev)


# ------------------------------------------------------------------------------------------------ main.py, TextSR.eval
def _csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_main_demo_dir_with_a_model(dev, tmp_path, monkeypatch):
    """--demo_dir on a few crops with --rec crnn --rec_lm FILE: the two columns in their place, their values read_beam's, the images
    those of a run without the flag, whose CSV keeps its header."""
    import main as cli
    from dpmn_amd import ops, workload
    from dpmn_amd.model.crnn import NativeCRNN
    from test_gpu_crnn_eval import _checkpoints, _crnn_sd
    sr, models, psn = workload.build("cfg0", batch=2)[:3]
    d = str(tmp_path)
    _checkpoints(d, models, psn)
    torch.save(_crnn_sd(), os.path.join(d, "crnn.pth"))
    src = os.path.join(d, "in")
    os.makedirs(src)
    rng = np.random.RandomState(8)
    for name in ("a.png", "b.png", "c.png"):
        Image.fromarray(rng.randint(0, 256, (16, 64, 3)).astype(np.uint8)).save(os.path.join(src, name))
    with open(os.path.join(d, "words.txt"), "w", encoding="utf-8") as fh:
        fh.write("clock\nblock\nlock\nlock\n7up\n")
    seen = []
    read_beam = NativeCRNN.read_beam

    def spy(self, images, lm=None, width=16, alpha=0.5, beta=0.0):
        out = read_beam(self, images, lm, width, alpha, beta)
        seen.append((out, lm, width, alpha, beta))
        return out
    monkeypatch.setattr(NativeCRNN, "read_beam", spy)

    def run(tag, **kw):
        args = workload.make_args("tsrn", 1, 1, 2)
        args.resume, args.test, args.test_data_dir, args.synthetic_steps, args.rec = d, False, None, 0, "crnn"
        args.vis_dir, args.demo_dir, args.demo_out = os.path.join(d, "vis_" + tag), src, os.path.join(d, tag)
        for k, v in kw.items():
            setattr(args, k, v)
        config = cli.AttrDict({"TRAIN": dict(vars(workload.make_config(2).TRAIN), ckpt_dir=os.path.join(d, "ckpt_" + tag),
                                             VAL={"crnn_pretrained": os.path.join(d, "crnn.pth")})})
        cli.main(config, args)
        return args.demo_out
    plain = run("plain")
    assert not seen
    beamed = run("beamed", rec_lm=os.path.join(d, "words.txt"), rec_lm_weight=0.7, rec_lm_bonus=0.1)
    old, new = _csv(os.path.join(plain, "demo_result.csv")), _csv(os.path.join(beamed, "demo_result.csv"))
    assert old[0] == ["file", "lr_string", "sr_string"] and new[0] == old[0] + ["sr_lm", "sr_lm_score"]
    assert [r[:3] for r in new] == old and len(new) == 4
    assert sorted(os.listdir(beamed)) == sorted(os.listdir(plain)) == ["a_sr.png", "b_sr.png", "c_sr.png", "demo_result.csv"]
    for f in ("a_sr.png", "b_sr.png", "c_sr.png"):
        with open(os.path.join(beamed, f), "rb") as g, open(os.path.join(plain, f), "rb") as p:
            assert g.read() == p.read(), f
    # the two columns are read_beam's, called with the flags' values and an order-3 model of the file (lock counts twice)
    assert seen and all(s[2:] == (16, 0.7, 0.1) and s[1].order == 3 for s in seen)
    assert np.array_equal(seen[0][1].table, bm.build_char_lm(["clock", "block", "lock", "lock", "7up"], 3))
    strings = [w for s in seen for w in s[0][1]]
    scores = [v for s in seen for v in s[0][2]]
    assert [r[3] for r in new[1:]] == strings and [r[4] for r in new[1:]] == ["%.6g" % v for v in scores]
    assert [r[2] for r in new[1:]] == [w for s in seen for w in s[0][0]]
    # with a lexicon and the confidence columns: sr_lm follows the lexicon's columns
    both = run("both", rec_lm=os.path.join(d, "words.txt"), rec_lexicon=os.path.join(d, "words.txt"), demo_conf=True)
    head = _csv(os.path.join(both, "demo_result.csv"))[0]
    assert head == ["file", "lr_string", "lr_conf", "sr_string", "sr_conf", "sr_lexicon", "sr_lexicon_score", "sr_lm", "sr_lm_score"]
    # without a lexicon they follow sr_conf and stand before turned
    up = run("up", rec_beam=4, demo_upright=True)
    rows = _csv(os.path.join(up, "demo_result.csv"))
    assert rows[0] == ["file", "lr_string", "lr_conf", "sr_string", "sr_conf", "sr_lm", "sr_lm_score", "turned"]
    assert seen[-1][1] is None and seen[-1][2] == 4 and all(len(r) == 8 and r[7] in ("0", "1") for r in rows[1:])
    print("main.py --rec_lm: %s" % new[1:])


def test_eval_counts_accuracy_lm(dev):
    from dpmn_amd import ops, workload
    from dpmn_amd.model.crnn import NativeCRNN
    from dpmn_amd.utils import synth
    from test_gpu_crnn_eval import _crnn_sd
    sr, models, psn = workload.build("cfg0", batch=2)[:3]
    rec = NativeCRNN(32, 1, 37, 256).to(dev).eval()
    rec.load_state_dict(_crnn_sd())
    b = synth.synth_batch(2, seed=5)
    loader = lambda: [(b["images_hr"], b["images_lr"], b["label_vecs"], ["ab", "7"])]
    plain = sr.eval(models, loader(), rec=rec, model_psn=psn)
    beam = {"lm": ops.CharLM(bc.table(2), 2), "width": 8, "alpha": 0.5, "beta": 0.0}
    got = sr.eval(models, loader(), rec=rec, model_psn=psn, beam=beam)
    assert "accuracy_lm" not in plain and set(got) == set(plain) | {"accuracy_lm"}
    assert got["accuracy"] == plain["accuracy"] and got["psnr_avg"] == plain["psnr_avg"]
    assert got["accuracy_lm"] is not None and 0.0 <= got["accuracy_lm"] <= 1.0
    with pytest.raises(ValueError, match="read_beam"):
        sr.eval(models, loader(), rec=lambda images: [""] * images.shape[0], model_psn=psn, beam=beam)
