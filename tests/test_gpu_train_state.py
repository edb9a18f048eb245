"""A training run that is stopped and continued from its state file (TextSR.train(state_path=...), main.py --train_state) ends with
bit-for-bit the weights, BatchNorm statistics, Adam moments and losses of the run that was never stopped.  Stack: TATT PSN + 2+2
PGRMs + 2 DistillModules + CMM at B = 4 (the one of test_training_step_is_bitwise_reproducible at its smallest), synthetic weights
and batches, a callable loader of 3 batches per epoch; the restart lands inside epoch 0 and the continuation crosses into epoch 1."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dpmn_amd.utils import synth

pytestmark = pytest.mark.gpu

B, B1, B2 = 4, 2, 2
CASES = {"drop": dict(drop=0.1, rotate=0.0), "rotate": dict(drop=0, rotate=3.0)}
_BATCHES = {}
_CACHE = {}        # (compute mode, case) -> {"A": the uninterrupted run's results, "state": the file run B left at it = 2}


def _loader(epoch):
    """3 synthetic batches per epoch, other ones in every epoch; made once, never changed"""
    for i in range(3):
        seed = 50 + 3 * epoch + i
        if seed not in _BATCHES:
            b = synth.synth_batch(B, seed=seed)
            _BATCHES[seed] = (b["images_hr"], b["images_lr"], b["label_vecs"])
        yield _BATCHES[seed]


def _mission(out_dir, drop=0, rotate=0.0, val_interval=None):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR

    class Filled(TextSR):
        def build_training(self, world_size=1, group=None):
            out = super().build_training(world_size, group)
            models, psn, distill = out[0], out[1], out[2]
            for i, m in enumerate([psn] + models + distill):      # (the parameters are views of the trainer's arena: written in place)
                sd = m.state_dict()
                synth.synth_fill_(sd, 300 + i)
                with torch.no_grad():
                    for k, v in m.state_dict().items():
                        v.copy_(sd[k])
            psn.eval()
            return out

    cfg = workload.make_config(B)
    cfg.TRAIN.ckpt_dir = out_dir
    cfg.TRAIN.displayInterval = 1000
    if val_interval:
        cfg.TRAIN.VAL = SimpleNamespace(valInterval=val_interval)
    args = workload.make_args("tatt", B1, B2, B, drop=drop)
    args.rotate_train = rotate
    sr = Filled(cfg, args)
    sr.vis_dir = out_dir
    return sr


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def _results(sr, models, distill):
    torch.cuda.synchronize()
    return dict(sd=[{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in models + distill],
                trainer=sr.trainer.state_dict(), loss=sr.last_loss.cpu().clone(), loop=sr.loop_state)


def _reference(case, tmp_path_factory):
    """Run A (never stopped) and the first phase of run B (stopped at it = 2) of a case, once per compute mode."""
    from dpmn_amd import _abi
    key = (_abi.lib.dpmn_get_compute_dtype(), case)
    if key not in _CACHE:
        d = tmp_path_factory.mktemp("train_state_%s" % case)
        _seed(1)
        sr = _mission(str(d / "a"), **CASES[case])
        a = _results(sr, *sr.train(_loader, steps=5, epochs=2))
        assert not os.path.exists(str(d / "a" / "state.pt"))
        _seed(1)
        sr = _mission(str(d / "b"), **CASES[case])
        state = str(d / "b" / "state.pt")
        sr.train(_loader, steps=2, epochs=2, state_path=state)
        assert sr.loop_state["it"] == 2 and sr.loop_state["epoch"] == 0 and sr.loop_state["done"] == 2
        _CACHE[key] = {"A": a, "state": state}
    return _CACHE[key]


def _continue(case, ref, tmp_path):
    """Second phase of run B: a NEW object under other seeds continues from (a hard link to) the state file to it = 5."""
    state = str(tmp_path / "state.pt")
    os.link(ref["state"], state)        # (the continuation REPLACES its file: the cached one stays as it was)
    _seed(99)
    sr = _mission(str(tmp_path), **CASES[case])
    got = _results(sr, *sr.train(_loader, steps=5, epochs=2, state_path=state))
    assert got["loop"]["it"] == 5 and got["loop"]["epoch"] == 1 and got["loop"]["done"] == 2
    return got


def _differing(a, b):
    """(differing words in the models' and DistillModules' state_dicts, in Adam's m and v, total words)"""
    nd_w = sum(int((x[k] != y[k]).sum()) for x, y in zip(a["sd"], b["sd"]) for k in x)
    nd_mv = sum(int((x != y).sum()) for key in ("m", "v") for x, y in zip(a["trainer"][key], b["trainer"][key]))
    return nd_w, nd_mv, sum(v.numel() for x in a["sd"] for v in x.values())


@pytest.mark.parametrize("case", ["drop", "rotate"])
def test_stop_and_continue_is_bitwise_the_uninterrupted_run(case, tmp_path, tmp_path_factory):
    """drop: Dropout = attn_drop = DropPath = 0.1 (torch's CPU generator feeds the seeds); rotate: rotate_train = 3 at rates 0
    (numpy's global state feeds the angles)."""
    from helpers import record
    ref = _reference(case, tmp_path_factory)
    a, b = ref["A"], _continue(case, ref, tmp_path)
    nd_w, nd_mv, n = _differing(a, b)
    record("train_state_%s" % case, "weight / buffer words differing after stop and continue (of %d)" % n, nd_w, 0)
    record("train_state_%s" % case, "Adam moment words differing after stop and continue", nd_mv, 0)
    assert [x.keys() for x in a["sd"]] == [x.keys() for x in b["sd"]]
    for i, (x, y) in enumerate(zip(a["sd"], b["sd"])):
        for k in x:
            assert torch.equal(x[k], y[k]), "model %d %s differs" % (i, k)
    assert a["trainer"]["t"] == b["trainer"]["t"] == 5
    for key in ("m", "v"):
        for i, (x, y) in enumerate(zip(a["trainer"][key], b["trainer"][key])):
            assert torch.equal(x, y), "Adam %s of model %d differs" % (key, i)
    assert torch.equal(a["loss"], b["loss"]), (float(a["loss"]), float(b["loss"]))
    assert nd_w == 0 and nd_mv == 0
    assert any(float(m.abs().sum()) > 0 for m in a["trainer"]["m"])


def test_without_the_saved_random_state_the_continuation_differs(tmp_path, tmp_path_factory, monkeypatch):
    """The guard of the test above: at rates 0.1 the run really draws from the restored streams -- a continuation that keeps
    its own (seed 99) streams ends somewhere else."""
    from dpmn_amd.interfaces import base
    ref = _reference("drop", tmp_path_factory)
    monkeypatch.setattr(base, "rng_restore", lambda state, device=None: None)
    b = _continue("drop", ref, tmp_path)
    nd_w, nd_mv, _ = _differing(ref["A"], b)
    assert nd_w > 0 and nd_mv > 0, (nd_w, nd_mv)
    assert ref["A"]["trainer"]["t"] == b["trainer"]["t"] == 5


def test_bookkeeping_and_log_rows_survive_stop_and_continue(tmp_path):
    """valInterval = 2: evaluations at it = 2 and 4 (best-model saves, log.csv rows).  Stopped at it = 2 -- right after the first
    evaluation -- and continued: best, best_hist, best_info, converge and log.csv equal the uninterrupted run's, no row twice."""
    vb = synth.synth_batch(B, seed=7)
    val = [(vb["images_hr"], vb["images_lr"], vb["label_vecs"])]
    _seed(1)
    sr = _mission(str(tmp_path / "a"), val_interval=2)
    sr.train(_loader, steps=5, epochs=2, val_loader=val)
    a = sr.loop_state
    _seed(1)
    sr = _mission(str(tmp_path / "b"), val_interval=2)
    state = str(tmp_path / "b" / "state.pt")
    sr.train(_loader, steps=2, epochs=2, val_loader=val, state_path=state)
    assert len(sr.loop_state["converge"]) == 1 and sr.loop_state["best"] is not None
    _seed(99)
    sr = _mission(str(tmp_path / "b"), val_interval=2)
    sr.train(_loader, steps=5, epochs=2, val_loader=val, state_path=state)
    b = sr.loop_state
    assert len(a["converge"]) == 2 and [c["iterator"] for c in a["converge"]] == [2, 4]
    for key in ("epoch", "it", "done", "saved_at", "best", "best_hist", "best_info", "converge"):
        assert a[key] == b[key], (key, a[key], b[key])
    rows_a = open(str(tmp_path / "a" / "log.csv")).read().splitlines()
    rows_b = open(str(tmp_path / "b" / "log.csv")).read().splitlines()
    assert rows_a == rows_b and sum(",val," in r for r in rows_b) == 2, (rows_a, rows_b)
    # a run killed after an evaluation whose rows reached log.csv but before the next state write: the continuation takes the rows
    # back and writes them again, once
    with open(str(tmp_path / "b" / "log.csv"), "a") as f:
        f.write("1,val,,9.0,0.9\n")
    _seed(5)
    sr = _mission(str(tmp_path / "b"), val_interval=2)
    sr.train(_loader, steps=5, epochs=2, val_loader=val, state_path=state)      # (nothing left to train)
    assert sr.loop_state["it"] == 5 and sr.last_loss is None
    assert open(str(tmp_path / "b" / "log.csv")).read().splitlines() == rows_a


def test_load_state_dict_sets_the_device_step_counter():
    """hipGraph training keeps Adam's step count in device memory (Trainer.device_step_counter): a loaded state must reach it."""
    sr = _mission(".")
    models, psn, distill, crit, trainer = sr.build_training()
    trainer.device_step_counter()
    sd = trainer.state_dict()
    assert sd["t"] == 0 and float(trainer.t_dev) == 0.0
    sd["t"] = 7
    sd["m"][0] = sd["m"][0] + 0.5
    trainer.load_state_dict(sd)
    assert trainer.t == 7 and float(trainer.t_dev) == 7.0
    back = trainer.state_dict()
    assert torch.equal(back["m"][0], sd["m"][0]) and float(back["m"][0][0]) == 0.5 and torch.equal(back["v"][-1], sd["v"][-1])
