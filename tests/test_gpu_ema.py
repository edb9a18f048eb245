"""Averaged weights (Trainer(ema_decay=...), TextSR.train(ema_decay=...), main.py --ema) on the GPU: the fused kernel
dpmn_adam_clip_ema_f32 against dpmn_adam_clip_f32 (bitwise) and the float64 restatement train/optim.py ema_reference, the trainer's
`e` beside `m` / `v`, the swap Trainer.ema_weights(), the captured step, and the training loop with its checkpoints and state file.

The bound on one update of the average, e' = fl(fl(d e) + fl(fl(1 - d) p)), u = 2^-24: the rounding of 1 - d, two products and a
sum give |e' - (d e + (1 - d) p)| <= 2u |d e| + 3u |(1 - d) p| + O(u^2) <= 4u (|d e| + |(1 - d) p|)."""
import os

import pytest
import torch

from dpmn_amd.utils import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _guarded(values):
    """values inside a buffer with GUARD sentinel elements on either side -> (buffer, the view the kernel gets)"""
    buf = torch.full((values.numel() + 2 * GUARD,), SENTINEL, device=values.device)
    buf[GUARD:GUARD + values.numel()] = values
    return buf, buf[GUARD:GUARD + values.numel()]


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 65537])
def test_fused_kernel_is_adam_clip_plus_the_average(dev, n):
    """20 steps per case; cases: gradient norm above / below max_norm = 0.25 and max_norm = 0 (no clip), the step as a host scalar and
    through step_dev, d = 0.5 and 0.999.  param / exp_avg / exp_avg_sq bitwise those of dpmn_adam_clip_f32; the average within the
    one-update bound of the restatement fed the kernel's own p_new and its own previous average; nothing written beyond n."""
    from dpmn_amd._abi import lib, check, dptr, stream
    from dpmn_amd.train.optim import ema_reference
    from helpers import record
    steps = 20
    gen = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=gen).to(dev)
    grads = torch.randn(steps, n, generator=gen).to(dev)
    grads = grads / grads.norm(dim=1, keepdim=True)
    worst = 0.0
    for d in (0.5, 0.999):
        for norm, max_norm in ((2.0, 0.25), (0.05, 0.25), (2.0, 0.0)):
            for on_device in (False, True):
                bufs = {k: _guarded(v) for k, v in dict(p=p0, m=torch.zeros_like(p0), v=torch.zeros_like(p0), e=p0).items()}
                p, m, v, e = (bufs[k][1] for k in "pmve")
                p2, m2, v2 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
                step_dev = torch.zeros(1, device=dev) if on_device else None
                bad_bits = torch.zeros((), device=dev, dtype=torch.int64)
                excess = torch.zeros((), device=dev, dtype=torch.float64)      # max of error / bound over elements and steps
                for t in range(1, steps + 1):
                    g = (grads[t - 1] * norm).contiguous()
                    normsq = (g.double() ** 2).sum().float().reshape(1)
                    if on_device:
                        step_dev.fill_(float(t))
                    step = 0 if on_device else t
                    e_prev = e.clone()
                    check(lib.dpmn_adam_clip_ema_f32(dptr(p), dptr(g), dptr(m), dptr(v), dptr(e), dptr(normsq), max_norm, 1e-2, 0.5, 0.999,
                                                     1e-8, step, dptr(step_dev, True), d, n, stream()))
                    check(lib.dpmn_adam_clip_f32(dptr(p2), dptr(g), dptr(m2), dptr(v2), dptr(normsq), max_norm, 1e-2, 0.5, 0.999, 1e-8,
                                                 step, dptr(step_dev, True), n, stream()))
                    bad_bits += (p != p2).sum() + (m != m2).sum() + (v != v2).sum()
                    d32 = float(torch.tensor(d, dtype=torch.float32))
                    ref = ema_reference(e_prev, p, d)
                    bound = 4 * U * ((d32 * e_prev.double()).abs() + ((1.0 - d32) * p.double()).abs())
                    err = (e.double() - ref).abs()
                    excess = torch.maximum(excess, torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
                case = "n=%d d=%g norm=%g max_norm=%g step_dev=%s" % (n, d, norm, max_norm, on_device)
                assert int(bad_bits) == 0, "param / moments differ from dpmn_adam_clip_f32: %s" % case
                assert float(excess) <= 1.0, "average outside the one-update bound (%.3f of it): %s" % (float(excess), case)
                assert float((p - p0).abs().max()) > 0 and float((e - p0).abs().max()) > 0, case
                for k, (buf, _) in bufs.items():
                    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "%s: wrote beyond n: %s" % (k, case)
                worst = max(worst, float(excess))
    record("adam_clip_ema_n%d" % n, "average: worst error / (4 u (|d e| + |(1 - d) p|)) over 12 cases x 20 steps", worst, 1.0)


# ---------------------------------------------------------------------------------------------------- 2. the trainer
class _TwoLayers(torch.nn.Module):
    """15 + 3 + 72 + 4 parameters: every view of the arena is padded (to 64, 64, 128, 64 floats)"""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(5, 3)
        self.conv = torch.nn.Conv2d(2, 4, 3)


def _elementwise_loss(module, t):
    """a loss whose backward is elementwise (no reduction order, no atomics): the twin trainers get bitwise the same gradients"""
    return sum(((p * (0.5 + 0.25 * i + t)).sin() * (1.0 + i)).sum() for i, p in enumerate(module.parameters()))


def test_trainer_keeps_e_beside_the_moments(dev):
    from dpmn_amd.train.optim import Trainer, ema_reference
    d, steps = 0.9, 5
    torch.manual_seed(11)
    mods = [_TwoLayers().to(dev), _TwoLayers().to(dev)]
    mods[1].load_state_dict(mods[0].state_dict())
    tr = Trainer([mods[0]], lr=1e-2, ema_decay=d)
    twin = Trainer([mods[1]], lr=1e-2)
    assert twin.ema_decay is None and all(g.e is None for g in twin.groups), "nothing is allocated without ema_decay"
    assert len(tr.groups) == 1 and tr.flat_p.numel() == 64 + 64 + 128 + 64
    g = tr.groups[0]
    assert torch.equal(g.e, tr.flat_p) and g.e.data_ptr() != tr.flat_p.data_ptr()      # the average starts as a copy
    d32 = float(torch.tensor(d, dtype=torch.float32))
    e64, err = tr.flat_p.double().clone(), torch.zeros_like(tr.flat_p, dtype=torch.float64)
    for t in range(steps):
        for trainer, mod in ((tr, mods[0]), (twin, mods[1])):
            trainer.zero_grad()
            _elementwise_loss(mod, t).backward()
            trainer.step()
        assert torch.equal(tr.flat_p, twin.flat_p), "parameters differ from the trainer without the average at step %d" % t
        assert torch.equal(g.m, twin.groups[0].m) and torch.equal(g.v, twin.groups[0].v), "moments differ at step %d" % t
        # the restatement driven by the recorded parameters, and how far fp32 may have drifted from it: one-update bound on the
        # kernel's own operands (|e_kernel| <= |e64| + err) plus the decayed earlier error
        p_t = tr.flat_p.double()
        err = d32 * err + 4 * U * (d32 * (e64.abs() + err) + (1.0 - d32) * p_t.abs())
        e64 = ema_reference(e64, p_t, d)
        assert bool(((g.e.double() - e64).abs() <= err).all()), "e differs from the restatement at step %d" % t
    assert float((g.e - tr.flat_p).abs().max()) > 0
    used = torch.zeros(g.n, dtype=torch.bool, device=dev)
    for gi, o, k in tr._moment_layout()[0]:
        used[o:o + k] = True
    assert int(used.sum()) == 15 + 3 + 72 + 4 and float(g.e[~used].abs().max()) == 0.0, "padding of e must stay zero"
    sd = tr.state_dict()
    assert sd["e"][0].shape == (94,) and torch.equal(sd["e"][0], g.e[used].cpu()) and "e" not in twin.state_dict()


# ---------------------------------------------------------------------------------------------------- 3. the swap
def _small_cmm(dev, seed=41):
    from dpmn_amd.model.cmm import ComplementationModulationModule
    m = ComplementationModulationModule(cnum=8)
    sd = m.state_dict()
    synth.synth_fill_(sd, seed)
    m.load_state_dict(sd)
    return m.to(dev)


def _given_gradient_step(trainer, t):
    """One optimizer step on a gradient that is written into the arena (the narrow CMM's weight gradients go through atomics, so two
    runs that are to be compared bitwise cannot take theirs from a backward pass)."""
    trainer.zero_grad()
    gen = torch.Generator().manual_seed(700 + t)
    g = torch.randn(trainer.flat_g.numel(), generator=gen) * 1e-3
    used = torch.zeros(g.numel(), dtype=torch.bool)
    assert len(trainer.groups) == 1
    for _, o, k in trainer._moment_layout()[0]:
        used[o:o + k] = True
    trainer.flat_g.copy_(g * used)          # (padding carries no gradient, as after a backward pass)
    trainer.step()


def test_ema_weights_swaps_the_averaged_weights_in_and_the_live_ones_back(dev):
    from dpmn_amd.model.cmm import ComplementationModulationModule
    from dpmn_amd.train.optim import Trainer
    x1 = synth.uniform("ema_x1", (2, 3, 32, 128), 0, 1, 7).to(dev)
    x2 = synth.uniform("ema_x2", (2, 3, 32, 128), 0, 1, 7).to(dev)
    cmm, cmm_never = _small_cmm(dev), _small_cmm(dev)
    for m in (cmm, cmm_never):
        for p in m.parameters():
            p.requires_grad = True
    tr, never = Trainer([cmm], lr=1e-3, ema_decay=0.5), Trainer([cmm_never], lr=1e-3, ema_decay=0.5)
    for trainer in (tr, never):
        for t in range(2):
            _given_gradient_step(trainer, t)
    cmm.eval()
    with torch.no_grad():
        out_live = cmm(x1, x2).clone()            # (leaves the eval packs of the LIVE weights behind)
    live = [p.detach().clone() for p in cmm.parameters()]
    e = tr.state_dict()["e"][0].to(dev)
    with tr.ema_weights():
        off = 0
        for p in cmm.parameters():
            assert torch.equal(p.detach().reshape(-1), e[off:off + p.numel()]), "inside ema_weights() the parameters are the averaged values"
            off += p.numel()
        assert off == e.numel() and any(not torch.equal(p.detach(), q) for p, q in zip(cmm.parameters(), live))
        with torch.no_grad():
            out_avg = cmm(x1, x2).clone()
        copy = ComplementationModulationModule(cnum=8)
        copy.load_state_dict({k: v.detach().cpu().clone() for k, v in cmm.state_dict().items()})
        copy = copy.to(dev).eval()
        with torch.no_grad():
            out_copy = copy(x1, x2)
        assert torch.equal(out_avg, out_copy), "the eval packs of the live weights were not dropped on entry"
        assert not torch.equal(out_avg, out_live)
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.zero_grad()
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.step()
        with pytest.raises(RuntimeError, match="nest"):
            with tr.ema_weights():
                pass
    for p, q in zip(cmm.parameters(), live):
        assert torch.equal(p.detach(), q), "after ema_weights() the parameters are bitwise the live ones"
    with torch.no_grad():
        assert torch.equal(cmm(x1, x2), out_live), "the eval packs of the averaged weights were not dropped on exit"
    cmm.train()
    _given_gradient_step(tr, 2)
    _given_gradient_step(never, 2)
    assert torch.equal(tr.flat_p, never.flat_p), "the step after a swap differs from the step of a run that never swapped"
    for a, b in zip(tr.groups, never.groups):
        assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.e, b.e)
    assert tr.t == never.t == 3


# ---------------------------------------------------------------------------------------------------- 4. / 5. the training stack
def _mission(out_dir, ema_decay=None, val_interval=None):
    """The stack of tests/test_gpu_train_state.py (TATT PSN + 2+2 PGRMs + 2 DistillModules + CMM at B = 4).  Its synthetic weights are
    written in place after the trainer was built, so the average is started again from them."""
    import test_gpu_train_state as ts
    sr = ts._mission(out_dir, val_interval=val_interval)
    build = sr.build_training

    def build_and_restart_the_average(world_size=1, group=None):
        out = build(world_size, group)
        if out[4].ema_decay is not None:
            out[4].reset_ema()
        return out
    sr.build_training = build_and_restart_the_average
    sr.ema_decay = ema_decay
    return sr


def _batches(dev, n=3):
    import test_gpu_train_state as ts
    out = []
    for i, (hr, lr, lv) in enumerate(ts._loader(0)):
        priors = [torch.floor(synth.uniform("ema_tp%d_%d" % (i, k), (ts.B, 2, 32, 128), 0, 256, 4)).to(dev) for k in range(ts.B1)]
        out.append((lr.to(dev), hr.to(dev), lv.to(dev), priors))
    return out[:n]


def _trained(models, distill, trainer):
    torch.cuda.synchronize()
    return dict(sd=[{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in models + distill], trainer=trainer.state_dict())


def _assert_same_training(a, b, what):
    for i, (x, y) in enumerate(zip(a["sd"], b["sd"])):
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: model %d %s differs" % (what, i, k)
    for key in ("m", "v", "e"):
        for i, (x, y) in enumerate(zip(a["trainer"][key], b["trainer"][key])):
            assert torch.equal(x, y), "%s: '%s' of model %d differs" % (what, key, i)


def test_graphed_train_step_with_the_average_equals_eager(dev):
    import test_gpu_train_state as ts
    ts._seed(1)
    batches = _batches(dev)
    runs = []
    for graphed in (False, True):
        ts._seed(1)
        sr = _mission(".", ema_decay=0.9)
        models, psn, distill, crit, trainer = sr.build_training()
        assert trainer.ema_decay == 0.9
        if graphed:
            run = sr.graphed_train_step(models, psn, distill, crit, trainer, *batches[0], warmup=2)
            for lr, hr, lv, priors in batches:
                run(lr, hr, lv, priors)
        else:
            for lr, hr, lv, priors in batches:
                sr.train_step(models, psn, distill, crit, trainer, lr, hr, lv, text_priors=priors)
        runs.append(_trained(models, distill, trainer))
        flat = torch.cat(runs[-1]["trainer"]["e"])
        live = torch.cat([p.detach().reshape(-1).cpu() for m in models + distill for p in m.parameters()])
        assert flat.shape == live.shape and not torch.equal(flat, live)
    _assert_same_training(runs[0], runs[1], "3 graph replays vs 3 eager steps")


def test_training_loop_scores_and_ships_the_average_and_continues_exactly(dev, tmp_path):
    import test_gpu_train_state as ts
    from dpmn_amd.interfaces import base
    d = 0.9
    vb = synth.synth_batch(ts.B, seed=7)
    val = [(vb["images_hr"], vb["images_lr"], vb["label_vecs"])]

    def train(out_dir, steps, state=None, ema=d, seed=1):
        ts._seed(seed)
        sr = _mission(str(out_dir), val_interval=2)
        models, distill = sr.train(ts._loader, steps=steps, epochs=2, val_loader=val, state_path=state, ema_decay=ema)
        return sr, models, distill

    # A: never stopped.  B: stopped at it = 2, right after the validation pass, and continued to it = 4 by a new object
    sr_a, models_a, distill_a = train(tmp_path / "a", 4)
    a = dict(_trained(models_a, distill_a, sr_a.trainer), loss=sr_a.last_loss.cpu().clone())
    state = str(tmp_path / "b" / "state.pt")
    sr_b, models_b, distill_b = train(tmp_path / "b", 2, state)
    assert sr_b.loop_state["it"] == 2 and sr_b.loop_state["best"] is not None and len(sr_b.loop_state["converge"]) == 1
    st = base.read_train_state(state)
    assert st["fingerprint"]["ema"] == d and st["trainer"]["t"] == 2
    # the best-model files written from the pass at it = 2 hold the averaged weights at step 2, checkpoint.pth the live ones
    ckpt = tmp_path / "b" / "ckpt"
    for i, m in enumerate(models_b):
        best = torch.load(str(ckpt / ("model_best_sum_0_%d.pth" % i)), map_location="cpu")["state_dict_G"]
        e, off = st["trainer"]["e"][i], 0
        for name, p in m.named_parameters():
            assert torch.equal(best[name].reshape(-1), e[off:off + p.numel()]), "best checkpoint %d: %s is not the averaged weight" % (i, name)
            off += p.numel()
        assert off == e.numel()
        for name, _ in m.named_buffers():
            assert torch.equal(best[name], st["models"][i][name]), "buffers are the live ones"
    last = torch.load(str(ckpt / "checkpoint.pth"), map_location="cpu")["state_dict_G"]      # (every model overwrites it: the CMM's)
    live = st["models"][len(models_b) - 1]
    assert last.keys() == live.keys() and all(torch.equal(last[k], live[k]) for k in live), "checkpoint.pth holds the live weights"
    best_cmm = torch.load(str(ckpt / ("model_best_sum_0_%d.pth" % (len(models_b) - 1))), map_location="cpu")["state_dict_G"]
    assert any(not torch.equal(best_cmm[k], live[k]) for k in live)
    # the continuation
    sr_c, models_c, distill_c = train(tmp_path / "b", 4, state, seed=99)
    c = dict(_trained(models_c, distill_c, sr_c.trainer), loss=sr_c.last_loss.cpu().clone())
    assert sr_c.loop_state["it"] == 4 and a["trainer"]["t"] == c["trainer"]["t"] == 4
    _assert_same_training(a, c, "stopped at 2 and continued vs never stopped")
    assert torch.equal(a["loss"], c["loss"]), (float(a["loss"]), float(c["loss"]))
    assert sr_a.loop_state["converge"] == sr_c.loop_state["converge"] and sr_a.loop_state["best"] == sr_c.loop_state["best"]
    # a state written with the average is refused by a run without it, and the other way round; a state from before the field is "off"
    with pytest.raises(ValueError, match=r"\bema = "):
        train(tmp_path / "r1", 4, state, ema=None)
    plain = dict(st, fingerprint=dict(st["fingerprint"], ema=None), trainer={k: v for k, v in st["trainer"].items() if k != "e"})
    path = str(tmp_path / "plain.pt")
    base.write_train_state(path, plain)
    with pytest.raises(ValueError, match=r"\bema = "):
        train(tmp_path / "r3", 2, path)
    old = dict(plain, fingerprint={k: v for k, v in st["fingerprint"].items() if k != "ema"})
    base.write_train_state(path, old)
    sr_o, _, _ = train(tmp_path / "r4", 2, path, ema=None)          # (it = 2 already: nothing left to train)
    assert sr_o.loop_state["it"] == 2 and sr_o.trainer.ema_decay is None and "e" not in sr_o.trainer.state_dict()
