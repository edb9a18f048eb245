"""Averaged weights on the CPU (dpmn_amd/train/optim.py Trainer(ema_decay=...), interfaces/base.py fingerprint, main.py --ema): the
float64 restatement, the layout of 'e' in the saved state across world sizes and ZeRO-1, the swap under gloo, the argument checks.
The optimizer kernels are GPU-only in the product; as in test_dp_gloo.py torch restatements are injected for them."""
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0.9


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torch_sumsq(g, out, part):
    out.copy_((g.double() ** 2).sum().float().reshape(1))


def _torch_adam_clip(p, g, m, v, normsq, max_norm, lr, b1, b2, eps, step, step_dev):
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (float(normsq[0]) ** 0.5 + 1e-6))
    gi = g * coef
    m.mul_(b1).add_(gi, alpha=1 - b1)
    v.mul_(b2).addcmul_(gi, gi, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.sub_((lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps))


def _torch_adam_clip_ema(p, g, m, v, e, normsq, max_norm, lr, b1, b2, eps, step, step_dev, d):
    _torch_adam_clip(p, g, m, v, normsq, max_norm, lr, b1, b2, eps, step, step_dev)
    d = torch.tensor(d, dtype=torch.float32)
    e.copy_(d * e + (1 - d) * p)


def _substitute(optim):
    optim._sumsq, optim._adam_clip, optim._adam_clip_ema = _torch_sumsq, _torch_adam_clip, _torch_adam_clip_ema


@pytest.fixture()
def optim(monkeypatch):
    from dpmn_amd.train import optim
    monkeypatch.setattr(optim, "_sumsq", _torch_sumsq)
    monkeypatch.setattr(optim, "_adam_clip", _torch_adam_clip)
    monkeypatch.setattr(optim, "_adam_clip_ema", _torch_adam_clip_ema)
    return optim


class ComplementationModulationModule(torch.nn.Module):     # same class NAME as the big model: scheduled first in the arenas
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 301)      # odd sizes: every parameter view is padded to 64 floats
        self.b = torch.nn.Linear(301, 3)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _build(seed):
    torch.manual_seed(seed)
    return [torch.nn.Linear(6, 5), ComplementationModulationModule(), torch.nn.Linear(3, 2)]


def _loss(models, x):
    head, big, tail = models
    return tail(big(head(x))).pow(2).mean() * 50


def _trainer(optim, models, world=1, zero1=None, group_mb=0.003, ema=D):
    # max_norm far above any gradient norm here: the clip coefficient is exactly 1 however the norm was summed (ZeRO-1 adds per-shard
    # partial sums), so a world-2 run on identical batches is bit for bit the world-1 run
    return optim.Trainer(models, lr=1e-2, beta1=0.5, max_norm=1e6, world_size=world, zero1=zero1, group_mb=group_mb, ema_decay=ema)


def _steps(tr, models, n=3):
    for step in range(n):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * step))      # the same batch on every rank
        tr.zero_grad()
        _loss(models, x).backward()
        tr.step()
    tr.sync_params()


def _params(models):
    return [torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone() for m in models]


# ---------------------------------------------------------------------------------------------------- restatement
def test_ema_reference_is_the_literal_loop():
    from dpmn_amd.train.optim import ema_reference
    gen = torch.Generator().manual_seed(3)
    e, p = torch.randn(257, generator=gen), torch.randn(257, generator=gen)
    for d in (0.5, 0.9, 0.999):
        got = ema_reference(e, p, d)
        assert got.dtype == torch.float64 and got.shape == e.shape
        d32 = float(torch.tensor(d, dtype=torch.float32))          # the decay as the kernel receives it
        want = [d32 * float(e[i]) + (1.0 - d32) * float(p[i]) for i in range(e.numel())]
        assert got.tolist() == want
    assert ema_reference(e, e, 0.999).float().allclose(e, rtol=1e-7, atol=0)      # a fixed point: the average of a constant


def test_world1_trainer_average_follows_the_restatement(optim):
    from dpmn_amd.train.optim import ema_reference
    models = _build(3)
    tr = _trainer(optim, models)
    assert len(tr.groups) >= 2 and all(torch.equal(g.e, g.flat_p) and g.e.data_ptr() != g.flat_p.data_ptr() for g in tr.groups)
    e64 = [p.double() for p in _params(models)]
    for step in range(3):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * step))
        tr.zero_grad()
        _loss(models, x).backward()
        tr.step()
        e64 = [ema_reference(e, p, D) for e, p in zip(e64, _params(models))]
    sd = tr.state_dict()
    assert len(sd["e"]) == 3
    for i, (got, want) in enumerate(zip(sd["e"], e64)):
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert float((got.double() - want).abs().max()) <= 3 * 4 * 2.0 ** -24 * float(want.abs().max()), i      # 3 one-update bounds
        assert not torch.equal(got, _params(models)[i])
    used = sum(p.numel() for m in models for p in m.parameters())
    assert sum(int((g.e != 0).sum()) for g in tr.groups) <= used < sum(g.n for g in tr.groups), "padding of e stays zero"
    off = optim.Trainer(_build(3), group_mb=0.003)
    assert off.ema_decay is None and all(g.e is None for g in off.groups) and "e" not in off.state_dict()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with off.ema_weights():
            pass
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            optim.Trainer(_build(3), ema_decay=bad)


def test_state_without_e_is_refused_by_a_trainer_with_the_average(optim):
    models = _build(3)
    tr = _trainer(optim, models)
    _steps(tr, models, 2)
    sd = tr.state_dict()
    before = [g.e.clone() for g in tr.groups]
    with pytest.raises(ValueError, match=r"no 'e' vectors.*without the average"):
        tr.load_state_dict({k: v for k, v in sd.items() if k != "e"})
    with pytest.raises(ValueError, match=r"model 1\b.*'e'"):
        tr.load_state_dict(dict(sd, e=[sd["e"][0], sd["e"][1][:-1], sd["e"][2]]))
    assert all(torch.equal(a, g.e) for a, g in zip(before, tr.groups))
    other = _trainer(optim, _build(4), group_mb=100.0)       # one group: another arena layout
    other.load_state_dict(sd)
    back = other.state_dict()
    assert all(torch.equal(a, b) for key in ("m", "v", "e") for a, b in zip(sd[key], back[key]))
    plain = _trainer(optim, _build(4), ema=None)
    plain.load_state_dict(sd)                                # (a trainer without the average ignores 'e')
    assert "e" not in plain.state_dict()


def test_swap_world1_and_its_guards(optim):
    models = _build(3)
    tr = _trainer(optim, models)
    _steps(tr, models, 2)
    live, e = _params(models), tr.state_dict()["e"]
    tr.pack_cache.fresh = tr.pack_cache.epoch
    with tr.ema_weights():
        assert tr.pack_cache.fresh == -1
        assert all(torch.equal(a, b) for a, b in zip(_params(models), e))
        tr.pack_cache.fresh = tr.pack_cache.epoch
        with pytest.raises(RuntimeError, match="nest"):
            with tr.ema_weights():
                pass
        for call in (tr.zero_grad, tr.step, tr.arm_early_step):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
    assert tr.pack_cache.fresh == -1 and tr.t == 2
    assert all(torch.equal(a, b) for a, b in zip(_params(models), live))
    with pytest.raises(KeyError):       # an exception inside the context still puts the live weights back
        with tr.ema_weights():
            raise KeyError("x")
    assert all(torch.equal(a, b) for a, b in zip(_params(models), live))
    _steps(tr, models, 1)               # and training goes on


# ---------------------------------------------------------------------------------------------------- world 2 (gloo)
def _worker(rank, world, port, tmp, zero1, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dpmn_amd.train import optim
        _substitute(optim)
        w1 = torch.load(os.path.join(tmp, "w1.pt"))
        models = _build(3)
        tr = _trainer(optim, models, world=world, zero1=zero1)
        assert tr.zero1 == zero1 and all((g.e.numel() * world == g.n) if zero1 else (g.e.numel() == g.n) for g in tr.groups)
        _steps(tr, models)
        sd = tr.state_dict()
        ok = sd["t"] == 3
        if rank == 0 or not zero1:
            ok = ok and all(torch.equal(a, b) for key in ("m", "v", "e") for a, b in zip(sd[key], w1[key]))
        else:
            ok = ok and sd["e"] is None and sd["m"] is None
        if rank == 0:
            torch.save(sd, os.path.join(tmp, "w2_%d.pt" % int(zero1)))
        # the swap: every rank gets the full averaged parameters, then bit for bit its live ones again
        live = _params(models)
        with tr.ema_weights():
            ok = ok and all(torch.equal(a, b) for a, b in zip(_params(models), w1["e"]))
        ok = ok and all(torch.equal(a, b) for a, b in zip(_params(models), live)) and not torch.equal(live[1], w1["e"][1])
        # a world-1 state loads into this world's shards and comes back out unchanged
        tr_b = _trainer(optim, _build(5), world=world, zero1=zero1)
        tr_b.load_state_dict(w1)
        back = tr_b.state_dict()
        if rank == 0:
            ok = ok and all(torch.equal(a, b) for key in ("m", "v", "e") for a, b in zip(w1[key], back[key]))
        q.put((rank, bool(ok)))
        dist.barrier()
    except Exception:
        import traceback
        traceback.print_exc()
        q.put((rank, False))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("zero1", [False, True])
def test_average_world2_gloo_equals_world1_and_loads_at_either(optim, tmp_path, zero1):
    models1 = _build(3)
    tr1 = _trainer(optim, models1)
    _steps(tr1, models1)
    w1 = tr1.state_dict()
    torch.save(w1, str(tmp_path / "w1.pt"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), zero1, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
    w2 = torch.load(str(tmp_path / ("w2_%d.pt" % int(zero1))))
    tr = _trainer(optim, _build(6), group_mb=100.0)
    tr.load_state_dict(w2)
    back = tr.state_dict()
    for i, (a, b, c) in enumerate(zip(w2["e"], back["e"], w1["e"])):
        assert torch.equal(a, b) and torch.equal(a, c), i
        assert float(a.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------- main.py --ema
def test_main_ema_argument():
    import argparse
    import main as m
    assert m.ema_decay_arg("0.999") == 0.999 and m.ema_decay_arg("0.5") == 0.5
    for bad in ("0", "1", "-0.1", "nan", "1.5", "inf", "x"):
        with pytest.raises(argparse.ArgumentTypeError, match="0 < DECAY < 1"):
            m.ema_decay_arg(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--ema", "nan"], capture_output=True, text=True)
    assert r.returncode == 2 and "error: argument --ema: --ema must be a decay with 0 < DECAY < 1" in r.stderr, r.stderr[-400:]


# ---------------------------------------------------------------------------------------------------- fingerprint
def _args(**kw):
    d = dict(arch="tatt", stu_iter_b1=2, stu_iter_b2=2, sr_share=False, window_num=3, patch_size="2,2,", embed_dim="96,96,", depths="1,1,",
             num_heads="6,6,", window_size="2,4,8,2,4,8,", mlp_ratio="4,4,")
    d.update(kw)
    return SimpleNamespace(**d)


def test_fingerprint_holds_the_decay(tmp_path):
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))
    off, on = base.state_fingerprint(_args(), cfg), base.state_fingerprint(_args(), cfg, ema=0.999)
    assert off["ema"] is None and on["ema"] == 0.999 and "ema" in base.FINGERPRINT_FIELDS and "ema" in base.DATA_FIELDS
    old = {k: v for k, v in off.items() if k != "ema"}           # a state written before the field existed
    base.check_fingerprint(off, off)
    base.check_fingerprint(on, base.state_fingerprint(_args(), cfg, ema=0.999))
    base.check_fingerprint(old, off)                              # ... loads as off
    for saved, current in ((off, on), (on, off), (old, on), (on, base.state_fingerprint(_args(), cfg, ema=0.99))):
        with pytest.raises(ValueError, match=r"\bema = "):
            base.check_fingerprint(saved, current, "state.pt")
    path = str(tmp_path / "state.pt")
    base.write_train_state(path, {"version": base.TRAIN_STATE_VERSION, "fingerprint": on})
    assert base.read_train_state(path, on)["fingerprint"]["ema"] == 0.999      # (survives the weights_only round trip)
    with pytest.raises(ValueError, match=r"\bema = 0.999.*\bema = None"):
        base.read_train_state(path, off)
