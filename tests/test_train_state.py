"""Training state on the CPU (dpmn_amd/train/optim.py Trainer.state_dict / load_state_dict, interfaces/base.py write_train_state /
read_train_state): the saved Adam state does not depend on world size, group plan or padding; the file is replaced atomically;
mismatches raise errors that name what differs.  The two optimizer kernels are GPU-only in the product; as in test_dp_gloo.py a
torch restatement is injected so the layout logic can be checked without one."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


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


@pytest.fixture(autouse=True)
def _torch_optimizer_kernels(monkeypatch):
    """in the pytest process the substitution ends with the test (the spawned children set it for their lifetime)"""
    from dpmn_amd.train import optim
    monkeypatch.setattr(optim, "_sumsq", _torch_sumsq)
    monkeypatch.setattr(optim, "_adam_clip", _torch_adam_clip)


def _trainer(optim, models, world=1, zero1=None, group_mb=0.003):
    return optim.Trainer(models, lr=1e-2, beta1=0.5, max_norm=0.25, world_size=world, zero1=zero1, group_mb=group_mb)


def _two_steps(tr, models, rank=0):
    for step in range(2):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * step + rank))
        tr.zero_grad()
        _loss(models, x).backward()
        tr.step()
    tr.sync_params()


def _per_param(tr):
    """{(model index, parameter index): (m, v)} read straight from the groups of a world-1 trainer"""
    out = {}
    for i, slices in enumerate(tr._moment_layout()):
        for j, (gi, o, k) in enumerate(slices):
            g = tr.groups[gi]
            assert g.shard_n == g.n
            out[(i, j)] = (g.m[o:o + k].clone(), g.v[o:o + k].clone())
    return out


def _assert_same_moments(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key][0], b[key][0]) and torch.equal(a[key][1], b[key][1]), key
        assert float(a[key][1].abs().sum()) > 0, "the moments are all zero: nothing was trained"


def test_trainer_state_round_trip_between_group_plans():
    from dpmn_amd.train import optim
    models = _build(3)
    tr = _trainer(optim, models, group_mb=0.003)
    assert len(tr.groups) >= 2, "several exchange groups"
    assert tr.flat_p.numel() > sum(p.numel() for m in models for p in m.parameters()), "the arenas are padded"
    _two_steps(tr, models)
    sd = tr.state_dict()
    assert sd["t"] == 2 and len(sd["m"]) == len(sd["v"]) == 3
    for i, m in enumerate(models):
        n = sum(p.numel() for p in m.parameters())
        assert sd["m"][i].shape == (n,) and sd["v"][i].shape == (n,) and sd["m"][i].dtype == torch.float32
    models2 = _build(4)
    tr2 = _trainer(optim, models2, group_mb=100.0)      # ONE group: another arena layout
    assert len(tr2.groups) == 1 and len(tr.groups) != len(tr2.groups)
    tr2.pack_cache.fresh = tr2.pack_cache.epoch
    tr2.load_state_dict(sd)
    assert tr2.t == 2 and tr2.pack_cache.fresh != tr2.pack_cache.epoch
    _assert_same_moments(_per_param(tr), _per_param(tr2))
    sd2 = tr2.state_dict()
    for key in ("m", "v"):
        for a, b in zip(sd[key], sd2[key]):
            assert torch.equal(a, b)


def _zero1_worker(rank, world, port, tmp, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dpmn_amd.train import optim
        optim._sumsq, optim._adam_clip = _torch_sumsq, _torch_adam_clip
        # (a) train two steps under ZeRO-1 at world 2, save collectively: the vectors are left on rank 0
        models = _build(3)
        tr = _trainer(optim, models, world=world, zero1=True)
        assert tr.zero1 and all(g.shard_n * world == g.n for g in tr.groups)
        _two_steps(tr, models, rank)
        sd = tr.state_dict()
        # (what each rank really holds, written without any collective: the parent rebuilds the vectors from these shards)
        torch.save([(g.lo, g.m.clone(), g.v.clone()) for g in tr.groups], os.path.join(tmp, "shards%d.pt" % rank))
        if rank == 0:
            torch.save(sd, os.path.join(tmp, "w2.pt"))
            torch.save(tr._moment_layout(), os.path.join(tmp, "layout.pt"))
        else:
            assert sd["m"] is None and sd["v"] is None and sd["t"] == 2
        dist.barrier()
        # (b) a state saved at world 1 loads into the ZeRO-1 shards of world 2 and comes back out unchanged
        w1 = torch.load(os.path.join(tmp, "w1.pt"))
        tr_b = _trainer(optim, _build(5), world=world, zero1=True)
        tr_b.load_state_dict(w1)
        back = tr_b.state_dict()
        ok = tr_b.t == w1["t"]
        if rank == 0:
            ok = ok and all(torch.equal(a, b) for key in ("m", "v") for a, b in zip(w1[key], back[key]))
        q.put((rank, bool(ok)))
        dist.barrier()
    except Exception:
        import traceback
        traceback.print_exc()
        q.put((rank, False))
    finally:
        dist.destroy_process_group()


def test_trainer_state_world2_zero1_to_world1_and_back(tmp_path):
    from dpmn_amd.train import optim
    # the world-1 state the children load: two steps on rank 0's batches
    models1 = _build(3)
    tr1 = _trainer(optim, models1)
    _two_steps(tr1, models1)
    w1 = tr1.state_dict()
    torch.save(w1, str(tmp_path / "w1.pt"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_zero1_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
    # world 2 -> world 1: the gathered vectors land, per parameter, in a one-group world-1 trainer and come back out bitwise
    w2 = torch.load(str(tmp_path / "w2.pt"))
    shards = [torch.load(str(tmp_path / ("shards%d.pt" % r))) for r in range(2)]
    layout = torch.load(str(tmp_path / "layout.pt"))
    for key, which in (("m", 1), ("v", 2)):
        groups = [torch.cat([shards[r][gi][which] for r in range(2)]) for gi in range(len(shards[0]))]      # rank r owns [r * shard_n, (r + 1) * shard_n)
        for i, slices in enumerate(layout):
            assert torch.equal(w2[key][i], torch.cat([groups[gi][o:o + k] for gi, o, k in slices])), (key, i)
    assert all(shards[1][gi][0] == shards[0][gi][1].numel() for gi in range(len(shards[0])))
    tr = _trainer(optim, _build(6), group_mb=100.0)
    tr.load_state_dict(w2)
    assert tr.t == 2
    back = tr.state_dict()
    for key in ("m", "v"):
        for i, (a, b) in enumerate(zip(w2[key], back[key])):
            assert torch.equal(a, b), (key, i)
            assert float(a.abs().sum()) > 0
    got = _per_param(tr)
    for (i, j), (m, v) in got.items():
        sizes = [p.numel() for p in tr.buckets[i].module.parameters()]
        a = sum(sizes[:j])
        assert torch.equal(m, w2["m"][i][a:a + sizes[j]]) and torch.equal(v, w2["v"][i][a:a + sizes[j]])


def test_moment_length_and_model_count_mismatch_name_the_model():
    from dpmn_amd.train import optim
    models = _build(3)
    tr = _trainer(optim, models)
    _two_steps(tr, models)
    sd = tr.state_dict()
    before = _per_param(tr)
    bad = dict(sd, v=[sd["v"][0], sd["v"][1][:-1], sd["v"][2]])
    n1 = sd["v"][1].numel()
    with pytest.raises(ValueError, match=r"model 1\b.*\b%d\b.*\b%d\b" % (n1 - 1, n1)):
        tr.load_state_dict(bad)
    with pytest.raises(ValueError, match=r"holds 2 'm' vectors.*3 models"):
        tr.load_state_dict(dict(sd, m=sd["m"][:2]))
    _assert_same_moments(before, _per_param(tr))       # a refused state changed nothing


def _args(**kw):
    d = dict(arch="tatt", stu_iter_b1=2, stu_iter_b2=2, sr_share=False, window_num=3, patch_size="2,2,", embed_dim="96,96,", depths="1,1,",
             num_heads="6,6,", window_size="2,4,8,2,4,8,", mlp_ratio="4,4,")
    d.update(kw)
    return SimpleNamespace(**d)


def _config(h=32, w=128):
    return SimpleNamespace(TRAIN=SimpleNamespace(height=h, width=w))


def _state(fp):
    from dpmn_amd.interfaces import base
    return {"version": base.TRAIN_STATE_VERSION, "fingerprint": fp, "payload": torch.arange(5)}


def test_fingerprint_mismatch_names_the_field(tmp_path):
    from dpmn_amd.interfaces import base
    path = str(tmp_path / "state.pt")
    fp = base.state_fingerprint(_args(), _config())
    assert set(fp) == set(base.FINGERPRINT_FIELDS)
    base.write_train_state(path, _state(fp))
    assert torch.equal(base.read_train_state(path, fp)["payload"], torch.arange(5))
    for field, other in (("stu_iter_b1", base.state_fingerprint(_args(stu_iter_b1=3), _config())),
                         ("arch", base.state_fingerprint(_args(arch="tsrn"), _config())),
                         ("embed_dim", base.state_fingerprint(_args(embed_dim="96,48,"), _config())),
                         ("sr_share", base.state_fingerprint(_args(sr_share=True), _config())),
                         ("width", base.state_fingerprint(_args(), _config(w=256)))):
        with pytest.raises(ValueError, match=r"\b%s = " % field):
            base.read_train_state(path, other)
    base.write_train_state(path, dict(_state(fp), version=base.TRAIN_STATE_VERSION + 1))
    with pytest.raises(ValueError, match="format version"):
        base.read_train_state(path, fp)


def test_failed_save_leaves_the_previous_state_and_stray_tmp_is_ignored(tmp_path, monkeypatch):
    from dpmn_amd.interfaces import base
    path = str(tmp_path / "state.pt")
    fp = base.state_fingerprint(_args(), _config())
    base.write_train_state(path, _state(fp))
    assert not os.path.exists(path + ".tmp")
    good = open(path, "rb").read()
    opened = []

    def dying_save(obj, f, *a, **k):
        opened.append(f.name)
        f.write(b"half a sta")
        f.flush()
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(OSError, match="disk full"):
        base.write_train_state(path, dict(_state(fp), payload=torch.arange(7)))
    monkeypatch.undo()
    assert opened == [path + ".tmp"] and os.path.getsize(path + ".tmp") > 0      # the failure happened inside the temp file, in the same directory
    assert open(path, "rb").read() == good
    assert torch.equal(base.read_train_state(path, fp)["payload"], torch.arange(5))      # the stray .tmp beside it is not looked at
    base.write_train_state(path, dict(_state(fp), payload=torch.arange(7)))               # ... and the next save replaces both
    assert torch.equal(base.read_train_state(path, fp)["payload"], torch.arange(7)) and not os.path.exists(path + ".tmp")


def test_rng_capture_restore_replays_every_stream():
    import random
    import numpy as np
    from dpmn_amd.interfaces import base
    torch.manual_seed(5)
    np.random.seed(5)
    random.seed(5)
    np.random.randn(3)          # (leaves a cached gaussian in numpy's state)
    st = base.rng_capture()
    st = torch.load(_roundtrip(st), weights_only=True)
    draw = lambda: (torch.randint(0, 2 ** 62, (4,)).tolist(), np.random.rand(3).tolist(), float(np.random.randn()), random.random(), random.gauss(0, 1))
    first = draw()
    assert draw() != first
    base.rng_restore(st)
    assert draw() == first


def _roundtrip(obj):
    import io
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return buf
