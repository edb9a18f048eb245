"""Stop and continue under data parallelism: two gloo ranks sharing ONE MI355X (as tests/test_gpu_dp.py: RCCL refuses two ranks on
a device, the exchange logic is backend-independent), ZeRO-1, per-rank batches and per-rank random streams.  A world-2 run stopped at
it = 2 and continued to it = 4 from its state file ends with the parameters (both ranks) and the gathered Adam moments (rank 0) of
the world-2 run that was never stopped; the same file then loads at world 1 with every weight and moment as saved."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

B, B1, B2 = 2, 2, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mission(out_dir, rank):
    from dpmn_amd import workload
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.utils import synth

    class Filled(TextSR):
        def build_training(self, world_size=1, group=None):
            out = super().build_training(world_size, group)
            models, psn, distill = out[0], out[1], out[2]
            for i, m in enumerate([psn] + models + distill):      # (the same on every rank; views of the trainer's arena, written in place)
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
    sr = Filled(cfg, workload.make_args("tatt", B1, B2, B, drop=0.1))
    sr.vis_dir = out_dir
    sr.rank_seed = 2 + rank          # as main.py: the ranks' random streams diverge once the replicas are built
    return sr


def _loader_of(rank, world):
    """DistributedSampler-style: batch j of an epoch is split over the ranks; 3 batches per epoch"""
    from dpmn_amd.utils import synth

    def loader(epoch):
        for j in range(3):
            b = synth.synth_batch(B * world, seed=80 + 3 * epoch + j)
            lo = rank * B
            yield b["images_hr"][lo:lo + B], b["images_lr"][lo:lo + B], b["label_vecs"][lo:lo + B]
    return loader


def _snapshot(sr, models, distill):
    torch.cuda.synchronize()
    return ([{k: v.detach().cpu().clone() for k, v in m.named_parameters()} for m in models + distill], sr.trainer.state_dict())


def _worker(rank, world, port, tmp, mode, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dpmn_amd import _abi
        _abi.check(_abi.lib.dpmn_set_compute_dtype(mode))
        loader = _loader_of(rank, world)
        state = os.path.join(tmp, "state.pt")
        torch.manual_seed(1)
        np.random.seed(1)
        sr = _mission(os.path.join(tmp, "a%d" % rank), rank)
        pa, ta = _snapshot(sr, *sr.train(loader, steps=4, epochs=2))
        assert sr.trainer.zero1 and sr.trainer.world == 2
        torch.manual_seed(1)
        np.random.seed(1)
        sr = _mission(os.path.join(tmp, "b%d" % rank), rank)
        sr.train(loader, steps=2, epochs=2, state_path=state)
        dist.barrier()               # (rank 0 wrote the file)
        torch.manual_seed(99)
        np.random.seed(99)
        sr = _mission(os.path.join(tmp, "b%d" % rank), rank)
        sr.rank_seed = 77 + rank
        pb, tb = _snapshot(sr, *sr.train(loader, steps=4, epochs=2, state_path=state))
        nd_p = sum(int((x[k] != y[k]).sum()) for x, y in zip(pa, pb) for k in x)
        nd_mv = -1
        if rank == 0:
            nd_mv = sum(int((x != y).sum()) for key in ("m", "v") for x, y in zip(ta[key], tb[key]))
            assert sum(float(x.abs().sum()) for x in ta["m"]) > 0
        else:
            assert ta["m"] is None and tb["m"] is None
        q.put((rank, nd_p, nd_mv, ta["t"], tb["t"], sr.loop_state["it"]))
        dist.barrier()
    except Exception:      # report instead of leaving the parent waiting for the queue
        import traceback
        traceback.print_exc()
        q.put((rank, -1, -1, -1, -1, -1))
    finally:
        dist.destroy_process_group()


def test_world2_zero1_stop_and_continue_then_load_at_world1(tmp_path):
    from dpmn_amd import _abi
    from dpmn_amd.interfaces import base
    from helpers import record
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    mode = _abi.lib.dpmn_get_compute_dtype()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), mode, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, nd_p, nd_mv, t_a, t_b, it in sorted(res):
        assert (t_a, t_b, it) == (4, 4, 4), (rank, t_a, t_b, it)
        record("train_state_dp_world2", "rank %d parameter words differing after stop and continue" % rank, nd_p, 0)
        assert nd_p == 0, (rank, nd_p)
        if rank == 0:
            record("train_state_dp_world2", "rank 0 gathered Adam moment words differing after stop and continue", nd_mv, 0)
            assert nd_mv == 0, nd_mv
    # the file the world-2 run left loads at world 1: weights through the state_dicts, moments into the one-rank groups
    sr = _mission(str(tmp_path / "w1"), 0)
    state = base.read_train_state(str(tmp_path / "state.pt"), base.state_fingerprint(sr.args, sr.config))
    assert state["world"] == 2 and len(state["rng"]) == 2 and state["loop"]["it"] == 4
    models, psn, distill, crit, trainer = sr.build_training()
    for m, sd in zip(models + distill, state["models"] + state["distill"]):
        m.load_state_dict(sd)
    trainer.load_state_dict(state["trainer"])
    assert trainer.t == 4 and not trainer.zero1
    back = trainer.state_dict()
    for key in ("m", "v"):
        assert len(back[key]) == len(models + distill)
        for i, (x, y) in enumerate(zip(state["trainer"][key], back[key])):
            assert torch.equal(x, y), (key, i)
    for i, (m, sd) in enumerate(zip(models + distill, state["models"] + state["distill"])):
        for k, v in m.state_dict().items():
            assert torch.equal(v.cpu(), sd[k]), (i, k)
    # ... and sit, per parameter, where this trainer's own layout keeps them
    for i, slices in enumerate(trainer._moment_layout()):
        a = 0
        for gi, o, k in slices:
            assert torch.equal(trainer.groups[gi].m[o:o + k].cpu(), state["trainer"]["m"][i][a:a + k])
            a += k
