"""GPU (-m gpu): ``sharded.ShardedTraining`` through the product path -- the HIP eigensolver, the HIP layer / small / native
kernels, the pair kernels of csrc/train_small.hip around the per-layer all-reduces and the bucket kernels of csrc/optim.hip
around the gradient all-reduce.  Two ranks share cuda:0 over gloo (a one-GPU box; RCCL wants one device per rank), as
tests/test_gpu_sharded.py does; ONE spawn computes what the two-rank tests assert on.

Yardstick: tests/test_training.py's ``check_grads`` against the imported reference's gradients of the WHOLE batch, unchanged,
on every rank; after the bucket all-reduce the ranks are ``torch.equal``.  Figures are printed.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import admm_net_amd as A
from admm_net_amd import sharded

import test_sharded_training_gloo as SG
import test_training as TT

pytestmark = pytest.mark.gpu
ROOT = SG.ROOT
DEV = "cuda:0"
ROUTES = SG.ROUTES


def _worker(rank, world, port, out):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from admm_net_amd import losses, optim, synth
    res = {}
    # ---- the reference's gradients on every rank, every route
    for path, name in zip(TT.CASES, SG.NAMES):
        for route in ROUTES:
            z, m, total, _ = SG.sharded_step(path, route, "global", rank, world, device=DEV, kernels=None, bucket=None)
            key = f"{name}/{route}"
            try:
                TT.check_grads(z, m, total)
                res[key + "/pass"] = 1
            except AssertionError as e:
                res[key + "/pass"] = 0
                res[key + "/why"] = str(e)
            res[key + "/ratio"] = SG.grad_ratio(z, m)
            res[key + "/ranks_equal"] = int(SG.ranks_agree(m))
    # ---- three optimiser steps: the ranks stay in step
    dev = torch.device(DEV)
    torch.manual_seed(3)
    m = A.PhiEstADMMNet(M=4, N=4, num_layers=3).to(dev)
    if rank:                                                    # rank 0's parameters must win
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05)
    m.train()
    m.train_route = "native"
    st = sharded.ShardedTraining(m, scope="global")
    res["steps/broadcast_equal"] = int(SG.ranks_agree_on([p.detach() for p in m.parameters()]))
    y, b, sigma, _ = synth.make_batch(5, 4, 4, seed=5)
    lo, hi = sharded.shard_bounds(5, world, rank)
    ty, tb, ts = (torch.from_numpy(v[lo:hi]).to(dev) for v in (y, b, sigma))
    target = ty / tb
    crit = losses.PhiAlignmentLoss()
    opt = optim.AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    hist, equal, norms = [], [], []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(st(ty, tb, ts), target)[0] * st.weight
        st.backward(loss)
        opt.step()
        total = loss.detach().to(torch.float64).reshape(1).clone()
        dist.all_reduce(total)
        hist.append(float(total))
        equal.append(int(SG.ranks_agree_on([p.detach() for p in m.parameters()])))
        norms.append(float(opt.last_grad_norm))
    res["steps/loss"], res["steps/params_equal"], res["steps/grad_norm"] = hist, equal, norms
    res["steps/weight"] = st.weight
    # ---- the harness's train-step inside a process group: --batch stays the per-rank batch
    from admm_net_amd import harness
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0")
    line = harness.time_train_step(layers=2, batch=3, steps=1, warmup=1, route="native", grid=(4, 4), optim="hip")
    res["harness"] = [line["n_ranks"], line["global_batch"], line["batch"], int(np.isfinite(line["loss_last"]))]
    np.savez(f"{out}.{rank}.npz", **{k: np.asarray(v) for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gpu_sharded_training") / "res")
    port = 29800 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    return [np.load(f"{out}.{r}.npz") for r in range(2)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SG.NAMES)
def test_two_ranks_give_the_reference_gradients(two_ranks, name, route):
    for rank, r in enumerate(two_ranks):
        key = f"{name}/{route}"
        print(f"rank {rank} {key}: worst gradient error / tolerance {float(r[key + '/ratio']):.3f}")
        assert int(r[key + "/pass"]) == 1, str(r[key + "/why"]) if key + "/why" in r.files else ""
        assert int(r[key + "/ranks_equal"]) == 1, "the ranks hold different gradients after the bucket all-reduce"


@pytest.mark.timeout(300)
def test_ranks_stay_in_step_over_optimiser_steps(two_ranks):
    """Three steps of optim.AdamW(lr=1e-3, max_grad_norm=1.0) on PhiEstADMMNet 4 x 4, K = 3, B = 5 (3 + 2) under
    PhiAlignmentLoss x st.weight: the parameters of the ranks are torch.equal after the broadcast and after every step, the
    clipping sees the same norm, and the loss of the whole batch falls."""
    a, b = two_ranks
    print("loss of the whole batch per step:", a["steps/loss"].tolist(), "gradient norms:", a["steps/grad_norm"].tolist())
    assert float(a["steps/weight"]) == 3 / 5 and float(b["steps/weight"]) == 2 / 5
    for r in two_ranks:
        assert int(r["steps/broadcast_equal"]) == 1
        assert r["steps/params_equal"].tolist() == [1, 1, 1]
        assert np.isfinite(r["steps/loss"]).all() and r["steps/loss"][2] < r["steps/loss"][0]
    assert a["steps/grad_norm"].tolist() == b["steps/grad_norm"].tolist() and np.isfinite(a["steps/grad_norm"]).all()
    assert a["steps/loss"].tolist() == b["steps/loss"].tolist()


@pytest.mark.timeout(300)
def test_harness_train_step_runs_sharded_under_a_process_group(two_ranks):
    for r in two_ranks:
        assert r["harness"].tolist() == [2, 6, 3, 1]             # n_ranks, global_batch, the per-rank batch, a finite loss


@pytest.mark.parametrize("route", ROUTES)
def test_world_size_one_is_the_plain_path(route):
    """No process group: the output and every gradient ``torch.equal`` to ``model.forward_autograd`` + ``backward``."""
    assert not dist.is_initialized()
    for path in TT.CASES:
        runs = []
        for through in (False, True):
            z, m, head, t = TT.load(path, DEV)
            m.eval()
            m.train_route = route
            if through:
                st = sharded.ShardedTraining(m)
                out = st(t("y"), t("b"), t("sigma"))
                assert st.weight == 1.0
                st.backward(TT.loss_of(out, t, head) * st.weight)
            else:
                out = m.forward_autograd(t("y"), t("b"), t("sigma"))
                TT.loss_of(out, t, head).backward()
            runs.append(([o.detach() for o in out] if head else [out.detach()], [p.grad for p in m.parameters()]))
        (out_a, g_a), (out_b, g_b) = runs
        assert all(torch.equal(x, y) for x, y in zip(out_a, out_b)), path
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(g_a, g_b)), path
