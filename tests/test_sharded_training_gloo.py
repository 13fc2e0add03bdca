"""CPU, world size 2 over gloo: ``sharded.ShardedTraining`` -- an optimisation step on a batch split across ranks with the
gradients of the whole batch.  The ranks run the differentiable forward with the Torch stand-ins (``torch.linalg.eigh``,
``TorchAssembler``, ``TorchLayerKernels``, ``TorchSmallKernels``, ``TorchNativeKernels``, ``TorchBucketKernels``), so what is
verified is the product's protocol and autograd wiring: the per-layer coupling through the batch mean in the forward AND the
backward, the one-bucket gradient all-reduce, the collective counts and the argument checks.

Yardstick: tests/test_training.py's ``check_grads`` (5e-4 max|grad| + 1e-6 per parameter against the imported reference's
gradients on the WHOLE batch, ``none:`` parameters None), unchanged, on every rank.  ``scope="shard"`` (DistributedDataParallel's
semantics: every rank its own mean) must FAIL it: that is why the feature exists.  Worst figures are printed.

One spawn of two ranks computes everything the world-size-2 tests assert on.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from admm_net_amd import sharded, training

import test_training as TT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ROUTES = ("tensor", "fused", "full", "native")
TSK = training.TorchSmallKernels
KERNELS = dict(solver=TT.cpu_eigh, assembler=training.TorchAssembler, layer_kernels=training.TorchLayerKernels,
               small_kernels=TSK, native_kernels=training.TorchNativeKernels)
NAMES = [os.path.basename(p)[:-4] for p in TT.CASES]
B4 = next(p for p in TT.CASES if "phiest_4x4_K3" in p)          # the B = 4, K = 3 fixture


def grad_ratio(z, m):
    """worst |grad - reference| / (5e-4 max|reference| + 1e-6) over the parameters: ``check_grads``' criterion as a number."""
    worst = 0.0
    for name, p in m.named_parameters():
        if "none:" + name in z.files:
            continue
        want = z["g:" + name]
        worst = max(worst, float(np.abs(p.grad.detach().cpu().numpy() - want).max() / (TT.RTOL * np.abs(want).max() + 1e-6)))
    return worst


def sharded_step(path, route, scope, rank, world, device="cpu", kernels=KERNELS, bucket=sharded.TorchBucketKernels, sub_batch=None,
                 bounds=None, after=lambda: None):
    """One ``ShardedTraining`` step on this rank's shard of a gradient fixture under the fixture's own loss (a SUM over signals:
    weight 1).  Returns (z, model, the all-reduced loss, st)."""
    z, m, head, t = TT.load(path, device)
    m.eval()                                                    # fixture convention: dropout off
    m.train_route, m.sub_batch = route, sub_batch
    lo, hi = bounds or sharded.shard_bounds(int(z["meta"][3]), world, rank, sub_batch)
    tl = lambda k: t(k)[lo:hi]
    st = sharded.ShardedTraining(m, scope=scope, kernels=kernels, bucket=bucket)
    out = st(tl("y"), tl("b"), tl("sigma"))
    after()                                                     # (the forward, then the backward: the tests count collectives)
    loss = TT.loss_of(out, tl, head)
    st.backward(loss)
    after()
    total = loss.detach().to(torch.float64).reshape(1).clone()
    dist.all_reduce(total)
    return z, m, total, st


def ranks_agree_on(tensors):
    """The tensors of the list are ``torch.equal`` on all ranks."""
    flat = torch.cat([t.reshape(-1) for t in tensors])
    both = [torch.empty_like(flat) for _ in range(dist.get_world_size())]
    dist.all_gather(both, flat)
    return all(torch.equal(both[0], o) for o in both[1:])


def ranks_agree(m):
    """The gradients of all ranks are ``torch.equal`` (the same parameters have one: the lists have the same length)."""
    return ranks_agree_on([p.grad for p in m.parameters() if p.grad is not None])


def _worker(rank, world, port, out):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_num_threads(2)
    res = {}
    for path, name in zip(TT.CASES, NAMES):
        for route, scope in [(r, "global") for r in ROUTES] + [("tensor", "shard")]:
            z, m, total, _ = sharded_step(path, route, scope, rank, world)
            key = f"{name}/{route}/{scope}"
            try:
                TT.check_grads(z, m, total)
                res[key + "/pass"] = 1
            except AssertionError as e:
                res[key + "/pass"] = 0
                res[key + "/why"] = str(e)
            res[key + "/ratio"] = grad_ratio(z, m)
            res[key + "/loss"] = float(total)
            res[key + "/ranks_equal"] = int(ranks_agree(m))
            res[key + "/none_kept"] = int(all(p.grad is None for n, p in m.named_parameters() if "none:" + n in z.files))
    # collective counts: a wrapper around all_reduce as the product calls it
    calls, plain = [], dist.all_reduce

    def counting(t, *a, **k):
        calls.append(t.numel())
        return plain(t, *a, **k)

    K = int(np.load(B4)["meta"][2])
    for route in ROUTES:
        for sub_batch in (2, None):
            for scope in ("global", "shard"):
                del calls[:]
                mark = []
                dist.all_reduce = counting
                try:
                    sharded_step(B4, route, scope, rank, world, sub_batch=sub_batch, after=lambda: mark.append(len(calls)))
                finally:
                    dist.all_reduce = plain
                res[f"count/{route}/{sub_batch}/{scope}"] = [mark[0], mark[1] - mark[0]]
    res["K"] = K
    # errors: an empty shard, a shard that starts inside a sub-batch
    for what, sub_batch, bounds in (("empty", None, [(0, 4), (4, 4)]), ("misaligned", 2, [(0, 1), (1, 4)])):
        try:
            sharded_step(B4, "tensor", "global", rank, world, sub_batch=sub_batch, bounds=bounds[rank])
            res["error/" + what] = "no error"
        except ValueError as e:
            res["error/" + what] = "ValueError: " + str(e)
    np.savez(f"{out}.{rank}.npz", **{k: np.asarray(v) for k, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sharded_training") / "res")
    port = 29700 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    return [np.load(f"{out}.{r}.npz") for r in range(2)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_global_scope_gives_the_reference_gradients_on_every_rank(two_ranks, name, route):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    for rank, r in enumerate(two_ranks):
        key = f"{name}/{route}/global"
        print(f"rank {rank} {key}: worst gradient error / tolerance {float(r[key + '/ratio']):.3f}, loss {float(r[key + '/loss']):.6f}")
        assert int(r[key + "/pass"]) == 1, str(r[key + "/why"]) if key + "/why" in r.files else ""
        assert abs(float(r[key + "/loss"]) - float(z["loss"])) <= 1e-4 * max(1.0, abs(float(z["loss"])))
        assert int(r[key + "/none_kept"]) == 1, "a parameter the reference leaves at None received a gradient"
        assert int(r[key + "/ranks_equal"]) == 1, "the ranks hold different gradients after the bucket all-reduce"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", NAMES)
def test_shard_scope_is_another_network(two_ranks, name):
    """Teeth: every rank its own mean (what DistributedDataParallel computes) misses the criterion ``scope="global"`` meets.
    Measured: worst error / tolerance 14 (phiest_4x4_K3_perturbed), 268 (phiest_10x10_K4_default), 315 (admmnet_3x4_K3_perturbed)."""
    for rank, r in enumerate(two_ranks):
        ratio = float(r[f"{name}/tensor/shard/ratio"])
        print(f"rank {rank} {name} scope=shard: worst gradient error / tolerance {ratio:.1f}")
        assert ratio > 1.0
        assert int(r[f"{name}/tensor/shard/pass"]) == 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", ROUTES)
def test_collective_counts(two_ranks, route):
    """[all-reduces in the forward, in the backward].  Aligned sub-batches: the bucket alone, in either scope.  One batch,
    scope="global": K - 1 pairs in the forward, K - 1 scalars and the bucket in the backward; scope="shard": the bucket alone."""
    for r in two_ranks:
        K = int(r["K"])
        assert r[f"count/{route}/2/global"].tolist() == [0, 1]
        assert r[f"count/{route}/2/shard"].tolist() == [0, 1]
        assert r[f"count/{route}/None/global"].tolist() == [K - 1, K]
        assert r[f"count/{route}/None/shard"].tolist() == [0, 1]


@pytest.mark.timeout(300)
def test_empty_and_misaligned_shards_raise_on_every_rank(two_ranks):
    for r in two_ranks:
        assert str(r["error/empty"]).startswith("ValueError") and "at least one signal" in str(r["error/empty"])
        assert str(r["error/misaligned"]).startswith("ValueError") and "inside a sub-batch" in str(r["error/misaligned"])


# ------------------------------------------------------------------------------------------------ no process group
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("path", TT.CASES, ids=NAMES)
def test_without_a_process_group_it_is_the_plain_path(path, route):
    assert not dist.is_initialized()
    grads = []
    for through in (False, True):
        z, m, head, t = TT.load(path)
        m.eval()
        m.train_route = route
        if through:
            st = sharded.ShardedTraining(m, kernels=KERNELS, bucket=None)      # the HIP bucket would raise on host tensors: never called
            out = st(t("y"), t("b"), t("sigma"))
            assert st.weight == 1.0 and st.global_batch == int(z["meta"][3])
            st.backward(TT.loss_of(out, t, head) * st.weight)
        else:
            out = training.unrolled_forward(m, t("y"), t("b"), t("sigma"), **training.route_kwargs(route, KERNELS))
            TT.loss_of(out, t, head).backward()
        grads.append(([o.detach() for o in out] if head else [out.detach()], [p.grad for p in m.parameters()]))
    (out_a, g_a), (out_b, g_b) = grads
    assert all(torch.equal(a, b) for a, b in zip(out_a, out_b))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g_a, g_b))


# ------------------------------------------------------------------------------------------------ the stand-in formulas, float64
@pytest.mark.parametrize("split", [3, 1], ids=["3+4", "1+6"])
def test_pair_formulas_on_two_parts_equal_the_whole_batch(split):
    """``stepsize_pair`` and ``bwd_pair_front`` -> sum of the two totals -> ``bwd_pair_back`` on the two parts of B = 7, with the
    pair of the whole batch, against ``stepsize`` / ``stepsize_bwd`` on the whole batch: elementwise within 1e-12 of the largest
    entry, the parameter sums within 1e-12 sum|terms| (tests/test_training_small.py's level for these formulas)."""
    F64 = torch.float64
    g = torch.Generator().manual_seed(70 + split)
    B, knorm = 7, 0.3
    rn, up = torch.rand(B, dtype=F64, generator=g) * 4 + 0.1, torch.randn(B, dtype=F64, generator=g)
    rho = torch.rand((), dtype=F64, generator=g) * 2 - 0.5
    net = nn.Sequential(nn.Linear(3, 32), nn.ReLU(), nn.Linear(32, 1), nn.Sigmoid()).to(F64)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, dtype=F64, generator=g) * 0.7)
    pars = [p.detach() for p in training._net_params(net)]
    parts = [slice(0, split), slice(split, B)]
    pair = sum(TSK.rnsum(rn[s]) for s in parts)
    assert pair.dtype == F64 and pair[1].item() == B

    def close(got, want, scale, name):
        err = (got - want).abs().max().item()
        print(f"  {name}: error {err:.3e}, scale {scale:.3e}")
        assert got.shape == want.shape and err <= 1e-12 * scale, f"{name}: {err:.3e} against {scale:.3e}"

    step = TSK.stepsize(rn, rho, *pars, knorm)
    close(torch.cat([TSK.stepsize_pair(rn[s], pair, rho, *pars, knorm) for s in parts]), step, step.abs().max().item(), "step")
    whole = TSK.stepsize_bwd(up, rn, rho, *pars, knorm)
    terms = TSK.stepsize_terms(up, rn, rho, *pars, knorm)
    fronts = [TSK.stepsize_bwd_pair_front(up[s], rn[s], pair, rho, *pars, knorm) for s in parts]
    total = fronts[0][1] + fronts[1][1]
    g_rn = torch.cat([TSK.stepsize_bwd_pair_back(f[0], pair, total) for f in fronts])
    g_u = torch.cat([f[0] for f in fronts])
    # g_rn is a difference of two parts that nearly cancel in a small group: its scale is the direct part's (tests/test_training_small.py)
    mean = pair[0] / pair[1]
    close(g_rn, whole[0], max(whole[0].abs().max().item(), (g_u / (mean + training.EPS)).abs().max().item()), "g_rn")
    for i, name in enumerate(("g_rho", "gW1", "gb1", "gW2", "gb2"), start=1):
        got = fronts[0][i + 1] + fronts[1][i + 1]
        mag = terms[i].abs().sum(dim=0).reshape(got.shape)
        err = ((got - whole[i]).abs() / (1e-12 * mag + 1e-300)).max().item()
        print(f"  {name}: error / (1e-12 sum|terms|) = {err:.3f}")
        assert got.shape == whole[i].shape and err <= 1.0, name
