"""CPU: independent sub-batches (``sub_batch = g``) on the host side -- the differentiable training route with the CPU
stand-ins of tests/test_training.py, the group-aligned shard split, the grouped sharding protocol over gloo with a
test-local engine, and the validation of the knob in Python and in the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import admm_net_amd as A
from admm_net_amd import _lib, sharded, synth, training
from oracle import admm_net_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cpu_eigh(Amat):
    return torch.linalg.eigh(Amat)


def _model(Nb, Nd, K, seed, head=True):
    sd = R.make_weights(Nb, Nd, K, seed=seed, head=head, perturb=0.3)
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, num_layers=K)
    m.load_state_dict(sd)
    return m.eval(), sd


def _inputs(B, Nb, Nd, seed):
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=seed)
    return torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)


def _loss(out, B, seed):
    """A fixed random linear functional of every output, so that every output carries gradient."""
    g = torch.Generator().manual_seed(seed)
    tau, f, conf, phi = out
    c_phi = torch.randn(phi.shape, dtype=torch.complex64, generator=g)
    return ((c_phi.conj() * phi).real.sum() + (torch.randn(tau.shape, generator=g) * tau).sum()
            + (torch.randn(f.shape, generator=g) * f).sum() + (torch.randn(conf.shape, generator=g) * conf).sum())


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


@pytest.mark.parametrize("B,g", [(11, 4), (9, 1), (10, 5)])
def test_training_route_groups_equal_separate_batches(B, g):
    """Outputs of one grouped call equal the per-group calls; the gradients equal the sum of the per-group graphs'
    gradients (gradient accumulation over those batches)."""
    Nb, Nd, K = 3, 4, 3
    m, _ = _model(Nb, Nd, K, seed=21)
    y, b, s = _inputs(B, Nb, Nd, seed=5)
    kw = dict(solver=_cpu_eigh, assembler=training.TorchAssembler)

    m.zero_grad(set_to_none=True)
    out = training.unrolled_forward(m, y, b, s, sub_batch=g, **kw)
    _loss(out, B, 1).backward()
    got = _grads(m)

    m.zero_grad(set_to_none=True)
    parts = []
    for lo in range(0, B, g):
        parts.append(training.unrolled_forward(m, y[lo:lo + g], b[lo:lo + g], s[lo:lo + g], **kw))
    sep = tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    _loss(sep, B, 1).backward()       # (the same functional: the sum over groups of each group's loss)
    want = _grads(m)

    for a, r in zip(out, sep):
        assert (a - r).abs().max() <= 1e-6 * r.abs().max()
    for name, w in want.items():
        if w is None:
            assert got[name] is None, name
            continue
        assert (got[name] - w).abs().max() <= 1e-5 * w.abs().max() + 1e-7, name

    # the groups really are independent batches: one mean over the whole call gives other outputs
    whole = training.unrolled_forward(m, y, b, s, **kw)
    assert (whole[3] - sep[3]).abs().max() > 1e-5 * sep[3].abs().max()


def test_training_route_one_group_is_the_default():
    Nb, Nd, K, B = 2, 3, 3, 6
    m, _ = _model(Nb, Nd, K, seed=4, head=False)
    y, b, s = _inputs(B, Nb, Nd, seed=2)
    kw = dict(solver=_cpu_eigh, assembler=training.TorchAssembler)
    ref = training.unrolled_forward(m, y, b, s, **kw)
    for g in (B, B + 1, 1000):
        assert torch.equal(training.unrolled_forward(m, y, b, s, sub_batch=g, **kw), ref)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, b, s, sub_batch=0, **kw)


def test_shard_bounds_cut_at_group_boundaries():
    for total in list(range(0, 40)) + [255, 256, 257, 1100, 65536]:
        for world in (1, 2, 3, 4, 7, 8):
            assert [sharded.shard_bounds(total, world, r, sub_batch=None) for r in range(world)] == \
                   [sharded.shard_bounds(total, world, r) for r in range(world)]
            for g in (1, 2, 3, 5, 7, 64, 256, 600):
                bounds = [sharded.shard_bounds(total, world, r, sub_batch=g) for r in range(world)]
                assert bounds[0][0] == 0 and bounds[-1][1] == total
                ngroups = -(-total // g)
                counts = []
                for r, (lo, hi) in enumerate(bounds):
                    assert lo <= hi
                    if r:
                        assert lo == bounds[r - 1][1]          # contiguous, in rank order
                    if hi > lo:
                        assert lo % g == 0                     # every non-empty shard starts a group
                        assert hi % g == 0 or hi == total      # ... and ends one (only the last group may be short)
                    counts.append(-(-(hi - lo) // g))
                assert sum(counts) == ngroups and max(counts) - min(counts) <= 1   # groups spread evenly
    with pytest.raises(ValueError):
        sharded.shard_bounds(10, 2, 0, sub_batch=0)


def test_sub_batch_knob_validation_and_workspace():
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    assert m.sub_batch is None and m.cfg().reserved[0] == 0
    m._ws = object()
    m.sub_batch = 4
    assert m.sub_batch == 4 and m.cfg().reserved[0] == 4 and m._ws is None   # (the setter drops the workspace)
    assert "sub_batch" not in str(list(m.state_dict().keys()))
    for bad in (0, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            m.sub_batch = bad
    assert m.sub_batch == 4
    m.sub_batch = None
    assert m.cfg().reserved[0] == 0


def test_c_abi_sub_batch_field():
    lib = _lib.load()
    ok = _lib.Cfg(4, 4, 3, 3, 0, 0, (ctypes.c_int32 * 2)(0, 0))
    assert ctypes.sizeof(ok) == 32
    base = lib.admmnet_workspace_bytes(ctypes.byref(ok), 1000)
    assert base > 0
    # one (sum, count) pair and one mean per sub-batch: more room for 1000 groups than for one batch
    one = _lib.Cfg(4, 4, 3, 3, 0, 0, (ctypes.c_int32 * 2)(1, 0))
    assert lib.admmnet_workspace_bytes(ctypes.byref(one), 1000) >= base + 1000 * 16 + 1000 * 4 - 512
    whole = _lib.Cfg(4, 4, 3, 3, 0, 0, (ctypes.c_int32 * 2)(5000, 0))
    assert lib.admmnet_workspace_bytes(ctypes.byref(whole), 1000) == base
    bad = _lib.Cfg(4, 4, 3, 3, 0, 0, (ctypes.c_int32 * 2)(-3, 0))
    assert lib.admmnet_workspace_bytes(ctypes.byref(bad), 8) < 0
    null = ctypes.c_void_p(0)
    rc = lib.admmnet_forward_f32(ctypes.byref(bad), null, null, null, null, 8, null, null, null, 0, null, null)
    assert rc == -1 and b"sub_batch" in lib.admmnet_last_error()          # ADMMNET_E_ARG


# ------------------------------------------------------------------ grouped sharding over gloo
class GroupOracleEngine:
    """Layer-at-a-time engine with the HipLayerEngine interface, computed by the oracle, with one (sum, count) pair and
    one mean per sub-batch of g signals."""

    def __init__(self, sd, M, N, K, g, y, b, sigma):
        self.R, self.sd, self.M, self.N, self.K, self.g = R, R.cast_weights(sd, "f32"), M, N, K, g
        self.y, self.b, self.sigma = y, b, sigma.reshape(-1)
        self.means = []

    def begin(self):
        B, n = self.y.shape[0], self.M * self.N + 1
        self.G = torch.zeros(B, n, n, dtype=torch.complex64)
        self.Z = torch.zeros(B, n, n, dtype=torch.complex64)

    def front(self, k):
        R = self.R
        self.phi = R.phi_layer(self.sd, k, self.y, self.b, self.G, self.Z)
        if k == self.K - 1:
            return None
        self.h = R.h_layer(self.sd, k, self.G, self.Z, self.sigma, self.M, self.N)
        self.G = R.g_layer(self.sd, k, self.phi, self.h, self.Z)
        corner = float(1.0 / (torch.nn.functional.softplus(self.sd[f"zLayers.{k}.lambda_param"]) ** 2 + R.EPS))
        self.Rm = self.G - R.block_matrix(self.phi, self.h, corner)
        self.rn = torch.linalg.norm(self.Rm, dim=(1, 2))
        pairs = []
        for lo in range(0, self.rn.numel(), self.g):
            part = self.rn[lo:lo + self.g]
            pairs += [float(part.double().sum()), float(part.numel())]
        return torch.tensor(pairs, dtype=torch.float64)

    def back(self, k, mean):
        self.means.append(mean.clone())
        per_signal = mean.to(torch.float32).repeat_interleave(self.g)[:self.rn.numel()]
        arho = self.R.z_step(self.sd, k, self.rn, mean_norm=per_signal)
        self.Z = self.Z + arho.reshape(-1, 1, 1) * self.Rm

    def finish(self):
        return self.phi, None


def _gloo_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)

    def no_all_reduce(*a, **k):
        raise AssertionError("grouped sharding must not all-reduce")
    dist.all_reduce = no_all_reduce

    Nb, Nd, K, B, g = 3, 4, 3, 11, 4
    sd = R.make_weights(Nb, Nd, K, seed=8, head=False, perturb=0.3)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=6)
    y, b, s = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    model = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K)
    model.sub_batch = g
    res = {}
    for scope in ("global", "shard"):
        engines = []

        def factory(yl, bl, sl):
            e = GroupOracleEngine(sd, Nb, Nd, K, g, yl, bl, sl)
            engines.append(e)
            return e
        lo, hi = sharded.shard_bounds(B, world, rank, sub_batch=g)
        phi, head = sharded.ShardedForward(model, scope=scope, engine_factory=factory)(y[lo:hi], b[lo:hi], s[lo:hi],
                                                                                       gather=True)
        assert head is None and len(engines[0].means) == K - 1
        assert all(mv.numel() == -(-(hi - lo) // g) for mv in engines[0].means)
        res[scope] = phi.numpy()
    # a shard that starts inside a group is refused on every rank, before any layer runs
    lo, hi = sharded.shard_bounds(B, world, rank)        # 6 | 5: rank 1 starts at signal 6, inside group 1
    try:
        sharded.ShardedForward(model, engine_factory=lambda *a: None)(y[lo:hi], b[lo:hi], s[lo:hi])
        res["raised"] = np.array(0)
    except ValueError:
        res["raised"] = np.array(1)
    np.savez(out % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_grouped_sharding_needs_no_collective(tmp_path):
    out = str(tmp_path / "rank%d.npz")
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    assert int(r0["raised"]) == 1 and int(r1["raised"]) == 1
    # the reference evaluated on each group of 4 signals on its own
    Nb, Nd, K, B, g = 3, 4, 3, 11, 4
    sd = R.make_weights(Nb, Nd, K, seed=8, head=False, perturb=0.3)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=6)
    want = np.concatenate([R.forward(sd, torch.from_numpy(y[lo:lo + g]), torch.from_numpy(b[lo:lo + g]),
                                     torch.from_numpy(s[lo:lo + g]), Nb, Nd, K, dtype="f32").numpy()
                           for lo in range(0, B, g)])
    for scope in ("global", "shard"):
        got = r0[scope]
        assert got.shape == want.shape
        assert np.abs(got - want).max() < 5e-6 * np.abs(want).max() + 2e-6, scope
    assert np.array_equal(r0["global"], r0["shard"])
