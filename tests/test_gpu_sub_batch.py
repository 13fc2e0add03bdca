"""GPU (-m gpu): independent sub-batches (``sub_batch = g``) in one forward call.  Every group of g consecutive signals
(the last one may be shorter) must come back with exactly the bits of a separate call on that group alone -- phi, the
head outputs and the status words (summed) -- at any chunk size, on either G-layer route, through the split protocol
and sharded over ranks without a collective."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import admm_net_amd as A
from admm_net_amd import _lib, sharded, synth
from oracle import admm_net_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_PHI = 1e-4   # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def _model(Nb, Nd, K, seed, head=True):
    sd = R.make_weights(Nb, Nd, K, seed=seed, head=head, perturb=0.3)
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd)
    return m, sd


def _outs(r):
    return [o.cpu() for o in (r if isinstance(r, tuple) else (r,))]


def _separate(m, args, g):
    """torch.cat of separate calls per group of g, and the summed status words."""
    m.sub_batch, m.chunk = None, 0
    B = args[0].shape[0]
    parts, status = [], np.zeros(4, dtype=np.int64)
    for lo in range(0, B, g):
        parts.append(_outs(m(*[t[lo:lo + g] for t in args])))
        status += np.array(m.last_status)
    return [torch.cat([p[i] for p in parts], dim=0) for i in range(len(parts[0]))], status.tolist()


GEOMS = [(10, 10, 5), (8, 16, 8), (12, 16, 4), (16, 16, 4)]


@pytest.mark.parametrize("geom", GEOMS, ids=["10x10K5", "8x16K8", "12x16K4", "16x16K4"])
def test_groups_are_bit_identical_to_separate_calls(dev, geom):
    """B = 1100 and g in {1, 7, 256, 600}; at g = 600 the groups of 600 and 500 signals take the two workgroup shapes of the
    matrix-function kernel at D <= 128, so the chunk loop splits at the last group.  chunk 0 and 512."""
    Nb, Nd, K = geom
    B = 1100
    m, _ = _model(Nb, Nd, K, seed=Nb * 10 + Nd)
    args = synth.make_batch_device(B, Nb, Nd, seed=40 + K, device=dev)[:3]
    whole = _outs(m(*args))
    for g in (1, 7, 256, 600):
        want, want_status = _separate(m, args, g)
        for chunk in (0, 512):
            m.chunk, m.sub_batch = chunk, g
            got = _outs(m(*args))
            for name, a, r in zip(("tau", "f", "conf", "phi"), got, want):
                assert torch.equal(a, r), (g, chunk, name)
            assert m.last_status == want_status, (g, chunk)
            assert m.last_status[2] > 0          # (the matrix-function route is in play)
        assert not torch.equal(got[3], whole[3])   # one mean over all 1100 signals is another result
    m.sub_batch, m.chunk = None, 0


@pytest.mark.parametrize("B", [300, 1100])
def test_one_group_is_the_default_call(dev, B):
    """sub_batch >= B and None give the bits of the default call (the grouped reduction of one group of B <= 1024 and of
    B > 1024 signals against rn_sum_kernel)."""
    Nb, Nd, K = 8, 16, 4
    m, _ = _model(Nb, Nd, K, seed=3, head=False)
    args = synth.make_batch_device(B, Nb, Nd, seed=7, device=dev)[:3]
    ref = m(*args).cpu()
    for g in (B, B + 1, 5000, None):
        m.sub_batch = g
        assert torch.equal(m(*args).cpu(), ref), g
    m.sub_batch = None


def test_groups_against_the_f64_oracle(dev):
    """The reference applied to each group of 5 on its own (13 signals: 5, 5, 3), float32 and float64 oracle."""
    Nb, Nd, K, B, g = 6, 6, 4, 13, 5
    m, sd = _model(Nb, Nd, K, seed=12)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=19)
    ty, tb, ts = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    m.sub_batch = g
    tau, f, conf, phi = m(ty.to(dev), tb.to(dev), ts.to(dev))
    m.sub_batch = None
    o32 = [R.forward(sd, ty[lo:lo + g], tb[lo:lo + g], ts[lo:lo + g], Nb, Nd, K, dtype="f32", head=True)
           for lo in range(0, B, g)]
    o64 = [R.forward(sd, ty[lo:lo + g], tb[lo:lo + g], ts[lo:lo + g], Nb, Nd, K, dtype="f64", head=True)
           for lo in range(0, B, g)]
    r32 = [torch.cat([o[i] for o in o32]).numpy() for i in range(4)]
    r64 = torch.cat([o[3] for o in o64]).numpy()
    rel = lambda a, r: float(np.abs(a - r).max() / np.abs(r).max())
    p = phi.cpu().numpy()
    assert rel(p, r32[3]) < TOL_PHI
    assert rel(p, r64) <= 3 * rel(r32[3], r64) + 2e-6
    for a, r in zip((tau, f, conf), r32[:3]):
        assert np.abs(a.cpu().numpy() - r).max() < 5e-5
    whole = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64", head=True)[3].numpy()
    assert rel(p, whole) > 10 * TOL_PHI        # (the per-group means matter at this size)


EIGEN_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
import torch
import admm_net_amd as A
from admm_net_amd import synth
from oracle import admm_net_ref as R
dev = torch.device("cuda:0")
out = {{}}
for Nb, Nd, K, B, g in ((8, 16, 4, 300, 64), (12, 16, 3, 50, 16), (5, 5, 4, 40, 1)):
    sd = R.make_weights(Nb, Nd, K, seed=Nb + Nd, head=True, perturb=0.3)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd)
    args = synth.make_batch_device(B, Nb, Nd, seed=B, device=dev)[:3]
    parts, status = [], [0, 0, 0, 0]
    for lo in range(0, B, g):
        parts.append([o.cpu() for o in m(*[t[lo:lo + g] for t in args])])
        status = [a + b for a, b in zip(status, m.last_status)]
    want = [torch.cat([p[i] for p in parts]) for i in range(4)]
    m.sub_batch = g
    got = [o.cpu() for o in m(*args)]
    out["%dx%d" % (Nb, Nd)] = dict(equal=all(torch.equal(a, r) for a, r in zip(got, want)),
                                   status=m.last_status == status, eigen=m.last_status[2] == 0)
print("RESULT " + json.dumps(out))
"""


def test_groups_on_the_eigensolver_route():
    """ADMMNET_SPECTRAL=0 (every dense G-layer through the eigensolver; read once per process: a child)."""
    env = dict(os.environ, ADMMNET_SPECTRAL="0")
    p = subprocess.run([sys.executable, "-c", EIGEN_CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert len(res) == 3
    for name, r in res.items():
        assert r == dict(equal=True, status=True, eigen=True), (name, r)


def test_split_protocol_pairs_and_means(dev):
    """Through the C ABI's layer-at-a-time calls: layer_front writes one (sum, count) pair per group, bit-equal to the
    pairs of separate calls; layer_back_pair on those pairs and layer_back on the per-group means both reproduce the
    grouped forward."""
    Nb, Nd, K, B, g = 8, 16, 4, 700, 300      # groups 300, 300, 100
    m, _ = _model(Nb, Nd, K, seed=5)
    args = synth.make_batch_device(B, Nb, Nd, seed=9, device=dev)[:3]
    m.sub_batch = g
    ref = _outs(m(*args))

    def run(model, a, use_pair):
        eng = sharded.HipLayerEngine(model, *a)
        eng.begin()
        pairs = []
        for k in range(K):
            sc = eng.front(k)
            if k == K - 1:
                break
            pairs.append(sc.clone().cpu())
            if use_pair:
                eng.back_pair(k, sc)
            else:
                eng.back(k, (sc[0::2] / sc[1::2]).to(torch.float32))
        phi, head = eng.finish()
        return pairs, [head[0].cpu(), head[1].cpu(), head[2].cpu(), phi.cpu()], eng.status.cpu().tolist()

    grouped_pairs, out_pair, st = run(m, args, True)
    assert all(p.numel() == 2 * 3 for p in grouped_pairs)
    _, out_mean, _ = run(m, args, False)
    for a, b_, r in zip(out_pair, out_mean, ref):
        assert torch.equal(a, r) and torch.equal(b_, r)
    assert st == m.last_status
    m.sub_batch = None
    for j, lo in enumerate(range(0, B, g)):
        sep_pairs, sep_out, _ = run(m, [t[lo:lo + g] for t in args], True)
        for k in range(K - 1):
            assert torch.equal(grouped_pairs[k][2 * j:2 * j + 2], sep_pairs[k]), (j, k)
        for a, r in zip(sep_out, ref):
            assert torch.equal(a, r[lo:lo + g])


def _sharded_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def no_all_reduce(*a, **k):
        raise AssertionError("grouped sharding must not all-reduce")
    dist.all_reduce = no_all_reduce
    dev = torch.device("cuda:0")
    Nb, Nd, K, B, g = 5, 6, 4, 27, 5
    m, _ = _model(Nb, Nd, K, seed=11)
    m.sub_batch = g
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=3)
    res = {}
    for scope in ("global", "shard"):
        lo, hi = sharded.shard_bounds(B, world, rank, sub_batch=g)
        args = [torch.from_numpy(v[lo:hi]).to(dev) for v in (y, b, s)]
        phi, head = sharded.ShardedForward(m, scope=scope)(*args, gather=True)
        res[scope + "_phi"], res[scope + "_head"] = phi.cpu().numpy(), head.cpu().numpy()
    lo, hi = sharded.shard_bounds(B, world, rank)          # 14 | 13: rank 1 starts inside a group
    try:
        sharded.ShardedForward(m)(*[torch.from_numpy(v[lo:hi]).to(dev) for v in (y, b, s)])
        res["raised"] = np.array(0)
    except ValueError:
        res["raised"] = np.array(1)
    if rank == 0:
        full = m(*[torch.from_numpy(v).to(dev) for v in (y, b, s)])
        res["phi_full"] = full[3].cpu().numpy()
        res["head_full"] = torch.stack(full[:3]).cpu().numpy()
    np.savez(out % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_groups_without_collective(tmp_path):
    """Two gloo ranks share cuda:0 (as tests/test_gpu_sharded.py): B = 27, g = 5 cut at group boundaries (15 | 12).  The
    gathered result equals the single-process grouped call bit for bit, in either scope, and no all-reduce is issued;
    shards that start inside a group raise ValueError on every rank."""
    out = str(tmp_path / "r%d.npz")
    port = 33600 + (os.getpid() % 2000)
    mp.spawn(_sharded_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    assert int(r0["raised"]) == 1 and int(r1["raised"]) == 1
    for scope in ("global", "shard"):
        assert np.array_equal(r0[scope + "_phi"], r0["phi_full"]), scope
        assert np.array_equal(r0[scope + "_head"], r0["head_full"]), scope
