"""GPU: the step size from a mean that comes from outside the call -- ``ops.train_rnsum``, ``ops.train_stepsize_pair``,
``ops.train_stepsize_bwd_pair_front`` and ``ops.train_stepsize_bwd_pair_back`` (csrc/train_small.hip), the device work around the
two per-layer all-reduces of ``sharded.ShardedTraining``.

Every case hands the kernels a pair that describes a LARGER, virtual batch -- three times the signals, a sum that is not the
local one -- and the back kernel a total that is not the local one either: a kernel that used its own mean or its own sum fails.

The definitions are ``training.TorchSmallKernels`` in float64 (tests/test_sharded_training_gloo.py ties its pair forms to the
whole-batch forms at 1e-12); the yardsticks are those of tests/test_gpu_training_small.py:
  * elementwise outputs (step, g_u, g_rn): no further from float64 than 3 x the float32 tensor formulation given the same pair,
    plus 1e-6 of the largest entry;
  * sums over the batch (the 162 parameter outputs, the float64 total): 2e-5 sum|terms|; the float64 sums themselves (the total
    over the kernel's own g_u, the pair) within 1e-12 relative of a float64 host sum;
  * every kernel run twice gives ``torch.equal`` results.
Each test prints the worst figures it saw; those measured on an MI355X are recorded in DESIGN.md section 5.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from admm_net_amd import ops, training

import test_gpu_training_small as GS

pytestmark = pytest.mark.gpu

DEV, EPS, TSK = GS.DEV, training.EPS, training.TorchSmallKernels
_f64 = GS._f64


def _case(B, seed):
    g = torch.Generator().manual_seed(seed)
    rn, up, rho = GS._dev(torch.rand(B, generator=g) * 4 + 0.1, torch.randn(B, generator=g), torch.rand((), generator=g) * 2 - 0.5)
    return rn, up, rho, training._net_params(GS._small_net(g, 3, 32))


# B: one signal, below and across a 256-thread slab, a ragged last slab, more than four slabs
@pytest.mark.parametrize("B", [1, 3, 255, 256, 257, 1025])
def test_pair_kernels_match_their_definition(B, k=3):
    worst = GS.Worst(f"pair B={B}")
    rn, up, rho, pars = _case(B, 9000 + B)
    knorm = float(np.float32(k / 10.0))
    # ---- this call's share of the pair
    (local,) = GS._same_twice(lambda: (ops.train_rnsum(rn),))
    host = _f64(rn).sum().item()
    err = abs(local[0].item() - host) / abs(host)
    print(f"  rnsum: relative error {err:.2e}")
    assert local.dtype == torch.float64 and local[1].item() == B and err <= 1e-12
    # ---- a virtual batch of three times the signals, its sum not three times the local one
    pair = torch.stack([local[0] * 4.5 + 1.3, local[1] * 3])          # its mean: 1.5 x the local one + 0.43 / B
    assert abs(pair[0].item() / pair[1].item() - host / B) > 0.05
    w64, p64 = [_f64(x) for x in (rn, rho, *pars)], pair.cpu()
    r, mean32 = F.softplus(rho), (pair[0] / pair[1]).to(torch.float32)
    feat = torch.stack([torch.full((B,), k / 10.0, device=DEV), torch.full((B,), r.item(), device=DEV), rn / (mean32 + EPS)], dim=1)
    parent = r * (0.5 + 1.5 * torch.sigmoid(F.linear(torch.relu(F.linear(feat, pars[0], pars[1])), pars[2], pars[3]))).squeeze(1)
    (step,) = GS._same_twice(lambda: (ops.train_stepsize_pair(rn, pair, rho, *pars, k / 10.0),))
    worst.elem(step, parent, TSK.stepsize_pair(w64[0], p64, *w64[1:], knorm), "step")
    # ---- the backward up to the collective
    got = GS._same_twice(lambda: ops.train_stepsize_bwd_pair_front(up, rn, pair, rho, *pars, k / 10.0))
    par32 = TSK.stepsize_bwd_pair_front(up, rn, pair, rho, *pars, knorm)                 # the float32 tensor formulation, same pair
    terms = TSK.stepsize_pair_terms(_f64(up), w64[0], p64, *w64[1:], knorm)
    worst.elem(got[0], par32[0], terms[0], "g_u")
    own = (_f64(got[0]) * w64[0]).sum().item()                                           # over the kernel's own g_u
    err = abs(got[1].item() - own) / abs(own)
    print(f"  total: relative error against the float64 host sum of g_u rn {err:.2e}")
    assert got[1].dtype == torch.float64 and tuple(got[1].shape) == (1,) and err <= 1e-12
    for x, t, name in zip(got[1:], terms[1:], ("total", "g_rho", "gW1", "gb1", "gW2", "gb2")):
        worst.red(x, t.sum(dim=0).reshape(x.shape), t.abs().sum(dim=0), name)
    # ---- the backward behind it, with a total that is not this call's
    total = got[1] * 3 + 0.5
    (g_rn,) = GS._same_twice(lambda: (ops.train_stepsize_bwd_pair_back(got[0], pair, total),))
    parent = TSK.stepsize_bwd_pair_back(par32[0], pair, par32[1] * 3 + 0.5)
    want = TSK.stepsize_bwd_pair_back(terms[0], p64, terms[1].sum().reshape(1) * 3 + 0.5)
    local_rule = TSK.stepsize_bwd_pair_back(terms[0], TSK.rnsum(w64[0]), terms[1].sum().reshape(1))
    assert (want - local_rule).abs().max() > 1e-3 * want.abs().max(), "the case must tell the outside mean from the local one"
    worst.elem(g_rn, parent, want, "g_rn")
    worst.done()


def test_a_pair_of_one_signal_keeps_the_eps_remainder():
    """pair = (rn, 1): g_u mean and total / count cancel exactly and g_rn = g_u eps / den^2 remains -- the case the kernel
    comment of ts_stepsize_bwd_kernel documents.  Round-off of the difference would be as large as the remainder itself."""
    rn, up, rho, pars = _case(1, 77)
    pair = ops.train_rnsum(rn)
    assert pair[0].item() == rn.item() and pair[1].item() == 1.0
    g_u, total, *_ = ops.train_stepsize_bwd_pair_front(up, rn, pair, rho, *pars, 0.3)
    g_rn = ops.train_stepsize_bwd_pair_back(g_u, pair, total)
    want = _f64(g_u) * EPS / (_f64(rn) + EPS) ** 2
    print(f"  g_u {g_u.item():.6e}, g_rn {g_rn.item():.6e}, g_u eps / den^2 {want.item():.6e}")
    assert g_u.item() != 0.0
    assert abs(g_rn.item() - want.item()) <= 1e-5 * abs(want.item())


def test_pair_ops_refuse_what_the_kernels_cannot_read():
    rn, up, rho, pars = _case(4, 5)
    pair = ops.train_rnsum(rn)
    with pytest.raises(ValueError):
        ops.train_stepsize_pair(rn, pair.to(torch.float32), rho, *pars, 0.3)
    with pytest.raises(ValueError):
        ops.train_stepsize_bwd_pair_back(rn, pair, pair)                    # total holds one element
    with pytest.raises(ops._lib.AdmmNetError):
        ops.train_rnsum(rn.cpu())
