"""GPU: the head kernels of the native training route (csrc/train_head.hip, ``ops.train_head`` / ``ops.train_head_bwd``) against
float64 evaluations of their definitions.

The float64 definitions are ``training.TorchNativeKernels.head`` / ``head_bwd`` in float64 on the float32 inputs the kernels read
(tests/test_training_native_head.py holds those formulas to autograd through ``training._peak_head`` at 1e-12).

Bounds (``Worst`` of tests/test_gpu_training_small.py, ``WorstSum`` of tests/test_gpu_training_native.py):
  * per-signal tensors (tau, f, conf, g_phi): the yardstick is the parent's arithmetic, ``training._peak_head`` in float32 on
    the GPU with gradients by autograd through it (with a mask: the head in ``train()`` with ``torch.nn.functional.dropout``
    patched to apply the same mask).  The kernel must be no further from float64 than 3 x that distance plus 1e-6 of the largest
    entry;
  * parameter gradients (batch sums): within 3 x the parent's max-norm distance for that tensor plus 2e-5 sum_b |terms|, the
    terms summed by magnitude in float64 (``head_bwd(..., mag=True)``; for the token side the magnitudes of gK and gV go through
    |Wk|, |Wv|, |P|, |Wp| and |position_encoder|);
  * every backward run twice gives ``torch.equal`` results.
Each test prints the worst ratios it saw.  Worst figures measured on an MI355X are recorded in DESIGN.md section 4.

Shapes: D in {1, 7, 100, 128, 192, 256} x B in {1, 3, 256}, (100, 257) and (100, 4099) at L = 3: a softmax over one token, ragged
strides of the 128 threads over 4 D scores and 2 D inputs, B odd and B = 1 for the k loop of the matrix cores, one signal past a
batch slab of 128 and 33 slabs with a ragged last one; L = 1 and L = 8 at three of them.
"""
from unittest import mock

import pytest
import torch

import admm_net_amd as A
from admm_net_amd import ops, training

from test_gpu_training_small import Worst, _f64, _same_twice
from test_gpu_training_native import SHAPES, WorstSum

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TNK = training.TorchNativeKernels
CASES = [(D, 3, B) for D, B in SHAPES] + [(D, L, B) for L in (1, 8) for D, B in ((7, 3), (100, 257), (256, 256))]
IDS = [f"D{D}-L{L}-B{B}" for D, L, B in CASES]
NAMES = ["position_encoder", "fe0.weight", "fe0.bias", "fe2.weight", "fe2.bias", "position_projection.weight",
         "position_projection.bias", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "pe0.weight", "pe0.bias",
         "pe2.weight", "pe2.bias", "pe4.weight", "pe4.bias", "conf0.weight", "conf0.bias", "conf2.weight", "conf2.bias"]


def head_case(D, L, B, seed, wrap=lambda t: t):
    torch.manual_seed(seed)
    head = A.modules.PeakSearchLayer(D, 1, L)
    with torch.no_grad():
        for p in head.parameters():
            p.add_(0.05 * torch.randn_like(p))
    head = head.to(DEV)
    with torch.no_grad():
        for p in head.parameters():
            p.data = wrap(p.data)
    g = torch.Generator().manual_seed(seed + 1)
    phi = wrap(torch.complex(torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)).to(DEV))
    ups = [wrap(torch.randn(B, L, generator=g).to(DEV)) for _ in range(3)]
    return head, phi, ups


def check_head(head, phi, ups, keep, p, what):
    B, D = phi.shape
    L = head.L_max
    hp = training._head_params(head)
    names = NAMES + [f"{r}.{t}.{k}" for t in range(L) for r in ("tau", "f") for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
    assert len(names) == len(hp)

    # the parent: _peak_head in float32 on the GPU
    a = phi.detach().clone().requires_grad_(True)
    if keep is None:
        head.eval()
        parent = training._peak_head(head, a)
    else:
        head.train()

        def masked(x, p=0.5, training=True, inplace=False):
            return x * keep.reshape(x.shape).to(x.dtype) / (1.0 - p)

        saved_p, head.attention.dropout = head.attention.dropout, p
        with mock.patch("torch.nn.functional.dropout", masked):
            parent = training._peak_head(head, a)
        head.attention.dropout = saved_p
    pg = torch.autograd.grad(parent, [a] + hp, ups)

    # float64 on the same float32 inputs
    hp64 = [_f64(t) for t in hp]
    phi64, ups64 = _f64(phi), [_f64(u) for u in ups]
    keep64 = None if keep is None else keep.cpu()
    want = TNK.head(phi64, keep64, p, L, hp64)[:3]
    w_phi, w_g = TNK.head_bwd(*ups64, phi64, keep64, p, L, hp64)
    _, mag = TNK.head_bwd(*ups64, phi64, keep64, p, L, hp64, mag=True)

    worst = WorstSum(what)
    tau, f, conf, saved = ops.train_head(phi, keep, p, L, hp)
    for got, par, w, name in zip((tau, f, conf), parent, want, ("tau", "f", "conf")):
        assert torch.isfinite(got).all(), name
        worst.elem(got, par, w, name)
    g_phi, g = ops.train_head_bwd(*ups, phi, keep, p, L, hp, saved)
    g_phi2, g2 = ops.train_head_bwd(*ups, phi, keep, p, L, hp, saved)
    assert torch.equal(torch.view_as_real(g_phi), torch.view_as_real(g_phi2)), "two runs must give the same bits"
    assert all(torch.equal(x, y) for x, y in zip(g, g2)), "two runs must give the same bits"
    assert torch.isfinite(torch.view_as_real(g_phi)).all()
    worst.elem(torch.view_as_real(g_phi), torch.view_as_real(pg[0]), torch.view_as_real(w_phi), "g_phi")
    for got, par, w, m, name in zip(g, pg[1:], w_g, mag, names):
        assert torch.isfinite(got).all(), name
        worst.red3(got, par, w, m, name)
    worst.done()
    return g


@pytest.mark.parametrize("D,L,B", CASES, ids=IDS)
def test_head_kernels_match_their_definition(D, L, B):
    head, phi, ups = head_case(D, L, B, seed=9000 + D + 7 * L + B)
    check_head(head, phi, ups, None, 0.1, f"head D={D} L={L} B={B}")


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D,L,B", [(7, 3, 3), (100, 3, 257), (256, 8, 5)])
def test_head_kernels_with_a_keep_mask(D, L, B, p):
    head, phi, ups = head_case(D, L, B, seed=9500 + D)
    keep = (torch.rand(B, 4, D, generator=torch.Generator().manual_seed(int(100 * p) + D)) >= p).to(DEV)
    assert D == 7 or 0 < int((~keep).sum()) < keep.numel()
    check_head(head, phi, ups, keep, p, f"masked head D={D} L={L} B={B} p={p}")
    check_head(head, phi, ups, keep.to(torch.uint8), p, f"masked (uint8) head D={D} L={L} B={B} p={p}")


def test_all_dropped_head_rows_give_finite_zeros():
    """One signal with one head's row dropped entirely and one signal with all four: outputs and gradients stay finite and under
    the bounds.  With EVERY row of the batch dropped the attention contributes out_proj's bias alone: the gradients of in_proj,
    position_projection and position_encoder are exact zeros."""
    D, L, B = 12, 3, 4
    head, phi, ups = head_case(D, L, B, seed=77)
    keep = (torch.rand(B, 4, D, generator=torch.Generator().manual_seed(5)) >= 0.5).to(DEV)
    keep[1, 2] = False
    keep[3] = False
    check_head(head, phi, ups, keep, 0.5, "head with dropped rows")
    g = check_head(head, phi, ups, torch.zeros_like(keep), 0.5, "head with every row dropped")
    for i in (0, 5, 6, 7, 8):
        assert torch.equal(g[i], torch.zeros_like(g[i])), i


def test_head_kernels_on_unaligned_views():
    """phi, the upstream gradients, the mask and every parameter start one element behind an aligned base, at an odd D."""
    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v

    head, phi, ups = head_case(7, 3, 5, seed=21, wrap=off)
    keep = off((torch.rand(5, 4, 7, generator=torch.Generator().manual_seed(2)) >= 0.3).to(DEV))
    check_head(head, phi, ups, None, 0.1, "unaligned head")
    check_head(head, phi, ups, keep, 0.3, "unaligned masked head")


def test_head_gradients_do_not_depend_on_the_rest_of_the_batch_slab():
    """The batch sums run over fixed slabs of 128 signals: the per-signal weight gradients of B = 128 plus those of the 3 signals
    behind them equal, to float64's addition of the two, those of B = 131 in one call."""
    D, L = 100, 3
    head, phi, ups = head_case(D, L, 131, seed=31)
    hp = training._head_params(head)

    def grads(lo, hi):
        s = slice(lo, hi)
        tau, f, conf, saved = ops.train_head(phi[s], None, 0.0, L, hp)
        g = ops.train_head_bwd(*(u[s] for u in ups), phi[s], None, 0.0, L, hp, saved)[1]
        return [g[i] for i in (1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23, 24)]

    whole, first, tail = grads(0, 131), grads(0, 128), grads(128, 131)
    for x, y, z in zip(whole, first, tail):
        assert torch.equal(x, (y.double() + z.double()).float())


def test_train_head_ops_check_their_arguments():
    head, phi, ups = head_case(7, 3, 2, seed=1)
    hp = training._head_params(head)
    good = torch.ones(2, 4, 7, dtype=torch.bool, device=DEV)
    for bad in (good.float(), good[:, :3], good.reshape(2, 7, 4)):
        with pytest.raises(ValueError):
            ops.train_head(phi, bad, 0.1, 3, hp)
    with pytest.raises(ValueError):
        ops.train_head(phi, good, 1.0, 3, hp)
    with pytest.raises(ValueError):
        ops.train_head(phi, None, 0.1, 3, hp[:-1])
    with pytest.raises(ValueError):
        ops.train_head(phi, None, 0.1, 2, hp)
