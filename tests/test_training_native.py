"""CPU: the native training route (``unrolled_forward(..., fused=True, small=True, native=True)`` /
``model.train_route = "native"``) with the tensor stand-in ``training.TorchNativeKernels`` for the HIP kernels of
csrc/train_hlayer.hip.

* ``_HLayerStep`` -- the H layer with its correction_net inside, hand-written backward -- in float64 against autograd through
  ``training._h_layer`` itself: the output and every gradient, the four correction_net tensors included, within 1e-12 of its
  largest entry (tests/test_training_fused.py's rule, at its sizes).  The inputs hold signals with the scale clamped at 1 and
  signals with it open, a signal with a negative ``cval`` and, where D > 2, a signal with a tie in max |tc|; the test asserts
  that each occurs;
* the unsummed ``hlayer_terms`` add up to ``hlayer_bwd``;
* the whole route on the committed reference-gradient fixtures under tests/test_training.py's own rule;
* ``sub_batch`` on the route under tests/test_training_fused.py's two bounds;
* the stacked ``1 / (softplus(rho) + eps)`` of the G layers, the ``train_route`` knob and the argument checks of
  ``unrolled_forward``, the ops and the C entry points.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import admm_net_amd as A
from admm_net_amd import synth, training

import test_training as TT
from test_training_fused import SIZES, _close, _leaves
from test_training_small import _sb_loss, _sb_model

TNK = training.TorchNativeKernels
EPS = training.EPS
CPU = dict(solver=TT.cpu_eigh, assembler=training.TorchAssembler)
NATIVE = dict(fused=True, layer_kernels=training.TorchLayerKernels, small=True, small_kernels=training.TorchSmallKernels,
              native=True, native_kernels=TNK, **CPU)
F64 = torch.float64


def h_layer_case(B, D, seed, dtype=F64):
    """2 B signals and a correction_net.  The first B are small and positive (0 < cval < sigmoid(pw): the scale is clamped at
    1), the others of size 5 (the scale is open).  Where D > 2: signal B has t[0] = t[1] = 20 and the net gives m[0] = m[1]
    exactly (two zero rows of W2 under equal biases), a tie in max |tc|; signal B + 1 is -3 throughout under sigma = 0.5, so
    that cval = A max|tc| + sum tc < 0."""
    g = torch.Generator().manual_seed(seed + 300)
    r = lambda *s: torch.randn(*s, dtype=F64, generator=g)
    g_dg = torch.cat([r(B, D).abs() * 0.02, r(B, D) * 5])
    z_dg = r(2 * B, D) * 0.01
    sigma = torch.rand(2 * B, dtype=F64, generator=g) + 0.5
    up = r(2 * B, D)
    net = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, D), nn.Tanh()).double()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(r(*p.shape) * 0.05)                                 # a small correction: the clamped half stays clamped
        if D > 2:
            net[2].weight[:2] = 0.0
            net[2].bias[1] = net[2].bias[0]
            g_dg[B, :2], z_dg[B, :2] = 20.0, 0.0
            if B > 1:
                g_dg[B + 1], z_dg[B + 1], sigma[B + 1] = -3.0, 0.0, 0.5
    rho = torch.rand((), dtype=F64, generator=g) * 2.5 - 1.0
    pw = torch.rand((), dtype=F64, generator=g) + 0.5
    return [x.to(dtype) for x in (g_dg, z_dg, sigma, rho, pw, up)], net.to(dtype)


def h_layer_facts(D, g_dg, z_dg, sigma, rho, pw, net):
    """(clamped signals, signals with a tie in max |tc|, signals with cval < 0) of a case."""
    t = g_dg + z_dg / (F.softplus(rho) + EPS)
    tc = (t + 0.1 * net(t)).detach()
    Acoef = (2 * torch.sqrt(torch.tensor(float(D))) * sigma + sigma ** 2).reshape(-1, 1).to(tc.device)
    cval = Acoef * tc.abs().max(dim=1, keepdim=True)[0] + tc.sum(dim=1, keepdim=True)
    ties = (tc.abs() == tc.abs().max(dim=1, keepdim=True)[0]).sum(dim=1) > 1
    return int((torch.sigmoid(pw) / (cval + EPS) > 1).sum()), int(ties.sum()), int((cval < 0).sum())


NAMES = ("g_gdg", "g_zdg", "g_rho", "g_pw", "gW1", "gb1", "gW2", "gb2")


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_h_layer_step_function_matches_autograd(B, D, seed):
    (g_dg, z_dg, sigma, rho, pw, up), net = h_layer_case(B, D, seed)
    clamped, ties, negative = h_layer_facts(D, g_dg, z_dg, sigma, rho, pw, net)
    print(f"B={B} D={D}: {clamped} of {2 * B} signals clamped, {ties} with a tie, {negative} with cval < 0")
    assert 0 < clamped < 2 * B, "the inputs must hold clamped and unclamped signals"
    if D > 2:
        assert ties >= 1, "the inputs must hold a tie in max |tc|"
        if B > 1:
            assert negative >= 1, "the inputs must hold a negative cval"
    params = list(net.parameters())
    a, b = _leaves(g_dg, z_dg, rho, pw), _leaves(g_dg, z_dg, rho, pw)
    h1 = training._HLayerStep.apply(a[0], a[1], sigma, a[2], a[3], *training._net_params(net), TNK)
    layer = SimpleNamespace(dim=D, rho=b[2], projection_weight=b[3], correction_net=net)
    h2 = training._h_layer(layer, None, None, sigma, (b[0], b[1]))
    _close(h1.detach(), h2.detach(), "h")
    g1 = torch.autograd.grad(h1, a + params, up)
    g2 = torch.autograd.grad(h2, b + params, up)
    assert len(g1) == len(NAMES)
    for x, y, name in zip(g1, g2, NAMES):
        _close(x, y, name)


def test_some_size_has_a_tie_and_a_negative_cval():
    assert any(D > 2 and B > 1 for B, D, _ in SIZES)


def test_h_layer_terms_sum_to_the_backward():
    (g_dg, z_dg, sigma, rho, pw, up), net = h_layer_case(3, 6, 5)
    W1, b1, W2, b2 = (p.detach() for p in training._net_params(net))
    _, t, a1, m = TNK.hlayer(g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2)
    args = (up, z_dg, sigma, rho, pw, W1, W2, t, a1, m)
    terms, bwd = TNK.hlayer_terms(*args), TNK.hlayer_bwd(*args)
    assert torch.equal(terms[0], bwd[0]) and torch.equal(terms[1], bwd[1])
    assert torch.equal(terms[2], bwd[8]) and torch.equal(terms[3], bwd[9])
    for x, y in zip(terms[4:], bwd[2:8]):
        total = x.sum() if y.dim() == 0 else x.sum(dim=0)
        assert total.shape == y.shape and torch.allclose(total, y, rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ the route
@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_native_route_matches_reference_gradients(path):
    z, m, head, t = TT.load(path)
    m.eval()   # fixture convention: dropout off
    out = training.unrolled_forward(m, t("y"), t("b"), t("sigma"), **NATIVE)
    phi = out[3] if head else out
    assert np.abs(phi.detach().numpy() - z["phi"]).max() <= 2e-5 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


@pytest.mark.parametrize("B,g", [(11, 4), (9, 1), (10, 5)])
def test_native_route_groups_equal_separate_batches(B, g):
    """tests/test_training_fused.py::test_fused_route_groups_equal_separate_batches on the native route, same two bounds: the
    outputs of one grouped call equal the per-group calls to 1e-6 of the largest entry, the parameter gradients the SUM of
    the per-group calls' gradients to 1e-5 max + 1e-7."""
    Nb, Nd, K = 3, 4, 3
    m = _sb_model(Nb, Nd, K, seed=21)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=5)
    y, b, s = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    grads = lambda: {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}

    m.zero_grad(set_to_none=True)
    out = training.unrolled_forward(m, y, b, s, sub_batch=g, **NATIVE)
    _sb_loss(out, 1).backward()
    got = grads()

    m.zero_grad(set_to_none=True)
    parts = [training.unrolled_forward(m, y[lo:lo + g], b[lo:lo + g], s[lo:lo + g], **NATIVE) for lo in range(0, B, g)]
    sep = tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    _sb_loss(sep, 1).backward()
    want = grads()

    for a, r in zip(out, sep):
        assert (a - r).abs().max() <= 1e-6 * r.abs().max()
    for name, w in want.items():
        if w is None:
            assert got[name] is None, name
            continue
        assert (got[name] - w).abs().max() <= 1e-5 * w.abs().max() + 1e-7, name
    whole = training.unrolled_forward(m, y, b, s, **NATIVE)
    assert (whole[3] - sep[3]).abs().max() > 1e-5 * sep[3].abs().max()


def test_stacked_rho_factor_has_the_values_and_gradients_of_the_per_layer_form():
    m = _sb_model(3, 4, 4, seed=3).double()
    got = training._resolve_rinv(m, 4)
    assert got.shape == (3,)
    want = [1.0 / (F.softplus(m.gLayers[k].rho) + EPS) for k in range(3)]
    for k in range(3):
        assert got[k].item() == want[k].item()
    up = torch.tensor([0.3, -1.1, 2.0], dtype=F64)
    rhos = [m.gLayers[k].rho for k in range(3)]
    g1 = torch.autograd.grad((got * up).sum(), rhos)
    g2 = torch.autograd.grad(sum(w * u for w, u in zip(want, up)), rhos)
    for x, y in zip(g1, g2):
        _close(x, y, "g_rho")


def test_single_layer_model_runs_on_the_native_route():
    m = A.PhiEstADMMNet(M=2, N=2, num_layers=1)
    y = torch.ones(2, 4, dtype=torch.complex64)
    phi = training.unrolled_forward(m, y, y, torch.ones(2), **NATIVE)
    want = training.unrolled_forward(m, y, y, torch.ones(2), **CPU)
    assert (phi - want).abs().max() <= 1e-6 * want.abs().max()


def test_train_route_knob_accepts_native():
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    keys = set(m.state_dict())
    m.train_route = "native"
    assert m.train_route == "native" and set(m.state_dict()) == keys
    for bad in ("Native", "", None, 1, "hip", "small", "head", ("native",)):
        with pytest.raises(ValueError):
            m.train_route = bad
    assert m.train_route == "native"
    m.train_route = "tensor"


def test_native_needs_small_and_native_kernels_need_native():
    m = A.PhiEstADMMNet(M=2, N=2, num_layers=2)
    y = torch.ones(1, 4, dtype=torch.complex64)
    fused = dict(fused=True, layer_kernels=training.TorchLayerKernels)
    small = dict(small=True, small_kernels=training.TorchSmallKernels)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), native=True, **CPU)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), native=True, native_kernels=TNK, **fused, **CPU)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), native_kernels=TNK, **fused, **small, **CPU)


def test_train_hlayer_ops_refuse_cpu_tensors():
    from admm_net_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    r, a1 = torch.randn(2, 3, generator=g), torch.randn(2, 64, generator=g)
    v, s = torch.rand(2, generator=g), torch.tensor(0.5)
    W1, b1, W2, b2 = training._net_params(nn.Sequential(nn.Linear(3, 64), nn.ReLU(), nn.Linear(64, 3), nn.Tanh()))
    for call in (lambda: ops.train_hlayer(r, r, v, s, s, W1, b1, W2, b2),
                 lambda: ops.train_hlayer_bwd(r, r, v, s, s, W1, W2, r, a1, r)):
        with pytest.raises(_lib.AdmmNetError):
            call()


def test_train_hlayer_entry_points_reject_bad_arguments():
    """ADMMNET_E_ARG (-1) for D outside 1 ... 256, B < 1, a batch beyond the slab grid and null pointers -- decided on the host
    before anything is launched; the workspace query answers -1 for the same sizes."""
    import ctypes
    from admm_net_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)
    work = lib.admmnet_train_hlayer_workspace
    # {g_rho, g_pw} per slab of four signals, then gW1, gb1, gW2, gb2 per slab of 128 signals, in bytes
    assert work(100, 256) == 4 * (2 * 64 + 2 * (129 * 100 + 64))
    assert work(7, 1) == 4 * (2 + 129 * 7 + 64) and work(256, 129) == 4 * (2 * 33 + 2 * (129 * 256 + 64))
    for d, B in ((0, 4), (257, 4), (100, 0), (100, 65535 * 128 + 1)):
        assert work(d, B) == -1
        assert lib.admmnet_train_hlayer_f32(d, B, *([p] * 13), null) == -1
        assert lib.admmnet_train_hlayer_bwd_f32(d, B, *([p] * 16), null) == -1
    assert b"train_hlayer_bwd" in lib.admmnet_last_error()
    for i in range(13):
        assert lib.admmnet_train_hlayer_f32(100, 4, *([p] * i + [null] + [p] * (12 - i)), null) == -1
    for i in range(16):
        assert lib.admmnet_train_hlayer_bwd_f32(100, 4, *([p] * i + [null] + [p] * (15 - i)), null) == -1
