"""GPU: the native training route -- the H-layer kernels and the batch-reduced product of csrc/train_hlayer.hip
(``ops.train_hlayer`` / ``ops.train_hlayer_bwd``) against float64 evaluations of their definitions, and
``model.train_route = "native"`` end to end (the head's kernels on their own: tests/test_gpu_training_native_head.py).

The float64 definitions are ``training.TorchNativeKernels`` in float64 on the float32 inputs the kernels read
(tests/test_training_native.py holds those formulas to autograd through ``training._h_layer`` at 1e-12).

Bounds (tests/test_gpu_training_small.py, whose ``Worst`` is used here):
  * per-signal tensors (h, g_gdg, g_zdg, delta1, delta2): the yardstick is the parent's arithmetic -- the float32 tensor
    formulation ``training._h_layer`` on the GPU, gradients by autograd through it (the deltas are its gradients at the two
    pre-activations).  The kernel must be no further from float64 than 3 x that distance plus 1e-6 of the largest entry;
  * parameter gradients (batch sums: g_rho, g_pw, gW1, gb1, gW2, gb2): within 3 x the parent's max-norm distance for that tensor
    plus 2e-5 sum_b |terms|, the per-signal products summed by magnitude in float64.  The first part covers the deltas' own
    float32 error, which the parent shares;
  * every backward run twice gives ``torch.equal`` results.
Each test prints the worst ratios it saw.  Worst figures measured on an MI355X are recorded in DESIGN.md section 4.

Shapes: D in {1, 7, 100, 128, 192, 256} x B in {1, 3, 256}, (100, 257) and (100, 4099): one element, ragged lanes, the
elements-per-lane boundaries, a ragged slab of four signals, B odd and B = 1 for the k loop of the matrix cores, one signal past a
batch slab of 128 (257 = 2 x 128 + 1) and 33 batch slabs with a ragged last one.
"""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import admm_net_amd as A
from admm_net_amd import ops, synth, training

import test_training as TT
from test_gpu_training_small import RED, Worst, _dev, _f64, _leaves, _run, _same_twice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TNK = training.TorchNativeKernels
TSK = training.TorchSmallKernels
SHAPES = [(D, B) for D in (1, 7, 100, 128, 192, 256) for B in (1, 3, 256)] + [(100, 257), (100, 4099)]
IDS = [f"D{D}-B{B}" for D, B in SHAPES]


class WorstSum(Worst):
    def red3(self, got, parent, want, mag, name):
        """|kernel - f64| <= 3 max|parent - f64| + 2e-5 sum|terms| for every entry; mag: the sum of magnitudes, float64."""
        want = _f64(want)
        mag = _f64(mag).reshape(want.shape)
        assert got.shape == want.shape and parent.shape == want.shape, name
        perr = (_f64(parent) - want).abs().max().item()
        err = (_f64(got) - want).abs()
        ratio = (err / (3 * perr + RED * mag + 1e-300)).max().item()
        print(f"  {self.what} {name}: kernel {err.max().item():.3e}, parent {perr:.3e}, error / (3 parent + 2e-5 sum|terms|) = {ratio:.3f}")
        self.red_ratio = max(self.red_ratio, ratio)
        assert ratio <= 1.0, f"{name}: error / (3 parent + 2e-5 sum|terms|) = {ratio:.3f}"


def h_case(D, B, seed):
    """Even signals: small positive g_dg with cval near 0.1, below sigmoid(pw) >= 0.62 -- the scale is clamped at 1.  Odd
    signals: g_dg of size 5 -- the scale is open, and the hidden units and the tanh are well into their non-linear range.  The
    biases shrink with D so that the correction of a small signal, 0.1 m summed over D elements, leaves it clamped.

    The open signals are kept WELL-CONDITIONED: h = tc sigmoid(pw) / (cval + eps) with cval = A max|tc| + sum tc, and where the
    signs of tc are free that sum can cancel to a few ulps of its terms; h then carries the rounding of one float32 addition
    magnified by |tc| / cval, a single such signal sets the max-norm error of the whole batch, and "3 x the parent's distance"
    compares two draws of that one rounding (the parent's own arithmetic with the columns permuted moves by 8 x on such a
    signal).  So signals 1 mod 4 are positive apart from one entry in eight (cval > 0 with little cancellation), and signals
    3 mod 4 negative apart from one entry in eight, under sigma = 0.05, where A max|tc| is small against sum |tc| (cval < 0,
    again with little cancellation; at D = 1 cval = (A - 1) |tc|).  ``check_hlayer`` asserts the premise: no open signal
    cancels below a tenth of A max|tc| + sum |tc|.  Measured on an MI355X with the odd signals left as randn * 5 with free signs,
    at D = 7, B = 256: h kernel 5.089e-06 / parent 6.094e-07 / bound 5.224e-06 (met), g_gdg kernel 1.225e-04 / parent 8.017e-06
    / bound 6.741e-05 (NOT met), both set by signal 145 alone, whose |h| / |cval| is 20 times any other signal's.
    ``test_hlayer_kernels_near_cancellation`` covers such signals, per signal and under a bound that has the amplification in
    it."""
    g = torch.Generator().manual_seed(seed)
    shrink = 1.0 / (D + 6 * D ** 0.5 + 1)
    small = torch.randn(B, D, generator=g).abs() * 0.1 * shrink
    kind = (torch.arange(B) % 4).reshape(-1, 1)
    flip = torch.where(torch.rand(B, D, generator=g) < 0.125, -1.0, 1.0)
    if D < 8:
        flip = torch.ones(B, D)                                        # a flipped entry of so few would cancel after all
    large = torch.randn(B, D, generator=g).abs() * 5 * flip * torch.where(kind == 3, -1.0, 1.0)
    g_dg = torch.where(kind % 2 == 0, small, large)
    z_dg = torch.randn(B, D, generator=g) * 0.1 * g_dg.abs().mean(dim=1, keepdim=True)
    sigma = torch.where(kind.reshape(-1) == 3, torch.tensor(0.05), torch.rand(B, generator=g) + 0.5)
    rho = torch.rand((), generator=g) * 2 - 0.5
    pw = torch.rand((), generator=g) + 0.5
    net = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, D), nn.Tanh())
    with torch.no_grad():
        net[0].weight.copy_((torch.rand(64, D, generator=g) * 2 - 1) / D ** 0.5)
        net[2].weight.copy_((torch.rand(D, 64, generator=g) * 2 - 1) / 8)
        net[0].bias.copy_(torch.randn(64, generator=g) * 0.5 * shrink)
        net[2].bias.copy_(torch.randn(D, generator=g) * 0.5 * shrink)
    return _dev(g_dg, z_dg, sigma, rho, pw, torch.randn(B, D, generator=g)), net.to(DEV)


def check_hlayer(D, B, g_dg, z_dg, sigma, rho, pw, up, net, what):
    worst = WorstSum(what)
    pars = training._net_params(net)
    W1, b1, W2, b2 = pars
    w = [_f64(x) for x in (g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2)]

    # the parent: _h_layer in float32 on the GPU; its correction_net keeps the two pre-activations, where autograd's gradients
    # are the deltas
    a, params, pre = _leaves(g_dg, z_dg, rho, pw), list(net.parameters()), []

    def recording_net(t):
        p1 = net[0](t)
        p2 = net[2](net[1](p1))
        pre.extend((p1, p2))
        return net[3](p2)

    layer = SimpleNamespace(dim=D, rho=a[2], projection_weight=a[3], correction_net=recording_net)
    parent = training._h_layer(layer, None, None, sigma, (a[0], a[1]))
    pg = torch.autograd.grad(parent, a + params + pre, up)
    p_gdg, p_zdg, p_rho, p_pw, pW1, pb1, pW2, pb2, p_d1, p_d2 = pg

    h, t, a1, m = ops.train_hlayer(g_dg, z_dg, sigma, rho, pw, *pars)
    h64, t64, a64, m64 = TNK.hlayer(*w)
    worst.elem(h, parent, h64, "h")
    got = _same_twice(lambda: ops.train_hlayer_bwd(up, z_dg, sigma, rho, pw, W1, W2, t, a1, m))
    g_gdg, g_zdg, g_rho, g_pw, gW1, gb1, gW2, gb2, d1, d2 = got
    u = _f64(up)
    w_gdg, w_zdg, w_d1, w_d2, t_rho, t_pw = _terms_light(u, w, t64, a64, m64)
    worst.elem(g_gdg, p_gdg, w_gdg, "g_gdg")
    worst.elem(g_zdg, p_zdg, w_zdg, "g_zdg")
    worst.elem(d1, p_d1, w_d1, "delta1")
    worst.elem(d2, p_d2, w_d2, "delta2")

    _, tc, _, den, sp = TSK._project_parts(t64, m64, w[2], w[4])
    q = sp / den
    clamped = int((q > 1).sum())
    print(f"  {what}: {clamped} of {B} signals clamped")
    if B > 1:
        assert 0 < clamped < B, "the inputs must hold clamped and unclamped signals"
    if B > 3:
        assert (den < 0).any(), "the inputs must hold a negative cval"
    Acoef = (2 * D ** 0.5 * w[2] + w[2] ** 2).reshape(-1, 1)
    cond = (den.abs() / (Acoef * tc.abs().max(dim=1, keepdim=True)[0] + tc.abs().sum(dim=1, keepdim=True)))[q <= 1]
    if cond.numel():
        print(f"  {what}: least |cval| / (A max|tc| + sum|tc|) among the open signals {cond.min().item():.3f}")
        assert cond.min().item() >= 0.1, "an open signal's cval cancels: the comparison would measure one rounding"
    worst.red3(g_rho, p_rho, t_rho.sum(), t_rho.abs().sum(), "g_rho")
    mag_pw = ((u * tc).abs().sum(dim=1, keepdim=True) * (q <= 1) / den.abs() * sp * (1 - sp)).sum()
    worst.red3(g_pw, p_pw, t_pw.sum(), mag_pw, "g_pw")
    # sum_b |delta_b| (x) |activation_b| as one product: the terms themselves are B x 64 x D numbers
    worst.red3(gW1, pW1, w_d1.t() @ t64, w_d1.abs().t() @ t64.abs(), "gW1")
    worst.red3(gb1, pb1, w_d1.sum(dim=0), w_d1.abs().sum(dim=0), "gb1")
    worst.red3(gW2, pW2, w_d2.t() @ a64, w_d2.abs().t() @ a64.abs(), "gW2")
    worst.red3(gb2, pb2, w_d2.sum(dim=0), w_d2.abs().sum(dim=0), "gb2")
    worst.done()


def _terms_light(u, w, t64, a64, m64):
    """``TorchNativeKernels.hlayer_terms`` without its two [B, 64, D]-sized outputs."""
    g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2 = w
    g_tc, _, t_pw = TSK.hproject_terms(u, t64, m64, sigma, pw)
    d2 = 0.1 * g_tc * (1 - m64 ** 2)
    d1 = (d2 @ W2) * (a64 > 0).to(u.dtype)
    g_gdg, g_zdg, t_rho = TSK.hinput_terms(g_tc + d1 @ W1, z_dg, rho)
    return g_gdg, g_zdg, d1, d2, t_rho, t_pw


def test_light_terms_are_the_stand_ins():
    """The helper above against ``hlayer_terms`` itself, so that the float64 reference of this file IS the stand-in's."""
    (g_dg, z_dg, sigma, rho, pw, up), net = h_case(7, 5, seed=1)
    w = [_f64(x) for x in (g_dg, z_dg, sigma, rho, pw, *training._net_params(net))]
    _, t64, a64, m64 = TNK.hlayer(*w)
    full = TNK.hlayer_terms(_f64(up), w[1], w[2], w[3], w[4], w[5], w[7], t64, a64, m64)
    for x, y in zip(_terms_light(_f64(up), w, t64, a64, m64), full[:6]):
        assert torch.equal(x, y)
    assert torch.allclose(full[6].abs().sum(dim=0), full[2].abs().t() @ t64.abs(), rtol=1e-13, atol=0)
    assert torch.allclose(full[8].abs().sum(dim=0), full[3].abs().t() @ a64.abs(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("D,B", SHAPES, ids=IDS)
def test_hlayer_kernels_match_their_definition(D, B):
    (g_dg, z_dg, sigma, rho, pw, up), net = h_case(D, B, seed=7000 + D + B)
    check_hlayer(D, B, g_dg, z_dg, sigma, rho, pw, up, net, f"hlayer D={D} B={B}")


def test_hlayer_kernels_on_unaligned_views():
    """[B, D], [B] and the weight tensors start 4 bytes behind an aligned base, at an odd D: the same definitions and bounds."""
    D, B = 7, 5

    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v

    (g_dg, z_dg, sigma, rho, pw, up), net = h_case(D, B, seed=9)
    with torch.no_grad():
        for p in net.parameters():
            p.data = off(p.data)
    check_hlayer(D, B, off(g_dg), off(z_dg), off(sigma), rho, pw, off(up), net, "unaligned hlayer")


U32 = 2.0 ** -24          # unit round-off of float32


def near_cancellation_case(D, seed):
    """Four signals with free signs (g_dg of size 5, sigma in [0.5, 1.5)): the natural inputs.  Signal 0 then gets the sigma,
    solved for in float64 on the host, at which cval = -(A max|tc| + sum|tc|) / 300: the scale is open (q < 0 <= 1) and
    h = tc sigmoid(pw) / cval magnifies whatever error cval carries 300 times."""
    g = torch.Generator().manual_seed(seed)
    B = 4
    g_dg = torch.randn(B, D, generator=g) * 5
    z_dg = torch.randn(B, D, generator=g) * 0.1
    sigma = torch.rand(B, generator=g) + 0.5
    rho, pw = torch.rand((), generator=g) * 2 - 0.5, torch.rand((), generator=g) + 0.5
    net = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, D), nn.Tanh())
    with torch.no_grad():
        net[0].weight.copy_((torch.rand(64, D, generator=g) * 2 - 1) / D ** 0.5)
        net[2].weight.copy_((torch.rand(D, 64, generator=g) * 2 - 1) / 8)
        pars = [x.detach().double() for x in training._net_params(net)]
        run = lambda: TNK.hlayer(g_dg.double(), z_dg.double(), sigma.double(), rho.double(), pw.double(), *pars)
        if run()[1][0].sum() > 0:                            # sum tc < 0 is what A max|tc| > 0 can cancel
            g_dg[0], z_dg[0] = -g_dg[0], -z_dg[0]
        _, t, _, m = run()
        tc = t[0] + 0.1 * m[0]                               # tc does not depend on sigma: one step solves for it
        A0 = (-tc.sum() - tc.abs().sum() / 300) / (tc.abs().max() * 301 / 300)
        sigma[0] = (-D ** 0.5 + (D + A0) ** 0.5).float()     # A = 2 sqrt(D) sigma + sigma^2
    return _dev(g_dg, z_dg, sigma, rho, pw, torch.randn(B, D, generator=g)), net.to(DEV)


@pytest.mark.parametrize("D", [7, 100, 128, 192, 256])
def test_hlayer_kernels_near_cancellation(D):
    """``test_hlayer_kernels_match_their_definition`` keeps cval away from cancellation; this test goes there.  Per signal b, with
    c = cval + eps, S = A max|tc| + sum|tc| and kappa = S / |c|: in float32 every tc carries at most 3 roundings (the division,
    the two additions), the sum of up to 256 of them three in-lane additions and an eight-level tree, the product A max|tc| two
    more: |delta c| <= 16 u S to first order, u = 2^-24, in ANY order of summation.  From h = tc sp / c, q = sp / c,
    g_c = -g_s sp / c^2 (g_s = sum g_h tc, itself 16 u sum|g_h tc| uncertain) and g_tc = g_h q + g_c (1 + [i = imax] A sign tc):
        |delta h|    <= 16 u kappa max|h_b|
        |delta g_tc| <= 16 u (kappa |q| max|g_h| + (1 + A) (2 kappa |g_c| + sp / c^2 sum|g_h tc|)),
    the latter doubled for g_gdg = g_tc + W1^T delta1, whose second part is a linear map of g_tc (W1^T relu' W2^T 0.1 tanh') whose
    max-norm the test evaluates per signal and asserts to be at most 1.  The kernel must be within 3 x the parent's distance for that signal + 1e-6 of the signal's
    largest entry + that amplification term: an error in the projection path near cancellation that is more than round-off
    (a wrong sign at imax, a lost A, a wrong power of c) is O(kappa) or O(1) RELATIVE and cannot hide under 16 u kappa ~ 3e-4.
    The test asserts that signal 0 is open with 100 <= kappa <= 1000 and prints every figure."""
    (g_dg, z_dg, sigma, rho, pw, up), net = near_cancellation_case(D, seed=8000 + D)
    pars = training._net_params(net)
    W1, b1, W2, b2 = pars
    w = [_f64(x) for x in (g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2)]
    a = _leaves(g_dg, z_dg)
    layer = SimpleNamespace(dim=D, rho=rho, projection_weight=pw, correction_net=net)
    parent = training._h_layer(layer, None, None, sigma, (a[0], a[1]))
    p_gdg = torch.autograd.grad(parent, a[0], up)[0]
    h, t, a1, m = ops.train_hlayer(g_dg, z_dg, sigma, rho, pw, *pars)
    g_gdg = ops.train_hlayer_bwd(up, z_dg, sigma, rho, pw, W1, W2, t, a1, m)[0]

    u = _f64(up)
    h64, t64, a64, m64 = TNK.hlayer(*w)
    w_gdg = _terms_light(u, w, t64, a64, m64)[0]
    A_, tc, _, c, sp = TSK._project_parts(t64, m64, w[2], w[4])
    S = A_ * tc.abs().max(dim=1, keepdim=True)[0] + tc.abs().sum(dim=1, keepdim=True)
    kappa, q = (S / c.abs()).reshape(-1), (sp / c).reshape(-1)
    print(f"  D={D}: kappa {[round(k, 1) for k in kappa.tolist()]}, q {[round(v, 3) for v in q.tolist()]}")
    assert q[0] <= 1 and 100 <= kappa[0] <= 1000, "signal 0 must be open and near cancellation"
    # the premise of the doubling: J = W1^T diag(relu') W2^T diag(0.1 tanh'), the map from g_tc to the second part of g_gdg, has
    # max-norm (largest absolute row sum) at most 1 for every signal of the case
    J = torch.einsum("ki,bk,jk,bj->bij", w[5], (a64 > 0).to(u.dtype), w[7], 0.1 * (1 - m64 ** 2))
    jnorm = J.abs().sum(dim=2).max(dim=1)[0]
    print(f"  D={D}: max-norm of the MLP's backward map per signal {[round(v, 3) for v in jnorm.tolist()]}")
    assert (jnorm <= 1).all(), "the amplification term doubles g_tc's error for g_gdg: the MLP's backward map must not expand"
    g_s = (u * tc).sum(dim=1)
    g_c = (-g_s * sp / c.reshape(-1) ** 2).abs() * (q <= 1)
    amp_h = 16 * U32 * kappa * h64.abs().max(dim=1)[0]
    amp_g = 32 * U32 * (kappa * q.abs().clamp(max=1.0) * u.abs().max(dim=1)[0]
                        + (1 + A_.reshape(-1)) * (2 * kappa * g_c + sp / c.reshape(-1) ** 2 * (u * tc).abs().sum(dim=1) * (q <= 1)))
    for got, par, want, amp, name in ((h, parent, h64, amp_h, "h"), (g_gdg, p_gdg, w_gdg, amp_g, "g_gdg")):
        err = (_f64(got) - want).abs().max(dim=1)[0]
        perr = (_f64(par) - want).abs().max(dim=1)[0]
        bound = 3 * perr + 1e-6 * want.abs().max(dim=1)[0] + amp
        for b in range(err.numel()):
            print(f"  D={D} {name} signal {b}: kernel {err[b]:.3e}, parent {perr[b]:.3e}, amplification term {amp[b]:.3e}, "
                  f"largest entry {want[b].abs().max():.3e}, error / bound {err[b] / bound[b]:.3f}")
        assert (err <= bound).all(), f"{name}: error / bound {(err / bound).max().item():.3f}"


def test_weight_gradients_do_not_depend_on_the_rest_of_the_batch_slab():
    """The batch-reduced product sums fixed slabs of 128 signals: signals appended BEHIND a full slab leave that slab's partial
    sums alone, so the gradients of B = 128 plus those of the 3 signals after them equal -- to float64's addition of the two --
    the gradients of B = 131 in one call, and a call's result is the same bits whatever else ran before it."""
    D = 100
    (g_dg, z_dg, sigma, rho, pw, up), net = h_case(D, 131, seed=11)
    W1, b1, W2, b2 = training._net_params(net)

    def grads(lo, hi):
        s = slice(lo, hi)
        _, t, a1, m = ops.train_hlayer(g_dg[s], z_dg[s], sigma[s], rho, pw, W1, b1, W2, b2)
        return ops.train_hlayer_bwd(up[s], z_dg[s], sigma[s], rho, pw, W1, W2, t, a1, m)[4:8]

    whole, head, tail = grads(0, 131), grads(0, 128), grads(128, 131)
    for x, y, z in zip(whole, head, tail):
        want = (y.double() + z.double()).float()
        assert torch.equal(x, want)
    assert all(torch.equal(x, y) for x, y in zip(whole, grads(0, 131)))


# ------------------------------------------------------------------------------------------------ the route, end to end
@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_native_route_gradients_match_reference(path):
    """tests/test_training.py::test_hip_training_gradients_match_reference with ``train_route = "native"``."""
    z, m, head, t, out = _run(path, "native")
    phi = out[3] if head else out
    assert phi.requires_grad and phi.is_cuda
    assert np.abs(phi.detach().cpu().numpy() - z["phi"]).max() <= 1e-4 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_native_and_full_route_give_the_same_outputs(path):
    """phi (and the head's outputs) in eval mode, route against route: 2e-5 of the largest entry, the rule of
    tests/test_gpu_training_small.py::test_full_and_tensor_route_give_the_same_phi."""
    z, m, head, t = TT.load(path, DEV)
    m.eval()
    outs = {}
    for route in ("native", "full"):
        m.train_route = route
        out = m.forward_autograd(t("y"), t("b"), t("sigma"))
        outs[route] = out if head else (out,)
    for x, y, name in zip(outs["native"], outs["full"], ("tau", "f", "conf", "phi") if head else ("phi",)):
        err = (x - y).abs().max().item() / y.abs().max().item()
        print(f"native against full route: {name} differs by {err:.2e} of its largest entry")
        assert err <= 2e-5, name


def test_native_route_trains_the_head_model_at_16x16():
    """One 16 x 16 (D = 256), K = 3 training step of ``ADMMNet`` in ``train()`` with ``sub_batch = 2``: every gradient is finite,
    and the parameters without a gradient are exactly those of the tensor route, which mirrors the reference (the H, G and Z
    layers of the last layer, every ``lambda_param`` and the unused ``step_adjust_net``): they stay None, everything else has
    a gradient."""
    dev = torch.device(DEV)
    torch.manual_seed(3)
    K = 3
    m = A.ADMMNet(M=16, N=16, num_layers=K).to(dev)
    m.sub_batch = 2
    m.train()
    y, b, sigma, _ = synth.make_batch(5, 16, 16, seed=5)
    ty, tb, ts = (torch.from_numpy(v).to(dev) for v in (y, b, sigma))

    def without_gradient(route):
        m.train_route = route
        m.zero_grad(set_to_none=True)
        tau, f, conf, phi = m(ty, tb, ts)
        loss = (phi - ty / tb).abs().pow(2).mean() + tau.pow(2).mean() + f.pow(2).mean() + (conf - 1).pow(2).mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        return {name for name, p in m.named_parameters() if p.grad is None}

    want = without_gradient("tensor")
    assert {f"hLayers.{K - 1}.correction_net.0.weight", f"gLayers.{K - 1}.rho", "gLayers.0.lambda_param"} <= want
    assert "hLayers.0.correction_net.0.weight" not in want and "gLayers.0.rho" not in want
    assert without_gradient("native") == want


def test_harness_train_step_on_the_native_route_with_the_head():
    """``python -m admm_net_amd.harness train-step --route native --head``: three steps on a small geometry, the loss finite and
    not rising."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "admm_net_amd.harness", "train-step", "--route", "native", "--head", "--layers", "3",
                        "--batch", "16", "--grid", "4x4", "--steps", "2", "--warmup", "1"], cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print(line)
    assert line["route"] == "native" and line["head"] is True
    assert np.isfinite(line["loss_first"]) and np.isfinite(line["loss_last"]) and line["loss_last"] <= line["loss_first"]
