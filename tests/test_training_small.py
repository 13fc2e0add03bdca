"""CPU: the full training route (``unrolled_forward(..., fused=True, small=True)`` / ``model.train_route = "full"``) with the
tensor stand-in ``training.TorchSmallKernels`` for the HIP kernels of csrc/train_small.hip.

* each of the five autograd functions with a hand-written backward (phi step, H input, H projection, eigenvalue map, step
  size), in complex128 / float64, against autograd through the existing tensor formulation (the bodies of
  ``training._phi_layer_gathered``, ``_h_layer``, ``_g_layer`` and ``_z_layer``): every output and every gradient, parameter
  gradients included, within 1e-12 of its largest entry -- tests/test_training_fused.py's rule, at its sizes.  The H
  projection's inputs hold signals with the scale clamped at 1 and signals with it open, and the test asserts that both occur;
  the step size runs with ``sub_batch`` and a short last group too (the one gradient whose own largest entry is no usable
  scale, g_rn where a group is a single signal, is explained at its assertion);
* the whole route on the committed reference-gradient fixtures under tests/test_training.py's own rule;
* ``sub_batch`` on the route under tests/test_training_fused.py's two bounds;
* the ``train_route`` knob and the argument checks of ``unrolled_forward``, the ops and the C entry points.
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
from oracle import admm_net_ref as R

import test_training as TT
from test_training_fused import SIZES, _close, _leaves

TSK = training.TorchSmallKernels
EPS = training.EPS
CPU = dict(solver=TT.cpu_eigh, assembler=training.TorchAssembler)
FULL = dict(fused=True, layer_kernels=training.TorchLayerKernels, small=True, small_kernels=TSK, **CPU)
F64, C128 = torch.float64, torch.complex128


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _scalar(g, lo=-1.0, hi=1.5):
    return (torch.rand((), dtype=F64, generator=g) * (hi - lo) + lo)


def _net(g, fan_in, hidden):
    """Linear - ReLU - Linear - Sigmoid in float64 with weights large enough that units sit on both sides of the ReLU."""
    net = nn.Sequential(nn.Linear(fan_in, hidden), nn.ReLU(), nn.Linear(hidden, 1), nn.Sigmoid()).double()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, dtype=F64, generator=g) * 0.7)
    return net


def _compare(out1, out2, a, b, up, names):
    _close(out1.detach(), out2.detach(), "output")
    g1 = torch.autograd.grad(out1, a, up)
    g2 = torch.autograd.grad(out2, b, up)
    assert len(g1) == len(names)
    for x, y, name in zip(g1, g2, names):
        _close(x, y, name)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_phi_step_function_matches_autograd(B, D, seed):
    g = _gen(seed)
    c = lambda: torch.randn(B, D, dtype=C128, generator=g)
    y, b, g_col, z_col, up = c(), c(), c(), c(), c()
    rho = _scalar(g)
    a = _leaves(g_col, z_col, rho)
    p1 = training._PhiStep.apply(y, b, a[0], a[1], a[2], TSK)
    q = _leaves(g_col, z_col, rho)
    p2 = training._phi_layer_gathered(SimpleNamespace(rho=q[2]), y, b, q[0], q[1])
    _compare(p1, p2, a, q, up, ("g_gcol", "g_zcol", "g_rho"))


def test_phi_step_above_the_softplus_threshold():
    """rho_raw > 20: softplus is the identity there and its derivative 1."""
    g = _gen(11)
    c = lambda: torch.randn(3, 5, dtype=C128, generator=g)
    y, b, g_col, z_col, up = c(), c(), c(), c(), c()
    rho = torch.tensor(23.5, dtype=F64)
    a, q = _leaves(g_col, z_col, rho), _leaves(g_col, z_col, rho)
    p1 = training._PhiStep.apply(y, b, a[0], a[1], a[2], TSK)
    p2 = training._phi_layer_gathered(SimpleNamespace(rho=q[2]), y, b, q[0], q[1])
    _compare(p1, p2, a, q, up, ("g_gcol", "g_zcol", "g_rho"))


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_h_input_function_matches_autograd(B, D, seed):
    g = _gen(seed + 100)
    r = lambda: torch.randn(B, D, dtype=F64, generator=g)
    g_dg, z_dg, up = r(), r(), r()
    rho = _scalar(g)
    a, q = _leaves(g_dg, z_dg, rho), _leaves(g_dg, z_dg, rho)
    t1 = training._HInput.apply(*a, TSK)
    t2 = q[0] + q[1] / (F.softplus(q[2]) + EPS)                        # the body of _h_layer
    _compare(t1, t2, a, q, up, ("g_gdg", "g_zdg", "g_rho"))


def _projection_inputs(B, D, seed):
    """2 B signals: the first B small and positive (0 < c < sigmoid(pw): the scale is clamped at 1), the others of size 5
    (the scale is open, or negative).  One entry of max |tc| is repeated with the other sign where D > 2, so that the
    argmax has a tie."""
    g = _gen(seed + 200)
    t = torch.cat([torch.randn(B, D, dtype=F64, generator=g).abs() * 0.02, torch.randn(B, D, dtype=F64, generator=g) * 5])
    m = torch.randn(2 * B, D, dtype=F64, generator=g) * 0.1
    if D > 2:
        tc = t + 0.1 * m
        i = tc.abs().argmax(dim=1)
        rows = torch.arange(2 * B)
        j = (i + 1) % D
        t[rows, j] = -tc[rows, i] - 0.1 * m[rows, j]                   # tc[j] = -tc[i]: the same magnitude
    sigma = torch.rand(2 * B, dtype=F64, generator=g) + 0.5
    pw = _scalar(g, 0.5, 1.5)
    up = torch.randn(2 * B, D, dtype=F64, generator=g)
    return t, m, sigma, pw, up


def _projection_body(D, t, m, sigma, pw):
    """The body of _h_layer behind its correction_net, with m in the place of ``layer.correction_net(t)``."""
    Acoef = (2 * torch.sqrt(torch.tensor(float(D))).to(t.device) * sigma + sigma ** 2).reshape(-1, 1)
    tc = t + 0.1 * m
    cval = Acoef * tc.abs().max(dim=1, keepdim=True)[0] + tc.sum(dim=1, keepdim=True)
    q = torch.sigmoid(pw) / (cval + EPS)
    return tc * torch.clamp(q, max=1.0), q


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_h_projection_function_matches_autograd(B, D, seed):
    t, m, sigma, pw, up = _projection_inputs(B, D, seed)
    a, b = _leaves(t, m, pw), _leaves(t, m, pw)
    h1 = training._HProject.apply(a[0], a[1], sigma, a[2], TSK)
    h2, q = _projection_body(D, b[0], b[1], sigma, b[2])
    clamped = int((q > 1).sum())
    print(f"B={B} D={D}: {clamped} of {2 * B} signals clamped")
    assert 0 < clamped < 2 * B, "the inputs must hold clamped and unclamped signals"
    _compare(h1, h2, a, b, up, ("g_t", "g_m", "g_pw"))


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_h_layer_through_both_functions_matches_autograd(B, D, seed):
    """_HInput, the correction_net module call and _HProject in a row against ``training._h_layer`` itself, the gradients of
    correction_net's weights included."""
    g = _gen(seed + 300)
    g_dg = torch.cat([torch.randn(B, D, dtype=F64, generator=g).abs() * 0.02, torch.randn(B, D, dtype=F64, generator=g) * 5])
    z_dg = torch.randn(2 * B, D, dtype=F64, generator=g) * 0.01
    sigma = torch.rand(2 * B, dtype=F64, generator=g) + 0.5
    up = torch.randn(2 * B, D, dtype=F64, generator=g)
    net = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, D), nn.Tanh()).double()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.05)                                                # a small correction: the clamped half stays clamped
    rho, pw = _scalar(g), _scalar(g, 0.5, 1.5)
    a, b = _leaves(g_dg, z_dg, rho, pw), _leaves(g_dg, z_dg, rho, pw)
    t = training._HInput.apply(a[0], a[1], a[2], TSK)
    h1 = training._HProject.apply(t, net(t), sigma, a[3], TSK)
    layer = SimpleNamespace(dim=D, rho=b[2], projection_weight=b[3], correction_net=net)
    h2 = training._h_layer(layer, None, None, sigma, (b[0], b[1]))
    params = list(net.parameters())
    _compare(h1, h2, a + params, b + params, up, ("g_gdg", "g_zdg", "g_rho", "g_pw", "gW1", "gb1", "gW2", "gb2"))


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_eigenvalue_map_function_matches_autograd(B, D, seed):
    g = _gen(seed + 400)
    n = D + 1
    w = torch.randn(B, n, dtype=F64, generator=g) * 3
    w[0, 0] = 0.0                                                       # d|w|/dw = 0 at 0
    up = torch.randn(B, n, dtype=F64, generator=g)
    net = _net(g, 1, 16)
    thr = _scalar(g)
    params = list(net.parameters())
    a, b = _leaves(w, thr), _leaves(w, thr)
    wp1 = training._EigMap.apply(a[0], a[1], *training._net_params(net), TSK)
    wp2 = F.softplus(b[0] - torch.sigmoid(b[1])) * net(b[0].abs().unsqueeze(-1)).squeeze(-1)       # the body of _g_layer
    _compare(wp1, wp2, a + params, b + params, up, ("g_w", "g_thr", "gW1", "gb1", "gW2", "gb2"))


def _step_body(rn, rho_raw, net, k, sub_batch, mean_constant=False):
    """The body of _z_layer between the residual norm and the update, with the two constant features in rn's dtype."""
    rho = F.softplus(rho_raw)
    mean = training._group_mean(rn, sub_batch)
    feat = torch.stack([torch.full_like(rn, k / 10.0), torch.full_like(rn, rho.item()),
                        rn / ((mean.detach() if mean_constant else mean) + EPS)], dim=1)
    return rho * (0.5 + 1.5 * net(feat)).squeeze(1)


STEP_CASES = [(B, seed, sb) for B, _, seed in SIZES for sb in (None, 2, 3)] + [(11, 9, 4), (7, 10, 7), (5, 11, 1)]


@pytest.mark.parametrize("B,seed,sub_batch", STEP_CASES)
def test_step_size_function_matches_autograd(B, seed, sub_batch):
    """(3, 2), (4, 3), (11, 4): a short last group; (7, 7): one group; (5, 1): single signals."""
    g = _gen(seed + 500)
    rn = torch.rand(B, dtype=F64, generator=g) * 4 + 0.1
    up = torch.randn(B, dtype=F64, generator=g)
    net = _net(g, 3, 32)
    rho = _scalar(g)
    k = 3
    params = list(net.parameters())
    a, b = _leaves(rn, rho), _leaves(rn, rho)
    s1 = training._StepSize.apply(a[0], a[1], *training._net_params(net), k / 10.0, sub_batch, TSK)
    s2 = _step_body(b[0], b[1], net, k, sub_batch)
    _close(s1.detach(), s2.detach(), "step")
    g1 = torch.autograd.grad(s1, a + params, up)
    g2 = torch.autograd.grad(s2, b + params, up)
    for x, y, name in list(zip(g1, g2, ("g_rn", "g_rho", "gW1", "gb1", "gW2", "gb2")))[1:]:
        _close(x, y, name)
    group = B if sub_batch is None else sub_batch
    if group > 1 and B % group != 1:
        _close(g1[0], g2[0], "g_rn")                 # every group has two signals or more: the rule of every other gradient
        return
    # A group of ONE signal occurs.  g_rn is the sum of a direct part (the mean held constant) and the mean's part, and in such
    # a group the two cancel to O(eps) of either: autograd's own value is then round-off of the parts, not of the sum, and
    # measured against its own largest entry no two evaluation orders agree to 1e-12 (an ulp of the parts is 1e-8 of the sum).
    # So here the error of g_rn is held to 1e-12 of the larger of its own largest entry and the direct part's largest entry --
    # float64 round-off on a sum of two terms.
    direct = torch.autograd.grad(_step_body(b[0], b[1], net, k, sub_batch, mean_constant=True), b[0], up)[0]
    err, scale = (g1[0] - g2[0]).abs().max().item(), max(g2[0].abs().max().item(), direct.abs().max().item())
    print(f"g_rn: error {err:.3e}, own largest entry {g2[0].abs().max().item():.3e}, direct part {direct.abs().max().item():.3e}")
    assert g1[0].shape == g2[0].shape and err <= 1e-12 * scale, f"g_rn: {err:.3e} against {scale:.3e}"


def test_some_step_case_has_a_short_last_group():
    assert any(sb is not None and sb < B and B % sb for B, _, sb in STEP_CASES)


def test_terms_sum_to_the_backward():
    """The unsummed ``_terms`` forms (what the GPU tests build their sum |terms| bounds from) add up to the ``_bwd`` forms."""
    g = _gen(77)
    t, m, sigma, pw, up = _projection_inputs(3, 6, 5)
    assert torch.equal(TSK.hproject_terms(up, t, m, sigma, pw)[2].sum(), TSK.hproject_bwd(up, t, m, sigma, pw)[2])
    rn, net = torch.rand(5, dtype=F64, generator=g) + 0.1, _net(g, 3, 32)
    gs = torch.randn(5, dtype=F64, generator=g)
    args = (gs, rn, _scalar(g), *training._net_params(net), 0.3, 2)
    terms, bwd = TSK.stepsize_terms(*args), TSK.stepsize_bwd(*args)
    assert torch.equal(terms[0], bwd[0])
    for x, y in zip(terms[1:], bwd[1:]):
        assert torch.allclose(x.sum(dim=0).reshape(y.shape), y, rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ the route
@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_full_route_matches_reference_gradients(path):
    z, m, head, t = TT.load(path)
    m.eval()   # fixture convention: dropout off
    out = training.unrolled_forward(m, t("y"), t("b"), t("sigma"), **FULL)
    phi = out[3] if head else out
    assert np.abs(phi.detach().numpy() - z["phi"]).max() <= 2e-5 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


def _sb_model(Nb, Nd, K, seed):
    sd = R.make_weights(Nb, Nd, K, seed=seed, head=True, perturb=0.3)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K)
    m.load_state_dict(sd)
    return m.eval()


def _sb_loss(out, seed):
    g = torch.Generator().manual_seed(seed)
    tau, f, conf, phi = out
    c_phi = torch.randn(phi.shape, dtype=torch.complex64, generator=g)
    return ((c_phi.conj() * phi).real.sum() + (torch.randn(tau.shape, generator=g) * tau).sum()
            + (torch.randn(f.shape, generator=g) * f).sum() + (torch.randn(conf.shape, generator=g) * conf).sum())


@pytest.mark.parametrize("B,g", [(11, 4), (9, 1), (10, 5)])
def test_full_route_groups_equal_separate_batches(B, g):
    """tests/test_training_fused.py::test_fused_route_groups_equal_separate_batches on the full route, same two bounds: the
    outputs of one grouped call equal the per-group calls to 1e-6 of the largest entry, the parameter gradients the SUM of
    the per-group calls' gradients to 1e-5 max + 1e-7."""
    Nb, Nd, K = 3, 4, 3
    m = _sb_model(Nb, Nd, K, seed=21)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=5)
    y, b, s = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    grads = lambda: {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}

    m.zero_grad(set_to_none=True)
    out = training.unrolled_forward(m, y, b, s, sub_batch=g, **FULL)
    _sb_loss(out, 1).backward()
    got = grads()

    m.zero_grad(set_to_none=True)
    parts = [training.unrolled_forward(m, y[lo:lo + g], b[lo:lo + g], s[lo:lo + g], **FULL) for lo in range(0, B, g)]
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
    whole = training.unrolled_forward(m, y, b, s, **FULL)
    assert (whole[3] - sep[3]).abs().max() > 1e-5 * sep[3].abs().max()


def test_corners_are_resolved_with_the_values_of_the_per_layer_reads():
    m = _sb_model(3, 4, 4, seed=3)
    got = training._resolve_corners(m, 4)
    assert len(got) == 3
    for k, (cg, cz) in enumerate(got):
        assert cg == (1.0 / (F.softplus(m.gLayers[k].lambda_param) ** 2 + EPS)).item()
        assert cz == (1.0 / (F.softplus(m.zLayers[k].lambda_param) ** 2 + EPS)).item()
    assert training._resolve_corners(m, 1) == []


def test_single_layer_model_runs_on_the_full_route():
    m = A.PhiEstADMMNet(M=2, N=2, num_layers=1)
    y = torch.ones(2, 4, dtype=torch.complex64)
    phi = training.unrolled_forward(m, y, y, torch.ones(2), **FULL)
    want = training.unrolled_forward(m, y, y, torch.ones(2), **CPU)
    assert (phi - want).abs().max() <= 1e-6 * want.abs().max()


def test_train_route_knob_accepts_full():
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    keys = set(m.state_dict())
    m.train_route = "full"
    assert m.train_route == "full" and set(m.state_dict()) == keys
    for bad in ("Fused", "", None, 1, "hip", "Full", "small", ("full",)):
        with pytest.raises(ValueError):
            m.train_route = bad
    assert m.train_route == "full"
    m.train_route = "tensor"


def test_small_needs_fused_and_small_kernels_need_small():
    m = A.PhiEstADMMNet(M=2, N=2, num_layers=2)
    y = torch.ones(1, 4, dtype=torch.complex64)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), small=True, **CPU)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), small=True, small_kernels=TSK, **CPU)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), fused=True, layer_kernels=training.TorchLayerKernels,
                                  small_kernels=TSK, **CPU)


def test_train_small_ops_refuse_cpu_tensors():
    from admm_net_amd import _lib, ops
    g = _gen(0)
    c = torch.randn(2, 3, dtype=torch.complex64, generator=g)
    r = torch.randn(2, 3, generator=g)
    w, v, s = torch.randn(2, 4, generator=g), torch.rand(2, generator=g), torch.tensor(0.5)
    e = training._net_params(nn.Sequential(nn.Linear(1, 16), nn.ReLU(), nn.Linear(16, 1), nn.Sigmoid()))
    z = training._net_params(nn.Sequential(nn.Linear(3, 32), nn.ReLU(), nn.Linear(32, 1), nn.Sigmoid()))
    for call in (lambda: ops.train_phi(c, c, c, c, s), lambda: ops.train_phi_bwd(c, c, c, c, c, s),
                 lambda: ops.train_hinput(r, r, s), lambda: ops.train_hinput_bwd(r, r, s),
                 lambda: ops.train_hproject(r, r, v, s), lambda: ops.train_hproject_bwd(r, r, r, v, s),
                 lambda: ops.train_eigmap(w, s, *e), lambda: ops.train_eigmap_bwd(w, w, s, *e),
                 lambda: ops.train_stepsize(v, s, *z, 0.3), lambda: ops.train_stepsize_bwd(v, v, s, *z, 0.3, 2)):
        with pytest.raises(_lib.AdmmNetError):
            call()


def test_train_small_entry_points_reject_bad_arguments():
    """ADMMNET_E_ARG (-1) for D outside 1 ... 256 (n outside 2 ... 257), B < 1, a negative sub_batch, a slab grid beyond 31 bits
    and null pointers -- decided on the host before anything is launched."""
    import ctypes
    from admm_net_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)
    PHI, HIN, HPR, EIG, STEP = range(5)
    part = lib.admmnet_train_small_partials
    assert part(PHI, 256, 0) == 64 and part(HIN, 257, 0) == 65 and part(HPR, 1, 0) == 1
    assert part(EIG, 256, 0) == 64 * 50 and part(EIG, 3, 0) == 50
    assert part(STEP, 256, 0) == 162 + 256 and part(STEP, 11, 4) == 3 * 162 + 11 and part(STEP, 4, 9) == 162 + 4
    assert part(5, 4, 0) == -1 and part(-1, 4, 0) == -1 and part(PHI, 0, 0) == -1 and part(STEP, 4, -1) == -1
    for d, B in ((0, 4), (257, 4), (100, 0), (100, 2 ** 33 + 1)):
        assert lib.admmnet_train_phi_c64(d, B, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_phi_bwd_c64(d, B, p, p, p, p, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_hinput_f32(d, B, p, p, p, p, null) == -1
        assert lib.admmnet_train_hinput_bwd_f32(d, B, p, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_hproject_f32(d, B, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_hproject_bwd_f32(d, B, p, p, p, p, p, p, p, p, p, null) == -1
    for n, B in ((1, 4), (258, 4), (101, 0), (101, 2 ** 33 + 1)):
        assert lib.admmnet_train_eigmap_f32(n, B, p, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_eigmap_bwd_f32(n, B, p, p, p, p, p, p, p, p, p, p, null) == -1
    for B, g in ((0, 0), (4, -1), (2 ** 33, 1)):
        assert lib.admmnet_train_stepsize_f32(B, g, 0.3, p, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_stepsize_bwd_f32(B, g, 0.3, p, p, p, p, p, p, p, p, p, p, null) == -1
    assert b"train_stepsize_bwd" in lib.admmnet_last_error()
    assert lib.admmnet_train_phi_c64(100, 4, p, p, null, p, p, p, null) == -1
    assert lib.admmnet_train_phi_bwd_c64(100, 4, p, p, p, p, p, p, p, p, p, null, null) == -1
    assert lib.admmnet_train_hinput_f32(100, 4, p, p, null, p, null) == -1
    assert lib.admmnet_train_hinput_bwd_f32(100, 4, p, p, p, p, p, null, p, null) == -1
    assert lib.admmnet_train_hproject_f32(100, 4, p, p, p, p, null, null) == -1
    assert lib.admmnet_train_hproject_bwd_f32(100, 4, p, p, p, null, p, p, p, p, p, null) == -1
    assert lib.admmnet_train_eigmap_f32(101, 4, p, null, p, p, p, p, p, null) == -1
    assert lib.admmnet_train_eigmap_bwd_f32(101, 4, p, p, p, p, p, p, p, p, null, p, null) == -1
    assert lib.admmnet_train_stepsize_f32(4, 0, 0.3, null, p, p, p, p, p, p, null) == -1
    assert lib.admmnet_train_stepsize_bwd_f32(4, 2, 0.3, p, p, p, p, p, p, p, p, p, null, null) == -1
