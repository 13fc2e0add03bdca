"""GPU: the full training route -- the kernels of csrc/train_small.hip (``ops.train_phi`` ... ``ops.train_stepsize`` and their
``_bwd`` forms) against float64 evaluations of their definitions, and ``model.train_route = "full"`` end to end.

The float64 definitions are ``training.TorchSmallKernels`` in float64 / complex128 on the float32 inputs the kernels read
(tests/test_training_small.py holds those formulas to autograd through the existing tensor formulation at 1e-12).

Bounds:
  * elementwise outputs (phi, t, h, wp, step and the [B, D]-shaped gradients): the steps chain exp / log1p-class functions in
    float32, so the yardstick is the parent's arithmetic for the same step -- the float32 tensor formulation of training.py
    evaluated on the GPU, gradients by autograd.  The kernel must be no further from float64 than 3 x that distance plus 1e-6
    of the largest entry;
  * reductions over the batch (parameter gradients, g_rho, g_pw): 2e-5 sum|terms| with the sum of magnitudes taken in float64 --
    tests/test_gpu_training_fused.py's bound;
  * every backward run twice gives ``torch.equal`` results.
Each test prints the worst figures it saw.

Worst figures measured on an MI355X are recorded in DESIGN.md section 4.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import admm_net_amd as A
from admm_net_amd import ops, synth, training

import test_training as TT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = training.EPS
TSK = training.TorchSmallKernels
RED = 2e-5
SHAPES = [(D, B) for D in (1, 7, 100, 128, 192, 256) for B in (1, 3, 256)] + [(100, 4099)]     # 4099: 1025 slabs, a ragged last one
IDS = [f"D{D}-B{B}" for D, B in SHAPES]


def _f64(t):
    return t.detach().cpu().to(torch.complex128 if t.is_complex() else torch.float64)


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


class Worst:
    def __init__(self, what):
        self.what, self.elem_ratio, self.red_ratio = what, 0.0, 0.0

    def elem(self, got, parent, want, name):
        """|kernel - f64| <= 3 |parent - f64| + 1e-6 max|f64|, all in the max norm over the tensor."""
        want = _f64(want)
        assert got.shape == want.shape, name
        err = (_f64(got) - want).abs().max().item()
        perr = (_f64(parent) - want).abs().max().item()
        bound = 3 * perr + 1e-6 * want.abs().max().item()
        print(f"  {self.what} {name}: kernel {err:.3e}, parent {perr:.3e}, bound {bound:.3e}")
        if bound > 0:
            self.elem_ratio = max(self.elem_ratio, err / bound)
        assert err <= bound, f"{name}: kernel {err:.3e} from float64, parent {perr:.3e}, bound {bound:.3e}"

    def red(self, got, want, mag, name):
        """mag: sum of the magnitudes of the terms of every entry, float64."""
        want, mag = _f64(want), _f64(mag).reshape(want.shape)
        assert got.shape == want.shape, name
        ratio = ((_f64(got) - want).abs() / (RED * mag + 1e-300)).max().item()
        print(f"  {self.what} {name}: error / (2e-5 sum|terms|) = {ratio:.3f}")
        self.red_ratio = max(self.red_ratio, ratio)
        assert ratio <= 1.0, f"{name}: error / (2e-5 sum|terms|) = {ratio:.3f}"

    def done(self):
        print(f"{self.what}: worst elementwise error / bound {self.elem_ratio:.3f}, worst reduction error / bound {self.red_ratio:.3f}")


def _same_twice(fn):
    a, b = fn(), fn()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "two runs on the same inputs must give the same bits"
    return a


def _small_net(g, fan_in, hidden):
    net = nn.Sequential(nn.Linear(fan_in, hidden), nn.ReLU(), nn.Linear(hidden, 1), nn.Sigmoid())
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.7)
    return net.to(DEV)


# ------------------------------------------------------------------------------------------------ phi
def _phi_case(D, B, seed, wrap=lambda t: t):
    g = torch.Generator().manual_seed(seed)
    c = lambda: wrap(torch.randn(B, D, dtype=torch.complex64, generator=g).to(DEV))
    return c(), c(), c(), c(), c(), (torch.rand((), generator=g) * 2 - 0.5).to(DEV)


def _check_phi(D, B, y, b, g_col, z_col, up, rho, what):
    worst = Worst(what)
    w = [_f64(t) for t in (y, b, g_col, z_col, rho)]
    a = _leaves(g_col, z_col, rho)
    parent = training._phi_layer_gathered(SimpleNamespace(rho=a[2]), y, b, a[0], a[1])
    pg = torch.autograd.grad(parent, a, up)
    phi = ops.train_phi(y, b, g_col, z_col, rho)
    worst.elem(phi, parent, TSK.phi(*w), "phi")
    g_gcol, g_zcol, g_rho = _same_twice(lambda: ops.train_phi_bwd(up, y, b, g_col, z_col, rho))
    want = TSK.phi_bwd(_f64(up), *w)
    worst.elem(g_gcol, pg[0], want[0], "g_gcol")
    worst.elem(g_zcol, pg[1], want[1], "g_zcol")
    # g_rho = softplus'(rho) sum Re(conj(g_phi) d), d = d phi / d r: per term |Re Re| + |Im Im| of the two factors, as
    # tests/test_gpu_training_fused.py takes its g_r and g_s
    r, coef, inner = TSK._phi_parts(*w)
    u, d = _f64(up), coef * w[2] - coef ** 2 * inner
    mag = ((u.real * d.real).abs() + (u.imag * d.imag).abs()).sum() * training._dsoftplus(w[4])
    worst.red(g_rho, want[2], mag, "g_rho")
    worst.done()


@pytest.mark.parametrize("D,B", SHAPES, ids=IDS)
def test_phi_kernels_match_their_definition(D, B):
    _check_phi(D, B, *_phi_case(D, B, seed=D + B), f"phi D={D} B={B}")


# ------------------------------------------------------------------------------------------------ H input
def _check_hinput(g_dg, z_dg, up, rho, what):
    worst = Worst(what)
    w = [_f64(t) for t in (g_dg, z_dg, rho)]
    a = _leaves(g_dg, z_dg, rho)
    parent = a[0] + a[1] / (F.softplus(a[2]) + EPS)                           # the body of _h_layer
    pg = torch.autograd.grad(parent, a, up)
    worst.elem(ops.train_hinput(g_dg, z_dg, rho), parent, TSK.hinput(*w), "t")
    g_gdg, g_zdg, g_rho = _same_twice(lambda: ops.train_hinput_bwd(up, z_dg, rho))
    want = TSK.hinput_terms(_f64(up), w[1], w[2])
    worst.elem(g_gdg, pg[0], want[0], "g_gdg")
    worst.elem(g_zdg, pg[1], want[1], "g_zdg")
    worst.red(g_rho, want[2].sum(), want[2].abs().sum(), "g_rho")
    worst.done()


@pytest.mark.parametrize("D,B", SHAPES, ids=IDS)
def test_hinput_kernels_match_their_definition(D, B):
    g = torch.Generator().manual_seed(1000 + D + B)
    r = lambda: torch.randn(B, D, generator=g).to(DEV)
    _check_hinput(r(), r(), r(), (torch.rand((), generator=g) * 2 - 0.5).to(DEV), f"hinput D={D} B={B}")


# ------------------------------------------------------------------------------------------------ H projection
def _project_case(D, B, seed):
    """Even signals: small positive t with c near 0.1, below sigmoid(pw) >= 0.62 -- the scale is clamped at 1; odd signals: t of
    size 5 -- the scale is open (or negative)."""
    g = torch.Generator().manual_seed(seed)
    small = torch.randn(B, D, generator=g).abs() * (0.1 / (D + 6 * D ** 0.5 + 1))
    t = torch.where((torch.arange(B) % 2 == 0).reshape(-1, 1), small, torch.randn(B, D, generator=g) * 5)
    m = torch.randn(B, D, generator=g) * 0.1 * t.abs().mean(dim=1, keepdim=True)
    sigma = torch.rand(B, generator=g) + 0.5
    pw = torch.rand((), generator=g) + 0.5
    return _dev(t, m, sigma, pw, torch.randn(B, D, generator=g))


def _check_hproject(D, B, t, m, sigma, pw, up, what):
    worst = Worst(what)
    w = [_f64(x) for x in (t, m, sigma, pw)]
    a = _leaves(t, m, pw)
    layer = SimpleNamespace(dim=D, rho=torch.zeros((), device=DEV), projection_weight=a[2], correction_net=lambda _t: a[1])
    parent = training._h_layer(layer, None, None, sigma, (a[0], torch.zeros_like(t)))     # t + 0 / (rho + eps) = t
    pg = torch.autograd.grad(parent, a, up)
    worst.elem(ops.train_hproject(t, m, sigma, pw), parent, TSK.hproject(*w), "h")
    g_t, g_m, g_pw = _same_twice(lambda: ops.train_hproject_bwd(up, t, m, sigma, pw))
    want = TSK.hproject_terms(_f64(up), *w)
    worst.elem(g_t, pg[0], want[0], "g_t")
    worst.elem(g_m, pg[1], want[1], "g_m")
    _, tc, _, den, sp = TSK._project_parts(*w)
    q = sp / den
    clamped = int((q > 1).sum())
    print(f"  {what}: {clamped} of {B} signals clamped")
    if B > 1:
        assert 0 < clamped < B, "the inputs must hold clamped and unclamped signals"
    mag = ((_f64(up) * tc).abs().sum(dim=1, keepdim=True) * (q <= 1) / den.abs() * sp * (1 - sp)).sum()
    worst.red(g_pw, want[2].sum(), mag, "g_pw")
    worst.done()


@pytest.mark.parametrize("D,B", SHAPES, ids=IDS)
def test_hproject_kernels_match_their_definition(D, B):
    _check_hproject(D, B, *_project_case(D, B, seed=2000 + D + B), f"hproject D={D} B={B}")


# ------------------------------------------------------------------------------------------------ eigenvalue map
def _check_eigmap(w_, up, thr, net, what):
    worst = Worst(what)
    pars = training._net_params(net)
    w64 = [_f64(x) for x in (w_, thr, *pars)]
    (a_w, a_thr), params = _leaves(w_, thr), list(net.parameters())
    parent = F.softplus(a_w - torch.sigmoid(a_thr)) * net(a_w.abs().unsqueeze(-1)).squeeze(-1)      # the body of _g_layer
    pg = torch.autograd.grad(parent, [a_w, a_thr] + params, up)
    worst.elem(ops.train_eigmap(w_, thr, *pars), parent, TSK.eigmap(*w64), "wp")
    got = _same_twice(lambda: ops.train_eigmap_bwd(up, w_, thr, *pars))
    terms = TSK.eigmap_terms(_f64(up), *w64)
    worst.elem(got[0], pg[0], terms[0], "g_w")
    for x, t, name in zip(got[1:], terms[1:], ("g_thr", "gW1", "gb1", "gW2", "gb2")):
        dims = (0, 1) if t.dim() == 3 else None
        worst.red(x, t.sum(dim=dims).reshape(x.shape), t.abs().sum(dim=dims), name)
    worst.done()


@pytest.mark.parametrize("D,B", SHAPES, ids=IDS)
def test_eigmap_kernels_match_their_definition(D, B):
    g = torch.Generator().manual_seed(3000 + D + B)
    n = D + 1
    w_ = torch.randn(B, n, generator=g) * 3
    w_[0, 0] = 0.0
    up = torch.randn(B, n, generator=g)
    net = _small_net(g, 1, 16)
    _check_eigmap(*_dev(w_, up, torch.rand((), generator=g) * 2 - 1), net, f"eigmap n={n} B={B}")


# ------------------------------------------------------------------------------------------------ step size
def _check_stepsize(B, sub_batch, seed, what, k=3, wrap=lambda t: t):
    worst = Worst(what)
    g = torch.Generator().manual_seed(seed)
    rn, up, rho = _dev(torch.rand(B, generator=g) * 4 + 0.1, torch.randn(B, generator=g), torch.rand((), generator=g) * 2 - 0.5)
    rn, up = wrap(rn), wrap(up)
    net = _small_net(g, 3, 32)
    pars = training._net_params(net)
    w64 = [_f64(x) for x in (rn, rho, *pars)]
    (a_rn, a_rho), params = _leaves(rn, rho), list(net.parameters())
    r = F.softplus(a_rho)                                                     # the body of _z_layer
    feat = torch.stack([torch.full((B,), k / 10.0, device=DEV), torch.full((B,), r.item(), device=DEV),
                        a_rn / (training._group_mean(a_rn, sub_batch) + EPS)], dim=1)
    parent = r * (0.5 + 1.5 * net(feat)).squeeze(1)
    pg = torch.autograd.grad(parent, [a_rn, a_rho] + params, up)
    knorm = float(np.float32(k / 10.0))                                       # the value the float32 feature holds
    worst.elem(ops.train_stepsize(rn, rho, *pars, k / 10.0, sub_batch), parent, TSK.stepsize(*w64, knorm, sub_batch), "step")
    got = _same_twice(lambda: ops.train_stepsize_bwd(up, rn, rho, *pars, k / 10.0, sub_batch))
    terms = TSK.stepsize_terms(_f64(up), *w64, knorm, sub_batch)
    worst.elem(got[0], pg[0], terms[0], "g_rn")
    for x, t, name in zip(got[1:], terms[1:], ("g_rho", "gW1", "gb1", "gW2", "gb2")):
        worst.red(x, t.sum(dim=0).reshape(x.shape), t.abs().sum(dim=0), name)
    worst.done()


@pytest.mark.parametrize("B,sub_batch", [(1, None), (3, None), (256, None), (4099, None), (256, 100), (11, 4), (3, 2), (7, 1),
                                         (4099, 2), (300, 300), (5, 9)])
def test_stepsize_kernels_match_their_definition(B, sub_batch):
    """(256, 100), (11, 4), (3, 2), (4099, 2): a short last group; (7, 1): single signals; 4099 signals in one group: more than
    one pass of the workgroup; (4099, 2): 2050 workgroups."""
    _check_stepsize(B, sub_batch, seed=4000 + B + (sub_batch or 0), what=f"stepsize B={B} sub_batch={sub_batch}")


# ------------------------------------------------------------------------------------------------ unaligned views
def test_kernels_on_unaligned_views():
    """[B, D] tensors (and the [B] ones of the step size) that start 4 bytes (float) / 8 bytes (complex64) behind an aligned
    base, at an odd D: the same definitions, the same bounds."""
    D, B = 7, 5

    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v

    _check_phi(D, B, *_phi_case(D, B, seed=5, wrap=off)[:5], torch.tensor(0.4, device=DEV), "unaligned phi")
    g = torch.Generator().manual_seed(6)
    r = lambda: off(torch.randn(B, D, generator=g).to(DEV))
    _check_hinput(r(), r(), r(), torch.tensor(0.4, device=DEV), "unaligned hinput")
    t, m, sigma, pw, up = _project_case(D, B, seed=7)
    _check_hproject(D, B, off(t), off(m), off(sigma), pw, off(up), "unaligned hproject")
    w_, up = off(torch.randn(B, D + 1, generator=g).to(DEV) * 3), off(torch.randn(B, D + 1, generator=g).to(DEV))
    _check_eigmap(w_, up, torch.tensor(0.2, device=DEV), _small_net(g, 1, 16), "unaligned eigmap")
    _check_stepsize(11, 4, seed=8, what="unaligned stepsize", wrap=off)


# ------------------------------------------------------------------------------------------------ the route, end to end
def _run(path, route):
    z, m, head, t = TT.load(path, DEV)
    m.train_route = route
    if head:
        m.eval()                                          # attention dropout off, as in the fixture
        out = m.forward_autograd(t("y"), t("b"), t("sigma"))
    else:
        m.train()                                         # the call trainPhi.py makes
        out = m(t("y"), t("b"), t("sigma"))
    return z, m, head, t, out


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_full_route_gradients_match_reference(path):
    """tests/test_training.py::test_hip_training_gradients_match_reference with ``train_route = "full"``."""
    z, m, head, t, out = _run(path, "full")
    phi = out[3] if head else out
    assert phi.requires_grad and phi.is_cuda
    assert np.abs(phi.detach().cpu().numpy() - z["phi"]).max() <= 1e-4 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_full_and_tensor_route_give_the_same_phi(path):
    """The rule of tests/test_gpu_training_fused.py::test_fused_and_tensor_route_give_the_same_phi."""
    _, _, head, _, a = _run(path, "full")
    _, _, _, _, b = _run(path, "tensor")
    pa, pb = (a[3], b[3]) if head else (a, b)
    err = (pa - pb).abs().max().item() / pb.abs().max().item()
    print(f"full against tensor route: phi differs by {err:.2e} of its largest entry")
    assert err <= 2e-5


@pytest.mark.parametrize("cls,sub_batch", [(A.PhiEstADMMNet, None), (A.PhiEstADMMNet, 2), (A.ADMMNet, None), (A.ADMMNet, 2)],
                         ids=["phi-net", "phi-net-sub2", "head-net", "head-net-sub2"])
def test_full_route_at_16x16_trains_and_matches_inference(cls, sub_batch):
    """16 x 16 (n = 257), K = 3, B = 8, as tests/test_gpu_training_fused.py::test_fused_route_at_16x16_trains_and_matches_inference:
    the train-mode phi of the full route agrees with the eval-mode inference phi to 1e-4, all gradients are finite, six AdamW
    steps lower the loss.  With the head the loss is still phi's (the head's dropout is live in train mode)."""
    dev = torch.device(DEV)
    torch.manual_seed(3)
    m = cls(M=16, N=16, num_layers=3).to(dev)
    m.train_route, m.sub_batch = "full", sub_batch
    y, b, sigma, _ = synth.make_batch(8, 16, 16, seed=5)
    ty, tb, ts = (torch.from_numpy(v).to(dev) for v in (y, b, sigma))
    target = ty / tb
    phi_of = lambda out: out[3] if isinstance(out, tuple) else out
    m.train()
    phi_train = phi_of(m(ty, tb, ts))
    m.eval()
    with torch.no_grad():
        phi_eval = phi_of(m(ty, tb, ts))
    err = (phi_train - phi_eval).abs().max().item() / phi_eval.abs().max().item()
    print(f"train-mode against inference phi: {err:.2e}")
    assert err <= 1e-4
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = (phi_of(m(ty, tb, ts)) - target).abs().pow(2).mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        losses.append(loss.item())
    print("losses:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
