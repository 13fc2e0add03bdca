"""GPU: the loss kernels of csrc/loss.hip (``ops.loss_anm`` / ``loss_phi`` and their ``_bwd`` forms) against the float64
tensor formulation ``losses.TensorLossKernels`` on the float32 inputs the kernels read (tests/test_losses.py holds that
formulation to the reference's own numbers and to autograd), the modules on ``route = "hip"``, and one training step end to end.

Bounds (the rule of tests/test_gpu_training_small.py, whose ``Worst`` keeps the figures):
  * elementwise outputs (the norms, every gradient): no further from float64 than 3 x the distance of the float32 tensor
    formulation evaluated on the GPU, plus 1e-6 of the largest entry;
  * sums over the batch (the three loss values): within 2e-5 sum|terms|.  Every term of param, reg, amplitude and phase is
    non-negative, so that sum is the float64 value itself; total adds two of them with non-negative weights;
  * gradients at j >= L and at phi = 0 are exactly 0; every forward and backward run twice gives equal bits.
Phase inputs keep 1e-3 rad from +-pi in the raw difference, a quarter of them beyond it (tests/loss_cases.py).
Each test prints the worst figures it saw; those measured on an MI355X are recorded in DESIGN.md section 4.
"""
import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import losses, ops, synth
from admm_net_amd.losses import TensorLossKernels as TLK

import loss_cases as LC
from test_gpu_training_small import Worst, _f64, _same_twice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("tau", "f", "conf", "tau_true", "f_true", "L_true", "phi")
LAM, AW, PW = 0.37, 0.8, 0.45
UP = (1.7, 0.3, -0.6)                              # gradients of (total, first part, second part)
SIZES = [(B, Lmax, D) for B in (1, 3, 4, 5, 257) for Lmax in (1, 3, 64) for D in (1, 7, 100, 256)]
PHI_SIZES = [(B, D) for B in (1, 3, 4, 5, 257) for D in (1, 7, 100, 256)]


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _args64(c):
    return [c[k].cpu() if k == "L_true" else _f64(c[k]) for k in KEYS]


def _check_anm(c, what, worst=None):
    """c: device inputs.  Forward and backward of the kernels against float64; returns what the kernels gave."""
    worst = worst or Worst(what)
    a = [c[k] for k in KEYS]
    a64 = _args64(c)
    out, norms, status = _same_twice(lambda: ops.loss_anm(*a, LAM))
    w_out, w_norms, _ = TLK.anm(*a64, LAM)
    p_out, p_norms, _ = TLK.anm(*a, LAM)                                       # the float32 tensor formulation on the GPU
    assert out.dtype == torch.float32 and out.shape == (3,) and status.item() == 0
    worst.red(out, w_out, w_out, "total, param, reg")
    worst.elem(norms, p_norms, w_norms, "norms")
    up = torch.tensor(UP, device=DEV)
    got = _same_twice(lambda: ops.loss_anm_bwd(up, *a, norms, LAM))
    want = TLK.anm_bwd(_f64(up), *a64, w_norms, LAM)
    parent = TLK.anm_bwd(up, *a, p_norms, LAM)
    for g, p, w, name in zip(got, parent, want, ("g_tau", "g_f", "g_conf", "g_phi")):
        worst.elem(g, p, w, name)
    Lmax = c["tau"].shape[1]
    L = c["L_true"].clamp(0, Lmax).reshape(-1, 1)
    j = torch.arange(Lmax, device=DEV)
    for g, name in zip(got[:3], ("g_tau", "g_f", "g_conf")):
        assert not g[(j >= L) & (L >= 1)].any(), f"{name} must be exactly 0 at j >= L"
    assert not got[0][(L == 0).reshape(-1)].any() and not got[1][(L == 0).reshape(-1)].any()
    assert not got[3][norms == 0].any(), "g_phi must be exactly 0 where the norm is 0"
    worst.done()
    return out, norms, got


@pytest.mark.parametrize("B,Lmax,D", SIZES, ids=[f"B{B}-L{L}-D{D}" for B, L, D in SIZES])
def test_anm_kernels_match_their_definition(B, Lmax, D):
    worst = Worst(f"anm B={B} Lmax={Lmax} D={D}")
    for L in ("mixed", "none", "all"):
        c = _dev(LC.anm_case(B, Lmax, D, seed=B + Lmax + D, L=L))
        if B > 1:
            assert not c["phi"][-1].any()
        _check_anm(c, None, worst)


def _check_phi(phi, phi_true, what):
    worst = Worst(what)
    LC.check_phase_margin(phi.cpu(), phi_true.cpu())
    p64, t64 = _f64(phi), _f64(phi_true)
    (out,) = _same_twice(lambda: (ops.loss_phi(phi, phi_true, AW, PW),))
    assert out.dtype == torch.float32 and out.shape == (3,)
    want = TLK.phi(p64, t64, AW, PW)
    worst.red(out, want, want, "total, amplitude, phase")
    up = torch.tensor(UP, device=DEV)
    (g,) = _same_twice(lambda: (ops.loss_phi_bwd(up, phi, phi_true, AW, PW),))
    worst.elem(g, TLK.phi_bwd(up, phi, phi_true, AW, PW), TLK.phi_bwd(_f64(up), p64, t64, AW, PW), "g_phi")
    assert not g[phi == 0].any(), "g_phi must be exactly 0 where phi is 0"
    worst.done()
    return out, g


@pytest.mark.parametrize("B,D", PHI_SIZES, ids=[f"B{B}-D{D}" for B, D in PHI_SIZES])
def test_phi_kernels_match_their_definition(B, D):
    phi, phi_true = (t.to(DEV) for t in LC.phase_pair(B, D, seed=B + D))
    if B * D > 1:
        assert (phi == 0).sum().item() == 1
    _check_phi(phi, phi_true, f"phi B={B} D={D}")


def _offset(t):
    """The same values one element behind an aligned base: 4 bytes (float), 8 bytes (complex64, int64)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _strided(t):
    """The same values as every second column (or entry) of a wider tensor."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=DEV)
    v = wide[..., ::2]
    v.copy_(t)
    assert not v.is_contiguous() or t.shape[-1] == 1
    return v


@pytest.mark.parametrize("view", [_offset, _strided], ids=["offset", "strided"])
def test_kernels_on_views(view):
    c = _dev(LC.anm_case(5, 3, 7, seed=11))
    plain = _check_anm(c, "anm plain")
    seen = _check_anm({k: view(v) for k, v in c.items()}, f"anm {view.__name__}")
    assert all(torch.equal(a, b) for a, b in zip((plain[0], plain[1], *plain[2]), (seen[0], seen[1], *seen[2])))
    phi, phi_true = (t.to(DEV) for t in LC.phase_pair(5, 7, seed=12))
    plain = _check_phi(phi, phi_true, "phi plain")
    seen = _check_phi(view(phi), view(phi_true), f"phi {view.__name__}")
    assert torch.equal(plain[0], seen[0]) and torch.equal(plain[1], seen[1])


def _anm_call(m, c, leaves=None):
    s = leaves or c
    return m({"tau_est": s["tau"], "f_est": s["f"], "confidences": s["conf"], "phi_final": s["phi"]},
             {"tau_true": c["tau_true"], "f_true": c["f_true"], "L_true": c["L_true"]})


def test_status_word_counts_out_of_range_targets():
    """Three of seven L_true lie outside [0, 3]: the status word says 3, the module raises, and with ``check_status = False``
    the call returns what the definition gives with L held to [0, 3] -- the kernel's own reads stay inside [B, Lmax]."""
    bad = [0, 4, 2, -1, 3, 1 << 40, 1]
    c = _dev(LC.anm_case(7, 3, 20, seed=13, L=bad))
    held = dict(c, L_true=c["L_true"].clamp(0, 3))
    a = lambda d: [d[k] for k in KEYS]
    out, norms, status = ops.loss_anm(*a(c), LAM)
    assert status.item() == 3
    want = ops.loss_anm(*a(held), LAM)
    assert want[2].item() == 0 and torch.equal(out, want[0]) and torch.equal(norms, want[1])
    up = torch.tensor(UP, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(ops.loss_anm_bwd(up, *a(c), norms, LAM), ops.loss_anm_bwd(up, *a(held), norms, LAM)))
    _check_anm(held, "anm held to range")
    m = losses.BasicANMLoss(lambda_reg=LAM)
    assert m.route == "hip" and m.check_status
    with pytest.raises(ValueError, match="3 sample"):
        _anm_call(m, c)
    m.check_status = False
    total, d = _anm_call(m, c)
    assert torch.equal(torch.stack([d["total_loss"], d["param_loss"], d["reg_loss"]]), out) and total is d["total_loss"]


@pytest.mark.parametrize("up", [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), UP], ids=["total", "first", "second", "weighted"])
def test_modules_on_the_hip_route_honour_every_output(up):
    """Gradients sent through the total and through either part, by autograd on the modules: hip against tensor route in
    float64 at the kernels' bounds; under ``no_grad`` the outputs carry no graph."""
    worst = Worst(f"modules up={up}")
    c = _dev(LC.anm_case(7, 3, 20, seed=14))
    keys = ("tau", "f", "conf", "phi")
    names = ("total_loss", "param_loss", "reg_loss")

    def run(route, dtype):
        cast = lambda t: t if t.dtype == torch.int64 else t.to(torch.complex128 if t.is_complex() else torch.float64) if dtype else t
        cc = {k: cast(v) for k, v in c.items()}
        leaves = {k: cc[k].clone().requires_grad_(True) for k in keys}
        m = losses.BasicANMLoss(lambda_reg=LAM)
        m.route = route
        _, d = _anm_call(m, cc, leaves)
        assert all(d[k].dim() == 0 for k in names)
        sum(u * d[k] for u, k in zip(up, names)).backward()
        return [d[k].detach() for k in names], [leaves[k].grad for k in keys]

    (hv, hg), (pv, pg), (wv, wg) = run("hip", None), run("tensor", None), run("tensor", torch.float64)
    worst.red(torch.stack(hv), torch.stack(wv), torch.stack(wv), "anm values")
    for g, p, w, k in zip(hg, pg, wg, keys):
        worst.elem(g, p, w, "g_" + k)
    with torch.no_grad():
        total, _ = _anm_call(losses.BasicANMLoss(), c, {k: c[k].clone().requires_grad_(True) for k in keys})
    assert not total.requires_grad

    phi, phi_true = (t.to(DEV) for t in LC.phase_pair(5, 20, seed=15))
    names = ("total_loss", "amplitude_loss", "phase_loss")

    def run_phi(route, f64):
        p, t = (_f64(phi).to(DEV), _f64(phi_true).to(DEV)) if f64 else (phi, phi_true)
        leaf = p.clone().requires_grad_(True)
        m = losses.PhiAlignmentLoss(amplitude_weight=AW, phase_weight=PW)
        m.route = route
        _, d = m(leaf, t)
        sum(u * d[k] for u, k in zip(up, names)).backward()
        return [d[k].detach() for k in names], leaf.grad

    (hv, hg), (pv, pg), (wv, wg) = run_phi("hip", False), run_phi("tensor", False), run_phi("tensor", True)
    worst.red(torch.stack(hv), torch.stack(wv), torch.stack(wv), "phi values")
    worst.elem(hg, pg, wg, "g_phi")
    worst.done()


# ------------------------------------------------------------------------------------------------ end to end
def _net(cls):
    torch.manual_seed(3)
    m = cls(M=4, N=4, num_layers=3).to(DEV)
    m.train_route = "full"
    m.eval()                                                   # the head's attention dropout off: one forward, two backwards
    y, b, sigma, truth = synth.make_batch(5, 4, 4, seed=5)
    return m, [torch.from_numpy(v).to(DEV) for v in (y, b, sigma)], truth


def _targets(B=5, Lmax=3):
    g = torch.Generator().manual_seed(7)
    return {"tau_true": torch.rand(B, Lmax, generator=g).to(DEV), "f_true": (torch.rand(B, Lmax, generator=g) - 0.5).to(DEV),
            "L_true": torch.tensor([3, 0, 1, 2, 3], device=DEV)}


def _loss_of(cls, m, inputs, route, truth):
    out = m.forward_autograd(*inputs)
    if cls is A.ADMMNet:
        crit = losses.BasicANMLoss()
        crit.route = route
        tau, f, conf, phi = out
        return crit({"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}, truth)[0], out
    crit = losses.PhiAlignmentLoss()
    crit.route = route
    return crit(out, truth)[0], out


@pytest.mark.parametrize("cls", [A.ADMMNet, A.PhiEstADMMNet], ids=["head-net-anm", "phi-net-phi"])
def test_training_step_through_the_hip_loss(cls):
    """4 x 4, K = 3, B = 5, ``train_route = "full"``: from ONE forward, a backward through the loss on ``route = "hip"`` and one on
    ``route = "tensor"`` give parameter gradients that agree within 5e-4 of each parameter's largest entry (check_grads'
    tolerance); six AdamW steps with the HIP loss lower it."""
    m, inputs, _ = _net(cls)
    truth = _targets() if cls is A.ADMMNet else LC.phase_pair(5, 16, seed=9, zeros=False)[1].to(DEV)
    out = m.forward_autograd(*inputs)
    params = [p for p in m.parameters()]
    grads = {}
    for route in ("hip", "tensor"):
        if cls is A.ADMMNet:
            crit = losses.BasicANMLoss()
            tau, f, conf, phi = out
            args = ({"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}, truth)
        else:
            crit = losses.PhiAlignmentLoss()
            args = (out, truth)
        crit.route = route
        total, _ = crit(*args)
        grads[route] = torch.autograd.grad(total, params, retain_graph=True, allow_unused=True)
    worst = 0.0
    for (name, _), gh, gt in zip(m.named_parameters(), grads["hip"], grads["tensor"]):
        assert (gh is None) == (gt is None), name
        if gh is None:
            continue
        assert torch.isfinite(gh).all(), name
        err, big = (gh - gt).abs().max().item(), gt.abs().max().item()
        if big > 0:
            worst = max(worst, err / (5e-4 * big))
        assert err <= 5e-4 * big, f"{name}: |dgrad| {err:.3e} > 5e-4 x {big:.3e}"
    print(f"{cls.__name__}: worst gradient difference / tolerance between the loss routes {worst:.2e}")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    history = []
    for _ in range(6):
        opt.zero_grad()
        loss, _ = _loss_of(cls, m, inputs, "hip", truth)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        history.append(loss.item())
    print("losses:", history)
    assert all(np.isfinite(history)) and history[-1] < history[0]
