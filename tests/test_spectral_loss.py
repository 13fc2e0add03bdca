"""CPU: the spectrum terms of ``losses.PhiSpectralLoss`` -- the float64 tensor formulation (``TensorLossKernels.spectrum`` /
``spectrum_bwd``, the stand-in for csrc/loss_spectrum.hip and the GPU tests' yardstick) against autograd through the per-sample
evaluation of tests/spectral_loss_cases.py, which builds explicit atom matrices and uses no separable product.

Bound: 1e-12 of the largest entry, the float64 bound of tests/test_losses.py.  The one-mistake stand-ins of
``spectral_loss_cases.explicit`` are each rejected, at that bound, by a named case.
"""
import os

import pytest
import torch

from admm_net_amd import _lib, losses, ops
from admm_net_amd.losses import TensorLossKernels as TLK

import spectral_loss_cases as SC

F64 = 1e-12
NAMES = ("total_loss", "spectral_loss", "distribution_loss", "target_loss")
WEIGHTS = dict(amplitude_weight=0.0, phase_weight=0.0, spectral_weight=0.6, distribution_weight=0.9, target_weight=0.7)
UPS = [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.7, 0.3, -0.6, 0.9)]
UP_IDS = ["total", "spectral", "distribution", "target", "weighted"]
# (B, xbase, ybase, r, Lmax, L, zero phi row, zero phi_true row)
CASES = {"5x3-r2": (4, 5, 3, 2, 3, "mixed", None, None), "1x7-r3": (3, 1, 7, 3, 1, "all", None, None),
         "7x1-r1": (2, 7, 1, 1, 16, "mixed", None, None), "4x4-r2-zero-rows": (5, 4, 4, 2, 3, "mixed", 1, 2),
         "3x2-r4-no-targets": (3, 3, 2, 4, 2, "none", None, None)}


def _f64(c):
    return {k: (v if k == "L_true" else v.to(torch.complex128 if v.is_complex() else torch.float64)) for k, v in c.items()}


def _module(xbase, ybase, r, route="tensor", **kw):
    m = losses.PhiSpectralLoss(xbase, ybase, oversample=r, **{**WEIGHTS, **kw})
    m.route = route
    return m


def _case(name):
    B, xbase, ybase, r, Lmax, L, zp, zt = CASES[name]
    return _f64(SC.case(B, xbase, ybase, Lmax, seed=B + xbase + ybase, L=L, zero_phi=zp, zero_true=zt)), xbase, ybase, r


def _want(leaf, c, xbase, ybase, r, mistake=None, with_true=True, with_truth=True):
    spec, dist, targ = SC.explicit(leaf, c["phi_true"] if with_true else None, SC.truth_of(c) if with_truth else None, xbase,
                                   ybase, r, mistake)
    return (WEIGHTS["spectral_weight"] * spec + WEIGHTS["distribution_weight"] * dist + WEIGHTS["target_weight"] * targ, spec,
            dist, targ)


def _grad(values, up, leaf):
    (g,) = torch.autograd.grad(sum(u * v for u, v in zip(up, values)), leaf, allow_unused=True, retain_graph=True)
    return torch.zeros_like(leaf) if g is None else g


def _agree(got, want, g_got, g_want, scale=None):
    """Values within 1e-12 of the largest of them, gradients within 1e-12 of their largest entry."""
    big = max(max(abs(w.item()) for w in want), 1e-300)
    ok = all(abs(g.item() - w.item()) <= F64 * big for g, w in zip(got, want))
    return ok and (g_got - g_want).abs().max().item() <= F64 * max(g_want.abs().max().item() if scale is None else scale, 1e-300)


@pytest.mark.parametrize("up", UPS, ids=UP_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_float64_matches_autograd_through_explicit_atoms(name, up):
    c, xbase, ybase, r = _case(name)
    a, b = c["phi"].clone().requires_grad_(True), c["phi"].clone().requires_grad_(True)
    total, d = _module(xbase, ybase, r)(a, c["phi_true"], SC.truth_of(c))
    got = [d[k] for k in NAMES]
    assert total is d["total_loss"] and all(g.dtype == torch.float64 and g.dim() == 0 for g in got)
    want = _want(b, c, xbase, ybase, r)
    g_got, g_want = _grad(got, up, a), _grad(want, up, b)
    assert _agree(got, want, g_got, g_want), ([g.item() for g in got], [w.item() for w in want],
                                               (g_got - g_want).abs().max().item())
    B, _, _, _, _, _, zp, zt = CASES[name]
    for row in (zp, zt):
        if row is not None:
            assert not g_got[row].any(), "a zero phi or phi_true row gets a zero gradient row"
    assert d["status"].tolist() == [0, int(zp is not None), int(zt is not None)]


@pytest.mark.parametrize("name", ["5x3-r2", "7x1-r1"])
def test_target_only_and_grid_only_calls(name):
    c, xbase, ybase, r = _case(name)
    for with_true, with_truth in ((False, True), (True, False)):
        a, b = c["phi"].clone().requires_grad_(True), c["phi"].clone().requires_grad_(True)
        kw = dict(spectral_weight=0.0, distribution_weight=0.0) if not with_true else dict(target_weight=0.0)
        _, d = _module(xbase, ybase, r, **kw)(a, c["phi_true"] if with_true else None, SC.truth_of(c) if with_truth else None)
        want = list(_want(b, c, xbase, ybase, r, with_true=with_true, with_truth=with_truth))
        want[0] = 0.7 * want[3] if not with_true else 0.6 * want[1] + 0.9 * want[2]
        got = [d[k] for k in NAMES]
        assert _agree(got, want, _grad(got, UPS[4], a), _grad(want, UPS[4], b))
        assert (d["target_loss"].item() == 0) == with_true and (d["spectral_loss"].item() == 0) == (not with_true)


@pytest.mark.parametrize("up", [UPS[0], UPS[4]], ids=["total", "weighted"])
def test_a_zero_phi_true_row_stays_dead_when_the_backward_skips_the_grid(up):
    """phi_true given with row 2 zero, both grid weights 0, target_weight 1: the forward counts the row as dead (status
    [0, 0, 1]); a gradient through the total alone lets the backward leave the grid terms out, and the row's gradient is
    still exactly 0 and the whole gradient that of the written-out definition."""
    c = _f64(SC.case(4, 4, 4, 3, seed=12, L="all", zero_true=2))
    a, b = c["phi"].clone().requires_grad_(True), c["phi"].clone().requires_grad_(True)
    _, d = _module(4, 4, 2, spectral_weight=0.0, distribution_weight=0.0, target_weight=1.0)(a, c["phi_true"], SC.truth_of(c))
    assert d["status"].tolist() == [0, 0, 1]
    got = [d[k] for k in NAMES]
    want = list(SC.explicit(b, c["phi_true"], SC.truth_of(c), 4, 4, 2))
    want = [want[2]] + want
    g_got, g_want = _grad(got, up, a), _grad(want, up, b)
    assert _agree(got, want, g_got, g_want)
    assert not g_got[2].any() and g_got[[0, 1, 3]].any(dim=1).all()
    eps = 1e-6                                                       # and the total does not move with phi[2, 0]
    moved = c["phi"].clone()
    moved[2, 0] += eps
    assert _module(4, 4, 2, spectral_weight=0.0, distribution_weight=0.0, target_weight=1.0)(moved, c["phi_true"], SC.truth_of(c))[0].item() \
        == d["total_loss"].item()


@pytest.mark.parametrize("r", [1, 2, 3])
def test_parseval_on_the_uniform_grid(r):
    """mean_grid S = ||phi||^2 for every oversampling: the grid covers one full period on both axes."""
    phi = SC.case(3, 5, 3, 1, seed=r)["phi"].to(torch.complex128)
    Sm, Dm = TLK.spectrum_tables(5, 3, r, phi.device, phi.dtype)
    z = torch.einsum("bsd,qs,pd->bqp", phi.reshape(3, 3, 5).conj(), Sm, Dm)
    assert z.shape == (3, 3 * r, 5 * r)
    n2 = (phi.abs() ** 2).sum(dim=1)
    assert ((z.abs() ** 2).mean(dim=(1, 2)) - n2).abs().max().item() <= 1e-13 * n2.max().item()
    A = SC.atoms(*SC.grid_points(5, 3, r), 5, 3)
    assert (z.reshape(3, -1) - phi.conj() @ A).abs().max().item() <= 1e-12          # the tables are the explicit atoms


def test_scale_and_phase_of_phi_do_not_matter():
    """phi = 0.3 e^{1.1j} phi_true: spectral and distribution and their gradients vanish; every term is unchanged by the factor."""
    c, xbase, ybase, r = _case("5x3-r2")
    m = _module(xbase, ybase, r)
    rnd = c["phi"].clone().requires_grad_(True)
    _, d0 = m(rnd, c["phi_true"], SC.truth_of(c))
    g_rnd = [_grad([d0[k]], (1.0,), rnd).abs().max().item() for k in ("spectral_loss", "distribution_loss")]
    same = (0.3 * torch.exp(torch.tensor(1.1j, dtype=torch.complex128)) * c["phi_true"]).requires_grad_(True)
    _, d = m(same, c["phi_true"], SC.truth_of(c))
    for k, big in zip(("spectral_loss", "distribution_loss"), g_rnd):
        assert abs(d[k].item()) <= 1e-12, (k, d[k].item())
        assert _grad([d[k]], (1.0,), same).abs().max().item() <= 1e-12 * big, k
    _, d1 = m((0.3 * torch.exp(torch.tensor(1.1j, dtype=torch.complex128)) * c["phi"]), c["phi_true"], SC.truth_of(c))
    for k in NAMES[1:]:
        assert abs(d1[k].item() - d0[k].item()) <= 1e-12 * max(abs(d0[k].item()), 1.0), k


def test_single_atom_names_its_target_and_rejects_an_axis_swap():
    """a(0.37, -0.21) on 5 x 3: rho = 1, target 0.  Read with x and y exchanged the same vector gives rho = 0.255."""
    phi, truth = SC.single_atom()
    _, d = _module(5, 3, 2, spectral_weight=0.0, distribution_weight=0.0)(phi, None, truth)
    assert abs(d["target_loss"].item()) <= 1e-12
    _, s = _module(3, 5, 2, spectral_weight=0.0, distribution_weight=0.0)(phi, None, truth)
    assert abs((1 - s["target_loss"].item()) - 0.255) <= 5e-4, 1 - s["target_loss"].item()


# ------------------------------------------------------------------------------------------------ one-mistake stand-ins
STAND_INS = {"the sign of tau in the atom": ("tau_sign", "5x3-r2"), "axes exchanged": ("axes", "5x3-r2"),
             "normalising by the maximum": ("max", "5x3-r2"), "L = 0 rows divided by 0": ("L0", "5x3-r2"),
             "the factor 2": ("factor2", "5x3-r2")}


@pytest.mark.parametrize("name", list(STAND_INS))
def test_a_one_mistake_stand_in_is_rejected(name):
    """The comparison of ``test_float64_matches_autograd_through_explicit_atoms`` fails for each stand-in on its named case (and
    passes for the definition itself on the same case, with the same code)."""
    mistake, case_name = STAND_INS[name]
    c, xbase, ybase, r = _case(case_name)
    a = c["phi"].clone().requires_grad_(True)
    _, d = _module(xbase, ybase, r)(a, c["phi_true"], SC.truth_of(c))
    got = [d[k] for k in NAMES]
    g_got = _grad(got, UPS[4], a)

    def verdict(mistake):
        b = c["phi"].clone().requires_grad_(True)
        want = _want(b, c, xbase, ybase, r, None if mistake == "factor2" else mistake)
        g_want = _grad(want, UPS[4], b)
        if mistake == "factor2":
            g_want = g_want / 2
        finite = all(torch.isfinite(w) for w in want) and torch.isfinite(g_want).all()
        return finite and _agree(got, want, g_got, g_want)

    assert verdict(None) and not verdict(mistake)


# ------------------------------------------------------------------------------------------------ the module's surface
def test_status_counts_and_the_range_check():
    c = _f64(SC.case(7, 4, 4, 3, seed=5, L=[0, 4, 2, -1, 3, 1 << 40, 1], zero_phi=2, zero_true=6))
    m = _module(4, 4, 2)
    assert m.check_status and losses.PhiSpectralLoss(4, 4).route == "hip"
    with pytest.raises(ValueError, match="3 sample"):
        m(c["phi"], c["phi_true"], SC.truth_of(c))
    m.check_status = False
    total, d = m(c["phi"], c["phi_true"], SC.truth_of(c))
    assert d["status"].tolist() == [3, 1, 1] and d["status"].dtype == torch.int32
    held = dict(c, L_true=c["L_true"].clamp(0, 3))
    assert torch.equal(total, _module(4, 4, 2)(c["phi"], c["phi_true"], SC.truth_of(held))[0])


def test_weight_and_argument_rules():
    c, xbase, ybase, r = _case("5x3-r2")
    truth = SC.truth_of(c)
    with pytest.raises(ValueError, match="without phi_true"):
        _module(xbase, ybase, r)(c["phi"], None, truth)                              # label weights not 0
    with pytest.raises(ValueError, match="without phi_true"):
        _module(xbase, ybase, r, spectral_weight=0.0, distribution_weight=0.0, target_weight=0.0)(c["phi"])
    with pytest.raises(ValueError, match="target_weight"):
        _module(xbase, ybase, r)(c["phi"], c["phi_true"])
    with pytest.raises(ValueError, match="rows of 15"):
        _module(xbase, ybase, r)(c["phi"][:, :14], c["phi_true"][:, :14], truth)
    with pytest.raises(ValueError, match="one shape"):
        _module(xbase, ybase, r)(c["phi"], c["phi_true"][:2], truth)
    with pytest.raises(ValueError, match="Lmax <= 16"):
        _module(xbase, ybase, r)(c["phi"], c["phi_true"], dict(truth, tau_true=torch.zeros(4, 17), f_true=torch.zeros(4, 17)))
    for k in ("tau_true", "f_true"):
        with pytest.raises(ValueError, match="requires grad"):
            _module(xbase, ybase, r)(c["phi"], c["phi_true"], dict(truth, **{k: truth[k].clone().requires_grad_(True)}))
    with pytest.raises(ValueError, match="requires grad"):
        _module(xbase, ybase, r)(c["phi"], c["phi_true"].clone().requires_grad_(True), truth)
    for bad in (0, 5, 2.5):
        with pytest.raises(ValueError, match="oversample"):
            losses.PhiSpectralLoss(5, 3, oversample=bad)
    with pytest.raises(ValueError, match="route"):
        _module(xbase, ybase, r, route="eager")(c["phi"], c["phi_true"], truth)
    with pytest.raises(_lib.AdmmNetError):                                           # no CPU fallback on the HIP route
        _module(xbase, ybase, r, route="hip")(c["phi"].to(torch.complex64), c["phi_true"].to(torch.complex64), truth)
    d = losses.PhiSpectralLoss(5, 3)
    assert (d.amplitude_weight, d.phase_weight, d.spectral_weight, d.distribution_weight, d.target_weight, d.oversample) == \
        (1.0, 0.5, 0.2, 0.3, 0.0, 2)


def test_the_alignment_entries_are_carried_through_unchanged():
    """With the default weights the total is PhiAlignmentLoss's total plus the weighted spectrum terms, the amplitude and
    phase entries and their gradients are that module's own; float32 inputs give float32 outputs."""
    c = SC.case(4, 5, 3, 3, seed=8)
    a, b = c["phi"].clone().requires_grad_(True), c["phi"].clone().requires_grad_(True)
    m = losses.PhiSpectralLoss(5, 3)
    pa = losses.PhiAlignmentLoss()
    m.route = pa.route = "tensor"
    total, d = m(a.reshape(2, 2, 15), c["phi_true"].reshape(2, 2, 15))
    want, w = pa(b, c["phi_true"])
    assert total.dtype == torch.float32 and torch.equal(d["amplitude_loss"], w["amplitude_loss"])
    assert torch.equal(d["phase_loss"], w["phase_loss"])
    assert torch.equal(total, want + (0.2 * d["spectral_loss"] + 0.3 * d["distribution_loss"] + 0.0 * d["target_loss"]))
    (d["amplitude_loss"] + 2 * d["phase_loss"]).backward()
    (w["amplitude_loss"] + 2 * w["phase_loss"]).backward()
    assert torch.equal(a.grad, b.grad)
    with torch.no_grad():
        assert not m(a, c["phi_true"])[0].requires_grad


def test_entry_points_and_the_drop_in_export():
    assert callable(ops.loss_spectrum) and callable(ops.loss_spectrum_bwd)
    for name in ("admmnet_loss_spectrum_workspace_bytes", "admmnet_loss_spectrum_f64", "admmnet_loss_spectrum_bwd_f64"):
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.admmnet_loss_spectrum_workspace_bytes(10, 10, 2, 256) > 0
    for bad in ((0, 10, 2, 1), (10, 10, 0, 1), (10, 10, 5, 1), (10, 10, 2, 0), (64, 64, 4, 1)):      # the last: beyond the LDS
        assert lib.admmnet_loss_spectrum_workspace_bytes(*bad) == -1, bad
    import importlib.util
    path = os.path.join(os.path.dirname(losses.__file__), "dropin", "optional", "loss.py")
    spec = importlib.util.spec_from_file_location("_dropin_loss_probe", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.PhiSpectralLoss is losses.PhiSpectralLoss and mod.PhiAlignmentLoss is losses.PhiAlignmentLoss
