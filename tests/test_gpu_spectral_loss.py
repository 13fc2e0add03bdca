"""GPU: the kernels of csrc/loss_spectrum.hip (``ops.loss_spectrum`` / ``ops.loss_spectrum_bwd``) against the float64 tensor
formulation ``losses.TensorLossKernels.spectrum`` / ``spectrum_bwd`` on the float32 inputs the kernels read (tests/
test_spectral_loss.py holds that formulation to autograd through explicit atoms), ``losses.PhiSpectralLoss`` on ``route = "hip"``,
and one training step end to end.

Bounds (the rule of tests/test_gpu_losses.py, ``Worst`` of tests/test_gpu_training_small.py keeps the figures):
  * the gradient, elementwise: no further from float64 than 3 x the distance of the float32 tensor formulation evaluated on
    the GPU, plus 1e-6 of the largest entry;
  * the four loss values, sums over grid and batch: within 2e-5 sum|terms|.  The terms of spectral and target are non-negative
    and distribution is 1 minus a sum of non-negative terms of at most 1, so sum|terms| is taken as |value| for spectral and
    target, as 1 for distribution, and as the weighted sum of those for the total;
  * the gradient rows of all-zero phi or phi_true rows, and the terms not asked for, are exactly 0; every call run twice
    gives equal bits.
Each test prints the worst figures it saw; those measured on an MI355X are recorded in DESIGN.md section 4.
"""
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import losses, ops, spectral_ops, synth
from admm_net_amd.losses import TensorLossKernels as TLK

import loss_cases as LC
import presentations as P
import spectral_loss_cases as SC
from test_gpu_training_small import Worst, _f64, _same_twice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W = (0.6, 0.9, 0.7)                                   # spectral, distribution, target weight
UP = (1.7, 0.3, -0.6, 0.9)                            # gradients of (total, spectral, distribution, target)
GRIDS = [(1, 7), (7, 1), (5, 3), (10, 10), (16, 16)]  # xbase x ybase
SIZES = [(B, g) for B in (1, 3, 4, 5, 257) for g in GRIDS]
MODES = ("none", "mixed", "all")


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _truth(c):
    return (c["tau_true"], c["f_true"], c["L_true"])


def _truth64(c):
    return (_f64(c["tau_true"]), _f64(c["f_true"]), c["L_true"].cpu())


def _mag(want, weights=W):
    m = torch.stack([want[1].abs(), torch.ones_like(want[2]), want[3].abs()])
    return torch.stack([(torch.tensor(weights, dtype=m.dtype) * m).sum(), *m])


def _check(c, xbase, ybase, r, worst, grid=True, target=True, weights=W, skip=None):
    """c: device inputs.  Forward and backward of the kernels against float64; returns (out, g_phi, rows).  ``skip``: the
    backward's, where it is to leave out more than the forward did."""
    B = c["phi"].shape[0]
    pt, tr = (c["phi_true"] if grid else None), (_truth(c) if target else None)
    pt64, tr64 = (_f64(c["phi_true"]) if grid else None), (_truth64(c) if target else None)
    def forward():                                   # (the workspace has padding and unused stretches: its rows are compared)
        out, ws, status = ops.loss_spectrum(c["phi"], pt, tr, xbase, ybase, weights, r)
        return out, status, spectral_ops.loss_spectrum_rows(ws, xbase, ybase, r, B), ws

    out, status, rows, ws = _same_twice(lambda: forward()[:3]) + (forward()[3],)
    want, _, w_status = TLK.spectrum(_f64(c["phi"]), pt64, tr64, xbase, ybase, weights, r)
    assert out.dtype == torch.float32 and out.shape == (4,) and status.tolist() == w_status.tolist()
    worst.red(out, want, _mag(want, weights), "total, spectral, distribution, target")
    if not grid:
        assert out[1].item() == 0 and out[2].item() == 0
    if not target:
        assert out[3].item() == 0
    up = torch.tensor(UP, device=DEV)
    skip = ((0 if grid else 3) | (0 if target else 4)) if skip is None else skip
    (g,) = _same_twice(lambda: (ops.loss_spectrum_bwd(up, c["phi"], tr, xbase, ybase, weights, r, ws, skip),))
    g64 = TLK.spectrum_bwd(_f64(up), _f64(c["phi"]), tr64, xbase, ybase, weights, r, pt64, skip)
    g32 = TLK.spectrum_bwd(up, c["phi"], tr, xbase, ybase, weights, r, pt, skip)
    worst.elem(g, g32, g64, "g_phi")
    dead = ~c["phi"].any(dim=1) | (~c["phi_true"].any(dim=1) if grid else False)
    assert not g[dead].any(), "a zero phi or phi_true row gets an exactly zero gradient row"
    assert not rows[dead][:, :3].any()
    return out, g, rows.clone()


@pytest.mark.parametrize("B,grid", SIZES, ids=[f"B{B}-{g[0]}x{g[1]}" for B, g in SIZES])
def test_kernels_match_their_definition(B, grid):
    """Every oversampling with every Lmax at B <= 5 (the three L_true patterns rotating), three combinations at B = 257; a zero
    phi row and a zero phi_true row wherever B >= 3."""
    xbase, ybase = grid
    worst = Worst(f"spectrum B={B} {xbase}x{ybase}")
    combos = [(r, Lmax, MODES[(i + j) % 3]) for i, r in enumerate((1, 2, 3)) for j, Lmax in enumerate((1, 3, 16))]
    if B == 257:
        combos = [(1, 1, "all"), (2, 3, "mixed"), (3, 16, "none")]
    for r, Lmax, mode in combos:
        c = _dev(SC.case(B, xbase, ybase, Lmax, seed=B + xbase + 3 * ybase + Lmax, L=mode, zero_phi=1 if B >= 3 else None,
                         zero_true=2 if B >= 3 else None))
        _check(c, xbase, ybase, r, worst)
    worst.done()


@pytest.mark.parametrize("grid", [(5, 3), (16, 16)], ids=["5x3", "16x16"])
def test_target_only_and_grid_only_calls(grid):
    xbase, ybase = grid
    worst = Worst(f"one-sided {xbase}x{ybase}")
    c = _dev(SC.case(5, xbase, ybase, 3, seed=21, zero_phi=1, zero_true=2))
    full = _check(c, xbase, ybase, 2, worst)
    only_t = _check(c, xbase, ybase, 2, worst, grid=False, weights=(0.0, 0.0, 0.7))
    only_g = _check(c, xbase, ybase, 2, worst, target=False, weights=(0.6, 0.9, 0.0))
    assert only_g[0][1].item() == full[0][1].item() and only_g[0][2].item() == full[0][2].item()
    # (row 2 has a zero phi_true row: it counts for the target term only where no grid term is asked for)
    assert torch.equal(only_t[2][[0, 3, 4], 2], full[2][[0, 3, 4], 2]) and only_t[2][2, 2].item() > 0 and full[2][2, 2].item() == 0
    worst.done()


@pytest.mark.parametrize("grid,r", [((20, 4), 4), ((40, 4), 2), ((3, 2), 4)], ids=["20x4-r4", "40x4-r2", "3x2-r4"])
def test_the_second_delay_chunk_and_the_largest_oversampling(grid, r):
    """nx = 80 delay points: the contraction runs 64 of them, then the other 16 (the x0 > 0 path of the forward); r = 4."""
    xbase, ybase = grid
    worst = Worst(f"chunks {xbase}x{ybase} r={r}")
    for B, mode in ((1, "all"), (3, "mixed")):
        c = _dev(SC.case(B, xbase, ybase, 3, seed=91 + B + xbase, L=mode, zero_phi=1 if B == 3 else None, zero_true=2 if B == 3 else None))
        _check(c, xbase, ybase, r, worst)
    worst.done()


def test_a_zero_phi_true_row_stays_dead_when_the_backward_skips_the_grid():
    """phi_true given with a zero row, both grid weights 0, the gradient through the total only: the forward counts the row as
    dead, so the backward -- which leaves the grid terms out -- gives it a zero gradient row, on both routes."""
    worst = Worst("dead row, grid skipped")
    c = _dev(SC.case(5, 4, 4, 3, seed=95, L="all", zero_true=2))
    out, g, rows = _check(c, 4, 4, 2, worst, weights=(0.0, 0.0, 1.0), skip=3)
    assert not g[2].any() and g[[0, 1, 3, 4]].any(dim=1).all() and rows[2, 2].item() == 0

    def run(route, f64):
        cast = lambda t: t.to(torch.complex128 if t.is_complex() else torch.float64) if f64 and t.dtype != torch.int64 else t
        leaf = cast(c["phi"]).clone().requires_grad_(True)
        m = _module(4, 4, route, amplitude_weight=0.0, phase_weight=0.0, spectral_weight=0.0, distribution_weight=0.0, target_weight=1.0)
        total, d = m(leaf, cast(c["phi_true"]), {k: cast(v) for k, v in SC.truth_of(c).items()})
        total.backward()
        assert d["status"].tolist() == [0, 0, 1]
        return leaf.grad

    hg, pg, wg = run("hip", False), run("tensor", False), run("tensor", True)
    assert not hg[2].any() and not pg[2].any() and not wg[2].any()
    worst.elem(hg, pg, wg, "g_phi through the total")
    worst.done()


def test_the_backward_ignores_terms_the_forward_did_not_run():
    """A forward without phi_true leaves no z in the workspace: a backward that does not skip the grid terms gives the bits of
    the one that does; the same for a forward without truth."""
    c = _dev(SC.case(4, 5, 3, 3, seed=97, L="all"))
    up = torch.tensor(UP, device=DEV)
    _, ws, _ = ops.loss_spectrum(c["phi"], None, _truth(c), 5, 3, W, 2)
    a, b = (ops.loss_spectrum_bwd(up, c["phi"], _truth(c), 5, 3, W, 2, ws, skip) for skip in (0, 3))
    assert torch.equal(a, b) and torch.isfinite(a).all() and a.any()
    _, ws, _ = ops.loss_spectrum(c["phi"], c["phi_true"], None, 5, 3, W, 2)
    a, b = (ops.loss_spectrum_bwd(up, c["phi"], tr, 5, 3, W, 2, ws, skip) for tr, skip in ((_truth(c), 0), (None, 4)))
    assert torch.equal(a, b) and torch.isfinite(a).all() and a.any()


def test_a_signal_has_the_same_bits_at_any_batch_size_and_place():
    """The per-signal rows (terms, scalars, z at the targets) of one signal alone, last of 7 and of 257, and beside zero-row
    neighbours; its gradient row beside other neighbours at one batch size."""
    xbase, ybase, r, Lmax = 10, 10, 2, 3
    c = SC.case(257, xbase, ybase, Lmax, seed=31, L="all")
    pick = lambda idx: _dev({k: v[idx] for k, v in c.items()})
    call = lambda d: ops.loss_spectrum(d["phi"], d["phi_true"], _truth(d), xbase, ybase, W, r)
    rows = lambda d: spectral_ops.loss_spectrum_rows(call(d)[1], xbase, ybase, r, d["phi"].shape[0])
    alone = rows(pick([5]))[0]
    assert alone[:3].all() and alone[16:16 + 2 * Lmax].all()
    assert torch.equal(rows(pick([0, 1, 2, 3, 4, 6, 5]))[6], alone) and torch.equal(rows(pick(list(range(5)) + list(range(6, 257)) + [5]))[256], alone)
    seven = pick([0, 1, 2, 5, 3, 4, 6])
    other = {k: v.clone() for k, v in seven.items()}
    other["phi"][2] = 0
    other["phi_true"][4] = 0
    assert torch.equal(rows(other)[3], alone)
    up = torch.tensor(UP, device=DEV)
    bwd = lambda d: ops.loss_spectrum_bwd(up, d["phi"], _truth(d), xbase, ybase, W, r, call(d)[1])
    ga, gb = bwd(seven), bwd(other)
    assert torch.equal(ga[3], gb[3]) and gb[3].any() and not gb[2].any() and not gb[4].any()
    assert torch.equal(bwd(pick([6, 4, 3, 5, 2, 1, 0]))[3], ga[3])


def _offset(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _strided(t):
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=DEV)
    v = wide[..., ::2]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def _lazy_conj(t):
    return t.conj().resolve_conj().conj() if t.is_complex() else t.double()      # the conj bit set / a wider dtype


@pytest.mark.parametrize("view", [_offset, _strided, _lazy_conj], ids=["offset", "strided", "lazy-conj-and-wide"])
def test_kernels_on_views(view):
    c = _dev(SC.case(5, 5, 3, 3, seed=41, zero_phi=1))
    plain = _check(c, 5, 3, 2, Worst("plain"))
    seen = _check({k: (v if k == "L_true" and view is _lazy_conj else view(v)) for k, v in c.items()}, 5, 3, 2, Worst(view.__name__))
    assert all(torch.equal(a, b) for a, b in zip(plain, seen))


@pytest.mark.parametrize("form", [f for f in P.FORMS if f not in P.ABSENT])
def test_every_input_form_gives_the_plain_tensor_bits(form):
    """The forms of tests/presentations.py (the table of tests/test_gpu_presentations.py holds the functions defined in ops.py
    to them): each tensor input of ``ops.loss_spectrum`` and ``ops.loss_spectrum_bwd`` in turn, the others plain."""
    c = _dev(SC.case(4, 5, 3, 3, seed=43, L="all"))
    if form == "expanded":
        c = {k: P.constant_along0(v) for k, v in c.items()}
    up = torch.tensor(UP, device=DEV)

    def run(d, g_out):
        out, ws, status = ops.loss_spectrum(d["phi"], d["phi_true"], _truth(d), 5, 3, W, 2)
        return out, status, ops.loss_spectrum_bwd(g_out, d["phi"], _truth(d), 5, 3, W, 2, ws)

    plain, seen = run(c, up), 0
    for k in list(c) + ["g_out"]:
        v = P.present(form, up if k == "g_out" else c[k])
        if v is None:
            continue
        got = run(c, v) if k == "g_out" else run(dict(c, **{k: v}), up)
        assert all(torch.equal(a, b) for a, b in zip(plain, got)), (form, k)
        seen += 1
    assert seen >= 1 and plain[2].any()


def _module(xbase, ybase, route, r=2, **kw):
    m = losses.PhiSpectralLoss(xbase, ybase, oversample=r, **{**dict(amplitude_weight=0.8, phase_weight=0.45, spectral_weight=W[0],
                                                                   distribution_weight=W[1], target_weight=W[2]), **kw})
    m.route = route
    return m


NAMES = ("total_loss", "spectral_loss", "distribution_loss", "target_loss")


@pytest.mark.parametrize("up", [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), UP],
                         ids=["total", "spectral", "distribution", "target", "weighted"])
def test_the_module_on_the_hip_route_honours_every_output(up):
    """Gradients sent through the total and through each part by autograd on the module: hip against the tensor route in
    float64 at the kernels' bounds (the label weights are 0 here: PhiAlignmentLoss's terms have their own test)."""
    worst = Worst(f"module up={up}")
    c = _dev(SC.case(7, 10, 10, 3, seed=51, zero_phi=3))
    truth = SC.truth_of(c)

    def run(route, f64):
        phi, pt = (c["phi"].to(torch.complex128), c["phi_true"].to(torch.complex128)) if f64 else (c["phi"], c["phi_true"])
        tr = {k: (v.double() if f64 and v.is_floating_point() else v) for k, v in truth.items()}
        leaf = phi.clone().requires_grad_(True)
        _, d = _module(10, 10, route, amplitude_weight=0.0, phase_weight=0.0)(leaf, pt, tr)
        sum(u * d[k] for u, k in zip(up, NAMES) if u != 0.0).backward()
        return torch.stack([d[k].detach() for k in NAMES]), leaf.grad

    (hv, hg), (pv, pg), (wv, wg) = run("hip", False), run("tensor", False), run("tensor", True)
    worst.red(hv, wv, _mag(wv.cpu()), "values")
    worst.elem(hg, pg, wg, "g_phi")
    worst.done()


def test_no_synchronising_call_with_check_status_off():
    c = _dev(SC.case(5, 10, 10, 3, seed=61))
    m = _module(10, 10, "hip")
    m.check_status = False
    leaf = c["phi"].clone().requires_grad_(True)
    m(leaf, c["phi_true"], SC.truth_of(c))[0].backward()                      # (the library is loaded, the first calls made)
    leaf.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, d = m(leaf, c["phi_true"], SC.truth_of(c))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(leaf.grad).all() and d["status"].tolist() == [0, 0, 0]
    bad = dict(SC.truth_of(c), L_true=torch.tensor([0, 4, 1, -1, 2], device=DEV))
    assert m(leaf, c["phi_true"], bad)[1]["status"].tolist() == [2, 0, 0]
    m.check_status = True
    with pytest.raises(ValueError, match="2 sample"):
        m(leaf, c["phi_true"], bad)


def test_invariance_and_the_single_atom_on_the_device():
    worst = Worst("invariance")
    c = _dev(SC.case(4, 5, 3, 3, seed=71))
    truth = _truth(c)
    out0, ws0, _ = ops.loss_spectrum(c["phi"], c["phi_true"], truth, 5, 3, W, 2)
    scaled = (0.25 * torch.exp(torch.tensor(1.1j))).to(DEV) * c["phi"]
    out1, _, _ = ops.loss_spectrum(scaled, c["phi_true"], truth, 5, 3, W, 2)
    worst.red(out1, _f64(out0), _mag(_f64(out0)), "c e^{j theta} phi")
    same = (0.3 * torch.exp(torch.tensor(1.1j))).to(DEV) * c["phi_true"]
    out2, ws2, _ = ops.loss_spectrum(same, c["phi_true"], truth, 5, 3, W, 2)
    # phi is 0.3 e^{1.1j} phi_true ROUNDED to float32: a relative deviation d <= 1e-7 per entry.  spectral is quadratic in it
    # (<= 1e-10 with a factor 1e4 to spare), distribution is 1 minus a float64 ratio (a few 1e-16 of rounding + d^2)
    assert abs(out2[1].item()) <= 1e-10 and abs(out2[2].item()) <= 1e-10
    only = torch.tensor([0.0, 1.0, 1.0, 0.0], device=DEV)
    g_same = ops.loss_spectrum_bwd(only, same, truth, 5, 3, W, 2, ws2)
    g_rnd = ops.loss_spectrum_bwd(only, c["phi"], truth, 5, 3, W, 2, ws0)
    print(f"  gradient at phi ~ phi_true / at a random phi: {g_same.abs().max().item() / g_rnd.abs().max().item():.3e}")
    assert g_same.abs().max().item() <= 1e-5 * g_rnd.abs().max().item()          # linear in d <= 1e-7, a factor 100 to spare
    phi, tr = SC.single_atom()
    tr = tuple(tr[k].to(DEV) for k in ("tau_true", "f_true", "L_true"))
    phi = phi.to(torch.complex64).to(DEV)
    out, _, _ = ops.loss_spectrum(phi, None, tr, 5, 3, (0.0, 0.0, 1.0), 2)
    swapped, _, _ = ops.loss_spectrum(phi, None, tr, 3, 5, (0.0, 0.0, 1.0), 2)
    print(f"  single atom: target {out[3].item():.3e}, rho with the axes exchanged {1 - swapped[3].item():.4f}")
    assert abs(out[3].item()) <= 1e-6 and abs((1 - swapped[3].item()) - 0.255) <= 5e-4
    worst.done()


def test_refusals_before_a_launch():
    c = _dev(SC.case(3, 5, 3, 3, seed=81))
    with pytest.raises(ValueError):
        ops.loss_spectrum(c["phi"], None, None, 5, 3, W, 2)
    with pytest.raises(ValueError):
        ops.loss_spectrum(c["phi"], c["phi_true"], _truth(c), 5, 4, W, 2)
    with pytest.raises(ValueError):
        ops.loss_spectrum(c["phi"], c["phi_true"], _truth(c), 5, 3, W, 5)
    with pytest.raises(ValueError):
        ops.loss_spectrum(c["phi"], c["phi_true"], (torch.zeros(3, 17, device=DEV), torch.zeros(3, 17, device=DEV), c["L_true"]), 5, 3, W, 2)
    big = torch.zeros(1, 64 * 64, dtype=torch.complex64, device=DEV)
    with pytest.raises(A._lib.AdmmNetError):
        ops.loss_spectrum(big, big, None, 64, 64, W, 4)
    _, ws, _ = ops.loss_spectrum(c["phi"], c["phi_true"], _truth(c), 5, 3, W, 2)
    with pytest.raises(ValueError, match="workspace"):
        ops.loss_spectrum_bwd(torch.ones(4, device=DEV), c["phi"], _truth(c), 5, 3, W, 2, ws[:-256])


# ------------------------------------------------------------------------------------------------ end to end
def test_training_step_through_the_hip_spectral_loss():
    """4 x 4, K = 3, B = 5, ``train_route = "full"``: from ONE forward, a backward through the loss on ``route = "hip"`` and one on
    ``route = "tensor"`` give parameter gradients that agree within 5e-4 of each parameter's largest entry; six AdamW steps with
    the HIP loss lower the total."""
    torch.manual_seed(3)
    m = A.PhiEstADMMNet(M=4, N=4, num_layers=3).to(DEV)
    m.train_route = "full"
    m.eval()
    y, b, sigma, _ = synth.make_batch(5, 4, 4, seed=5)
    inputs = [torch.from_numpy(v).to(DEV) for v in (y, b, sigma)]
    g = torch.Generator().manual_seed(7)
    truth = {"tau_true": torch.rand(5, 3, generator=g).to(DEV), "f_true": (torch.rand(5, 3, generator=g) - 0.5).to(DEV),
             "L_true": torch.tensor([3, 0, 1, 2, 3], device=DEV)}
    phi_true = LC.phase_pair(5, 16, seed=9, zeros=False)[1].to(DEV)
    crit = lambda route: _module(4, 4, route, amplitude_weight=1.0, phase_weight=0.5, spectral_weight=0.2, distribution_weight=0.3,
                                 target_weight=0.5)
    out = m.forward_autograd(*inputs)
    params = list(m.parameters())
    grads = {route: torch.autograd.grad(crit(route)(out, phi_true, truth)[0], params, retain_graph=True, allow_unused=True)
             for route in ("hip", "tensor")}
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
    print(f"worst gradient difference / tolerance between the loss routes {worst:.2e}")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    history = []
    for _ in range(6):
        opt.zero_grad()
        loss, _ = crit("hip")(m.forward_autograd(*inputs), phi_true, truth)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        history.append(loss.item())
    print("losses:", history)
    assert all(h == h for h in history) and history[-1] < history[0]
