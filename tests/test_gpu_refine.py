"""GPU: the refinement kernel (csrc/refine.hip, ``refine.refine_targets``) against its float64 host statement ``refine.refine_host``.

Every case of tests/refine_cases.py -- states, flips, symbols and absent rows exactly; where both sides converged (and the mirror
contracts with q < 1/2) tau and f within 4 tol cells -- and, independent of the iteration path, the host Gauss-Newton step at the
kernel's output; the Monte-Carlo scene of the host tests at B = 2000 in one call; the planted symbol errors; bits (twice, place,
B = 1 / 7 / 2500, the input forms of tests/presentations.py); the refusals; no host read; ``model.estimate_refined`` and
``harness.evaluate_snr(refine=)``.  Shapes: the table's (P = 4 .. 64, both axes down to length 1, Nd = 131 and 262 above a wave and
above the workgroup, the largest D = 3406 with the largest LDS).
"""
import numpy as np
import pytest
import torch

from admm_net_amd import _lib, harness, metrics, modules, refine

import presentations as P
import refine_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in RC.cases()]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(c, **kw):
    return refine.refine_targets(dev(c.y), dev(c.b), dev(c.rows), c.grid, n_est=dev(c.n_est), **{**c.kw, **kw})


def host(r):
    info = torch.stack((r.cost, r.noise_var, r.iterations.double(), r.flips.double(), r.state.double()), dim=1)
    return r.rows.cpu().numpy(), r.C.cpu().numpy(), info.cpu().numpy(), r.symbols.cpu().numpy()


def status_of(states):
    return [sum(s == k for s in states) for k in (refine.OUTSIDE, refine.NONFINITE, refine.GAVE_UP, refine.LIMIT)]


# ---- (a) the case table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_against_refine_host(name):
    c = RC.case(name)
    r = run(c)
    rows, C, info, sym = host(r)
    worst = RC.compare(name, rows, C, info, sym, "kernel")
    ref = RC.reference(name)
    print(f"{name}: worst distance / (4 tol) {worst:.3g}; iterations {info[:, 2].astype(int).tolist()} against {[q.iterations for q in ref]}")
    assert r.status.tolist() == status_of([q.state for q in ref])
    D = c.grid[0] * c.grid[1]
    fitted = np.isfinite(info[:, 0])
    assert np.array_equal(info[fitted, 1], info[fitted, 0] / D)
    assert np.allclose(rows[:, :, 2][~np.isnan(rows[:, :, 2])], np.abs(C)[~np.isnan(rows[:, :, 2])], rtol=4e-16, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_the_output_is_stationary_whatever_the_path(name):
    """The host Gauss-Newton step (undamped, on the unit-diagonal matrix) evaluated at the kernel's converged output moves no
    target by more than 2 tol cells, and Q is not above the host's Q at the start."""
    c, ref = RC.case(name), RC.reference(name)
    rows, C, info, sym = host(run(c))
    pts = refine.psk_points(*RC.PSK)
    checked = 0
    for i, q in enumerate(ref):
        here = ~np.isnan(rows[i, :, 0])
        if info[i, 4] in (refine.NONFINITE, refine.OUTSIDE) or not here.any() or not np.isfinite(info[i, 0]):
            continue
        assert info[i, 0] <= q.start_cost * (1 + 1e-12), (name, i, info[i, 0], q.start_cost)
        if info[i, 4] != refine.CONVERGED or i not in RC.comparable(name):
            continue
        y, b = c.y[i].astype(np.complex128), c.b[i].astype(np.complex128)
        x = y * np.conj(pts[sym[i]] if c.symbols == "psk" else b / np.abs(b))
        tau, f = rows[i, here, 0], rows[i, here, 1]
        Q, g, G = refine.linearise(tau, f, C[i, here], x, c.grid)
        assert np.isclose(Q, info[i, 0], rtol=1e-9), (name, i)
        A, d = refine.unit_diagonal(G)
        step = np.linalg.solve(A, d * g) * d
        L = int(here.sum())
        nt, nf = (L if c.grid[1] > 1 else 0), (L if c.grid[0] > 1 else 0)
        _, moved = refine.limit_step(step[:nt], step[nt:nt + nf], c.grid)
        print(f"{name}[{i}]: the host step at the kernel's output moves {moved:.3g} cells")
        assert moved <= 2 * RC.TOL, (name, i, moved)
        checked += 1
    assert checked or not RC.comparable(name) or all(len(q.moves) == 0 for q in ref)


# ---- (b) statistics --------------------------------------------------------------------------------------------------------------------
def test_monte_carlo_attains_the_bound_on_the_device():
    y, b, rows, bound = RC.monte_carlo()
    r = refine.refine_targets(dev(y), dev(b), dev(rows), RC.SCENE_GRID)
    ratios = RC.mc_ratios(r.rows.cpu().numpy(), bound)
    print("mean squared error over bound:", np.round(ratios, 3), "band 1 +-", round(RC.MC_BAND, 3), "iterations at most",
          int(r.iterations.max()))
    assert r.status.tolist() == [0, 0, 0, 0] and (r.state == refine.CONVERGED).all()
    assert int(r.iterations.max()) <= 16
    assert np.all(np.abs(ratios - 1.0) <= RC.MC_BAND), ratios


def test_planted_symbol_errors_are_recovered_on_the_device():
    data = [RC.planted(seed) for seed in RC.PLANTED_SEEDS]
    y, b, rows = (np.stack([d[j] for d in data]) for j in range(3))
    r = refine.refine_targets(dev(y), dev(b), dev(rows), RC.SCENE_GRID, symbols="psk")
    sym = r.symbols.cpu().numpy()
    for i, d in enumerate(data):
        want = refine.refine_host(d[0], d[1], d[2], RC.SCENE_GRID, symbols="psk")
        assert np.array_equal(sym[i], want.symbols) and np.array_equal(sym[i], d[3]), i
    assert r.flips.tolist() == [RC.PLANTED] * len(data) and (r.state == refine.CONVERGED).all()


# ---- (c) bits --------------------------------------------------------------------------------------------------------------------------
def _batch(B, symbols="given"):
    c = RC.case("L3_8x8_psk")
    pick = np.arange(B) % len(c.y)
    return dev(c.y[pick]), dev(c.b[pick]), dev(c.rows[pick]), c


@pytest.mark.parametrize("symbols", ["given", "psk"])
@pytest.mark.parametrize("B", [1, 7, 2500])
def test_bits_do_not_depend_on_the_call_the_place_or_the_batch(B, symbols):
    y, b, rows, c = _batch(B)
    first = refine.refine_targets(y, b, rows, c.grid, symbols=symbols)
    second = refine.refine_targets(y, b, rows, c.grid, symbols=symbols)
    assert all(P.same_bits(u, v) for u, v in zip(first, second))
    alone = [refine.refine_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), dev(c.rows[i:i + 1]), c.grid, symbols=symbols)
             for i in range(len(c.y))]
    for row in sorted({0, B // 2, B - 1}):
        for name in ("rows", "C", "cost", "noise_var", "iterations", "flips", "state", "symbols"):
            assert P.same_bits(getattr(first, name)[row], getattr(alone[row % len(c.y)], name)[0]), (row, name)
    assert first.status.tolist()[:3] == [0, 0, 0]                      # ("given" on these rotated symbols may use its 16 iterations up)


def test_a_scene_does_not_depend_on_its_neighbours():
    c = RC.case("L3_8x8")
    alone = [refine.refine_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), dev(c.rows[i:i + 1]), c.grid, **c.kw) for i in range(3)]
    order = [2, 0, 0, 1, 0]                                 # scenes 2, (NaN in y), (coincident rows), 1, 0
    y, b, rows = c.y[order].copy(), c.b[order].copy(), c.rows[order].copy()
    y[1, 7] = np.inf
    rows[2, 1, :2] = rows[2, 0, :2]
    r = refine.refine_targets(dev(y), dev(b), dev(rows), c.grid, **c.kw)
    assert r.state.tolist() == [0, refine.NONFINITE, refine.GAVE_UP, 0, 0] and r.status.tolist() == [0, 1, 1, 0]
    assert torch.isnan(r.rows[1]).all() and torch.isnan(r.C[2]).all() and (r.symbols[1] == -1).all()
    assert torch.equal(r.rows[2, :, :2].cpu(), torch.from_numpy(rows[2, :, :2])) and torch.isnan(r.rows[2, :, 2]).all()
    for row, scene in ((0, 2), (3, 1), (4, 0)):
        for name in ("rows", "C", "cost", "iterations", "symbols"):
            assert P.same_bits(getattr(r, name)[row], getattr(alone[scene], name)[0]), (row, scene, name)


@pytest.mark.parametrize("form", ["sliced", "permuted", "expanded", "offset", "neg_view", "lazy_conj", "wide", "leaf"])
def test_every_input_form_gives_the_plain_bits(form):
    if form in P.ABSENT:
        pytest.fail(f"torch lacks what the form {form} needs")
    c = RC.case("L3_8x8_psk")
    t = dict(y=dev(c.y), b=dev(c.b), rows=dev(c.rows), n_est=dev(np.array([3, 2, 3], dtype=np.int32)))
    if form == "expanded":
        t = {k: P.constant_along0(v) for k, v in t.items()}
    call = lambda t: refine.refine_targets(t["y"], t["b"], t["rows"], c.grid, n_est=t["n_est"], symbols="psk")  # noqa: E731
    plain = call(t)
    assert (plain.state == 0).all()
    applied = 0
    for name in t:
        v = P.present(form, t[name])
        if v is None:
            continue
        applied += 1
        got = call({**t, name: v})
        assert all(P.same_bits(g, p) for g, p in zip(got, plain)), (form, name)
        assert torch.equal(v.detach().resolve_conj().resolve_neg().to(t[name].dtype), t[name]), (form, name)
    assert applied


# ---- (d) refusals and host reads -------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_the_next_call_works():
    c = RC.case("L3_8x8")
    y, b, rows = dev(c.y), dev(c.b), dev(c.rows)
    wide = torch.zeros(3, 17, 3, dtype=torch.float64, device=DEV)
    skinny = torch.zeros(1, 3406, dtype=torch.complex64, device=DEV)
    bad = [
        (ValueError, lambda: refine.refine_targets(y, b, rows, (8, 4))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, (8,))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, (0, 64))),
        (ValueError, lambda: refine.refine_targets(y, b, wide, c.grid)),
        (ValueError, lambda: refine.refine_targets(y, b, rows[:, :, :2], c.grid)),
        (ValueError, lambda: refine.refine_targets(y[:0], b[:0], rows[:0], c.grid)),
        (ValueError, lambda: refine.refine_targets(y, b[:2], rows, c.grid)),
        (ValueError, lambda: refine.refine_targets(y.real, b, rows, c.grid)),
        (ValueError, lambda: refine.refine_targets(y, b, rows.to(torch.complex128), c.grid)),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, symbols="qam")),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, psk=(1, 0.0))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, psk=(65, 0.0))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, psk=(4, float("nan")))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, iters=0)),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, iters=65)),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, tol=0.0)),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, n_est=torch.ones(3, device=DEV))),
        (ValueError, lambda: refine.refine_targets(y, b, rows, c.grid, n_est=torch.ones(2, dtype=torch.int32, device=DEV))),
        (TypeError, lambda: refine.refine_targets(c.y, b, rows, c.grid)),
        (_lib.AdmmNetError, lambda: refine.refine_targets(y.cpu(), b, rows, c.grid)),
        (_lib.AdmmNetError, lambda: refine.refine_targets(torch.zeros(1, 59 * 59, dtype=torch.complex64, device=DEV),
                                                          torch.zeros(1, 59 * 59, dtype=torch.complex64, device=DEV), rows[:1], (59, 59))),
        (_lib.AdmmNetError, lambda: refine.refine_targets(skinny, skinny, rows[:1], (1, 3406))),          # the tables of 3 targets
    ]
    torch.cuda.synchronize()
    for err, call in bad:
        with pytest.raises(err):
            call()
    assert b"refine" in _lib.load().admmnet_last_error()
    fits = refine.refine_targets(skinny + 1, skinny + 1, rows[:1, :1], (1, 3406))                           # ... of one target fit
    assert torch.isfinite(fits.cost).all() and fits.status.tolist()[:2] == [0, 0]
    RC.compare(c.name, *host(run(c)), "after the refusals")


def test_outputs_given_as_views_are_refused_with_nothing_written():
    c = RC.case("L3_8x8")
    plain = run(c)
    rows, C = torch.full((3, 3, 3), 7.0, dtype=torch.float64, device=DEV), torch.full((3, 3), 7.0 + 0j, dtype=torch.complex128, device=DEV)
    given = run(c, out=(rows, C))
    assert given.rows is rows and given.C is C and all(P.same_bits(g, p) for g, p in zip(given, plain))
    for form in P.REFUSAL_FORMS + ("permuted",):
        for which in (0, 1):
            pair = [torch.full_like(rows, 7.0), torch.full_like(C, 7.0)]
            if form == "wide":
                view = pair[which].to(torch.float32 if which == 0 else torch.complex64)          # (no wider type: the narrower one)
            else:
                view = P.present(form, pair[which])
            if view is None:
                continue
            before = view.detach().resolve_conj().resolve_neg().clone()
            other = pair[1 - which]
            with pytest.raises(ValueError):
                run(c, out=(view, other) if which == 0 else (other, view))
            torch.cuda.synchronize()
            assert torch.equal(view.detach().resolve_conj().resolve_neg(), before) and (other == 7.0).all(), (form, which)
    with pytest.raises(ValueError):
        run(c, out=rows)
    with pytest.raises(ValueError):
        run(c, out=(rows[:2], C[:2]))
    with pytest.raises(ValueError):
        run(c, out=(rows.cpu(), C))


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    c = RC.case("n_est")
    args = (dev(c.y), dev(c.b), dev(c.rows), c.grid)
    n = dev(c.n_est)
    refine.refine_targets(*args)                          # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = refine.refine_targets(*args, n_est=n)
        q = refine.refine_targets(*args, symbols="psk", iters=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert r.iterations[0].item() == 0 and r.state.tolist() == [0] * 4 and q.iterations.max().item() <= 3


def test_the_noise_variance_feeds_the_bound():
    """INTEGRATION.md's three lines: a predicted standard deviation per estimate, close to the true-parameter bound at 20 dB."""
    y, b, rows, bound = RC.monte_carlo()
    r = refine.refine_targets(dev(y[:64]), dev(b[:64]), dev(rows[:64]), RC.SCENE_GRID)
    pred = metrics.crb(r.rows[..., 0], r.rows[..., 1], r.C, RC.SCENE_GRID, noise_var=r.noise_var)
    assert pred.status.tolist() == [0, 0, 0]
    ratio = pred.bound.cpu().numpy().mean(axis=0).T.reshape(-1) / bound                  # (tau_1..3, f_1..3)
    print("predicted over true bound:", np.round(ratio, 3))
    assert np.all(np.abs(ratio - 1.0) < 0.25)              # v is estimated from 128 - 12 real degrees of freedom; C from 20 dB


# ---- (e) through the public interface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [modules.PhiEstADMMNet, modules.ADMMNet])
def test_estimate_refined(cls):
    from admm_net_amd import synth
    torch.manual_seed(0)
    net = cls(num_layers=2, M=4, N=6, L=3).eval()
    y, b, sigma, truth = synth.make_batch_device(64, 4, 6, L=3, seed=5, snr_range=(25.0, 25.0), device=DEV)
    tau0, f0, _, counts0, phi0 = net.estimate(y, b, sigma)
    tau, f, amp, C, counts, phi, state = net.estimate_refined(y, b, sigma, symbols="psk", iters=8)
    assert tau.shape == f.shape == amp.shape == C.shape == (64, 3) and state.shape == (64,) and tau.device == y.device
    assert P.same_bits(counts, counts0) and P.same_bits(phi, phi0)
    assert torch.equal(torch.isnan(tau), torch.isnan(tau0)) and torch.equal(torch.isnan(C.real), torch.isnan(tau0))
    assert C.dtype == torch.complex128 and torch.allclose(amp[~torch.isnan(amp)], C.abs()[~torch.isnan(amp)], rtol=4e-16, atol=0)
    assert ((state >= 0) & (state <= refine.GAVE_UP)).all()
    rows = torch.stack((tau0, f0, torch.zeros_like(tau0)), dim=2)
    direct = refine.refine_targets(y, b, rows, (4, 6), symbols="psk", iters=8)
    assert P.same_bits(direct.rows[:, :, 0], tau) and P.same_bits(direct.C, C) and P.same_bits(direct.state, state)
    on_host = net.estimate_refined(y.cpu(), b.cpu(), sigma.cpu(), symbols="psk", iters=8)
    assert all(not t.is_cuda for t in on_host) and P.same_bits(on_host[0], tau.cpu())


PLAIN_KEYS = {"snr", "method", "grid", "layers", "signals", "targets", "cutoff", "pd", "false_per_signal", "rmse_tau", "rmse_f",
              "gospa", "hits", "misses", "false_alarms"}
CRB_KEYS = {"crb_tau", "crb_f", "rmse_over_crb_tau", "rmse_over_crb_f"}


def test_evaluate_snr_with_and_without_the_refinement():
    kw = dict(grid=(4, 6), layers=2, snrs=(25.0,), signals=64, targets=3, baseline="classical", device=DEV, crb=True)
    without = list(harness.evaluate_snr(**kw))
    lines = list(harness.evaluate_snr(**kw, refine="psk"))
    assert [l["method"] for l in lines] == ["net", "net+refine", "classical", "classical+refine"]
    assert [l for l in lines if not l["method"].endswith("+refine")] == without          # bit-equal: the same numbers
    for line in lines:
        print(line)
        assert set(line) == PLAIN_KEYS | CRB_KEYS
        assert line["hits"] > 0 and all(np.isfinite(line[k]) and line[k] > 0 for k in CRB_KEYS), line
    given = list(harness.evaluate_snr(**{**kw, "crb": False}, refine="given"))
    assert [l["method"] for l in given] == [l["method"] for l in lines] and set(given[1]) == PLAIN_KEYS
    with pytest.raises(ValueError):
        list(harness.evaluate_snr(**kw, refine="qam"))
