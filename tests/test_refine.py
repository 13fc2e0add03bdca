"""Host: the float64 statement of the refinement (``refine.refine_host``), the kernel's scalar core under sanitizers
(tests/host_model/refine_model.cpp) and the refusals and signatures of the new entry points.  No GPU.

The mirror is what tests/test_gpu_refine.py holds the kernel to, so it is itself held to things that do not depend on it: the
Cramer-Rao bound over 2000 noise draws, central differences of Q, planted symbol errors, and stand-ins with one defect each.
"""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from admm_net_amd import harness, metrics, modules, refine

import refine_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "admm_net_amd", "csrc")
HOST = os.path.join(HERE, "host_model")


# ---- 1. the mirror attains the bound -------------------------------------------------------------------------------------------------
def test_the_mirror_attains_the_bound():
    """The issue's 8 x 8 scene, known symbols, 20 dB, 2000 draws, start = truth +- 0.3 cell: the mean squared error over the bound
    of each of the six parameters lies in 1 +- 4.5 sqrt(2 / 2000), and every draw converges within 16 iterations."""
    y, b, rows, bound = RC.monte_carlo()
    fits = [refine.refine_host(y[i], b[i], rows[i], RC.SCENE_GRID) for i in range(len(y))]
    ratios = RC.mc_ratios(np.stack([r.rows for r in fits]), bound)
    most = max(r.iterations for r in fits)
    print("mean squared error over bound:", np.round(ratios, 3), "band 1 +-", round(RC.MC_BAND, 3), "iterations at most", most)
    assert all(r.state == refine.CONVERGED and r.flips == 0 for r in fits) and most <= 16
    assert np.all(np.abs(ratios - 1.0) <= RC.MC_BAND), ratios


def test_the_scene_has_the_decision_margin_of_the_issue():
    mu = metrics.crb_signal(*RC.SCENE, RC.SCENE_GRID)
    assert round(float(np.abs(mu).min() / np.sqrt((np.abs(mu) ** 2).mean())), 3) == 0.155


# ---- 2. the gradient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(8, 8), (4, 6), (1, 12), (12, 1)])
def test_gradient_and_G_against_central_differences(grid):
    """g = Re(J^H r) is -1/2 dQ/dtheta; G = Re(J^H J) is the Gauss-Newton part of 1/2 d2Q/dtheta2 -- exactly so where r = 0."""
    rng = np.random.default_rng(7)
    tau, f = rng.uniform(0.2, 0.8, 2), rng.uniform(-0.3, 0.3, 2)
    C = rng.normal(size=2) + 1j * rng.normal(size=2)
    D = grid[0] * grid[1]
    mu, _ = refine.signal_model(tau, f, C, grid)
    nt, nf = (2 if grid[1] > 1 else 0), (2 if grid[0] > 1 else 0)

    def unpack(theta):
        return (theta[:nt] if nt else tau, theta[nt:nt + nf] if nf else f, theta[nt + nf:nt + nf + 2] + 1j * theta[nt + nf + 2:])

    theta = np.concatenate([tau[:nt], f[:nf], C.real, C.imag])
    for x in (mu + 0.3 * (rng.normal(size=D) + 1j * rng.normal(size=D)), mu):
        Q = lambda th: refine.linearise(*unpack(th), x, grid)[0]  # noqa: E731
        _, g, G = refine.linearise(tau, f, C, x, grid)
        h = 1e-6
        num = np.array([(Q(theta + h * e) - Q(theta - h * e)) / (2 * h) for e in np.eye(len(theta))])
        assert np.allclose(-0.5 * num, g, rtol=1e-6, atol=1e-6 * np.abs(g).max() + 1e-7), grid
        if x is mu:                                          # r = 0: the Hessian of Q / 2 is G
            grad = lambda th: -refine.linearise(*unpack(th), x, grid)[1]  # noqa: E731
            hess = np.array([(grad(theta + h * e) - grad(theta - h * e)) / (2 * h) for e in np.eye(len(theta))])
            assert np.allclose(hess, G, rtol=1e-6, atol=1e-6 * np.abs(G).max()), grid


# ---- 3. planted symbol errors ---------------------------------------------------------------------------------------------------------
def test_the_mirror_recovers_planted_symbol_errors():
    """40 dB, 5 of 64 symbols of b rotated, start = truth +- 0.1 cell: "psk" ends with exactly the planted entries flipped on every
    seed; "given" on the same data ends more than 3 root bounds away in some parameter -- on all 12 draws of the list."""
    tau, f, C = RC.SCENE
    far = 0
    for seed in RC.PLANTED_SEEDS:
        y, b, rows, sent, at, v = RC.planted(seed)
        r = refine.refine_host(y, b, rows, RC.SCENE_GRID, symbols="psk")
        assert r.state == refine.CONVERGED and r.flips == RC.PLANTED and np.array_equal(r.symbols, sent), seed
        assert np.array_equal(np.flatnonzero(r.symbols != refine.nearest_point(b, refine.psk_points(*RC.PSK))), at), seed
        root = np.sqrt(metrics.crb_host(tau, f, C, RC.SCENE_GRID, noise_var=v).bound)
        err = lambda q: float(np.maximum(np.abs(q.rows[:, 0] - tau) / root[:, 0], np.abs(q.rows[:, 1] - f) / root[:, 1]).max())  # noqa: E731
        assert err(r) < 4.5, (seed, err(r))
        g = refine.refine_host(y, b, rows, RC.SCENE_GRID, symbols="given")
        assert g.flips == 0
        far += err(g) > 3.0
    print(f"'given' ends more than 3 root bounds away on {far} of {len(RC.PLANTED_SEEDS)} draws")
    assert far == len(RC.PLANTED_SEEDS)


# ---- the table itself -----------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    names = [c.name for c in RC.cases()]
    assert len(set(names)) == len(names) >= 20
    assert {c.rows.shape[1] for c in RC.cases()} >= {1, 3, 16} and {c.grid for c in RC.cases()} >= {(1, 12), (12, 1), (4, 6), (8, 8), (26, 131)}
    assert max(c.grid[0] * c.grid[1] for c in RC.cases()) == 3406
    states = {r.state for c in RC.cases() for r in RC.reference(c.name)}
    assert states == {refine.CONVERGED, refine.LIMIT, refine.GAVE_UP, refine.NONFINITE, refine.OUTSIDE}
    for c in RC.cases():
        for i, r in enumerate(RC.reference(c.name)):
            if c.states is not None and c.states[i] is not None:
                assert r.state == c.states[i], (c.name, i, r.state)
            assert all(m <= 0.5 * (1 + 1e-12) for m in r.moves), (c.name, i)
    assert RC.reference("n_est")[0].iterations == 0 and np.isnan(RC.reference("n_est")[0].rows).all()
    assert np.isnan(RC.reference("absent_in_the_middle")[0].rows[1:3]).all()
    assert np.isnan(RC.reference("coincident_pair")[0].C).all() and not np.isnan(RC.reference("coincident_pair")[0].rows[:, :2]).any()
    assert sum(r.flips for r in RC.reference("L3_8x8_psk")) == 12 and RC.reference("L3_13x262_psk")[0].flips > 60


def test_the_converging_cases_contract():
    """The comparison of two fits at 4 tol rests on q < 1/2 for the ratio of consecutive steps: the mirror holds every converged
    scene of the table to it, but for at most MAX_DROPPED that are then left out of that comparison only."""
    dropped = RC.dropped()
    print("left out of the 4 tol comparison:", dropped)
    assert len(dropped) <= RC.MAX_DROPPED
    for c in RC.cases():
        for i in RC.comparable(c.name):
            assert RC.contraction(RC.reference(c.name)[i]) < RC.Q_MAX


# ---- 4. the host model under sanitizers -------------------------------------------------------------------------------------------------
def test_refine_core_under_sanitizers(tmp_path):
    """tests/host_model/refine_model.cpp (its own main, csrc/refine_core.h with the workgroup emulated, built with
    -fsanitize=address,undefined) on every scene of the case table, held to ``refine_host`` as the kernel is."""
    exe, inp = str(tmp_path / "refine_model"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "refine_model.cpp"), "-o", exe])
    lines, scenes = [], 0
    for c in RC.cases():
        for i in range(len(c.y)):
            n = "none" if c.n_est is None else int(c.n_est[i])
            lines.append(f"{c.grid[0]} {c.grid[1]} {c.rows.shape[1]} {n} {refine.MODES[c.symbols]} {RC.PSK[0]} {RC.PSK[1]!r} {c.iters} {RC.TOL!r}")
            lines += [" ".join(repr(float(v)) for v in row) for row in c.rows[i]]
            lines += [f"{float(a.real)!r} {float(a.imag)!r} {float(s.real)!r} {float(s.imag)!r}" for a, s in zip(c.y[i], c.b[i])]
            scenes += 1
    with open(inp, "w") as fh:
        fh.write(f"{scenes}\n" + "\n".join(lines) + "\n")
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-500:] + p.stderr)[-3000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = iter(p.stdout.split("\n"))
    worst = {}
    for c in RC.cases():
        B, Le = c.rows.shape[:2]
        D = c.y.shape[1]
        rows, C, info, sym = np.zeros((B, Le, 3)), np.zeros((B, Le), complex), np.zeros((B, 5)), np.zeros((B, D), int)
        for i in range(B):
            state, used, flips, Q = next(out).split()
            info[i] = [float(Q), float(Q) / D, int(used), int(flips), int(state)]
            for j in range(Le):
                v = [float(t) for t in next(out).split()]
                rows[i, j], C[i, j] = v[:3], complex(v[3], v[4])
            sym[i] = [int(t) for t in next(out).split()]
        worst[c.name] = RC.compare(c.name, rows, C, info, sym, "host model")
    print("worst distance / (4 tol):", {k: float(f"{v:.2g}") for k, v in worst.items()})


# ---- 5. one mistake is rejected ---------------------------------------------------------------------------------------------------------
def _fit(c, i=0, **kw):
    return refine.refine_host(c.y[i], c.b[i], c.rows[i], c.grid, n_est=None if c.n_est is None else int(c.n_est[i]), **{**c.kw, **kw})


def _same(name, got, i=0):
    c, r = RC.case(name), RC.reference(name)[i]
    here = ~np.isnan(r.rows[:, 0])
    return (got.state == r.state and np.array_equal(got.symbols, r.symbols) and
            float(np.abs(got.rows[here, 0] - r.rows[here, 0]).max()) * c.grid[1] <= 4 * RC.TOL and
            float(np.abs(got.rows[here, 1] - r.rows[here, 1]).max()) * c.grid[0] <= 4 * RC.TOL)


def test_one_mistake_is_rejected(monkeypatch):
    """Stand-ins -- the mirror with ONE of its parts replaced by a defective one -- are each rejected by a named case: held to the
    table's reference the way the kernel is, they fail."""
    model, limit, scaled, decide = refine.signal_model, refine.limit_step, refine.unit_diagonal, refine.decide

    def tau_sign(tau, f, C, grid):                       # the tau column of J with the sign of the f column
        mu, J = model(tau, f, C, grid)
        if grid[1] > 1:
            J[:, :len(tau)] *= -1.0
        return mu, J

    def exchanged(tau, f, C, grid):                      # i = i_d Nb + i_b
        mu, J = model(tau, f, C, grid)
        order = np.arange(grid[0] * grid[1]).reshape(grid).T.reshape(-1)
        return mu[order], J[order]

    def unscaled(G):
        return (G.copy(), np.ones(len(G))) if (np.diag(G) > 0).all() else None

    def against_x(y, x, mu, pts):
        return refine.nearest_point(x * np.conj(mu), pts)

    stand_ins = {
        "the sign of the tau column": ("signal_model", tau_sign, "L3_8x8"),
        "i_b and i_d exchanged": ("signal_model", exchanged, "L1_4x6"),
        "no unit-diagonal scaling": ("unit_diagonal", unscaled, "pair_26x131_far_start"),
        "a step not limited": ("limit_step", lambda dt, df, grid, cells=0.5: limit(dt, df, grid, cells=1e9), "L3_8x8_far_start"),
        "symbols re-decided against x": ("decide", against_x, "L3_8x8_psk"),
    }
    for what, (name, stand_in, case) in stand_ins.items():
        assert _same(case, _fit(RC.case(case))), case                 # the mirror itself passes ...
        with monkeypatch.context() as mp:
            mp.setattr(refine, name, stand_in)
            try:
                got = _fit(RC.case(case))
                rejected = not _same(case, got) or max(got.moves, default=0.0) > 0.5 * (1 + 1e-12)
            except np.linalg.LinAlgError:
                rejected = True
        print(f"{what}: rejected by {case}")
        assert rejected, what                                         # ... and the stand-in does not
    assert (refine.signal_model, refine.limit_step, refine.unit_diagonal, refine.decide) == (model, limit, scaled, decide)


# ---- 6. arguments and signatures --------------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_statement():
    c = RC.case("L3_8x8")
    for kw in (dict(symbols="qam"), dict(psk=(1, 0.0)), dict(psk=(65, 0.0)), dict(psk=(4, math.inf)), dict(psk=4), dict(iters=0),
               dict(iters=65), dict(tol=0.0), dict(tol=math.nan)):
        with pytest.raises(ValueError):
            refine.refine_host(c.y[0], c.b[0], c.rows[0], c.grid, **kw)
    for grid in ((8,), (0, 64), (4, 8)):
        with pytest.raises(ValueError):
            refine.refine_host(c.y[0], c.b[0], c.rows[0], grid)
    with pytest.raises(TypeError):
        refine.refine_targets(c.y, c.b, c.rows, c.grid)               # numpy arrays: the device call takes tensors
    import torch
    with pytest.raises(refine._lib.AdmmNetError):                      # ... on the device: no CPU fallback
        refine.refine_targets(torch.from_numpy(c.y), torch.from_numpy(c.b), torch.from_numpy(c.rows), c.grid)


def test_signatures():
    sig = inspect.signature(refine.refine_targets)
    assert list(sig.parameters) == ["y", "b", "rows", "grid", "n_est", "symbols", "psk", "iters", "tol", "out"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("n_est", "symbols", "psk", "iters", "tol", "out"))
    assert [sig.parameters[k].default for k in ("n_est", "symbols", "psk", "iters", "tol")] == [None, "given", (4, math.pi / 4), 16, 1e-6]
    assert list(inspect.signature(refine.refine_host).parameters) == list(sig.parameters)[:-1] and sig.parameters["out"].default is None
    assert refine.RefineResult._fields[:8] == ("rows", "C", "cost", "noise_var", "iterations", "flips", "state", "status")
    for cls in (modules.PhiEstADMMNet, modules.ADMMNet):
        s = inspect.signature(cls.estimate_refined)
        assert list(s.parameters) == ["self", "y", "b", "sigma", "top", "top_n", "opts", "symbols", "refine_kw"]
        assert s.parameters["symbols"].kind is inspect.Parameter.KEYWORD_ONLY and s.parameters["symbols"].default == "given"
        assert s.parameters["refine_kw"].kind is inspect.Parameter.VAR_KEYWORD
    names = list(inspect.signature(harness.evaluate_snr).parameters)
    assert names[-2:] == ["refine", "crb"] and inspect.signature(harness.evaluate_snr).parameters["refine"].default is None
    assert refine.STATES == ("converged", "limit", "gave up", "non-finite", "outside")


def test_refine_on_the_command_line(monkeypatch, capsys):
    seen, evaluate_snr = [], harness.evaluate_snr
    monkeypatch.setattr(harness, "evaluate_snr", lambda *a, **kw: seen.append(kw) or iter(()))
    harness.main(["evaluate", "--refine", "psk", "--crb"])
    harness.main(["evaluate"])
    assert [(kw["refine"], kw["crb"]) for kw in seen] == [("psk", True), (None, False)]
    with pytest.raises(SystemExit):
        harness.main(["evaluate", "--refine", "qam"])
    with pytest.raises(ValueError):
        next(evaluate_snr(refine="qam"))
