"""Host: the float64 statement of the Cramer-Rao bound (``metrics.crb_host``) against closed forms, finite differences, the scene
generator's noise and a Monte-Carlo run; the kernel's scalar core (tests/host_model/crb_model.cpp) under the sanitizers against it
on the case table; one-mistake stand-ins; signatures and the symbol table.  tests/test_gpu_crb.py holds the kernel to the same
statement on the GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, build, harness, metrics

import crb_cases as CC
import synth_mirror as SM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host_model")


# ---- 1. crb_host itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(4, 6), (6, 4)])
def test_single_target_closed_form(grid):
    """L = 1: 6 v / ((2 pi)^2 |C|^2 Nb Nd (Nd^2 - 1)) for tau, the same with Nb^2 - 1 for f; independent of tau, f and arg C."""
    Nb, Nd = grid
    for tau, f, C, v in ((0.3, 0.1, 0.5 - 0.2j, 0.1), (0.77, -0.35, -1.3j, 2.5e-3)):
        r = metrics.crb_host([tau], [f], [C], grid, noise_var=v)
        scale = 6.0 * v / ((2 * np.pi) ** 2 * abs(C) ** 2 * Nb * Nd)
        assert r.state == -1 and r.bound.shape == (1, 2)
        assert np.allclose(r.bound[0], [scale / (Nd ** 2 - 1), scale / (Nb ** 2 - 1)], rtol=1e-13, atol=0), r.bound


def test_jacobian_against_central_differences():
    """d mu / d theta of ``crb_host`` against central differences of the signal built from ``synth.steering``; with h = 1e-5 the
    truncation error is (2 pi N h)^2 / 6 < 2e-7 relative and the rounding error 1e-16 / h = 1e-11."""
    c = CC.case("L3_10x10")
    tau, f, C = c.tau[0].astype(np.float64), c.f[0].astype(np.float64), c.C[0].astype(np.complex128)
    L, h = len(tau), 1e-5
    J = metrics.crb_host(tau, f, C, c.grid, noise_var=1.0).jacobian
    assert J.shape == (100, 4 * L)
    theta = np.concatenate([tau, f, C.real, C.imag])
    signal = lambda t: metrics.crb_signal(t[:L], t[L:2 * L], t[2 * L:3 * L] + 1j * t[3 * L:], c.grid)  # noqa: E731
    for p in range(4 * L):
        step = np.zeros(4 * L)
        step[p] = h
        fd = (signal(theta + step) - signal(theta - step)) / (2 * h)
        assert np.abs(fd - J[:, p]).max() <= 1e-6 * np.abs(J[:, p]).max(), p


def test_snr_noise_is_the_generators():
    """``snr_db`` gives the square of the device generator's noise deviation, from the mirror's float64 truth."""
    r = SM.mirror(np.arange(6), 4, 6, 3, seed=77)
    for i in range(6):
        v = metrics.crb_host(r["tau"][i], r["f"][i], r["C"][i], (4, 6), snr_db=float(r["snr"][i, 0])).noise_var
        assert abs(v - r["w_std"][i, 0] ** 2) <= 1e-12 * v, (i, v, r["w_std"][i, 0] ** 2)


def test_monte_carlo_attains_the_bound():
    """L = 1 on a 4 x 6 grid at 30 dB, 4000 noise draws, known symbols: the maximum-likelihood estimate (the peak of the
    zero-padded periodogram, then two Newton steps on |a(tau, f)^H y|^2) has sample variance / bound within 4.5 standard errors,
    sqrt(2 / 4000) each, of 1 -- this pins the constant (the 2, the 2 pi, the v) that no comparison of two formulas can."""
    Nb, Nd, n, pad = 4, 6, 4000, 64
    tau, f, C, snr = 0.3712, 0.1234, 0.6 - 0.45j, 30.0
    ref = metrics.crb_host([tau], [f], [C], (Nb, Nd), snr_db=snr)
    assert abs(ref.noise_var - abs(C) ** 2 / 1000.0) <= 1e-12 * ref.noise_var
    rng = np.random.default_rng(20260104)
    mu = metrics.crb_signal([tau], [f], [C], (Nb, Nd)).reshape(Nb, Nd)
    w = np.sqrt(ref.noise_var / 2) * (rng.standard_normal((n, Nb, Nd)) + 1j * rng.standard_normal((n, Nb, Nd)))
    y = mu[None] + w
    ib, idd = np.arange(Nb)[None, :, None], np.arange(Nd)[None, None, :]
    est = np.empty((n, 2))
    for lo in range(0, n, 500):
        yy = y[lo:lo + 500]
        Z = np.fft.ifft(np.fft.fft(yy, n=pad, axis=1), n=pad, axis=2)             # sum y exp(-j 2 pi (i_b f - i_d tau)) / pad
        k = np.abs(Z).reshape(len(yy), -1).argmax(axis=1)
        fe, te = (k // pad) / pad, (k % pad) / pad
        fe = np.where(fe >= 0.5, fe - 1.0, fe)
        for _ in range(2):
            a = yy * np.exp(-2j * np.pi * (ib * fe[:, None, None] - idd * te[:, None, None]))
            df, dt = -2j * np.pi * ib, 2j * np.pi * idd
            z, zf, zt = a.sum((1, 2)), (df * a).sum((1, 2)), (dt * a).sum((1, 2))
            zff, ztt, zft = (df * df * a).sum((1, 2)), (dt * dt * a).sum((1, 2)), (df * dt * a).sum((1, 2))
            g = 2 * np.stack([(np.conj(z) * zt).real, (np.conj(z) * zf).real], axis=1)
            H = 2 * np.array([[(np.conj(zt) * zt + np.conj(z) * ztt).real, (np.conj(zf) * zt + np.conj(z) * zft).real],
                              [(np.conj(zt) * zf + np.conj(z) * zft).real, (np.conj(zf) * zf + np.conj(z) * zff).real]])
            step = np.linalg.solve(H.transpose(2, 0, 1), g[:, :, None])[:, :, 0]
            te, fe = te - step[:, 0], fe - step[:, 1]
        est[lo:lo + 500] = np.stack([te, fe], axis=1)
    assert np.abs(est - [tau, f]).max() < 0.05                                     # no outlier: every draw found the main lobe
    ratio = est.var(axis=0, ddof=1) / ref.bound[0]
    print("sample variance / bound (tau, f):", ratio)
    assert np.all(np.abs(ratio - 1.0) <= 4.5 * np.sqrt(2.0 / n)), ratio


# ---- 2. the case table -------------------------------------------------------------------------------------------------------------
def test_cases_are_well_conditioned_or_exactly_degenerate():
    """Nothing sits near the 2^-40 pivot threshold: a scene is bounded with kappa < 1e9, or refused, or its unit-diagonal matrix
    is singular to rounding (a diagonal entry of 0, or a least eigenvalue below 1e-13)."""
    assert len({c.name for c in CC.cases()}) == len(CC.cases()) >= 20
    for c in CC.cases():
        r = CC.reference(c.name)
        assert r.status == c.status, (c.name, r.status)
        for i, state in enumerate(r.states):
            if state == -1 and r.params[i]:
                assert r.kappa[i] < CC.KAPPA_MAX, (c.name, i, r.kappa[i])
            if state == 2:
                L = c.tau.shape[1] if c.L_true is None else int(c.L_true[i])
                F = metrics.crb_host(c.tau[i, :L], c.f[i, :L], c.C[i, :L], c.grid, **CC.noise_of(c, i)).fisher
                g = np.diag(F)
                if (g > 0).all():
                    assert np.linalg.eigvalsh(F / np.sqrt(np.multiply.outer(g, g))).min() < 1e-13, (c.name, i)
    kappas = {n: np.nanmax(CC.reference(n).kappa) for n in ("pair_0.5_cells", "pair_0.1_cells", "pair_0.02_cells")}
    assert kappas["pair_0.5_cells"] < 1e3 < kappas["pair_0.1_cells"] < 1e6 < kappas["pair_0.02_cells"], kappas
    assert np.isposinf(CC.reference("1x1").bound).all()
    assert np.isposinf(CC.reference("1x12").bound[:, :, 1]).all() and np.isfinite(CC.reference("1x12").bound[:, :, 0]).all()
    assert np.isposinf(CC.reference("12x1").bound[:, :, 0]).all() and np.isfinite(CC.reference("12x1").bound[:, :, 1]).all()
    assert CC.reference("L16_16x16").params.max() == 64


def _scenes(c):
    """(index, L) of the scenes of a case whose L_true lies inside."""
    B, Lt = c.tau.shape
    Ls = [Lt if c.L_true is None else int(c.L_true[i]) for i in range(B)]
    return [(i, L) for i, L in enumerate(Ls) if 0 <= L <= Lt]


def test_crb_core_under_sanitizers(tmp_path):
    """tests/host_model/crb_model.cpp (its own main, csrc/crb_core.h with the lane loop emulated, built with
    -fsanitize=address,undefined) on every scene of the case table: states exactly, bounds within the table's tolerance."""
    exe, inp = str(tmp_path / "crb_model"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "crb_model.cpp"), "-o", exe])
    lines, index = [], []
    for c in CC.cases():
        for i, L in _scenes(c):
            (key, value), = CC.noise_of(c, i).items()
            lines.append(f"{c.grid[0]} {c.grid[1]} {L} {int(key == 'snr_db')} {value!r}")
            lines += [f"{float(c.tau[i, l])!r} {float(c.f[i, l])!r} {float(c.C[i, l].real)!r} {float(c.C[i, l].imag)!r}" for l in range(L)]
            index.append((c.name, i, L))
    with open(inp, "w") as fh:
        fh.write(f"{len(index)}\n" + "\n".join(lines) + "\n")
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = iter(p.stdout.split("\n"))
    got = {c.name: np.full(c.tau.shape + (2,), np.nan) for c in CC.cases()}
    states = {c.name: [0] * len(c.tau) for c in CC.cases()}
    for name, i, L in index:
        state, _ = next(out).split()
        states[name][i] = int(state)
        for l in range(L):
            got[name][i, l] = [float(v) for v in next(out).split()]
    worst = {}
    for c in CC.cases():
        status = tuple(sum(s == k for s in states[c.name]) for k in range(3))
        assert tuple(states[c.name]) == CC.reference(c.name).states, c.name
        worst[c.name] = CC.compare(c.name, got[c.name], status, "host model")
    print("host model, worst error / tolerance:", max(worst.values()), max(worst, key=worst.get))


# ---- 3. one mistake at a time ------------------------------------------------------------------------------------------------------
def _separable_worst(name, mistake):
    """Worst error / tolerance of ``separable`` over the scenes of a case; inf where its NaN / inf pattern differs."""
    c, r = CC.case(name), CC.reference(name)
    worst = 0.0
    for i, L in _scenes(c):
        if r.states[i] == 1 or L == 0:
            continue
        b = CC.separable(c.tau[i, :L], c.f[i, :L], c.C[i, :L], c.grid, mistake=mistake, **CC.noise_of(c, i))
        ref = r.bound[i, :L]
        if not (np.array_equal(np.isnan(b), np.isnan(ref)) and np.array_equal(np.isinf(b), np.isinf(ref))):
            return np.inf
        fin = np.isfinite(ref)
        if fin.any():
            worst = max(worst, float((np.abs(b[fin] - ref[fin]) / ref[fin]).max() / CC.tolerance(name)[i, 0, 0]))
    return worst


def test_the_separable_form_agrees_on_every_case():
    """The second formulation (power sums, Cholesky) against the first (explicit Jacobian, ``inv``): the reference is well inside
    the tolerance it is used with."""
    worst = {c.name: _separable_worst(c.name, None) for c in CC.cases()}
    print("separable form, worst error / tolerance:", max(worst.values()))
    assert max(worst.values()) <= 0.05, worst


@pytest.mark.parametrize("mistake, name", [("factor_2_dropped", "L1_4x6"), ("k_for_k_squared", "L1_4x6"), ("tau_sign", "L3_10x10"),
                                           ("Nb_Nd_exchanged", "L1_4x6"), ("no_scaling", "weak_target"),
                                           ("energy_per_target", "L3_10x10")])
def test_one_mistake_is_rejected_by_a_named_case(mistake, name):
    assert mistake in CC.MISTAKES and _separable_worst(name, None) <= 1.0
    assert _separable_worst(name, mistake) > 1.0, (mistake, name)


def test_hits_pooled_over_all_targets_is_rejected():
    """``pool`` follows ``match``; summing over all targets instead gives other totals wherever a target was missed."""
    r = CC.reference("L3_10x10")
    match = np.array([[0, -1, 2], [-1, -1, -1], [1, 0, 2]], dtype=np.int32)
    t = CC.pool(r.bound, None, match)
    assert t[2:4].tolist() == [9.0, 9.0] and t[6:8].tolist() == [5.0, 5.0]
    assert np.isclose(t[4], r.bound[:, :, 0][match >= 0].sum(), rtol=1e-15)
    everyone = CC.pool(r.bound, None, np.zeros_like(match))
    assert np.array_equal(everyone[4:], everyone[:4]) and not np.allclose(everyone[4:], t[4:], rtol=1e-3)
    assert CC.pool(r.bound, None, None)[4:].tolist() == [0.0] * 4
    mixed = CC.reference("mixed_L_true")
    assert CC.pool(mixed.bound, CC.case("mixed_L_true").L_true, None)[2:4].tolist() == [11.0, 11.0]


# ---- 4. the public surface ---------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_sources():
    c = ctypes
    assert _lib.SYMBOLS["admmnet_crb_partials"] == (c.c_int64, [c.c_int64])
    res, args = _lib.SYMBOLS["admmnet_crb_f64"]
    assert res is c.c_int32 and args == [c.c_int32, c.c_int32, c.c_int32, c.c_int64] + [c.c_void_p] * 6 + [c.c_int32] + [c.c_void_p] * 5
    hdr = open(os.path.join(ROOT, "include", "admmnet.h")).read()
    for name in ("admmnet_crb_partials", "admmnet_crb_f64"):
        assert hdr.count(name + "(") >= 1 and hasattr(_lib.load(), name)
    assert str(inspect.signature(metrics.crb)) == \
        "(tau_true, f_true, C, grid, *, snr_db=None, noise_var=None, L_true=None, match=None) -> 'CrbResult'"
    assert str(inspect.signature(metrics.crb_summary)) == "(result) -> 'dict'"
    assert str(inspect.signature(metrics.crb_host)) == "(tau, f, C, grid, *, snr_db=None, noise_var=None) -> 'CrbHost'"
    assert metrics.CrbResult._fields == ("bound", "totals", "status") and metrics.PIVOT_MIN == 2.0 ** -40
    assert "knows" in metrics.crb.__doc__.lower() and "lower bound" in metrics.crb.__doc__
    assert list(inspect.signature(harness.evaluate_snr).parameters)[-1] == "crb"
    assert inspect.signature(harness.evaluate_snr).parameters["crb"].default is False
    assert "crb.hip" in build.SOURCES and "crb_core.h" in build.HEADERS
    assert "crb_kernel" in open(os.path.join(CSRC, "crb.hip")).read()


def test_the_c_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.admmnet_crb_partials(0) == -1 and lib.admmnet_crb_partials(2 ** 31) == -1
    assert lib.admmnet_crb_partials(7) == 7 * lib.admmnet_crb_partials(1) > 0
    p = ctypes.c_void_p(64)                      # never read: every case below is refused before a launch

    def call(Nb=4, Nd=6, Lt=3, B=4, tau=p, C=p, noise=p, is_snr=1, bound=p, part=p):
        return lib.admmnet_crb_f64(Nb, Nd, Lt, B, tau, p, C, None, None, noise, is_snr, bound, p, p, part, None)

    for kw in (dict(Lt=0), dict(Lt=17), dict(B=0), dict(B=2 ** 31), dict(Nb=0), dict(Nd=0), dict(Nb=59, Nd=59), dict(tau=None),
               dict(C=None), dict(noise=None), dict(is_snr=2), dict(bound=None), dict(part=None)):
        assert call(**kw) != 0, kw
        assert b"crb" in lib.admmnet_last_error()


def test_python_refusals_on_the_host():
    t, C = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.complex64)
    with pytest.raises(_lib.AdmmNetError, match="device tensor"):
        metrics.crb(t, t, C, (4, 6), snr_db=10.0)
    with pytest.raises(TypeError):
        metrics.crb(t.numpy(), t, C, (4, 6), snr_db=10.0)
    with pytest.raises(TypeError):
        metrics.crb_summary(torch.zeros(8))
    for kw in ({}, dict(snr_db=1.0, noise_var=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            metrics.crb_host([0.3], [0.1], [1.0], (4, 6), **kw)


def test_harness_arguments_parse(monkeypatch):
    seen = {}

    def fake(*args, **kw):
        seen.update(kw, n=len(args))
        return iter(())

    monkeypatch.setattr(harness, "evaluate_snr", fake)
    harness.main(["evaluate", "--snr", "5", "--crb"])
    assert seen["crb"] is True
    harness.main(["evaluate", "--snr", "5"])
    assert seen["crb"] is False
    with pytest.raises(SystemExit):
        harness.main(["evaluate", "--crb", "yes"])
