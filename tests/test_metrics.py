"""Host: the float64 statement of the scoring kernels (admm_net_amd/metrics.py), the scalar core under the sanitizers, the
argument checks and the symbol table.  tests/test_gpu_metrics.py holds the kernels to ``match_host`` on the GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, metrics

import metrics_cases as MC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host_model")


# ---- 1. match_host is the optimum ------------------------------------------------------------------------------------------------
def test_match_host_against_brute_force_and_scipy_on_4000_cases():
    """ne, nt in 1 .. 5: the cost of ``match_host`` equals the least cost of a plain loop over every assignment and scipy's, in
    all 4 000 cases; no case has two hit sets within 1e-9 relative of each other (so ``match`` itself is pinned); the stats follow
    from the match; and a nearest-neighbour matcher is worse in some of them, so these cases tell an optimal solver from it."""
    rng = np.random.default_rng(20260104)
    greedy_worse = close = 0
    for case in range(4000):
        Le, Lt = (int(v) for v in rng.integers(1, 6, size=2))
        est, tt, ft, L = MC.draw(1000 + case, 1, Le, Lt, partial=False, absent=0.1 if case % 3 == 0 else 0.0)
        match, stats, gap = metrics.match_host(est[0, :, 0], est[0, :, 1], tt[0], ft[0], cutoff=MC.CUTOFF, with_gap=True)
        live, cost, d2 = MC.cost_matrix(est[0], tt[0], ft[0])
        want = MC.brute_cost(cost)
        assert abs(stats[7] - want) <= 1e-12 * want, (case, stats[7], want)
        assert abs(MC.scipy_cost(cost) - want) <= 1e-12 * want, case
        close += gap <= 1e-9
        greedy_worse += MC.greedy_cost(cost) > want * (1 + 1e-9)
        # the stats are what the match says
        hits = [(e, j) for j, e in enumerate(match) if e >= 0]
        assert len({e for e, _ in hits}) == len(hits) and all(e in live for e, _ in hits)
        got, per_hit = MC.cost_of_match(match, stats, est[0], tt[0], ft[0])
        assert (per_hit < MC.CUTOFF ** 2).all() and abs(got - stats[7]) <= 1e-12 * stats[7]
        assert stats[0] == len(hits) and stats[0] + stats[1] == Lt and stats[0] + stats[2] == len(live)
        assert abs(stats[6] - (stats[5] + MC.CUTOFF ** 2 / 2 * (stats[1] + stats[2]))) <= 1e-15
    assert close == 0, f"{close} cases with two optimal hit sets"
    assert greedy_worse >= 20, f"a nearest-neighbour matcher is worse in only {greedy_worse} of 4000 cases"


def test_match_host_above_the_enumeration_uses_scipy_and_agrees_with_it_below():
    est, tt, ft, L = MC.draw(7, 6, 9, 8, partial=False)
    for b in range(6):
        match, stats = metrics.match_host(est[b, :, 0], est[b, :, 1], tt[b], ft[b], cutoff=MC.CUTOFF)
        live, cost, _ = MC.cost_matrix(est[b], tt[b], ft[b])
        assert abs(stats[7] - MC.scipy_cost(cost)) <= 1e-12 * stats[7]
        with pytest.raises(ValueError, match="with_gap"):
            metrics.match_host(est[b, :, 0], est[b, :, 1], tt[b], ft[b], cutoff=MC.CUTOFF, with_gap=True)


def test_the_named_cases_of_the_definition():
    # the chain: the identity is optimal, a nearest-neighbour matcher pays 0.4055 at m = 64
    for m in (3, 8, 64):
        tt = (0.1 + 0.01 * np.arange(m)).astype(np.float32)
        te = tt.astype(np.float64) + 0.006
        match, stats = metrics.match_host(te, np.zeros(m), tt, np.zeros(m), cutoff=10.0)
        assert np.array_equal(match, np.arange(m)) and abs(stats[7] - 3.6e-5 * m) < 1e-9
    _, cost, _ = MC.cost_matrix(np.stack([te, np.zeros(m), np.zeros(m)], axis=1), tt, np.zeros(m), cutoff=10.0)
    assert abs(MC.greedy_cost(cost) - 0.4055) < 1e-3
    # the truncation is inside the solve
    te, tt = np.array([0.26, 0.33]), np.array([0.20, 0.27], dtype=np.float32)
    match, stats = metrics.match_host(te, np.zeros(2), tt, np.zeros(2), cutoff=10.0)
    assert match.tolist() == [0, 1]
    match, stats = metrics.match_host(te, np.zeros(2), tt, np.zeros(2), cutoff=0.05)
    assert match.tolist() == [-1, 0] and stats[0] == 1 and abs(stats[7] - 0.0026) < 1e-8
    # the wrap
    for axis in (0, 1):
        e, t = ([0.01], [0.98]) if axis == 0 else ([-0.49], [0.49])
        args = (e, [0.0], t, [0.0]) if axis == 0 else ([0.3], e, [0.3], t)
        match, stats = metrics.match_host(*args, cutoff=0.1, period=(1.0, 1.0))
        assert match.tolist() == [0] and abs(stats[5] - (0.03 ** 2 if axis == 0 else 0.02 ** 2)) < 1e-9
        match, stats = metrics.match_host(*args, cutoff=0.1)
        assert match.tolist() == [-1] and stats[:3].tolist() == [0, 1, 1]
    # absent rows, no target
    match, stats = metrics.match_host([np.nan, 0.3], [0.0, np.inf], [0.3], [0.0], cutoff=0.1)
    assert match.tolist() == [-1] and stats[:3].tolist() == [0, 1, 0] and stats[6] == 0.5 * (0.1 * 0.1)
    match, stats = metrics.match_host([0.3], [0.0], [], [], cutoff=0.1)
    assert match.shape == (0,) and stats[:3].tolist() == [0, 0, 1]


# ---- 2. the ordered RMSE ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lmax,zero_only", [(1, 1, False), (37, 3, False), (9, 64, False), (5, 3, True)])
def test_ordered_rmse_host_is_the_loop_of_train_py(B, Lmax, zero_only):
    te, fe, tt, ft, L = MC.ordered_case(B + Lmax, B, Lmax, zero_only)
    per, out = metrics.ordered_rmse_host(te.numpy(), fe.numpy(), tt.numpy(), ft.numpy(), L.numpy())
    mt, mf, lt, lf = MC.train_py_loop(te, fe, tt, ft, L)
    assert out[2] == len(lt) and np.isnan(per[L.numpy() == 0]).all()
    assert np.allclose(per[L.numpy() > 0, 0], lt, rtol=1e-6, atol=0) and np.allclose(per[L.numpy() > 0, 1], lf, rtol=1e-6, atol=0)
    assert abs(out[0] - mt) <= 1e-6 * abs(mt) and abs(out[1] - mf) <= 1e-6 * abs(mf)


# ---- 3. summary ------------------------------------------------------------------------------------------------------------------
def test_summary():
    totals = torch.tensor([6.0, 2.0, 3.0, 6 * 0.01, 6 * 0.04, 1.0, 8.0, 0.0], dtype=torch.float64)
    s = metrics.summary(totals, signals=4)
    assert s["pd"] == 0.75 and s["false_per_signal"] == 0.75 and s["signals"] == 4
    assert abs(s["rmse_tau"] - 0.1) < 1e-15 and abs(s["rmse_f"] - 0.2) < 1e-15 and abs(s["gospa"] - np.sqrt(2.0)) < 1e-15
    res = metrics.MatchResult(torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, 8, dtype=torch.float64), totals,
                              torch.tensor([1, 0], dtype=torch.int32))
    assert metrics.summary(res)["signals"] == 4
    none = metrics.summary(torch.zeros(8, dtype=torch.float64), signals=0)
    assert all(np.isnan(none[k]) for k in ("pd", "rmse_tau", "rmse_f", "gospa", "false_per_signal"))
    with pytest.raises(ValueError, match="signals"):
        metrics.summary(totals)
    with pytest.raises(ValueError, match="8 entries"):
        metrics.summary(torch.zeros(7), signals=1)


# ---- 4. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    est, tt, ft = torch.zeros(2, 3, 3, dtype=torch.float64), torch.zeros(2, 3), torch.zeros(2, 3)
    with pytest.raises(_lib.AdmmNetError, match="HIP device tensor"):
        metrics.match_targets(est, tt, ft, cutoff=0.1)
    with pytest.raises(_lib.AdmmNetError, match="HIP device tensor"):
        metrics.ordered_rmse(tt, ft, tt, ft, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="tensor"):
        metrics.match_targets(est.numpy(), tt, ft, cutoff=0.1)
    with pytest.raises(ValueError, match="pair"):
        metrics.match_targets((tt, ft, tt), tt, ft, cutoff=0.1)
    with pytest.raises(TypeError):
        metrics.match_targets(est, tt, ft)                                # cutoff has no default
    for bad in (dict(cutoff=0.0), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(cutoff=1e200),
                dict(cutoff=0.1, scale=(0.0, 1.0)), dict(cutoff=0.1, scale=(1.0,)), dict(cutoff=0.1, scale=(1.0, float("inf"))),
                dict(cutoff=0.1, period=(-1.0, 0.0)), dict(cutoff=0.1, period=1.0)):
        with pytest.raises(ValueError):
            metrics.match_host([0.1], [0.0], [0.1], [0.0], **bad)
    with pytest.raises(ValueError, match="not finite"):
        metrics.match_host([0.1], [0.0], [np.nan], [0.0], cutoff=0.1)
    assert metrics._options(0.1, (2.0, 3.0), (None, 1.0)) == (2.0, 3.0, 0.1, 0.0, 1.0)
    assert metrics._options(0.1, (1.0, 1.0), None)[3:] == (0.0, 0.0)


def test_the_c_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.admmnet_score_partials(0) == -1 and lib.admmnet_score_partials(-5) == -1
    assert lib.admmnet_score_partials(1) == lib.admmnet_score_partials(4) and lib.admmnet_score_partials(5) == 2 * lib.admmnet_score_partials(4)
    p = ctypes.c_void_p(64)                      # never read: every case below is refused before a launch
    good = (ctypes.c_double * 5)(1.0, 1.0, 0.1, 0.0, 0.0)

    def match(Le=3, Lt=3, B=4, est=p, opts=good, part=p):
        return lib.admmnet_score_match_f64(Le, Lt, B, est, None, p, p, None, opts, p, p, p, p, part, None)

    for kw in (dict(Le=0), dict(Le=65), dict(Lt=0), dict(Lt=65), dict(B=0), dict(est=None), dict(part=None), dict(opts=None),
               dict(opts=(ctypes.c_double * 5)(0.0, 1.0, 0.1, 0.0, 0.0)), dict(opts=(ctypes.c_double * 5)(1.0, 1.0, 0.0, 0.0, 0.0)),
               dict(opts=(ctypes.c_double * 5)(1.0, 1.0, float("nan"), 0.0, 0.0)),
               dict(opts=(ctypes.c_double * 5)(1.0, 1.0, 1e200, 0.0, 0.0)),
               dict(opts=(ctypes.c_double * 5)(1.0, 1.0, 0.1, -1.0, 0.0))):
        assert match(**kw) != 0, kw
        assert b"score_match" in lib.admmnet_last_error()
    for Lmax, B, L_true in ((0, 4, p), (65, 4, p), (3, 0, p), (3, 4, None)):
        assert lib.admmnet_score_ordered_f32(Lmax, B, p, p, p, p, L_true, p, p, p, p, None) != 0
        assert b"score_ordered" in lib.admmnet_last_error()


# ---- 5. the symbol table and the public surface ----------------------------------------------------------------------------------
def test_symbols_and_signatures():
    c = ctypes
    assert _lib.SYMBOLS["admmnet_score_partials"] == (c.c_int64, [c.c_int64])
    res, args = _lib.SYMBOLS["admmnet_score_match_f64"]
    assert res is c.c_int32 and args == [c.c_int32, c.c_int32, c.c_int64] + [c.c_void_p] * 5 + [c.POINTER(c.c_double)] + [c.c_void_p] * 6
    res, args = _lib.SYMBOLS["admmnet_score_ordered_f32"]
    assert res is c.c_int32 and args == [c.c_int32, c.c_int64] + [c.c_void_p] * 10
    hdr = open(os.path.join(ROOT, "include", "admmnet.h")).read()
    for name in ("admmnet_score_partials", "admmnet_score_match_f64", "admmnet_score_ordered_f32"):
        assert hdr.count(name + "(") >= 1 and hasattr(_lib.load(), name)
    assert str(inspect.signature(metrics.match_targets)) == \
        "(est, tau_true, f_true, L_true=None, n_est=None, *, cutoff, scale=(1.0, 1.0), period=None) -> 'MatchResult'"
    assert str(inspect.signature(metrics.ordered_rmse)) == "(tau_est, f_est, tau_true, f_true, L_true)"
    for cls in (A.ADMMNet, A.PhiEstADMMNet):
        assert str(inspect.signature(cls.evaluate)) == ("(self, y, b, sigma, tau_true, f_true, L_true=None, *, cutoff, scale=None, "
                                                        "period=(1.0, 1.0), top=None, opts=None)")
    assert metrics.MatchResult._fields == ("match", "stats", "totals", "status") and len(metrics.STATS) == 8
    from admm_net_amd import build
    assert "score.hip" in build.SOURCES and "score_core.h" in build.HEADERS


def test_harness_commands_parse():
    from admm_net_amd import harness
    for argv in (["evaluate", "--grid", "10by10"], ["evaluate", "--baseline", "greedy"], ["score-step", "--steps", "x"]):
        with pytest.raises(SystemExit):
            harness.main(argv)
    with pytest.raises(ValueError, match="baseline"):
        next(harness.evaluate_snr(baseline="greedy"))


# ---- 6. the scalar core under the sanitizers -------------------------------------------------------------------------------------
def test_score_core_under_sanitizers(tmp_path):
    """tests/host_model/score_model.cpp (its own main, csrc/score_core.h only, the lane loop emulated): the search against brute
    force and a serial Hungarian method up to 64 x 64, absent rows, the chain, the truncation, wrap and clamp."""
    exe = str(tmp_path / "score_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "score_model.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "ok"
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
