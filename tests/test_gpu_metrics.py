"""GPU: the scoring kernels (csrc/score.hip, admm_net_amd/metrics.py) against their float64 host statement.

``match_targets`` is held to optimality -- the cost of what it reports equals scipy's optimum to 1e-12 relative, both float64
and apart only in the order of their sums -- and, where the optimum's hit set is unique beyond rounding, to ``match_host``'s hit
set; the named cases of the definition (a chain that needs a whole augmenting path, the truncation inside the solve, the wrap,
absent rows, the status words), the batch sums, ``ordered_rmse`` against the literal loop of train.py:262-274,
``model.evaluate`` against ``estimate`` + ``match_host``, the input forms of tests/presentations.py and the absence of any
host read.  Shapes: every (Le, Lt) class the kernel treats differently -- one row, one column, rows on either side, more rows
than a nearest-neighbour pass can get right, the full 64 lanes; B = 64 spans 16 workgroups.
"""
import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import metrics, ops, synth

import metrics_cases as MC
import presentations as P
from golden_util import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 3), (3, 1), (3, 3), (2, 5), (5, 2), (8, 8), (17, 33), (64, 3), (3, 64), (64, 64)]
C2 = MC.CUTOFF * MC.CUTOFF


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(est, tt, ft, L=None, n_est=None, **kw):
    kw.setdefault("cutoff", MC.CUTOFF)
    r = metrics.match_targets(dev(est), dev(tt), dev(ft), dev(L), dev(n_est), **kw)
    return r.match.cpu().numpy(), r.stats.cpu().numpy(), r.totals.cpu().numpy(), r.status.cpu().numpy()


@pytest.fixture(scope="module")
def random_cases():
    """{(Le, Lt): (inputs, device outputs)}, computed once and left unchanged."""
    out = {}
    for i, (Le, Lt) in enumerate(SHAPES):
        case = MC.draw(500 + i, 8 if (Le, Lt) == (64, 64) else 64, Le, Lt)
        out[Le, Lt] = (case, run(*case))
    return out


# ---- (a) optimality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_match_is_an_optimal_assignment(random_cases, shape):
    (est, tt, ft, L), (match, stats, totals, status) = random_cases[shape]
    assert status.tolist() == [0, 0] and np.isfinite(stats).all()
    worst = 0.0
    for b in range(len(L)):
        m = match[b]
        hits = m[m >= 0]
        assert (m[L[b]:] == -1).all() and len(set(hits.tolist())) == len(hits), (b, m)          # injective, inside the targets
        live, cost, _ = MC.cost_matrix(est[b], tt[b, :L[b]], ft[b, :L[b]])
        assert set(hits.tolist()) <= set(live.tolist()), (b, m)                                   # only present rows
        assert stats[b, 0] == len(hits) and stats[b, 1] == L[b] - len(hits) and stats[b, 2] == len(live) - len(hits)
        got, per_hit = MC.cost_of_match(m[:L[b]], stats[b], est[b], tt[b, :L[b]], ft[b, :L[b]])
        assert (per_hit < C2).all(), (b, per_hit)                                                  # every reported pair is a hit
        want = MC.scipy_cost(cost)
        assert abs(got - stats[b, 7]) <= 1e-12 * abs(got), (b, got, stats[b, 7])
        assert abs(stats[b, 7] - want) <= 1e-12 * abs(want), (b, stats[b, 7], want)
        assert abs(stats[b, 5] - per_hit.sum()) <= 1e-12 * per_hit.sum()
        assert abs(stats[b, 6] - (stats[b, 5] + C2 / 2 * (stats[b, 1] + stats[b, 2]))) <= 1e-12 * stats[b, 6]
        worst = max(worst, abs(stats[b, 7] - want) / want if want else 0.0)
    print(f"{shape}: largest relative distance to scipy's optimum {worst:.3e}")


# ---- (b) the hit set ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in SHAPES if min(s) <= 5], ids=lambda s: "%dx%d" % s)
def test_match_equals_match_host_where_the_hit_set_is_unique(random_cases, shape):
    (est, tt, ft, L), (match, stats, _, _) = random_cases[shape]
    n = len(L) if max(shape) < 64 else 16                      # (the enumeration of 64 x 3 is 250 000 assignments a signal)
    want, wstats, gaps = MC.host_batch(est[:n], tt[:n], ft[:n], L[:n], with_gap=True)
    unique = gaps > 1e-9
    left_out = 1.0 - unique.mean()
    print(f"{shape}: {left_out:.2%} of {n} signals left out (two hit sets within 1e-9)")
    assert left_out == 0.0                                     # the seed leaves out none (the cap is 1 %)
    assert np.array_equal(match[:n][unique], want[unique])
    assert np.allclose(stats[:n][unique], wstats[unique], rtol=1e-12, atol=0)


# ---- (c) chains that need a full augmenting path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 8, 64])
def test_chain_needs_the_whole_augmenting_path(m):
    tt = (0.1 + 0.01 * np.arange(m)).astype(np.float32)[None]
    est = np.zeros((1, m, 3))
    est[0, :, 0] = tt[0].astype(np.float64) + 0.006
    match, stats, _, _ = run(est, tt, np.zeros_like(tt), cutoff=10.0)
    print(f"m={m}: cost {stats[0, 7]:.12g}")
    assert np.array_equal(match[0], np.arange(m))
    assert abs(stats[0, 7] - 3.6e-5 * m) < 1e-9 and stats[0, 0] == m          # (a nearest-neighbour pass pays 0.4055 at m = 64)
    hmatch, hstats = metrics.match_host(est[0, :, 0], est[0, :, 1], tt[0], np.zeros(m), cutoff=10.0)
    assert np.array_equal(match[0], hmatch) and np.allclose(stats[0], hstats, rtol=1e-12, atol=0)


# ---- (d) the truncation is inside the solve --------------------------------------------------------------------------------------------
def test_truncation_is_part_of_the_assignment():
    est = np.array([[[0.26, 0.0, 1.0], [0.33, 0.0, 0.5]]])
    tt, ft = np.array([[0.20, 0.27]], dtype=np.float32), np.zeros((1, 2), dtype=np.float32)
    match, stats, _, _ = run(est, tt, ft, cutoff=10.0)
    assert match.tolist() == [[0, 1]] and stats[0, :3].tolist() == [2, 0, 0]
    match, stats, _, _ = run(est, tt, ft, cutoff=0.05)
    print(f"c = 0.05: match {match.tolist()}, cost {stats[0, 7]:.12g}")
    assert match.tolist() == [[-1, 0]] and stats[0, :3].tolist() == [1, 1, 1]   # gating the untruncated optimum would give none
    assert abs(stats[0, 7] - 0.0026) < 1e-8


# ---- (e) the wrap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_periodic_axes_wrap(axis):
    est, tt, ft = np.zeros((1, 1, 3)), np.zeros((1, 1), dtype=np.float32), np.zeros((1, 1), dtype=np.float32)
    if axis == 0:
        est[0, 0, 0], tt[0, 0] = 0.01, 0.98
    else:
        est[0, 0, 1], ft[0, 0] = -0.49, 0.49
    match, stats, _, _ = run(est, tt, ft, period=(1.0, 1.0))
    want = 0.03 if axis == 0 else 0.02
    assert match.tolist() == [[0]] and abs(stats[0, 3 + axis] - want ** 2) < 1e-8 and stats[0, 4 - axis] == 0
    match, stats, _, _ = run(est, tt, ft)
    assert match.tolist() == [[-1]] and stats[0, :3].tolist() == [0, 1, 1] and stats[0, 6] == C2     # a miss and a false alarm
    match, stats, _, _ = run(est, tt, ft, period=(1.0, 0.0) if axis == 0 else (None, 1.0))
    assert match.tolist() == [[0]]


# ---- (f) absent rows and the status words ----------------------------------------------------------------------------------------------
def test_absent_rows_and_status_words():
    B, Le, Lt = 9, 4, 3
    est, tt, ft, _ = MC.draw(77, B, Le, Lt, partial=False, absent=0.0)
    L = np.full(B, Lt, dtype=np.int64)
    n_est = np.full(B, Le, dtype=np.int32)
    est[0, 2:] = np.nan                  # NaN rows, as peak_top pads them
    est[1, 1, 1] = np.inf                # one coordinate not finite: the row is absent
    n_est[2] = 2                         # only the first two rows count
    n_est[3], n_est[4] = -5, 99          # held to 0 .. Le
    L[5] = 0                             # no target
    est[6] = np.nan                      # no estimate
    L[7] = Lt + 1                        # outside: status[0]
    tt[8, 1] = np.nan                    # a target that is no number: status[1]
    match, stats, totals, status = run(est, tt, ft, L, n_est)
    assert status.tolist() == [1, 1]
    assert np.isnan(stats[7:]).all() and (match[7:] == -1).all()
    ok = np.arange(7)
    Lh = L.copy()
    want, wstats, _ = MC.host_batch(est[ok], tt[ok], ft[ok], Lh[ok], n_est[ok])
    assert np.array_equal(match[ok], want) and np.allclose(stats[ok], wstats, rtol=1e-12, atol=0)
    assert stats[0, 0] + stats[0, 2] == 2 and stats[1, 0] + stats[1, 2] == Le - 1 and stats[2, 0] + stats[2, 2] == 2
    assert stats[3, :3].tolist() == [0, Lt, 0] and stats[4, 0] + stats[4, 2] == Le
    assert stats[5, :3].tolist() == [0, 0, Le] and stats[5, 6] == C2 / 2 * Le and (match[5] == -1).all()
    assert stats[6, :3].tolist() == [0, Lt, 0] and stats[6, 7] == 0
    assert np.allclose(totals, stats[ok].sum(axis=0), rtol=1e-12, atol=0)              # the two NaN signals are left out
    # a NaN truth beyond L_true is not read as a target
    L[8] = 1
    _, stats, _, status = run(est, tt, ft, L, n_est)
    assert status.tolist() == [1, 0] and np.isfinite(stats[8]).all()
    # L_true = None: every slot counts
    m1, s1, _, _ = run(est[:5], tt[:5], ft[:5])
    m2, s2, _, _ = run(est[:5], tt[:5], ft[:5], np.full(5, Lt, dtype=np.int64))
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)
    # the pair form is the row form
    r = metrics.match_targets((dev(est[:5, :, 0].astype(np.float32)), dev(est[:5, :, 1].astype(np.float32))), dev(tt[:5]),
                              dev(ft[:5]), cutoff=MC.CUTOFF)
    e32 = est[:5].astype(np.float32).astype(np.float64)
    m3, s3, _, _ = run(e32, tt[:5], ft[:5])
    assert np.array_equal(r.match.cpu().numpy(), m3) and np.array_equal(r.stats.cpu().numpy(), s3, equal_nan=True)


# ---- (g) the batch sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257, 70000])
def test_totals_are_the_column_sums_and_repeat_bit_for_bit(B):
    rng = np.random.default_rng(B)
    tt = rng.uniform(0.1, 0.9, size=(B, 3)).astype(np.float32)
    ft = rng.uniform(-0.4, 0.4, size=(B, 3)).astype(np.float32)
    est = np.stack([tt[:, ::-1] + rng.normal(0, 0.03, size=(B, 3)), ft[:, ::-1] + rng.normal(0, 0.03, size=(B, 3)),
                    np.ones((B, 3))], axis=2)
    args = (dev(est), dev(tt), dev(ft))
    a = metrics.match_targets(*args, cutoff=MC.CUTOFF)
    b = metrics.match_targets(*args, cutoff=MC.CUTOFF)
    stats, totals = a.stats.cpu().numpy(), a.totals.cpu().numpy()
    want = stats.sum(axis=0)
    print(f"B={B}: totals {totals.tolist()}, largest relative distance {np.max(np.abs(totals - want) / np.maximum(want, 1e-300)):.3e}")
    assert np.isfinite(stats).all() and totals[0] > 0 and totals[0] + totals[1] == 3 * B
    assert np.allclose(totals, want, rtol=1e-12, atol=0)
    assert P.same_bits(a.totals, b.totals) and P.same_bits(a.stats, b.stats) and P.same_bits(a.match, b.match)
    assert a.status.tolist() == [0, 0]


# ---- (h) the ordered RMSE --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lmax,zero_only", [(1, 1, False), (37, 3, False), (9, 64, False), (5, 3, True), (1030, 3, False)])
def test_ordered_rmse_is_the_loop_of_train_py(B, Lmax, zero_only):
    te, fe, tt, ft, L = MC.ordered_case(B + Lmax, B, Lmax, zero_only)
    per, out, status = metrics.ordered_rmse(*(t.to(DEV) for t in (te, fe, tt, ft, L)))
    per, out = per.cpu().numpy(), out.cpu().numpy()
    mt, mf, lt, lf = MC.train_py_loop(te, fe, tt, ft, L)
    some = L.numpy() > 0
    assert status.tolist() == [0] and out[2] == len(lt) and np.isnan(per[~some]).all()
    assert np.allclose(per[some, 0], lt, rtol=1e-6, atol=0) and np.allclose(per[some, 1], lf, rtol=1e-6, atol=0)
    assert abs(out[0] - mt) <= 1e-6 * abs(mt) and abs(out[1] - mf) <= 1e-6 * abs(mf)
    hper, hout = metrics.ordered_rmse_host(te.numpy(), fe.numpy(), tt.numpy(), ft.numpy(), L.numpy())
    assert np.allclose(per, hper, rtol=1e-13, atol=0, equal_nan=True) and np.allclose(out, hout, rtol=1e-12, atol=0)
    if not zero_only and B > 2:                            # an L_true outside [0, Lmax] is counted and held to the range
        L2 = L.clone()
        L2[0], L2[1] = -1, Lmax + 3
        per2, _, status2 = metrics.ordered_rmse(*(t.to(DEV) for t in (te, fe, tt, ft, L2)))
        hper2, _ = metrics.ordered_rmse_host(te.numpy(), fe.numpy(), tt.numpy(), ft.numpy(), L2.numpy())
        assert status2.tolist() == [2] and np.allclose(per2.cpu().numpy(), hper2, rtol=1e-13, atol=0, equal_nan=True)


# ---- (i) model.evaluate ----------------------------------------------------------------------------------------------------------------
def test_evaluate_is_estimate_then_match(golden_dir):
    import os
    z, sd, (Nb, Nd, K, _, L, head, _) = load_fixture(os.path.join(golden_dir, "phiest_10x10_K10_trained.npz"))
    m = A.PhiEstADMMNet(M=Nb, N=Nd, L=L, num_layers=K).eval()
    m.load_state_dict(sd)
    B = 12
    y, b, sigma, truth = synth.make_batch_device(B, Nb, Nd, L=L, seed=31, device=DEV)
    res = m.evaluate(y, b, sigma, truth["tau"], truth["f"], cutoff=1.0)
    tau, f, height, counts, phi = m.estimate(y, b, sigma)
    tt, ft = truth["tau"].cpu().numpy(), truth["f"].cpu().numpy()
    match, stats = res.match.cpu().numpy(), res.stats.cpu().numpy()
    for i in range(B):
        hm, hs = metrics.match_host(tau[i].cpu().numpy(), f[i].cpu().numpy(), tt[i], ft[i], cutoff=1.0, scale=(Nd, Nb),
                                    period=(1.0, 1.0))
        assert np.array_equal(match[i], hm), (i, match[i], hm)
        assert np.allclose(stats[i], hs, rtol=1e-12, atol=0), (i, stats[i], hs)
    s = metrics.summary(res)
    print("evaluate:", s)
    assert s["signals"] == B and s["hits"] + s["misses"] == B * L and s["hits"] > 0
    half = m.evaluate(y, b, sigma, truth["tau"], truth["f"], torch.full((B,), 1, device=DEV), cutoff=1.0, scale=(2.0 * Nd, 2.0 * Nb))
    assert half.stats[:, :2].sum(dim=1).tolist() == [1.0] * B


# ---- (j) the input forms ---------------------------------------------------------------------------------------------------------------
def _forms_case(constant):
    est, tt, ft, L = MC.draw(5, 6, 4, 3, absent=0.0)
    t = dict(est=torch.from_numpy(est), tau_true=torch.from_numpy(tt), f_true=torch.from_numpy(ft), L_true=torch.from_numpy(L),
             n_est=torch.tensor([4, 3, 2, 4, 1, 0], dtype=torch.int32))
    if constant:
        t = {k: P.constant_along0(v) for k, v in t.items()}
    return {k: v.to(DEV) for k, v in t.items()}


def _match_call(t, pair):
    est = (t["tau_est"], t["f_est"]) if pair else t["est"]
    r = metrics.match_targets(est, t["tau_true"], t["f_true"], t["L_true"], t["n_est"], cutoff=MC.CUTOFF, period=(1.0, 1.0))
    return list(r)


def _ordered_call(t, pair):
    return list(metrics.ordered_rmse(t["tau_est"], t["f_est"], t["tau_true"], t["f_true"], t["L_true"]))


@pytest.mark.parametrize("entry", ["match_rows", "match_pair", "ordered"])
@pytest.mark.parametrize("form", ["neg_view", "sliced", "permuted", "expanded", "offset", "wide", "leaf"])
def test_every_input_form_gives_the_plain_bits(entry, form):
    """(``lazy_conj`` applies to complex tensors only: neither entry point takes one.)"""
    if form in P.ABSENT:
        pytest.fail(f"torch lacks what the form {form} needs")
    t = _forms_case(constant=form == "expanded")
    if entry != "match_rows":
        t["tau_est"], t["f_est"] = (t["est"][:, :3, i].to(torch.float32).contiguous() for i in (0, 1))
        del t["est"]
    if entry == "ordered":
        del t["n_est"]
    call = _ordered_call if entry == "ordered" else _match_call
    plain = call(t, entry == "match_pair")
    assert not all(torch.isnan(o.double()).all() for o in plain)
    applied = 0
    for name in t:
        v = P.present(form, t[name])
        if v is None:
            continue
        applied += 1
        got = call({**t, name: v}, entry == "match_pair")
        assert all(P.same_bits(g, p) for g, p in zip(got, plain)), (entry, form, name)
        assert torch.equal(v.detach().resolve_neg().to(t[name].dtype), t[name]), (entry, form, name)          # the input still holds its value
    assert applied, (entry, form)


# ---- (k) no host read ------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    t = _forms_case(constant=False)
    te, fe = (t["est"][:, :3, i].to(torch.float32).contiguous() for i in (0, 1))
    metrics.match_targets(t["est"], t["tau_true"], t["f_true"], cutoff=MC.CUTOFF)          # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = metrics.match_targets(t["est"], t["tau_true"], t["f_true"], t["L_true"], t["n_est"], cutoff=MC.CUTOFF, period=(1.0, 1.0))
        q = metrics.match_targets((te, fe), t["tau_true"], t["f_true"], cutoff=MC.CUTOFF)
        o = metrics.ordered_rmse(te, fe, t["tau_true"], t["f_true"], t["L_true"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert r.totals[0].item() > 0 and q.status.tolist() == [0, 0] and o[1][2].item() > 0
