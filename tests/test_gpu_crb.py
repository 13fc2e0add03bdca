"""GPU: the Cramer-Rao bound kernel (csrc/crb.hip, ``metrics.crb``) against its float64 host statement ``metrics.crb_host``.

Every case of tests/crb_cases.py at the table's tolerance 64 (P + Nb + Nd) kappa 2^-53, status counts, inf and NaN positions
exactly; the batch totals against the float64 sum of the per-target bounds and bit for bit across two calls; the ``match`` pool
against a host mask; the two noise inputs; independence of a scene from its place and its neighbours; the input forms of
tests/presentations.py; the refusals; ``harness.evaluate_snr(crb=True)``.  Shapes: the table's (P = 4 .. 64, both axes down to
length 1, Nd = 131 > 64 for the serial loop); B = 2500 spans 2500 workgroups and 40 rows per slice of the finishing sum.
"""
import numpy as np
import pytest
import torch

from admm_net_amd import _lib, harness, metrics

import crb_cases as CC
import presentations as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in CC.cases()]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def noise_kw(noise):
    return {k: dev(v) if np.ndim(v) else v for k, v in noise.items()}


def run(c, match=None, **noise):
    return metrics.crb(dev(c.tau), dev(c.f), dev(c.C), c.grid, L_true=dev(c.L_true), match=dev(match), **noise_kw(noise or c.noise))


def host(r):
    return r.bound.cpu().numpy(), r.totals.cpu().numpy(), r.status.cpu().numpy()


# ---- (a) the case table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_against_crb_host(name):
    c = CC.case(name)
    bound, totals, status = host(run(c))
    worst = CC.compare(name, bound, status, "kernel")
    print(f"{name}: worst error / tolerance {worst:.3g}, kappa {np.nanmax(CC.reference(name).kappa) if worst else 0:.3g}")
    want = CC.pool(CC.reference(name).bound, c.L_true, None)
    assert np.array_equal(totals[2:4], want[2:4]) and totals[4:].tolist() == [0.0] * 4
    tol = float(CC.tolerance(name).max()) + bound[:, :, 0].size * 2.0 ** -52
    assert np.allclose(totals[:2], want[:2], rtol=tol, atol=0), (totals, want)


def test_summary_is_one_read_of_the_totals():
    c = CC.case("mixed_L_true")
    match = np.array([[0, 1, 2, 3], [-1, 0, 0, 0], [2, -1, 0, -1], [0, 1, 5, 5], [-1, -1, -1, -1]], dtype=np.int32)
    r = run(c, match=match)
    s = metrics.crb_summary(r)
    t = CC.pool(r.bound.cpu().numpy(), c.L_true, match)
    assert (s["targets_tau"], s["targets_f"], s["hits_tau"], s["hits_f"]) == (11, 11, 4, 4) == tuple(int(v) for v in t[[2, 3, 6, 7]])
    for key, num, den in (("crb_tau", 0, 2), ("crb_f", 1, 3), ("crb_tau_hits", 4, 6), ("crb_f_hits", 5, 7)):
        assert np.isclose(s[key], np.sqrt(t[num] / t[den]), rtol=1e-14, atol=0), key
    assert (s["outside"], s["nonfinite"], s["not_positive_definite"]) == (0, 0, 0)
    none = metrics.crb_summary(run(c))
    assert np.isnan(none["crb_tau_hits"]) and none["hits_f"] == 0 and none["crb_tau"] == s["crb_tau"]


# ---- (b) reproducibility and pooling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 2500])
def test_totals_are_the_sum_of_the_bounds_and_reproducible(B):
    """The totals equal the float64 sum of the per-target bounds (numpy's pairwise sum and the kernel's fixed order differ by at
    most the number of terms times 2^-53 each, all terms positive), the counts exactly, and two calls give the same bits."""
    Lt = 3
    tau, f, C = CC.draw(100 + B, B, Lt)
    rng = np.random.default_rng(B)
    L = rng.integers(0, Lt + 1, B)
    match = rng.integers(-1, Lt, (B, Lt)).astype(np.int32)
    args = (dev(tau), dev(f), dev(C), (10, 10))
    kw = dict(snr_db=15.0, L_true=dev(L), match=dev(match))
    first, second = metrics.crb(*args, **kw), metrics.crb(*args, **kw)
    for a, b in zip(first, second):
        assert P.same_bits(a, b)
    bound, totals, status = host(first)
    want = CC.pool(bound, L, match)
    assert status[0] == 0 and status[1] == 0 and status[2] <= B // 100          # a random pair may coincide to rounding; few do
    assert np.array_equal(totals[[2, 3, 6, 7]], want[[2, 3, 6, 7]]), (totals, want)
    assert totals[2] == totals[3] > 0 or B == 1
    assert np.allclose(totals[[0, 1, 4, 5]], want[[0, 1, 4, 5]], rtol=B * Lt * 2.0 ** -52, atol=0), (totals, want)
    everyone = CC.pool(bound, L, np.zeros_like(match))
    assert B == 1 or not np.allclose(totals[4:6], everyone[4:6], rtol=1e-3)      # the hits are not all the targets


# ---- (c) noise input and placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L3_10x10", "mixed_L_true"])
def test_snr_against_noise_var_from_the_host(name):
    c = CC.case(name)
    v = np.ones(len(c.tau))
    for i in range(len(c.tau)):
        L = c.tau.shape[1] if c.L_true is None else int(c.L_true[i])
        if L:
            v[i] = metrics.crb_host(c.tau[i, :L], c.f[i, :L], c.C[i, :L], c.grid, **CC.noise_of(c, i)).noise_var
    bound, _, status = host(run(c, noise_var=v))
    CC.compare(name, bound, status, "noise_var from the host")


def test_a_number_is_a_constant_tensor():
    c = CC.case("L3_10x10")
    plain = run(c)
    for value in (np.full(3, 15.0), np.full(3, 15.0, dtype=np.float32), np.full(3, 15, dtype=np.int64)):
        assert all(P.same_bits(a, b) for a, b in zip(run(c, snr_db=value), plain))
    byvar = run(c, noise_var=0.02)
    assert all(P.same_bits(a, b) for a, b in zip(run(c, noise_var=np.full(3, 0.02)), byvar))
    assert not P.same_bits(byvar.bound, plain.bound)


def test_a_scene_does_not_depend_on_its_place_or_neighbours():
    c = CC.case("L3_10x10")
    alone = [metrics.crb(dev(c.tau[i:i + 1]), dev(c.f[i:i + 1]), dev(c.C[i:i + 1]), c.grid, snr_db=15.0).bound[0] for i in range(3)]
    order = [2, 0, 0, 1, 0]                                  # scenes 2, (NaN), (coincident), 1, 0
    tau, f, C = c.tau[order].copy(), c.f[order].copy(), c.C[order].copy()
    tau[1, 1] = np.nan
    tau[2, 1], f[2, 1] = tau[2, 0], f[2, 0]
    r = metrics.crb(dev(tau), dev(f), dev(C), c.grid, snr_db=15.0)
    assert r.status.tolist() == [0, 1, 1]
    assert torch.isnan(r.bound[1:3]).all()
    for row, scene in ((0, 2), (3, 1), (4, 0)):
        assert P.same_bits(r.bound[row], alone[scene]), (row, scene)


# ---- (d) the input forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sliced", "permuted", "expanded", "offset", "neg_view", "lazy_conj"])
def test_every_input_form_gives_the_plain_bits(form):
    if form in P.ABSENT:
        pytest.fail(f"torch lacks what the form {form} needs")
    c = CC.case("L3_10x10")
    t = dict(tau_true=dev(c.tau), f_true=dev(c.f), C=dev(c.C))
    if form == "expanded":
        t = {k: P.constant_along0(v) for k, v in t.items()}
    call = lambda t: metrics.crb(t["tau_true"], t["f_true"], t["C"], c.grid, snr_db=15.0)  # noqa: E731
    plain = call(t)
    assert torch.isfinite(plain.bound).all() and plain.status.tolist() == [0, 0, 0]
    applied = 0
    for name in (("C",) if form == "lazy_conj" else tuple(t)):
        v = P.present(form, t[name])
        assert v is not None, (form, name)
        applied += 1
        got = call({**t, name: v})
        assert all(P.same_bits(g, p) for g, p in zip(got, plain)), (form, name)
        assert torch.equal(v.detach().resolve_conj().resolve_neg(), t[name]), (form, name)     # the input still holds its value
    assert applied


# ---- (e) refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_the_next_call_works():
    c = CC.case("L3_10x10")
    tau, f, C = dev(c.tau), dev(c.f), dev(c.C)
    wide = torch.zeros(2, 17, device=DEV)
    bad = [
        (ValueError, lambda: metrics.crb(tau, f, C, c.grid)),
        (ValueError, lambda: metrics.crb(tau, f, C, c.grid, snr_db=1.0, noise_var=1.0)),
        (ValueError, lambda: metrics.crb(wide, wide, wide.to(torch.complex64), c.grid, snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau[:0], f[:0], C[:0], c.grid, snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau, f, C, (0, 4), snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau, f, C, (4,), snr_db=1.0)),
        (_lib.AdmmNetError, lambda: metrics.crb(tau, f, C, (59, 59), snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau, f, C.real, c.grid, snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau, f[:, :2], C, c.grid, snr_db=1.0)),
        (ValueError, lambda: metrics.crb(tau, f, C, c.grid, snr_db=torch.zeros(4, device=DEV))),
        (TypeError, lambda: metrics.crb(tau, f, C, c.grid, snr_db="loud")),
        (ValueError, lambda: metrics.crb(tau, f, C, c.grid, snr_db=1.0, L_true=torch.ones(3, device=DEV))),
        (ValueError, lambda: metrics.crb(tau, f, C, c.grid, snr_db=1.0, match=torch.zeros(3, 2, dtype=torch.int32, device=DEV))),
        (_lib.AdmmNetError, lambda: metrics.crb(tau, f, C, c.grid, snr_db=1.0, match=torch.zeros(3, 3, dtype=torch.int32))),
    ]
    torch.cuda.synchronize()
    for err, call in bad:
        with pytest.raises(err):
            call()
    assert b"crb" in _lib.load().admmnet_last_error()
    bound, _, status = host(run(c))
    CC.compare(c.name, bound, status, "after the refusals")


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    c = CC.case("L3_10x10")
    args = (dev(c.tau), dev(c.f), dev(c.C), c.grid)
    L, match, snr = dev(np.array([3, 2, 0])), torch.zeros(3, 3, dtype=torch.int32, device=DEV), dev(np.full(3, 15.0))
    metrics.crb(*args, snr_db=15.0)                       # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = metrics.crb(*args, snr_db=snr, L_true=L, match=match)
        q = metrics.crb(*args, noise_var=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert r.totals[6].item() == 5 and q.status.tolist() == [0, 0, 0]


# ---- (f) the harness -----------------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"snr", "method", "grid", "layers", "signals", "targets", "cutoff", "pd", "false_per_signal", "rmse_tau", "rmse_f",
               "gospa", "hits", "misses", "false_alarms"}
ADDED_KEYS = {"crb_tau", "crb_f", "rmse_over_crb_tau", "rmse_over_crb_f"}


def test_evaluate_snr_with_and_without_the_bound():
    kw = dict(grid=(4, 6), layers=2, snrs=(25.0,), signals=64, targets=3, baseline="classical", device=DEV)
    without = list(harness.evaluate_snr(**kw))
    lines = list(harness.evaluate_snr(**kw, crb=True))
    assert [l["method"] for l in lines] == ["net", "classical"] == [l["method"] for l in without]
    for plain, line in zip(without, lines):
        print(line)
        assert set(plain) == PARENT_KEYS and set(line) == PARENT_KEYS | ADDED_KEYS
        assert {k: line[k] for k in plain} == plain
        assert line["hits"] > 0 and all(np.isfinite(line[k]) and line[k] > 0 for k in ADDED_KEYS), line
        assert np.isclose(line["rmse_over_crb_tau"], line["rmse_tau"] / line["crb_tau"], rtol=1e-15)
