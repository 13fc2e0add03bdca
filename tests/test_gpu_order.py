"""GPU: the model-order kernel (csrc/order.hip, ``order.select_targets``) against its float64 host statement ``order.select_host``,
and the selection-and-refinement loop ``order.select_refined`` against the same loop on the mirror.

Every case of tests/order_cases.py under the rules of the host model (decisions exactly, numbers within 8 times what the host
model shows); bits (twice, B = 1 / 7 / 2500, neighbours, the input forms of tests/presentations.py); the residual recomputed from
the outputs; the hand-over to ``refine_targets``; the grown candidate; the Monte-Carlo scene at B = 2000; the refusals; no host
read; ``model.estimate_selected`` and ``harness.evaluate_snr(order=)``.  Shapes: the table's (Le = 1, 6, 16, both axes down to
length 1, Nd = 131 and 262 above a wave and above the workgroup, the largest D = 3406).
"""
import numpy as np
import pytest
import torch

from admm_net_amd import _lib, harness, metrics, modules, ops, order, refine

import order_cases as OC
import presentations as P
import refine_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("perm", "n_sel", "rss", "rows_out", "C", "residual", "cost", "noise_var", "ranked", "state")


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(c, **kw):
    return order.select_targets(dev(c.y), dev(c.b), dev(c.rows), c.grid, n_cand=dev(c.n_cand), n_held=dev(c.n_held),
                                symbols=dev(c.symbols), **{**c.kw, **kw})


def host(r):
    info = torch.stack((r.cost, r.noise_var, r.ranked.double(), r.state.double()), dim=1)
    return tuple(t.cpu().numpy() for t in (r.perm, r.n_sel, r.rss, r.rows_out, r.C, r.residual, info))


# ---- (a) the case table, in one pass --------------------------------------------------------------------------------------------------
def test_the_case_table_against_select_host():
    worst = {}
    for c in OC.cases():
        r = run(c)
        worst[c.name] = OC.compare(c.name, *host(r), "kernel")
        states = [q.state for q in OC.reference(c.name)]
        assert r.status.tolist() == [states.count(order.NONFINITE), states.count(order.OUTSIDE)], c.name
    print("worst (rss / RSS_0, C / max |C|) against the mirror:", {k: (float(f"{a:.2g}"), float(f"{b:.2g}")) for k, (a, b) in worst.items()})
    print("the largest:", max(a for a, _ in worst.values()), max(b for _, b in worst.values()), "allowed:", OC.RSS_TOL, OC.C_TOL)


# ---- (b) bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 2500])
def test_bits_do_not_depend_on_the_call_the_place_or_the_batch(B):
    c = OC.case("L3_of_6_8x8")
    pick = np.arange(B) % len(c.y)
    y, b, rows = dev(c.y[pick]), dev(c.b[pick]), dev(c.rows[pick])
    first = order.select_targets(y, b, rows, c.grid)
    second = order.select_targets(y, b, rows, c.grid)
    assert all(P.same_bits(u, v) for u, v in zip(first, second))
    alone = [order.select_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), dev(c.rows[i:i + 1]), c.grid) for i in range(len(c.y))]
    for row in sorted({0, B // 2, B - 1}):
        for name in FIELDS:
            assert P.same_bits(getattr(first, name)[row], getattr(alone[row % len(c.y)], name)[0]), (row, name)
    assert first.status.tolist() == [0, 0]


def test_a_scene_does_not_depend_on_its_neighbours():
    c = OC.case("L3_of_6_8x8")
    alone = [order.select_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), dev(c.rows[i:i + 1]), c.grid) for i in range(3)]
    place = [2, 0, 0, 1, 0]                                 # scenes 2, (NaN in y), (coincident rows), 1, 0
    for neighbour in ("nan", "coincident"):
        y, b, rows = c.y[place].copy(), c.b[place].copy(), c.rows[place].copy()
        if neighbour == "nan":
            y[1, 7] = np.inf
        else:
            rows[2, 1, :2] = rows[2, 0, :2]
        r = order.select_targets(dev(y), dev(b), dev(rows), c.grid)
        assert r.state.tolist() == ([0, order.NONFINITE, 0, 0, 0] if neighbour == "nan" else [0] * 5)
        if neighbour == "coincident":
            assert r.ranked.tolist() == [6, 6, 5, 6, 6] and r.perm[2, 5].item() == 1
        for row, scene in ((0, 2), (3, 1), (4, 0)):
            for name in FIELDS:
                assert P.same_bits(getattr(r, name)[row], getattr(alone[scene], name)[0]), (neighbour, row, scene, name)


@pytest.mark.parametrize("form", ["sliced", "permuted", "expanded", "offset", "neg_view", "lazy_conj", "wide", "leaf"])
def test_every_input_form_gives_the_plain_bits(form):
    if form in P.ABSENT:
        pytest.fail(f"torch lacks what the form {form} needs")
    c = OC.case("symbols_given")
    t = dict(y=dev(c.y), b=dev(c.b), rows=dev(c.rows), symbols=dev(np.ascontiguousarray(c.symbols[[0, 0, 0]])),
             n_cand=dev(np.array([6, 5, 6], dtype=np.int32)), n_held=dev(np.array([0, 1, 2], dtype=np.int32)))
    if form == "expanded":
        t = {k: P.constant_along0(v) for k, v in t.items()}
    call = lambda t: order.select_targets(t["y"], t["b"], t["rows"], c.grid, n_cand=t["n_cand"], n_held=t["n_held"],  # noqa: E731
                                          symbols=t["symbols"])
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


# ---- (c) what the outputs mean -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L3_of_6_8x8", "L5_of_16_16x16", "L3_of_16_13x262", "symbols_given", "n_cand"])
def test_the_residual_is_x_less_the_selected_atoms(name):
    """x - A C recomputed in float64 torch from rows_out, C and n_sel, to the rounding of complex64."""
    c = OC.case(name)
    r = run(c)
    Nb, Nd = c.grid
    y, b = dev(c.y).to(torch.complex128), dev(c.b).to(torch.complex128)
    if c.symbols is None:
        s = b / b.abs()
    else:
        s = dev(refine.psk_points(*OC.PSK))[dev(c.symbols).clamp(0, OC.PSK[0] - 1).long()]
    x = y * s.conj()
    ib, idd = torch.arange(Nb * Nd, device=DEV) // Nd, torch.arange(Nb * Nd, device=DEV) % Nd
    tau, f = r.rows_out[:, :, 0].nan_to_num(0.0, 0.0, 0.0), r.rows_out[:, :, 1].nan_to_num(0.0, 0.0, 0.0)
    A = torch.exp(2j * np.pi * (ib[None, :, None] * f[:, None, :] - idd[None, :, None] * tau[:, None, :]))
    C = torch.where(torch.arange(r.C.shape[1], device=DEV)[None, :] < r.n_sel[:, None], r.C, torch.zeros_like(r.C))
    want = x - (A * C[:, None, :]).sum(dim=2)
    ok = r.state == 0
    assert ok.any()
    top = y.abs().amax(dim=1, keepdim=True)
    assert ((r.residual.to(torch.complex128) - want).abs() <= 2.0 ** -22 * top)[ok].all()
    cost = (want.abs() ** 2).sum(dim=1)
    assert torch.allclose(r.cost[ok], cost[ok], rtol=1e-10, atol=0)          # (k tau is rounded before the exponential: ~1e-13 rad)
    assert torch.isnan(r.residual.real[~ok]).all()


def test_the_selected_rows_go_to_the_refinement_as_they_are():
    """``refine_targets(rows_out, n_est=n_sel)`` = the refinement of the rows permuted by hand, bit for bit."""
    c = OC.case("L3_of_6_8x8")
    r = run(c)
    y, b = dev(c.y), dev(c.b)
    direct = refine.refine_targets(y, b, r.rows_out, c.grid, n_est=r.n_sel)
    perm, n_sel = r.perm.cpu().numpy(), r.n_sel.cpu().numpy()
    by_hand = np.stack([c.rows[i][perm[i]] for i in range(len(c.y))])
    by_hand[:, :, 2] = 0.0                                                      # (the third column is not read)
    want = refine.refine_targets(y, b, dev(by_hand), c.grid, n_est=dev(n_sel.astype(np.int32)))
    assert all(P.same_bits(u, v) for u, v in zip(direct, want))
    assert (direct.state == refine.CONVERGED).all() and (~torch.isnan(direct.rows[:, :, 0])).sum(dim=1).tolist() == n_sel.tolist()


def test_a_grown_candidate_is_the_peak_of_the_residual():
    """One target on the 8 x 8 grid without noise, the only candidate two cells away: the row grown from the residual's highest
    peak lies within one coarse step (a tenth of a cell) of the truth and is selected.  ``peak_top``'s spectrum of the residual
    is the matched filter of the atoms only if the residual is laid out (Nb, Nd) with x = tau -- this pins it."""
    tau, f, C = np.array([0.4130]), np.array([-0.2170]), np.array([0.8 - 0.3j])
    mu = metrics.crb_signal(tau, f, C, (8, 8))
    k = np.random.default_rng(3).integers(0, 4, 64)
    pts = refine.psk_points(*OC.PSK)
    y, b = (mu * pts[k]).astype(np.complex64)[None], pts[k].astype(np.complex64)[None]
    rows = np.array([[[0.61, 0.05, 0.0], [tau[0] + 2.0 / 8, f[0] + 2.0 / 8, 0.0]]])
    plain, _ = order.select_refined(dev(y), dev(b), dev(rows), (8, 8), rounds=0, grow=0)
    sel, fit = order.select_refined(dev(y), dev(b), dev(rows), (8, 8), rounds=0, grow=1)
    assert sel.n_sel.item() >= 1 and sel.state.item() == 0
    got = sel.rows_out[0, 0].cpu().numpy()
    print("grown and refined:", got, "truth:", tau[0], f[0], "cost before and after:", plain.cost.item(), sel.cost.item())
    assert abs(got[0] - tau[0]) * 8 <= 0.1 and abs(got[1] - f[0]) * 8 <= 0.1 and abs(got[2] - abs(C[0])) < 1e-3
    assert sel.cost.item() < 1e-6 * plain.cost.item()
    peak, _ = ops.peak_top(plain.residual, 8, 8, {"xstep": 1 / 80, "ystep": 1 / 80, "iter": 3}, top=1)
    assert abs(peak[0, 0, 0].item() - tau[0]) * 8 <= 0.1 and abs(peak[0, 0, 1].item() - f[0]) * 8 <= 0.1


# ---- (d) the loop --------------------------------------------------------------------------------------------------------------------------
def test_the_loop_on_the_monte_carlo_scene_selects_as_the_mirror_does():
    """B = 2000 draws of the 8 x 8 scene at 15 dB through ``select_refined(rounds=1)``: select, refine, select.  The outcome of
    every scene (right, too many, other) equals the mirror loop's but on scenes below the decision margin: at most 1 % may differ,
    and the mirror alone has the margin on at least 99 %.  Measured: the mirror's shares after the second selection 0.9465 right,
    0.033 too many (after the first 0.833, 0.155); margin held on 100 % of the draws, 0 scenes counted differently."""
    y, b, rows = OC.monte_carlo()
    sel, fit = order.select_refined(dev(y), dev(b), dev(rows), RC.SCENE_GRID, rounds=1)
    n_sel, origin = sel.n_sel.cpu().numpy(), sel.perm.cpu().numpy()
    got = np.array([OC.outcome(n_sel[i], origin[i]) for i in range(len(y))])
    first, second = OC.mirror_loop(OC.MC_DRAWS)
    want, margin = second[0], np.minimum(first[1], second[1])
    held = float((margin > OC.MARGIN).mean())
    differ = int((got != want).sum())
    print(f"shares (right, too many, other): device {OC.shares(got)}, mirror {OC.shares(want)}, mirror after the first selection "
          f"{OC.shares(first[0])}; margin held on {held:.4f} of the draws; {differ} scenes counted differently")
    assert sel.status.tolist() == [0, 0] and fit.status.tolist()[:2] == [0, 0]
    assert held >= 0.99 and differ <= 0.01 * len(y)
    assert all(abs(g - w) <= differ / len(y) + 1e-12 for g, w in zip(OC.shares(got), OC.shares(want)))
    assert OC.shares(got)[0] > OC.shares(first[0])[0] and OC.shares(got)[1] < OC.shares(first[0])[1]


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    """Nothing synchronises across ``select_targets`` and the rounds of ``select_refined``.  A grown round calls ``ops.peak_top``,
    which uploads its two coarse axes -- a copy of constants TO the device, which torch counts as synchronising too: run in
    "warn" mode, every such report comes from that upload in ops.py and none from order.py or refine.py."""
    import warnings
    c = OC.case("symbols_given")
    args = (dev(c.y), dev(c.b), dev(c.rows), c.grid)
    sym, n = dev(c.symbols), dev(np.array([6, 5, 6], dtype=np.int32))
    order.select_refined(*args, rounds=1, grow=1, symbols="psk")        # (the library is loaded, the first calls made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = order.select_targets(*args, n_cand=n, n_held=n - 5, symbols=sym)
        given, _ = order.select_refined(*args, rounds=2)
        psk, fit = order.select_refined(*args, rounds=1, symbols="psk", iters=4)
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            grown, _ = order.select_refined(*args, rounds=1, grow=1, symbols="psk", iters=4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    reports = [w for w in seen if "synchronizing" in str(w.message)]
    print("synchronising calls of a grown round:", [(w.filename.rsplit("/", 1)[-1], w.lineno) for w in reports])
    assert reports and all(w.filename.endswith("ops.py") for w in reports)
    assert r.state.tolist() == [0, 4, 4] and given.state.tolist() == [0, 0, 0] and psk.state.tolist() == [0, 0, 0]
    assert fit.iterations.max().item() <= 4 and grown.state.tolist() == [0, 0, 0]


# ---- (e) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_the_next_call_works():
    c = OC.case("L3_of_6_8x8")
    y, b, rows = dev(c.y), dev(c.b), dev(c.rows)
    wide = torch.zeros(3, 17, 3, dtype=torch.float64, device=DEV)
    skinny = torch.zeros(1, 3406, dtype=torch.complex64, device=DEV)
    ones = torch.ones(3, dtype=torch.int32, device=DEV)
    bad = [
        (ValueError, lambda: order.select_targets(y, b, rows, (8, 4))),
        (ValueError, lambda: order.select_targets(y, b, rows, (8,))),
        (ValueError, lambda: order.select_targets(y, b, rows, (0, 64))),
        (ValueError, lambda: order.select_targets(y, b, wide, c.grid)),
        (ValueError, lambda: order.select_targets(y, b, rows[:, :, :2], c.grid)),
        (ValueError, lambda: order.select_targets(y[:0], b[:0], rows[:0], c.grid)),
        (ValueError, lambda: order.select_targets(y, b[:2], rows, c.grid)),
        (ValueError, lambda: order.select_targets(y.real, b, rows, c.grid)),
        (ValueError, lambda: order.select_targets(y, b, rows.to(torch.complex128), c.grid)),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, psk=(1, 0.0))),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, psk=(4, float("nan")))),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, penalty=-1.0)),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, penalty=float("inf"))),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, max_order=0)),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, max_order=7)),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, n_cand=ones.double())),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, n_held=ones[:2])),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, symbols=torch.zeros(3, 64, device=DEV))),
        (ValueError, lambda: order.select_targets(y, b, rows, c.grid, symbols=torch.zeros(3, 63, dtype=torch.int32, device=DEV))),
        (TypeError, lambda: order.select_targets(c.y, b, rows, c.grid)),
        (_lib.AdmmNetError, lambda: order.select_targets(y.cpu(), b, rows, c.grid)),
        (_lib.AdmmNetError, lambda: order.select_targets(torch.zeros(1, 59 * 59, dtype=torch.complex64, device=DEV),
                                                         torch.zeros(1, 59 * 59, dtype=torch.complex64, device=DEV), rows[:1], (59, 59))),
        (_lib.AdmmNetError, lambda: order.select_targets(skinny, skinny, rows[:1], (1, 3406))),            # the tables of 6 rows
    ]
    torch.cuda.synchronize()
    for err, call in bad:
        with pytest.raises(err):
            call()
    lib = _lib.load()
    assert b"order" in lib.admmnet_last_error()
    assert lib.admmnet_order_lds_bytes(1, 3406, 6) == -1 and lib.admmnet_order_lds_bytes(59, 59, 1) == -1
    assert 0 < lib.admmnet_order_lds_bytes(13, 262, 16) <= 160 * 1024 and 0 < lib.admmnet_order_lds_bytes(1, 3406, 1)
    one = order.select_targets(skinny + 1, skinny + 1, rows[:1, :1], (1, 3406))                              # ... of one row fit
    assert torch.isfinite(one.cost).all() and one.status.tolist() == [0, 0]
    OC.compare(c.name, *host(run(c)), "after the refusals")


def test_outputs_given_as_views_are_refused_with_nothing_written():
    c = OC.case("L3_of_6_8x8")
    plain = run(c)
    rows, C = torch.full((3, 6, 3), 7.0, dtype=torch.float64, device=DEV), torch.full((3, 6), 7.0 + 0j, dtype=torch.complex128, device=DEV)
    given = run(c, out=(rows, C))
    assert given.rows_out is rows and given.C is C and all(P.same_bits(g, p) for g, p in zip(given, plain))
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
    own = dev(c.rows)
    with pytest.raises(ValueError):
        order.select_targets(dev(c.y), dev(c.b), own, c.grid, out=(own, C))


# ---- (f) through the public interface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [modules.PhiEstADMMNet, modules.ADMMNet])
def test_estimate_selected(cls):
    from admm_net_amd import synth
    torch.manual_seed(0)
    net = cls(num_layers=2, M=4, N=6, L=3).eval()
    y, b, sigma, truth = synth.make_batch_device(64, 4, 6, L=3, seed=5, snr_range=(25.0, 25.0), device=DEV)
    _, _, _, counts0, phi0 = net.estimate(y, b, sigma)
    tau, f, amp, C, n_sel, counts, phi, state = net.estimate_selected(y, b, sigma, rounds=1, iters=8)
    assert tau.shape == f.shape == amp.shape == C.shape == (64, 6) and n_sel.shape == state.shape == (64,) and tau.device == y.device
    assert P.same_bits(counts, counts0) and P.same_bits(phi, phi0)
    slot = torch.arange(6, device=DEV)[None, :]
    past = slot >= n_sel[:, None]
    assert torch.equal(torch.isnan(tau), past) and torch.equal(torch.isnan(f), past) and torch.equal(torch.isnan(C.real), past)
    assert C.dtype == torch.complex128 and torch.allclose(amp[~past], C.abs()[~past], rtol=4e-16, atol=0)
    assert (state == 0).all() and ((n_sel >= 0) & (n_sel <= 6)).all()
    rows, _, _ = net._estimate_rows(y, b, sigma, 6)
    direct, _ = order.select_refined(y, b, rows, (4, 6), rounds=1, iters=8)
    assert P.same_bits(direct.n_sel, n_sel) and P.same_bits(direct.C, C)
    on_host = net.estimate_selected(y.cpu(), b.cpu(), sigma.cpu(), rounds=1, iters=8)
    assert all(not t.is_cuda for t in on_host) and P.same_bits(on_host[0], tau.cpu()) and P.same_bits(on_host[4], n_sel.cpu())


def test_evaluate_snr_with_and_without_the_order():
    kw = dict(grid=(4, 6), layers=2, snrs=(25.0,), signals=64, targets=3, baseline="classical", device=DEV, crb=True)
    without = list(harness.evaluate_snr(**kw, refine="given"))
    lines = list(harness.evaluate_snr(**kw, refine="given", order=6))
    assert [l["method"] for l in lines] == ["net", "net+refine", "net+order", "classical", "classical+refine", "classical+order"]
    assert [l for l in lines if not l["method"].endswith("+order")] == without               # bit-equal: the same numbers
    for line in lines:
        print(line)
        assert set(line) == set(without[0]) and line["hits"] > 0
    bare = list(harness.evaluate_snr(**{**kw, "crb": False, "baseline": None}, order=6))
    assert [l["method"] for l in bare] == ["net", "net+order"]
    assert bare[0] == list(harness.evaluate_snr(**{**kw, "crb": False, "baseline": None}))[0]
    with pytest.raises(ValueError):
        list(harness.evaluate_snr(**kw, order=2))
