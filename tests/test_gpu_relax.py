"""GPU: successive cancellation on the periodogram (csrc/cfar_relax.hip, ``detect.cfar_relax``) against its float64 host statement
``detect.cfar_relax_host``.

Every case of tests/relax_cases.py under the rules of the host model (decisions exactly, numbers within 8 times what the host model
shows); bits (twice, B = 1 / 7 / 2500, neighbours); on-grid cancellation against ``cfar_targets``, the independent code path; the
Monte Carlo at B = 2000 with and without targets; the hand-over to ``refine_targets`` and ``select_refined``; no host read; the
refusals; ``harness.evaluate_snr(cancel=...)``.
"""
import numpy as np
import pytest
import torch

from admm_net_amd import _lib, detect, harness, order, refine, synth

import detect_cases as DC
import presentations as P
import relax_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("rows", "amp", "n_det", "more", "maps", "level", "resid", "state", "map")


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(c, **kw):
    return detect.cfar_relax(dev(c.y), dev(c.b), c.grid, **{**c.kw, **dict(noise_var=dev(c.noise_var), symbols=dev(c.symbols),
                                                                          psk=RC.PSK, return_map=True), **kw})


def host(r):
    return tuple(getattr(r, k).cpu().numpy() for k in FIELDS)


# ---- (a) the case table, in one pass --------------------------------------------------------------------------------------------------
def test_the_case_table_against_cfar_relax_host():
    worst = {}
    for c in RC.cases():
        r = run(c)
        worst[c.name] = RC.compare(c.name, *host(r), "kernel")
        states = [q.state for q in RC.reference(c.name)]
        assert r.status.tolist() == [states.count(detect.NONFINITE), states.count(detect.OUTSIDE)], c.name
        assert torch.equal(r.n_est, r.n_det) and r.n_est.dtype == torch.int32 and r.amp.dtype == torch.complex128
    print("worst (point in resolution cells, power / E, amp / sqrt(E / D)) against the mirror:",
          {k: tuple(float(f"{a:.2g}") for a in v) for k, v in worst.items()})
    print("the largest:", tuple(max(v[k] for v in worst.values()) for k in range(3)), "allowed:", (RC.POINT_TOL, RC.POWER_TOL, RC.AMP_TOL))


# ---- (b) bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 2500])
def test_bits_do_not_depend_on_the_call_the_place_or_the_batch(B):
    c = RC.case("os_8x8_r2")
    pick = np.arange(B) % len(c.y)
    y, b = dev(c.y[pick]), dev(c.b[pick])
    kw = {**c.kw, "return_map": True}
    first = detect.cfar_relax(y, b, c.grid, **kw)
    second = detect.cfar_relax(y, b, c.grid, **kw)
    assert all(P.same_bits(u, v) for u, v in zip(first, second))
    alone = [detect.cfar_relax(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), c.grid, **kw) for i in range(len(c.y))]
    for row in sorted({0, B // 2, B - 1}):
        for name in FIELDS:
            assert P.same_bits(getattr(first, name)[row], getattr(alone[row % len(c.y)], name)[0]), (row, name)
    assert first.status.tolist() == [0, 0] and (first.n_det > 0).all()


def test_a_scene_does_not_depend_on_its_neighbours():
    """Beside a scene with a NaN and beside one that ends with ``more = 1``."""
    c, many = RC.case("ca_8x8_r2"), RC.case("masked_centre")
    kw = {**c.kw, "top": 6, "return_map": True}
    alone = [detect.cfar_relax(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), c.grid, **kw) for i in range(2)]
    y = np.stack([c.y[1], c.y[0], many.y[0], c.y[0], c.y[1]])
    b = np.stack([c.b[1], c.b[0], many.b[0], c.b[0], c.b[1]])
    y[1, 7] = np.inf
    r = detect.cfar_relax(dev(y), dev(b), c.grid, **kw)
    assert r.state.tolist() == [0, detect.NONFINITE, 0, 0, 0] and r.more.tolist() == [0, 0, 1, 0, 0] and r.status.tolist() == [1, 0]
    assert r.n_det[2].item() == 6 and r.maps[2].item() == 7
    assert torch.isnan(r.rows[1]).all() and torch.isnan(r.map[1]).all() and r.n_det[1].item() == 0 and r.maps[1].item() == 0
    for row, scene in ((0, 1), (3, 0), (4, 1)):
        for name in FIELDS:
            assert P.same_bits(getattr(r, name)[row], getattr(alone[scene], name)[0]), (row, scene, name)


# ---- (c) the independent code path: on-grid cancellation against cfar_targets -----------------------------------------------------------
def test_on_grid_cancellation_is_cfar_targets_bit_for_bit():
    """``known``, ``iters = 0``, ``sweeps = 0``, ``top = 1``: the first target is ``cfar_targets``' highest detection -- the row
    (tau, f, height) bit for bit; and the map of a scene without a detection is ``cfar_targets``' map bit for bit."""
    for name in ("known_8x8_r2", "known_5x7_r3", "Le_1"):
        c = RC.case(name)
        kw = dict(top=1, oversample=c.kw["oversample"], method="known", pfa=c.kw["pfa"], noise_var=dev(c.noise_var))
        plain = detect.cfar_targets(dev(c.y), dev(c.b), c.grid, **kw)
        got = detect.cfar_relax(dev(c.y), dev(c.b), c.grid, iters=0, sweeps=0, **kw)
        assert (plain.n_det > 0).all() and (got.n_det == 1).all()
        assert P.same_bits(got.rows, plain.rows), (name, got.rows, plain.rows)
    c = RC.case("no_detection")
    kw = dict(top=6, oversample=2, method="known", pfa=c.kw["pfa"], noise_var=dev(c.noise_var), return_map=True)
    plain = detect.cfar_targets(dev(c.y), dev(c.b), c.grid, **kw)
    for settings in (dict(iters=0, sweeps=0), dict()):
        got = detect.cfar_relax(dev(c.y), dev(c.b), c.grid, **kw, **settings)
        assert (got.n_det == 0).all() and (got.maps == 1).all() and P.same_bits(got.map, plain.map)
        assert P.same_bits(got.level, plain.level) and torch.isnan(got.rows).all()
    # round 0's map under ca too: a scene where nothing is over
    c = RC.case("ca_12x1_r2")
    kw = {k: v for k, v in c.kw.items() if k not in ("iters", "sweeps")}
    plain, got = detect.cfar_targets(dev(c.y), dev(c.b), c.grid, **kw, return_map=True), run(c)
    assert (got.n_det == 0).all() and P.same_bits(got.map, plain.map) and P.same_bits(got.level, plain.level)


# ---- (d) Monte Carlo --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targets", [False, True])
@pytest.mark.parametrize("method", ["known", "ca", "os"])
def test_monte_carlo_against_the_mirror(method, targets):
    """8 x 8, r = 2, B = 2000: noise only, and scenes of ``make_scenes_device(targets=(1, 3))`` at 15 dB.  ``n_det``, ``more`` and
    ``maps`` equal the mirror's on every scene that holds the margin; at most 1 % of the scenes may be left out."""
    B = RC.MC_DRAWS
    if targets:
        y, b, _, truth = synth.make_scenes_device(B, 8, 8, targets=(1, 3), seed=31, snr_range=(15.0, 15.0), device=DEV)
        noise = truth["noise_var"]
    else:
        y0, b0, noise0 = DC.monte_carlo(False)
        y, b, noise = dev(y0), dev(b0), dev(noise0)
    r = detect.cfar_relax(y, b, RC.MC_GRID, top=6, oversample=RC.MC_R, method=method, pfa=RC.MC_PFA,
                          noise_var=noise if method == "known" else None)
    n_det, more, maps, margin = RC.mc_host(y.cpu().numpy(), b.cpu().numpy(), noise.cpu().numpy(), method)
    held = margin > RC.MARGIN
    print(f"{method}, targets={targets}: {int((~held).sum())} of {B} scenes left out; mean n_det {n_det.mean():.3f}, mean maps "
          f"{maps.mean():.3f}, more in {int(more.sum())}; least margin {margin.min():.2g}")
    assert (~held).mean() <= RC.MC_LEFT_OUT
    for got, want in ((r.n_det, n_det), (r.more, more), (r.maps, maps)):
        assert np.array_equal(got.cpu().numpy()[held], want[held])
    assert (r.state == 0).all() and r.status.tolist() == [0, 0]


# ---- (e) the hand-over ------------------------------------------------------------------------------------------------------------------
def test_rows_and_n_est_go_to_the_refinement_and_the_selection_as_they_are():
    c = RC.case("known_8x8_r2")
    y, b = dev(np.concatenate([c.y, RC.case("more_than_Le").y])), dev(np.concatenate([c.b, RC.case("more_than_Le").b]))
    r = detect.cfar_relax(y, b, (8, 8), top=6, oversample=2, pfa=1e-3)
    n = r.n_est
    assert n.tolist() == r.n_det.tolist() and (n > 0).all()
    by_hand = r.rows.clone()
    slot = torch.arange(6, device=DEV)[None, :]
    assert torch.equal(torch.isnan(by_hand[:, :, 0]), slot >= n[:, None])
    fit = refine.refine_targets(y, b, r.rows, (8, 8), n_est=n)
    fit_hand = refine.refine_targets(y, b, by_hand, (8, 8), n_est=torch.tensor(n.tolist(), dtype=torch.int32, device=DEV))
    assert all(P.same_bits(u, v) for u, v in zip(fit, fit_hand)) and (fit.state != refine.OUTSIDE).all()
    sel, _ = order.select_refined(y, b, r.rows, (8, 8), n_cand=n)
    sel_hand, _ = order.select_refined(y, b, by_hand, (8, 8))            # the rows beyond n_est are NaN: absent either way
    assert all(P.same_bits(u, v) for u, v in zip(sel, sel_hand)) and (sel.state == 0).all()
    assert (sel.n_sel <= n).all()


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    c = RC.case("symbols_given")
    y, b, sym = dev(c.y), dev(c.b), dev(c.symbols)
    noise = dev(np.array([0.05, 0.05, 0.05]))
    detect.cfar_relax(y, b, c.grid, top=6, oversample=2)                 # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ca = detect.cfar_relax(y, b, c.grid, top=6, oversample=2, symbols=sym)
        osr = detect.cfar_relax(y, b, c.grid, top=6, oversample=2, method="os", rank=7, symbols=sym, return_map=True)
        known = detect.cfar_relax(y, b, c.grid, top=6, oversample=2, method="known", noise_var=noise, symbols=sym)
        n = known.n_est
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ca.state.tolist() == osr.state.tolist() == known.state.tolist() == [0, 4, 4] and n.tolist()[1:] == [0, 0]


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_the_next_call_works():
    c = RC.case("ca_8x8_r2")
    y, b = dev(c.y), dev(c.b)
    lib = _lib.load()
    assert lib.admmnet_cfar_relax_lds_bytes(13, 262, 1) == detect.relax_lds_bytes((13, 262), 1) <= 160 * 1024
    assert lib.admmnet_cfar_relax_lds_bytes(13, 262, 2) == -1 and lib.admmnet_cfar_relax_lds_bytes(8, 8, 9) == -1
    assert lib.admmnet_cfar_relax_lds_bytes(0, 8, 1) == -1
    for g, rr in (((8, 8), 2), ((16, 16), 4), ((5, 7), 3), ((1, 12), 2), ((24, 24), 4)):
        assert lib.admmnet_cfar_relax_lds_bytes(g[0], g[1], rr) == detect.relax_lds_bytes(g, rr)
    big = torch.ones(1, 625, dtype=torch.complex64, device=DEV)
    bad = [
        (ValueError, lambda: detect.cfar_relax(big, big, (25, 25), oversample=4)),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), oversample=9)),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), guard=1, train=3)),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), iters=17)),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), sweeps=9)),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 4))),
        (ValueError, lambda: detect.cfar_relax(y[:0], b[:0], (8, 8))),
        (ValueError, lambda: detect.cfar_relax(y, b[:1], (8, 8))),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), method="known", noise_var=torch.ones(3, device=DEV))),
        (ValueError, lambda: detect.cfar_relax(y, b, (8, 8), symbols=torch.zeros(2, 64, device=DEV))),
        (TypeError, lambda: detect.cfar_relax(c.y, b, (8, 8))),
        (_lib.AdmmNetError, lambda: detect.cfar_relax(y.cpu(), b, (8, 8))),
    ]
    torch.cuda.synchronize()
    for err, call in bad:
        with pytest.raises(err):
            call()
    # the entry itself refuses what the Python layer would: before a launch, with a message
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rows, amp = torch.zeros(2, 6, 3, dtype=torch.float64, device=DEV), torch.zeros(2, 6, dtype=torch.complex128, device=DEV)
    counts = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    info, status = torch.zeros(2, 3, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    entry = lambda Nb=8, Nd=8, r=2, Le=6, method=1, guard=1, train=2, rank=30, alpha=9.0, noise=None, iters=3, sweeps=2, out=amp: (  # noqa: E731
        lib.admmnet_cfar_relax_f64(Nb, Nd, r, Le, 2, p(y), p(b), None, 4, 0.785, method, guard, train, rank, alpha, p(noise), iters, sweeps,
                                   p(rows), p(out), p(counts), p(info), None, p(status), None))
    for kw in (dict(r=0), dict(r=9), dict(Le=0), dict(Le=17), dict(method=3), dict(guard=-1), dict(train=0), dict(guard=2, train=2),
               dict(guard=5, train=4), dict(method=2, rank=0), dict(method=2, rank=41), dict(alpha=0.0), dict(alpha=float("nan")),
               dict(method=0), dict(noise=info), dict(Nb=30, Nd=30, r=4), dict(iters=-1), dict(iters=17), dict(sweeps=-1),
               dict(sweeps=9), dict(out=None)):
        assert entry(**kw) != 0, kw
        assert b"cfar_relax" in lib.admmnet_last_error()
    torch.cuda.synchronize()
    assert (rows == 0).all() and (counts == 0).all() and (amp == 0).all()
    RC.compare(c.name, *host(run(c)), "after the refusals")


def test_outputs_given_as_views_are_refused_with_nothing_written():
    c = RC.case("ca_8x8_r2")
    plain = run(c)
    rows = torch.full((2, 1, 3), 7.0, dtype=torch.float64, device=DEV)
    given = run(c, out=rows)
    assert given.rows is rows and all(P.same_bits(g, p) for g, p in zip(given, plain))
    for form in P.REFUSAL_FORMS + ("permuted",):
        view = torch.full_like(rows, 7.0).to(torch.float32) if form == "wide" else P.present(form, torch.full_like(rows, 7.0))
        if view is None:
            continue
        before = view.detach().resolve_conj().resolve_neg().clone()
        with pytest.raises(ValueError):
            run(c, out=view)
        torch.cuda.synchronize()
        assert torch.equal(view.detach().resolve_conj().resolve_neg(), before), form
    for out in (rows[:1], rows.cpu(), torch.zeros(2, 2, 3, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            run(c, out=out)
    with pytest.raises(TypeError):
        run(c, out=(rows,))


# ---- (g) through the harness ------------------------------------------------------------------------------------------------------------
def test_evaluate_snr_with_and_without_the_cancellation():
    kw = dict(grid=(8, 8), layers=2, snrs=(15.0,), signals=64, device=DEV, baseline="periodogram")
    without = list(harness.evaluate_snr(**kw, order=6, refine="given"))
    lines = list(harness.evaluate_snr(**kw, order=6, refine="given", cancel=(3, 2)))
    assert [l["method"] for l in lines] == ["net", "net+refine", "net+order", "periodogram", "periodogram+refine", "periodogram+order",
                                            "periodogram+relax", "periodogram+relax+refine"]
    assert [l for l in lines if "+relax" not in l["method"]] == without                        # bit-equal: the same numbers
    for line in lines[6:]:
        print(line)
        assert set(line) == set(without[0]) and line["hits"] > 0
    varied = dict(**kw, targets_min=1, crb=True)
    for cfar in (("ca", 1e-4), ("known", 1e-4)):
        without = list(harness.evaluate_snr(**varied, cfar=cfar))
        lines = list(harness.evaluate_snr(**varied, cfar=cfar, cancel=(3, 2)))
        assert [l["method"] for l in lines] == ["net", "periodogram", "periodogram+relax"] and lines[:2] == without
        print(cfar, lines[2])
        assert set(lines[2]) == set(without[1]) and lines[2]["hits"] > 0                       # the keys of the periodogram line
        assert abs(lines[2]["order_under"] + lines[2]["order_exact"] + lines[2]["order_over"] - 1.0) < 1e-12
    with pytest.raises(ValueError):
        next(harness.evaluate_snr(**{**kw, "baseline": None}, cancel=(3, 2)))
