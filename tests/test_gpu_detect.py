"""GPU: the CFAR detector kernel (csrc/cfar.hip, ``detect.cfar_targets``) against its float64 host statement ``detect.cfar_host``.

Every case of tests/detect_cases.py under the rules of the host model (decisions exactly, numbers within 8 times what the host
model shows); bits (twice, B = 1 / 7 / 2500, neighbours, the input forms of tests/presentations.py); ``return_map``; the Monte
Carlo at B = 2000 with and without targets; the hand-over to ``refine_targets`` and ``select_refined``; no host read; the
refusals; ``harness.evaluate_snr(baseline="periodogram")``.  Shapes: the table's (Le = 1, 6, 16, both axes down to length 1,
315 and 4096 cells above one pass of the workgroup, the largest grid D = 3406).
"""
import numpy as np
import pytest
import torch

from admm_net_amd import _lib, detect, harness, order, refine, synth

import detect_cases as DC
import presentations as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("rows", "n_det", "n_over", "level", "state", "map")


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(c, **kw):
    return detect.cfar_targets(dev(c.y), dev(c.b), c.grid, **{**c.kw, **dict(noise_var=dev(c.noise_var), symbols=dev(c.symbols),
                                                                            psk=DC.PSK, return_map=True), **kw})


def host(r):
    return tuple(t.cpu().numpy() for t in (r.rows, r.n_det, r.n_over, r.level, r.state, r.map))


# ---- (a) the case table, in one pass --------------------------------------------------------------------------------------------------
def test_the_case_table_against_cfar_host():
    worst = {}
    for c in DC.cases():
        r = run(c)
        worst[c.name] = DC.compare(c.name, *host(r), "kernel")
        states = [q.state for q in DC.reference(c.name)]
        assert r.status.tolist() == [states.count(detect.NONFINITE), states.count(detect.OUTSIDE)], c.name
        assert torch.equal(r.n_est, r.n_det.clamp(0, c.kw["top"])) and r.n_est.dtype == torch.int32
    print("worst (map / largest cell, level) against the mirror:", {k: (float(f"{a:.2g}"), float(f"{b:.2g}")) for k, (a, b) in worst.items()})
    print("the largest:", max(a for a, _ in worst.values()), max(b for _, b in worst.values()), "allowed:", DC.MAP_TOL, DC.LEVEL_TOL)


# ---- (b) bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 2500])
def test_bits_do_not_depend_on_the_call_the_place_or_the_batch(B):
    c = DC.case("os_8x8_r2")
    pick = np.arange(B) % len(c.y)
    y, b = dev(c.y[pick]), dev(c.b[pick])
    kw = {**c.kw, "return_map": True}
    first = detect.cfar_targets(y, b, c.grid, **kw)
    second = detect.cfar_targets(y, b, c.grid, **kw)
    assert all(P.same_bits(u, v) for u, v in zip(first, second))
    alone = [detect.cfar_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), c.grid, **kw) for i in range(len(c.y))]
    for row in sorted({0, B // 2, B - 1}):
        for name in FIELDS:
            assert P.same_bits(getattr(first, name)[row], getattr(alone[row % len(c.y)], name)[0]), (row, name)
    assert first.status.tolist() == [0, 0]


def test_a_scene_does_not_depend_on_its_neighbours():
    """Beside a scene with a NaN and beside one with more detections than rows."""
    c, many = DC.case("ca_8x8_r2"), DC.case("noise_many_over")
    kw = {**c.kw, "top": 6, "return_map": True}
    alone = [detect.cfar_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), c.grid, **kw) for i in range(2)]
    y = np.stack([c.y[1], c.y[0], many.y[0], c.y[0], c.y[1]])
    b = np.stack([c.b[1], c.b[0], many.b[0], c.b[0], c.b[1]])
    y[1, 7] = np.inf
    r = detect.cfar_targets(dev(y), dev(b), c.grid, **{**kw, "pfa": many.kw["pfa"]})
    quiet = detect.cfar_targets(dev(y), dev(b), c.grid, **kw)
    assert r.state.tolist() == [0, detect.NONFINITE, 0, 0, 0] and r.n_det[2].item() > 6 and r.status.tolist() == [1, 0]
    assert torch.isnan(quiet.rows[1]).all() and torch.isnan(quiet.map[1]).all() and quiet.n_det[1].item() == 0
    for row, scene in ((0, 1), (3, 0), (4, 1)):
        for name in FIELDS:
            assert P.same_bits(getattr(quiet, name)[row], getattr(alone[scene], name)[0]), (row, scene, name)
    loud = [detect.cfar_targets(dev(c.y[i:i + 1]), dev(c.b[i:i + 1]), c.grid, **{**kw, "pfa": many.kw["pfa"]}) for i in range(2)]
    for row, scene in ((0, 1), (3, 0), (4, 1)):
        for name in FIELDS:
            assert P.same_bits(getattr(r, name)[row], getattr(loud[scene], name)[0]), (row, scene, name)


@pytest.mark.parametrize("form", ["sliced", "permuted", "expanded", "offset", "neg_view", "lazy_conj", "wide", "leaf"])
def test_every_input_form_gives_the_plain_bits(form):
    if form in P.ABSENT:
        pytest.fail(f"torch lacks what the form {form} needs")
    c = DC.case("symbols_given")
    t = dict(y=dev(c.y[[0, 0, 0]]), b=dev(c.b[[0, 0, 0]]), symbols=dev(np.ascontiguousarray(c.symbols[[0, 0, 0]])),
             noise_var=dev(np.array([0.05, 0.07, 0.05])))
    if form == "expanded":
        t = {k: P.constant_along0(v) for k, v in t.items()}
    call = lambda t: detect.cfar_targets(t["y"], t["b"], c.grid, top=6, oversample=2, method="known", pfa=1e-3,  # noqa: E731
                                         noise_var=t["noise_var"], symbols=t["symbols"], return_map=True)
    plain = call(t)
    assert (plain.state == 0).all() and (plain.n_det > 0).all()
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
@pytest.mark.parametrize("name", ["os_5x7_r3", "ca_16x16_r4", "known_13x262_r1", "noise_many_over"])
def test_the_rows_are_cells_of_the_returned_map(name):
    c = DC.case(name)
    with_map, without = run(c), run(c, return_map=False)
    assert without.map is None and all(P.same_bits(u, v) for u, v in zip(with_map[:5], without[:5]))
    nf, nt = c.cells
    assert with_map.map.shape == (len(c.y), nf, nt) and with_map.map.dtype == torch.float64
    rows, pmap = with_map.rows.cpu().numpy(), with_map.map.cpu().numpy()
    for i in range(len(c.y)):
        n = min(int(with_map.n_det[i]), c.kw["top"])
        assert n > 0
        for l in range(n):
            j, k = round((rows[i, l, 1] + 0.5) * nf), round(rows[i, l, 0] * nt)
            assert rows[i, l, 2] == pmap[i, j, k] and rows[i, l, 0] == k / nt and rows[i, l, 1] == j / nf - 0.5
            around = [pmap[i, (j + dj) % nf, (k + dk) % nt] for dj in (-1, 0, 1) for dk in (-1, 0, 1)]
            assert pmap[i, j, k] == max(around)
        assert np.all(np.diff(rows[i, :n, 2]) <= 0)


# ---- (d) Monte Carlo --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targets", [False, True])
@pytest.mark.parametrize("method", ["known", "ca", "os"])
def test_monte_carlo_against_the_mirror(method, targets):
    """8 x 8, r = 2, B = 2000: noise only, and scenes of ``make_scenes_device(targets=(1, 3))`` at 15 dB.  ``n_over`` and ``n_det``
    equal the mirror's on every scene that holds the margin; at most 1 % of the scenes may be left out."""
    B = DC.MC_DRAWS
    if targets:
        y, b, _, truth = synth.make_scenes_device(B, 8, 8, targets=(1, 3), seed=31, snr_range=(15.0, 15.0), device=DEV)
        noise = truth["noise_var"]
    else:
        y0, b0, noise0 = DC.monte_carlo(False)
        y, b, noise = dev(y0), dev(b0), dev(noise0)
    r = detect.cfar_targets(y, b, DC.MC_GRID, top=6, oversample=DC.MC_R, method=method, pfa=DC.MC_PFA,
                            noise_var=noise if method == "known" else None)
    n_over, n_det, margin = DC.mc_host(y.cpu().numpy(), b.cpu().numpy(), noise.cpu().numpy(), method)
    held = margin > DC.MARGIN
    print(f"{method}, targets={targets}: {int((~held).sum())} of {B} scenes left out; mean n_det {n_det.mean():.3f}, mean n_over "
          f"{n_over.mean():.3f}")
    assert (~held).mean() <= DC.MC_LEFT_OUT
    assert np.array_equal(r.n_over.cpu().numpy()[held], n_over[held]) and np.array_equal(r.n_det.cpu().numpy()[held], n_det[held])
    assert (r.state == 0).all() and r.status.tolist() == [0, 0]


# ---- (e) the hand-over ------------------------------------------------------------------------------------------------------------------
def test_rows_and_n_est_go_to_the_refinement_and_the_selection_as_they_are():
    c = DC.case("known_8x8_r2")
    y, b = dev(np.concatenate([c.y, DC.case("more_than_Le").y])), dev(np.concatenate([c.b, DC.case("more_than_Le").b]))
    r = detect.cfar_targets(y, b, (8, 8), top=6, oversample=2, pfa=1e-3)
    n = r.n_est
    assert n.tolist() == [min(v, 6) for v in r.n_det.tolist()] and (n > 0).all()
    by_hand = r.rows.clone()
    slot = torch.arange(6, device=DEV)[None, :]
    assert torch.equal(torch.isnan(by_hand[:, :, 0]), slot >= n[:, None])
    fit = refine.refine_targets(y, b, r.rows, (8, 8), n_est=n)
    fit_hand = refine.refine_targets(y, b, by_hand, (8, 8), n_est=torch.tensor(n.tolist(), dtype=torch.int32, device=DEV))
    assert all(P.same_bits(u, v) for u, v in zip(fit, fit_hand))
    sel, _ = order.select_refined(y, b, r.rows, (8, 8), n_cand=n)
    sel_hand, _ = order.select_refined(y, b, by_hand, (8, 8))            # the rows beyond n_est are NaN: absent either way
    assert all(P.same_bits(u, v) for u, v in zip(sel, sel_hand)) and (sel.state == 0).all()
    assert (sel.n_sel <= n).all()
    first = order.select_targets(y, b, r.rows, (8, 8), n_cand=n)
    assert torch.equal(first.ranked, n)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_read():
    c = DC.case("symbols_given")
    y, b, sym = dev(c.y), dev(c.b), dev(c.symbols)
    noise = dev(np.array([0.05, 0.05, 0.05]))
    detect.cfar_targets(y, b, c.grid, top=6, oversample=2)               # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ca = detect.cfar_targets(y, b, c.grid, top=6, oversample=2, symbols=sym)
        osr = detect.cfar_targets(y, b, c.grid, top=6, oversample=2, method="os", rank=7, symbols=sym, return_map=True)
        known = detect.cfar_targets(y, b, c.grid, top=6, oversample=2, method="known", noise_var=noise, symbols=sym)
        n = known.n_est
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ca.state.tolist() == osr.state.tolist() == known.state.tolist() == [0, 4, 4] and n.tolist()[1:] == [0, 0]


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_the_next_call_works():
    c = DC.case("ca_8x8_r2")
    y, b = dev(c.y), dev(c.b)
    lib = _lib.load()
    grid, r = DC.LARGEST
    assert lib.admmnet_cfar_lds_bytes(grid[0], grid[1], r) == detect.lds_bytes(grid, r) <= 160 * 1024
    assert lib.admmnet_cfar_lds_bytes(grid[0], grid[1], r + 1) == -1 and lib.admmnet_cfar_lds_bytes(25, 25, 4) == -1
    assert lib.admmnet_cfar_lds_bytes(8, 8, 9) == -1 and lib.admmnet_cfar_lds_bytes(0, 8, 1) == -1
    for g, rr in (((8, 8), 2), ((16, 16), 4), ((5, 7), 3), ((1, 12), 2), ((24, 24), 4)):
        assert lib.admmnet_cfar_lds_bytes(g[0], g[1], rr) == detect.lds_bytes(g, rr)
    big = torch.ones(1, 625, dtype=torch.complex64, device=DEV)
    bad = [
        (ValueError, lambda: detect.cfar_targets(big, big, (25, 25), oversample=4)),                    # past the LDS
        (ValueError, lambda: detect.cfar_targets(y, b, (8, 8), oversample=9)),
        (ValueError, lambda: detect.cfar_targets(y, b, (8, 8), guard=1, train=3)),
        (ValueError, lambda: detect.cfar_targets(y, b, (8, 4))),
        (ValueError, lambda: detect.cfar_targets(y[:0], b[:0], (8, 8))),
        (ValueError, lambda: detect.cfar_targets(y, b[:1], (8, 8))),
        (ValueError, lambda: detect.cfar_targets(y, b, (8, 8), method="known", noise_var=torch.ones(3, device=DEV))),
        (ValueError, lambda: detect.cfar_targets(y, b, (8, 8), symbols=torch.zeros(2, 64, device=DEV))),
        (TypeError, lambda: detect.cfar_targets(c.y, b, (8, 8))),
        (_lib.AdmmNetError, lambda: detect.cfar_targets(y.cpu(), b, (8, 8))),
    ]
    torch.cuda.synchronize()
    for err, call in bad:
        with pytest.raises(err):
            call()
    # the entry itself refuses what the Python layer would: before a launch, with a message
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rows, counts = torch.zeros(2, 6, 3, dtype=torch.float64, device=DEV), torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    info, status = torch.zeros(2, 2, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    entry = lambda Nb=8, Nd=8, r=2, Le=6, method=1, guard=1, train=2, rank=30, alpha=9.0, noise=None: lib.admmnet_cfar_f64(  # noqa: E731
        Nb, Nd, r, Le, 2, p(y), p(b), None, 4, 0.785, method, guard, train, rank, alpha, p(noise), p(rows), p(counts), p(info), None,
        p(status), None)
    for kw in (dict(r=0), dict(r=9), dict(Le=0), dict(Le=17), dict(method=3), dict(guard=-1), dict(train=0), dict(guard=2, train=2),
               dict(guard=5, train=4), dict(method=2, rank=0), dict(method=2, rank=41), dict(alpha=0.0), dict(alpha=float("nan")),
               dict(method=0), dict(noise=info), dict(Nb=25, Nd=25, r=4)):
        assert entry(**kw) != 0, kw
        assert b"cfar" in lib.admmnet_last_error()
    torch.cuda.synchronize()
    assert (rows == 0).all() and (counts == 0).all()
    DC.compare(c.name, *host(run(c)), "after the refusals")


def test_outputs_given_as_views_are_refused_with_nothing_written():
    c = DC.case("ca_8x8_r2")
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
def test_evaluate_snr_with_and_without_the_periodogram():
    kw = dict(grid=(8, 8), layers=2, snrs=(15.0,), signals=64, device=DEV)
    without = list(harness.evaluate_snr(**kw, order=6, refine="given"))
    lines = list(harness.evaluate_snr(**kw, baseline="periodogram", order=6, refine="given"))
    assert [l["method"] for l in lines] == ["net", "net+refine", "net+order", "periodogram", "periodogram+refine", "periodogram+order"]
    assert [l for l in lines if not l["method"].startswith("periodogram")] == without          # bit-equal: the same numbers
    for line in lines[3:]:
        print(line)
        assert set(line) == set(without[0]) and line["hits"] > 0
    varied = dict(**kw, targets_min=1, crb=True)
    without = list(harness.evaluate_snr(**varied, order=6, refine="given"))
    for cfar in (("ca", 1e-4), ("os", 1e-3), ("known", 1e-4)):
        lines = list(harness.evaluate_snr(**varied, baseline="periodogram", cfar=cfar, order=6, refine="given"))
        assert [l for l in lines if not l["method"].startswith("periodogram")] == without
        new = [l for l in lines if l["method"].startswith("periodogram")]
        assert [l["method"] for l in new] == ["periodogram", "periodogram+refine", "periodogram+order"]
        for line in new:
            print(cfar, line)
            assert set(line) == set(without[2]) and line["hits"] > 0                           # the keys of a +order line
            assert abs(line["order_under"] + line["order_exact"] + line["order_over"] - 1.0) < 1e-12
    both = list(harness.evaluate_snr(**kw, baseline="periodogram"))
    assert [l["method"] for l in both] == ["net", "periodogram"]
    with pytest.raises(ValueError):
        next(harness.evaluate_snr(**kw, baseline="periodogram", cfar=("known", 1e-4)))
