"""CPU: the table of tests/peak_cases.py is sound, reaches what it names, and rejects mistakes.

Sound: the engine of the table returns the bits of the literal oracle (oracle/peak_search_ref.py) on every case, and the
product's host mirror (admm_net_amd.peak_search) agrees with it -- positions by bits, heights at 1e-12 of the largest.
Reaches: every counter that names a case is non-zero there, the local grids cover 1 x 1 .. 3 x 3, and no decision of any
case is a numerical tie (peak_cases: THE TIE RULE), so tests/test_gpu_peak_cases.py compares every row of every case.
Rejects: fourteen stand-ins, one mistake each, are each refused by a named case or image -- a device kernel with the same
mistake fails the same case."""
import numpy as np
import pytest

import peak_cases as P
from admm_net_amd import peak_search
from oracle import peak_search_ref as PO


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def runs(name):
    c = P.CASES[name]
    return [(s, P.phi_of(name, s), c["xbase"], c["ybase"], c["opts"], *P.oracle_of(name, s)) for s in P.SEEDS]


# ---- 1. sound ---------------------------------------------------------------------------------------------------------------
def test_table_holds_the_cases_of_the_issue():
    assert P.NOISE == 0.05 and len(P.SEEDS) == 2
    geoms = {(c["xbase"], c["ybase"]) for c in P.CASES.values()}
    assert {(6, 5), (7, 4), (17, 3), (16, 3), (1, 12), (12, 1), (2, 2), (1, 1)} <= geoms
    assert {P.CASES[n]["opts"].get("reducefactor") for n in P.CASES if n.startswith("high_edge")} == {0.9, 1.0, 2.0}
    assert P.CASES["deep"]["opts"]["iter"] == 5 and P.CASES["xbase17"]["opts"]["xstep"] == 1 / 68
    for name in P.CASES:
        b = P.batch_of(name)
        assert b.dtype == np.complex64 and b.shape == (2, P.CASES[name]["xbase"] * P.CASES[name]["ybase"])
        assert not np.array_equal(b[0], b[1])


@pytest.mark.parametrize("name", list(P.CASES))
def test_engine_is_the_literal_oracle(name):
    for seed, phi, xb, yb, opts, rows, tr in runs(name):
        lit = PO.alt_peak_search_literal({"phi": phi.astype(np.complex128), "xbase": xb, "ybase": yb}, opts)
        assert same_rows(rows, lit), (name, seed)


@pytest.mark.parametrize("name", list(P.CASES))
def test_host_mirror_equals_the_oracle(name):
    """Positions by bits, heights at 1e-12 of the largest; on the base-1 cases this needs spectrum_grid's exactly constant
    axis (a BLAS product breaks the full-row plateaus of base1_x: 55 and 65 maxima for the oracle's 99)."""
    for seed, phi, xb, yb, opts, rows, tr in runs(name):
        got = peak_search.alt_peak_search({"phi": phi, "xbase": xb, "ybase": yb}, opts)
        assert got.shape == rows.shape, (name, seed, got.shape, rows.shape)
        assert same_rows(got[:, :2], rows[:, :2]), (name, seed)
        if len(rows):
            assert np.abs(got[:, 2] - rows[:, 2]).max() <= 1e-12 * max(rows[:, 2].max(), 1.0)
            assert np.array_equal(got[:, 2] == 0.0, rows[:, 2] == 0.0)


@pytest.mark.parametrize("name", P.BASE1)
def test_mirror_image_is_exactly_constant_along_a_base_1_axis(name):
    c = P.CASES[name]
    ax, ay = peak_search.coarse_axes(c["opts"])
    for seed in P.SEEDS:
        Z = peak_search.spectrum_grid(P.phi_of(name, seed), ax, c["xbase"], ay, c["ybase"])
        lit = P.oracle_of(name, seed)[1].coarse
        assert Z.shape == lit.shape == (len(ay), len(ax))
        if c["xbase"] == 1:
            assert np.array_equal(_bits(Z), _bits(np.broadcast_to(Z[:, :1], Z.shape)))
            assert np.array_equal(_bits(lit), _bits(np.broadcast_to(lit[:, :1], lit.shape)))
        if c["ybase"] == 1:
            assert np.array_equal(_bits(Z), _bits(np.broadcast_to(Z[:1, :], Z.shape)))
            assert np.array_equal(_bits(lit), _bits(np.broadcast_to(lit[:1, :], lit.shape)))
        assert np.abs(Z - lit).max() <= 1e-12 * lit.max()


# ---- 2. reaches -------------------------------------------------------------------------------------------------------------
def test_counters_that_name_a_case_are_non_zero():
    tr = {n: [P.oracle_of(n, s)[1] for s in P.SEEDS] for n in P.CASES}
    for t in tr["corner"]:
        assert t.lower > 0 and t.upper == 0
    for n in ("high_edge_rf0.9", "high_edge_rf1.0", "high_edge_rf2.0"):
        for t in tr[n]:
            assert t.upper > 0 and t.ran > 0
    for t in tr["skipped_round"]:
        assert t.coarse.shape == (1, 19) and t.skipped > 0 and t.ran > 0 and t.late_skips == 0
    for s, t in zip(P.SEEDS, tr["no_round_runs"]):
        rows = P.oracle_of("no_round_runs", s)[0]
        assert t.ran == 0 and t.skipped == 2 * t.maxima and t.maxima >= 2 and not rows[:, 2].any()
    for t in tr["late_skip"]:
        assert t.late_skips > 0 and t.ran > 0                       # a round that ran, then a skipped one
    for s, t in zip(P.SEEDS, tr["late_skip"]):
        assert (P.oracle_of("late_skip", s)[0][:, 2] > 0).all()
    assert tr["xbase17"][0].coarse.shape[1] == 67 and tr["xbase16"][0].coarse.shape[1] == 63
    for t in tr["base1_x"]:
        assert t.maxima % t.coarse.shape[1] == 0 and t.maxima >= 2 * t.coarse.shape[1]      # full-row plateaus
    for t in tr["base1_y"]:
        assert t.maxima % t.coarse.shape[0] == 0 and t.maxima >= 2 * t.coarse.shape[0]      # full-column plateaus
    for t in tr["tiny_1x1"]:
        assert t.maxima == 0                                        # a constant image has no maximum
    for t in tr["tiny_2x2"]:
        assert t.maxima > 0
    for t in tr["deep"]:
        assert t.ran == 5 * t.maxima
    # default-factor cases never clip above: that half of the window needs the high-edge cases
    for n in ("corner", "xbase17", "xbase16", "base1_x", "base1_y", "tiny_2x2", "deep"):
        assert all(t.upper == 0 for t in tr[n]), n
    shapes = set().union(*(t.shapes for ts in tr.values() for t in ts))
    assert {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)} <= shapes


def test_no_decision_of_any_case_is_a_numerical_tie():
    worst = {}
    for name in P.CASES:
        for seed in P.SEEDS:
            t = P.oracle_of(name, seed)[1]
            assert t.tied == 0, (name, seed, t.min_margin / t.eps, t.min_where)
            if t.decisions:
                worst[name] = min(worst.get(name, np.inf), t.min_margin / t.eps)
        assert name == "tiny_1x1" or t.decisions > 0
    print("FIGURES smallest margin in eps:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert min(worst.values()) > 1e3       # the table keeps three decades of room (deep, round 5, is the closest)


def test_ranking_of_two_heights_is_a_tie_in_one_named_pair_only():
    """peak_top orders the refined heights: two heights are either the same bits (0.0 when no round ran, the pixels of one
    plateau on a base-1 axis -- then the list order decides, on the device as in top_rows) or further apart than eps.  The
    one exception is named: high_edge_rf2.0 refines two coarse maxima to one point (peak_cases.ranking_ties)."""
    for name in P.CASES:
        for seed in P.SEEDS:
            rows, t = P.oracle_of(name, seed)
            ties = P.ranking_ties(rows, t.eps)
            if name == "high_edge_rf2.0":
                assert len(ties) == 2 and ties[1] == ties[0] + 1
                pair = peak_search.top_rows(rows, len(rows))[ties]
                assert np.abs(pair[0, :2] - pair[1, :2]).max() < 1e-12 and not same_rows(pair[0, :2], pair[1, :2])
            else:
                assert ties == [], (name, seed)
            if name not in P.BASE1 + ("no_round_runs", "high_edge_rf2.0"):
                assert len(set(rows[:, 2])) == len(rows), (name, seed)
    assert all(len(P.oracle_of("many_maxima", s)[0]) > 256 for s in P.SEEDS)


# ---- 3. rejects -------------------------------------------------------------------------------------------------------------
REJECTED_BY = {   # mistake: the case that names it
    "ay_minus_ystep": "skipped_round",
    "upper_clip_at_max": "high_edge_rf0.9",
    "step_kept_by_skipped_round": "skipped_round",
    "height_reset_by_skipped_round": "late_skip",
    "floor_for_ceil": "deep",
    "points_start_plus_i_step": "corner",
    "last_argmax": "base1_x",
    "reshape_xbase_ybase": "custom_range",
    "min_exchanged": "custom_range",
    "reducefactor_once": "deep",
}


def test_every_search_mistake_has_its_case():
    assert set(REJECTED_BY) == set(P.MISTAKES)


@pytest.mark.parametrize("mistake", list(P.MISTAKES))
def test_search_mistake_is_rejected(mistake):
    name = REJECTED_BY[mistake]
    for seed, phi, xb, yb, opts, rows, tr in runs(name):
        got = P.search(phi, xb, yb, opts, mistake=mistake)
        assert not same_rows(got, rows), (mistake, name, seed)
        # and by the mirror's arithmetic as well: the rejection is no artefact of the literal spectrum
        got = P.search(phi, xb, yb, opts, spectrum=peak_search.spectrum_grid, mistake=mistake)
        assert not same_rows(got[:, :2], rows[:, :2]) or not np.allclose(got[:, 2], rows[:, 2], rtol=1e-9, atol=0)


MAXIMA_STANDINS = {   # name: (stand-in, the image that rejects it)
    "four_connectivity": (lambda im: P.maxima_by_passes(im, connectivity=4)[0], "diagonal_step"),
    "plateau_kept_beside_a_higher_pixel": (lambda im: P.maxima_by_passes(im, spread=False)[0], "snake_9x11_head"),
    "sixteen_passes": (lambda im: P.maxima_by_passes(im, passes=16)[0], "snake_9x11_head"),
}


@pytest.mark.parametrize("name", list(MAXIMA_STANDINS))
def test_maxima_mistake_is_rejected(name):
    fn, image = MAXIMA_STANDINS[name]
    assert not np.array_equal(fn(P.images()[image]), P.image_mask(image))
    assert np.array_equal(P.maxima_by_passes(P.images()[image])[0], P.image_mask(image))   # the stand-in's base is right


def test_top_rows_order_among_equal_heights_is_pinned():
    """no_round_runs leaves every height 0.0: top_rows must keep the list order; the reversed stand-in is rejected."""
    for seed in P.SEEDS:
        rows = P.oracle_of("no_round_runs", seed)[0]
        assert len(rows) >= 2 and not rows[:, 2].any()
        for top in (1, 3, 64):
            want = peak_search.top_rows(rows, top)
            assert same_rows(want, rows[:top])
            assert not same_rows(P.top_rows_reversed_ties(rows, top), want)
    rows = P.oracle_of("deep", P.SEEDS[0])[0]                       # distinct heights: both orders agree
    assert same_rows(P.top_rows_reversed_ties(rows, 3), peak_search.top_rows(rows, 3))


# ---- 4. the regional-maxima images ------------------------------------------------------------------------------------------
def test_designed_images_have_the_maxima_they_were_built_for():
    count = {n: int(P.image_mask(n).sum()) for n in P.images()}
    assert (count["snake_9x11"], count["snake_9x11_head"]) == (59, 1)
    assert (count["snake_big"], count["snake_big_head"]) == (5885, 1)
    assert count["spiral_21"] == int((P.images()["spiral_21"] == P.PLATEAU).sum()) > 200 and count["spiral_21_head"] == 1
    assert P.image_mask("snake_big_head")[0, 0] and P.image_mask("spiral_21_head")[0, 0]
    assert count["checkerboard_7x9"] == 32 and count["single_1x1"] == 0
    assert np.array_equal(P.image_mask("row_1x13"), P.image_mask("column_13x1").T) and count["row_1x13"] == 6
    frame = P.images()["border_plateau_6x8"] == 4.0
    assert np.array_equal(P.image_mask("border_plateau_6x8") & frame, frame) and count["border_plateau_6x8"] == frame.sum() + 1
    assert P.images()["snake_big"].shape == P.BIG
    assert P.lds_bytes(P.BIG[0] * P.BIG[1]) <= 160 * 1024 < P.lds_bytes(P.REFUSED[0] * P.REFUSED[1])
    assert P.lds_bytes(P.BIG[0] * (P.BIG[1] + 1)) > 160 * 1024      # no larger image of either shape fits


def test_mirror_maxima_equal_the_flood_fill_and_the_snake_needs_thousands_of_passes():
    for n, im in P.images().items():
        assert np.array_equal(peak_search.regional_maxima(im), P.image_mask(n)), n
    passes = {n: P.maxima_by_passes(P.images()[n])[1] for n in ("snake_9x11_head", "snake_big_head", "spiral_21_head")}
    print("FIGURES propagation passes:", passes)
    assert passes["snake_9x11_head"] > 16 and passes["spiral_21_head"] > 16
    npix = P.BIG[0] * P.BIG[1]
    assert npix // 2 - 108 <= passes["snake_big_head"] < npix       # about npix / 2, inside pk_maxima's guard of npix
