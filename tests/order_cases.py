"""The case table of the model-order tests (no test in this module): tests/test_order.py holds the host model
(tests/host_model/order_model.cpp) to ``order.select_host`` on it, tests/test_gpu_order.py the kernel.

A case is a small batch of scenes built like those of tests/refine_cases.py: truth, QPSK symbols, y = s mu + w cast to complex64,
b = the transmitted symbols, and candidate rows = the truths moved by up to ``start`` cells followed by ``spare`` rows drawn at
random.  Also here: the comparison every holder of the table uses, the Monte-Carlo scene of the selection-and-refinement loop and
that loop on the mirror.

What is compared how.  ``perm``, ``n_sel``, ``ranked`` and ``state`` are decisions: they equal the mirror's exactly wherever the
mirror's decision margin (``OrderHost.margin``: the relative gap between the gain taken and the next, and between the two lowest
criteria) exceeds MARGIN; the table is chosen so that every scene does (tests/test_order.py asserts it and prints the margins).
``rss``, ``C`` and ``cost`` are numbers: the mirror solves every subset afresh with an SVD, the kernel downdates a Cholesky factor
of the Gram matrix, and they agree to RSS_TOL, C_TOL (relative to RSS_0 and to the largest |C| of the scene).  The largest
difference measured between the host model and the mirror on this table is RSS_SEEN and C_SEEN; the tolerances are 8 times that.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

from admm_net_amd import order, refine

import refine_cases as RC

MARGIN = 1e-9
RSS_SEEN, C_SEEN = 2.4e-15, 2.8e-14            # host model against mirror, the largest over the table (tests/test_order.py prints them)
RSS_TOL, C_TOL = 8 * RSS_SEEN, 8 * C_SEEN
PSK = RC.PSK


class Case(NamedTuple):
    name: str
    grid: tuple          # (Nb, Nd)
    y: np.ndarray        # [B, D] complex64
    b: np.ndarray        # [B, D] complex64
    rows: np.ndarray     # [B, Le, 3] float64
    n_cand: object       # None or [B] int32
    n_held: object       # None or [B] int32
    symbols: object      # None or [B, D] int32
    penalty: object      # None or a float
    max_order: object    # None or an int
    states: tuple        # the expected state of every scene
    n_sel: object        # None or the expected n_sel of every scene

    @property
    def kw(self):
        return dict(psk=PSK, penalty=self.penalty, max_order=self.max_order)


def build(name, grid, truth, *, seed, spare=0, snr_db=20.0, start=0.2, n_cand=None, n_held=None, given=False, penalty=None,
          max_order=None, states=None, n_sel=None, edit=None):
    """``spare`` rows drawn uniformly follow the displaced truths; ``given``: the transmitted symbols go in as ``symbols`` and b is
    all ones; ``edit(y, b, rows, symbols)`` changes the arrays in place."""
    rng = np.random.default_rng(seed)
    tau, f, C = (np.asarray(v) for v in truth)
    B, L = tau.shape
    D = grid[0] * grid[1]
    y, b, sent = np.zeros((B, D), np.complex64), np.zeros((B, D), np.complex64), np.zeros((B, D), np.int32)
    rows = np.zeros((B, L + spare, 3))
    for i in range(B):
        yi, _, k = RC.signal(tau[i], f[i], C[i], grid, snr_db, rng)
        y[i], sent[i] = yi, k
        b[i] = 1.0 if given else refine.psk_points(*PSK)[k]
        rows[i, :L, 0] = tau[i] + rng.uniform(-start, start, L) / grid[1]
        rows[i, :L, 1] = f[i] + rng.uniform(-start, start, L) / grid[0]
        rows[i, L:, 0], rows[i, L:, 1] = rng.uniform(0.0, 1.0, spare), rng.uniform(-0.5, 0.5, spare)
    symbols = sent if given else None
    if edit:
        edit(y, b, rows, symbols)
    as_i32 = lambda v: None if v is None else np.asarray(v, dtype=np.int32)  # noqa: E731
    return Case(name, grid, y, b, rows, as_i32(n_cand), as_i32(n_held), symbols, penalty, max_order,
                tuple(states) if states is not None else (order.RANKED,) * B, None if n_sel is None else tuple(n_sel))


def _coincide(y, b, rows, symbols):
    rows[:, 3, :2] = rows[:, 0, :2]


def _near_pair(y, b, rows, symbols):
    rows[:, 3, 0] = rows[:, 1, 0] + 0.35 / 8
    rows[:, 3, 1] = rows[:, 1, 1]


def _absent(y, b, rows, symbols):
    rows[:, 1, 0] = np.nan
    rows[:, 4, 1] = np.inf


def _spare_first(y, b, rows, symbols):
    rows[:] = rows[:, [3, 4, 0, 1, 2, 5]]


def _nan_y(y, b, rows, symbols):
    y[1, 3] = np.nan


def _zero_b(y, b, rows, symbols):
    b[0, 5] = 0.0


def _minus_one(y, b, rows, symbols):
    symbols[1, 7] = -1
    symbols[2, 9] = PSK[0]


TIE_ROW = (0.2871, 0.1693)


def _tie(y, b, rows, symbols):
    """x real: the rows (tau, f) and (-tau, -f) are conjugates of each other and gain exactly the same, in every arithmetic."""
    ib, idd = np.divmod(np.arange(64), 8)
    rng = np.random.default_rng(77)
    y[0] = (2.0 * np.cos(2 * np.pi * (ib * TIE_ROW[1] - idd * TIE_ROW[0])) + 0.05 * rng.normal(size=64)).astype(np.float32)
    b[0] = 1.0
    rows[0, :, :2] = [[0.61, -0.33], [TIE_ROW[0], TIE_ROW[1]], [-TIE_ROW[0], -TIE_ROW[1]]]


def _constant(y, b, rows, symbols):
    """x = 1/2 exactly: the row (0, 0) leaves RSS_1 = 0, below the floor."""
    y[0], b[0] = 0.5, 1.0
    rows[0, :, :2] = [[0.25, 0.125], [0.0, 0.0]]


def on_grid(grid, cells):
    """Rows on the grid's own frequencies (tau = k / Nd, f = k / Nb): their atoms are exactly orthogonal."""
    return np.array([[kd / grid[1], kb / grid[0], 0.0] for kb, kd in cells])


def _on_grid(y, b, rows, symbols):
    rows[0] = on_grid((8, 8), [(1, 2), (3, 5), (6, 1), (2, 2), (5, 7), (0, 4)])


def _truth_on_grid():
    r = on_grid((8, 8), [(1, 2), (3, 5), (6, 1)])
    return r[None, :, 0], r[None, :, 1], np.array([[0.9 - 0.2j, -0.4 + 0.5j, 0.3 + 0.3j]])


@functools.lru_cache(maxsize=None)
def cases():
    S = RC.SCENE
    scene = lambda B: tuple(np.repeat(v[None], B, axis=0) for v in S)  # noqa: E731
    N, O = order.NONFINITE, order.OUTSIDE
    out = [
        build("L1_of_1_1x12", (1, 12), RC.draw(1, 2, 1), seed=1, n_sel=(1, 1)),
        build("L2_of_6_12x1", (12, 1), RC.draw(3, 2, 2, spread=0.1), seed=3, spare=4),
        build("L1_of_6_4x6", (4, 6), RC.draw(2, 2, 1), seed=2, spare=5),
        build("L3_of_6_8x8", (8, 8), scene(3), seed=4, spare=3, snr_db=15.0),
        build("L5_of_16_16x16", (16, 16), RC.draw(5, 2, 5, spread=0.15), seed=6, spare=11, snr_db=25.0),
        build("L16_of_16_16x16", (16, 16), RC.draw(5, 1, 16, spread=0.15), seed=7, snr_db=30.0, start=0.05),
        build("L3_of_16_13x262", (13, 262), RC.draw(10, 1, 3), seed=10, spare=13, snr_db=10.0),
        build("L3_of_6_26x131", (26, 131), RC.draw(8, 1, 3), seed=8, spare=3, snr_db=5.0),
        build("coincident_pair", (8, 8), scene(1), seed=15, spare=3, edit=_coincide),
        build("pair_0.35_cells", (8, 8), scene(2), seed=16, spare=3, snr_db=30.0, start=0.05, edit=_near_pair),
        build("duplicate_before_the_weak_target", (8, 8), scene(1), seed=133, spare=3, edit=_near_pair),
        build("absent_in_the_middle", (8, 8), scene(2), seed=12, spare=3, edit=_absent),
        build("n_cand", (8, 8), scene(4), seed=13, spare=3, n_cand=[0, 2, 6, 3], n_sel=(0, None, None, None)),
        build("outside", (8, 8), scene(4), seed=14, spare=3, n_cand=[7, -1, 6, 4], n_held=[0, 0, 7, 5], states=(O, O, O, O)),
        build("n_held_2_not_the_best", (8, 8), scene(2), seed=17, spare=3, n_held=[2, 2], edit=_spare_first),
        build("exact_tie", (8, 8), scene(1), seed=18, edit=_tie),
        build("noiseless_below_the_floor", (8, 8), RC.draw(19, 1, 2), seed=19, edit=_constant, n_sel=(1,)),
        build("penalty_0", (8, 8), scene(2), seed=20, spare=3, penalty=0.0, n_sel=(6, 6)),
        build("huge_penalty", (8, 8), scene(2), seed=21, spare=3, penalty=1e9, n_held=[1, 0], n_sel=(1, 0)),
        build("max_order_2", (8, 8), scene(2), seed=22, spare=3, max_order=2, n_sel=(2, 2)),
        build("nan_y", (8, 8), scene(3), seed=23, spare=3, edit=_nan_y, states=(0, N, 0)),
        build("zero_b", (8, 8), scene(2), seed=24, spare=3, edit=_zero_b, states=(N, 0)),
        build("symbols_given", (8, 8), scene(3), seed=25, spare=3, given=True, edit=_minus_one, states=(0, O, O)),
        build("orthogonal_on_grid", (8, 8), _truth_on_grid(), seed=26, spare=3, snr_db=10.0, edit=_on_grid),
    ]
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def host(c, i, **kw):
    pick = lambda v: None if v is None else v[i]  # noqa: E731
    return order.select_host(c.y[i], c.b[i], c.rows[i], c.grid,
                             **{**dict(n_cand=pick(c.n_cand), n_held=pick(c.n_held), symbols=pick(c.symbols)), **c.kw, **kw})


@functools.lru_cache(maxsize=None)
def reference(name):
    """``select_host`` scene by scene.  Computed once per case."""
    c = case(name)
    return tuple(host(c, i) for i in range(len(c.y)))


def compare(name, perm, n_sel, rss, rows_out, C, residual, info, what):
    """Decisions exactly (every scene of the table has the margin), numbers within RSS_TOL and C_TOL, the residual to complex64
    rounding.  perm [B, Le], n_sel [B], rss [B, Le + 1], rows_out [B, Le, 3], C [B, Le], residual [B, D], info [B, 4] = (cost,
    cost / D, ranked, state).  Returns (the worst rss difference / RSS_0, the worst C difference / max |C|)."""
    c, ref = case(name), reference(name)
    worst_rss = worst_C = 0.0
    for i, r in enumerate(ref):
        assert r.margin > MARGIN, (what, name, i, r.margin)
        state = int(info[i][3])
        assert state == r.state == c.states[i], (what, name, i, state, r.state)
        assert np.array_equal(perm[i], r.perm), (what, name, i, perm[i], r.perm)
        assert int(n_sel[i]) == r.n_sel and int(info[i][2]) == r.ranked, (what, name, i, n_sel[i], r.n_sel, info[i][2], r.ranked)
        if c.n_sel is not None and c.n_sel[i] is not None:
            assert r.n_sel == c.n_sel[i], (what, name, i, r.n_sel)
        assert np.array_equal(np.isnan(rss[i]), np.isnan(r.rss)), (what, name, i)
        assert np.array_equal(np.isnan(C[i]), np.isnan(r.C)), (what, name, i)
        if state != order.RANKED:
            assert np.isnan(info[i][0]) and np.isnan(rows_out[i]).all() and np.isnan(residual[i]).all() and np.isnan(rss[i]).all()
            continue
        assert np.array_equal(rows_out[i][:, :2], c.rows[i][r.perm][:, :2], equal_nan=True), (what, name, i)
        k = r.ranked + 1
        d_rss = float(np.abs(rss[i][:k] - r.rss[:k]).max()) / max(r.rss[0], 1e-300)
        sel = slice(0, r.n_sel)
        d_C = float(np.abs(C[i][sel] - r.C[sel]).max(initial=0.0)) / max(float(np.abs(r.C[sel]).max(initial=0.0)), 1e-300)
        d_cost = abs(info[i][0] - r.cost) / max(r.rss[0], 1e-300)
        worst_rss, worst_C = max(worst_rss, d_rss, d_cost), max(worst_C, d_C)
        assert d_rss <= RSS_TOL and d_cost <= RSS_TOL, (what, name, i, d_rss, d_cost)
        assert d_C <= C_TOL, (what, name, i, d_C)
        assert np.allclose(rows_out[i][sel, 2], np.abs(C[i][sel]), rtol=4e-16, atol=0) and np.isnan(rows_out[i][r.n_sel:, 2]).all()
        assert info[i][1] == info[i][0] / (c.grid[0] * c.grid[1])
        top = float(np.abs(c.y[i]).max())
        assert np.allclose(residual[i], r.residual, rtol=0, atol=2.0 ** -22 * top), (what, name, i)
    return worst_rss, worst_C


# ---- the Monte-Carlo scene of the loop --------------------------------------------------------------------------------------------------
MC_DRAWS = 2000
MC_ROWS = 6


@functools.lru_cache(maxsize=None)
def monte_carlo(draws=MC_DRAWS, snr_db=15.0, seed=4242):
    """(y, b, rows): ``draws`` noise draws of refine_cases.SCENE (8 x 8, three targets) at 15 dB with known symbols, and six
    candidates each: rows 0 .. 2 the truths moved by up to 0.2 cell, rows 3 and 4 drawn at random, row 5 a duplicate 0.35 cell in
    tau and 0.3 cell in f from one of the truths."""
    tau, f, C = RC.SCENE
    Nb, Nd = RC.SCENE_GRID
    rng = np.random.default_rng(seed)
    y, b, rows = np.zeros((draws, Nb * Nd), np.complex64), np.zeros((draws, Nb * Nd), np.complex64), np.zeros((draws, MC_ROWS, 3))
    for i in range(draws):
        yi, _, k = RC.signal(tau, f, C, RC.SCENE_GRID, snr_db, rng)
        y[i], b[i] = yi, refine.psk_points(*PSK)[k]
        rows[i, :3, 0] = tau + rng.uniform(-0.2, 0.2, 3) / Nd
        rows[i, :3, 1] = f + rng.uniform(-0.2, 0.2, 3) / Nb
        rows[i, 3:5, 0], rows[i, 3:5, 1] = rng.uniform(0.0, 1.0, 2), rng.uniform(-0.5, 0.5, 2)
        twin = rng.integers(0, 3)
        rows[i, 5, 0], rows[i, 5, 1] = tau[twin] + 0.35 / Nd, f[twin] + 0.3 / Nb
    return y, b, rows


RIGHT, TOO_MANY, OTHER = range(3)


def outcome(n_sel, origin):
    """RIGHT: exactly the three displaced truths (rows 0 .. 2 of the input) are selected; TOO_MANY: more than three rows are."""
    if n_sel > 3:
        return TOO_MANY
    return RIGHT if n_sel == 3 and sorted(int(v) for v in origin[:3]) == [0, 1, 2] else OTHER


def loop_host(y, b, rows, grid, rounds):
    """``order.select_refined`` for ONE scene on the mirror (``select_host`` and ``refine_host``, symbols "given"): the
    (n_sel, origin, margin) of every selection, origin[j] = the input row that row j of that selection's rows_out started as."""
    sel = order.select_host(y, b, rows, grid)
    origin = sel.perm.copy()
    stages = [(sel.n_sel, origin, sel.margin)]
    for _ in range(rounds):
        fit = refine.refine_host(y, b, sel.rows_out, grid, n_est=sel.n_sel)
        merged = sel.rows_out.copy()
        fitted = (np.arange(len(merged)) < sel.n_sel) & np.isfinite(fit.rows[:, 0]) & np.isfinite(fit.rows[:, 1])
        merged[fitted] = fit.rows[fitted]
        sel = order.select_host(y, b, merged, grid)
        origin = origin[sel.perm]
        stages.append((sel.n_sel, origin, sel.margin))
    return stages


@functools.lru_cache(maxsize=None)
def mirror_loop(draws, rounds=1):
    """Per selection of the loop: (outcome [draws], margin [draws]) over the first ``draws`` scenes of ``monte_carlo()``."""
    y, b, rows = monte_carlo()
    stages = [loop_host(y[i], b[i], rows[i], RC.SCENE_GRID, rounds) for i in range(draws)]
    return tuple((np.array([outcome(s[r][0], s[r][1]) for s in stages]), np.array([s[r][2] for s in stages]))
                 for r in range(rounds + 1))


def shares(outcomes):
    return tuple(float((np.asarray(outcomes) == k).mean()) for k in (RIGHT, TOO_MANY, OTHER))
