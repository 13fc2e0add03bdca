"""The case table of the refinement tests (no test in this module): tests/test_refine.py holds the host model
(tests/host_model/refine_model.cpp) to ``refine.refine_host`` on it, tests/test_gpu_refine.py the kernel.

A case is a small batch of scenes: truth drawn like ``synth.make_batch`` (or on a jittered lattice, so that many targets stay
apart), QPSK symbols, y = s mu + w cast to complex64 as the generator returns it, b = the transmitted symbols with ``wrong`` of
them rotated, and starting rows = truth moved by up to ``start`` resolution cells.  Also here: the scene of the Monte-Carlo and
planted-symbol tests (the issue's 8 x 8 scene) and the comparison every holder of the table uses.

Two fits of one scene that both report ``converged`` with a contraction q < 1/2 of consecutive steps each stopped within
tol q / (1 - q) <= tol of the stationary point, their paths differing only in rounding: the allowed distance is 4 tol cells.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

from admm_net_amd import metrics, refine

TOL = 1e-6
PSK = (4, math.pi / 4)
Q_MAX = 0.5                    # the ratio of the last two accepted steps below which a converging case is compared
MAX_DROPPED = 2


class Case(NamedTuple):
    name: str
    grid: tuple          # (Nb, Nd)
    y: np.ndarray        # [B, D] complex64
    b: np.ndarray        # [B, D] complex64
    rows: np.ndarray     # [B, Le, 3] float64
    n_est: object        # None or [B] int32
    symbols: str
    truth: tuple         # (tau, f, C) [B, L]
    sent: np.ndarray     # [B, D] the k of the transmitted symbols
    states: tuple        # the expected state of every scene, None: whatever the mirror says
    iters: int

    @property
    def kw(self):
        return dict(symbols=self.symbols, psk=PSK, iters=self.iters, tol=TOL)


def signal(tau, f, C, grid, snr_db, rng):
    """(y, v, k): the received signal in complex128, its noise variance and the transmitted QPSK symbols of one scene."""
    D = grid[0] * grid[1]
    mu = metrics.crb_signal(tau, f, C, grid)
    v = float((np.abs(mu) ** 2).sum() / (10.0 ** (snr_db / 10.0) * D))
    k = rng.integers(0, PSK[0], D)
    w = math.sqrt(v / 2.0) * (rng.normal(size=D) + 1j * rng.normal(size=D))
    return mu * refine.psk_points(*PSK)[k] + w, v, k


def rotate(k, wrong, rng):
    """k with ``wrong`` entries moved by a random non-zero multiple of a quarter turn; (k', the entries)."""
    at = rng.choice(len(k), wrong, replace=False)
    out = k.copy()
    out[at] = (out[at] + rng.integers(1, PSK[0], wrong)) % PSK[0]
    return out, np.sort(at)


def draw(seed, B, L, spread=None):
    rng = np.random.default_rng(seed)
    if spread:
        side = int(np.ceil(np.sqrt(L)))
        cell = np.stack([rng.permutation(side * side)[:L] for _ in range(B)])
        tau = 0.1 + 0.8 * ((cell // side) + 0.5 + rng.uniform(-spread, spread, (B, L))) / side
        f = -0.4 + 0.8 * ((cell % side) + 0.5 + rng.uniform(-spread, spread, (B, L))) / side
    else:
        tau, f = rng.uniform(0.1, 0.9, (B, L)), rng.uniform(-0.4, 0.4, (B, L))
    mag = rng.uniform(0.5, 1.0, (B, L))
    return tau, f, mag * np.exp(2j * np.pi * rng.uniform(size=(B, L)))


def build(name, grid, truth, *, seed, snr_db=20.0, start=0.2, wrong=0, symbols="given", pad=0, n_est=None, states=None, edit=None, iters=16):
    """``pad`` absent rows (NaN) are put in the MIDDLE of the rows; ``edit(y, b, rows)`` changes the arrays in place."""
    rng = np.random.default_rng(seed)
    tau, f, C = (np.asarray(v) for v in truth)
    B, L = tau.shape
    D = grid[0] * grid[1]
    y, b, sent = np.zeros((B, D), np.complex64), np.zeros((B, D), np.complex64), np.zeros((B, D), np.int64)
    rows = np.full((B, L + pad, 3), np.nan)
    keep = [j for j in range(L + pad) if not L // 2 <= j < L // 2 + pad]
    for i in range(B):
        yi, _, k = signal(tau[i], f[i], C[i], grid, snr_db, rng)
        y[i], sent[i] = yi, k
        b[i] = refine.psk_points(*PSK)[rotate(k, wrong, rng)[0]]
        rows[i, keep, 0] = tau[i] + rng.uniform(-start, start, L) / grid[1]
        rows[i, keep, 1] = f[i] + rng.uniform(-start, start, L) / grid[0]
        rows[i, keep, 2] = np.abs(C[i])
    if edit:
        edit(y, b, rows)
    return Case(name, grid, y, b, rows, None if n_est is None else np.asarray(n_est, dtype=np.int32), symbols, (tau, f, C), sent,
                None if states is None else tuple(states), iters)


def _pair(cells, grid):
    tau = np.array([[0.4, 0.4 + cells / grid[1]]])
    f = np.array([[-0.1, -0.1 + cells / grid[0]]])
    return tau, f, np.array([[0.6 - 0.3j, -0.2 + 0.7j]])


def _coincide(y, b, rows):
    rows[:, 1, :2] = rows[:, 0, :2]


def _nan_y(y, b, rows):
    y[1, 3] = np.nan


def _zero_b(y, b, rows):
    b[0, 5] = 0.0


@functools.lru_cache(maxsize=None)
def cases():
    C, G, L = refine.CONVERGED, refine.GAVE_UP, refine.LIMIT
    out = [
        build("L1_4x6", (4, 6), draw(1, 2, 1), seed=1),
        build("L1_1x12", (1, 12), draw(2, 2, 1), seed=2),
        build("L2_12x1", (12, 1), draw(3, 2, 2, spread=0.1), seed=3),
        build("L3_8x8", (8, 8), draw(4, 3, 3), seed=4),
        build("L3_8x8_psk", (8, 8), draw(4, 3, 3), seed=4, snr_db=30.0, start=0.1, wrong=4, symbols="psk"),
        build("L3_8x8_wrong_given", (8, 8), draw(4, 2, 3), seed=5, snr_db=30.0, wrong=4),
        build("L16_16x16", (16, 16), draw(5, 2, 16, spread=0.15), seed=6, start=0.1),
        build("L16_16x16_psk", (16, 16), draw(5, 1, 16, spread=0.15), seed=7, snr_db=30.0, start=0.05, wrong=6, symbols="psk"),
        build("L3_26x131", (26, 131), draw(8, 1, 3), seed=8, snr_db=5.0),
        build("L16_26x131", (26, 131), draw(9, 1, 16, spread=0.15), seed=9, snr_db=10.0, start=0.1),
        build("L3_13x262_psk", (13, 262), draw(10, 1, 3), seed=10, snr_db=10.0, wrong=60, symbols="psk"),
        build("pair_0.5_cells", (10, 10), _pair(0.5, (10, 10)), seed=11, snr_db=30.0, start=0.05),
        build("pair_26x131_far_start", (26, 131), _pair(0.5, (26, 131)), seed=0, snr_db=10.0, start=0.45),
        build("L3_8x8_far_start", (8, 8), draw(2, 1, 3), seed=2, start=0.6),
        build("absent_in_the_middle", (8, 8), draw(12, 2, 3), seed=12, pad=2),
        build("n_est", (8, 8), draw(13, 4, 3), seed=13, n_est=[0, 2, 3, 1]),
        build("n_est_outside", (8, 8), draw(13, 3, 3), seed=14, n_est=[3, 4, -1], states=(None, refine.OUTSIDE, refine.OUTSIDE)),
        build("coincident_pair", (10, 10), _pair(0.5, (10, 10)), seed=15, edit=_coincide, states=(G,)),
        build("nan_y", (8, 8), draw(16, 3, 3), seed=16, edit=_nan_y, states=(None, refine.NONFINITE, None)),
        build("zero_b_given", (8, 8), draw(17, 2, 2), seed=17, edit=_zero_b, states=(refine.NONFINITE, None)),
        build("zero_b_psk", (8, 8), draw(17, 2, 2), seed=17, symbols="psk", edit=_zero_b, states=(C, C)),
        build("one_iteration_is_the_limit", (8, 8), draw(18, 1, 3), seed=18, states=(L,), iters=1),
    ]
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """``refine_host`` scene by scene.  Computed once per case."""
    c = case(name)
    return tuple(refine.refine_host(c.y[i], c.b[i], c.rows[i], c.grid, n_est=None if c.n_est is None else int(c.n_est[i]), **c.kw)
                 for i in range(len(c.y)))


def contraction(r):
    """The ratio of the last two accepted steps of a fit (0 where it made fewer than two, or the last one did not move)."""
    return r.moves[-1] / r.moves[-2] if len(r.moves) >= 2 and r.moves[-2] > 0 else 0.0


def comparable(name):
    """The scenes of a case in which the mirror converged with a contraction below Q_MAX."""
    return [i for i, r in enumerate(reference(name)) if r.state == refine.CONVERGED and contraction(r) < Q_MAX]


def dropped():
    """(case, scene) of every converged scene of the table that the mirror does not hold to q < 1/2."""
    return [(c.name, i) for c in cases() for i, r in enumerate(reference(c.name))
            if r.state == refine.CONVERGED and i not in comparable(c.name)]


def compare(name, rows, C, info, symbols, what):
    """state, iterations' sanity, flips, absent rows and symbols exactly; where both converged (and the mirror contracts),
    |dtau| Nd and |df| Nb within 4 tol.  rows [B, Le, 3], C [B, Le], info [B, 5] = (Q, Q / D, iterations, flips, state),
    symbols [B, D].  Returns the worst distance / (4 tol)."""
    c, ref = case(name), reference(name)
    worst = 0.0
    for i, r in enumerate(ref):
        state = int(info[i][4])
        assert state == r.state, (what, name, i, state, r.state)
        if c.states is not None and c.states[i] is not None:
            assert state == c.states[i], (what, name, i, state)
        assert np.array_equal(np.isnan(rows[i]), np.isnan(r.rows)), (what, name, i)
        assert np.array_equal(np.isnan(C[i]), np.isnan(r.C)), (what, name, i)
        assert int(info[i][3]) == r.flips, (what, name, i, info[i][3], r.flips)
        assert np.array_equal(np.asarray(symbols[i]), r.symbols), (what, name, i)
        if state in (refine.NONFINITE, refine.OUTSIDE):
            assert np.isnan(info[i][0]) and np.isnan(rows[i]).all()
            continue
        if state == refine.CONVERGED and i in comparable(name):
            here = ~np.isnan(r.rows[:, 0])
            d = max(float(np.abs(rows[i][here, 0] - r.rows[here, 0]).max(initial=0.0)) * c.grid[1],
                    float(np.abs(rows[i][here, 1] - r.rows[here, 1]).max(initial=0.0)) * c.grid[0])
            worst = max(worst, d / (4.0 * TOL))
            assert d <= 4.0 * TOL, (what, name, i, d)
            assert np.allclose(C[i][here], r.C[here], rtol=0, atol=1e-4 * np.abs(r.C[here]).max(initial=0.0)), (what, name, i)
            assert math.isclose(info[i][0], r.cost, rel_tol=1e-6), (what, name, i, info[i][0], r.cost)
    return worst


# ---- the scene of the Monte-Carlo and the planted-symbol tests -----------------------------------------------------------------------
SCENE_GRID = (8, 8)
SCENE = (np.array([0.3093, 0.3388, 0.7514]), np.array([-0.3265, 0.0801, 0.1828]),
         np.array([-0.228 - 0.388j, 0.542 + 0.684j, 0.197 - 0.217j]))
MC_DRAWS = 2000
MC_BAND = 4.5 * math.sqrt(2.0 / MC_DRAWS)


@functools.lru_cache(maxsize=None)
def monte_carlo(draws=MC_DRAWS, snr_db=20.0, start=0.3, seed=2024):
    """(y, b, rows, bound): ``draws`` noise draws of SCENE with KNOWN symbols (b = the transmitted ones), start = truth +- ``start``
    cell uniform; bound [6] = the Cramer-Rao bound of (tau_1..3, f_1..3) at the scene's noise variance."""
    tau, f, C = SCENE
    rng = np.random.default_rng(seed)
    D = SCENE_GRID[0] * SCENE_GRID[1]
    y, b, rows = np.zeros((draws, D), np.complex64), np.zeros((draws, D), np.complex64), np.zeros((draws, 3, 3))
    for i in range(draws):
        yi, v, k = signal(tau, f, C, SCENE_GRID, snr_db, rng)
        y[i], b[i] = yi, refine.psk_points(*PSK)[k]
        rows[i, :, 0] = tau + rng.uniform(-start, start, 3) / SCENE_GRID[1]
        rows[i, :, 1] = f + rng.uniform(-start, start, 3) / SCENE_GRID[0]
    bound = metrics.crb_host(tau, f, C, SCENE_GRID, noise_var=v).bound
    return y, b, rows, np.concatenate([bound[:, 0], bound[:, 1]])


def mc_ratios(rows, bound):
    """Mean squared error over bound of the six parameters, from the fitted rows [draws, 3, 3]."""
    err = np.concatenate([rows[:, :, 0] - SCENE[0], rows[:, :, 1] - SCENE[1]], axis=1)
    return (err ** 2).mean(axis=0) / bound


PLANTED_SEEDS = tuple(range(100, 112))
PLANTED = 5


@functools.lru_cache(maxsize=None)
def planted(seed, snr_db=40.0, start=0.1):
    """(y, b, rows, sent, at, v): SCENE at 40 dB with PLANTED of the 64 symbols of b rotated, start = truth +- 0.1 cell."""
    tau, f, C = SCENE
    rng = np.random.default_rng(seed)
    yi, v, k = signal(tau, f, C, SCENE_GRID, snr_db, rng)
    kb, at = rotate(k, PLANTED, rng)
    rows = np.zeros((3, 3))
    rows[:, 0] = tau + rng.uniform(-start, start, 3) / SCENE_GRID[1]
    rows[:, 1] = f + rng.uniform(-start, start, 3) / SCENE_GRID[0]
    return yi.astype(np.complex64), refine.psk_points(*PSK)[kb].astype(np.complex64), rows, k, at, v
