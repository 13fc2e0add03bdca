"""The case table of the CFAR detector tests (no test in this module): tests/test_detect.py holds the host model
(tests/host_model/cfar_model.cpp) to ``detect.cfar_host`` on it, tests/test_gpu_detect.py the kernel.

A case is one setting (grid, oversampling, method, window, Le) and a small batch of scenes: truth, QPSK symbols, y = s mu + w cast
to complex64, b = the transmitted symbols.  Also here: the comparison every holder of the table uses and the Monte-Carlo draws.

What is compared how.  ``n_over``, ``n_det``, ``state`` and the (tau, f) of every row are decisions: they equal the mirror's
exactly wherever the mirror's decision margin (``CfarHost.margin``: the least relative gap of P against alpha Z over the cells, of
an over cell against each of its 8 neighbours, and of consecutive heights among the first Le + 1 detections) exceeds MARGIN.  The
cap on scenes left out is 0: the table is chosen so that every scene has the margin (tests/test_detect.py asserts it and prints
the margins).  Pairs that tie by construction are exempt: the pair of the tie case, and cells that differ only along an axis of
length 1, along which the map is constant by definition.  The heights, the map and ``level`` are numbers: the mirror takes FFTs,
``np.mean`` and ``np.sort``, the kernel direct sums in index order, and they agree to MAP_TOL (relative to the largest cell of the
scene) and LEVEL_TOL (relative).  The largest differences measured between the host model and the mirror on this table are
MAP_SEEN and LEVEL_SEEN; the tolerances are 8 times that.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

from admm_net_amd import detect, refine

MARGIN = 1e-9
MAP_SEEN, LEVEL_SEEN = 1.7e-15, 1.4e-15       # host model against mirror, the largest over the table (tests/test_detect.py prints them)
MAP_TOL, LEVEL_TOL = 8 * MAP_SEEN, 8 * LEVEL_SEEN
PSK = (4, math.pi / 4)
D_, N_, O_ = detect.DONE, detect.NONFINITE, detect.OUTSIDE


class Case(NamedTuple):
    name: str
    grid: tuple          # (Nb, Nd)
    y: np.ndarray        # [B, D] complex64
    b: np.ndarray        # [B, D] complex64
    symbols: object      # None or [B, D] int32
    noise_var: object    # None or [B] float64
    kw: dict             # top, oversample, method, pfa, guard, train, rank
    states: tuple        # the expected state of every scene
    exempt: tuple        # pairs of cells that tie by construction
    truth: tuple         # (tau, f, C) lists per scene

    @property
    def cells(self):
        r = self.kw["oversample"]
        return r * self.grid[0], r * self.grid[1]


def atoms(tau, f, grid):
    Nb, Nd = grid
    ib, idd = np.divmod(np.arange(Nb * Nd), Nd)
    return np.exp(2j * np.pi * (np.multiply.outer(ib, np.asarray(f, dtype=np.float64)) -
                                np.multiply.outer(idd, np.asarray(tau, dtype=np.float64))))


def scene(grid, tau, f, C, noise_var, rng):
    """(y, b, k): y = s mu + w in complex128, b = s the transmitted QPSK symbols, k their indices."""
    D = grid[0] * grid[1]
    mu = atoms(tau, f, grid) @ np.asarray(C, dtype=np.complex128) if len(tau) else np.zeros(D, np.complex128)
    k = rng.integers(0, PSK[0], D)
    s = refine.psk_points(*PSK)[k]
    w = math.sqrt(noise_var / 2.0) * (rng.normal(size=D) + 1j * rng.normal(size=D))
    return mu * s + w, s, k


def cell_of(tau, f, grid, r):
    """The linear index of the map cell at (tau, f), which must lie on the map."""
    nf, nt = r * grid[0], r * grid[1]
    j, i = (f + 0.5) * nf, tau * nt
    assert abs(j - round(j)) < 1e-9 and abs(i - round(i)) < 1e-9
    return int(round(j)) % nf * nt + int(round(i)) % nt


def build(name, grid, scenes, *, seed, method="ca", top=6, oversample=2, pfa=1e-3, guard=1, train=2, rank=None, noise_var=1.0,
          known=None, given=False, states=None, exempt=(), edit=None):
    """``scenes``: per scene (tau, f, C) lists; ``noise_var`` the variance of the noise drawn; ``known``: what a "known" case is
    told per scene (None: the truth); ``given``: the transmitted symbols go in as ``symbols`` and b is all ones;
    ``edit(y, b, symbols)`` changes the arrays in place."""
    rng = np.random.default_rng(seed)
    B, D = len(scenes), grid[0] * grid[1]
    y, b, sent = np.zeros((B, D), np.complex64), np.zeros((B, D), np.complex64), np.zeros((B, D), np.int32)
    for i, (tau, f, C) in enumerate(scenes):
        y[i], s, sent[i] = scene(grid, tau, f, C, noise_var, rng)
        b[i] = 1.0 if given else s
    symbols = sent if given else None
    if edit:
        edit(y, b, symbols)
    told = None
    if method == "known":
        told = np.full(B, float(noise_var)) if known is None else np.asarray(known, dtype=np.float64)
    kw = dict(top=top, oversample=oversample, method=method, pfa=pfa, guard=guard, train=train, rank=rank)
    return Case(name, grid, y, b, symbols, told, kw, tuple(states) if states is not None else (D_,) * B, tuple(exempt), tuple(scenes))


def draw(seed, B, grid, lo=1, hi=3, snr_db=15.0):
    """B scenes of lo .. hi targets of magnitude 0.5 .. 1 whose weakest stands ``snr_db`` above noise of variance 1 after the
    matched filter's gain is left out (|C|^2 / noise_var)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        L = int(rng.integers(lo, hi + 1))
        mag = rng.uniform(0.5, 1.0, L) * math.sqrt(10.0 ** (snr_db / 10.0) / 0.25) / math.sqrt(grid[0] * grid[1])
        out.append((rng.uniform(0.05, 0.95, L), rng.uniform(-0.45, 0.45, L), mag * np.exp(2j * np.pi * rng.uniform(size=L))))
    return out


GRIDS = (   # grid, oversample, guard, train, scenes
    ((1, 12), 2, 1, 2, 2),
    ((12, 1), 2, 1, 2, 2),
    ((4, 6), 3, 0, 1, 2),
    ((5, 7), 3, 1, 1, 2),       # 315 cells: no power of two, more than one pass of a 256-thread group
    ((8, 8), 1, 1, 2, 2),
    ((8, 8), 2, 1, 2, 2),
    ((16, 16), 4, 1, 2, 2),
    ((13, 262), 1, 1, 2, 2),    # the largest grid admitted (Nb Nd = 3406, 154 176 bytes of LDS)
)
LARGEST = ((13, 262), 1)
TOPS = (1, 6, 16)


def _nan_y(y, b, symbols):
    y[1, 3] = np.nan
    y[2, 0] = np.inf
    b[3, 5] = 0.0
    b[4, 7] = np.nan


def _bad_symbols(y, b, symbols):
    symbols[1, 7] = -1
    symbols[2, 9] = PSK[0]
    y[2, 1] = np.nan                # state 4 is looked for first


TIE_AT = (3 / 16, 2 / 16)


def _tie(y, b, symbols):
    """x real: the map cells (tau, f) and (-tau, -f) are conjugates of each other and exactly as high, in every arithmetic
    that treats a number and its conjugate alike (16 map cells per axis: every twiddle argument is a dyadic fraction)."""
    ib, idd = np.divmod(np.arange(64), 8)
    rng = np.random.default_rng(77)
    y[0] = (2.0 * np.cos(2 * np.pi * (ib * TIE_AT[1] - idd * TIE_AT[0])) + 0.05 * rng.normal(size=64)).astype(np.float32)
    b[0] = 1.0


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for g, (grid, r, guard, train, B) in enumerate(GRIDS):
        for k, method in enumerate(("known", "ca", "os")):
            out.append(build(f"{method}_{grid[0]}x{grid[1]}_r{r}", grid, draw(100 + 3 * g + k, B, grid), seed=200 + 3 * g + k,
                             method=method, top=TOPS[(g + k) % 3], oversample=r, guard=guard, train=train))
    on = lambda jb, i_d, r=2, grid=(8, 8): (i_d / (r * grid[1]), jb / (r * grid[0]) - 0.5)  # noqa: E731  (tau, f) of a map cell
    one = lambda tf, C: ([tf[0]], [tf[1]], [C])  # noqa: E731
    # a target in cell (0, 0): tau = 0, f = -1/2 -- the window and the neighbourhood wrap both axes
    for method in ("ca", "os"):
        out.append(build(f"cell_0_0_{method}", (8, 8), [one(on(0, 0), 1.0 + 0.5j)], seed=301, method=method, noise_var=0.05))
    # two targets two resolution cells apart on both axes, the weaker 10 dB down: inside the stronger one's training ring
    pair = ([on(8, 6)[0], on(12, 10)[0]], [on(8, 6)[1], on(12, 10)[1]], [1.0, 0.316j])
    for method in ("ca", "os"):
        out.append(build(f"masked_pair_{method}", (8, 8), [pair], seed=302, method=method, pfa=1e-4, noise_var=2e-3, top=16))
    three = ([0.21, 0.55, 0.83], [-0.31, 0.12, 0.33], [1.0, 0.8j, -0.9])
    out.append(build("more_than_Le", (8, 8), [three], seed=303, top=1, noise_var=0.05))
    out.append(build("noise_many_over", (8, 8), [([], [], [])] * 2, seed=304, top=6, pfa=0.2, method="os"))
    out.append(build("no_detection", (8, 8), [([], [], [])] * 2, seed=305, method="known", known=[100.0, 50.0]))
    out.append(build("silence", (8, 8), [([], [], [])], seed=314, noise_var=0.0))            # y = 0: P = alpha Z = 0 in every cell
    out.append(build("exact_tie", (8, 8), [([], [], [])], seed=306, top=2, edit=_tie,
                     exempt=[(cell_of(TIE_AT[0], TIE_AT[1], (8, 8), 2), cell_of(1 - TIE_AT[0], -TIE_AT[1], (8, 8), 2))]))
    out.append(build("rank_1", (8, 8), [three, pair], seed=307, method="os", rank=1, noise_var=0.05))
    out.append(build("rank_N", (8, 8), [three, pair], seed=308, method="os", rank=40, noise_var=0.05))
    out.append(build("guard_0", (8, 8), [three, pair], seed=309, guard=0, train=2, noise_var=0.05))
    out.append(build("guard_0_os", (8, 8), [three], seed=310, method="os", guard=0, train=3, noise_var=0.05, top=16))
    out.append(build("nonfinite", (8, 8), [three] * 5, seed=311, noise_var=0.05, edit=_nan_y, states=(D_, N_, N_, N_, N_)))
    out.append(build("symbols_given", (8, 8), [three] * 3, seed=312, noise_var=0.05, given=True, edit=_bad_symbols,
                     states=(D_, O_, O_)))
    out.append(build("known_noise_var", (8, 8), [three] * 5, seed=313, method="known", noise_var=0.05,
                     known=[0.05, 0.0, -1.0, math.nan, math.inf], states=(D_, O_, O_, N_, N_)))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def host(c, i, **kw):
    pick = lambda v: None if v is None else v[i]  # noqa: E731
    nv = pick(c.noise_var)
    return detect.cfar_host(c.y[i], c.b[i], c.grid, **{**c.kw, **dict(noise_var=None if nv is None else float(nv),
                                                                     symbols=pick(c.symbols), psk=PSK, exempt=c.exempt), **kw})


@functools.lru_cache(maxsize=None)
def reference(name):
    """``cfar_host`` scene by scene.  Computed once per case."""
    c = case(name)
    return tuple(host(c, i) for i in range(len(c.y)))


def compare(name, rows, n_det, n_over, level, state, pmap, what):
    """Decisions exactly (every scene of the table has the margin), numbers within MAP_TOL and LEVEL_TOL.  rows [B, Le, 3],
    n_det, n_over, level, state [B], pmap [B, n_f, n_tau].  Returns (the worst height or map difference / the largest cell, the
    worst relative level difference)."""
    c, ref = case(name), reference(name)
    Le = c.kw["top"]
    worst_map = worst_level = 0.0
    for i, r in enumerate(ref):
        assert r.margin > MARGIN, (what, name, i, r.margin)
        assert int(state[i]) == r.state == c.states[i], (what, name, i, int(state[i]), r.state)
        assert int(n_det[i]) == r.n_det and int(n_over[i]) == r.n_over, (what, name, i, int(n_det[i]), r.n_det, int(n_over[i]), r.n_over)
        if r.state != D_:
            assert r.n_det == 0 and r.n_over == 0 and np.isnan(level[i]) and np.isnan(rows[i]).all() and np.isnan(pmap[i]).all()
            continue
        assert np.array_equal(rows[i][:, :2], r.rows[:, :2], equal_nan=True), (what, name, i, rows[i], r.rows)
        n = min(r.n_det, Le)
        assert np.isnan(rows[i][n:]).all() and np.isfinite(rows[i][:n]).all()
        top = max(float(r.map.max()), 1e-300)
        d_map = max(float(np.abs(pmap[i] - r.map).max()), float(np.abs(rows[i][:n, 2] - r.rows[:n, 2]).max(initial=0.0))) / top
        d_level = abs(float(level[i]) - r.level) / max(r.level, 1e-300)
        worst_map, worst_level = max(worst_map, d_map), max(worst_level, d_level)
        assert d_map <= MAP_TOL, (what, name, i, d_map)
        assert d_level <= LEVEL_TOL, (what, name, i, d_level)
        # the rows are cells of the map that came with them
        nf, nt = c.cells
        for l in range(n):
            j, k = round((rows[i][l, 1] + 0.5) * nf), round(rows[i][l, 0] * nt)
            assert rows[i][l, 2] == pmap[i][j, k], (what, name, i, l)
    return worst_map, worst_level


# ---- Monte Carlo -----------------------------------------------------------------------------------------------------------------------
MC_GRID, MC_R, MC_DRAWS, MC_PFA = (8, 8), 2, 2000, 1e-3
MC_LEFT_OUT = 0.01


@functools.lru_cache(maxsize=None)
def monte_carlo(targets, draws=MC_DRAWS, seed=977):
    """(y, b, noise_var): ``draws`` scenes of the 8 x 8 grid with noise of variance 1 -- noise only, or with 1 .. 3 targets at
    15 dB (``draw``) -- drawn with numpy: the law of the GPU test's scenes, not their bits."""
    rng = np.random.default_rng(seed)
    scenes = draw(seed + 1, draws, MC_GRID) if targets else [([], [], [])] * draws
    D = MC_GRID[0] * MC_GRID[1]
    y, b = np.zeros((draws, D), np.complex64), np.zeros((draws, D), np.complex64)
    for i, (tau, f, C) in enumerate(scenes):
        y[i], b[i], _ = scene(MC_GRID, tau, f, C, 1.0, rng)
    return y, b, np.ones(draws)


def mc_host(y, b, noise_var, method):
    """(n_over, n_det, margin) [draws] of ``cfar_host`` on every scene."""
    res = [detect.cfar_host(y[i], b[i], MC_GRID, top=6, oversample=MC_R, method=method, pfa=MC_PFA,
                            noise_var=float(noise_var[i]) if method == "known" else None) for i in range(len(y))]
    return (np.array([r.n_over for r in res]), np.array([r.n_det for r in res]), np.array([r.margin for r in res]))


# ---- noise only: the false-alarm rate -----------------------------------------------------------------------------------------------------
def noise_scenes(B, grid, seed):
    rng = np.random.default_rng(seed)
    D = grid[0] * grid[1]
    return (rng.normal(size=(B, D)) + 1j * rng.normal(size=(B, D))) / math.sqrt(2.0)
