"""The case table of the successive-cancellation tests (no test in this module): tests/test_relax.py holds the host model
(tests/host_model/relax_model.cpp) to ``detect.cfar_relax_host`` on it, tests/test_gpu_relax.py the kernel.

A case is one setting (grid, oversampling, method, window, Le, iters, sweeps) and a small batch of scenes built as in
tests/detect_cases.py, whose scenes, draws and helpers it reuses.

What is compared how.  ``n_det``, ``more``, ``maps`` and ``state`` are decisions: they equal the mirror's exactly wherever the
mirror's decision margin (``CfarRelaxHost.margin``) exceeds MARGIN.  The cap on scenes left out is 0: the table is chosen so that
every scene has the margin (tests/test_relax.py asserts it and prints the margins).  No pair of cells is listed as exempt; exempt by
construction are only two cells that differ along an axis of length 1, along which the map is constant by definition (the 1 x 12 and
12 x 1 cases).  The clamped case ("half_cell") keeps its partner in the margin: the noise breaks the tie of the four cells round
the target, and "near_bound" moves the target 0.1 map cell off the bound.  Everything else is a number, held to the mirror within 8
times the largest difference measured between the host model (under sanitizers) and the mirror on this table (the *_SEEN below;
tests/test_relax.py prints them):
    tau, f                in resolution cells (the difference times Nd, Nb)
    heights, level, map   relative to E = sum |y|^2, which bounds every cell of every map: a rounding error of the residual is one
                          of the SIGNAL, so the last map -- of a residual near the noise -- errs by a share of E, not of itself
    resid                 times D, relative to E
    amp                   relative to sqrt(E / D), which bounds |c|
"""
import functools
import math

import numpy as np

from admm_net_amd import detect

import detect_cases as DC

MARGIN = DC.MARGIN
POINT_SEEN, POWER_SEEN, AMP_SEEN = 1.6e-14, 1.9e-15, 9.7e-15   # host model against mirror, the largest over the table
POINT_TOL, POWER_TOL, AMP_TOL = 8 * POINT_SEEN, 8 * POWER_SEEN, 8 * AMP_SEEN
PSK = DC.PSK
D_, N_, O_ = DC.D_, DC.N_, DC.O_
on = lambda jb, i_d, r=2, grid=(8, 8): (i_d / (r * grid[1]), jb / (r * grid[0]) - 0.5)  # noqa: E731  (tau, f) of a map cell
one = lambda tf, C: ([tf[0]], [tf[1]], [C])  # noqa: E731


def build(name, grid, scenes, *, iters=3, sweeps=2, **kw):
    c = DC.build(name, grid, scenes, **kw)
    return c._replace(kw={**c.kw, "iters": iters, "sweeps": sweeps})


def from_detect(name, *, iters=3, sweeps=2, **kw):
    """A case of tests/detect_cases.py with the two settings added."""
    c = DC.case(name)
    return c._replace(name=name, kw={**c.kw, "iters": iters, "sweeps": sweeps, **kw}, exempt=())


GRIDS = DC.GRIDS[:6]          # 1 x 12 and 12 x 1 at r = 2, 4 x 6 and 5 x 7 at r = 3, 8 x 8 at r = 1, 2: all three methods
CLOSE = ([0.30, 0.30 + 1.5 / 8], [0.10, 0.10], [1.0, 1.0])        # two equal targets 1.5 resolution cells apart (along tau)
THREE = ([0.21, 0.55, 0.83], [-0.31, 0.12, 0.33], [1.0, 0.8j, -0.9])
CLOSE_SEED = 0
BLOCK = ([on(2 * p, 2 * q, 1)[0] for p in range(3) for q in range(3)], [on(2 * p, 2 * q, 1)[1] for p in range(3) for q in range(3)],
         [1.1 if (p, q) == (1, 1) else 1.0 - 0.01 * (3 * p + q) for p in range(3) for q in range(3)])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for g, (grid, r, guard, train, B) in enumerate(GRIDS):
        for k, method in enumerate(("known", "ca", "os")):
            out.append(build(f"{method}_{grid[0]}x{grid[1]}_r{r}", grid, DC.draw(100 + 3 * g + k, B, grid), seed=200 + 3 * g + k,
                             method=method, top=DC.TOPS[(g + k) % 3], oversample=r, guard=guard, train=train))
    out.append(build("os_16x16_r4", (16, 16), DC.draw(130, 1, (16, 16)), seed=230, method="os", top=6, oversample=4))
    out.append(build("ca_13x262_r1", (13, 262), DC.draw(131, 1, (13, 262)), seed=231, method="ca", top=6, oversample=1))
    # one target exactly on a map cell, no noise but the rounding of y to float32: the fit stays within 1e-6 of a map cell
    out.append(build("on_cell", (8, 8), [one(on(11, 5), 1.0 + 0.5j)], seed=401, method="known", noise_var=0.0, known=[0.05]))
    # half a map cell off on both axes: four cells round the target tie but for the noise, a Newton step overshoots to the bound
    half = (on(11, 5)[0] + 0.5 / 16, on(11, 5)[1] + 0.5 / 16)
    out.append(build("half_cell", (8, 8), [one(half, 1.0 + 0.5j)], seed=402, method="known", noise_var=0.05))
    near = (on(11, 5)[0] + 0.4 / 16, on(11, 5)[1] + 0.4 / 16)
    out.append(build("near_bound", (8, 8), [one(near, 1.0 + 0.5j)], seed=403, method="known", noise_var=0.0, known=[0.05]))
    # cell (0, 0), the fit crossing tau = 0 and f = -1/2
    below = (1.0 - 0.3 / 16, 0.5 - 0.3 / 16)
    for method in ("ca", "os"):
        out.append(build(f"wraps_{method}", (8, 8), [one(below, 1.0 + 0.5j)], seed=404, method=method, noise_var=0.05))
    # two equal targets 1.5 resolution cells apart at 25 dB: plain CLEAN leaves a residue that is detected, two sweeps do not
    for sweeps in (0, 2):
        out.append(build(f"close_pair_sweeps_{sweeps}", (8, 8), [CLOSE], seed=410 + CLOSE_SEED, method="known", pfa=1e-4,
                         noise_var=10.0 ** -2.5, top=6, sweeps=sweeps))
    # the weaker target 10 dB down inside the stronger one's ring: cfar_targets with "ca" misses it
    out.append(from_detect("masked_pair_ca"))
    out.append(from_detect("masked_pair_os"))
    out.append(build("more_than_Le", (8, 8), [THREE], seed=303, top=1, noise_var=0.05))                   # Le = 1 too
    out.append(build("more_than_Le_2", (8, 8), [THREE], seed=303, top=2, noise_var=0.05, method="os"))
    # a 3 x 3 block of targets two resolution cells apart, the strongest in the middle with eight of them in its ring: under "ca" the
    # highest cell of the map is not over, the highest OVER cell is a corner of the block
    out.append(build("masked_centre", (8, 8), [BLOCK], seed=411, top=6, noise_var=0.05))
    out.append(build("Le_1", (8, 8), [one((0.37, 0.21), 1.0)], seed=405, top=1, noise_var=0.05, method="known"))
    out.append(from_detect("no_detection"))
    out.append(from_detect("silence"))
    out.append(build("on_grid_clean", (8, 8), [THREE], seed=406, noise_var=0.05, iters=0, sweeps=0))
    out.append(build("on_grid_sweeps", (8, 8), [THREE], seed=406, noise_var=0.05, iters=0, sweeps=1, method="known"))
    out.append(build("plain_clean", (8, 8), [THREE], seed=407, noise_var=0.05, sweeps=0, method="os"))
    out.append(build("one_step", (8, 8), [THREE], seed=408, noise_var=0.05, iters=1, sweeps=1, method="known"))
    # r = 1, half a cell off on both axes: beyond the inflection of the main lobe, the Hessian at the cell is not negative definite
    far = (on(5, 3, 1)[0] + 0.5 / 8, on(5, 3, 1)[1] + 0.5 / 8)
    out.append(build("not_definite", (8, 8), [one(far, 1.0 + 0.5j)], seed=409, method="known", oversample=1, noise_var=0.05))
    out.append(from_detect("nonfinite"))
    out.append(from_detect("symbols_given"))
    out.append(from_detect("known_noise_var"))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def host(c, i, **kw):
    pick = lambda v: None if v is None else v[i]  # noqa: E731
    nv = pick(c.noise_var)
    return detect.cfar_relax_host(c.y[i], c.b[i], c.grid, **{**c.kw, **dict(noise_var=None if nv is None else float(nv),
                                                                           symbols=pick(c.symbols), psk=PSK, exempt=c.exempt), **kw})


@functools.lru_cache(maxsize=None)
def reference(name):
    """``cfar_relax_host`` scene by scene.  Computed once per case."""
    c = case(name)
    return tuple(host(c, i) for i in range(len(c.y)))


def differences(c, i, r, rows, amp, level, resid, pmap):
    """(point, power, amp) of scene i against the mirror's result r, in the units of the module docstring."""
    Nb, Nd = c.grid
    E = max(float((np.abs(c.y[i].astype(np.complex128)) ** 2).sum()), 1e-300)
    n = r.n_det
    wrap = lambda d: np.abs(d - np.round(d))  # noqa: E731  a point a rounding error away from a wrap is as near
    point = max(float((wrap(rows[:n, 0] - r.rows[:n, 0]) * Nd).max(initial=0.0)),
                float((wrap(rows[:n, 1] - r.rows[:n, 1]) * Nb).max(initial=0.0)))
    power = max(float(np.abs(pmap - r.map).max()), float(np.abs(rows[:n, 2] - r.rows[:n, 2]).max(initial=0.0)),
                abs(float(level) - r.level), abs(float(resid) - r.resid) * Nb * Nd) / E
    return point, power, float(np.abs(amp[:n] - r.amp[:n]).max(initial=0.0)) / math.sqrt(E / (Nb * Nd))


def compare(name, rows, amp, n_det, more, maps, level, resid, state, pmap, what):
    """Decisions exactly (every scene of the table has the margin), numbers within the tolerances.  rows [B, Le, 3], amp [B, Le]
    complex, the rest [B], pmap [B, n_f, n_tau].  Returns the worst (point, power, amp) differences."""
    c, ref = case(name), reference(name)
    worst = (0.0, 0.0, 0.0)
    for i, r in enumerate(ref):
        assert r.margin > MARGIN, (what, name, i, r.margin)
        assert int(state[i]) == r.state == c.states[i], (what, name, i, int(state[i]), r.state)
        assert (int(n_det[i]), int(more[i]), int(maps[i])) == (r.n_det, r.more, r.maps), (what, name, i, int(n_det[i]), int(more[i]),
                                                                                         int(maps[i]), r.n_det, r.more, r.maps)
        if r.state != D_:
            assert r.n_det == 0 and np.isnan(level[i]) and np.isnan(resid[i]) and np.isnan(rows[i]).all() and np.isnan(pmap[i]).all()
            assert np.isnan(amp[i]).all()
            continue
        n = r.n_det
        assert np.isnan(rows[i][n:]).all() and np.isfinite(rows[i][:n]).all() and np.isnan(amp[i][n:]).all()
        assert ((rows[i][:n, 0] >= 0) & (rows[i][:n, 0] < 1) & (rows[i][:n, 1] >= -0.5) & (rows[i][:n, 1] < 0.5)).all()
        d = differences(c, i, r, rows[i], amp[i], level[i], resid[i], pmap[i])
        worst = tuple(max(a, v) for a, v in zip(worst, d))
        assert d[0] <= POINT_TOL and d[1] <= POWER_TOL and d[2] <= AMP_TOL, (what, name, i, d)
    return worst


# ---- Monte Carlo -----------------------------------------------------------------------------------------------------------------------
MC_GRID, MC_R, MC_DRAWS, MC_PFA, MC_LEFT_OUT = DC.MC_GRID, DC.MC_R, DC.MC_DRAWS, DC.MC_PFA, DC.MC_LEFT_OUT


def mc_host(y, b, noise_var, method):
    """(n_det, more, maps, margin) [draws] of ``cfar_relax_host`` on every scene."""
    res = [detect.cfar_relax_host(y[i], b[i], MC_GRID, top=6, oversample=MC_R, method=method, pfa=MC_PFA,
                                  noise_var=float(noise_var[i]) if method == "known" else None) for i in range(len(y))]
    return tuple(np.array([getattr(r, k) for r in res]) for k in ("n_det", "more", "maps", "margin"))
