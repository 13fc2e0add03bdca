"""The case table of the Cramer-Rao bound tests (no test in this module): tests/test_crb.py holds the host model and a second numpy
formulation to ``metrics.crb_host`` on it, tests/test_gpu_crb.py the kernel.

Truth is cast through float32 / complex64, as the generator returns it.  The allowed relative error of a bound is

    64 (P + Nb + Nd) kappa 2^-53,

kappa = the 2-norm condition number of the unit-diagonal information matrix from ``crb_host``, P its size: the sums over k < Nb, Nd
and the P-term recurrences of the factorisation each lose a few units in the last place times their length, the inverse amplifies
that by kappa.  ``separable`` is the kernel's formulation in numpy (power sums, Cholesky) with switches for ONE mistake each.
"""
import functools
from typing import NamedTuple

import numpy as np

from admm_net_amd import metrics

EPS = 2.0 ** -53
KAPPA_MAX = 1e9                # every case is below it or exactly degenerate: nothing sits near the 2^-40 pivot threshold


class Case(NamedTuple):
    name: str
    grid: tuple          # (Nb, Nd)
    tau: np.ndarray      # [B, Lt] float32
    f: np.ndarray        # [B, Lt] float32
    C: np.ndarray        # [B, Lt] complex64
    L_true: object       # None or [B] int64
    noise: dict          # {"snr_db": x} or {"noise_var": x}: a number or a [B] float64 array
    status: tuple        # the expected (outside, nonfinite, not positive definite)


def draw(seed, B, L, spread=None):
    """Truth drawn like ``synth.make_batch``; ``spread``: targets on a jittered lattice instead, so that many stay apart."""
    rng = np.random.default_rng(seed)
    if spread:
        side = int(np.ceil(np.sqrt(L)))
        cell = np.stack([rng.permutation(side * side)[:L] for _ in range(B)])
        tau = 0.1 + 0.8 * ((cell // side) + 0.5 + rng.uniform(-spread, spread, (B, L))) / side
        f = -0.4 + 0.8 * ((cell % side) + 0.5 + rng.uniform(-spread, spread, (B, L))) / side
    else:
        tau, f = rng.uniform(0.1, 0.9, (B, L)), rng.uniform(-0.4, 0.4, (B, L))
    C = rng.normal(0, 0.7, (B, L)) + 1j * rng.normal(0, 0.7, (B, L))
    return tau.astype(np.float32), f.astype(np.float32), C.astype(np.complex64)


def _pair(cells, grid=(10, 10)):
    """Two targets ``cells`` resolution cells apart on both axes."""
    tau = np.array([[0.4, 0.4 + cells / grid[1]]], dtype=np.float32)
    f = np.array([[-0.1, -0.1 + cells / grid[0]]], dtype=np.float32)
    C = np.array([[0.6 - 0.3j, -0.2 + 0.7j]], dtype=np.complex64)
    return tau, f, C


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda name, grid, truth, L_true=None, status=(0, 0, 0), **noise: out.append(  # noqa: E731
        Case(name, grid, *truth, None if L_true is None else np.asarray(L_true, dtype=np.int64), noise, status))
    add("L1_4x6", (4, 6), draw(1, 2, 1), snr_db=12.0)
    add("L1_6x4", (6, 4), draw(1, 2, 1), snr_db=12.0)
    add("L3_10x10", (10, 10), draw(2, 3, 3), snr_db=15.0)
    add("L3_16x16", (16, 16), draw(3, 3, 3), noise_var=0.02)
    add("L8_8x16", (8, 16), draw(4, 2, 8, spread=0.2), snr_db=20.0)
    add("L16_16x16", (16, 16), draw(5, 2, 16, spread=0.15), snr_db=10.0)
    add("1x12", (1, 12), draw(6, 2, 2), snr_db=10.0)
    add("12x1", (12, 1), draw(6, 2, 2), noise_var=0.1)
    add("1x1", (1, 1), draw(7, 2, 1), noise_var=0.5)
    add("26x131", (26, 131), draw(8, 2, 3), snr_db=5.0)
    add("pair_0.5_cells", (10, 10), _pair(0.5), snr_db=15.0)
    add("pair_0.1_cells", (10, 10), _pair(0.1), snr_db=15.0)
    add("pair_0.02_cells", (10, 10), _pair(0.02), snr_db=15.0)
    add("coincident_pair", (10, 10), _pair(0.0), status=(0, 0, 1), snr_db=15.0)
    tau, f, C = draw(9, 3, 3)
    C[1, 2] = 0.0
    add("zero_amplitude", (10, 10), (tau, f, C), status=(0, 0, 1), snr_db=15.0)
    tau, f, C = draw(10, 2, 2)
    C[0, 1] = 1e-11 * (1 + 1j)
    add("weak_target", (10, 10), (tau, f, C), noise_var=0.01)
    add("mixed_L_true", (8, 8), draw(11, 5, 4), L_true=[0, 1, 4, 2, 4], snr_db=np.array([5.0, 10.0, 15.0, 20.0, 25.0]))
    add("L_true_outside", (8, 8), draw(12, 3, 3), L_true=[3, 4, -1], status=(2, 0, 0), snr_db=15.0)
    tau, f, C = draw(13, 3, 3)
    tau[1, 0] = np.nan
    add("nan_truth", (8, 8), (tau, f, C), status=(0, 1, 0), snr_db=15.0)
    add("zero_noise_var", (8, 8), draw(14, 3, 2), status=(0, 1, 0), noise_var=np.array([0.1, 0.0, 0.1]))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def noise_of(c, i):
    (key, value), = c.noise.items()
    return {key: float(np.asarray(value).reshape(-1)[i] if np.ndim(value) else value)}


class Reference(NamedTuple):
    bound: np.ndarray     # [B, Lt, 2]
    status: tuple
    kappa: np.ndarray     # [B], NaN where nothing was inverted
    params: np.ndarray    # [B] P
    states: tuple         # per scene: -1 or the column of status


@functools.lru_cache(maxsize=None)
def reference(name, host=metrics.crb_host):
    """``crb_host`` scene by scene, with the batch semantics of ``metrics.crb`` around it.  Computed once per case."""
    c = case(name)
    B, Lt = c.tau.shape
    bound = np.full((B, Lt, 2), np.nan)
    kappa, params, states = np.full(B, np.nan), np.zeros(B, dtype=np.int64), []
    for i in range(B):
        L = Lt if c.L_true is None else int(c.L_true[i])
        if not 0 <= L <= Lt:
            states.append(0)
            continue
        r = host(c.tau[i, :L].astype(np.float64), c.f[i, :L].astype(np.float64), c.C[i, :L].astype(np.complex128), c.grid,
                 **noise_of(c, i))
        states.append(r.state)
        if r.state < 0:
            bound[i, :L] = r.bound
            kappa[i], params[i] = r.kappa, r.fisher.shape[0]
    return Reference(bound, tuple(sum(s == k for s in states) for k in range(3)), kappa, params, tuple(states))


def tolerance(name):
    """[B, 1, 1] allowed relative error of the bounds of each scene."""
    c, r = case(name), reference(name)
    return (64.0 * (r.params + sum(c.grid)) * np.nan_to_num(r.kappa) * EPS)[:, None, None]


def compare(name, bound, status, what):
    """Status counts, inf and NaN positions exactly; finite bounds within ``tolerance``.  Returns the worst error / tolerance."""
    r = reference(name)
    bound = np.asarray(bound, dtype=np.float64)
    assert tuple(int(v) for v in status) == r.status == case(name).status, (what, name, tuple(status), r.status)
    assert np.array_equal(np.isnan(bound), np.isnan(r.bound)) and np.array_equal(np.isinf(bound), np.isinf(r.bound)), (what, name)
    assert not (bound[np.isinf(bound)] < 0).any()
    fin = np.isfinite(r.bound)
    ratio = np.abs(bound[fin] - r.bound[fin]) / r.bound[fin] / np.broadcast_to(np.maximum(tolerance(name), 1e-300), bound.shape)[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (what, name, worst)
    return worst


def pool(bound, L_true, match):
    """totals [8] of ``metrics.crb`` from the per-target bounds on the host."""
    bound = np.asarray(bound, dtype=np.float64)
    B, Lt, _ = bound.shape
    L = np.full(B, Lt) if L_true is None else np.asarray(L_true)
    live = (np.arange(Lt)[None, :] < L[:, None]) & ((L >= 0) & (L <= Lt))[:, None]
    hit = live & (np.asarray(match) >= 0) if match is not None else np.zeros_like(live)
    out = []
    for mask in (live, hit):
        use = [mask & np.isfinite(bound[:, :, a]) for a in (0, 1)]
        out += [bound[:, :, a][use[a]].sum() for a in (0, 1)] + [float(use[a].sum()) for a in (0, 1)]
    return np.array(out)


# ---- the kernel's formulation in numpy, with one mistake at a time ----------------------------------------------------------------
MISTAKES = ("factor_2_dropped", "k_for_k_squared", "tau_sign", "Nb_Nd_exchanged", "no_scaling", "energy_per_target")


def power_sum(p, x, N):
    k = np.arange(N, dtype=np.float64)
    t = k * x
    return (k ** p * np.exp(2j * np.pi * (t - np.rint(t)))).sum()


def separable(tau, f, C, grid, *, snr_db=None, noise_var=None, mistake=None):
    """``crb_host``'s answer from the separable form: power sums per target pair, unit-diagonal scaling, Cholesky."""
    Nb, Nd = grid if mistake != "Nb_Nd_exchanged" else grid[::-1]
    tau, f, C = np.asarray(tau, np.float64), np.asarray(f, np.float64), np.asarray(C, np.complex128)
    L = len(tau)
    kinds = ([("tau", 0, 1)] if grid[1] > 1 else []) + ([("f", 1, 0)] if grid[0] > 1 else []) + [("re", 0, 0), ("im", 0, 0)]
    coef = {"tau": lambda l: -2j * np.pi * C[l], "f": lambda l: 2j * np.pi * C[l], "re": lambda l: 1.0, "im": lambda l: 1j}
    power = (lambda p: min(p, 1)) if mistake == "k_for_k_squared" else (lambda p: p)
    sign = 1.0 if mistake == "tau_sign" else -1.0
    P = len(kinds) * L
    G = np.zeros((P, P))
    energy = 0.0
    for l in range(L):
        for m in range(L):
            Sb = [power_sum(power(p), f[m] - f[l], Nb) for p in range(3)]
            St = [power_sum(power(q), sign * (tau[m] - tau[l]), Nd) for q in range(3)]
            if mistake != "energy_per_target" or l == m:
                energy += (np.conj(C[l]) * C[m] * Sb[0] * St[0]).real
            for a, (ka, pa, qa) in enumerate(kinds):
                for b, (kb, pb, qb) in enumerate(kinds):
                    G[a * L + l, b * L + m] = (np.conj(coef[ka](l)) * coef[kb](m) * Sb[pa + pb] * St[qa + qb]).real
    v = energy / (10.0 ** (snr_db / 10.0) * Nb * Nd) if noise_var is None else noise_var
    F = (1.0 if mistake == "factor_2_dropped" else 2.0) / v * G
    nan = np.full((L, 2), np.nan)
    g = np.diag(F)
    if not (g > 0).all():
        return nan
    d = np.ones(P) if mistake == "no_scaling" else 1.0 / np.sqrt(g)
    A = F * np.multiply.outer(d, d)
    R = A.copy()
    for j in range(P):
        if not R[j, j] >= metrics.PIVOT_MIN:
            return nan
        R[j + 1:, j + 1:] -= np.multiply.outer(R[j + 1:, j], R[j + 1:, j]) / R[j, j]
    Linv = np.linalg.solve(np.linalg.cholesky(A), np.eye(P))
    var = (Linv ** 2).sum(axis=0) * d * d
    bound = np.full((L, 2), np.inf)
    if grid[1] > 1:
        bound[:, 0] = var[:L]
    if grid[0] > 1:
        bound[:, 1] = var[L:2 * L] if grid[1] > 1 else var[:L]
    return bound
