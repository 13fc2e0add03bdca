"""Random scoring cases shared by tests/test_metrics.py (host) and tests/test_gpu_metrics.py (no test in this module).

Scenes are drawn like ``synth.make_batch`` (tau ~ U(0.1, 0.9), f ~ U(-0.4, 0.4), float32); the estimates of a signal are its
targets in a random order with N(0, 0.03) added, one in five of them replaced by a stray drawn like a target, strays filling the
rows beyond the targets; the rows are then shuffled (peak-search rows come in height order, not truth order).  ``CUTOFF`` = 0.1.
"""
import itertools

import numpy as np
import torch

from admm_net_amd import metrics
from admm_net_amd.synth import F_RANGE, TAU_RANGE

CUTOFF = 0.1
NOISE = 0.03


def draw(seed, B, Le, Lt, partial=True, absent=0.1):
    """(est [B, Le, 3] float64, tau_true, f_true [B, Lt] float32, L_true [B] int64).  ``partial``: L_true ~ U{1 .. Lt} (every
    seventh signal keeps all Lt); ``absent``: the share of estimate rows turned into the NaN rows ``peak_top`` pads with."""
    rng = np.random.default_rng(seed)
    tt = rng.uniform(*TAU_RANGE, size=(B, Lt)).astype(np.float32)
    ft = rng.uniform(*F_RANGE, size=(B, Lt)).astype(np.float32)
    L = rng.integers(1, Lt + 1, size=B) if partial else np.full(B, Lt)
    L[::7] = Lt
    est = np.stack([rng.uniform(*TAU_RANGE, size=(B, Le)), rng.uniform(*F_RANGE, size=(B, Le)), rng.uniform(size=(B, Le))], axis=2)
    for b in range(B):
        k = min(Le, int(L[b]))
        pick = rng.permutation(int(L[b]))[:k]
        keep = rng.random(k) < 0.8
        est[b, :k, 0][keep] = (tt[b, pick] + rng.normal(0, NOISE, k))[keep]
        est[b, :k, 1][keep] = (ft[b, pick] + rng.normal(0, NOISE, k))[keep]
    order = rng.random((B, Le)).argsort(axis=1)
    est = np.take_along_axis(est, order[:, :, None], axis=1)
    if absent and Le > 1:
        est[rng.random((B, Le)) < absent] = np.nan
    return est, tt, ft, L.astype(np.int64)


def host_batch(est, tt, ft, L, n_est=None, cutoff=CUTOFF, with_gap=False, **kw):
    """``metrics.match_host`` signal by signal: (match [B, Lt] int32, stats [B, 8], gaps [B] or None)."""
    B, Lt = tt.shape
    match = np.full((B, Lt), -1, dtype=np.int32)
    stats = np.zeros((B, 8))
    gaps = np.full(B, np.inf) if with_gap else None
    for b in range(B):
        n = est.shape[1] if n_est is None else int(np.clip(n_est[b], 0, est.shape[1]))
        out = metrics.match_host(est[b, :n, 0], est[b, :n, 1], tt[b, :L[b]], ft[b, :L[b]], cutoff=cutoff, with_gap=with_gap, **kw)
        match[b, :L[b]], stats[b] = out[0], out[1]
        if with_gap:
            gaps[b] = out[2]
    return match, stats, gaps


def cost_matrix(est_b, tt_b, ft_b, cutoff=CUTOFF, **kw):
    """(rows of est_b that are present, their truncated cost matrix [ne, nt], d2)."""
    live = np.flatnonzero(np.isfinite(est_b[:, 0]) & np.isfinite(est_b[:, 1]))
    _, _, d2 = metrics.pair_terms(est_b[live, 0], est_b[live, 1], tt_b, ft_b, **kw)
    return live, np.minimum(d2, cutoff * cutoff), d2


def brute_cost(cost):
    """The least cost over every assignment of the smaller side, by a plain loop."""
    ne, nt = cost.shape
    if min(ne, nt) == 0:
        return 0.0
    c = cost if ne <= nt else cost.T
    k, m = c.shape
    return min(sum(c[i, p[i]] for i in range(k)) for p in itertools.permutations(range(m), k))


def scipy_cost(cost):
    from scipy.optimize import linear_sum_assignment
    if min(cost.shape) == 0:
        return 0.0
    r, c = linear_sum_assignment(cost)
    return float(cost[r, c].sum())


def greedy_cost(cost):
    """Nearest neighbour: the cheapest free pair again and again."""
    c = cost.copy()
    total = 0.0
    for _ in range(min(c.shape)):
        i, j = np.unravel_index(np.argmin(c), c.shape)
        total += c[i, j]
        c[i, :] = np.inf
        c[:, j] = np.inf
    return total


def cost_of_match(match_b, stats_b, est_b, tt_b, ft_b, cutoff=CUTOFF, **kw):
    """The truncated cost of the assignment a ``match`` row stands for: its hits at d2, the other matched pairs at c^2."""
    n_est, n_true = int(stats_b[0] + stats_b[2]), int(stats_b[0] + stats_b[1])
    hits = [(int(e), j) for j, e in enumerate(match_b) if e >= 0]
    _, _, d2 = metrics.pair_terms(est_b[[e for e, _ in hits], 0], est_b[[e for e, _ in hits], 1], tt_b[[j for _, j in hits]],
                                  ft_b[[j for _, j in hits]], **kw) if hits else (None, None, np.zeros((0, 0)))
    return float(np.diag(d2).sum()) + cutoff * cutoff * (min(n_est, n_true) - len(hits)), np.diag(d2)


def train_py_loop(tau_est, f_est, tau_true, f_true, L_true):
    """train.py:262-274 and :279-280, literally (float32 tensors)."""
    tau_errors, f_errors = [], []
    for i in range(len(L_true)):
        L = L_true[i].item()
        if L > 0:
            tau_error = torch.sqrt(torch.mean((tau_est[i, :L] - tau_true[i, :L]) ** 2)).item()
            f_error = torch.sqrt(torch.mean((f_est[i, :L] - f_true[i, :L]) ** 2)).item()
            tau_errors.append(tau_error)
            f_errors.append(f_error)
    return (np.mean(tau_errors) if len(tau_errors) > 0 else 0, np.mean(f_errors) if len(f_errors) > 0 else 0, tau_errors, f_errors)


def ordered_case(seed, B, Lmax, zero_only=False):
    g = torch.Generator().manual_seed(seed)
    te, fe, tt, ft = (torch.rand(B, Lmax, generator=g) - off for off in (0.0, 0.5, 0.0, 0.5))
    L = torch.zeros(B, dtype=torch.int64) if zero_only else torch.randint(0, Lmax + 1, (B,), generator=g)
    return te, fe, tt, ft, L
