"""Target estimates scored against ground truth on the device (csrc/score.hip), in place of a host loop over the samples.

The reference compares estimates with the truth in two places, both per-sample host loops: train.py:262-274 and :388-408 (the
validation / test RMSE of ``ADMMNet``, three ``.item()`` reads per sample) and test/test_model_peaksearch.py:85-97, which sorts
and cuts the peaks of ``phi`` and of ``phi_true`` and then only prints them -- peak-search rows come in height order, not truth
order, so comparing them needs an assignment, and that part was never written.

``match_targets``  one optimal assignment per signal.  All in float64: with the present estimates i and the targets j,

        d2_ij = (sx dtau_ij)^2 + (sy df_ij)^2,   dtau, df wrapped into [-P/2, P/2) where a period P is given,

    the assignment matches k = min(n_est, n_true) pairs and minimises sum min(d2, c^2); a matched pair with d2 < c^2 is a HIT and
    no other pair is reported.  This is the GOSPA assignment (alpha = 2, p = 2).  The truncation belongs inside the cost that is
    minimised: solving without it and gating afterwards gives another, wrong answer (estimates 0.26, 0.33 against targets 0.20,
    0.27 with c = 0.05: the one hit is 0.26 on 0.27, while the untruncated optimum pairs 0.26 with 0.20 and 0.33 with 0.27 and
    gating it leaves nothing).
``ordered_rmse``   the reference's RMSE, slot j against slot j (``ADMMNet``'s head is trained in truth order under
                   ``BasicANMLoss``; one trained with ``losses.SetANMLoss`` has no slot order and is scored by
                   ``ADMMNet.evaluate_head``, an assignment with the count taken from the confidences).
``summary``        the one host read: detection probability, false alarms, pooled RMSE and GOSPA of a batch.
``order_counts``   scenes whose selected number of targets lies below, at and above the true one, without a host read.
``match_host``     the float64 numpy statement of ``match_targets`` for one signal.  The tests hold the kernel to it; it is NOT a
                   fallback -- the device calls raise without the HIP library.
``crb``            the Cramer-Rao bound of every target of every scene (csrc/crb.hip), the yardstick of the pooled RMSE;
``crb_summary``    its one host read; ``crb_host`` the float64 numpy statement for one scene (a test yardstick, no fallback).

Tensor inputs follow INTEGRATION.md section 3: every pointer is taken through ``ops._f32`` / ``ops._num`` (``ops._plain``).
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops

STATS = ("n_hit", "n_miss", "n_false", "sum_dtau2", "sum_df2", "sum_d2", "gospa2", "cost")
MAX_ROWS = 64
BRUTE_MIN = 6               # match_host enumerates every assignment where min(n_est, n_true) <= BRUTE_MIN ...
BRUTE_ASSIGNMENTS = 300_000   # ... and there are at most this many (64 x 3 has 249 984); scipy's solver above that


class MatchResult(NamedTuple):
    match: torch.Tensor    # [B, Lt] int32: the index of the estimate that hit target j, else -1
    stats: torch.Tensor    # [B, 8] float64, the columns of STATS; NaN for a signal counted in status
    totals: torch.Tensor   # [8] float64: the column sums of stats over the signals that were scored
    status: torch.Tensor   # [2] int32: signals with L_true outside [0, Lt], signals with a non-finite truth


def _options(cutoff, scale, period):
    try:
        sx, sy = (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError(f"scale must be a pair of numbers (tau, f), got {scale!r}") from None
    if period is None:
        period = (0.0, 0.0)
    try:
        pt, pf = (0.0 if v is None else float(v) for v in period)
    except (TypeError, ValueError):
        raise ValueError(f"period must be None or a pair (tau, f) of numbers or None, got {period!r}") from None
    c = float(cutoff)
    if not (sx > 0 and sy > 0 and math.isfinite(sx) and math.isfinite(sy)):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    if not (c > 0 and math.isfinite(c) and math.isfinite(c * c)):
        raise ValueError(f"cutoff must be positive and finite, got {cutoff!r}")
    if not (pt >= 0 and pf >= 0 and math.isfinite(pt) and math.isfinite(pf)):
        raise ValueError(f"a period must be 0 (none) or positive and finite, got {period!r}")
    return sx, sy, c, pt, pf


def _integers(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold integers, got {t.dtype}")


def _partials(lib, B, dev):
    need = lib.admmnet_score_partials(B)
    if need < 0:
        raise _lib.AdmmNetError(f"score: bad size (B={B})")
    return torch.empty(need, dtype=torch.float64, device=dev)


def match_targets(est, tau_true, f_true, L_true=None, n_est=None, *, cutoff, scale=(1.0, 1.0), period=None) -> MatchResult:
    """One optimal assignment of estimates to targets per signal (the module docstring has the definition), in one kernel and
    without a host read.

    est       [B, Le, 3] rows (tau, f, height) as ``ops.peak_top`` returns them -- the height is ignored, a row whose tau or f is
              not finite is absent (``peak_top`` pads with NaN) -- or a pair (tau_est, f_est) of [B, Le] tensors, as ``ADMMNet``
              returns them.  1 <= Le <= 64.
    tau_true, f_true   [B, Lt], 1 <= Lt <= 64;  L_true: None (every slot is a target) or [B] integers.
    n_est     None or [B] integers: only the first n_est rows count (held to 0 .. Le).
    cutoff    c > 0; scale = (sx, sy) > 0; period: None, or (P_tau, P_f) with 0 / None for an axis that does not wrap.
    """
    pair = isinstance(est, (tuple, list))
    tensors = list(est) if pair else [est]
    if pair and len(tensors) != 2:
        raise ValueError(f"est must be [B, Le, 3] rows or a pair (tau_est, f_est), got {len(tensors)} tensors")
    for t, name in zip(tensors + [tau_true, f_true], (["tau_est", "f_est"] if pair else ["est"]) + ["tau_true", "f_true"]):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    opts = (ctypes.c_double * 5)(*_options(cutoff, scale, period))
    lib = _lib.load()
    dev = tau_true.device
    if tau_true.dim() != 2:
        raise ValueError(f"tau_true must be [B, Lt], got {tuple(tau_true.shape)}")
    B, Lt = tau_true.shape
    shape = tuple(tensors[0].shape)
    if (len(shape) != 2 if pair else len(shape) != 3 or shape[2] != 3) or shape[0] != B:
        raise ValueError(f"est must be [{B}, Le, 3] rows or a pair of [{B}, Le] tensors, got {shape}")
    Le = shape[1]
    if not (1 <= Le <= MAX_ROWS and 1 <= Lt <= MAX_ROWS and B >= 1):
        raise ValueError(f"match_targets needs 1 <= Le, Lt <= {MAX_ROWS} and B >= 1, got Le={Le}, Lt={Lt}, B={B}")
    with torch.cuda.device(dev):
        if pair:
            te, fe = (ops._num(t, dev, torch.float64, (B, Le), name) for t, name in zip(tensors, ("tau_est", "f_est")))
            rows = torch.stack((te, fe, torch.zeros_like(te)), dim=2)
        else:
            rows = ops._num(est, dev, torch.float64, (B, Le, 3), "est")
        tau_true, f_true = ops._f32(tau_true, dev, (B, Lt), "tau_true"), ops._f32(f_true, dev, (B, Lt), "f_true")
        if L_true is not None:
            _integers(L_true, "L_true")
            L_true = ops._num(L_true, dev, torch.int64, (B,), "L_true")
        if n_est is not None:
            _integers(n_est, "n_est")
            n_est = ops._num(n_est, dev, torch.int32, (B,), "n_est")
        match = torch.empty(B, Lt, dtype=torch.int32, device=dev)
        stats = torch.empty(B, len(STATS), dtype=torch.float64, device=dev)
        totals = torch.empty(len(STATS), dtype=torch.float64, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        part = _partials(lib, B, dev)
        _lib.check(lib.admmnet_score_match_f64(Le, Lt, B, ops._ptr(rows), ops._ptr(n_est), ops._ptr(tau_true), ops._ptr(f_true),
                                               ops._ptr(L_true), opts, ops._ptr(match), ops._ptr(stats), ops._ptr(totals),
                                               ops._ptr(status), ops._ptr(part), ops._stream(dev)), "admmnet_score_match_f64")
    return MatchResult(match, stats, totals, status)


def ordered_rmse(tau_est, f_est, tau_true, f_true, L_true):
    """The validation RMSE of train.py:262-274 (and :388-408) without its loop: for L = L_true[b] > 0,
    sqrt(mean_{j<L} (tau_est - tau_true)^2) and the same for f, in float64 from the float32 values.

    tau_est, f_est, tau_true, f_true [B, Lmax] (1 <= Lmax <= 64), L_true [B] integers.  Returns (per_sample [B, 2] float64, NaN
    where L = 0; out [3] float64 = the mean of each column over the signals with L > 0 -- ``np.mean`` of the reference's two
    lists, 0 when they are empty -- and their count; status [1] int32 = signals whose L_true lies outside [0, Lmax], evaluated
    with L held to it).  No host read."""
    names = ("tau_est", "f_est", "tau_true", "f_true")
    for t, name in zip((tau_est, f_est, tau_true, f_true, L_true), names + ("L_true",)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    _integers(L_true, "L_true")
    if tau_est.dim() != 2:
        raise ValueError(f"tau_est must be [B, Lmax], got {tuple(tau_est.shape)}")
    lib = _lib.load()
    dev = tau_est.device
    B, Lmax = tau_est.shape
    if not (1 <= Lmax <= MAX_ROWS and B >= 1):
        raise ValueError(f"ordered_rmse needs 1 <= Lmax <= {MAX_ROWS} and B >= 1, got Lmax={Lmax}, B={B}")
    with torch.cuda.device(dev):
        real = [ops._f32(t, dev, (B, Lmax), name) for t, name in zip((tau_est, f_est, tau_true, f_true), names)]
        L_true = ops._num(L_true, dev, torch.int64, (B,), "L_true")
        per_sample = torch.empty(B, 2, dtype=torch.float64, device=dev)
        out = torch.empty(3, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        part = _partials(lib, B, dev)
        _lib.check(lib.admmnet_score_ordered_f32(Lmax, B, *(ops._ptr(t) for t in real), ops._ptr(L_true), ops._ptr(per_sample),
                                                 ops._ptr(out), ops._ptr(status), ops._ptr(part), ops._stream(dev)),
                   "admmnet_score_ordered_f32")
    return per_sample, out, status


def summary(totals, signals=None, extra=None) -> dict:
    """The figures of a batch from ``match_targets``' totals, with ONE device-to-host read.

    totals: a ``MatchResult`` -- the signals that were scored are then its batch less the two counts of ``status`` -- or the [8]
    tensor itself (or a sum of several) with ``signals`` given.  Returns a dict: ``pd`` = hits / (hits + misses),
    ``false_per_signal``, ``rmse_tau`` / ``rmse_f`` pooled over the hits (NaN without a hit; the wrapped, unscaled differences),
    ``gospa`` = sqrt(mean gospa^2), ``signals``, and the three counts.  ``extra`` (with a ``MatchResult``): a dict of device
    tensors that travel in the same read and come back under their names, as a float or a list of floats."""
    if isinstance(totals, MatchResult):
        if signals is not None:
            raise ValueError("signals is taken from the MatchResult")
        more = {k: v.to(device=totals.totals.device, dtype=torch.float64).reshape(-1) for k, v in (extra or {}).items()}
        t = torch.cat((totals.totals.reshape(-1), totals.status.to(torch.float64).reshape(-1), *more.values())).tolist()   # the read
        signals = totals.stats.shape[0] - int(t[8]) - int(t[9])
    else:
        if extra is not None:
            raise ValueError("extra= goes with a MatchResult")
        if signals is None:
            raise ValueError("summary of a bare totals tensor needs signals=")
        t = torch.as_tensor(totals).reshape(-1).to(torch.float64).tolist()                                   # the read
        if len(t) != len(STATS):
            raise ValueError(f"totals must have {len(STATS)} entries, got {len(t)}")
        signals = int(signals)
    hit, miss, false = t[0], t[1], t[2]
    nan = float("nan")
    line = {"pd": hit / (hit + miss) if hit + miss > 0 else nan,
            "false_per_signal": false / signals if signals > 0 else nan,
            "rmse_tau": math.sqrt(t[3] / hit) if hit > 0 else nan,
            "rmse_f": math.sqrt(t[4] / hit) if hit > 0 else nan,
            "gospa": math.sqrt(t[6] / signals) if signals > 0 else nan,
            "signals": signals, "hits": int(hit), "misses": int(miss), "false_alarms": int(false)}
    at = 10
    for k, v in (more.items() if isinstance(totals, MatchResult) else ()):
        line[k] = t[at] if v.numel() == 1 else t[at:at + v.numel()]
        at += v.numel()
    return line


def order_counts(n_sel, L_true) -> torch.Tensor:
    """How a selected number of targets compares with the true one: [3] int64 on the device = the scenes with ``n_sel`` <, ==, >
    ``L_true`` ([B] integer tensors, e.g. ``order.select_targets(...).n_sel`` and ``make_scenes_device``'s ``L_true``).
    Comparisons and sums only: no host read."""
    _integers(n_sel, "n_sel")
    _integers(L_true, "L_true")
    if n_sel.dim() != 1 or n_sel.shape != L_true.shape:
        raise ValueError(f"order_counts needs two [B] tensors, got {tuple(n_sel.shape)} and {tuple(L_true.shape)}")
    L_true = L_true.to(n_sel.device)
    return torch.stack(((n_sel < L_true).sum(), (n_sel == L_true).sum(), (n_sel > L_true).sum()))


# ---- the float64 host statement ----------------------------------------------------------------------------------------------
def _wrap(d, P):
    return d - P * np.floor(d / P + 0.5) if P > 0 else d


def pair_terms(tau_est, f_est, tau_true, f_true, scale=(1.0, 1.0), period=None):
    """(dtau, df, d2), each [ne, nt] float64: estimate i against target j, as the kernel forms them (every product rounded on
    its own)."""
    sx, sy, _, pt, pf = _options(1.0, scale, period)
    te, fe = (np.asarray(v, dtype=np.float64).reshape(-1, 1) for v in (tau_est, f_est))
    tt, ft = (np.asarray(v, dtype=np.float64).reshape(1, -1) for v in (tau_true, f_true))
    with np.errstate(over="ignore", invalid="ignore"):
        dtau, df = _wrap(te - tt, pt), _wrap(fe - ft, pf)
        a, b = sx * dtau, sy * df
        return dtau, df, a * a + b * b


@functools.lru_cache(maxsize=32)
def _arrangements(m, k):
    """Every ordered choice of k out of m columns, [m! / (m - k)!, k]."""
    return np.array(list(itertools.permutations(range(m), k)), dtype=np.int64).reshape(-1, k)


def match_host(tau_est, f_est, tau_true, f_true, *, cutoff, scale=(1.0, 1.0), period=None, with_gap=False):
    """``match_targets`` for ONE signal in float64 numpy: estimates (1-d, a non-finite tau or f = absent) against targets (1-d,
    all of them count).  Enumerates every assignment where min(n_est, n_true) <= 6 and there are at most 300 000 of them, and
    calls ``scipy.optimize.linear_sum_assignment`` on the truncated cost matrix above that.

    Returns (match [n_true] int32, stats [8] float64); with ``with_gap=True`` (enumeration only) also the relative distance
    between the optimal cost and the least cost of an assignment with ANOTHER set of hits (inf if there is none): where it is
    tiny, two hit sets are both optimal to rounding and a comparison of ``match`` says nothing."""
    sx, sy, c, pt, pf = _options(cutoff, scale, period)
    c2 = c * c
    te, fe = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tau_est, f_est))
    tt, ft = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tau_true, f_true))
    if te.shape != fe.shape or tt.shape != ft.shape:
        raise ValueError("tau and f must have one length per side")
    if not (np.isfinite(tt).all() and np.isfinite(ft).all()):
        raise ValueError("a target is not finite")
    live = np.flatnonzero(np.isfinite(te) & np.isfinite(fe))
    ne, nt = len(live), len(tt)
    dtau, df, d2 = pair_terms(te[live], fe[live], tt, ft, (sx, sy), (pt, pf))
    hit = d2 < c2
    cost = np.where(hit, d2, c2)
    k, m = min(ne, nt), max(ne, nt)
    gap = math.inf
    brute = k <= BRUTE_MIN and math.perm(m, k) <= BRUTE_ASSIGNMENTS
    if with_gap and not brute:
        raise ValueError(f"with_gap needs the enumeration ({ne} x {nt} is solved by scipy)")
    if k == 0:
        pairs = np.zeros((0, 2), dtype=np.int64)
    elif brute:
        by_rows = cost if ne <= nt else cost.T                     # rows = the smaller side
        hits_rows = hit if ne <= nt else hit.T
        P = _arrangements(m, k)
        r = np.arange(k)
        total = by_rows[r, P].sum(axis=1)
        best = int(np.argmin(total))
        if with_gap:
            key = (np.where(hits_rows[r, P], P + 1, 0) * (m + 1) ** r).sum(axis=1)
            other = total[key != key[best]]
            if other.size:
                gap = float((other.min() - total[best]) / total[best]) if total[best] > 0 else math.inf
        pairs = np.stack((r, P[best]), axis=1) if ne <= nt else np.stack((P[best], r), axis=1)
    else:
        from scipy.optimize import linear_sum_assignment
        pairs = np.stack(linear_sum_assignment(cost), axis=1)
    match = np.full(nt, -1, dtype=np.int32)
    s_tau = s_f = s_d2 = 0.0
    n_hit = 0
    for i, j in pairs:
        if hit[i, j]:
            match[j] = live[i]
            n_hit += 1
            s_tau += dtau[i, j] ** 2
            s_f += df[i, j] ** 2
            s_d2 += d2[i, j]
    miss, false = nt - n_hit, ne - n_hit
    stats = np.array([n_hit, miss, false, s_tau, s_f, s_d2, s_d2 + 0.5 * c2 * (miss + false), s_d2 + c2 * (k - n_hit)],
                     dtype=np.float64)
    return (match, stats, gap) if with_gap else (match, stats)


def ordered_rmse_host(tau_est, f_est, tau_true, f_true, L_true):
    """``ordered_rmse`` in float64 numpy, without a loop: (per_sample [B, 2], out [3])."""
    te, fe, tt, ft = (np.asarray(v, dtype=np.float64) for v in (tau_est, f_est, tau_true, f_true))
    L = np.clip(np.asarray(L_true, dtype=np.int64), 0, te.shape[1])
    mask = np.arange(te.shape[1])[None, :] < L[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.stack([np.sqrt(np.where(mask, (a - b) ** 2, 0.0).sum(axis=1) / L) for a, b in ((te, tt), (fe, ft))], axis=1)
    per[L == 0] = np.nan
    n = int((L > 0).sum())
    out = np.array([per[L > 0, 0].mean() if n else 0.0, per[L > 0, 1].mean() if n else 0.0, float(n)])
    return per, out


# ---- the Cramer-Rao bound of a scene ---------------------------------------------------------------------------------------------
MAX_TARGETS = 16                 # crb: 4 parameters per target, one lane each
PIVOT_MIN = 2.0 ** -40           # a pivot of the unit-diagonal Cholesky below this: not positive definite


class CrbResult(NamedTuple):
    bound: torch.Tensor    # [B, Lt, 2] float64: the variance bound of tau_j and of f_j; +inf on an axis of length 1, NaN past L_true
    totals: torch.Tensor   # [8] float64: sum tau, sum f, count tau, count f over j < L_true; the same four over match >= 0
    status: torch.Tensor   # [3] int32 scenes: L_true outside [0, Lt]; non-finite input or noise; not positive definite


def _noise(snr_db, noise_var, B, dev):
    if (snr_db is None) == (noise_var is None):
        raise ValueError("crb needs exactly one of snr_db= and noise_var=")
    value, name = (snr_db, "snr_db") if noise_var is None else (noise_var, "noise_var")
    if isinstance(value, torch.Tensor):
        if value.is_complex() or value.dtype == torch.bool:
            raise ValueError(f"{name} must hold real numbers, got {value.dtype}")
        ops._need_cuda(value, name)
        return ops._num(value, dev, torch.float64, (B,), name), noise_var is None
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise TypeError(f"{name} must be a number or a [B] tensor, got {type(value).__name__}") from None
    return torch.full((B,), value, dtype=torch.float64, device=dev), noise_var is None


def crb(tau_true, f_true, C, grid, *, snr_db=None, noise_var=None, L_true=None, match=None) -> CrbResult:
    """The Cramer-Rao bound of the targets of every scene, in one kernel and without a host read.

    Scene model (``synth.make_batch``), grid = (Nb, Nd) = the (M, N) of a model, D = Nb Nd:

        mu[i_b Nd + i_d] = s[i] sum_l C_l exp(j 2 pi (i_b f_l - i_d tau_l)),  |s[i]| = 1 (PSK),     y = mu + w,  w ~ CN(0, v).

    theta = (tau_1..L, f_1..L, Re C_1..L, Im C_1..L); the information matrix is F = (2 / v) Re(J^H J), J = d mu / d theta, and the
    bound of target l is [F^-1] at the diagonal entries of tau_l and f_l.  This is the bound of a receiver that KNOWS the
    transmitted symbols s: with |s| = 1 they drop out of J^H J.  The network only knows the demodulated ``b``, so for it the
    figure is a lower bound, not one it could reach.

    tau_true, f_true [B, Lt], C [B, Lt] complex (1 <= Lt <= 16); L_true: None (every slot is a target) or [B] integers.
    Exactly one of ``snr_db`` (the generator's definition, v = sum |mu|^2 / (10^(snr / 10) D)) and ``noise_var`` (v itself), as a
    number or a [B] tensor.  match: None or a ``MatchResult.match`` ([B, Lt] int32), for the totals over the hits.

    An axis of length 1 carries no information about its parameter: the bound is +inf and is left out of sums and counts.  A scene
    whose unit-diagonal F is not positive definite (coincident targets, C_l = 0) has NaN bounds and is counted in ``status[2]``."""
    for t, name in ((tau_true, "tau_true"), (f_true, "f_true"), (C, "C")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    try:
        Nb, Nd = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"grid must be a pair (Nb, Nd), got {grid!r}") from None
    if tau_true.dim() != 2:
        raise ValueError(f"tau_true must be [B, Lt], got {tuple(tau_true.shape)}")
    if not C.is_complex():
        raise ValueError(f"C must be complex, got {C.dtype}")
    lib = _lib.load()
    dev = tau_true.device
    B, Lt = tau_true.shape
    if not (1 <= Lt <= MAX_TARGETS and B >= 1 and Nb >= 1 and Nd >= 1):
        raise ValueError(f"crb needs 1 <= Lt <= {MAX_TARGETS}, B >= 1 and a grid of at least 1 x 1, got Lt={Lt}, B={B}, grid={grid!r}")
    with torch.cuda.device(dev):
        noise, is_snr = _noise(snr_db, noise_var, B, dev)
        tau_true, f_true = ops._f32(tau_true, dev, (B, Lt), "tau_true"), ops._f32(f_true, dev, (B, Lt), "f_true")
        C = ops._c64(C, dev, (B, Lt), "C")
        if L_true is not None:
            _integers(L_true, "L_true")
            L_true = ops._num(L_true, dev, torch.int64, (B,), "L_true")
        if match is not None:
            _integers(match, "match")
            ops._need_cuda(match, "match")
            match = ops._num(match, dev, torch.int32, (B, Lt), "match")
        need = lib.admmnet_crb_partials(B)
        if need < 0:
            raise _lib.AdmmNetError(f"crb: bad size (B={B})")
        part = torch.empty(need, dtype=torch.float64, device=dev)
        bound = torch.empty(B, Lt, 2, dtype=torch.float64, device=dev)
        totals = torch.empty(8, dtype=torch.float64, device=dev)
        status = torch.empty(3, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_crb_f64(Nb, Nd, Lt, B, ops._ptr(tau_true), ops._ptr(f_true), ops._ptr(C), ops._ptr(L_true),
                                       ops._ptr(match), ops._ptr(noise), int(is_snr), ops._ptr(bound), ops._ptr(totals),
                                       ops._ptr(status), ops._ptr(part), ops._stream(dev)), "admmnet_crb_f64")
    return CrbResult(bound, totals, status)


def crb_summary(result) -> dict:
    """The figures of a batch from ``crb``'s totals, with ONE device-to-host read: root-mean bounds, to be held against the pooled
    RMSE of ``summary``.  ``crb_tau`` / ``crb_f`` = sqrt(mean bound) over the targets j < L_true, ``crb_tau_hits`` / ``crb_f_hits``
    over the targets with ``match >= 0`` -- the pool of ``summary``'s ``rmse_tau`` / ``rmse_f`` -- (NaN for an empty pool), the four
    counts, and the three scene counts of ``status``."""
    if not isinstance(result, CrbResult):
        raise TypeError(f"crb_summary takes a CrbResult, got {type(result).__name__}")
    t = torch.cat((result.totals.reshape(-1), result.status.to(torch.float64).reshape(-1))).tolist()   # the read
    root = lambda s, n: math.sqrt(s / n) if n > 0 else float("nan")  # noqa: E731
    return {"crb_tau": root(t[0], t[2]), "crb_f": root(t[1], t[3]), "crb_tau_hits": root(t[4], t[6]), "crb_f_hits": root(t[5], t[7]),
            "targets_tau": int(t[2]), "targets_f": int(t[3]), "hits_tau": int(t[6]), "hits_f": int(t[7]),
            "outside": int(t[8]), "nonfinite": int(t[9]), "not_positive_definite": int(t[10])}


class CrbHost(NamedTuple):
    bound: np.ndarray      # [L, 2] float64
    state: int             # -1: bounded; 1: non-finite input or noise; 2: not positive definite (the columns of ``status``)
    noise_var: float
    kappa: float           # the 2-norm condition number of the unit-diagonal information matrix
    jacobian: np.ndarray   # [D, P] complex: d mu / d theta, the columns of an axis of length 1 left out
    fisher: np.ndarray     # [P, P]


def crb_signal(tau, f, C, grid):
    """mu [Nb Nd] of the scene model with s = 1, from ``synth.steering``."""
    from .synth import steering
    Nb, Nd = grid
    tau, f, C = (np.asarray(v).reshape(-1) for v in (tau, f, C))
    return np.einsum("l,li,lj->ij", C.astype(np.complex128), steering(f.astype(np.float64), Nb),
                     np.conj(steering(tau.astype(np.float64), Nd))).reshape(Nb * Nd)


def crb_host(tau, f, C, grid, *, snr_db=None, noise_var=None) -> CrbHost:
    """``crb`` for ONE scene in float64 numpy (all L targets count), written the other way round: the explicit D x P Jacobian with
    ``np.exp``, F = (2 / v) Re(J^H J), ``np.linalg.inv`` of the unit-diagonal matrix.  The tests hold the kernel to it; it is NOT
    a fallback."""
    if (snr_db is None) == (noise_var is None):
        raise ValueError("crb_host needs exactly one of snr_db= and noise_var=")
    Nb, Nd = (int(v) for v in grid)
    tau, f = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tau, f))
    C = np.asarray(C, dtype=np.complex128).reshape(-1)
    L, D = len(tau), Nb * Nd
    nan = np.full((L, 2), np.nan)
    empty = CrbHost(nan, -1, float("nan"), float("nan"), np.zeros((D, 0), dtype=np.complex128), np.zeros((0, 0)))
    given = float(snr_db if noise_var is None else noise_var)
    if not (np.isfinite(tau).all() and np.isfinite(f).all() and np.isfinite(C).all() and math.isfinite(given)) or \
            (noise_var is not None and not given > 0):
        return empty._replace(state=1)
    if L == 0:
        return empty
    ib, idd = np.divmod(np.arange(D), Nd)
    E = np.exp(2j * np.pi * (np.multiply.outer(ib, f) - np.multiply.outer(idd, tau)))          # [D, L]
    v = float((np.abs(E @ C) ** 2).sum() / (10.0 ** (given / 10.0) * D)) if noise_var is None else given
    if not (v > 0 and math.isfinite(v)):
        return empty._replace(state=1, noise_var=v)
    cols = ([-2j * np.pi * idd[:, None] * C * E] if Nd > 1 else []) + ([2j * np.pi * ib[:, None] * C * E] if Nb > 1 else []) + [E, 1j * E]
    J = np.concatenate(cols, axis=1)
    F = (2.0 / v) * (J.conj().T @ J).real
    out = empty._replace(noise_var=v, jacobian=J, fisher=F)
    g = np.diag(F)
    if not (np.isfinite(F).all() and (g > 0).all()):
        return out._replace(state=2)
    d = 1.0 / np.sqrt(g)
    A = F * np.multiply.outer(d, d)
    np.fill_diagonal(A, 1.0)
    R = A.copy()                                            # the pivots of its Cholesky, by elimination
    for j in range(len(R)):
        if not R[j, j] >= PIVOT_MIN:
            return out._replace(state=2)
        R[j + 1:, j + 1:] -= np.multiply.outer(R[j + 1:, j], R[j + 1:, j]) / R[j, j]
    var = np.diag(np.linalg.inv(A)) * d * d
    bound = np.full((L, 2), np.inf)
    if Nd > 1:
        bound[:, 0] = var[:L]
    if Nb > 1:
        bound[:, 1] = var[L:2 * L] if Nd > 1 else var[:L]
    return out._replace(bound=bound, kappa=float(np.linalg.cond(A, 2)))
