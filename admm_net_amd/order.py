"""The number of targets of every scene selected on the device (csrc/order.hip): the stage between the peak search and the fit.

``refine.refine_targets`` fits as many targets as it is given rows.  ``select_targets`` takes MORE candidate rows than there may be
targets, ranks them against the received signal by greedy orthogonal least squares and keeps the number of rows that minimises a
penalised log residual (the definition is with ``admmnet_order_f64`` in include/admmnet.h):

    x_i = y_i conj(s_i),   a_l(i) = exp(j 2 pi (i_b f_l - i_d tau_l)),   gain_j = |a~_j^H r|^2 / |a~_j|^2,
    RSS_0 = sum |x_i|^2,   RSS_k = RSS_(k-1) - gain_k,   n_sel = argmin_k  D ln(RSS_k / D) + penalty k,

a~_j being a_j made orthogonal to the rows already taken and r the residual of x on them.  A peak displaced from its target leaves
a misfit that a duplicate row soaks up, so a selection is only as good as its rows: ``select_refined`` alternates the selection
with ``refine.refine_targets`` of the selected rows, and may grow the candidates by the highest peak of the residual.

``select_targets``  the batch on the device, one kernel, no host read.
``select_host``     the float64 numpy statement of the definition for ONE scene, written the other way round (explicit D x k
                    matrices and ``np.linalg.lstsq`` for every trial subset of every step, no Gram matrix, no downdate).  The
                    tests hold the kernel to it; it is NOT a fallback -- the device call raises without the HIP library.
``select_refined``  the loop, all of it on the device.

Tensor inputs follow INTEGRATION.md section 3: every pointer is taken through ``ops._c64`` / ``ops._num`` (``ops._plain``).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .metrics import MAX_TARGETS, PIVOT_MIN, _integers
from .refine import MAX_PSK, MODES, NONFINITE, OUTSIDE, _output, psk_points, refine_targets

RANKED = 0
RSS_FLOOR = 2.0 ** -80           # times sum |x|^2: the least RSS_k the criterion takes the logarithm of
INFO = ("cost", "noise_var", "ranked", "state")
TIE = 1e-12                      # ``select_host`` only: gains this close (relative) are a tie, which goes to the smaller index


class OrderResult(NamedTuple):
    perm: torch.Tensor        # [B, Le] int32: the ranked rows in the order they were taken, then the other rows in index order
    n_sel: torch.Tensor       # [B] int32: the selected order -- ``refine_targets(rows_out, n_est=n_sel)`` fits the selected rows
    rss: torch.Tensor         # [B, Le + 1] float64: RSS_0 .. RSS_K, NaN past the K rows ranked
    rows_out: torch.Tensor    # [B, Le, 3] float64: the input rows in ``perm`` order, (tau, f, |C|), |C| NaN from n_sel on
    C: torch.Tensor           # [B, Le] complex128: the least-squares amplitudes of the selected rows, NaN from n_sel on
    residual: torch.Tensor    # [B, D] complex64: x - sum_(l < n_sel) C_l a_l
    cost: torch.Tensor        # [B] float64: sum |residual|^2, added in float64
    noise_var: torch.Tensor   # [B] float64: cost / D
    ranked: torch.Tensor      # [B] int32: K
    state: torch.Tensor       # [B] int32: 0 ranked, 3 non-finite, 4 outside (the codes of ``refine.STATES``)
    status: torch.Tensor      # [2] int32 scenes: non-finite; outside


def default_penalty(grid):
    """4 ln D per target: twice the leading term of BIC's 2 ln(2 D) (DESIGN.md section 4 says where the factor comes from)."""
    return 4.0 * math.log(int(grid[0]) * int(grid[1]))


def _settings(grid, psk, penalty, max_order, Le):
    try:
        Nb, Nd = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"grid must be a pair (Nb, Nd), got {grid!r}") from None
    if Nb < 1 or Nd < 1:
        raise ValueError(f"grid must be at least 1 x 1, got {grid!r}")
    try:
        m, phase = psk
        m, phase = int(m), float(phase)
    except (TypeError, ValueError):
        raise ValueError(f"psk must be a pair (points, phase of point 0), got {psk!r}") from None
    if not (2 <= m <= MAX_PSK and math.isfinite(phase)):
        raise ValueError(f"psk needs 2 .. {MAX_PSK} points and a finite phase, got {psk!r}")
    penalty = default_penalty((Nb, Nd)) if penalty is None else float(penalty)
    if not (penalty >= 0.0 and math.isfinite(penalty)):
        raise ValueError(f"penalty must be a finite number >= 0, got {penalty!r}")
    if not 1 <= Le <= MAX_TARGETS:
        raise ValueError(f"rows must hold 1 <= Le <= {MAX_TARGETS} rows per scene, got Le={Le}")
    if max_order is None:
        max_order = Le
    if isinstance(max_order, bool) or int(max_order) != max_order or not 1 <= int(max_order) <= Le:
        raise ValueError(f"max_order must be an int in 1 .. Le = {Le}, got {max_order!r}")
    return Nb, Nd, m, phase, penalty, int(max_order)


def select_targets(y, b, rows, grid, *, n_cand=None, n_held=None, symbols=None, psk=(4, math.pi / 4), penalty=None, max_order=None,
                   out=None) -> OrderResult:
    """The candidate rows of every scene ranked and the number of targets selected (the module docstring has the definition),
    in one kernel and without a host read.

    y, b      [B, D] complex, D = Nb Nd: the received signal and the demodulated symbols, as ``synth.make_batch`` returns them.
    rows      [B, Le, 3] rows (tau, f, height) as ``ops.peak_top`` returns them -- the height is ignored, a row whose tau or f is
              not finite is absent -- 1 <= Le <= 16.
    grid      (Nb, Nd) = the (M, N) of a model.
    n_cand    None or [B] integers: only the first n_cand rows are candidates; outside 0 .. Le the scene is not ranked.
    n_held    None or [B] integers: the first n_held rows are taken first, in their order, and stay selected; 0 .. n_cand.
    symbols   None (s = b / |b|) or [B, D] integers k with s = p_k of ``psk = (points, phase of point 0)`` -- what
              ``RefineResult.symbols`` holds; a scene with a k outside 0 .. points - 1 (``refine_targets`` marks a scene it did not
              fit with -1) is not ranked.
    penalty   per selected row, a finite float >= 0; None: ``default_penalty(grid)`` = 4 ln D.
    max_order the most rows ranked, 1 .. Le; None: Le.
    out       None, or a pair (rows_out [B, Le, 3] float64, C [B, Le] complex128) of device tensors to write into (the result holds
              these very tensors): dense and of exactly that dtype, anything else is refused with nothing written.
    """
    for t, name in ((y, "y"), (b, "b"), (rows, "rows")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    if rows.dim() != 3 or rows.shape[2] != 3 or y.dim() != 2 or rows.shape[0] != y.shape[0]:
        raise ValueError(f"y must be [B, D] and rows [B, Le, 3], got {tuple(y.shape)} and {tuple(rows.shape)}")
    B, Le = rows.shape[:2]
    Nb, Nd, m, phase, penalty, max_order = _settings(grid, psk, penalty, max_order, Le)
    D = Nb * Nd
    if not (y.is_complex() and b.is_complex()):
        raise ValueError(f"y and b must be complex, got {y.dtype} and {b.dtype}")
    if rows.is_complex() or rows.dtype == torch.bool:
        raise ValueError(f"rows must hold real numbers, got {rows.dtype}")
    if y.shape[1] != D:
        raise ValueError(f"y must be [B, {D}] for the grid {Nb} x {Nd}, got {tuple(y.shape)}")
    if B < 1:
        raise ValueError("select_targets needs B >= 1")
    lib = _lib.load()
    dev = y.device
    with torch.cuda.device(dev):
        y, b = ops._c64(y, dev, (B, D), "y"), ops._c64(b, dev, (B, D), "b")
        rows = ops._num(rows, dev, torch.float64, (B, Le, 3), "rows")
        counts = []
        for t, name in ((n_cand, "n_cand"), (n_held, "n_held")):
            if t is not None:
                _integers(t, name)
                ops._need_cuda(t, name)
                t = ops._num(t, dev, torch.int32, (B,), name)
            counts.append(t)
        if symbols is not None:
            _integers(symbols, "symbols")
            ops._need_cuda(symbols, "symbols")
            symbols = ops._num(symbols, dev, torch.int32, (B, D), "symbols")
        if out is None:
            out, C = torch.empty(B, Le, 3, dtype=torch.float64, device=dev), torch.empty(B, Le, dtype=torch.complex128, device=dev)
        else:
            try:
                out, C = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (rows_out, C) of tensors") from None
            out, C = _output(out, dev, torch.float64, (B, Le, 3), "out rows"), _output(C, dev, torch.complex128, (B, Le), "out C")
            if out.data_ptr() == rows.data_ptr():
                raise ValueError("out rows must not be the input rows: the rows change places")
        perm = torch.empty(B, Le, dtype=torch.int32, device=dev)
        n_sel = torch.empty(B, dtype=torch.int32, device=dev)
        rss = torch.empty(B, Le + 1, dtype=torch.float64, device=dev)
        residual = torch.empty(B, D, dtype=torch.complex64, device=dev)
        info = torch.empty(B, len(INFO), dtype=torch.float64, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_order_f64(Nb, Nd, Le, B, ops._ptr(y), ops._ptr(b), ops._ptr(rows), ops._ptr(counts[0]),
                                         ops._ptr(counts[1]), ops._ptr(symbols), m, phase, penalty, max_order, ops._ptr(perm),
                                         ops._ptr(n_sel), ops._ptr(rss), ops._ptr(out), ops._ptr(C), ops._ptr(residual),
                                         ops._ptr(info), ops._ptr(status), ops._stream(dev)), "admmnet_order_f64")
        ints = info[:, 2:].to(torch.int32)
    return OrderResult(perm, n_sel, rss, out, C, residual, info[:, 0], info[:, 1], ints[:, 0], ints[:, 1], status)


def select_refined(y, b, rows, grid, *, rounds=2, grow=0, symbols="given", penalty=None, peak_opts=None, **refine_kw):
    """Selection and refinement in turns, all on the device and without a host read: ``rounds`` times ``select_targets`` and
    ``refine.refine_targets(rows_out, n_est=n_sel)`` -- the refined rows replace the selected ones, the rows left over stay where
    they are -- and a last ``select_targets``.  Every selection starts afresh (no row is held), so a row that the refinement has
    made superfluous is dropped.

    symbols   "given" or "psk", as in ``refine_targets``; with "psk" the selection after a refinement takes that refinement's
              symbols (a scene it did not fit is then not ranked either).
    grow      extra rounds that add a candidate first: the highest peak of the residual (``ops.peak_top(residual, Nd, Nb,
              peak_opts, top=1)``, whose spectrum is the matched filter of the atoms) replaces the LAST row of every scene with
              n_sel < Le, then one refinement and selection follow.
    peak_opts the options of ``peak_top``; None: steps of a tenth of a cell and 3 refinements, ``estimate``'s.
    refine_kw ``psk``, ``iters``, ``tol`` of ``refine_targets``; ``psk`` goes to the selection too.  ``n_cand`` ([B] integers, as in
              ``select_targets``; what ``detect.CfarResult.n_est`` holds) is taken out of it: only the first n_cand rows of a scene
              are candidates, in every round -- the rows from n_cand on are absent.

    Returns (OrderResult of the last selection, RefineResult of the last refinement or None if there was none).  The result's
    ``perm`` is carried through the rounds: perm[j] is the row of the ``rows`` given here that row j of ``rows_out`` started as,
    -1 for a grown one."""
    if symbols not in MODES:
        raise ValueError(f"symbols must be one of {sorted(MODES)}, got {symbols!r}")
    for value, name in ((rounds, "rounds"), (grow, "grow")):
        if isinstance(value, bool) or int(value) != value or not 0 <= int(value) <= 16:
            raise ValueError(f"{name} must be an int in 0 .. 16, got {value!r}")
    if not isinstance(rows, torch.Tensor):
        raise TypeError(f"rows must be a tensor, got {type(rows).__name__}")
    Nb, Nd = (int(v) for v in grid)
    if peak_opts is None:
        peak_opts = {"xstep": 1 / (10 * Nd), "ystep": 1 / (10 * Nb), "iter": 3}
    psk = refine_kw.get("psk", (4, math.pi / 4))
    n_cand = refine_kw.pop("n_cand", None)
    if n_cand is not None:
        _integers(n_cand, "n_cand")
        if rows.dim() != 3 or tuple(n_cand.shape) != (rows.shape[0],):
            raise ValueError(f"n_cand must be [B] beside rows [B, Le, 3], got {tuple(n_cand.shape)} and {tuple(rows.shape)}")
        beyond = torch.arange(rows.shape[1], device=rows.device)[None, :] >= n_cand.to(rows.device)[:, None]
        rows = torch.where(beyond[:, :, None], math.nan, rows.to(torch.float64))
    sel = select_targets(y, b, rows, grid, n_cand=n_cand, psk=psk, penalty=penalty)
    Le = sel.rows_out.shape[1]
    slot = torch.arange(Le, device=sel.n_sel.device)
    fit = None
    origin = sel.perm.long()

    def turn(sel):
        fit = refine_targets(y, b, sel.rows_out, grid, n_est=sel.n_sel, symbols=symbols, **refine_kw)
        fitted = (slot[None, :] < sel.n_sel[:, None]) & torch.isfinite(fit.rows[:, :, 0]) & torch.isfinite(fit.rows[:, :, 1])
        merged = torch.where(fitted[:, :, None], fit.rows, sel.rows_out)
        return select_targets(y, b, merged, grid, symbols=fit.symbols if symbols == "psk" else None, psk=psk, penalty=penalty), fit

    for _ in range(int(rounds)):
        sel, fit = turn(sel)
        origin = torch.gather(origin, 1, sel.perm.long())
    for _ in range(int(grow)):
        peak, _ = ops.peak_top(sel.residual, Nd, Nb, peak_opts, top=1)
        room = (sel.n_sel < Le)[:, None, None] & (slot == Le - 1)[None, :, None]
        grown = torch.where(room, peak.expand(-1, Le, -1), sel.rows_out)
        first = select_targets(y, b, grown, grid, symbols=fit.symbols if symbols == "psk" and fit is not None else None, psk=psk,
                               penalty=penalty)
        origin = torch.gather(torch.where(room[:, :, 0], -1, origin), 1, first.perm.long())
        sel, fit = turn(first)
        origin = torch.gather(origin, 1, sel.perm.long())
    return sel._replace(perm=origin.to(torch.int32)), fit


# ---- the float64 host statement ------------------------------------------------------------------------------------------------------
class OrderHost(NamedTuple):
    perm: np.ndarray         # [Le] int32
    n_sel: int
    rss: np.ndarray          # [Le + 1]
    rows_out: np.ndarray     # [Le, 3]
    C: np.ndarray            # [Le] complex128
    residual: np.ndarray     # [D] complex128 (the kernel rounds it to complex64)
    cost: float
    noise_var: float
    ranked: int
    state: int
    margin: float            # the least relative gap between the gain taken and the next one (outside a tie), and between the two
                             # lowest criteria: below it a rounding error may change perm or n_sel


def atoms(tau, f, grid):
    """[D, L]: a_l(i) = exp(j 2 pi (i_b f_l - i_d tau_l)), i = i_b Nd + i_d."""
    Nb, Nd = grid
    ib, idd = np.divmod(np.arange(Nb * Nd), Nd)
    return np.exp(2j * np.pi * (np.multiply.outer(ib, np.asarray(f, dtype=np.float64)) -
                                np.multiply.outer(idd, np.asarray(tau, dtype=np.float64))))


def least_squares(A, x):
    """(c, r, RSS) of min |x - A c|: ``np.linalg.lstsq`` on the explicit matrix; no column: (empty, x, |x|^2)."""
    if A.shape[1] == 0:
        return np.zeros(0, dtype=np.complex128), x.copy(), float((np.abs(x) ** 2).sum())
    c = np.linalg.lstsq(A, x, rcond=None)[0]
    r = x - A @ c
    return c, r, float((np.abs(r) ** 2).sum())


def gain_of(A, taken, j, x, rss_before):
    """(gain, |a~_j|^2) of adding column j to the columns ``taken``, whose least-squares residual is ``rss_before``: the drop of
    that residual, and the residual of column j itself on them -- a ``lstsq`` each."""
    return rss_before - least_squares(A[:, taken + [j]], x)[2], least_squares(A[:, taken], A[:, j])[2]


def pick_next(gains, norms, eligible, D):
    """The eligible row of greatest gain whose |a~|^2 is not below 2^-40 D -- the smaller index within TIE -- or None; and the
    relative gap to the best row outside the tie."""
    ok = [j for j in eligible if norms[j] >= PIVOT_MIN * D]
    if not ok:
        return None, math.inf
    top = max(gains[j] for j in ok)
    tied = [j for j in ok if top - gains[j] <= TIE * abs(top)]
    rest = [gains[j] for j in ok if j not in tied]
    return tied[0], ((top - max(rest)) / abs(top) if rest and top != 0 else math.inf)


def held_in_order(held):
    """The order in which the held rows are taken: as given."""
    return list(held)


def select_host(y, b, rows, grid, *, n_cand=None, n_held=None, symbols=None, psk=(4, math.pi / 4), penalty=None,
                max_order=None) -> OrderHost:
    """``select_targets`` for ONE scene in float64 numpy.  y, b [D]; rows [Le, 3]; symbols None or [D] integers."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    Le = len(rows)
    Nb, Nd, m, phase, penalty, max_order = _settings(grid, psk, penalty, max_order, Le)
    grid, D = (Nb, Nd), Nb * Nd
    y, b = (np.asarray(v, dtype=np.complex128).reshape(-1) for v in (y, b))
    if len(y) != D or len(b) != D:
        raise ValueError(f"y and b must have {D} entries")
    nan_C = np.full(Le, np.nan + 1j * np.nan)
    none = OrderHost(np.arange(Le, dtype=np.int32), 0, np.full(Le + 1, np.nan), np.full((Le, 3), np.nan), nan_C,
                     np.full(D, np.nan + 1j * np.nan), math.nan, math.nan, 0, RANKED, math.inf)
    n = Le if n_cand is None else int(n_cand)
    held = 0 if n_held is None else int(n_held)
    if symbols is not None:
        symbols = np.asarray(symbols).reshape(-1)
    if not 0 <= n <= Le or not 0 <= held <= n or (symbols is not None and ((symbols < 0) | (symbols >= m)).any()):
        return none._replace(state=OUTSIDE)
    if not (np.isfinite(y).all() and np.isfinite(b).all()) or (symbols is None and (b == 0).any()):
        return none._replace(state=NONFINITE)
    x = y * np.conj(b / np.abs(b) if symbols is None else psk_points(m, phase)[symbols])
    present = [j for j in range(n) if np.isfinite(rows[j, 0]) and np.isfinite(rows[j, 1])]
    A = np.zeros((D, Le), dtype=np.complex128)
    A[:, present] = atoms(rows[present, 0], rows[present, 1], grid)
    taken, n_fixed, margin = [], 0, math.inf
    rss = [float((np.abs(x) ** 2).sum())]
    waiting = held_in_order([j for j in present if j < held])
    while len(taken) < max_order:
        if waiting:
            j = waiting.pop(0)
            if gain_of(A, taken, j, x, rss[-1])[1] < PIVOT_MIN * D:
                continue
            n_fixed += 1
        else:
            left = [j for j in present if j not in taken]
            trial = {j: gain_of(A, taken, j, x, rss[-1]) for j in left}
            j, gap = pick_next({j: v[0] for j, v in trial.items()}, {j: v[1] for j, v in trial.items()}, left, D)
            if j is None:
                break
            margin = min(margin, gap)
        taken.append(j)
        rss.append(least_squares(A[:, taken], x)[2])
    K = len(taken)
    crit = [D * math.log(max(rss[k], RSS_FLOOR * rss[0]) / D) + penalty * k if max(rss[k], RSS_FLOOR * rss[0]) > 0 else -math.inf
            for k in range(K + 1)]
    n_sel = min(range(n_fixed, K + 1), key=lambda k: (crit[k], k))
    others = sorted(crit[k] for k in range(n_fixed, K + 1) if k != n_sel)
    if others:
        margin = min(margin, (others[0] - crit[n_sel]) / max(1.0, abs(crit[n_sel])) if math.isfinite(crit[n_sel]) else 0.0)
    C, residual, cost = least_squares(A[:, taken[:n_sel]], x)
    perm = np.array(taken + [j for j in range(Le) if j not in taken], dtype=np.int32)
    rows_out = rows[perm].copy()
    rows_out[:, 2] = np.nan
    rows_out[:n_sel, 2] = np.abs(C)
    Cs = nan_C.copy()
    Cs[:n_sel] = C
    return OrderHost(perm, n_sel, np.array(rss + [math.nan] * (Le - K)), rows_out, Cs, residual, cost, cost / D, K, RANKED, margin)
