"""A CFAR detector on the zero-padded 2-D periodogram, on the device (csrc/cfar.hip): the radar baseline, and a detector that is
not handed the number of targets.

What an OFDM radar runs: strip the symbols, x_i = y_i conj(s_i); take the periodogram on a grid oversampled ``r`` times,

    P[j][i] = |sum x[i_b Nd + i_d] exp(-j 2 pi (i_b f_j - i_d tau_i))|^2 / D,   f_j = -1/2 + j / (r Nb),   tau_i = i / (r Nd),

the matched filter of the atoms of ``refine`` and ``order``, E[P] = the noise variance under white noise; call a cell a detection
when it exceeds ``alpha`` times a noise level Z and beats its 8 neighbours on the torus.  Z is the known variance (``known``), the
mean of N training cells round the cell (``ca``) or their k-th smallest (``os``); the training cells lie ``r`` map cells apart (one
resolution cell: independent samples of an orthogonal DFT), outside a guard ring, and ``alpha`` follows from the false-alarm rate
in closed form (``cfar_alpha``).  The definition is with ``admmnet_cfar_f64`` in include/admmnet.h.

``cfar_targets``  the batch on the device, one kernel, no host read.  Its rows are the ``[B, Le, 3]`` rows (tau, f, height) that
                  ``refine.refine_targets(rows, n_est=res.n_est)`` and ``order.select_refined(..., n_cand=res.n_est)`` take.
``cfar_relax``    successive cancellation with cyclic re-fitting on that map, one kernel (csrc/cfar_relax.hip): the highest cell
                  over the threshold is fitted off the grid, subtracted from the residual and re-fitted with the targets found
                  before; the map is taken again of the residual until no cell is over.  ``cfar_relax_host`` is its float64 numpy
                  statement for one scene, with the margin of every decision it took.
``cfar_alpha``    the threshold factor of a method, on the host in float64.
``cfar_host``     the float64 numpy statement of the definition for ONE scene, written the other way round (zero-padded ``np.fft``
                  for the map, ``np.roll`` for the window, ``np.sort`` for the rank).  The tests hold the kernel to it; it is NOT a
                  fallback -- the device call raises without the HIP library.

Tensor inputs follow INTEGRATION.md section 3: every pointer is taken through ``ops._c64`` / ``ops._num`` (``ops._plain``).
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .metrics import MAX_TARGETS, _integers
from .refine import MAX_PSK, NONFINITE, OUTSIDE, _output, psk_points

DONE = 0
METHODS = {"known": 0, "ca": 1, "os": 2}
MAX_OVERSAMPLE = 8
MAX_REACH = 8                    # guard + train at most: N <= 288 training cells
MAX_CELLS = 65535                # map cells: a detection is listed by a 16-bit index
MAX_GRID = 3406                  # Nb Nd, the generator's ceiling
LDS_LIMIT = 160 * 1024
TIE = 1e-12                      # ``cfar_host`` only: heights this close (relative) are a tie, which goes to the smaller index


class CfarResult(NamedTuple):
    rows: torch.Tensor        # [B, Le, 3] float64 (tau, f, P): the detections by height, NaN beyond them
    n_det: torch.Tensor       # [B] int32: all detections -- it may exceed Le
    n_over: torch.Tensor      # [B] int32: the cells over the threshold
    level: torch.Tensor       # [B] float64: the mean of Z over the map (``known``: the given value)
    state: torch.Tensor       # [B] int32: 0 done, 3 non-finite, 4 outside (the codes of ``refine.STATES``)
    map: torch.Tensor | None  # [B, r Nb, r Nd] float64 with ``return_map``
    status: torch.Tensor      # [2] int32 scenes: non-finite; outside

    @property
    def n_est(self):
        """[B] int32: clamp(n_det, 0, Le) -- the rows present, what ``refine_targets(rows, n_est=)`` and
        ``select_refined(..., n_cand=)`` take."""
        return self.n_det.clamp(0, self.rows.shape[1])


def train_count(grid, guard, train):
    """N = |Omega|: the cells within guard + train resolution cells on every axis longer than 1, less those within guard."""
    Nb, Nd = grid
    reach = lambda n, c: c if n > 1 else 0  # noqa: E731
    return ((2 * reach(Nb, guard + train) + 1) * (2 * reach(Nd, guard + train) + 1) -
            (2 * reach(Nb, guard) + 1) * (2 * reach(Nd, guard) + 1))


def default_rank(n_train):
    return -(-3 * n_train // 4)      # ceil(3 N / 4)


def lds_bytes(grid, oversample):
    """What ``admmnet_cfar_lds_bytes`` returns where the shape is admitted: the arrays of csrc/cfar.hip's layout, each rounded up
    to 16 bytes."""
    Nb, Nd = grid
    r = oversample
    D, nf, nt = Nb * Nd, r * Nb, r * Nd
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    return (up(16 * D) + up(16 * nf * Nd) + up(8 * nf * nt) + up(16 * nf) + up(16 * nt) + up(16 * MAX_PSK) + up(4 * 288) +
            up(nf * nt) + up(2 * nf * nt) + up(4 * 257) + up(4 * MAX_TARGETS) + up(8 * 4))


def cfar_alpha(method, n_train, pfa, rank=None):
    """The factor alpha with P(a noise cell > alpha Z) = pfa, in float64 on the host.

    known   -ln(pfa): P / w is exponential.
    ca      N (pfa^(-1/N) - 1): the sum of N exponentials is a gamma variable.
    os      the root of prod_(m < k) (N - m) / (N - m + alpha) = pfa by bisection on its logarithm; k = ``rank``, None: ceil(3N/4).
    """
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    pfa = float(pfa)
    if not 0.0 < pfa < 1.0:
        raise ValueError(f"pfa must lie in (0, 1), got {pfa!r}")
    if method == "known":
        return -math.log(pfa)
    if isinstance(n_train, bool) or int(n_train) != n_train or n_train < 1:
        raise ValueError(f"n_train must be an int >= 1, got {n_train!r}")
    N = int(n_train)
    if method == "ca":
        return N * math.expm1(-math.log(pfa) / N)
    k = default_rank(N) if rank is None else rank
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= N:
        raise ValueError(f"rank must be an int in 1 .. N = {N}, got {rank!r}")
    k, target = int(k), math.log(pfa)
    g = lambda a: sum(math.log(N - m) - math.log(N - m + a) for m in range(k)) - target  # noqa: E731  decreasing in a
    lo, hi = 0.0, 1.0
    while g(hi) > 0.0:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        lo, hi = (mid, hi) if g(mid) > 0.0 else (lo, mid)
    return 0.5 * (lo + hi)


def _settings(grid, top, oversample, method, pfa, guard, train, rank, psk, has_noise):
    try:
        Nb, Nd = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"grid must be a pair (Nb, Nd), got {grid!r}") from None
    if Nb < 1 or Nd < 1 or Nb * Nd > MAX_GRID:
        raise ValueError(f"grid must be at least 1 x 1 with Nb Nd <= {MAX_GRID}, got {grid!r}")
    try:
        m, phase = psk
        m, phase = int(m), float(phase)
    except (TypeError, ValueError):
        raise ValueError(f"psk must be a pair (points, phase of point 0), got {psk!r}") from None
    if not (2 <= m <= MAX_PSK and math.isfinite(phase)):
        raise ValueError(f"psk needs 2 .. {MAX_PSK} points and a finite phase, got {psk!r}")
    for value, name, lo, hi in ((top, "top", 1, MAX_TARGETS), (oversample, "oversample", 1, MAX_OVERSAMPLE)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
            raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {value!r}")
    r = int(oversample)
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    if has_noise != (method == "known"):
        raise ValueError("noise_var is given with method 'known' and only with it")
    if Nb * Nd * r * r > MAX_CELLS or lds_bytes((Nb, Nd), r) > LDS_LIMIT:
        raise ValueError(f"a {Nb} x {Nd} grid oversampled {r} times needs {lds_bytes((Nb, Nd), r)} bytes of LDS for "
                         f"{Nb * Nd * r * r} map cells; a workgroup has {LDS_LIMIT} bytes and lists at most {MAX_CELLS} cells")
    if method == "known":
        if rank is not None:
            raise ValueError("rank belongs to method 'os'")
        return Nb, Nd, m, phase, r, 0, 0, 1, cfar_alpha("known", None, pfa)
    for value, name, lo in ((guard, "guard", 0), (train, "train", 1)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo:
            raise ValueError(f"{name} must be an int >= {lo}, got {value!r}")
    W = int(guard) + int(train)
    if W > MAX_REACH:
        raise ValueError(f"guard + train must be at most {MAX_REACH}, got {W}")
    for n, name in ((Nb, "Nb"), (Nd, "Nd")):
        if n > 1 and 2 * W + 1 > n:
            raise ValueError(f"the window of 2 (guard + train) + 1 = {2 * W + 1} resolution cells does not fit {name} = {n}")
    N = train_count((Nb, Nd), int(guard), int(train))
    if N < 1:
        raise ValueError("the window holds no training cell")
    if method != "os" and rank is not None:
        raise ValueError("rank belongs to method 'os'")
    k = default_rank(N) if rank is None else rank
    alpha = cfar_alpha(method, N, pfa, k if method == "os" else None)
    return Nb, Nd, m, phase, r, int(guard), int(train), int(k), alpha


def _check_scenes(what, y, b, Nb, Nd, noise_var, symbols):
    """The checks of the scene tensors that need no library: (B, noise_var as a tensor, a float or None)."""
    for t, name in ((y, "y"), (b, "b")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    D = Nb * Nd
    if y.dim() != 2 or y.shape[1] != D or tuple(b.shape) != tuple(y.shape):
        raise ValueError(f"y and b must be [B, {D}] for the grid {Nb} x {Nd}, got {tuple(y.shape)} and {tuple(b.shape)}")
    if not (y.is_complex() and b.is_complex()):
        raise ValueError(f"y and b must be complex, got {y.dtype} and {b.dtype}")
    B = y.shape[0]
    if B < 1:
        raise ValueError(f"{what} needs B >= 1")
    if noise_var is not None and not isinstance(noise_var, torch.Tensor):
        try:
            noise_var = float(noise_var)
        except (TypeError, ValueError):
            raise ValueError(f"noise_var must be a tensor [B] or a float, got {noise_var!r}") from None
    if isinstance(noise_var, torch.Tensor) and (noise_var.is_complex() or noise_var.dtype == torch.bool or tuple(noise_var.shape) != (B,)):
        raise ValueError(f"noise_var must hold {B} real numbers, got {noise_var.dtype} {tuple(noise_var.shape)}")
    if symbols is not None:
        _integers(symbols, "symbols")
        if tuple(symbols.shape) != (B, D):
            raise ValueError(f"symbols must be [B, {D}], got {tuple(symbols.shape)}")
    return B, noise_var


def _on_device(y, b, noise_var, symbols, B, D):
    """The scene tensors as the kernels read them, on y's device."""
    dev = y.device
    y, b = ops._c64(y, dev, (B, D), "y"), ops._c64(b, dev, (B, D), "b")
    if isinstance(noise_var, float):
        noise_var = torch.full((B,), noise_var, dtype=torch.float64, device=dev)
    elif noise_var is not None:
        ops._need_cuda(noise_var, "noise_var")
        noise_var = ops._num(noise_var, dev, torch.float64, (B,), "noise_var")
    if symbols is not None:
        ops._need_cuda(symbols, "symbols")
        symbols = ops._num(symbols, dev, torch.int32, (B, D), "symbols")
    return y, b, noise_var, symbols


def cfar_targets(y, b, grid, *, top=16, oversample=4, method="ca", pfa=1e-4, guard=1, train=2, rank=None, noise_var=None,
                 symbols=None, psk=(4, math.pi / 4), return_map=False, out=None) -> CfarResult:
    """The detections of every scene (the module docstring has the definition), in one kernel and without a host read.

    y, b        [B, D] complex, D = Nb Nd: the received signal and the demodulated symbols, as ``synth.make_batch`` returns them.
    grid        (Nb, Nd) = the (M, N) of a model.
    top         Le, 1 .. 16: the rows per scene.
    oversample  r, 1 .. 8: map cells per resolution cell and axis.
    method      "known", "ca" or "os";  pfa the false-alarm rate per cell, in (0, 1).
    guard, train  the window in resolution cells (not read by "known"): guard >= 0, train >= 1, guard + train <= 8 and
                2 (guard + train) + 1 <= every axis longer than 1.
    rank        "os" only: 1 .. N; None: ceil(3 N / 4).
    noise_var   "known" only: [B] real numbers (``make_scenes_device``'s ``truth["noise_var"]``) or one float.
    symbols     None (s = b / |b|) or [B, D] integers k with s = p_k of ``psk``, as in ``select_targets``.
    return_map  also return the map [B, r Nb, r Nd].
    out         None, or the rows tensor [B, Le, 3] float64 to write into (the result holds this very tensor): dense and of exactly
                that dtype, anything else is refused with nothing written.
    Every bad argument is a ValueError before the library is touched."""
    Nb, Nd, m, phase, r, guard, train, rank, alpha = _settings(grid, top, oversample, method, pfa, guard, train, rank, psk,
                                                               noise_var is not None)
    D, Le = Nb * Nd, int(top)
    B, noise_var = _check_scenes("cfar_targets", y, b, Nb, Nd, noise_var, symbols)
    dev = y.device
    if out is not None:
        out = _output(out, dev, torch.float64, (B, Le, 3), "out")
    ops._need_cuda(y, "y")
    ops._need_cuda(b, "b")
    lib = _lib.load()
    with torch.cuda.device(dev):
        y, b, noise_var, symbols = _on_device(y, b, noise_var, symbols, B, D)
        rows = torch.empty(B, Le, 3, dtype=torch.float64, device=dev) if out is None else out
        counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
        info = torch.empty(B, 2, dtype=torch.float64, device=dev)
        pmap = torch.empty(B, r * Nb, r * Nd, dtype=torch.float64, device=dev) if return_map else None
        status = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_cfar_f64(Nb, Nd, r, Le, B, ops._ptr(y), ops._ptr(b), ops._ptr(symbols), m, phase, METHODS[method],
                                        guard, train, rank, alpha, ops._ptr(noise_var), ops._ptr(rows), ops._ptr(counts),
                                        ops._ptr(info), ops._ptr(pmap), ops._ptr(status), ops._stream(dev)), "admmnet_cfar_f64")
        state = info[:, 1].to(torch.int32)
    return CfarResult(rows, counts[:, 0], counts[:, 1], info[:, 0], state, pmap, status)


# ---- the float64 host statement ------------------------------------------------------------------------------------------------------
class CfarHost(NamedTuple):
    rows: np.ndarray         # [Le, 3]
    n_det: int
    n_over: int
    level: float
    state: int
    map: np.ndarray          # [n_f, n_tau]
    margin: float            # the least relative gap of a decision: below it a rounding error may change a count or a row


def periodogram(x, grid, oversample):
    """[r Nb, r Nd]: the map of x [D] by zero-padded FFTs.  The -1/2 of f_j is the modulation (-1)^i_b; the sum over i_d has the
    sign of an inverse transform."""
    Nb, Nd = grid
    X = np.asarray(x, dtype=np.complex128).reshape(Nb, Nd) * ((-1.0) ** np.arange(Nb))[:, None]
    nf, nt = oversample * Nb, oversample * Nd
    S = np.fft.ifft(np.fft.fft(X, n=nf, axis=0), n=nt, axis=1) * nt
    return (S.real ** 2 + S.imag ** 2) / (Nb * Nd)


def window_offsets(grid, guard, train):
    """Omega in resolution cells, p outer and q inner, both ascending."""
    Nb, Nd = grid
    Wb, Wd = (guard + train if n > 1 else 0 for n in (Nb, Nd))
    Gb, Gd = (guard if n > 1 else 0 for n in (Nb, Nd))
    return [(p, q) for p in range(-Wb, Wb + 1) for q in range(-Wd, Wd + 1) if not (abs(p) <= Gb and abs(q) <= Gd)]


def training_cells(P, offsets, oversample):
    """[N, n_f, n_tau]: entry n at (j, i) is P[(j + p r) mod n_f][(i + q r) mod n_tau] of offset n."""
    return np.stack([np.roll(P, (-p * oversample, -q * oversample), axis=(0, 1)) for p, q in offsets])


def noise_level(cells, method, rank):
    return cells.mean(axis=0) if method == "ca" else np.sort(cells, axis=0)[rank - 1]


def is_over(P, threshold):
    return P > threshold


def beats(Pc, c, Pd, d):
    """Cell c (height Pc) beats cell d: higher, or within TIE and the smaller index."""
    tie = np.abs(Pc - Pd) <= TIE * np.maximum(Pc, Pd)
    return np.where(tie, c < d, Pc > Pd)


def neighbours(P):
    """The 8 (heights, indices) of the cells one map cell away on the torus, and the cells' own indices."""
    idx = np.arange(P.size).reshape(P.shape)
    return [(np.roll(P, (-dj, -di), axis=(0, 1)), np.roll(idx, (-dj, -di), axis=(0, 1)))
            for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dj, di) != (0, 0)], idx


def cfar_host(y, b, grid, *, top=16, oversample=4, method="ca", pfa=1e-4, guard=1, train=2, rank=None, noise_var=None, symbols=None,
              psk=(4, math.pi / 4), exempt=()) -> CfarHost:
    """``cfar_targets`` for ONE scene in float64 numpy.  y, b [D]; symbols None or [D] integers; noise_var None or a float.
    ``exempt``: pairs of cells (c, c') that tie by construction and do not enter the margin.  So do not two cells that differ only
    along an axis of length 1, along which the map is constant by definition."""
    Nb, Nd, m, phase, r, guard, train, rank, alpha = _settings(grid, top, oversample, method, pfa, guard, train, rank, psk,
                                                               noise_var is not None)
    grid, D, Le, nf, nt = (Nb, Nd), Nb * Nd, int(top), r * Nb, r * Nd
    y, b = (np.asarray(v, dtype=np.complex128).reshape(-1) for v in (y, b))
    if len(y) != D or len(b) != D:
        raise ValueError(f"y and b must have {D} entries")
    none = CfarHost(np.full((Le, 3), np.nan), 0, 0, math.nan, DONE, np.full((nf, nt), np.nan), math.inf)
    if symbols is not None:
        symbols = np.asarray(symbols).reshape(-1)
    if (symbols is not None and ((symbols < 0) | (symbols >= m)).any()) or (method == "known" and noise_var <= 0):
        return none._replace(state=OUTSIDE)
    if (not (np.isfinite(y).all() and np.isfinite(b).all()) or (symbols is None and (b == 0).any()) or
            (method == "known" and not math.isfinite(noise_var))):
        return none._replace(state=NONFINITE)
    x = y * np.conj(b / np.abs(b) if symbols is None else psk_points(m, phase)[symbols])
    P = periodogram(x, grid, r)
    if method == "known":
        Z = np.full_like(P, float(noise_var))
    else:
        Z = noise_level(training_cells(P, window_offsets(grid, guard, train), r), method, rank)
    threshold = alpha * Z
    over = is_over(P, threshold)
    rel = lambda a, c: np.abs(a - c) / np.where(np.maximum(a, c) > 0, np.maximum(a, c), 1.0)  # noqa: E731
    both_zero = (P == 0) & (threshold == 0)              # sums of exact zeros, in every arithmetic: no decision hangs on a rounding
    margin = float(np.where(both_zero, np.inf, rel(P, threshold)).min())
    around, idx = neighbours(P)
    peak = np.ones_like(over)
    allowed = {tuple(sorted(pair)) for pair in exempt}
    for Pn, cn in around:
        other = cn != idx
        peak &= ~other | beats(P, idx, Pn, cn)
        # an over cell against every neighbour, won or lost; not the pairs equal by construction
        jn, i_n = np.divmod(cn, nt)
        j, i = np.divmod(idx, nt)
        by_definition = ((Nb == 1) & (i == i_n)) | ((Nd == 1) & (j == jn))
        listed = np.array([tuple(sorted(pr)) in allowed for pr in zip(idx.ravel().tolist(), cn.ravel().tolist())]).reshape(P.shape) \
            if allowed else np.zeros_like(over)
        counted = over & other & ~by_definition & ~listed
        if counted.any():
            margin = min(margin, float(rel(P, Pn)[counted].min()))
    det = [int(c) for c in idx[over & peak]]
    flat = P.ravel()
    det.sort(key=functools.cmp_to_key(lambda c, d: -1 if beats(flat[c], c, flat[d], d) else 1))
    for c, d in zip(det[:Le], det[1:Le + 1]):
        if tuple(sorted((c, d))) not in allowed:
            margin = min(margin, float((flat[c] - flat[d]) / flat[c]))
    rows = np.full((Le, 3), np.nan)
    for l, c in enumerate(det[:Le]):
        j, i = divmod(c, nt)
        rows[l] = (i / nt, j / nf - 0.5, flat[c])
    level = float(noise_var) if method == "known" else float(Z.mean())
    return CfarHost(rows, len(det), int(over.sum()), level, DONE, P, margin)


# ---- successive cancellation with cyclic re-fitting (csrc/cfar_relax.hip) ---------------------------------------------------------------
MAX_ITERS = 16
MAX_SWEEPS = 8


class CfarRelaxResult(NamedTuple):
    rows: torch.Tensor        # [B, Le, 3] float64 (tau in [0, 1), f in [-1/2, 1/2), |c|^2 D) in detection order, NaN beyond n_det
    amp: torch.Tensor         # [B, Le] complex128: c of every row
    n_det: torch.Tensor       # [B] int32: the targets found, 0 .. Le
    more: torch.Tensor        # [B] int32: 1 where a cell was still over the threshold after Le targets
    maps: torch.Tensor        # [B] int32: the maps computed
    level: torch.Tensor       # [B] float64: the mean of Z over the last map (``known``: the given value)
    resid: torch.Tensor       # [B] float64: the mean of |residual|^2 at the end, a noise estimate
    state: torch.Tensor       # [B] int32: 0 done, 3 non-finite, 4 outside
    map: torch.Tensor | None  # [B, r Nb, r Nd] float64 with ``return_map``: the last map, the one the stop was decided on
    status: torch.Tensor      # [2] int32 scenes: non-finite; outside

    @property
    def n_est(self):
        """[B] int32: the rows present, what ``refine_targets(rows, n_est=)`` and ``select_refined(..., n_cand=)`` take."""
        return self.n_det.clamp(0, self.rows.shape[1])


def relax_lds_bytes(grid, oversample):
    """What ``admmnet_cfar_relax_lds_bytes`` returns where the shape is admitted: the arrays of csrc/cfar_relax.hip's layout, each
    rounded up to 16 bytes."""
    Nb, Nd = grid
    r = oversample
    D, nf, nt = Nb * Nd, r * Nb, r * Nd
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    return (up(16 * D) + up(16 * nf * Nd) + up(8 * nf * nt) + up(16 * nf) + up(16 * nt) + up(16 * MAX_PSK) + up(4 * 288) +
            up(nf * nt) + up(16 * Nb) + up(16 * Nd) + up(40 * MAX_TARGETS) + up(8 * 4 * 12) + up(4 * 4))


def _relax_settings(grid, oversample, iters, sweeps):
    for value, name, hi in ((iters, "iters", MAX_ITERS), (sweeps, "sweeps", MAX_SWEEPS)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= value <= hi:
            raise ValueError(f"{name} must be an int in 0 .. {hi}, got {value!r}")
    Nb, Nd = (int(v) for v in grid)
    if relax_lds_bytes((Nb, Nd), int(oversample)) > LDS_LIMIT:
        raise ValueError(f"a {Nb} x {Nd} grid oversampled {oversample} times needs {relax_lds_bytes((Nb, Nd), int(oversample))} bytes "
                         f"of LDS; a workgroup has {LDS_LIMIT}")
    return int(iters), int(sweeps)


def cfar_relax(y, b, grid, *, top=16, oversample=4, method="ca", pfa=1e-4, guard=1, train=2, rank=None, noise_var=None,
               symbols=None, psk=(4, math.pi / 4), iters=3, sweeps=2, return_map=False, out=None) -> CfarRelaxResult:
    """Successive cancellation on the periodogram, in one kernel and without a host read: round after round the map of
    ``cfar_targets`` is taken of a residual (at first x = y conj(s)), the highest cell over the threshold is fitted off the grid by
    at most ``iters`` Newton steps on the matched filter F = |S|^2 / D (clamped to half a map cell round the start), c a(tau, f)
    with c = S / D is subtracted, and with two or more targets ``sweeps`` sweeps of cyclic re-fitting follow (each target added
    back, fitted from where it is, subtracted again).  It stops when no cell is over, or with ``more = 1`` after ``top`` targets.
    The definition is with ``admmnet_cfar_relax_f64`` in include/admmnet.h.

    The arguments of ``cfar_targets``, and
    iters       0 .. 16 Newton steps per fit; 0 leaves the grid point (with ``sweeps = 0``: on-grid CLEAN).
    sweeps      0 .. 8 sweeps after every detection from the second on; 0: plain CLEAN.
    return_map  also return the LAST map [B, r Nb, r Nd], the one the stop was decided on.
    out         None, or the rows tensor [B, Le, 3] float64 to write into, as in ``cfar_targets``.
    Every bad argument is a ValueError / TypeError before the library is touched."""
    Nb, Nd, m, phase, r, guard, train, rank, alpha = _settings(grid, top, oversample, method, pfa, guard, train, rank, psk,
                                                               noise_var is not None)
    iters, sweeps = _relax_settings((Nb, Nd), r, iters, sweeps)
    D, Le = Nb * Nd, int(top)
    B, noise_var = _check_scenes("cfar_relax", y, b, Nb, Nd, noise_var, symbols)
    dev = y.device
    if out is not None:
        out = _output(out, dev, torch.float64, (B, Le, 3), "out")
    ops._need_cuda(y, "y")
    ops._need_cuda(b, "b")
    lib = _lib.load()
    with torch.cuda.device(dev):
        y, b, noise_var, symbols = _on_device(y, b, noise_var, symbols, B, D)
        rows = torch.empty(B, Le, 3, dtype=torch.float64, device=dev) if out is None else out
        amp = torch.empty(B, Le, dtype=torch.complex128, device=dev)
        counts = torch.empty(B, 3, dtype=torch.int32, device=dev)
        info = torch.empty(B, 3, dtype=torch.float64, device=dev)
        pmap = torch.empty(B, r * Nb, r * Nd, dtype=torch.float64, device=dev) if return_map else None
        status = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_cfar_relax_f64(Nb, Nd, r, Le, B, ops._ptr(y), ops._ptr(b), ops._ptr(symbols), m, phase,
                                              METHODS[method], guard, train, rank, alpha, ops._ptr(noise_var), iters, sweeps,
                                              ops._ptr(rows), ops._ptr(amp), ops._ptr(counts), ops._ptr(info), ops._ptr(pmap),
                                              ops._ptr(status), ops._stream(dev)), "admmnet_cfar_relax_f64")
        state = info[:, 2].to(torch.int32)
    return CfarRelaxResult(rows, amp, counts[:, 0], counts[:, 1], counts[:, 2], info[:, 0], info[:, 1], state, pmap, status)


# ---- its float64 host statement -------------------------------------------------------------------------------------------------------
class CfarRelaxHost(NamedTuple):
    rows: np.ndarray         # [Le, 3]
    amp: np.ndarray          # [Le] complex128
    n_det: int
    more: int
    maps: int
    level: float
    resid: float
    state: int
    map: np.ndarray          # [n_f, n_tau] the last map
    margin: float            # the least relative gap of a decision (``cfar_relax_host`` lists them)
    not_definite: int        # fits that met a Hessian that is not negative definite
    clamped: int             # Newton steps that a bound of the box cut short


def atom(tau, f, grid):
    """a(tau, f) [D] = exp(+j 2 pi (i_b f - i_d tau))."""
    ib, idd = np.divmod(np.arange(grid[0] * grid[1]), grid[1])
    return np.exp(2j * np.pi * (ib * f - idd * tau))


def moments(x, tau, f, grid):
    """(S, S_b, S_d, S_bb, S_dd, S_bd): sum_i x_i w_i conj(a_i) for the weights 1, i_b, i_d, i_b^2, i_d^2, i_b i_d."""
    ib, idd = np.divmod(np.arange(grid[0] * grid[1]), grid[1])
    e = np.asarray(x) * np.conj(atom(tau, f, grid))
    return tuple(complex((e * w).sum()) for w in (1.0, ib, idd, ib * ib, idd * idd, ib * idd))


def amplitude(S, D):
    return S / D


def clamp_box(grid, oversample):
    """(half_tau, half_f): half a MAP cell on each axis."""
    return 0.5 / (oversample * grid[1]), 0.5 / (oversample * grid[0])


def newton_step(mom, grid):
    """(d_tau, d_f, definite, gap) of one Newton step on |S|^2 (its gradient and Hessian over 4 pi); ``gap``: the least relative
    gap of the tests on the Hessian -- h against the larger of the two terms it is the difference of, det against |h_tt h_ff|."""
    S, Sb, Sd, Sbb, Sdd, Sbd = mom
    K = 2.0 * math.pi
    g_tau, g_f = -(np.conj(S) * Sd).imag, (np.conj(S) * Sb).imag
    t_a, t_b, f_a, f_b = abs(Sd) ** 2, (np.conj(S) * Sdd).real, abs(Sb) ** 2, (np.conj(S) * Sbb).real
    h_tt, h_ff, h_tf = K * (t_a - t_b), K * (f_a - f_b), K * ((np.conj(S) * Sbd).real - (np.conj(Sd) * Sb).real)
    rel = lambda a, c: abs(a - c) / max(abs(a), abs(c), 1e-300)  # noqa: E731
    if grid[0] > 1 and grid[1] > 1:
        det = h_tt * h_ff - h_tf * h_tf
        gap = min(rel(t_a, t_b), abs(det) / max(abs(h_tt * h_ff), 1e-300))
        if not (h_tt < 0 and det > 0):
            return 0.0, 0.0, False, gap
        return -(h_ff * g_tau - h_tf * g_f) / det, -(h_tt * g_f - h_tf * g_tau) / det, True, gap
    if grid[1] > 1:
        return (-g_tau / h_tt, 0.0, True, rel(t_a, t_b)) if h_tt < 0 else (0.0, 0.0, False, rel(t_a, t_b))
    return (0.0, -g_f / h_ff, True, rel(f_a, f_b)) if h_ff < 0 else (0.0, 0.0, False, rel(f_a, f_b))


def fit(x, grid, oversample, tau0, f0, iters):
    """(tau, f, S, margin, not_definite, clamped): at most ``iters`` Newton steps from (tau0, f0) inside the box."""
    half_tau, half_f = clamp_box(grid, oversample)
    tau, f, margin, not_definite, clamped = tau0, f0, math.inf, 0, 0
    for step in range(iters + 1):
        mom = moments(x, tau, f, grid)
        if step == iters or grid == (1, 1):
            break
        d_tau, d_f, definite, gap = newton_step(mom, grid)
        margin = min(margin, gap)
        if not definite:
            not_definite += 1
            break
        for moved, at, start, half in ((grid[1] > 1, tau + d_tau, tau0, half_tau), (grid[0] > 1, f + d_f, f0, half_f)):
            if moved:
                margin = min(margin, abs(at - (start - half)) / half, abs(at - (start + half)) / half)
                clamped += int(not start - half <= at <= start + half)
        tau, f = min(max(tau + d_tau, tau0 - half_tau), tau0 + half_tau), min(max(f + d_f, f0 - half_f), f0 + half_f)
    return tau, f, mom[0], margin, not_definite, clamped


def add_back(x, c, a):
    return x + c * a


def threshold_map(P, first):
    """The map the level Z is taken on: the residual's, not round 0's."""
    return P


def candidates(P, over):
    """The heights the highest over cell is chosen among."""
    return np.where(over, P, -np.inf)


def limit_reached(n, Le, fitted):
    """The test k == Le comes BEFORE the fit of round k."""
    return n == Le and not fitted


def cfar_relax_host(y, b, grid, *, top=16, oversample=4, method="ca", pfa=1e-4, guard=1, train=2, rank=None, noise_var=None,
                    symbols=None, psk=(4, math.pi / 4), iters=3, sweeps=2, exempt=()) -> CfarRelaxHost:
    """``cfar_relax`` for ONE scene in float64 numpy, written the other way round: ``np.fft`` for every map, vectorised moments.
    ``margin`` is the least relative gap of every decision taken: P against alpha Z over all cells of every round; the chosen cell
    against the next-highest over cell (not a pair of ``exempt``, nor two cells that differ only along an axis of length 1); in
    every fit the tests on the Hessian (``newton_step``) and the distance of every unclamped step from both bounds of the box, over
    half a map cell.  Below it a rounding error may change a count or a row."""
    Nb, Nd, m, phase, r, guard, train, rank, alpha = _settings(grid, top, oversample, method, pfa, guard, train, rank, psk,
                                                               noise_var is not None)
    iters, sweeps = _relax_settings((Nb, Nd), r, iters, sweeps)
    grid, D, Le, nf, nt = (Nb, Nd), Nb * Nd, int(top), r * Nb, r * Nd
    y, b = (np.asarray(v, dtype=np.complex128).reshape(-1) for v in (y, b))
    if len(y) != D or len(b) != D:
        raise ValueError(f"y and b must have {D} entries")
    none = CfarRelaxHost(np.full((Le, 3), np.nan), np.full(Le, np.nan + 0j), 0, 0, 0, math.nan, math.nan, DONE,
                         np.full((nf, nt), np.nan), math.inf, 0, 0)
    if symbols is not None:
        symbols = np.asarray(symbols).reshape(-1)
    if (symbols is not None and ((symbols < 0) | (symbols >= m)).any()) or (method == "known" and noise_var <= 0):
        return none._replace(state=OUTSIDE)
    if (not (np.isfinite(y).all() and np.isfinite(b).all()) or (symbols is None and (b == 0).any()) or
            (method == "known" and not math.isfinite(noise_var))):
        return none._replace(state=NONFINITE)
    x = y * np.conj(b / np.abs(b) if symbols is None else psk_points(m, phase)[symbols])
    rel = lambda a, c: np.abs(a - c) / np.where(np.maximum(a, c) > 0, np.maximum(a, c), 1.0)  # noqa: E731
    allowed = {tuple(sorted(pair)) for pair in exempt}
    offsets = window_offsets(grid, guard, train) if method != "known" else None
    targets, margin, not_definite, clamped, more, maps, first = [], math.inf, 0, 0, 0, 0, None

    def fitted(tau0, f0):
        nonlocal margin, not_definite, clamped
        tau, f, S, gap, nd, cl = fit(x, grid, r, tau0, f0, iters)
        margin, not_definite, clamped = min(margin, gap), not_definite + nd, clamped + cl
        return [tau, f, amplitude(S, D)]

    while True:
        P = periodogram(x, grid, r)
        maps += 1
        first = P if first is None else first
        Z = np.full_like(P, float(noise_var)) if method == "known" else noise_level(training_cells(threshold_map(P, first), offsets, r),
                                                                                    method, rank)
        threshold = alpha * Z
        over = is_over(P, threshold)
        margin = min(margin, float(np.where((P == 0) & (threshold == 0), np.inf, rel(P, threshold)).min()))
        if not over.any():
            break
        if limit_reached(len(targets), Le, False):
            more = 1
            break
        flat = candidates(P, over).ravel()
        order = sorted(np.flatnonzero(flat > -np.inf).tolist(),
                       key=functools.cmp_to_key(lambda c, d: -1 if beats(flat[c], c, flat[d], d) else 1))
        c = order[0]
        j, i = divmod(c, nt)
        for d in order[1:]:
            jd, i_d = divmod(d, nt)
            if tuple(sorted((c, d))) in allowed or (Nb == 1 and i == i_d) or (Nd == 1 and j == jd):
                continue
            margin = min(margin, float((flat[c] - flat[d]) / flat[c]))
            break
        t = fitted(i / nt, j / nf - 0.5)
        x = x - t[2] * atom(t[0], t[1], grid)
        if limit_reached(len(targets), Le, True):
            more = 1
            break
        targets.append(t)
        for _ in range(sweeps if len(targets) >= 2 else 0):
            for l, t in enumerate(targets):
                x = add_back(x, t[2], atom(t[0], t[1], grid))
                targets[l] = t = fitted(t[0], t[1])
                x = x - t[2] * atom(t[0], t[1], grid)
    rows, amp = np.full((Le, 3), np.nan), np.full(Le, np.nan + 0j)
    for l, (tau, f, c) in enumerate(targets):
        if tau < 0.0 or tau >= 1.0:
            tau -= math.floor(tau)
            tau = 0.0 if tau >= 1.0 else tau
        if f < -0.5 or f >= 0.5:
            f -= math.floor(f + 0.5)
            f = -0.5 if f >= 0.5 else f
        rows[l], amp[l] = (tau, f, abs(c) ** 2 * D), c
    level = float(noise_var) if method == "known" else float(Z.mean())
    return CfarRelaxHost(rows, amp, len(targets), more, maps, level, float((np.abs(x) ** 2).mean()), DONE, P, margin,
                         not_definite, clamped)
