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
    for t, name in ((y, "y"), (b, "b")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    D, Le = Nb * Nd, int(top)
    if y.dim() != 2 or y.shape[1] != D or tuple(b.shape) != tuple(y.shape):
        raise ValueError(f"y and b must be [B, {D}] for the grid {Nb} x {Nd}, got {tuple(y.shape)} and {tuple(b.shape)}")
    if not (y.is_complex() and b.is_complex()):
        raise ValueError(f"y and b must be complex, got {y.dtype} and {b.dtype}")
    B = y.shape[0]
    if B < 1:
        raise ValueError("cfar_targets needs B >= 1")
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
    dev = y.device
    if out is not None:
        out = _output(out, dev, torch.float64, (B, Le, 3), "out")
    ops._need_cuda(y, "y")
    ops._need_cuda(b, "b")
    lib = _lib.load()
    with torch.cuda.device(dev):
        y, b = ops._c64(y, dev, (B, D), "y"), ops._c64(b, dev, (B, D), "b")
        if isinstance(noise_var, float):
            noise_var = torch.full((B,), noise_var, dtype=torch.float64, device=dev)
        elif noise_var is not None:
            ops._need_cuda(noise_var, "noise_var")
            noise_var = ops._num(noise_var, dev, torch.float64, (B,), "noise_var")
        if symbols is not None:
            ops._need_cuda(symbols, "symbols")
            symbols = ops._num(symbols, dev, torch.int32, (B, D), "symbols")
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
