"""Target estimates refined against the received signal on the device (csrc/refine.hip): the stage after the peak search.

``model.estimate`` ends with the peaks of ``|phi^H a(tau, f)|^2``; nothing looks at the received ``y`` again after the network.
``refine_targets`` fits the targets to ``y`` itself, a local maximum-likelihood fit started at the peaks (the definition is with
``admmnet_refine_f64`` in include/admmnet.h):

    mu_i(theta) = sum_l C_l exp(j 2 pi (i_b f_l - i_d tau_l)),   x_i = y_i conj(s_i),   Q(theta, s) = sum_i |x_i - mu_i(theta)|^2,

minimised over theta = (Re C, Im C, tau, f) by Gauss-Newton steps with Levenberg-Marquardt damping on the unit-diagonal normal
matrix, each step held to half a resolution cell.  The symbols s are either ``"given"`` (s = b / |b|, the demodulated symbols of the
generator, some of them wrong) or ``"psk"`` (re-decided before every linearisation as the constellation point nearest to
y_i conj(mu_i): the joint maximum-likelihood fit over symbols and targets, ``b`` only starts it).

``refine_targets``  the batch on the device, one kernel, no host read.
``refine_host``     the float64 numpy statement of the definition for ONE scene, written the other way round (the explicit D x P
                    Jacobian, ``np.exp``, theta ordered (tau, f, Re C, Im C)).  The tests hold the kernel to it; it is NOT a fallback --
                    the device call raises without the HIP library.

Tensor inputs follow INTEGRATION.md section 3: every pointer is taken through ``ops._c64`` / ``ops._num`` (``ops._plain``).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .metrics import MAX_TARGETS, PIVOT_MIN, _integers

STATES = ("converged", "limit", "gave up", "non-finite", "outside")
CONVERGED, LIMIT, GAVE_UP, NONFINITE, OUTSIDE = range(5)
MODES = {"given": 0, "psk": 1}
MAX_ITERS = 64
MAX_PSK = 64
LAMBDA_START = 1e-4
LAMBDA_MAX = 1e8
INFO = ("cost", "noise_var", "iterations", "flips", "state")


class RefineResult(NamedTuple):
    rows: torch.Tensor        # [B, Le, 3] float64 (tau, f, |C|): the order of the input rows, NaN on absent rows
    C: torch.Tensor           # [B, Le] complex128
    cost: torch.Tensor        # [B] float64: Q at the returned estimates
    noise_var: torch.Tensor   # [B] float64: Q / D -- feeds ``metrics.crb(..., noise_var=)`` unchanged
    iterations: torch.Tensor  # [B] int32: linearisations used
    flips: torch.Tensor       # [B] int32: entries whose final symbol differs from the constellation point nearest to b
    state: torch.Tensor       # [B] int32: the index into STATES
    status: torch.Tensor      # [4] int32 scenes: n_est outside 0 .. Le; non-finite; gave up; limit reached
    symbols: torch.Tensor     # [B, D] int32: the k of the final symbol ("given": of the point nearest to b); -1: scene not fitted


def _settings(grid, symbols, psk, iters, tol):
    try:
        Nb, Nd = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"grid must be a pair (Nb, Nd), got {grid!r}") from None
    if Nb < 1 or Nd < 1:
        raise ValueError(f"grid must be at least 1 x 1, got {grid!r}")
    if symbols not in MODES:
        raise ValueError(f"symbols must be one of {sorted(MODES)}, got {symbols!r}")
    try:
        m, phase = psk
        m, phase = int(m), float(phase)
    except (TypeError, ValueError):
        raise ValueError(f"psk must be a pair (points, phase of point 0), got {psk!r}") from None
    if not (2 <= m <= MAX_PSK and math.isfinite(phase)):
        raise ValueError(f"psk needs 2 .. {MAX_PSK} points and a finite phase, got {psk!r}")
    iters, tol = int(iters), float(tol)
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError(f"iters must be in 1 .. {MAX_ITERS}, got {iters}")
    if not (tol > 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be positive and finite, got {tol!r}")
    return Nb, Nd, m, phase, iters, tol


def _output(t, dev, dtype, shape, name):
    """A tensor the kernel is to write: exactly the dense tensor it writes, so a view of another dtype, device, shape or strides
    and a lazily conjugated or negated one are refused -- a copy would take the results."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype or t.device != dev or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.requires_grad:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev} that does not require grad, "
                         f"got {t.dtype} {tuple(t.shape)} with strides {t.stride()} on {t.device}")
    ops._no_lazy_bits(t, name)
    return t


def refine_targets(y, b, rows, grid, *, n_est=None, symbols="given", psk=(4, math.pi / 4), iters=16, tol=1e-6, out=None) -> RefineResult:
    """The targets of every scene fitted to its received signal (the module docstring has the definition), in one kernel and
    without a host read.

    y, b      [B, D] complex, D = Nb Nd: the received signal and the demodulated symbols, as ``synth.make_batch`` returns them.
    rows      [B, Le, 3] rows (tau, f, height) as ``ops.peak_top`` returns them -- the height is ignored, a row whose tau or f is
              not finite is absent -- 1 <= Le <= 16.
    grid      (Nb, Nd) = the (M, N) of a model.
    n_est     None or [B] integers: only the first n_est rows count; a scene whose n_est lies outside 0 .. Le is not fitted.
    symbols   "given" or "psk"; psk = (points, phase of point 0), the generator's QPSK by default.
    iters     linearisations at most, 1 .. 64; tol: the step in resolution cells at which a scene is converged.
    out       None, or a pair (rows [B, Le, 3] float64, C [B, Le] complex128) of device tensors to write the estimates into (the
              result holds these very tensors): dense and of exactly that dtype, anything else is refused with nothing written.

    ``noise_var`` with ``(rows[..., 0], rows[..., 1], C)`` feeds ``metrics.crb(..., noise_var=)`` unchanged: a predicted variance
    per estimate."""
    for t, name in ((y, "y"), (b, "b"), (rows, "rows")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    Nb, Nd, m, phase, iters, tol = _settings(grid, symbols, psk, iters, tol)
    D = Nb * Nd
    if not (y.is_complex() and b.is_complex()):
        raise ValueError(f"y and b must be complex, got {y.dtype} and {b.dtype}")
    if rows.is_complex() or rows.dtype == torch.bool:
        raise ValueError(f"rows must hold real numbers, got {rows.dtype}")
    if y.dim() != 2 or y.shape[1] != D:
        raise ValueError(f"y must be [B, {D}] for the grid {Nb} x {Nd}, got {tuple(y.shape)}")
    if rows.dim() != 3 or rows.shape[2] != 3 or rows.shape[0] != y.shape[0]:
        raise ValueError(f"rows must be [{y.shape[0]}, Le, 3], got {tuple(rows.shape)}")
    B, Le = rows.shape[:2]
    if not (1 <= Le <= MAX_TARGETS and B >= 1):
        raise ValueError(f"refine_targets needs 1 <= Le <= {MAX_TARGETS} and B >= 1, got Le={Le}, B={B}")
    lib = _lib.load()
    dev = y.device
    with torch.cuda.device(dev):
        y, b = ops._c64(y, dev, (B, D), "y"), ops._c64(b, dev, (B, D), "b")
        rows = ops._num(rows, dev, torch.float64, (B, Le, 3), "rows")
        if n_est is not None:
            _integers(n_est, "n_est")
            ops._need_cuda(n_est, "n_est")
            n_est = ops._num(n_est, dev, torch.int32, (B,), "n_est")
        if out is None:
            out, C = torch.empty(B, Le, 3, dtype=torch.float64, device=dev), torch.empty(B, Le, dtype=torch.complex128, device=dev)
        else:
            try:
                out, C = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (rows, C) of tensors") from None
            out, C = _output(out, dev, torch.float64, (B, Le, 3), "out rows"), _output(C, dev, torch.complex128, (B, Le), "out C")
        info = torch.empty(B, len(INFO), dtype=torch.float64, device=dev)
        sym = torch.empty(B, D, dtype=torch.int32, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_refine_f64(Nb, Nd, Le, B, ops._ptr(y), ops._ptr(b), ops._ptr(rows), ops._ptr(n_est), MODES[symbols], m,
                                          phase, iters, tol, ops._ptr(out), ops._ptr(C), ops._ptr(info), ops._ptr(sym),
                                          ops._ptr(status), ops._stream(dev)), "admmnet_refine_f64")
        counts = info[:, 2:].to(torch.int32)       # (NaN on a scene that was not fitted: 0 iterations, 0 flips)
    return RefineResult(out, C, info[:, 0], info[:, 1], counts[:, 0], counts[:, 1], counts[:, 2], status, sym)


# ---- the float64 host statement ------------------------------------------------------------------------------------------------------
class RefineHost(NamedTuple):
    rows: np.ndarray         # [Le, 3]
    C: np.ndarray            # [Le] complex128
    cost: float
    noise_var: float
    iterations: int
    flips: int
    state: int
    symbols: np.ndarray      # [D] int32
    moves: tuple             # the cells moved by every accepted step, in order
    start_cost: float        # Q at the starting (tau, f) with the least-squares C and the starting symbols


def psk_points(m, phase):
    return np.exp(1j * (2.0 * np.pi * np.arange(m) / m + phase))


def nearest_point(w, pts):
    """The k of the point nearest in angle to each w: the greatest Re(w conj(p_k)), the smaller k on ties."""
    return np.argmax((np.asarray(w)[..., None] * np.conj(pts)).real, axis=-1).astype(np.int32)


def signal_model(tau, f, C, grid):
    """(mu [D], J [D, P]) of the present targets, theta = (tau, f, Re C, Im C) with the columns of an axis of length 1 left out."""
    Nb, Nd = grid
    ib, idd = np.divmod(np.arange(Nb * Nd), Nd)
    E = np.exp(2j * np.pi * (np.multiply.outer(ib, f) - np.multiply.outer(idd, tau)))          # [D, L]
    cols = ([-2j * np.pi * idd[:, None] * C * E] if Nd > 1 else []) + ([2j * np.pi * ib[:, None] * C * E] if Nb > 1 else []) + [E, 1j * E]
    return E @ C, np.concatenate(cols, axis=1)


def linearise(tau, f, C, x, grid):
    """(Q, g, G) at theta: Q = sum |x - mu|^2, g = Re(J^H r), G = Re(J^H J)."""
    mu, J = signal_model(tau, f, C, grid)
    r = x - mu
    return float((np.abs(r) ** 2).sum()), (J.conj().T @ r).real, (J.conj().T @ J).real


def unit_diagonal(G):
    """(A, d): A = D G D with D = diag(d), d = diag(G)^-1/2; None where a diagonal entry is not positive and finite."""
    g = np.diag(G)
    if not (np.isfinite(G).all() and (g > 0).all()):
        return None
    d = 1.0 / np.sqrt(g)
    A = G * np.multiply.outer(d, d)
    np.fill_diagonal(A, 1.0)
    return A, d


def solve_spd(A, rhs):
    """A^-1 rhs, or None where a pivot of A's Cholesky is below 2^-40."""
    R = A.copy()
    for j in range(len(R)):
        if not R[j, j] >= PIVOT_MIN:
            return None
        R[j + 1:, j + 1:] -= np.multiply.outer(R[j + 1:, j], R[j + 1:, j]) / R[j, j]
    return np.linalg.solve(A, rhs)


def limit_step(dtau, df, grid, cells=0.5):
    """(scale, moved): the factor that holds every target's move to ``cells`` resolution cells, and the largest move after it."""
    Nb, Nd = grid
    moved = max(float(np.abs(dtau).max(initial=0.0)) * Nd, float(np.abs(df).max(initial=0.0)) * Nb)
    scale = cells / moved if moved > cells else 1.0
    return scale, moved * scale


def decide(y, x, mu, pts):
    """The symbols re-decided: the point nearest to y conj(mu) (x, the data with the present symbols removed, is not used)."""
    return nearest_point(y * np.conj(mu), pts)


def refine_host(y, b, rows, grid, *, n_est=None, symbols="given", psk=(4, math.pi / 4), iters=16, tol=1e-6) -> RefineHost:
    """``refine_targets`` for ONE scene in float64 numpy.  y, b [D]; rows [Le, 3]."""
    Nb, Nd, m, phase, iters, tol = _settings(grid, symbols, psk, iters, tol)
    grid, D = (Nb, Nd), Nb * Nd
    y, b = (np.asarray(v, dtype=np.complex128).reshape(-1) for v in (y, b))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    Le = len(rows)
    if len(y) != D or len(b) != D:
        raise ValueError(f"y and b must have {D} entries")
    nan_rows, nan_C = np.full((Le, 3), np.nan), np.full(Le, np.nan + 1j * np.nan)
    none = RefineHost(nan_rows, nan_C, math.nan, math.nan, 0, 0, CONVERGED, np.full(D, -1, dtype=np.int32), (), math.nan)
    n = Le if n_est is None else int(n_est)
    if not 0 <= n <= Le:
        return none._replace(state=OUTSIDE)
    if not (np.isfinite(y).all() and np.isfinite(b).all()) or (symbols == "given" and (b == 0).any()):
        return none._replace(state=NONFINITE)
    pts = psk_points(m, phase)
    k0 = nearest_point(b, pts)
    k = k0.copy()
    s = b / np.abs(b) if symbols == "given" else pts[k]
    x = y * np.conj(s)
    here = np.flatnonzero((np.arange(Le) < n) & np.isfinite(rows[:, 0]) & np.isfinite(rows[:, 1]))
    L = len(here)
    tau, f = rows[here, 0].copy(), rows[here, 1].copy()
    has_tau, has_f = Nd > 1, Nb > 1
    nt, nf = (L if has_tau else 0), (L if has_f else 0)

    def result(C, Q, it, state, moves, Q0):
        out, Cs = nan_rows.copy(), nan_C.copy()
        out[here, 0], out[here, 1], out[here, 2], Cs[here] = tau, f, np.abs(C), C
        return RefineHost(out, Cs, Q, Q / D, it, int((k != k0).sum()), state, k, tuple(moves), Q0)

    if L == 0:
        Q = float((np.abs(y) ** 2).sum())
        return result(np.zeros(0, dtype=np.complex128), Q, 0, CONVERGED, (), Q)
    # the starting C: least squares at the starting (tau, f)
    _, J = signal_model(tau, f, np.ones(L, dtype=np.complex128), grid)
    Jc = J[:, nt + nf:]
    start = unit_diagonal((Jc.conj().T @ Jc).real)
    c = None if start is None else solve_spd(start[0], start[1] * (Jc.conj().T @ x).real)
    if c is None:
        return result(nan_C[:L], math.nan, 0, GAVE_UP, (), math.nan)
    c = c * start[1]
    C = c[:L] + 1j * c[L:]
    Q, _, _ = linearise(tau, f, C, x, grid)
    Q0, lam, it, moves = Q, LAMBDA_START, 0, []
    while True:
        if it == iters:
            return result(C, Q, it, LIMIT, moves, Q0)
        it += 1
        if symbols == "psk":
            k = decide(y, x, signal_model(tau, f, C, grid)[0], pts)
            x = y * np.conj(pts[k])
        Q, g, G = linearise(tau, f, C, x, grid)
        scaled = unit_diagonal(G)
        if scaled is None:
            return result(C, Q, it, GAVE_UP, moves, Q0)
        A, d = scaled
        while True:
            step = solve_spd(A + lam * np.eye(len(A)), d * g)
            moved, Qt = math.inf, math.nan
            if step is not None:
                step = step * d
                dtau, df = step[:nt], step[nt:nt + nf]
                scale, moved = limit_step(dtau, df, grid)
                step = step * scale
                t_tau = tau + step[:nt] if has_tau else tau
                t_f = f + step[nt:nt + nf] if has_f else f
                t_C = C + step[nt + nf:nt + nf + L] + 1j * step[nt + nf + L:]
                Qt = linearise(t_tau, t_f, t_C, x, grid)[0]
            if Qt <= Q:
                tau, f, C, Q, lam = t_tau, t_f, t_C, Qt, lam / 10.0
                moves.append(moved)
                if moved <= tol:
                    return result(C, Q, it, CONVERGED, moves, Q0)
                break
            if moved <= tol:
                return result(C, Q, it, CONVERGED, moves, Q0)
            lam *= 10.0
            if lam > LAMBDA_MAX:
                return result(C, Q, it, GAVE_UP, moves, Q0)
