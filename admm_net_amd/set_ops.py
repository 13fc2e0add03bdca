"""``ops.loss_set`` / ``ops.loss_set_bwd``: the torch wrappers of ``admmnet_loss_set_f32`` and its backward (csrc/loss_set.hip),
re-exported by ``admm_net_amd.ops``.  They follow the tensor-input contract of ``ops``: every input
passes through ``ops._f32`` / ``ops._num`` / ``ops._c64``, so a strided, offset, lazily conjugated or wider-dtype tensor gives the
bits of the plain tensor of the same value.  No host read, no synchronisation."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, ops

MAX_ROWS = 64                                       # SC_MAX of csrc/score_core.h: one lane per slot and per target
ROW = 6                                             # SET_COLS of csrc/set_core.h
ROW_NAMES = ("loss", "match", "conf", "norm", "outside", "nonfinite")


def set_options(scale=(1.0, 1.0), period=None, w_conf=0.1, lambda_reg=0.0):
    """(sx, sy, period_tau, period_f, w_conf, lambda_reg) as floats, checked: scales > 0, a period None / 0 (no wrap) or > 0,
    the two weights >= 0, all finite."""
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
    wc, lam = float(w_conf), float(lambda_reg)
    if not (sx > 0 and sy > 0 and math.isfinite(sx) and math.isfinite(sy)):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    if not (pt >= 0 and pf >= 0 and math.isfinite(pt) and math.isfinite(pf)):
        raise ValueError(f"a period must be 0 (none) or positive and finite, got {period!r}")
    if not (wc >= 0 and lam >= 0 and math.isfinite(wc) and math.isfinite(lam)):
        raise ValueError(f"w_conf and lambda_reg must be non-negative and finite, got {w_conf!r}, {lambda_reg!r}")
    return sx, sy, pt, pf, wc, lam


def _args(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg, w_conf, scale, period):
    """(lib, device, B, Lmax, Lt, D, the seven tensors as the kernels read them, the options as a host double[6])."""
    named = (("tau", tau), ("f", f), ("conf", conf), ("tau_true", tau_true), ("f_true", f_true), ("L_true", L_true), ("phi", phi))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        ops._need_cuda(t, name)
    opts = (ctypes.c_double * 6)(*set_options(scale, period, w_conf, lambda_reg))
    if tau.dim() != 2 or tau_true.dim() != 2 or phi.dim() != 2:
        raise ValueError(f"tau must be [B, Lmax], tau_true [B, Lt] and phi [B, D], got {tuple(tau.shape)}, {tuple(tau_true.shape)} "
                         f"and {tuple(phi.shape)}")
    if L_true.is_floating_point() or L_true.is_complex() or L_true.dtype == torch.bool:
        raise ValueError(f"L_true must hold integers, got {L_true.dtype}")
    dev, (B, Lmax), Lt, D = tau.device, tau.shape, tau_true.shape[1], phi.shape[1]
    if not (1 <= Lmax <= MAX_ROWS and 1 <= Lt <= MAX_ROWS and D >= 1 and B >= 1):
        raise ValueError(f"loss_set needs 1 <= Lmax, Lt <= {MAX_ROWS}, D >= 1, B >= 1, got Lmax={Lmax}, Lt={Lt}, D={D}, B={B}")
    with torch.cuda.device(dev):
        slots = [ops._f32(t, dev, (B, Lmax), name) for name, t in named[:3]]
        truths = [ops._f32(t, dev, (B, Lt), name) for name, t in named[3:5]]
        L_true = ops._num(L_true, dev, torch.int64, (B,), "L_true")
        phi = ops._c64(phi, dev, (B, D), "phi")
    return _lib.load(), dev, B, Lmax, Lt, D, (*slots, *truths, L_true, phi), opts


def loss_set(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg: float = 0.0, w_conf: float = 0.1, scale=(1.0, 1.0),
             period=None):
    """The assignment loss of the head (definition: include/admmnet.h, ``admmnet_loss_set_f32``).

    tau, f, conf [B, Lmax] float32; tau_true, f_true [B, Lt] float32; L_true [B] integers; phi [B, D] complex64; 1 <= Lmax, Lt <=
    64.  Returns (out [4] float32 = (total, match, conf, reg), assign [B, Lmax] int32 = the target of each slot or -1, norms [B]
    = ||phi_b|| for ``loss_set_bwd``, status [2] int32 = (signals with L_true outside [0, Lt], signals with a non-finite value),
    rows [B, 6] float64 = every signal's (loss_b, match_b, conf_b, ||phi_b||, outside, nonfinite))."""
    lib, dev, B, Lmax, Lt, D, t, opts = _args(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg, w_conf, scale, period)
    need = lib.admmnet_loss_set_partials(B)
    if need < 0:
        raise _lib.AdmmNetError(f"loss_set: bad size (B={B})")
    with torch.cuda.device(dev):
        out = torch.empty(4, dtype=torch.float32, device=dev)
        assign = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
        norms = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        rows = torch.empty(need, dtype=torch.float64, device=dev)
        _lib.check(lib.admmnet_loss_set_f32(Lmax, Lt, D, B, *(ops._ptr(x) for x in t), opts, ops._ptr(out), ops._ptr(assign),
                                            ops._ptr(norms), ops._ptr(status), ops._ptr(rows), ops._stream(dev)),
                   "admmnet_loss_set_f32")
    return out, assign, norms, status, rows.reshape(B, ROW)


def loss_set_bwd(g_out, tau, f, conf, tau_true, f_true, L_true, phi, assign, norms, lambda_reg: float = 0.0, w_conf: float = 0.1,
                 scale=(1.0, 1.0), period=None):
    """Backward of ``loss_set`` from g_out [4] and the ``assign`` and ``norms`` that call returned: (g_tau, g_f, g_conf [B, Lmax]
    float32, g_phi [B, D] complex64)."""
    lib, dev, B, Lmax, Lt, D, t, opts = _args(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg, w_conf, scale, period)
    for x, name in ((g_out, "g_out"), (assign, "assign"), (norms, "norms")):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
        ops._need_cuda(x, name)
    if assign.is_floating_point() or assign.is_complex() or assign.dtype == torch.bool:
        raise ValueError(f"assign must hold integers, got {assign.dtype}")
    with torch.cuda.device(dev):
        g_out, norms = ops._f32(g_out, dev, (4,), "g_out"), ops._f32(norms, dev, (B,), "norms")
        assign = ops._num(assign, dev, torch.int32, (B, Lmax), "assign")
        g_tau, g_f, g_conf = (torch.empty(B, Lmax, dtype=torch.float32, device=dev) for _ in range(3))
        g_phi = torch.empty(B, D, dtype=torch.complex64, device=dev)
        _lib.check(lib.admmnet_loss_set_bwd_f32(Lmax, Lt, D, B, ops._ptr(g_out), *(ops._ptr(x) for x in t), ops._ptr(assign),
                                                ops._ptr(norms), opts, ops._ptr(g_tau), ops._ptr(g_f), ops._ptr(g_conf),
                                                ops._ptr(g_phi), ops._stream(dev)), "admmnet_loss_set_bwd_f32")
    return g_tau, g_f, g_conf, g_phi
