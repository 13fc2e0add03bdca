"""``ops.loss_spectrum`` / ``ops.loss_spectrum_bwd``: the torch wrappers of ``admmnet_loss_spectrum_f64`` and its backward
(csrc/loss_spectrum.hip), re-exported by ``admm_net_amd.ops``.  They follow the tensor-input contract of ``ops`` (INTEGRATION.md
section 3): every input passes through ``ops._c64`` / ``ops._f32`` / ``ops._num``, so a strided, offset, lazily conjugated or
wider-dtype tensor gives the bits of the plain tensor of the same value.  No host read, no synchronisation."""
from __future__ import annotations

import torch

from . import _lib, ops

MAX_TARGETS, MAX_OVERSAMPLE = 16, 4                 # LS_MAX_TARGETS, LS_MAX_OVERSAMPLE of csrc/common.h


def _args(phi, truth, xbase, ybase, oversample, weights):
    """(lib, device, B, Lmax, workspace bytes, phi, (tau_true, f_true, L_true) or three Nones, the three weights)."""
    ops._need_cuda(phi, "phi")
    if phi.dim() != 2 or phi.shape[1] != xbase * ybase or phi.shape[0] < 1:
        raise ValueError(f"phi must be [B >= 1, {xbase} * {ybase}], got {tuple(phi.shape)}")
    if int(oversample) != oversample or not 1 <= oversample <= MAX_OVERSAMPLE:
        raise ValueError(f"oversample must be an integer in 1 .. {MAX_OVERSAMPLE}, got {oversample}")
    if len(weights) != 3:
        raise ValueError("weights must be (spectral_weight, distribution_weight, target_weight)")
    lib, dev, B = _lib.load(), phi.device, phi.shape[0]
    need = lib.admmnet_loss_spectrum_workspace_bytes(xbase, ybase, int(oversample), B)
    if need < 0:
        raise _lib.AdmmNetError(f"loss_spectrum: a {xbase} x {ybase} grid at oversample {oversample} does not fit the kernels")
    Lmax, targets = 0, (None, None, None)
    with torch.cuda.device(dev):
        phi = ops._c64(phi, dev, (B, xbase * ybase), "phi")
        if truth is not None:
            tau_true, f_true, L_true = truth
            for t, name in ((tau_true, "tau_true"), (f_true, "f_true"), (L_true, "L_true")):
                ops._need_cuda(t, name)
            if tau_true.dim() != 2 or not 1 <= tau_true.shape[1] <= MAX_TARGETS:
                raise ValueError(f"tau_true must be [B, 1 <= Lmax <= {MAX_TARGETS}], got {tuple(tau_true.shape)}")
            if L_true.is_floating_point() or L_true.is_complex() or L_true.dtype == torch.bool:
                raise ValueError(f"L_true must hold integers, got {L_true.dtype}")
            Lmax = tau_true.shape[1]
            targets = (ops._f32(tau_true, dev, (B, Lmax), "tau_true"), ops._f32(f_true, dev, (B, Lmax), "f_true"),
                       ops._num(L_true, dev, torch.int64, (B,), "L_true"))
    return lib, dev, B, Lmax, need, phi, targets, tuple(float(w) for w in weights)


def loss_spectrum(phi, phi_true, truth, xbase: int, ybase: int, weights, oversample: int = 2):
    """The spectral, distribution and target terms of ``losses.PhiSpectralLoss`` (definitions: include/admmnet.h).

    phi [B, ybase * xbase] complex64; phi_true the same or None (no grid terms); truth None (no target term) or (tau_true,
    f_true [B, Lmax <= 16] float32, L_true [B] integers); weights = (spectral, distribution, target).  Returns (out [4] float32 =
    (total, spectral, distribution, target), the workspace ``loss_spectrum_bwd`` reads, status [3] int32 = (L_true outside
    [0, Lmax], zero phi rows, zero phi_true rows))."""
    if phi_true is None and truth is None:
        raise ValueError("loss_spectrum needs phi_true, truth or both")
    lib, dev, B, Lmax, need, phi, targets, w = _args(phi, truth, xbase, ybase, oversample, weights)
    with torch.cuda.device(dev):
        if phi_true is not None:
            ops._need_cuda(phi_true, "phi_true")
            phi_true = ops._c64(phi_true, dev, tuple(phi.shape), "phi_true")
        out = torch.empty(4, dtype=torch.float32, device=dev)
        status = torch.empty(3, dtype=torch.int32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(lib.admmnet_loss_spectrum_f64(xbase, ybase, int(oversample), Lmax, B, ops._ptr(phi), ops._ptr(phi_true),
                                                 *(ops._ptr(t) for t in targets), *w, ops._ptr(out), ops._ptr(status),
                                                 ops._ptr(ws), need, ops._stream(dev)), "admmnet_loss_spectrum_f64")
    return out, ws, status


ROW = 48                                            # LS_ROW of csrc/loss_spectrum.hip


def loss_spectrum_rows(workspace, xbase: int, ybase: int, oversample: int, B: int) -> torch.Tensor:
    """The per-signal rows the forward left in its workspace, as a float64 [B, 48] view: columns 0 .. 2 the signal's spectral,
    distribution and target term, 3 .. 5 its three status flags, then the scalars of the backward and z at the targets."""
    align = lambda v: (v + 255) // 256 * 256
    nx, ny = (oversample * xbase if xbase > 1 else 1), (oversample * ybase if ybase > 1 else 1)
    start = align(16 * nx * xbase) + align(16 * ny * ybase) + align(8 * (nx + ny))
    return workspace[start:start + 8 * ROW * B].view(torch.float64).reshape(B, ROW)


def loss_spectrum_bwd(g_out, phi, truth, xbase: int, ybase: int, weights, oversample: int, workspace, skip: int = 0):
    """Backward of ``loss_spectrum`` from g_out [4] and the workspace that call returned (left unchanged): g_phi [B, D]
    complex64.  ``skip``: bit 0 the spectral, bit 1 the distribution, bit 2 the target term is left out of the gradient; the
    terms the forward did not evaluate (phi_true or truth None there) add nothing whatever ``skip`` says."""
    if truth is None:
        skip |= 4
    lib, dev, B, Lmax, need, phi, targets, w = _args(phi, None if skip & 4 else truth, xbase, ybase, oversample, weights)
    ops._need_cuda(g_out, "g_out")
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev or \
            workspace.numel() != need or not workspace.is_contiguous():
        raise ValueError(f"workspace must be the uint8 tensor of {need} bytes that loss_spectrum returned for these sizes")
    with torch.cuda.device(dev):
        g_out = ops._f32(g_out, dev, (4,), "g_out")
        g_phi = torch.empty_like(phi)
        _lib.check(lib.admmnet_loss_spectrum_bwd_f64(xbase, ybase, int(oversample), Lmax, B, ops._ptr(g_out), ops._ptr(phi),
                                                     *(ops._ptr(t) for t in targets), *w, int(skip), ops._ptr(workspace), need,
                                                     ops._ptr(g_phi), ops._stream(dev)), "admmnet_loss_spectrum_bwd_f64")
    return g_phi
