"""The reference's training losses (loss.py: ``BasicANMLoss``, ``PhiAlignmentLoss``, ``basic_parameter_loss``) with one forward
and one hand-written backward kernel each (csrc/loss.hip), in place of a Python loop over the samples of the batch.

Definitions, with B signals, Lmax target slots, L = L_true[b]:

    BasicANMLoss      loss_b = sum_j conf_j^2                                                            if L = 0
                      loss_b = mean_{j<L} (tau_j - tau_true_j)^2 + mean_{j<L} (f_j - f_true_j)^2
                               + 0.1 mean_{j<L} (conf_j - 1)^2                                           if L >= 1
                      param = mean_b loss_b,  reg = lambda_reg mean_b ||phi_b||_2,  total = param + reg
    PhiAlignmentLoss  amplitude = mean (|phi| - |phi_true|)^2,  phase = mean wrap(arg phi - arg phi_true)^2,
                      wrap(d) = ((d + pi) mod 2 pi) - pi (Python's %, so +pi maps to -pi),
                      total = amplitude_weight amplitude + phase_weight phase

Two sets of kernels evaluate them (in the manner of ``training.SmallKernels`` / ``TorchSmallKernels``): ``HipLossKernels`` (the
device entry points of ``ops``) and ``TensorLossKernels``, the same formulas as masked [B, Lmax] tensor operations without a
per-sample loop or a device-to-host read -- any device, any float dtype; the CPU tests' stand-in and, in float64, the yardstick
of the GPU tests.  The modules pick one by their ``route`` attribute ("hip", the default, or "tensor").

What differs from the reference's classes:
  * an ``L_true`` outside [0, Lmax] raises ``ValueError`` after ONE device-to-host read per call (``check_status = True``; the
    reference reads every sample's L).  ``check_status = False`` skips the read; such a sample is then evaluated with L held
    to [0, Lmax];
  * the targets are constants: one that requires grad raises ``ValueError`` (the kernels return no such gradient).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops

ROUTES = ("hip", "tensor")


class HipLossKernels:
    """The losses and their backwards on the HIP kernels of csrc/loss.hip, in the order of the comments below."""

    anm = staticmethod(ops.loss_anm)           # (tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg) -> out [3], norms, status
    anm_bwd = staticmethod(ops.loss_anm_bwd)   # (g_out, tau, ..., phi, norms, lambda_reg) -> g_tau, g_f, g_conf, g_phi
    phi = staticmethod(ops.loss_phi)           # (phi, phi_true, amplitude_weight, phase_weight) -> out [3]
    phi_bwd = staticmethod(ops.loss_phi_bwd)   # (g_out, phi, phi_true, amplitude_weight, phase_weight) -> g_phi


class TensorLossKernels:
    """The same forward / backward formulas as tensor operations, any device, in the dtype they are given."""

    @staticmethod
    def wrap(d):
        return torch.remainder(d + math.pi, 2 * math.pi) - math.pi

    @staticmethod
    def _anm_parts(tau, L_true):
        """(L held to [0, Lmax] as [B, 1], the mask j < L, the count of L_true outside the range)."""
        Lmax = tau.shape[1]
        L = L_true.clamp(0, Lmax).reshape(-1, 1)
        mask = (torch.arange(Lmax, device=tau.device) < L).to(tau.dtype)
        outside = ((L_true < 0) | (L_true > Lmax)).sum().to(torch.int32).reshape(1)
        return L, mask, outside

    @staticmethod
    def anm_terms(tau, f, conf, tau_true, f_true, L_true, phi):
        """(loss_b [B], ||phi_b|| [B], status [1]): the per-signal terms of the two batch means, none of them negative."""
        L, mask, outside = TensorLossKernels._anm_parts(tau, L_true)
        sq = (tau - tau_true) ** 2 + (f - f_true) ** 2 + 0.1 * (conf - 1) ** 2
        found = (sq * mask).sum(dim=1) / L.clamp(min=1).reshape(-1)
        loss_b = torch.where(L.reshape(-1) == 0, (conf ** 2).sum(dim=1), found)
        return loss_b, torch.sqrt((phi.real ** 2 + phi.imag ** 2).sum(dim=1)), outside

    @staticmethod
    def anm(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg):
        loss_b, norms, outside = TensorLossKernels.anm_terms(tau, f, conf, tau_true, f_true, L_true, phi)
        param, reg = loss_b.mean(), lambda_reg * norms.mean()
        return torch.stack([param + reg, param, reg]), norms, outside

    @staticmethod
    def anm_bwd(g_out, tau, f, conf, tau_true, f_true, L_true, phi, norms, lambda_reg):
        B = tau.shape[0]
        L, mask, _ = TensorLossKernels._anm_parts(tau, L_true)
        cp, cr = g_out[0] + g_out[1], g_out[0] + g_out[2]
        s = mask * (2 * cp / (L.clamp(min=1) * B))
        g_conf = torch.where(L == 0, 2 * cp / B * conf, s * (0.1 * (conf - 1)))
        live = (norms > 0).reshape(-1, 1)
        unit = phi / torch.where(live, norms.reshape(-1, 1), torch.ones_like(norms).reshape(-1, 1))
        g_phi = torch.where(live, (cr * lambda_reg / B) * unit, torch.zeros_like(phi))
        return s * (tau - tau_true), s * (f - f_true), g_conf, g_phi

    @staticmethod
    def phi_terms(phi, phi_true):
        """((|phi| - |phi_true|)^2, wrap(arg phi - arg phi_true)^2), both [B, D]: the terms of the two means."""
        w = TensorLossKernels.wrap(torch.angle(phi) - torch.angle(phi_true))
        return (phi.abs() - phi_true.abs()) ** 2, w ** 2

    @staticmethod
    def phi(phi, phi_true, amplitude_weight, phase_weight):
        a, p = TensorLossKernels.phi_terms(phi, phi_true)
        amp, ph = a.mean(), p.mean()
        return torch.stack([amplitude_weight * amp + phase_weight * ph, amp, ph])

    @staticmethod
    def phi_bwd(g_out, phi, phi_true, amplitude_weight, phase_weight):
        r = phi.abs()
        live = r > 0
        rs = torch.where(live, r, torch.ones_like(r))
        unit = phi / rs
        w = TensorLossKernels.wrap(torch.angle(phi) - torch.angle(phi_true))
        ca = (g_out[0] * amplitude_weight + g_out[1]) * (2.0 / phi.numel())
        cp = (g_out[0] * phase_weight + g_out[2]) * (2.0 / phi.numel())
        g = (ca * (r - phi_true.abs())) * unit + (cp * w / rs) * (1j * unit)      # i (x + i y) = -y + i x
        return torch.where(live, g, torch.zeros_like(phi))


def _kernels(route):
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")
    return HipLossKernels if route == "hip" else TensorLossKernels


def _constant(**targets):
    for name, t in targets.items():
        if t.requires_grad:
            raise ValueError(f"{name} requires grad: the losses treat their targets as constants and return no gradient for them")


def _g_out(grads, like):
    return torch.stack([g.to(like.dtype) for g in grads])


class _ANMLossFn(torch.autograd.Function):
    """(total, param, reg, status) of BasicANMLoss; gradients arriving through any of the first three are honoured."""

    @staticmethod
    def forward(ctx, tau, f, conf, phi, tau_true, f_true, L_true, lambda_reg, lk):
        out, norms, status = lk.anm(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg)
        ctx.save_for_backward(tau, f, conf, phi, tau_true, f_true, L_true, norms)
        ctx.lambda_reg, ctx.lk = lambda_reg, lk
        ctx.mark_non_differentiable(status)
        return (*out.unbind(0), status)

    @staticmethod
    def backward(ctx, g_total, g_param, g_reg, _g_status):
        tau, f, conf, phi, tau_true, f_true, L_true, norms = ctx.saved_tensors
        g = ctx.lk.anm_bwd(_g_out((g_total, g_param, g_reg), norms), tau, f, conf, tau_true, f_true, L_true, phi, norms,
                           ctx.lambda_reg)
        g_tau, g_f, g_conf, g_phi = (x.to(t.dtype) for x, t in zip(g, (tau, f, conf, phi)))
        return g_tau, g_f, g_conf, g_phi, None, None, None, None, None


class _PhiLossFn(torch.autograd.Function):
    """(total, amplitude, phase) of PhiAlignmentLoss."""

    @staticmethod
    def forward(ctx, phi, phi_true, amplitude_weight, phase_weight, lk):
        ctx.save_for_backward(phi, phi_true)
        ctx.weights, ctx.lk = (amplitude_weight, phase_weight), lk
        return tuple(lk.phi(phi, phi_true, amplitude_weight, phase_weight).unbind(0))

    @staticmethod
    def backward(ctx, g_total, g_amp, g_phase):
        phi, phi_true = ctx.saved_tensors
        g_phi = ctx.lk.phi_bwd(_g_out((g_total, g_amp, g_phase), g_total), phi, phi_true, *ctx.weights)
        return g_phi.to(phi.dtype), None, None, None, None


def _anm_loss(tau, f, conf, phi, tau_true, f_true, L_true, lambda_reg, route, check_status):
    _constant(tau_true=tau_true, f_true=f_true)
    total, param, reg, status = _ANMLossFn.apply(tau, f, conf, phi, tau_true, f_true, L_true, float(lambda_reg), _kernels(route))
    if check_status:
        bad = int(status.item())                       # the call's one device-to-host read
        if bad:
            raise ValueError(f"L_true of {bad} sample(s) lies outside [0, {tau.shape[1]}]")
    return total, param, reg


def basic_parameter_loss(tau_pred, f_pred, tau_true, f_true, confidences, L_true):
    """The ``param_loss`` of ``BasicANMLoss`` on its own (loss.py:6-30).  ``basic_parameter_loss.route`` and
    ``basic_parameter_loss.check_status`` select the kernels and the range check, as the modules' attributes do."""
    phi = torch.zeros(tau_pred.shape[0], 1, dtype=torch.complex128 if tau_pred.dtype == torch.float64 else torch.complex64,
                      device=tau_pred.device)
    return _anm_loss(tau_pred, f_pred, confidences, phi, tau_true, f_true, L_true, 0.0, basic_parameter_loss.route,
                     basic_parameter_loss.check_status)[1]


basic_parameter_loss.route = "hip"
basic_parameter_loss.check_status = True


class BasicANMLoss(nn.Module):
    def __init__(self, lambda_reg=1e-4):
        super().__init__()
        self.lambda_reg = lambda_reg
        self.route = "hip"
        self.check_status = True

    def forward(self, model_outputs, ground_truth):
        total, param, reg = _anm_loss(model_outputs['tau_est'], model_outputs['f_est'], model_outputs['confidences'],
                                      model_outputs['phi_final'], ground_truth['tau_true'], ground_truth['f_true'],
                                      ground_truth['L_true'], self.lambda_reg, self.route, self.check_status)
        return total, {'total_loss': total, 'param_loss': param, 'reg_loss': reg}


class PhiAlignmentLoss(nn.Module):
    def __init__(self, amplitude_weight=1.0, phase_weight=0.5, spectral_weight=0.2, distribution_weight=0.3):
        super().__init__()
        self.amplitude_weight = amplitude_weight
        self.phase_weight = phase_weight
        self.spectral_weight = spectral_weight              # (kept, unused, as in the reference)
        self.distribution_weight = distribution_weight
        self.route = "hip"

    def forward(self, phi_final, phi_true):
        _constant(phi_true=phi_true)
        if phi_final.shape != phi_true.shape or phi_final.dim() < 1:
            raise ValueError(f"phi_final and phi_true must have one shape, got {tuple(phi_final.shape)} and {tuple(phi_true.shape)}")
        if phi_final.dim() != 2:                            # a mean over all entries: any leading split into rows serves
            phi_final, phi_true = (t.reshape(t.shape[0], -1) for t in (phi_final, phi_true))
        total, amp, phase = _PhiLossFn.apply(phi_final, phi_true, float(self.amplitude_weight), float(self.phase_weight),
                                             _kernels(self.route))
        return total, {'total_loss': total, 'amplitude_loss': amp, 'phase_loss': phase}
