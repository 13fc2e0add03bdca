"""What every training script of the reference does after ``backward()`` (train.py:177-207, trainPhi.py:165-178),

    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    optimizer.step()                                  # optim.AdamW over two parameter groups

on the multi-tensor kernels of csrc/optim.hip: ``clip_grad_norm_`` and ``AdamW`` below, opt-in.  The model has some 250 small
parameter tensors; torch walks them in a dozen multi-tensor passes of several launches each, the kernels here take the whole
list in ceil(T / 256) + 1 launches for the norm and ceil(T / 64) for the update, which can apply the clipping as it reads the
gradients (``AdamW(..., max_grad_norm=1.0)``), so that the pair costs no launch more.

Definitions, per element in the parameter's dtype, with the scalars computed in Python double
(``torch.optim.adam._single_tensor_adam``: decoupled weight decay, not capturable, t = the parameter's step count AFTER it
advanced):

    p <- p (1 - lr wd);   m <- m + (g - m)(1 - beta1);   v <- beta2 v + (1 - beta2) g g
    p <- p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
    total_norm = sqrt(sum g^2) over ALL tensors (squares and sums in float64, rounded once to the gradients' dtype)
    coef = clamp(max_norm / (total_norm + 1e-6), max=1)       # torch's own expression, in the gradients' dtype

Two sets of kernels evaluate them, chosen by a ``route`` attribute as in ``losses``: ``HipOptimKernels`` (the device entry
points of ``ops``; float32 contiguous device tensors only -- anything else raises, there is no other path) and
``TensorOptimKernels``, the same formulas as tensor operations on any device in any float dtype: the CPU tests' stand-in and, in
float64, the yardstick of the GPU tests.
"""
from __future__ import annotations

import torch

from . import ops

ROUTES = ("hip", "tensor")


def _step_dtype():
    """The dtype torch gives a new ``step`` scalar: float32, or float64 under a float64 default dtype."""
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


def hyper_set(lr, beta1, beta2, eps, weight_decay, step):
    """The update's constants for one (group, step count) pair, in Python double, in the order of ``admmnet_adamw_hyper``."""
    return (1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5, eps)


class HipOptimKernels:
    """The norm, the scaling and the update on the HIP kernels of csrc/optim.hip."""

    gradnorm = staticmethod(lambda grads, max_norm: ops.optim_gradnorm(grads, max_norm)[:2])   # -> total_norm (0-dim), coef [1]
    scale = staticmethod(ops.optim_scale)       # (grads, coef): g <- g coef in place
    adamw = staticmethod(ops.optim_adamw)       # (params, grads, exp_avgs, exp_avg_sqs, hyper_index, hyper, coef=None), in place


class TensorOptimKernels:
    """The same formulas as tensor operations, any device, in the dtype they are given."""

    @staticmethod
    def gradnorm(grads, max_norm):
        sumsq = torch.stack([g.detach().double().square().sum() for g in grads]).sum()
        total = sumsq.sqrt().to(grads[0].dtype)
        return total, torch.clamp(max_norm / (total + 1e-6), max=1.0).reshape(1)

    @staticmethod
    def scale(grads, coef):
        for g in grads:
            g.mul_(coef.reshape(()).to(g.device))

    @staticmethod
    def adamw(params, grads, exp_avgs, exp_avg_sqs, hyper_index, hyper, coef=None):
        for p, g, m, v, i in zip(params, grads, exp_avgs, exp_avg_sqs, hyper_index):
            decay, omb1, beta2, omb2, step_size, bc2s, eps = hyper[i]
            if coef is not None:
                g = g * coef.reshape(()).to(g.device)
            p.mul_(decay)
            m.add_((g - m) * omb1)
            v.mul_(beta2).addcmul_(g, g, value=omb2)
            p.addcdiv_(m, (v.sqrt() / bc2s).add_(eps), value=-step_size)


def _kernels(route):
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")
    return HipOptimKernels if route == "hip" else TensorOptimKernels


_NONFINITE = ("The total norm of order {} for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
              "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` for the 2-norm: scales every gradient in place by ``coef`` and returns the total norm,
    a 0-dim tensor.  Two stream-ordered calls (norm, scaling) without a host read; ``error_if_nonfinite=True`` costs one.
    ``foreach`` is accepted and ignored.  ``clip_grad_norm_.route`` selects the kernels."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ computes the 2-norm only, got norm_type={norm_type!r}")
    k = _kernels(clip_grad_norm_.route)
    if not grads:
        return torch.tensor(0.0)
    total, coef = k.gradnorm(grads, float(max_norm))
    if error_if_nonfinite and not bool(torch.isfinite(total)):     # the call's one device-to-host read
        raise RuntimeError(_NONFINITE.format(float(norm_type)))
    k.scale(grads, coef)
    return total


clip_grad_norm_.route = "hip"


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` with ``step`` on the kernels above: the constructor, the parameter groups (with every key torch
    writes), ``zero_grad``, the per-parameter state {step: CPU float32 scalar, exp_avg, exp_avg_sq}, ``state_dict`` and
    ``load_state_dict`` are torch's own, so a checkpoint of either optimiser loads into the other and schedulers work on it.

    ``step`` takes, over ALL groups, the parameters that have a gradient (the others are left alone and their step count does
    not advance), advances their step counts on the host and updates them in ONE call, without a device-to-host read.
    ``max_grad_norm``: clip the 2-norm of all those gradients to it first, as ``clip_grad_norm_`` would, inside the update: the
    gradients themselves stay unscaled; ``last_grad_norm`` is then the total norm, a 0-dim device tensor.
    Not done, and refused with ``ValueError`` / ``TypeError`` at construction and again in ``step``: ``amsgrad``, ``maximize``,
    ``capturable``, ``differentiable``, coupled weight decay, a tensor ``lr`` or tensor betas; on ``route = "hip"`` also whatever
    is not a contiguous float32 device tensor.  ``foreach`` and ``fused`` are accepted and ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None, route="hip",
                 **torch_kwargs):
        _kernels(route)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **torch_kwargs)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.route = route
        self.last_grad_norm = None
        self._check_groups()

    def _check_groups(self):
        for i, group in enumerate(self.param_groups):
            for key in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(key):
                    raise ValueError(f"parameter group {i}: {key}=True is not implemented by admm_net_amd.optim.AdamW")
            if not group.get("decoupled_weight_decay", True):
                raise ValueError(f"parameter group {i}: coupled weight decay (Adam's) is not implemented by admm_net_amd.optim.AdamW")
            if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
                raise TypeError(f"parameter group {i}: a tensor lr or tensor betas would cost a device-to-host read per step; "
                                "pass Python floats")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        k = _kernels(self.route)
        params, grads, exp_avgs, exp_avg_sqs, index, hyper, sets = [], [], [], [], [], [], {}
        try:
            self._collect(params, grads, exp_avgs, exp_avg_sqs, index, hyper, sets)
            coef = None
            if self.max_grad_norm is not None and grads:
                self.last_grad_norm, coef = k.gradnorm(grads, self.max_grad_norm)
            if params:
                k.adamw(params, grads, exp_avgs, exp_avg_sqs, index, hyper, coef)
        except (TypeError, ValueError):                              # refused before anything ran: no step was taken
            for p in params:
                self.state[p]["step"] -= 1
            raise
        return loss

    def _collect(self, params, grads, exp_avgs, exp_avg_sqs, index, hyper, sets):
        """The lists of one update over all groups; advances the step count of every parameter it lists."""
        for gi, group in enumerate(self.param_groups):
            lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("admm_net_amd.optim.AdamW does not take sparse gradients")
                if p.grad.device != p.device:
                    raise ValueError(f"a parameter on {p.device} has its gradient on {p.grad.device}")
                state = self.state[p]
                if len(state) == 0:                                  # as torch creates it
                    state["step"] = torch.tensor(0.0, dtype=_step_dtype())
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if state["step"].device.type != "cpu":               # (a checkpoint of a capturable / fused torch optimiser)
                    state["step"] = state["step"].cpu()
                state["step"] += 1
                t = int(state["step"])                               # a host tensor: no device is asked
                if (gi, t) not in sets:
                    sets[gi, t] = len(hyper)
                    hyper.append(hyper_set(lr, beta1, beta2, eps, wd, t))
                params.append(p)
                grads.append(p.grad)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                index.append(sets[gi, t])
