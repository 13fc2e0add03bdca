"""The opt-in rebinding behind ``--hip-optim`` / ``activate(optim=True)``: for this process ``torch.optim.AdamW`` and
``torch.nn.utils.clip_grad_norm_`` become the two wrappers below, so that the reference's

    optimizer = optim.AdamW([{'params': ..., 'lr': lr}, {'params': ..., 'lr': lr / 2}], weight_decay=...)
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    optimizer.step()

run on the kernels of ``admm_net_amd.optim`` unchanged.  A call outside the kernels' domain goes to torch's original: a norm
other than the 2-norm or a gradient that is not a contiguous float32 device tensor for the clipping, parameters that are not all
float32 device tensors for the optimiser.  That delegation lives here only; ``admm_net_amd.optim``'s own functions raise.
"""
import torch

from .. import optim as hip_optim

TORCH_ADAMW = hip_optim.AdamW.__mro__[1]                       # torch's class, whatever ``torch.optim.AdamW`` names by now
TORCH_CLIP = getattr(torch.nn.utils.clip_grad_norm_, "torch_original", torch.nn.utils.clip_grad_norm_)


def _on_kernels(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided


class _AdamWType(type):
    """``isinstance(opt, torch.optim.AdamW)`` stays true for what the rebound name constructs (both are torch's class or its
    subclass); a user's subclass of the rebound name keeps the ordinary rule."""

    def __instancecheck__(cls, obj):
        return isinstance(obj, TORCH_ADAMW) if cls is AdamW else super().__instancecheck__(obj)


class AdamW(TORCH_ADAMW, metaclass=_AdamWType):
    """The name ``torch.optim.AdamW`` after the rebinding, still a type.  Calling it gives an ``admm_net_amd.optim.AdamW`` where
    every parameter is a float32 device tensor and torch's own ``AdamW`` otherwise; a class derived from it is an ordinary
    subclass of torch's ``AdamW`` (its instances are built by torch's constructor, nothing is dispatched)."""

    def __new__(cls, params=None, *args, **kwargs):
        if cls is not AdamW:
            return super().__new__(cls)
        params = list(params)
        if params and isinstance(params[0], dict):               # groups: their lists may be generators, read them once
            params = [dict(g, params=[g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])) for g in params]
            flat = [p for g in params for p in g["params"]]
        else:
            flat = params
        flat = [p[1] if isinstance(p, tuple) else p for p in flat]   # (named parameters)
        if flat and all(_on_kernels(p) for p in flat):
            return hip_optim.AdamW(params, *args, **kwargs)      # (neither result is an instance of this class by type(), so
        return TORCH_ADAMW(params, *args, **kwargs)              #  Python does not call __init__ a second time)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``admm_net_amd.optim.clip_grad_norm_`` for the 2-norm of contiguous float32 device gradients, torch's own otherwise."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if float(norm_type) == 2.0 and grads and all(_on_kernels(g) and g.is_contiguous() and g.device == grads[0].device for g in grads):
        return hip_optim.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    return TORCH_CLIP(parameters, max_norm, norm_type, error_if_nonfinite, foreach)


clip_grad_norm_.torch_original = TORCH_CLIP


def rebind():
    torch.optim.AdamW = AdamW
    torch.nn.utils.clip_grad_norm_ = clip_grad_norm_
