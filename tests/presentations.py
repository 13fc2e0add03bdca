"""The forms in which a caller may hand one and the same VALUE to a device entry point (no test in this module).

The contract ("Tensor inputs"): for any tensor that is equal by value to a plain one --
contiguous, of the kernel's dtype, fresh, without conj or neg bit -- a non-in-place entry point gives the bits of the call on that
plain tensor.  Each form below maps a plain tensor X to one with ``torch.equal(form(X), X)`` and asserts, when it is built, the
property that defines it; ``NotApplicable`` says that X has no such form (a real tensor has no conj bit, one element has no
strides to speak of).  tests/test_presentations.py checks the forms and the helpers of ``ops`` against them on the host,
tests/test_gpu_presentations.py every entry point on the GPU.

    lazy_conj    X.conj().resolve_conj().conj(): the conj bit over the conjugate's memory              complex
    neg_view     torch._neg_view(-X): the neg bit over the negative's memory, contiguous               real, complex
    sliced       a window of a larger buffer filled with NaN (integers: the type's maximum)
    permuted     reversed (column-major) strides; 1-d: stride 2
    expanded     stride 0 along dim 0, as autograd's gradient of a sum; X must be constant along dim 0 (``constant_along0``)
    offset       contiguous, one element behind an aligned base
    wide         complex128 / float64 / int64 holding exactly the complex64 / float32 / int32 values
    leaf         requires_grad_(True)                                                                   real, complex
    conj_sliced  the conj bit AND the strides of ``sliced``                                             complex

``torch._neg_view`` is a private function of torch and the only route to a contiguous tensor with the neg bit; where the installed
torch lacks it, ``ABSENT`` names the form (tests/test_presentations.py reports it, nothing skips quietly).
"""
import ctypes

import torch


class NotApplicable(Exception):
    """X has no such form."""


def _kind(X):
    return "complex" if X.is_complex() else "real" if X.is_floating_point() else "int"


def _filler(X):
    if X.is_complex():
        return complex(float("nan"), float("nan"))
    if X.is_floating_point():
        return float("nan")
    if X.dtype == torch.bool:
        raise NotApplicable("a bool tensor has no filler that differs from every value")
    return torch.iinfo(X.dtype).max


def _same(v, X):
    assert v.shape == X.shape and v.device == X.device and torch.equal(v.detach(), X), "the form changed the value"
    return v


def lazy_conj(X):
    if not X.is_complex():
        raise NotApplicable("the conj bit exists on complex tensors only")
    v = X.conj().resolve_conj().conj()
    assert v.is_conj() and not v.is_neg()
    return _same(v, X)


def neg_view(X):
    if _kind(X) == "int":
        raise NotApplicable("lazy negation is used on floating-point and complex tensors")
    v = torch._neg_view(-X)
    assert v.is_neg() and v.is_contiguous() and not v.is_conj()
    return _same(v, X)


def sliced(X):
    if X.numel() < 2:
        raise NotApplicable("fewer than two elements are contiguous in every view")
    buf = torch.full([s + 2 for s in X.shape] + [2], _filler(X), dtype=X.dtype, device=X.device)
    window = tuple(slice(1, s + 1) for s in X.shape) + (1,)
    buf[window] = X
    v = buf[window]
    assert not v.is_contiguous() and v.data_ptr() != buf.data_ptr()
    return _same(v, X)


def permuted(X):
    if X.dim() == 0:
        raise NotApplicable("0-dim")
    if X.dim() == 1:
        if X.numel() < 2:
            raise NotApplicable("one element")
        buf = torch.zeros(2 * X.numel(), dtype=X.dtype, device=X.device)
        buf[::2] = X
        v = buf[::2]
        assert v.stride() == (2,)
    else:
        rev = tuple(reversed(range(X.dim())))
        v = X.permute(rev).contiguous().permute(rev)
        if v.is_contiguous():
            raise NotApplicable("the reversed strides of this shape are contiguous")
        assert v.stride()[0] == 1 or X.shape[0] == 1
    assert not v.is_contiguous()
    return _same(v, X)


def constant_along0(X):
    """The plain tensor ``expanded`` applies to: row 0 of X in every row."""
    return X if X.dim() == 0 else X[:1].expand(X.shape).contiguous()


def expanded(X):
    if X.dim() == 0 or X.shape[0] < 2 or X.numel() < 2:
        raise NotApplicable("needs a first dimension of at least two rows")
    if not torch.equal(X, constant_along0(X)):
        raise NotApplicable("the value is not constant along dim 0 (use constant_along0)")
    v = X[:1].clone().expand(X.shape)
    assert v.stride(0) == 0 and not v.is_contiguous()
    return _same(v, X)


def offset(X):
    buf = torch.zeros(X.numel() + 1, dtype=X.dtype, device=X.device)
    v = buf[1:].view(X.shape)
    v.copy_(X)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + X.element_size()
    return _same(v, X)


_WIDE = {torch.complex64: torch.complex128, torch.float32: torch.float64, torch.int32: torch.int64}


def wide(X):
    if X.dtype not in _WIDE:
        raise NotApplicable(f"{X.dtype} has no wider form here")
    v = X.to(_WIDE[X.dtype])
    assert v.dtype != X.dtype and torch.equal(v.to(X.dtype), X) and torch.equal(v, X.to(v.dtype))
    return v


def leaf(X):
    if _kind(X) == "int":
        raise NotApplicable("only floating-point and complex tensors require grad")
    v = X.detach().clone().requires_grad_(True)
    assert v.requires_grad and v.is_leaf
    return _same(v, X)


def conj_sliced(X):
    if not X.is_complex():
        raise NotApplicable("the conj bit exists on complex tensors only")
    v = sliced(X.conj().resolve_conj()).conj()
    assert v.is_conj() and not v.is_contiguous()
    return _same(v, X)


def wide_lazy_conj(X):
    """Not one of the listed forms: the composite that tells a helper whose dtype cast does the resolving from one that resolves
    (tests/test_presentations.py's mutation cases)."""
    if not X.is_complex():
        raise NotApplicable("the conj bit exists on complex tensors only")
    v = wide(X).conj().resolve_conj().conj()
    assert v.is_conj() and v.dtype != X.dtype
    return v


FORMS = {f.__name__: f for f in (lazy_conj, neg_view, sliced, permuted, expanded, offset, wide, leaf, conj_sliced)}
ABSENT = tuple(name for name, needs in (("neg_view", "_neg_view"),) if not hasattr(torch, needs))
REFUSAL_FORMS = ("lazy_conj", "neg_view", "sliced", "wide")           # what an in-place / output argument must refuse


def present(name, X):
    """``FORMS[name](X)``, or None where X has no such form."""
    try:
        return FORMS[name](X)
    except NotApplicable:
        return None


# ---- bits -----------------------------------------------------------------------------------------------------------------------
def raw_bytes(t, numel=None):
    """The ``numel`` elements behind ``t.data_ptr()`` of a HOST tensor as bytes, whatever its strides and bits say."""
    assert t.device.type == "cpu"
    n = (t.numel() if numel is None else numel) * t.element_size()
    return bytes((ctypes.c_char * n).from_address(t.data_ptr())) if n else b""


def plain_bytes(X, dtype=None):
    """The bytes a kernel must see for the value of X (in ``dtype``)."""
    X = X.detach().resolve_conj().resolve_neg().to(dtype or X.dtype).contiguous()
    return raw_bytes(X.clone())


def same_bits(a, b):
    """Equal shape, dtype and bits: NaN compared by mask (as tests/test_gpu_top_peaks.py does), everything else by its bytes, so
    -0.0 != 0.0."""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().resolve_conj().resolve_neg(), b.detach().resolve_conj().resolve_neg()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    if a.is_floating_point():
        nan = torch.isnan(a)
        if not torch.equal(nan, torch.isnan(b)):
            return False
        a, b = a.masked_fill(nan, 0.0), b.masked_fill(nan, 0.0)
    return raw_bytes(a) == raw_bytes(b)
