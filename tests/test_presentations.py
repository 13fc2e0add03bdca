"""Host: the forms of tests/presentations.py, the input helpers of ``admm_net_amd.ops`` under them, mutation evidence, and the
completeness of the GPU table (tests/test_gpu_presentations.py).

The helpers -- ``ops._c64``, ``ops._f32``, ``ops._num``, all ``ops._plain`` -- are the only place a caller's input tensor becomes a
pointer.  Called here with ``dev = cpu``: the memory behind ``helper(form(x)).data_ptr()``, read raw through ctypes as ``numel``
elements, must hold the bits of x, and the result carries neither conj nor neg bit and no graph.  The stand-in helpers at the
bottom carry one mistake each; every one is rejected by a form that the test names.
"""
import inspect

import pytest
import torch

from admm_net_amd import ops

import presentations as P
import test_gpu_presentations as T

CPU = torch.device("cpu")


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


def _samples(dtype):
    """Plain tensors of ``dtype`` (the narrow one where ``wide`` applies): 0-dim, one element, 1-d, ragged 2-d and 3-d, and the
    same 2-d and 3-d made constant along dim 0 for ``expanded``."""
    g = _g(3)
    shapes = [(), (1,), (5,), (3, 7), (2, 3, 5), (1, 4)]
    if dtype.is_complex or dtype.is_floating_point:
        out = [torch.randn(s, dtype=dtype, generator=g) for s in shapes]
    else:
        out = [torch.randint(0 if dtype == torch.uint8 else -99, 100, s, dtype=dtype, generator=g) for s in shapes]
    return out + [P.constant_along0(out[3]), P.constant_along0(out[4])]


NARROW = (torch.complex64, torch.float32, torch.int32, torch.float64, torch.int64, torch.uint8)


def test_no_form_is_absent():
    """``torch._neg_view`` is private: should a torch without it be installed, this names the form that then goes untested."""
    assert P.ABSENT == (), f"the installed torch {torch.__version__} lacks what these forms need: {P.ABSENT}"


@pytest.mark.parametrize("name", list(P.FORMS))
def test_form_equals_its_plain_tensor_and_has_its_property(name):
    if name in P.ABSENT:
        pytest.fail(f"form {name} is absent from torch {torch.__version__}")
    applied = 0
    for dtype in NARROW:
        for X in _samples(dtype):
            keep = X.clone()
            v = P.present(name, X)
            if v is None:
                continue
            applied += 1
            assert v.shape == X.shape and torch.equal(v.detach(), X) and P.same_bits(X, keep)
            got = dict(lazy_conj=v.is_conj(), neg_view=v.is_neg() and v.is_contiguous(), sliced=not v.is_contiguous(),
                       permuted=not v.is_contiguous() and (X.dim() > 1 or v.stride() == (2,)),
                       expanded=v.dim() > 0 and v.stride(0) == 0,
                       offset=v.is_contiguous() and v.storage_offset() == 1,
                       wide=v.dtype != X.dtype and v.element_size() == 2 * X.element_size(),
                       leaf=v.requires_grad and v.is_leaf, conj_sliced=v.is_conj() and not v.is_contiguous())[name]
            assert got, (name, dtype, tuple(X.shape))
            if name == "sliced":                                     # the window lies inside a buffer of fillers
                base = v._base
                assert base is not None and base.numel() > 2 * X.numel()
                filler = base.flatten()[0]
                assert torch.isnan(torch.view_as_real(filler) if filler.is_complex() else filler).all() if dtype.is_complex or \
                    dtype.is_floating_point else filler == torch.iinfo(dtype).max
    assert applied >= 2, f"{name} applied to {applied} samples"
    # what a form does not apply to, by kind
    assert P.present("lazy_conj", torch.zeros(3)) is None and P.present("conj_sliced", torch.zeros(3)) is None
    assert P.present("expanded", torch.arange(6.0).reshape(3, 2)) is None
    assert P.present("wide", torch.zeros(3, dtype=torch.float64)) is None
    assert P.present("leaf", torch.zeros(3, dtype=torch.int32)) is None


def test_same_bits_is_exact():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert P.same_bits(a, a.clone()) and not P.same_bits(a, torch.tensor([-0.0, 1.0, float("nan")]))
    assert not P.same_bits(a, torch.tensor([0.0, 1.0, 2.0])) and not P.same_bits(a, a.double()) and not P.same_bits(a, a[:2])
    assert not P.same_bits(a, a + torch.tensor([0.0, 1.1920929e-07, 0.0]))
    z = torch.tensor([1 + 2j], dtype=torch.complex64)
    assert P.same_bits(z.conj().conj(), z) and not P.same_bits(z.conj(), z) and P.same_bits(None, None) and not P.same_bits(z, None)


# ---- the helpers ----------------------------------------------------------------------------------------------------------------
HELPERS = {
    "_c64": (lambda t: ops._c64(t, CPU), torch.complex64),
    "_f32": (lambda t: ops._f32(t, CPU), torch.float32),
    "_num-float64": (lambda t: ops._num(t, CPU, torch.float64), torch.float64),
    "_num-int32": (lambda t: ops._num(t, CPU, torch.int32), torch.int32),
    "_num-int64": (lambda t: ops._num(t, CPU, torch.int64), torch.int64),
}
ALL_FORMS = dict(P.FORMS, wide_lazy_conj=P.wide_lazy_conj)


def rejects(helper, dtype, form, samples=None):
    """The first sample on which ``helper(form(x))`` does not hold the bits of x plainly, or None.  ``helper`` may raise
    ``NotApplicable`` through the form; a form that applies to no sample fails the caller's count."""
    applied = 0
    for X in samples or _samples(dtype):
        try:
            v = ALL_FORMS[form](X)
        except P.NotApplicable:
            continue
        applied += 1
        out = helper(v)
        ok = (out.dtype == dtype and out.shape == X.shape and not out.is_conj() and not out.is_neg() and out.is_contiguous()
              and not out.requires_grad and out.device == CPU and out.data_ptr() % 16 == 0
              and P.raw_bytes(out, X.numel()) == P.plain_bytes(X, dtype))
        if not ok:
            return tuple(X.shape), applied
    return None, applied


@pytest.mark.parametrize("form", list(ALL_FORMS))
@pytest.mark.parametrize("helper", list(HELPERS))
def test_helper_hands_over_the_plain_bits(helper, form):
    if form in P.ABSENT:
        pytest.fail(f"form {form} is absent from torch {torch.__version__}")
    f, dtype = HELPERS[helper]
    bad, applied = rejects(f, dtype, form)
    assert bad is None, f"{helper} under {form}: the memory behind data_ptr() is not the plain tensor's at shape {bad}"
    if dtype in (torch.int64, torch.float64) and form in ("wide", "wide_lazy_conj") or not dtype.is_complex and "conj" in form or \
            not (dtype.is_complex or dtype.is_floating_point) and form in ("neg_view", "leaf"):
        assert applied == 0
    else:
        assert applied >= 2, (helper, form, applied)


def test_helpers_convert_between_dtypes_and_check_shapes():
    x = torch.randn(3, 4, generator=_g(1))
    assert P.raw_bytes(ops._num(x.double(), CPU, torch.float64)) == P.plain_bytes(x, torch.float64)
    assert P.raw_bytes(ops._f32(x.double().t().contiguous().t(), CPU)) == P.plain_bytes(x)
    assert P.raw_bytes(ops._c64(x, CPU)) == P.plain_bytes(x, torch.complex64)
    assert ops._f32(x, CPU).data_ptr() == x.data_ptr()                     # a plain tensor is handed over as it is, no copy
    z = torch.randn(5, dtype=torch.complex64, generator=_g(2))
    assert ops._c64(z, CPU, (5,), "z").data_ptr() == z.data_ptr()
    for helper in (ops._c64, ops._f32):
        with pytest.raises(ValueError, match=r"x must be \(4, 3\), got \(3, 4\)"):
            helper(x, CPU, (4, 3), "x")
    with pytest.raises(ValueError, match="top_n must be"):
        ops._num(torch.zeros(2, dtype=torch.int64), CPU, torch.int32, (3,), "top_n")


def test_in_place_checks_refuse_lazy_bits_on_the_host():
    """The refusals that need no device: ``_no_lazy_bits`` itself, ``_f64``, ``_optim_flat`` and ``_optim_coef`` with
    ``dev = cpu`` (``_optim_lists`` and ``glayer_spectral`` refuse a host tensor first; the GPU file covers them)."""
    if "neg_view" in P.ABSENT:
        pytest.fail(f"form neg_view is absent from torch {torch.__version__}")
    x = torch.randn(4, generator=_g(4))
    z = torch.randn(4, dtype=torch.complex64, generator=_g(5))
    with pytest.raises(ValueError, match="lazily conjugated"):
        ops._no_lazy_bits(P.lazy_conj(z), "Z")
    with pytest.raises(ValueError, match="lazily negated"):
        ops._no_lazy_bits(P.neg_view(x), "rn")
    ops._no_lazy_bits(x, "rn")
    ops._no_lazy_bits(z, "Z")
    pair = x[:2].double()
    assert ops._f64(pair, CPU, 2, "pair").data_ptr() == pair.data_ptr()
    assert P.raw_bytes(ops._f64(P.permuted(pair), CPU, 2, "pair")) == P.plain_bytes(pair)
    for bad in (P.neg_view(pair), pair.float(), x.double()):
        with pytest.raises(ValueError):
            ops._f64(bad, CPU, 2, "pair")
    assert ops._optim_flat("t", x, [x[:3]], CPU).data_ptr() == x.data_ptr()
    for bad, err in ((P.neg_view(x), ValueError), (P.permuted(x), ValueError), (x.double(), TypeError)):
        with pytest.raises(err):
            ops._optim_flat("t", bad, [x[:3]], CPU)
    coef = x[:1].clone()
    assert ops._optim_coef("t", coef, CPU).data_ptr() == coef.data_ptr()
    for bad, err in ((P.neg_view(coef), ValueError), (coef.double(), TypeError), (x, ValueError)):
        with pytest.raises(err):
            ops._optim_coef("t", bad, CPU)


# ---- mutation evidence: stand-in helpers with one mistake each ---------------------------------------------------------------------
def _right(t, dtype):
    t = t.detach().to(device=CPU, dtype=dtype).resolve_conj().resolve_neg().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


MUTANTS = {
    # name: (the stand-in, the dtype it serves, the form that must reject it)
    "the pre-change body of ops.eigh's preparation": (lambda t, d: t.to(d).contiguous(), torch.complex64, "lazy_conj"),
    "no resolve_conj": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_neg().contiguous(), torch.complex64, "lazy_conj"),
    "no resolve_neg": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_conj().contiguous(), torch.float32, "neg_view"),
    "no contiguous (sliced)": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_conj().resolve_neg(), torch.float32, "sliced"),
    "no contiguous (permuted)": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_conj().resolve_neg(), torch.complex64,
                                 "permuted"),
    "no contiguous (expanded)": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_conj().resolve_neg(), torch.float32,
                                 "expanded"),
    # .contiguous() first and the dtype cast left to do the resolving: the cast of a complex128 conj view does materialise it,
    # so ``wide_lazy_conj`` passes -- and the cast of a complex64 one is a no-op that keeps the bit, which ``lazy_conj`` sees
    "contiguous before the cast, the cast left to resolve": (lambda t, d: t.detach().contiguous().to(device=CPU, dtype=d),
                                                             torch.complex64, "lazy_conj"),
    "no dtype cast": (lambda t, d: t.detach().resolve_conj().resolve_neg().contiguous(), torch.float32, "wide"),
    "no realignment": (lambda t, d: t.detach().to(device=CPU, dtype=d).resolve_conj().resolve_neg().contiguous(), torch.complex64,
                       "offset"),
    "no detach": (lambda t, d: t.to(device=CPU, dtype=d).resolve_conj().resolve_neg().contiguous(), torch.float32, "leaf"),
}


def test_the_right_helper_passes_every_form():
    for dtype in (torch.complex64, torch.float32, torch.float64, torch.int32):
        for form in ALL_FORMS:
            assert rejects(lambda t: _right(t, dtype), dtype, form)[0] is None, (dtype, form)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_wrong_helper_is_rejected_by_a_named_form(name):
    mutant, dtype, form = MUTANTS[name]
    if form in P.ABSENT:
        pytest.fail(f"form {form} is absent from torch {torch.__version__}")
    bad, applied = rejects(lambda t: mutant(t, dtype), dtype, form)
    assert applied > 0 and bad is not None, f"'{name}' passes under {form}"
    print(f"'{name}' is rejected by {form} at shape {bad}")


def test_a_strided_conj_view_is_resolved_by_contiguous_itself():
    """Why ``conj_sliced`` does NOT reject the pre-change body (and why the wrappers before this contract were right for it):
    ``.contiguous()`` keeps the conj bit only where it has nothing to copy; the copy it makes of a strided view holds the value."""
    mutant, dtype, _ = MUTANTS["the pre-change body of ops.eigh's preparation"]
    x = torch.randn(3, 5, dtype=dtype, generator=_g(6))
    assert not P.conj_sliced(x).contiguous().is_conj() and P.lazy_conj(x).contiguous().is_conj()
    assert P.raw_bytes(mutant(P.conj_sliced(x), dtype)) == P.plain_bytes(x)
    assert P.raw_bytes(mutant(P.lazy_conj(x), dtype)) != P.plain_bytes(x)


def test_the_cast_first_mutant_passes_the_wide_composite():
    """Why the plain ``lazy_conj`` is needed next to ``wide``: the mutant that leaves the resolving to the cast is right on every
    wide input, the composite of the two included."""
    mutant, dtype, _ = MUTANTS["contiguous before the cast, the cast left to resolve"]
    assert rejects(lambda t: mutant(t, dtype), dtype, "wide_lazy_conj") == (None, 8)
    assert rejects(lambda t: mutant(t, dtype), dtype, "wide")[0] is None


# ---- completeness of the GPU table -------------------------------------------------------------------------------------------------
def _public_ops():
    return sorted(n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_"))


def test_every_public_entry_point_has_a_row_or_an_exemption():
    """Public: a function defined in ``admm_net_amd.ops`` without a leading underscore (all of them take tensors).  A new entry
    point without a row in tests/test_gpu_presentations.py::ROWS fails here, on the host."""
    names = _public_ops()
    assert len(names) >= 45 and "eigh" in names and "optim_adamw" in names
    missing = [n for n in names if n not in T.ROWS and n not in T.EXEMPT]
    assert not missing, f"no row and no exemption for: {missing}"
    assert all(isinstance(reason, str) and len(reason.split()) >= 3 and "\n" not in reason for reason in T.EXEMPT.values())
    stale = [n for n in list(T.ROWS) + list(T.EXEMPT) if n not in names]
    assert not stale, f"rows or exemptions for what ops no longer has: {stale}"
    assert not set(T.ROWS) & set(T.EXEMPT)


def test_every_row_marks_its_tensor_arguments_and_meets_a_form():
    kinds = {"in-place / output", "strict float64 input", "complex input", "real input", "float64 / int input"}
    for name, row in T.ROWS.items():
        marks = row.marks()
        assert marks and set(marks.values()) <= kinds, name
        assert all(a in marks for a in row.io + row.strict), name
        inputs = [a for a, k in marks.items() if k != "in-place / output"]
        forms = {f for n, f in T.FORM_CASES if n == name}
        assert (not inputs and not forms) or forms >= {"sliced", "permuted", "offset", "expanded"}, (name, forms)
        if "complex input" in marks.values():
            assert {"lazy_conj", "conj_sliced"} <= forms, name
        if row.io:
            assert {(a, f) for n, a, f, _ in T.REFUSAL_CASES if n == name} >= {(a, "neg_view") for a in row.io}, name
    # the in-place arguments the contract names
    assert T.ROWS["glayer_spectral"].io == ("Z", "G", "rn")
    assert all(T.ROWS[n].io for n in T.ROWS if n.startswith("optim_"))
