"""GPU: every device entry point under ONE tensor-input contract (INTEGRATION.md "Tensor inputs").

For any tensor that is equal by value to a plain one -- contiguous, of the kernel's dtype, fresh, without conj or neg bit -- a
non-in-place entry point gives the BITS of the call on the plain tensor; an in-place or caller-owned output argument (Z, G, rn
of ``glayer_spectral``, the optimiser's lists, ``flat``, ``coef``) refuses, before any launch, a tensor the kernel could not write
faithfully.  The kernels' own arithmetic is pinned elsewhere; this file covers the path from a caller's tensor to the pointer a
kernel gets, with the forms of tests/presentations.py, at the smallest ragged shape each wrapper accepts: D = 7, B = 3 for the
``train_*``, loss and contraction kernels, D = 9 (3 x 3, K = 3) for the G-layer and the models, n = 8 for ``eigh``, the lists
of ``tests/test_gpu_optim.py::SHAPES`` for the optimiser.

``ROWS`` has one row per public function of ``admm_net_amd.ops`` (tests/test_presentations.py fails on a function without a row
or an exemption).  Per row: the plain outputs are finite and not all zero; every form applied to every input it applies to gives
the plain bits (on a mismatch the call is repeated one argument at a time, so the message names the argument); the inputs still
hold their values afterwards; every in-place argument refuses the forms of ``presentations.REFUSAL_FORMS`` with nothing written;
a call under a side stream gives the plain bits.  Above the table: the inference forward and ``estimate`` of both models on both
G-layer routes, the sharded engine, ``forward_autograd`` on the four training routes under a loss whose backward hands them
conj-bit, stride-0 gradients, the loss drop-ins and the optimiser.

Every comparison is of bits or of a raised exception; no tolerance appears.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import admm_net_amd as A
from admm_net_amd import losses, ops, optim, sharded, synth, training

import loss_cases
import presentations as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D, B, N = 7, 3, 8                  # n = D + 1 for the train_* kernels; n = 8 for eigh
GD, GN, GK, GB = 9, 10, 3, 5       # the G-layer and the models: 3 x 3, K = 3, B = 5
LH = 2                             # targets of the head
OPT_SHAPES = [(), (0,), (1,), (3,), (1023,), (1024,), (1025,), (4097,), (64, 100), (0, 5)]   # tests/test_gpu_optim.py::SHAPES


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def c(g, *s):
    return torch.randn(s, dtype=torch.complex64, generator=g)


def r(g, *s):
    return torch.randn(s, generator=g)


def pos(g, *s):
    return torch.rand(s, generator=g) + 0.5


def herm(X):
    return 0.5 * (X + X.transpose(-1, -2).conj())


@functools.lru_cache(maxsize=None)
def model(head=False, spectral=None, route=None):
    """3 x 3, K = 3; ``spectral``: None for the default options, 0 for ``Options(spectral=0)`` (the eigensolver route);
    ``route``: a train_route, with the parameters on the device."""
    torch.manual_seed(5)
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=3, N=3, num_layers=GK).eval()
    if spectral is not None:
        m.options = A.Options(spectral=spectral)
    if route is not None:
        m = m.to(DEV)
        m.train_route = route
    return m


def signals(seed=3):
    y, b, s, _ = synth.make_batch(GB, 3, 3, seed=seed)
    return dict(y=torch.from_numpy(y).to(torch.complex64), b=torch.from_numpy(b).to(torch.complex64),
                sigma=torch.from_numpy(s).to(torch.float32))


# ---- the table ------------------------------------------------------------------------------------------------------------------
class Row:
    """``build(g)``: {name: plain host tensor, list of tensors, or None}; ``call(t)``: the entry point on the namespace of device
    tensors.  ``io``: the in-place / caller-owned arguments (cloned for every call, part of the outputs, refusing);
    ``strict``: float64 arguments read without conversion (``ops._f64``: any strides, but no other dtype and no neg bit);
    ``wide_error``: what an ``io`` argument of the wider dtype raises, as the wrapper's docstring says; ``nan_ok``: outputs pad
    with NaN by definition; ``outputs``: picks what is compared out of the return value (default: all of it)."""

    def __init__(self, name, build, call, io=(), strict=(), wide_error=ValueError, nan_ok=False, outputs=None):
        self.name, self.build, self.call, self.io, self.strict = name, build, call, tuple(io), tuple(strict)
        self.wide_error, self.nan_ok, self.outputs = wide_error, nan_ok, outputs

    def plain(self, constant=False):
        t = self.build(_gen(sum(map(ord, self.name))))
        if constant:
            t = {k: _map(P.constant_along0, v) if k not in self.io else v for k, v in t.items()}
        return t

    def marks(self):
        """{argument: "in-place / output" | "strict float64 input" | "complex input" | "real input" | "float64 / int input"}."""
        out = {}
        for k, v in self.plain().items():
            x = v[0] if isinstance(v, list) else v
            if x is None:
                continue
            out[k] = ("in-place / output" if k in self.io else "strict float64 input" if k in self.strict else
                      "complex input" if x.dtype == torch.complex64 else "real input" if x.dtype == torch.float32 else
                      "float64 / int input")
        return out


def _map(f, v):
    return None if v is None else [f(x) for x in v] if isinstance(v, list) else f(v)


def _flat(out):
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


def _head_hp(g):
    return [0.2 * r(g, *s) for s in ops._head_shapes(D, LH)]


def _stepnet(g):
    return dict(W1=0.5 * r(g, 32, 3), b1=0.1 * r(g, 32), W2=0.5 * r(g, 1, 32), b2=0.1 * r(g, 1))


def _valnet(g):
    return dict(W1=r(g, 16, 1), b1=0.1 * r(g, 16), W2=0.5 * r(g, 1, 16), b2=0.1 * r(g, 1))


def _corrnet(g, bias=True):
    d = dict(W1=r(g, 64, D) / D ** 0.5, W2=r(g, D, 64) / 8)
    if bias:
        d.update(b1=0.1 * r(g, 64), b2=0.1 * r(g, D))
    return d


def _mats(g, *names):
    return {k: c(g, B, D + 1, D + 1) for k in names}


def _phih(g):
    return dict(phi=c(g, B, D), h=r(g, B, D))


def _anm(g):
    return loss_cases.anm_case(B, 2, D, seed=int(torch.randint(1 << 30, (1,), generator=g)), zero_row=False)


def _anm_bwd(t):
    out, norms, _ = ops.loss_anm(t.tau, t.f, t.conf, t.tau_true, t.f_true, t.L_true, t.phi, 1e-2)
    return ops.loss_anm_bwd(t.g_out, t.tau, t.f, t.conf, t.tau_true, t.f_true, t.L_true, t.phi, norms, 1e-2)


def _phase(g):
    phi, phi_true = loss_cases.phase_pair(B, D, seed=int(torch.randint(1 << 30, (1,), generator=g)), zeros=False)
    return dict(phi=phi, phi_true=phi_true)


def _keep(g):
    return (torch.rand(B, 4, D, generator=g) >= 0.25).to(torch.uint8)


def _head_bwd(t):
    saved = ops.train_head(t.phi, t.keep, 0.25, LH, t.hp)[3]
    return ops.train_head_bwd(t.g_tau, t.g_f, t.g_conf, t.phi, t.keep, 0.25, LH, t.hp, saved)


def _opt(g, *names):
    d = {k: [r(g, *s) for s in OPT_SHAPES] for k in names}
    if "v" in d:
        d["v"] = [x.abs() for x in d["v"]]
    return d


def _total(shapes):
    n = 0
    for s in shapes:
        k = 1
        for x in s:
            k *= x
        n += k
    return n


_HYPER = [optim.hyper_set(1e-3, 0.9, 0.999, 1e-8, 1e-2, 3)]


def _pair(g):
    rn = pos(g, B)
    return rn, torch.stack([rn.double().sum(), torch.tensor(float(B), dtype=torch.float64)])


def _with_pair(g, **more):
    rn, pair = _pair(g)
    return dict(rn=rn, pair=pair, **more)


def _glayer_inputs(g):
    return dict(phi=c(g, GB, GD), h=pos(g, GB, GD), Z=0.1 * herm(c(g, GB, GN, GN)))


def _spectral_inputs(g):
    return dict(phi=c(g, GB, GD), h=pos(g, GB, GD), Z=0.1 * herm(c(g, GB, GN, GN)), G=herm(c(g, GB, GN, GN)), rn=pos(g, GB),
                alpha=0.1 * pos(g, GB), phi_prev=c(g, GB, GD), h_prev=pos(g, GB, GD))


ROWS = {row.name: row for row in (
    # ---- eigensolver and contractions
    Row("eigh", lambda g: dict(A=herm(c(g, B, N, N))), lambda t: ops.eigh(t.A)),
    Row("vdvh", lambda g: dict(V=c(g, B, D, D), d=r(g, B, D)), lambda t: ops.vdvh(t.V, t.d)),
    Row("vhsv", lambda g: dict(V=c(g, B, D, D), S=herm(c(g, B, D, D))), lambda t: ops.vhsv(t.V, t.S)),
    # ---- csrc/train_layer.hip
    Row("train_matrix", lambda g: dict(**_phih(g), **_mats(g, "Z"), r=pos(g)),
        lambda t: ops.train_matrix(t.phi, t.h, t.Z, t.r, 0.5)),
    Row("train_matrix_bwd", lambda g: dict(**_mats(g, "gA", "Z"), r=pos(g)), lambda t: ops.train_matrix_bwd(t.gA, t.Z, t.r)),
    Row("train_resnorm", lambda g: dict(**_mats(g, "G"), **_phih(g)), lambda t: ops.train_resnorm(t.G, t.phi, t.h, 0.5)),
    Row("train_resnorm_bwd", lambda g: dict(g_rn=r(g, B), rn=pos(g, B), **_mats(g, "G"), **_phih(g)),
        lambda t: ops.train_resnorm_bwd(t.g_rn, t.rn, t.G, t.phi, t.h, 0.5)),
    Row("train_zupdate", lambda g: dict(**_mats(g, "Z", "G"), **_phih(g), s=pos(g, B)),
        lambda t: ops.train_zupdate(t.Z, t.G, t.phi, t.h, t.s, 0.5)),
    Row("train_zupdate_bwd", lambda g: dict(**_mats(g, "g", "G"), **_phih(g), s=pos(g, B)),
        lambda t: ops.train_zupdate_bwd(t.g, t.G, t.phi, t.h, t.s, 0.5)),
    Row("train_gather", lambda g: _mats(g, "X"), lambda t: ops.train_gather(t.X)),
    Row("train_scatter", lambda g: dict(g_col=c(g, B, D), g_dg=r(g, B, D)), lambda t: ops.train_scatter(t.g_col, t.g_dg)),
    Row("train_herm", lambda g: dict(**_mats(g, "g"), g_col=c(g, B, D), g_dg=r(g, B, D)),
        lambda t: ops.train_herm(t.g, t.g_col, t.g_dg)),
    # ---- csrc/train_small.hip, train_hlayer.hip, train_head.hip
    Row("train_phi", lambda g: dict(y=c(g, B, D), b=c(g, B, D), g_col=c(g, B, D), z_col=c(g, B, D), rho=r(g)),
        lambda t: ops.train_phi(t.y, t.b, t.g_col, t.z_col, t.rho)),
    Row("train_phi_bwd", lambda g: dict(g_phi=c(g, B, D), y=c(g, B, D), b=c(g, B, D), g_col=c(g, B, D), z_col=c(g, B, D), rho=r(g)),
        lambda t: ops.train_phi_bwd(t.g_phi, t.y, t.b, t.g_col, t.z_col, t.rho)),
    Row("train_hinput", lambda g: dict(g_dg=r(g, B, D), z_dg=r(g, B, D), rho=r(g)),
        lambda t: ops.train_hinput(t.g_dg, t.z_dg, t.rho)),
    Row("train_hinput_bwd", lambda g: dict(g_t=r(g, B, D), z_dg=r(g, B, D), rho=r(g)),
        lambda t: ops.train_hinput_bwd(t.g_t, t.z_dg, t.rho)),
    Row("train_hproject", lambda g: dict(t=pos(g, B, D), m=torch.tanh(r(g, B, D)), sigma=pos(g, B), pw=r(g)),
        lambda t: ops.train_hproject(t.t, t.m, t.sigma, t.pw)),
    Row("train_hproject_bwd", lambda g: dict(g_h=r(g, B, D), t=pos(g, B, D), m=torch.tanh(r(g, B, D)), sigma=pos(g, B), pw=r(g)),
        lambda t: ops.train_hproject_bwd(t.g_h, t.t, t.m, t.sigma, t.pw)),
    Row("train_hlayer", lambda g: dict(g_dg=pos(g, B, D), z_dg=0.1 * r(g, B, D), sigma=pos(g, B), rho=r(g), pw=r(g), **_corrnet(g)),
        lambda t: ops.train_hlayer(t.g_dg, t.z_dg, t.sigma, t.rho, t.pw, t.W1, t.b1, t.W2, t.b2)),
    Row("train_hlayer_bwd", lambda g: dict(g_h=r(g, B, D), z_dg=0.1 * r(g, B, D), sigma=pos(g, B), rho=r(g), pw=r(g),
                                           **_corrnet(g, bias=False), t=pos(g, B, D), a1=torch.relu(r(g, B, 64)),
                                           m=torch.tanh(r(g, B, D))),
        lambda t: ops.train_hlayer_bwd(t.g_h, t.z_dg, t.sigma, t.rho, t.pw, t.W1, t.W2, t.t, t.a1, t.m)),
    Row("train_head", lambda g: dict(phi=c(g, B, D), keep=_keep(g), hp=_head_hp(g)),
        lambda t: ops.train_head(t.phi, t.keep, 0.25, LH, t.hp), outputs=lambda out: out[:3]),   # ``saved``: see train_head_bwd
    Row("train_head_bwd", lambda g: dict(g_tau=r(g, B, LH), g_f=r(g, B, LH), g_conf=r(g, B, LH), phi=c(g, B, D), keep=_keep(g),
                                         hp=_head_hp(g)), _head_bwd),
    Row("train_eigmap", lambda g: dict(w=r(g, B, D + 1), thr=r(g), **_valnet(g)),
        lambda t: ops.train_eigmap(t.w, t.thr, t.W1, t.b1, t.W2, t.b2)),
    Row("train_eigmap_bwd", lambda g: dict(g_wp=r(g, B, D + 1), w=r(g, B, D + 1), thr=r(g), **_valnet(g)),
        lambda t: ops.train_eigmap_bwd(t.g_wp, t.w, t.thr, t.W1, t.b1, t.W2, t.b2)),
    Row("train_stepsize", lambda g: dict(rn=pos(g, B), rho=r(g), **_stepnet(g)),
        lambda t: ops.train_stepsize(t.rn, t.rho, t.W1, t.b1, t.W2, t.b2, 0.3)),
    Row("train_stepsize_bwd", lambda g: dict(g_step=r(g, B), rn=pos(g, B), rho=r(g), **_stepnet(g)),
        lambda t: ops.train_stepsize_bwd(t.g_step, t.rn, t.rho, t.W1, t.b1, t.W2, t.b2, 0.3)),
    # ---- the step size from a whole-batch pair
    Row("train_rnsum", lambda g: dict(rn=pos(g, B)), lambda t: ops.train_rnsum(t.rn)),
    Row("train_stepsize_pair", lambda g: _with_pair(g, rho=r(g), **_stepnet(g)),
        lambda t: ops.train_stepsize_pair(t.rn, t.pair, t.rho, t.W1, t.b1, t.W2, t.b2, 0.3), strict=("pair",)),
    Row("train_stepsize_bwd_pair_front", lambda g: _with_pair(g, g_step=r(g, B), rho=r(g), **_stepnet(g)),
        lambda t: ops.train_stepsize_bwd_pair_front(t.g_step, t.rn, t.pair, t.rho, t.W1, t.b1, t.W2, t.b2, 0.3), strict=("pair",)),
    Row("train_stepsize_bwd_pair_back", lambda g: dict(g_u=r(g, B), pair=_pair(g)[1], total=r(g, 1).double()),
        lambda t: ops.train_stepsize_bwd_pair_back(t.g_u, t.pair, t.total), strict=("pair", "total")),
    # ---- csrc/loss.hip
    Row("loss_anm", _anm, lambda t: ops.loss_anm(t.tau, t.f, t.conf, t.tau_true, t.f_true, t.L_true, t.phi, 1e-2)),
    Row("loss_anm_bwd", lambda g: dict(g_out=pos(g, 3), **_anm(g)), _anm_bwd),
    Row("loss_phi", _phase, lambda t: ops.loss_phi(t.phi, t.phi_true, 1.0, 0.5)),
    Row("loss_phi_bwd", lambda g: dict(g_out=pos(g, 3), **_phase(g)), lambda t: ops.loss_phi_bwd(t.g_out, t.phi, t.phi_true, 1.0, 0.5)),
    # ---- csrc/optim.hip: every tensor is the caller's own
    Row("optim_gradnorm", lambda g: _opt(g, "grads"), lambda t: ops.optim_gradnorm(t.grads, 1.0), io=("grads",),
        wide_error=TypeError),
    Row("optim_scale", lambda g: dict(**_opt(g, "grads"), coef=pos(g, 1)), lambda t: ops.optim_scale(t.grads, t.coef),
        io=("grads", "coef"), wide_error=TypeError),
    Row("optim_pack", lambda g: dict(**_opt(g, "tensors"), flat=r(g, _total(OPT_SHAPES) + 3)),
        lambda t: ops.optim_pack(t.tensors, t.flat), io=("tensors", "flat"), wide_error=TypeError),
    Row("optim_unpack", lambda g: dict(**_opt(g, "tensors"), flat=r(g, _total(OPT_SHAPES) + 3)),
        lambda t: ops.optim_unpack(t.tensors, t.flat), io=("tensors", "flat"), wide_error=TypeError),
    Row("optim_adamw", lambda g: dict(**_opt(g, "p", "g", "m", "v"), coef=pos(g, 1)),
        lambda t: ops.optim_adamw(t.p, t.g, t.m, t.v, [0] * len(OPT_SHAPES), _HYPER, t.coef), io=("p", "g", "m", "v", "coef"),
        wide_error=TypeError),
    # ---- the G-layer and the peak search
    Row("glayer", _glayer_inputs, lambda t: ops.glayer(model(), 1, t.phi, t.h, t.Z)),
    Row("glayer_spectral", _spectral_inputs,
        lambda t: ops.glayer_spectral(model(), 1, t.phi, t.h, t.Z, t.G, t.rn, 1, t.alpha, t.phi_prev, t.h_prev), io=("Z", "G", "rn")),
    Row("spectrum", lambda g: dict(phi=c(g, B, GD), taus=torch.rand(5, generator=g, dtype=torch.float64),
                                   fs=torch.rand(4, generator=g, dtype=torch.float64) - 0.5),
        lambda t: ops.spectrum(t.phi, 3, 3, t.taus, t.fs)),
    Row("peak_search", lambda g: dict(phi=c(g, B, GD)), lambda t: ops.peak_search(t.phi, 3, 3, max_peaks=16)),
    Row("peak_top", lambda g: dict(phi=c(g, B, GD), top_n=torch.tensor([3, 1, 2], dtype=torch.int32)),
        lambda t: ops.peak_top(t.phi, 3, 3, top=3, top_n=t.top_n), nan_ok=True),
    Row("regional_maxima", lambda g: dict(Z=torch.rand(B, 5, 7, generator=g, dtype=torch.float64)),
        lambda t: ops.regional_maxima(t.Z)),
)}

# public functions of ``ops`` that need no row, each with its reason (tests/test_presentations.py reads this)
EXEMPT = {}

FORM_NAMES = tuple(n for n in P.FORMS if n not in P.ABSENT)
STRICT_FORMS = ("sliced", "permuted", "expanded", "offset", "leaf")     # the forms that keep float64 and carry no neg bit


# ---- running a row --------------------------------------------------------------------------------------------------------------
def _forms_for(row, name, form):
    if name in row.io:
        return None
    if name in row.strict and form not in STRICT_FORMS:
        return None
    return form


def _present(form, X):
    """X on the device in ``form`` (None: plain, or no such form for X); returns (what is passed, whether the form applied)."""
    Xd = X.to(DEV).clone()
    v = None if form is None else P.present(form, Xd)
    return (Xd, False) if v is None else (v, True)


def run(row, plain, form=None, only=None, side_stream=False):
    """One call: the arguments of ``plain`` on the device, every input (or the one named ``only``) presented in ``form``.
    Returns (outputs, number of tensors the form applied to).  Asserts that every argument still has its value afterwards."""
    passed, applied = {}, 0
    for name, v in plain.items():
        f = _forms_for(row, name, form) if only in (None, name) else None
        if v is None:
            passed[name] = None
        elif isinstance(v, list):
            pairs = [_present(f, x) for x in v]
            passed[name], applied = [p for p, _ in pairs], applied + sum(a for _, a in pairs)
        else:
            passed[name], a = _present(f, v)
            applied += a
    torch.cuda.synchronize()
    if side_stream:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = row.call(SimpleNamespace(**passed))
        st.synchronize()
    else:
        out = row.call(SimpleNamespace(**passed))
    torch.cuda.synchronize()
    if row.outputs is not None:
        out = row.outputs(out)
    for name, v in plain.items():                                       # inputs are only read
        if name not in row.io and v is not None:
            for x, p in zip(v if isinstance(v, list) else [v], passed[name] if isinstance(v, list) else [passed[name]]):
                assert P.same_bits(p.detach().to(x.dtype), x), f"{row.name}: argument {name} changed under the call ({form})"
    return _flat(out) + [t for name in row.io for t in _flat(passed[name])], applied


@functools.lru_cache(maxsize=None)
def reference(name, constant=False):
    """The plain call's outputs, computed once per row (``constant``: on the inputs made constant along dim 0, for ``expanded``)."""
    row = ROWS[name]
    out, _ = run(row, row.plain(constant))
    return tuple(o.cpu() for o in out)


def _equal(got, want):
    return len(got) == len(want) and all(P.same_bits(a, b) for a, b in zip(got, want))


def applicable(row, form):
    """Whether ``form`` applies to at least one input of the row (decided on the host tensors)."""
    for name, v in row.plain(form == "expanded").items():
        if v is not None and _forms_for(row, name, form) is not None:
            if any(P.present(form, x) is not None for x in (v if isinstance(v, list) else [v])):
                return True
    return False


FORM_CASES = [(name, form) for name, row in ROWS.items() for form in FORM_NAMES if applicable(row, form)]


@pytest.mark.parametrize("name", list(ROWS))
def test_plain_outputs_are_finite_and_not_all_zero(name):
    row = ROWS[name]
    out = reference(name)
    assert out, name
    for i, o in enumerate(out):
        if o.numel() == 0 or not (o.is_floating_point() or o.is_complex()):
            continue
        x = torch.view_as_real(o) if o.is_complex() else o
        assert row.nan_ok or torch.isfinite(x).all(), f"{name}: output {i} is not finite"
        assert (torch.nan_to_num(x, nan=0.0) != 0).any(), f"{name}: output {i} is all zero"
    assert _equal(run(row, row.plain())[0], out), f"{name}: a second plain call gives other bits"


@pytest.mark.parametrize("name,form", FORM_CASES, ids=[f"{n}-{f}" for n, f in FORM_CASES])
def test_same_bits_per_form(name, form):
    row = ROWS[name]
    constant = form == "expanded"
    plain, want = row.plain(constant), reference(name, constant)
    got, applied = run(row, plain, form)
    assert applied > 0, (name, form)
    if not _equal(got, want):
        bad = [arg for arg in plain if arg not in row.io and plain[arg] is not None
               and not _equal(run(row, plain, form, only=arg)[0], want)]
        pytest.fail(f"{name}: the outputs differ from the plain call's under {form}; alone, the arguments {bad} differ")


def _refusals(row):
    out = []
    for arg in row.io:
        v = row.plain()[arg]
        for form in P.REFUSAL_FORMS:
            if form in P.ABSENT:
                continue
            idx = [i for i, x in enumerate(v if isinstance(v, list) else [v]) if P.present(form, x) is not None]
            if idx:
                out.append((row.name, arg, form, idx[-1]))
    return out


REFUSAL_CASES = [case for row in ROWS.values() for case in _refusals(row)]


@pytest.mark.parametrize("name,arg,form,idx", REFUSAL_CASES, ids=[f"{n}-{a}-{f}" for n, a, f, _ in REFUSAL_CASES])
def test_in_place_arguments_refuse(name, arg, form, idx):
    """An in-place / output argument in a form the kernel could not write faithfully raises before any launch (``ValueError``;
    ``TypeError`` for the wrong dtype where the wrapper's docstring says so), the argument and every other in-place argument
    keep their bits, and a plain call afterwards gives the plain bits."""
    row = ROWS[name]
    plain = row.plain()
    passed = {k: _map(lambda x: x.to(DEV).clone(), v) for k, v in plain.items()}
    X = passed[arg][idx] if isinstance(passed[arg], list) else passed[arg]
    bad = P.FORMS[form](X)
    if isinstance(passed[arg], list):
        passed[arg][idx] = bad
    else:
        passed[arg] = bad
    before = bad.detach().clone()
    with pytest.raises(row.wide_error if form == "wide" else ValueError):
        row.call(SimpleNamespace(**passed))
    torch.cuda.synchronize()
    assert P.same_bits(bad.detach().clone(), before), f"{name}: the refused {arg} was written"
    for k in row.io:
        for x, p in zip(_flat(plain[k]), _flat(passed[k])):
            assert P.same_bits(p.detach().to(x.dtype), x), f"{name}: {k} changed under a refused call"
    assert _equal(run(row, plain)[0], reference(name)), f"{name}: the plain call after the refusal gives other bits"


STRICT_CASES = [(row.name, arg) for row in ROWS.values() for arg in row.strict]


@pytest.mark.parametrize("name,arg", STRICT_CASES, ids=[f"{n}-{a}" for n, a in STRICT_CASES])
def test_strict_float64_arguments_refuse_what_they_would_misread(name, arg):
    """``ops._f64`` makes no conversion: float32 and, where torch has it, a lazily negated float64 raise ``ValueError``."""
    row = ROWS[name]
    plain = row.plain()
    for what, f in (("float32", lambda x: x.float()),) + ((("neg_view", P.neg_view),) if "neg_view" not in P.ABSENT else ()):
        passed = {k: _map(lambda x: x.to(DEV).clone(), v) for k, v in plain.items()}
        passed[arg] = f(passed[arg])
        with pytest.raises(ValueError):
            row.call(SimpleNamespace(**passed))
    assert _equal(run(row, plain)[0], reference(name))


@pytest.mark.parametrize("name", list(ROWS))
def test_on_a_side_stream(name):
    """tests/test_gpu_contract.py::test_on_a_side_stream for every row: one plain call under a side stream has the plain bits.
    ONE-SIDED: a wrapper that enqueues on another stream than the current one is caught only when the race loses -- when its
    kernel runs before the inputs are ready or the outputs are read before it ends; a race that happens to win passes."""
    row = ROWS[name]
    assert _equal(run(row, row.plain(), side_stream=True)[0], reference(name))


# ---- the models' inference forward and estimate ----------------------------------------------------------------------------------
MODELS = [(head, spectral) for head in (False, True) for spectral in (None, 0)]
MODEL_IDS = [f"{'ADMMNet' if h else 'PhiEstADMMNet'}-{'default' if s is None else 'spectral0'}" for h, s in MODELS]


def _signals(form=None, device=DEV):
    t = signals()
    if form == "expanded":
        t = {k: P.constant_along0(v) for k, v in t.items()}
    plain = {k: v.to(device).clone() for k, v in t.items()}
    formed = {k: (P.present(form, v) if form else None) for k, v in plain.items()}
    return plain, {k: plain[k] if formed[k] is None else formed[k] for k in plain}


def _infer(m, t):
    """(the forward's outputs, estimate's outputs) as one flat list of host tensors."""
    with torch.no_grad():
        out = _flat(m(t["y"], t["b"], t["sigma"])) + _flat(m.estimate(t["y"], t["b"], t["sigma"]))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


@functools.lru_cache(maxsize=None)
def _infer_reference(head, spectral, constant):
    return tuple(_infer(model(head, spectral), _signals("expanded" if constant else None)[0]))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("head,spectral", MODELS, ids=MODEL_IDS)
def test_model_inference_and_estimate(head, spectral, form):
    """``model(y, b, sigma)`` in eval mode and ``model.estimate`` with y, b, sigma in every form: the plain bits, on the
    matrix-function route (default) and on the eigensolver route (``Options(spectral=0)``)."""
    m = model(head, spectral)
    want = _infer_reference(head, spectral, form == "expanded")
    assert all(torch.isfinite(torch.view_as_real(o) if o.is_complex() else o.double()).any() for o in want)
    plain, formed = _signals(form)
    assert _equal(_infer(m, formed), want), f"{form}: y, b, sigma in this form give other bits"
    for k in plain:
        assert P.same_bits(formed[k].detach().to(plain[k].dtype), plain[k]), k


@pytest.mark.parametrize("form", ["lazy_conj", "sliced"])
@pytest.mark.parametrize("head,spectral", MODELS, ids=MODEL_IDS)
def test_model_inference_from_host_tensors(head, spectral, form):
    """Host tensors in ``lazy_conj`` / ``sliced`` form agree with the plain host call (the one host-to-device case)."""
    m = model(head, spectral)
    plain, formed = _signals(form, device="cpu")
    assert formed["y"] is not plain["y"]
    assert _equal(_infer(m, formed), _infer(m, plain))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("head", [False, True], ids=["PhiEstADMMNet", "ADMMNet"])
def test_sharded_engine_one_rank(head, form):
    """``sharded.ShardedForward`` over ``HipLayerEngine`` on one rank: the plain bits for every form of y, b, sigma."""
    fwd = sharded.ShardedForward(model(head), scope="global")

    def call(t):
        out = _flat(fwd(t["y"], t["b"], t["sigma"]))
        torch.cuda.synchronize()
        return [o.cpu().clone() for o in out]

    plain, formed = _signals(form)
    want = call(plain)
    assert all((torch.view_as_real(o) if o.is_complex() else o).abs().sum() > 0 for o in want)
    assert _equal(call(formed), want), form


# ---- autograd: gradients that arrive with the conj bit and stride 0 ---------------------------------------------------------------
@pytest.mark.parametrize("head", [False, True], ids=["PhiEstADMMNet", "ADMMNet"])
@pytest.mark.parametrize("route", training.TRAIN_ROUTES)
def test_autograd_functions_take_conj_bit_stride0_gradients(route, head):
    """``loss = phi.conj().sum().real (+ tau.sum() + f.sum() + conf.sum())``.  Without the head, autograd hands the route's
    functions a gradient of phi with the conj bit and strides 0; with it, the head's functions get stride-0 gradients of tau, f
    and conf (there phi's own gradient is the sum of two and arrives dense).  Hooks on phi / tau assert that this is what
    arrived -- otherwise the case tests nothing.  phi and every parameter gradient equal, bit for bit, those of the same forward
    under the resolved form ``(phi.conj().resolve_conj() * ones).sum().real + (tau * ones).sum() + ...`` with the watched
    gradient made a plain tensor of the same values on its way in (the hooks assert that too)."""
    m = model(head, None, route)
    t = {k: v.to(DEV) for k, v in signals().items()}
    params = [p for p in m.parameters() if p.requires_grad]

    def step(resolved):
        seen = []

        def hook(g):
            if resolved:
                g = g.resolve_conj().resolve_neg().contiguous().clone()
            seen.append((g.is_conj(), g.is_neg(), g.is_contiguous(), 0 in g.stride()))
            return g

        out = m.forward_autograd(t["y"], t["b"], t["sigma"])
        tau, f, conf, phi = out if head else (None, None, None, out)
        (tau if head else phi).register_hook(hook)
        if resolved:
            loss = (phi.conj().resolve_conj() * torch.ones_like(phi)).sum().real
            if head:
                loss = loss + sum((x * torch.ones_like(x)).sum() for x in (tau, f, conf))
        else:
            loss = phi.conj().sum().real
            if head:
                loss = loss + tau.sum() + f.sum() + conf.sum()
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        torch.cuda.synchronize()
        return [phi.detach().cpu()] + [None if g is None else g.cpu() for g in grads], seen

    got, seen = step(False)
    assert seen == [(not head, False, False, True)], f"the watched gradient did not arrive as meant: {seen}"
    want, seen_plain = step(True)
    assert seen_plain == [(False, False, True, False)], seen_plain
    assert any(g is not None and bool((g != 0).any()) for g in want[1:])
    names = ["phi"] + [n for n, p in m.named_parameters() if p.requires_grad]
    bad = [n for n, a, b in zip(names, got, want) if not P.same_bits(a, b)]
    assert not bad, f"{route}: these differ from the plain-gradient run: {bad}"


# ---- the loss drop-ins -----------------------------------------------------------------------------------------------------------
def _loss_inputs(kind):
    if kind == "anm":
        return loss_cases.anm_case(B, 2, D, seed=41, zero_row=False), ("tau", "f", "conf", "phi")
    phi, phi_true = loss_cases.phase_pair(B, D, seed=42, zeros=False)
    return dict(phi=phi, phi_true=phi_true), ("phi",)


def _loss_call(kind, t):
    if kind == "anm":
        total, parts = losses.BasicANMLoss(lambda_reg=1e-2)(
            dict(tau_est=t["tau"], f_est=t["f"], confidences=t["conf"], phi_final=t["phi"]),
            dict(tau_true=t["tau_true"], f_true=t["f_true"], L_true=t["L_true"]))
    else:
        total, parts = losses.PhiAlignmentLoss()(t["phi"], t["phi_true"])
    return total, [parts[k] for k in sorted(parts)]


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("kind", ["anm", "phi"])
def test_loss_drop_ins(kind, form):
    """``losses.BasicANMLoss`` / ``PhiAlignmentLoss`` (route "hip") with predictions and targets in every form: the loss and its
    parts have the plain bits, and so have the gradients of the predictions, which reach the plain leaves THROUGH the form.
    ``leaf`` applies to the predictions only (a target that requires grad is refused by design); under ``expanded`` the
    gradients are summed over the rows by the form itself, so only the forward is compared."""
    case, preds = _loss_inputs(kind)
    if form == "expanded":
        case = {k: P.constant_along0(v) for k, v in case.items()}

    def run_loss(form):
        leaves = {k: v.to(DEV).clone().requires_grad_(k in preds) for k, v in case.items()}
        t = dict(leaves)
        applied = 0
        for k, v in leaves.items():
            if form is None or (form == "leaf" and k not in preds):
                continue
            p = P.present(form, v.detach() if form == "leaf" else v)
            if p is not None:
                t[k], applied = p, applied + 1
        total, parts = _loss_call(kind, t)
        grads = torch.autograd.grad(total, [t[k] if form == "leaf" else leaves[k] for k in preds], allow_unused=True)
        torch.cuda.synchronize()
        return [total.detach()] + [p.detach() for p in parts], [g for g in grads], applied

    want, want_g, _ = run_loss(None)
    got, got_g, applied = run_loss(form)
    assert applied > 0 and all(torch.isfinite(o).all() and (o != 0).any() for o in want)
    assert _equal(got, want), f"{kind} under {form}: the loss differs"
    if form != "expanded":
        assert all(g is not None for g in want_g) and _equal(got_g, want_g), f"{kind} under {form}: the gradients differ"


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f for f in ("permuted", "neg_view") if f not in P.ABSENT])
def test_optimiser_refuses_a_gradient_it_could_not_read(form):
    """INTEGRATION.md ("Tensor inputs"): ``optim.AdamW.step`` and ``optim.clip_grad_norm_`` on route "hip" read the caller's own
    gradient memory, so a ``.grad`` with permuted strides or the neg bit raises ``ValueError`` before any launch: no parameter,
    state or step count moves, and the plain step afterwards has the bits of a plain step on a fresh optimiser."""
    g = _gen(77)
    P0, G0 = [r(g, 64, 100), r(g, 1025)], [r(g, 64, 100), r(g, 1025)]

    def fresh():
        params = [torch.nn.Parameter(p.to(DEV).clone()) for p in P0]
        for p, gr in zip(params, G0):
            p.grad = gr.to(DEV).clone()
        return params, optim.AdamW(params, lr=1e-2, max_grad_norm=1.0)

    params, opt = fresh()
    opt.step()
    torch.cuda.synchronize()
    want = [p.detach().cpu() for p in params] + [opt.last_grad_norm.cpu()]
    assert all(not P.same_bits(a, b) for a, b in zip(want, P0))

    params, opt = fresh()
    for i in range(len(params)):
        bad = P.FORMS[form](params[i].grad)
        assert torch.equal(bad, G0[i].to(DEV))
        good, params[i].grad = params[i].grad, bad
        with pytest.raises(ValueError):
            opt.step()
        with pytest.raises(ValueError):
            optim.clip_grad_norm_(params, 1.0)
        torch.cuda.synchronize()
        assert _equal([p.detach() for p in params], P0) and _equal([p.grad.detach().to(torch.float32) for p in params], G0)
        assert all(int(opt.state[p]["step"]) == 0 for p in params if opt.state[p])
        params[i].grad = good
    opt.step()
    torch.cuda.synchronize()
    assert _equal([p.detach().cpu() for p in params] + [opt.last_grad_norm.cpu()], want)
