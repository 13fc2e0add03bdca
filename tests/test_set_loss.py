"""CPU: the assignment loss of the head (``losses.SetANMLoss``, csrc/loss_set.hip) without a GPU -- the float64 host statement
``losses.set_assign_host`` against the enumeration of the definition written here, the tensor formulation
(``TensorLossKernels.set`` / ``set_bwd``, the stand-in for the kernels) against an explicit per-signal loop, autograd through it
and central differences, the scalar core csrc/set_core.h under the sanitizers on the whole table, one-mistake stand-ins that a
named case each rejects, the module's surface and the C entry points' refusals.

Every comparison of an assignment rests on the margin of tests/set_loss_cases.py: ``test_every_case_keeps_its_margin`` asserts it
for every case the CPU and the GPU tests use, none left out.
Tolerances: float64 against float64 at 1e-12 of the largest entry; the host model's values within 64 x 2^-53 of the sum of the
magnitudes of their terms (the sums run in another order there).
"""
import ctypes
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, losses, metrics, ops
from admm_net_amd.losses import TensorLossKernels as TLK

import set_loss_cases as SC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host_model")
F64 = 1e-12
SMALL = [s for s in SC.SHAPES if max(s) <= 5]
UP = (1.7, 0.3, -0.6, 0.9)


# ---- the definition, written out: one signal, every assignment -------------------------------------------------------------------
def _wrap(d, P):
    return d - P * np.floor(d / P + 0.5) if P > 0 else d


def enumerate_definition(tau, f, conf, tau_true, f_true, n, *, w_conf, scale, period, mistake=None, **_):
    """(least value, its assign) of the definition over ALL assignments of k = min(Lmax, n) slots to targets j < n.  ``mistake``: one
    of MISTAKES, a stand-in that gets one thing wrong."""
    tau, f, conf, tau_true, f_true = (np.asarray(v, dtype=np.float64) for v in (tau, f, conf, tau_true, f_true))
    Lmax, Lt = len(tau), len(tau_true)
    n = min(max(int(n), 0), Lt)
    pool = Lt if mistake == "truths past n used" else n
    pt, pf = (0.0, 0.0) if period is None or mistake == "no wrap" else period
    k = min(Lmax, pool)
    best = (np.inf, None, None)
    for slots in itertools.combinations(range(Lmax), k):
        for targets in itertools.permutations(range(pool), k):
            d2 = sum((scale[0] * _wrap(tau[i] - tau_true[j], pt)) ** 2 + (scale[1] * _wrap(f[i] - f_true[j], pf)) ** 2
                     for i, j in zip(slots, targets))
            t = np.zeros(Lmax)
            t[list(targets) if mistake == "t on the target's index" and k and max(targets) < Lmax else list(slots)] = 1.0
            sq = (conf - t) ** 2
            if mistake == "unmatched slots without a conf target":
                sq = sq * t
            match = d2 / max(k if mistake == "a normaliser of k" else n, 1)
            value = match + w_conf * sq.sum() / Lmax
            if mistake == "the sign of the per-slot term":       # the search sees c_ij with + (w_conf / Lmax)(1 - 2 conf) flipped
                key = match - w_conf / Lmax * sum(1 - 2 * conf[i] for i in slots)
            elif mistake == "matching on d2 alone":
                key = match
            else:
                key = value
            if key < best[0]:
                assign = np.full(Lmax, -1, dtype=np.int32)
                assign[list(slots)] = targets
                best = (key, value, assign)
    return best[1], best[2]


def _signal(c, b):
    return [c[k][b].double().numpy() for k in SC.KEYS[:5]] + [int(c["L_true"][b])]


# ---- 1. the margin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SC.BATCHES)
def test_every_case_keeps_its_margin(B):
    """No case is left out: every signal of every case of the table, at every batch size the GPU test runs, has its second-best
    assignment at least 1e-9 (relative) above the optimum; so have the designed cases.  The ties have a gap of exactly 0."""
    least = np.inf
    for Lmax, Lt in SC.SHAPES:
        for v in SC.variants_of(B):
            gaps = SC.margins(SC.table_case(B, Lmax, Lt, v), **SC.options(v))
            assert SC.gap_is_kept(gaps), (B, Lmax, Lt, v, min(gaps))
            least = min([least] + gaps)
    print(f"B={B}: the least relative gap of the table is {least:.3e}")
    if B == 1:
        for name, (c, o, _) in SC.DESIGNED.items():
            assert SC.gap_is_kept(SC.margins(c, **o)), name
        for name, (c, o) in SC.TIES.items():
            assert SC.margins(c, **o) == [0.0], name
        for c, o in (SC.with_bad_values()[:2], SC.out_of_range()[:2], (SC.out_of_range()[2], SC.out_of_range()[1])):
            assert SC.gap_is_kept(SC.margins(c, **o))


def test_the_periodic_cases_hold_pairs_across_the_wrap():
    for Lmax, Lt in SC.SHAPES[3:]:
        for v in ("periodic", "periodic-w5-scaled-all"):
            assign = SC.reference(5, Lmax, Lt, v)[1]
            assert SC.crosses_the_wrap(SC.table_case(5, Lmax, Lt, v), assign, SC.VARIANTS[v][3]) >= 1, (Lmax, Lt, v)


# ---- 2. the host statement against the enumeration ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Lmax,Lt", SMALL)
def test_set_assign_host_equals_the_enumeration(Lmax, Lt):
    for v in SC.VARIANTS:
        c, o = SC.table_case(5, Lmax, Lt, v), SC.options(v)
        for b in range(5):
            s = _signal(c, b)
            assign, value = losses.set_assign_host(*s, w_conf=o["w_conf"], scale=o["scale"], period=o["period"])
            want_value, want_assign = enumerate_definition(*s, **o)
            assert np.array_equal(assign, want_assign), (v, b)
            assert abs(value - want_value) <= F64 * max(want_value, 1e-300), (v, b)


def test_the_designed_cases_and_the_ties():
    for name, (c, o, want) in SC.DESIGNED.items():
        s = _signal(c, 0)
        assign, value = losses.set_assign_host(*s, w_conf=o["w_conf"], scale=o["scale"], period=o["period"])
        assert assign.tolist() == want, name
        assert np.array_equal(enumerate_definition(*s, **o)[1], assign), name
        assert TLK.set(*SC.args(SC.f64(c)), **o)[1].tolist() == [want], name
    for name in ("confident-first", "confident-second"):
        c, o, _ = SC.DESIGNED[name]
        assert abs(TLK.set(*SC.args(SC.f64(c)), **o)[0][0].item() - 0.0011) < 1e-8          # float32 inputs
    for name, (c, o) in SC.TIES.items():
        s = _signal(c, 0)
        assign, value = losses.set_assign_host(*s, w_conf=o["w_conf"], scale=o["scale"], period=o["period"])
        want_value, _ = enumerate_definition(*s, **o)
        assert value == want_value and (assign >= 0).sum() == 1, name                     # the returned assignment attains it


def test_above_the_enumeration_scipy_agrees_with_the_brute_force_below():
    """16 x 8 is solved by scipy; cut to 6 x 6 the same signals are enumerated: both routes of set_assign_host on a size both take."""
    c = SC.table_case(5, 16, 8, "plain")
    for b in range(5):
        s = [v[:6] for v in _signal(c, b)[:5]]
        a1, v1, g1 = losses.set_assign_host(*s, 6, w_conf=0.1, with_gap=True)
        old = metrics.BRUTE_MIN
        try:
            metrics.BRUTE_MIN = 0
            a2, v2, g2 = losses.set_assign_host(*s, 6, w_conf=0.1, with_gap=True)
        finally:
            metrics.BRUTE_MIN = old
        assert np.array_equal(a1, a2) and v1 == v2 and abs(g1 - g2) <= 1e-9 * g1


# ---- 3. the tensor formulation against an explicit loop ----------------------------------------------------------------------------
def loop_loss(c, assign, lambda_reg, w_conf, scale, period):
    """The definition as a per-signal loop over torch scalars at a GIVEN assignment (the minimiser): (total, match, conf, reg)."""
    B, Lmax = c["tau"].shape
    Lt = c["tau_true"].shape[1]
    pt, pf = (0.0, 0.0) if period is None else period
    wrap = lambda d, P: d - P * torch.floor(d / P + 0.5) if P > 0 else d
    match = conf = reg = 0.0
    for b in range(B):
        n = min(max(int(c["L_true"][b]), 0), Lt)
        vals = torch.cat([c["tau"][b], c["f"][b], c["conf"][b], c["tau_true"][b, :n], c["f_true"][b, :n]])
        if not torch.isfinite(vals).all():
            continue
        m = 0.0
        for i in range(Lmax):
            j = int(assign[b, i])
            t = 1.0 if j >= 0 else 0.0
            conf = conf + (c["conf"][b, i] - t) ** 2 / Lmax
            if j >= 0:
                m = m + (scale[0] * wrap(c["tau"][b, i] - c["tau_true"][b, j], pt)) ** 2 + \
                    (scale[1] * wrap(c["f"][b, i] - c["f_true"][b, j], pf)) ** 2
        match = match + m / max(n, 1)
        reg = reg + torch.sqrt((c["phi"][b].real ** 2 + c["phi"][b].imag ** 2).sum())
    match, conf, reg = match / B, conf / B, lambda_reg * reg / B
    return match + w_conf * conf + reg, match, conf, reg


def _cases_for_the_formulation():
    for Lmax, Lt in SMALL + [(16, 8)]:
        for v in SC.VARIANTS:
            yield f"{Lmax}x{Lt}-{v}", SC.table_case(5, Lmax, Lt, v), SC.options(v)
    c, o, _, _ = SC.with_bad_values()
    yield "bad-values", c, o
    c, o, _, _ = SC.out_of_range()
    yield "out-of-range", c, o


def test_the_tensor_formulation_equals_the_loop_and_autograd_through_it():
    worst = 0.0
    for name, c32, o in _cases_for_the_formulation():
        c = SC.f64(c32)
        out, assign, norms, status, rows = TLK.set(*SC.args(c), **o)
        leaves = dict(c, **{k: c[k].clone().requires_grad_(True) for k in ("tau", "f", "conf", "phi")})
        want = loop_loss(leaves, assign, **o)
        for got, w in zip(out, want):
            w = float(w.detach()) if isinstance(w, torch.Tensor) else float(w)
            assert abs(got.item() - w) <= F64 * max(abs(w), 1e-300), name
        assert torch.allclose(rows[:, 0], rows[:, 1] + o["w_conf"] * rows[:, 2], rtol=1e-14, atol=0)
        up = torch.tensor(UP, dtype=torch.float64)
        auto = torch.autograd.grad(sum(u * w for u, w in zip(up, want)), [leaves[k] for k in ("tau", "f", "conf", "phi")],
                                   allow_unused=True)
        hand = TLK.set_bwd(up, *SC.args(c), assign, norms, **o)
        for g, a, k in zip(hand, auto, ("tau", "f", "conf", "phi")):
            a = torch.zeros_like(g) if a is None else torch.nan_to_num(a)     # (a dead signal is skipped by the loop)
            big = max(a.abs().max().item(), 1e-300)
            worst = max(worst, (g - a).abs().max().item() / big)
            assert (g - a).abs().max().item() <= F64 * big, (name, k)
            assert torch.isfinite(g).all(), (name, k)
        unmatched = assign < 0
        assert not hand[0][unmatched].any() and not hand[1][unmatched].any(), name
    print(f"hand-written backward against autograd through the loop: worst {worst:.2e} of the largest entry")


def test_status_words_and_dead_signals():
    c, o, dead, status = SC.with_bad_values()
    out, assign, norms, st, rows = TLK.set(*SC.args(SC.f64(c)), **o)
    assert st.tolist() == status and st.dtype == torch.int32
    assert (assign[dead] == -1).all() and not rows[dead, :4].any() and rows[dead, 5].tolist() == [1.0] * 3
    assert (assign[4] >= 0).sum() == 1 and rows[4, 5] == 0                       # the NaN truth past n does not count
    g = TLK.set_bwd(torch.tensor(UP, dtype=torch.float64), *SC.args(SC.f64(c)), assign, norms, **o)
    assert all(not x[dead].any() and torch.isfinite(x).all() for x in g)
    assert torch.isfinite(out).all()
    c, o, held, status = SC.out_of_range()
    a, b = TLK.set(*SC.args(SC.f64(c)), **o), TLK.set(*SC.args(SC.f64(held)), **o)
    assert a[3].tolist() == status and b[3].tolist() == [0, 0]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4][:, :4], b[4][:, :4])


def test_central_differences_of_the_loop():
    """On cases with margin a step of 1e-6 changes no assignment: the loss is smooth there and its gradient is the gradient at the
    minimiser."""
    h = 1e-6
    for Lmax, Lt, v in ((3, 3, "plain"), (5, 3, "w5-scaled"), (3, 5, "periodic"), (5, 3, "periodic-w5-scaled-all")):
        c, o = SC.f64(SC.table_case(5, Lmax, Lt, v)), SC.options(v)
        out, assign, norms, _, _ = TLK.set(*SC.args(c), **o)
        g = TLK.set_bwd(torch.tensor([1.0, 0, 0, 0], dtype=torch.float64), *SC.args(c), assign, norms, **o)
        for k, gk in zip(("tau", "f", "conf"), g):
            for b, i in itertools.product(range(5), range(Lmax)):
                vals = []
                for s in (h, -h):
                    moved = dict(c, **{k: c[k].clone()})
                    moved[k][b, i] += s
                    o2, a2 = TLK.set(*SC.args(moved), **o)[:2]
                    assert torch.equal(a2, assign)
                    vals.append(o2[0].item())
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - gk[b, i].item()) <= 1e-7 * max(1.0, abs(fd)) + 1e-9, (v, k, b, i, fd, gk[b, i].item())


def _call(m, c, leaves=None):
    s = leaves or c
    return m({"tau_est": s["tau"], "f_est": s["f"], "confidences": s["conf"], "phi_final": s["phi"]},
             {"tau_true": c["tau_true"], "f_true": c["f_true"], "L_true": c["L_true"]})


@pytest.mark.parametrize("up", [(1.0, 0, 0, 0), (0, 1.0, 0, 0), (0, 0, 1.0, 0), (0, 0, 0, 1.0), UP], ids=["total", "match", "conf", "reg", "weighted"])
def test_the_module_honours_every_output(up):
    v = "periodic-w5-scaled-all"
    c, o = SC.f64(SC.table_case(5, 5, 3, v)), SC.options(v)
    m = losses.SetANMLoss(**o)
    m.route = "tensor"
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("tau", "f", "conf", "phi")}
    total, d = _call(m, c, leaves)
    names = ("total_loss", "match_loss", "conf_loss", "reg_loss")
    assert tuple(d) == names and total is d["total_loss"] and all(d[k].dim() == 0 for k in names)
    assert m.last_assign.shape == (5, 5) and m.last_assign.dtype == torch.int32 and m.last_status.tolist() == [0, 0]
    sum(u * d[k] for u, k in zip(up, names)).backward()
    want = TLK.set_bwd(torch.tensor(up, dtype=torch.float64), *SC.args(c), m.last_assign, TLK.set(*SC.args(c), **o)[2], **o)
    for k, w in zip(("tau", "f", "conf", "phi"), want):
        assert torch.equal(leaves[k].grad, w), k
    with torch.no_grad():
        assert not _call(m, c, leaves)[0].requires_grad


def test_the_module_s_surface():
    assert str(inspect.signature(losses.SetANMLoss.__init__)) == "(self, lambda_reg=0.0001, w_conf=0.1, scale=(1.0, 1.0), period=None)"
    m = losses.SetANMLoss()
    assert m.route == "hip" and m.check_status and m.last_assign is None and m.last_status is None
    m.route = "tensor"
    c, o, _, _ = SC.with_bad_values()
    with pytest.raises(ValueError, match="3 sample.*non-finite"):
        _call(m, c)
    c, o, held, _ = SC.out_of_range()
    with pytest.raises(ValueError, match=r"2 sample.*outside \[0, 4\]"):
        _call(m, c)
    m.check_status = False
    total, _ = _call(m, c)
    assert torch.equal(total, _call(m, held)[0]) and m.last_status.tolist() == [0, 0]
    with pytest.raises(ValueError, match="requires grad"):
        _call(m, dict(c, tau_true=c["tau_true"].clone().requires_grad_(True)))
    m.route = "eager"
    with pytest.raises(ValueError, match="route"):
        _call(m, c)
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(1.0,)), dict(period=(-1.0, 0.0)), dict(period=1.0), dict(w_conf=-0.1),
                dict(w_conf=float("nan")), dict(lambda_reg=-1.0), dict(lambda_reg=float("inf"))):
        with pytest.raises(ValueError):
            losses.SetANMLoss(**bad)
    import importlib.util
    path = os.path.join(os.path.dirname(losses.__file__), "dropin", "optional", "loss.py")
    spec = importlib.util.spec_from_file_location("_dropin_set_loss_probe", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SetANMLoss is losses.SetANMLoss and mod.BasicANMLoss is losses.BasicANMLoss


# ---- 4. the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_wrappers_and_the_build_list():
    c = ctypes
    assert _lib.SYMBOLS["admmnet_loss_set_partials"] == (c.c_int64, [c.c_int64])
    res, a = _lib.SYMBOLS["admmnet_loss_set_f32"]
    assert res is c.c_int32 and a == [c.c_int32] * 3 + [c.c_int64] + [c.c_void_p] * 7 + [c.POINTER(c.c_double)] + [c.c_void_p] * 6
    res, a = _lib.SYMBOLS["admmnet_loss_set_bwd_f32"]
    assert res is c.c_int32 and a == [c.c_int32] * 3 + [c.c_int64] + [c.c_void_p] * 10 + [c.POINTER(c.c_double)] + [c.c_void_p] * 5
    hdr = open(os.path.join(ROOT, "include", "admmnet.h")).read()
    for name in ("admmnet_loss_set_partials", "admmnet_loss_set_f32", "admmnet_loss_set_bwd_f32"):
        assert hdr.count(name + "(") >= 1 and hasattr(_lib.load(), name)
    from admm_net_amd import build, set_ops
    assert "loss_set.hip" in build.SOURCES and "set_core.h" in build.HEADERS
    assert ops.loss_set is set_ops.loss_set and ops.loss_set_bwd is set_ops.loss_set_bwd
    assert ops.loss_set.__module__ == "admm_net_amd.set_ops"                  # ops' own table of functions is as it was
    assert losses.HipLossKernels.set is ops.loss_set and losses.HipLossKernels.set_bwd is ops.loss_set_bwd
    for hip, tensor in ((ops.loss_set, TLK.set), (ops.loss_set_bwd, TLK.set_bwd)):          # one call serves both routes
        a, b = (inspect.signature(fn).parameters for fn in (hip, tensor))
        assert list(a) == list(b) and [p.default for p in a.values()] == [p.default for p in b.values()]
    with pytest.raises(_lib.AdmmNetError, match="HIP device tensor"):
        ops.loss_set(*SC.args(SC.table_case(1, 3, 3, "plain")))


def test_the_c_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.admmnet_loss_set_partials(0) == -1 and lib.admmnet_loss_set_partials(-3) == -1
    assert lib.admmnet_loss_set_partials(1) == 6 and lib.admmnet_loss_set_partials(257) == 6 * 257
    assert lib.admmnet_loss_partials(2, 5) == -1                                # the enum of the other losses has no new value
    p = ctypes.c_void_p(64)                                                     # never read: every case is refused before a launch
    good = (ctypes.c_double * 6)(1.0, 1.0, 0.0, 0.0, 0.1, 1e-4)
    opt = lambda **kw: (ctypes.c_double * 6)(*[kw.get(k, d) for k, d in zip(("sx", "sy", "pt", "pf", "wc", "lam"), good)])

    def fwd(Lmax=3, Lt=3, D=4, B=4, tau=p, opts=good, part=p):
        return lib.admmnet_loss_set_f32(Lmax, Lt, D, B, tau, p, p, p, p, p, p, opts, p, p, p, p, part, None)

    def bwd(Lmax=3, Lt=3, D=4, B=4, assign=p, opts=good, g_phi=p):
        return lib.admmnet_loss_set_bwd_f32(Lmax, Lt, D, B, p, p, p, p, p, p, p, p, assign, p, opts, p, p, p, g_phi, None)

    sizes = (dict(Lmax=0), dict(Lmax=65), dict(Lt=0), dict(Lt=65), dict(D=0), dict(B=0), dict(B=-1), dict(opts=None))
    options = [dict(opts=opt(**kw)) for kw in (dict(sx=0.0), dict(sy=-1.0), dict(sx=float("inf")), dict(sy=float("nan")),
                                               dict(pt=-1.0), dict(pf=float("inf")), dict(wc=-0.1), dict(wc=float("nan")),
                                               dict(lam=-1e-4), dict(lam=float("inf")))]
    for kw in sizes + tuple(options) + (dict(tau=None), dict(part=None)):
        assert fwd(**kw) == -1, kw
        assert b"loss_set" in lib.admmnet_last_error()
    for kw in sizes + tuple(options) + (dict(assign=None), dict(g_phi=None)):
        assert bwd(**kw) == -1, kw
        assert b"loss_set_bwd" in lib.admmnet_last_error()


def test_the_head_s_estimate_and_the_harness_surface(monkeypatch):
    from admm_net_amd import harness, modules
    tau, f = torch.tensor([[3.0, 1.0, 2.0], [4.0, 5.0, 6.0]]), torch.tensor([[0.3, 0.1, 0.2], [0.4, 0.5, 0.6]])
    conf = torch.tensor([[0.5, 0.7, 0.5], [0.1, 0.2, 0.9]])
    t, ff, c, n = modules.order_by_confidence(tau, f, conf, 0.5)
    assert t.tolist() == [[1.0, 3.0, 2.0], [6.0, 5.0, 4.0]] and torch.equal(ff, t / 10) and n.tolist() == [3, 1] and n.dtype == torch.int32
    assert torch.equal(c, torch.tensor([[0.7, 0.5, 0.5], [0.9, 0.2, 0.1]]))
    assert modules.HeadEstimate._fields == ("tau", "f", "conf", "n_est", "phi")
    for cls, name in ((modules.ADMMNet, "estimate_head"), (modules.ADMMNet, "evaluate_head")):
        assert callable(getattr(cls, name)) and not hasattr(modules.PhiEstADMMNet, name)
    assert str(inspect.signature(modules.ADMMNet.estimate_head)) == "(self, y, b, sigma, threshold=0.5)"
    p = inspect.signature(harness.evaluate_snr).parameters
    assert p["head"].default is False
    p = inspect.signature(harness.time_train_step).parameters
    assert [p[k].default for k in ("loss", "targets", "min_sep", "checkpoint")] == [None, None, 0.0, None]
    for kw in (dict(loss="set"), dict(head=True, loss="sets"), dict(head=True, targets=(1, 3))):
        with pytest.raises(ValueError):
            harness.time_train_step(device="cpu", **kw)
    for argv in (["train-step", "--head", "--loss", "ordered"], ["train-step", "--targets-min", "1"], ["loss-step", "--set", "--spectral"]):
        with pytest.raises(SystemExit):
            harness.main(argv)
    seen = []
    monkeypatch.setattr(harness, "evaluate_snr", lambda *a, **kw: seen.append(kw) or iter(()))
    monkeypatch.setattr(harness, "time_train_step", lambda *a, **kw: seen.append(kw) or {})
    harness.main(["evaluate", "--head", "--targets-min", "1"])
    harness.main(["evaluate"])
    harness.main(["train-step", "--head", "--loss", "set", "--targets-min", "1", "--min-sep", "1.5"])
    harness.main(["train-step", "--head"])
    assert [kw["head"] for kw in seen] == [True, False, True, True]
    assert seen[2]["loss"] == "set" and seen[2]["targets"] == (1, 3) and seen[2]["min_sep"] == 1.5 and "loss" not in seen[3]


# ---- 5. the scalar core under the sanitizers ---------------------------------------------------------------------------------------
def _table_for_the_host_model():
    for Lmax, Lt in SC.SHAPES:
        for v in SC.VARIANTS:
            yield SC.table_case(5, Lmax, Lt, v), SC.options(v), SC.reference(5, Lmax, Lt, v)
    for c, o, _ in SC.DESIGNED.values():
        yield c, o, TLK.set(*SC.args(SC.f64(c)), **o)
    for c, o in (SC.with_bad_values()[:2], SC.out_of_range()[:2]):
        yield c, o, TLK.set(*SC.args(SC.f64(c)), **o)


def test_set_core_under_sanitizers(tmp_path):
    """tests/host_model/set_model.cpp (its own main, csrc/set_core.h and csrc/score_core.h only, the lane loop emulated): its own
    checks against the brute-forced definition, then the whole table -- ``assign`` equal to the float64 mirror's exactly, the
    values within 64 x 2^-53 of the sum of the magnitudes of their terms (all terms are non-negative: the value itself)."""
    exe = str(tmp_path / "set_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "set_model.cpp"), "-o", exe])

    def run(*argv):
        p = subprocess.run([exe, *argv], capture_output=True, text=True)
        assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
        return p.stdout

    assert run().strip() == "ok"
    lines, want = [], []
    for c, o, ref in _table_for_the_host_model():
        pt, pf = (0.0, 0.0) if o["period"] is None else o["period"]
        for b in range(c["tau"].shape[0]):
            vals = np.concatenate([c[k][b].double().numpy() for k in SC.KEYS[:5]])
            lines.append(" ".join([str(c["tau"].shape[1]), str(c["tau_true"].shape[1]), str(int(c["L_true"][b])),
                                   *(repr(float(x)) for x in (*o["scale"], pt, pf, o["w_conf"])), *(repr(float(x)) for x in vals)]))
            want.append((ref[1][b].tolist(), ref[4][b].tolist()))
    path = tmp_path / "table.txt"
    path.write_text("\n".join(lines) + "\n")
    got = run(str(path)).strip().split("\n")
    assert len(got) == len(want) > 280
    worst, eps = 0.0, 64 * 2.0 ** -53
    for line, (assign, row) in zip(got, want):
        t = line.split()
        assert int(t[0]) == int(row[5]) and [int(x) for x in t[1:-3]] == assign, (line, assign)
        for g, w in zip(t[-3:], row[:3]):
            assert abs(float(g) - w) <= eps * w, (line, row)
            worst = max(worst, abs(float(g) - w) / (eps * w) if w > 0 else 0.0)
    print(f"host model against the float64 mirror on {len(want)} signals: worst value error / bound {worst:.3f}")


# ---- 6. one-mistake stand-ins ------------------------------------------------------------------------------------------------------
MISTAKES = {   # the mistake: the case that rejects it
    "the sign of the per-slot term": "confident-second",
    "a normaliser of k": "n-above-slots",
    "matching on d2 alone": "term-decides",
    "truths past n used": "truth-past-n",
    "no wrap": "across-the-wrap",
    "unmatched slots without a conf target": "shuffled",
    "t on the target's index": "shuffled",
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_stand_in_with_one_mistake_is_rejected(mistake):
    """Each stand-in differs from the definition in one thing; the named case tells them apart by the assignment or, at 1e-6
    relative, by the value -- and the same comparison accepts the definition itself."""
    c, o, want = SC.DESIGNED[MISTAKES[mistake]]
    s = _signal(c, 0)
    ref = TLK.set(*SC.args(SC.f64(c)), **o)
    same = lambda value, assign: assign.tolist() == ref[1][0].tolist() and abs(value - ref[4][0, 0].item()) <= 1e-6 * ref[4][0, 0].item()
    assert same(*enumerate_definition(*s, **o))
    assert not same(*enumerate_definition(*s, mistake=mistake, **o))


# ---- 7. why the loss exists ----------------------------------------------------------------------------------------------------------
def test_the_ordered_loss_prefers_the_mean_and_the_set_loss_the_exact_answer():
    """Scenes of three targets drawn as the generator draws them (truths in draw order).  ``BasicANMLoss`` scores the EXACT targets,
    listed by ascending tau, worse than one constant in every slot; ``SetANMLoss`` gives the exact answer a match term of 0 and
    only its confidence term."""
    g = torch.Generator().manual_seed(0)
    N, L = 20000, 3
    tau_true = (0.1 + 0.8 * torch.rand(N, L, generator=g, dtype=torch.float64))
    f_true = 0.8 * torch.rand(N, L, generator=g, dtype=torch.float64) - 0.4
    order = tau_true.argsort(dim=1)
    exact = dict(tau=tau_true.gather(1, order), f=f_true.gather(1, order))
    const = dict(tau=tau_true.mean().expand(N, L), f=f_true.mean().expand(N, L))
    conf = torch.ones(N, L, dtype=torch.float64)
    phi = torch.zeros(N, 1, dtype=torch.complex128)
    truth = dict(tau_true=tau_true, f_true=f_true, L_true=torch.full((N,), L))
    basic = losses.BasicANMLoss(lambda_reg=0.0)
    basic.route = "tensor"
    ordered = {k: _call(basic, dict(truth, conf=conf, phi=phi, **p))[0].item() for k, p in (("exact", exact), ("const", const))}
    print("BasicANMLoss: the exact targets by ascending tau", ordered["exact"], "one constant in every slot", ordered["const"])
    assert ordered["const"] < 0.8 * ordered["exact"]
    m = losses.SetANMLoss(lambda_reg=0.0)
    m.route = "tensor"
    few = slice(0, 500)
    cut = lambda d: {k: v[few] for k, v in d.items()}
    half = torch.full((500, L), 0.5, dtype=torch.float64)
    total, d = _call(m, dict(cut(truth), conf=half, phi=phi[few], **cut(exact)))
    assert d["match_loss"].item() == 0.0 and abs(total.item() - 0.1 * 0.25) < 1e-15
    assert torch.equal(m.last_assign.long(), order[few])                         # slot i holds the target listed i-th
    worse, _ = _call(m, dict(cut(truth), conf=half, phi=phi[few], **cut(const)))
    assert worse.item() > total.item() + 0.01
