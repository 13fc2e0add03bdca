"""GPU: the assignment loss of the head on the kernels of csrc/loss_set.hip (``ops.loss_set`` / ``ops.loss_set_bwd``,
``losses.SetANMLoss`` on ``route = "hip"``) against the float64 tensor formulation ``losses.TensorLossKernels.set`` on the float32
inputs the kernels read (tests/test_set_loss.py holds that formulation to the definition), and ``ADMMNet.estimate_head``.

Bounds (the rule of tests/test_gpu_losses.py, whose ``Worst`` keeps the figures):
  * ``assign`` equals the float64 mirror's EXACTLY -- every case keeps a relative margin of 1e-9 between its best and its
    second-best assignment (tests/set_loss_cases.py; asserted on the host for every case run here, none left out);
  * sums over the batch (total, match, conf, reg) and the per-signal rows: within 2e-5 sum|terms|; every term of match, conf and reg
    is non-negative, so that sum is the float64 value itself;
  * elementwise outputs (the norms, every gradient): no further from float64 than 3 x the distance of the float32 tensor
    formulation evaluated on the GPU, plus 1e-6 of the largest entry;
  * gradients of tau and f on unmatched slots, and every gradient of a signal with a non-finite value, are exactly 0; every forward
    and backward run twice gives equal bits; a signal's bits depend on neither B, nor its place, nor its neighbours.
Each test prints the worst figures it saw; those measured on an MI355X are recorded in DESIGN.md section 4.
"""
import ctypes

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, harness, losses, metrics, ops, synth
from admm_net_amd.losses import TensorLossKernels as TLK

import presentations as P
import set_loss_cases as SC
from test_gpu_training_small import Worst, _f64, _same_twice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UP = (1.7, 0.3, -0.6, 0.9)                        # gradients of (total, match, conf, reg)
GRADS = ("g_tau", "g_f", "g_conf", "g_phi")


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _check(c, o, ref, worst):
    """c: host inputs, ref: the float64 mirror's returns.  Forward and backward of the kernels; returns what they gave."""
    d = _dev(c)
    a, a64 = SC.args(d), SC.args(SC.f64(c))
    out, assign, norms, status, rows = _same_twice(lambda: ops.loss_set(*a, **o))
    w_out, w_assign, w_norms, w_status, w_rows = ref
    assert out.dtype == torch.float32 and out.shape == (4,) and assign.dtype == torch.int32 and rows.dtype == torch.float64
    assert torch.equal(assign.cpu(), w_assign), "the assignment differs from the float64 mirror's"
    assert status.tolist() == w_status.tolist()
    worst.red(out, w_out, w_out, "total, match, conf, reg")
    worst.red(rows[:, :4], w_rows[:, :4], w_rows[:, :4], "per-signal rows")
    assert torch.equal(rows[:, 4:].cpu(), w_rows[:, 4:])
    p_norms = torch.sqrt((d["phi"].real ** 2 + d["phi"].imag ** 2).sum(dim=1))            # the float32 formulation on the GPU
    worst.elem(norms, p_norms, w_norms, "norms")
    up = torch.tensor(UP, device=DEV)
    got = _same_twice(lambda: ops.loss_set_bwd(up, *a, assign, norms, **o))
    want = TLK.set_bwd(_f64(up), *a64, w_assign, w_norms, **o)
    parent = TLK.set_bwd(up, *a, assign, p_norms, **o)
    for g, p, w, name in zip(got, parent, want, GRADS):
        assert g.dtype == (torch.complex64 if name == "g_phi" else torch.float32)
        worst.elem(g, p, w, name)
    assert not got[0][assign < 0].any() and not got[1][assign < 0].any(), "g_tau, g_f must be exactly 0 on unmatched slots"
    dead = rows[:, 5] > 0
    assert all(not g[dead].any() for g in got), "a signal with a non-finite value gets zero gradients"
    assert not got[3][norms == 0].any()
    return out, assign, norms, rows, got


@pytest.mark.parametrize("Lmax,Lt", SC.SHAPES, ids=[f"{a}x{b}" for a, b in SC.SHAPES])
@pytest.mark.parametrize("B", SC.BATCHES)
def test_kernels_match_their_definition(B, Lmax, Lt):
    worst = Worst(f"set B={B} {Lmax}x{Lt}")
    for v in SC.variants_of(B):
        _check(SC.table_case(B, Lmax, Lt, v), SC.options(v), SC.reference(B, Lmax, Lt, v), worst)
    worst.done()


def test_designed_cases_ties_and_bad_values():
    worst = Worst("set designed")
    for name, (c, o, want) in SC.DESIGNED.items():
        out, assign, *_ = _check(c, o, TLK.set(*SC.args(SC.f64(c)), **o), worst)
        assert assign.tolist() == [want], name
    for name, (c, o) in SC.TIES.items():                                  # two optimal assignments: the values only
        out, assign, norms, status, rows = ops.loss_set(*SC.args(_dev(c)), **o)
        w = TLK.set(*SC.args(SC.f64(c)), **o)
        worst.red(out, w[0], w[0], name)
        assert (assign >= 0).sum().item() == 1 and status.tolist() == [0, 0]
        at = TLK.set_bwd(torch.ones(4, dtype=torch.float64), *SC.args(SC.f64(c)), assign.cpu(), w[2], **o)   # attains the optimum
        assert all(torch.isfinite(g).all() for g in at)
    c, o, dead, status = SC.with_bad_values()
    out, assign, norms, rows, got = _check(c, o, TLK.set(*SC.args(SC.f64(c)), **o), worst)
    assert rows[:, 5].nonzero().reshape(-1).tolist() == dead and (assign[dead] == -1).all() and torch.isfinite(out).all()
    assert all(torch.isfinite(g).all() for g in got)
    c, o, held, status = SC.out_of_range()
    out, assign, norms, rows, got = _check(c, o, TLK.set(*SC.args(SC.f64(c)), **o), worst)
    h = ops.loss_set(*SC.args(_dev(held)), **o)
    assert torch.equal(out, h[0]) and torch.equal(assign, h[1]) and h[3].tolist() == [0, 0]
    worst.done()


def test_a_signal_s_bits_depend_on_neither_batch_nor_place_nor_neighbours():
    v = "w5-scaled"
    c, o = _dev(SC.table_case(257, 5, 3, v)), SC.options(v)
    pick = lambda r, b: (r[1][b], r[2][b], r[4][b])                        # assign, norms, the per-signal row
    full = ops.loss_set(*SC.args(c), **o)
    for count in (1, 7):
        part = ops.loss_set(*SC.args({k: t[-count:] for k, t in c.items()}), **o)
        assert all(torch.equal(x, y) for x, y in zip(pick(part, -1), pick(full, -1))), count
    alone = ops.loss_set(*SC.args({k: t[100:101] for k, t in c.items()}), **o)
    assert all(torch.equal(x, y) for x, y in zip(pick(alone, 0), pick(full, 100)))
    # beside a NaN neighbour: signals 1 and 3 of five are dead, the others keep their bits, forward and backward
    five = {k: t[100:105].clone() for k, t in c.items()}
    clean = ops.loss_set(*SC.args(five), **o)
    up = torch.tensor(UP, device=DEV)
    g_clean = ops.loss_set_bwd(up, *SC.args(five), clean[1], clean[2], **o)
    five["tau"][1, 0] = float("nan")
    five["f_true"][3, 0] = float("nan")
    five["L_true"][3] = 2
    beside = ops.loss_set(*SC.args(five), **o)
    g_beside = ops.loss_set_bwd(up, *SC.args(five), beside[1], beside[2], **o)
    assert beside[3].tolist() == [0, 2]
    for b in (0, 2, 4):
        assert all(torch.equal(x, y) for x, y in zip(pick(beside, b), pick(clean, b)))
        assert all(torch.equal(x[b], y[b]) for x, y in zip(g_beside, g_clean))
    assert all(not g[[1, 3]].any() for g in g_beside)


@pytest.mark.parametrize("form", [f for f in P.FORMS if f not in P.ABSENT])
def test_every_input_form_gives_the_plain_tensor_bits(form):
    """The forms of tests/presentations.py (the table of tests/test_gpu_presentations.py holds the functions defined in ops.py to
    them): each tensor input of ``ops.loss_set`` and ``ops.loss_set_bwd`` in turn, the others plain."""
    v = "periodic-w5-scaled-all"
    c, o = _dev(SC.table_case(4, 5, 3, v)), SC.options(v)
    if form == "expanded":
        c = {k: P.constant_along0(t) for k, t in c.items()}
    fwd = ops.loss_set(*SC.args(c), **o)
    extra = {"g_out": torch.tensor(UP, device=DEV), "assign": fwd[1], "norms": fwd[2]}
    if form == "expanded":
        assert torch.equal(fwd[1], P.constant_along0(fwd[1])) and torch.equal(fwd[2], P.constant_along0(fwd[2]))

    def run(d, e):
        return (*ops.loss_set(*SC.args(d), **o), *ops.loss_set_bwd(e["g_out"], *SC.args(d), e["assign"], e["norms"], **o))

    plain, seen = run(c, extra), 0
    for k in list(c) + list(extra):
        t = P.present(form, extra[k] if k in extra else c[k])
        if t is None:
            continue
        got = run(c, dict(extra, **{k: t})) if k in extra else run(dict(c, **{k: t}), extra)
        assert all(P.same_bits(x, y) for x, y in zip(got, plain)), (form, k)
        seen += 1
    assert seen >= (1 if form in ("lazy_conj", "conj_sliced") else 3), form


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _lib.load()
    c = _dev(SC.table_case(4, 3, 3, "plain"))
    t = [c[k].contiguous() for k in SC.KEYS]
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [1.0, 1.0, 0.0, 0.0, 0.1, 1e-4]
    outs = dict(out=torch.full((4,), 7.0, device=DEV), assign=torch.full((4, 3), 7, dtype=torch.int32, device=DEV),
                norms=torch.full((4,), 7.0, device=DEV), status=torch.full((2,), 7, dtype=torch.int32, device=DEV),
                part=torch.full((24,), 7.0, dtype=torch.float64, device=DEV))
    grads = dict(g_tau=torch.full((4, 3), 7.0, device=DEV), g_f=torch.full((4, 3), 7.0, device=DEV),
                 g_conf=torch.full((4, 3), 7.0, device=DEV), g_phi=torch.full((4, 7), 7.0, dtype=torch.complex64, device=DEV))
    up = torch.tensor(UP, device=DEV)

    def fwd(Lmax=3, Lt=3, D=7, B=4, opts=good, null=None):
        o = None if opts is None else (ctypes.c_double * 6)(*opts)
        p = [None if null == i else ptr(x) for i, x in enumerate(t)]
        return lib.admmnet_loss_set_f32(Lmax, Lt, D, B, *p, o, *(ptr(x) for x in outs.values()), stream)

    def bwd(Lmax=3, Lt=3, D=7, B=4, opts=good, null=None):
        o = None if opts is None else (ctypes.c_double * 6)(*opts)
        p = [None if null == i else ptr(x) for i, x in enumerate(t)]
        return lib.admmnet_loss_set_bwd_f32(Lmax, Lt, D, B, ptr(up), *p, ptr(outs["assign"]), ptr(outs["norms"]), o,
                                            *(ptr(x) for x in grads.values()), stream)

    bad = lambda i, v: good[:i] + [v] + good[i + 1:]
    cases = [dict(Lmax=0), dict(Lmax=65), dict(Lt=0), dict(Lt=65), dict(D=0), dict(B=0), dict(opts=None), dict(null=0), dict(null=5),
             dict(null=6)] + [dict(opts=bad(i, v)) for i, v in ((0, 0.0), (0, float("inf")), (1, -1.0), (1, float("nan")), (2, -1.0),
                                                               (3, float("inf")), (4, -0.1), (4, float("nan")), (5, -1.0),
                                                               (5, float("inf")))]
    for kw in cases:
        assert fwd(**kw) == -1 and b"loss_set" in lib.admmnet_last_error(), kw
        assert bwd(**kw) == -1 and b"loss_set_bwd" in lib.admmnet_last_error(), kw
    torch.cuda.synchronize()
    assert all((x == 7).all() for x in list(outs.values()) + list(grads.values())), "a refused call wrote to an output"
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert all(not (x == 7).all() for x in list(outs.values())[:4] + list(grads.values()))


def _call(m, c, leaves=None):
    s = leaves or c
    return m({"tau_est": s["tau"], "f_est": s["f"], "confidences": s["conf"], "phi_final": s["phi"]},
             {"tau_true": c["tau_true"], "f_true": c["f_true"], "L_true": c["L_true"]})


def test_no_synchronising_call_across_forward_and_backward():
    v = "periodic"
    c, o = _dev(SC.table_case(5, 5, 3, v)), SC.options(v)
    m = losses.SetANMLoss(**o)
    m.check_status = False
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("tau", "f", "conf", "phi")}
    _call(m, c, leaves)[0].backward()                                      # (the library is loaded, the first calls made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, d = _call(m, c, leaves)
        (total + d["conf_loss"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert m.last_status.tolist() == [0, 0] and torch.isfinite(leaves["tau"].grad).all()
    m.check_status = True
    bad, _, _, _ = SC.with_bad_values()
    with pytest.raises(ValueError, match="3 sample.*non-finite"):
        _call(m, _dev(bad))
    bad, _, _, _ = SC.out_of_range()
    with pytest.raises(ValueError, match="2 sample.*outside"):
        _call(m, _dev(bad))


@pytest.mark.parametrize("up", [(1.0, 0, 0, 0), (0, 1.0, 0, 0), (0, 0, 1.0, 0), (0, 0, 0, 1.0), UP], ids=["total", "match", "conf", "reg", "weighted"])
def test_the_module_on_both_routes_honours_every_output(up):
    worst = Worst(f"SetANMLoss up={up}")
    v = "periodic-w5-scaled-all"
    c, o = _dev(SC.table_case(5, 5, 3, v)), SC.options(v)
    keys, names = ("tau", "f", "conf", "phi"), ("total_loss", "match_loss", "conf_loss", "reg_loss")

    def run(route, wide):
        cc = _dev(SC.f64({k: t.cpu() for k, t in c.items()})) if wide else c
        leaves = {k: cc[k].clone().requires_grad_(True) for k in keys}
        m = losses.SetANMLoss(**o)
        m.route = route
        _, d = _call(m, cc, leaves)
        sum(u * d[k] for u, k in zip(up, names)).backward()
        return [d[k].detach() for k in names], [leaves[k].grad for k in keys], m.last_assign

    (hv, hg, ha), (pv, pg, pa), (wv, wg, wa) = run("hip", False), run("tensor", False), run("tensor", True)
    assert torch.equal(ha, wa) and torch.equal(pa, wa)
    worst.red(torch.stack(hv), torch.stack(wv), torch.stack(wv), "values")
    for g, p, w, k in zip(hg, pg, wg, keys):
        worst.elem(g, p, w, "g_" + k)
    worst.done()


# ------------------------------------------------------------------------------------------------ end to end
def _net_and_scenes():
    torch.manual_seed(3)
    m = A.ADMMNet(M=4, N=4, num_layers=3).to(DEV)
    m.train_route = "full"
    m.eval()                                                   # the head's attention dropout off: one forward, two backwards
    return m, synth.make_scenes_device(5, 4, 4, targets=(1, 3), seed=5, device=DEV)


def _scene_parts(s):
    y, b, sigma, truth = s
    return (y, b, sigma), {"tau_true": truth["tau"], "f_true": truth["f"], "L_true": truth["L_true"]}


def test_training_step_through_the_set_loss_on_both_routes():
    """4 x 4, K = 3, B = 5 on ``make_scenes_device(targets=(1, 3))``: from ONE forward, a backward through the loss on ``route =
    "hip"`` and one on ``route = "tensor"`` give parameter gradients that agree within 5e-4 of each parameter's largest entry
    (check_grads' tolerance); six AdamW steps with the HIP loss lower the total."""
    m, s = _net_and_scenes()
    inputs, truth = _scene_parts(s)
    assert truth["L_true"].min().item() >= 1 and truth["L_true"].max().item() <= 3
    tau, f, conf, phi = m.forward_autograd(*inputs)
    outputs = {"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}
    params, grads, assigns = list(m.parameters()), {}, {}
    for route in ("hip", "tensor"):
        crit = losses.SetANMLoss()
        crit.route = route
        total, _ = crit(outputs, truth)
        grads[route] = torch.autograd.grad(total, params, retain_graph=True, allow_unused=True)
        assigns[route] = crit.last_assign
    assert torch.equal(assigns["hip"], assigns["tensor"])
    worst = 0.0
    for (name, _), gh, gt in zip(m.named_parameters(), grads["hip"], grads["tensor"]):
        assert (gh is None) == (gt is None), name
        if gh is None:
            continue
        assert torch.isfinite(gh).all(), name
        err, big = (gh - gt).abs().max().item(), gt.abs().max().item()
        if big > 0:
            worst = max(worst, err / (5e-4 * big))
        assert err <= 5e-4 * big, f"{name}: |dgrad| {err:.3e} > 5e-4 x {big:.3e}"
    print(f"ADMMNet: worst gradient difference / tolerance between the routes of SetANMLoss {worst:.2e}")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    crit, history = losses.SetANMLoss(), []
    for _ in range(6):
        opt.zero_grad()
        tau, f, conf, phi = m.forward_autograd(*inputs)
        loss, _ = crit({"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}, truth)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        history.append(loss.item())
    print("losses:", history)
    assert all(np.isfinite(history)) and history[-1] < history[0]


def test_estimate_head_orders_by_confidence_and_counts():
    m, s = _net_and_scenes()
    inputs, truth = _scene_parts(s)
    with torch.no_grad():
        tau, f, conf, phi = m(*inputs)
    for threshold in (0.5, float(conf.median())):
        e = m.estimate_head(*inputs, threshold=threshold)
        order = torch.sort(conf, dim=1, descending=True, stable=True).indices
        assert torch.equal(e.conf, conf.gather(1, order)) and torch.equal(e.tau, tau.gather(1, order))
        assert torch.equal(e.f, f.gather(1, order)) and torch.equal(e.phi, phi)
        assert e.n_est.dtype == torch.int32 and torch.equal(e.n_est, (conf >= threshold).sum(dim=1).to(torch.int32))
        assert all(torch.isfinite(t).all() for t in (e.tau, e.f, e.conf)) and not e.tau.requires_grad
        assert (e.conf[:, :-1] >= e.conf[:, 1:]).all()
    # equal confidences keep slot order
    tied = A.modules.order_by_confidence(torch.tensor([[3.0, 1.0, 2.0]]), torch.zeros(1, 3), torch.tensor([[0.5, 0.7, 0.5]]), 0.5)
    assert tied[0].tolist() == [[1.0, 3.0, 2.0]] and tied[3].tolist() == [3]
    e = m.estimate_head(*inputs)
    r = m.evaluate_head(*inputs, truth["tau_true"], truth["f_true"], truth["L_true"], cutoff=0.1)
    by_hand = metrics.match_targets((e.tau, e.f), truth["tau_true"], truth["f_true"], truth["L_true"], n_est=e.n_est, cutoff=0.1,
                                    period=(1.0, 1.0))
    assert all(torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() for x, y in zip(r, by_hand))
    assert torch.equal(r.match, by_hand.match) and torch.equal(r.totals, by_hand.totals)


def test_evaluate_snr_yields_the_head_line_and_leaves_the_others():
    kw = dict(grid=(4, 4), layers=3, signals=8, snrs=(15.0,), seed=2, targets=3, targets_min=1)
    plain = list(harness.evaluate_snr(**kw))
    with_head = list(harness.evaluate_snr(head=True, **kw))
    heads = [line for line in with_head if line["method"] == "head"]
    others = [line for line in with_head if line["method"] != "head"]
    assert len(heads) == 1 and all(k in heads[0] for k in ("pd", "gospa", "order_under", "order_exact", "order_over"))
    assert abs(heads[0]["order_under"] + heads[0]["order_exact"] + heads[0]["order_over"] - 1.0) < 1e-12
    assert len(others) == len(plain)
    for a, b in zip(others, plain):
        assert list(a) == list(b)
        for k in a:
            assert a[k] == b[k] or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])), k
