"""admm_net_amd.optim on its tensor stand-in (route = "tensor"; no GPU): one step of clipping + AdamW against the float64
oracle of tests/optim_checks.py under the "3 x the float32 parent + 4 u" bound, one-line mistakes that the check must reject,
the interchange of state with torch.optim.AdamW, the properties of ``step`` and ``clip_grad_norm_``, and the drop-in rebinding."""
import math
import os
import subprocess
import sys

import pytest
import torch

import optim_checks as OC
from admm_net_amd import PhiEstADMMNet, harness, optim

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
case = OC.size_case


# ------------------------------------------------------------------------------------------------- one step against the oracle
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("wd", [0.0, 1e-3, 0.1])
@pytest.mark.parametrize("step", [0, 1, 9, 999])
def test_one_step_matches_the_oracle(step, wd, dtype):
    P, G, M, V, steps, hp = case(step, wd)
    got, opt, params = OC.module_step(optim.AdamW, P, G, M, V, steps, hp, dtype=dtype, route="tensor")
    res = OC.check_step(P, G, M, V, steps, hp, got)
    print("OPTIMCHECK", step, wd, dtype, {k: f"{r[0]:.3g} (parent {r[4]:.3g})" for k, r in res.items()})
    assert OC.worst(res) <= 1.0, res
    assert all(int(opt.state[q]["step"]) == step + 1 for q in params)


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e-3])
def test_one_step_with_parameters_of_one_group_at_different_step_counts(max_norm):
    P, G, M, V, steps, hp = case(None, 1e-3, seed=3, steps=[0, 1, 9, 999, 1, 0, 999])
    got, opt, _ = OC.module_step(optim.AdamW, P, G, M, V, steps, hp, max_norm=max_norm, route="tensor")
    res = OC.check_step(P, G, M, V, steps, hp, got, max_norm=max_norm)
    assert OC.worst(res) <= 1.0, res
    if max_norm is not None:
        total, coef = optim.TensorOptimKernels.gradnorm(G, max_norm)       # the stand-in's own norm and coefficient
        ratio, same = OC.check_norm(G, max_norm, total, coef)
        assert ratio <= 1.0 and same and OC.same_bits([total], [opt.last_grad_norm])


def test_the_float32_parent_passes_its_own_check():
    P, G, M, V, steps, hp = case(9, 0.1, seed=1)
    par = OC.parent_step(P, G, M, V, steps, hp, max_norm=1.0)
    assert OC.worst(OC.check_step(P, G, M, V, steps, hp, par, max_norm=1.0, parent=par)) <= 1.0 / 3 + 1e-12


# ------------------------------------------------------------------------------------------------------- one-line mistakes
def mutant_step(P, G, M, V, steps, hp, max_norm, mut):
    """The step in float32 tensor operations with ONE mistake; returns ((P', M', V'), the step counts it keeps)."""
    live = [g for g in G if g is not None]

    def coef_of(grads):
        norm = torch.stack([g.double().square().sum() for g in grads]).sum().sqrt().float()
        c = max_norm / (norm + (0.0 if mut == "coef_without_1e-6" else 1e-6))
        return c if mut == "coef_unclamped" else torch.clamp(c, max=1.0)

    coef = coef_of(live) if max_norm is not None else None
    out, new_steps = ([], [], []), []
    for i, (p, g, m, v, t, h) in enumerate(zip(P, G, M, V, steps, hp)):
        p, m, v = p.clone(), m.clone(), v.clone()
        if g is None:
            new_steps.append(t + 1 if mut == "step_without_grad" else t)
        else:
            t += 1
            new_steps.append(t)
            lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
            if mut == "one_lr_for_all":
                lr = hp[0]["lr"]
            c = coef
            if c is not None and mut == "norm_per_group":
                c = coef_of([x for x, hx in zip(G, hp) if x is not None and hx["lr"] == h["lr"]])
            gs = g if c is None else g * c
            gv = g if mut == "raw_gradient_for_v" else gs
            if mut == "coupled_decay":
                gs = gv = gs + wd * p
            elif mut != "decay_after_update":
                p = p * (1 - lr * wd)
            m = m + (gs - m) * (1 - b1)
            v = v * b2 + (1 - b2) * gv * gv
            tb = t - 1 if mut == "beta_power_t_minus_1" else t
            bc2s = math.sqrt(1 - b2 ** tb) if tb else 1.0
            step_size = lr / (1 - b1 ** tb) if tb else lr
            if mut == "eps_inside_division":
                denom = (v.sqrt() + eps) / bc2s
            elif mut == "eps_under_root":
                denom = (v + eps).sqrt() / bc2s
            else:
                denom = v.sqrt() / bc2s + eps
            p = p - step_size * (m / denom)
            if mut == "decay_after_update":
                p = p * (1 - lr * wd)
        for o, x in zip(out, (p, m, v)):
            o.append(x)
    return out, new_steps


def mutant_case():
    """Large learning rates and weight decay (every term of the update well above the rounding of p), step 1 -> 2, the gradient
    norm far above max_norm = 1, small and large gradient scales in both groups."""
    shapes = [(33,)] * 8
    gscales = [1e-9, 1e-9, 1e-4, 1e-4, 1.0, 1.0, 10.0, 10.0]
    steps = [1] * 8
    hp = [OC.hyper(lr=0.1 if i % 2 == 0 else 0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1) for i in range(8)]
    return (*OC.make_inputs(shapes, gscales, steps, seed=7), steps, hp)


# mistake -> (the output that must fail, the factor by which it must exceed its bound)
MUTANTS = {
    "coupled_decay": ("m", 1e3),
    "decay_after_update": ("p", 1e2),
    "beta_power_t_minus_1": ("p", 1e3),
    "eps_inside_division": ("p", 1e3),
    "eps_under_root": ("p", 1e3),
    "one_lr_for_all": ("p", 1e3),
    "coef_without_1e-6": ("m", 10),
    "coef_unclamped": ("m", 1e3),
    "norm_per_group": ("m", 1e3),
    "raw_gradient_for_v": ("v", 1e3),
}


def test_the_unmutated_float32_step_passes():
    for max_norm in (1.0, 1e9):
        P, G, M, V, steps, hp = mutant_case()
        got, _ = mutant_step(P, G, M, V, steps, hp, max_norm, None)
        assert OC.worst(OC.check_step(P, G, M, V, steps, hp, got, max_norm=max_norm)) <= 1.0


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    P, G, M, V, steps, hp = mutant_case()
    max_norm = 1.0
    if mut == "coef_unclamped":
        max_norm = 1e9                              # a norm far below max_norm: the clamp is what keeps coef at 1
    if mut == "coef_without_1e-6":                  # a norm of the order of 1e-6 clipped to 1e-7: the 1e-6 is half the divisor
        G = [g * (1e-6 / max(float(g.abs().max()), 1e-30)) for g in G]
        M, V = [m * 0 for m in M], [v * 0 for v in V]
        max_norm = 1e-7
    got, _ = mutant_step(P, G, M, V, steps, hp, max_norm, mut)
    res = OC.check_step(P, G, M, V, steps, hp, got, max_norm=max_norm)
    output, factor = MUTANTS[mut]
    print("OPTIMCHECK mutant", mut, {k: f"{r[0]:.3g}" for k, r in res.items()})
    assert res[output][0] > factor, (mut, res)


def test_mutant_step_advanced_without_a_gradient_is_rejected():
    """The mistake shows one step later, in the bias corrections of the parameter that had no gradient."""
    P, G, M, V, steps, hp = mutant_case()
    G1 = [None if i == 4 else g for i, g in enumerate(G)]
    for mut, passes in ((None, True), ("step_without_grad", False)):
        (P1, M1, V1), kept = mutant_step(P, G1, M, V, steps, hp, None, mut)
        got, _ = mutant_step(P1, G, M1, V1, kept, hp, None, None)
        true_steps = [t + (g is not None) for t, g in zip(steps, G1)]
        res = OC.check_step(P1, G, M1, V1, true_steps, hp, got)
        print("OPTIMCHECK mutant step_without_grad" if mut else "OPTIMCHECK two honest steps", {k: f"{r[0]:.3g}" for k, r in res.items()})
        assert (OC.worst(res) <= 1.0) if passes else (res["p"][0] > 1e3 and res["p"][1] == 4), res


# ------------------------------------------------------------------------------------------------- interchange with torch
def _model_and_grads(seed=0, steps=6):
    torch.manual_seed(seed)
    model = PhiEstADMMNet(num_layers=3, M=3, N=4)
    gen = torch.Generator().manual_seed(seed + 1)
    dead = [n for n, _ in model.named_parameters() if "step_adjust_net" in n]      # parameters that never get a gradient
    assert dead
    grads = [{n: None if n in dead else torch.randn(p.shape, generator=gen) * 3.0 for n, p in model.named_parameters()}
             for _ in range(steps)]
    return model, grads


def _groups(model):
    """The reference's two groups (train.py:107-121): some layers at lr / 2, the rest at lr."""
    slow = [p for n, p in model.named_parameters() if "phiLayers" in n or "hLayers" in n]
    fast = [p for n, p in model.named_parameters() if not any(p is q for q in slow)]
    return [{"params": slow, "lr": 5e-4}, {"params": fast, "lr": 1e-3}]


def _make(cls, model, **kw):
    opt = cls(_groups(model), lr=1e-3, weight_decay=1e-3, **kw)
    return opt, torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, eta_min=1e-6)


def _torch_step(model, opt, sched, grads):
    for n, p in model.named_parameters():
        p.grad = None if grads[n] is None else grads[n].clone()
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    opt.step()
    sched.step()


def _snapshot(model, opt):
    """(P, M, V, steps, hp) of every parameter as float32 clones, in named_parameters order."""
    lr = {id(p): g for g in opt.param_groups for p in g["params"]}
    P, M, V, steps, hp = [], [], [], [], []
    for _, p in model.named_parameters():
        st, g = opt.state.get(p, {}), lr[id(p)]
        P.append(p.detach().clone())
        M.append(st["exp_avg"].clone() if st else torch.zeros_like(p))
        V.append(st["exp_avg_sq"].clone() if st else torch.zeros_like(p))
        steps.append(int(st["step"]) if st else 0)
        hp.append(OC.hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"]))
    return P, M, V, steps, hp


def _same_state(model_a, opt_a, model_b, opt_b):
    """Parameters, exp_avg, exp_avg_sq and step counts of two (model, optimiser) pairs have equal bits."""
    Pa, Ma, Va, ta, _ = _snapshot(model_a, opt_a)
    Pb, Mb, Vb, tb, _ = _snapshot(model_b, opt_b)
    return ta == tb and all(OC.same_bits(x, y) for x, y in ((Pa, Pb), (Ma, Mb), (Va, Vb)))


def _module_step(model, opt, sched, grads, fused):
    for n, p in model.named_parameters():
        p.grad = None if grads[n] is None else grads[n].clone()
    if not fused:
        optim.clip_grad_norm_(model.parameters(), max_norm=1.0)
    opt.step()
    sched.step()


def _paired_steps(grads, fused, torch_side, module_side, yardstick):
    """One further step with each optimiser, both free-running.  The side that is NOT the yardstick must land within the one-step
    bound of the float64 oracle computed from the YARDSTICK side's state before the step -- the two trajectories are compared
    with each other, step after step -- and, as an addition, each side within the bound from its own state before the step."""
    names = [n for n, _ in torch_side[0].named_parameters()]
    G = [grads[n] for n in names]
    before = {"torch": _snapshot(*torch_side[:2]), "module": _snapshot(*module_side[:2])}
    _torch_step(*torch_side, grads)
    _module_step(*module_side, grads, fused)
    after = {"torch": _snapshot(*torch_side[:2]), "module": _snapshot(*module_side[:2])}
    other = "module" if yardstick == "torch" else "torch"
    ratios = {}
    for name, frm, got in (("cross", yardstick, other), ("torch_own", "torch", "torch"), ("module_own", "module", "module")):
        P, M, V, steps, hp = before[frm]
        res = OC.check_step(P, G, M, V, steps, hp, after[got][:3], max_norm=1.0)
        ratios[name] = {k: round(r[0], 3) for k, r in res.items()}
        assert OC.worst(res) <= 1.0, (name, res)
    assert after["torch"][3] == after["module"][3] == [t + (g is not None) for t, g in zip(before["torch"][3], G)]
    return ratios


@pytest.mark.parametrize("fused", [False, True], ids=["clip_then_step", "max_grad_norm"])
def test_checkpoints_interchange_with_torch(fused, tmp_path, monkeypatch):
    monkeypatch.setattr(optim.clip_grad_norm_, "route", "tensor")
    kw = dict(route="tensor", max_grad_norm=1.0 if fused else None)
    # torch -> module: three steps with torch, its checkpoint into the module, three more steps with each
    model, grads = _model_and_grads()
    opt, sched = _make(torch.optim.AdamW, model)
    for s in range(3):
        _torch_step(model, opt, sched, grads[s])
    ours_model, _ = _model_and_grads(seed=9)                    # other initial weights: everything must come from the file
    ours, ours_sched = _make(optim.AdamW, ours_model, **kw)
    path = str(tmp_path / "torch.pth")
    harness.save_checkpoint(path, model, opt, sched, epoch=3)
    harness.load_checkpoint(path, ours_model, ours, ours_sched)
    assert _same_state(model, opt, ours_model, ours)            # parameters and state arrived bit for bit
    assert ours.state_dict()["state"].keys() == opt.state_dict()["state"].keys()
    assert [sorted(g) for g in ours.state_dict()["param_groups"]] == [sorted(g) for g in opt.state_dict()["param_groups"]]
    assert [g["lr"] for g in ours.param_groups] == [g["lr"] for g in opt.param_groups]
    for s in range(3, 6):
        r = _paired_steps(grads[s], fused, (model, opt, sched), (ours_model, ours, ours_sched), yardstick="torch")
        print("OPTIMCHECK interchange torch -> module, step", s + 1, r)
    assert [g["lr"] for g in ours.param_groups] == [g["lr"] for g in opt.param_groups]       # the scheduler ran on both
    for (n, p), q in zip(model.named_parameters(), ours_model.parameters()):
        assert (n, opt.state.get(p, {}).keys()) == (n, ours.state.get(q, {}).keys())
        if opt.state.get(p):
            assert float(opt.state[p]["step"]) == float(ours.state[q]["step"]) == 6.0
    # module -> torch: the module's checkpoint into a fresh torch optimiser, three more steps with each
    path = str(tmp_path / "ours.pth")
    harness.save_checkpoint(path, ours_model, ours, ours_sched, epoch=6)
    back_model, _ = _model_and_grads(seed=10)
    back, back_sched = _make(torch.optim.AdamW, back_model)
    harness.load_checkpoint(path, back_model, back, back_sched)
    assert _same_state(ours_model, ours, back_model, back)
    assert back.state_dict()["state"].keys() == ours.state_dict()["state"].keys()
    assert [sorted(g) for g in back.state_dict()["param_groups"]] == [sorted(g) for g in ours.state_dict()["param_groups"]]
    assert [g["lr"] for g in back.param_groups] == [g["lr"] for g in ours.param_groups]
    extra = _model_and_grads(seed=5, steps=3)[1]
    for s in range(3):
        r = _paired_steps(extra[s], fused, (back_model, back, back_sched), (ours_model, ours, ours_sched), yardstick="module")
        print("OPTIMCHECK interchange module -> torch, step", s + 7, r)
    assert [g["lr"] for g in back.param_groups] == [g["lr"] for g in ours.param_groups]


# ---------------------------------------------------------------------------------------------------------------- properties
def test_fused_clipping_equals_clip_then_step_bit_for_bit(monkeypatch):
    monkeypatch.setattr(optim.clip_grad_norm_, "route", "tensor")
    P, G, M, V, steps, hp = case(9, 1e-3, seed=2)
    fused, opt, params = OC.module_step(optim.AdamW, P, G, M, V, steps, hp, max_norm=1.0, route="tensor")
    assert OC.same_bits([q.grad for q in params], G)                        # the gradients stay unscaled
    two, params2 = OC._as_optimizer(optim.AdamW, P, G, M, V, steps, hp, "cpu", torch.float32, route="tensor")
    total = optim.clip_grad_norm_(params2, 1.0)
    two.step()
    got2 = OC._read_back(two, params2, M, V)
    assert all(OC.same_bits(a, b) for a, b in zip(fused, got2))
    assert OC.same_bits([total], [opt.last_grad_norm]) and total.dim() == 0 and float(total) > 1.0
    ref = [q.detach().clone().requires_grad_() for q in G]
    for r, g in zip(ref, G):
        r.grad = g.clone()
    assert abs(float(torch.nn.utils.clip_grad_norm_(ref, 1.0)) - float(total)) <= 2 * OC.U * float(total)


def test_parameters_without_a_gradient_are_untouched_and_stateless():
    P, G, M, V, steps, hp = case(0, 0.1, seed=4)
    G = [None if i % 3 == 0 else g for i, g in enumerate(G)]
    got, opt, params = OC.module_step(optim.AdamW, P, G, M, V, steps, hp, max_norm=1.0, route="tensor")
    assert OC.worst(OC.check_step(P, G, M, V, steps, hp, got, max_norm=1.0)) <= 1.0
    for q, g, p in zip(params, G, P):
        if g is None:
            assert q not in opt.state and OC.same_bits([q], [p])
        else:
            assert set(opt.state[q]) == {"step", "exp_avg", "exp_avg_sq"} and opt.state[q]["step"].device.type == "cpu"
            assert opt.state[q]["step"].dtype == torch.float32 and float(opt.state[q]["step"]) == 1.0


def test_argument_errors():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        optim.AdamW([])
    with pytest.raises(ValueError):
        optim.AdamW([p], route="eager")
    for key in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=key):
            optim.AdamW([p], route="tensor", **{key: True})
    with pytest.raises(TypeError):
        optim.AdamW([p], lr=torch.tensor(1e-3), route="tensor", foreach=False)
    opt = optim.AdamW([p], route="tensor", foreach=True, fused=None)            # accepted and ignored
    p.grad = torch.ones(3)
    opt.step()
    opt.param_groups[0]["amsgrad"] = True                                        # as load_state_dict could
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = False
    opt.param_groups[0]["betas"] = (torch.tensor(0.9), 0.999)
    with pytest.raises(TypeError):
        opt.step()
    assert float(opt.state[p]["step"]) == 1.0                                    # a refused step is not counted
    # the "hip" route takes float32 device tensors only, and says so instead of taking another path
    hip = optim.AdamW([p])
    with pytest.raises(ValueError, match="device"):
        hip.step()
    assert hip.state[p] == {} or float(hip.state[p]["step"]) == 0.0
    d = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
    d.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(TypeError, match="float32"):
        optim.AdamW([d]).step()
    s = torch.nn.Parameter(torch.zeros(4, 2))
    s.grad = torch.zeros(4, 2).to_sparse()
    with pytest.raises(ValueError, match="sparse"):
        optim.AdamW([s], route="tensor").step()
    with pytest.raises(ValueError, match="device"):
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_([p], 1.0, norm_type=float("inf"))


def test_clip_grad_norm_edge_cases(monkeypatch):
    monkeypatch.setattr(optim.clip_grad_norm_, "route", "tensor")
    empty = optim.clip_grad_norm_([], 1.0)
    assert empty.dim() == 0 and float(empty) == 0.0
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0       # no gradient at all
    for bad in (float("inf"), float("nan")):
        ours = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(()))]
        theirs = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(()))]
        for q in ours + theirs:
            q.grad = torch.full_like(q, 2.0)
        ours[0].grad[1] = theirs[0].grad[1] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            optim.clip_grad_norm_(ours, 1.0, error_if_nonfinite=True)
        assert float(ours[0].grad[0]) == 2.0                                                     # nothing was scaled
        a, b = optim.clip_grad_norm_(ours, 1.0), torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.isinf(), b.isinf())
        for q, r in zip(ours, theirs):                  # torch: coef = 0 for an infinite norm, inf * 0 = NaN, NaN stays NaN
            assert torch.equal(q.grad.isnan(), r.grad.isnan()) and torch.equal(q.grad.nan_to_num(), r.grad.nan_to_num())


def test_an_infinite_gradient_gives_what_torch_gives():
    P, G, M, V, steps, hp = case(1, 1e-3, seed=6)
    G[5].reshape(-1)[0] = float("inf")
    G[9].reshape(-1)[-1] = float("-inf")
    for max_norm in (None, 1.0):
        got, _, _ = OC.module_step(optim.AdamW, P, G, M, V, steps, hp, max_norm=max_norm, route="tensor")
        par = OC.parent_step(P, G, M, V, steps, hp, max_norm=max_norm)
        for a, b in zip(got, par):
            for x, y in zip(a, b):
                assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.isinf(), y.isinf()), max_norm
                assert torch.equal(x.isinf() & (x > 0), y.isinf() & (y > 0))


# ------------------------------------------------------------------------------------------------------------------ drop-in
CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
adamw, clip = torch.optim.AdamW, torch.nn.utils.clip_grad_norm_
from admm_net_amd import dropin
dropin.activate(optim={flag})
rebound = (torch.optim.AdamW is not adamw, torch.nn.utils.clip_grad_norm_ is not clip)
assert rebound == ({flag}, {flag}), rebound
def run(cls, clipper):
    torch.manual_seed(0)
    w = [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(()))]
    opt = cls([{{'params': (q for q in w[:1]), 'lr': 1e-2}}, {{'params': w[1:]}}], lr=1e-3, weight_decay=1e-3)
    for _ in range(3):
        for q in w:
            q.grad = torch.randn(q.shape) * 5
        norm = clipper(w, max_norm=1.0)
        opt.step()
    return opt, [q.detach() for q in w] + [norm]
opt, got = run(torch.optim.AdamW, torch.nn.utils.clip_grad_norm_)
assert type(opt) is adamw, type(opt)                    # CPU parameters: torch's own class took the call
assert isinstance(torch.optim.AdamW, type) and isinstance(opt, torch.optim.AdamW)      # the name is still a type
class Mine(torch.optim.AdamW):
    pass
mine = Mine([torch.nn.Parameter(torch.zeros(2))], lr=1e-2)
assert type(mine) is Mine and isinstance(mine, adamw) and mine.param_groups[0]['lr'] == 1e-2
assert isinstance(mine, torch.optim.AdamW) and not isinstance(opt, Mine)
_, want = run(adamw, clip)
assert all(torch.equal(a, b) for a, b in zip(got, want))
print("CHILD OK")
"""


@pytest.mark.parametrize("flag", [True, False], ids=["optim", "plain"])
def test_activate_rebinds_only_on_request(flag):
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, flag=flag)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout + r.stderr


def test_activate_optim_submodule_and_launcher_flags(tmp_path):
    script = tmp_path / "probe.py"
    script.write_text("import sys, torch\nprint('PROBE', torch.optim.AdamW.__module__, any(p.endswith('optional') for p in sys.path), sys.argv[1:])\n")
    for flags, module, loss in ((["--hip-loss", "--hip-optim"], "admm_net_amd.dropin._rebind_optim", True),
                                (["--hip-optim", "--hip-loss"], "admm_net_amd.dropin._rebind_optim", True),
                                (["--hip-optim"], "admm_net_amd.dropin._rebind_optim", False),
                                ([], "torch.optim.adamw", False)):
        r = subprocess.run([sys.executable, "-m", "admm_net_amd.dropin", *flags, str(script), "--hip-optim"], capture_output=True,
                           text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert f"PROBE {module} {loss} ['--hip-optim']" in r.stdout, (flags, r.stdout)
    r = subprocess.run([sys.executable, "-c", "import torch, admm_net_amd.dropin.activate_optim as a; print(torch.optim.AdamW.__module__)"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "_rebind_optim" in r.stdout, r.stdout + r.stderr
