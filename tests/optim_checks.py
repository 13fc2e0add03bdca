"""The comparison behind tests/test_optim.py and tests/test_gpu_optim.py: ONE step of clipping + AdamW from given float32 inputs.

Inputs: lists P, G, M, V of float32 tensors (G[i] None: the parameter has no gradient), per tensor the step count BEFORE the call
and its hyper-parameters ``{"lr", "betas", "eps", "weight_decay"}``, optionally ``max_norm`` (clip the 2-norm of all gradients).

* oracle: torch's formulas (torch.optim.adam._single_tensor_adam, decoupled weight decay; clip_grad_norm_) evaluated in float64
  from the same float32 values with Python-double scalars -- ``oracle_step``.
* parent: torch's own float32 single-tensor AdamW (``foreach=False``; ``torch.nn.utils.clip_grad_norm_`` before it when
  ``max_norm``) on the same inputs, on the device of the code under test -- ``parent_step``.
* bound, per tensor and output ("3 x the float32 parent + 4 u"):
      3 max|parent - oracle|  +  4 u max(terms),   u = 2^-24,
  terms = |p| + |dp| for p (dp: the oracle's change of p), |m| + |g| for m, |v| + g^2 for v, all from the oracle.
  A parameter without a gradient must come back bit for bit (bound 0).
* norm: |total_norm - sqrt(sum g^2)_f64| <= 1 u norm (the float64 sum of <= 1e7 terms adds < 1e-9 relative, the cast 1/2 u), and
  coef must have exactly the bits of torch's float32 expression clamp(max_norm / (total_norm + 1e-6), max=1) applied to the
  returned total_norm -- ``check_norm``.
"""
import math

import torch

U = 2.0 ** -24
OUTPUTS = ("p", "m", "v")


def hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    return {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay}


def make_inputs(shapes, gscales, steps, seed, zero_state_at_step0=True):
    """Seeded float32 (P, G, M, V) on the CPU: tensor i of shape shapes[i], gradient scale gscales[i], every fifth gradient entry
    exactly zero; the state of a tensor at step 0 is zero (as torch creates it), otherwise of the gradient's scale."""
    gen = torch.Generator().manual_seed(seed)
    P, G, M, V = [], [], [], []
    for shape, gs, t in zip(shapes, gscales, steps):
        r = lambda: torch.randn(shape, generator=gen, dtype=torch.float32)
        g = r() * gs
        if g.numel():
            flat = g.reshape(-1)
            flat[::5] = 0.0
        live = 0.0 if (t == 0 and zero_state_at_step0) else 1.0
        P.append(r())
        G.append(g)
        M.append(r() * (gs * 0.3 * live))
        V.append((r() * gs).square() * (0.5 * live))
    return P, G, M, V


SIZES = [(), (1,), (3,), (1023,), (1024,), (5, 205), (4097,)]      # 0-dim, 1, 3, 1023, 1024, 1025, 4097 elements
GSCALES = [1e-9, 1e-4, 1.0, 1e3]
HYPERS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-8)]   # two groups


def size_case(step, wd, seed=0, steps=None):
    """Every size at every gradient scale (28 tensors), the two hyper-parameter sets alternating; ``steps``: per-tensor counts."""
    shapes = [s for s in SIZES for _ in GSCALES]
    gscales = [g for _ in SIZES for g in GSCALES]
    steps = [step] * len(shapes) if steps is None else [steps[i % len(steps)] for i in range(len(shapes))]
    hp = [hyper(weight_decay=wd, **HYPERS[(i // 2) % 2]) for i in range(len(shapes))]
    return (*make_inputs(shapes, gscales, steps, seed), steps, hp)


def f64_coef(G, max_norm):
    """(norm, coef) in float64 over the gradients that are not None."""
    ss = sum(float(g.detach().double().cpu().square().sum()) for g in G if g is not None)
    norm = math.sqrt(ss)
    return norm, min(1.0, max_norm / (norm + 1e-6))


def oracle_step(P, G, M, V, steps, hp, max_norm=None):
    """float64 (P', M', V') from the float32 inputs."""
    coef = f64_coef(G, max_norm)[1] if max_norm is not None else None
    out = ([], [], [])
    for p, g, m, v, t, h in zip(P, G, M, V, steps, hp):
        p, m, v = (x.detach().double().cpu().clone() for x in (p, m, v))
        if g is not None:
            g = g.detach().double().cpu()
            if coef is not None:
                g = g * coef
            lr, (b1, b2), eps, wd, t = h["lr"], h["betas"], h["eps"], h["weight_decay"], t + 1
            p = p * (1 - lr * wd)
            m = m + (g - m) * (1 - b1)
            v = v * b2 + (1 - b2) * g * g
            denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
            p = p - (lr / (1 - b1 ** t)) * (m / denom)
        for o, x in zip(out, (p, m, v)):
            o.append(x)
    return out


def _as_optimizer(cls, P, G, M, V, steps, hp, device, dtype, **kwargs):
    """An optimiser of class ``cls`` with one parameter group per tensor and the state loaded as torch keeps it."""
    params = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in P]
    opt = cls([dict(h, params=[q]) for q, h in zip(params, hp)], **kwargs)
    for q, g, m, v, t in zip(params, G, M, V, steps):
        q.grad = None if g is None else g.detach().to(device=device, dtype=dtype).clone()
        if t > 0:
            opt.state[q] = {"step": torch.tensor(float(t), dtype=torch.float32),
                            "exp_avg": m.detach().to(device=device, dtype=dtype).clone(),
                            "exp_avg_sq": v.detach().to(device=device, dtype=dtype).clone()}
    return opt, params


def _read_back(opt, params, M, V):
    state = lambda q, key, old: opt.state[q][key].detach() if key in opt.state.get(q, {}) else old
    return ([q.detach() for q in params], [state(q, "exp_avg", m) for q, m in zip(params, M)],
            [state(q, "exp_avg_sq", v) for q, v in zip(params, V)])


def parent_step(P, G, M, V, steps, hp, max_norm=None, device="cpu"):
    """torch's float32 single-tensor AdamW (and clip_grad_norm_) on the same inputs on ``device``."""
    opt, params = _as_optimizer(torch.optim.AdamW, P, G, M, V, steps, hp, device, torch.float32, foreach=False)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    opt.step()
    return _read_back(opt, params, M, V)


def module_step(cls, P, G, M, V, steps, hp, max_norm=None, device="cpu", dtype=torch.float32, **kwargs):
    """The optimiser under test (``admm_net_amd.optim.AdamW``) on the same inputs: returns ((P', M', V'), the optimiser, params)."""
    opt, params = _as_optimizer(cls, P, G, M, V, steps, hp, device, dtype, max_grad_norm=max_norm, **kwargs)
    opt.step()
    return _read_back(opt, params, M, V), opt, params


def _max(x):
    return float(x.abs().max()) if x.numel() else 0.0


def check_step(P, G, M, V, steps, hp, got, max_norm=None, device="cpu", parent=None, oracle=None):
    """{output: (worst error / bound over the tensors, that tensor, its error, its bound, the parent's error / bound there)}.
    An output passes when its ratio is <= 1; a non-finite error or a change of an untouched tensor gives inf.
    ``parent`` / ``oracle``: results computed elsewhere (the GPU tests' float64 stand-in run is their oracle)."""
    ora = oracle if oracle is not None else oracle_step(P, G, M, V, steps, hp, max_norm)
    ora = tuple([x.detach().double().cpu() for x in o] for o in ora)
    par = parent if parent is not None else parent_step(P, G, M, V, steps, hp, max_norm, device)
    coef = f64_coef(G, max_norm)[1] if max_norm is not None else 1.0
    res = {k: (0.0, -1, 0.0, 0.0, 0.0) for k in OUTPUTS}
    for i, g in enumerate(G):
        old = {"p": P[i], "m": M[i], "v": V[i]}
        for k, o, pa, go in zip(OUTPUTS, ora, par, got):
            o, pa, go = o[i], pa[i].detach().double().cpu(), go[i].detach().double().cpu()
            assert go.shape == o.shape, (k, i, go.shape, o.shape)
            err, perr = _max(go - o), _max(pa - o)
            if g is None:
                bound = 0.0
            else:
                g64 = g.detach().double().cpu() * coef
                x = old[k].detach().double().cpu()
                terms = {"p": x.abs() + (o - x).abs(), "m": o.abs() + g64.abs(), "v": o.abs() + g64 * g64}[k]
                bound = 3 * perr + 4 * U * _max(terms)
            if not math.isfinite(err):
                ratio = math.inf
            elif bound == 0.0:
                ratio = 0.0 if err == 0.0 else math.inf
            else:
                ratio = err / bound
            if ratio > res[k][0] or res[k][1] < 0:
                res[k] = (ratio, i, err, bound, (perr / bound) if bound else 0.0)
    return res


def worst(res):
    return max(r[0] for r in res.values())


def torch_coef(total_norm, max_norm):
    """torch's own float32 expression (clip_grad._clip_grads_with_norm_) applied to a float32 total norm, on the CPU."""
    t = total_norm.detach().float().cpu().reshape(())
    return torch.clamp(max_norm / (t + 1e-6), max=1.0)


def check_norm(G, max_norm, total_norm, coef):
    """(|total_norm - norm_f64| / (u norm), coef has the bits of torch's expression on total_norm)."""
    norm = f64_coef(G, max_norm)[0]
    got = float(total_norm.detach().double().cpu())
    want = torch_coef(total_norm, max_norm)
    same = torch.equal(coef.detach().float().cpu().reshape(()).view(torch.int32), want.view(torch.int32))
    ratio = abs(got - norm) / (U * norm) if norm > 0 else (0.0 if got == 0.0 else math.inf)
    return ratio, same


def same_bits(a, b):
    return all(x.shape == y.shape and torch.equal(x.detach().cpu().contiguous().view(torch.int32), y.detach().cpu().contiguous().view(torch.int32))
               for x, y in zip(a, b))
