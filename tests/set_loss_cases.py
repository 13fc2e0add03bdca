"""Inputs for the tests of the assignment loss of the head (tests/test_set_loss.py, tests/test_gpu_set_loss.py; no test here).

The loss is the minimum over assignments of one expression.  Where two assignments are optimal to rounding, which one a solver
returns is a property of the solver, not of the loss, and a comparison of ``assign`` says nothing.  So every signal of every case
of the table keeps a MARGIN: the best value with another assignment lies at least ``MIN_GAP`` (relative to loss_b) above the
optimum (``margins``; tests/test_set_loss.py asserts it for every case, none left out -- the seeds below were chosen on the
host so that it holds).  The two exact ties (``TIES``) are kept apart: there only the values are compared.

    SHAPES    (Lmax, Lt): a single slot and target, more targets than slots and the reverse, one wave's worth of both
    VARIANTS  L_true all 0 / 0 .. Lt in turn / all Lt; w_conf 0, 0.1, 5; scales (1, 1) and (16, 10); no period and (1, 1) with pairs
              that are closest across the wrap
"""
import functools
import math

import numpy as np
import torch

from admm_net_amd import losses

MIN_GAP = 1e-9
SHAPES = [(1, 1), (1, 3), (3, 1), (3, 3), (5, 3), (3, 5), (16, 8), (64, 64), (64, 3)]
# name: (L, w_conf, scale, period)
VARIANTS = {
    "plain": ("mixed", 0.1, (1.0, 1.0), None),
    "none": ("none", 0.1, (1.0, 1.0), None),
    "all-w0": ("all", 0.0, (1.0, 1.0), None),
    "w5-scaled": ("mixed", 5.0, (16.0, 10.0), None),
    "periodic": ("mixed", 0.1, (1.0, 1.0), (1.0, 1.0)),
    "periodic-w5-scaled-all": ("all", 5.0, (16.0, 10.0), (1.0, 1.0)),
}
LAM = 0.37
BATCHES = (1, 3, 4, 5, 257)                          # one signal, a slab less one, a slab, a slab and one, 64 slabs and one


def variants_of(B):
    """The variants a batch size is run with, on the host and on the GPU: all of them up to B = 5, two at 257 (the float64 mirror
    of 257 signals is a host loop)."""
    return list(VARIANTS) if B <= 5 else ["w5-scaled", "periodic"]


KEYS = ("tau", "f", "conf", "tau_true", "f_true", "L_true", "phi")


def options(variant):
    """The keyword options of ``TensorLossKernels.set`` / ``ops.loss_set`` of a variant."""
    _, w_conf, scale, period = VARIANTS[variant]
    return dict(lambda_reg=LAM, w_conf=w_conf, scale=scale, period=period)


def draw(B, Lmax, Lt, seed, L="mixed", periodic=False, D=7, zero_row=True):
    """tau, f, conf float32 [B, Lmax]; tau_true, f_true float32 [B, Lt]; L_true int64 [B]; phi complex64 [B, D].  Slots are noisy
    copies of targets in a shuffled order (four in five) or strays, the confidences uniform.  ``periodic``: the targets fill the
    whole period and the copies are folded back into it, so some pairs are closest across the wrap.  ``L``: "mixed" (0 .. Lt in
    turn), "none", "all" or a list."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    if periodic:
        tau_true, f_true = u(B, Lt), u(B, Lt) - 0.5
    else:
        tau_true, f_true = 0.1 + 0.8 * u(B, Lt), 0.8 * u(B, Lt) - 0.4
    if L == "mixed":
        L_true = torch.arange(B) % (Lt + 1)
    elif L in ("none", "all"):
        L_true = torch.full((B,), 0 if L == "none" else Lt)
    else:
        L_true = torch.tensor(L)
    tau, f = torch.empty(B, Lmax, dtype=torch.float64), torch.empty(B, Lmax, dtype=torch.float64)
    for b in range(B):
        order = torch.randperm(Lt, generator=g)
        place = torch.randperm(Lmax, generator=g)
        for i in range(Lmax):
            copy = i < Lt and u(1).item() < 0.8
            s = place[i]
            if copy:
                tau[b, s] = tau_true[b, order[i]] + 0.03 * torch.randn(1, generator=g, dtype=torch.float64).item()
                f[b, s] = f_true[b, order[i]] + 0.03 * torch.randn(1, generator=g, dtype=torch.float64).item()
            else:
                tau[b, s], f[b, s] = (u(1).item(), u(1).item() - 0.5) if periodic else (0.1 + 0.8 * u(1).item(), 0.8 * u(1).item() - 0.4)
        if periodic:                                     # target 0 at the upper edge of both axes, one slot just beyond it
            tau_true[b, 0], f_true[b, 0] = 0.98 + 0.01 * u(1).item(), 0.485 + 0.01 * u(1).item()
            tau[b, place[0]], f[b, place[0]] = tau_true[b, 0] + 0.03, f_true[b, 0] + 0.02
    if periodic:
        tau, f = tau - torch.floor(tau), f - torch.floor(f + 0.5)
    phi = torch.randn(B, D, generator=g, dtype=torch.complex64)
    if zero_row and B > 1:
        phi[-1] = 0
    f32 = lambda t: t.to(torch.float32)
    return dict(tau=f32(tau), f=f32(f), conf=f32(u(B, Lmax)), tau_true=f32(tau_true), f_true=f32(f_true),
                L_true=L_true.to(torch.int64), phi=phi)


@functools.lru_cache(maxsize=None)
def table_case(B, Lmax, Lt, variant):
    """One case of the table (cached: a reference is computed once and shared; treat the tensors as read-only)."""
    L, _, _, period = VARIANTS[variant]
    seed = 1000 * B + 10 * Lmax + Lt + 7 * list(VARIANTS).index(variant)
    return draw(B, Lmax, Lt, seed, L=L, periodic=period is not None)


def f64(c):
    return {k: (v if k == "L_true" else v.to(torch.complex128 if v.is_complex() else torch.float64)) for k, v in c.items()}


def args(c):
    return [c[k] for k in KEYS]


@functools.lru_cache(maxsize=None)
def reference(B, Lmax, Lt, variant):
    """``TensorLossKernels.set`` in float64 on the host for a case of the table: (out, assign, norms, status, rows)."""
    return losses.TensorLossKernels.set(*args(f64(table_case(B, Lmax, Lt, variant))), **options(variant))


def margins(c, w_conf, scale, period, **_):
    """The relative gap of every live signal of a case with n >= 1, as ``set_assign_host`` measures it."""
    n = c["L_true"].clamp(0, c["tau_true"].shape[1])
    gaps = []
    for b in range(c["tau"].shape[0]):
        rows = [c[k][b].double().numpy() for k in KEYS[:5]]
        if n[b] == 0 or not all(np.isfinite(r).all() for r in rows[:3]) or not all(np.isfinite(r[:n[b]]).all() for r in rows[3:]):
            continue
        gaps.append(losses.set_assign_host(*rows, int(n[b]), w_conf=w_conf, scale=scale, period=period, with_gap=True)[2])
    return gaps


def crosses_the_wrap(c, assign, period):
    """How many matched pairs of a case are closest across the wrap of either axis."""
    at = assign.clamp(min=0).long()
    far = ((c["tau"].double() - c["tau_true"].double().gather(1, at)).abs() > period[0] / 2) | \
          ((c["f"].double() - c["f_true"].double().gather(1, at)).abs() > period[1] / 2)
    return int((far & (assign >= 0)).sum())


def one(tau, f, conf, tau_true, f_true, n, D=3):
    """A batch of one signal from lists."""
    t = lambda v: torch.tensor([v], dtype=torch.float32)
    return dict(tau=t(tau), f=t(f), conf=t(conf), tau_true=t(tau_true), f_true=t(f_true), L_true=torch.tensor([n], dtype=torch.int64),
                phi=torch.ones(1, D, dtype=torch.complex64))


# ---- designed cases: name -> (case, options, the assignment the definition gives) -------------------------------------------------
PLAIN = dict(lambda_reg=0.0, w_conf=0.1, scale=(1.0, 1.0), period=None)
DESIGNED = {
    # two slots astride one target: the confident one is matched (loss 0.0011 either way)
    "confident-first": (one([0.30, 0.32], [0.0, 0.0], [0.9, 0.1], [0.31], [0.0], 1), PLAIN, [0, -1]),
    "confident-second": (one([0.30, 0.32], [0.0, 0.0], [0.1, 0.9], [0.31], [0.0], 1), PLAIN, [-1, 0]),
    # the per-slot term changes the assignment: the nearer slot (d2 1e-4 against 4e-4) is unsure, 0.05 (1 - 2 conf) decides
    "term-decides": (one([0.30, 0.33], [0.0, 0.0], [0.1, 0.9], [0.31], [0.0], 1), PLAIN, [-1, 0]),
    # a truth past n lies on the slot: it must not be used
    "truth-past-n": (one([0.5], [0.0], [0.7], [0.1, 0.5], [0.0, 0.0], 1), PLAIN, [0]),
    # more targets than slots: the normaliser is n = 3, not k = 2
    "n-above-slots": (one([0.2, 0.6], [0.1, -0.1], [0.8, 0.6], [0.62, 0.9, 0.23], [-0.1, 0.3, 0.1], 3), PLAIN, [2, 0]),
    # closest across the wrap: 0.98 to 0.01 is 0.03 apart with period 1, and f 0.49 to -0.49 is 0.02 apart
    "across-the-wrap": (one([0.98, 0.40], [0.49, 0.0], [0.9, 0.8], [0.45, 0.01], [0.05, -0.49], 2),
                        dict(PLAIN, period=(1.0, 1.0)), [1, 0]),
    # five slots, three targets, the matched slots are not the first three and not in order
    "shuffled": (one([0.9, 0.5, 0.1, 0.31, 0.7], [0.0] * 5, [0.2, 0.9, 0.7, 0.1, 0.6], [0.72, 0.12, 0.52], [0.0] * 3, 3), PLAIN,
                 [-1, 2, 1, -1, 0]),
}
# mirror-image slots: two assignments with equal values exactly
TIES = {
    "mirror-tau": (one([0.25, 0.75], [0.0, 0.0], [0.5, 0.5], [0.5], [0.0], 1), PLAIN),
    "mirror-f": (one([0.5, 0.5, 0.5], [-0.125, 0.125, 0.375], [0.25, 0.25, 0.75], [0.5], [0.0], 1), PLAIN),
}


def with_bad_values():
    """(case, options, dead signals, status): B = 6, 3 x 3; signal 1 has a NaN prediction, signal 3 a NaN truth inside its first
    n, signal 4 a NaN truth PAST n (it counts as usual), signal 2 an infinite confidence."""
    c = {k: v.clone() for k, v in draw(6, 3, 3, seed=77, L=[3, 2, 1, 2, 1, 3]).items()}
    c["tau"][1, 2] = float("nan")
    c["conf"][2, 0] = float("inf")
    c["f_true"][3, 1] = float("nan")
    c["tau_true"][4, 2] = float("nan")
    return c, dict(PLAIN, lambda_reg=LAM), [1, 2, 3], [0, 3]


def out_of_range():
    """(case, options, the same case with L_true held to [0, Lt], status): B = 5, 3 x 4 with one L_true of -1 and one of Lt + 1."""
    c = draw(5, 3, 4, seed=78, L=[2, -1, 4, 5, 0])
    return c, dict(PLAIN, lambda_reg=LAM), dict(c, L_true=c["L_true"].clamp(0, 4)), [2, 0]


def gap_is_kept(gaps):
    return all(g >= MIN_GAP and not math.isnan(g) for g in gaps)
