"""Inputs for the loss tests (tests/test_losses.py, tests/test_gpu_losses.py) and for tests/golden/make_golden_loss.py.

The phase loss wraps ``arg phi - arg phi_true`` into [-pi, pi).  At a raw difference of exactly +-pi a last-bit change of
atan2 flips the sign of the wrapped value: a property of the loss, not of an implementation.  So phases here are built from
explicit angles whose raw difference keeps ``MARGIN`` from +-pi, and a share of the entries is placed beyond +-pi on purpose,
so the wrap is exercised.  ``check_phase_margin`` asserts both on the float32 numbers a test really feeds in (1e-3 rad, a
quarter of the entries); random draws do not satisfy it.
"""
import math

import torch

MARGIN = 0.01          # construction margin, rad; check_phase_margin asserts 1e-3 on the rounded inputs


def check_phase_margin(phi, phi_true):
    d = (torch.angle(phi) - torch.angle(phi_true)).double().reshape(-1)
    live = (phi.reshape(-1) != 0) & (phi_true.reshape(-1) != 0)
    gap = (d[live].abs() - math.pi).abs().min().item()
    beyond = (d.abs() > math.pi).double().mean().item()
    assert gap >= 1e-3, f"a raw phase difference lies {gap:.2e} rad from +-pi"
    assert beyond >= 0.25, f"only {beyond:.2f} of the raw phase differences lie beyond +-pi"
    return gap, beyond


def phase_pair(B, D, seed, zeros=True):
    """(phi, phi_true) complex64 [B, D].  Of every five entries two have |raw difference| > pi by construction; the others
    draw both angles from [-3.1, 3.1] and are redrawn while the difference is within MARGIN of +-pi.  ``zeros``: one entry of phi
    (the third, one of those not placed beyond +-pi; the first of two) is 0 -- the gradient there is defined as 0."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: torch.rand(B, D, generator=g, dtype=torch.float64) * (hi - lo) + lo
    th, tt = u(-3.1, 3.1), u(-3.1, 3.1)
    for _ in range(64):
        near = ((th - tt).abs() - math.pi).abs() < MARGIN
        if not near.any():
            break
        th = torch.where(near, u(-3.1, 3.1), th)
    assert not (((th - tt).abs() - math.pi).abs() < MARGIN).any()
    far = (torch.arange(B * D).reshape(B, D) % 5) < 2                        # |difference| in [3.4, 6.2]
    sign = torch.where(torch.rand(B, D, generator=g) < 0.5, -1.0, 1.0).double()
    th = torch.where(far, sign * u(1.7, 3.1), th)
    tt = torch.where(far, -sign * u(1.7, 3.1), tt)
    r, rt = u(0.2, 2.0), u(0.2, 2.0)
    phi, phi_true = torch.polar(r, th).to(torch.complex64), torch.polar(rt, tt).to(torch.complex64)
    if zeros and B * D > 1:
        phi.view(-1)[2 if B * D >= 3 else 0] = 0
    check_phase_margin(phi, phi_true)
    return phi, phi_true


def anm_case(B, Lmax, D, seed, L="mixed", zero_row=True):
    """Inputs of BasicANMLoss: tau, f, conf, tau_true, f_true float32 [B, Lmax], L_true int64 [B], phi complex64 [B, D].
    ``L``: "mixed" (0, 1, ..., Lmax in turn), "none" (all 0), "all" (all Lmax) or a list.  ``zero_row``: the last signal's phi
    is all zero (its norm has gradient 0) when B > 1."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(B, Lmax, generator=g)
    tau, f, conf, tau_true, f_true = r(), r() - 0.5, r(), r(), r() - 0.5
    if L == "mixed":
        L_true = torch.arange(B) % (Lmax + 1)
    elif L in ("none", "all"):
        L_true = torch.full((B,), 0 if L == "none" else Lmax)
    else:
        L_true = torch.tensor(L)
    phi = torch.randn(B, D, generator=g, dtype=torch.complex64)
    if zero_row and B > 1:
        phi[-1] = 0
    return dict(tau=tau, f=f, conf=conf, tau_true=tau_true, f_true=f_true, L_true=L_true.to(torch.int64), phi=phi)
