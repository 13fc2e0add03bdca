"""Inputs and the written-out definition behind tests/test_spectral_loss.py and tests/test_gpu_spectral_loss.py.

``explicit`` evaluates the three spectrum terms of ``losses.PhiSpectralLoss`` one sample at a time from explicit D x points atom
matrices built with ``torch.exp`` -- no separable product, no table -- in differentiable float64 operations:

    a(tau, f)[ks xbase + kd] = exp(j 2 pi (ks f - kd tau)),  z = sum_i conj(phi[i]) a[i],  S = |z|^2
    grid: taus_p = p / nx, fs_q = -0.5 + q / ny, nx = r xbase, ny = r ybase (one point on an axis of base 1)
    spectral = mean_grid (S / mean S - S* / mean S*)^2,  distribution = 1 - sum |z| |z*| / sqrt(sum S sum S*),
    target = mean_{l<L} (1 - |z(tau_l, f_l)|^2 / (D ||phi||^2)), 0 for L = 0; an all-zero phi or phi_true row gives 0 everywhere.

``mistake`` turns it into one of the one-mistake stand-ins that tests/test_spectral_loss.py shows to be rejected.
"""
import math

import torch

MISTAKES = ("tau_sign", "axes", "max", "L0")         # (the fifth, the factor 2 of the gradient, is applied to the gradient)


def case(B, xbase, ybase, Lmax, seed, L="mixed", zero_phi=None, zero_true=None):
    """{phi, phi_true [B, D] complex64, tau_true, f_true [B, Lmax] float32, L_true [B] int64}; phi is a scaled, rotated phi_true
    plus noise of the same size, so the terms are neither 0 nor saturated."""
    g = torch.Generator().manual_seed(seed)
    D = xbase * ybase
    c = lambda: torch.randn(B, D, dtype=torch.complex64, generator=g)
    phi_true = c()
    phi = (0.6 - 0.3j) * phi_true + 0.8 * c()
    if zero_phi is not None:
        phi[zero_phi] = 0
    if zero_true is not None:
        phi_true[zero_true] = 0
    tau = torch.rand(B, Lmax, generator=g)
    f = torch.rand(B, Lmax, generator=g) - 0.5
    if L == "mixed":
        L_true = torch.arange(B) % (Lmax + 1)
    elif L == "none":
        L_true = torch.zeros(B, dtype=torch.int64)
    elif L == "all":
        L_true = torch.full((B,), Lmax, dtype=torch.int64)
    else:
        L_true = torch.tensor(L, dtype=torch.int64)
    return {"phi": phi, "phi_true": phi_true, "tau_true": tau, "f_true": f, "L_true": L_true}


def truth_of(c):
    return {k: c[k] for k in ("tau_true", "f_true", "L_true")}


def atoms(taus, fs, xbase, ybase, tau_sign=-1.0):
    """[D, len(taus)] complex128: column j is a(taus[j], fs[j])."""
    ks = torch.arange(ybase, dtype=torch.float64).repeat_interleave(xbase).reshape(-1, 1)
    kd = torch.arange(xbase, dtype=torch.float64).repeat(ybase).reshape(-1, 1)
    return torch.exp(2j * math.pi * (ks * fs.reshape(1, -1) + tau_sign * kd * taus.reshape(1, -1)))


def grid_points(xbase, ybase, r):
    nx, ny = (r * xbase if xbase > 1 else 1), (r * ybase if ybase > 1 else 1)
    taus = torch.arange(nx, dtype=torch.float64) / nx
    fs = -0.5 + torch.arange(ny, dtype=torch.float64) / ny
    F, T = torch.meshgrid(fs, taus, indexing="ij")
    return T.reshape(-1), F.reshape(-1)


def explicit(phi, phi_true, truth, xbase, ybase, r, mistake=None):
    """(spectral, distribution, target), each the mean over the batch of the per-sample value; complex128 / float64 inputs."""
    if mistake == "axes":
        xbase, ybase = ybase, xbase
    sign = 1.0 if mistake == "tau_sign" else -1.0
    B, D = phi.shape
    A = atoms(*grid_points(xbase, ybase, r), xbase, ybase, sign)
    norm = (lambda S: S.max()) if mistake == "max" else (lambda S: S.mean())
    zero = phi.new_zeros((), dtype=torch.float64)
    spec, dist, targ = [], [], []
    for b in range(B):
        dead = not phi[b].detach().abs().any() or (phi_true is not None and not phi_true[b].abs().any())
        if phi_true is None or dead:
            spec.append(zero)
            dist.append(zero)
        else:
            z, zt = phi[b].conj() @ A, phi_true[b].conj() @ A
            S, St = z.real ** 2 + z.imag ** 2, zt.real ** 2 + zt.imag ** 2
            spec.append(((S / norm(S) - St / norm(St)) ** 2).mean())
            live = S.detach() > 0                                     # d|z| / dz is taken as 0 at z = 0
            h = (torch.sqrt(S[live]) * torch.sqrt(St[live])).sum()
            dist.append(1 - h / torch.sqrt(S.sum() * St.sum()))
        L = 0 if truth is None else int(truth["L_true"][b].clamp(0, truth["tau_true"].shape[1]))
        if truth is None or dead or (L == 0 and mistake != "L0"):
            targ.append(zero)
        else:
            Al = atoms(truth["tau_true"][b, :L].double(), truth["f_true"][b, :L].double(), xbase, ybase, sign)
            zl = phi[b].conj() @ Al
            rho = (zl.real ** 2 + zl.imag ** 2) / (D * (phi[b].real ** 2 + phi[b].imag ** 2).sum())
            targ.append((1 - rho).sum() / L)                          # (the stand-in "L0" divides 0 by 0 here)
    return tuple(torch.stack(t).sum() / B for t in (spec, dist, targ))


def single_atom(xbase=5, ybase=3, tau=0.37, f=-0.21):
    """phi = a(tau, f) on the xbase x ybase grid, and the truth that names it."""
    phi = atoms(torch.tensor([tau], dtype=torch.float64), torch.tensor([f], dtype=torch.float64), xbase, ybase).reshape(1, -1)
    truth = {"tau_true": torch.tensor([[tau]], dtype=torch.float64), "f_true": torch.tensor([[f]], dtype=torch.float64),
             "L_true": torch.tensor([1])}
    return phi, truth
