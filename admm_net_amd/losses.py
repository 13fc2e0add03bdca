"""The reference's training losses (loss.py: ``BasicANMLoss``, ``PhiAlignmentLoss``, ``basic_parameter_loss``) with one forward
and one hand-written backward kernel each (csrc/loss.hip), in place of a Python loop over the samples of the batch.

Definitions, with B signals, Lmax target slots, L = L_true[b]:

    BasicANMLoss      loss_b = sum_j conf_j^2                                                            if L = 0
                      loss_b = mean_{j<L} (tau_j - tau_true_j)^2 + mean_{j<L} (f_j - f_true_j)^2
                               + 0.1 mean_{j<L} (conf_j - 1)^2                                           if L >= 1
                      param = mean_b loss_b,  reg = lambda_reg mean_b ||phi_b||_2,  total = param + reg
    PhiAlignmentLoss  amplitude = mean (|phi| - |phi_true|)^2,  phase = mean wrap(arg phi - arg phi_true)^2,
                      wrap(d) = ((d + pi) mod 2 pi) - pi (Python's %, so +pi maps to -pi),
                      total = amplitude_weight amplitude + phase_weight phase
    PhiSpectralLoss   PhiAlignmentLoss plus three terms on the delay-Doppler spectrum |phi^H a(tau, f)|^2 (csrc/loss_spectrum.hip):
                      the spectral and distribution terms whose weights the reference declares and never uses, and a term on
                      the scene's true targets; the definitions are in the class's docstring

Two sets of kernels evaluate them (in the manner of ``training.SmallKernels`` / ``TorchSmallKernels``): ``HipLossKernels`` (the
device entry points of ``ops``) and ``TensorLossKernels``, the same formulas as masked [B, Lmax] tensor operations without a
per-sample loop or a device-to-host read -- any device, any float dtype; the CPU tests' stand-in and, in float64, the yardstick
of the GPU tests.  The modules pick one by their ``route`` attribute ("hip", the default, or "tensor").

What differs from the reference's classes:
  * an ``L_true`` outside [0, Lmax] raises ``ValueError`` after ONE device-to-host read per call (``check_status = True``; the
    reference reads every sample's L).  ``check_status = False`` skips the read; such a sample is then evaluated with L held
    to [0, Lmax];
  * the targets are constants: one that requires grad raises ``ValueError`` (the kernels return no such gradient).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .set_ops import set_options

ROUTES = ("hip", "tensor")


class HipLossKernels:
    """The losses and their backwards on the HIP kernels of csrc/loss.hip, in the order of the comments below."""

    anm = staticmethod(ops.loss_anm)           # (tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg) -> out [3], norms, status
    anm_bwd = staticmethod(ops.loss_anm_bwd)   # (g_out, tau, ..., phi, norms, lambda_reg) -> g_tau, g_f, g_conf, g_phi
    phi = staticmethod(ops.loss_phi)           # (phi, phi_true, amplitude_weight, phase_weight) -> out [3]
    phi_bwd = staticmethod(ops.loss_phi_bwd)   # (g_out, phi, phi_true, amplitude_weight, phase_weight) -> g_phi
    # csrc/loss_spectrum.hip: (phi, phi_true, truth, xbase, ybase, weights, oversample) -> out [4], workspace, status [3]
    spectrum = staticmethod(ops.loss_spectrum)
    spectrum_bwd = staticmethod(ops.loss_spectrum_bwd)   # (g_out, phi, truth, ..., oversample, workspace, skip) -> g_phi
    # csrc/loss_set.hip: (tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg, w_conf, scale, period)
    #   -> out [4], assign [B, Lmax], norms, status [2], rows [B, 6]
    set = staticmethod(ops.loss_set)
    set_bwd = staticmethod(ops.loss_set_bwd)   # (g_out, tau, ..., phi, assign, norms, lambda_reg, ...) -> g_tau, g_f, g_conf, g_phi


class TensorLossKernels:
    """The same forward / backward formulas as tensor operations, any device, in the dtype they are given."""

    @staticmethod
    def wrap(d):
        return torch.remainder(d + math.pi, 2 * math.pi) - math.pi

    @staticmethod
    def _anm_parts(tau, L_true):
        """(L held to [0, Lmax] as [B, 1], the mask j < L, the count of L_true outside the range)."""
        Lmax = tau.shape[1]
        L = L_true.clamp(0, Lmax).reshape(-1, 1)
        mask = (torch.arange(Lmax, device=tau.device) < L).to(tau.dtype)
        outside = ((L_true < 0) | (L_true > Lmax)).sum().to(torch.int32).reshape(1)
        return L, mask, outside

    @staticmethod
    def anm_terms(tau, f, conf, tau_true, f_true, L_true, phi):
        """(loss_b [B], ||phi_b|| [B], status [1]): the per-signal terms of the two batch means, none of them negative."""
        L, mask, outside = TensorLossKernels._anm_parts(tau, L_true)
        sq = (tau - tau_true) ** 2 + (f - f_true) ** 2 + 0.1 * (conf - 1) ** 2
        found = (sq * mask).sum(dim=1) / L.clamp(min=1).reshape(-1)
        loss_b = torch.where(L.reshape(-1) == 0, (conf ** 2).sum(dim=1), found)
        return loss_b, torch.sqrt((phi.real ** 2 + phi.imag ** 2).sum(dim=1)), outside

    @staticmethod
    def anm(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg):
        loss_b, norms, outside = TensorLossKernels.anm_terms(tau, f, conf, tau_true, f_true, L_true, phi)
        param, reg = loss_b.mean(), lambda_reg * norms.mean()
        return torch.stack([param + reg, param, reg]), norms, outside

    @staticmethod
    def anm_bwd(g_out, tau, f, conf, tau_true, f_true, L_true, phi, norms, lambda_reg):
        B = tau.shape[0]
        L, mask, _ = TensorLossKernels._anm_parts(tau, L_true)
        cp, cr = g_out[0] + g_out[1], g_out[0] + g_out[2]
        s = mask * (2 * cp / (L.clamp(min=1) * B))
        g_conf = torch.where(L == 0, 2 * cp / B * conf, s * (0.1 * (conf - 1)))
        live = (norms > 0).reshape(-1, 1)
        unit = phi / torch.where(live, norms.reshape(-1, 1), torch.ones_like(norms).reshape(-1, 1))
        g_phi = torch.where(live, (cr * lambda_reg / B) * unit, torch.zeros_like(phi))
        return s * (tau - tau_true), s * (f - f_true), g_conf, g_phi

    @staticmethod
    def phi_terms(phi, phi_true):
        """((|phi| - |phi_true|)^2, wrap(arg phi - arg phi_true)^2), both [B, D]: the terms of the two means."""
        w = TensorLossKernels.wrap(torch.angle(phi) - torch.angle(phi_true))
        return (phi.abs() - phi_true.abs()) ** 2, w ** 2

    @staticmethod
    def phi(phi, phi_true, amplitude_weight, phase_weight):
        a, p = TensorLossKernels.phi_terms(phi, phi_true)
        amp, ph = a.mean(), p.mean()
        return torch.stack([amplitude_weight * amp + phase_weight * ph, amp, ph])

    @staticmethod
    def phi_bwd(g_out, phi, phi_true, amplitude_weight, phase_weight):
        r = phi.abs()
        live = r > 0
        rs = torch.where(live, r, torch.ones_like(r))
        unit = phi / rs
        w = TensorLossKernels.wrap(torch.angle(phi) - torch.angle(phi_true))
        ca = (g_out[0] * amplitude_weight + g_out[1]) * (2.0 / phi.numel())
        cp = (g_out[0] * phase_weight + g_out[2]) * (2.0 / phi.numel())
        g = (ca * (r - phi_true.abs())) * unit + (cp * w / rs) * (1j * unit)      # i (x + i y) = -y + i x
        return torch.where(live, g, torch.zeros_like(phi))

    # ---- the terms on the delay-Doppler spectrum (PhiSpectralLoss; csrc/loss_spectrum.hip) --------------------------------------
    @staticmethod
    def spectrum_tables(xbase, ybase, oversample, device, cdtype):
        """(Sm [ny, ybase] = s_q[ks], Dm [nx, xbase] = conj(d_p[kd])) of the uniform full-period grid taus_p = p / nx,
        fs_q = -0.5 + q / ny, so that the atom of grid point (q, p) is Sm[q, ks] Dm[p, kd]; evaluated in float64 from the
        argument reduced to a fraction of a turn, then cast."""
        def table(points, base, sign):
            t = points.reshape(-1, 1) * torch.arange(base, dtype=torch.float64, device=device)
            return torch.polar(torch.ones_like(t), sign * 2 * math.pi * (t - torch.round(t))).to(cdtype)
        nx, ny = (oversample * xbase if xbase > 1 else 1), (oversample * ybase if ybase > 1 else 1)
        taus = torch.arange(nx, dtype=torch.float64, device=device) / nx
        fs = -0.5 + torch.arange(ny, dtype=torch.float64, device=device) / ny
        return table(fs, ybase, 1.0), table(taus, xbase, -1.0)

    @staticmethod
    def _spectrum_parts(phi, phi_true, truth, xbase, ybase, oversample, grid=True):
        """Everything the forward and the backward share, as a dict; rows that contribute nothing (``live`` false) are
        evaluated with their divisors set to 1 and masked afterwards.  ``grid = False`` (a backward that leaves both grid terms
        out) skips the contraction over the grid and nothing else: ``live`` is the forward's, zero phi_true rows included."""
        B, D = phi.shape
        if D != xbase * ybase:
            raise ValueError(f"phi must be [B, {xbase * ybase}] for a {xbase} x {ybase} grid, got {tuple(phi.shape)}")
        rdt, dev = phi.real.dtype, phi.device
        P = phi.reshape(B, ybase, xbase)
        n2 = (phi.real ** 2 + phi.imag ** 2).sum(dim=1)
        zero = n2 == 0
        zero_true = torch.zeros_like(zero)
        p = {"P": P, "n2s": torch.where(zero, torch.ones_like(n2), n2), "zero": zero}
        zeros = torch.zeros_like(n2)
        p["spec"] = p["dist"] = p["targ"] = zeros
        if phi_true is not None:
            T = phi_true.to(phi.dtype).reshape(B, ybase, xbase)
            zero_true = (T.real ** 2 + T.imag ** 2).sum(dim=(1, 2)) == 0
        live = ~zero & ~zero_true
        p["live"], p["zero_true"] = live, zero_true
        if phi_true is not None and grid:
            Sm, Dm = TensorLossKernels.spectrum_tables(xbase, ybase, oversample, dev, phi.dtype)
            z = torch.einsum("bsd,qs,pd->bqp", P.conj(), Sm, Dm)
            zt = torch.einsum("bsd,qs,pd->bqp", T.conj(), Sm, Dm)
            S, St = z.real ** 2 + z.imag ** 2, zt.real ** 2 + zt.imag ** 2
            G = S.shape[1] * S.shape[2]
            one = torch.ones_like(n2)
            A, At = torch.where(live, S.sum(dim=(1, 2)), one), torch.where(live, St.sum(dim=(1, 2)), one)
            m, mt = (A / G).reshape(B, 1, 1), (At / G).reshape(B, 1, 1)
            u, v = S / m, St / mt
            H = (z.abs() * zt.abs()).sum(dim=(1, 2))
            p.update(Sm=Sm, Dm=Dm, z=z, S=S, St=St, G=G, A=A, At=At, m=m, u=u, v=v, H=H)
            p["spec"] = torch.where(live, ((u - v) ** 2).mean(dim=(1, 2)), zeros)
            p["dist"] = torch.where(live, 1 - H / torch.sqrt(A * At), zeros)
        outside = torch.zeros((), dtype=torch.int64, device=dev)
        if truth is not None:
            tau, f, L_true = truth
            Lmax = tau.shape[1]
            L = L_true.clamp(0, Lmax).reshape(B, 1)
            mask = (torch.arange(Lmax, device=dev) < L).to(rdt)
            turn = lambda t: torch.polar(torch.ones_like(t), 2 * math.pi * (t - torch.round(t))).to(phi.dtype)
            ef = turn(f.to(rdt).unsqueeze(-1) * torch.arange(ybase, dtype=rdt, device=dev))        # [B, Lmax, ybase]
            et = turn(-(tau.to(rdt).unsqueeze(-1) * torch.arange(xbase, dtype=rdt, device=dev)))   # [B, Lmax, xbase]
            zl = torch.einsum("bsd,bls,bld->bl", P.conj(), ef, et)
            rho = (zl.real ** 2 + zl.imag ** 2) / (D * p["n2s"]).reshape(B, 1)
            use = (live & (L.reshape(-1) > 0)).reshape(B, 1)
            p.update(ef=ef, et=et, zl=zl, rho=rho, Lc=L.clamp(min=1).to(rdt), mask=mask * use.to(rdt))
            p["targ"] = ((1 - rho) * p["mask"]).sum(dim=1) / p["Lc"].reshape(-1)
            outside = ((L_true < 0) | (L_true > Lmax)).sum()
        p["status"] = torch.stack([outside, zero.sum(), zero_true.sum()]).to(torch.int32)
        return p

    @staticmethod
    def spectrum(phi, phi_true, truth, xbase, ybase, weights, oversample):
        """(out [4] = (total, spectral, distribution, target), what ``spectrum_bwd`` needs beside its arguments (here phi_true),
        status [3] = (L_true outside [0, Lmax], zero phi rows, zero phi_true rows)).  ``truth``: None or (tau_true, f_true
        [B, Lmax], L_true [B]); ``phi_true``: None for the target term alone; ``weights``: (spectral, distribution, target)."""
        p = TensorLossKernels._spectrum_parts(phi, phi_true, truth, xbase, ybase, oversample)
        spec, dist, targ = p["spec"].mean(), p["dist"].mean(), p["targ"].mean()
        return torch.stack([weights[0] * spec + weights[1] * dist + weights[2] * targ, spec, dist, targ]), phi_true, p["status"]

    @staticmethod
    def spectrum_bwd(g_out, phi, truth, xbase, ybase, weights, oversample, saved, skip=0):
        """g_phi from g_out [4]; ``skip``: bit 0 the spectral, bit 1 the distribution, bit 2 the target term is left out."""
        phi_true = saved
        B, D = phi.shape
        grid = phi_true is not None and (skip & 3) != 3
        if skip & 4:
            truth = None
        p = TensorLossKernels._spectrum_parts(phi, phi_true, truth, xbase, ybase, oversample, grid)
        g_out = g_out.to(phi.real.dtype)
        cs, cd, ct = ((0.0 if skip & (1 << i) else (g_out[0] * weights[i] + g_out[i + 1]) / B) for i in range(3))
        g = torch.zeros_like(p["P"])
        if grid:
            S, St, u, v, m, A, At, G = (p[k] for k in ("S", "St", "u", "v", "m", "A", "At", "G"))
            E = ((u - v) * u).mean(dim=(1, 2), keepdim=True)
            c = cs * 2 / (G * m) * ((u - v) - E)
            some = S > 0                                               # d|z| / dz is taken as 0 at z = 0
            ratio = torch.sqrt(St / torch.where(some, S, torch.ones_like(S)))
            c = c - torch.where(some, cd / (2 * torch.sqrt(A * At)).reshape(B, 1, 1) * (ratio - (p["H"] / A).reshape(B, 1, 1)),
                                torch.zeros_like(S))
            g = g + 2 * torch.einsum("bqp,qs,pd->bsd", c * p["z"].conj(), p["Sm"], p["Dm"])
        if truth is not None:
            coef = -2 * ct / p["Lc"] * p["mask"]                       # [B, Lmax]
            dn = (D * p["n2s"]).reshape(B, 1)
            g = g + torch.einsum("bl,bls,bld->bsd", (coef * p["zl"].conj() / dn).to(phi.dtype), p["ef"], p["et"])
            g = g - ((coef * p["rho"]).sum(dim=1) / p["n2s"]).reshape(B, 1, 1) * p["P"]
        return torch.where(p["live"].reshape(B, 1), g.reshape(B, D), torch.zeros_like(phi))

    # ---- the assignment loss of the head (SetANMLoss; csrc/loss_set.hip) --------------------------------------------------------
    @staticmethod
    def period_wrap(d, P):
        """d into [-P / 2, P / 2) for a period P > 0; P = 0: d itself (sc_wrap of csrc/score_core.h)."""
        return d - P * torch.floor(d / P + 0.5) if P > 0 else d

    @staticmethod
    def set_dead(tau, f, conf, tau_true, f_true, L_true):
        """(n = L_true held to [0, Lt] [B], the signals with a non-finite value among tau, f, conf or their first n truths [B])."""
        Lt = tau_true.shape[1]
        n = L_true.clamp(0, Lt)
        first = torch.arange(Lt, device=tau.device) < n.reshape(-1, 1)
        dead = ~(torch.isfinite(tau) & torch.isfinite(f) & torch.isfinite(conf)).all(dim=1)
        return n, dead | (~(torch.isfinite(tau_true) & torch.isfinite(f_true)) & first).any(dim=1)

    @staticmethod
    def set_assign(tau, f, conf, tau_true, f_true, L_true, w_conf, scale, period):
        """assign [B, Lmax] int32 from ``set_assign_host``: ONE HOST LOOP OVER THE SIGNALS of the batch, after a device-to-host
        copy of the six inputs.  This is the float64 yardstick and the CPU stand-in, not a fast path."""
        n, dead = TensorLossKernels.set_dead(tau, f, conf, tau_true, f_true, L_true)
        host = [t.detach().cpu().to(torch.float64).numpy() for t in (tau, f, conf, tau_true, f_true)]
        n_host, dead_host = n.cpu().numpy(), dead.cpu().numpy()
        assign = np.full(tuple(tau.shape), -1, dtype=np.int32)
        for b in range(tau.shape[0]):                       # the per-signal host loop
            if not dead_host[b]:
                assign[b] = set_assign_host(*(h[b] for h in host), int(n_host[b]), w_conf=w_conf, scale=scale, period=period)[0]
        return torch.from_numpy(assign).to(tau.device)

    @staticmethod
    def _set_parts(tau, f, conf, tau_true, f_true, L_true, assign, scale, period):
        """(n [B], dead [B], matched [B, Lmax], wrapped dtau and df (0 off the matched slots), t = 1 on a matched slot)."""
        sx, sy, pt, pf, _, _ = set_options(scale, period)
        n, dead = TensorLossKernels.set_dead(tau, f, conf, tau_true, f_true, L_true)
        matched = (assign >= 0) & ~dead.reshape(-1, 1)
        at = assign.clamp(min=0).to(torch.int64)
        zero = torch.zeros_like(tau)
        dt = torch.where(matched, TensorLossKernels.period_wrap(tau - tau_true.gather(1, at).to(tau.dtype), pt), zero)
        df = torch.where(matched, TensorLossKernels.period_wrap(f - f_true.gather(1, at).to(f.dtype), pf), zero)
        return n, dead, matched, dt, df, matched.to(tau.dtype)

    @staticmethod
    def set(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg=0.0, w_conf=0.1, scale=(1.0, 1.0), period=None):
        """(out [4] = (total, match, conf, reg), assign [B, Lmax] int32, norms [B], status [2] int32, rows [B, 6] = each signal's
        loss_b, match_b, conf_b, ||phi_b|| as it enters reg, and its two status flags): ``ops.loss_set``'s returns."""
        sx, sy, _, _, w_conf, lambda_reg = set_options(scale, period, w_conf, lambda_reg)
        Lmax, Lt = tau.shape[1], tau_true.shape[1]
        assign = TensorLossKernels.set_assign(tau, f, conf, tau_true, f_true, L_true, w_conf, scale, period)
        n, dead, matched, dt, df, t = TensorLossKernels._set_parts(tau, f, conf, tau_true, f_true, L_true, assign, scale, period)
        zero = torch.zeros_like(tau)
        match_b = ((sx * dt) ** 2 + (sy * df) ** 2).sum(dim=1) / n.clamp(min=1)
        conf_b = torch.where(dead.reshape(-1, 1), zero, (conf - t) ** 2).sum(dim=1) / Lmax
        norms = torch.sqrt((phi.real ** 2 + phi.imag ** 2).sum(dim=1))
        counted = torch.where(dead, torch.zeros_like(norms), norms)
        outside = (L_true < 0) | (L_true > Lt)
        match, cf, reg = match_b.mean(), conf_b.mean(), lambda_reg * counted.mean()
        rows = torch.stack([match_b + w_conf * conf_b, match_b, conf_b, counted, outside.to(tau.dtype), dead.to(tau.dtype)], dim=1)
        status = torch.stack([outside.sum(), dead.sum()]).to(torch.int32)
        return torch.stack([match + w_conf * cf + reg, match, cf, reg]), assign, norms, status, rows

    @staticmethod
    def set_bwd(g_out, tau, f, conf, tau_true, f_true, L_true, phi, assign, norms, lambda_reg=0.0, w_conf=0.1, scale=(1.0, 1.0),
                period=None):
        sx, sy, _, _, w_conf, lambda_reg = set_options(scale, period, w_conf, lambda_reg)
        B, Lmax = tau.shape
        n, dead, matched, dt, df, t = TensorLossKernels._set_parts(tau, f, conf, tau_true, f_true, L_true, assign, scale, period)
        g_out = g_out.to(tau.dtype)
        cm, cc, cr = g_out[0] + g_out[1], g_out[0] * w_conf + g_out[2], g_out[0] + g_out[3]
        s = cm * 2 / (n.clamp(min=1).reshape(-1, 1) * B)
        g_conf = torch.where(dead.reshape(-1, 1), torch.zeros_like(conf), cc * 2 * (conf - t) / (Lmax * B))
        live = ((norms > 0) & ~dead).reshape(-1, 1)
        unit = phi / torch.where(live, norms.reshape(-1, 1), torch.ones_like(norms).reshape(-1, 1))
        g_phi = torch.where(live, (cr * lambda_reg / B) * unit, torch.zeros_like(phi))
        return s * (sx * sx) * dt, s * (sy * sy) * df, g_conf, g_phi


def set_assign_host(tau, f, conf, tau_true, f_true, n=None, *, w_conf=0.1, scale=(1.0, 1.0), period=None, with_gap=False):
    """The assignment of ``SetANMLoss`` for ONE signal in float64 numpy: slots (tau, f, conf, 1-d, all live) against the first ``n``
    of the targets (1-d; None: all of them; held to [0, Lt]).  Enumerates every assignment where min(Lmax, n) <=
    ``metrics.BRUTE_MIN`` and there are at most ``metrics.BRUTE_ASSIGNMENTS`` of them, and calls
    ``scipy.optimize.linear_sum_assignment`` on c_ij = d2_ij / n + (w_conf / Lmax)(1 - 2 conf_i) above that, as
    ``metrics.match_host`` does.

    Returns (assign [Lmax] int32 = the target of slot i or -1, loss_b from the definition at that assignment); with
    ``with_gap=True`` also the distance to the best value with ANOTHER assignment relative to loss_b (inf if there is none): by
    enumeration, else by excluding each matched pair in turn and solving again."""
    from . import metrics
    sx, sy, pt, pf, w_conf, _ = set_options(scale, period, w_conf)
    ts, fs, cs = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tau, f, conf))
    tt, ft = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (tau_true, f_true))
    if not (ts.shape == fs.shape == cs.shape and tt.shape == ft.shape and len(ts) >= 1):
        raise ValueError("tau, f and conf must have one length >= 1, tau_true and f_true one length")
    Lmax = len(ts)
    n = len(tt) if n is None else min(max(int(n), 0), len(tt))
    tt, ft = tt[:n], ft[:n]
    if not all(np.isfinite(v).all() for v in (ts, fs, cs, tt, ft)):
        raise ValueError("a slot or a target is not finite")
    wl = w_conf / Lmax
    assign = np.full(Lmax, -1, dtype=np.int32)
    gap_abs, d2 = math.inf, np.zeros((Lmax, 0))
    if n > 0:
        _, _, d2 = metrics.pair_terms(ts, fs, tt, ft, (sx, sy), (pt, pf))
        cost = d2 / n + (wl * (1.0 - 2.0 * cs)).reshape(-1, 1)
        k, m = min(Lmax, n), max(Lmax, n)
        by_rows = cost if Lmax <= n else cost.T                      # rows = the smaller side (on a tie the slots)
        r = np.arange(k)
        if k <= metrics.BRUTE_MIN and math.perm(m, k) <= metrics.BRUTE_ASSIGNMENTS:
            P = metrics._arrangements(m, k)
            total = by_rows[r, P].sum(axis=1)
            best = int(np.argmin(total))
            cols = P[best]
            if with_gap and len(total) > 1:
                gap_abs = float(np.delete(total, best).min() - total[best])
        else:
            from scipy.optimize import linear_sum_assignment
            r, cols = linear_sum_assignment(by_rows)
            if with_gap and m > 1:
                least = by_rows[r, cols].sum()
                for i, j in zip(r, cols):
                    other = by_rows.copy()
                    other[i, j] = np.inf
                    try:
                        ro, co = linear_sum_assignment(other)
                    except ValueError:                              # no assignment without this pair
                        continue
                    gap_abs = min(gap_abs, float(other[ro, co].sum() - least))
        if Lmax <= n:
            assign[r] = cols
        else:
            assign[cols] = r
    matched = assign >= 0
    at = assign[matched]
    value = float(d2[matched, at].sum() / max(n, 1) + w_conf * ((cs - matched) ** 2).sum() / Lmax)
    if not with_gap:
        return assign, value
    return assign, value, (gap_abs / value if value > 0 else math.inf)


def _kernels(route):
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")
    return HipLossKernels if route == "hip" else TensorLossKernels


def _constant(**targets):
    for name, t in targets.items():
        if t.requires_grad:
            raise ValueError(f"{name} requires grad: the losses treat their targets as constants and return no gradient for them")


def _g_out(grads, like):
    return torch.stack([g.to(like.dtype) for g in grads])


class _ANMLossFn(torch.autograd.Function):
    """(total, param, reg, status) of BasicANMLoss; gradients arriving through any of the first three are honoured."""

    @staticmethod
    def forward(ctx, tau, f, conf, phi, tau_true, f_true, L_true, lambda_reg, lk):
        out, norms, status = lk.anm(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg)
        ctx.save_for_backward(tau, f, conf, phi, tau_true, f_true, L_true, norms)
        ctx.lambda_reg, ctx.lk = lambda_reg, lk
        ctx.mark_non_differentiable(status)
        return (*out.unbind(0), status)

    @staticmethod
    def backward(ctx, g_total, g_param, g_reg, _g_status):
        tau, f, conf, phi, tau_true, f_true, L_true, norms = ctx.saved_tensors
        g = ctx.lk.anm_bwd(_g_out((g_total, g_param, g_reg), norms), tau, f, conf, tau_true, f_true, L_true, phi, norms,
                           ctx.lambda_reg)
        g_tau, g_f, g_conf, g_phi = (x.to(t.dtype) for x, t in zip(g, (tau, f, conf, phi)))
        return g_tau, g_f, g_conf, g_phi, None, None, None, None, None


class _PhiLossFn(torch.autograd.Function):
    """(total, amplitude, phase) of PhiAlignmentLoss."""

    @staticmethod
    def forward(ctx, phi, phi_true, amplitude_weight, phase_weight, lk):
        ctx.save_for_backward(phi, phi_true)
        ctx.weights, ctx.lk = (amplitude_weight, phase_weight), lk
        return tuple(lk.phi(phi, phi_true, amplitude_weight, phase_weight).unbind(0))

    @staticmethod
    def backward(ctx, g_total, g_amp, g_phase):
        phi, phi_true = ctx.saved_tensors
        g_phi = ctx.lk.phi_bwd(_g_out((g_total, g_amp, g_phase), g_total), phi, phi_true, *ctx.weights)
        return g_phi.to(phi.dtype), None, None, None, None


def _anm_loss(tau, f, conf, phi, tau_true, f_true, L_true, lambda_reg, route, check_status):
    _constant(tau_true=tau_true, f_true=f_true)
    total, param, reg, status = _ANMLossFn.apply(tau, f, conf, phi, tau_true, f_true, L_true, float(lambda_reg), _kernels(route))
    if check_status:
        bad = int(status.item())                       # the call's one device-to-host read
        if bad:
            raise ValueError(f"L_true of {bad} sample(s) lies outside [0, {tau.shape[1]}]")
    return total, param, reg


def basic_parameter_loss(tau_pred, f_pred, tau_true, f_true, confidences, L_true):
    """The ``param_loss`` of ``BasicANMLoss`` on its own (loss.py:6-30).  ``basic_parameter_loss.route`` and
    ``basic_parameter_loss.check_status`` select the kernels and the range check, as the modules' attributes do."""
    phi = torch.zeros(tau_pred.shape[0], 1, dtype=torch.complex128 if tau_pred.dtype == torch.float64 else torch.complex64,
                      device=tau_pred.device)
    return _anm_loss(tau_pred, f_pred, confidences, phi, tau_true, f_true, L_true, 0.0, basic_parameter_loss.route,
                     basic_parameter_loss.check_status)[1]


basic_parameter_loss.route = "hip"
basic_parameter_loss.check_status = True


class BasicANMLoss(nn.Module):
    def __init__(self, lambda_reg=1e-4):
        super().__init__()
        self.lambda_reg = lambda_reg
        self.route = "hip"
        self.check_status = True

    def forward(self, model_outputs, ground_truth):
        total, param, reg = _anm_loss(model_outputs['tau_est'], model_outputs['f_est'], model_outputs['confidences'],
                                      model_outputs['phi_final'], ground_truth['tau_true'], ground_truth['f_true'],
                                      ground_truth['L_true'], self.lambda_reg, self.route, self.check_status)
        return total, {'total_loss': total, 'param_loss': param, 'reg_loss': reg}


class _SetLossFn(torch.autograd.Function):
    """(total, match, conf, reg, status, assign) of SetANMLoss; gradients arriving through any of the first four are honoured."""

    @staticmethod
    def forward(ctx, tau, f, conf, phi, tau_true, f_true, L_true, opts, lk):
        out, assign, norms, status, _ = lk.set(tau, f, conf, tau_true, f_true, L_true, phi, *opts)
        ctx.save_for_backward(tau, f, conf, phi, tau_true, f_true, L_true, assign, norms)
        ctx.opts, ctx.lk = opts, lk
        ctx.mark_non_differentiable(status, assign)
        return (*out.unbind(0), status, assign)

    @staticmethod
    def backward(ctx, g_total, g_match, g_conf, g_reg, _g_status, _g_assign):
        tau, f, conf, phi, tau_true, f_true, L_true, assign, norms = ctx.saved_tensors
        g = ctx.lk.set_bwd(_g_out((g_total, g_match, g_conf, g_reg), norms), tau, f, conf, tau_true, f_true, L_true, phi, assign,
                           norms, *ctx.opts)
        g_tau, g_f, g_c, g_phi = (x.to(t.dtype) for x, t in zip(g, (tau, f, conf, phi)))
        return g_tau, g_f, g_c, g_phi, None, None, None, None, None


class SetANMLoss(nn.Module):
    """A permutation-invariant loss for the head of ``ADMMNet`` (csrc/loss_set.hip): ``BasicANMLoss`` compares slot j with truth j,
    but the truths of a scene come in draw order, so slot j has no meaning.  Here the Lmax slots of a signal are matched to its
    n = L_true targets (``tau_true``, ``f_true`` [B, Lt], any Lt <= 64) by the assignment sigma that minimises the loss itself:

        match_b = (1 / max(n, 1)) sum over matched (i, j) of (sx wrap(tau_i - tau_true_j))^2 + (sy wrap(f_i - f_true_j))^2
        conf_b  = (1 / Lmax) sum_i (conf_i - t_i)^2,    t_i = 1 on a matched slot and 0 elsewhere
        loss_b  = min_sigma [match_b + w_conf conf_b],  total = mean_b loss_b + lambda_reg mean_b ||phi_b||_2

    so matched slots learn tau, f and conf -> 1, unmatched ones conf -> 0, and ``conf`` comes to say how many targets there are
    (``ADMMNet.estimate_head``).  ``scale = (sx, sy)``; ``period``: None, or (P_tau, P_f) with 0 / None for an axis that does not
    wrap.  Takes ``BasicANMLoss``'s call and returns (total, dict) with ``total_loss``, ``match_loss``, ``conf_loss``,
    ``reg_loss``.  ``last_assign`` ([B, Lmax] int32, the target of each slot or -1) and ``last_status`` (int32 [2]: L_true
    outside [0, Lt]; signals with a non-finite value, which add nothing and get no gradient) are those of the last call, on the
    device; ``check_status = True`` reads the status once per call and raises ``ValueError`` on either word."""

    def __init__(self, lambda_reg=1e-4, w_conf=0.1, scale=(1.0, 1.0), period=None):
        super().__init__()
        set_options(scale, period, w_conf, lambda_reg)
        self.lambda_reg, self.w_conf, self.scale, self.period = lambda_reg, w_conf, tuple(scale), period
        self.route = "hip"
        self.check_status = True
        self.last_assign = self.last_status = None

    def forward(self, model_outputs, ground_truth):
        tau, f, conf, phi = (model_outputs[k] for k in ('tau_est', 'f_est', 'confidences', 'phi_final'))
        tau_true, f_true, L_true = (ground_truth[k] for k in ('tau_true', 'f_true', 'L_true'))
        _constant(tau_true=tau_true, f_true=f_true)
        opts = (float(self.lambda_reg), float(self.w_conf), tuple(float(v) for v in self.scale),
                None if self.period is None else tuple(self.period))
        total, match, cf, reg, status, assign = _SetLossFn.apply(tau, f, conf, phi, tau_true, f_true, L_true, opts,
                                                                 _kernels(self.route))
        self.last_assign, self.last_status = assign, status
        if self.check_status:
            outside, nonfinite = status.tolist()            # the call's one device-to-host read
            if outside:
                raise ValueError(f"L_true of {outside} sample(s) lies outside [0, {tau_true.shape[1]}]")
            if nonfinite:
                raise ValueError(f"{nonfinite} sample(s) hold a non-finite tau, f, confidence or target")
        return total, {'total_loss': total, 'match_loss': match, 'conf_loss': cf, 'reg_loss': reg}


class PhiAlignmentLoss(nn.Module):
    def __init__(self, amplitude_weight=1.0, phase_weight=0.5, spectral_weight=0.2, distribution_weight=0.3):
        super().__init__()
        self.amplitude_weight = amplitude_weight
        self.phase_weight = phase_weight
        self.spectral_weight = spectral_weight              # (kept, unused, as in the reference)
        self.distribution_weight = distribution_weight
        self.route = "hip"

    def forward(self, phi_final, phi_true):
        _constant(phi_true=phi_true)
        if phi_final.shape != phi_true.shape or phi_final.dim() < 1:
            raise ValueError(f"phi_final and phi_true must have one shape, got {tuple(phi_final.shape)} and {tuple(phi_true.shape)}")
        if phi_final.dim() != 2:                            # a mean over all entries: any leading split into rows serves
            phi_final, phi_true = (t.reshape(t.shape[0], -1) for t in (phi_final, phi_true))
        total, amp, phase = _PhiLossFn.apply(phi_final, phi_true, float(self.amplitude_weight), float(self.phase_weight),
                                             _kernels(self.route))
        return total, {'total_loss': total, 'amplitude_loss': amp, 'phase_loss': phase}


SKIP_SPECTRAL, SKIP_DISTRIBUTION, SKIP_TARGET = 1, 2, 4     # ADMMNET_LOSS_SPECTRUM_SKIP_* of include/admmnet.h


class _PhiSpectralFn(torch.autograd.Function):
    """(total, spectral, distribution, target, status) of the spectrum terms of PhiSpectralLoss; gradients arriving through any
    of the first four are honoured.  A term is left out of the backward (a launch argument, no host read) when its weight is
    0 and autograd sent no gradient through its own output, or when the forward did not evaluate it."""

    @staticmethod
    def forward(ctx, phi, phi_true, tau_true, f_true, L_true, xbase, ybase, weights, oversample, lk):
        truth = None if L_true is None else (tau_true, f_true, L_true)
        out, saved, status = lk.spectrum(phi, phi_true, truth, xbase, ybase, weights, oversample)
        ctx.save_for_backward(phi, saved, tau_true, f_true, L_true)
        ctx.args, ctx.lk = (xbase, ybase, weights, oversample), lk
        ctx.absent = (SKIP_SPECTRAL | SKIP_DISTRIBUTION if phi_true is None else 0) | (SKIP_TARGET if L_true is None else 0)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(status)
        return (*out.unbind(0), status)

    @staticmethod
    def backward(ctx, g_total, *g_parts):
        phi, saved, tau_true, f_true, L_true = ctx.saved_tensors
        xbase, ybase, weights, oversample = ctx.args
        skip = ctx.absent
        for i, g in enumerate(g_parts[:3]):
            if g is None and (g_total is None or weights[i] == 0):
                skip |= 1 << i
        zero = torch.zeros((), dtype=phi.real.dtype, device=phi.device)
        g_out = _g_out([zero if g is None else g for g in (g_total, *g_parts[:3])], zero)
        truth = None if L_true is None else (tau_true, f_true, L_true)
        g_phi = ctx.lk.spectrum_bwd(g_out, phi, truth, xbase, ybase, weights, oversample, saved, skip)
        return (g_phi.to(phi.dtype),) + (None,) * 9


class PhiSpectralLoss(nn.Module):
    """``PhiAlignmentLoss`` plus the terms that are defined on the delay-Doppler spectrum S = |phi^H a(tau, f)|^2 -- the
    quantity ``peak_top``, ``estimate`` and ``select_refined`` read -- on the uniform full-period grid of
    ``oversample`` x (xbase, ybase) points (x = delay: ``xbase = Nd``, ``ybase = Nb`` for the generator's scenes):

        spectral      mean_b mean_grid (S / mean_grid S - S* / mean_grid S*)^2
        distribution  mean_b 1 - sum_grid |z| |z*| / sqrt(sum_grid S sum_grid S*)      (squared Hellinger distance, in [0, 1])
        target        mean_b mean_{l<L} (1 - |z(tau_true_l, f_true_l)|^2 / (D ||phi||^2)), 0 for L = 0

    with S*, z* those of ``phi_true``.  All three are unchanged by phi -> c e^{j theta} phi.  ``forward(phi_final, phi_true,
    truth)`` returns (total, dict); ``truth`` holds ``tau_true``, ``f_true`` [B, Lmax <= 16] and ``L_true`` [B].  With
    ``phi_true=None`` only the target term runs (the four label weights must be 0); with ``truth=None`` ``target_weight`` must
    be 0.  A signal whose phi row (or phi_true row) is all zero contributes 0 to the three terms and gets no gradient from them.
    The grid terms count as asked for whenever ``phi_true`` is given, whatever their weights: both are evaluated and reported,
    and a gradient may arrive through their dict entries; so a zero phi_true row is then dead for the target term too, in the
    forward and in the backward alike (pass ``phi_true=None`` for the target term on its own).
    The dict carries ``PhiAlignmentLoss``'s entries, ``spectral_loss``, ``distribution_loss``, ``target_loss`` and ``status``
    (device int32 [3]: L_true outside [0, Lmax], zero phi rows, zero phi_true rows); ``check_status = True`` reads it once per
    call and raises ``ValueError`` for the first count."""

    def __init__(self, xbase, ybase, amplitude_weight=1.0, phase_weight=0.5, spectral_weight=0.2, distribution_weight=0.3,
                 target_weight=0.0, oversample=2):
        super().__init__()
        if int(xbase) < 1 or int(ybase) < 1 or int(oversample) != oversample or not 1 <= oversample <= 4:
            raise ValueError(f"PhiSpectralLoss needs xbase, ybase >= 1 and an integer oversample in 1 .. 4, got {xbase}, {ybase}, {oversample}")
        self.xbase, self.ybase, self.oversample = int(xbase), int(ybase), int(oversample)
        self.amplitude_weight = amplitude_weight
        self.phase_weight = phase_weight
        self.spectral_weight = spectral_weight
        self.distribution_weight = distribution_weight
        self.target_weight = target_weight
        self.route = "hip"
        self.check_status = True

    def forward(self, phi_final, phi_true=None, truth=None):
        D = self.xbase * self.ybase
        if phi_final.dim() < 1 or phi_final.numel() == 0 or phi_final.numel() % D:
            raise ValueError(f"phi_final must hold rows of {D} entries, got {tuple(phi_final.shape)}")
        label_weights = (self.amplitude_weight, self.phase_weight, self.spectral_weight, self.distribution_weight)
        if phi_true is None and (truth is None or any(w != 0 for w in label_weights)):
            raise ValueError("without phi_true the loss is the target term alone: pass truth, and set amplitude_weight, phase_weight, "
                             "spectral_weight and distribution_weight to 0")
        if truth is None and self.target_weight != 0:
            raise ValueError("target_weight is not 0 but truth (tau_true, f_true, L_true) was not given")
        lk = _kernels(self.route)
        phi = phi_final.reshape(-1, D)
        if phi_true is not None:
            _constant(phi_true=phi_true)
            if phi_true.shape != phi_final.shape:
                raise ValueError(f"phi_final and phi_true must have one shape, got {tuple(phi_final.shape)} and {tuple(phi_true.shape)}")
            phi_true = phi_true.reshape(-1, D)
            label, amp, phase = _PhiLossFn.apply(phi, phi_true, float(self.amplitude_weight), float(self.phase_weight), lk)
        tau_true = f_true = L_true = None
        if truth is not None:
            tau_true, f_true, L_true = truth["tau_true"], truth["f_true"], truth["L_true"]
            _constant(tau_true=tau_true, f_true=f_true)
            if tau_true.dim() != 2 or tau_true.shape != f_true.shape or tau_true.shape[0] != phi.shape[0] or \
                    not 1 <= tau_true.shape[1] <= 16 or L_true.shape != (phi.shape[0],):
                raise ValueError(f"tau_true and f_true must be [{phi.shape[0]}, Lmax <= 16] and L_true [{phi.shape[0]}], got "
                                 f"{tuple(tau_true.shape)}, {tuple(f_true.shape)}, {tuple(L_true.shape)}")
        weights = (float(self.spectral_weight), float(self.distribution_weight), float(self.target_weight))
        total, spec, dist, targ, status = _PhiSpectralFn.apply(phi, phi_true, tau_true, f_true, L_true, self.xbase, self.ybase,
                                                               weights, self.oversample, lk)
        if phi_true is None:
            amp = phase = total.new_zeros(())
        else:
            total = label + total
        if self.check_status:
            bad = int(status[0].item())                    # the call's one device-to-host read
            if bad:
                raise ValueError(f"L_true of {bad} sample(s) lies outside [0, {tau_true.shape[1]}]")
        return total, {'total_loss': total, 'amplitude_loss': amp, 'phase_loss': phase, 'spectral_loss': spec,
                       'distribution_loss': dist, 'target_loss': targ, 'status': status}
