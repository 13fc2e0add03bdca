"""Differentiable forward of the unrolled network for the reference's training scripts
(``trainPhi.py`` / ``train.py``).

The inference path (``modules._FusedBase._run``) keeps nothing a backward pass could use, so training
takes this route instead: the layers are evaluated as differentiable tensor operations on the GPU and
the Hermitian eigendecomposition -- the dominant cost of every layer (admm_net.py:303) -- runs on the
HIP eigensolver behind ``admmnet_eigh_c64`` with the gradient the reference defines for it: the
eigenvectors are detached (admm_net.py:306), so only the eigenvalues carry gradient,
``dL/dA = V diag(dL/dw) V^H``.  The two n^3 contractions around it -- the rebuild ``G = V f(L) V^H`` of
admm_net.py:336-354 (forward, and its adjoint ``Re(v_c^H S v_c)`` in the backward) and that ``V diag(gw) V^H`` -- run on
the library's matrix-core kernels too (``admmnet_vdvh_c64`` / ``admmnet_vhsv_f32``, csrc/vdvh.hip), not on framework
GEMMs; the remaining layer steps are O(n^2) tensor operations.

``fused=True`` (``model.train_route = "fused"``) replaces the n^2-sized tensor operations of a layer -- the block matrices, the
symmetrisation, the residual, its norm, the dual update, the border-column / diagonal reads of the phi and H layers, and
everything autograd records for them -- by autograd functions with hand-written backwards over the streaming kernels of
csrc/train_layer.hip (``LayerKernels``;
``TorchLayerKernels`` is the same arithmetic as tensor operations, for the CPU tests).  The O(n)- and O(B)-sized parts (phi
layer, H layer, eigenvalue map, step network, group mean, head) are the same tensor operations on both routes.

``small=True`` on top of ``fused=True`` (``model.train_route = "full"``) also replaces those O(B D)-sized parts -- the phi layer,
the H layer around its ``correction_net``, the eigenvalue map and the step-size network with its group mean -- by autograd
functions over one forward and one backward kernel each (csrc/train_small.hip, ``SmallKernels``; ``TorchSmallKernels`` for the
CPU tests).  Those kernels read the raw parameters and return raw-parameter gradients.  ``correction_net``, the head, and the
``1 / (softplus(rho) + eps)`` factor of the G layer stay framework operations.  On this route the two detached corner values of
every layer are resolved with ONE device-to-host read per forward, and the detached rho feature never leaves the device.

Gradient flow mirrors the reference as written:
  * the corner values ``1 / (softplus(lambda)^2 + eps)`` go through ``.item()`` (admm_net.py:271, 426):
    ``gLayers.k.lambda_param`` / ``zLayers.k.lambda_param`` receive no gradient;
  * the ``rho`` FEATURE of the step network is a detached number (admm_net.py:458), the multiplying
    ``rho_base`` is not (admm_net.py:469);
  * the residual norm is divided by the mean over the batch the call sees (admm_net.py:459), or with ``sub_batch = g``
    over each group of g consecutive signals: the gradients are then the sum of the per-group graphs' gradients, i.e.
    gradient accumulation over those batches;
  * H, G, Z of the last layer are dead (admm_net.py:757-764): they are not evaluated, and, as in the
    reference, their parameters end up with ``grad = None``.
There is no CPU fallback: without the HIP library ``ops.eigh`` raises.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn.functional as F

from . import ops

EPS = 1e-8   # every layer's epsilon (admm_net.py:74, 114, 211, 360)


class Assembler:
    """The two contractions with a constant eigenvector matrix: ``vdvh(V, d) = V diag(d) V^H`` (exactly Hermitian)
    and its adjoint ``vhsv(V, S)[c] = Re(v_c^H S v_c)`` for Hermitian S.  The product uses the HIP kernels; the CPU unit
    tests hand in ``TorchAssembler`` to check the autograd wiring without a GPU."""

    vdvh = staticmethod(ops.vdvh)
    vhsv = staticmethod(ops.vhsv)


class TorchAssembler:
    """Stand-in for tests (tensor operations on whatever device the inputs live on)."""

    @staticmethod
    def vdvh(V, d):
        G = torch.matmul(V * d.unsqueeze(1).to(V.dtype), V.transpose(1, 2).conj())
        return 0.5 * (G + G.transpose(1, 2).conj())

    @staticmethod
    def vhsv(V, S):
        return (V.conj() * torch.matmul(S, V)).sum(dim=1).real


class _EighValuesOnly(torch.autograd.Function):
    """(w, V) = eigh(A) with V constant: backward is V diag(gw) V^H (admm_net.py:303-306)."""

    @staticmethod
    def forward(ctx, A, solver, asm):
        w, V = solver(A.detach())
        ctx.save_for_backward(V)
        ctx.asm = asm
        ctx.mark_non_differentiable(V)
        return w, V

    @staticmethod
    def backward(ctx, gw, _gV):
        (V,) = ctx.saved_tensors
        return ctx.asm.vdvh(V, gw.to(torch.float32)), None, None


class _Rebuild(torch.autograd.Function):
    """G = (G0 + G0^H) / 2 with G0 = V diag(d) V^H, V constant (admm_net.py:336-354); d carries the gradient
    Re(v_c^H S v_c) with S = (g + g^H) / 2, the backward of the symmetrisation followed by that of the two products."""

    @staticmethod
    def forward(ctx, V, d, asm):
        ctx.save_for_backward(V)
        ctx.asm = asm
        return asm.vdvh(V, d)

    @staticmethod
    def backward(ctx, g):
        (V,) = ctx.saved_tensors
        S = 0.5 * (g + g.transpose(1, 2).conj())
        return None, ctx.asm.vhsv(V, S), None


def _block_matrix(phi: torch.Tensor, h: torch.Tensor, corner: float) -> torch.Tensor:
    """[[diag(h), phi], [phi^H, corner]]  (admm_net.py:273-284, 428-439)."""
    B = phi.shape[0]
    top = torch.cat([torch.diag_embed(h).to(phi.dtype), phi.unsqueeze(-1)], dim=2)
    low = torch.cat([phi.conj().unsqueeze(1),
                     torch.full((B, 1, 1), corner, dtype=phi.dtype, device=phi.device)], dim=2)
    return torch.cat([top, low], dim=1)


def _herm(X):
    return 0.5 * (X + X.transpose(1, 2).conj())


def _inner(X, Y):
    """<X, Y> = Re sum conj(X_ij) Y_ij per signal."""
    return (X.conj() * Y).real.sum(dim=(1, 2))


def _diag(X, D):
    return torch.diagonal(X, dim1=1, dim2=2)[:, :D]


class LayerKernels:
    """The three n^2-sized layer steps and their backwards on the HIP kernels of csrc/train_layer.hip
    (C = ``_block_matrix``, never stored; r a 0-dim tensor, s [B], c a Python float):
      matrix(phi, h, Z, r, c) = herm(C - r Z);  resnorm(G, phi, h, c) = ||G - C||_F;  zupdate(Z, G, phi, h, s, c) = Z + s (G - C)
    The ``_bwd`` forms return the input gradients in the order of their signatures below."""

    matrix = staticmethod(ops.train_matrix)
    matrix_bwd = staticmethod(ops.train_matrix_bwd)              # (gA, Z, r) -> g_phi, g_h, gZ, g_r
    resnorm = staticmethod(ops.train_resnorm)
    resnorm_bwd = staticmethod(ops.train_resnorm_bwd)            # (g_rn, rn, G, phi, h, c) -> gG, g_phi, g_h
    zupdate = staticmethod(ops.train_zupdate)
    zupdate_bwd = staticmethod(ops.train_zupdate_bwd)            # (g, G, phi, h, s, c) -> gG, g_phi, g_h, g_s
    # the border column and the diagonal, all that the phi and H layers read of G and Z
    gather = staticmethod(ops.train_gather)                      # X -> X[:, :D, D], Re diag X[:, :D]
    scatter = staticmethod(ops.train_scatter)                    # its backward: (g_col, g_dg) -> dense E(g_col, g_dg)
    herm = staticmethod(ops.train_herm)                          # (g, g_col, g_dg) -> herm(g + E(g_col, g_dg))


class TorchLayerKernels:
    """Stand-in for tests: the same forward / backward formulas as tensor operations, any device, any dtype."""

    @staticmethod
    def matrix(phi, h, Z, r, c):
        return _herm(_block_matrix(phi, h, c) - r * Z)

    @staticmethod
    def matrix_bwd(gA, Z, r):
        S, D = _herm(gA), Z.shape[1] - 1
        return 2 * S[:, :D, D], _diag(S, D).real, -r * S, -_inner(S, Z).sum()

    @staticmethod
    def resnorm(G, phi, h, c):
        return torch.linalg.matrix_norm(G - _block_matrix(phi, h, c))

    @staticmethod
    def resnorm_bwd(g_rn, rn, G, phi, h, c):
        R, D = G - _block_matrix(phi, h, c), G.shape[1] - 1
        q = (g_rn / rn).reshape(-1, 1)
        return q.unsqueeze(-1) * R, -q * (R[:, :D, D] + R[:, D, :D].conj()), -q * _diag(R, D).real

    @staticmethod
    def zupdate(Z, G, phi, h, s, c):
        return Z + s.reshape(-1, 1, 1) * (G - _block_matrix(phi, h, c))

    @staticmethod
    def zupdate_bwd(g, G, phi, h, s, c):
        R, D = G - _block_matrix(phi, h, c), G.shape[1] - 1
        sd = s.reshape(-1, 1)
        return sd.unsqueeze(-1) * g, -sd * (g[:, :D, D] + g[:, D, :D].conj()), -sd * _diag(g, D).real, _inner(R, g)


    @staticmethod
    def gather(X):
        D = X.shape[1] - 1
        return X[:, :D, D].clone(), _diag(X, D).real.clone()

    @staticmethod
    def scatter(g_col, g_dg):
        B, D = g_col.shape
        E = torch.zeros(B, D + 1, D + 1, dtype=g_col.dtype, device=g_col.device)
        E[:, :D, D] = g_col
        _diag(E, D).copy_(g_dg.to(E.dtype))
        return E

    @staticmethod
    def herm(g, g_col=None, g_dg=None):
        return _herm(g if g_col is None else g + TorchLayerKernels.scatter(g_col, g_dg))


class _LayerMatrix(torch.autograd.Function):
    """A = herm(C(phi, h, c) - r Z) (admm_net.py:262-300).  A goes to the eigensolver only; the tape keeps Z and r."""

    @staticmethod
    def forward(ctx, phi, h, Z, r, c, lk):
        ctx.save_for_backward(Z, r)
        ctx.lk = lk
        return lk.matrix(phi, h, Z, r, c)

    @staticmethod
    def backward(ctx, gA):
        Z, r = ctx.saved_tensors
        g_phi, g_h, gZ, g_r = ctx.lk.matrix_bwd(gA, Z, r)
        return g_phi, g_h, gZ, g_r, None, None


class _ResidualNorm(torch.autograd.Function):
    """rn = ||G - C(phi, h, c)||_F (admm_net.py:428-459); the residual is recomputed in the backward."""

    @staticmethod
    def forward(ctx, G, phi, h, c, lk):
        rn = lk.resnorm(G, phi, h, c)
        ctx.save_for_backward(G, phi, h, rn)
        ctx.c, ctx.lk = c, lk
        return rn

    @staticmethod
    def backward(ctx, g_rn):
        G, phi, h, rn = ctx.saved_tensors
        gG, g_phi, g_h = ctx.lk.resnorm_bwd(g_rn, rn, G, phi, h, ctx.c)
        return gG, g_phi, g_h, None, None


class _StateUpdate(torch.autograd.Function):
    """Z' = Z + s (G - C(phi, h, c)) (admm_net.py:460-474); the gradient of Z is the incoming tensor itself."""

    @staticmethod
    def forward(ctx, Z, G, phi, h, s, c, lk):
        ctx.save_for_backward(G, phi, h, s)
        ctx.c, ctx.lk = c, lk
        return lk.zupdate(Z, G, phi, h, s, c)

    @staticmethod
    def backward(ctx, g):
        G, phi, h, s = ctx.saved_tensors
        gG, g_phi, g_h, g_s = ctx.lk.zupdate_bwd(g, G, phi, h, s, ctx.c)
        return g, gG, g_phi, g_h, g_s, None, None


class _Gather(torch.autograd.Function):
    """(X[:, :D, D], Re diag X[:, :D]) as ONE function: autograd answers each of the four slicing steps behind these two
    reads with a zero-filled dense tensor of its own; this backward writes the dense gradient once."""

    @staticmethod
    def forward(ctx, X, lk):
        ctx.lk = lk
        return lk.gather(X)

    @staticmethod
    def backward(ctx, g_col, g_dg):
        return ctx.lk.scatter(g_col, g_dg), None


class _RebuildGather(torch.autograd.Function):
    """``_Rebuild`` for the fused route, with the border column and the diagonal of G as outputs of their own: their
    gradients come back as [B, D] vectors and are folded into the symmetrisation, S = herm(g + E(g_col, g_dg)), so no dense
    tensor is made for them."""

    @staticmethod
    def forward(ctx, V, d, asm, lk):
        ctx.save_for_backward(V)
        ctx.asm, ctx.lk = asm, lk
        G = asm.vdvh(V, d)
        col, dg = lk.gather(G)
        return G, col, dg

    @staticmethod
    def backward(ctx, g, g_col, g_dg):
        (V,) = ctx.saved_tensors
        return None, ctx.asm.vhsv(V, ctx.lk.herm(g, g_col, g_dg)), None, None


class SmallKernels:
    """The O(B D)-sized layer steps and their backwards on the HIP kernels of csrc/train_small.hip.  Every parameter is the
    RAW tensor (softplus / sigmoid are applied inside) and every ``_bwd`` returns raw-parameter gradients, in the order of the
    comments below."""

    phi = staticmethod(ops.train_phi)                            # (y, b, g_col, z_col, rho) -> phi
    phi_bwd = staticmethod(ops.train_phi_bwd)                    # (g_phi, y, b, g_col, z_col, rho) -> g_gcol, g_zcol, g_rho
    hinput = staticmethod(ops.train_hinput)                      # (g_dg, z_dg, rho) -> t
    hinput_bwd = staticmethod(ops.train_hinput_bwd)              # (g_t, z_dg, rho) -> g_gdg, g_zdg, g_rho
    hproject = staticmethod(ops.train_hproject)                  # (t, m, sigma, pw) -> h
    hproject_bwd = staticmethod(ops.train_hproject_bwd)          # (g_h, t, m, sigma, pw) -> g_t, g_m, g_pw
    eigmap = staticmethod(ops.train_eigmap)                      # (w, thr, W1, b1, W2, b2) -> wp
    eigmap_bwd = staticmethod(ops.train_eigmap_bwd)              # (g_wp, w, thr, W1, b1, W2, b2) -> g_w, g_thr, gW1, gb1, gW2, gb2
    stepsize = staticmethod(ops.train_stepsize)                  # (rn, rho, W1, b1, W2, b2, knorm, sub_batch) -> step
    stepsize_bwd = staticmethod(ops.train_stepsize_bwd)          # (g_step, rn, ...) -> g_rn, g_rho, gW1, gb1, gW2, gb2


def _dsoftplus(x):
    """softplus'(x) as torch defines it: 1 above the linear threshold."""
    return torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))


def _dsigmoid(x):
    """sigmoid'(x) = s (1 - s) as e / (1 + e)^2 with e = exp(-|x|): 1 - s itself loses every digit as s nears 1."""
    e = torch.exp(-x.abs())
    return e / (1 + e) ** 2


def _group_total(x: torch.Tensor, sub_batch: Optional[int]):
    """(sum of x over every signal's group, the group's size), both broadcastable against x [B]."""
    B = x.shape[0]
    if sub_batch is None or sub_batch >= B:
        return x.sum(), B
    gid = torch.arange(B, device=x.device) // sub_batch
    sums = torch.zeros(int(gid[-1]) + 1, dtype=x.dtype, device=x.device).index_add(0, gid, x)
    return sums[gid], torch.bincount(gid).to(x.dtype)[gid]


class TorchSmallKernels:
    """Stand-in for tests: the same forward / backward formulas as tensor operations, any device, in the dtype it is given.
    The ``_terms`` forms return the batch sums of their ``_bwd`` forms unsummed (one term per signal and element), which is
    what an error bound in terms of sum |terms| needs."""

    @staticmethod
    def _phi_parts(y, b, g_col, z_col, rho):
        r = F.softplus(rho)
        bs = torch.abs(b) ** 2 + EPS
        coef = bs / (1 + r * bs)
        return r, coef, y / (b + EPS) + r * g_col + z_col

    @staticmethod
    def phi(y, b, g_col, z_col, rho):
        _, coef, inner = TorchSmallKernels._phi_parts(y, b, g_col, z_col, rho)
        return coef * inner

    @staticmethod
    def phi_terms(g_phi, y, b, g_col, z_col, rho):
        r, coef, inner = TorchSmallKernels._phi_parts(y, b, g_col, z_col, rho)
        d = coef * g_col - coef ** 2 * inner                       # d phi / d r
        return coef * r * g_phi, coef * g_phi, (g_phi.conj() * d).real * _dsoftplus(rho)

    @staticmethod
    def phi_bwd(g_phi, y, b, g_col, z_col, rho):
        g_gcol, g_zcol, terms = TorchSmallKernels.phi_terms(g_phi, y, b, g_col, z_col, rho)
        return g_gcol, g_zcol, terms.sum()

    @staticmethod
    def hinput(g_dg, z_dg, rho):
        return g_dg + z_dg / (F.softplus(rho) + EPS)

    @staticmethod
    def hinput_terms(g_t, z_dg, rho):
        den = F.softplus(rho) + EPS
        return g_t, g_t / den, -g_t * z_dg / den ** 2 * _dsoftplus(rho)

    @staticmethod
    def hinput_bwd(g_t, z_dg, rho):
        g_gdg, g_zdg, terms = TorchSmallKernels.hinput_terms(g_t, z_dg, rho)
        return g_gdg, g_zdg, terms.sum()

    @staticmethod
    def _project_parts(t, m, sigma, pw):
        D = t.shape[1]
        A = (2 * torch.sqrt(torch.tensor(float(D))).to(t.device) * sigma + sigma ** 2).reshape(-1, 1)
        tc = t + 0.1 * m
        a = tc.abs()
        mx = a.max(dim=1, keepdim=True)[0]
        imax = torch.where(a == mx, torch.arange(D, device=t.device).expand_as(a), D).min(dim=1, keepdim=True)[0]
        den = A * mx + tc.sum(dim=1, keepdim=True) + EPS
        return A, tc, imax, den, torch.sigmoid(pw)

    @staticmethod
    def hproject(t, m, sigma, pw):
        _, tc, _, den, sp = TorchSmallKernels._project_parts(t, m, sigma, pw)
        return tc * torch.clamp(sp / den, max=1.0)

    @staticmethod
    def hproject_terms(g_h, t, m, sigma, pw):
        A, tc, imax, den, sp = TorchSmallKernels._project_parts(t, m, sigma, pw)
        q = sp / den
        open_ = (q <= 1).to(t.dtype)                                # the clamp passes the gradient where q <= 1
        g_s = (g_h * tc).sum(dim=1, keepdim=True) * open_
        g_c = -g_s * sp / den ** 2
        at_max = torch.zeros_like(tc).scatter_(1, imax, 1.0)
        g_tc = g_h * torch.clamp(q, max=1.0) + g_c * (1 + at_max * A * torch.sign(tc))
        return g_tc, 0.1 * g_tc, (g_s / den * _dsigmoid(pw)).reshape(-1)

    @staticmethod
    def hproject_bwd(g_h, t, m, sigma, pw):
        g_t, g_m, terms = TorchSmallKernels.hproject_terms(g_h, t, m, sigma, pw)
        return g_t, g_m, terms.sum()

    @staticmethod
    def _eig_parts(w, thr, W1, b1, W2, b2):
        st = torch.sigmoid(thr)
        pre = w.abs().unsqueeze(-1) * W1.reshape(-1) + b1          # [B, n, 16]
        o = (torch.relu(pre) * W2.reshape(-1)).sum(dim=-1) + b2
        return st, pre, o, F.softplus(w - st), torch.sigmoid(o)

    @staticmethod
    def eigmap(w, thr, W1, b1, W2, b2):
        _, _, _, a, v = TorchSmallKernels._eig_parts(w, thr, W1, b1, W2, b2)
        return a * v

    @staticmethod
    def eigmap_terms(g_wp, w, thr, W1, b1, W2, b2):
        st, pre, o, a, v = TorchSmallKernels._eig_parts(w, thr, W1, b1, W2, b2)
        g_a, g_o = g_wp * v, g_wp * a * _dsigmoid(o)
        da = _dsoftplus(w - st)
        dh = g_o.unsqueeze(-1) * W2.reshape(-1) * (pre > 0).to(w.dtype)
        g_w = g_a * da + torch.sign(w) * (dh * W1.reshape(-1)).sum(dim=-1)
        return (g_w, -g_a * da * _dsigmoid(thr), dh * w.abs().unsqueeze(-1), dh, g_o.unsqueeze(-1) * torch.relu(pre), g_o)

    @staticmethod
    def eigmap_bwd(g_wp, w, thr, W1, b1, W2, b2):
        g_w, t_thr, tW1, tb1, tW2, tb2 = TorchSmallKernels.eigmap_terms(g_wp, w, thr, W1, b1, W2, b2)
        return (g_w, t_thr.sum(), tW1.sum(dim=(0, 1)).reshape(W1.shape), tb1.sum(dim=(0, 1)),
                tW2.sum(dim=(0, 1)).reshape(W2.shape), tb2.sum().reshape(b2.shape))

    @staticmethod
    def _step_parts(rn, rho, W1, b1, W2, b2, knorm, sub_batch):
        r = F.softplus(rho)
        total, count = _group_total(rn, sub_batch)
        mean = total / count
        den = mean + EPS
        u = rn / den
        feat = torch.stack([torch.full_like(rn, knorm), r.detach().expand_as(rn), u], dim=1)       # [B, 3]
        pre = feat @ W1.t() + b1                                                                    # [B, 32]
        o = torch.relu(pre) @ W2.reshape(-1) + b2
        return r, mean, den, feat, pre, o

    @staticmethod
    def stepsize(rn, rho, W1, b1, W2, b2, knorm, sub_batch=None):
        r, _, _, _, _, o = TorchSmallKernels._step_parts(rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        return r * (0.5 + 1.5 * torch.sigmoid(o))

    @staticmethod
    def stepsize_terms(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch=None):
        r, mean, den, feat, pre, o = TorchSmallKernels._step_parts(rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        dy = g_step * r * 1.5 * _dsigmoid(o)
        dh = dy.unsqueeze(1) * W2.reshape(-1) * (pre > 0).to(rn.dtype)                              # [B, 32]
        g_u = dh @ W1[:, 2]
        # g_u / den - mean(g_u rn) / den^2 with both parts over den^2: in a group of ONE signal they cancel to g_u eps / den^2,
        # which this form keeps (g_u mean - mean(g_u rn) is then an exact zero) and the plain difference loses to round-off
        total, count = _group_total(g_u * rn, sub_batch)
        g_rn = ((g_u * mean - total / count) + g_u * EPS) / den ** 2
        return (g_rn, g_step * (0.5 + 1.5 * torch.sigmoid(o)) * _dsoftplus(rho), dh.unsqueeze(2) * feat.unsqueeze(1), dh,
                dy.unsqueeze(1) * torch.relu(pre), dy)

    @staticmethod
    def stepsize_bwd(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch=None):
        g_rn, t_rho, tW1, tb1, tW2, tb2 = TorchSmallKernels.stepsize_terms(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        return g_rn, t_rho.sum(), tW1.sum(dim=0), tb1.sum(dim=0), tW2.sum(dim=0).reshape(W2.shape), tb2.sum().reshape(b2.shape)


class _PhiStep(torch.autograd.Function):
    """``_phi_layer_gathered`` as one function (admm_net.py:79-105); y and b carry no gradient."""

    @staticmethod
    def forward(ctx, y, b, g_col, z_col, rho, sk):
        ctx.save_for_backward(y, b, g_col, z_col, rho)
        ctx.sk = sk
        return sk.phi(y, b, g_col, z_col, rho)

    @staticmethod
    def backward(ctx, g_phi):
        g_gcol, g_zcol, g_rho = ctx.sk.phi_bwd(g_phi, *ctx.saved_tensors)
        return None, None, g_gcol, g_zcol, g_rho, None


class _HInput(torch.autograd.Function):
    """t = g_dg + z_dg / (softplus(rho) + eps) (admm_net.py:150-152)."""

    @staticmethod
    def forward(ctx, g_dg, z_dg, rho, sk):
        ctx.save_for_backward(z_dg, rho)
        ctx.sk = sk
        return sk.hinput(g_dg, z_dg, rho)

    @staticmethod
    def backward(ctx, g_t):
        g_gdg, g_zdg, g_rho = ctx.sk.hinput_bwd(g_t, *ctx.saved_tensors)
        return g_gdg, g_zdg, g_rho, None


class _HProject(torch.autograd.Function):
    """h from t and m = correction_net(t) (admm_net.py:160-194); sigma carries no gradient."""

    @staticmethod
    def forward(ctx, t, m, sigma, pw, sk):
        ctx.save_for_backward(t, m, sigma, pw)
        ctx.sk = sk
        return sk.hproject(t, m, sigma, pw)

    @staticmethod
    def backward(ctx, g_h):
        g_t, g_m, g_pw = ctx.sk.hproject_bwd(g_h, *ctx.saved_tensors)
        return g_t, g_m, None, g_pw, None


class _EigMap(torch.autograd.Function):
    """The learned eigenvalue map with value_net inside (admm_net.py:310-334)."""

    @staticmethod
    def forward(ctx, w, thr, W1, b1, W2, b2, sk):
        ctx.save_for_backward(w, thr, W1, b1, W2, b2)
        ctx.sk = sk
        return sk.eigmap(w, thr, W1, b1, W2, b2)

    @staticmethod
    def backward(ctx, g_wp):
        return (*ctx.sk.eigmap_bwd(g_wp, *ctx.saved_tensors), None)


class _StepSize(torch.autograd.Function):
    """The adaptive step with the group mean and residual_scale_net inside (admm_net.py:440-474)."""

    @staticmethod
    def forward(ctx, rn, rho, W1, b1, W2, b2, knorm, sub_batch, sk):
        ctx.save_for_backward(rn, rho, W1, b1, W2, b2)
        ctx.knorm, ctx.sub_batch, ctx.sk = knorm, sub_batch, sk
        return sk.stepsize(rn, rho, W1, b1, W2, b2, knorm, sub_batch)

    @staticmethod
    def backward(ctx, g_step):
        return (*ctx.sk.stepsize_bwd(g_step, *ctx.saved_tensors, ctx.knorm, ctx.sub_batch), None, None, None)


def _net_params(net):
    """(W1, b1, W2, b2) of a Linear - ReLU - Linear - Sigmoid module."""
    return net[0].weight, net[0].bias, net[2].weight, net[2].bias


def _resolve_corners(model, K):
    """The corner values ``1 / (softplus(lambda)^2 + eps)`` of gLayers[k], zLayers[k], k < K - 1, with one device-to-host read
    (the per-layer ``.item()`` of admm_net.py:271, 426 is a read each): [(corner_g, corner_z)] per layer."""
    if K < 2:
        return []
    lam = torch.stack([layer.lambda_param.detach() for k in range(K - 1) for layer in (model.gLayers[k], model.zLayers[k])])
    c = (1.0 / (F.softplus(lam) ** 2 + EPS)).tolist()
    return list(zip(c[0::2], c[1::2]))


def _phi_layer(layer, y, b, G, Z):
    """admm_net.py:79-105."""
    rho = F.softplus(layer.rho)
    b_sq = torch.abs(b) ** 2 + EPS
    return b_sq / (1 + rho * b_sq) * (y / (b + EPS) + rho * G[:, :-1, -1] + Z[:, :-1, -1])


def _phi_layer_gathered(layer, y, b, g_col, z_col):
    """``_phi_layer`` on the border columns of G and Z."""
    rho = F.softplus(layer.rho)
    b_sq = torch.abs(b) ** 2 + EPS
    return b_sq / (1 + rho * b_sq) * (y / (b + EPS) + rho * g_col + z_col)


def _h_layer(layer, G, Z, sigma, diags=None):
    """admm_net.py:134-194; returns the diagonal h [B, D].  ``diags``: (Re diag G, Re diag Z) [B, D] on the fused route."""
    D = layer.dim
    rho = F.softplus(layer.rho)
    if diags is None:
        t = (torch.diagonal(G, dim1=1, dim2=2)[:, :D] + torch.diagonal(Z, dim1=1, dim2=2)[:, :D] / (rho + EPS)).real
    else:
        t = diags[0] + diags[1] / (rho + EPS)
    A = (2 * torch.sqrt(torch.tensor(float(D))).to(t.device) * sigma + sigma ** 2).reshape(-1, 1)
    tc = t + 0.1 * layer.correction_net(t)
    cval = A * tc.abs().max(dim=1, keepdim=True)[0] + tc.sum(dim=1, keepdim=True)
    scale = torch.clamp(torch.sigmoid(layer.projection_weight) / (cval + EPS), max=1.0)
    return tc * scale


def _g_layer(layer, phi, h, Z, solver, asm, lk=None, sk=None, corner=None):
    """admm_net.py:237-354.  ``lk``: layer kernels of the fused route (None: tensor operations); ``sk``: small kernels of the
    full route; ``corner``: the detached corner value where the caller has resolved it already."""
    if corner is None:
        corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
    if lk is None:
        A = _block_matrix(phi, h, corner) - (1.0 / (F.softplus(layer.rho) + EPS)) * Z
        A = 0.5 * (A + A.transpose(1, 2).conj())
    else:
        A = _LayerMatrix.apply(phi, h, Z, 1.0 / (F.softplus(layer.rho) + EPS), corner, lk)
    w, V = _EighValuesOnly.apply(A, solver, asm)
    # learned eigenvalue map, every eigenvalue through the same 1 -> 16 -> 1 network (admm_net.py:310-334)
    if sk is None:
        wp = F.softplus(w - torch.sigmoid(layer.threshold)) * layer.value_net(w.abs().unsqueeze(-1)).squeeze(-1)
    else:
        wp = _EigMap.apply(w, layer.threshold, *_net_params(layer.value_net), sk)
    if lk is not None:
        return _RebuildGather.apply(V, wp, asm, lk)       # (G, G[:, :D, D], Re diag G)
    return _Rebuild.apply(V, wp, asm)


def _group_mean(rn: torch.Tensor, sub_batch: Optional[int]) -> torch.Tensor:
    """The batch mean of admm_net.py:459 for every signal: over the whole call, or over its group of ``sub_batch``
    consecutive signals (the last group may be shorter)."""
    B = rn.shape[0]
    if sub_batch is None or sub_batch >= B:
        return rn.mean()
    gid = torch.arange(B, device=rn.device) // sub_batch
    sums = torch.zeros(int(gid[-1]) + 1, dtype=rn.dtype, device=rn.device).index_add(0, gid, rn)
    return (sums / torch.bincount(gid).to(rn.dtype))[gid]


def _z_layer(layer, k, phi, h, G, Z, sub_batch=None, lk=None, sk=None, corner=None):
    """admm_net.py:388-474.  ``lk``, ``sk``, ``corner``: as for ``_g_layer``."""
    if corner is None:
        corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
    if sk is not None:
        rn = _ResidualNorm.apply(G, phi, h, corner, lk)
        step = _StepSize.apply(rn, layer.rho, *_net_params(layer.residual_scale_net), k / 10.0, sub_batch, sk)
        return _StateUpdate.apply(Z, G, phi, h, step, corner, lk)
    rho = F.softplus(layer.rho)
    if lk is None:
        R = G - _block_matrix(phi, h, corner)
        rn = torch.linalg.matrix_norm(R)                               # Frobenius, [B]
    else:
        rn = _ResidualNorm.apply(G, phi, h, corner, lk)
    B = rn.shape[0]
    feat = torch.stack([torch.full((B,), k / 10.0, device=rn.device),
                        torch.full((B,), rho.item(), device=rn.device),
                        rn / (_group_mean(rn, sub_batch) + EPS)], dim=1)
    step = rho * (0.5 + 1.5 * layer.residual_scale_net(feat)).squeeze(1)
    if lk is None:
        return Z + step.reshape(-1, 1, 1) * R
    return _StateUpdate.apply(Z, G, phi, h, step, corner, lk)


def _peak_head(head, phi):
    """admm_net.py:570-630 (dropout of the attention is live in train mode, as in the reference)."""
    B = phi.shape[0]
    x = head.feature_extractor(torch.cat([phi.real, phi.imag], dim=1))
    pos = head.position_projection(head.position_encoder.unsqueeze(0).expand(B, -1, -1))
    att, _ = head.attention(query=x.unsqueeze(1), key=pos, value=pos)
    xp = head.peak_extractor(x + att.squeeze(1))
    taus, fs, cs = [], [], []
    for t in range(head.L_max):
        z = xp + torch.tensor(t / head.L_max, device=phi.device)
        taus.append(head.tau_regressor[t](z))
        fs.append(head.f_regressor[t](z))
        cs.append(head.confidence_net(z))
    return torch.cat(taus, 1), torch.cat(fs, 1), torch.cat(cs, 1)


def unrolled_forward(model, y: torch.Tensor, b: torch.Tensor, sigma: torch.Tensor,
                     solver: Optional[Callable] = None, assembler=None, sub_batch: Optional[int] = None,
                     fused: bool = False, layer_kernels=None, small: bool = False, small_kernels=None):
    """Differentiable K-layer forward on the device of ``y`` (admm_net.py:742-764 / 791-816).

    ``sub_batch = g`` evaluates the consecutive groups of g signals as independent batches, each with its own mean
    (``_FusedBase.sub_batch``); None: the call is one batch.

    ``solver(A) -> (w, V)`` defaults to the HIP eigensolver (under ``model.options``) and ``assembler`` to the HIP contractions; the CPU unit
    tests pass stand-ins (``torch.linalg.eigh``, ``TorchAssembler``) to check the autograd wiring against the reference's
    gradients without a GPU.

    ``fused = True`` evaluates the n^2-sized steps of every layer through ``layer_kernels`` (default ``LayerKernels``, the
    HIP kernels of csrc/train_layer.hip; the CPU tests pass ``TorchLayerKernels``) instead of tensor operations.
    ``small = True`` (needs ``fused = True``) also evaluates the phi layer, the H layer around its ``correction_net``, the
    eigenvalue map and the step-size network through ``small_kernels`` (default ``SmallKernels``, the HIP kernels of
    csrc/train_small.hip; the CPU tests pass ``TorchSmallKernels``), and reads the detached corner values of all layers from
    the device once.
    Returns phi, or (tau, f, confidences, phi) when the model has a PeakSearchLayer.
    """
    if sub_batch is not None and sub_batch < 1:
        raise ValueError(f"sub_batch must be None or >= 1, got {sub_batch}")
    if solver is None:   # the HIP eigensolver under the model's own option set (``model.options``; None = the process defaults)
        opts = getattr(model, "options", None)
        solver = ops.eigh if opts is None else (lambda A: ops.eigh(A, options=opts))
    asm = Assembler if assembler is None else assembler
    if layer_kernels is not None and not fused:
        raise ValueError("layer_kernels is only used with fused=True")
    lk = (LayerKernels if layer_kernels is None else layer_kernels) if fused else None
    if small and not fused:
        raise ValueError("small=True needs fused=True")
    if small_kernels is not None and not small:
        raise ValueError("small_kernels is only used with small=True")
    sk = (SmallKernels if small_kernels is None else small_kernels) if small else None
    K, D = model.num_layers, model.M * model.N
    if y.dim() != 2 or y.shape[1] != D or b.shape != y.shape:
        raise ValueError(f"y, b must be [B, {D}] complex; got {tuple(y.shape)}, {tuple(b.shape)}")
    y = y.to(torch.complex64)
    b = b.to(torch.complex64)
    sigma = sigma.to(torch.float32).reshape(-1)
    B, n = y.shape[0], D + 1
    G = torch.zeros(B, n, n, dtype=torch.complex64, device=y.device)
    Z = torch.zeros_like(G)
    phi = None
    if lk is not None:
        # the phi and H layers read only the border column and the diagonal of G and Z: gathered once per layer
        g_col = z_col = torch.zeros(B, D, dtype=torch.complex64, device=y.device)
        g_dg = z_dg = torch.zeros(B, D, dtype=torch.float32, device=y.device)
    corners = _resolve_corners(model, K) if sk is not None else None
    for k in range(K):
        if sk is not None:
            phi = _PhiStep.apply(y, b, g_col, z_col, model.phiLayers[k].rho, sk)
            if k == K - 1:
                break
            hl = model.hLayers[k]
            t = _HInput.apply(g_dg, z_dg, hl.rho, sk)
            h = _HProject.apply(t, hl.correction_net(t), sigma, hl.projection_weight, sk)
            G, g_col, g_dg = _g_layer(model.gLayers[k], phi, h, Z, solver, asm, lk, sk, corners[k][0])
            Z = _z_layer(model.zLayers[k], k, phi, h, G, Z, sub_batch, lk, sk, corners[k][1])
            z_col, z_dg = _Gather.apply(Z, lk)
            continue
        if lk is None:
            phi = _phi_layer(model.phiLayers[k], y, b, G, Z)
        else:
            phi = _phi_layer_gathered(model.phiLayers[k], y, b, g_col, z_col)
        if k == K - 1:
            break
        if lk is None:
            h = _h_layer(model.hLayers[k], G, Z, sigma)
            G = _g_layer(model.gLayers[k], phi, h, Z, solver, asm)
            Z = _z_layer(model.zLayers[k], k, phi, h, G, Z, sub_batch)
        else:
            h = _h_layer(model.hLayers[k], None, None, sigma, (g_dg, z_dg))
            G, g_col, g_dg = _g_layer(model.gLayers[k], phi, h, Z, solver, asm, lk)
            Z = _z_layer(model.zLayers[k], k, phi, h, G, Z, sub_batch, lk)
            z_col, z_dg = _Gather.apply(Z, lk)
    if getattr(model, "_HAS_HEAD", False):
        tau, f, conf = _peak_head(model.peakSearchLayer, phi)
        return tau, f, conf, phi
    return phi
