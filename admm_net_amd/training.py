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


def _g_layer(layer, phi, h, Z, solver, asm, lk=None):
    """admm_net.py:237-354.  ``lk``: layer kernels of the fused route (None: tensor operations)."""
    corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
    if lk is None:
        A = _block_matrix(phi, h, corner) - (1.0 / (F.softplus(layer.rho) + EPS)) * Z
        A = 0.5 * (A + A.transpose(1, 2).conj())
    else:
        A = _LayerMatrix.apply(phi, h, Z, 1.0 / (F.softplus(layer.rho) + EPS), corner, lk)
    w, V = _EighValuesOnly.apply(A, solver, asm)
    # learned eigenvalue map, every eigenvalue through the same 1 -> 16 -> 1 network (admm_net.py:310-334)
    wp = F.softplus(w - torch.sigmoid(layer.threshold)) * layer.value_net(w.abs().unsqueeze(-1)).squeeze(-1)
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


def _z_layer(layer, k, phi, h, G, Z, sub_batch=None, lk=None):
    """admm_net.py:388-474.  ``lk``: layer kernels of the fused route (None: tensor operations)."""
    corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
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
                     fused: bool = False, layer_kernels=None):
    """Differentiable K-layer forward on the device of ``y`` (admm_net.py:742-764 / 791-816).

    ``sub_batch = g`` evaluates the consecutive groups of g signals as independent batches, each with its own mean
    (``_FusedBase.sub_batch``); None: the call is one batch.

    ``solver(A) -> (w, V)`` defaults to the HIP eigensolver and ``assembler`` to the HIP contractions; the CPU unit
    tests pass stand-ins (``torch.linalg.eigh``, ``TorchAssembler``) to check the autograd wiring against the reference's
    gradients without a GPU.

    ``fused = True`` evaluates the n^2-sized steps of every layer through ``layer_kernels`` (default ``LayerKernels``, the
    HIP kernels of csrc/train_layer.hip; the CPU tests pass ``TorchLayerKernels``) instead of tensor operations.
    Returns phi, or (tau, f, confidences, phi) when the model has a PeakSearchLayer.
    """
    if sub_batch is not None and sub_batch < 1:
        raise ValueError(f"sub_batch must be None or >= 1, got {sub_batch}")
    solver = ops.eigh if solver is None else solver
    asm = Assembler if assembler is None else assembler
    if layer_kernels is not None and not fused:
        raise ValueError("layer_kernels is only used with fused=True")
    lk = (LayerKernels if layer_kernels is None else layer_kernels) if fused else None
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
    for k in range(K):
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
