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

``native=True`` on top of ``small=True`` (``model.train_route = "native"``) moves ``correction_net`` into the H layer's kernels: the
whole H layer is one autograd function over one forward kernel, one backward kernel and a batch-reduced product on the matrix
cores for the MLP's weight gradients (csrc/train_hlayer.hip, ``NativeKernels``; ``TorchNativeKernels`` for the CPU tests), and the G
layers' ``1 / (softplus(rho) + eps)`` is evaluated once per forward on the stacked rhos.  The PeakSearchLayer head of ``ADMMNet``
is one autograd function too (``_PeakHead``, csrc/train_head.hip): a K/V kernel for the batch-independent position tokens, one
per-signal forward and one per-signal backward kernel, the weight gradients and the token side's gK, gV as batch-reduced products
on the matrix cores, and a token-backward kernel.  The attention dropout is an INPUT of that function, a keep mask [B, 4, D]
drawn with one ``torch.rand`` call (``draw_keep_mask``) when the head is in train mode: the same distribution as
``nn.MultiheadAttention``'s dropout, another realisation under the same seed.

The four routes nest, ``TRAIN_ROUTES = ("tensor", "fused", "full", "native")``, and ``route_kwargs`` is the one place that turns a
name into the flags and kernel sets of ``unrolled_forward``.  ``unrolled_forward`` resolves its arguments once into the kernel sets
``lk``, ``sk``, ``nk`` (None where the route does not use them) and runs ONE layer loop -- phi step, H step, G step, Z step, the last
two leaving the gathered border column and diagonal of their result for the next layer -- in which every step function
(``_phi_step``, ``_h_step``, ``_g_step`` / ``_g_layer``, ``_z_step`` / ``_z_layer``) holds its own choice between the tensor form and
the kernels.  A new route is a new name in ``TRAIN_ROUTES``, its flag in ``route_kwargs`` and a branch in the steps it changes.

``reducer`` (``unrolled_forward(..., reducer=...)``, set by ``sharded.ShardedTraining``) makes the call one SHARD of a batch that is
split across the ranks of a process group: the mean of every Z layer is then over the signals of all ranks.  On the ``tensor`` and
``fused`` routes the coupling is ``_ReducedSum``, whose forward and backward are both an all-reduce sum; on ``full`` and ``native``
``_StepSize`` runs the ``pair`` kernels of csrc/train_small.hip around the two reductions.  With the default None nothing of this
runs.

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

from types import SimpleNamespace
from typing import Callable, Optional

import torch
import torch.nn.functional as F

from . import ops

EPS = 1e-8   # every layer's epsilon (admm_net.py:74, 114, 211, 360)
TRAIN_ROUTES = ("tensor", "fused", "full", "native")   # ``model.train_route``: each name adds a kernel set to the one before it
_STAND_INS = ("solver", "assembler", "layer_kernels", "small_kernels", "native_kernels")


def route_kwargs(route: str, kernels: Optional[dict] = None) -> dict:
    """The keyword arguments of ``unrolled_forward`` for a ``train_route`` name: the flags ``fused``, ``small``, ``native`` and,
    out of ``kernels`` (stand-ins by keyword, as the CPU tests pass them), the eigensolver, the assembler and the kernel sets
    that the route uses.  This is the one place that knows what a route name means."""
    if not isinstance(route, str) or route not in TRAIN_ROUTES:
        raise ValueError(f"train_route must be one of {TRAIN_ROUTES}, got {route!r}")
    level = TRAIN_ROUTES.index(route)
    kw = {"fused": level >= 1, "small": level >= 2, "native": level >= 3}
    kw.update({name: kernels[name] for name in _STAND_INS[:2 + level] if kernels and name in kernels})
    return kw


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
    # the step size from a (sum of rn, count) pair that comes from outside the call: the mean over the ranks of a sharded batch
    rnsum = staticmethod(ops.train_rnsum)                        # rn -> this call's pair, float64 [2]
    stepsize_pair = staticmethod(ops.train_stepsize_pair)        # (rn, pair, rho, W1, b1, W2, b2, knorm) -> step
    stepsize_bwd_pair_front = staticmethod(ops.train_stepsize_bwd_pair_front)   # (g_step, rn, pair, ...) -> g_u, total [1] f64, g_rho,
    #                                                                             gW1, gb1, gW2, gb2 (this call's sums)
    stepsize_bwd_pair_back = staticmethod(ops.train_stepsize_bwd_pair_back)     # (g_u, pair, total over the ranks) -> g_rn


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
    def _step_parts(rn, rho, W1, b1, W2, b2, knorm, sub_batch, pair=None):
        r = F.softplus(rho)
        if pair is None:
            total, count = _group_total(rn, sub_batch)
            mean = total / count
        else:                                                       # the mean of a larger batch, rounded to the dtype as the kernels do
            mean = (pair[0] / pair[1]).to(rn.dtype)
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
    def _step_net_terms(g_step, rn, rho, W1, W2, r, feat, pre, o):
        """(g_u [B], then one term per signal of g_rho, gW1, gb1, gW2, gb2): everything of the backward but the coupling."""
        dy = g_step * r * 1.5 * _dsigmoid(o)
        dh = dy.unsqueeze(1) * W2.reshape(-1) * (pre > 0).to(rn.dtype)                              # [B, 32]
        return (dh @ W1[:, 2], g_step * (0.5 + 1.5 * torch.sigmoid(o)) * _dsoftplus(rho), dh.unsqueeze(2) * feat.unsqueeze(1), dh,
                dy.unsqueeze(1) * torch.relu(pre), dy)

    @staticmethod
    def stepsize_terms(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch=None):
        r, mean, den, feat, pre, o = TorchSmallKernels._step_parts(rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        g_u, *terms = TorchSmallKernels._step_net_terms(g_step, rn, rho, W1, W2, r, feat, pre, o)
        # g_u / den - mean(g_u rn) / den^2 with both parts over den^2: in a group of ONE signal they cancel to g_u eps / den^2,
        # which this form keeps (g_u mean - mean(g_u rn) is then an exact zero) and the plain difference loses to round-off
        total, count = _group_total(g_u * rn, sub_batch)
        g_rn = ((g_u * mean - total / count) + g_u * EPS) / den ** 2
        return (g_rn, *terms)

    @staticmethod
    def stepsize_bwd(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch=None):
        g_rn, t_rho, tW1, tb1, tW2, tb2 = TorchSmallKernels.stepsize_terms(g_step, rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        return g_rn, t_rho.sum(), tW1.sum(dim=0), tb1.sum(dim=0), tW2.sum(dim=0).reshape(W2.shape), tb2.sum().reshape(b2.shape)

    # ---- the step size from a pair (sum of rn, count) float64 [2] of a LARGER batch than the call (the ranks of a sharded batch)
    @staticmethod
    def rnsum(rn):
        return torch.stack([rn.to(torch.float64).sum(), torch.tensor(float(rn.shape[0]), dtype=torch.float64, device=rn.device)])

    @staticmethod
    def stepsize_pair(rn, pair, rho, W1, b1, W2, b2, knorm):
        r, _, _, _, _, o = TorchSmallKernels._step_parts(rn, rho, W1, b1, W2, b2, knorm, None, pair)
        return r * (0.5 + 1.5 * torch.sigmoid(o))

    @staticmethod
    def stepsize_pair_terms(g_step, rn, pair, rho, W1, b1, W2, b2, knorm):
        """(g_u [B], then one term per signal of total (float64), g_rho, gW1, gb1, gW2, gb2)."""
        r, _, _, feat, pre, o = TorchSmallKernels._step_parts(rn, rho, W1, b1, W2, b2, knorm, None, pair)
        g_u, *terms = TorchSmallKernels._step_net_terms(g_step, rn, rho, W1, W2, r, feat, pre, o)
        return (g_u, g_u.to(torch.float64) * rn.to(torch.float64), *terms)

    @staticmethod
    def stepsize_bwd_pair_front(g_step, rn, pair, rho, W1, b1, W2, b2, knorm):
        g_u, t_tot, t_rho, tW1, tb1, tW2, tb2 = TorchSmallKernels.stepsize_pair_terms(g_step, rn, pair, rho, W1, b1, W2, b2, knorm)
        return (g_u, t_tot.sum().reshape(1), t_rho.sum(), tW1.sum(dim=0), tb1.sum(dim=0), tW2.sum(dim=0).reshape(W2.shape),
                tb2.sum().reshape(b2.shape))

    @staticmethod
    def stepsize_bwd_pair_back(g_u, pair, total):
        """``stepsize_terms``' cancellation-safe g_rn with the mean and the coupling sum of the larger batch; the difference is
        taken in float64, where the product of two float32 numbers is exact (a pair of ONE signal leaves g_u eps / den^2)."""
        mean = (pair[0] / pair[1]).to(g_u.dtype)
        diff = (g_u.to(torch.float64) * mean.to(torch.float64) - total.reshape(()) / pair[1]).to(g_u.dtype)
        return (diff + g_u * EPS) / (mean + EPS) ** 2


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
    def forward(ctx, rn, rho, W1, b1, W2, b2, knorm, sub_batch, sk, reducer=None):
        ctx.knorm, ctx.sub_batch, ctx.sk, ctx.reducer = knorm, sub_batch, sk, reducer
        if reducer is None:
            ctx.save_for_backward(rn, rho, W1, b1, W2, b2)
            return sk.stepsize(rn, rho, W1, b1, W2, b2, knorm, sub_batch)
        pair = reducer(sk.rnsum(rn))                  # (sum of rn, count) over all ranks
        ctx.save_for_backward(rn, rho, W1, b1, W2, b2, pair)
        return sk.stepsize_pair(rn, pair, rho, W1, b1, W2, b2, knorm)

    @staticmethod
    def backward(ctx, g_step):
        if ctx.reducer is None:
            return (*ctx.sk.stepsize_bwd(g_step, *ctx.saved_tensors, ctx.knorm, ctx.sub_batch), None, None, None, None)
        rn, rho, W1, b1, W2, b2, pair = ctx.saved_tensors
        g_u, total, *g_par = ctx.sk.stepsize_bwd_pair_front(g_step, rn, pair, rho, W1, b1, W2, b2, ctx.knorm)
        g_rn = ctx.sk.stepsize_bwd_pair_back(g_u, pair, ctx.reducer(total))     # the adjoint of the forward's sum: a sum again
        return (g_rn, *g_par, None, None, None, None)


class _ReducedSum(torch.autograd.Function):
    """(sum of rn over the signals of ALL ranks, their number), both float64 0-dim: ``reducer`` all-reduces (sum) a float64
    tensor across the ranks.  The forward moves the pair, the backward the one float64 gradient of the sum; the count carries
    none."""

    @staticmethod
    def forward(ctx, rn, reducer):
        ctx.reducer, ctx.dtype, ctx.B = reducer, rn.dtype, rn.shape[0]
        pair = reducer(TorchSmallKernels.rnsum(rn))
        total, count = pair[0].clone(), pair[1].clone()
        ctx.mark_non_differentiable(count)
        return total, count

    @staticmethod
    def backward(ctx, g_total, _g_count):
        g = ctx.reducer(g_total.to(torch.float64).reshape(1).clone())
        return g.to(ctx.dtype).expand(ctx.B), None


class NativeKernels:
    """The whole H layer, ``correction_net`` included, on the HIP kernels of csrc/train_hlayer.hip: one forward and one backward
    kernel per signal slab, and the weight gradients as one batch-reduced product on the matrix cores; and the PeakSearchLayer
    head on those of csrc/train_head.hip.  RAW parameters in, raw-parameter gradients out, as for ``SmallKernels``."""

    hlayer = staticmethod(ops.train_hlayer)            # (g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2) -> h, t, a1, m
    hlayer_bwd = staticmethod(ops.train_hlayer_bwd)    # (g_h, z_dg, sigma, rho, pw, W1, W2, t, a1, m) -> g_gdg, g_zdg, g_rho, g_pw,
    #                                                    gW1, gb1, gW2, gb2, delta1, delta2
    head = staticmethod(ops.train_head)                # (phi, keep, p, L, hp) -> tau, f, conf, saved
    head_bwd = staticmethod(ops.train_head_bwd)        # (g_tau, g_f, g_conf, phi, keep, p, L, hp, saved) -> g_phi, [g of hp]


class TorchNativeKernels:
    """Stand-in for tests: the same forward / backward formulas as tensor operations, any device, in the dtype it is given.
    ``hlayer_terms`` returns the batch sums of ``hlayer_bwd`` unsummed, as the ``_terms`` forms of ``TorchSmallKernels`` do;
    ``head_bwd(..., mag=True)`` returns the sums of the magnitudes of the head's terms (the terms themselves would be
    B x 128 x 2 D numbers).  The head is written out without ``nn.MultiheadAttention``."""

    @staticmethod
    def hlayer(g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2):
        t = TorchSmallKernels.hinput(g_dg, z_dg, rho)
        a1 = torch.relu(t @ W1.t() + b1)
        m = torch.tanh(a1 @ W2.t() + b2)
        return TorchSmallKernels.hproject(t, m, sigma, pw), t, a1, m

    @staticmethod
    def hlayer_terms(g_h, z_dg, sigma, rho, pw, W1, W2, t, a1, m):
        """(g_gdg, g_zdg, delta1, delta2, then one term per signal and element of g_rho [B, D], g_pw [B], gW1 [B, 64, D],
        gb1 [B, 64], gW2 [B, D, 64], gb2 [B, D])."""
        g_tc, _, t_pw = TorchSmallKernels.hproject_terms(g_h, t, m, sigma, pw)
        d2 = 0.1 * g_tc * (1 - m ** 2)
        d1 = (d2 @ W2) * (a1 > 0).to(t.dtype)                       # relu'(0) = 0
        g_gdg, g_zdg, t_rho = TorchSmallKernels.hinput_terms(g_tc + d1 @ W1, z_dg, rho)
        return g_gdg, g_zdg, d1, d2, t_rho, t_pw, d1.unsqueeze(2) * t.unsqueeze(1), d1, d2.unsqueeze(2) * a1.unsqueeze(1), d2

    @staticmethod
    def hlayer_bwd(g_h, z_dg, sigma, rho, pw, W1, W2, t, a1, m):
        g_gdg, g_zdg, d1, d2, t_rho, t_pw, tW1, tb1, tW2, tb2 = TorchNativeKernels.hlayer_terms(g_h, z_dg, sigma, rho, pw, W1, W2,
                                                                                                t, a1, m)
        return g_gdg, g_zdg, t_rho.sum(), t_pw.sum(), tW1.sum(dim=0), tb1.sum(dim=0), tW2.sum(dim=0), tb2.sum(dim=0), d1, d2


    # ---- the PeakSearchLayer head.  ``hp``: the head's RAW parameters in the order of ``_head_params``
    @staticmethod
    def _head_parts(phi, keep, p, L, hp):
        B, D = phi.shape
        pos, fe0w, fe0b, fe2w, fe2b, ppw, ppb, inw, inb, outw, outb, pe0w, pe0b, pe2w, pe2b, pe4w, pe4b = hp[:17]
        s = SimpleNamespace()
        s.feat = torch.cat([phi.real, phi.imag], dim=1)
        s.x1 = torch.relu(s.feat @ fe0w.t() + fe0b)
        s.x = torch.relu(s.x1 @ fe2w.t() + fe2b)
        s.P = pos @ ppw.t() + ppb                                                                # [D, 128], batch independent
        s.q = ((s.x @ inw[:128].t() + inb[:128]) * _ATT_SCALE).reshape(B, 4, 32)                 # scaled before the product
        s.K = (s.P @ inw[128:256].t() + inb[128:256]).reshape(D, 4, 32)
        s.V = (s.P @ inw[256:].t() + inb[256:]).reshape(D, 4, 32)
        s.a = torch.softmax(torch.einsum("bhj,dhj->bhd", s.q, s.K), dim=2)
        s.km = None if keep is None else keep.to(s.a.dtype) / (1.0 - p)
        s.am = s.a if keep is None else s.a * s.km
        s.ctx = torch.einsum("bhd,dhj->bhj", s.am, s.V).reshape(B, 128)
        s.xf = s.x + s.ctx @ outw.t() + outb
        s.u0 = torch.relu(s.xf @ pe0w.t() + pe0b)
        s.u1 = torch.relu(s.u0 @ pe2w.t() + pe2b)
        s.xp = torch.relu(s.u1 @ pe4w.t() + pe4b)
        off = torch.tensor([t / L for t in range(L)], dtype=torch.float32).to(s.xp)               # t / L is a float32 constant
        s.z = s.xp.unsqueeze(1) + off.reshape(1, L, 1)                                           # [B, L, 16]
        return s

    @staticmethod
    def head(phi, keep, p, L, hp):
        """(tau, f, conf [B, L], saved): ``_peak_head`` with ``keep`` [B, 4, D] (None: no dropout) as the attention's keep
        mask, a <- a keep / (1 - p) between the softmax and the value product."""
        s = TorchNativeKernels._head_parts(phi, keep, p, L, hp)
        c0w, c0b, c2w, c2b = hp[17:21]
        taus, fs, cs = [], [], []
        for t in range(L):
            tw0, tb0, tw2, tb2, fw0, fb0, fw2, fb2 = hp[21 + 8 * t:29 + 8 * t]
            z = s.z[:, t]
            taus.append(torch.sigmoid(torch.relu(z @ tw0.t() + tb0) @ tw2.t() + tb2))
            fs.append(torch.tanh(torch.relu(z @ fw0.t() + fb0) @ fw2.t() + fb2))
            cs.append(torch.sigmoid(torch.relu(z @ c0w.t() + c0b) @ c2w.t() + c2b))
        return torch.cat(taus, 1), torch.cat(fs, 1), torch.cat(cs, 1), ()

    @staticmethod
    def head_bwd(g_tau, g_f, g_conf, phi, keep, p, L, hp, saved=(), mag=False):
        """(g_phi, [gradient of every tensor of ``hp``]).  ``mag = True`` returns, instead of each batch sum, the sum of the
        magnitudes of its terms (what an error bound in terms of sum |terms| needs); g_phi is then meaningless."""
        B, D = phi.shape
        s = TorchNativeKernels._head_parts(phi, keep, p, L, hp)
        pos, fe0w, _, fe2w, _, ppw, _, inw, _, outw, _, pe0w, _, pe2w, _, pe4w, _, c0w, c0b, c2w, c2b = hp[:21]
        ab = (lambda v: v.abs()) if mag else (lambda v: v)
        bs = lambda d, v: ab(d).t() @ ab(v)                                  # sum_b d_b (x) v_b
        cs = lambda d: ab(d).sum(dim=0)
        g = [None] * len(hp)
        g_xp = torch.zeros_like(s.xp)
        g[17], g[18], g[19], g[20] = (torch.zeros_like(v) for v in hp[17:21])
        for t in range(L):
            tw0, tb0, tw2, tb2, fw0, fb0, fw2, fb2 = hp[21 + 8 * t:29 + 8 * t]
            z, o = s.z[:, t], 21 + 8 * t
            for w0, b0, w2, b2, gout, act, at in ((tw0, tb0, tw2, tb2, g_tau, "s", o), (fw0, fb0, fw2, fb2, g_f, "t", o + 4),
                                                  (c0w, c0b, c2w, c2b, g_conf, "s", 17)):
                hid = torch.relu(z @ w0.t() + b0)
                out = hid @ w2.t() + b2
                out = torch.sigmoid(out) if act == "s" else torch.tanh(out)
                do = gout[:, t:t + 1] * (out * (1 - out) if act == "s" else 1 - out ** 2)     # [B, 1]
                dh = (do @ w2) * (hid > 0).to(z.dtype)                                        # relu'(0) = 0
                g_xp = g_xp + dh @ w0
                new = (bs(dh, z), cs(dh), bs(do, hid), cs(do))
                for i, v in enumerate(new):                                                   # confidence_net sums over t
                    g[at + i] = v if at != 17 else g[at + i] + v
        d4 = g_xp * (s.xp > 0).to(g_xp.dtype)
        d2 = (d4 @ pe4w) * (s.u1 > 0).to(d4.dtype)
        d0 = (d2 @ pe2w) * (s.u0 > 0).to(d4.dtype)
        g[15], g[16], g[13], g[14], g[11], g[12] = bs(d4, s.u1), cs(d4), bs(d2, s.u0), cs(d2), bs(d0, s.xf), cs(d0)
        g_xf = d0 @ pe0w
        g[9], g[10] = bs(g_xf, s.ctx), cs(g_xf)
        g_ctx = (g_xf @ outw).reshape(B, 4, 32)
        g_am = torch.einsum("bhj,dhj->bhd", g_ctx, s.V)
        g_a = g_am if keep is None else g_am * s.km
        g_s = s.a * (g_a - (s.a * g_a).sum(dim=2, keepdim=True))
        gV = torch.einsum("bhd,bhj->dhj", ab(s.am), ab(g_ctx)).reshape(D, 128)
        gK = torch.einsum("bhd,bhj->dhj", ab(g_s), ab(s.q)).reshape(D, 128)
        dq = torch.einsum("bhd,dhj->bhj", g_s, s.K).reshape(B, 128) * _ATT_SCALE
        g_x = g_xf + dq @ inw[:128]
        dp2 = g_x * (s.x > 0).to(g_x.dtype)
        dp1 = (dp2 @ fe2w) * (s.x1 > 0).to(g_x.dtype)
        g[3], g[4], g[1], g[2] = bs(dp2, s.x1), cs(dp2), bs(dp1, s.feat), cs(dp1)
        g_feat = dp1 @ fe0w
        # the token side: sums over the batch first (gK, gV), then through the K and V slices of in_proj to the tokens
        g_P = gK @ ab(inw[128:256]) + gV @ ab(inw[256:])
        g[7] = torch.cat([bs(dq, s.x), bs(gK, s.P), bs(gV, s.P)])
        g[8] = torch.cat([cs(dq), cs(gK), cs(gV)])                            # in_proj_bias's K slice receives sum_d gK
        g[5], g[6], g[0] = bs(g_P, pos), cs(g_P), g_P @ ab(ppw)
        return torch.complex(g_feat[:, :D], g_feat[:, D:]), g


_ATT_SCALE = 32 ** -0.5


def _head_params(head):
    """The head's parameters in the order of the kernels' pointer table: 21 tensors, then 8 per target."""
    fe, pe, at, cn = head.feature_extractor, head.peak_extractor, head.attention, head.confidence_net
    hp = [head.position_encoder, fe[0].weight, fe[0].bias, fe[2].weight, fe[2].bias, head.position_projection.weight,
          head.position_projection.bias, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
          pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias, pe[4].weight, pe[4].bias,
          cn[0].weight, cn[0].bias, cn[2].weight, cn[2].bias]
    for t in range(head.L_max):
        for net in (head.tau_regressor[t], head.f_regressor[t]):
            hp += [net[0].weight, net[0].bias, net[2].weight, net[2].bias]
    return hp


def draw_keep_mask(B, D, p, device, generator=None):
    """The attention dropout's keep mask [B, 4, D], one byte per element, with one framework call: kept with probability
    1 - p.  The kernels scale the kept entries by exactly 1 / (1 - p)."""
    return torch.rand(B, 4, D, device=device, generator=generator) >= p


def _check_keep_mask(keep, B, D):
    if keep is None:
        return
    if not torch.is_tensor(keep) or keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"the keep mask must be a bool or uint8 tensor, got {getattr(keep, 'dtype', type(keep))}")
    if tuple(keep.shape) != (B, 4, D):
        raise ValueError(f"the keep mask must be [{B}, 4, {D}], got {tuple(keep.shape)}")


class _PeakHead(torch.autograd.Function):
    """``_peak_head`` as one function with a hand-written backward (admm_net.py:570-630).  ``keep``: the attention dropout's
    keep mask [B, 4, D] or None; it carries no gradient and is kept for the backward."""

    @staticmethod
    def forward(ctx, phi, keep, p, L, nk, *hp):
        _check_keep_mask(keep, *phi.shape)
        tau, f, conf, saved = nk.head(phi, keep, p, L, hp)
        ctx.save_for_backward(phi, *hp, *saved)
        ctx.keep, ctx.p, ctx.L, ctx.nk, ctx.nhp = keep, p, L, nk, len(hp)
        return tau, f, conf

    @staticmethod
    def backward(ctx, g_tau, g_f, g_conf):
        phi, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        hp, saved = rest[:ctx.nhp], rest[ctx.nhp:]
        g_phi, g = ctx.nk.head_bwd(g_tau, g_f, g_conf, phi, ctx.keep, ctx.p, ctx.L, hp, saved)
        return (g_phi, None, None, None, None, *g)


def _peak_head_native(head, phi, nk, keep=None):
    """The head on the native route.  In train mode with dropout p > 0 the keep mask is drawn here unless given."""
    p = float(head.attention.dropout)
    if keep is None and head.training and p > 0:
        keep = draw_keep_mask(phi.shape[0], phi.shape[1], p, phi.device)
    return _PeakHead.apply(phi, keep, p, head.L_max, nk, *_head_params(head))


class _HLayerStep(torch.autograd.Function):
    """``_h_layer`` on the gathered diagonals as one function, correction_net inside (admm_net.py:134-194); sigma carries no
    gradient.  The tape keeps t, a1 and m."""

    @staticmethod
    def forward(ctx, g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2, nk):
        h, t, a1, m = nk.hlayer(g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2)
        ctx.save_for_backward(z_dg, sigma, rho, pw, W1, W2, t, a1, m)
        ctx.nk = nk
        return h

    @staticmethod
    def backward(ctx, g_h):
        g_gdg, g_zdg, g_rho, g_pw, gW1, gb1, gW2, gb2, _, _ = ctx.nk.hlayer_bwd(g_h, *ctx.saved_tensors)
        return g_gdg, g_zdg, None, g_rho, g_pw, gW1, gb1, gW2, gb2, None


def _resolve_rinv(model, K):
    """``1 / (softplus(rho) + eps)`` of gLayers[k], k < K - 1, evaluated once on the stacked rhos (differentiable): [K - 1]."""
    return 1.0 / (F.softplus(torch.stack([model.gLayers[k].rho for k in range(K - 1)])) + EPS)


def _net_params(net):
    """(W1, b1, W2, b2) of a Linear - ReLU - Linear - Sigmoid (or Tanh) module."""
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
    """admm_net.py:79-105: the phi layer reads the border columns of G and Z only."""
    return _phi_layer_gathered(layer, y, b, G[:, :-1, -1], Z[:, :-1, -1])


def _phi_layer_gathered(layer, y, b, g_col, z_col):
    """``_phi_layer`` on the border columns of G and Z (slices on the tensor route, gathered vectors on the fused one)."""
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


def _g_layer(layer, phi, h, Z, solver, asm, lk=None, sk=None, corner=None, rinv=None):
    """admm_net.py:237-354.  ``lk``: layer kernels of the fused route (None: tensor operations); ``sk``: small kernels of the
    full route; ``corner``: the detached corner value where the caller has resolved it already; ``rinv``: likewise
    ``1 / (softplus(rho) + eps)`` (the native route evaluates it for all layers at once)."""
    if corner is None:
        corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
    if lk is None:
        A = _block_matrix(phi, h, corner) - (1.0 / (F.softplus(layer.rho) + EPS)) * Z
        A = 0.5 * (A + A.transpose(1, 2).conj())
    else:
        A = _LayerMatrix.apply(phi, h, Z, 1.0 / (F.softplus(layer.rho) + EPS) if rinv is None else rinv, corner, lk)
    w, V = _EighValuesOnly.apply(A, solver, asm)
    # learned eigenvalue map, every eigenvalue through the same 1 -> 16 -> 1 network (admm_net.py:310-334)
    if sk is None:
        wp = F.softplus(w - torch.sigmoid(layer.threshold)) * layer.value_net(w.abs().unsqueeze(-1)).squeeze(-1)
    else:
        wp = _EigMap.apply(w, layer.threshold, *_net_params(layer.value_net), sk)
    if lk is not None:
        return _RebuildGather.apply(V, wp, asm, lk)       # (G, G[:, :D, D], Re diag G)
    return _Rebuild.apply(V, wp, asm)


def _group_mean(rn: torch.Tensor, sub_batch: Optional[int], reducer: Optional[Callable] = None) -> torch.Tensor:
    """The batch mean of admm_net.py:459 for every signal: over the whole call, or over its group of ``sub_batch``
    consecutive signals (the last group may be shorter).  ``reducer`` (see ``unrolled_forward``): the mean over the signals of
    all ranks, the float64 quotient rounded to the dtype of ``rn``."""
    B = rn.shape[0]
    if reducer is not None:
        total, count = _ReducedSum.apply(rn, reducer)
        return (total / count).to(rn.dtype)
    if sub_batch is None or sub_batch >= B:
        return rn.mean()
    gid = torch.arange(B, device=rn.device) // sub_batch
    sums = torch.zeros(int(gid[-1]) + 1, dtype=rn.dtype, device=rn.device).index_add(0, gid, rn)
    return (sums / torch.bincount(gid).to(rn.dtype))[gid]


def _z_layer(layer, k, phi, h, G, Z, sub_batch=None, lk=None, sk=None, corner=None, reducer=None):
    """admm_net.py:388-474.  ``lk``, ``sk``, ``corner``: as for ``_g_layer``; ``reducer``: as for ``unrolled_forward``.  Residual
    norm and update follow ``lk``, the step size between them follows ``sk``."""
    if corner is None:
        corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + EPS)).item()
    if lk is None:
        R = G - _block_matrix(phi, h, corner)
        rn = torch.linalg.matrix_norm(R)                               # Frobenius, [B]
    else:
        rn = _ResidualNorm.apply(G, phi, h, corner, lk)
    if sk is None:
        rho, B = F.softplus(layer.rho), rn.shape[0]
        feat = torch.stack([torch.full((B,), k / 10.0, device=rn.device),
                            torch.full((B,), rho.item(), device=rn.device),
                            rn / (_group_mean(rn, sub_batch, reducer) + EPS)], dim=1)
        step = rho * (0.5 + 1.5 * layer.residual_scale_net(feat)).squeeze(1)
    else:
        step = _StepSize.apply(rn, layer.rho, *_net_params(layer.residual_scale_net), k / 10.0, sub_batch, sk, reducer)
    return Z + step.reshape(-1, 1, 1) * R if lk is None else _StateUpdate.apply(Z, G, phi, h, step, corner, lk)


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


# ---- the four steps of a layer.  ``r``: what ``unrolled_forward`` resolved its arguments to (kernel sets that are None where the
# route does not use them); ``s``: the running state G, Z and, with layer kernels, their gathered border columns and diagonals
def _phi_step(r, s, layer, y, b):
    if r.sk is not None:
        return _PhiStep.apply(y, b, s.g_col, s.z_col, layer.rho, r.sk)
    if r.lk is not None:
        return _phi_layer_gathered(layer, y, b, s.g_col, s.z_col)
    return _phi_layer(layer, y, b, s.G, s.Z)


def _h_step(r, s, layer, sigma):
    if r.nk is not None:
        return _HLayerStep.apply(s.g_dg, s.z_dg, sigma, layer.rho, layer.projection_weight, *_net_params(layer.correction_net), r.nk)
    if r.sk is not None:
        t = _HInput.apply(s.g_dg, s.z_dg, layer.rho, r.sk)
        return _HProject.apply(t, layer.correction_net(t), sigma, layer.projection_weight, r.sk)
    return _h_layer(layer, s.G, s.Z, sigma, None if r.lk is None else (s.g_dg, s.z_dg))


def _g_step(r, s, layer, k, phi, h):
    out = _g_layer(layer, phi, h, s.Z, r.solver, r.asm, r.lk, r.sk, r.corners[k][0], r.rinv[k])
    if r.lk is None:
        s.G = out
    else:
        s.G, s.g_col, s.g_dg = out


def _z_step(r, s, layer, k, phi, h):
    s.Z = _z_layer(layer, k, phi, h, s.G, s.Z, r.sub_batch, r.lk, r.sk, r.corners[k][1], r.reducer)
    if r.lk is not None:
        s.z_col, s.z_dg = _Gather.apply(s.Z, r.lk)


def unrolled_forward(model, y: torch.Tensor, b: torch.Tensor, sigma: torch.Tensor,
                     solver: Optional[Callable] = None, assembler=None, sub_batch: Optional[int] = None,
                     fused: bool = False, layer_kernels=None, small: bool = False, small_kernels=None,
                     native: bool = False, native_kernels=None, reducer: Optional[Callable] = None):
    """Differentiable K-layer forward on the device of ``y`` (admm_net.py:742-764 / 791-816).

    The flags ``fused`` ⊂ ``small`` ⊂ ``native`` and the ``*_kernels`` stand-ins are what ``route_kwargs(model.train_route,
    kernels)`` returns; a stand-in without its flag, or a flag without the one below it, raises ``ValueError``.  The arguments
    are resolved once; the layer loop below is the same for every route, and the step functions choose the form.

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
    ``native = True`` (needs ``small = True``) evaluates every H layer, its ``correction_net`` included, through
    ``native_kernels`` (default ``NativeKernels``, the HIP kernels of csrc/train_hlayer.hip; the CPU tests pass
    ``TorchNativeKernels``), the G layers' ``1 / (softplus(rho) + eps)`` once per forward on the stacked rhos, and the head of
    ``ADMMNet`` through ``_PeakHead`` (csrc/train_head.hip).
    ``reducer(t) -> t`` all-reduces (sum) a small float64 tensor across the ranks of a batch-sharded step
    (``sharded.ShardedTraining``): the mean of every Z layer is then over the signals of ALL ranks, one reduction of a
    (sum, count) pair per live layer (K - 1) in the forward and one of a scalar per live layer in the backward.  None (default):
    the call is the whole batch and no reduction runs.  Not combined with ``sub_batch``: groups never span ranks.
    Returns phi, or (tau, f, confidences, phi) when the model has a PeakSearchLayer.
    """
    if sub_batch is not None and sub_batch < 1:
        raise ValueError(f"sub_batch must be None or >= 1, got {sub_batch}")
    if reducer is not None and sub_batch is not None:
        raise ValueError("reducer and sub_batch exclude each other: a sub-batch never spans ranks")
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
    if native and not small:
        raise ValueError("native=True needs small=True")
    if native_kernels is not None and not native:
        raise ValueError("native_kernels is only used with native=True")
    nk = (NativeKernels if native_kernels is None else native_kernels) if native else None
    K, D = model.num_layers, model.M * model.N
    if y.dim() != 2 or y.shape[1] != D or b.shape != y.shape:
        raise ValueError(f"y, b must be [B, {D}] complex; got {tuple(y.shape)}, {tuple(b.shape)}")
    y = y.to(torch.complex64)
    b = b.to(torch.complex64)
    sigma = sigma.to(torch.float32).reshape(-1)
    B, n = y.shape[0], D + 1
    # the phi and H layers read only the border column and the diagonal of G and Z: with layer kernels, gathered once per layer
    col = None if lk is None else torch.zeros(B, D, dtype=torch.complex64, device=y.device)
    dg = None if lk is None else torch.zeros(B, D, dtype=torch.float32, device=y.device)
    s = SimpleNamespace(G=torch.zeros(B, n, n, dtype=torch.complex64, device=y.device), g_col=col, z_col=col, g_dg=dg, z_dg=dg)
    s.Z = torch.zeros_like(s.G)
    # what the call resolved to.  Per layer (corner_g, corner_z) and rinv; None: the layer evaluates it itself
    r = SimpleNamespace(solver=solver, asm=asm, lk=lk, sk=sk, nk=nk, sub_batch=sub_batch, reducer=reducer,
                        corners=_resolve_corners(model, K) if sk is not None else [(None, None)] * K,
                        rinv=_resolve_rinv(model, K) if nk is not None and K > 1 else [None] * K)
    phi = None
    for k in range(K):
        phi = _phi_step(r, s, model.phiLayers[k], y, b)
        if k == K - 1:
            break
        h = _h_step(r, s, model.hLayers[k], sigma)
        _g_step(r, s, model.gLayers[k], k, phi, h)
        _z_step(r, s, model.zLayers[k], k, phi, h)
    if getattr(model, "_HAS_HEAD", False):
        if nk is not None:
            tau, f, conf = _peak_head_native(model.peakSearchLayer, phi, nk)
        else:
            tau, f, conf = _peak_head(model.peakSearchLayer, phi)
        return tau, f, conf, phi
    return phi
