"""Thin torch wrappers over the building-block entry points of include/admmnet.h.

Every function takes CUDA (HIP) tensors, enqueues on the current stream and
returns device tensors.  No CPU path exists.

Tensor inputs: an input in any form -- strided, lazily conjugated or negated, of a wider dtype, part
of a graph, unaligned -- gives the bits of the call on the plain tensor of the same value (``_plain``); an in-place or
caller-owned argument is never copied and refuses what the kernel could not write faithfully (``_no_lazy_bits`` and the
checks around it).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import Cfg


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise _lib.AdmmNetError(f"{name} must be a HIP device tensor (no CPU fallback)")


def eigh(A: torch.Tensor, options=None):
    """Batched Hermitian eigendecomposition (torch.linalg.eigh at admm_net.py:303).

    A: [B, n, n] complex64 (lower triangle read).  Returns (w [B, n] unsorted, V [B, n, n]).
    options: an ``admm_net_amd.Options`` choosing the eigensolver variant for this call (None = the process defaults).
    """
    _need_cuda(A, "A")
    lib = _lib.load()
    A = _c64(A, A.device, None, "A")
    B, n, _ = A.shape
    dev = A.device
    with torch.cuda.device(dev):
        handle = 0 if options is None else options.handle
        need = lib.admmnet_eigh_workspace_bytes_o(n, B, handle)
        if need < 0:
            raise _lib.AdmmNetError(f"eigh: unsupported n={n}")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        w = torch.empty(B, n, dtype=torch.float32, device=dev)
        V = torch.empty(B, n, n, dtype=torch.complex64, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_eigh_c64_o(n, B, _ptr(A), _ptr(w), _ptr(V), _ptr(ws), need, _ptr(status),
                                          _stream(dev), handle), "admmnet_eigh_c64")
        bad = int(status[0].item())
        if bad:
            raise _lib.AdmmNetError(f"eigensolver failed on {bad} matrices")
    return w, V


def vdvh(V: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """out = V diag(d) V^H, exactly Hermitian (admm_net.py:336-354; backward of the eigenvalue-only eigh, :303-306).

    V: [B, n, n] complex64 (columns = eigenvectors), d: [B, n] float32.  Returns [B, n, n] complex64."""
    _need_cuda(V, "V")
    lib = _lib.load()
    V = _c64(V, V.device, None, "V")
    B, n, _ = V.shape
    d = _f32(d, V.device, (B, n), "d")
    with torch.cuda.device(V.device):
        out = torch.empty_like(V)
        _lib.check(lib.admmnet_vdvh_c64(n, B, _ptr(V), _ptr(d), _ptr(out), _stream(V.device)), "admmnet_vdvh_c64")
    return out


def vhsv(V: torch.Tensor, S: torch.Tensor) -> torch.Tensor:
    """q[b, c] = Re(v_c^H S v_c) for Hermitian S (lower triangle read): the adjoint of ``vdvh`` with respect to d.

    V, S: [B, n, n] complex64.  Returns [B, n] float32."""
    _need_cuda(V, "V")
    lib = _lib.load()
    V = _c64(V, V.device, None, "V")
    B, n, _ = V.shape
    S = _c64(S, V.device, V.shape, "S")
    with torch.cuda.device(V.device):
        q = torch.empty(B, n, dtype=torch.float32, device=V.device)
        _lib.check(lib.admmnet_vhsv_f32(n, B, _ptr(V), _ptr(S), _ptr(q), _stream(V.device)), "admmnet_vhsv_f32")
    return q


# ---- training route: the n^2-sized steps of one layer (csrc/train_layer.hip) --------------------------------------------------
# C(phi, h, c) = [[diag h, phi], [phi^H, c]], herm(X) = (X + X^H) / 2.  Matrices [B, n, n] complex64, phi [B, D] complex64,
# h [B, D] float32 (D = n - 1); r (0-dim) and s [B] are float32 DEVICE tensors, corner a Python float.
def _plain(t, dev, dtype, shape, name):
    """THE place a caller's input tensor becomes what a kernel may read through ``data_ptr()``: detached, on ``dev``, of
    ``dtype``, with the conj and the neg bit resolved (both survive ``.to`` of the same dtype, ``.detach()`` and
    ``.contiguous()``, and the memory behind them holds the conjugate / the negative) and contiguous.  A tensor that is all of
    that already comes back as it is, without a copy.  The memory is 16-byte aligned, as a fresh allocation is: the streaming
    kernels of csrc/train_layer.hip choose their vector path, and with it the order of their sums, by the pointers' alignment,
    so a contiguous view one element into a buffer would otherwise give other bits than its own copy.  ``shape``: checked
    unless None."""
    t = t.detach()
    if not (t.dtype == dtype and t.device == dev and t.is_contiguous() and t.data_ptr() % 16 == 0) or t.is_conj() or t.is_neg():
        t = t.to(device=dev, dtype=dtype).resolve_conj().resolve_neg().contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _c64(t, dev, shape=None, name="tensor"):
    return _plain(t, dev, torch.complex64, shape, name)


def _f32(t, dev, shape=None, name="tensor"):
    return _plain(t, dev, torch.float32, shape, name)


def _num(t, dev, dtype, shape=None, name="tensor"):
    """``_plain`` for the inputs the kernels read as float64 or as integers (grids, images, counts, masks)."""
    return _plain(t, dev, dtype, shape, name)


def _no_lazy_bits(t, what):
    """Refuses a tensor a kernel is to WRITE (or reads without a copy) whose conj or neg bit is set: its memory holds the
    conjugate / the negative of its value, and resolving the bit would hand the kernel a copy."""
    if t.is_conj() or t.is_neg():
        raise ValueError(f"{what} is a lazily {'conjugated' if t.is_conj() else 'negated'} view (its memory holds the "
                         f"{'conjugate' if t.is_conj() else 'negative'} of its value); pass a resolved tensor")


def _train_args(M, name):
    """(lib, device, B, n) of a [B, n, n] matrix batch."""
    _need_cuda(M, name)
    if M.dim() != 3 or M.shape[1] != M.shape[2]:
        raise ValueError(f"{name} must be [B, n, n], got {tuple(M.shape)}")
    return _lib.load(), M.device, M.shape[0], M.shape[1]


def train_matrix(phi, h, Z, r, corner: float) -> torch.Tensor:
    """A = herm(C(phi, h, corner) - r Z), exactly Hermitian: GLayer's block matrix, ``- Z / rho`` and symmetrisation
    (admm_net.py:262-300)."""
    lib, dev, B, n = _train_args(Z, "Z")
    with torch.cuda.device(dev):
        Z, phi, h, r = _c64(Z, dev, (B, n, n), "Z"), _c64(phi, dev, (B, n - 1), "phi"), _f32(h, dev, (B, n - 1), "h"), _f32(r, dev, (), "r")
        A = torch.empty_like(Z)
        _lib.check(lib.admmnet_train_matrix_f32(n, B, _ptr(phi), _ptr(h), _ptr(Z), _ptr(r), float(corner), _ptr(A), _stream(dev)),
                   "admmnet_train_matrix_f32")
    return A


def train_matrix_bwd(gA, Z, r):
    """Backward of ``train_matrix`` with S = herm(gA): returns (g_phi = 2 S[:, :D, D], g_h = Re diag S, gZ = -r S,
    g_r = -sum_b <S_b, Z_b> as a 0-dim tensor)."""
    lib, dev, B, n = _train_args(gA, "gA")
    with torch.cuda.device(dev):
        gA, Z, r = _c64(gA, dev, (B, n, n), "gA"), _c64(Z, dev, (B, n, n), "Z"), _f32(r, dev, (), "r")
        gZ = torch.empty_like(gA)
        g_phi = torch.empty(B, n - 1, dtype=torch.complex64, device=dev)
        g_h = torch.empty(B, n - 1, dtype=torch.float32, device=dev)
        g_r = torch.empty((), dtype=torch.float32, device=dev)
        part = torch.empty(lib.admmnet_train_partials(n, B), dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_matrix_bwd_f32(n, B, _ptr(gA), _ptr(Z), _ptr(r), _ptr(gZ), _ptr(g_phi), _ptr(g_h), _ptr(g_r),
                                                    _ptr(part), _stream(dev)), "admmnet_train_matrix_bwd_f32")
    return g_phi, g_h, gZ, g_r


def train_resnorm(G, phi, h, corner: float) -> torch.Tensor:
    """rn[b] = ||G_b - C(phi, h, corner)||_F without storing the residual (admm_net.py:428-459).  Returns [B] float32."""
    lib, dev, B, n = _train_args(G, "G")
    with torch.cuda.device(dev):
        G, phi, h = _c64(G, dev, (B, n, n), "G"), _c64(phi, dev, (B, n - 1), "phi"), _f32(h, dev, (B, n - 1), "h")
        rn = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_resnorm_f32(n, B, _ptr(G), _ptr(phi), _ptr(h), float(corner), _ptr(rn), _stream(dev)),
                   "admmnet_train_resnorm_f32")
    return rn


def train_resnorm_bwd(g_rn, rn, G, phi, h, corner: float):
    """Backward of ``train_resnorm`` with q = g_rn / rn, R = G - C: returns (gG = q R, g_phi = -q (R[:, :D, D] +
    conj R[:, D, :D]), g_h = -q Re diag R)."""
    lib, dev, B, n = _train_args(G, "G")
    with torch.cuda.device(dev):
        G, phi, h = _c64(G, dev, (B, n, n), "G"), _c64(phi, dev, (B, n - 1), "phi"), _f32(h, dev, (B, n - 1), "h")
        g_rn, rn = _f32(g_rn, dev, (B,), "g_rn"), _f32(rn, dev, (B,), "rn")
        gG = torch.empty_like(G)
        g_phi = torch.empty(B, n - 1, dtype=torch.complex64, device=dev)
        g_h = torch.empty(B, n - 1, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_resnorm_bwd_f32(n, B, _ptr(g_rn), _ptr(rn), _ptr(G), _ptr(phi), _ptr(h), float(corner),
                                                     _ptr(gG), _ptr(g_phi), _ptr(g_h), _stream(dev)),
                   "admmnet_train_resnorm_bwd_f32")
    return gG, g_phi, g_h


def train_zupdate(Z, G, phi, h, s, corner: float) -> torch.Tensor:
    """Z + s_b (G - C(phi, h, corner)): the dual update (admm_net.py:460-474)."""
    lib, dev, B, n = _train_args(Z, "Z")
    with torch.cuda.device(dev):
        Z, G = _c64(Z, dev, (B, n, n), "Z"), _c64(G, dev, (B, n, n), "G")
        phi, h, s = _c64(phi, dev, (B, n - 1), "phi"), _f32(h, dev, (B, n - 1), "h"), _f32(s, dev, (B,), "s")
        Zn = torch.empty_like(Z)
        _lib.check(lib.admmnet_train_zupdate_c64(n, B, _ptr(Z), _ptr(G), _ptr(phi), _ptr(h), _ptr(s), float(corner), _ptr(Zn),
                                                 _stream(dev)), "admmnet_train_zupdate_c64")
    return Zn


def train_zupdate_bwd(g, G, phi, h, s, corner: float):
    """Backward of ``train_zupdate`` from g (the gradient of Z is g itself): returns (gG = s g, g_phi = -s (g[:, :D, D] +
    conj g[:, D, :D]), g_h = -s Re diag g, g_s[b] = <R_b, g_b>)."""
    lib, dev, B, n = _train_args(g, "g")
    with torch.cuda.device(dev):
        g, G = _c64(g, dev, (B, n, n), "g"), _c64(G, dev, (B, n, n), "G")
        phi, h, s = _c64(phi, dev, (B, n - 1), "phi"), _f32(h, dev, (B, n - 1), "h"), _f32(s, dev, (B,), "s")
        gG = torch.empty_like(G)
        g_phi = torch.empty(B, n - 1, dtype=torch.complex64, device=dev)
        g_h = torch.empty(B, n - 1, dtype=torch.float32, device=dev)
        g_s = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_zupdate_bwd_c64(n, B, _ptr(g), _ptr(G), _ptr(phi), _ptr(h), _ptr(s), float(corner), _ptr(gG),
                                                     _ptr(g_phi), _ptr(g_h), _ptr(g_s), _stream(dev)),
                   "admmnet_train_zupdate_bwd_c64")
    return gG, g_phi, g_h, g_s


def train_gather(X):
    """(X[:, :D, D], Re diag X[:, :D]): all that the phi layer (admm_net.py:98-99) and the H layer (:150-152) read of G and
    Z.  Returns ([B, D] complex64, [B, D] float32)."""
    lib, dev, B, n = _train_args(X, "X")
    with torch.cuda.device(dev):
        X = _c64(X, dev, (B, n, n), "X")
        col = torch.empty(B, n - 1, dtype=torch.complex64, device=dev)
        dg = torch.empty(B, n - 1, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_gather_c64(n, B, _ptr(X), _ptr(col), _ptr(dg), _stream(dev)), "admmnet_train_gather_c64")
    return col, dg


def train_scatter(g_col, g_dg) -> torch.Tensor:
    """Backward of ``train_gather``: the [B, n, n] matrix with g_col in the border column, g_dg on the diagonal (rows < D)
    and zeros elsewhere."""
    _need_cuda(g_col, "g_col")
    lib, dev = _lib.load(), g_col.device
    B, D = g_col.shape
    with torch.cuda.device(dev):
        g_col, g_dg = _c64(g_col, dev, (B, D), "g_col"), _f32(g_dg, dev, (B, D), "g_dg")
        gX = torch.empty(B, D + 1, D + 1, dtype=torch.complex64, device=dev)
        _lib.check(lib.admmnet_train_scatter_c64(D + 1, B, _ptr(g_col), _ptr(g_dg), _ptr(gX), _stream(dev)),
                   "admmnet_train_scatter_c64")
    return gX


def train_herm(g, g_col=None, g_dg=None) -> torch.Tensor:
    """herm(g + E) with E = ``train_scatter(g_col, g_dg)`` (E = 0 when both are None), exactly Hermitian: the symmetrisation
    in the backward of the rebuild (admm_net.py:354) with the gather's gradient folded in."""
    lib, dev, B, n = _train_args(g, "g")
    if (g_col is None) != (g_dg is None):
        raise ValueError("g_col and g_dg go together")
    with torch.cuda.device(dev):
        g = _c64(g, dev, (B, n, n), "g")
        if g_col is not None:
            g_col, g_dg = _c64(g_col, dev, (B, n - 1), "g_col"), _f32(g_dg, dev, (B, n - 1), "g_dg")
        S = torch.empty_like(g)
        _lib.check(lib.admmnet_train_herm_c64(n, B, _ptr(g), _ptr(g_col), _ptr(g_dg), _ptr(S), _stream(dev)),
                   "admmnet_train_herm_c64")
    return S


# ---- training route "full": the O(B D)-sized steps of one layer (csrc/train_small.hip) ---------------------------------------
# [B, D] tensors complex64 / float32; every parameter (rho, projection_weight, threshold, the two small networks) is handed
# over as the RAW device tensor -- the kernels apply softplus / sigmoid and the ``_bwd`` forms return raw-parameter gradients.
_TS_PHI, _TS_HINPUT, _TS_HPROJECT, _TS_EIGMAP, _TS_STEPSIZE = range(5)


def _small_args(x, name):
    """(lib, device, B, D) of a [B, D] tensor."""
    _need_cuda(x, name)
    if x.dim() != 2:
        raise ValueError(f"{name} must be [B, D], got {tuple(x.shape)}")
    return _lib.load(), x.device, x.shape[0], x.shape[1]


def _small_partials(lib, step, B, dev, sub_batch=0):
    need = lib.admmnet_train_small_partials(step, B, sub_batch)
    if need < 0:
        raise _lib.AdmmNetError(f"train_small: bad size (B={B}, sub_batch={sub_batch})")
    return torch.empty(need, dtype=torch.float32, device=dev)


def _net(dev, W1, b1, W2, b2, hidden, fan_in):
    return (_f32(W1, dev, (hidden, fan_in), "W1"), _f32(b1, dev, (hidden,), "b1"), _f32(W2, dev, (1, hidden), "W2"),
            _f32(b2, dev, (1,), "b2"))


def train_phi(y, b, g_col, z_col, rho) -> torch.Tensor:
    """phi = bs / (1 + r bs) (y / (b + eps) + r g_col + z_col) with r = softplus(rho), bs = |b|^2 + eps (admm_net.py:79-105)."""
    lib, dev, B, D = _small_args(y, "y")
    with torch.cuda.device(dev):
        y, b, g_col, z_col = (_c64(t, dev, (B, D), nm) for t, nm in ((y, "y"), (b, "b"), (g_col, "g_col"), (z_col, "z_col")))
        rho = _f32(rho, dev, (), "rho")
        phi = torch.empty_like(y)
        _lib.check(lib.admmnet_train_phi_c64(D, B, _ptr(y), _ptr(b), _ptr(g_col), _ptr(z_col), _ptr(rho), _ptr(phi), _stream(dev)),
                   "admmnet_train_phi_c64")
    return phi


def train_phi_bwd(g_phi, y, b, g_col, z_col, rho):
    """Backward of ``train_phi``: returns (g_gcol, g_zcol [B, D] complex64, g_rho 0-dim, for the raw rho)."""
    lib, dev, B, D = _small_args(g_phi, "g_phi")
    with torch.cuda.device(dev):
        g_phi, y, b, g_col, z_col = (_c64(t, dev, (B, D), nm) for t, nm in ((g_phi, "g_phi"), (y, "y"), (b, "b"), (g_col, "g_col"),
                                                                           (z_col, "z_col")))
        rho = _f32(rho, dev, (), "rho")
        g_gcol, g_zcol = torch.empty_like(y), torch.empty_like(y)
        g_rho = torch.empty((), dtype=torch.float32, device=dev)
        part = _small_partials(lib, _TS_PHI, B, dev)
        _lib.check(lib.admmnet_train_phi_bwd_c64(D, B, _ptr(g_phi), _ptr(y), _ptr(b), _ptr(g_col), _ptr(z_col), _ptr(rho),
                                                 _ptr(g_gcol), _ptr(g_zcol), _ptr(g_rho), _ptr(part), _stream(dev)),
                   "admmnet_train_phi_bwd_c64")
    return g_gcol, g_zcol, g_rho


def train_hinput(g_dg, z_dg, rho) -> torch.Tensor:
    """t = g_dg + z_dg / (softplus(rho) + eps): the H layer's input from the two real diagonals (admm_net.py:150-152)."""
    lib, dev, B, D = _small_args(g_dg, "g_dg")
    with torch.cuda.device(dev):
        g_dg, z_dg, rho = _f32(g_dg, dev, (B, D), "g_dg"), _f32(z_dg, dev, (B, D), "z_dg"), _f32(rho, dev, (), "rho")
        t = torch.empty_like(g_dg)
        _lib.check(lib.admmnet_train_hinput_f32(D, B, _ptr(g_dg), _ptr(z_dg), _ptr(rho), _ptr(t), _stream(dev)),
                   "admmnet_train_hinput_f32")
    return t


def train_hinput_bwd(g_t, z_dg, rho):
    """Backward of ``train_hinput``: returns (g_gdg, g_zdg [B, D], g_rho 0-dim)."""
    lib, dev, B, D = _small_args(g_t, "g_t")
    with torch.cuda.device(dev):
        g_t, z_dg, rho = _f32(g_t, dev, (B, D), "g_t"), _f32(z_dg, dev, (B, D), "z_dg"), _f32(rho, dev, (), "rho")
        g_gdg, g_zdg = torch.empty_like(g_t), torch.empty_like(g_t)
        g_rho = torch.empty((), dtype=torch.float32, device=dev)
        part = _small_partials(lib, _TS_HINPUT, B, dev)
        _lib.check(lib.admmnet_train_hinput_bwd_f32(D, B, _ptr(g_t), _ptr(z_dg), _ptr(rho), _ptr(g_gdg), _ptr(g_zdg), _ptr(g_rho),
                                                    _ptr(part), _stream(dev)), "admmnet_train_hinput_bwd_f32")
    return g_gdg, g_zdg, g_rho


def train_hproject(t, m, sigma, pw) -> torch.Tensor:
    """h = tc s with tc = t + 0.1 m, c = A max|tc| + sum tc, A = 2 sqrt(D) sigma + sigma^2, s = min(sigmoid(pw) / (c + eps), 1)
    (admm_net.py:160-194); m = correction_net(t)."""
    lib, dev, B, D = _small_args(t, "t")
    with torch.cuda.device(dev):
        t, m, sigma, pw = _f32(t, dev, (B, D), "t"), _f32(m, dev, (B, D), "m"), _f32(sigma, dev, (B,), "sigma"), _f32(pw, dev, (), "pw")
        h = torch.empty_like(t)
        _lib.check(lib.admmnet_train_hproject_f32(D, B, _ptr(t), _ptr(m), _ptr(sigma), _ptr(pw), _ptr(h), _stream(dev)),
                   "admmnet_train_hproject_f32")
    return h


def train_hproject_bwd(g_h, t, m, sigma, pw):
    """Backward of ``train_hproject``: returns (g_t, g_m [B, D], g_pw 0-dim)."""
    lib, dev, B, D = _small_args(g_h, "g_h")
    with torch.cuda.device(dev):
        g_h, t, m = _f32(g_h, dev, (B, D), "g_h"), _f32(t, dev, (B, D), "t"), _f32(m, dev, (B, D), "m")
        sigma, pw = _f32(sigma, dev, (B,), "sigma"), _f32(pw, dev, (), "pw")
        g_t, g_m = torch.empty_like(t), torch.empty_like(t)
        g_pw = torch.empty((), dtype=torch.float32, device=dev)
        part = _small_partials(lib, _TS_HPROJECT, B, dev)
        _lib.check(lib.admmnet_train_hproject_bwd_f32(D, B, _ptr(g_h), _ptr(t), _ptr(m), _ptr(sigma), _ptr(pw), _ptr(g_t), _ptr(g_m),
                                                      _ptr(g_pw), _ptr(part), _stream(dev)), "admmnet_train_hproject_bwd_f32")
    return g_t, g_m, g_pw


def _correction_net(dev, D, W1, b1, W2, b2):
    return (_f32(W1, dev, (64, D), "W1"), None if b1 is None else _f32(b1, dev, (64,), "b1"), _f32(W2, dev, (D, 64), "W2"),
            None if b2 is None else _f32(b2, dev, (D,), "b2"))


def train_hlayer(g_dg, z_dg, sigma, rho, pw, W1, b1, W2, b2):
    """The whole H layer, ``train_hinput`` -> correction_net -> ``train_hproject`` in one kernel (csrc/train_hlayer.hip;
    admm_net.py:134-194): t = g_dg + z_dg / (softplus(rho) + eps), a1 = relu(W1 t + b1), m = tanh(W2 a1 + b2), h from
    tc = t + 0.1 m.  W1 [64, D], b1 [64], W2 [D, 64], b2 [D] are correction_net's RAW parameters.  Returns (h, t, a1, m);
    t, m [B, D] and a1 [B, 64] are what ``train_hlayer_bwd`` reads."""
    lib, dev, B, D = _small_args(g_dg, "g_dg")
    with torch.cuda.device(dev):
        g_dg, z_dg, sigma = _f32(g_dg, dev, (B, D), "g_dg"), _f32(z_dg, dev, (B, D), "z_dg"), _f32(sigma, dev, (B,), "sigma")
        rho, pw = _f32(rho, dev, (), "rho"), _f32(pw, dev, (), "pw")
        W1, b1, W2, b2 = _correction_net(dev, D, W1, b1, W2, b2)
        h, t, m = torch.empty_like(g_dg), torch.empty_like(g_dg), torch.empty_like(g_dg)
        a1 = torch.empty(B, 64, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_hlayer_f32(D, B, _ptr(g_dg), _ptr(z_dg), _ptr(sigma), _ptr(rho), _ptr(pw), _ptr(W1), _ptr(b1),
                                                _ptr(W2), _ptr(b2), _ptr(h), _ptr(t), _ptr(a1), _ptr(m), _stream(dev)),
                   "admmnet_train_hlayer_f32")
    return h, t, a1, m


def train_hlayer_bwd(g_h, z_dg, sigma, rho, pw, W1, W2, t, a1, m):
    """Backward of ``train_hlayer``: returns (g_gdg, g_zdg [B, D], g_rho, g_pw 0-dim, gW1 [64, D], gb1 [64], gW2 [D, 64],
    gb2 [D], delta1 [B, 64], delta2 [B, D]) -- the deltas are the pre-activation gradients whose batch-reduced products with
    t and a1 the weight gradients are."""
    lib, dev, B, D = _small_args(g_h, "g_h")
    with torch.cuda.device(dev):
        g_h, z_dg, sigma = _f32(g_h, dev, (B, D), "g_h"), _f32(z_dg, dev, (B, D), "z_dg"), _f32(sigma, dev, (B,), "sigma")
        rho, pw = _f32(rho, dev, (), "rho"), _f32(pw, dev, (), "pw")
        W1, _, W2, _ = _correction_net(dev, D, W1, None, W2, None)
        t, a1, m = _f32(t, dev, (B, D), "t"), _f32(a1, dev, (B, 64), "a1"), _f32(m, dev, (B, D), "m")
        g_gdg, g_zdg, d2 = torch.empty_like(g_h), torch.empty_like(g_h), torch.empty_like(g_h)
        d1 = torch.empty_like(a1)
        gpar = torch.empty(2 + 129 * D + 64, dtype=torch.float32, device=dev)
        need = lib.admmnet_train_hlayer_workspace(D, B)
        if need < 0:
            raise _lib.AdmmNetError(f"train_hlayer_bwd: bad size (D={D}, B={B})")
        work = torch.empty(need // 4, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_hlayer_bwd_f32(D, B, _ptr(g_h), _ptr(z_dg), _ptr(sigma), _ptr(rho), _ptr(pw), _ptr(W1),
                                                    _ptr(W2), _ptr(t), _ptr(a1), _ptr(m), _ptr(g_gdg), _ptr(g_zdg), _ptr(d1),
                                                    _ptr(d2), _ptr(gpar), _ptr(work), _stream(dev)),
                   "admmnet_train_hlayer_bwd_f32")
    o = 2 + 64 * D
    return (g_gdg, g_zdg, gpar[0], gpar[1], gpar[2:o].view(64, D), gpar[o:o + 64], gpar[o + 64:o + 64 + 64 * D].view(D, 64),
            gpar[o + 64 + 64 * D:], d1, d2)


_HEAD_SAVED, _HEAD_WORK, _HEAD_GRADS = 0, 1, 2                 # ADMMNET_TRAIN_HEAD_* of include/admmnet.h


def _head_shapes(D, L):
    """The shapes of the head's parameters in the order of ``training._head_params`` (the kernels' pointer table)."""
    s = [(D, 2), (128, 2 * D), (128,), (128, 128), (128,), (128, 2), (128,), (384, 128), (384,), (128, 128), (128,),
         (64, 128), (64,), (32, 64), (32,), (16, 32), (16,), (16, 16), (16,), (1, 16), (1,)]
    return s + [(32, 16), (32,), (1, 32), (1,)] * (2 * L)


def _head_args(phi, keep, p, L, hp):
    _need_cuda(phi, "phi")
    if phi.dim() != 2:
        raise ValueError(f"phi must be [B, D], got {tuple(phi.shape)}")
    lib, dev, (B, D) = _lib.load(), phi.device, phi.shape
    shapes = _head_shapes(D, L)
    if len(hp) != len(shapes):
        raise ValueError(f"the head has {len(shapes)} parameters at L = {L}, got {len(hp)}")
    hp = [_f32(t, dev, s, f"head parameter {i}") for i, (t, s) in enumerate(zip(hp, shapes))]
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (B, 4, D):
            raise ValueError(f"keep must be a bool or uint8 [{B}, 4, {D}] tensor, got {keep.dtype} {tuple(keep.shape)}")
        if not 0.0 <= p < 1.0:
            raise ValueError(f"the dropout probability must be in [0, 1), got {p}")
        _need_cuda(keep, "keep")
        keep = _num(keep, dev, keep.dtype, None, "keep")
    table = (ctypes.c_void_p * len(hp))(*[t.data_ptr() for t in hp])
    return lib, dev, B, D, hp, keep, table


def _head_bytes(lib, D, L, B, part):
    need = lib.admmnet_train_head_workspace(D, L, B, part)
    if need < 0:
        raise _lib.AdmmNetError(f"train_head: bad size (D={D}, L={L}, B={B})")
    return need // 4


def train_head(phi, keep, p, L, hp):
    """The PeakSearchLayer head (csrc/train_head.hip; admm_net.py:570-630) on phi [B, D] complex64: returns (tau, f, conf [B, L],
    saved).  ``hp``: the head's RAW parameters in the order of ``training._head_params``; ``keep``: the attention dropout's keep
    mask [B, 4, D] (bool or uint8; applied as a <- a keep / (1 - p) between the softmax and the value product) or None for no
    dropout.  ``saved`` is what ``train_head_bwd`` reads."""
    lib, dev, B, D, hp, keep, table = _head_args(phi, keep, p, L, hp)
    with torch.cuda.device(dev):
        phi = _c64(phi, dev, (B, D), "phi")
        tau, f, conf = (torch.empty(B, L, dtype=torch.float32, device=dev) for _ in range(3))
        act = torch.empty(_head_bytes(lib, D, L, B, _HEAD_SAVED), dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_head_f32(D, L, B, _ptr(phi), table, _ptr(keep), float(p), _ptr(tau), _ptr(f), _ptr(conf),
                                              _ptr(act), _stream(dev)), "admmnet_train_head_f32")
    return tau, f, conf, (act, tau, f, conf)


def train_head_bwd(g_tau, g_f, g_conf, phi, keep, p, L, hp, saved):
    """Backward of ``train_head``: returns (g_phi [B, D] complex64, [the gradient of every tensor of ``hp``]); the gradients are
    views of one buffer."""
    lib, dev, B, D, hp, keep, table = _head_args(phi, keep, p, L, hp)
    act, tau, f, conf = saved
    with torch.cuda.device(dev):
        phi = _c64(phi, dev, (B, D), "phi")
        g_tau, g_f, g_conf = (_f32(t, dev, (B, L), n) for t, n in ((g_tau, "g_tau"), (g_f, "g_f"), (g_conf, "g_conf")))
        tau, f, conf = (_f32(t, dev, (B, L), n) for t, n in ((tau, "tau"), (f, "f"), (conf, "conf")))
        act = _f32(act, dev, (_head_bytes(lib, D, L, B, _HEAD_SAVED),), "saved")
        g_phi = torch.empty(B, D, dtype=torch.complex64, device=dev)
        g = torch.empty(_head_bytes(lib, D, L, B, _HEAD_GRADS), dtype=torch.float32, device=dev)
        work = torch.empty(_head_bytes(lib, D, L, B, _HEAD_WORK), dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_head_bwd_f32(D, L, B, _ptr(g_tau), _ptr(g_f), _ptr(g_conf), _ptr(phi), table, _ptr(keep),
                                                  float(p), _ptr(tau), _ptr(f), _ptr(conf), _ptr(act), _ptr(g_phi), _ptr(g),
                                                  _ptr(work), _stream(dev)), "admmnet_train_head_bwd_f32")
    # the buffer's layout (include/admmnet.h): confidence_net, region A, in_proj, position_projection, position_encoder
    cur = [0]

    def take(*shape):
        n = 1
        for s in shape:
            n *= s
        v = g[cur[0]:cur[0] + n].view(*shape)
        cur[0] += n
        return v

    out = [None] * len(hp)
    out[17], out[18], out[19], out[20] = take(16, 16), take(16), take(1, 16), take(1)
    out[1], out[2], out[3], out[4] = take(128, 2 * D), take(128), take(128, 128), take(128)
    out[9], out[10] = take(128, 128), take(128)
    out[11], out[12], out[13], out[14], out[15], out[16] = take(64, 128), take(64), take(32, 64), take(32), take(16, 32), take(16)
    for t in range(L):
        o = 21 + 8 * t
        out[o], out[o + 4] = take(32, 16), take(32, 16)
        out[o + 1], out[o + 5] = take(32), take(32)
        out[o + 2], out[o + 3], out[o + 6], out[o + 7] = take(1, 32), take(1), take(1, 32), take(1)
    cur[0] += 256 * D                                            # gK, gV: the sums over the batch the token side starts from
    out[7], out[8], out[5], out[6], out[0] = take(384, 128), take(384), take(128, 2), take(128), take(D, 2)
    assert cur[0] == g.numel()
    return g_phi, out


def train_eigmap(w, thr, W1, b1, W2, b2) -> torch.Tensor:
    """wp = softplus(w - sigmoid(thr)) sigmoid(W2 relu(W1 |w| + b1) + b2) over [B, n] (admm_net.py:310-334); W1 [16, 1],
    b1 [16], W2 [1, 16], b2 [1] are value_net's parameters."""
    lib, dev, B, n = _small_args(w, "w")
    with torch.cuda.device(dev):
        w, thr = _f32(w, dev, (B, n), "w"), _f32(thr, dev, (), "thr")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 16, 1)
        wp = torch.empty_like(w)
        _lib.check(lib.admmnet_train_eigmap_f32(n, B, _ptr(w), _ptr(thr), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(wp),
                                                _stream(dev)), "admmnet_train_eigmap_f32")
    return wp


def train_eigmap_bwd(g_wp, w, thr, W1, b1, W2, b2):
    """Backward of ``train_eigmap``: returns (g_w [B, n], g_thr 0-dim, gW1 [16, 1], gb1 [16], gW2 [1, 16], gb2 [1])."""
    lib, dev, B, n = _small_args(g_wp, "g_wp")
    with torch.cuda.device(dev):
        g_wp, w, thr = _f32(g_wp, dev, (B, n), "g_wp"), _f32(w, dev, (B, n), "w"), _f32(thr, dev, (), "thr")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 16, 1)
        g_w = torch.empty_like(w)
        g = torch.empty(50, dtype=torch.float32, device=dev)
        part = _small_partials(lib, _TS_EIGMAP, B, dev)
        _lib.check(lib.admmnet_train_eigmap_bwd_f32(n, B, _ptr(g_wp), _ptr(w), _ptr(thr), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2),
                                                    _ptr(g_w), _ptr(g), _ptr(part), _stream(dev)), "admmnet_train_eigmap_bwd_f32")
    return g_w, g[0], g[1:17].reshape(16, 1), g[17:33], g[33:49].reshape(1, 16), g[49:50]


def train_stepsize(rn, rho, W1, b1, W2, b2, knorm: float, sub_batch=None) -> torch.Tensor:
    """step_b = r (0.5 + 1.5 sigmoid(W2 relu(W1 [knorm, r, u_b] + b1) + b2)) with r = softplus(rho), u_b = rn_b / (mean + eps)
    (admm_net.py:440-474); the mean is over the call or over each group of ``sub_batch`` consecutive signals.  W1 [32, 3],
    b1 [32], W2 [1, 32], b2 [1] are residual_scale_net's parameters."""
    _need_cuda(rn, "rn")
    lib, dev, B = _lib.load(), rn.device, rn.shape[0]
    with torch.cuda.device(dev):
        rn, rho = _f32(rn, dev, (B,), "rn"), _f32(rho, dev, (), "rho")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 32, 3)
        step = torch.empty_like(rn)
        _lib.check(lib.admmnet_train_stepsize_f32(B, int(sub_batch or 0), float(knorm), _ptr(rn), _ptr(rho), _ptr(W1), _ptr(b1),
                                                  _ptr(W2), _ptr(b2), _ptr(step), _stream(dev)), "admmnet_train_stepsize_f32")
    return step


def train_stepsize_bwd(g_step, rn, rho, W1, b1, W2, b2, knorm: float, sub_batch=None):
    """Backward of ``train_stepsize``: returns (g_rn [B] with the coupling through the mean, g_rho 0-dim through the leading
    factor only, gW1 [32, 3], gb1 [32], gW2 [1, 32], gb2 [1])."""
    _need_cuda(g_step, "g_step")
    lib, dev, B = _lib.load(), g_step.device, g_step.shape[0]
    g = int(sub_batch or 0)
    with torch.cuda.device(dev):
        g_step, rn, rho = _f32(g_step, dev, (B,), "g_step"), _f32(rn, dev, (B,), "rn"), _f32(rho, dev, (), "rho")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 32, 3)
        g_rn = torch.empty_like(rn)
        out = torch.empty(162, dtype=torch.float32, device=dev)
        part = _small_partials(lib, _TS_STEPSIZE, B, dev, g)
        _lib.check(lib.admmnet_train_stepsize_bwd_f32(B, g, float(knorm), _ptr(g_step), _ptr(rn), _ptr(rho), _ptr(W1), _ptr(b1),
                                                      _ptr(W2), _ptr(b2), _ptr(g_rn), _ptr(out), _ptr(part), _stream(dev)),
                   "admmnet_train_stepsize_bwd_f32")
    return g_rn, out[0], out[1:97].reshape(32, 3), out[97:129], out[129:161].reshape(1, 32), out[161:162]


# ---- the step size from a mean that comes from outside the call (the sharded training of admm_net_amd/sharded.py) ---------------
# ``pair``: device float64 [2] = (sum of rn, number of signals) of the WHOLE batch; the kernels form the mean themselves.
def _f64(t, dev, numel, name):
    """A dense float64 device tensor of ``numel`` elements, as the kernels read it: no conversion is made, so another dtype or
    device and a lazily negated view are refused (``ValueError``)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != dev or t.numel() != numel:
        raise ValueError(f"{name} must be a float64 tensor of {numel} element(s) on {dev}")
    _no_lazy_bits(t, name)
    return t.detach().contiguous().reshape(numel)


def train_rnsum(rn) -> torch.Tensor:
    """This call's share of the pair: float64 [2] = (sum of rn in a fixed order, B)."""
    _need_cuda(rn, "rn")
    lib, dev, B = _lib.load(), rn.device, rn.shape[0]
    with torch.cuda.device(dev):
        rn = _f32(rn, dev, (B,), "rn")
        pair = torch.empty(2, dtype=torch.float64, device=dev)
        _lib.check(lib.admmnet_train_rnsum_f64(B, _ptr(rn), _ptr(pair), _stream(dev)), "admmnet_train_rnsum_f64")
    return pair


def train_stepsize_pair(rn, pair, rho, W1, b1, W2, b2, knorm: float) -> torch.Tensor:
    """``train_stepsize`` with mean = float32(pair[0] / pair[1]) instead of the mean over the call."""
    _need_cuda(rn, "rn")
    lib, dev, B = _lib.load(), rn.device, rn.shape[0]
    with torch.cuda.device(dev):
        rn, rho, pair = _f32(rn, dev, (B,), "rn"), _f32(rho, dev, (), "rho"), _f64(pair, dev, 2, "pair")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 32, 3)
        step = torch.empty_like(rn)
        _lib.check(lib.admmnet_train_stepsize_pair_f32(B, float(knorm), _ptr(rn), _ptr(pair), _ptr(rho), _ptr(W1), _ptr(b1),
                                                       _ptr(W2), _ptr(b2), _ptr(step), _stream(dev)),
                   "admmnet_train_stepsize_pair_f32")
    return step


def train_stepsize_bwd_pair_front(g_step, rn, pair, rho, W1, b1, W2, b2, knorm: float):
    """The backward of ``train_stepsize_pair`` up to the sum over the ranks: returns (g_u [B], total float64 [1] = this call's
    sum of g_u rn, g_rho 0-dim, gW1 [32, 3], gb1 [32], gW2 [1, 32], gb2 [1]), the parameter gradients summed over this call."""
    _need_cuda(g_step, "g_step")
    lib, dev, B = _lib.load(), g_step.device, g_step.shape[0]
    with torch.cuda.device(dev):
        g_step, rn, rho = _f32(g_step, dev, (B,), "g_step"), _f32(rn, dev, (B,), "rn"), _f32(rho, dev, (), "rho")
        pair = _f64(pair, dev, 2, "pair")
        W1, b1, W2, b2 = _net(dev, W1, b1, W2, b2, 32, 3)
        g_u = torch.empty_like(rn)
        out = torch.empty(162, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float64, device=dev)
        need = lib.admmnet_train_stepsize_pair_partials(B)
        if need < 0:
            raise _lib.AdmmNetError(f"train_stepsize_bwd_pair_front: bad size (B={B})")
        part = torch.empty(need, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_train_stepsize_bwd_pair_front_f32(B, float(knorm), _ptr(g_step), _ptr(rn), _ptr(pair), _ptr(rho),
                                                                 _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(g_u), _ptr(out),
                                                                 _ptr(total), _ptr(part), _stream(dev)),
                   "admmnet_train_stepsize_bwd_pair_front_f32")
    return g_u, total, out[0], out[1:97].reshape(32, 3), out[97:129], out[129:161].reshape(1, 32), out[161:162]


def train_stepsize_bwd_pair_back(g_u, pair, total) -> torch.Tensor:
    """g_rn = ((g_u mean - total / count) + g_u eps) / (mean + eps)^2 from the pair and ``total`` summed over the ranks."""
    _need_cuda(g_u, "g_u")
    lib, dev, B = _lib.load(), g_u.device, g_u.shape[0]
    with torch.cuda.device(dev):
        g_u, pair, total = _f32(g_u, dev, (B,), "g_u"), _f64(pair, dev, 2, "pair"), _f64(total, dev, 1, "total")
        g_rn = torch.empty_like(g_u)
        _lib.check(lib.admmnet_train_stepsize_bwd_pair_back_f32(B, _ptr(g_u), _ptr(pair), _ptr(total), _ptr(g_rn), _stream(dev)),
                   "admmnet_train_stepsize_bwd_pair_back_f32")
    return g_rn


# ---- the training losses (csrc/loss.hip) --------------------------------------------------------------------------------------
# out [3] float32 = (total, first part, second part); g_out [3] = the gradients of those three, a device tensor.
_LOSS_ANM, _LOSS_PHI = range(2)


def _loss_partials(lib, loss, B, dev):
    need = lib.admmnet_loss_partials(loss, B)
    if need < 0:
        raise _lib.AdmmNetError(f"loss: bad size (B={B})")
    return torch.empty(need, dtype=torch.float32, device=dev)


def _anm_args(tau, f, conf, tau_true, f_true, L_true, phi):
    """(lib, device, B, Lmax, D, the seven tensors as the kernels read them)."""
    for t, name in ((tau, "tau"), (f, "f"), (conf, "conf"), (tau_true, "tau_true"), (f_true, "f_true"), (L_true, "L_true"),
                    (phi, "phi")):
        _need_cuda(t, name)
    if tau.dim() != 2 or phi.dim() != 2:
        raise ValueError(f"tau must be [B, Lmax] and phi [B, D], got {tuple(tau.shape)} and {tuple(phi.shape)}")
    if L_true.is_floating_point() or L_true.is_complex() or L_true.dtype == torch.bool:
        raise ValueError(f"L_true must hold integers, got {L_true.dtype}")
    dev, (B, Lmax), D = tau.device, tau.shape, phi.shape[1]
    if not 1 <= Lmax <= 64 or D < 1 or B < 1:
        raise ValueError(f"loss_anm needs 1 <= Lmax <= 64, D >= 1, B >= 1, got Lmax={Lmax}, D={D}, B={B}")
    with torch.cuda.device(dev):
        real = [_f32(t, dev, (B, Lmax), name) for t, name in ((tau, "tau"), (f, "f"), (conf, "conf"), (tau_true, "tau_true"),
                                                              (f_true, "f_true"))]
        L_true = _num(L_true, dev, torch.int64, (B,), "L_true")
        phi = _c64(phi, dev, (B, D), "phi")
    return _lib.load(), dev, B, Lmax, D, (*real, L_true, phi)


def loss_anm(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg: float):
    """BasicANMLoss (loss.py:6-60): returns (out [3] = (total, param, reg), norms [B] = ||phi_b|| for ``loss_anm_bwd``,
    status [1] int32 = the number of signals whose L_true lies outside [0, Lmax] -- they are evaluated with L held to it)."""
    lib, dev, B, Lmax, D, t = _anm_args(tau, f, conf, tau_true, f_true, L_true, phi)
    with torch.cuda.device(dev):
        out = torch.empty(3, dtype=torch.float32, device=dev)
        norms = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        part = _loss_partials(lib, _LOSS_ANM, B, dev)
        _lib.check(lib.admmnet_loss_anm_f32(Lmax, D, B, *(_ptr(x) for x in t), float(lambda_reg), _ptr(out), _ptr(norms),
                                            _ptr(status), _ptr(part), _stream(dev)), "admmnet_loss_anm_f32")
    return out, norms, status


def loss_anm_bwd(g_out, tau, f, conf, tau_true, f_true, L_true, phi, norms, lambda_reg: float):
    """Backward of ``loss_anm`` from g_out [3]: returns (g_tau, g_f, g_conf [B, Lmax], g_phi [B, D] complex64)."""
    lib, dev, B, Lmax, D, t = _anm_args(tau, f, conf, tau_true, f_true, L_true, phi)
    _need_cuda(g_out, "g_out")
    with torch.cuda.device(dev):
        g_out, norms = _f32(g_out, dev, (3,), "g_out"), _f32(norms, dev, (B,), "norms")
        g_tau, g_f, g_conf = (torch.empty(B, Lmax, dtype=torch.float32, device=dev) for _ in range(3))
        g_phi = torch.empty(B, D, dtype=torch.complex64, device=dev)
        _lib.check(lib.admmnet_loss_anm_bwd_f32(Lmax, D, B, _ptr(g_out), *(_ptr(x) for x in t), _ptr(norms), float(lambda_reg),
                                                _ptr(g_tau), _ptr(g_f), _ptr(g_conf), _ptr(g_phi), _stream(dev)),
                   "admmnet_loss_anm_bwd_f32")
    return g_tau, g_f, g_conf, g_phi


def loss_phi(phi, phi_true, amplitude_weight: float, phase_weight: float) -> torch.Tensor:
    """PhiAlignmentLoss (loss.py:62-98): returns out [3] = (total, amplitude, phase)."""
    _need_cuda(phi_true, "phi_true")
    lib, dev, B, D = _small_args(phi, "phi")
    with torch.cuda.device(dev):
        phi, phi_true = _c64(phi, dev, (B, D), "phi"), _c64(phi_true, dev, (B, D), "phi_true")
        out = torch.empty(3, dtype=torch.float32, device=dev)
        part = _loss_partials(lib, _LOSS_PHI, B, dev)
        _lib.check(lib.admmnet_loss_phi_c64(D, B, _ptr(phi), _ptr(phi_true), float(amplitude_weight), float(phase_weight),
                                            _ptr(out), _ptr(part), _stream(dev)), "admmnet_loss_phi_c64")
    return out


def loss_phi_bwd(g_out, phi, phi_true, amplitude_weight: float, phase_weight: float) -> torch.Tensor:
    """Backward of ``loss_phi`` from g_out [3]: returns g_phi [B, D] complex64."""
    _need_cuda(phi_true, "phi_true")
    _need_cuda(g_out, "g_out")
    lib, dev, B, D = _small_args(phi, "phi")
    with torch.cuda.device(dev):
        g_out = _f32(g_out, dev, (3,), "g_out")
        phi, phi_true = _c64(phi, dev, (B, D), "phi"), _c64(phi_true, dev, (B, D), "phi_true")
        g_phi = torch.empty_like(phi)
        _lib.check(lib.admmnet_loss_phi_bwd_c64(D, B, _ptr(g_out), _ptr(phi), _ptr(phi_true), float(amplitude_weight),
                                                float(phase_weight), _ptr(g_phi), _stream(dev)), "admmnet_loss_phi_bwd_c64")
    return g_phi


# ---- AdamW and gradient-norm clipping over a tensor list (csrc/optim.hip) --------------------------------------------------------
def _optim_lists(what, *lists):
    """(lib, device, count, numel array, one pointer array per list) of same-length lists of dense float32 device tensors of
    pairwise equal shapes.  ``TypeError`` for what is no float32 tensor, ``ValueError`` for a sparse, non-contiguous, lazily
    negated or host tensor and for tensors on different devices: there is no other path."""
    count = len(lists[0])
    if any(len(l) != count for l in lists):
        raise ValueError(f"{what}: the tensor lists have different lengths {[len(l) for l in lists]}")
    dev = None
    for i in range(count):
        for l in lists:
            t = l[i]
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}: entry {i} is a {type(t).__name__}, not a tensor")
            if t.is_sparse or t.layout != torch.strided:
                raise ValueError(f"{what}: tensor {i} is sparse ({t.layout}); the kernels read dense tensors")
            if t.dtype != torch.float32:
                raise TypeError(f"{what}: tensor {i} is {t.dtype}; the kernels read float32")
            if not t.is_cuda:
                raise ValueError(f"{what}: tensor {i} is on {t.device}; the kernels read HIP device tensors (no CPU path)")
            if not t.is_contiguous():
                raise ValueError(f"{what}: tensor {i} of shape {tuple(t.shape)} and strides {t.stride()} is not contiguous")
            _no_lazy_bits(t, f"{what}: tensor {i}")
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError(f"{what}: tensor {i} is on {t.device}, the list began on {dev}")
            if t.shape != lists[0][i].shape:
                raise ValueError(f"{what}: tensor {i} has shapes {tuple(lists[0][i].shape)} and {tuple(t.shape)} in two lists")
    numel = (ctypes.c_int64 * count)(*[t.numel() for t in lists[0]])
    tables = [(ctypes.c_void_p * count)(*[t.data_ptr() for t in l]) for l in lists]
    return _lib.load(), dev, count, numel, tables


def _optim_coef(what, coef, dev):
    """``coef`` as the kernels read it: ONE float32 element on the list's device, refused otherwise like every other tensor."""
    if not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32:
        raise TypeError(f"{what}: coef must be a float32 tensor, got {coef.dtype if isinstance(coef, torch.Tensor) else type(coef).__name__}")
    if coef.numel() != 1 or coef.device != dev:
        raise ValueError(f"{what}: coef must hold one element on {dev}, got {coef.numel()} on {coef.device} (no copy is made)")
    _no_lazy_bits(coef, f"{what}: coef")
    return coef.detach().reshape(1)


def optim_gradnorm(grads, max_norm: float):
    """The 2-norm of all of ``grads`` (a non-empty list) and the clipping coefficient of ``clip_grad_norm_``: returns
    (total_norm, 0-dim float32; coef [1] float32 = clamp(max_norm / (total_norm + 1e-6), max=1); sumsq [1] float64), all on the
    device, nothing read back."""
    lib, dev, count, numel, (g,) = _optim_lists("optim_gradnorm", list(grads))
    if count == 0:
        raise ValueError("optim_gradnorm: the list is empty")
    need = lib.admmnet_optim_partials(count, numel)
    if need < 0:
        raise _lib.AdmmNetError("optim_gradnorm: the list has more than 2^31 - 1 blocks of 1024 elements")
    with torch.cuda.device(dev):
        part = torch.empty(max(need, 1) + 1, dtype=torch.float64, device=dev)     # the last entry: sumsq
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.admmnet_optim_gradnorm_f32(count, g, numel, float(max_norm), _ptr(part), _ptr(part[-1:]), _ptr(out[0:1]),
                                                  _ptr(out[1:2]), _stream(dev)), "admmnet_optim_gradnorm_f32")
    return out[0], out[1:2], part[-1:]


def optim_scale(grads, coef) -> None:
    """g <- g coef in place for every tensor of ``grads``; ``coef`` a device float32 tensor of one element."""
    lib, dev, count, numel, (g,) = _optim_lists("optim_scale", list(grads))
    if count == 0:
        return
    coef = _optim_coef("optim_scale", coef, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.admmnet_optim_scale_f32(count, g, numel, _ptr(coef), _stream(dev)), "admmnet_optim_scale_f32")


def _optim_flat(what, flat, tensors, dev):
    """``flat`` as the bucket kernels take it: a contiguous float32 device tensor with room for every element of the list."""
    if not isinstance(flat, torch.Tensor) or flat.dtype != torch.float32:
        raise TypeError(f"{what}: flat must be a float32 tensor, got {flat.dtype if isinstance(flat, torch.Tensor) else type(flat).__name__}")
    total = sum(t.numel() for t in tensors)
    if flat.device != dev or not flat.is_contiguous() or flat.dim() != 1 or flat.numel() < total:
        raise ValueError(f"{what}: flat must be a contiguous 1-d tensor of at least {total} elements on {dev}, got "
                         f"{tuple(flat.shape)} on {flat.device}")
    _no_lazy_bits(flat, f"{what}: flat")
    return flat.detach()


def optim_pack(tensors, flat) -> None:
    """The tensors of the list copied, in list order, into the front of ``flat`` (what ``torch.cat([t.reshape(-1) ...])`` would
    hold); the elements of ``flat`` behind the list's total stay as they are."""
    tensors = list(tensors)
    lib, dev, count, numel, (t,) = _optim_lists("optim_pack", tensors)
    if count == 0:
        return
    flat = _optim_flat("optim_pack", flat, tensors, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.admmnet_optim_pack_f32(count, t, numel, _ptr(flat), _stream(dev)), "admmnet_optim_pack_f32")


def optim_unpack(tensors, flat) -> None:
    """The inverse of ``optim_pack``: the front of ``flat`` copied back into the tensors of the list, in place."""
    tensors = list(tensors)
    lib, dev, count, numel, (t,) = _optim_lists("optim_unpack", tensors)
    if count == 0:
        return
    flat = _optim_flat("optim_unpack", flat, tensors, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.admmnet_optim_unpack_f32(count, t, numel, _ptr(flat), _stream(dev)), "admmnet_optim_unpack_f32")


def optim_adamw(params, grads, exp_avgs, exp_avg_sqs, hyper_index, hyper, coef=None) -> None:
    """One AdamW update of every tensor of ``params`` in place (with its state ``exp_avgs``, ``exp_avg_sqs``), tensor i with the
    constants ``hyper[hyper_index[i]]``: 7-tuples (1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t),
    eps) of Python floats.  ``coef``: a device float32 tensor of one element that multiplies every gradient as it is read (the
    fused clipping; the gradients stay as they are), or None."""
    lib, dev, count, numel, (p, g, m, v) = _optim_lists("optim_adamw", list(params), list(grads), list(exp_avgs),
                                                        list(exp_avg_sqs))
    if count == 0:
        return
    if len(hyper_index) != count or not hyper or not all(0 <= int(i) < len(hyper) for i in hyper_index):
        raise ValueError(f"optim_adamw: {count} tensors need {count} indices into the {len(hyper)} hyper-parameter sets")
    if coef is not None:
        coef = _optim_coef("optim_adamw", coef, dev)
    index = (ctypes.c_int32 * count)(*[int(i) for i in hyper_index])
    table = (_lib.AdamWHyper * len(hyper))(*[_lib.AdamWHyper(*(float(x) for x in h)) for h in hyper])
    with torch.cuda.device(dev):
        _lib.check(lib.admmnet_optim_adamw_f32(count, p, g, m, v, numel, index, len(hyper), table, _ptr(coef), _stream(dev)),
                   "admmnet_optim_adamw_f32")


def glayer(model, k: int, phi: torch.Tensor, h: torch.Tensor, Z=None):
    """GLayer.forward (admm_net.py:237-354) of layer k of ``model`` plus the Z-layer residual norm.

    Returns (G [B,n,n] c64, w [B,n] f32, rn [B] f32).
    """
    _need_cuda(phi, "phi")
    lib = _lib.load()
    dev = phi.device
    B, D = phi.shape
    n = D + 1
    cfg = model.cfg()
    with torch.cuda.device(dev):
        W = model.packed_weights(dev)
        off = lib.admmnet_layer_weight_offset(ctypes.byref(cfg), k)
        lw = W[off:]
        need = lib.admmnet_glayer_workspace_bytes(ctypes.byref(cfg), B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        G = torch.empty(B, n, n, dtype=torch.complex64, device=dev)
        w = torch.empty(B, n, dtype=torch.float32, device=dev)
        rn = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        phi, h = _c64(phi, dev, (B, D), "phi"), _f32(h, dev, (B, D), "h")
        Zc = None if Z is None else _c64(Z, dev, (B, n, n), "Z")
        _lib.check(lib.admmnet_glayer_f32(ctypes.byref(cfg), _ptr(lw), _ptr(phi), _ptr(h), _ptr(Zc), B, _ptr(G),
                                          _ptr(w), _ptr(rn), _ptr(ws), need, _ptr(status), _stream(dev)),
                   "admmnet_glayer_f32")
        bad = int(status[0].item())
        if bad:
            raise _lib.AdmmNetError(f"eigensolver failed on {bad} matrices")
    return G, w, rn


def glayer_spectral(model, k: int, phi: torch.Tensor, h: torch.Tensor, Z: torch.Tensor, G: torch.Tensor, rn: torch.Tensor,
                    mode: int = 0, alpha=None, phi_prev=None, h_prev=None, waves: int = 0):
    """The matrix-function G-layer of layer k of ``model`` (csrc/spectral_fused.hip, admmnet_glayer_spectral_f32) on
    caller-supplied state, IN PLACE: Z, G [B, n, n] complex64 and rn [B] float32 must be contiguous device tensors without conj
    or neg bit (``ValueError`` otherwise, before any launch); only their lower triangles are read or written, G and rn only for
    accepted matrices.

    mode 0: Z is the state layer k reads.  mode 1: the Z-layer update of layer k-1, Z <- Z + alpha (G - C_prev), is applied
    first (G holds G of layer k-1 on entry; alpha [B], phi_prev [B, D], h_prev [B, D] of layer k-1).  mode 2: as 1 with
    the stored Z taken as zero.  waves: 0 = the forward's choice for a call of B signals, 12, or 4 (D <= 128).

    Returns (flag [B] int32: 0 = accepted, else the check that rejected the matrix; status [4] int32)."""
    _need_cuda(phi, "phi")
    lib = _lib.load()
    dev = phi.device
    B, D = phi.shape
    n = D + 1
    for t, name, dt, shape in ((Z, "Z", torch.complex64, (B, n, n)), (G, "G", torch.complex64, (B, n, n)),
                               (rn, "rn", torch.float32, (B,))):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor {shape} on {dev}")
        _no_lazy_bits(t, name)
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be 0, 1 or 2, got {mode}")
    cfg = model.cfg()
    with torch.cuda.device(dev):
        W = model.packed_weights(dev)
        lw = W[lib.admmnet_layer_weight_offset(ctypes.byref(cfg), k):]
        lwp = W[lib.admmnet_layer_weight_offset(ctypes.byref(cfg), k - 1):] if mode else None
        phi, h = _c64(phi, dev, (B, D), "phi"), _f32(h, dev, (B, D), "h")
        if mode:
            alpha = _f32(alpha, dev, (B,), "alpha")
            phi_prev, h_prev = _c64(phi_prev, dev, (B, D), "phi_prev"), _f32(h_prev, dev, (B, D), "h_prev")
        else:
            alpha = phi_prev = h_prev = None
        flag = torch.full((B,), -1, dtype=torch.int32, device=dev)
        status = torch.full((4,), -1, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_glayer_spectral_f32(ctypes.byref(cfg), _ptr(lw), _ptr(phi), _ptr(h), _ptr(Z), mode, _ptr(lwp),
                                                   _ptr(alpha), _ptr(phi_prev), _ptr(h_prev), B, _ptr(G), _ptr(rn),
                                                   _ptr(flag), _ptr(status), waves, _stream(dev)),
                   "admmnet_glayer_spectral_f32")
    return flag, status


def spectrum(phi: torch.Tensor, xbase: int, ybase: int, taus: torch.Tensor, fs: torch.Tensor):
    """|phi^H kron(s(f), conj d(tau))|^2 on the grid fs x taus (peakSearchUtils.py:9-60), float64.

    phi [B, ybase*xbase] complex64; returns [B, len(fs), len(taus)] float64.
    """
    _need_cuda(phi, "phi")
    lib = _lib.load()
    dev = phi.device
    phi = _c64(phi, dev, None, "phi")
    B = phi.shape[0]
    taus, fs = _num(taus, dev, torch.float64, None, "taus"), _num(fs, dev, torch.float64, None, "fs")
    nx, ny = taus.numel(), fs.numel()
    with torch.cuda.device(dev):
        need = lib.admmnet_spectrum_workspace_bytes(xbase, ybase, nx, ny)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(B, ny, nx, dtype=torch.float64, device=dev)
        _lib.check(lib.admmnet_spectrum_f64(_ptr(phi), B, xbase, ybase, _ptr(taus), nx, _ptr(fs), ny, _ptr(out),
                                            _ptr(ws), need, _stream(dev)), "admmnet_spectrum_f64")
    return out


def peak_search(phi: torch.Tensor, xbase: int, ybase: int, opts=None, max_peaks: int = 256):
    """alt_peak_search (utils/peakSearchUtils.py:63-173) for a whole batch on the device: coarse spectrum,
    regional maxima and the refinement rounds, one signal per workgroup.

    Returns (peaks [B, max_peaks, 3] float64 = (tau, f, height) in np.where order of the coarse maxima,
    counts [B] int32 = number of regional maxima; rows >= counts[b] are zero, counts above max_peaks mean
    the list was truncated).
    """
    from . import peak_search as ps
    import ctypes as _ct
    _need_cuda(phi, "phi")
    lib = _lib.load()
    dev = phi.device
    B, D = phi.shape
    if D != xbase * ybase:
        raise ValueError(f"phi has {D} entries, expected xbase*ybase = {xbase * ybase}")
    so = {**ps.DEFAULT_OPTS, **(opts or {})}
    ax, ay = ps.coarse_axes(opts)
    nx, ny = len(ax), len(ay)
    with torch.cuda.device(dev):
        peaks = torch.zeros(B, max_peaks, 3, dtype=torch.float64, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        if nx == 0 or ny == 0:
            return peaks, counts
        tx = torch.from_numpy(ax).to(dev)
        ty = torch.from_numpy(ay).to(dev)
        need = lib.admmnet_peak_search_workspace_bytes(xbase, ybase, nx, ny, B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        o7 = (_ct.c_double * 7)(so["xmin"], so["xmax"], so["xstep"], so["ymin"], so["ymax"], so["ystep"],
                               so["reducefactor"])
        phi = _c64(phi, dev, (B, D), "phi")
        _lib.check(lib.admmnet_peak_search_f64(_ptr(phi), B, xbase, ybase, _ptr(tx), nx, _ptr(ty), ny, o7,
                                               int(so["iter"]), max_peaks, _ptr(peaks), _ptr(counts), _ptr(ws), need,
                                               _stream(dev)), "admmnet_peak_search_f64")
    return peaks, counts


def peak_top(phi: torch.Tensor, xbase: int, ybase: int, opts=None, top: int = 3, top_n=None):
    """The ``top`` highest peaks of every signal on the device in one kernel (csrc/estimate.hip): ``peak_search``
    followed by the two lines both inference callers of the reference add, sort by refined height (descending, stable)
    and cut (main_for_net.py:117-126, test/test_model_peaksearch.py:85-96).  Every regional maximum takes part: there
    is no ``max_peaks``, and the coarse spectrum never leaves the chip.

    phi [B, ybase*xbase] complex64; opts as for ``peak_search``; top: 1 .. 64; top_n: None, or [B] integers, the
    number of rows wanted per signal (clamped to 0 .. top; test_model_peaksearch.py:91 cuts at the sample's L_true).
    Returns (rows [B, top, 3] float64 = (tau, f, height) in rank order, ``peak_search.top_rows`` of the signal's peak
    list bit for bit; rows beyond min(counts[b], top_n[b]) are NaN, counts [B] int32 = number of regional maxima).
    """
    from . import peak_search as ps
    _need_cuda(phi, "phi")
    lib = _lib.load()
    dev = phi.device
    B, D = phi.shape
    if D != xbase * ybase:
        raise ValueError(f"phi has {D} entries, expected xbase*ybase = {xbase * ybase}")
    if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= 64:
        raise ValueError(f"top must be an int in 1 .. 64, got {top!r}")
    top = int(top)
    so = {**ps.DEFAULT_OPTS, **(opts or {})}
    ax, ay = ps.coarse_axes(opts)
    nx, ny = len(ax), len(ay)
    with torch.cuda.device(dev):
        rows = torch.full((B, top, 3), float("nan"), dtype=torch.float64, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        if top_n is not None:
            top_n = _num(torch.as_tensor(top_n), dev, torch.int32, (B,), "top_n")
        if nx == 0 or ny == 0:
            return rows, counts
        tx = torch.from_numpy(ax).to(dev)
        ty = torch.from_numpy(ay).to(dev)
        need = lib.admmnet_peak_top_workspace_bytes(xbase, ybase, nx, ny)
        if need < 0:
            _lib.check(-1, "admmnet_peak_top_workspace_bytes")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        o7 = (ctypes.c_double * 7)(so["xmin"], so["xmax"], so["xstep"], so["ymin"], so["ymax"], so["ystep"],
                                   so["reducefactor"])
        phi = _c64(phi, dev, (B, D), "phi")
        _lib.check(lib.admmnet_peak_top_f64(_ptr(phi), B, xbase, ybase, _ptr(tx), nx, _ptr(ty), ny, o7, int(so["iter"]),
                                            top, _ptr(top_n), _ptr(rows), _ptr(counts), _ptr(ws), need, _stream(dev)),
                   "admmnet_peak_top_f64")
    return rows, counts


def regional_maxima(Z: torch.Tensor):
    """skimage.morphology.local_maxima(connectivity=2) (utils/peakSearchUtils.py:118) of a batch of images on the
    device (the maxima stage of the peak-search kernel).  Z [B, ny, nx] float64 -> bool mask [B, ny, nx]."""
    _need_cuda(Z, "Z")
    lib = _lib.load()
    dev = Z.device
    Z = _num(Z, dev, torch.float64, None, "Z")
    B, ny, nx = Z.shape
    cap = nx * ny
    with torch.cuda.device(dev):
        peaks = torch.zeros(B, cap, 3, dtype=torch.float64, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        _lib.check(lib.admmnet_regional_maxima_f64(_ptr(Z), B, nx, ny, cap, _ptr(peaks), _ptr(counts), _stream(dev)),
                   "admmnet_regional_maxima_f64")
    mask = torch.zeros(B, ny, nx, dtype=torch.bool, device=dev)
    cnt = counts.cpu()
    for i in range(B):
        k = int(cnt[i])
        if k:
            mask[i, peaks[i, :k, 1].long(), peaks[i, :k, 0].long()] = True
    return mask


# ---- the spectral terms of the phi loss (csrc/loss_spectrum.hip); defined in spectral_ops.py on the helpers above ------------------
from .spectral_ops import loss_spectrum, loss_spectrum_bwd  # noqa: E402,F401
# ---- the assignment loss of the head (csrc/loss_set.hip); defined in set_ops.py on the helpers above ------------------------------
from .set_ops import loss_set, loss_set_bwd  # noqa: E402,F401
