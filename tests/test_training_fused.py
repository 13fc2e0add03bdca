"""CPU: the fused training route (``unrolled_forward(..., fused=True)`` / ``model.train_route = "fused"``) with the tensor
stand-in ``training.TorchLayerKernels`` for the HIP layer kernels.

* each of the autograd functions with a hand-written backward (layer matrix, residual norm, state update, the gather of
  the border column and diagonal, the rebuild with that gather folded in), in complex128 / float64, against autograd through the
  existing tensor formulation (``training._block_matrix`` and the bodies of ``_g_layer`` / ``_z_layer``): every gradient
  within 1e-12 of its largest entry (float64 round-off on <= n^2 terms at n <= 13 is 1e-13-class);
* the whole route on the committed reference-gradient fixtures under tests/test_training.py's own rule;
* ``sub_batch`` on the fused route under tests/test_sub_batch.py's two bounds;
* the ``train_route`` knob.
"""
import os

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import training
from oracle import admm_net_ref as R
from admm_net_amd import synth

import test_training as TT

TLK = training.TorchLayerKernels
CPU = dict(solver=TT.cpu_eigh, assembler=training.TorchAssembler)
FUSED = dict(fused=True, layer_kernels=TLK, **CPU)
herm = lambda X: 0.5 * (X + X.transpose(1, 2).conj())


def _case(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    n = D + 1
    c = lambda *s: torch.randn(*s, dtype=torch.complex128, generator=g)
    phi = c(B, D)
    h = torch.randn(B, D, dtype=torch.float64, generator=g)
    Z, G = herm(c(B, n, n)) * 2, herm(c(B, n, n)) * 2          # Hermitian state
    up = c(B, n, n)                                            # NON-Hermitian upstream gradient
    r = torch.rand((), dtype=torch.float64, generator=g) + 0.3
    s = torch.rand(B, dtype=torch.float64, generator=g)
    grn = torch.randn(B, dtype=torch.float64, generator=g)
    return phi, h, Z, G, up, r, s, grn


def _close(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= 1e-12 * scale, f"{name}: {err:.3e} against max {scale:.3e}"


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


SIZES = [(3, 6, 0), (2, 12, 1), (4, 1, 2), (1, 9, 3)]      # (B, D, seed): n = 7, 13, 2, 10 (even n included)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_layer_matrix_function_matches_autograd(B, D, seed):
    phi, h, Z, _, gA, r, _, _ = _case(B, D, seed)
    corner = 1.3
    a = _leaves(phi, h, Z, r)
    A1 = training._LayerMatrix.apply(*a, corner, TLK)
    b = _leaves(phi, h, Z, r)
    A2 = training._block_matrix(b[0], b[1], corner) - b[3] * b[2]          # the body of _g_layer
    A2 = 0.5 * (A2 + A2.transpose(1, 2).conj())
    _close(A1.detach(), A2.detach(), "A")
    assert torch.equal(A1, A1.transpose(1, 2).conj())
    g1 = torch.autograd.grad(A1, a, gA)
    g2 = torch.autograd.grad(A2, b, gA)
    for x, y, name in zip(g1, g2, ("g_phi", "g_h", "gZ", "g_r")):
        _close(x, y, name)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_residual_norm_function_matches_autograd(B, D, seed):
    phi, h, _, G, _, _, _, grn = _case(B, D, seed)
    corner = 0.8
    a = _leaves(G, phi, h)
    rn1 = training._ResidualNorm.apply(*a, corner, TLK)
    b = _leaves(G, phi, h)
    rn2 = torch.linalg.matrix_norm(b[0] - training._block_matrix(b[1], b[2], corner))    # the body of _z_layer
    _close(rn1.detach(), rn2.detach(), "rn")
    g1 = torch.autograd.grad(rn1, a, grn)
    g2 = torch.autograd.grad(rn2, b, grn)
    for x, y, name in zip(g1, g2, ("gG", "g_phi", "g_h")):
        _close(x, y, name)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_state_update_function_matches_autograd(B, D, seed):
    phi, h, Z, G, g, _, s, _ = _case(B, D, seed)
    corner = 0.8
    a = _leaves(Z, G, phi, h, s)
    Z1 = training._StateUpdate.apply(*a, corner, TLK)
    b = _leaves(Z, G, phi, h, s)
    Z2 = b[0] + b[4].reshape(-1, 1, 1) * (b[1] - training._block_matrix(b[2], b[3], corner))   # the body of _z_layer
    _close(Z1.detach(), Z2.detach(), "Z'")
    g1 = torch.autograd.grad(Z1, a, g)
    g2 = torch.autograd.grad(Z2, b, g)
    for x, y, name in zip(g1, g2, ("gZ", "gG", "g_phi", "g_h", "g_s")):
        _close(x, y, name)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_gather_function_matches_autograd_through_the_slices(B, D, seed):
    """``_Gather`` against the slicing the phi layer (border column) and the H layer (real diagonal) do on the dense matrix."""
    _, _, Z, _, _, _, _, _ = _case(B, D, seed)
    g = torch.Generator().manual_seed(seed + 50)
    g_col = torch.randn(B, D, dtype=torch.complex128, generator=g)
    g_dg = torch.randn(B, D, dtype=torch.float64, generator=g)
    (a,), (b,) = _leaves(Z), _leaves(Z)
    col1, dg1 = training._Gather.apply(a, TLK)
    col2, dg2 = b[:, :-1, -1], torch.diagonal(b, dim1=1, dim2=2)[:, :D].real
    assert torch.equal(col1, col2) and torch.equal(dg1, dg2)
    (g1,) = torch.autograd.grad((col1, dg1), a, (g_col, g_dg))
    (g2,) = torch.autograd.grad((col2, dg2), b, (g_col, g_dg))
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("B,D,seed", SIZES)
def test_rebuild_gather_function_matches_rebuild_plus_slices(B, D, seed):
    """``_RebuildGather`` (G, its border column and its diagonal as three outputs, the slices' gradients folded into the
    symmetrisation) against ``_Rebuild`` followed by autograd's slicing."""
    n = D + 1
    g = torch.Generator().manual_seed(seed + 70)
    X = torch.randn(B, n, n, dtype=torch.complex128, generator=g)
    V = torch.linalg.eigh(X + X.transpose(1, 2).conj())[1]
    d = torch.randn(B, n, dtype=torch.float64, generator=g)
    up = torch.randn(B, n, n, dtype=torch.complex128, generator=g)            # non-Hermitian
    g_col = torch.randn(B, D, dtype=torch.complex128, generator=g)
    g_dg = torch.randn(B, D, dtype=torch.float64, generator=g)
    (d1,), (d2,) = _leaves(d), _leaves(d)
    G1, col1, dg1 = training._RebuildGather.apply(V, d1, training.TorchAssembler, TLK)
    G2 = training._Rebuild.apply(V, d2, training.TorchAssembler)
    col2, dg2 = G2[:, :-1, -1], torch.diagonal(G2, dim1=1, dim2=2)[:, :D].real
    assert torch.equal(G1, G2) and torch.equal(col1, col2) and torch.equal(dg1, dg2)
    (q1,) = torch.autograd.grad((G1, col1, dg1), d1, (up, g_col, g_dg))
    (q2,) = torch.autograd.grad((G2, col2, dg2), d2, (up, g_col, g_dg))
    _close(q1, q2, "g_d")
    S = TLK.herm(up, g_col, g_dg)
    assert torch.equal(S, S.transpose(1, 2).conj())


def test_state_update_passes_the_incoming_gradient_through():
    """gZ of the update is the incoming tensor itself, not a copy."""
    phi, h, Z, G, g, _, s, _ = _case(2, 5, 7)
    ctx = type("Ctx", (), {"saved_tensors": (G, phi, h, s), "c": 0.5, "lk": TLK})()
    out = training._StateUpdate.backward(ctx, g)
    assert out[0] is g and len(out) == 7 and out[5] is None and out[6] is None


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_fused_route_matches_reference_gradients(path):
    z, m, head, t = TT.load(path)
    m.eval()   # fixture convention: dropout off
    out = training.unrolled_forward(m, t("y"), t("b"), t("sigma"), **FUSED)
    phi = out[3] if head else out
    assert np.abs(phi.detach().numpy() - z["phi"]).max() <= 2e-5 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


def _sb_model(Nb, Nd, K, seed):
    sd = R.make_weights(Nb, Nd, K, seed=seed, head=True, perturb=0.3)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K)
    m.load_state_dict(sd)
    return m.eval()


def _sb_loss(out, seed):
    """A fixed random linear functional of every output, so that every output carries gradient."""
    g = torch.Generator().manual_seed(seed)
    tau, f, conf, phi = out
    c_phi = torch.randn(phi.shape, dtype=torch.complex64, generator=g)
    return ((c_phi.conj() * phi).real.sum() + (torch.randn(tau.shape, generator=g) * tau).sum()
            + (torch.randn(f.shape, generator=g) * f).sum() + (torch.randn(conf.shape, generator=g) * conf).sum())


@pytest.mark.parametrize("B,g", [(11, 4), (9, 1), (10, 5)])
def test_fused_route_groups_equal_separate_batches(B, g):
    """tests/test_sub_batch.py::test_training_route_groups_equal_separate_batches on the fused stand-in route: the outputs
    of one grouped call equal the per-group calls to 1e-6 of the largest entry, the parameter gradients the SUM of the
    per-group calls' gradients to 1e-5 max + 1e-7."""
    Nb, Nd, K = 3, 4, 3
    m = _sb_model(Nb, Nd, K, seed=21)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=5)
    y, b, s = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    grads = lambda: {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}

    m.zero_grad(set_to_none=True)
    out = training.unrolled_forward(m, y, b, s, sub_batch=g, **FUSED)
    _sb_loss(out, 1).backward()
    got = grads()

    m.zero_grad(set_to_none=True)
    parts = [training.unrolled_forward(m, y[lo:lo + g], b[lo:lo + g], s[lo:lo + g], **FUSED) for lo in range(0, B, g)]
    sep = tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    _sb_loss(sep, 1).backward()
    want = grads()

    for a, r in zip(out, sep):
        assert (a - r).abs().max() <= 1e-6 * r.abs().max()
    for name, w in want.items():
        if w is None:
            assert got[name] is None, name
            continue
        assert (got[name] - w).abs().max() <= 1e-5 * w.abs().max() + 1e-7, name
    whole = training.unrolled_forward(m, y, b, s, **FUSED)
    assert (whole[3] - sep[3]).abs().max() > 1e-5 * sep[3].abs().max()


def test_fused_route_agrees_with_tensor_route_under_the_fixture_rule():
    """The two routes differ in the last bits of the layer matrix and torch.linalg.eigh may then return another basis inside
    the clustered bulk, so the gradients are compared with the fixtures' rule 5e-4 max|grad| + 1e-6, not tighter."""
    path = TT.CASES[0]
    z, m1, head, t = TT.load(path)
    _, m0, _, _ = TT.load(path)
    m1.eval(), m0.eval()
    TT.loss_of(training.unrolled_forward(m1, t("y"), t("b"), t("sigma"), **FUSED), t, head).backward()
    TT.loss_of(training.unrolled_forward(m0, t("y"), t("b"), t("sigma"), **CPU), t, head).backward()
    for (name, p1), p0 in zip(m1.named_parameters(), m0.parameters()):
        if p0.grad is None:
            assert p1.grad is None, name
            continue
        assert (p1.grad - p0.grad).abs().max() <= TT.RTOL * p0.grad.abs().max() + 1e-6, name


def test_layer_kernels_need_the_fused_flag():
    m = A.PhiEstADMMNet(M=2, N=2, num_layers=2)
    y = torch.ones(1, 4, dtype=torch.complex64)
    with pytest.raises(ValueError):
        training.unrolled_forward(m, y, y, torch.ones(1), layer_kernels=TLK, **CPU)


def test_train_route_knob():
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    assert m.train_route == "tensor"
    keys = set(m.state_dict())
    m.train_route = "fused"
    assert m.train_route == "fused" and set(m.state_dict()) == keys
    for bad in ("Fused", "", None, 1, "hip"):
        with pytest.raises(ValueError):
            m.train_route = bad
    assert m.train_route == "fused"
    m.train_route = "tensor"
    assert A.ADMMNet(M=2, N=2, num_layers=2).train_route == "tensor"


def test_train_ops_refuse_cpu_tensors():
    from admm_net_amd import _lib, ops
    phi, h, Z, G, g, r, s, grn = (x.to(torch.complex64) if x.is_complex() else x.float() for x in _case(2, 3, 0))
    for call in (lambda: ops.train_matrix(phi, h, Z, r, 1.0), lambda: ops.train_matrix_bwd(g, Z, r),
                 lambda: ops.train_resnorm(G, phi, h, 1.0), lambda: ops.train_resnorm_bwd(grn, grn, G, phi, h, 1.0),
                 lambda: ops.train_zupdate(Z, G, phi, h, s, 1.0), lambda: ops.train_zupdate_bwd(g, G, phi, h, s, 1.0),
                 lambda: ops.train_gather(Z), lambda: ops.train_scatter(phi, h), lambda: ops.train_herm(g, phi, h)):
        with pytest.raises(_lib.AdmmNetError):
            call()


def test_train_entry_points_reject_bad_arguments():
    """ADMMNET_E_ARG (-1) for n outside 2 ... 257, B < 1, a tile-pair grid beyond 31 bits and null pointers -- decided on the
    host before anything is launched."""
    import ctypes
    from admm_net_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)
    assert lib.admmnet_train_partials(101, 256) == 256 * 10 and lib.admmnet_train_partials(257, 65536) == 65536 * 45
    assert lib.admmnet_train_partials(1, 4) == -1 and lib.admmnet_train_partials(258, 4) == -1
    for n, B in ((1, 4), (258, 4), (101, 0), (257, 2 ** 31 // 45 + 1)):
        assert lib.admmnet_train_matrix_f32(n, B, p, p, p, p, 1.0, p, null) == -1
        assert lib.admmnet_train_matrix_bwd_f32(n, B, p, p, p, p, p, p, p, p, null) == -1
        assert lib.admmnet_train_resnorm_f32(n, B, p, p, p, 1.0, p, null) == -1
        assert lib.admmnet_train_resnorm_bwd_f32(n, B, p, p, p, p, p, 1.0, p, p, p, null) == -1
        assert lib.admmnet_train_zupdate_c64(n, B, p, p, p, p, p, 1.0, p, null) == -1
        assert lib.admmnet_train_zupdate_bwd_c64(n, B, p, p, p, p, p, 1.0, p, p, p, p, null) == -1
        assert lib.admmnet_train_gather_c64(n, B, p, p, p, null) == -1
        assert lib.admmnet_train_scatter_c64(n, B, p, p, p, null) == -1
        assert lib.admmnet_train_herm_c64(n, B, p, p, p, p, null) == -1
    assert b"train_" in lib.admmnet_last_error()
    assert lib.admmnet_train_matrix_f32(101, 4, p, p, null, p, 1.0, p, null) == -1
    assert lib.admmnet_train_matrix_bwd_f32(101, 4, p, p, p, p, p, p, p, null, null) == -1
    assert lib.admmnet_train_resnorm_f32(101, 4, p, p, p, 1.0, null, null) == -1
    assert lib.admmnet_train_resnorm_bwd_f32(101, 4, p, null, p, p, p, 1.0, p, p, p, null) == -1
    assert lib.admmnet_train_zupdate_c64(101, 4, p, p, p, p, null, 1.0, p, null) == -1
    assert lib.admmnet_train_zupdate_bwd_c64(101, 4, p, p, p, p, p, 1.0, p, p, p, null, null) == -1
    assert lib.admmnet_train_gather_c64(101, 4, p, null, p, null) == -1
    assert lib.admmnet_train_scatter_c64(101, 4, p, p, null, null) == -1
    assert lib.admmnet_train_herm_c64(101, 4, p, p, null, p, null) == -1          # g_col without g_diag
    assert lib.admmnet_train_herm_c64(101, 4, p, null, null, null, null) == -1
