"""GPU: the fused training route -- the streaming layer kernels of csrc/train_layer.hip (``ops.train_*``) against float64
evaluations of their definitions, and ``model.train_route = "fused"`` end to end.

Kernel bounds (from the number formats, not from what the kernels give):
  * elementwise outputs (A, Z', gZ, gG): 1e-6 max|out| -- at most three float32 roundings of 6e-8 each, with headroom for
    cancellation against the largest entry;
  * reductions (rn^2, g_s, g_phi, g_h, g_r): 2e-5 sum|terms| with the sum of magnitudes taken in float64 -- the worst case of
    <= ~260 serial float32 additions per thread plus a tree.
The float64 references start from the float32 inputs the kernels read.  Each test prints the worst error / bound it saw.
"""
import os

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import ops, synth, training

import test_training as TT

pytestmark = pytest.mark.gpu

SHAPES = [(101, 5), (7, 3), (257, 2), (129, 4), (33, 4)]      # (n, B); (10, 3): an even n, every matrix 16-byte aligned
SHAPES_ALL = SHAPES + [(10, 3), (2, 5)]
ELEM, RED = 1e-6, 2e-5
DEV = "cuda:0"


def _inputs(n, B, seed):
    g = torch.Generator().manual_seed(seed)
    D = n - 1
    c = lambda *s: torch.randn(*s, dtype=torch.complex64, generator=g)
    herm = lambda X: X + X.transpose(1, 2).conj()
    t = dict(phi=c(B, D), h=torch.randn(B, D, generator=g), Z=herm(c(B, n, n)), G=herm(c(B, n, n)),
             up=c(B, n, n),                                     # non-Hermitian upstream gradient
             r=torch.rand((), generator=g) + 0.3, s=torch.rand(B, generator=g) + 0.1, grn=torch.randn(B, generator=g))
    return t, {k: v.to(DEV) for k, v in t.items()}


def _f64(t):
    return {k: v.to(torch.complex128 if v.is_complex() else torch.float64) for k, v in t.items()}


def _block(phi, h, c):
    return training._block_matrix(phi, h, c)


class Worst:
    def __init__(self):
        self.ratio = 0.0

    def elem(self, got, want, name):
        got = got.cpu().to(want.dtype)
        err, bound = (got - want).abs().max().item(), ELEM * want.abs().max().item()
        self.ratio = max(self.ratio, err / bound)
        assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"

    def red(self, got, want, mag, name):
        """mag: sum of the magnitudes of the terms of every entry, float64."""
        got = got.cpu().to(want.dtype)
        ratio = ((got - want).abs() / (RED * mag)).max().item()
        self.ratio = max(self.ratio, ratio)
        assert ratio <= 1.0, f"{name}: error / (2e-5 sum|terms|) = {ratio:.3f}"


def _herm(X):
    return 0.5 * (X + X.transpose(1, 2).conj())


@pytest.mark.parametrize("n,B", SHAPES_ALL)
def test_matrix_kernels_match_their_definition(n, B):
    t, d = _inputs(n, B, seed=n)
    w, D, c, worst = _f64(t), n - 1, 1.3, Worst()
    Am = ops.train_matrix(d["phi"], d["h"], d["Z"], d["r"], c)
    worst.elem(Am, _herm(_block(w["phi"], w["h"], c) - w["r"] * w["Z"]), "A")
    assert torch.equal(Am, Am.transpose(1, 2).conj()), "A must be Hermitian bit for bit"
    assert torch.equal(Am, ops.train_matrix(d["phi"], d["h"], d["Z"], d["r"], c))
    g_phi, g_h, gZ, g_r = ops.train_matrix_bwd(d["up"], d["Z"], d["r"])
    S = _herm(w["up"])
    worst.elem(gZ, -w["r"] * S, "gZ")
    worst.red(g_phi, 2 * S[:, :D, D], w["up"][:, :D, D].abs() + w["up"][:, D, :D].abs(), "g_phi")
    dg = torch.diagonal(w["up"], dim1=1, dim2=2)[:, :D].real
    worst.red(g_h, dg, dg.abs() + 1e-300, "g_h")
    terms = (S.real * w["Z"].real).abs() + (S.imag * w["Z"].imag).abs()
    worst.red(g_r, -(S.conj() * w["Z"]).real.sum(), terms.sum(), "g_r")
    again = ops.train_matrix_bwd(d["up"], d["Z"], d["r"])
    assert all(torch.equal(a, b) for a, b in zip((g_phi, g_h, gZ, g_r), again))
    print(f"n={n} B={B} matrix: worst error / bound {worst.ratio:.3f}")


@pytest.mark.parametrize("n,B", SHAPES_ALL)
def test_resnorm_kernels_match_their_definition(n, B):
    t, d = _inputs(n, B, seed=1000 + n)
    w, D, c, worst = _f64(t), n - 1, 0.8, Worst()
    rn = ops.train_resnorm(d["G"], d["phi"], d["h"], c)
    R = w["G"] - _block(w["phi"], w["h"], c)
    sq = (R.abs() ** 2).sum(dim=(1, 2))
    worst.red(rn.double() ** 2, sq, sq, "rn^2")
    assert torch.equal(rn, ops.train_resnorm(d["G"], d["phi"], d["h"], c))
    gG, g_phi, g_h = ops.train_resnorm_bwd(d["grn"], rn, d["G"], d["phi"], d["h"], c)
    q = (w["grn"] / rn.cpu().double()).reshape(-1, 1)
    worst.elem(gG, q.unsqueeze(-1) * R, "gG")
    worst.red(g_phi, -q * (R[:, :D, D] + R[:, D, :D].conj()),
              q.abs() * (w["G"][:, :D, D].abs() + w["G"][:, D, :D].abs() + 2 * w["phi"].abs()), "g_phi")
    dG = torch.diagonal(w["G"], dim1=1, dim2=2)[:, :D].real
    worst.red(g_h, -q * (dG - w["h"]), q.abs() * (dG.abs() + w["h"].abs()), "g_h")
    again = ops.train_resnorm_bwd(d["grn"], rn, d["G"], d["phi"], d["h"], c)
    assert all(torch.equal(a, b) for a, b in zip((gG, g_phi, g_h), again))
    print(f"n={n} B={B} resnorm: worst error / bound {worst.ratio:.3f}")


@pytest.mark.parametrize("n,B", SHAPES_ALL)
def test_zupdate_kernels_match_their_definition(n, B):
    t, d = _inputs(n, B, seed=2000 + n)
    w, D, c, worst = _f64(t), n - 1, 0.8, Worst()
    Zn = ops.train_zupdate(d["Z"], d["G"], d["phi"], d["h"], d["s"], c)
    R = w["G"] - _block(w["phi"], w["h"], c)
    sd = w["s"].reshape(-1, 1)
    worst.elem(Zn, w["Z"] + sd.unsqueeze(-1) * R, "Z'")
    assert torch.equal(Zn, ops.train_zupdate(d["Z"], d["G"], d["phi"], d["h"], d["s"], c))
    gG, g_phi, g_h, g_s = ops.train_zupdate_bwd(d["up"], d["G"], d["phi"], d["h"], d["s"], c)
    g = w["up"]
    worst.elem(gG, sd.unsqueeze(-1) * g, "gG")
    worst.red(g_phi, -sd * (g[:, :D, D] + g[:, D, :D].conj()), sd * (g[:, :D, D].abs() + g[:, D, :D].abs()), "g_phi")
    dg = torch.diagonal(g, dim1=1, dim2=2)[:, :D].real
    worst.red(g_h, -sd * dg, sd * dg.abs() + 1e-300, "g_h")
    terms = (R.real * g.real).abs() + (R.imag * g.imag).abs()
    worst.red(g_s, (R.conj() * g).real.sum(dim=(1, 2)), terms.sum(dim=(1, 2)), "g_s")
    again = ops.train_zupdate_bwd(d["up"], d["G"], d["phi"], d["h"], d["s"], c)
    assert all(torch.equal(a, b) for a, b in zip((gG, g_phi, g_h, g_s), again))
    print(f"n={n} B={B} zupdate: worst error / bound {worst.ratio:.3f}")


@pytest.mark.parametrize("n,B", SHAPES_ALL)
def test_gather_kernels_match_their_definition(n, B):
    """gather copies and scatter places values: exact.  herm(g + E) is elementwise: 1e-6 max|out|, Hermitian bit for bit."""
    t, d = _inputs(n, B, seed=3000 + n)
    w, D, worst = _f64(t), n - 1, Worst()
    col, dg = ops.train_gather(d["G"])
    assert torch.equal(col.cpu(), t["G"][:, :D, D]) and torch.equal(dg.cpu(), torch.diagonal(t["G"], dim1=1, dim2=2)[:, :D].real)
    E = ops.train_scatter(d["phi"], d["h"])
    want = training.TorchLayerKernels.scatter(t["phi"], t["h"])
    assert torch.equal(E.cpu(), want)
    S = ops.train_herm(d["up"], d["phi"], d["h"])
    worst.elem(S, _herm(w["up"] + want.to(torch.complex128)), "S")
    assert torch.equal(S, S.transpose(1, 2).conj())
    S0 = ops.train_herm(d["up"])
    worst.elem(S0, _herm(w["up"]), "herm(g)")
    assert torch.equal(S0, S0.transpose(1, 2).conj()) and torch.equal(S, ops.train_herm(d["up"], d["phi"], d["h"]))
    print(f"n={n} B={B} gather: worst error / bound {worst.ratio:.3f}")


def test_kernels_on_unaligned_matrices():
    """A batch whose base is only 8-byte aligned takes the 8-byte stream; same definitions, same bounds."""
    n, B = 33, 3
    t, d = _inputs(n, B, seed=5)
    w, c, worst = _f64(t), 0.8, Worst()
    off = {}
    for k in ("Z", "G", "up"):
        buf = torch.empty(B * n * n + 1, dtype=torch.complex64, device=DEV)
        off[k] = buf[1:].view(B, n, n)
        off[k].copy_(d[k])
        assert off[k].data_ptr() % 16 == 8 and off[k].is_contiguous()
    R = w["G"] - _block(w["phi"], w["h"], c)
    sd = w["s"].reshape(-1, 1, 1)
    rn = ops.train_resnorm(off["G"], d["phi"], d["h"], c)
    sq = (R.abs() ** 2).sum(dim=(1, 2))
    worst.red(rn.double() ** 2, sq, sq, "rn^2")
    worst.elem(ops.train_zupdate(off["Z"], off["G"], d["phi"], d["h"], d["s"], c), w["Z"] + sd * R, "Z'")
    worst.elem(ops.train_zupdate_bwd(off["up"], off["G"], d["phi"], d["h"], d["s"], c)[0], sd * w["up"], "gG")
    q = (w["grn"] / rn.cpu().double()).reshape(-1, 1, 1)
    worst.elem(ops.train_resnorm_bwd(d["grn"], rn, off["G"], d["phi"], d["h"], c)[0], q * R, "gG")
    print(f"unaligned: worst error / bound {worst.ratio:.3f}")


def test_state_update_gradient_of_z_is_the_incoming_tensor():
    t, d = _inputs(33, 2, seed=9)
    ctx = type("Ctx", (), {"saved_tensors": (d["G"], d["phi"], d["h"], d["s"]), "c": 0.5, "lk": training.LayerKernels})()
    out = training._StateUpdate.backward(ctx, d["up"])
    assert out[0] is d["up"]


def test_large_batch_grid():
    """B = 65 536 at a small n: the grids (B workgroups, B * tile pairs workgroups) do not overflow."""
    n, B = 5, 65536
    t, d = _inputs(n, B, seed=3)
    w, c, worst = _f64(t), 0.8, Worst()
    R = w["G"] - _block(w["phi"], w["h"], c)
    worst.elem(ops.train_matrix(d["phi"], d["h"], d["Z"], d["r"], c), _herm(_block(w["phi"], w["h"], c) - w["r"] * w["Z"]), "A")
    worst.elem(ops.train_zupdate(d["Z"], d["G"], d["phi"], d["h"], d["s"], c), w["Z"] + w["s"].reshape(-1, 1, 1) * R, "Z'")
    sq = (R.abs() ** 2).sum(dim=(1, 2))
    worst.red(ops.train_resnorm(d["G"], d["phi"], d["h"], c).double() ** 2, sq, sq, "rn^2")
    S = _herm(w["up"])
    terms = (S.real * w["Z"].real).abs() + (S.imag * w["Z"].imag).abs()
    worst.red(ops.train_matrix_bwd(d["up"], d["Z"], d["r"])[3], -(S.conj() * w["Z"]).real.sum(), terms.sum(), "g_r")


# ------------------------------------------------------------------------------------------------ the route, end to end
def _run(path, route):
    z, m, head, t = TT.load(path, DEV)
    m.train_route = route
    if head:
        m.eval()                                          # attention dropout off, as in the fixture
        out = m.forward_autograd(t("y"), t("b"), t("sigma"))
    else:
        m.train()                                         # the call trainPhi.py makes
        out = m(t("y"), t("b"), t("sigma"))
    return z, m, head, t, out


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_fused_route_gradients_match_reference(path):
    """tests/test_training.py::test_hip_training_gradients_match_reference with ``train_route = "fused"``."""
    z, m, head, t, out = _run(path, "fused")
    phi = out[3] if head else out
    assert phi.requires_grad and phi.is_cuda
    assert np.abs(phi.detach().cpu().numpy() - z["phi"]).max() <= 1e-4 * np.abs(z["phi"]).max()
    loss = TT.loss_of(out, t, head)
    loss.backward()
    print("worst gradient error / tolerance:", TT.check_grads(z, m, loss))


@pytest.mark.parametrize("path", TT.CASES, ids=[os.path.basename(p)[:-4] for p in TT.CASES])
def test_fused_and_tensor_route_give_the_same_phi(path):
    _, _, head, _, a = _run(path, "fused")
    _, _, _, _, b = _run(path, "tensor")
    pa, pb = (a[3], b[3]) if head else (a, b)
    err = (pa - pb).abs().max().item() / pb.abs().max().item()
    print(f"fused against tensor route: phi differs by {err:.2e} of its largest entry")
    assert err <= 2e-5


def _model16(K, B, seed=3):
    dev = torch.device(DEV)
    torch.manual_seed(seed)
    m = A.PhiEstADMMNet(M=16, N=16, num_layers=K).to(dev)
    y, b, sigma, _ = synth.make_batch(B, 16, 16, seed=5)
    return m, tuple(torch.from_numpy(v).to(dev) for v in (y, b, sigma))


def test_fused_route_at_16x16_trains_and_matches_inference():
    """16 x 16 (n = 257), K = 3, B = 8: the train-mode phi of the fused route agrees with the eval-mode inference phi to 1e-4,
    all gradients are finite, six AdamW steps lower the loss.  (No gradient comparison between eigensolvers or routes here:
    the eigenvalue-only gradient depends on the basis returned inside the clustered bulk.  The G layer's forward and backward at
    this size are compared with float64 on a FROZEN basis in tests/test_gpu_glayer_grad.py.)"""
    m, (ty, tb, ts) = _model16(3, 8)
    m.train_route = "fused"
    target = ty / tb
    m.train()
    phi_train = m(ty, tb, ts)
    m.eval()
    with torch.no_grad():
        phi_eval = m(ty, tb, ts)
    err = (phi_train - phi_eval).abs().max().item() / phi_eval.abs().max().item()
    print(f"train-mode against inference phi: {err:.2e}")
    assert err <= 1e-4
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = (m(ty, tb, ts) - target).abs().pow(2).mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        losses.append(loss.item())
    print("losses:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_fused_route_keeps_less_memory():
    """16 x 16, K = 3, B = 64: the peak of one forward + backward is strictly below the tensor route's (no residual, block
    matrix or diag_embed tensors on the tape)."""
    peak = {}
    for route in ("tensor", "fused"):
        m, (ty, tb, ts) = _model16(3, 64)
        m.train_route = route
        m.train()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m(ty, tb, ts).abs().pow(2).mean().backward()
        torch.cuda.synchronize()
        peak[route] = torch.cuda.max_memory_allocated() - base
        del m
    print(f"peak bytes above the model: tensor {peak['tensor']}, fused {peak['fused']}")
    assert peak["fused"] < peak["tensor"]
