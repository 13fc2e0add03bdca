"""GPU (-m gpu): both G-layer routes, layer by layer, on weights a user has trained.

Every other weight set the suite feeds the G-layer is the default init or the init with its scalars perturbed.  Training moves
value_net, threshold, rho and the H-layer MLPs together, and those decide whether a ReLU kink of the eigenvalue map
f(w) = softplus(w - thr) sigmoid(value_net(|w|)) falls into the bulk of a layer matrix, i.e. which matrices the matrix-function
kernel (csrc/spectral_fused.hip) accepts and which go to the eigensolver pipeline.

  * the reference-trained fixtures (tests/golden/phiest_*_trained.npz, make_golden.py --trained-only): for every layer k >= 1
    of a float64 oracle trace of the held-out batch, the matrix-function kernel (mode 0 in both workgroup shapes where D <= 128;
    the folded Z update of modes 1 / 2) and the eigensolver route (ops.glayer) on every matrix, at the bounds of
    tests/test_gpu_glayer_route.py and tests/test_gpu_parity.py::test_glayer_block_vs_oracle;
  * the same fixtures through the whole forward with ADMMNET_SPECTRAL=0 (a child process: the switch is read once);
  * 300 steps of training on the product's own training route, then both checks on the state it reached.
The accepted fraction and the flags are printed per layer; only "the route still runs" is asserted about them.
"""
import collections
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, ops, synth
from oracle import admm_net_ref as R
from golden_util import load_fixture
from test_gpu_glayer_route import (S_CORNER_Z, SENT_G, SENT_RN, TOL_G, TOL_RN, U32, _bits, _bulk_stats, _check_status, _corner,
                                   _fmap, _g_errors, _lipschitz, _mode0_inputs, _model, _run, _split, _tril)
from test_gpu_parity import TOL_PHI, ref_arith_error, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINED = ["phiest_10x10_K10_trained", "phiest_8x16_K8_trained", "phiest_16x16_K4_trained"]
# the state 300 steps of GPU training reached (test_gpu_training_then_both_routes; not bit-reproducible run to run): its last
# layer has the worst-conditioned matrices met so far -- kappa up to 6e-5, LAPACK fp32 9.5e-5 off in G
STATES = ["state_gpu_trained_10x10_K10"]
TOL_W = 1e-5     # eigenvalues of the eigensolver route, relative to the matrix's largest (test_glayer_block_vs_oracle)
# Bounds per matrix: max(TOL, C * kappa), kappa = L_f 8 2^-24 ||A||_2 / scale the float32 conditioning of the G-layer on that
# matrix (L_f: f's Lipschitz bound on the bulk interval; scale = max(|f(c)|, |f(lam_k)|) = ||G||_2); the float32 input rounding
# and arithmetic of ANY implementation moves G by ~kappa (LAPACK fp32 on trained weights: 0.9 .. 1.5 kappa).  Where kappa is
# below ~1e-5 -- every default-init and perturbed state of the suite -- the bounds are the plain TOL_G / TOL_W / TOL_RN.
C_SPECTRAL, C_EIGEN = 2.0, 3.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _fixture(name):
    z, sd, (Nb, Nd, K, B, L, head, _) = load_fixture(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    tr = []
    R.forward(sd, torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"]), Nb, Nd, K, L,
              dtype="f64", trace=tr)
    return z, sd, (Nb, Nd, K), tr


def _reference(sd, k, phi, h, Z, dtype=torch.float64):
    """G, eigenvalues, rn of layer k on the float32-valued inputs the kernels receive, by the oracle in float64 (the reference
    values) or in float32 (the reference's own arithmetic)."""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    sdk = {key: v.to(dtype) for key, v in sd.items() if key.startswith(f"gLayers.{k}.")}
    phi, h, Z = phi.to(cdt), h.to(dtype), Z.to(cdt)
    G, w, _ = R.g_layer(sdk, k, phi, h, Z, return_eig=True)
    Cz = R.block_matrix(phi, h, _corner(sd, f"zLayers.{k}.lambda_param"))
    return G, w, torch.linalg.norm(G - Cz, dim=(1, 2))


def _kappa(sd, k, w):
    """kappa (see above) of every matrix of layer k, from its float64 spectrum w [B, n]."""
    p = f"gLayers.{k}."
    gp = (float(torch.sigmoid(sd[p + "threshold"].double())), sd[p + "value_net.0.weight"].double().numpy()[:, 0],
          sd[p + "value_net.0.bias"].double().numpy(), sd[p + "value_net.2.weight"].double().numpy()[0],
          float(sd[p + "value_net.2.bias"].double()))
    out = []
    for wi in w.numpy():
        o, bulk = _split(wi)
        c, r, delta = _bulk_stats(wi[bulk])
        scale = max(abs(float(_fmap(gp, c))), float(np.abs(_fmap(gp, wi[o])).max()), 1e-6)
        half = 1.05 * max(r, delta)
        out.append(_lipschitz(gp, c - half, c + half) * 8 * U32 * float(np.abs(wi).max()) / scale)
    return np.array(out)


def _check_accepted(G, rn, flag, G_ref, rn_ref, tri, kappa, what):
    """test_gpu_glayer_route._check_accepted with the bounds max(TOL, C_SPECTRAL kappa) per matrix; -> worst G error."""
    acc = (flag == 0).numpy()
    err = _g_errors(G, G_ref, tri)
    for i in np.flatnonzero(acc):
        assert err[i] <= max(TOL_G, C_SPECTRAL * kappa[i]), (what, "G", i, err[i], kappa[i])
        assert torch.all(G[i].diagonal().imag == 0), (what, "diag imag", i)
        rerr = abs(float(rn[i]) - float(rn_ref[i])) / float(rn_ref[i])
        assert rerr <= max(TOL_RN, C_SPECTRAL * kappa[i]), (what, "rn", i, rerr, kappa[i])
    return float(err[acc].max()) if acc.any() else 0.0


def _both_routes(dev, sd, Nb, Nd, K, tr, what, layers=None):
    """Check (a) of the module docstring on every layer k >= 1 of the trace (or on `layers`); returns (accepted, total)."""
    m = _model(sd, Nb, Nd, K)
    D, n = Nb * Nd, Nb * Nd + 1
    tri = _tril(n)
    W = m.packed_weights(dev).cpu()
    lib = _lib.load()
    shapes = (4, 12) if D <= 128 else (12,)
    accepted, total, worst_sp, worst_eig, worst_ref, worst_kappa, lines = 0, 0, 0.0, 0.0, 0.0, 0.0, []
    for k in (range(1, K) if layers is None else layers):
        phi, h, Z = _mode0_inputs(tr, k)
        B = phi.shape[0]
        G_ref, w_ref, rn_ref = _reference(sd, k, phi, h, Z)
        kappa = _kappa(sd, k, w_ref)
        worst_kappa = max(worst_kappa, float(kappa.max()))
        hist = {}
        for waves in shapes:   # mode 0
            G0, rn0 = torch.full((B, n, n), SENT_G, dtype=torch.complex64), torch.full((B,), SENT_RN)
            Zo, G, rn, flag, st = _run(dev, m, k, phi, h, Z, G0, rn0, waves=waves)
            _check_status(flag, st)
            worst_sp = max(worst_sp, _check_accepted(G, rn, flag, G_ref, rn_ref, tri, kappa, (what, k, waves)))
            rej = flag != 0
            assert torch.equal(_bits(G[rej]), _bits(G0[rej])) and torch.equal(_bits(rn[rej]), _bits(rn0[rej]))
            assert torch.equal(_bits(Zo), _bits(Z))
            hist[waves] = dict(sorted(collections.Counter(flag.tolist()).items()))
            accepted += int((flag == 0).sum())
            total += B
        # modes 2 (layer 1: the stored Z is zero) and 1: the folded Z update of layer k-1, then G_k
        mode = 2 if k == 1 else 1
        p = tr[k - 1]
        phi_p, h_p, G_p = p["phi"].to(torch.complex64), p["h"].float(), p["G"].to(torch.complex64)
        alpha = p["arho"].float()
        Zs = tr[k - 2]["Z"].to(torch.complex64) if k >= 2 else torch.zeros(B, n, n, dtype=torch.complex64)
        corner_zp = float(W[lib.admmnet_layer_weight_offset(ctypes.byref(m.cfg()), k - 1) + S_CORNER_Z])
        C_p = R.block_matrix(phi_p.to(torch.complex128), h_p.double(), corner_zp)
        a64 = alpha.double().reshape(-1, 1, 1)
        Z_exp = Zs.to(torch.complex128) + a64 * (G_p.to(torch.complex128) - C_p)
        bound = 4 * U32 * (Zs.abs().double() + a64.abs() * (G_p.abs().double() + C_p.abs()))
        Zo, G, rn, flag, st = _run(dev, m, k, phi, h, Zs, G_p, torch.full((B,), SENT_RN), mode, (alpha, phi_p, h_p))
        bad = ((Zo.to(torch.complex128) - Z_exp).abs() > bound) & tri
        assert not bad.any(), (what, k, "fold", [tuple(i.tolist()) for i in bad.nonzero()[:8]])
        G_fref, _, rn_fref = _reference(sd, k, phi, h, Z_exp)
        worst_sp = max(worst_sp, _check_accepted(G, rn, flag, G_fref, rn_fref, tri, kappa, (what, k, f"mode {mode}")))
        _check_status(flag, st)
        # the eigensolver route on every matrix: G within max(TOL_G, C_EIGEN kappa); eigenvalues and rn within TOL_W / TOL_RN, or
        # 3x what the reference's own fp32 arithmetic (LAPACK eigh, the oracle in float32) does on that matrix, at most 10x
        Ge, we, rne = ops.glayer(m, k, phi.to(dev), h.to(dev), Z.to(dev))
        G32, w32, rn32 = _reference(sd, k, phi, h, Z, dtype=torch.float32)
        werr_of = lambda w: ((torch.sort(w.double(), 1).values - w_ref).abs().max(1).values /   # noqa: E731
                             w_ref.abs().max(1).values).numpy()
        rerr_of = lambda r: ((r.double() - rn_ref).abs() / rn_ref).numpy()                         # noqa: E731
        Ge, we, rne = Ge.cpu(), we.cpu(), rne.cpu()
        e, e32 = _g_errors(Ge, G_ref, tri), _g_errors(G32, G_ref, tri)
        assert (e <= np.maximum(TOL_G, C_EIGEN * kappa)).all(), (what, k, "eigensolver G", e, kappa)
        worst_eig, worst_ref = max(worst_eig, float(e.max())), max(worst_ref, float(e32.max()))
        for label, e, e32, tol in (("w", werr_of(we), werr_of(w32), TOL_W), ("rn", rerr_of(rne), rerr_of(rn32), TOL_RN)):
            assert (e <= np.clip(3 * e32, tol, 10 * tol)).all(), (what, k, "eigensolver " + label, e, e32)
        assert torch.equal(Ge, Ge.mH) and torch.all(Ge.diagonal(dim1=1, dim2=2).imag == 0), (what, k, "Hermitian")
        acc = {w: hist[w].get(0, 0) for w in shapes}
        lines.append(f"  layer {k}: accepted {acc} of {B}, flags {hist}")
    print(f"TRAINED {what} D={D}: accepted {accepted}/{total} ({100.0 * accepted / total:.1f} %), worst accepted G error "
          f"{worst_sp:.2e} (matrix function), {worst_eig:.2e} (eigensolver, every matrix; LAPACK fp32 {worst_ref:.2e}); "
          f"largest kappa {worst_kappa:.2e}")
    print("\n".join(lines))
    return accepted, total


@pytest.mark.parametrize("name", TRAINED + STATES)
def test_trained_fixture_both_routes_per_layer(dev, name):
    z, sd, (Nb, Nd, K), tr = _fixture(name)
    accepted, total = _both_routes(dev, sd, Nb, Nd, K, tr, name)
    assert accepted > 0, (name, "the matrix-function route accepted nothing")


EIGEN_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import admm_net_amd as A
from golden_util import load_fixture
dev = torch.device("cuda:0")
for name in {names!r}:
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load_fixture(os.path.join({root!r}, "tests", "golden", name + ".npz"))
    m = A.PhiEstADMMNet(M=Nb, N=Nd, L=L, num_layers=K)
    m.load_state_dict(sd)
    m.eval()
    y, b, s = (torch.from_numpy(z[k]).to(dev) for k in ("y", "b", "sigma"))
    phi = m(y, b, s)
    torch.cuda.synchronize()
    np.save(os.path.join({out!r}, name + ".npy"), phi.cpu().numpy())
    print("STATUS", name, json.dumps([int(v) for v in m.last_status]))
"""


def test_trained_fixtures_through_the_eigensolver_only(dev, tmp_path):
    """ADMMNET_SPECTRAL=0: every G-layer of every layer through the eigensolver pipeline, at the default route's tolerance
    (tests/test_gpu_parity.py::test_forward_matches_reference_fixture)."""
    env = dict(os.environ, ADMMNET_SPECTRAL="0")
    p = subprocess.run([sys.executable, "-c", EIGEN_CHILD.format(root=ROOT, names=TRAINED, out=str(tmp_path))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    status = {ln.split()[1]: ln for ln in p.stdout.splitlines() if ln.startswith("STATUS ")}
    for name in TRAINED:
        z, sd, (Nb, Nd, K), _ = _fixture(name)
        phi = np.load(os.path.join(str(tmp_path), name + ".npy"))
        y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
        ref = z["phi"]
        p64 = R.forward(sd, y, b, s, Nb, Nd, K, dtype="f64").numpy()
        yard = max(rel(ref, p64), ref_arith_error(sd, y, b, s, Nb, Nd, K, variants=4 if K >= 8 else 1))
        print(f"EIGEN_ONLY {name}: rel err {rel(phi, ref):.2e} vs reference, {rel(phi, p64):.2e} vs f64 (yardstick "
              f"{yard:.2e}); {status[name]}")
        assert rel(phi, ref) < TOL_PHI, name
        assert rel(phi, p64) <= 3 * yard + 2e-6, name
        st = json.loads(status[name].split(None, 2)[2])
        assert st[0] == 0 and st[2] == 0, (name, st)   # no eigensolver failure; not one matrix on the matrix-function route


GPU_TRAIN_GEOM = (10, 10, 10)


def _gpu_train(dev, batch=256, steps=300):
    """trainPhi.py's recipe on the product's training route; -> (state_dict on the host, losses)."""
    Nb, Nd, K = GPU_TRAIN_GEOM
    torch.manual_seed(41)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, L=3, num_layers=K).to(dev)
    m.train()
    params = [p for n, p in m.named_parameters() if any(s in n for s in ("phiLayers", "hLayers", "gLayers", "zLayers"))]
    assert len(params) == len(list(m.parameters()))
    opt = torch.optim.AdamW([{"params": params, "lr": 2.5e-3}], lr=5e-3, weight_decay=1e-3)
    losses = []
    for step in range(steps):
        y, b, s, extra = synth.make_batch_device(batch, Nb, Nd, seed=90210 + step, device=dev, labels=True)
        label = extra["phi"]
        opt.zero_grad(set_to_none=True)
        loss = (m(y, b, s) - label).abs().pow(2).mean() / label.abs().pow(2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().numpy()
    assert np.isfinite(losses).all()
    return {key: v.detach().cpu().clone() for key, v in m.state_dict().items()}, losses


def test_gpu_training_then_both_routes(dev, tmp_path):
    """300 steps of the reference's training recipe (trainPhi.py: 10 x 10, K = 10; AdamW lr 5e-3 with the ADMM-layer group
    at 0.5 lr, weight decay 1e-3; gradient norm clipped at 1.0) on the product's training route (model.train(), batch 256,
    labels of the classical solver from synth.make_batch_device, the normalised squared error of harness.time_train_step).
    Then the per-layer check of both routes and the forward against the float64 oracle on a held-out batch.  A failing state is saved under tmp_path, to be turned into a fixture."""
    Nb, Nd, K = GPU_TRAIN_GEOM
    sd, losses = _gpu_train(dev)
    print(f"GPU TRAINING {len(losses)} steps: loss {losses[:10].mean():.4f} (first 10) -> {losses[-10:].mean():.4f} (last 10)")
    path = os.path.join(str(tmp_path), "gpu_trained_10x10_K10.pt")
    torch.save(sd, path)
    try:
        y, b, s, _ = synth.make_batch(16, Nb, Nd, seed=4242)
        ty, tb, ts = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
        tr = []
        o64 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64", trace=tr).numpy()
        accepted, total = _both_routes(dev, sd, Nb, Nd, K, tr, "gpu-trained")
        assert accepted > 0
        me = _model(sd, Nb, Nd, K)
        phi = me(ty.to(dev), tb.to(dev), ts.to(dev)).cpu().numpy()
        o32 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f32").numpy()
        yard = max(rel(o32, o64), ref_arith_error(sd, ty, tb, ts, Nb, Nd, K, variants=3))
        print(f"GPU TRAINING forward: rel err {rel(phi, o32):.2e} vs oracle f32, {rel(phi, o64):.2e} vs f64 (yardstick "
              f"{yard:.2e}); G-layer routes {me.last_status}")
        assert rel(phi, o32) < TOL_PHI
        assert rel(phi, o64) <= 3 * yard + 2e-6
    except AssertionError:
        print(f"GPU TRAINING: the failing state_dict is saved at {path}")
        raise
