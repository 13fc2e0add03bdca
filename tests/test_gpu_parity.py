"""GPU (-m gpu): parity of the HIP path, called through the C ABI, against the oracle, the golden
fixtures generated from the reference, and size-independent properties at the BASELINE sizes.

Tolerances (fp32 path, stated per north_star):
  * phi: max-abs error <= 1e-4 * max|phi| against the reference fixtures.  The reference itself sits
    6e-7 .. 7e-6 from the float64 evaluation of its own formulas (tests/test_oracle_golden.py); the HIP
    path is additionally required to be no further than 3x the reference's own distance + 2e-6.
    At the cfg3 depth (K = 16, n = 257) fp32 round-off of ANY implementation reaches 1e-4: tolerance 5e-4.
  * G (one layer): 2e-5 relative; eigenvalues 1e-5 relative to the spectral radius.
  * spectrum (float64): 1e-10 relative; peak indices bit-exact.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, ops, peak_search, sharded, synth
from oracle import admm_net_ref as R
from golden_util import load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = sorted(p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))
              if os.path.basename(p).startswith(("phiest_", "admmnet_")))
TOL_PHI = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def load_case(p):
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load_fixture(p)
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, L=L, num_layers=K)
    m.load_state_dict(sd)
    return z, m.eval(), sd, (Nb, Nd, K, B, L, head, s2d)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def ref_arith_error(sd, y, b, s, Nb, Nd, K, L=3, head=False, variants=4):
    """How far the REFERENCE arithmetic (the oracle's fp32 evaluation = admm_net.py on LAPACK) lands from float64 on
    this problem, as a range rather than one sample: the same problem with y scaled by (1 + k 2^-22), k = 0 .. 3 --
    last-bit changes of the input.  At depth the unrolled iteration amplifies rounding noise chaotically, so the distance
    of ONE fp32 evaluation is a draw from a distribution (tests/gpu_bisect_cfg3.py: over seeds the HIP / LAPACK distance
    ratio scatters 0.2 .. 2.5 around a geometric mean of 1.0); the largest of a few draws is the yardstick."""
    errs = []
    for k in range(variants):
        yk = (y.to(torch.complex128) * (1.0 + k * 2.0 ** -22)).to(torch.complex64)
        o32 = R.forward(sd, yk, b, s, Nb, Nd, K, L, dtype="f32", head=head)
        o64 = R.forward(sd, yk, b, s, Nb, Nd, K, L, dtype="f64", head=head)
        o32, o64 = (o32[3] if head else o32).numpy(), (o64[3] if head else o64).numpy()
        errs.append(rel(o32, o64))
    return max(errs)


# ------------------------------------------------------------------ building blocks
@pytest.mark.parametrize("n", [2, 3, 10, 17, 65, 101, 129, 130, 169, 200, 229, 256, 257])
def test_eigh_block(dev, n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((6, n, n)) + 1j * rng.standard_normal((6, n, n))
    Ah = ((X + X.conj().transpose(0, 2, 1)) / 2).astype(np.complex64)
    Ah[5] = np.diag(rng.standard_normal(n)).astype(np.complex64)          # already diagonal: tau = 0 path
    w, V = ops.eigh(torch.from_numpy(Ah).to(dev))
    w, V = w.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.complex128)
    A64 = Ah.astype(np.complex128)
    assert np.abs(A64 @ V - V * w[:, None, :]).max() < 3e-5 * np.abs(A64).max()
    assert np.abs(V.conj().transpose(0, 2, 1) @ V - np.eye(n)).max() < 3e-5
    assert np.abs(np.sort(w, 1) - np.linalg.eigvalsh(A64)).max() < 1e-5 * np.abs(A64).max() * max(1, n / 32)


@pytest.mark.parametrize("n", [129, 257])
@pytest.mark.parametrize("scale", [1e-17, 1e-10, 1e-5, 1e8, 1e16])
def test_eigh_is_scale_invariant(dev, n, scale):
    """torch.linalg.eigh (LAPACK) works at any scale: sstedc normalises T (slascl) before the merges, whose
    deflation tests are absolute on a unit-norm matrix -- dc_kernel does the same with a power of two; and at n = 257
    column norms squared outside 1e-30 .. 1e30 take the pre / post scaling of the panel kernel's branch-free reflector
    (tridiag_panel.hip, pn_householder).  Eigenvalues scale linearly, eigenvectors do not change."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((3, n, n)) + 1j * rng.standard_normal((3, n, n))
    A1 = ((X + X.conj().transpose(0, 2, 1)) / 2).astype(np.complex64)
    As = (A1.astype(np.complex128) * scale).astype(np.complex64)
    w, V = ops.eigh(torch.from_numpy(As).to(dev))
    w, V = w.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.complex128)
    A64 = As.astype(np.complex128)
    amax = np.abs(A64).max()
    assert np.isfinite(w).all() and np.isfinite(V).all()
    assert np.abs(A64 @ V - V * w[:, None, :]).max() < 3e-5 * amax
    assert np.abs(V.conj().transpose(0, 2, 1) @ V - np.eye(n)).max() < 3e-5
    assert np.abs(np.sort(w, 1) - np.linalg.eigvalsh(A64)).max() < 1e-5 * amax * n / 32


def test_eigh_graded_and_clustered(dev):
    """(scalar I + tiny diagonal + large low rank): the shape of the real layer matrices, where a QL
    sweep in the wrong direction stalls -- exercises the direction choice of the QL kernel."""
    n, rng = 129, np.random.default_rng(5)
    mats = []
    for scale in (1.0, 50.0, 1000.0):
        U = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
        M = 0.003 * np.eye(n) + np.diag(1e-4 * rng.standard_normal(n)) + scale * U @ np.diag([5.0, -7.0, 2.0]) @ U.conj().T
        mats.append((M + M.conj().T) / 2)
        mats.append(mats[-1][::-1, ::-1].copy())                             # graded the other way
    Ah = np.stack(mats).astype(np.complex64)
    w, V = ops.eigh(torch.from_numpy(Ah).to(dev))
    w, V = w.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.complex128)
    A64 = Ah.astype(np.complex128)
    rec = (V * w[:, None, :]) @ V.conj().transpose(0, 2, 1)
    for i in range(len(mats)):
        assert np.abs(rec[i] - A64[i]).max() < 3e-5 * np.abs(A64[i]).max()
        assert np.abs(V[i].conj().T @ V[i] - np.eye(n)).max() < 3e-5


def test_glayer_block_vs_oracle(dev):
    z, m, sd, (Nb, Nd, K, B, L, head, _) = load_case(os.path.join(ROOT, "tests/golden/phiest_8x16_K3_perturbed.npz"))
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    tr = []
    R.forward(sd, y, b, s, Nb, Nd, K, L, dtype="f64", trace=tr)
    for k, t in enumerate(tr):
        Zin = None if k == 0 else tr[k - 1]["Z"].to(torch.complex64).to(dev)
        G, w, rn = ops.glayer(m, k, t["phi"].to(torch.complex64).to(dev), t["h"].float().to(dev), Zin)
        G = G.cpu().numpy()
        assert rel(G, t["G"].numpy()) < 2e-5
        assert np.array_equal(G, G.conj().transpose(0, 2, 1))               # exactly Hermitian, as admm_net.py:352
        assert np.all(G[:, np.arange(G.shape[1]), np.arange(G.shape[1])].imag == 0)
        assert rel(np.sort(w.cpu().numpy(), 1), t["w"].numpy()) < 1e-5
        assert rel(rn.cpu().numpy(), t["rn"].numpy()) < 1e-5


@pytest.mark.parametrize("fixture", ["phiest_8x16_K3_perturbed", "phiest_16x16_K3_perturbed"],
                         ids=["fused_D128", "global_image_D256"])
def test_glayer_first_layer_arrowhead_edge_cases(dev, fixture):
    """Layer 0 (Z = 0) runs the direct arrowhead eigensolver (arrow.hip; D <= 128 fused with the rebuild, larger D
    through the global eigenvector image): repeated h (rotation deflation), zero phi entries (trivial deflation),
    all-equal h, strong coupling -- against the oracle's G-layer in f64."""
    z, m, sd, (Nb, Nd, K, B, L, head, _) = load_case(os.path.join(ROOT, f"tests/golden/{fixture}.npz"))
    D = Nb * Nd
    rng = np.random.default_rng(17)
    phis, hs = [], []
    for case in range(6):
        h = rng.uniform(0.05, 1.0, D)
        p = (rng.standard_normal(D) + 1j * rng.standard_normal(D)) * 0.1
        if case == 1: h = np.round(h, 2)
        if case == 2: p[::3] = 0
        if case == 3: h[:] = 0.37
        if case == 4: p *= 40
        if case == 5: h = np.sort(h); h[10:30] = h[10]; p[50:70] *= 1e-7
        phis.append(p); hs.append(h)
    phi = torch.from_numpy(np.stack(phis)).to(torch.complex128)
    h = torch.from_numpy(np.stack(hs)).to(torch.float64)
    sd64 = {k_: (v.double() if v.is_floating_point() else v) for k_, v in sd.items()}
    Zero = torch.zeros(phi.shape[0], D + 1, D + 1, dtype=torch.complex128)
    Gref, wref, _ = R.g_layer(sd64, 0, phi, h, Zero, return_eig=True)
    G, w, rn = ops.glayer(m, 0, phi.to(torch.complex64).to(dev), h.float().to(dev), None)
    G = G.cpu().numpy()
    assert rel(G, Gref.numpy()) < 2e-5
    assert np.array_equal(G, G.conj().transpose(0, 2, 1))
    assert rel(np.sort(w.cpu().numpy(), 1), wref.numpy()) < 1e-5
    _, rn_ref, _ = R.z_layer(sd64, 0, phi, h, Gref, Zero, return_aux=True)   # residual norm of the Z-layer (its own corner)
    assert rel(rn.cpu().numpy(), rn_ref.numpy()) < 2e-5


# ------------------------------------------------------------------ whole forward vs the reference
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_forward_matches_reference_fixture(dev, path):
    z, m, sd, (Nb, Nd, K, B, L, head, s2d) = load_case(path)
    y, b = torch.from_numpy(z["y"]), torch.from_numpy(z["b"])
    s = torch.from_numpy(z["sigma"])
    if s2d:
        s = s.reshape(-1, 1)                                                  # both shapes occur
    out = m(y, b, s)                                                          # CPU in, CPU out; no no_grad: as main_for_net.py
    phi = out[3] if head else out
    assert phi.device.type == "cpu" and phi.dtype == torch.complex64 and not phi.requires_grad
    ref = z["phi"]
    e_ref = rel(phi.numpy(), ref)
    assert e_ref < TOL_PHI
    p64 = R.forward(sd, y, b, s, Nb, Nd, K, L, dtype="f64", head=bool(head))
    p64 = (p64[3] if head else p64).numpy()
    # distance to float64: within 3x the reference arithmetic's own distance (the reference's stored result and, because
    # that distance is a draw from a distribution at depth, the oracle's fp32 evaluation on last-bit-perturbed inputs)
    yard = max(rel(ref, p64), ref_arith_error(sd, y, b, s.reshape(-1), Nb, Nd, K, L, head=bool(head),
                                              variants=4 if K >= 8 else 1))
    assert rel(phi.numpy(), p64) <= 3 * yard + 2e-6
    if head:
        for i, key in enumerate(["tau", "f", "conf"]):
            assert out[i].shape == (B, L) and out[i].dtype == torch.float32
            assert np.abs(out[i].numpy() - z[key]).max() < 2e-5


@pytest.mark.parametrize("shape", [(10, 10, 10, 12, 0.0), (10, 10, 5, 9, 0.5), (8, 16, 8, 10, 0.5), (16, 16, 4, 4, 0.5),
                                   (1, 1, 3, 5, 0.5), (2, 1, 2, 1, 0.0), (5, 7, 1, 9, 0.5)])
def test_forward_vs_oracle_seeded(dev, shape):
    Nb, Nd, K, B, pert = shape
    sd = R.make_weights(Nb, Nd, K, seed=Nb * 100 + K, head=True, perturb=pert)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    missing = m.load_state_dict(sd, strict=True)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=B)
    ty, tb, ts = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    tau, f, conf, phi = m(ty.to(dev), tb.to(dev), ts.to(dev))
    assert phi.is_cuda
    o32 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f32", head=True)
    o64 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64", head=True)
    assert rel(phi.cpu().numpy(), o32[3].numpy()) < TOL_PHI
    yard = max(rel(o32[3].numpy(), o64[3].numpy()),
               ref_arith_error(sd, ty, tb, ts, Nb, Nd, K, head=True, variants=3) if K >= 4 else 0.0)
    assert rel(phi.cpu().numpy(), o64[3].numpy()) <= 3 * yard + 2e-6
    for a, r in zip((tau, f, conf), o32[:3]):
        assert np.abs(a.cpu().numpy() - r.numpy()).max() < 5e-5


@pytest.mark.parametrize("geom", [(8, 16), (16, 16)], ids=["D128", "D256"])
@pytest.mark.parametrize("yscale", [1e-6, 1e-3, 1e3])
def test_forward_with_small_and_large_measurements(dev, geom, yscale):
    """The reference runs on LAPACK, which is scale invariant; measurements in volts or in ADC counts must not change
    which path is numerically safe here either (the D&C's deflation tests are absolute on the unit-norm T)."""
    Nb, Nd = geom
    K, B = 3, 3
    sd = R.make_weights(Nb, Nd, K, seed=5, head=False, perturb=0.3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd, strict=True)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=17)
    ty, tb, ts = torch.from_numpy((y * yscale).astype(np.complex64)), torch.from_numpy(b), torch.from_numpy(s)
    phi = m(ty.to(dev), tb.to(dev), ts.to(dev)).cpu().numpy()
    o64 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64").numpy()
    o32 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f32").numpy()
    assert np.isfinite(phi).all()
    assert rel(phi, o64) <= 3 * rel(o32, o64) + 1e-5


def test_forward_is_bitwise_reproducible(dev):
    """Same inputs, same bits: the D&C places by counting (no append-by-atomic), the batch mean is a fixed-order float64
    sum, no kernel accumulates through floating-point atomics."""
    Nb, Nd, K, B = 16, 16, 4, 24
    sd = R.make_weights(Nb, Nd, K, seed=11, head=True, perturb=0.3)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd, strict=True)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=23)
    ty, tb, ts = torch.from_numpy(y).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
    outs = [tuple(o.cpu().numpy().copy() for o in m(ty, tb, ts)) for _ in range(3)]
    for o in outs[1:]:
        for a0, a1 in zip(outs[0], o):
            assert np.array_equal(a0, a1)


def test_chunking_is_invisible(dev):
    """Eigensolver work chunks (workspace reuse) must not change anything."""
    Nb, Nd, K, B = 4, 5, 3, 37
    torch.manual_seed(3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=1)
    args = [torch.from_numpy(v).to(dev) for v in (y, b, s)]
    m.chunk = 0
    ref = m(*args).cpu()
    m.chunk = 8          # (the setter drops the cached workspace)
    assert torch.equal(m(*args).cpu(), ref)


@pytest.mark.parametrize("grid", [(16, 16), (12, 16)])
def test_chunking_is_invisible_on_the_large_matrix_pipeline(dev, grid):
    """The same for the D > 128 pipeline (half-image prep, panel tridiagonalisation with its per-chunk T factors and
    hand-over tiles, D&C buffers, block-reflector back-transform, resident-tile rebuild): the `b0 * n * n` offsets of
    the lower-triangle G / Z state and the reuse of every chunk buffer across chunks.  B = 5 at chunk = 2 is three
    chunks, the last one ragged; head outputs included (ADMMNet)."""
    Nb, Nd = grid
    K, B = 3, 5
    torch.manual_seed(8)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=4)
    args = [torch.from_numpy(v).to(dev) for v in (y, b, s)]
    m.chunk = 0
    ref = [o.cpu() for o in m(*args)]
    m.chunk = 2
    got = [o.cpu() for o in m(*args)]
    for a0, a1 in zip(ref, got):
        assert torch.equal(a0, a1)


@pytest.mark.parametrize("chunk", [512, 600])
@pytest.mark.parametrize("grid", [(10, 10), (8, 16)])
def test_chunking_is_invisible_across_the_workgroup_shapes(dev, grid, chunk):
    """The matrix-function kernel has two workgroup shapes at D <= 128 (4 waves per matrix for calls of more than 512
    signals, 12 below) that sum in different orders: the shape must follow the call, not the chunk.  B = 1100 at chunk = 512
    is the chunks 512, 512, 76; at chunk = 600 the chunks 600 and 500 lie on both sides of the switch."""
    Nb, Nd = grid
    K, B = 4, 1100
    sd = R.make_weights(Nb, Nd, K, seed=9, head=False, perturb=0.3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd)
    args = synth.make_batch_device(B, Nb, Nd, seed=31, device=dev)[:3]
    m.chunk = 0
    ref = m(*args).cpu()
    assert m.last_status[2] > 0
    m.chunk = chunk
    assert torch.equal(m(*args).cpu(), ref)


def test_ragged_last_chunk_is_invisible_at_cfg2(dev):
    """B = 8292 at the default chunk (8192) leaves a ragged tail of 100 signals -- the same bits as one chunk of 8292."""
    Nb, Nd, K, B = 8, 16, 4, 8292
    sd = R.make_weights(Nb, Nd, K, seed=10, head=False, perturb=0.3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd)
    args = synth.make_batch_device(B, Nb, Nd, seed=32, device=dev)[:3]
    m.chunk = 0
    ref = m(*args).cpu()
    m.chunk = B
    assert torch.equal(m(*args).cpu(), ref)


def test_layer_api_and_sharded_single_rank(dev):
    Nb, Nd, K, B = 6, 6, 4, 20
    torch.manual_seed(4)
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=2)
    args = [torch.from_numpy(v).to(dev) for v in (y, b, s)]
    tau, f, conf, phi = m(*args)
    sphi, shead = sharded.ShardedForward(m, scope="global")(*args)
    assert torch.equal(sphi, phi) and torch.equal(shead[0], tau) and torch.equal(shead[2], conf)
    # 'shard' scope on two halves == two independent forwards (reference semantics on sub-batches)
    h = B // 2
    a = m(*[t[:h] for t in args])[3]
    c = sharded.ShardedForward(m, scope="shard")(*[t[:h] for t in args])[0]
    assert torch.equal(a, c)


@pytest.mark.parametrize("geom", [(8, 16, 4), (16, 16, 3)], ids=["8x16", "16x16"])
def test_degenerate_inputs_match_oracle(dev, geom):
    """Edge inputs of the data domain: an all-zero observation (phi = 0: the arrowhead layer deflates everything,
    later layers see diagonal + corner matrices), a single non-zero sample, a batch of one, identical signals
    (equal residual norms in the batch mean), a huge and a tiny overall scale."""
    Nb, Nd, K = geom
    torch.manual_seed(6)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    y, b, s, _ = synth.make_batch(6, Nb, Nd, seed=9)
    y[0] = 0
    y[1] = 0
    y[1, 5] = 1.0 + 0.5j
    y[2] = y[3]
    b[2] = b[3]
    s[2] = s[3]
    y[4] *= 1e3
    y[5] *= 1e-4
    for sl in (slice(0, 6), slice(0, 1)):
        ty, tb, ts = (torch.from_numpy(v[sl]) for v in (y, b, s))
        ref = R.forward(sd, ty, tb, ts, Nb, Nd, K, 3, dtype="f64").numpy()
        got = m(ty.to(dev), tb.to(dev), ts.to(dev)).cpu().numpy()
        assert np.isfinite(got).all()
        # per signal: the scales differ by 1e7 across the batch
        for i in range(got.shape[0]):
            den = max(np.abs(ref[i]).max(), 1e-30)
            assert np.abs(got[i] - ref[i]).max() <= 2e-4 * den + 1e-12, (i, np.abs(got[i] - ref[i]).max(), den)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("geom", [(3, 3), (16, 16), (12, 16), (10, 16)])
def test_fails_loudly_on_nonfinite_input(dev, K, geom):
    """torch.linalg.eigh raises on non-finite input (admm_net.py:303); so must every eigen-path: K = 2 has the arrowhead
    solver as its ONLY G-layer (arrow.hip), K = 3 adds a dense layer; 16x16 takes the D = 256 kernels, 12x16 the same
    pipeline on the padded matrix (the back-transform follows the D&C's column map, which the early exit must still
    write), 10x16 the per-reflector sweep at its own size."""
    Nb, Nd = geom
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    y, b, s, _ = synth.make_batch(2, Nb, Nd, seed=1)
    for bad in (np.nan, np.inf):
        yy = y.copy()
        yy[0, 0] = bad
        with pytest.raises(_lib.AdmmNetError):
            m(torch.from_numpy(yy).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev))
    # and the single G-layer entry point with Z = None (arrowhead path)
    phi = torch.from_numpy(y[:, :]).to(dev)
    h = torch.rand(2, Nb * Nd, device=dev)
    h[1, 2] = float("nan")
    with pytest.raises(_lib.AdmmNetError):
        ops.glayer(m, 0, phi, h, None)


def test_bad_shapes_raise(dev):
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2).eval()
    with pytest.raises(ValueError):
        m(torch.zeros(2, 8, dtype=torch.complex64), torch.zeros(2, 8, dtype=torch.complex64), torch.ones(2))
    with pytest.raises(_lib.AdmmNetError):
        ops.eigh(torch.zeros(1, 3, 3, dtype=torch.complex64))               # CPU tensor: no fallback


# ------------------------------------------------------------------ properties at the BASELINE sizes
def test_cfg2_full_batch_properties(dev):
    """BASELINE cfg 2 (K=8, D=128, B=4096): too big for the oracle in seconds -> properties.
    (i) a sub-batch evaluated by the oracle with the full-batch means injected agrees;
    (ii) permuting the batch permutes the output (the only coupling is the batch mean)."""
    Nb, Nd, K, B = 8, 16, 8, 4096
    torch.manual_seed(0)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=20260104)
    ty, tb, ts = (torch.from_numpy(v).to(dev) for v in (y, b, s))
    phi = m(ty, tb, ts)
    assert torch.isfinite(torch.view_as_real(phi)).all()
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(dev)
    phi_p = m(ty[perm], tb[perm], ts[perm])
    assert rel(phi_p.cpu().numpy(), phi[perm].cpu().numpy()) < 2e-5
    # oracle on 6 signals, batch means taken from a layer-wise HIP run of the full batch
    eng = sharded.HipLayerEngine(m, ty, tb, ts)
    eng.begin()
    means = []
    for k in range(K):
        sc = eng.front(k)
        if k == K - 1:
            break
        means.append(float(sc[0].item()) / B)
        eng.back(k, sc[0] / sc[1])
    phi2, _ = eng.finish()
    assert torch.equal(phi2, phi)
    sd = {k_: v.detach() for k_, v in m.state_dict().items()}
    idx = torch.tensor([0, 1, 777, 2048, 4000, 4095])
    o = R.forward(sd, torch.from_numpy(y)[idx], torch.from_numpy(b)[idx], torch.from_numpy(s)[idx], Nb, Nd, K,
                  dtype="f64", skip_dead_tail=True,
                  mean_norm_fn=lambda k, rn: torch.tensor(means[k], dtype=rn.dtype))
    assert rel(phi[idx.to(dev)].cpu().numpy(), o.numpy()) < TOL_PHI


def test_deep_accuracy_is_statistically_the_references(dev):
    """is the D > 128 pipeline systematically less accurate than the reference arithmetic at cfg3 depth?
    tests/gpu_bisect_cfg3.py: fed identical inputs, every G-layer of the HIP path is as close to float64 as LAPACK's
    fp32 eigh (2e-7 .. 5e-6, either one ahead), and over weight / data seeds the end-to-end distance ratio
    hip / lapack32 scatters 0.5 .. 2.3 around a geometric mean of 1.00.  Pinned here: over 6 seeds at K = 16, n = 257
    the geometric mean of that ratio stays below 1.6, no seed exceeds 4, and every result is 1e-4-class."""
    Nb, Nd, K = 16, 16, 16
    ratios = []
    for seed in range(6):
        sd = R.make_weights(Nb, Nd, K, seed=100 + seed, head=False, perturb=0.3 if seed % 2 else 0.0)
        m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
        m.load_state_dict(sd)
        y, b, s, _ = synth.make_batch(2, Nb, Nd, seed=200 + seed)
        ty, tb, ts = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
        phi = m(ty.to(dev), tb.to(dev), ts.to(dev)).cpu().numpy()
        o32 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f32").numpy()
        o64 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64").numpy()
        assert rel(phi, o64) < TOL_PHI and rel(phi, o32) < TOL_PHI
        ratios.append(rel(phi, o64) / rel(o32, o64))
    assert max(ratios) < 4.0, ratios
    assert float(np.exp(np.mean(np.log(ratios)))) < 1.6, ratios


@pytest.mark.timeout(900)
def test_cfg3_full_batch_properties(dev):
    """BASELINE cfg 3 at ITS size (K = 16, D = 256, B = 65 536: eight eigen-chunks of 8192, ~90 GB of state, 5 s per
    forward on the MI355X) -- far beyond the oracle, so properties, as for cfg 2:
    (i) the layer-at-a-time forward (what bench.py times) equals the one-call forward bit for bit;
    (ii) six signals spread over the chunks, evaluated by the float64 oracle with the full-batch means of the HIP run
         injected, agree to the fp32 tolerance -- this pins the chunked D = 256 pipeline at the bench's own geometry;
    (iii) reversing the batch reverses the output (the only coupling is the batch mean; a reversal moves every signal
          to a different chunk and chunk position)."""
    Nb, Nd, K, B = 16, 16, 16, 65536
    free, _total = torch.cuda.mem_get_info(dev)
    if free < 120e9:
        pytest.skip("needs ~100 GB of free HBM")
    torch.manual_seed(0)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    ty, tb, ts, _ = synth.make_batch_device(B, Nb, Nd, seed=20260104, device=dev)
    phi = m(ty, tb, ts)
    assert torch.isfinite(torch.view_as_real(phi)).all()
    eng = sharded.HipLayerEngine(m, ty, tb, ts)
    eng.begin()
    means = []
    for k in range(K):
        sc = eng.front(k)
        if k == K - 1:
            break
        means.append(float(sc[0].item()) / B)
        eng.back(k, sc[0] / sc[1])
    phi2, _ = eng.finish()
    assert torch.equal(phi2, phi)
    idx = torch.tensor([0, 8191, 8192, 30000, 57344, 65535])
    sd = {k_: v.detach() for k_, v in m.state_dict().items()}
    o = R.forward(sd, ty[idx.to(dev)].cpu(), tb[idx.to(dev)].cpu(), ts[idx.to(dev)].cpu(), Nb, Nd, K, dtype="f64",
                  skip_dead_tail=True, mean_norm_fn=lambda k, rn: torch.tensor(means[k], dtype=rn.dtype))
    assert rel(phi[idx.to(dev)].cpu().numpy(), o.numpy()) < TOL_PHI
    keep = phi[idx.to(dev)].clone()
    del phi, phi2
    phi_r = m(ty.flip(0), tb.flip(0), ts.flip(0))
    assert rel(phi_r[(B - 1 - idx).to(dev)].cpu().numpy(), keep.cpu().numpy()) < 2e-5


def test_cfg3_shape_small_batch(dev):
    """BASELINE cfg 3/4/5 geometry (D=256, n=257, K=16) on a batch the oracle finishes in seconds."""
    Nb, Nd, K, B = 16, 16, 16, 3
    sd = R.make_weights(Nb, Nd, K, seed=7, head=False, perturb=0.3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    m.load_state_dict(sd)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=5)
    ty, tb, ts = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    phi = m(ty.to(dev), tb.to(dev), ts.to(dev)).cpu().numpy()
    o32 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f32").numpy()
    o64 = R.forward(sd, ty, tb, ts, Nb, Nd, K, dtype="f64").numpy()
    # 15 dense 257x257 eigen-functions deep: same bound as every other case -- no further from float64 than 3x the
    # reference arithmetic's own distance (+2e-6) -- with that distance taken over last-bit-perturbed copies of the input
    # (ref_arith_error), and 1e-4-class against the fp32 evaluation.  (tests/gpu_bisect_cfg3.py: each G-layer of this
    # case, fed identical inputs, is as close to float64 as LAPACK's fp32 eigh, 2e-7 .. 5e-6, either one ahead.)
    yard = max(rel(o32, o64), ref_arith_error(sd, ty, tb, ts, Nb, Nd, K))
    assert rel(phi, o64) <= 3 * yard + 2e-6
    assert rel(phi, o32) <= 3 * TOL_PHI


# ------------------------------------------------------------------ spectrum / peak search
# Expected values come from oracle/peak_search_ref.py: the LITERAL restatement of utils/peakSearchUtils.py (one
# kron + dot per grid point, flood-fill regional maxima).  skimage is not installed here and the reference records
# no expected outputs, so parity with skimage.local_maxima itself is UNPINNED (definition-level only).
from oracle import peak_search_ref as PO   # noqa: E402


def _top(rows, k=3):
    return rows[np.argsort(-rows[:, 2], kind="stable")][:k]


def test_spectrum_and_peak_indices(dev):
    """ops.spectrum against the literal double loop (peakSearchUtils.py:37-60) and the regional-maxima indices of
    both images (bit-exact), then the whole device peak search against alt_peak_search as written (:63-173)."""
    Nb = Nd = 10
    y, b, s, truth = synth.make_batch(4, Nb, Nd, seed=11, snr_range=(20.0, 20.0))
    torch.manual_seed(1)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=4).eval()
    phi = m(torch.from_numpy(y).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev))
    opts = {"xstep": 1 / (10 * Nd), "ystep": 1 / (10 * Nb), "iter": 3}        # main_for_net.py:112-116
    ax, ay = peak_search.coarse_axes(opts)
    Zg = ops.spectrum(phi, Nb, Nd, torch.from_numpy(ax), torch.from_numpy(ay))
    mask_dev = ops.regional_maxima(Zg).cpu().numpy()
    Zg = Zg.cpu().numpy()
    ph = phi.cpu().numpy()
    X, Y = np.meshgrid(ax, ay)
    got = peak_search.batched_peak_search(phi, Nb, Nd, opts, top=3)
    for i in range(4):
        Zo = PO.peak_search(ph[i].astype(np.complex128), X, Nb, Y, Nd)          # oracle: 99 x 99 kron + dot
        assert np.abs(Zg[i] - Zo).max() < 1e-10 * Zo.max()
        want = PO.regional_maxima_floodfill(Zo)
        assert np.array_equal(mask_dev[i], want)                                 # indices bit-exact
        assert np.array_equal(PO.regional_maxima_floodfill(Zg[i]), want)
        host = _top(PO.alt_peak_search_literal({"phi": ph[i].astype(np.complex128), "xbase": Nb, "ybase": Nd}, opts))
        assert np.array_equal(got[i][:, :2], host[:, :2])                        # refined (tau, f) bit-exact
        assert np.abs(got[i][:, 2] - host[:, 2]).max() < 1e-9 * host[:, 2].max()


@pytest.mark.parametrize("geom", [(10, 10, 1), (8, 16, 2), (16, 16, 1)], ids=["10x10", "8x16", "16x16"])
def test_device_peak_search_matches_oracle(dev, geom):
    """ops.peak_search (spectrum + regional maxima + refinement on the device, peaks.hip) against the oracle's
    literal alt_peak_search on the same phi: same maxima in the same (np.where) order, coordinates bit-exact,
    heights to float64 rounding.  The product's host mirror must agree as well."""
    Nb, Nd, iters = geom
    y, b, s, _ = synth.make_batch(6, Nb, Nd, seed=23, snr_range=(10.0, 20.0))
    torch.manual_seed(2)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=3).eval()
    phi = m(torch.from_numpy(y).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev))
    opts = {"xstep": 1 / (4 * Nd), "ystep": 1 / (4 * Nb), "iter": iters}
    pk, cnt = ops.peak_search(phi, Nb, Nd, opts, max_peaks=512)
    pk, cnt = pk.cpu().numpy(), cnt.cpu().numpy()
    ph = phi.cpu().numpy()
    for i in range(ph.shape[0]):
        want = PO.alt_peak_search_literal({"phi": ph[i].astype(np.complex128), "xbase": Nb, "ybase": Nd}, opts)
        assert cnt[i] == want.shape[0] and cnt[i] > 0
        got = pk[i, :cnt[i]]
        assert np.array_equal(got[:, :2], want[:, :2])
        assert np.abs(got[:, 2] - want[:, 2]).max() <= 1e-9 * want[:, 2].max()
        assert not pk[i, cnt[i]:].any()
        mirror = peak_search.alt_peak_search({"phi": ph[i], "xbase": Nb, "ybase": Nd}, opts)
        assert np.array_equal(mirror[:, :2], want[:, :2])


def test_regional_maxima_known_inputs_on_device(dev):
    """The reference's own example image (peakSearchUtils.py:427-432: a 2 x 2 plateau of 5s in a 4 x 5 matrix; it
    prints the mask, records none) plus plateau-rich random images, on the device path, against the flood fill."""
    imgs = [np.array([[1, 2, 3, 2, 1], [2, 5, 5, 3, 2], [3, 5, 5, 4, 3], [2, 3, 4, 3, 2]], dtype=np.float64)]
    want0 = np.zeros((4, 5), dtype=bool)
    want0[1:3, 1:3] = True                                       # the plateau is the one regional maximum
    rng = np.random.default_rng(3)
    for levels in (2, 3, 5, 50):
        imgs.append(rng.integers(0, levels, size=(4, 5)).astype(np.float64))
    imgs.append(np.full((4, 5), 7.0))                             # constant image: no maximum
    got = ops.regional_maxima(torch.from_numpy(np.stack(imgs)).to(dev)).cpu().numpy()
    assert np.array_equal(got[0], want0)
    for g, im in zip(got, imgs):
        assert np.array_equal(g, PO.regional_maxima_floodfill(im))
    big = rng.integers(0, 4, size=(3, 37, 41)).astype(np.float64)  # ragged sizes, many touching plateaus
    gb = ops.regional_maxima(torch.from_numpy(big).to(dev)).cpu().numpy()
    for g, im in zip(gb, big):
        assert np.array_equal(g, PO.regional_maxima_floodfill(im))


def test_delta_phi_known_input_on_device(dev):
    """The reference's test_peak_searching input (peakSearchUtils.py:360-394): phi = e_2 of length 400 (20 x 20),
    step 0.02, two refinement rounds.  |phi^H a|^2 = 1 at EVERY grid point, so which pixels are 'maxima' is decided
    by rounding noise of the evaluation (a numerical tie everywhere; the reference prints whatever it gets and records
    nothing): indices are not comparable between two evaluations.  What is checked: the device returns maxima, every
    height is 1 to rounding and every refined position lies on the grid range, as for the oracle."""
    phi = np.zeros(400, dtype=np.complex64)
    phi[2] = 1.0
    opts = {"xstep": 0.02, "ystep": 0.02, "iter": 2}
    pk, cnt = ops.peak_search(torch.from_numpy(phi[None]).to(dev), 20, 20, opts, max_peaks=2048)
    pk, cnt = pk.cpu().numpy()[0], int(cnt.cpu()[0])
    want = PO.alt_peak_search_literal({"phi": phi.astype(np.complex128), "xbase": 20, "ybase": 20}, opts)
    for rows in (pk[:min(cnt, 2048)], want):
        assert rows.shape[0] > 0
        assert np.abs(rows[:, 2] - 1.0).max() < 1e-12
        assert rows[:, 0].min() >= 0.0 and rows[:, 0].max() <= 1.0 and np.abs(rows[:, 1]).max() <= 0.5


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_peaks_of_hip_phi_equal_peaks_of_reference_phi(dev, path):
    """north_star: 'recovered peak indices bit-exact' end to end.  For every golden fixture the coarse regional-maxima
    indices and the refined (tau, f) of the top-3 peaks computed from phi_HIP equal those computed (by the oracle's
    literal peak search) from the REFERENCE's phi stored in the fixture."""
    z, m, sd, (Nb, Nd, K, B, L, head, s2d) = load_case(path)
    if Nb * Nd < 9:
        pytest.skip("grid too small for a peak search")
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    out = m(y.to(dev), b.to(dev), s.to(dev))
    phi = out[3] if head else out
    opts = {"xstep": 1 / (4 * Nd), "ystep": 1 / (4 * Nb), "iter": 2}
    ax, ay = peak_search.coarse_axes(opts)
    X, Y = np.meshgrid(ax, ay)
    mask = ops.regional_maxima(ops.spectrum(phi, Nb, Nd, torch.from_numpy(ax), torch.from_numpy(ay))).cpu().numpy()
    got = peak_search.batched_peak_search(phi, Nb, Nd, opts, top=3, max_peaks=1024)
    for i in range(B):
        ref_phi = z["phi"][i].astype(np.complex128)
        Zr = PO.peak_search(ref_phi, X, Nb, Y, Nd)
        want_mask = PO.regional_maxima_floodfill(Zr)
        # a maximum whose margin over a neighbour is below the fp32 difference of the two phis is a numerical tie
        # (none occurs on these fixtures; the assertion is exact)
        assert np.array_equal(mask[i], want_mask)
        want = _top(PO.alt_peak_search_literal({"phi": ref_phi, "xbase": Nb, "ybase": Nd}, opts))
        # refined positions: same arg-max cell of the same np.arange grids
        assert np.array_equal(got[i][:, :2], want[:, :2]), (got[i], want)
        assert np.abs(got[i][:, 2] - want[:, 2]).max() <= 5e-4 * want[:, 2].max()
