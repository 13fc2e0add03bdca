"""GPU (-m gpu): the first G-layer at 128 < D <= 256 -- the fused arrowhead kernel (csrc/arrow.hip, arrow_fused_tail:
eigenvector slabs in LDS, real S on the matrix cores, phases in the epilogue) and, behind ADMMNET_ARROW_FUSED=0, the
former pair of kernels -- against the float64 oracle R.g_layer(..., Z = 0).

Bounds (both forms): rel(G) < 2e-5, sorted eigenvalues < 1e-5, rn < 2e-5, G == G^H exactly; non-finite input is counted
in `status` (ops.glayer raises); >= 16 384 matrices at D = 256 are bitwise reproducible, and a matrix's bits depend
neither on its index in the launch nor on the chunk size.

Run as a script (`python tests/test_gpu_arrow_fused.py accuracy`) it performs the accuracy checks in this process: the
test of the two-kernel form starts that as a child with the switch set, since the library reads its switches once.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import admm_net_amd as A                      # noqa: E402
from admm_net_amd import _lib, ops, synth     # noqa: E402
from oracle import admm_net_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu
GEOM = {129: (3, 43), 160: (10, 16), 192: (12, 16), 255: (15, 17), 256: (16, 16)}   # D -> (M, N)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def make_model(D):
    Nb, Nd = GEOM[D]
    sd = R.make_weights(Nb, Nd, 2, seed=D, head=False, perturb=0.3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=2).eval()
    m.load_state_dict(sd)
    return m, sd, Nb, Nd


def edge_cases(D):
    """The six cases of test_gpu_parity.test_glayer_first_layer_arrowhead_edge_cases at dimension D."""
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
    return torch.from_numpy(np.stack(phis)).to(torch.complex128), torch.from_numpy(np.stack(hs)).to(torch.float64)


def layer0_inputs(sd, Nb, Nd, B=6):
    """phi and h as the first G-layer of a forward really sees them: synthetic signals through the model's first prep."""
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=Nb * Nd)
    tr = []
    R.forward(sd, torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s), Nb, Nd, 2, dtype="f64", trace=tr)
    return tr[0]["phi"].to(torch.complex128), tr[0]["h"].to(torch.float64)


def check_accuracy(D, dev):
    m, sd, Nb, Nd = make_model(D)
    sd64 = {k_: (v.double() if v.is_floating_point() else v) for k_, v in sd.items()}
    for name, (phi, h) in (("edge", edge_cases(D)), ("layer0", layer0_inputs(sd, Nb, Nd))):
        Zero = torch.zeros(phi.shape[0], D + 1, D + 1, dtype=torch.complex128)
        Gref, wref, _ = R.g_layer(sd64, 0, phi, h, Zero, return_eig=True)
        _, rn_ref, _ = R.z_layer(sd64, 0, phi, h, Gref, Zero, return_aux=True)
        G, w, rn = ops.glayer(m, 0, phi.to(torch.complex64).to(dev), h.float().to(dev), None)
        G = G.cpu().numpy()
        eg, ew = rel(G, Gref.numpy()), rel(np.sort(w.cpu().numpy(), 1), wref.numpy())
        er = rel(rn.cpu().numpy(), rn_ref.numpy())
        herm = bool(np.array_equal(G, G.conj().transpose(0, 2, 1)))
        print(f"D={D} {name}: rel(G) {eg:.2e}  eigenvalues {ew:.2e}  rn {er:.2e}  hermitian {herm}", flush=True)
        assert eg < 2e-5
        assert herm
        assert np.all(G[:, np.arange(D + 1), np.arange(D + 1)].imag == 0)
        assert ew < 1e-5
        assert er < 2e-5


@pytest.mark.parametrize("D", sorted(GEOM))
def test_fused_first_layer_vs_oracle(dev, D):
    assert os.environ.get("ADMMNET_ARROW_FUSED", "1") != "0", "this test pins the default (fused) form"
    check_accuracy(D, dev)


def test_two_kernel_form_vs_oracle_in_child_process():
    """ADMMNET_ARROW_FUSED=0 (image in global memory + the dense path's rebuild kernel): the same bounds."""
    env = dict(os.environ, ADMMNET_ARROW_FUSED="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "accuracy"], env=env, capture_output=True, text=True,
                       timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("rel(G)") == 2 * len(GEOM)


@pytest.mark.parametrize("D", [129, 256])
def test_nonfinite_input_is_counted(dev, D):
    """The contract of test_gpu_parity.test_fails_loudly_on_nonfinite_input on this kernel: NaN / Inf in phi or h is
    reported through `status` (the workgroup leaves before the sort, nothing is written), and the next call is sound."""
    m, sd, Nb, Nd = make_model(D)
    phi, h = edge_cases(D)
    phi, h = phi.to(torch.complex64).to(dev), h.float().to(dev)
    for bad in (float("nan"), float("inf")):
        hb = h.clone(); hb[1, 2] = bad
        with pytest.raises(_lib.AdmmNetError):
            ops.glayer(m, 0, phi, hb, None)
        pb = phi.clone(); pb[4, D - 1] = complex(bad, 0.0)
        with pytest.raises(_lib.AdmmNetError):
            ops.glayer(m, 0, pb, h, None)
    G, w, rn = ops.glayer(m, 0, phi, h, None)
    assert torch.isfinite(torch.view_as_real(G)).all() and torch.isfinite(w).all() and torch.isfinite(rn).all()


def test_bitwise_reproducible_at_scale(dev):
    """16 384 matrices at D = 256 (every 64th with repeated h: the rotation path), twice: equal bits.  A sample of them
    alone, in another order, and the first 4096 with another chunk size: the same bits per matrix."""
    D, B = 256, 16384
    m, sd, Nb, Nd = make_model(D)
    gen = torch.Generator(device=dev).manual_seed(5)
    h = torch.rand(B, D, device=dev, generator=gen) * 0.95 + 0.05
    h[::64] = torch.round(h[::64] * 100) / 100
    phi = torch.complex(torch.randn(B, D, device=dev, generator=gen), torch.randn(B, D, device=dev, generator=gen)) * 0.1
    G1, w1, rn1 = ops.glayer(m, 0, phi, h, None)
    G2, w2, rn2 = ops.glayer(m, 0, phi, h, None)
    assert torch.equal(torch.view_as_real(G1), torch.view_as_real(G2))
    assert torch.equal(w1, w2) and torch.equal(rn1, rn2)
    del G2
    idx = torch.from_numpy(np.random.default_rng(1).permutation(B)[:320]).to(dev)
    idx[:8] = torch.arange(0, 512, 64, device=dev)             # some of the rotation cases among them
    G3, w3, rn3 = ops.glayer(m, 0, phi[idx], h[idx], None)
    assert torch.equal(torch.view_as_real(G3), torch.view_as_real(G1[idx]))
    assert torch.equal(w3, w1[idx]) and torch.equal(rn3, rn1[idx])
    m.chunk = 1000
    G4, w4, rn4 = ops.glayer(m, 0, phi[:4096], h[:4096], None)
    assert torch.equal(torch.view_as_real(G4), torch.view_as_real(G1[:4096]))
    assert torch.equal(w4, w1[:4096]) and torch.equal(rn4, rn1[:4096])


if __name__ == "__main__":
    if sys.argv[1:] == ["accuracy"]:
        torch.set_num_threads(min(4, os.cpu_count() or 1))
        device = torch.device("cuda:0")
        _lib.load()
        for D_ in sorted(GEOM):
            check_accuracy(D_, device)
    else:
        sys.exit("usage: test_gpu_arrow_fused.py accuracy")
