"""CPU: the fused first G-layer at D > 128 (csrc/arrow.hip, arrow_fused_tail) as a sequential host model.

tests/host_model/arrow_fused_model.cpp runs the solver cores of arrow_core.h / dc_core.h and then the kernel's own
formulas -- real eigenvector entries, rotations row by row, real S as an fma chain, phases, arrow row, corner -- and is
compared with V diag(f) V^H from numpy.linalg.eigh in float64.  Bounds: G within 2e-5 of max|G| (the bound
test_glayer_first_layer_arrowhead_edge_cases puts on this path on the GPU), G exactly Hermitian, diagonal exactly real.
The last test compiles arrow.hip for gfx950 and reads the resource-usage remarks of the fused kernel: no scratch.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")
KINDS = ["plain", "repeated", "zeros", "equal", "strong", "mixed"]


@pytest.fixture(scope="module")
def model():
    so = os.path.join(ROOT, "tests", "host_model", "libarrow_fused_model.so")
    src = os.path.join(ROOT, "tests", "host_model", "arrow_fused_model.cpp")
    cores = [os.path.join(CSRC, f) for f in ("arrow_core.h", "dc_core.h", "eig_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + cores):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.arrow_fused_g.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 6
    return lib


def arrow_case(kind, D, seed=3):
    """The case kinds of test_host_logic.arrow_cases() at a chosen D: plain, repeated h (rotation deflation), zero arrow
    entries (trivial deflation), all-equal h (D - 1 rotations), strong coupling, mixed."""
    rng = np.random.default_rng(seed + D)
    h = rng.uniform(0.1, 1.0, D)
    z = (rng.standard_normal(D) + 1j * rng.standard_normal(D)) * 0.1
    alpha = 2.5
    if kind == "repeated": h = np.round(h, 2)
    if kind == "zeros": z[::3] = 0
    if kind == "equal": h[:] = 0.5
    if kind == "strong": alpha, z = -3.0, z * 30
    if kind == "mixed":
        h = np.sort(h); h[10:20] = h[10]; z[40:60] *= 1e-6; z *= 10.0; alpha = -0.7
    return alpha, z.astype(np.complex64), h.astype(np.float32)


def eig_map(lam):
    """A map shaped like the layer's: softplus(lam - thr) times a sigmoid gate of |lam| (smooth, so equal eigenvalues get
    equal values and the result does not depend on the basis of an eigenspace)."""
    lam = np.asarray(lam, np.float64)
    return np.logaddexp(0.0, lam - 0.6) / (1.0 + np.exp(-(0.8 * np.abs(lam) - 0.3)))


@pytest.mark.parametrize("D", [129, 192, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_model_vs_eigh(model, kind, D):
    alpha, z, h = arrow_case(kind, D)
    n = D + 1
    lam = np.zeros(n, np.float32); st = (ctypes.c_int * 4)()
    assert model.arrow_fused_g(D, alpha, z.ctypes.data, h.ctypes.data, None, lam.ctypes.data, None, st) == 0
    assert np.all(np.diff(lam) >= 0)
    f = eig_map(lam).astype(np.float32)
    G = np.zeros((n, n), np.complex64)
    assert model.arrow_fused_g(D, alpha, z.ctypes.data, h.ctypes.data, f.ctypes.data, lam.ctypes.data, G.ctypes.data, st) == 0
    C = np.zeros((n, n), np.complex128)                      # the layer's order: arrow last
    C[:D, :D] = np.diag(h.astype(np.float64)); C[:D, D] = z; C[D, :D] = z.conj(); C[D, D] = alpha
    w, V = np.linalg.eigh(C)
    Gref = (V * eig_map(w)) @ V.conj().T
    err = np.abs(G - Gref).max() / np.abs(Gref).max()
    print(f"{kind} D={D}: k={st[0]} rotations={st[2]} rel err {err:.2e}")
    # eigenvalues: ~30 ulp of float32 at the spectral radius (the scale every root's rounding error is relative to)
    assert np.abs(lam - w).max() < 2e-6 * np.abs(w).max()
    assert err < 2e-5
    assert np.array_equal(G, G.conj().T)                     # exactly Hermitian
    assert np.all(np.diagonal(G).imag == 0)                  # diagonal exactly real
    if kind == "equal":
        assert st[2] == D - 1                                # the heavy rotation case really is one
    if kind in ("repeated", "mixed"):
        assert st[2] > 0
    if kind == "zeros":
        assert st[1] >= (D + 2) // 3 and st[2] == 0


def test_fused_kernel_compiles_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 on arrow.hip: the fused kernel (mode 2 of arrow_rebuild_kernel) keeps all nine
    accumulator tiles in registers -- no scratch, no spilled vector registers, two waves per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    from admm_net_amd import build as B
    r = subprocess.run([hipcc] + B.FLAGS + B.EXTRA_FLAGS.get("arrow.hip", []) +
                       ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "arrow.hip"), "-o",
                        str(tmp_path / "arrow.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)
    mine = [b for b in blocks if b.startswith("_ZN7admmnet20arrow_rebuild_kernelILi2E")]
    assert len(mine) == 1, [b[:60] for b in blocks]
    get = lambda key: int(re.search(re.escape(key) + r": (\d+)", mine[0]).group(1))
    print({k: get(k) for k in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]")})
    assert get("ScratchSize [bytes/lane]") == 0
    assert get("VGPRs Spill") == 0
    assert get("Occupancy [waves/SIMD]") >= 2
