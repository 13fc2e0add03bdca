"""The alternative kernel paths stay correct: each A/B switch of INTEGRATION.md section 6 is read once per
process, so every variant runs in a child process on the golden fixtures of the reference and must meet the
same tolerance as the default path."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import glob, json, os, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
import admm_net_amd as A
dev = torch.device("cuda:0")
out = {{}}
for name in ("phiest_8x16_K3_perturbed", "admmnet_10x10_K3_default", "phiest_16x16_K3_perturbed",
             "phiest_12x16_K3_perturbed"):
    z = np.load(os.path.join({root!r}, "tests", "golden", name + ".npz"))
    Nb, Nd, K, B, L, head, s2d = [int(v) for v in z["meta"]]
    sd = {{k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}}
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, L=L, num_layers=K)
    m.load_state_dict(sd)
    m.eval()
    m.chunk = int(os.environ.get("ADMMNET_TEST_CHUNK", "0"))    # (several eigen-chunks for the variants that act across chunks)
    y, b, s = (torch.from_numpy(z[k]).to(dev) for k in ("y", "b", "sigma"))
    r = m(y, b, s)
    phi = (r[3] if head else r).cpu().numpy()
    ref = z["phi"]
    out[name] = float(np.abs(phi - ref).max() / np.abs(ref).max())
print("RESULT " + json.dumps(out))
"""

# The forward's default G-layer route is the matrix function of csrc/spectral_fused.hip, which leaves the eigensolver pipeline only
# the matrices it rejects: the A/B switches of that pipeline are therefore tested with ADMMNET_SPECTRAL=0 (every matrix through
# the eigensolver), and the matrix-function route has variants of its own.
EIGEN = {"ADMMNET_SPECTRAL": "0"}
VARIANTS = {
    "eigen_only": dict(EIGEN),
    "eig_ql": dict(EIGEN, ADMMNET_EIG="ql"),
    "no_arrow": dict(EIGEN, ADMMNET_ARROW="0"),
    "unfused_back": dict(EIGEN, ADMMNET_FUSE_BACK="0", ADMMNET_ARROW="0"),
    "tridiag_lds": dict(EIGEN, ADMMNET_TRIDIAG="lds", ADMMNET_ARROW="0"),
    "full_storage": dict(EIGEN, ADMMNET_LEAN="0"),
    # 128 < D <= 256: per-reflector register sweep + explicit Q + Q W; D = 192 runs at its own size instead of padded to 256
    "sweep_big": dict(EIGEN, ADMMNET_TRIDIAG_BIG="sweep"),
    "rebuild_tiles": dict(EIGEN, ADMMNET_REBUILD="tiles"),      # D = 256: rebuild_kernel instead of rebuild_big_kernel
    "explicit_q": dict(EIGEN, ADMMNET_BACK="q"),               # D = 256: panel tridiagonalisation, explicit Q + Q W
    "panel_one_stage": dict(EIGEN, ADMMNET_PN_SPLIT="0"),      # D = 256: the whole panel reduction in the 8-wave kernel
    "panel_two_stages": dict(EIGEN, ADMMNET_PN_SPLIT="8"),     # D = 256: panels 0..7 | 8..15 (default: 0..7 | 8..11 | 12..15)
    "two_streams": dict(EIGEN, ADMMNET_STREAMS="2", ADMMNET_TEST_CHUNK="1"),   # two chunks in flight (B = 2 .. 3 at chunk = 1)
    "dc_poison": dict(EIGEN, ADMMNET_DC_POISON="1"),           # D&C ping-pong buffers start as NaN instead of whatever they hold
    # the matrix-function route (default): several chunks on two streams; its multi-kernel form; every matrix rejected by the
    # model check (tolerance 0), i.e. the flag / skip machinery carrying the whole batch; full storage turns the route off
    "spectral_two_streams": {"ADMMNET_STREAMS": "2", "ADMMNET_TEST_CHUNK": "1"},
    "spectral_chunks": {"ADMMNET_TEST_CHUNK": "1"},
    "spectral_unfused": {"ADMMNET_SPECTRAL_FUSED": "0"},
    "spectral_no_fold": {"ADMMNET_SF_FOLD": "0"},          # the lazy Z update streamed by prep_kernel instead of the kernel's first sweep
    "spectral_all_rejected": {"ADMMNET_SPECTRAL_TOL": "0"},
    "spectral_one_pass_cap": {"ADMMNET_SPECTRAL_ITERS": "1"},   # (one subspace pass cannot pass the residual check either)
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_matches_reference_fixtures(variant):
    env = dict(os.environ, **VARIANTS[variant])
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    errs = json.loads(line[len("RESULT "):])
    assert len(errs) == 4
    for name, e in errs.items():
        assert e < 1e-4, (variant, name, e)


POISON_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from admm_net_amd import ops
rng = np.random.default_rng(3)
worst = 0.0
for n in (17, 65, 129, 130, 200, 257):
    mats = []
    X = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    mats.append((X + X.conj().T) / 2)                                            # generic: no deflation
    U = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    mats.append(0.3 * np.eye(n) + 1e-4 * np.diag(rng.standard_normal(n)) + U @ np.diag([5.0, -7.0, 2.0]) @ U.conj().T)
    Q, _ = np.linalg.qr(X)
    lam = np.repeat(rng.standard_normal(max(2, n // 8)), 8)[:n]                  # eightfold eigenvalues: rotations
    lam = np.concatenate([lam, rng.standard_normal(n - len(lam))])
    mats.append((Q * lam) @ Q.conj().T)
    mats.append(np.diag(rng.standard_normal(n)).astype(complex))                 # everything deflates
    A = np.stack([(M + M.conj().T) / 2 for M in mats]).astype(np.complex64)
    w, V = ops.eigh(torch.from_numpy(A).cuda())
    w, V = w.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.complex128)
    assert np.isfinite(w).all() and np.isfinite(V).all(), n
    A64 = A.astype(np.complex128)
    for i in range(len(mats)):
        sc = np.abs(A64[i]).max()
        worst = max(worst, np.abs(A64[i] @ V[i] - V[i] * w[i][None, :]).max() / sc,
                    np.abs(V[i].conj().T @ V[i] - np.eye(n)).max())
print("RESULT", worst)
"""


def test_dc_never_reads_an_unwritten_element():
    """dc_kernel does not clear its ping-pong eigenvector buffers (0.53 MB of zero writes per matrix at n = 257): rows of
    a source column outside its own block are zero by definition (a select), not by content, unless a deflation
    rotation filled them.  With the buffers poisoned by NaN, generic, clustered, multiple-eigenvalue and diagonal
    matrices must come back finite and accurate."""
    env = dict(os.environ, ADMMNET_DC_POISON="1")
    p = subprocess.run([sys.executable, "-c", POISON_CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    worst = float([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()[1])
    assert worst < 5e-5
