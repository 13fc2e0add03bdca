"""CPU: the arrowhead solver core (csrc/arrow_core.h) keeps its bits.

tests/golden/arrow_core_parent_sha256.json holds, for the six case kinds of test_arrow_fused_host.py at D = 1, 2, 3, 64, 127,
128, 129, 130, 192, 255, 256, the SHA-256 of
  roots : origin pole (int32) and tau (float32) of the k + 1 secular roots,
  zhat  : the k recomputed arrow entries (float32),
  G     : V f(Lambda) V^H of the sequential model of the fused first layer (complex64, tests/host_model/arrow_fused_model.cpp),
recorded from the host models built against the header as it was before the root solver read its poles from plain arrays
(ArrowPoles) and zeta-hat ran as two loops.  The tree's models must reproduce every one: the rewrite reorders memory accesses,
not floating-point operations.  The eigenvalue map is exact float32 arithmetic (no libm), so the hashes do not depend on it.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_arrow_fused_host import KINDS, arrow_case   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "arrow_core_parent_sha256.json")
DIMS = [1, 2, 3, 64, 127, 128, 129, 130, 192, 255, 256]


def load_models(root=ROOT):
    """(bits model, fused model) of the tree at `root`, built when missing or older than their sources."""
    csrc = os.path.join(root, "admm_net_amd", "csrc")
    cores = [os.path.join(csrc, f) for f in ("arrow_core.h", "dc_core.h", "eig_core.h")]
    libs = []
    for name in ("arrow_core_bits_model", "arrow_fused_model"):
        src = os.path.join(ROOT if name == "arrow_core_bits_model" else root, "tests", "host_model", name + ".cpp")
        so = os.path.join(root, "tests", "host_model", "lib%s.so" % name)
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + cores):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", csrc, src, "-o", so])
        libs.append(ctypes.CDLL(so))
    libs[0].arrow_core_bits.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 5
    libs[1].arrow_fused_g.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 6
    return libs


def sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def case(kind, D):
    """arrow_case(kind, D); its "mixed" recipe names pole 10, so below D = 11 the same recipe runs with that index clamped to
    the last pole (the slices clamp by themselves)."""
    if kind != "mixed" or D > 10:
        return arrow_case(kind, D)
    _, z, h = arrow_case("plain", D)
    h = np.sort(h); h[D - 1:20] = h[D - 1]; z[40:60] *= np.float32(1e-6); z = z * np.float32(10.0)
    return -0.7, z.astype(np.complex64), h.astype(np.float32)


def case_hashes(models, kind, D):
    bits, fused = models
    alpha, z, h = case(kind, D)
    n = D + 1
    org = np.full(n, -1, np.int32); tau = np.zeros(n, np.float32); zh = np.zeros(D, np.float32)
    k = bits.arrow_core_bits(D, alpha, z.ctypes.data, h.ctypes.data, org.ctypes.data, tau.ctypes.data, zh.ctypes.data)
    lam = np.zeros(n, np.float32); st = (ctypes.c_int * 4)()
    assert fused.arrow_fused_g(D, alpha, z.ctypes.data, h.ctypes.data, None, lam.ctypes.data, None, st) == 0
    f = lam * lam * np.float32(0.25) + np.float32(0.5)       # exact float32 operations
    G = np.zeros((n, n), np.complex64)
    assert fused.arrow_fused_g(D, alpha, z.ctypes.data, h.ctypes.data, f.ctypes.data, lam.ctypes.data, G.ctypes.data, st) == 0
    assert st[0] == k
    nr = k + 1 if k > 0 else 0
    return {"k": int(k), "roots": sha(org[:nr], tau[:nr]), "zhat": sha(zh[:k]), "G": sha(lam, G)}


def all_hashes(root=ROOT):
    models = load_models(root)
    return {"%s/%d" % (kind, D): case_hashes(models, kind, D) for D in DIMS for kind in KINDS}


@pytest.fixture(scope="module")
def models():
    return load_models()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("D", DIMS)
def test_core_bits_equal_recorded(models, golden, D):
    for kind in KINDS:
        got, want = case_hashes(models, kind, D), golden["%s/%d" % (kind, D)]
        assert got == want, (kind, D, got, want)


def test_cases_cover_the_paths(golden):
    """The recorded cases really contain what they are chosen for: full problems, deflated ones and a single pole."""
    ks = {key: v["k"] for key, v in golden.items()}
    assert ks["plain/256"] == 256 and ks["plain/129"] == 129 and ks["plain/1"] == 1
    assert ks["equal/256"] == 1 and ks["zeros/1"] == 0
    assert 0 < ks["zeros/192"] < 192 and 0 < ks["repeated/255"] < 255


if __name__ == "__main__":   # record: python tests/test_arrow_core_bits_host.py <tree whose header and fused model to use>
    out = all_hashes(os.path.abspath(sys.argv[1]))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "cases")
