"""The shared table of the eigensolver route tests (tests/test_eigh_cases_host.py on the CPU, tests/test_gpu_eigh_routes.py on
the device): option sets, sizes, matrices, metrics and bounds, and the guard the in-process device tests share.  Imports nothing
that needs a GPU (DeviceGuard.run imports torch and the library when it is called).

Sizes are D = n - 1, the dimension csrc/route.h routes on.  SMALL walks the template buckets of launch_tridiag_reg
(ceil(D / 16), edges D = 16 k | 16 k + 1) and the divide & conquer leaf edge n = 15 | 16; BIG walks the buckets of
launch_tridiag_big (ceil(D / 32)), the boundary 138 | 139 where tridiag=lds moves its matrix from LDS to the global image, and
the pad_min boundary 175 | 176 of spectral=0.

Bounds are the suite's own for the default route: res, orth < 3e-5 and ev < 1e-5 for the generic and the diagonal matrix
(test_gpu_parity.test_eigh_block), res, orth < 5e-5 for the layer-shaped and the multiple-eigenvalue one
(test_gpu_variants.test_dc_never_reads_an_unwritten_element) with the same ev < 1e-5.  float32 LAPACK stays below a quarter of
each on every matrix of the table (test_eigh_cases_host.py), so a miss on the device is the kernel's."""
import numpy as np

OPTION_SETS = {   # name: keyword arguments of admm_net_amd.Options
    "default": {},
    "eigen_only": dict(spectral=0),
    "ql": dict(eig="ql"),
    "lds": dict(tridiag="lds"),
    "lds_ql": dict(tridiag="lds", eig="ql"),        # the complete first-generation pipeline
    "sweep": dict(tridiag_big="sweep"),
    "explicit_q": dict(back="q"),
    "pn0": dict(pn_split=0),
    "pn8": dict(pn_split=8),
    "dc_plain": dict(dc_blocks=0),
    "tr_occ2": dict(tr_occ=2),
    "dc_occ4": dict(dc_occ=4),
    "dc_occ5": dict(dc_occ=5),
    "dc_occ6": dict(dc_occ=6),
    "dc_occ8": dict(dc_occ=8),
}

SMALL = [1, 2, 14, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128]
BIG = [129, 138, 139, 160, 161, 175, 176, 192, 193, 224, 225, 255, 256]
SIZE_CLASSES = {"small": SMALL, "big": BIG}
KINDS = ("gue", "diag", "layer", "eightfold")
BOUNDS = {   # kind: (res, orth, ev)
    "gue": (3e-5, 3e-5, 1e-5), "diag": (3e-5, 3e-5, 1e-5),
    "layer": (5e-5, 5e-5, 1e-5), "eightfold": (5e-5, 5e-5, 1e-5),
}


def sizes(name, size_class):
    """The D an option set runs in a size class: every one, but D = 128 and 256 only for the dc_occ* sets (separately compiled
    instances of one kernel, the largest matrix of each D&C variant) and none above 128 for tr_occ2 (a switch of tridiag_reg)."""
    if name.startswith("dc_occ"):
        return [D for D in SIZE_CLASSES[size_class] if D in (128, 256)]
    if name == "tr_occ2" and size_class == "big":
        return []
    return list(SIZE_CLASSES[size_class])


def cases():
    """(option set, size class) with at least one size."""
    return [(name, sc) for name in OPTION_SETS for sc in SIZE_CLASSES if sizes(name, sc)]


def environment(name):
    """An option set in the environment's spelling (ADMMNET_*), as Options writes it."""
    return {"ADMMNET_" + k.upper(): str(v) for k, v in OPTION_SETS[name].items()}


def _gue(rng, n):
    X = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return X, (X + X.conj().T) / 2


def matrices(n, more_gue=0):
    """[4 + more_gue, n, n] complex64, Hermitian: the four kinds in the order of KINDS, then further generic matrices.
    Generated in float64 from seed 1000 + n, symmetrised and cast."""
    rng = np.random.default_rng(1000 + n)
    X, gue = _gue(rng, n)
    diag = np.diag(rng.standard_normal(n)).astype(complex)       # every reflector the identity, everything deflates
    k = min(3, n - 1)
    U = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    layer = 0.3 * np.eye(n) + 1e-4 * np.diag(rng.standard_normal(n)) + U @ np.diag([5.0, -7.0, 2.0][:k]) @ U.conj().T
    Q, _ = np.linalg.qr(X)
    lam = np.repeat(rng.standard_normal(max(2, n // 8)), 8)[:n]   # eightfold eigenvalues: deflation by rotations
    lam = np.concatenate([lam, rng.standard_normal(n - len(lam))])
    eightfold = (Q * lam) @ Q.conj().T
    mats = [gue, diag, layer, eightfold] + [_gue(rng, n)[1] for _ in range(more_gue)]
    return np.stack([(M + M.conj().T) / 2 for M in mats]).astype(np.complex64)


def kind_of(i):
    return KINDS[i] if i < len(KINDS) else "gue"


def metrics(A, w, V):
    """(res, orth, ev, finite) of one returned (w, V) for the complex64 input A, in float64:
    res = max|A V - V diag(w)| / max|A|, orth = max|V^H V - I|, ev = max|sort(w) - eigvalsh(A)| / (max|A| max(1, n / 32))."""
    A64, w64, V64 = A.astype(np.complex128), np.asarray(w, np.float64), np.asarray(V).astype(np.complex128)
    n = A64.shape[-1]
    finite = bool(np.isfinite(w64).all() and np.isfinite(V64).all())
    if not finite:
        return float("inf"), float("inf"), float("inf"), False
    amax = np.abs(A64).max()
    res = np.abs(A64 @ V64 - V64 * w64[None, :]).max() / amax
    orth = np.abs(V64.conj().T @ V64 - np.eye(n)).max()
    ev = np.abs(np.sort(w64) - np.linalg.eigvalsh(A64)).max() / (amax * max(1.0, n / 32))
    return float(res), float(orth), float(ev), finite


def within(kind, m, fraction=1.0):
    """Whether the metrics m meet `fraction` of the bounds of `kind`."""
    return m[3] and all(v < fraction * b for v, b in zip(m[:3], BOUNDS[kind]))


def lapack32(A):
    """float32 LAPACK on one complex64 matrix: the yardstick the bounds are set against."""
    w, V = np.linalg.eigh(A.astype(np.complex64))
    assert w.dtype == np.float32 and V.dtype == np.complex64
    return w, V


E_HIP = -2   # ADMMNET_E_HIP of include/admmnet.h; _lib.check writes it into its message as "(code -2)"


def is_hip_error(e):
    """An AdmmNetError that carries ADMMNET_E_HIP, or a HIP RuntimeError of torch."""
    from admm_net_amd import _lib
    text = str(e)
    if isinstance(e, _lib.AdmmNetError):
        return "(code %d)" % E_HIP in text
    return isinstance(e, RuntimeError) and ("HIP error" in text or "hipError" in text)


class DeviceGuard:
    """Device hygiene of a test file whose cases share one process: once a case meets a HIP error, the remaining cases fail at
    once without touching the device.  No retries."""

    def __init__(self):
        self.first = None   # the first HIP error met, one line of it

    def run(self, fn):
        """fn() on the device, synchronised, unless an earlier case met a HIP error; a HIP error met here is remembered."""
        import pytest
        import torch
        if self.first is not None:
            pytest.fail("not run: an earlier case of this file met a HIP error (%s)" % self.first)
        assert torch.cuda.is_available(), "these tests need the MI355X"
        try:
            out = fn()
            torch.cuda.synchronize()
            return out
        except RuntimeError as e:   # (AdmmNetError is one)
            if is_hip_error(e):
                self.first = (str(e).splitlines() or ["?"])[0][:200]
            raise
