"""GPU (-m gpu): the slabs of the matrix-function G-layer kernel (csrc/spectral_fused.hip, P2 / P3) at the sizes where their
staging and their readers change path.  The border row of E^2 reads each slab with 16-byte LDS reads, a quarter slab ahead of its
multiply-adds, and whatever stages or reads the slabs must not change a value.  What can go wrong shows at particular sizes -- n at,
one past and two past a slab (D = 31, 32, 33; 63, 64, 65; 95, 96), the change of shape (128, 129), slabs whose work does not divide
by the waves (160, 192, 224), column 256 (255, 256):

  1. equal bits against the parent commit: the lower triangles of G and Z, rn and the flags of every case have the SHA-256 values
     recorded from a build of the parent (tests/golden/sf_staging_parent_sha256.json, written by
     tests/golden/make_sf_staging_golden.py, which runs THIS module's case builder).  The file also holds the parent's flags and
     the seeds of each size: the first pair of SEED_CANDIDATES with which the parent accepts at least 4 of the 5 matrices in
     every case of that size (a case in which everything is rejected pins nothing): (7, 13), the default of the pipeline
     module, everywhere except D = 63, 128 and 129, which take (2, 13) as they do there;
  2. the float64 oracle at the sizes tests/test_gpu_sf_pipeline.py does not have, with its bounds;
  3. NaN above the diagonal of Z and of the incoming G changes no output bit, and nothing above the diagonal or in the guard
     matrices around the B matrices is written: the staging reads the lower triangle only.

All through ops.glayer_spectral, B = 5 matrices per case, update modes 0, 1, 2, both shapes where D <= 128.
"""
import functools
import hashlib
import json
import os

import pytest
import torch

import test_gpu_sf_pipeline as P
from test_gpu_glayer_route import _bits, _check_accepted, _check_status, _tril

pytestmark = pytest.mark.gpu

B = P.B
SIZES = (31, 32, 33, 63, 64, 65, 95, 96, 128, 129, 160, 192, 224, 255, 256)
NEW_SIZES = tuple(D for D in SIZES if D not in P.EDGES)          # (the oracle test of the pipeline module has the others)
# grids of the sizes the pipeline module's table lacks (its builders look the grid up there: entries are only ever added)
for _D, _grid in {31: (1, 31), 32: (4, 8), 33: (3, 11), 95: (5, 19), 96: (8, 12), 160: (10, 16), 224: (14, 16)}.items():
    P.GRIDS.setdefault(_D, _grid)
SEED_CANDIDATES = ((7, 13), (2, 13), (3, 13), (5, 13), (7, 5), (2, 5), (11, 3), (4, 9))   # (weights, signals)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sf_staging_parent_sha256.json")
CASES = P._cases(SIZES)


def case_id(D, waves, mode):
    return f"D{D}-W{waves}-mode{mode}"


def shapes_of(D):
    return (12, 4) if D <= 128 else (12,)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def seeds_of(D):
    return tuple(_golden()["seeds"][str(D)])


def _sha(t):
    return hashlib.sha256(_bits(t).numpy().tobytes()).hexdigest()


def run_case(dev, D, waves, mode, seeds, poison=False):
    """One call on the inputs of the pipeline module (layer 2, or 1 in mode 2, of an oracle forward of B signals), between two
    guard matrices.  poison: NaN above the diagonal of Z and of the incoming G.  Returns the inputs and the host images."""
    x = P._inputs(D, mode, seeds)
    Z, G = x["Z"].clone(), x["G"].clone()
    if poison:
        upper = ~_tril(D + 1)
        Z[:, upper] = P.NAN
        G[:, upper] = P.NAN
    Zo, Go, rn, flag, st = P._run(dev, D, waves, mode, Z, G, seeds)
    return dict(x=x, Zin=Z, Gin=G, Z=Zo, G=Go, rn=rn, flag=flag, st=st)


def digest(r):
    """What a case is pinned by: SHA-256 of the lower triangles of G and Z (the B matrices), of rn and of the flags."""
    tri = _tril(r["Z"].shape[-1])
    return {"G": _sha(r["G"][1:B + 1][:, tri]), "Z": _sha(r["Z"][1:B + 1][:, tri]), "rn": _sha(r["rn"]), "flag": _sha(r["flag"]),
            "flags": r["flag"].tolist()}


@pytest.fixture(scope="module")
def dev():
    from admm_net_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _clean(D, waves, mode):
    """The un-poisoned run of a case, shared by the three tests and never modified."""
    return run_case(torch.device("cuda:0"), D, waves, mode, seeds_of(D))


# ------------------------------------------------------------------------------------------------------ 1. the parent's bits
@pytest.mark.parametrize("D,waves,mode", CASES)
def test_slabs_give_the_parents_bits(dev, D, waves, mode):
    want = _golden()["cases"][case_id(D, waves, mode)]
    assert sum(f == 0 for f in want["flags"]) >= 4, want["flags"]      # (the recording's promise: the case pins something)
    got = digest(_clean(D, waves, mode))
    print(f"SFSTAGE {case_id(D, waves, mode)}: seeds {seeds_of(D)} flags {got['flags']}")
    assert got == want


# ------------------------------------------------------------------------------------------------------- 2. the float64 oracle
@pytest.mark.parametrize("D,waves,mode", P._cases(NEW_SIZES))
def test_new_sizes_match_the_oracle(dev, D, waves, mode):
    r = _clean(D, waves, mode)
    x, tri = r["x"], _tril(D + 1)
    Zo, G, rn, flag = r["Z"][1:B + 1], r["G"][1:B + 1], r["rn"], r["flag"]
    _check_status(flag, r["st"])
    if mode == 0:
        assert torch.equal(_bits(Zo), _bits(x["Z"]))
    else:
        dz = (Zo.to(torch.complex128) - x["Z_exp"]).abs()
        bad = (dz > x["bound"]) & tri
        assert not bad.any(), ("fold", [tuple(i.tolist()) for i in bad.nonzero()[:8]], float((dz - x["bound"])[bad].max()))
    worst = _check_accepted(G, rn, flag, x["G_ref"], x["rn_ref"], tri, case_id(D, waves, mode))
    rej = flag != 0
    assert torch.equal(_bits(G[rej]), _bits(x["G"][rej])) and bool((rn[rej] == P.SENT_RN).all())
    print(f"SFSTAGE {case_id(D, waves, mode)}: flags {flag.tolist()} worst G error {worst:.2e}")
    assert int(rej.sum()) <= 1


# ---------------------------------------------------------------------------------------------- 3. poison above the diagonal
@pytest.mark.parametrize("D,waves,mode", CASES)
def test_nan_above_the_diagonal_changes_no_bit(dev, D, waves, mode):
    n = D + 1
    tri = _tril(n)
    upper = ~tri
    a = _clean(D, waves, mode)
    b = run_case(dev, D, waves, mode, seeds_of(D), poison=True)
    guard = _bits(torch.full((n, n), P.NAN, dtype=torch.complex64))
    for r in (a, b):   # what lies above the diagonal and around the B matrices is as it was
        for out, src in ((r["Z"], r["Zin"]), (r["G"], r["Gin"])):
            assert torch.equal(_bits(out[1:B + 1])[:, upper], _bits(src)[:, upper])
            assert torch.equal(_bits(out[0]), guard) and torch.equal(_bits(out[B + 1]), guard)
    assert torch.equal(a["flag"], b["flag"]), (a["flag"].tolist(), b["flag"].tolist())
    assert torch.equal(a["st"], b["st"])
    assert torch.isfinite(b["Z"][1:B + 1][:, tri]).all() and torch.isfinite(b["G"][1:B + 1][:, tri]).all()
    for name in ("G", "Z"):
        assert torch.equal(_bits(a[name][1:B + 1])[:, tri], _bits(b[name][1:B + 1])[:, tri]), name
    assert torch.equal(_bits(a["rn"]), _bits(b["rn"]))
    assert (a["flag"] == 0).any()
