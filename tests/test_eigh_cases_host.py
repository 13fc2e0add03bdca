"""CPU: the table of tests/eigh_cases.py is fair and complete.

Fair: float32 LAPACK (numpy.linalg.eigh on complex64) stays below a quarter of each bound on every matrix the device tests
run, so tests/test_gpu_eigh_routes.py never blames a kernel for a hard input.  Complete: the kernels admmnet_eigh_c64_o
launches for every (option set, size) of the table, derived from csrc/route.h through tests/host_model/route_model the way
tests/test_route_host.py does, contain every template instance and every back-transform the launchers dispatch on -- a table
edit that loses one fails here, not silently on the device."""
import os
import re

import numpy as np
import pytest

import eigh_cases as E
from test_route_host import CSRC, model, read_routes   # noqa: F401  (model: the fixture that builds and runs route_model)


# ---- 1. the reference meets the bounds --------------------------------------------------------------------------------------
def test_tables_are_the_issue_sets():
    assert len(E.SMALL) == 20 and len(E.BIG) == 13 and max(E.SMALL) == 128 and min(E.BIG) == 129 and max(E.BIG) == 256
    for k in range(1, 8):
        assert 16 * k in E.SMALL and 16 * k + 1 in E.SMALL            # tridiag_reg bucket edges
    for D in (14, 15, 138, 139, 160, 161, 175, 176, 192, 193, 224, 225):
        assert D in E.SMALL + E.BIG
    assert [E.sizes("dc_occ8", sc) for sc in ("small", "big")] == [[128], [256]]
    assert E.sizes("tr_occ2", "small") == E.SMALL and ("tr_occ2", "big") not in E.cases()
    assert len(E.cases()) == 2 * len(E.OPTION_SETS) - 1


@pytest.mark.parametrize("size_class", list(E.SIZE_CLASSES))
def test_float32_lapack_stays_within_a_quarter_of_every_bound(size_class):
    worst = {}
    for D in E.SIZE_CLASSES[size_class]:
        n = D + 1
        # (the three further generic matrices are those of the batch-position and chunk-boundary tests)
        A = E.matrices(n, more_gue=3)
        assert A.dtype == np.complex64 and np.array_equal(A, A.conj().transpose(0, 2, 1))
        for i in range(len(A)):
            kind = E.kind_of(i)
            m = E.metrics(A[i], *E.lapack32(A[i]))
            assert E.within(kind, m, 0.25), (D, i, kind, m)
            worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0, 0, 0)), m[:3]))
    print(size_class, {k: tuple(f"{v:.1e}" for v in w) for k, w in worst.items()})


def test_metrics_see_a_wrong_eigenvector():
    """The metrics are sharper than the forward tests: a rotation inside a well-separated pair, which V f(L) V^H forgives
    when f is flat there, fails res; a lost orthogonality fails orth; a swapped batch neighbour fails everything."""
    A = E.matrices(33)
    w, V = E.lapack32(A[0])
    assert E.within("gue", E.metrics(A[0], w, V))
    c, s = np.cos(1e-2), np.sin(1e-2)
    Vr = V.copy()
    Vr[:, 0], Vr[:, 1] = c * V[:, 0] + s * V[:, 1], -s * V[:, 0] + c * V[:, 1]
    assert not E.within("gue", E.metrics(A[0], w, Vr))
    Vs = V.copy()
    Vs[:, 3] = V[:, 3] + 1e-3 * V[:, 4]
    assert not E.within("gue", E.metrics(A[0], w, Vs))
    assert not E.within("layer", E.metrics(A[2], w, V))
    Vn = V.copy()
    Vn[5, 5] = np.nan
    assert not E.within("gue", E.metrics(A[0], w, Vn))


# ---- 2. the table reaches every kernel --------------------------------------------------------------------------------------
def _td_parts():
    """TD_PARTS of tridiag.hip, read once: the one constant of td_lds_bytes() that is tuned."""
    with open(os.path.join(CSRC, "tridiag.hip")) as fh:
        return int(re.search(r"constexpr int TD_PARTS = (\d+);", fh.read()).group(1))


TD_PARTS = _td_parts()


def td_lds_image(D):
    """tridiag.hip, launch_tridiag: the matrix stays in LDS while td_lds_bytes(D, true) <= 160 KiB -- float2 vectors
    v, w, v0s, taus and TD_PARTS partial sums of Dp = D rounded up to 4, 16 scratch entries, D rows of pitch D + 2."""
    Dp = (D + 3) & ~3
    return 8 * (Dp * (4 + TD_PARTS) + 16) + 8 * D * (D + 2) <= 160 * 1024


def launched(r, sw):
    """What admmnet_eigh_c64_o launches for one route (api.hip eig_chunk with io == nullptr, and the launchers behind it):
    (tridiagonalisation, template bucket or image, explicit Q, tridiagonal solver, back-transform, padded, pn_split)."""
    D, E_ = int(r["D"]), int(r["eig_dim"])
    td = r["tridiag"]
    if td == "reg":
        inst = -(-E_ // 16)
    elif td in ("sweep", "panel"):
        inst = -(-E_ // 32)
    else:
        inst = "lds_image" if td_lds_image(E_) else "global_image"
    blocks = sw.get("ADMMNET_DC_BLOCKS") != "0"
    solver = "ql" if r["dc"] == "0" else ("dc_block" if E_ + 1 > 129 and blocks else "dc")
    pn = {"0": 0, "8": 8}.get(sw.get("ADMMNET_PN_SPLIT"), 84)
    return dict(td=td, inst=inst, q=r["explicit_q"] == "1", solver=solver, back=r["back_v"], padded=E_ != D, E=E_, pn=pn,
                occ=sw.get("ADMMNET_DC_OCC"))


@pytest.fixture(scope="module")
def union(model):
    out = []
    for name in E.OPTION_SETS:
        Ds = E.sizes(name, "small") + E.sizes(name, "big")
        env = E.environment(name)
        for r in read_routes(model, env, Ds):
            out.append(dict(launched(r, env), name=name, D=int(r["D"])))
    return out


def has(union, **want):
    return any(all(u[k] == v for k, v in want.items()) for u in union)


def test_hip_error_code_is_the_header_s():
    with open(os.path.join(CSRC, "..", "..", "include", "admmnet.h")) as fh:
        assert int(re.search(r"ADMMNET_E_HIP\s*=\s*(-?\d+)", fh.read()).group(1)) == E.E_HIP
    from admm_net_amd import _lib
    assert E.is_hip_error(_lib.AdmmNetError("admmnet_eigh_c64 failed (code %d): hipErrorLaunchFailure" % E.E_HIP))
    assert not E.is_hip_error(_lib.AdmmNetError("admmnet_eigh_c64 failed (code -1): eigh: bad argument (n=1)"))
    assert not E.is_hip_error(_lib.AdmmNetError("eigensolver failed on 2 matrices"))
    assert E.is_hip_error(RuntimeError("HIP error: an illegal memory access was encountered")) and not E.is_hip_error(ValueError("HIP error"))


def test_environment_spelling_is_the_one_options_uses():
    assert E.environment("lds_ql") == {"ADMMNET_TRIDIAG": "lds", "ADMMNET_EIG": "ql"}
    assert E.environment("pn0") == {"ADMMNET_PN_SPLIT": "0"} and E.environment("default") == {}


def test_every_tridiag_reg_bucket_under_both_solvers(union):
    for b in range(1, 9):
        assert has(union, td="reg", inst=b, solver="dc", back="vgemm"), b
        assert has(union, td="reg", inst=b, solver="ql", back="rotation"), b
    # both sides of every bucket edge really are two instances
    for k in range(1, 8):
        assert has(union, td="reg", inst=k, D=16 * k) and has(union, td="reg", inst=k + 1, D=16 * k + 1)
    assert has(union, name="tr_occ2", td="reg", inst=7)


def test_every_sweep_bucket_under_both_back_transforms(union):
    for b in (5, 6, 7, 8):
        assert has(union, td="sweep", inst=b, q=True, back="vgemm_big"), b
        assert has(union, td="sweep", inst=b, q=True, back="rotation"), b
    for D in (160, 192, 224):
        assert has(union, td="sweep", inst=D // 32, D=D) and has(union, td="sweep", inst=D // 32 + 1, D=D + 1)


def test_panel_routes(union):
    assert has(union, td="panel", q=False, back="wy_apply", padded=True)
    assert has(union, td="panel", q=False, back="wy_apply", padded=False, D=256)
    assert has(union, td="panel", q=True, back="vgemm_big")
    for pn in (0, 8, 84):
        assert has(union, td="panel", E=256, pn=pn, solver="dc_block"), pn
    # the pad_min boundary of spectral=0: 175 at its own size, 176 in the D = 256 pipeline
    assert has(union, name="eigen_only", D=175, td="sweep", padded=False) and has(union, name="eigen_only", D=176, td="panel", padded=True)


def test_lds_tridiagonalisation_both_images_both_solvers(union):
    for image in ("lds_image", "global_image"):
        assert has(union, td="lds", inst=image, solver="ql", back="rotation"), image
        assert any(u["td"] == "lds" and u["inst"] == image and u["solver"].startswith("dc") for u in union), image
    assert has(union, td="lds", inst="lds_image", D=138) and has(union, td="lds", inst="global_image", D=139)


def test_divide_and_conquer_variants(union):
    big = [u for u in union if u["E"] + 1 > 129]
    assert any(u["solver"] == "dc" for u in big) and any(u["solver"] == "dc_block" for u in big)
    assert has(union, name="dc_plain", solver="dc", E=256)
    for occ in ("4", "5", "6", "8"):
        assert has(union, occ=occ, solver="dc", E=128) and has(union, occ=occ, solver="dc_block", E=256), occ
    # one leaf up to n = 15, two from n = 16
    assert has(union, D=14, solver="dc") and has(union, D=15, solver="dc")


# ---- the option sets the at-occupancy test leaves out ---------------------------------------------------------------------------
def test_sets_left_out_at_occupancy_launch_the_kernels_of_the_set_kept(model):
    """tests/test_gpu_eigh_occupancy.py runs one of two option sets where csrc/route.h gives both the same kernel list at a size:
    the same eigen dimension, tridiagonalisation, explicit Q, solver and back-transform of ops.eigh, and the same pn_split,
    dc_blocks, dc_occ and tr_occ.  Every pair of its table is such a pair, the table leaves out no other, and what is kept is
    itself run."""
    import test_gpu_eigh_occupancy as O
    from test_route_host import read_switches

    def kernels(name, D):
        env = E.environment(name)
        (r,), sw = read_routes(model, env, [D]), read_switches(model, env)
        return tuple(r[k] for k in ("eig_dim", "tridiag", "explicit_q", "dc", "back_v")) + \
            tuple(sw["ADMMNET_" + k] for k in ("PN_SPLIT", "DC_BLOCKS", "DC_OCC", "TR_OCC"))

    for D in O.SIZES:
        seen, same = {}, {}
        for name in O.sets_at(D):
            k = kernels(name, D)
            if k in seen:
                same[(name, D)] = seen[k]
            seen.setdefault(k, name)
        assert same == {c: kept for c, kept in O.SAME_KERNELS.items() if c[1] == D}, D
        for (name, _), kept in same.items():
            assert D in O.sizes_of(kept), (name, D, kept)
    assert sorted(O.SIZES) == [128, 129, 175, 176, 193, 256] and O.B_EIGH == 2050 and O.B_EIGH % O.P == 0
