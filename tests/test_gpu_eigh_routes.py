"""GPU: every eigensolver route an ``Options`` can select, per size class, against LAPACK in float64 (tests/eigh_cases.py holds
the option sets, sizes, matrices, metrics and bounds; tests/test_eigh_cases_host.py shows on the CPU that the table reaches every
template instance of the launchers and that float32 LAPACK meets a quarter of each bound).  All in this process through
``ops.eigh(A, options=...)``: the eigenvectors themselves are checked (residual, orthogonality), not a function of them.

Three things are asked of a route: the bounds of the default route on the four matrix kinds at every size; the same bits for
a matrix wherever it stands in the batch (across the 64-matrix groups of the dT / eT layout, with a ragged last group); the
same across the 8192-matrix chunk loop of admmnet_eigh_c64_o.

Device hygiene (eigh_cases.DeviceGuard): once a case meets a HIP error (AdmmNetError with ADMMNET_E_HIP, or a HIP RuntimeError
of torch) the remaining cases of the file fail at once without touching the device.

Measured on MI355X, worst over the sizes and the four kinds of a case, res / orth / ev, next to float32 LAPACK on the same
matrices (a record: the bounds stay those of eigh_cases.BOUNDS, 3e-5 / 3e-5 / 1e-5 and 5e-5 / 5e-5 / 1e-5):
  default    small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  default    big    1.8e-05 / 2.8e-06 / 2.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  eigen_only small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  eigen_only big    1.8e-05 / 2.8e-06 / 2.2e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  ql         small  8.2e-06 / 1.9e-06 / 3.2e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  ql         big    9.5e-06 / 2.8e-06 / 3.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  lds        small  6.0e-06 / 1.5e-06 / 3.0e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  lds        big    1.1e-05 / 1.8e-06 / 1.7e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  lds_ql     small  5.5e-06 / 2.0e-06 / 3.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  lds_ql     big    9.7e-06 / 3.2e-06 / 3.1e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  sweep      small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  sweep      big    1.0e-05 / 2.0e-06 / 1.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  explicit_q small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  explicit_q big    1.0e-05 / 2.2e-06 / 1.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  pn0        small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  pn0        big    1.8e-05 / 3.2e-06 / 2.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  pn8        small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  pn8        big    1.8e-05 / 2.8e-06 / 2.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  dc_plain   small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  dc_plain   big    1.8e-05 / 2.8e-06 / 2.4e-06   (float32 LAPACK 4.4e-07 / 7.6e-08 / 2.6e-07)
  tr_occ2    small  8.8e-06 / 1.4e-06 / 2.5e-06   (float32 LAPACK 2.7e-07 / 7.5e-08 / 2.8e-07)
  dc_occ4    small  8.8e-06 / 1.1e-06 / 1.0e-06   (float32 LAPACK 1.9e-07 / 6.8e-08 / 7.8e-08)
  dc_occ4    big    7.8e-06 / 2.1e-06 / 5.7e-07   (float32 LAPACK 3.0e-07 / 6.4e-08 / 6.2e-08)
  dc_occ5    small  8.8e-06 / 1.1e-06 / 1.0e-06   (float32 LAPACK 1.9e-07 / 6.8e-08 / 7.8e-08)
  dc_occ5    big    7.8e-06 / 2.1e-06 / 5.7e-07   (float32 LAPACK 3.0e-07 / 6.4e-08 / 6.2e-08)
  dc_occ6    small  8.8e-06 / 1.1e-06 / 1.0e-06   (float32 LAPACK 1.9e-07 / 6.8e-08 / 7.8e-08)
  dc_occ6    big    7.8e-06 / 2.1e-06 / 5.7e-07   (float32 LAPACK 3.0e-07 / 6.4e-08 / 6.2e-08)
  dc_occ8    small  8.8e-06 / 1.1e-06 / 1.0e-06   (float32 LAPACK 1.9e-07 / 6.8e-08 / 7.8e-08)
  dc_occ8    big    7.8e-06 / 2.1e-06 / 5.7e-07   (float32 LAPACK 3.0e-07 / 6.4e-08 / 6.2e-08)

Found and fixed with these tests: the block-reflector back-transform (wy_apply.hip; the routes default, eigen_only, pn0, pn8,
dc_plain and dc_occ* above D = 128) formed Z = Y^H X, a reduction over 256 rows, with three real matrix-core products per
complex one (T3 = (Yr + Yi)(Xi - Xr), Zi = T3 + T1 - T2), whose parts cancel.  On the kind `layer` the eigenvector of the
outlying eigenvalue (40 and 44 times max|A| at D = 193 and 256, where res divides by max|A|) came back 1e-6 off in the
directions of the bulk: res 5.16e-5 at D = 193 (padded to 256), over the bound 5e-5, and 4.1e-5 at D = 256, where
Options(back="q") on the same reflectors and a bit-identical D&C gave 1.0e-5.  With four products in that reduction the same
two cases give 1.43e-5 and 3.5e-6; the table above is of that kernel.  The cost, measured on 2048 matrices of n = 257: the
back-transform (wy_apply_kernel + wy_lastcol_kernel) 2.68 -> 2.90 ms, the whole ops.eigh call 15.05 -> 15.15 ms.  Which of
the kernel's two products mattered was measured on the device by building it three ways (worst res of the class `big` /
of D = 256 alone, over the four kinds): four products in Z = Y^H X alone 1.8e-5 / 7.8e-6 -- the kernel as it is; in the
update X -= Y Zt alone 5.4e-5 / 4.2e-5, as with three in both; in both 1.8e-5 / 8.1e-6.  So the update keeps its three
products.  (A float32 emulation of the two forms on the CPU with BLAS products gave res 3.5e-6 for either form: BLAS does not
accumulate a 256-term sum in one chain as the matrix-core loop does, so the emulation does not model the device kernel and
neither supports nor contradicts the measurement.)"""
import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import ops

import eigh_cases as E

pytestmark = pytest.mark.gpu
GUARD = E.DeviceGuard()   # once a case meets a HIP error the remaining cases do not touch the device


def eigh(mats, opts):
    def run():
        w, V = ops.eigh(torch.from_numpy(mats).cuda(), options=opts)
        return w.cpu().numpy(), V.cpu().numpy()
    return GUARD.run(run)


def options(name):
    return A.Options(**E.OPTION_SETS[name])


def resolved_value(key, value):
    """What Options.resolved() reads for an override: a word switch 1 where its word is set, tr_occ 1 for the three-workgroup
    build (so 0 for tr_occ=2), a number itself."""
    return int(value != 2) if key == "tr_occ" else 1 if isinstance(value, str) else value


def assert_switch_took(name, opts):
    got, base = opts.resolved(), A.options.describe(0)
    for key, value in E.OPTION_SETS[name].items():
        assert got[key] == resolved_value(key, value), (name, key, got[key])
    assert {k: v for k, v in got.items() if k not in E.OPTION_SETS[name]} == {k: v for k, v in base.items() if k not in E.OPTION_SETS[name]}


def check_distinct(what, mats, kinds, w, V):
    worst = [0.0, 0.0, 0.0]
    for i, kind in enumerate(kinds):
        m = E.metrics(mats[i], w[i], V[i])
        worst = [max(a, b) for a, b in zip(worst, m[:3])]
        assert E.within(kind, m), (what, kind, "res %.2e orth %.2e ev %.2e finite %s" % m, "bounds", E.BOUNDS[kind])
    return worst


@pytest.mark.parametrize("name,size_class", E.cases(), ids=["%s-%s" % c for c in E.cases()])
def test_route_meets_the_eigh_bounds(name, size_class):
    """One ops.eigh call per size with the four kinds (B = 4); every (size, kind) that misses is reported, not the first."""
    opts = options(name)
    assert_switch_took(name, opts)
    worst, ref, failures = [0.0] * 3, [0.0] * 3, []
    for D in E.sizes(name, size_class):
        n = D + 1
        mats = E.matrices(n)
        w, V = eigh(mats, opts)
        for i, kind in enumerate(E.KINDS):
            m = E.metrics(mats[i], w[i], V[i])
            r = E.metrics(mats[i], *E.lapack32(mats[i]))
            worst = [max(a, b) for a, b in zip(worst, m[:3])]
            ref = [max(a, b) for a, b in zip(ref, r[:3])]
            if not E.within(kind, m):
                failures.append((D, kind, "res %.2e orth %.2e ev %.2e finite %s" % m))
    print("FIGURES %-10s %-5s res %.1e orth %.1e ev %.1e | float32 LAPACK res %.1e orth %.1e ev %.1e" %
          ((name, size_class) + tuple(worst) + tuple(ref)))
    assert not failures, (name, size_class, failures)


POSITION_SETS = ["default", "eigen_only", "ql", "lds", "sweep"]


def assert_copies_are_bit_identical(what, w, V, distinct):
    for j in range(len(w)):
        src = j % distinct
        assert np.array_equal(w[j], w[src]), (what, "w of copy %d differs from position %d" % (j, src), float(np.abs(w[j] - w[src]).max()))
        assert np.array_equal(V[j], V[src]), (what, "V of copy %d differs from position %d" % (j, src), float(np.abs(V[j] - V[src]).max()))


@pytest.mark.parametrize("name", POSITION_SETS)
def test_a_matrix_has_the_same_bits_at_any_batch_position(name):
    """B = 130 from 5 distinct matrices repeated cyclically: two boundaries of the 64-matrix groups and a ragged last group;
    at D = 16 also B = 1, 63, 64, 65.  A result that depends on the neighbours is a bug, not a tolerance question."""
    opts = options(name)
    for D, batches in ((16, (130, 1, 63, 64, 65)), (128, (130,)), (129, (130,))):
        n = D + 1
        pick = [0, 2, 3, 4, 5]                              # gue, layer, eightfold and two more gue
        five = E.matrices(n, more_gue=2)[pick]
        kinds = [E.kind_of(i) for i in pick]
        first = None
        for B in batches:
            mats = five[np.arange(B) % 5]
            w, V = eigh(mats, opts)
            what = (name, D, B)
            assert_copies_are_bit_identical(what, w, V, 5)
            k = min(B, 5)
            check_distinct(what, five[:k], kinds[:k], w[:k], V[:k])
            if first is None:
                first = (w[:5], V[:5])
            else:   # (and the batch size is a neighbourhood too)
                assert np.array_equal(w[:k], first[0][:k]) and np.array_equal(V[:k], first[1][:k]), what


@pytest.mark.parametrize("name", ["default", "ql"])
@pytest.mark.parametrize("n", [3, 17])
def test_eigh_across_the_chunk_boundary(name, n):
    """B = 8193: the chunk is 8192 matrices, the second one holds a single matrix."""
    opts = options(name)
    seven = E.matrices(n, more_gue=3)
    kinds = [E.kind_of(i) for i in range(7)]
    B = 8193
    w, V = eigh(seven[np.arange(B) % 7], opts)
    assert_copies_are_bit_identical((name, n, B), w, V, 7)
    check_distinct((name, n, B), seven, kinds, w[:7], V[:7])
