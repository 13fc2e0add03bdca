"""GPU: ``ops.vdvh`` / ``ops.vhsv`` (csrc/vdvh.hip) under the checks of tests/contract_checks.py -- float64 definitions, bounds
derived from the accumulation depth ((2 n + 4) u and (2 n + 64) u of the sum of the magnitudes of the terms), the structure of
vdvh's output -- at every tile edge, for exactly unitary, general and eigensolver-made V, on one-hot d, and the behaviour the
kernels' comments promise: equal bits on a second run, independence of the neighbours in the batch, only the lower triangle and
the real diagonal of S read, any stream, any input layout, a large grid, and the wrappers' refusals.

tests/test_contract_checks.py shows on the CPU that these checks reject sixteen wrong implementations size by size.
Each case prints its worst error / bound, and, unasserted, how far the framework's own complex64 matmul formulation on the GPU is
from float64 on the same inputs next to the kernel's distance (DESIGN.md section 4 records both).
"""
import pytest
import torch

from admm_net_amd import _lib, ops

import contract_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = C.KINDS + ("solver",)
CASES = [(n, kind) for n in C.NS for kind in KINDS if not (kind == "solver" and n < 2)]


def _inputs(n, B, seed, kind):
    """``contract_checks.inputs`` on the device; kind "solver": V is what ``ops.eigh`` returns for herm(randn), float32, columns
    unsorted and only nearly unitary -- what training hands to the kernels."""
    if kind != "solver":
        return tuple(t.to(DEV) for t in C.inputs(n, B, seed, kind))
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, n, n, dtype=torch.complex64, generator=g)
    _, V = ops.eigh(C.herm(X).to(DEV))
    d, S = C.d_and_s(n, B, g)
    return V, d.to(DEV), S.to(DEV)


def _check(V, d, S, what):
    """Both kernels under their bounds; returns the two worst error / bound figures."""
    res = C.check_vdvh(V, d, ops.vdvh(V, d))
    rq = C.check_vhsv(V, S, ops.vhsv(V, S))
    print(f"{what}: vdvh error / bound {res['ratio']:.4f}, vhsv error / bound {rq:.4f}")
    assert C.vdvh_ok(res), (what, res)
    assert rq <= 1.0, (what, rq)
    return res["ratio"], rq


@pytest.mark.parametrize("n,kind", CASES, ids=[f"n{n}-{kind}" for n, kind in CASES])
def test_kernels_within_derived_bounds(n, kind):
    V, d, S = _inputs(n, C.B, seed=100 + n, kind=kind)
    _check(V, d, S, f"n={n} {kind}")
    wg, wq = C.vdvh_f64(V, d), C.vhsv_f64(V, S)
    print(f"n={n} {kind}: max-norm distance from float64, kernel / torch complex64 matmul: "
          f"vdvh {C.max_distance(ops.vdvh(V, d), wg):.3e} / {C.max_distance(C.torch_vdvh(V, d), wg):.3e}, "
          f"vhsv {C.max_distance(ops.vhsv(V, S), wq):.3e} / {C.max_distance(C.torch_vhsv(V, S), wq):.3e}")


@pytest.mark.parametrize("n", [33, 64, 65, 101, 256, 257])
def test_one_hot_d(n):
    """d = 1.5 e_c for the columns next to the k-step, lane-half and tile edges: every output entry is ONE term, so a wrong column
    index cannot hide among n terms."""
    V, d, S, cols = C.one_hot(n, seed=200 + n)
    V, d, S = V.to(DEV), d.to(DEV), S.to(DEV)
    _check(V, d, S, f"one-hot n={n} columns {cols}")
    got = C.f64(ops.vdvh(V, d))
    for k, c in enumerate(cols):
        v = C.f64(V[k, :, c])
        want = 1.5 * v.unsqueeze(1) * v.conj().unsqueeze(0)
        # the single term's own depth: x d, the product, the sum of the part's two real products (adding zeros is exact) =
        # 3 roundings, + 1 for the second order, against the (2 n + 4) of the general bound
        bound = 4 * C.U * 1.5 * C.abs1(v).unsqueeze(1) * C.abs1(v).unsqueeze(0)
        err = torch.maximum((got[k].real - want.real).abs(), (got[k].imag - want.imag).abs())
        print(f"one-hot n={n} column {c}: single-term error / (4 u |term|) {(err / (bound + 1e-300)).max().item():.3f}")
        assert (err <= bound).all(), (n, c)


@pytest.mark.parametrize("n,kind", [(33, "general"), (101, "solver"), (257, "general")])
def test_equal_bits_on_a_second_run(n, kind):
    V, d, S = _inputs(n, C.B, seed=300 + n, kind=kind)
    assert C.same_bits(ops.vdvh(V, d), ops.vdvh(V, d))
    assert C.same_bits(ops.vhsv(V, S), ops.vhsv(V, S))


@pytest.mark.parametrize("n", [5, 65, 129])
def test_a_matrix_does_not_depend_on_its_neighbours(n):
    """B = 5: matrix 2 alone has the bits it has in the batch; NaN in all of matrix 3's V leaves matrices 0, 1, 2 and 4 as they were."""
    V, d, S = _inputs(n, 5, seed=400 + n, kind="general")
    G, q = ops.vdvh(V, d), ops.vhsv(V, S)
    assert C.same_bits(ops.vdvh(V[2:3], d[2:3])[0], G[2])
    assert C.same_bits(ops.vhsv(V[2:3], S[2:3])[0], q[2])
    Vn = V.clone()
    Vn[3] = complex(float("nan"), float("nan"))
    Gn, qn = ops.vdvh(Vn, d), ops.vhsv(Vn, S)
    keep = [0, 1, 2, 4]
    assert C.same_bits(Gn[keep], G[keep]) and C.same_bits(qn[keep], q[keep])
    assert torch.isnan(Gn[3].real).all() and torch.isnan(qn[3]).all()


@pytest.mark.parametrize("n", [1, 2, 33, 64, 129, 257])
def test_vhsv_reads_the_lower_triangle_and_the_real_diagonal_only(n):
    V, _, S = _inputs(n, C.B, seed=500 + n, kind="general")
    nan = float("nan")
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), 1)
    Sn = torch.where(upper, torch.full_like(S, complex(nan, nan)), S)
    dg = torch.diagonal(Sn, dim1=1, dim2=2)
    dg.copy_(torch.complex(dg.real.clone(), torch.full_like(dg.real, nan)))
    assert torch.isnan(torch.view_as_real(Sn)).sum().item() == C.B * (n * (n - 1) + n)
    assert C.same_bits(ops.vhsv(V, Sn), ops.vhsv(V, S))


def test_on_a_side_stream():
    V, d, S = _inputs(101, C.B, seed=600, kind="general")
    G, q = ops.vdvh(V, d), ops.vhsv(V, S)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        G2, q2 = ops.vdvh(V, d), ops.vhsv(V, S)
    st.synchronize()
    assert C.same_bits(G2, G) and C.same_bits(q2, q)


@pytest.mark.parametrize("n", [7, 65])
def test_input_layout(n):
    """Views that are not plain contiguous memory give the bits of the contiguous call: a double transpose-conjugate, a slice of
    a larger buffer, column-major strides, and a lazily conjugated tensor (the conj bit set over the conjugate's memory)."""
    V, d, S = _inputs(n, C.B, seed=700 + n, kind="general")
    G, q = ops.vdvh(V, d), ops.vhsv(V, S)

    def sliced(X):
        buf = torch.full((X.shape[0], n + 3, n + 2), complex(float("nan"), float("nan")), dtype=X.dtype, device=DEV)
        buf[:, 1:n + 1, 2:n + 2] = X
        v = buf[:, 1:n + 1, 2:n + 2]
        assert not v.is_contiguous()
        return v

    def lazy_conj(X):
        v = X.conj().resolve_conj().conj()
        assert v.is_conj() and torch.equal(v, X)
        return v

    forms = {"transpose-conj twice": lambda X: X.transpose(1, 2).conj().transpose(1, 2).conj(), "slice": sliced,
             "column-major": lambda X: X.transpose(1, 2).contiguous().transpose(1, 2), "lazy conjugate": lazy_conj}
    for name, f in forms.items():
        assert C.same_bits(ops.vdvh(f(V), d), G), name
        assert C.same_bits(ops.vhsv(f(V), f(S)), q), name
    assert C.same_bits(ops.vdvh(V, d.t().contiguous().t()), G)


def test_large_grid():
    """B = 65 536 workgroups at n = 5 (tests/test_gpu_training_fused.py::test_large_batch_grid), and one workgroup at n = 257."""
    _check(*_inputs(5, 65536, seed=800, kind="general"), "n=5 B=65536")
    _check(*_inputs(257, 1, seed=801, kind="general"), "n=257 B=1")


def test_refusals():
    """The argument checks answer before any launch: the library's own ("bad argument") for n - 1 > 256, the wrappers' for a
    wrong shape or a CPU tensor."""
    n = 258
    V = torch.zeros(1, n, n, dtype=torch.complex64, device=DEV)
    with pytest.raises(_lib.AdmmNetError, match="bad argument"):
        ops.vdvh(V, torch.zeros(1, n, device=DEV))
    with pytest.raises(_lib.AdmmNetError, match="bad argument"):
        ops.vhsv(V, V)
    V, d, S = _inputs(9, 2, seed=900, kind="general")
    with pytest.raises(ValueError):
        ops.vdvh(V, d[:, :8])
    with pytest.raises(ValueError):
        ops.vhsv(V, S[:, :8, :8])
    with pytest.raises(ValueError):
        ops.vhsv(V, S[:1])
    with pytest.raises(_lib.AdmmNetError, match="device tensor"):
        ops.vdvh(V.cpu(), d)
    with pytest.raises(_lib.AdmmNetError, match="device tensor"):
        ops.vhsv(V.cpu(), S)
    torch.cuda.synchronize()
    _check(V, d, S, "after the refusals")
