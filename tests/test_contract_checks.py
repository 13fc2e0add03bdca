"""CPU: the checks of tests/contract_checks.py accept a right float32 implementation of the two eigenbasis contractions and
reject wrong ones, and its float64 G-layer definition agrees with the project's own autograd wiring.

* the right stand-ins (the same formulas in complex64 / float32 torch) pass at every n of ``NS``, for both V kinds and for the
  one-hot batches: the derived bounds are feasible for plain float32 arithmetic;
* each of the sixteen wrong stand-ins is rejected at EVERY n of ``NS`` at which it differs from the right one, for both V kinds
  (size by size, not "somewhere"), and passes where it is the right one;
* known limit, stated and not skipped: at n = 256 and 257 the worst-case vhsv bound admits "V rounded to bf16"
  (``contract_checks.ADMITTED``); that stand-in must be rejected at every n <= 129;
* ``glayer_definition`` against ``training._g_layer`` with a frozen solver and ``TorchAssembler`` in float64 at n = 17, in the shapes of
  the four training routes (plain; ``TorchLayerKernels``; + ``TorchSmallKernels``; + the ``rinv`` form).
"""
import pytest
import torch
import torch.nn.functional as F

import admm_net_amd as A
from admm_net_amd import training

import contract_checks as C


@pytest.fixture(scope="module")
def cases():
    """{(n, kind): (V, d, S)} and {n: one-hot batch}, made once."""
    return ({(n, kind): C.inputs(n, C.B, seed=100 + n, kind=kind) for n in C.NS for kind in C.KINDS},
            {n: C.one_hot(n, seed=200 + n) for n in C.NS})


@pytest.mark.parametrize("n", C.NS)
def test_right_stand_ins_pass(cases, n):
    batches = [(f"{kind}", *cases[0][(n, kind)]) for kind in C.KINDS] + [("one-hot", *cases[1][n][:3])]
    for what, V, d, S in batches:
        res = C.check_vdvh(V, d, C.right_vdvh(V, d))
        rq = C.check_vhsv(V, S, C.right_vhsv(V, S))
        print(f"n={n} {what}: vdvh error / bound {res['ratio']:.4f}, vhsv error / bound {rq:.4f}")
        assert C.vdvh_ok(res), (what, res)
        assert rq <= 1.0, (what, rq)


@pytest.mark.parametrize("name", list(C.WRONG_VDVH))
def test_wrong_vdvh_is_rejected_at_every_size(cases, name):
    fn, identical = C.WRONG_VDVH[name]
    for n in C.NS:
        for kind in C.KINDS:
            V, d, _ = cases[0][(n, kind)]
            res = C.check_vdvh(V, d, fn(V, d))
            print(f"{name}: n={n} {kind}: error / bound {res['ratio']:.3g}, hermitian {res['hermitian']}")
            if identical(n, kind):
                assert C.vdvh_ok(res), (n, kind, res)
            else:
                assert res["ratio"] > 1.0, f"{name} passes the value check at n={n}, {kind}: {res}"


@pytest.mark.parametrize("name", list(C.WRONG_VHSV))
def test_wrong_vhsv_is_rejected_at_every_size(cases, name):
    fn, identical = C.WRONG_VHSV[name]
    admitted = C.ADMITTED.get(("vhsv", name), ())
    for n in C.NS:
        for kind in C.KINDS:
            V, _, S = cases[0][(n, kind)]
            ratio = C.check_vhsv(V, S, fn(V, S))
            print(f"{name}: n={n} {kind}: error / bound {ratio:.3g}" + (" (known limit: not required to fail)" if n in admitted else ""))
            if identical(n, kind):
                assert ratio <= 1.0, (n, kind, ratio)
            elif n not in admitted:
                assert ratio > 1.0, f"{name} passes at n={n}, {kind}: error / bound {ratio:.3g}"


def test_the_known_limit_is_what_it_says():
    """The one admitted pair is vhsv's bf16 stand-in at n = 256, 257 and nothing else; it must fail at every n <= 129."""
    assert C.ADMITTED == {("vhsv", "V rounded to bf16"): (256, 257)}
    assert [n for n in C.NS if n not in (256, 257)] == [n for n in C.NS if n <= 129]


def test_checks_flag_non_finite_and_structure():
    V, d, S = C.inputs(5, 2, seed=1, kind="general")
    G = C.right_vdvh(V, d)
    bad = G.clone()
    bad[1, 3, 2] = complex(float("nan"), 0.0)
    assert C.check_vdvh(V, d, bad)["ratio"] == float("inf")
    up = G.clone()
    up[0, 1, 3] = up[0, 1, 3] + complex(0.0, 1e-7) * abs(up[0, 1, 3])      # an upper entry off by one rounding
    assert not C.check_vdvh(V, d, up)["hermitian"]
    dg = G.clone()
    dg[0, 2, 2] = complex(dg[0, 2, 2].real.item(), 1e-30)
    assert not C.check_vdvh(V, d, dg)["real_diagonal"]
    q = C.right_vhsv(V, S)
    q[1, 4] = float("inf")
    assert C.check_vhsv(V, S, q) == float("inf")


# ------------------------------------------------------------------------------------------------ the G-layer definition
def _routes():
    T = training
    return {"tensor": dict(), "fused": dict(lk=T.TorchLayerKernels), "full": dict(lk=T.TorchLayerKernels, sk=T.TorchSmallKernels),
            "native": dict(lk=T.TorchLayerKernels, sk=T.TorchSmallKernels, rinv=True)}


@pytest.mark.parametrize("route", ["tensor", "fused", "full", "native"])
def test_glayer_definition_matches_the_wiring(route):
    """float64, n = 17, B = 3.  G and the gradients of threshold and value_net to 1e-12; the gradients of phi, h, Z and rho to
    1e-7 of their largest entry: ``_EighValuesOnly.backward`` casts gw to float32 on the project's side.  (rho's gradient is ONE
    sum over all entries, so that cast shows relative to the sum's terms: the seeds are such that the sum is not a cancelled one,
    |g_rho| > 0.03 against 5e-3 at other seeds.)"""
    n, Bn = 17, 3
    torch.manual_seed(0)
    layer = C.perturbed_glayer(A.PhiEstADMMNet(M=4, N=4, num_layers=3), seed=41).double()
    phi, h, Z, ups = C.glayer_inputs(n, Bn, seed=42)
    phi, h, Z = C.f64(phi), C.f64(h), C.f64(Z)
    ups = tuple(C.f64(u) for u in ups)
    corner = (1.0 / (F.softplus(layer.lambda_param) ** 2 + C.EPS)).item()
    with torch.no_grad():
        w0, V = torch.linalg.eigh(C.herm(training._block_matrix(phi, h, corner) - Z / (F.softplus(layer.rho) + C.EPS)))
    solver = lambda Amat: (w0, V)
    kw = dict(_routes()[route])
    border = "lk" in kw

    a = [t.clone().requires_grad_(True) for t in (phi, h, Z)]
    want = C.glayer_definition(layer, *a, w0, V, corner)
    gw = C.glayer_grads(layer, a, want[:3], ups, border)

    b = [t.clone().requires_grad_(True) for t in (phi, h, Z)]
    if kw.pop("rinv", False):
        kw["rinv"] = 1.0 / (F.softplus(layer.rho) + C.EPS)
    if "sk" in kw:
        kw["corner"] = corner
    got = training._g_layer(layer, *b, solver, training.TorchAssembler, **kw)
    gg = C.glayer_grads(layer, b, got, ups, border)

    outs = got if border else (got,)
    for x, y, name in zip(outs, want, ("G", "column", "diagonal")):
        assert (x - y).abs().max().item() <= 1e-12, name
    for name in C.GLAYER_PARAMS[1:]:
        assert (gg[name] - gw[name]).abs().max().item() <= 1e-12, name
    for name in ("phi", "h", "Z", "rho"):
        err, big = (gg[name] - gw[name]).abs().max().item(), gw[name].abs().max().item()
        print(f"{route} {name}: {err:.2e} of {big:.2e}")
        assert err <= 1e-7 * big, name
    assert gg["lambda_param"] is None and gw["lambda_param"] is None
