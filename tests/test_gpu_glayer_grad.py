"""GPU: forward and backward of ONE G layer above one 32 x 32 tile, through ``training._g_layer`` in the shapes of the four
training routes, against a float64 definition on a frozen eigenbasis.

The eigenvalue-only gradient depends on the basis the eigensolver returns inside a cluster, so two solvers' gradients cannot be
compared.  Here the basis is frozen: ``(w0, V) = ops.eigh(A)`` once (default route, float32 layer matrix on the device), and the
solver handed to every side is ``lambda A: (w0, V)``.  The definition (``contract_checks.glayer_definition``: plain autograd, none
of the project's hand-written backwards) is evaluated in float64 / complex128 on a ``.double()`` copy of the layer from the
float32 inputs, and, as the parent, in float32 / complex64 on the GPU.  tests/test_contract_checks.py holds that definition to the
project's wiring in float64.

Sizes (n, B): (33, 3), (101, 4), (129, 3), (257, 2) -- 2, 4, 5 and 9 tiles per side; the reference's gradient fixtures stop at
n = 17, one tile.  Layer: ``gLayers[0]`` of a seeded ``PhiEstADMMNet(num_layers=3)`` with perturbations of about 0.3 on rho, threshold
and value_net; phi = randn, h = |randn|, Z = 0.1 herm(randn); upstream gradients randn (not Hermitian for G).

Bound (as tests/test_gpu_training_small.py): per tensor, in the max norm,
    |kernel - f64| <= 3 |parent - f64| + 1e-6 max|f64|
for G, the border column, the diagonal, and the gradients of phi, h, Z, rho, threshold and the four value_net tensors.  Every
backward run twice gives equal bits.  The worst ratio per route is printed (recorded in DESIGN.md section 4).

Preconditions on the inputs (conditions, not tolerances), both evaluated on the float64 side alone and asserted:
  * no hidden pre-activation of value_net in the float64 evaluation lies within 1e-5 of zero -- a ReLU that flips between the
    precisions would be an artefact of the inputs;
  * the gradient of rho is not a cancelled sum.  It is ONE sum over all B n^2 entries, g_rho = c sum_ij Re(conj(gZ_ij) Z_ij) with
    gZ the gradient of Z, and any float32 evaluation of it errs at the scale u sum|terms| (u = 2^-24; the terms, entries of gZ, are
    n-term contractions with errors of several u each).  The bound's floor 1e-6 |g_rho| reaches that scale only while
    sum|terms| <= |sum terms| / (1e6 u) = 16.8 |sum terms|; beyond it the comparison is decided by whether the float32 parent's own
    draw of that error happens to be small (seen on the MI355X at a seed with sum|terms| = 53 |sum terms|: parent 8e-9,
    tensor route 1.3e-7 of a gradient of 0.076, every other tensor within its bound).
The seeds are the first per size at which both hold (with LAPACK's eigenvalues, a margin of 3e-4 for the first): nothing is left
out of any comparison.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import admm_net_amd as A
from admm_net_amd import ops, training

import contract_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = {33: (3, 4, 8), 101: (4, 10, 10), 129: (3, 8, 16), 257: (2, 16, 16)}       # n -> (B, M, N)
SEEDS = {33: 2, 101: 3, 129: 20, 257: 37}                # see "Preconditions" above
MAX_CANCELLATION = 1.0 / (1e6 * C.U)                     # 16.8
ROUTES = {"tensor": dict(), "fused": dict(lk=training.LayerKernels),
          "full": dict(lk=training.LayerKernels, sk=training.SmallKernels),
          "native": dict(lk=training.LayerKernels, sk=training.SmallKernels, rinv=True)}
NAMES = ("G", "column", "diagonal")


def host_case(n, seed):
    """(layer, phi, h, Z, upstream gradients), float32 on the CPU."""
    B, M, N = SIZES[n]
    torch.manual_seed(seed)
    layer = C.perturbed_glayer(A.PhiEstADMMNet(M=M, N=N, num_layers=3), seed=seed + 1000)
    return (layer, *C.glayer_inputs(n, B, seed=seed + 2000))


def layer_matrix(layer, phi, h, Z, corner):
    with torch.no_grad():
        return C.herm(training._block_matrix(phi, h, corner) - Z / (F.softplus(layer.rho) + C.EPS))


def min_preactivation(layer, w0):
    """min |W1 |w| + b1| over every eigenvalue and hidden unit, float64."""
    return layer.value_net[0](w0.abs().unsqueeze(-1)).abs().min().item()


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def _evaluate(layer, phi, h, Z, ups, w0, V, corner):
    """The definition and its gradients, with and without the border terms in the loss."""
    a = _leaves(phi, h, Z)
    out = C.glayer_definition(layer, *a, w0, V, corner)
    return {"out": out[:3], "pre": out[3], True: C.glayer_grads(layer, a, out[:3], ups, True),
            False: C.glayer_grads(layer, a, out[:3], ups, False)}


_CACHE = {}


def reference(n):
    """The frozen basis, the float64 evaluation and the float32 parent for size n, computed once and left unchanged."""
    if n in _CACHE:
        return _CACHE[n]
    layer, phi, h, Z, ups = host_case(n, SEEDS[n])
    dev = lambda ts: tuple(t.to(DEV) for t in ts)
    layer32 = copy.deepcopy(layer).to(DEV)
    phi32, h32, Z32 = dev((phi, h, Z))
    ups32 = dev(ups)
    corner = (1.0 / (F.softplus(layer32.lambda_param) ** 2 + C.EPS)).item()
    w0, V = ops.eigh(layer_matrix(layer32, phi32, h32, Z32, corner))
    w0, V = w0.detach(), V.detach()
    layer64 = copy.deepcopy(layer).double()
    want = _evaluate(layer64, C.f64(phi), C.f64(h), C.f64(Z), tuple(C.f64(u) for u in ups), C.f64(w0), C.f64(V), corner)
    parent = _evaluate(layer32, phi32, h32, Z32, ups32, w0, V, corner)
    _CACHE[n] = dict(layer=layer32, inputs=(phi32, h32, Z32), ups=ups32, w0=w0, V=V, corner=corner, want=want, parent=parent)
    return _CACHE[n]


def rho_cancellation(r, border):
    """sum|terms| / |sum terms| of the gradient of rho, from the float64 evaluation."""
    t = (r["want"][border]["Z"].conj() * C.f64(r["inputs"][2])).real
    return (t.abs().sum() / t.sum().abs()).item()


def preconditions(r, border):
    return r["want"]["pre"].abs().min().item() > 1e-5 and rho_cancellation(r, border) <= MAX_CANCELLATION


@pytest.mark.parametrize("n", list(SIZES))
def test_preconditions_on_the_inputs(n):
    r = reference(n)
    lo = r["want"]["pre"].abs().min().item()
    k = [rho_cancellation(r, border) for border in (False, True)]
    print(f"n={n}: smallest |hidden pre-activation of value_net| {lo:.3e}; sum|terms| / |sum terms| of the gradient of rho "
          f"{k[0]:.1f} (G alone), {k[1]:.1f} (with the border terms)")
    assert lo > 1e-5
    assert max(k) <= MAX_CANCELLATION


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", list(SIZES))
def test_glayer_on_a_frozen_basis(n, route):
    r = reference(n)
    layer, w0, V, corner = r["layer"], r["w0"], r["V"], r["corner"]
    solver = lambda Amat: (w0, V)
    kw = dict(ROUTES[route])
    border = "lk" in kw
    assert preconditions(r, border), "the inputs miss a precondition (test_preconditions_on_the_inputs prints the figures)"
    if kw.pop("rinv", False):
        kw["rinv"] = 1.0 / (F.softplus(layer.rho) + C.EPS)
    if "sk" in kw:
        kw["corner"] = corner
    a = _leaves(*r["inputs"])
    out = training._g_layer(layer, *a, solver, training.Assembler, **kw)
    g1 = C.glayer_grads(layer, a, out, r["ups"], border)
    g2 = C.glayer_grads(layer, a, out, r["ups"], border)
    assert g1["lambda_param"] is None
    names = ("phi", "h", "Z") + C.GLAYER_PARAMS
    assert all(C.same_bits(g1[k], g2[k]) for k in names), "two backward runs must give the same bits"

    worst = 0.0

    def hold(got, parent, want, name):
        nonlocal worst
        want = C.f64(want)
        assert got.shape == want.shape, name
        err, perr = (C.f64(got) - want).abs().max().item(), (C.f64(parent) - want).abs().max().item()
        bound = 3 * perr + 1e-6 * want.abs().max().item()
        print(f"  n={n} {route} {name}: kernel {err:.3e}, parent {perr:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        worst = max(worst, err / bound)
        return err <= bound, f"{name}: kernel {err:.3e} from float64, parent {perr:.3e}, bound {bound:.3e}"

    results = []
    outs = out if border else (out,)
    for x, p, w, name in zip(outs, r["parent"]["out"], r["want"]["out"], NAMES):
        results.append(hold(x, p, w, name))
    for k in names:
        results.append(hold(g1[k], r["parent"][border][k], r["want"][border][k], "gradient of " + k))
    print(f"n={n} {route}: worst error / bound {worst:.3f}")
    bad = [msg for ok, msg in results if not ok]
    assert not bad, bad
