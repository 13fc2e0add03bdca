"""GPU: per-model option sets (admm_net_amd.Options, model.options) choose the kernel route of ONE model in a process that runs
others.  The yardstick is the environment route of the same commit: what ADMMNET_* variables select in a child process, an
``Options`` must select in this one -- to the reference's tolerance for every variant of tests/test_gpu_variants.py, and bit for
bit (outputs and status words) for five of them.  The four K = 3 golden fixtures are those of test_gpu_variants.py: D = 128, 100,
256 and 192, one geometry per eigen-pipeline and padding case."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, ops
from admm_net_amd.sharded import ShardedForward
from test_gpu_variants import VARIANTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("phiest_8x16_K3_perturbed", "admmnet_10x10_K3_default", "phiest_16x16_K3_perturbed", "phiest_12x16_K3_perturbed")
_loaded = {}


def fixture(name):
    """(state_dict, meta, (y, b, sigma) on the device, reference phi), loaded once and left unchanged."""
    if name not in _loaded:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        meta = [int(v) for v in z["meta"]]
        sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
        dev = torch.device("cuda:0")
        _loaded[name] = (sd, meta, tuple(torch.from_numpy(z[k]).to(dev) for k in ("y", "b", "sigma")), z["phi"])
    return _loaded[name]


def build(name, options=None, chunk=0):
    sd, (Nb, Nd, K, B, L, head, _), _, _ = fixture(name)
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, L=L, num_layers=K)
    m.load_state_dict(sd)
    m.eval()
    m.chunk = chunk
    m.options = options
    return m


def run(m, name):
    """-> (phi as numpy, status words)."""
    r = m(*fixture(name)[2])
    phi = (r[3] if isinstance(r, tuple) else r).cpu().numpy()
    return phi, list(m.last_status)


def as_options(env):
    return A.Options(**{k[len("ADMMNET_"):].lower(): v for k, v in env.items() if k != "ADMMNET_TEST_CHUNK"})


# ---- every variant in one process ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_as_options_matches_reference_fixtures(variant):
    """test_gpu_variants.test_variant_matches_reference_fixtures without the child process: the variant's variables as
    ``Options``, ADMMNET_TEST_CHUNK as ``model.chunk``, the same four fixtures and the same bound."""
    env = VARIANTS[variant]
    opts = as_options(env)
    for name in FIXTURES:
        m = build(name, opts, int(env.get("ADMMNET_TEST_CHUNK", "0")))
        phi, st = run(m, name)
        ref = fixture(name)[3]
        e = float(np.abs(phi - ref).max() / np.abs(ref).max())
        print(f"{variant} {name}: rel err {e:.3e}, status {st}")
        assert e < 1e-4, (variant, name, e)
        if opts.resolved()["spectral"] == 0:
            assert st[2] == 0, (variant, name, st)   # (the route was really switched: no matrix evaluated as a matrix function)


# ---- the environment's routes, bit for bit ---------------------------------------------------------------------------------------------
BITWISE = {"default": {}, "eigen_only": VARIANTS["eigen_only"], "spectral_all_rejected": VARIANTS["spectral_all_rejected"],
           "sweep_big": VARIANTS["sweep_big"], "eig_ql": VARIANTS["eig_ql"]}


def eigh_inputs():
    rng = np.random.default_rng(5)
    out = []
    for n in (17, 129):
        X = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))).astype(np.complex64)
        out.append(((X + X.conj().T) / 2)[None])
    return out


ENV_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join({root!r}, "tests"))
sys.path.insert(0, {root!r})
import test_gpu_options as T
out = {{}}
for name in T.FIXTURES:
    m = T.build(name)
    assert m.options is None
    out["phi:" + name], st = T.run(m, name)
    out["status:" + name] = np.array(st)
if {eigh}:
    for A_ in T.eigh_inputs():
        w, V = T.ops.eigh(torch.from_numpy(A_).cuda())
        out["w:%d" % A_.shape[-1]] = w.cpu().numpy()
        out["V:%d" % A_.shape[-1]] = V.cpu().numpy()
np.savez({path!r}, **out)
print("DONE")
"""


@pytest.fixture(scope="module")
def environment_runs(tmp_path_factory):
    """One child process per case, one after the other, each under its own time limit: the four fixtures (and for eig_ql two
    ops.eigh calls) under the case's ADMMNET_* variables.  A child that does not end cleanly ends the sequence: nothing more is
    started on the device behind an abort, a fault or a timeout."""
    d = tmp_path_factory.mktemp("env_runs")
    runs, stopped = {}, None
    for case, env in BITWISE.items():
        path = str(d / (case + ".npz"))
        code = ENV_CHILD.format(root=ROOT, path=path, eigh=case == "eig_ql")
        try:
            p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            stopped = f"the child of {case!r} ran into its time limit"
            break
        if p.returncode != 0 or "DONE" not in p.stdout:
            stopped = f"the child of {case!r} ended with status {p.returncode}: {p.stderr[-2000:]}"
            break
        runs[case] = dict(np.load(path))
    return runs, stopped


@pytest.mark.parametrize("case", list(BITWISE))
def test_options_are_the_environment_routes_bit_for_bit(environment_runs, case):
    runs, stopped = environment_runs
    if case not in runs:
        pytest.fail(f"no environment run of {case!r}: {stopped}")
    want = runs[case]
    opts = as_options(BITWISE[case])
    for name in FIXTURES:
        phi, st = run(build(name, opts), name)
        assert np.array_equal(phi, want["phi:" + name]), (case, name, float(np.abs(phi - want["phi:" + name]).max()))
        assert st == want["status:" + name].tolist(), (case, name, st, want["status:" + name].tolist())
    if case == "eig_ql":
        for A_ in eigh_inputs():
            n = A_.shape[-1]
            w, V = ops.eigh(torch.from_numpy(A_).cuda(), options=opts)
            assert np.array_equal(w.cpu().numpy(), want["w:%d" % n]) and np.array_equal(V.cpu().numpy(), want["V:%d" % n]), n
            w0, _ = ops.eigh(torch.from_numpy(A_).cuda())   # (and the default solver is another one: the option did something)
            assert not np.array_equal(w0.cpu().numpy(), want["w:%d" % n]), n


# ---- two models, two routes, one process -----------------------------------------------------------------------------------------------
PAIRS = ("admmnet_10x10_K3_default", "phiest_16x16_K3_perturbed")


def eigen_layers(m, B):
    """Matrix-layers of a forward that go through the dense eigen-pipeline: the G-layers k = 0 .. K - 2 of every signal (the last
    layer only produces phi) minus layer 0 where the arrowhead solver serves it (ADMMNET_ARROW, route.h Route::first)."""
    arrow = (m.options.resolved() if m.options is not None else A.options.describe(0))["arrow"]
    return B * (m.num_layers - 1) - (B if arrow else 0)


@pytest.fixture(scope="module")
def interleaved():
    """Per fixture: models A (options None) and B (Options(spectral=0)) called A, B, A, B; every call's (phi, status)."""
    out = {}
    for name in PAIRS:
        a, b = build(name), build(name, A.Options(spectral=0))
        out[name] = (a, b, [run(m, name) for m in (a, b, a, b)])
    return out


@pytest.mark.parametrize("name", PAIRS)
def test_no_leakage_between_models(interleaved, name):
    a, b, calls = interleaved[name]
    assert a.options is None and a.cfg().reserved[1] == 0 and b.cfg().reserved[1] >= 1
    (phi_a, st_a), (phi_b, st_b), (phi_a2, st_a2), (phi_b2, st_b2) = calls
    assert np.array_equal(phi_a2, phi_a) and st_a2 == st_a
    assert np.array_equal(phi_b2, phi_b) and st_b2 == st_b
    assert st_b[2] == 0 and st_a[2] > 0, (st_a, st_b)
    assert st_a[0] == 0 and st_b[0] == 0
    B = fixture(name)[1][3]
    assert st_a[1] + st_a[2] == eigen_layers(a, B), (st_a, B)   # every dense matrix-layer of A: evaluated or handed over
    assert not np.array_equal(phi_a, phi_b)                     # (two routes: close, not equal)
    ref = fixture(name)[3]
    assert max(float(np.abs(p - ref).max()) for p in (phi_a, phi_b)) / np.abs(ref).max() < 1e-4


@pytest.mark.parametrize("name", PAIRS)
def test_status_counts_the_eigen_layers_of_the_eigen_only_model(interleaved, name):
    """last_status[1] of the Options(spectral=0) model = B (K - 1) matrix-layers minus those the arrowhead layer serves: with the
    matrix-function route off for the call, every matrix of every dense layer goes through the eigensolver and is counted
    (admmnet_layer_front; with the route on, its kernel counts the matrices it hands over).  The same under the second call."""
    _, b, calls = interleaved[name]
    B = fixture(name)[1][3]
    st_b = calls[1][1]
    print(f"{name}: B = {B}, K = {b.num_layers}, status of the eigen-only model {st_b}, expected [1] = {eigen_layers(b, B)}")
    assert st_b[1] == eigen_layers(b, B), (st_b, eigen_layers(b, B))
    assert calls[3][1] == st_b and st_b[0] == 0 and st_b[2] == 0 and st_b[3] == 0


def launches():
    """Kernel launches per class since the last read (the measurement hooks of include/admmnet.h)."""
    lib = _lib.load()
    ms, n = (ctypes.c_double * 9)(), (ctypes.c_int64 * 9)()
    _lib.check(lib.admmnet_profile_read(ms, n, 9), "admmnet_profile_read")
    return list(n)


def test_errors_stay_per_model():
    """ADMMNET_REBUILD=tiles with the matrix-function route on is the one combination no kernel serves at D = 256: the model
    that asks for it gets the argument error before anything is launched, the next model its usual bits."""
    name = "phiest_16x16_K3_perturbed"
    good = build(name)
    phi0, st0 = run(good, name)
    bad = build(name, A.Options(rebuild="tiles"))
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.admmnet_profile_enable(1), "admmnet_profile_enable")
    try:
        launches()
        with pytest.raises(_lib.AdmmNetError, match=r"code -1.*ADMMNET_REBUILD=tiles"):
            bad(*fixture(name)[2])
        assert launches() == [0] * 9
        phi1, st1 = run(good, name)
        assert sum(launches()) > 0   # (the hook sees launches when there are any)
    finally:
        lib.admmnet_profile_enable(0)
    assert np.array_equal(phi1, phi0) and st1 == st0
    # with the route off the same switch is a variant like any other (rebuild_tiles above), still in this process
    phi2, st2 = run(build(name, A.Options(rebuild="tiles", spectral=0)), name)
    ref = fixture(name)[3]
    assert float(np.abs(phi2 - ref).max() / np.abs(ref).max()) < 1e-4 and st2[2] == 0
    phi3, st3 = run(good, name)
    assert np.array_equal(phi3, phi0) and st3 == st0


@pytest.mark.parametrize("name", PAIRS)
def test_sharded_forward_follows_the_model(name):
    m = build(name, A.Options(spectral=0))
    phi, st = run(m, name)
    sf = ShardedForward(m)
    phi_s, _ = sf(*fixture(name)[2])
    assert np.array_equal(phi_s.cpu().numpy(), phi)
    assert sf.last_status == st and st[2] == 0
    d = build(name)
    phi_d, st_d = run(d, name)
    sd = ShardedForward(d)
    phi_ds, _ = sd(*fixture(name)[2])
    assert np.array_equal(phi_ds.cpu().numpy(), phi_d) and sd.last_status == st_d and st_d[2] > 0


def test_training_route_follows_the_model():
    """forward_autograd's eigensolver runs under model.options: with Options(eig="ql") the differentiable forward gives the bits
    of the QL solver (ops.eigh under the same options handed in as the solver), which are not those of the default solver."""
    from admm_net_amd import training
    name = "phiest_8x16_K3_perturbed"
    dev = torch.device("cuda:0")
    y, b, s = fixture(name)[2]
    o = A.Options(eig="ql")
    out = {}
    for key, opts, solver in (("default", None, None), ("ql", o, None), ("ql_explicit", None, lambda X: ops.eigh(X, options=o))):
        m = build(name, opts).to(dev)
        with torch.no_grad():
            out[key] = training.unrolled_forward(m, y, b, s, solver=solver).cpu().numpy()
    assert np.array_equal(out["ql"], out["ql_explicit"])
    assert not np.array_equal(out["ql"], out["default"])
    ref = fixture(name)[3]
    assert max(float(np.abs(v - ref).max()) for v in out.values()) / np.abs(ref).max() < 1e-4
