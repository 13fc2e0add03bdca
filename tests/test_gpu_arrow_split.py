"""GPU (-m gpu): the first G-layer keeps its bits -- the leaner root solver (csrc/arrow_core.h ArrowPoles) at every D, and at
128 < D <= 256 the split form (arrow_rebuild_kernel<AR_SOLVE> + arrow_tail_kernel, the default) against the one-kernel form
(ADMMNET_ARROW_FUSED=2).

(a) ops.glayer(m, 0, phi, h, None) on the numpy-seeded inputs of test_gpu_arrow_fused.py (edge_cases, layer0_inputs, B = 6) at
    D = 1, 2, 64, 100, 127, 128, 129, 130, 160, 255, 256: G, w and rn have the SHA-256 recorded on the device from the build
    before this change (tests/golden/arrow_layer0_parent_sha256.json; `python tests/test_gpu_arrow_split.py record FILE` with
    that build's package imported first).  One and two lanes per root, the last root on the whole wave, NT = 5 and 8 tile rows,
    a single pole, rotations and deflated poles are among them.
(b) one process, through Options: at each D > 128 the split and the one-kernel form give equal bits, for the full-G entry and
    for a K = 2 forward (lower-triangle storage: phi, head, status words).
(c) NaN / Inf in phi or h: counted in status, nothing written by either kernel, the next call sound.
(d) m.chunk = 2 with B = 5: the bits of one chunk.
(e) 10 x 13 and 16 x 16, K = 3, spectral tolerance 0 (every matrix of layers >= 1 goes to the eigen-pipeline, which reuses the
    chunk buffers the records lived in): split and one-kernel form equal, also on a stream of the caller's and with the event
    profiler on.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import admm_net_amd as A                                  # noqa: E402
from admm_net_amd import _lib, ops, synth                 # noqa: E402
from oracle import admm_net_ref as R                      # noqa: E402
from test_gpu_arrow_fused import edge_cases, layer0_inputs   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "arrow_layer0_parent_sha256.json")
GEOM = {1: (1, 1), 2: (1, 2), 64: (8, 8), 100: (10, 10), 127: (1, 127), 128: (8, 16), 129: (3, 43), 130: (10, 13),
        160: (10, 16), 255: (15, 17), 256: (16, 16)}   # D -> (M, N)
BIG = [D for D in sorted(GEOM) if D > 128]
B = 6
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def options(**kw):
    from admm_net_amd.options import Options
    return Options(**kw)


def weights(D, layers=2, head=False):
    Nb, Nd = GEOM[D]
    return R.make_weights(Nb, Nd, layers, seed=D, head=head, perturb=0.3)


def phi_model(D, **overrides):
    Nb, Nd = GEOM[D]
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=2).eval()
    m.load_state_dict(weights(D))
    if overrides:
        m.options = options(**overrides)
    return m


def edge_cases_any(D):
    """edge_cases(D); its last case names pole 10, so below D = 11 the same recipe (same draws) runs with that index clamped."""
    if D > 10:
        return edge_cases(D)
    rng = np.random.default_rng(17)
    phis, hs = [], []
    for case in range(6):
        h = rng.uniform(0.05, 1.0, D)
        p = (rng.standard_normal(D) + 1j * rng.standard_normal(D)) * 0.1
        if case == 1: h = np.round(h, 2)
        if case == 2: p[::3] = 0
        if case == 3: h[:] = 0.37
        if case == 4: p *= 40
        if case == 5: h = np.sort(h); h[D - 1:30] = h[D - 1]; p[50:70] *= 1e-7
        phis.append(p); hs.append(h)
    return torch.from_numpy(np.stack(phis)).to(torch.complex128), torch.from_numpy(np.stack(hs)).to(torch.float64)


def layer0_cases(D):
    """{"edge", "layer0"} -> (phi c64, h f32) on the host, built once and left unchanged."""
    if D not in _cache:
        Nb, Nd = GEOM[D]
        out = {}
        for name, (phi, h) in (("edge", edge_cases_any(D)), ("layer0", layer0_inputs(weights(D), Nb, Nd, B))):
            out[name] = (phi.to(torch.complex64), h.float())
        _cache[D] = out
    return _cache[D]


def sha(t):
    t = (torch.view_as_real(t) if t.is_complex() else t).contiguous().cpu().numpy()
    return hashlib.sha256(t.tobytes()).hexdigest()


def glayer_hashes(m, D, dev):
    res = {}
    for name, (phi, h) in layer0_cases(D).items():
        G, w, rn = ops.glayer(m, 0, phi.to(dev), h.to(dev), None)
        res["D%d-%s" % (D, name)] = {"G": sha(G), "w": sha(w), "rn": sha(rn)}
    return res


# ------------------------------------------------------------------------------------------------ (a) the recorded bits
@pytest.mark.parametrize("D", sorted(GEOM))
def test_layer0_bits_equal_recorded(dev, D):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = glayer_hashes(phi_model(D), D, dev)
    for key, val in got.items():
        print("ARROWSPLIT", key, val["G"][:16], val["w"][:16], val["rn"][:16])
    for key, val in got.items():
        assert val == golden[key], key


# ------------------------------------------------------------------------------------------------ (b) split == one kernel
def test_the_switch_is_a_setting_of_its_own():
    one, split = options(arrow_fused=2), options()
    assert split.handle == 0 and one.handle != 0 and one.handle != options(arrow_fused=0).handle
    assert one.resolved()["arrow_fused"] == 1 and options(arrow_fused=0).resolved()["arrow_fused"] == 0


@pytest.mark.parametrize("D", BIG)
def test_split_equals_one_kernel_full_g(dev, D):
    assert glayer_hashes(phi_model(D), D, dev) == glayer_hashes(phi_model(D, arrow_fused=2), D, dev)


def forward_inputs(D, dev, n=B):
    Nb, Nd = GEOM[D]
    y, b, s, _ = synth.make_batch(n, Nb, Nd, seed=Nb * Nd)
    return [torch.from_numpy(t).to(dev) for t in (y, b, s)]


def net(D, layers, **overrides):
    Nb, Nd = GEOM[D]
    m = A.ADMMNet(M=Nb, N=Nd, num_layers=layers).eval()
    m.load_state_dict(weights(D, layers, head=True))
    if overrides:
        m.options = options(**overrides)
    return m


def forward_bits(m, inp):
    with torch.no_grad():
        out = m(*inp)
    torch.cuda.synchronize()
    return [sha(t) for t in out], list(m.last_status)


@pytest.mark.parametrize("D", BIG)
def test_split_equals_one_kernel_forward(dev, D):
    inp = forward_inputs(D, dev)
    got, want = forward_bits(net(D, 2), inp), forward_bits(net(D, 2, arrow_fused=2), inp)
    assert got == want and got[1][0] == 0, (got, want)


# ------------------------------------------------------------------------------------------------ (c) non-finite input
def raw_glayer(m, phi, h, fill):
    """admmnet_glayer_f32 as ops.glayer calls it, on outputs pre-filled with `fill`; -> (G, w, rn, status) without raising."""
    lib = _lib.load()
    dev = phi.device
    n_b, D = phi.shape
    n = D + 1
    cfg = m.cfg()
    W = m.packed_weights(dev)
    lw = W[lib.admmnet_layer_weight_offset(ctypes.byref(cfg), 0):]
    need = lib.admmnet_glayer_workspace_bytes(ctypes.byref(cfg), n_b)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    G = torch.full((n_b, n, n), complex(fill, fill), dtype=torch.complex64, device=dev)
    w = torch.full((n_b, n), fill, dtype=torch.float32, device=dev)
    rn = torch.full((n_b,), fill, dtype=torch.float32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    _lib.check(lib.admmnet_glayer_f32(ctypes.byref(cfg), ops._ptr(lw), ops._ptr(phi), ops._ptr(h), None, n_b, ops._ptr(G),
                                      ops._ptr(w), ops._ptr(rn), ops._ptr(ws), need, ops._ptr(status), ops._stream(dev)),
               "admmnet_glayer_f32")
    torch.cuda.synchronize()
    return G, w, rn, status.tolist()


@pytest.mark.parametrize("form", ["split", "one_kernel"])
@pytest.mark.parametrize("D", [129, 256])
def test_nonfinite_input_counted_nothing_written(dev, D, form):
    m = phi_model(D, **({"arrow_fused": 2} if form == "one_kernel" else {}))
    phi, h = (t.to(dev) for t in layer0_cases(D)["edge"])
    fill = -7.0
    Gc, wc, rnc, st = raw_glayer(m, phi, h, fill)
    assert st[0] == 0
    for bad in (float("nan"), float("inf")):
        hb = h.clone(); hb[1, 2] = bad
        pb = phi.clone(); pb[4, D - 1] = complex(bad, 0.0)
        G, w, rn, st = raw_glayer(m, pb, hb, fill)
        assert st[0] == 2, st
        for i in range(B):
            if i in (1, 4):   # left exactly as they were
                assert bool((torch.view_as_real(G[i]) == fill).all()) and bool((w[i] == fill).all()) and float(rn[i]) == fill
            else:
                assert torch.equal(torch.view_as_real(G[i]), torch.view_as_real(Gc[i]))
                assert torch.equal(w[i], wc[i]) and torch.equal(rn[i], rnc[i])
        with pytest.raises(_lib.AdmmNetError):
            ops.glayer(m, 0, pb, hb, None)
    G, w, rn, st = raw_glayer(m, phi, h, fill)   # the next call is sound
    assert st[0] == 0 and torch.equal(torch.view_as_real(G), torch.view_as_real(Gc)) and torch.equal(w, wc) and torch.equal(rn, rnc)


# ------------------------------------------------------------------------------------------------ (d) chunks
@pytest.mark.parametrize("D", [130, 256])
def test_chunk_of_two_gives_the_bits_of_one_chunk(dev, D):
    phi, h = (t[:5].to(dev) for t in layer0_cases(D)["edge"])
    m = phi_model(D)
    want = [sha(t) for t in ops.glayer(m, 0, phi, h, None)]
    m.chunk = 2
    assert [sha(t) for t in ops.glayer(m, 0, phi, h, None)] == want


# ------------------------------------------------------------------------------------------------ (e) the buffers' next user
@pytest.mark.parametrize("how", ["plain", "own_stream", "profiler"])
@pytest.mark.parametrize("D", [130, 256])
def test_records_and_the_eigen_pipeline_share_buffers(dev, D, how):
    inp = forward_inputs(D, dev)
    lib = _lib.load()
    res = []
    if how == "profiler":
        _lib.check(lib.admmnet_profile_enable(1), "admmnet_profile_enable")
    try:
        for extra in ({}, {"arrow_fused": 2}):
            m = net(D, 3, spectral_tol="0", **extra)
            m.chunk = 4                                     # two chunks, the second short
            if how == "own_stream":
                s = torch.cuda.Stream(dev)
                s.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(s):
                    res.append(forward_bits(m, inp))
            else:
                res.append(forward_bits(m, inp))
    finally:
        if how == "profiler":
            lib.admmnet_profile_enable(0)
    assert res[0] == res[1], res
    st = res[0][1]
    assert st[0] == 0 and st[1] >= B and st[2] == 0, st   # no matrix was accepted as a matrix function: all went to the eigen-pipeline


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        device = torch.device("cuda:0")
        _lib.load()
        out = {}
        for D_ in sorted(GEOM):
            out.update(glayer_hashes(phi_model(D_), D_, device))
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("recorded", len(out), "entries from", os.path.dirname(A.__file__))
    else:
        sys.exit("usage: test_gpu_arrow_split.py record FILE")
