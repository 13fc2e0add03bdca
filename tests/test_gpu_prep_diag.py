"""GPU (-m gpu): the compact diagonals (csrc/common.h, Ws::diag / Ws::diag_ok).  From layer 2 on prep_kernel takes Re diag G and
Re diag Z from two rows that sp_fused_kernel of the layer before left for it, and gathers them from the matrices only where that
kernel rejected the matrix.  The rows hold the very floats of G[i][i].x and Z[i][i].x, so nothing may move by a bit.

The reference of every comparison is this tree with the consumer switched off -- ``Options(sf_fold=2)``, ADMMNET_SF_FOLD=2: the
fold as by default, prep_kernel gathering in every layer -- on the same inputs in the same process; phi, the three head outputs and
the four status words must be equal bit for bit (no tolerance anywhere in this file).  The buffers themselves are read out of
the workspace and compared with the diagonals of G and Z.

K = 4 unless stated: layer 0 is the arrowhead layer, layer 1 the first producer, layer 2 the first (and only) layer whose
prep_kernel reads the rows and whose h reaches phi of layer 3; batches of 5 to 32 signals, and 520 where the four-wave shape of
sp_fused_kernel (more than 512 signals, D <= 128) is meant.
"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, ops, sharded, synth
from admm_net_amd.options import Options
from oracle import admm_net_ref as R

pytestmark = pytest.mark.gpu

K = 4
GRIDS = {24: (4, 6), 25: (5, 5), 31: (1, 31), 32: (4, 8), 33: (3, 11), 63: (7, 9), 64: (8, 8), 65: (5, 13), 100: (10, 10),
         128: (8, 16), 129: (3, 43), 192: (12, 16), 255: (15, 17), 256: (16, 16)}   # D -> (M, N)
# weights that make sp_fused_kernel reject nothing: R.make_weights(seed, perturb=0.3), seed 7 except where it rejects -- seed 2 at
# D = 63, 128, 129 (profiles/r13/README.md section 6).  D = 31 and 33 are not in that list: measured on the MI355X with the 5 signals
# of these tests, K = 4, rejected of 10 matrix-layers -- D = 31: seed 7 1, 2 0, 1 1, 3 1, 5 0; D = 33: seed 7 3, 2 5, 1 0, 3 0, 5 0
WEIGHT_SEED = {31: 5, 33: 5, 63: 2, 128: 2, 129: 2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glayer_spectral_parent_sha256.json")
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def inputs(D, B):
    """(y, b, sigma) on the device, generated once per (size, batch) and left unchanged."""
    if (D, B) not in _cache:
        M, N = GRIDS[D]
        _cache[D, B] = synth.make_batch_device(B, M, N, seed=20260104, device=torch.device("cuda:0"))[:3]
    return _cache[D, B]


def model(D, layers=K, init_seed=None, **overrides):
    """ADMMNet on the grid of D: R.make_weights(seed 7, or WEIGHT_SEED) -- or, with init_seed, the default initialisation under
    torch.manual_seed(init_seed), as tests/test_gpu_fallback_stream.py builds its models."""
    M, N = GRIDS[D]
    if init_seed is not None:
        torch.manual_seed(init_seed)
    m = A.ADMMNet(M=M, N=N, L=3, num_layers=layers).eval()
    if init_seed is None:
        m.load_state_dict(R.make_weights(M, N, layers, L=3, seed=WEIGHT_SEED.get(D, 7), head=True, perturb=0.3))
    if overrides:
        m.options = Options(**overrides)
    return m


def forward(m, D, B):
    """-> ([tau, f, confidence, phi] on the host, the four status words)."""
    with torch.no_grad():
        out = m(*inputs(D, B))
    torch.cuda.synchronize()
    return [t.cpu() for t in out], list(m.last_status)


def bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def assert_same(got, want, what):
    (g, sg), (w, sw) = got, want
    print(f"PREPDIAG {what}: status on {sg} off {sw}")
    assert sg == sw, what
    assert len(g) == len(w) == 4
    for i, (a, b) in enumerate(zip(g, w)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i)
        assert bool(torch.isfinite(torch.view_as_real(b) if b.is_complex() else b).all()), (what, i)
        assert torch.equal(bits(a), bits(b)), (what, i, int((bits(a) != bits(b)).sum()))


def on_and_off(D, B, chunk=0, layers=K, init_seed=None, sub_batch=None, **overrides):
    res = []
    for extra in ({}, {"sf_fold": 2}):
        m = model(D, layers, init_seed, **dict(overrides, **extra))
        m.chunk = chunk
        if sub_batch:
            m.sub_batch = sub_batch
        res.append(forward(m, D, B))
    return res


# --------------------------------------------------------------------------------------- the switch, the route and the workspace
def test_the_switch_is_a_setting_of_its_own():
    """ADMMNET_SF_FOLD=2 keeps the fold (the value the switch prints stays 1) and is compared when option sets are interned."""
    off, on = Options(sf_fold=2), Options()
    assert on.handle == 0 and off.handle != 0 and off.handle != Options(sf_fold=0).handle
    assert off.resolved()["sf_fold"] == 1 and Options(sf_fold=0).resolved()["sf_fold"] == 0


def _cfg(D, layers, opts=None):
    M, N = GRIDS[D]
    return _lib.Cfg(M, N, 3, layers, 0, 0, (ctypes.c_int32 * 2)(0, 0 if opts is None else Options(**opts).handle))


def _align(x):
    return -(-x // 256) * 256


def _diag_offsets(D, B):
    """Byte offsets of diag and diag_ok: behind sum (one pair), mean (four floats) and headkv, which follow the reported spans."""
    _, end, _ = sharded.state_layout(_cfg(D, K), B)
    diag = end + 256 + 256 + _align(4 * 2 * D * 128)
    return diag, diag + _align(4 * B * 2 * D)


# admmnet_state_layout of the parent commit, (D, B) -> the nine offsets, read from its build: the new buffers lie behind them
PARENT_OFFSETS = {
    (100, 5): [0, 408064, 816128, 820224, 824320, 826368, 828416, 828672, 828928],
    (256, 20): [0, 10567936, 21135872, 21176832, 21217792, 21238272, 21258752, 21259008, 21259264],
}


@pytest.mark.parametrize("D,B", sorted(PARENT_OFFSETS))
def test_reported_offsets_are_the_parents_and_the_buffers_lie_behind_them(D, B):
    lib = _lib.load()
    for layers in (3, 4, 16):
        off = (ctypes.c_int64 * 9)()
        _lib.check(lib.admmnet_state_layout(ctypes.byref(_cfg(D, layers)), B, off, None), "admmnet_state_layout")
        assert list(off) == PARENT_OFFSETS[D, B], layers
    need = {layers: lib.admmnet_workspace_bytes(ctypes.byref(_cfg(D, layers, o)), B)
            for layers, o in ((3, None), (4, None), (16, None))}
    grow = _align(4 * B * 2 * D) + _align(4 * B)
    assert need[4] == need[16] == need[3] + grow, need           # fewer than four layers: no layer reads the rows, no buffers
    for o in (dict(sf_fold=0), dict(spectral_fused=0), dict(spectral=0)):   # routes that never write them
        assert lib.admmnet_workspace_bytes(ctypes.byref(_cfg(D, 4, o)), B) == lib.admmnet_workspace_bytes(ctypes.byref(_cfg(D, 3, o)), B)
    assert lib.admmnet_workspace_bytes(ctypes.byref(_cfg(D, 4, dict(sf_fold=2))), B) == need[4]   # (the producer stays on)
    diag, ok = _diag_offsets(D, B)
    assert ok + _align(4 * B) <= need[4]


# ----------------------------------------------------------------------------------------- whole forward, switch on against off
@pytest.mark.parametrize("D", sorted(GRIDS))
def test_forward_keeps_its_bits(dev, D):
    """Partial diagonal tiles (24, 25, 31, 33, 63, 65, 100, 129, 255), full ones, the last tile row, one to three tiles per wave
    of the twelve-wave shape and the padded route (129, 192, 255).  Nothing is rejected, so every matrix of layer 2 takes the rows."""
    on, off = on_and_off(D, 5)
    assert_same(on, off, f"D={D}")
    assert on[1][0] == 0 and on[1][1] == 0 and on[1][2] == 2 * 5, on[1]


@pytest.mark.parametrize("D", [25, 65, 100, 128])
def test_forward_keeps_its_bits_in_the_four_wave_shape(dev, D):
    """More than 512 signals at D <= 128: four waves per matrix, one, two and three tiles per wave (D = 25, 65, 100 / 128)."""
    on, off = on_and_off(D, 520)
    assert_same(on, off, f"D={D} B=520")
    assert on[1][2] > 0, on[1]


@pytest.mark.parametrize("tol", [None, "0"])
def test_mixed_batch(dev, tol):
    """10 x 10, default-init weights of seed 4, 32 signals in chunks of 8 (tests/test_gpu_fallback_stream.py: 42 of the 64
    matrix-layers rejected): accepted matrices take the rows and rejected ones the gather, in one launch.  With tolerance 0
    every matrix is rejected and diag_ok is zero throughout."""
    over = {} if tol is None else {"spectral_tol": tol}
    on, off = on_and_off(100, 32, chunk=8, init_seed=4, **over)
    assert_same(on, off, f"mixed tol {tol}")
    st = on[1]
    if tol is None:
        assert 0 < st[1] < 2 * 32 and st[2] > 0, st
    else:
        assert st[1] == 2 * 32 and st[2] == 0, st


@pytest.mark.parametrize("how", ["side_stream", "streams_1", "streams_2", "sub_batches", "profiler"])
def test_chunks_and_streams(dev, how):
    """20 signals in chunks of 8: a short last chunk, slices of both buffers at b0 > 0.  With the eigensolver fallback on the side
    stream (weights that reject some matrices), on one stream, with two chunks in flight, with two sub-batches of unequal size
    and with the event profiler on."""
    over = {"streams": 1} if how == "streams_1" else {"streams": 2} if how == "streams_2" else {}
    lib = _lib.load()
    if how == "profiler":
        _lib.check(lib.admmnet_profile_enable(1), "admmnet_profile_enable")
    try:
        on, off = on_and_off(100, 20, chunk=8, init_seed=4, sub_batch=12 if how == "sub_batches" else None, **over)
    finally:
        if how == "profiler":
            lib.admmnet_profile_enable(0)
    assert_same(on, off, how)
    assert on[1][2] > 0, on[1]


# ------------------------------------------------------------------------------------------------------------------- staleness
def _engine_run(eng):
    eng.begin()
    for k in range(K):
        sc = eng.front(k)
        if k < K - 1:
            eng.back_pair(k, sc)
    phi, head = eng.finish()
    torch.cuda.synchronize()
    return [head.cpu().clone(), phi.cpu().clone()], eng.status.cpu().tolist()


def test_rows_of_an_earlier_call_are_never_read(dev):
    """One workspace: a forward that accepts everything, then one at tolerance 0 (every matrix rejected).  A diag_ok left over
    from the first call would hand the second one rows of other matrices; it must equal the gather."""
    D, B = 64, 8
    y, b, s = inputs(D, B)
    first = sharded.HipLayerEngine(model(D), y, b, s)
    _, st = _engine_run(first)
    assert st[1] == 0 and st[2] == 2 * B, st
    res = []
    for extra in ({}, {"sf_fold": 2}):
        eng = sharded.HipLayerEngine(model(D, spectral_tol="0", **extra), y, b, s)
        assert eng.ws.numel() == first.ws.numel()
        eng.ws = first.ws                                    # the workspace the accepting forward left behind
        res.append(_engine_run(eng))
        ok_off = _diag_offsets(D, B)[1]
        assert int(first.ws[ok_off:ok_off + 4 * B].view(torch.int32).abs().sum()) == 0   # all rejected: no row is valid
    (g, sg), (w, sw) = res
    assert sg == sw and sg[1] == 2 * B and sg[2] == 0, (sg, sw)
    for a, c in zip(g, w):
        assert torch.equal(bits(a), bits(c))


# --------------------------------------------------------------------------------------------------------- the buffers themselves
@pytest.mark.parametrize("D,init_seed,tol", [(25, None, None), (64, None, None), (129, None, None), (256, None, None),
                                             (100, 4, None), (64, None, "0")],
                         ids=["D25", "D64", "D129", "D256", "D100-mixed", "D64-all-rejected"])
def test_rows_are_the_diagonals(dev, D, init_seed, tol):
    """begin, front(0), back(0), front(1) through the layer-at-a-time C ABI, then G, Z, diag and diag_ok out of the workspace: for
    every matrix the kernel accepted, row 0 is Re diag G and row 1 Re diag Z of the D x D block, bit for bit, and diag_ok is
    (flag == 0) -- the flags from the single-layer entry (ops.glayer_spectral) on the same inputs."""
    B = 16 if init_seed is not None else 6
    y, b, s = inputs(D, B)
    m = model(D, K, init_seed, **({} if tol is None else {"spectral_tol": tol}))
    eng = sharded.HipLayerEngine(m, y, b, s)
    eng.ws.zero_()                                           # (a row that was not stored reads as zeros)
    eng.begin()
    eng.back_pair(0, eng.front(0))
    st = eng.state()
    G0, alpha = st.G.clone(), st.alpha.clone()
    eng.front(1)
    torch.cuda.synchronize()
    doff, ooff = _diag_offsets(D, B)
    diag = eng.ws[doff:doff + 4 * B * 2 * D].view(torch.float32).view(B, 2, D).cpu()
    ok = eng.ws[ooff:ooff + 4 * B].view(torch.int32).cpu()
    G, Z = st.G.cpu(), st.Z.cpu()
    # the flags of the same launch, from the single-layer entry: mode 2 (stored Z taken as zero), the forward's shape for B signals
    Zs, rn = torch.zeros_like(st.Z), torch.zeros(B, device=dev)
    flag, _ = ops.glayer_spectral(m, 1, st.phi(1).clone(), st.h(1).clone(), Zs, G0, rn, 2, alpha, st.phi(0).clone(), st.h(0).clone())
    torch.cuda.synchronize()
    flag = flag.cpu()
    print(f"PREPDIAG buffers D={D}: flags {flag.tolist()} diag_ok {ok.tolist()} status {eng.status.tolist()}")
    assert torch.equal(ok, (flag == 0).to(torch.int32))
    assert int(eng.status[2]) == int(ok.sum()) and int(eng.status[1]) == B - int(ok.sum())
    if tol is None and init_seed is None:
        assert bool(ok.all())
    if tol is not None:
        assert not bool(ok.any())
    if init_seed is not None:
        assert 0 < int(ok.sum()) < B, ok.tolist()
    acc = ok != 0
    gd = torch.diagonal(G, dim1=1, dim2=2)[:, :D].real.contiguous()
    zd = torch.diagonal(Z, dim1=1, dim2=2)[:, :D].real.contiguous()
    assert torch.equal(bits(diag[acc, 0]), bits(gd[acc]))
    assert torch.equal(bits(diag[acc, 1]), bits(zd[acc]))
    assert bool((diag[~acc] == 0).all())                          # a rejected matrix leaves no row


# ------------------------------------------------------------------------------------------------------------------ null pointers
def _sha(t):
    return hashlib.sha256(bits(t).numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("D,waves,mode", [(25, 12, 0), (25, 12, 1), (25, 12, 2), (25, 4, 0), (25, 4, 1), (25, 4, 2),
                                          (256, 12, 0), (256, 12, 1), (256, 12, 2)])
def test_single_layer_entry_gives_the_parents_bits(dev, D, waves, mode):
    """ops.glayer_spectral passes no buffers: on the inputs of tests/test_gpu_sf_pipeline.py it returns the Z, G, rn and flags the
    parent commit returned (SHA-256 of each whole allocation, guard matrices and upper triangles included, recorded from the
    parent's build in tests/golden/glayer_spectral_parent_sha256.json)."""
    import test_gpu_sf_pipeline as P
    with open(GOLDEN) as fh:
        want = json.load(fh)[f"D{D}-W{waves}-mode{mode}"]
    x = P._inputs(D, mode)
    Z, G, rn, flag, st = P._run(dev, D, waves, mode, x["Z"], x["G"])
    got = {"Z": _sha(Z), "G": _sha(G), "rn": _sha(rn), "flag": _sha(flag), "status": st.tolist()}
    assert got == want
