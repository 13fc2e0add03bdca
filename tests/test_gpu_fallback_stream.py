"""GPU: the eigensolver fallback of a chunk on the side stream, beside the next chunk's matrix-function kernel (csrc/api.hip,
admmnet_layer_front), gives the bits of the serial order.  "Serial" is ``ADMMNET_STREAMS=1`` -- everything on the caller's
stream -- carried per model by ``Options(streams=1)``, so both sides run in this process on the same inputs: the outputs (phi and
the three head outputs) and the four status words must be equal bit for bit.  Every model is an ``ADMMNet`` with default-init
weights (``torch.manual_seed``, seed 0 except at 10 x 10: WEIGHT_SEED): its head writes the K / V buffer whose memory the second
flag buffer borrows while the layers run.  Nothing here can see which stream a kernel ran on; the cases are chosen so that a
missing wait, a flag buffer overwritten too early or a join left out changes the bits or the status words."""
import ctypes

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, synth

pytestmark = pytest.mark.gpu
K = 4   # layer 0 is the arrowhead layer, layers 1 and 2 are dense (the side stream and both flag buffers are used again), layer 3 is phi only
# 10 x 10, K = 4, 32 signals: how many of the 2 x 32 dense matrix-layers the serial path hands to the eigensolver (status word 1),
# measured on the MI355X per weight seed -- 0: 0, 1: 32, 2: 0, 3: 0, 4: 42, 5: 0, 6: 5, 7: 14.  There is no host model of the kernel's
# acceptance checks to ask beforehand.  Seed 0 rejects nothing at this depth; seed 1's 32 may be one whole layer, which would
# leave every chunk with all or none of its matrices flagged; seed 4 is the first whose count is no multiple of 32, i.e.
# certainly a mix inside a layer.
WEIGHT_SEED = {(10, 10): 4}
_cache = {}


def inputs(M, N, B):
    """(y, b, sigma) on the device, generated once per (geometry, batch) and left unchanged."""
    key = ("in", M, N, B)
    if key not in _cache:
        _cache[key] = synth.make_batch_device(B, M, N, seed=20260104, device=torch.device("cuda:0"))[:3]
    return _cache[key]


def model(M, N, chunk, **overrides):
    torch.manual_seed(WEIGHT_SEED.get((M, N), 0))
    m = A.ADMMNet(M=M, N=N, L=3, num_layers=K).eval()
    m.chunk = chunk
    m.options = A.Options(**overrides) if overrides else None
    return m


def run(m, M, N, B):
    """-> ([tau, f, confidence, phi] as numpy, the four status words)."""
    with torch.no_grad():
        out = m(*inputs(M, N, B))
    return [t.cpu().numpy() for t in out], list(m.last_status)


def serial(M, N, B, chunk, **overrides):
    """The same call with everything on the caller's stream; computed once per case."""
    key = ("serial", M, N, B, chunk, tuple(sorted(overrides.items())))
    if key not in _cache:
        _cache[key] = run(model(M, N, chunk, streams=1, **overrides), M, N, B)
    return _cache[key]


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i)
        assert np.isfinite(w.view(np.float32)).all(), (what, i)
        assert g.tobytes() == w.tobytes(), (what, i, float(np.abs(g - w).max()))


def test_the_escape_hatch_is_a_setting_of_its_own():
    """``streams=1`` interns a handle of its own (the field is compared), and the value ``ADMMNET_STREAMS`` prints stays the
    two-chunk switch."""
    one, none_, two = A.Options(streams=1), A.Options(), A.Options(streams=2)
    assert none_.handle == 0 and one.handle != 0 and two.handle not in (0, one.handle)
    assert one.resolved()["streams"] == 0 and two.resolved()["streams"] == 1


def test_mixed_accept_and_reject_d_le_128():
    """10 x 10, B = 32 in 4 chunks of 8, weights that make the kernel reject some matrices of a layer and accept others
    (WEIGHT_SEED): the side stream, both flag buffers and the skip filter of every fallback kernel carry a real mix."""
    M, N, B, chunk = 10, 10, 32, 8
    want, st_want = serial(M, N, B, chunk)
    got, st = run(model(M, N, chunk), M, N, B)
    print("status", st, "serial", st_want)
    assert 0 < st[1] < 2 * B, st   # neither an empty nor a total fallback: two dense layers of B matrices
    assert st[1] % B != 0, st      # (nor one whole layer and nothing of the other)
    assert st == st_want
    assert_same_bits(got, want, "10x10")


@pytest.mark.parametrize("tol", [None, "0"])
@pytest.mark.parametrize("M,N", [(10, 13), (16, 16)])
def test_padded_pipeline_with_late_half_image(M, N, tol):
    """D > 128 (D = 130 runs padded in the D = 256 pipeline; D = 256 itself): the half image is built on the side stream for the
    flagged matrices.  B = 5 in chunks of 2, a short last chunk; with tolerance 0 every matrix goes through the fallback."""
    B, chunk = 5, 2
    over = {} if tol is None else {"spectral_tol": tol}
    want, st_want = serial(M, N, B, chunk, **over)
    got, st = run(model(M, N, chunk, **over), M, N, B)
    print("status", st, "serial", st_want)
    if tol is not None:
        assert st[1] == 2 * B and st[2] == 0, st
    assert st == st_want
    assert_same_bits(got, want, f"{M}x{N} tol {tol}")


@pytest.mark.parametrize("M,N,B,chunk", [(10, 10, 32, 8), (10, 13, 5, 2)])
def test_same_forward_twice(M, N, B, chunk):
    """The second call finds the head's K / V values where its second flag buffer lies and the chunk buffers as the first left
    them: a reuse-ordering mistake shows as a difference."""
    m = model(M, N, chunk)
    first, st1 = run(m, M, N, B)
    second, st2 = run(m, M, N, B)
    assert st1 == st2
    assert_same_bits(second, first, "second call")
    assert_same_bits(first, serial(M, N, B, chunk)[0], "first call")


def test_caller_on_a_non_default_stream():
    """The forward enqueued on a torch stream of the caller's, its outputs consumed on that stream without a device
    synchronise: the join puts everything the side stream did in front of what the caller enqueues next."""
    M, N, B, chunk = 10, 10, 32, 8
    want, _ = serial(M, N, B, chunk)
    y, b, s = inputs(M, N, B)
    m = model(M, N, chunk)
    m.check_status = False   # (its read of the status words would wait for the stream)
    side = torch.cuda.Stream(device=y.device)
    side.wait_stream(torch.cuda.current_stream(y.device))
    with torch.cuda.stream(side), torch.no_grad():
        out = m(y, b, s)
        doubled = [torch.view_as_real(t) * 2 if t.is_complex() else t * 2 for t in out]   # consumers on the same stream
        got = [t.cpu().numpy() for t in out]
        twice = [t.cpu().numpy() for t in doubled]
    assert_same_bits(got, want, "non-default stream")
    for t2, w in zip(twice, want):
        assert t2.tobytes() == (w.view(np.float32) * np.float32(2)).tobytes()   # (complex64 viewed as pairs: the same bytes)


def test_profiler_on_keeps_one_stream_and_the_bits():
    M, N, B, chunk = 10, 10, 32, 8
    want, st_want = serial(M, N, B, chunk)
    lib = _lib.load()
    m = model(M, N, chunk)
    _lib.check(lib.admmnet_profile_enable(1), "admmnet_profile_enable")
    try:
        got, st = run(m, M, N, B)
        assert int(lib.admmnet_profile_dropped()) == 0
        ms, cnt = (ctypes.c_double * 9)(), (ctypes.c_int64 * 9)()
        _lib.check(lib.admmnet_profile_read(ms, cnt, 9), "admmnet_profile_read")
        assert sum(cnt) > 0
    finally:
        lib.admmnet_profile_enable(0)
    assert st == st_want
    assert_same_bits(got, want, "profiler on")


def test_chunk_too_large_for_the_aliased_flag_buffer():
    """2 x 4: the head's K / V buffer holds 256 D = 2048 flags, a chunk of 2049 does not fit -- the call stays on one stream
    (and must not write flags behind that buffer)."""
    M, N, chunk = 2, 4, 256 * 8 + 1
    B = 2 * chunk + 1
    want, st_want = serial(M, N, B, chunk)
    got, st = run(model(M, N, chunk), M, N, B)
    assert st == st_want
    assert_same_bits(got, want, "2x4")
