"""GPU (-m gpu): batched top-L target estimation on the device (csrc/estimate.hip, ``ops.peak_top``,
``model.estimate``).  Every comparison is exact (bit patterns; NaN rows by mask) except the heights against the
oracle's literal search, which carry the tolerances of tests/test_gpu_parity.py.

Two yardsticks:
  * the DEFINITION: ``peak_search.top_rows`` (the reference callers' sort and cut, main_for_net.py:119,126) applied
    to the device's own uncapped peak list (``ops.peak_search`` with ``max_peaks`` >= the number of maxima);
  * the REFERENCE'S SEMANTICS: the same two lines applied to oracle/peak_search_ref.py's literal alt_peak_search.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, ops, peak_search, synth
from golden_util import load_fixture
from oracle import peak_search_ref as PO

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = sorted(p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))
              if os.path.basename(p).startswith(("phiest_", "admmnet_")))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_rows_equal(got, want):
    """Exact: NaN rows by mask, everything else by bit pattern."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    mask = np.isnan(want)
    assert np.array_equal(np.isnan(got), mask)
    assert np.array_equal(_bits(got)[~mask], _bits(want)[~mask])


def definition(pk, cnt, L, top_n=None):
    """[B, L, 3]: ``top_rows`` of every signal's full peak list, NaN-padded."""
    B = pk.shape[0]
    want = np.full((B, L, 3), np.nan)
    for i in range(B):
        assert cnt[i] <= pk.shape[1], "the comparison list must hold every maximum"
        Lb = L if top_n is None else min(max(int(top_n[i]), 0), L)
        rows = peak_search.top_rows(pk[i, :cnt[i]], Lb)
        want[i, :rows.shape[0]] = rows
    return want


def oracle_top(phi_row, xbase, ybase, opts, L):
    res = PO.alt_peak_search_literal({"phi": np.asarray(phi_row).astype(np.complex128), "xbase": xbase, "ybase": ybase}, opts)
    res = sorted(res, key=lambda x: x[2], reverse=True)
    return np.asarray(res[:L], dtype=np.float64).reshape(-1, 3)


def forward_phi(dev, Nb, Nd, B, seed=23, layers=3):
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=seed, snr_range=(10.0, 20.0))
    torch.manual_seed(2)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=layers).eval()
    return m(torch.from_numpy(y).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev))


# ------------------------------------------------------------------ 3. the definition
@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("geom", [(10, 10), (8, 16), (16, 16)], ids=["10x10", "8x16", "16x16"])
def test_peak_top_equals_top_rows_of_the_device_peak_list(dev, geom, iters):
    """ops.peak_top == top_rows(ops.peak_search rows), all three columns bit for bit, and equal counts; L in
    {1, 3, 8, 64}, B in {1, 6, 257}, with and without a per-signal top_n holding 0, values below L and values above the
    count.  iters = 0 leaves every height 0.0: the whole selection is then decided by the tie rule."""
    Nb, Nd = geom
    opts = {"xstep": 1 / (4 * Nd), "ystep": 1 / (4 * Nb), "iter": iters}
    ax, ay = peak_search.coarse_axes(opts)
    cap = len(ax) * len(ay)
    for B in (1, 6, 257):
        phi = forward_phi(dev, Nb, Nd, B)
        pk, cnt = ops.peak_search(phi, Nb, Nd, opts, max_peaks=cap)
        pk, cnt = pk.cpu().numpy(), cnt.cpu().numpy()
        assert (cnt > 0).all() and (cnt <= cap).all()
        if iters == 0:
            assert not pk[:, :, 2].any()
        pattern = np.array([0, 1, 2, 7, 10 ** 6, 63, 3, -5], dtype=np.int64)    # 10^6 > any count (<= cap)
        shifts = range(len(pattern)) if B < len(pattern) else [0]
        for L in (1, 3, 8, 64):
            top, c = ops.peak_top(phi, Nb, Nd, opts, top=L)
            assert top.shape == (B, L, 3) and top.dtype == torch.float64 and top.device == phi.device
            assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), cnt)
            assert_rows_equal(top.cpu().numpy(), definition(pk, cnt, L))
            for sh in shifts:
                tn = np.roll(np.resize(pattern, max(B, len(pattern))), -sh)[:B]
                top, c = ops.peak_top(phi, Nb, Nd, opts, top=L, top_n=torch.from_numpy(tn))
                assert np.array_equal(c.cpu().numpy(), cnt)
                assert_rows_equal(top.cpu().numpy(), definition(pk, cnt, L, tn))


# ------------------------------------------------------------------ 4. the reference's semantics
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_estimate_equals_sorted_and_cut_oracle_search_on_the_reference_phi(dev, path):
    """model.estimate on every golden fixture, options of test_peaks_of_hip_phi_equal_peaks_of_reference_phi, top = 3:
    (tau, f) equal, bit for bit, those of sorted(..)[:3] of the oracle's literal alt_peak_search on the REFERENCE's
    stored phi; heights within that test's 5e-4 of the largest."""
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load_fixture(path)
    assert Nb * Nd >= 9
    m = (A.ADMMNet if head else A.PhiEstADMMNet)(M=Nb, N=Nd, L=L, num_layers=K)
    m.load_state_dict(sd)
    m.eval()
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    opts = {"xstep": 1 / (4 * Nd), "ystep": 1 / (4 * Nb), "iter": 2}
    tau, f, height, counts, phi = m.estimate(y.to(dev), b.to(dev), s.to(dev), top=3, opts=opts)
    assert tau.shape == (B, 3) and phi.shape == (B, Nb * Nd)
    tau, f, height = tau.cpu().numpy(), f.cpu().numpy(), height.cpu().numpy()
    for i in range(B):
        want = oracle_top(z["phi"][i], Nb, Nd, opts, 3)
        assert want.shape == (3, 3)
        assert np.array_equal(_bits(tau[i]), _bits(want[:, 0])), (tau[i], want)
        assert np.array_equal(_bits(f[i]), _bits(want[:, 1])), (f[i], want)
        assert np.abs(height[i] - want[:, 2]).max() <= 5e-4 * want[:, 2].max()


# ------------------------------------------------------------------ 5. more maxima than any old capacity
def test_every_maximum_takes_part_beyond_the_old_capacity(dev):
    """Noise phi of length 1024 on a 64 x 64 grid: well over 256 regional maxima per signal, the highest ones deep in
    the np.where list.  peak_top == the definition (uncapped list) == the oracle's literal search sorted and cut;
    the host route at its default capacity refuses the input."""
    rng = np.random.default_rng(1)
    phi_h = np.stack([(rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex64) for _ in range(3)])
    phi = torch.from_numpy(phi_h).to(dev)
    opts = {"xstep": 1 / 65, "ystep": 1 / 65, "iter": 1}
    ax, ay = peak_search.coarse_axes(opts)
    assert (len(ax), len(ay)) == (64, 64)
    top, cnt = ops.peak_top(phi, 32, 32, opts, top=3)
    top, cnt = top.cpu().numpy(), cnt.cpu().numpy()
    assert (cnt > 256).all(), cnt
    pk, c2 = ops.peak_search(phi, 32, 32, opts, max_peaks=4096)
    pk, c2 = pk.cpu().numpy(), c2.cpu().numpy()
    assert np.array_equal(cnt, c2)
    assert_rows_equal(top, definition(pk, c2, 3))
    for i in range(3):
        want = oracle_top(phi_h[i], 32, 32, opts, 3)
        assert np.array_equal(_bits(top[i, :, :2]), _bits(want[:, :2])), (top[i], want)
        assert np.abs(top[i, :, 2] - want[:, 2]).max() <= 1e-9 * want[:, 2].max()
    with pytest.raises(ValueError):
        peak_search.batched_peak_search(phi, 32, 32, opts, top=3)


# ------------------------------------------------------------------ 6. estimate
def test_estimate_is_forward_then_peak_top(dev):
    Nb = Nd = 10
    y, b, s, _ = synth.make_batch(10, Nb, Nd, seed=41, snr_range=(10.0, 20.0))
    y, b, s = torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)
    torch.manual_seed(3)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, L=3, num_layers=4).eval()
    default_opts = {"xstep": 1 / (10 * Nd), "ystep": 1 / (10 * Nb), "iter": 3}      # main_for_net.py:112-116

    def check(out, phi_fwd, top, opts, device, top_n=None):
        tau, f, h, cnt, phi = out
        assert all(t.device == device for t in out)
        assert torch.equal(phi.cpu(), phi_fwd.cpu())
        rows, c = ops.peak_top(phi_fwd.to(dev), Nb, Nd, opts, top=top, top_n=top_n)
        assert torch.equal(cnt.cpu(), c.cpu()) and cnt.dtype == torch.int32
        assert_rows_equal(torch.stack([tau, f, h], dim=2).cpu().numpy(), rows.cpu().numpy())
        assert tau.shape == (phi.shape[0], top)

    phi_fwd = m(y.to(dev), b.to(dev), s.to(dev))
    check(m.estimate(y.to(dev), b.to(dev), s.to(dev)), phi_fwd, 3, default_opts, dev)       # the defaults
    opts = {"xstep": 1 / 30, "ystep": 1 / 30, "iter": 1}
    tn = torch.tensor([0, 1, 2, 3, 4, 5, 1, 2, 3, 0])
    check(m.estimate(y.to(dev), b.to(dev), s.to(dev), top=5, top_n=tn, opts=opts), phi_fwd, 5, opts, dev, tn)
    # CPU tensors in, CPU tensors out
    check(m.estimate(y, b, s), phi_fwd, 3, default_opts, torch.device("cpu"))
    # train mode: the same inference forward, no graph
    m.train()
    out = m.estimate(y.to(dev), b.to(dev), s.to(dev))
    assert m.training and not any(t.requires_grad for t in out) and all(t.grad_fn is None for t in out)
    check(out, phi_fwd, 3, default_opts, dev)
    m.eval()
    # sub_batch: each group's rows are those of a separate call on the group
    whole = m.estimate(y.to(dev), b.to(dev), s.to(dev))
    m.sub_batch = 4
    grouped = m.estimate(y.to(dev), b.to(dev), s.to(dev))
    m.sub_batch = None
    assert not torch.equal(grouped[4], whole[4])          # the groups' own batch means: a different phi
    for g0 in (0, 4, 8):
        sl = slice(g0, min(g0 + 4, 10))
        alone = m.estimate(y[sl].to(dev), b[sl].to(dev), s[sl].to(dev))
        for a, g in zip(alone, grouped):
            a, g = a.cpu(), g[sl].cpu()
            if a.dtype == torch.float64:
                assert_rows_equal(g.numpy(), a.numpy())
            else:
                assert torch.equal(g, a)


def test_admmnet_estimate_leaves_the_head_outputs_alone(dev):
    Nb, Nd = 4, 4
    y, b, s, _ = synth.make_batch(5, Nb, Nd, seed=2)
    y, b, s = (torch.from_numpy(t).to(dev) for t in (y, b, s))
    torch.manual_seed(4)
    m = A.ADMMNet(M=Nb, N=Nd, L=3, num_layers=3).eval()
    before = m(y, b, s)
    tau, f, h, cnt, phi = m.estimate(y, b, s)
    after = m(y, b, s)
    assert len(before) == 4 and all(torch.equal(p, q) for p, q in zip(before, after))
    assert torch.equal(phi, before[3]) and tau.shape == (5, 3) and int(cnt.min()) > 0
    opts = {"xstep": 1 / (10 * Nd), "ystep": 1 / (10 * Nb), "iter": 3}
    rows, c = ops.peak_top(before[3], Nb, Nd, opts, top=3)
    assert_rows_equal(torch.stack([tau, f, h], dim=2).cpu().numpy(), rows.cpu().numpy())
    assert torch.equal(c, cnt)


# ------------------------------------------------------------------ 7. contracts of the C entry point
def test_peak_top_entry_point_contracts(dev):
    lib = _lib.load()
    res, args = _lib.SYMBOLS["admmnet_peak_top_workspace_bytes"]
    assert len(args) == 4                                            # (xbase, ybase, nx, ny): no B to depend on
    Nb = Nd = 10
    opts = {"xstep": 1 / 40, "ystep": 1 / 40, "iter": 1}
    ax, ay = peak_search.coarse_axes(opts)
    nx, ny = len(ax), len(ay)
    need = lib.admmnet_peak_top_workspace_bytes(Nb, Nd, nx, ny)
    assert need == lib.admmnet_spectrum_workspace_bytes(Nb, Nd, nx, ny) > 0      # the two steering tables
    phi = forward_phi(dev, Nb, Nd, 300)
    tx, ty = torch.from_numpy(ax).to(dev), torch.from_numpy(ay).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    o7 = (ctypes.c_double * 7)(0, 1, opts["xstep"], -0.5, 0.5, opts["ystep"], 0.1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(B, L, tx=tx, nx=nx, ty=ty, ny=ny, ws=ws):
        top = torch.zeros(max(B, 1), max(L, 1), 3, dtype=torch.float64, device=dev)
        cnt = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
        rc = lib.admmnet_peak_top_f64(phi.data_ptr(), B, Nb, Nd, tx.data_ptr(), nx, ty.data_ptr(), ny, o7, 1, L, None,
                                      top.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        torch.cuda.synchronize()
        return rc, top, cnt

    # the same workspace, sized without B, serves 1 and 300 signals
    want, wcnt = ops.peak_top(phi, Nb, Nd, opts, top=3)
    for B in (1, 300):
        rc, top, cnt = call(B, 3)
        assert rc == 0
        assert_rows_equal(top.cpu().numpy(), want[:B].cpu().numpy())
        assert torch.equal(cnt, wcnt[:B])
    for L in (0, 65):
        rc, _, cnt = call(4, L)
        assert rc == -1 and int(cnt[0]) == -7                       # ADMMNET_E_ARG, nothing launched
    rc, top, cnt = call(0, 3)
    assert rc == 0 and int(cnt[0]) == -7 and not top.any()           # B = 0: OK, nothing written
    big = torch.linspace(0, 0.9, 200, dtype=torch.float64, device=dev)          # 200 x 200 doubles: 320 kB
    wsb = torch.empty(lib.admmnet_peak_top_workspace_bytes(Nb, Nd, 200, 200), dtype=torch.uint8, device=dev)
    rc, _, cnt = call(4, 3, tx=big, nx=200, ty=big, ny=200, ws=wsb)
    assert rc == -1 and int(cnt[0]) == -7
    assert b"does not fit the LDS" in lib.admmnet_last_error()
    with pytest.raises(_lib.AdmmNetError, match="does not fit the LDS"):
        ops.peak_top(phi, Nb, Nd, {"xstep": 1 / 201, "ystep": 1 / 201}, top=3)
    with pytest.raises(ValueError):
        ops.peak_top(phi, Nb, Nd, opts, top=0)
    with pytest.raises(ValueError):
        ops.peak_top(phi, Nb, Nd, opts, top=65)
    # empty axes: all-NaN rows and zero counts without a launch
    top, cnt = ops.peak_top(phi, Nb, Nd, {"xstep": 2.0, "ystep": 2.0}, top=3)
    assert top.shape == (300, 3, 3) and bool(torch.isnan(top).all()) and not cnt.any()


# ------------------------------------------------------------------ 8. full size
@pytest.mark.timeout(900)
def test_cfg5_full_batch_top_peaks(dev):
    """K = 32, 16 x 16, 65 536 signals, cfg5's search options, top = 3 (the setting of
    tests/test_gpu_tools.py::test_cfg5_full_batch_properties): the signals that test samples equal the oracle's
    literal search sorted and cut; the result for the reversed batch is the result reversed."""
    Nb = Nd = 16
    K, B = 32, 65536
    free, _total = torch.cuda.mem_get_info(dev)
    if free < 120e9:
        pytest.skip("needs ~100 GB of free HBM")
    opts = {"xstep": 1.0 / 65, "ystep": 1.0 / 32, "iter": 2}
    torch.manual_seed(0)
    m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=K).eval()
    ty, tb, ts, _ = synth.make_batch_device(B, Nb, Nd, seed=20260104, device=dev)
    tau, f, h, cnt, phi = m.estimate(ty, tb, ts, top=3, opts=opts, xbase=Nd, ybase=Nb)
    assert torch.isfinite(torch.view_as_real(phi)).all()
    idx = [0, 8191, 8192, 40000, 65535]
    ph = phi[idx].cpu().numpy()
    got = torch.stack([tau, f, h], dim=2)[idx].cpu().numpy()
    for i in range(len(idx)):
        want = oracle_top(ph[i], Nd, Nb, opts, 3)
        assert np.array_equal(_bits(got[i][:, :2]), _bits(want[:, :2])), (got[i], want)
        assert np.abs(got[i][:, 2] - want[:, 2]).max() <= 1e-9 * want[:, 2].max()
    rows, c = ops.peak_top(phi, Nd, Nb, opts, top=3)
    rows_r, c_r = ops.peak_top(phi.flip(0).contiguous(), Nd, Nb, opts, top=3)
    assert torch.equal(c_r.flip(0), c) and torch.equal(c, cnt)
    assert torch.equal(rows_r.flip(0).view(torch.int64), rows.view(torch.int64))
    assert torch.equal(rows.view(torch.int64), torch.stack([tau, f, h], dim=2).view(torch.int64))
