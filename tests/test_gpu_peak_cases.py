"""GPU (-m gpu): the device peak search (csrc/spectrum.hip, peaks.hip, estimate.hip, peak_core.h) on the designed spectra and
images of tests/peak_cases.py, against the literal oracle (oracle/peak_search_ref.py).

Positions (tau, f) are compared by bit pattern on every row of every case: tests/test_peak_cases_host.py shows that no decision
of any case is a numerical tie, so nothing is left out.  Heights follow test_gpu_parity.test_device_peak_search_matches_oracle:
within 1e-9 of the largest, and exactly 0.0 where the oracle's are.  The oracle's results are computed once per case
(peak_cases.oracle_of) and shared."""
import numpy as np
import pytest
import torch

import admm_net_amd as A
import peak_cases as P
from admm_net_amd import _lib, ops, peak_search, synth
from eigh_cases import DeviceGuard
from oracle import peak_search_ref as PO

pytestmark = pytest.mark.gpu
GUARD = DeviceGuard()
TOPS = (1, 3, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_rows_equal(got, want):
    """Exact: NaN by mask, everything else by bit pattern."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    mask = np.isnan(want)
    assert np.array_equal(np.isnan(got), mask)
    assert np.array_equal(_bits(got)[~mask], _bits(want)[~mask])


def assert_rows_match_oracle(got, want, what, exchangeable=()):
    """got, want [n, 3]: tau and f by bits, heights within 1e-9 of the largest and 0.0 exactly where the oracle's are.
    ``exchangeable``: ranks whose order is a numerical tie (peak_cases.ranking_ties): there a row may be its neighbour's,
    the same point up to the last bits of its coordinates."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not len(want):
        return
    for r in range(len(want)):
        ok = np.array_equal(_bits(got[r, :2]), _bits(want[r, :2]))
        if not ok and r in exchangeable:    # the pair is one point up to the last bits (asserted by the host test)
            ok = np.abs(got[r, :2] - want[r, :2]).max() < 1e-12
        assert ok, (what, r, got[:, :2], want[:, :2])
    assert np.abs(got[:, 2] - want[:, 2]).max() <= 1e-9 * want[:, 2].max(), what
    assert np.array_equal(got[:, 2] == 0.0, want[:, 2] == 0.0), what


def geometry(name):
    c = P.CASES[name]
    ax, ay = peak_search.coarse_axes(c["opts"])
    return c["xbase"], c["ybase"], c["opts"], len(ax) * len(ay)


_FULL = {}


def full_list(dev, name):
    """The device's untruncated list of a case, both seeds as one batch: (rows [2, cap, 3], counts [2]), computed once."""
    if name not in _FULL:
        xb, yb, opts, cap = geometry(name)
        phi = torch.from_numpy(P.batch_of(name)).to(dev)
        pk, cnt = GUARD.run(lambda: ops.peak_search(phi, xb, yb, opts, max_peaks=cap))
        assert pk.shape == (len(P.SEEDS), cap, 3) and pk.dtype == torch.float64 and cnt.dtype == torch.int32
        _FULL[name] = pk.cpu().numpy(), cnt.cpu().numpy()
    return _FULL[name]


# ---- 1. ops.peak_search -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_peak_search_equals_the_oracle(dev, name):
    pk, cnt = full_list(dev, name)
    for i, seed in enumerate(P.SEEDS):
        want = P.oracle_of(name, seed)[0]
        assert cnt[i] == want.shape[0], (name, seed, cnt[i], want.shape[0])
        assert_rows_match_oracle(pk[i, :cnt[i]], want, (name, seed))
        assert not pk[i, cnt[i]:].any()


# ---- 2. ops.peak_top --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_peak_top_equals_the_definition_and_the_oracle(dev, name):
    xb, yb, opts, cap = geometry(name)
    pk, cnt = full_list(dev, name)
    phi = torch.from_numpy(P.batch_of(name)).to(dev)
    for L in TOPS:
        for top_n in (None, np.array([2, 0]), np.array([1, 10 ** 6]), np.array([-3, L])):
            tn = None if top_n is None else torch.from_numpy(top_n)
            top, c = GUARD.run(lambda: ops.peak_top(phi, xb, yb, opts, top=L, top_n=tn))
            assert top.shape == (len(P.SEEDS), L, 3) and np.array_equal(c.cpu().numpy(), cnt)
            top = top.cpu().numpy()
            for i, seed in enumerate(P.SEEDS):
                Lb = L if top_n is None else min(max(int(top_n[i]), 0), L)
                mine = peak_search.top_rows(pk[i, :cnt[i]], Lb)
                assert_rows_equal(top[i, :len(mine)], mine)                      # the definition, on the device's own list
                assert np.isnan(top[i, len(mine):]).all()
                rows, tr = P.oracle_of(name, seed)
                assert_rows_match_oracle(top[i, :len(mine)], peak_search.top_rows(rows, Lb), (name, seed, L, top_n),
                                         exchangeable=P.ranking_ties(rows, tr.eps))


# ---- 3. ops.spectrum --------------------------------------------------------------------------------------------------------
def _grid_axes(nx, ny):
    return np.arange(nx) / max(nx, 2) + 0.003, -0.5 + np.arange(ny) / max(ny, 2)


def _odd_axes():
    """No arange: shuffled, negative, above 1, repeated points; 70 columns cross SP_XCHUNK."""
    rng = np.random.default_rng(8)
    taus = np.concatenate([[-0.7, -0.01, 0.0, 0.3, 0.3, 0.999, 1.0, 1.5, 2.25, 0.3], rng.uniform(-1.0, 2.0, 60)])
    fs = np.array([0.45, -0.5, -1.3, 0.45, 0.5, 0.0, 1.75])
    return rng.permutation(taus), fs


SPECTRUM_AXES = [(f"{nx}x{ny}", _grid_axes(nx, ny)) for nx in (1, 63, 64, 65, 128, 129) for ny in (1, 5)]
SPECTRUM_AXES.append(("odd_axes", _odd_axes()))
_RATIOS = {}


@pytest.mark.parametrize("axes", [a for _, a in SPECTRUM_AXES], ids=[n for n, _ in SPECTRUM_AXES])
def test_spectrum_equals_the_literal_double_loop(dev, axes, request):
    taus, fs = axes
    X, Y = np.meshgrid(taus, fs)
    worst_eps = worst_max = 0.0
    for name, c in P.CASES.items():
        xb, yb = c["xbase"], c["ybase"]
        phi = P.batch_of(name)
        Z = GUARD.run(lambda: ops.spectrum(torch.from_numpy(phi).to(dev), xb, yb, torch.from_numpy(taus), torch.from_numpy(fs)))
        assert Z.shape == (len(P.SEEDS), len(fs), len(taus)) and Z.dtype == torch.float64
        Z = Z.cpu().numpy()
        for i in range(len(P.SEEDS)):
            want = PO.peak_search(phi[i].astype(np.complex128), X, xb, Y, yb)
            err = np.abs(Z[i] - want).max()
            assert err <= 1e-10 * want.max(), (name, i, err, want.max())
            worst_eps = max(worst_eps, err / P.eps_of(phi[i], xb, yb))
            worst_max = max(worst_max, err / want.max())
            if xb == 1:
                assert np.array_equal(_bits(Z[i]), _bits(np.broadcast_to(Z[i][:, :1], Z[i].shape))), name
            if yb == 1:
                assert np.array_equal(_bits(Z[i]), _bits(np.broadcast_to(Z[i][:1, :], Z[i].shape))), name
    _RATIOS[request.node.callspec.id] = (worst_eps, worst_max)
    print(f"FIGURES spectrum {request.node.callspec.id}: worst |Z - oracle| = {worst_eps:.3g} eps = {worst_max:.3g} max Z;"
          f" so far {max(v[0] for v in _RATIOS.values()):.3g} eps, {max(v[1] for v in _RATIOS.values()):.3g} max Z")
    assert worst_eps < 1.0                                             # the tie rule's eps bounds the evaluation error


# ---- 4. ops.regional_maxima -------------------------------------------------------------------------------------------------
def test_regional_maxima_equal_the_flood_fill_on_the_designed_images(dev):
    by_shape = {}
    for n, im in P.images().items():
        by_shape.setdefault(im.shape, []).append(n)
    for shape, names in by_shape.items():
        Z = torch.from_numpy(np.stack([P.images()[n] for n in names])).to(dev)
        got = GUARD.run(lambda: ops.regional_maxima(Z)).cpu().numpy()
        assert got.shape == (len(names),) + shape and got.dtype == bool
        for g, n in zip(got, names):
            assert np.array_equal(g, P.image_mask(n)), (n, int(g.sum()), int(P.image_mask(n).sum()))


def test_regional_maxima_do_not_leak_between_batch_neighbours(dev):
    """The snake without and with its head, interleaved: 59 | 1 | 59 | 1 maxima and 5885 | 1 | 5885."""
    for a, b, order in (("snake_9x11", "snake_9x11_head", (0, 1, 0, 1, 1, 0)), ("snake_big", "snake_big_head", (0, 1, 0))):
        names = [(a, b)[k] for k in order]
        Z = torch.from_numpy(np.stack([P.images()[n] for n in names])).to(dev)
        got = GUARD.run(lambda: ops.regional_maxima(Z)).cpu().numpy()
        for g, n in zip(got, names):
            assert np.array_equal(g, P.image_mask(n)), (n, int(g.sum()))


def test_first_image_past_the_lds_is_refused_and_the_next_call_works(dev):
    Z = torch.from_numpy(np.stack([P.snake(*P.REFUSED, True)])).to(dev)
    with pytest.raises(_lib.AdmmNetError, match="does not fit the LDS"):
        ops.regional_maxima(Z)
    im = "snake_9x11_head"
    got = GUARD.run(lambda: ops.regional_maxima(torch.from_numpy(P.images()[im][None]).to(dev))).cpu().numpy()
    assert np.array_equal(got[0], P.image_mask(im))


# ---- 5. truncated lists -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in P.CASES if n != "tiny_1x1"])
def test_truncated_list_is_the_head_of_the_full_one(dev, name):
    xb, yb, opts, cap = geometry(name)
    pk, cnt = full_list(dev, name)
    assert cnt.min() >= 2                                              # (the host test pins the counts to the oracle's)
    phi = torch.from_numpy(P.batch_of(name)).to(dev)
    for max_peaks in sorted({1, max(1, int(cnt.min()) - 1)}):
        got, c = GUARD.run(lambda: ops.peak_search(phi, xb, yb, opts, max_peaks=max_peaks))
        assert got.shape == (len(P.SEEDS), max_peaks, 3)
        assert np.array_equal(c.cpu().numpy(), cnt) and (cnt > max_peaks).all()       # counts say the list was cut
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(pk[:, :max_peaks]))


# ---- 6. more maxima than EST_TILE -------------------------------------------------------------------------------------------
def test_many_maxima_case_passes_the_tile_of_the_estimator(dev):
    """More than 256 maxima on the oracle's side; top = 64 and top = 1 are part of test_peak_top_... above.  Here: the
    count, and that the 64 best of over 400 come from all four waves' lists and from beyond the first tile."""
    xb, yb, opts, cap = geometry("many_maxima")
    pk, cnt = full_list(dev, "many_maxima")
    for i, seed in enumerate(P.SEEDS):
        want = P.oracle_of("many_maxima", seed)[0]
        assert len(want) > 256 and cnt[i] == len(want)
        order = np.argsort(-want[:, 2], kind="stable")[:64]
        assert (order >= 256).any() and len(set(order % 4)) == 4
    phi = torch.from_numpy(P.batch_of("many_maxima")).to(dev)
    for L in (1, 64):
        top, c = GUARD.run(lambda: ops.peak_top(phi, xb, yb, opts, top=L))
        top = top.cpu().numpy()
        for i, seed in enumerate(P.SEEDS):
            assert_rows_equal(top[i], peak_search.top_rows(pk[i, :cnt[i]], L))
            assert_rows_match_oracle(top[i], peak_search.top_rows(P.oracle_of("many_maxima", seed)[0], L), (seed, L))


# ---- 7. batch position ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "base1_x", "xbase17"])
def test_results_do_not_depend_on_the_batch_position(dev, name):
    """B = 7 from 3 distinct signals repeated: copies bit-identical, B = 1 of each the same bits, the reversed batch the
    reversed result -- peak_search, peak_top and spectrum, every comparison of bits."""
    xb, yb, opts, cap = geometry(name)
    c = P.CASES[name]
    three = np.stack([P.phi_of(name, P.SEEDS[0]), P.phi_of(name, P.SEEDS[1]), P.make_phi(xb, yb, c["tones"], 3)])
    order = np.array([0, 1, 2, 0, 1, 2, 0])
    ax, ay = peak_search.coarse_axes(opts)
    tx, ty = torch.from_numpy(ax), torch.from_numpy(ay)

    def run(batch):
        phi = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
        pk, cnt = GUARD.run(lambda: ops.peak_search(phi, xb, yb, opts, max_peaks=cap))
        top, cnt2 = GUARD.run(lambda: ops.peak_top(phi, xb, yb, opts, top=3))
        Z = GUARD.run(lambda: ops.spectrum(phi, xb, yb, tx, ty))
        return [t.cpu().numpy() for t in (pk, cnt, top, cnt2, Z)]

    def same(a, b):
        for u, v in zip(a, b):
            if u.dtype == np.float64:
                assert_rows_equal(u, v)
            else:
                assert np.array_equal(u, v)

    seven = run(three[order])
    assert (seven[1] > 0).all()
    for pos, k in enumerate(order):
        same([t[pos] for t in seven], [t[int(np.flatnonzero(order == k)[0])] for t in seven])
    for k in range(3):
        same([t[0] for t in run(three[k:k + 1])], [t[k] for t in seven])
    same([t[::-1] for t in run(three[order][::-1])], seven)


# ---- 8. model.estimate on degenerate grids ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(1, 12), (2, 2)], ids=["1x12", "2x2"])
def test_estimate_on_a_degenerate_grid_equals_peak_top_of_its_phi(dev, geom):
    M, N = geom
    B = 5
    y, b, s, _ = synth.make_batch(B, M, N, seed=23, snr_range=(10.0, 20.0))
    torch.manual_seed(2)
    m = A.PhiEstADMMNet(M=M, N=N, num_layers=3).eval()
    tau, f, height, counts, phi = GUARD.run(
        lambda: m.estimate(torch.from_numpy(y).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), top=3))
    assert tau.shape == (B, 3) and phi.shape == (B, M * N) and torch.isfinite(torch.view_as_real(phi)).all()
    opts = {"xstep": 1 / (10 * N), "ystep": 1 / (10 * M), "iter": 3}         # estimate's documented defaults
    rows, cnt = GUARD.run(lambda: ops.peak_top(phi.to(dev), M, N, opts, top=3))
    rows = rows.cpu().numpy()
    assert np.array_equal(cnt.cpu().numpy(), counts.cpu().numpy()) and (cnt.cpu().numpy() > 0).all()
    assert_rows_equal(np.stack([tau.cpu().numpy(), f.cpu().numpy(), height.cpu().numpy()], axis=2), rows)
    assert np.isfinite(rows[:, 0]).all()
