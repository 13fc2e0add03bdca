"""GPU (-m gpu): scenes_kernel (csrc/synth.hip, behind admmnet_synth_scenes / synth.make_scenes_device) against its float64 host
mirror, against synth_kernel, and through the calls that consume a scene.

  * every case of tests/scene_checks.CASES against tests/scene_mirror.py: the float outputs through synth_checks.compare
    unchanged, snr_db / noise_var / ser to one spacing of their type plus 64 * 2^-53 of their magnitude, L_true and state exactly,
    nothing left out (tests/test_scene_mirror.py shows on the CPU that seven one-line mistakes fail this at these cases);
  * targets = (L, L), min_sep = 0 has the bits of make_batch_device, with and without labels;
  * on the device outputs: separation where state is 0, bit-zero padding, the same bits at B = 1, 7, 2500 and on a second call,
    labels on or off;
  * the scene's L_true / snr_db / noise_var feed metrics.crb and metrics.match_targets as they are;
  * the refusals of the C entry, with the outputs untouched; no synchronising call; harness.evaluate_snr(targets_min=, min_sep=).

Measured on the MI355X, over the twelve cases of the table: tau, f, C, b, y, sigma, phi and ser bit-equal to the cast mirror
(error / bound 0, no symbol and no scene left out); snr_db within 0.03 and noise_var within 0.14 of their bound (float64 outputs:
one spacing + 64 * 2^-53 of the magnitude); L_true and state equal.  The bounds from snr_db and from noise_var differ by 8.6e-8
at 4 x 6 and 1.4e-7 at 16 x 16 (allowed 9.0e-6 and 2.4e-5).  The file runs in under two seconds.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, harness, metrics, synth
import scene_checks as K
import scene_mirror as M

pytestmark = pytest.mark.gpu
SHARED = ("y", "b", "sigma", "tau", "f", "C")
EXTRAS = ("L_true", "snr_db", "noise_var", "ser", "state")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def mirror_of(name):
    return K.mirror_of(K.CASES[name])


def device_scenes(c, dev, labels=True, B=None):
    y, b, sigma, t = synth.make_scenes_device(c["B"] if B is None else B, c["Nb"], c["Nd"], targets=c["targets"], min_sep=c["min_sep"],
                                              seed=c["seed"], snr_range=c["snr_range"], snr_e=c["snr_e"], device=dev, labels=labels,
                                              rho=c["rho"], label_iters=c["label_iters"])
    return dict(y=y, b=b, sigma=sigma, **t)


def rows(out, samples):
    idx = torch.as_tensor(samples, device=out["y"].device)
    return {k: v[idx].cpu().numpy() for k, v in out.items()}


def bits(t):
    """The int32 view of a real or complex 4-byte tensor, the int64 view of an 8-byte one."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- 1. against the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_device_scenes_equal_the_float64_mirror(dev, name):
    c = K.CASES[name]
    rep = K.compare(rows(device_scenes(c, dev), c["samples"]), mirror_of(name))
    print("%s: %s" % (name, K.SC.describe(rep)))
    assert rep["left_out"] == 0 and rep["left_out_scenes"] == 0 and not rep["failures"], rep["failures"]


# ---- 2. against synth_kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("Nb,Nd,L,B", [(4, 6, 3, 16), (15, 17, 8, 4), (26, 131, 3, 2)])
def test_a_fixed_count_without_separation_has_the_bits_of_make_batch_device(dev, Nb, Nd, L, B, labels):
    kw = dict(seed=5, snr_range=(5.0, 25.0), device=dev, labels=labels, rho=2.0, label_iters=5)
    y0, b0, s0, t0 = synth.make_batch_device(B, Nb, Nd, L=L, **kw)
    for targets in ((L, L), L):
        y, b, s, t = synth.make_scenes_device(B, Nb, Nd, targets=targets, min_sep=0.0, **kw)
        assert same_bits(y, y0) and same_bits(b, b0) and same_bits(s, s0)
        for k in ("tau", "f", "C") + (("phi",) if labels else ()):
            assert same_bits(t[k], t0[k]), k
        assert ("phi" in t) == labels
        assert t["L_true"].dtype == torch.int64 and bool((t["L_true"] == L).all())
        assert t["state"].dtype == torch.int32 and not bool(t["state"].any())


# ---- 3. properties of the device outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4x6_2to3_sep2.5", "15x17_1to8_sep1.5", "1x12_1to3_sep1", "4x6_2to3_sep10"])
def test_separation_and_padding_on_the_float32_outputs(dev, name):
    """The float32 outputs are within 2^-24 relative of the float64 positions the kernel compared, so distances computed from
    them are held to min_sep (1 - 2^-20)."""
    c = K.CASES[name]
    out = {k: v.cpu().numpy() for k, v in device_scenes(c, dev, labels=False).items()}
    hi = c["targets"][1]
    closest = []
    for s in range(c["B"]):
        n = int(out["L_true"][s])
        assert c["targets"][0] <= n <= hi
        for k in ("tau", "f", "C"):
            assert out[k].shape == (c["B"], hi) and not out[k][s, n:].view(np.uint32).any(), (s, k)
        closest.append(M.pair_distances(out["tau"][s], out["f"][s], n, c["Nb"], c["Nd"]).min())
    closest, state = np.array(closest), out["state"]
    assert set(state.tolist()) <= {0, 1}
    assert (closest[state == 0] >= c["min_sep"] * (1.0 - 2.0 ** -20)).all()
    assert (closest[state == 1] < c["min_sep"]).all()
    assert np.array_equal(state, mirror_of(name)["state"])


def test_a_scene_does_not_depend_on_the_batch_or_the_call(dev):
    c = K.CASES["15x17_1to8_sep1.5"]
    big = device_scenes(c, dev, B=2500)
    for B in (1, 7, 2500):
        out = device_scenes(c, dev, B=B)
        for k in big:
            assert same_bits(out[k], big[k][:B]), (B, k)


@pytest.mark.parametrize("name", ["4x6_2to3_sep2.5", "26x131_2to3_sep8"])
def test_labels_do_not_change_the_scene(dev, name):
    c = K.CASES[name]
    with_l, without = device_scenes(c, dev, labels=True), device_scenes(c, dev, labels=False)
    assert "phi" in with_l and "phi" not in without
    for k in SHARED + EXTRAS:
        assert same_bits(with_l[k], without[k]), k


# ---- 4. downstream -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nb,Nd", [(4, 6), (16, 16)])
def test_the_bound_and_the_score_take_the_scene_as_it_is(dev, Nb, Nd):
    """crb from the drawn SNR recomputes the signal energy from the float32 tau, f, C; from noise_var it takes the float64 one.
    The bound is linear in the noise variance, so the two differ by the relative error of that energy: a phase error of
    2 pi max(Nb, Nd) 2^-24 per position and 2^-24 per amplitude, squared -- within 8 pi max(Nb, Nd) 2^-24."""
    B = 64
    y, b, sigma, t = synth.make_scenes_device(B, Nb, Nd, targets=(1, 3), min_sep=1.0, seed=5, device=dev)
    by_snr = metrics.crb(t["tau"], t["f"], t["C"], (Nb, Nd), snr_db=t["snr_db"], L_true=t["L_true"])
    by_var = metrics.crb(t["tau"], t["f"], t["C"], (Nb, Nd), noise_var=t["noise_var"], L_true=t["L_true"])
    assert by_snr.status.tolist() == [0, 0, 0] and by_var.status.tolist() == [0, 0, 0]
    a, v = by_snr.bound.cpu().numpy(), by_var.bound.cpu().numpy()
    live = np.arange(3)[None, :] < t["L_true"].cpu().numpy()[:, None]
    assert np.isfinite(a[live]).all() and np.isnan(a[~live]).all() and np.isnan(v[~live]).all()
    worst = float(np.abs(a[live] / v[live] - 1.0).max())
    print("%d x %d: bounds from snr_db and from noise_var differ by at most %.3g (allowed %.3g)"
          % (Nb, Nd, worst, 8 * math.pi * max(Nb, Nd) * 2.0 ** -24))
    assert worst <= 8 * math.pi * max(Nb, Nd) * 2.0 ** -24
    res = metrics.match_targets((t["tau"], t["f"]), t["tau"], t["f"], t["L_true"], n_est=t["L_true"], cutoff=1.0,
                                scale=(float(Nd), float(Nb)), period=(1.0, 1.0))
    assert res.status.tolist() == [0, 0]
    line = metrics.summary(res)
    assert line["hits"] == int(t["L_true"].sum()) and line["misses"] == 0 and line["false_alarms"] == 0


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.25
NAMES = ("y", "b", "sigma", "tau", "f", "C", "phi", "L_true", "snr_db", "noise_var", "ser", "state")
REFUSALS = {"L_min_0": dict(L_min=0), "L_max_9": dict(L_max=9), "L_min_above_L_max": dict(L_min=3, L_max=2),
            "min_sep_negative": dict(min_sep=-0.5), "min_sep_nan": dict(min_sep=float("nan")), "min_sep_inf": dict(min_sep=float("inf")),
            "label_iters_negative": dict(label_iters=-1), "B_0": dict(B=0), "B_2^31": dict(B=2 ** 31),
            "D_above_the_bound": dict(Nb=K.SC.OVER_D_GRID[0], Nd=K.SC.OVER_D_GRID[1]),
            **{"null_" + k: dict(null=k) for k in NAMES if k != "phi"}}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_entry_point_refuses_before_launching(dev, name):
    """ADMMNET_E_ARG with a message on the host; outputs pre-filled with a sentinel keep it."""
    a = dict(B=2, Nb=4, Nd=6, L_min=1, L_max=3, min_sep=1.0, label_iters=5, null=None)
    a.update(REFUSALS[name])
    n, D, hi = 2, a["Nb"] * a["Nd"], min(max(a["L_max"], 1), 8)
    fill = {torch.complex64: complex(SENTINEL, SENTINEL), torch.int64: int(SENTINEL), torch.int32: int(SENTINEL)}
    full = lambda dtype, *s: torch.full(s, fill.get(dtype, SENTINEL), dtype=dtype, device=dev)  # noqa: E731
    bufs = dict(y=full(torch.complex64, n, D), b=full(torch.complex64, n, D), sigma=full(torch.float32, n),
                tau=full(torch.float32, n, hi), f=full(torch.float32, n, hi), C=full(torch.complex64, n, hi),
                phi=full(torch.complex64, n, D), L_true=full(torch.int64, n), snr_db=full(torch.float64, n),
                noise_var=full(torch.float64, n), ser=full(torch.float32, n), state=full(torch.int32, n))
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ptrs = [ctypes.c_void_p(0 if k == a["null"] else bufs[k].data_ptr()) for k in NAMES]
        rc = lib.admmnet_synth_scenes(a["B"], a["Nb"], a["Nd"], a["L_min"], a["L_max"], a["min_sep"], 5, 5.0, 25.0, 7.0, 1.0,
                                      a["label_iters"], *ptrs, stream)
        assert rc == -1                                                         # ADMMNET_E_ARG
        with pytest.raises(_lib.AdmmNetError, match="synth_scenes"):
            _lib.check(rc, "admmnet_synth_scenes")
        torch.cuda.synchronize(dev)
    for k, t in bufs.items():
        want = fill.get(t.dtype, SENTINEL)
        assert bool((torch.view_as_real(t) if t.is_complex() else t).eq(SENTINEL if t.is_complex() else want).all()), k


def test_a_null_label_pointer_is_accepted_and_python_refuses_a_bad_range(dev):
    y, b, sigma, t = synth.make_scenes_device(2, 4, 6, targets=2, device=dev)
    assert "phi" not in t and t["tau"].shape == (2, 2)
    for bad in ((0, 3), (2, 9), (3, 2)):
        with pytest.raises(ValueError):
            synth.make_scenes_device(2, 4, 6, targets=bad, device=dev)
    with pytest.raises(_lib.AdmmNetError):
        synth.make_scenes_device(2, 4, 6, min_sep=-1.0, device=dev)


# ---- 6. no host read ---------------------------------------------------------------------------------------------------------------
def test_no_synchronising_call(dev):
    synth.make_scenes_device(4, 4, 6, device=dev)                                # (the library is loaded, the first call made)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, b, sigma, t = synth.make_scenes_device(64, 4, 6, targets=(1, 3), min_sep=2.0, seed=5, device=dev, labels=True)
        counts = metrics.order_counts(torch.full_like(t["L_true"], 2, dtype=torch.int32), t["L_true"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    L = t["L_true"].cpu().numpy()
    assert counts.is_cuda and counts.dtype == torch.int64
    assert counts.tolist() == [int((2 < L).sum()), int((2 == L).sum()), int((2 > L).sum())] and min(counts.tolist()) > 0


# ---- 7. harness.evaluate_snr ---------------------------------------------------------------------------------------------------------
KW = dict(grid=(4, 6), layers=2, snrs=(25.0,), signals=64, targets=3, baseline="classical", device="cuda:0", crb=True,
          refine="given", order=6)
METHODS = ["net", "net+refine", "net+order", "classical", "classical+refine", "classical+order"]
NEW_KEYS = {"targets_min", "min_sep", "unseparated", "ser"}
ORDER_KEYS = {"order_under", "order_exact", "order_over"}


@pytest.fixture(scope="module")
def plain():
    return list(harness.evaluate_snr(**KW))


def test_evaluate_snr_given_the_defaults_explicitly(plain):
    lines = list(harness.evaluate_snr(**KW, targets_min=3, min_sep=0.0))
    assert [l["method"] for l in lines] == [l["method"] for l in plain] == METHODS
    for line, old in zip(lines, plain):
        assert {k: line[k] for k in old} == old                                # bit-equal: the same numbers
        assert set(line) - set(old) == NEW_KEYS | (ORDER_KEYS if line["method"].endswith("+order") else set())
        assert line["targets_min"] == 3 and line["min_sep"] == 0.0 and line["unseparated"] == 0 and 0.0 < line["ser"] < 100.0
    assert all(not (NEW_KEYS | ORDER_KEYS) & set(l) for l in plain)


@pytest.mark.parametrize("min_sep", [0.0, 1.5])
def test_evaluate_snr_with_a_varying_count(plain, min_sep):
    lines = list(harness.evaluate_snr(**KW, targets_min=1, min_sep=min_sep))
    assert [l["method"] for l in lines] == METHODS
    _, _, _, truth = synth.make_scenes_device(64, 4, 6, targets=(1, 3), min_sep=min_sep, seed=20260104, snr_range=(25.0, 25.0),
                                              device="cuda:0")
    total = int(truth["L_true"].sum())
    assert 64 < total < 192
    for line in lines:
        print(line)
        assert set(line) == set(plain[0]) | NEW_KEYS | (ORDER_KEYS if line["method"].endswith("+order") else set())
        assert line["targets_min"] == 1 and line["min_sep"] == min_sep and line["signals"] == 64
        assert line["hits"] + line["misses"] == total and line["unseparated"] == int(truth["state"].sum())
        assert line["ser"] == pytest.approx(float(truth["ser"].double().mean()), rel=1e-6)
        if line["method"].endswith("+order"):
            assert line["order_under"] + line["order_exact"] + line["order_over"] == 1
            assert min(line[k] for k in ORDER_KEYS) >= 0
        else:                                                                   # given the count: never more rows than targets
            assert line["hits"] + line["false_alarms"] <= total
    if min_sep == 0.0:
        assert lines[0]["unseparated"] == 0


def test_evaluate_snr_refuses_a_count_outside_the_range():
    for bad in (0, 4, 1.5, True):
        with pytest.raises(ValueError):
            list(harness.evaluate_snr(**KW, targets_min=bad))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            list(harness.evaluate_snr(**KW, min_sep=bad))
