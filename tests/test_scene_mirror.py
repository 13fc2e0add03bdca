"""CPU: the float64 mirror of the scene generator with a varying number of targets (tests/scene_mirror.py) and the comparison the
device is held to (tests/scene_checks.py), without a GPU.

  * with the count fixed and no separation the mirror IS synth_mirror.SynthMirror, on every key;
  * the count is uniform on lo .. hi (20 000 scenes);
  * separation holds where the state says so and does not where it says not; zeros past the count; ser counts dd != data;
  * what the cases of the device test exercise: redraws up to the last attempt, both states, every count, the margins;
  * seven copies of the mirror with one mistake each fail the comparison at named cases;
  * the Python surface that needs no device: the target range, order_counts, the symbol table, the new parameters.
"""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, harness, metrics, synth
import scene_checks as K
import scene_mirror as M
import synth_mirror as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirrors():
    return {name: K.mirror_of(c) for name, c in K.CASES.items()}


@pytest.mark.parametrize("Nb,Nd,L", [(4, 6, 3), (3, 7, 8), (1, 1, 1)])
def test_fixed_count_without_separation_is_the_batch_mirror(Nb, Nd, L):
    samples = [0, 1, 5, 65536]
    want = SM.SynthMirror().run(samples, Nb, Nd, L, 5, rho=2.0)
    for targets in (L, (L, L)):
        got = M.SceneMirror().run(samples, Nb, Nd, targets, 5, rho=2.0, min_sep=0.0)
        for k, v in want.items():
            assert np.array_equal(got[k], v), k
        assert (got["L_true"] == L).all() and not got["state"].any() and np.isinf(got["sep_margin"]).all()


def test_the_count_is_uniform():
    """2 x 2, (1, 4), seed 5, samples 0 .. 19999: each count within 4 standard deviations of 5000."""
    n = M.SceneMirror().counts(np.arange(20000), 1, 4, 5)
    counts = np.bincount(n, minlength=5)
    print("counts", counts[1:])
    assert counts[0] == 0 and counts.sum() == 20000 and counts[1:].tolist() == [5083, 4957, 4996, 4964]
    sd = math.sqrt(20000 * 0.25 * 0.75)
    assert (np.abs(counts[1:] - 5000) <= 4 * sd).all()
    assert (M.SceneMirror().counts(np.arange(64), 3, 3, 5) == 3).all()


def test_separation_padding_and_symbol_errors(mirrors):
    for name, r in mirrors.items():
        c = K.CASES[name]
        for s in range(len(c["samples"])):
            n = int(r["L_true"][s])
            assert c["targets"][0] <= n <= c["targets"][1]
            d = M.pair_distances(r["tau"][s], r["f"][s], n, c["Nb"], c["Nd"])
            assert (d.min() >= c["min_sep"]) == (r["state"][s] == 0), (name, s, d.min())
            for k in ("tau", "f", "C"):
                assert not r[k][s, n:].any() and (r[k][s, :n] != 0).all(), (name, s, k)
            assert (r["attempt"][s, :n] >= 0).all() and (r["attempt"][s, n:] == -1).all()
        assert np.array_equal(r["ser"], 100.0 * (r["dd"] != r["data"]).sum(axis=1) / (c["Nb"] * c["Nd"]))
        assert np.array_equal(r["noise_var"], r["w_std"][:, 0] ** 2) and np.array_equal(r["snr_db"], r["snr"][:, 0])
        assert (r["ser"] > 0).any() or c["Nb"] * c["Nd"] < 12          # (a few symbols at 7 dB: often none wrong)
        # C is the draw of (stream C, pair l) whatever the attempt
        raw = SM.SynthMirror().run(c["samples"], 1, 1, c["targets"][1], c["seed"])["C"]
        assert np.array_equal(r["C"], M.SceneMirror().pad(raw, r["L_true"]))


def test_what_the_cases_exercise(mirrors):
    r = mirrors["4x6_1to3_sep2"]
    assert np.bincount(r["L_true"], minlength=4)[1:].tolist() == [7, 5, 4] and not r["state"].any()
    assert r["attempt"].max() == 23 and (r["attempt"] > 0).sum() >= 6
    assert 1.0e-3 < r["sep_margin"].min() < 1.2e-3
    r = mirrors["4x6_2to3_sep2.5"]
    assert r["state"].sum() == 5 and (r["attempt"] == M.ATTEMPTS).sum() == 6                # all 32 attempts refused
    assert np.array_equal((r["attempt"] == M.ATTEMPTS).any(axis=1), r["state"] == 1)
    assert 3.2e-4 < r["sep_margin"].min() < 3.4e-4
    assert mirrors["6x4_2to3_sep2"]["state"].sum() == 1
    r = mirrors["15x17_1to8_sep1.5"]
    assert (np.bincount(r["L_true"], minlength=9)[1:] > 0).all() and not r["state"].any()
    assert 0.08 < (r["attempt"] > 0).sum() / (r["attempt"] >= 0).sum() < 0.12
    assert 3.2e-3 < r["sep_margin"].min() < 3.4e-3
    assert mirrors["4x6_2to3_sep10"]["state"].all()
    assert not mirrors["1x12_1to3_sep1"]["state"].any() and (mirrors["1x12_1to3_sep1"]["attempt"] > 0).any()
    assert mirrors["26x131_2to3_sep8"]["phi"].shape == (2, K.SC.MAX_D)


def test_cases_are_clean_and_the_mirror_passes_its_own_comparison(mirrors):
    """No placement was decided closer than 3.3e-4 (relative) and no symbol closer than 1e-6 to its boundary, so the comparison
    leaves nothing out: the cap on scenes and symbols left out is 0."""
    assert min(r["sep_margin"].min() for r in mirrors.values()) >= 3.3e-4
    for name, r in mirrors.items():
        assert r["margin"].min() >= 1e-6, name
        rep = K.compare(K.cast_outputs(r), r)
        assert rep["left_out"] == 0 and rep["left_out_scenes"] == 0 and not rep["failures"], (name, rep["failures"])
        assert all(v == 0.0 for v in rep["share"].values())


def test_compare_notices_wrong_integers_and_scalars(mirrors):
    r = mirrors["4x6_1to3_sep2"]
    for key, change in (("L_true", lambda v: v + (np.arange(v.size) == 3)), ("state", lambda v: 1 - v),
                        ("ser", lambda v: v + np.float32(100.0 / 24)), ("snr_db", lambda v: v * (1 + 1e-13)),
                        ("noise_var", lambda v: v.astype(np.float32).astype(np.float64))):
        got = K.cast_outputs(r)
        got[key] = change(got[key]).astype(got[key].dtype)
        rep = K.compare(got, r)
        assert len(rep["failures"]) == 1 and rep["failures"][0].startswith(key), (key, rep["failures"])


# ---- copies of the mirror with one mistake each ------------------------------------------------------------------------------------
class CountWithoutTheTop(M.SceneMirror):
    def count(self, u, lo, hi):
        return lo + np.minimum(hi - lo, np.floor(u * (hi - lo)).astype(np.int64))


class AttemptsPerTarget(M.SceneMirror):
    def attempt_index(self, l, t):
        return l * M.ATTEMPTS + t


class NoWrap(M.SceneMirror):
    def wrap(self, d):
        return d


class AxesExchanged(M.SceneMirror):
    def distance2(self, dtau, df, Nb, Nd):
        return (Nb * self.wrap(dtau)) ** 2 + (Nd * self.wrap(df)) ** 2


class RejectedAttemptKept(M.SceneMirror):
    def stops(self, accepted):
        return True


class PaddingLeftAtTheDraw(M.SceneMirror):
    def pad(self, values, n):
        return values


class NoiseVarIsTheDeviation(M.SceneMirror):
    def noise_variance(self, w_std):
        return w_std


# mistake -> (cases at which it must fail, cases at which it cannot show)
MISTAKES = {
    CountWithoutTheTop: (["4x6_1to3_sep2", "15x17_1to8_sep1.5", "grid_2x2_B70000"], ["1x1_1to1_sep0.5"]),
    AttemptsPerTarget: (["4x6_1to3_sep2", "4x6_2to3_sep2.5", "15x17_1to8_sep1.5"], ["1x1_1to1_sep0.5"]),
    # (tau and f span 0.8 of their period: the wrap shows only where min_sep exceeds 0.2 Nd or 0.2 Nb cells)
    NoWrap: (["4x6_1to3_sep2", "4x6_2to3_sep2.5", "6x4_2to3_sep2"], ["15x17_1to8_sep1.5", "1x12_1to3_sep1"]),
    AxesExchanged: (["4x6_1to3_sep2", "6x4_2to3_sep2", "1x12_1to3_sep1"], ["1x1_1to1_sep0.5"]),
    RejectedAttemptKept: (["4x6_1to3_sep2", "4x6_2to3_sep10", "1x12_1to3_sep1"], ["1x1_1to1_sep0.5", "26x131_2to3_sep8"]),
    PaddingLeftAtTheDraw: (["4x6_1to3_sep2", "15x17_1to8_sep1.5"], ["1x1_1to1_sep0.5"]),
    NoiseVarIsTheDeviation: (["4x6_1to3_sep2", "1x1_1to1_sep0.5", "26x131_2to3_sep8"], []),
}


@pytest.mark.parametrize("mistake", list(MISTAKES), ids=lambda m: m.__name__)
def test_the_comparison_notices_one_mistake(mirrors, mistake):
    fails, blind = MISTAKES[mistake]
    for name in fails + blind:
        wrong = K.mirror_of(K.CASES[name], mistake)
        rep = K.compare(K.cast_outputs(wrong), mirrors[name])
        print("%s at %s: %s" % (mistake.__name__, name, rep["failures"] or "passes"))
        assert bool(rep["failures"]) == (name in fails), (mistake.__name__, name, rep["failures"])


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_target_range():
    assert synth._target_range(3) == (3, 3) and synth._target_range((1, 8)) == (1, 8) and synth._target_range([2, 2]) == (2, 2)
    for bad in (0, 9, (0, 3), (3, 2), (1, 9), (1, 2, 3), 2.5, (1.5, 3), True, "3", None):
        with pytest.raises(ValueError):
            synth._target_range(bad)


def test_order_counts_on_the_host():
    n_sel = torch.tensor([1, 2, 3, 3, 0, 5], dtype=torch.int32)
    L_true = torch.tensor([2, 2, 2, 3, 1, 1], dtype=torch.int64)
    got = metrics.order_counts(n_sel, L_true)
    assert got.dtype == torch.int64 and got.tolist() == [2, 2, 2]
    with pytest.raises(ValueError):
        metrics.order_counts(n_sel.float(), L_true)
    with pytest.raises(ValueError):
        metrics.order_counts(n_sel[:3], L_true)
    assert "bincount" not in inspect.getsource(metrics.order_counts)


def test_symbols_and_signatures():
    c = ctypes
    res, args = _lib.SYMBOLS["admmnet_synth_scenes"]
    assert res is c.c_int32 and args == [c.c_int64, c.c_int32, c.c_int32, c.c_int32, c.c_int32, c.c_double, c.c_uint64,
                                         c.c_double, c.c_double, c.c_double, c.c_double, c.c_int32] + [c.c_void_p] * 13
    hdr = open(os.path.join(ROOT, "include", "admmnet.h")).read()
    assert hdr.count("admmnet_synth_scenes(") == 1 and "#define ADMMNET_ABI_VERSION 1" in hdr
    assert str(inspect.signature(synth.make_scenes_device)) == (
        "(batch, Nb, Nd, targets=(1, 3), min_sep=0.0, seed=20260104, snr_range=(5.0, 25.0), snr_e=7.0, device=None, labels=False, "
        "rho=1.0, label_iters=5)")
    assert str(inspect.signature(metrics.order_counts)) == "(n_sel, L_true) -> 'torch.Tensor'"
    p = inspect.signature(harness.evaluate_snr).parameters
    assert list(p)[-5:] == ["targets_min", "min_sep", "order", "refine", "crb"]
    assert p["targets_min"].default is None and p["min_sep"].default == 0.0


def test_evaluate_command_parses_the_new_flags():
    for argv in (["evaluate", "--targets-min", "one"], ["evaluate", "--min-sep", "wide"]):
        with pytest.raises(SystemExit):
            harness.main(argv)
