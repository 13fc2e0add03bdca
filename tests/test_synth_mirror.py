"""CPU: the float64 mirror of the device generator (tests/synth_mirror.py) and the comparison the device is held to
(tests/synth_checks.py), without a GPU.

  * known answers of splitmix64;
  * the mirror's raw draws pushed through the host recipe the rest of the suite uses (admm_net_amd.synth) give the mirror's
    psi, b, e, y, sigma;
  * the mirror's labels equal the literal classical solver, the product's host solver and the dense recursion, at non-square
    grids and rho != 1;
  * the generator's distributions and the independence of its streams (the device inherits them through
    tests/test_gpu_synth.py, which pins it to the mirror element by element);
  * no symbol of any device case lies near a decision boundary, so the comparison leaves none out;
  * twelve copies of the mirror with one mistake each fail the comparison at the device test's cases.
"""
import contextlib
import io
import math

import numpy as np
import pytest
from scipy.special import ndtr

from admm_net_amd import classical, synth
from oracle import classical_ref as CO
import synth_checks as SC
import synth_mirror as SM


def test_splitmix64_known_answers():
    """The first two outputs of splitmix64 from state 0."""
    assert int(SM.sy_mix(0)) == 0xE220A8397B1DCDAF
    assert int(SM.sy_mix(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert int(SM.sy_mix(2 ** 64 - 1)) == int(SM.sy_mix(np.uint64(2 ** 64 - 1)))            # wraps, no overflow error
    m = SM.SynthMirror()
    assert np.array_equal(m.bits(-1, [0, 7], SM.TAU, [0, 1]), m.bits(2 ** 64 - 1, [0, 7], SM.TAU, [0, 1]))
    u = SM.uniform(np.array([0, 2 ** 64 - 1], dtype=np.uint64))
    # never 0 (ln u is finite); the largest draw, 2^53 - 1/2, rounds to 2^53 in float64 and gives exactly 1 (harmless:
    # ln 1 = 0, and tau = 0.9, f = 0.4 stay in range)
    assert u[0] == 2.0 ** -54 and u[1] == 1.0


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("Nb,Nd,L,seed", [(8, 16, 3, 5), (4, 6, 3, 5), (6, 4, 2, 9), (3, 7, 8, 2 ** 63 + 12345)])
def test_raw_draws_through_the_host_recipe_give_the_mirror_scene(Nb, Nd, L, seed):
    """synth.make_batch's lines with the mirror's draws in place of numpy's generator."""
    B, D = 6, Nb * Nd
    r = SM.mirror(np.arange(B), Nb, Nd, L, seed, snr_range=(5.0, 25.0), snr_e=7.0)
    S, Dm = synth.steering(r["f"], Nb), synth.steering(r["tau"], Nd)
    psi = np.einsum("bl,bli,blj->bij", r["C"], S, np.conj(Dm)).reshape(B, D)
    sig = synth.pskmod(r["data"], 4, np.pi / 4)
    p_sig = np.mean(np.abs(sig) ** 2, axis=1, keepdims=True)
    p_noise = p_sig / (10 ** (7.0 / 10))
    sig_n = sig + np.sqrt(p_noise / 2) * (r["demod_normals"].real + 1j * r["demod_normals"].imag)
    dd = synth.pskdemod(sig_n, 4, np.pi / 4)
    b = synth.pskmod(dd, 4, np.pi / 4)
    e = sig - b
    real_y = (b + e) * psi
    w = np.sqrt(0.5) * (r["noise_normals"].real + 1j * r["noise_normals"].imag)
    w_var = np.sum(np.abs(real_y) ** 2, axis=1, keepdims=True) / (10 ** (r["snr"] / 10) * D)
    y = real_y + np.sqrt(w_var) * w
    sigma = np.linalg.norm(e / b, axis=1) + 1.0
    assert np.array_equal(dd, r["dd"])
    for name, val in (("psi", psi), ("b", b), ("y", y), ("sigma", sigma), ("real_y", real_y)):
        assert rel(val, r[name]) <= 1e-12, name
    assert np.abs(e - r["e"]).max() <= 1e-12                  # (e is exactly 0 where the symbol was decided correctly)
    assert (r["tau"] > 0.1).all() and (r["tau"] < 0.9).all() and (np.abs(r["f"]) < 0.4).all()
    assert (r["snr"] >= 5.0).all() and (r["snr"] <= 25.0).all()


OPTS = {"eta_abs": 1e-7, "eta_rel": 1e-7, "max_iter": 100}


@pytest.mark.parametrize("rho", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("Nb,Nd", [(4, 6), (6, 4), (10, 10)])
def test_labels_equal_the_classical_solver_and_the_dense_recursion(Nb, Nd, rho):
    """phi on the float32-cast scene (what a caller of the classical solver would hold) = admm_for_us as written."""
    r = SM.mirror([0, 3], Nb, Nd, 3, 11, rho=rho)
    y, b = r["y"].astype(np.complex64).astype(np.complex128), r["b"].astype(np.complex64).astype(np.complex128)
    sigma = r["sigma"].astype(np.float32)
    phi5 = SM.label_recursion(y, b, rho, 5)
    for i in range(2 if Nb * Nd < 100 else 1):
        want, it = CO.admm_for_us_literal(y[i], b[i], Nd, Nb, 1, float(sigma[i]), dict(OPTS, rho=rho))
        assert it == 5 and rel(phi5[i], want) <= 1e-9
        with contextlib.redirect_stdout(io.StringIO()):
            prod, it = classical.admm_for_us(y[i], b[i], Nd, Nb, 1, float(sigma[i]), dict(OPTS, rho=rho))
        assert it == 5 and rel(phi5[i], prod) <= 1e-9
        for iters in (0, 1, 5, 12):
            W = np.linalg.inv(np.diag(1.0 / np.abs(b[i]) ** 2) + rho * np.ones((Nb * Nd, Nb * Nd)))
            dense = np.zeros(Nb * Nd, dtype=complex)
            for _ in range(iters):
                dense = W @ (y[i] / b[i] + rho * dense)
            got = SM.label_recursion(y[i:i + 1], b[i:i + 1], rho, iters)[0]
            if iters == 0:
                assert not got.any()
            else:
                assert rel(got, dense) <= 1e-10, iters
    # the float32 oracle-style figure: labels of the complex64-cast scene, held to the bound the device is held to
    rep = SC.compare(dict(SC.cast_outputs(r), phi=phi5.astype(np.complex64)), r)
    print("labels of the complex64-cast scene, %d x %d rho %g: error/bound %.3g, not bit-equal %.3g"
          % (Nb, Nd, rho, rep["ratio"]["phi"], rep["share"]["phi"]))
    assert rep["share"]["phi"] > SC.SHARE_CAP                  # a float32 scene behind the labels does not pass


# ---- distributions ---------------------------------------------------------------------------------------------------
def kolmogorov(x, cdf):
    """sqrt(n) D_n."""
    x = np.sort(np.ravel(x))
    n = x.size
    F = cdf(x)
    return math.sqrt(n) * max(float((np.arange(1, n + 1) / n - F).max()), float((F - np.arange(n) / n).max()))


def corr(a, b):
    return float(np.corrcoef(np.ravel(a), np.ravel(b))[0, 1])


@pytest.fixture(scope="module")
def targets():
    return SM.mirror(np.arange(2048), 1, 1, 8, 20261019)       # 16 384 draws each of tau, f, Re C, Im C


@pytest.fixture(scope="module")
def scene():
    return SM.mirror(np.arange(256), 16, 16, 3, 20261020, snr_range=(5.0, 25.0))      # 65 536 symbols


def test_target_parameters_follow_their_distributions(targets):
    t = targets
    assert t["tau"].size >= 16000
    assert kolmogorov(t["tau"], lambda x: (x - 0.1) / 0.8) < 2.3
    assert kolmogorov(t["f"], lambda x: (x + 0.4) / 0.8) < 2.3
    assert kolmogorov(t["C"].real, lambda x: ndtr(x / 0.7)) < 2.3
    assert kolmogorov(t["C"].imag, lambda x: ndtr(x / 0.7)) < 2.3
    assert abs(corr(t["C"].real, t["C"].imag)) < 4.5 / math.sqrt(t["C"].size)
    assert abs(corr(t["tau"], t["f"])) < 4.5 / math.sqrt(t["tau"].size)


def test_symbols_and_symbol_errors(scene):
    n = scene["data"].size
    for v in range(4):
        assert abs((scene["data"] == v).mean() - 0.25) < 4.5 * math.sqrt(0.25 * 0.75 / n), v
    Q = 1.0 - ndtr(math.sqrt(10 ** 0.7))
    p = 2 * Q - Q * Q
    ser = (scene["dd"] != scene["data"]).mean()
    print("symbol-error share %.4f over %d symbols, theory %.4f" % (ser, n, p))
    assert abs(ser - p) < 4.5 * math.sqrt(p * (1 - p) / n)
    assert kolmogorov(scene["demod_normals"].real, ndtr) < 2.3 and kolmogorov(scene["noise_normals"].imag, ndtr) < 2.3


def test_realised_noise_power_is_the_snr_draw(scene):
    """sum |noise|^2 = w_std^2 sum |w|^2 with |w|^2 exponential (mean 1, variance 1): relative spread 1 / sqrt(D) per
    sample, 1 / sqrt(B D) pooled -- a noise power wrong by a few percent fails the pooled bound (1.8 %)."""
    B, D = scene["y"].shape
    signal = (np.abs(scene["real_y"]) ** 2).sum(axis=1)
    noise = (np.abs(scene["y"] - scene["real_y"]) ** 2).sum(axis=1)
    ratio = noise * 10 ** (scene["snr"][:, 0] / 10) / signal        # realised / nominal noise power
    print("realised / nominal noise power: per sample %.3f .. %.3f, pooled %.4f" % (ratio.min(), ratio.max(), ratio.mean()))
    assert np.abs(ratio - 1.0).max() < 4.5 / math.sqrt(D)
    assert abs(ratio.mean() - 1.0) < 4.5 / math.sqrt(B * D)
    assert kolmogorov(scene["snr"], lambda x: (x - 5.0) / 20.0) < 2.3


def test_streams_samples_and_seeds_are_uncorrelated(scene):
    n = scene["noise_normals"].size
    lim = 4.5 / math.sqrt(n)
    nz, dz = scene["noise_normals"], scene["demod_normals"]
    assert abs(corr(nz.real, nz.imag)) < lim and abs(corr(dz.real, dz.imag)) < lim      # the two normals of a pair
    for a in (nz.real, nz.imag):
        for b in (dz.real, dz.imag):
            assert abs(corr(a, b)) < lim                                                  # demodulation / channel noise
    lim1 = 4.5 / math.sqrt(nz[1:].size)
    assert abs(corr(nz[:-1].real, nz[1:].real)) < lim1 and abs(corr(nz[:-1].imag, nz[1:].imag)) < lim1   # sample s / s + 1
    assert abs(corr(nz[:, :-1].real, nz[:, 1:].real)) < lim                               # index i / i + 1
    other = SM.mirror(np.arange(256), 16, 16, 3, 20261021, snr_range=(5.0, 25.0))         # seed + 1
    assert abs(corr(nz.real, other["noise_normals"].real)) < lim
    assert abs(corr(scene["data"], other["data"])) < lim
    assert abs(corr(scene["snr"], other["snr"])) < 4.5 / math.sqrt(256)


# ---- the device cases ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mirrors():
    return {name: SC.mirror_of(c) for name, c in SC.CASES.items()}


def test_device_cases_are_clean_and_the_mirror_passes_its_own_comparison(mirrors):
    """Smallest margin >= 1e-6 on every case, so compare() leaves out no symbol there."""
    assert SC.MAX_D_GRID[0] * SC.MAX_D_GRID[1] == SC.MAX_D
    assert 48 * SC.MAX_D + 352 <= 160 * 1024 < 48 * (SC.MAX_D + 1) + 352
    for name, r in mirrors.items():
        assert r["margin"].min() >= 1e-6, (name, r["margin"].min())
        rep = SC.compare(SC.cast_outputs(r), r)
        assert rep["left_out"] == 0 and not rep["failures"], (name, rep)
        assert all(v == 0.0 for v in rep["share"].values())


def test_compare_leaves_out_and_counts_symbols_on_a_boundary(mirrors):
    r = dict(mirrors["4x6_L3_B16"])
    r["margin"] = r["margin"].copy()
    r["margin"][2, 5] = 1e-10
    got = SC.cast_outputs(r)
    got["b"] = got["b"].copy()
    got["b"][2, 5] *= 1j                                        # the neighbouring symbol
    rep = SC.compare(got, r)
    assert rep["left_out"] == 1 and rep["wrong_symbols"] == 0
    got["b"][3, 5] *= 1j
    assert SC.compare(got, r)["wrong_symbols"] == 1


# Copies of the mirror with one mistake each.  Mistakes that change nothing are not in the list: d = |b|^2 against
# 1 / |b|^2 and a missing division by d in y / b = y conj(b) / d (|b| = 1); real_y = sig psi against (b + e) psi (equal to
# a float64 ulp); |e / b| against |e|; p_noise = p_sig / 10^(snr_e / 10) with p_sig measured against p_sig = 1; the two
# pi / 4 of pskdemod cancelling; np.mod against fmod with the negative branch (same value).
class Transposed(SM.SynthMirror):
    def grid_index(self, Nb, Nd):                               # the grid taken as Nd x Nb: i = i_b Nb + i_d
        i = np.arange(Nb * Nd)
        return i // Nb, i % Nb


class TauSign(SM.SynthMirror):
    def phase(self, ib, idd, f, tau):
        return ib[None, None, :] * f[:, :, None] + idd[None, None, :] * tau[:, :, None]


class NoiseReusesDemodStream(SM.SynthMirror):
    noise_stream = SM.DEMOD


class SecondNormalFromNextPair(SM.SynthMirror):
    second_normal_offset = 2


class PNoiseNotHalved(SM.SynthMirror):
    def demod_noise_scale(self, p_noise):
        return np.sqrt(p_noise)


class WStdWithoutD(SM.SynthMirror):
    def noise_std(self, y2, snr_w, D):
        return np.sqrt(y2 / 10.0 ** (snr_w / 10.0))


class SnrPerElement(SM.SynthMirror):
    def snr_draw(self, seed, samples, D, snr_range):
        u = SM.uniform(self.bits(seed, samples, SM.SNR, np.arange(D)))
        return snr_range[0] + (snr_range[1] - snr_range[0]) * u


class EnergyInFloat32(SM.SynthMirror):
    def energy(self, real_y):
        p = (real_y.real ** 2 + real_y.imag ** 2).astype(np.float32)
        return p.sum(axis=1, keepdims=True, dtype=np.float32).astype(np.float64)


class PhaseInFloat32(SM.SynthMirror):
    def phase(self, ib, idd, f, tau):
        f32 = np.float32
        return (ib.astype(f32)[None, None, :] * f.astype(f32)[:, :, None]
                - idd.astype(f32)[None, None, :] * tau.astype(f32)[:, :, None]).astype(np.float64)


class RhoPlusSd(SM.SynthMirror):
    def label_denominator(self, rho, sum_d):
        return rho + sum_d


class OneIterationTooMany(SM.SynthMirror):
    extra_label_iters = 1


class LabelsInComplex64(SM.SynthMirror):
    label_dtype = np.complex64


# mistake -> (cases at which it must fail, cases at which it cannot show)
MISTAKES = {
    Transposed: (["4x6_L3_B16", "6x4_L3_B16", "8x16_L3_B64", "1x257_L2_B3", "24x32_L3_B2"], ["10x10_L3_B8", "16x16_L3_B4", "1x1_L1_B3"]),
    TauSign: (["4x6_L3_B16", "10x10_L3_B8"], ["1x1_L1_B3"]),
    NoiseReusesDemodStream: (["1x1_L1_B3", "4x6_L3_B16"], []),
    SecondNormalFromNextPair: (["1x1_L1_B3", "4x6_L3_B16"], []),
    PNoiseNotHalved: (["8x16_L3_B64"], []),
    WStdWithoutD: (["4x6_L3_B16", "10x10_L3_B8"], ["1x1_L1_B3"]),
    SnrPerElement: (["snr_5_25", "snr_-5_0", "4x6_L3_B16"], ["snr_20_20"]),
    EnergyInFloat32: (["8x16_L3_B64", "24x32_L3_B2", "26x131_L3_B2"], []),
    PhaseInFloat32: (["4x6_L3_B16", "8x16_L3_B64"], []),
    RhoPlusSd: (["labels_4x6_it5_rho2", "labels_10x10_it1_rho0.5", "4x6_L3_B16"], ["labels_4x6_it5_rho1", "labels_4x6_it0_rho2"]),
    OneIterationTooMany: (["labels_4x6_it0_rho1", "labels_4x6_it5_rho1", "labels_10x10_it12_rho2"], []),
    LabelsInComplex64: (["labels_4x6_it5_rho1", "labels_10x10_it12_rho0.5", "8x16_L3_B64"], ["labels_4x6_it0_rho1"]),
}


@pytest.mark.parametrize("mistake", list(MISTAKES), ids=lambda m: m.__name__)
def test_the_comparison_notices_one_mistake(mirrors, mistake):
    fails, blind = MISTAKES[mistake]
    for name in fails + blind:
        wrong = SC.mirror_of(SC.CASES[name], mistake)
        rep = SC.compare(SC.cast_outputs(wrong), mirrors[name])
        print("%s at %s: %s" % (mistake.__name__, name, rep["failures"] or "passes"))
        assert bool(rep["failures"]) == (name in fails), (mistake.__name__, name, rep["failures"])
