"""GPU (-m gpu): synth_kernel (csrc/synth.hip, behind admmnet_synth_batch / synth.make_batch_device) against its float64 host
mirror, element by element.

The kernel's generator is counter based, so tests/synth_mirror.py reproduces every draw exactly and restates the recipe
(generate_data.py:133-221, :410-463) in float64; tests/synth_checks.compare holds every output -- tau, f, C, b, y, sigma, phi
-- to one float32 spacing plus 64 * 2^-53 of the magnitude of its terms, the decided symbols to equality, and the share of
elements that are not bit-equal to the cast mirror to 1e-3.  tests/test_synth_mirror.py (CPU) ties the mirror to the host
recipe and to the literal classical solver, and shows that twelve one-line mistakes fail this comparison at these cases.

Cases (synth_checks.CASES): the geometries 1 x 1 .. 24 x 32 and the largest D the entry point accepts (26 x 131 = 3406), with
labels at rho = 2; seeds 0, 5, 2^63 + 12345, 2^64 - 1 and -1; three SNR ranges; label_iters x rho at 4 x 6 and 10 x 10;
B = 70 000 at 2 x 2; the argument contracts of the entry point.

Measured on the MI355X, over all 45 comparisons above (every geometry including D = 3406, every seed, SNR range and
label_iters x rho combination, the five samples of the B = 70 000 grid, the scenes generated without labels):
  output   worst error / bound   share of elements not bit-equal to the cast mirror
  tau      0                     0
  f        0                     0
  C        0                     0
  b        0                     0        (no decided symbol differs, none left out)
  y        0                     0
  sigma    0                     0
  phi      0                     0
Every element the kernel wrote has the bits of the float64 mirror's value cast to float32: the device's sincos / log / atan2 /
pow and its FMA contraction stay within the few float64 ulps the slack allows for, and over these ~1e5 elements none of those
differences crossed a float32 rounding boundary (expected share ~1e-8).  For comparison (tests/test_synth_mirror.py, CPU): labels
computed from the complex64-cast scene instead of the float64 one miss the same bound by 5x .. 340x with 49 % .. 98 % of the
elements not bit-equal; the y2 block sum in float32 moves 1 % .. 13 % of y and phi.  D = 3406 uses exactly the 160 KiB of LDS of a
CU and the runtime launches it; D = 3407 is refused on the host.  No check failed on the device and the kernel was not changed.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, synth
import synth_checks as SC

pytestmark = pytest.mark.gpu
OUTPUTS = ("y", "b", "sigma", "tau", "f", "C")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def mirror_of(name):
    return SC.mirror_of(SC.CASES[name])


def device_batch(c, dev, labels=True, seed=None):
    """The whole batch of case ``c`` on the device; dict of device tensors."""
    y, b, sigma, t = synth.make_batch_device(c["B"], c["Nb"], c["Nd"], L=c["L"], seed=c["seed"] if seed is None else seed,
                                             snr_range=c["snr_range"], snr_e=c["snr_e"], device=dev, labels=labels,
                                             rho=c["rho"], label_iters=c["label_iters"])
    return dict(y=y, b=b, sigma=sigma, **t)


def rows(out, samples):
    idx = torch.as_tensor(samples, device=out["y"].device)
    return {k: v[idx].cpu().numpy() for k, v in out.items()}


def check(name, got):
    rep = SC.compare(got, mirror_of(name))
    print("%s: %s" % (name, SC.describe(rep)))
    assert rep["left_out"] == 0 and not rep["failures"], rep["failures"]
    return rep


@pytest.mark.parametrize("name", list(SC.GEOMETRIES) + list(SC.SEEDS) + list(SC.SNR_RANGES) + list(SC.LABELS))
def test_device_generator_equals_the_float64_mirror(dev, name):
    """Every output of every sample, with labels; the D = 3406 case is the largest the entry point accepts."""
    c = SC.CASES[name]
    got = rows(device_batch(c, dev), c["samples"])
    check(name, got)
    if c["label_iters"] == 0:
        assert not got["phi"].view(np.uint32).any()                      # phi_0 = 0: exact zeros


def test_seed_minus_one_has_the_bits_of_the_largest_seed(dev):
    c = SC.CASES["seed_%d" % (2 ** 64 - 1)]
    got = rows(device_batch(c, dev, seed=-1), c["samples"])
    check("seed_%d" % (2 ** 64 - 1), got)
    top = rows(device_batch(c, dev), c["samples"])
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), top[k].view(np.uint32)), k


@pytest.mark.parametrize("name", ["4x6_L3_B16", "24x32_L3_B2"])
def test_labels_do_not_change_the_scene(dev, name):
    """labels=False and labels=True: bit-identical y, b, sigma, tau, f, C; the scene without labels equals the mirror's."""
    c = SC.CASES[name]
    with_l, without = device_batch(c, dev, labels=True), device_batch(c, dev, labels=False)
    assert "phi" not in without
    for k in OUTPUTS:
        a, b = with_l[k].cpu().numpy(), without[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    check(name, rows(without, c["samples"]))


def test_grid_of_70000_workgroups(dev):
    """B = 70 000 (past 65 535 blocks): everything finite, |b| = 1 to float32, and samples 0, 1, 65535, 65536 and 69999 equal
    the mirror evaluated at those indices only."""
    c = SC.CASES["grid_2x2_B70000"]
    out = device_batch(c, dev)
    for k, v in out.items():
        assert torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all(), k
    assert float((out["b"].abs() - 1.0).abs().max()) <= 2.0 ** -23
    check("grid_2x2_B70000", rows(out, c["samples"]))


SENTINEL = 7.25
CONTRACTS = {"L0": dict(L=0), "L9": dict(L=9), "label_iters_negative": dict(label_iters=-1),
             "D_above_the_bound": dict(Nb=SC.OVER_D_GRID[0], Nd=SC.OVER_D_GRID[1])}


@pytest.mark.parametrize("name", list(CONTRACTS))
def test_entry_point_refuses_before_launching(dev, name):
    """The argument check is on the host: AdmmNetError, and outputs pre-filled with a sentinel keep it."""
    a = dict(B=2, Nb=4, Nd=6, L=3, label_iters=5)
    a.update(CONTRACTS[name])
    assert SC.OVER_D_GRID[0] * SC.OVER_D_GRID[1] == SC.MAX_D + 1
    D, Lr = a["Nb"] * a["Nd"], max(a["L"], 1)
    cx = lambda *s: torch.full(s, complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)   # noqa: E731
    fl = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)                        # noqa: E731
    bufs = [cx(a["B"], D), cx(a["B"], D), fl(a["B"]), fl(a["B"], Lr), fl(a["B"], Lr), cx(a["B"], Lr), cx(a["B"], D)]
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.admmnet_synth_batch(a["B"], a["Nb"], a["Nd"], a["L"], 5, 5.0, 25.0, 7.0, 1.0, a["label_iters"],
                                     *[ctypes.c_void_p(t.data_ptr()) for t in bufs], stream)
        with pytest.raises(_lib.AdmmNetError):
            _lib.check(rc, "admmnet_synth_batch")
        torch.cuda.synchronize(dev)
    for t in bufs:
        assert bool((torch.view_as_real(t) if t.is_complex() else t).eq(SENTINEL).all())
