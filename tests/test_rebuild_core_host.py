"""CPU: the shared pieces of csrc/rebuild_core.h that compile for the host -- the learned eigenvalue map
f(lam) = softplus(lam - thr) * sigmoid(value_net(|lam|)) in float and in double, and the lower-triangle tile decode --
through tests/host_model/rebuild_core_model.cpp.  Every G-layer route inlines exactly these functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from admm_net_amd import modules

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "admm_net_amd", "csrc")


@pytest.fixture(scope="module")
def model():
    so = os.path.join(ROOT, "tests", "host_model", "librebuild_core_model.so")
    src = os.path.join(ROOT, "tests", "host_model", "rebuild_core_model.cpp")
    cores = [os.path.join(CSRC, f) for f in ("rebuild_core.h", "eig_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + cores):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.eig_map_f32.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    lib.eig_map_f64_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.tri_tiles.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return lib


def layer_weights(perturb):
    """value_net and threshold of a seeded GLayer, as the kernels get them: vn = w1[16] b1[16] w2[16] b2[1] in float32
    and thr = sigmoid(threshold); perturb > 0 adds N(0, perturb) to every one of them."""
    torch.manual_seed(11)
    g = modules.GLayer(4, 4)
    gen = torch.Generator().manual_seed(12)
    parts = [g.value_net[0].weight.detach().reshape(-1), g.value_net[0].bias.detach(),
             g.value_net[2].weight.detach().reshape(-1), g.value_net[2].bias.detach(), g.threshold.detach().reshape(1)]
    if perturb > 0:
        parts = [p + perturb * torch.randn(p.shape, generator=gen) for p in parts]
    vn = torch.cat(parts[:4]).numpy().astype(np.float32)
    thr = np.float32(1.0 / (1.0 + np.exp(-np.float64(parts[4].numpy().astype(np.float32)[0]))))
    assert vn.shape == (49,)
    return vn, thr


def points(vn, thr):
    """0, +-tiny, both sides of every ReLU kink |lam| = -b1_j / W1_j, lam - thr on both sides of 20 (the softplus
    switch), +-1e3."""
    w1, b1 = vn[:16].astype(np.float64), vn[16:32].astype(np.float64)
    kinks = np.array([-b / w for w, b in zip(w1, b1) if w != 0 and -b / w > 0])
    lam = [0.0, 1e-30, -1e-30, 1e-6, -1e-6, 1e3, -1e3, 0.3, -0.3, 2.5, -2.5]
    for k in kinks:
        for s in (1.0, -1.0):
            lam += [s * k * (1 - 1e-6), s * k, s * k * (1 + 1e-6)]
    t = float(thr)
    lam += [t + 20.0 - 1e-4, t + 20.0, t + 20.0 + 1e-4, t + 19.0, t + 21.0]
    return np.array(lam, np.float64)


def ref_f64(lam, thr, vn):
    """The formula in numpy float64, the 17-term sum in the order of the C++ loop.  Returns f and the gate's terms."""
    v = vn.astype(np.float64)
    x = lam - float(thr)
    with np.errstate(over="ignore"):
        base = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
    a = np.abs(lam)
    acc = np.full_like(lam, v[48])
    mag = np.full_like(lam, abs(v[48]))
    for j in range(16):
        pre = v[j] * a + v[16 + j]
        term = v[32 + j] * np.where(pre > 0.0, pre, 0.0)
        acc = acc + term
        mag = mag + np.abs(term)
    return base / (1.0 + np.exp(-acc)), mag


@pytest.mark.parametrize("perturb", [0.0, 0.3], ids=["default", "perturbed"])
def test_eig_map_f64_matches_numpy(model, perturb):
    vn, thr = layer_weights(perturb)
    lam = points(vn, thr)
    out = np.zeros_like(lam)
    model.eig_map_f64_host(len(lam), lam.ctypes.data, float(thr), vn.ctypes.data, out.ctypes.data)
    ref, _ = ref_f64(lam, thr, vn)
    err = np.abs(out - ref)
    print("max rel err", float((err / np.maximum(np.abs(ref), 1e-300)).max()))
    assert np.all(err <= 1e-14 * np.abs(ref) + 1e-300)


@pytest.mark.parametrize("perturb", [0.0, 0.3], ids=["default", "perturbed"])
def test_eig_map_float_matches_double(model, perturb):
    """Bound from the terms themselves: the gate's argument is a 17-term float sum, each term and each partial sum
    rounded once -- 2^-23 (|b2| + sum_j |W2_j relu(pre_j)|) covers it -- and sigmoid' <= 1/4 carries that into the gate;
    softplus, sigmoid and the product add 8 float ulps of the result."""
    vn, thr = layer_weights(perturb)
    lam64 = points(vn, thr)
    lam32 = lam64.astype(np.float32)
    lam64 = lam32.astype(np.float64)                      # the same points in both precisions
    f32 = np.zeros_like(lam32)
    f64 = np.zeros_like(lam64)
    model.eig_map_f32(len(lam32), lam32.ctypes.data, thr, vn.ctypes.data, f32.ctypes.data)
    model.eig_map_f64_host(len(lam64), lam64.ctypes.data, float(thr), vn.ctypes.data, f64.ctypes.data)
    ref, mag = ref_f64(lam64, thr, vn)
    x = lam64 - float(thr)
    with np.errstate(over="ignore"):
        base = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
    ulp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    bound = base * 0.25 * 2.0 ** -23 * mag + 8.0 * ulp
    err = np.abs(f32.astype(np.float64) - f64)
    print("max err / bound", float((err / bound).max()))
    assert np.all(err <= bound)


def test_tri_tile_enumerates_the_lower_triangle(model):
    IJ = np.zeros((45, 2), np.int32)
    model.tri_tiles(45, IJ.ctypes.data)
    assert [tuple(r) for r in IJ] == [(i, j) for i in range(9) for j in range(i + 1)]
