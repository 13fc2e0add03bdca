"""CPU: the PeakSearchLayer head of the native training route, ``training._PeakHead`` with the tensor stand-in
``training.TorchNativeKernels`` for the HIP kernels of csrc/train_head.hip, in float64.

* without a mask, on a head in ``eval()``: ``tau``, ``f``, ``conf``, ``g_phi`` and every head parameter's gradient --
  ``position_encoder`` and the three ``in_proj`` slices included -- against autograd through ``training._peak_head`` within 1e-12
  of the largest entry, at D = 1, 7, 12, L = 1, 3, B = 1, 5;
* with a keep mask: the hand-written backward against autograd through the stand-in's own forward at 1e-12, and the forward
  against ``_peak_head`` on a head in ``train()`` with ``torch.nn.functional.dropout`` patched to apply the same mask;
* the drawn mask: the dropped share over 10^6 draws within 4.5 sigma of p, the scale exactly 1 / (1 - p);
* ``mag = True`` bounds every batch sum's magnitude; a wrong mask shape or dtype raises.
"""
import math
from unittest import mock

import pytest
import torch

import admm_net_amd as A
from admm_net_amd import training

from test_training_fused import _close

TNK = training.TorchNativeKernels
F64 = torch.float64
GEOMETRIES = [(1, 1), (7, 1), (3, 4)]          # D = 1, 7, 12
CASES = [(M, N, L, B) for M, N in GEOMETRIES for L in (1, 3) for B in (1, 5)]


def head_case(M, N, L, B, seed=0):
    torch.manual_seed(seed + 17 * M + 5 * L + B)
    head = A.modules.PeakSearchLayer(M, N, L).double()
    with torch.no_grad():
        for p in head.parameters():                                       # biases off zero, position_encoder perturbed
            p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(seed + 1)
    phi = torch.complex(torch.randn(B, M * N, dtype=F64, generator=g), torch.randn(B, M * N, dtype=F64, generator=g))
    ups = [torch.randn(B, L, dtype=F64, generator=g) for _ in range(3)]
    return head, phi, ups


def grads_of(outs, ups, phi, head):
    params = list(head.parameters())
    got = torch.autograd.grad(outs, [phi] + params, ups, allow_unused=True)
    return got[0], dict(zip([n for n, _ in head.named_parameters()], got[1:]))


def compare(head, phi, ups, reference, keep):
    a, b = phi.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    o1 = training._PeakHead.apply(a, keep, 0.1, head.L_max, TNK, *training._head_params(head))
    o2 = reference(b)
    for x, y, name in zip(o1, o2, ("tau", "f", "conf")):
        assert x.shape == y.shape == (phi.shape[0], head.L_max)
        _close(x.detach(), y.detach(), name)
    gp1, g1 = grads_of(o1, ups, a, head)
    gp2, g2 = grads_of(o2, ups, b, head)
    _close(gp1, gp2, "g_phi")
    assert set(g1) == set(g2)
    for name, want in g2.items():
        assert want is not None and g1[name] is not None, name
        assert g1[name].shape == want.shape, name
        _close(g1[name], want, name)
    for k, sl in enumerate(("q", "k", "v")):                               # the slices on their own, not under one maximum
        s = slice(128 * k, 128 * (k + 1))
        _close(g1["attention.in_proj_weight"][s], g2["attention.in_proj_weight"][s], "in_proj_weight." + sl)
        if sl != "k":   # the K slice of the bias is zero but for round-off (it shifts a head's scores by a constant, which the
            #             softmax does not see): it is held to the whole tensor's largest entry above
            _close(g1["attention.in_proj_bias"][s], g2["attention.in_proj_bias"][s], "in_proj_bias." + sl)


@pytest.mark.parametrize("M,N,L,B", CASES)
def test_peak_head_without_mask_matches_autograd_through_peak_head(M, N, L, B):
    head, phi, ups = head_case(M, N, L, B)
    head.eval()
    compare(head, phi, ups, lambda x: training._peak_head(head, x), None)


def _mask(B, D, p, seed):
    return torch.rand(B, 4, D, generator=torch.Generator().manual_seed(seed)) >= p


@pytest.mark.parametrize("M,N,L,B", CASES)
def test_peak_head_with_mask_backward_matches_autograd_through_the_stand_in(M, N, L, B):
    head, phi, ups = head_case(M, N, L, B, seed=3)
    keep = _mask(B, M * N, 0.3, 7)
    hp = training._head_params(head)
    compare(head, phi, ups, lambda x: TNK.head(x, keep, 0.1, L, hp)[:3], keep)


@pytest.mark.parametrize("M,N,L,B", [(7, 1, 3, 5), (3, 4, 1, 1)])
def test_peak_head_with_mask_forward_matches_peak_head_in_train_mode(M, N, L, B):
    """``F.multi_head_attention_forward`` calls ``torch.nn.functional.dropout`` on the softmax's output [B * 4, 1, D] (it is the
    only dropout of the head), so patching it applies the given mask in the reference's own graph."""
    head, phi, ups = head_case(M, N, L, B, seed=5)
    head.train()
    p = head.attention.dropout
    keep = _mask(B, M * N, 0.4, 11)
    calls = []

    def masked(x, p=0.5, training=True, inplace=False):
        calls.append((tuple(x.shape), p, training))
        return x * keep.reshape(x.shape).to(x.dtype) / (1.0 - p)

    with mock.patch("torch.nn.functional.dropout", masked):
        want = training._peak_head(head, phi)
    assert calls == [((B * 4, 1, M * N), p, True)]
    got = training._PeakHead.apply(phi, keep, p, L, TNK, *training._head_params(head))
    for x, y, name in zip(got, want, ("tau", "f", "conf")):
        _close(x.detach(), y.detach(), name)


def test_all_dropped_row_gives_finite_zeros():
    head, phi, ups = head_case(3, 4, 3, 2, seed=9)
    keep = _mask(2, 12, 0.5, 2)
    keep[1, 2] = False
    a = phi.clone().requires_grad_(True)
    outs = training._PeakHead.apply(a, keep, 0.5, 3, TNK, *training._head_params(head))
    g_phi, g = grads_of(outs, ups, a, head)
    assert all(torch.isfinite(o).all() for o in outs) and torch.isfinite(g_phi).all()
    assert all(torch.isfinite(v).all() for v in g.values())


def test_mask_share_and_scale():
    p, n = 0.1, 10 ** 6
    keep = training.draw_keep_mask(250, 1000, p, "cpu", generator=torch.Generator().manual_seed(4))
    assert keep.shape == (250, 4, 1000) and keep.dtype == torch.bool and keep.element_size() == 1
    assert keep.numel() == n
    dropped = float((~keep).sum()) / n
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"dropped share {dropped:.6f}, p = {p}, {abs(dropped - p) / sigma:.2f} sigma")
    assert abs(dropped - p) <= 4.5 * sigma
    # the scale: the stand-in multiplies a kept weight by exactly 1 / (1 - p), a dropped one by 0
    head, phi, _ = head_case(7, 1, 1, 3)
    k = _mask(3, 7, 0.5, 1)
    for pp in (0.1, 0.5):
        s = TNK._head_parts(phi, k, pp, 1, training._head_params(head))
        assert torch.equal(s.km, k.to(F64) * (1.0 / (1.0 - pp)))
        assert torch.equal(s.am, s.a * s.km)


def test_head_draws_a_mask_only_in_train_mode():
    head, phi, _ = head_case(3, 4, 3, 5)
    head.eval()
    a = training._peak_head_native(head, phi, TNK)
    b = training._peak_head_native(head, phi, TNK)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    head.train()
    torch.manual_seed(1)
    c = training._peak_head_native(head, phi, TNK)
    torch.manual_seed(2)
    d = training._peak_head_native(head, phi, TNK)
    assert not torch.equal(c[0], d[0]) and not torch.equal(a[0], c[0])
    torch.manual_seed(1)
    assert torch.equal(training._peak_head_native(head, phi, TNK)[0], c[0])


def test_magnitude_form_bounds_every_batch_sum():
    head, phi, ups = head_case(3, 4, 3, 5)
    hp = [p.detach() for p in training._head_params(head)]
    keep = _mask(5, 12, 0.2, 3)
    _, g = TNK.head_bwd(*ups, phi, keep, 0.2, 3, hp)
    _, mag = TNK.head_bwd(*ups, phi, keep, 0.2, 3, hp, mag=True)
    for x, y in zip(g, mag):
        assert x.shape == y.shape and (x.abs() <= y * (1 + 1e-12) + 1e-300).all()


def test_wrong_mask_shape_or_dtype_raises():
    head, phi, _ = head_case(3, 4, 1, 2)
    hp = training._head_params(head)
    good = _mask(2, 12, 0.1, 0)
    for bad in (good.float(), good.to(torch.int32), good[:, :3], good[:1], good.reshape(2, 12, 4), good.reshape(2, 48), "mask"):
        with pytest.raises(ValueError):
            training._PeakHead.apply(phi, bad, 0.1, 1, TNK, *hp)
    training._PeakHead.apply(phi, good.to(torch.uint8), 0.1, 1, TNK, *hp)


def test_train_head_ops_refuse_cpu_tensors():
    from admm_net_amd import _lib, ops
    head, phi, ups = head_case(3, 4, 1, 2)
    head.float()
    hp = training._head_params(head)
    with pytest.raises(_lib.AdmmNetError):
        ops.train_head(phi.to(torch.complex64), None, 0.1, 1, hp)


def training_head_grad_floats(D, L):
    """Every parameter of the head once, the 256 D floats of gK / gV scratch between them."""
    head = A.modules.PeakSearchLayer(D, 1, L)
    return sum(p.numel() for p in head.parameters()) + 256 * D


def test_train_head_entry_points_reject_bad_arguments():
    """ADMMNET_E_ARG (-1) for D outside 1 ... 256, L outside 1 ... 16, B < 1 and null pointers, decided on the host before
    anything is launched; the workspace query answers -1 for the same sizes."""
    import ctypes
    from admm_net_amd import _lib
    lib = _lib.load()
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)
    work = lib.admmnet_train_head_workspace
    assert work(100, 3, 256, 0) == 4 * (256 * (4 * 100 + 752 + 80 * 3) + 3 * 100 * 128)
    assert work(100, 3, 256, 1) > 0 and work(100, 3, 256, 3) == -1
    assert work(100, 3, 256, 2) == 4 * training_head_grad_floats(100, 3)
    full = (ctypes.c_void_p * 149)(*([64] * 149))                      # a table without a null, read on the host only
    assert lib.admmnet_train_head_f32(100, 16, 65535 * 8 + 1, p, full, null, ctypes.c_float(0.1), p, p, p, p, null) == -1
    for d, L, B in ((0, 3, 4), (257, 3, 4), (100, 0, 4), (100, 17, 4), (100, 3, 0)):
        assert work(d, L, B, 0) == -1 and work(d, L, B, 1) == -1
        assert lib.admmnet_train_head_f32(d, L, B, p, full, p, ctypes.c_float(0.1), p, p, p, p, null) == -1
        assert lib.admmnet_train_head_bwd_f32(d, L, B, p, p, p, p, full, p, ctypes.c_float(0.1), p, p, p, p, p, p, p, null) == -1
    assert b"train_head_bwd" in lib.admmnet_last_error()
    assert lib.admmnet_train_head_f32(100, 3, 4, p, null, null, ctypes.c_float(0.1), p, p, p, p, null) == -1
    table = (ctypes.c_void_p * 45)(*([64] * 45))                       # the pointer table itself is read on the host
    for prob in (1.0, -0.1, 1.5):                                     # with a mask, p must lie in [0, 1)
        assert lib.admmnet_train_head_f32(100, 3, 4, p, table, p, ctypes.c_float(prob), p, p, p, p, null) == -1
    table[44] = None                                                  # a null parameter
    assert lib.admmnet_train_head_f32(100, 3, 4, p, table, null, ctypes.c_float(0.1), p, p, p, p, null) == -1
    for i in (0, 3, 4, 5, 6):                                         # phi, tau, f, conf, saved
        a = [p, table, null, p, p, p, p]
        a[i] = null
        assert lib.admmnet_train_head_f32(100, 3, 4, a[0], a[1], a[2], ctypes.c_float(0.1), *a[3:], null) == -1
