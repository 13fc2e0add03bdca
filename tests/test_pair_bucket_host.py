"""CPU: the host side of the entry points behind ``sharded.ShardedTraining`` -- the step size from an outside (sum, count) pair
(csrc/train_small.hip) and the gradient bucket (csrc/optim.hip).  Argument checks are decided on the host before anything is
launched, the ops refuse host tensors (there is no CPU path), and the bucket's Torch stand-in is the copy it says it is."""
import ctypes

import pytest
import torch
import torch.nn as nn

from admm_net_amd import _lib, ops, sharded, training

E_ARG = -1


def test_pair_entry_points_reject_bad_arguments():
    lib = _lib.load()
    p, odd, null = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(0)     # never dereferenced: every call fails its check
    part = lib.admmnet_train_stepsize_pair_partials
    assert part(1) == 164 and part(256) == 164 and part(257) == 2 * 164 and part(0) == -1 and part(-3) == -1
    for B in (0, -1, 2 ** 40):
        assert lib.admmnet_train_rnsum_f64(B, p, p, null) == E_ARG
        assert lib.admmnet_train_stepsize_pair_f32(B, 0.3, p, p, p, p, p, p, p, p, null) == E_ARG
        assert lib.admmnet_train_stepsize_bwd_pair_front_f32(B, 0.3, p, p, p, p, p, p, p, p, p, p, p, p, null) == E_ARG
        assert lib.admmnet_train_stepsize_bwd_pair_back_f32(B, p, p, p, p, null) == E_ARG
    assert b"train_stepsize_bwd_pair_back" in lib.admmnet_last_error()
    # a null pointer, float64 data off its 8-byte alignment
    assert lib.admmnet_train_rnsum_f64(4, null, p, null) == E_ARG and lib.admmnet_train_rnsum_f64(4, p, odd, null) == E_ARG
    assert lib.admmnet_train_stepsize_pair_f32(4, 0.3, p, odd, p, p, p, p, p, p, null) == E_ARG
    assert lib.admmnet_train_stepsize_pair_f32(4, 0.3, p, p, p, p, p, p, p, null, null) == E_ARG
    assert lib.admmnet_train_stepsize_bwd_pair_front_f32(4, 0.3, p, p, p, p, p, p, p, p, p, p, odd, p, null) == E_ARG
    assert lib.admmnet_train_stepsize_bwd_pair_front_f32(4, 0.3, p, p, p, p, p, p, p, p, p, p, p, odd, null) == E_ARG
    assert lib.admmnet_train_stepsize_bwd_pair_front_f32(4, 0.3, p, p, p, p, p, p, p, p, null, p, p, p, null) == E_ARG
    assert lib.admmnet_train_stepsize_bwd_pair_back_f32(4, p, p, odd, p, null) == E_ARG
    assert lib.admmnet_train_stepsize_bwd_pair_back_f32(4, p, p, p, null, null) == E_ARG


def test_bucket_entry_points_reject_bad_arguments():
    lib = _lib.load()
    ptr, n, none = (ctypes.c_void_p * 1)(64), (ctypes.c_int64 * 1)(8), (ctypes.c_void_p * 1)(0)
    flat = ctypes.c_void_p(64)
    for fn in (lib.admmnet_optim_pack_f32, lib.admmnet_optim_unpack_f32):
        assert fn(0, None, None, None, None) == 0                                  # an empty list does nothing
        assert fn(-1, ptr, n, flat, None) == E_ARG and b"count" in lib.admmnet_last_error()
        assert fn(1, ptr, n, None, None) == E_ARG                                  # no flat buffer
        assert fn(1, None, n, flat, None) == E_ARG
        assert fn(1, none, n, flat, None) == E_ARG and b"null" in lib.admmnet_last_error()
        assert fn(1, ptr, (ctypes.c_int64 * 1)(-2), flat, None) == E_ARG


def test_pair_and_bucket_ops_refuse_host_tensors():
    v, s = torch.rand(3), torch.tensor(0.5)
    z = training._net_params(nn.Sequential(nn.Linear(3, 32), nn.ReLU(), nn.Linear(32, 1), nn.Sigmoid()))
    pair, total = torch.tensor([3.0, 3.0], dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    for call in (lambda: ops.train_rnsum(v), lambda: ops.train_stepsize_pair(v, pair, s, *z, 0.3),
                 lambda: ops.train_stepsize_bwd_pair_front(v, v, pair, s, *z, 0.3),
                 lambda: ops.train_stepsize_bwd_pair_back(v, pair, total)):
        with pytest.raises(_lib.AdmmNetError):
            call()
    for call in (ops.optim_pack, ops.optim_unpack):
        with pytest.raises(ValueError):
            call([torch.zeros(4)], torch.zeros(4))
        with pytest.raises(TypeError):
            call([torch.zeros(4, dtype=torch.float64)], torch.zeros(4))
        call([], torch.zeros(0))                                                    # an empty list does nothing
    assert sharded.BucketKernels.pack is ops.optim_pack and training.SmallKernels.rnsum is ops.train_rnsum


def test_torch_bucket_stand_in_is_cat_and_its_inverse():
    g = torch.Generator().manual_seed(0)
    tensors = [torch.randn(s, generator=g) for s in ((0,), (1,), (3, 5), (7,))]
    total = sum(t.numel() for t in tensors)
    flat = torch.full((total + 3,), -5.0)
    sharded.TorchBucketKernels.pack(tensors, flat)
    assert torch.equal(flat[:total], torch.cat([t.reshape(-1) for t in tensors])) and (flat[total:] == -5.0).all()
    back = [torch.zeros_like(t) for t in tensors]
    sharded.TorchBucketKernels.unpack(back, flat)
    assert all(torch.equal(a, b) for a, b in zip(back, tensors))


def test_sharded_training_checks_its_scope():
    with pytest.raises(ValueError):
        sharded.ShardedTraining(nn.Linear(1, 1), scope="rank")
