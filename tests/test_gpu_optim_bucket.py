"""GPU: ``ops.optim_pack`` / ``ops.optim_unpack`` (csrc/optim.hip) -- a tensor list to and from ONE flat buffer, the bucket of
``sharded.ShardedTraining``'s parameter broadcast and gradient all-reduce.  They are copies, so the rule is bit equality:
``pack`` gives ``torch.cat([t.reshape(-1) ...])``, ``unpack(pack(x))`` gives x, and what lies behind the list's total in the
flat buffer stays untouched (a canary)."""
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import ops, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = -12345.0


def _roundtrip(tensors, what):
    total = sum(t.numel() for t in tensors)
    flat = torch.full((total + 9,), CANARY, device=DEV)
    ops.optim_pack(tensors, flat)
    want = torch.cat([t.reshape(-1) for t in tensors]) if tensors else torch.empty(0, device=DEV)
    assert torch.equal(flat[:total], want), f"{what}: pack differs from torch.cat"
    assert (flat[total:] == CANARY).all(), f"{what}: pack wrote behind the list's total"
    back = [torch.full_like(t, 7.0) for t in tensors]
    ops.optim_unpack(back, flat)
    assert all(torch.equal(a, b) for a, b in zip(back, tensors)), f"{what}: unpack(pack(x)) differs from x"
    assert (flat[total:] == CANARY).all() and torch.equal(flat[:total], want), f"{what}: unpack wrote into the flat buffer"


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def test_every_block_shape_and_both_access_widths():
    g = torch.Generator().manual_seed(1)
    # 0, 1, 3: less than a thread's four; 1023, 1024, 1025: around a block; 4099: five blocks, a ragged last one.  The places in
    # the flat buffer (0, 0, 1, 4, 1027, ...) are mostly not 16-byte aligned: the 4-byte path
    _roundtrip([_rand(g, n) for n in (0, 1, 3, 1023, 1024, 1025, 4099)], "mixed counts")
    # aligned tensors at aligned places: the 16-byte path, several blocks, 2-d shapes
    _roundtrip([_rand(g, 32, 32), _rand(g, 2048), _rand(g, 4), _rand(g, 3, 1024)], "aligned")
    # a view one element behind an aligned base, at a place that is aligned: the 4-byte path through the tensor's pointer
    buf = _rand(g, 2049)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _roundtrip([_rand(g, 1024), view, _rand(g, 8)], "odd offset")
    _roundtrip([], "empty list")


def test_a_list_longer_than_one_launch():
    g = torch.Generator().manual_seed(2)
    _roundtrip([_rand(g, (i * 37) % 11 if i % 50 else 1024 + i) for i in range(300)], "300 tensors")


def test_a_models_gradient_list_and_parameters():
    torch.manual_seed(4)
    m = A.ADMMNet(M=4, N=4, num_layers=3).to(DEV).eval()
    y, b, sigma, _ = synth.make_batch(3, 4, 4, seed=5)
    out = m.forward_autograd(*(torch.from_numpy(v).to(DEV) for v in (y, b, sigma)))
    (out[3].abs().pow(2).sum() + out[0].sum() + out[1].sum() + out[2].sum()).backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert 0 < len(grads) < len(list(m.parameters()))            # the detached corners and the dead last layer have none
    _roundtrip(grads, "gradients")
    _roundtrip([p.detach() for p in m.parameters()], "parameters")


def test_argument_checks():
    t = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        ops.optim_pack([t], torch.zeros(7, device=DEV))            # no room
    with pytest.raises(ValueError):
        ops.optim_pack([t.cpu()], torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        ops.optim_unpack([t], torch.zeros(8))                      # a host buffer
    with pytest.raises(TypeError):
        ops.optim_pack([t], torch.zeros(8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.optim_pack([torch.zeros(4, 4, device=DEV).t()], torch.zeros(16, device=DEV))
