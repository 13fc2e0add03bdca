"""CPU: the one place that knows what a ``train_route`` name means -- ``training.TRAIN_ROUTES`` and ``training.route_kwargs`` --
and the single layer loop of ``training.unrolled_forward`` behind it.

  * the helper's table for the four names, which stand-ins it takes out of a full ``kernels`` dict, ``ValueError`` otherwise;
  * the ``train_route`` setter and the harness's ``--route`` accept exactly ``TRAIN_ROUTES``;
  * per route, with the Torch stand-ins and ``torch.linalg.eigh`` at 4 x 4, K = 3, B = 5: the forward through
    ``route_kwargs`` is ``torch.equal`` to the forward through the flags written out, and a counting reducer is called
    K - 1 times in the forward and K - 1 times in the backward.
"""
import pytest
import torch

import admm_net_amd as A
from admm_net_amd import harness, synth, training

KERNELS = dict(solver=torch.linalg.eigh, assembler=training.TorchAssembler, layer_kernels=training.TorchLayerKernels,
               small_kernels=training.TorchSmallKernels, native_kernels=training.TorchNativeKernels)
# route -> (fused, small, native, the stand-ins it uses): written out here, not derived
TABLE = {"tensor": (False, False, False, {"solver", "assembler"}),
         "fused": (True, False, False, {"solver", "assembler", "layer_kernels"}),
         "full": (True, True, False, {"solver", "assembler", "layer_kernels", "small_kernels"}),
         "native": (True, True, True, {"solver", "assembler", "layer_kernels", "small_kernels", "native_kernels"})}
M, N, K, B = 4, 4, 3, 5


def test_the_route_names():
    assert training.TRAIN_ROUTES == ("tensor", "fused", "full", "native") == tuple(TABLE)


@pytest.mark.parametrize("route", TABLE)
def test_route_kwargs_table(route):
    fused, small, native, _ = TABLE[route]
    assert training.route_kwargs(route) == {"fused": fused, "small": small, "native": native}
    assert training.route_kwargs(route, None) == training.route_kwargs(route, {}) == training.route_kwargs(route)


@pytest.mark.parametrize("route", TABLE)
def test_route_kwargs_takes_exactly_the_stand_ins_the_route_uses(route):
    fused, small, native, uses = TABLE[route]
    kw = training.route_kwargs(route, KERNELS)
    assert set(kw) == {"fused", "small", "native"} | uses
    assert all(kw[name] is KERNELS[name] for name in uses)
    assert (kw["fused"], kw["small"], kw["native"]) == (fused, small, native)
    only_solver = training.route_kwargs(route, {"solver": KERNELS["solver"]})        # a partial dict: what is there, no more
    assert set(only_solver) == {"fused", "small", "native", "solver"}


@pytest.mark.parametrize("bad", ["hip", "", "Tensor", "tensor ", None, 1, ("tensor",)])
def test_unknown_route_raises(bad):
    with pytest.raises(ValueError):
        training.route_kwargs(bad)
    with pytest.raises(ValueError):
        training.route_kwargs(bad, KERNELS)
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    with pytest.raises(ValueError):
        m.train_route = bad
    assert m.train_route == "tensor"


def test_setter_and_harness_accept_exactly_the_route_names(monkeypatch, capsys):
    m = A.PhiEstADMMNet(M=3, N=3, num_layers=2)
    seen = []
    monkeypatch.setattr(harness, "time_train_step", lambda *a, **kw: seen.append(kw["route"]) or {"route": kw["route"]})
    for route in training.TRAIN_ROUTES:
        m.train_route = route
        assert m.train_route == route
        harness.main(["train-step", "--route", route])
    assert tuple(seen) == training.TRAIN_ROUTES
    for bad in ("hip", "Tensor", ""):
        with pytest.raises(SystemExit) as e:
            harness.main(["train-step", "--route", bad])
        assert e.value.code == 2
    assert tuple(seen) == training.TRAIN_ROUTES
    capsys.readouterr()


class CountingReducer:
    """The identity (a group of one rank) that counts its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, t):
        self.calls += 1
        return t


@pytest.fixture(scope="module")
def batch():
    y, b, sigma, _ = synth.make_batch(B, M, N, seed=5)
    return [torch.from_numpy(v) for v in (y, b, sigma)]


def model_of(head):
    torch.manual_seed(7)
    return (A.ADMMNet if head else A.PhiEstADMMNet)(M=M, N=N, L=3, num_layers=K).eval()


def outputs(out):
    return [o.detach() for o in out] if isinstance(out, tuple) else [out.detach()]


@pytest.mark.parametrize("head", [False, True], ids=["phiest", "admmnet"])
@pytest.mark.parametrize("route", TABLE)
def test_forward_through_the_helper_equals_the_explicit_flags(batch, route, head):
    fused, small, native, uses = TABLE[route]
    runs = []
    for kw in (training.route_kwargs(route, KERNELS),
               dict(fused=fused, small=small, native=native, **{name: KERNELS[name] for name in uses})):
        m = model_of(head)
        out = training.unrolled_forward(m, *batch, **kw)
        sum(o.abs().sum() for o in (out if head else [out])).backward()
        runs.append((outputs(out), [p.grad for p in m.parameters()]))
    (out_a, g_a), (out_b, g_b) = runs
    assert len(out_a) == len(out_b) and all(torch.equal(a, b) for a, b in zip(out_a, out_b))
    assert any(g is not None for g in g_a)
    assert all((a is None and b is None) or (a is not None and b is not None and torch.equal(a, b)) for a, b in zip(g_a, g_b))


@pytest.mark.parametrize("route", TABLE)
def test_reducer_is_called_once_per_live_layer_each_way(batch, route):
    """K - 1 live Z layers: one (sum, count) pair each in the forward, one scalar each in the backward."""
    m, red = model_of(False), CountingReducer()
    out = training.unrolled_forward(m, *batch, reducer=red, **training.route_kwargs(route, KERNELS))
    assert red.calls == K - 1
    out.abs().sum().backward()
    assert red.calls == 2 * (K - 1)
