"""CPU: admmnet_state_layout (include/admmnet.h) and the view sharded.LayerState builds on it.  The entry point is host only,
so the library answers without a GPU."""
import ctypes

import pytest
import torch

from admm_net_amd import _lib, sharded
from admm_net_amd._lib import Cfg
from admm_net_amd.options import Options

GEOMS = [(1, 1), (2, 4), (10, 10), (8, 16), (3, 43), (7, 25), (11, 16), (16, 16)]   # D = 1, 8, 100, 128, 129, 175, 176, 256
BATCHES = [1, 5, 8193]
OPTION_SETS = {"default": None, "spectral0": dict(spectral=0), "arrow0": dict(arrow=0)}


def _cfg(M, N, sub_batch, opts, K=3):
    handle = 0 if opts is None else Options(**opts).handle
    return Cfg(M, N, 3, K, 0, 0, (ctypes.c_int32 * 2)(sub_batch, handle))


def _full_storage(D, opts):
    """route_for (csrc/route.h): full storage with the arrowhead first layer off, and at 128 < D < 176 without the
    matrix-function route (no padding below 176 there, so no panel tridiagonalisation to read lower triangles)."""
    opts = opts or {}
    return opts.get("arrow", 1) == 0 or (opts.get("spectral", 1) == 0 and 128 < D < 176)


@pytest.mark.parametrize("opt", sorted(OPTION_SETS))
@pytest.mark.parametrize("sub_batch", [0, 3])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("M,N", GEOMS, ids=[f"D{a * b}" for a, b in GEOMS])
def test_state_layout(M, N, B, sub_batch, opt):
    lib = _lib.load()
    opts = OPTION_SETS[opt]
    cfg = _cfg(M, N, sub_batch, opts)
    D, n = M * N, M * N + 1
    spans, end, lower_only = sharded.state_layout(cfg, B)
    # (the sizes come from sharded.state_layout's own table, so ``size == want`` only guards that table; what pins the C layout
    #  is the chain below: every offset the library reports is the aligned end of the documented buffer before it)
    want = dict(G=8 * B * n * n, Z=8 * B * n * n, phi0=8 * B * D, phi1=8 * B * D, h0=4 * B * D, h1=4 * B * D, alpha=4 * B, rn=4 * B)
    assert tuple(spans) == sharded.STATE_SPANS == ("G", "Z", "phi0", "phi1", "h0", "h1", "alpha", "rn")
    pos = 0
    for name in sharded.STATE_SPANS:                       # the documented order, each span right behind the one before
        off, size = spans[name]
        assert off % 256 == 0 and size == want[name], (name, off, size)
        assert off == pos, (name, off, pos)                # no gap beyond the alignment, no overlap
        pos = -(-(off + size) // 256) * 256
    assert end == pos and end % 256 == 0
    total = lib.admmnet_workspace_bytes(ctypes.byref(cfg), B)
    assert 0 < end <= total, (end, total)
    assert lower_only == (not _full_storage(D, opts)), (D, opts, lower_only)


def test_state_layout_rejects_bad_arguments():
    lib = _lib.load()
    off = (ctypes.c_int64 * 9)()
    assert lib.admmnet_state_layout(ctypes.byref(_cfg(10, 10, 0, None)), 0, off, None) != 0
    assert lib.admmnet_state_layout(ctypes.byref(_cfg(10, 10, 0, None)), 4, None, None) != 0
    assert lib.admmnet_state_layout(ctypes.byref(_cfg(17, 16, 0, None)), 4, off, None) != 0     # D > 256
    assert lib.admmnet_state_layout(ctypes.byref(_cfg(10, 10, 0, None)), 4, off, None) == 0     # lower_only may be NULL


@pytest.mark.parametrize("opt", ["default", "arrow0"])
def test_layer_state_views_alias_the_workspace(opt):
    """LayerState on a host buffer: the views are the documented shapes and dtypes, share the workspace's memory (writes go
    through, nothing is copied) and do not overlap."""
    cfg = _cfg(3, 11, 0, OPTION_SETS[opt])
    B, D, n = 5, 33, 34
    need = _lib.load().admmnet_workspace_bytes(ctypes.byref(cfg), B)
    ws = torch.zeros(need, dtype=torch.uint8)
    st = sharded.LayerState(ws, cfg, B)
    assert st.lower_only == (opt == "default")
    views = dict(G=st.G, Z=st.Z, phi0=st.phi(0), phi1=st.phi(1), h0=st.h(0), h1=st.h(1), alpha=st.alpha, rn=st.rn)
    assert st.phi(2) is st.phi(0) and st.h(3) is st.h(1)
    assert st.G.shape == st.Z.shape == (B, n, n) and st.G.dtype == st.Z.dtype == torch.complex64
    assert st.phi(0).shape == (B, D) and st.phi(1).dtype == torch.complex64
    assert st.h(0).shape == (B, D) and st.h(1).dtype == torch.float32 and st.alpha.shape == st.rn.shape == (B,)
    for i, (name, v) in enumerate(views.items()):
        off, size = st.spans[name]
        assert v.data_ptr() == ws.data_ptr() + off and v.numel() * v.element_size() == size
        v.fill_(i + 1)
    for i, (name, v) in enumerate(views.items()):
        off, size = st.spans[name]
        assert bool((v == i + 1).all()), name                       # no later fill reached it
        assert int(ws[off:off + size].count_nonzero()) > 0          # and the write went into the workspace
    assert int(ws[st.end:].count_nonzero()) == 0                    # nothing behind the state was touched
