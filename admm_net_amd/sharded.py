"""Batch-sharded forward: one process per GPU, signals split across ranks.

Every signal is independent EXCEPT for one scalar per layer: the Z layer divides
each residual norm by the batch mean (admm_net.py:459).  ``scope='global'``
all-reduces (sum, count) of the residual norms once per layer -- two float64
over RCCL/xGMI -- so the sharded result equals the reference evaluated on the
whole batch; ``scope='shard'`` uses each rank's own mean (zero communication,
equals the reference evaluated on each sub-batch).  Nothing else crosses
ranks until the optional final all-gather of the outputs.

A model with ``sub_batch = g`` (independent groups of g signals, each with
its own mean) needs no per-layer collective at all when every rank starts at
a group boundary (``shard_bounds(..., sub_batch=g)``): each rank's own
per-group (sum, count) pairs go straight back, in either scope.  One
all-gather of the shard sizes per call checks the alignment.

The layer engine is injected so the protocol can be exercised on CPU ranks
(gloo) in tests; the product engine is ``HipLayerEngine`` (C ABI layer-at-a-time
entry points of include/admmnet.h).

``ShardedTraining`` is the same split for an optimisation step: the differentiable
forward of ``training.unrolled_forward`` on every rank's shard with the layers' means
over the whole batch (one float64 pair per layer in the forward, one float64 scalar
per layer in the backward), and ONE all-reduce of all gradients per step.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional

import torch
import torch.distributed as dist

from . import _lib, ops


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


STATE_SPANS = ("G", "Z", "phi0", "phi1", "h0", "h1", "alpha", "rn")   # admmnet_state_layout's order (include/admmnet.h)


def state_layout(cfg, B: int):
    """admmnet_state_layout as ({name: (byte offset, byte size of the buffer)}, end of the last span, lower_only): where the
    per-forward state of (cfg, B) lies in the workspace.  Host only; needs no GPU."""
    lib = _lib.load()
    off = (ctypes.c_int64 * (len(STATE_SPANS) + 1))()
    low = ctypes.c_int32(0)
    _lib.check(lib.admmnet_state_layout(ctypes.byref(cfg), B, off, ctypes.byref(low)), "admmnet_state_layout")
    D = cfg.M * cfg.N
    n = D + 1
    size = dict(G=8 * B * n * n, Z=8 * B * n * n, phi0=8 * B * D, phi1=8 * B * D, h0=4 * B * D, h1=4 * B * D,
                alpha=4 * B, rn=4 * B)
    return {name: (int(off[i]), size[name]) for i, name in enumerate(STATE_SPANS)}, int(off[len(STATE_SPANS)]), bool(low.value)


class LayerState:
    """Writable views (no copies) of the per-forward state inside a workspace: ``G``, ``Z`` complex64 [B, n, n], ``alpha``,
    ``rn`` float32 [B], ``phi(k)`` complex64 / ``h(k)`` float32 [B, D] of layer k (the buffer ``k & 1``: layer k + 1 reads
    them and writes the other one).  ``lower_only``: G and Z hold the lower triangle (row >= column) only, the other
    triangle is neither read nor written.  ``spans``: {name: (byte offset, byte size)} of every buffer, ``end`` the first
    byte behind them."""

    def __init__(self, ws: torch.Tensor, cfg, B: int):
        self.spans, self.end, self.lower_only = state_layout(cfg, B)
        D = cfg.M * cfg.N
        n = D + 1

        def view(name, dtype, *shape):
            o, sz = self.spans[name]
            return ws[o:o + sz].view(dtype).view(*shape)

        self.G = view("G", torch.complex64, B, n, n)
        self.Z = view("Z", torch.complex64, B, n, n)
        self._phi = (view("phi0", torch.complex64, B, D), view("phi1", torch.complex64, B, D))
        self._h = (view("h0", torch.float32, B, D), view("h1", torch.float32, B, D))
        self.alpha = view("alpha", torch.float32, B)
        self.rn = view("rn", torch.float32, B)

    def phi(self, k: int) -> torch.Tensor:
        return self._phi[k & 1]

    def h(self, k: int) -> torch.Tensor:
        return self._h[k & 1]


class HipLayerEngine:
    """begin / front(k) / back(k, mean) / finish over admmnet_begin ... admmnet_finish."""

    def __init__(self, model, y, b, sigma):
        self.lib = _lib.load()
        self.m = model
        dev = model._compute_device(y)
        self.dev = dev
        D = model.M * model.N
        self.B = y.shape[0]
        g = model.sub_batch
        self.ngroups = -(-self.B // g) if g else 1   # (sum, count) pairs per layer: one per sub-batch
        self.y, self.b = ops._c64(y, dev, (self.B, D), "y"), ops._c64(b, dev, (self.B, D), "b")
        self.sigma = ops._f32(sigma.reshape(-1), dev, None, "sigma")
        with torch.cuda.device(dev):
            self.W = model.packed_weights(dev)
            self.ws = model.workspace(self.B, dev)
            self.status = torch.zeros(4, dtype=torch.int32, device=dev)
            self.sumcnt = torch.zeros(2 * self.ngroups, dtype=torch.float64, device=dev)
            self.mean = torch.zeros(max(4, self.ngroups), dtype=torch.float32, device=dev)
            self.phi = torch.empty(self.B, D, dtype=torch.complex64, device=dev)
            self.head = (torch.empty(3, self.B, model.L, dtype=torch.float32, device=dev)
                         if model._HAS_HEAD else None)
        self.cfg = model.cfg()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def state(self) -> LayerState:
        """The per-forward state the layer calls keep in ``self.ws``, as writable views: read it, or overwrite it, between
        any two of begin / front / back / finish (on the stream the calls run on).  One exception: from layer 2 on, ``front``
        takes the diagonals of G and Z from rows the layer before left behind the state (``diag``); to
        overwrite those diagonals by hand between two layers, run the model under ``Options(sf_fold=2)``."""
        return LayerState(self.ws, self.cfg, self.B)

    def begin(self):
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.admmnet_begin(ctypes.byref(self.cfg), self.B, _ptr(self.ws), self.ws.numel(),
                                              _ptr(self.status), self._stream()), "admmnet_begin")

    def front(self, k: int) -> torch.Tensor:
        """Runs layer k up to G; returns device float64 [2] = (local sum of r_b, local count), with sub-batches
        [2 * ngroups]: that pair for every sub-batch."""
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.admmnet_layer_front(ctypes.byref(self.cfg), _ptr(self.W), k, _ptr(self.y),
                                                    _ptr(self.b), _ptr(self.sigma), self.B, _ptr(self.ws),
                                                    _ptr(self.sumcnt), _ptr(self.status), self._stream()),
                       "admmnet_layer_front")   # (writes the pair: local sum, local count)
        return self.sumcnt

    def back(self, k: int, mean: torch.Tensor):
        """ZLayer step from the batch mean, or with sub-batches from [ngroups] means."""
        with torch.cuda.device(self.dev):
            if self.m.sub_batch:
                self.mean[:self.ngroups] = mean.reshape(-1).to(torch.float32)
            else:
                self.mean[0] = mean.to(torch.float32)
            _lib.check(self.lib.admmnet_layer_back(ctypes.byref(self.cfg), _ptr(self.W), k, self.B, _ptr(self.ws),
                                                   _ptr(self.mean), self._stream()), "admmnet_layer_back")

    def back_pair(self, k: int, sum_count: torch.Tensor):
        """ZLayer step from the (all-reduced) device float64 pair (sum of r_b, number of signals): the batch mean is formed
        on the device, no host arithmetic between the calls."""
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.admmnet_layer_back_pair(ctypes.byref(self.cfg), _ptr(self.W), k, self.B, _ptr(self.ws),
                                                        _ptr(sum_count), self._stream()), "admmnet_layer_back_pair")

    def finish(self):
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.admmnet_finish(ctypes.byref(self.cfg), _ptr(self.W), self.B, _ptr(self.ws),
                                               _ptr(self.phi), _ptr(self.head), self._stream()), "admmnet_finish")
            if self.m.check_status:
                bad = int(self.status[0].item())
                if bad:
                    raise _lib.AdmmNetError(f"eigensolver failed to converge on {bad} matrices")
        return self.phi, self.head


def shard_bounds(total: int, world: int, rank: int, sub_batch: Optional[int] = None):
    """Contiguous, as-even-as-possible split of ``total`` signals; with ``sub_batch = g`` an as-even-as-possible split
    of the ceil(total / g) groups, so every shard starts at a group boundary and only the last group may be short."""
    if sub_batch is None:
        base, rem = divmod(total, world)
        lo = rank * base + min(rank, rem)
        return lo, lo + base + (1 if rank < rem else 0)
    if sub_batch < 1:
        raise ValueError(f"sub_batch must be None or >= 1, got {sub_batch}")
    glo, ghi = shard_bounds(-(-total // sub_batch), world, rank)
    return min(glo * sub_batch, total), min(ghi * sub_batch, total)


def _shard_sizes(n_local: int, world: int, dev, group):
    """The number of signals of every rank, in rank order: one all-gather."""
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([n_local], dtype=torch.int64, device=dev), group=group)
    return [int(s.item()) for s in sizes]


def _check_aligned(sizes, g: int):
    start = 0
    for r, n in enumerate(sizes):
        if n and start % g:
            raise ValueError(f"sub_batch={g}: the shard of rank {r} starts at signal {start}, inside a sub-batch "
                             f"(shard sizes {sizes}); split with shard_bounds(total, world, rank, sub_batch={g})")
        start += n


def _layer_back(eng, k: int, sc: torch.Tensor, grouped: bool):
    """The Z step of layer k from its (sum, count) pairs ``sc`` (``grouped``: one pair per sub-batch): the means are formed on
    the device (csrc/zstep.hip) where the engine has the pair call and ``sc`` is what it takes, else here."""
    if hasattr(eng, "back_pair") and sc.is_cuda and sc.dtype == torch.float64:
        eng.back_pair(k, sc)
    else:
        eng.back(k, sc[0::2] / sc[1::2] if grouped else sc[0] / sc[1])


class ShardedForward:
    def __init__(self, model, scope: str = "global", group=None,
                 engine_factory: Optional[Callable] = None):
        if scope not in ("global", "shard"):
            raise ValueError("scope must be 'global' or 'shard'")
        self.model = model
        self.scope = scope
        self.group = group
        self.engine_factory = engine_factory or (lambda y, b, s: HipLayerEngine(model, y, b, s))

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    @torch.no_grad()
    def __call__(self, y_local, b_local, sigma_local, gather: bool = False):
        """Forward of this rank's shard.  Returns (phi, head) for the shard, or for the whole
        batch (rank order) when ``gather`` is set.  ``head`` is None for PhiEstADMMNet."""
        K = self.model.num_layers
        world = self._world()
        g = getattr(self.model, "sub_batch", None)
        if g and world > 1:
            self._check_group_aligned(y_local.shape[0], g, world, y_local.device)
        eng = self.engine_factory(y_local, b_local, sigma_local)
        eng.begin()
        for k in range(K):
            sc = eng.front(k)
            if k == K - 1:
                break
            # sub-batches never span ranks: each rank's own per-group pairs, no collective
            if not g and self.scope == "global" and world > 1:
                dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=self.group)
            _layer_back(eng, k, sc, bool(g))
        phi, head = eng.finish()
        # status words of the C ABI after the forward: [0] eigensolver failures, [1] matrix-layers the matrix-function route
        # handed to the eigensolver, [2] matrix-layers it evaluated itself, [3] of [1] those rejected by the model of f
        self.last_status = [int(v) for v in eng.status.tolist()] if hasattr(eng, "status") else [0, 0, 0, 0]
        if gather and world > 1:
            phi = self._gather(phi, dim=0)
            if head is not None:
                head = self._gather(head, dim=1)
        return phi, head

    def _check_group_aligned(self, n_local: int, g: int, world: int, dev):
        """Every shard must start at a group boundary of the whole batch, i.e. every rank before the last non-empty one
        holds whole groups (shard_bounds(..., sub_batch=g) cuts that way).  Raises ValueError on every rank otherwise."""
        _check_aligned(_shard_sizes(n_local, world, dev, self.group), g)

    def _gather(self, t, dim):
        if t.is_complex():   # collectives move real tensors
            return torch.view_as_complex(self._gather(torch.view_as_real(t).contiguous(), dim))
        world = self._world()
        sizes = [torch.zeros(1, dtype=torch.int64, device=t.device) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([t.shape[dim]], dtype=torch.int64, device=t.device), group=self.group)
        sizes = [int(s.item()) for s in sizes]
        mx = max(sizes)
        pad_shape = list(t.shape)
        pad_shape[dim] = mx
        buf = torch.zeros(pad_shape, dtype=t.dtype, device=t.device)
        buf.narrow(dim, 0, t.shape[dim]).copy_(t)
        outs = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(outs, buf, group=self.group)
        return torch.cat([o.narrow(dim, 0, s) for o, s in zip(outs, sizes)], dim=dim)


class BucketKernels:
    """A tensor list to and from ONE flat buffer on the HIP kernels of csrc/optim.hip (one launch per 128 tensors): the bucket of
    ``ShardedTraining``'s parameter broadcast and gradient all-reduce."""

    pack = staticmethod(ops.optim_pack)          # (tensors, flat): flat[: total] <- the tensors in list order
    unpack = staticmethod(ops.optim_unpack)      # (tensors, flat): the tensors <- flat[: total]


class TorchBucketKernels:
    """Stand-in for tests: the same copies as tensor operations, any device."""

    @staticmethod
    def pack(tensors, flat):
        o = 0
        for t in tensors:
            flat[o:o + t.numel()].copy_(t.reshape(-1))
            o += t.numel()

    @staticmethod
    def unpack(tensors, flat):
        o = 0
        for t in tensors:
            t.copy_(flat[o:o + t.numel()].view_as(t))
            o += t.numel()


class ShardedTraining:
    """One optimisation step on a batch that is split across the ranks of a process group, with the gradients of the WHOLE batch:

        st = ShardedTraining(model, scope="global")          # broadcasts rank 0's parameters once, as one bucket
        out = st(y_local, b_local, sigma_local)              # differentiable forward of this rank's shard
        loss = criterion(out, ...) * st.weight               # st.weight = B_local / B_global, set by the call
        st.backward(loss)                                    # loss.backward(), then ONE all-reduce (sum) of every gradient
        optimizer.step()                                     # any optimiser; the ranks stay bit-identical

    The call honours ``model.train_route``, ``model.sub_batch`` and ``model.options`` and returns what
    ``model.forward_autograd`` returns.  After ``backward`` every rank holds in ``p.grad`` the gradient of the SUM of the ranks'
    losses, the network evaluated on the concatenated batch: what one process computes on that batch.  Parameters the reference
    leaves at ``grad = None`` (the detached corners, the dead last layer) stay None on every rank; that set is structural, the
    same on every rank, and the bucket holds the others in ``model.parameters()`` order.  Gradients are not accumulated across
    calls of ``backward``: clear them (``optimizer.zero_grad()``) before every step.

    Weight the LOSS before ``backward``, not the gradients after it.  Both losses of the reference are means over the batch, so
    the local means times ``st.weight`` sum to the mean over the whole batch.  With ``scope="global"`` the backward's per-layer
    all-reduce carries the other ranks' upstream gradients into this rank's graph, so the weights have to be in the seeds of the
    backward; scaling ``p.grad`` afterwards cannot undo a wrong mixture.

    ``scope="global"``: the mean of every Z layer (admm_net.py:459) is over the signals of all ranks -- per layer one all-reduce
    of the float64 (sum of the residual norms, count) pair in the forward and one of a float64 scalar, the adjoint, in the
    backward.  ``scope="shard"``: every rank uses its own mean, no per-layer collective; this is what wrapping the model in
    ``DistributedDataParallel`` computes, and it is ANOTHER network than the one a single process evaluates on the batch.
    ``model.sub_batch = g``: groups never span ranks (split with ``shard_bounds(total, world, rank, sub_batch=g)``; a shard that
    starts inside a group raises ``ValueError`` on every rank), so neither scope issues a per-layer collective and the gradient
    all-reduce is the only one of the step.

    Every rank's loss must depend on its output: a rank whose loss does not reach the Z layers never issues the backward's
    collectives and the others wait for it.  An empty shard raises ``ValueError`` on every rank.  On the ``native`` route every
    rank draws its own keep mask for the head's attention dropout, from its own generator state.

    Without a process group, or in a group of one, no collective and none of the bucket or pair kernels run: the result is
    ``torch.equal`` to ``model.forward_autograd`` followed by ``loss.backward()``.

    ``kernels``: keyword arguments of ``training.unrolled_forward`` that replace the HIP eigensolver and kernels (``solver``,
    ``assembler``, ``layer_kernels``, ``small_kernels``, ``native_kernels``) and ``bucket`` a stand-in for ``BucketKernels``: the
    CPU tests drive the protocol over gloo with the Torch stand-ins.  None: the product path."""

    def __init__(self, model, scope: str = "global", group=None, kernels: Optional[dict] = None, bucket=None):
        if scope not in ("global", "shard"):
            raise ValueError("scope must be 'global' or 'shard'")
        self.model, self.scope, self.group, self.kernels = model, scope, group, kernels
        self.bucket = BucketKernels if bucket is None else bucket
        self.weight = 1.0
        self.global_batch = None
        self._flat = None
        if self._world() > 1:
            params = [p.detach() for p in model.parameters()]
            self._flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
            self.bucket.pack(params, self._flat)
            dist.broadcast(self._flat, src=0 if group is None else dist.get_global_rank(group, 0), group=group)
            self.bucket.unpack(params, self._flat)

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _reduce(self, t):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def __call__(self, y_local, b_local, sigma_local):
        world, g = self._world(), self.model.sub_batch
        n = y_local.shape[0]
        reducer = None
        if world > 1:
            sizes = _shard_sizes(n, world, y_local.device, self.group)
            if min(sizes) == 0:
                raise ValueError(f"every rank needs at least one signal, got shard sizes {sizes}")
            if g:
                _check_aligned(sizes, g)
            elif self.scope == "global":
                reducer = self._reduce
            self.global_batch = sum(sizes)
        else:
            self.global_batch = n
        self.weight = n / self.global_batch
        if self.kernels is None:           # the product path: the model places the tensors and checks its parameters' device
            return self.model.forward_autograd(y_local, b_local, sigma_local, reducer=reducer)
        from . import training
        return training.unrolled_forward(self.model, y_local, b_local, sigma_local, sub_batch=g, reducer=reducer,
                                         **training.route_kwargs(self.model.train_route, self.kernels))

    def backward(self, loss):
        """``loss.backward()``, then -- in a group of more than one rank -- one all-reduce (sum) of all gradients through the flat
        buffer.  ``loss`` must already carry ``st.weight``."""
        loss.backward()
        if self._world() == 1:
            return
        grads = [p.grad for p in self.model.parameters() if p.grad is not None]
        n = sum(t.numel() for t in grads)
        self.bucket.pack(grads, self._flat)
        self._reduce(self._flat[:n])
        self.bucket.unpack(grads, self._flat)
