"""Drop-in ``ADMMNet`` / ``PhiEstADMMNet`` for /root/reference/admm_net.py.

Same constructor (``M, N, L=3, num_layers=10``), same ``forward(y, b, sigma)``
return values and the same ``state_dict`` key set / parameter names
(admm_net.py:724-816), so ``main_for_net.py``, ``test/test_time_net.py`` and
``load_state_dict`` of a reference checkpoint work unchanged.  The sub-modules
below are parameter containers registered in the reference's order (so
``torch.manual_seed(s)`` + construction yields the reference's initial
weights); all arithmetic happens in the fused HIP path behind the C ABI of
``include/admmnet.h``.  There is no CPU or eager fallback.

Inference (``.eval()`` or ``torch.no_grad()``) runs the fused forward.  In train mode with gradients
enabled the call goes through ``training.unrolled_forward`` instead: differentiable tensor operations
around the HIP eigensolver, with the reference's eigenvalue-only gradient;
``model.train_route = "fused"`` moves the n^2-sized layer steps of that route onto HIP kernels too, ``"full"`` the
O(B D)-sized ones as well, ``"native"`` the H layer's MLP and the head too.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import Cfg
from .options import Options

HIDDEN = 128   # PeakSearchLayer hidden_dim (admm_net.py:496)
HEADS = 4


def _no_forward(self, *a, **k):
    raise NotImplementedError(
        f"{type(self).__name__} is a parameter container: the layer is executed inside the fused "
        "HIP forward of ADMMNet / PhiEstADMMNet (include/admmnet.h)")


class PhiLayer(nn.Module):
    """Parameters of admm_net.py:71-105."""
    def __init__(self, epsilon=1e-8):
        super().__init__()
        self.rho = nn.Parameter(torch.tensor(1.0))
        self.epsilon = epsilon
    forward = _no_forward


class HLayer(nn.Module):
    """Parameters of admm_net.py:108-205."""
    def __init__(self, M, N, epsilon=1e-8):
        super().__init__()
        self.M, self.N = M, N
        self.dim = M * N
        self.epsilon = epsilon
        self.rho = nn.Parameter(torch.tensor(1.0))
        self.projection_weight = nn.Parameter(torch.tensor(1.0))
        self.correction_net = nn.Sequential(nn.Linear(self.dim, 64), nn.ReLU(),
                                            nn.Linear(64, self.dim), nn.Tanh())
    forward = _no_forward


class GLayer(nn.Module):
    """Parameters of admm_net.py:208-354."""
    def __init__(self, M, N, epsilon=1e-8):
        super().__init__()
        self.M, self.N = M, N
        self.dim = M * N + 1
        self.epsilon = epsilon
        self.lambda_param = nn.Parameter(torch.tensor(0.1))
        self.rho = nn.Parameter(torch.tensor(1.0))
        self.threshold = nn.Parameter(torch.tensor(0.0))
        self.value_net = nn.Sequential(nn.Linear(1, 16), nn.ReLU(), nn.Linear(16, 1), nn.Sigmoid())
    forward = _no_forward


class ZLayer(nn.Module):
    """Parameters of admm_net.py:357-490 (step_adjust_net is unused by forward but is in the state_dict)."""
    def __init__(self, M, N, epsilon=1e-8):
        super().__init__()
        self.M, self.N = M, N
        self.dim_h = M * N
        self.dim_z = M * N + 1
        self.epsilon = epsilon
        self.rho = nn.Parameter(torch.tensor(1.0))
        self.lambda_param = nn.Parameter(torch.tensor(1.0))
        self.residual_scale_net = nn.Sequential(nn.Linear(3, 32), nn.ReLU(), nn.Linear(32, 1), nn.Sigmoid())
        self.step_adjust_net = nn.Sequential(nn.Linear(3, 8), nn.ReLU(), nn.Linear(8, 1), nn.Sigmoid())
    forward = _no_forward


class PeakSearchLayer(nn.Module):
    """Parameters of admm_net.py:494-630."""
    def __init__(self, M, N, L=3, hidden_dim=HIDDEN, num_heads=HEADS):
        super().__init__()
        if hidden_dim != HIDDEN or num_heads != HEADS:
            raise ValueError("the HIP head is built for hidden_dim=128, num_heads=4 (reference defaults)")
        self.M, self.N, self.L_max = M, N, L
        self.dim = M * N
        self.feature_extractor = nn.Sequential(nn.Linear(2 * self.dim, hidden_dim), nn.ReLU(),
                                               nn.Linear(hidden_dim, hidden_dim), nn.ReLU())
        tau_grid = torch.linspace(0, 1, M)
        f_grid = torch.linspace(-0.5, 0.5, N)
        tg, fg = torch.meshgrid(tau_grid, f_grid, indexing="ij")
        self.position_encoder = nn.Parameter(torch.stack([tg.flatten(), fg.flatten()], dim=1), requires_grad=True)
        self.position_projection = nn.Linear(2, hidden_dim)
        self.attention = nn.MultiheadAttention(embed_dim=hidden_dim, num_heads=num_heads, batch_first=True,
                                               dropout=0.1)
        self.peak_extractor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(),
                                            nn.Linear(hidden_dim // 2, hidden_dim // 4), nn.ReLU(),
                                            nn.Linear(hidden_dim // 4, hidden_dim // 8), nn.ReLU())
        self.tau_regressor = nn.ModuleList([
            nn.Sequential(nn.Linear(hidden_dim // 8, 32), nn.ReLU(), nn.Linear(32, 1), nn.Sigmoid())
            for _ in range(L)])
        self.f_regressor = nn.ModuleList([
            nn.Sequential(nn.Linear(hidden_dim // 8, 32), nn.ReLU(), nn.Linear(32, 1), nn.Tanh())
            for _ in range(L)])
        self.confidence_net = nn.Sequential(nn.Linear(hidden_dim // 8, 16), nn.ReLU(), nn.Linear(16, 1),
                                            nn.Sigmoid())
    forward = _no_forward


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class _FusedBase(nn.Module):
    _HAS_HEAD = False

    def __init__(self, M, N, L=3, num_layers=10):
        super().__init__()
        self.num_layers = num_layers
        self.M, self.N, self.L = M, N, L
        self.phiLayers = nn.ModuleList([PhiLayer() for _ in range(num_layers)])
        self.hLayers = nn.ModuleList([HLayer(M, N) for _ in range(num_layers)])
        self.gLayers = nn.ModuleList([GLayer(M, N) for _ in range(num_layers)])
        self.zLayers = nn.ModuleList([ZLayer(M, N) for _ in range(num_layers)])
        if self._HAS_HEAD:
            self.peakSearchLayer = PeakSearchLayer(M, N, L)
        # execution knobs (not part of the reference API)
        self._chunk = 0                # signals per eigensolver chunk (0 = library default); see the `chunk` property
        self._sub_batch = None         # signals per independent sub-batch (None = the call is one batch); see `sub_batch`
        self._options = None           # per-model kernel routes and tolerances (None = the process defaults); see `options`
        self._train_route = "tensor"   # how the differentiable forward evaluates the n^2-sized layer steps; see `train_route`
        self.check_status = True       # one D2H read per forward: raise if the eigensolver failed
        self._wcache = None
        self._ws = None

    @property
    def chunk(self) -> int:
        """Signals per eigensolver work chunk (0 = library default, 8192).  Setting it drops the cached workspace: its
        carve depends on the chunk size."""
        return self._chunk

    @chunk.setter
    def chunk(self, value: int):
        value = int(value)
        if value < 0:
            raise ValueError("chunk must be >= 0")
        if value != self._chunk:
            self._chunk = value
            self._ws = None

    @property
    def sub_batch(self) -> Optional[int]:
        """Signals per independent sub-batch (None = the whole call is one batch, the reference's semantics).  With g set,
        a call on B signals evaluates the consecutive groups [i g, min((i + 1) g, B)) -- the last one may be shorter --
        each with its own batch mean (admm_net.py:459), and every group gets exactly the outputs a separate call on it
        returns: g = 256 reproduces the reference's DataLoader batches, g = 1 its single-signal scripts.  Honoured by the
        fused forward, by ``forward_autograd`` and by ``sharded.ShardedForward``.  Not part of the state_dict.  Setting it
        drops the cached workspace."""
        return self._sub_batch

    @sub_batch.setter
    def sub_batch(self, value: Optional[int]):
        if value is not None:
            if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= 2 ** 31 - 1:
                raise ValueError(f"sub_batch must be None or an int >= 1, got {value!r}")
            value = int(value)
        if value != self._sub_batch:
            self._sub_batch = value
            self._ws = None

    @property
    def options(self) -> Optional[Options]:
        """Kernel routes and tolerances of THIS model: an ``Options`` of overrides over the process defaults (the
        ``ADMMNET_*`` environment), or None for the defaults themselves.  Everything that takes its ``cfg`` from the model
        follows -- the fused forward, ``estimate``, ``ops.glayer``, ``ops.glayer_spectral``, ``sharded.HipLayerEngine`` and
        ``ShardedForward`` -- and so does the eigensolver of ``forward_autograd``; other models of the process are not
        affected.  Not part of the state_dict; pickled and deep-copied with the module (as its overrides: a new process
        interns them again).  Setting it drops the cached workspace: its carve depends on the route."""
        return getattr(self, "_options", None)

    @options.setter
    def options(self, value: Optional[Options]):
        if value is not None and not isinstance(value, Options):
            raise TypeError(f"options must be None or an admm_net_amd.Options, got {type(value).__name__}")
        self._options = value
        self._ws = None

    @property
    def train_route(self) -> str:
        """How the differentiable forward (train mode, ``forward_autograd``) evaluates the n^2-sized steps of a layer:
        ``"tensor"`` (default) as framework tensor operations, ``"fused"`` through the streaming HIP kernels of
        csrc/train_layer.hip with hand-written backwards (``training.LayerKernels``), ``"full"`` as ``"fused"`` and with the
        O(B D)-sized steps -- phi layer, H layer around its correction_net, eigenvalue map, step-size network -- on the kernels
        of csrc/train_small.hip too (``training.SmallKernels``), ``"native"`` as ``"full"`` and with the whole H layer, its
        correction_net included, on the kernels of csrc/train_hlayer.hip and ``ADMMNet``'s PeakSearchLayer head on those of
        csrc/train_head.hip (``training.NativeKernels``); on this route the head's attention dropout draws its keep mask with
        one ``torch.rand`` call, so under the same seed it drops other entries than the other routes do (same distribution).
        All use the HIP eigensolver and contractions; inference is not affected.  Not part of the state_dict."""
        return self._train_route

    @train_route.setter
    def train_route(self, value: str):
        from .training import TRAIN_ROUTES
        if not isinstance(value, str) or value not in TRAIN_ROUTES:
            raise ValueError(f"train_route must be one of {TRAIN_ROUTES}, got {value!r}")
        self._train_route = value

    # ---- weights -----------------------------------------------------------
    def cfg(self) -> Cfg:
        opt = self.options
        return Cfg(self.M, self.N, self.L, self.num_layers, int(self._HAS_HEAD), int(self.chunk),   # reserved[0] = admmnet_cfg.sub_batch,
                   (ctypes.c_int32 * 2)(self.sub_batch or 0, 0 if opt is None else opt.handle))    # [1] = its option handle

    def _raw_params(self):
        """Parameters in the raw order documented in include/admmnet.h."""
        out = []
        for k in range(self.num_layers):
            hl, gl, zl = self.hLayers[k], self.gLayers[k], self.zLayers[k]
            out += [self.phiLayers[k].rho, hl.rho, hl.projection_weight,
                    hl.correction_net[0].weight, hl.correction_net[0].bias,
                    hl.correction_net[2].weight, hl.correction_net[2].bias,
                    gl.lambda_param, gl.rho, gl.threshold,
                    gl.value_net[0].weight, gl.value_net[0].bias, gl.value_net[2].weight, gl.value_net[2].bias,
                    zl.rho, zl.lambda_param,
                    zl.residual_scale_net[0].weight, zl.residual_scale_net[0].bias,
                    zl.residual_scale_net[2].weight, zl.residual_scale_net[2].bias]
        if self._HAS_HEAD:
            p = self.peakSearchLayer
            out += [p.position_encoder, p.feature_extractor[0].weight, p.feature_extractor[0].bias,
                    p.feature_extractor[2].weight, p.feature_extractor[2].bias,
                    p.position_projection.weight, p.position_projection.bias,
                    p.attention.in_proj_weight, p.attention.in_proj_bias,
                    p.attention.out_proj.weight, p.attention.out_proj.bias]
            for i in (0, 2, 4):
                out += [p.peak_extractor[i].weight, p.peak_extractor[i].bias]
            for t in range(self.L):
                out += [p.tau_regressor[t][0].weight, p.tau_regressor[t][0].bias,
                        p.tau_regressor[t][2].weight, p.tau_regressor[t][2].bias,
                        p.f_regressor[t][0].weight, p.f_regressor[t][0].bias,
                        p.f_regressor[t][2].weight, p.f_regressor[t][2].bias]
            out += [p.confidence_net[0].weight, p.confidence_net[0].bias,
                    p.confidence_net[2].weight, p.confidence_net[2].bias]
        return out

    def packed_weights(self, device) -> torch.Tensor:
        """Host-pack (admmnet_pack_weights) and upload; cached until a parameter changes."""
        lib = _lib.load()
        params = self._raw_params()
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        if self._wcache is not None and self._wcache[0] == key:
            return self._wcache[1]
        cfg = self.cfg()
        raw = torch.cat([p.detach().to("cpu", torch.float32).reshape(-1) for p in params]).contiguous()
        nraw = lib.admmnet_raw_weight_count(ctypes.byref(cfg))
        if nraw != raw.numel():
            raise _lib.AdmmNetError(f"raw weight count mismatch: library {nraw}, module {raw.numel()}")
        packed = torch.empty(lib.admmnet_packed_weight_count(ctypes.byref(cfg)), dtype=torch.float32)
        _lib.check(lib.admmnet_pack_weights(ctypes.byref(cfg), _ptr(raw), _ptr(packed)), "admmnet_pack_weights")
        dev = packed.to(device)
        self._wcache = (key, dev)
        return dev

    def workspace(self, B: int, device) -> torch.Tensor:
        lib = _lib.load()
        cfg = self.cfg()
        need = lib.admmnet_workspace_bytes(ctypes.byref(cfg), B)
        if need < 0:
            _lib.check(-1, "admmnet_workspace_bytes")
        if self._ws is None or self._ws.numel() < need or self._ws.device != torch.device(device):
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    # ---- forward -------------------------------------------------------------
    @staticmethod
    def _compute_device(y: torch.Tensor) -> torch.device:
        if y.is_cuda:
            return y.device
        if not torch.cuda.is_available():
            raise _lib.AdmmNetError("no HIP device: the ADMM-Net forward runs only on the GPU (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def _run(self, y, b, sigma, to_caller=True):
        lib = _lib.load()
        dev = self._compute_device(y)
        D = self.M * self.N
        if y.dim() != 2 or y.shape[1] != D or b.shape != y.shape:
            raise ValueError(f"y, b must be [B, {D}] complex; got {tuple(y.shape)}, {tuple(b.shape)}")
        B = y.shape[0]
        yd, bd = ops._c64(y, dev, (B, D), "y"), ops._c64(b, dev, (B, D), "b")   # the one place a caller's tensor becomes a pointer
        sd = ops._f32(sigma.reshape(-1), dev, None, "sigma")
        if sd.numel() != B:
            raise ValueError("sigma must have one entry per signal")
        with torch.cuda.device(dev):
            W = self.packed_weights(dev)
            ws = self.workspace(B, dev)
            phi = torch.empty(B, D, dtype=torch.complex64, device=dev)
            head = torch.empty(3, B, self.L, dtype=torch.float32, device=dev) if self._HAS_HEAD else None
            status = torch.zeros(4, dtype=torch.int32, device=dev)
            cfg = self.cfg()
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = lib.admmnet_forward_f32(ctypes.byref(cfg), _ptr(W), _ptr(yd), _ptr(bd), _ptr(sd), B, _ptr(phi),
                                         _ptr(head), _ptr(ws), ws.numel(), _ptr(status), stream)
            _lib.check(rc, "admmnet_forward_f32")
            if self.check_status:
                # [0] eigensolver failures; with ADMMNET_SPECTRAL=1: [1] matrix-layers that took the eigensolver after all,
                # [2] matrix-layers evaluated as a matrix function (csrc/spectral.hip)
                self.last_status = status.tolist()
                bad = int(self.last_status[0])
                if bad:
                    raise _lib.AdmmNetError(f"eigensolver failed to converge on {bad} matrices")
        if not to_caller:
            return phi, head   # still on the compute device
        out_dev = y.device
        phi = phi.to(out_dev)
        if head is not None:
            head = head.to(out_dev)
        return phi, head

    # ---- estimation ----------------------------------------------------------
    def estimate(self, y, b, sigma, top=None, top_n=None, opts=None, xbase=None, ybase=None):
        """The inference flow of main_for_net.py:99-126 / test/test_model_peaksearch.py:79-96 in one call: the forward,
        alt_peak_search on its phi, the rows sorted by refined height and cut -- all on the device (``ops.peak_top``);
        only the results below go back to ``y.device``.

        Runs the inference forward under ``torch.no_grad()`` whatever the training flag (``chunk``, ``sub_batch`` and
        ``check_status`` act as in ``forward``).  Defaults are main_for_net.py:107-116 read literally: ``top = self.L``,
        ``xbase = self.M``, ``ybase = self.N``, ``opts = {'xstep': 1 / (10 * N), 'ystep': 1 / (10 * M), 'iter': 3}``.
        ``top_n``: optional [B] integers, rows wanted per signal (the sample's L_true).

        Returns (tau [B, top], f [B, top], height [B, top] float64, rank order, NaN where a signal has fewer peaks;
        counts [B] int32, the number of regional maxima; phi [B, M*N] complex64)."""
        rows, counts, phi = self._estimate_rows(y, b, sigma, top, top_n, opts, xbase, ybase)
        out = y.device
        return (rows[:, :, 0].contiguous().to(out), rows[:, :, 1].contiguous().to(out),
                rows[:, :, 2].contiguous().to(out), counts.to(out), phi.to(out))

    def _estimate_rows(self, y, b, sigma, top=None, top_n=None, opts=None, xbase=None, ybase=None):
        """``estimate`` up to its device results: (rows [B, top, 3] float64, counts [B] int32, phi) on the compute device."""
        top = self.L if top is None else top
        xbase = self.M if xbase is None else xbase
        ybase = self.N if ybase is None else ybase
        if opts is None:
            opts = {"xstep": 1 / (10 * self.N), "ystep": 1 / (10 * self.M), "iter": 3}
        with torch.no_grad():
            phi, _ = self._run(y, b, sigma, to_caller=False)
            rows, counts = ops.peak_top(phi, xbase, ybase, opts, top=top, top_n=top_n)
        return rows, counts, phi

    def estimate_refined(self, y, b, sigma, top=None, top_n=None, opts=None, *, symbols="given", **refine_kw):
        """``estimate`` followed by the stage every delay-Doppler estimator puts after the peak search: a local maximum-
        likelihood fit of the targets to the RECEIVED signal ``y``, started at the peaks (``refine.refine_targets``: one more
        kernel on the compute device, no host read).  ``top``, ``top_n`` and ``opts`` as in ``estimate`` (``top`` <= 16);
        ``symbols``: "given" (s = b / |b|) or "psk" (the symbols re-decided inside the fit); ``refine_kw``: ``psk``, ``iters``,
        ``tol`` of ``refine_targets``.

        Returns (tau [B, top], f [B, top], amplitude [B, top] = |C| float64, in the peak search's rank order, NaN where a
        signal has fewer peaks; C [B, top] complex128; counts [B] int32; phi [B, M*N] complex64; state [B] int32, the index
        into ``refine.STATES``) on ``y.device``."""
        from . import refine
        rows, counts, phi = self._estimate_rows(y, b, sigma, top, top_n, opts)
        dev, out = rows.device, y.device
        r = refine.refine_targets(y.to(dev), b.to(dev), rows, (self.M, self.N), symbols=symbols, **refine_kw)
        return (r.rows[:, :, 0].contiguous().to(out), r.rows[:, :, 1].contiguous().to(out), r.rows[:, :, 2].contiguous().to(out),
                r.C.to(out), counts.to(out), phi.to(out), r.state.to(out))

    def estimate_selected(self, y, b, sigma, top=None, opts=None, *, rounds=2, grow=0, symbols="given", penalty=None, **refine_kw):
        """``estimate`` for an UNKNOWN number of targets: ``top`` candidate peaks (None: min(2 L, 16)) go through the selection-
        and-refinement loop of ``order.select_refined`` -- the candidates ranked against the received signal ``y``, their number
        chosen by a penalised log residual, the chosen ones fitted, ``rounds`` times, ``grow`` more times with the highest peak
        of the residual added -- on the compute device, without a host read.  ``opts`` as in ``estimate``; ``symbols``,
        ``penalty`` and ``refine_kw`` as in ``select_refined``.

        Returns (tau [B, top], f [B, top], amplitude [B, top] = |C| float64, NaN past n_sel; C [B, top] complex128; n_sel [B]
        int32, the number of targets selected; counts [B] int32; phi [B, M*N] complex64; state [B] int32: 0, or the code of
        ``refine.STATES`` for a scene that was not ranked) on ``y.device``."""
        from . import order
        top = min(2 * self.L, 16) if top is None else top
        rows, counts, phi = self._estimate_rows(y, b, sigma, top, None, opts)
        dev, out = rows.device, y.device
        sel, _ = order.select_refined(y.to(dev), b.to(dev), rows, (self.M, self.N), rounds=rounds, grow=grow, symbols=symbols,
                                      penalty=penalty, **refine_kw)
        chosen = (torch.arange(rows.shape[1], device=dev)[None, :] < sel.n_sel[:, None])
        est = torch.where(chosen[:, :, None], sel.rows_out, torch.full_like(sel.rows_out, float("nan")))
        return (est[:, :, 0].contiguous().to(out), est[:, :, 1].contiguous().to(out), est[:, :, 2].contiguous().to(out),
                sel.C.to(out), sel.n_sel.to(out), counts.to(out), phi.to(out), sel.state.to(out))

    def evaluate(self, y, b, sigma, tau_true, f_true, L_true=None, *, cutoff, scale=None, period=(1.0, 1.0), top=None, opts=None):
        """``estimate`` scored against the truth in one call: the forward, the peak search, the top rows and the optimal
        assignment of ``metrics.match_targets`` run on the device with no host loop and, with ``check_status = False``, no host
        read; the rows never leave it.  ``top`` and ``opts`` as in ``estimate``; tau_true, f_true [B, Lt] and L_true as in
        ``match_targets`` (moved to the compute device if they are elsewhere); ``cutoff`` in units of ``scale``.

        ``scale = None`` means one resolution cell per axis, the length of that axis's steering vector: in the signal model
        (synth.py:47-48, ``make_batch(B, M, N)``) tau's steering vector has N entries and f's has M, and the flattening
        index = i_f N + i_tau is the ``phi.reshape(ybase, xbase)`` of peak_search.py with x = tau, so scale = (N, M) -- a
        distance of 1 is one cell of the tau axis (1 / N) or of the f axis (1 / M).  (``estimate``'s default bases read
        main_for_net.py literally, xbase = M; on the square grids the reference uses the two are the same.)
        ``period = (1.0, 1.0)``: both axes are periodic with period 1, as the steering vectors are.

        Returns a ``metrics.MatchResult`` of device tensors; ``metrics.summary`` reads it."""
        from . import metrics
        rows, _, _ = self._estimate_rows(y, b, sigma, top, None, opts)
        dev = rows.device
        if scale is None:
            scale = (float(self.N), float(self.M))
        tau_true, f_true = tau_true.to(dev), f_true.to(dev)
        if L_true is not None:
            L_true = L_true.to(dev)
        return metrics.match_targets(rows, tau_true, f_true, L_true, cutoff=cutoff, scale=scale, period=period)

    # ---- training ----------------------------------------------------------
    def forward_autograd(self, y, b, sigma, reducer=None):
        """Differentiable forward (what ``forward`` does in train mode); usable in eval mode too, e.g. to
        take gradients without the attention dropout.  The parameters must live on the GPU.  ``reducer``: the all-reduce of a
        batch-sharded step (``sharded.ShardedTraining``, ``training.unrolled_forward``); None: the call is the whole batch."""
        from . import training
        _lib.load()                                   # fail loudly without the HIP library
        dev = self._compute_device(y)
        pdev = next(self.parameters()).device
        if pdev != dev:
            raise _lib.AdmmNetError(f"training runs on the GPU: parameters are on {pdev}, expected {dev} "
                                    "(move the model with .to(device) as train.py / trainPhi.py do)")
        out = training.unrolled_forward(self, y.to(dev), b.to(dev), sigma.to(dev), sub_batch=self.sub_batch, reducer=reducer,
                                        **training.route_kwargs(self.train_route))
        if isinstance(out, tuple):
            return tuple(o.to(y.device) for o in out)
        return out.to(y.device)

    def _wants_grad(self) -> bool:
        return self.training and torch.is_grad_enabled()


class PhiEstADMMNet(_FusedBase):
    """admm_net.py:724-764: K unrolled ADMM layers, returns phi [B, M*N] complex64."""
    _HAS_HEAD = False

    def forward(self, y, b, sigma):
        if self._wants_grad():
            return self.forward_autograd(y, b, sigma)
        phi, _ = self._run(y, b, sigma)
        return phi


class ADMMNet(_FusedBase):
    """admm_net.py:767-816: unrolled layers + PeakSearchLayer; returns (tau, f, confidences, phi)."""
    _HAS_HEAD = True

    def forward(self, y, b, sigma):
        if self._wants_grad():
            return self.forward_autograd(y, b, sigma)
        phi, head = self._run(y, b, sigma)
        return head[0], head[1], head[2], phi

    def _head_rows(self, y, b, sigma, threshold):
        """``estimate_head`` on the compute device."""
        with torch.no_grad():
            phi, head = self._run(y, b, sigma, to_caller=False)
            return HeadEstimate(*order_by_confidence(head[0], head[1], head[2], threshold), phi)

    def estimate_head(self, y, b, sigma, threshold=0.5):
        """The learned head's own estimate, for a head trained with ``losses.SetANMLoss`` (matched slots learn conf -> 1, the
        others conf -> 0, so the confidences say how many targets there are): the inference forward under ``torch.no_grad()``,
        then plain tensor operations on the compute device, no host read.

        Returns a ``HeadEstimate`` on ``y.device``: tau, f, conf [B, L] float32 ordered by descending ``conf`` (stable: equal
        values keep slot order); n_est [B] int32, the number of slots with ``conf >= threshold``, so the first n_est rows are
        the estimate; phi [B, M*N] complex64."""
        return HeadEstimate(*(t.to(y.device) for t in self._head_rows(y, b, sigma, threshold)))

    def evaluate_head(self, y, b, sigma, tau_true, f_true, L_true=None, *, cutoff, threshold=0.5, scale=None, period=(1.0, 1.0)):
        """``estimate_head`` scored against the truth: ``metrics.match_targets`` of its rows with ``n_est`` from the confidences,
        on the device.  ``cutoff``, ``scale`` (None: one resolution cell per axis, (N, M)) and ``period`` as in ``evaluate``.
        Returns a ``metrics.MatchResult`` of device tensors."""
        from . import metrics
        e = self._head_rows(y, b, sigma, threshold)
        dev = e.tau.device
        if scale is None:
            scale = (float(self.N), float(self.M))
        return metrics.match_targets((e.tau, e.f), tau_true.to(dev), f_true.to(dev), None if L_true is None else L_true.to(dev),
                                     n_est=e.n_est, cutoff=cutoff, scale=scale, period=period)


class HeadEstimate(NamedTuple):
    tau: torch.Tensor      # [B, L] float32, by descending confidence
    f: torch.Tensor        # [B, L] float32
    conf: torch.Tensor     # [B, L] float32
    n_est: torch.Tensor    # [B] int32: the slots with conf >= threshold
    phi: torch.Tensor      # [B, M*N] complex64


def order_by_confidence(tau, f, conf, threshold=0.5):
    """(tau, f, conf [B, L] ordered by descending ``conf``, equal values in slot order; n_est [B] int32 = the number of slots
    with ``conf >= threshold``).  Tensor operations only: no host read."""
    order = torch.sort(conf, dim=1, descending=True, stable=True).indices
    n_est = (conf >= threshold).sum(dim=1).to(torch.int32)
    return tau.gather(1, order), f.gather(1, order), conf.gather(1, order), n_est
