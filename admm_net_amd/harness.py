"""Timing harnesses and checkpoint I/O in the reference's own formats.

* ``time_net`` / ``time_admm`` are the MI355X-path equivalents of /root/reference/test/test_time_net.py:10-137 and
  /root/reference/test/test_time_admm.py:7-110: the same 10 x 10 demo scene with fresh noise per run, one
  ``time.perf_counter`` bracket around one call, ``np.savetxt`` of the list -- so the files drop into
  /root/reference/results/plot_compute_time.py next to ``time.txt`` / ``time_net.txt`` / ``time_net_5.txt``.
* ``save_checkpoint`` / ``load_checkpoint`` write and read the dict of /root/reference/train.py:306-314
  (``epoch, model_state_dict, optimizer_state_dict, scheduler_state_dict, best_val_loss, config, history``) that
  ``main_for_net.py:100-101`` and ``train.py:137-145`` load.

CLI:  python -m admm_net_amd.harness time-net  --layers 5 --runs 1000 --out time_net_5.txt [--checkpoint best_model.pth]
      python -m admm_net_amd.harness time-admm --runs 1000 --out time.txt
      python -m admm_net_amd.harness train-step --layers 10 --batch 256 --steps 20 [--route fused|full|native] [--grid 16x16] [--optim hip]   (one JSON line)
      python -m torch.distributed.run --nproc-per-node N -m admm_net_amd.harness train-step ...   (the step through sharded.ShardedTraining; --batch per rank; rank 0's line gains n_ranks, global_batch)
      python -m admm_net_amd.harness loss-step --batch 256 --targets 3 --dim 100 --steps 200                              (one JSON line)
      python -m admm_net_amd.harness score-step [--steps 50] [--repeats 5] [--host-signals 2048]                          (one JSON line)
      python -m admm_net_amd.harness cfar-step [--signals 4096] [--grid 16x16] [--oversample 4] [--steps 50] [--cancel [--sweeps S] [--newton I]]   (one JSON line)
      python -m admm_net_amd.harness evaluate --grid 10x10 --layers 10 [--checkpoint P] --snr 5 15 25 --signals 4096 --targets 3 --cutoff 1.0 [--baseline classical|periodogram [--cfar ca|os|known] [--pfa P] [--cancel [--sweeps S] [--newton I]]] [--refine given|psk] [--crb] [--order TOP]
                                                                                                    (one JSON line per SNR and method)
"""
from __future__ import annotations

import argparse
import contextlib
import io
import math
import time

import numpy as np
import torch

from . import classical
from .synth import pskdemod, pskmod, steering
from .training import TRAIN_ROUTES

NB = ND = 10
F = np.array([-0.25, 0, 0.14])                       # test_time_net.py:16-18
TAU = np.array([0.45, 0.25, 0.63])
C = np.array([-0.5 + 1j, 0.6 - 0.2j, 0.3 + 0.7j])


def demo_scene(rng, sig=None, e=None, data_type=0, snr_e=7.0, snr_w=20.0):
    """One draw of the scene both timing scripts build per run (test_time_net.py:13-92, test_time_admm.py:11-82):
    ``data_type`` 0 = fresh QPSK symbols, 1 = fixed ``sig`` + fresh demodulation noise, 2 = fixed ``sig`` and ``e``
    (the two arrays of data/data.npz).  Returns (y [100, 1], b [100], sigma) in float64 / complex128."""
    S, Dm = steering(F, NB), steering(TAU, ND)
    Psi = np.einsum("l,li,lj->ij", C, S, np.conj(Dm)).reshape(NB * ND, 1)
    if data_type == 0:
        sig = pskmod(rng.integers(0, 4, NB * ND), 4, np.pi / 4)
    if data_type in (0, 1):
        p = np.mean(np.abs(sig) ** 2) / (10 ** (snr_e / 10))
        sig_n = sig + np.sqrt(p / 2) * (rng.standard_normal(len(sig)) + 1j * rng.standard_normal(len(sig)))
        b = pskmod(pskdemod(sig_n, 4, np.pi / 4), 4, np.pi / 4)
        e = sig - b
    else:
        b = sig - e
    real_y = np.diag(b + e) @ Psi
    w = np.sqrt(1 / 2) * (rng.standard_normal((NB * ND, 1)) + 1j * rng.standard_normal((NB * ND, 1)))
    w_var = np.linalg.norm(real_y) ** 2 / (10 ** (snr_w / 10) * NB * ND)
    y = real_y + np.sqrt(w_var) * w
    sigma = np.linalg.norm(e / b) + 1
    return y, b, sigma


def time_net(model, runs=1000, out_path=None, seed=0, sig=None, e=None, data_type=0, verbose=False):
    """test_time_net.py:94-102,131-137: per run a fresh scene, CPU tensors in (as the script passes them), one bracket
    around ``model(y, b, sigma)`` -- which includes the host-to-device copies and the result's return to the CPU, as
    it does for the reference module.  Returns the list of seconds; writes it with ``np.savetxt`` when ``out_path``."""
    rng = np.random.default_rng(seed)
    model.eval()
    times = []
    for i in range(runs):
        y, b, sigma = demo_scene(rng, sig, e, data_type)
        ty = torch.from_numpy(y.flatten().reshape(1, -1)).to(torch.complex64)
        tb = torch.from_numpy(b.reshape(1, -1)).to(torch.complex64)
        ts = torch.from_numpy(np.asarray(sigma).reshape(1, -1)).to(torch.float32)
        start = time.perf_counter()
        phi = model(ty, tb, ts)
        if phi.is_cuda:                         # (GPU tensors in: wait for the result, as .numpy() would)
            torch.cuda.synchronize(phi.device)
        end = time.perf_counter()
        times.append(end - start)
        if verbose:
            print(f"Time: {end - start:.6f} s ")
    if out_path:
        np.savetxt(out_path, times)
    return times


def time_admm(runs=1000, out_path=None, seed=0, sig=None, e=None, data_type=0, verbose=False):
    """test_time_admm.py:85-94,104-110 with the classical solver of admm_net_amd.classical (host, complex128)."""
    rng = np.random.default_rng(seed)
    opts = {"eta_abs": 1e-7, "eta_rel": 1e-7, "max_iter": 100}
    times = []
    for i in range(runs):
        y, b, sigma = demo_scene(rng, sig, e, data_type)
        sink = contextlib.nullcontext() if verbose else contextlib.redirect_stdout(io.StringIO())
        with sink:
            start = time.perf_counter()
            classical.admm_for_us(y, b, ND, NB, 1, sigma, opts)
            end = time.perf_counter()
        times.append(end - start)
    if out_path:
        np.savetxt(out_path, times)
    return times


def save_checkpoint(path, model, optimizer=None, scheduler=None, epoch=0, best_val_loss=float("inf"), config=None,
                    history=None):
    """The dict train.py:306-314 / trainPhi.py:238-246 save on every validation improvement."""
    torch.save({
        "epoch": epoch,
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else {},
        "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else {},
        "best_val_loss": best_val_loss,
        "config": config if config is not None else {},
        "history": history if history is not None else {},
    }, path)


def _numpy_scalar_globals():
    """What pickle needs to rebuild a numpy scalar (``np.float64`` ...): train.py:279-282 appends ``np.mean(...)`` results
    to ``history['tau_rmse']`` / ``['f_rmse']`` and saves ``history`` in the checkpoint (train.py:306-314).  These three
    reconstruct plain numbers and run nothing from the file, so the loader stays ``weights_only=True``."""
    try:
        from numpy._core import multiarray as ma          # numpy >= 2
    except ImportError:                                    # numpy 1.x
        from numpy.core import multiarray as ma
    kinds = {type(np.dtype(t)) for t in ("float64", "float32", "float16", "int64", "int32", "bool", "complex64",
                                         "complex128")}
    return [ma.scalar, np.dtype] + sorted(kinds, key=lambda k: k.__name__)


def load_checkpoint(path, model, optimizer=None, scheduler=None, map_location="cpu"):
    """train.py:137-145 (resume) / main_for_net.py:100-101 (inference).  Checkpoints written by train.py / trainPhi.py
    are dicts of tensors, plain Python values and numpy scalars (the RMSE history): the no-code loader with numpy
    scalar reconstruction allowed reads them; anything else in the file is refused (never ``weights_only=False``).
    Returns the dict."""
    with torch.serialization.safe_globals(_numpy_scalar_globals()):
        ckpt = torch.load(path, map_location=map_location, weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])
    if optimizer is not None and ckpt.get("optimizer_state_dict"):
        optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    if scheduler is not None and ckpt.get("scheduler_state_dict"):
        scheduler.load_state_dict(ckpt["scheduler_state_dict"])
    return ckpt


def time_train_step(layers=10, batch=256, steps=20, warmup=3, seed=0, device="cuda:0", route="tensor", grid=(NB, ND), head=False,
                    optim="torch", loss=None, targets=None, min_sep=0.0, checkpoint=None):
    """Wall time of one optimisation step at the reference's own training configuration (trainPhi.py:16-38: 10 x 10 grid,
    num_layers = 10, batch_size = 256, AdamW lr 1e-3 / weight decay 1e-3, gradient clipping at 1.0, :179-190): forward in
    train mode (the differentiable route of admm_net_amd.training: HIP eigensolver + HIP contractions), a phi-alignment
    loss against the classical solver's phi labels (generated on the device, csrc/synth.hip), backward, clip, step.
    The loss is a plain normalised squared error: the reference's loss.py is user code outside this path.
    ``route``: ``model.train_route`` (one of ``training.TRAIN_ROUTES``); ``grid`` = (M, N) of another geometry, same recipe.
    ``head = True`` times ``ADMMNet`` (the model of train.py) instead: the loss is then that phi error plus the plain squared
    error of tau and f against the generator's labels.
    ``optim``: "torch" (``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.AdamW``) or "hip": ``admm_net_amd.optim.AdamW`` with
    ``max_grad_norm=1.0``, the clipping inside the update (csrc/optim.hip).
    Under ``torch.distributed.run`` (WORLD_SIZE > 1; backend ADMMNET_DIST_BACKEND, default nccl = RCCL) every rank takes a batch
    of ``batch`` signals of its own and the step runs through ``sharded.ShardedTraining``: the mean loss times ``st.weight``, one
    gradient all-reduce.  The dict then holds ``n_ranks`` and ``global_batch``; ``signals_per_second`` counts the global batch.
    ``loss`` (with ``head=True``): None, the loss above; "set" (``losses.SetANMLoss``) or "basic" (``losses.BasicANMLoss``), each
    with ``check_status = False``, on scenes of ``synth.make_scenes_device(targets=(lo, hi), min_sep=...)`` (``targets``: a pair,
    default (1, 3)) -- a fresh batch of scenes every step, drawn on the device.  ``checkpoint``: a path the model is saved to
    after the last step (``save_checkpoint``).  Not combined with a sharded run.
    Returns a dict (seconds per step, signals per second, route, geometry)."""
    import os
    import torch.distributed as dist
    from . import ADMMNet, PhiEstADMMNet, sharded, synth
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()     # (rehearsals put several ranks on one GPU)
        torch.cuda.set_device(local)
        device = f"cuda:{local}"
        if not dist.is_initialized():
            backend = os.environ.get("ADMMNET_DIST_BACKEND", "nccl")
            kw = {"device_id": torch.device(device)} if backend == "nccl" else {}
            dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    dev = torch.device(device)
    torch.manual_seed(seed)
    M, N = grid
    if loss not in (None, "set", "basic"):
        raise ValueError(f"loss must be None, 'set' or 'basic', got {loss!r}")
    if loss is None and (targets is not None or min_sep != 0.0):
        raise ValueError("targets= and min_sep= go with loss='set' or loss='basic'")
    if loss is not None and (not head or world > 1):
        raise ValueError("loss= needs head=True and a single process")
    lo, hi = (1, 3) if targets is None else synth._target_range(targets)
    model = (ADMMNet if head else PhiEstADMMNet)(num_layers=layers, M=M, N=N, L=hi if loss else 3).to(dev)
    model.train_route = route
    model.train()
    if optim not in ("torch", "hip"):
        raise ValueError(f"optim must be 'torch' or 'hip', got {optim!r}")
    if optim == "hip":
        from . import optim as hip_optim
        opt = hip_optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-3)
    y, b, sigma, extra = synth.make_batch_device(batch, M, N, seed=20260104 + seed + 7919 * rank, device=dev, labels=True)
    label = extra["phi"].to(torch.complex64)
    scale = label.abs().pow(2).mean()
    st = sharded.ShardedTraining(model) if world > 1 else None
    if st is not None:                                      # one normalisation for the whole batch
        dist.all_reduce(scale)
        scale = scale / world

    crit, drawn = None, [0]
    if loss is not None:
        from . import losses
        crit = losses.SetANMLoss() if loss == "set" else losses.BasicANMLoss()
        crit.check_status = False

    def scene_step():
        opt.zero_grad(set_to_none=True)
        drawn[0] += 1
        ys, bs, ss, truth = synth.make_scenes_device(batch, M, N, targets=(lo, hi), min_sep=min_sep,
                                                     seed=20260104 + seed + 104729 * drawn[0], device=dev)
        tau, f, conf, phi = model(ys, bs, ss)
        total, _ = crit({"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi},
                        {"tau_true": truth["tau"], "f_true": truth["f"], "L_true": truth["L_true"]})
        total.backward()
        if optim == "torch":
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        return total

    def step():
        if crit is not None:
            return scene_step()
        opt.zero_grad(set_to_none=True)
        out = model(y, b, sigma) if st is None else st(y, b, sigma)
        if head:
            tau, f, _, phi = out
            loss = (phi - label).abs().pow(2).mean() / scale + (tau - extra["tau"]).pow(2).mean() + (f - extra["f"]).pow(2).mean()
        else:
            loss = (out - label).abs().pow(2).mean() / scale
        if st is None:
            loss.backward()
        else:
            st.backward(loss * st.weight)
        if optim == "torch":
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        return loss

    losses = []
    for _ in range(warmup):
        losses.append(float(step().item()))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    losses.append(float(last.item()))
    out = {"config": f"{type(model).__name__} {M}x{N} K={layers}, batch {batch}, AdamW + clip 1.0 (trainPhi.py:16-38, 179-190)",
           "route": route, "optim": optim, "head": bool(head), "grid": [M, N], "layers": layers, "batch": batch,
           "seconds_per_step": round(dt, 6), "signals_per_second": round(batch * world / dt, 1), "steps": steps,
           "loss_first": round(losses[0], 6), "loss_last": round(losses[-1], 6)}
    if st is not None:                                      # (the losses are this rank's mean, not the whole batch's)
        out.update(n_ranks=world, global_batch=st.global_batch)
    if loss is not None:
        out.update(loss=loss, targets=[lo, hi], min_sep=float(min_sep))
    if checkpoint:
        save_checkpoint(checkpoint, model, opt, epoch=warmup + steps, config={"M": M, "N": N, "num_layers": layers, "L": hi if loss else 3})
    return out


def time_loss_step(batch=256, targets=3, dim=100, steps=200, warmup=10, seed=0, device="cuda:0"):
    """Median wall time of one forward + backward of each loss of admm_net_amd.losses (``BasicANMLoss``, ``PhiAlignmentLoss``)
    on ``route = "hip"`` and ``route = "tensor"``, on synthetic device tensors: [batch, targets] head outputs and labels with
    L_true cycling through 0 .. targets, [batch, dim] complex phi.  Each step is bracketed by a device synchronisation, so a
    figure is the latency of the loss alone, as a training loop sees it between the model's forward and backward.
    Returns a dict of milliseconds per loss and route."""
    from . import losses
    dev = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g).to(dev)
    tau, f, conf = (r(batch, targets).requires_grad_(True) for _ in range(3))
    truth = {"tau_true": r(batch, targets), "f_true": r(batch, targets) - 0.5,
             "L_true": (torch.arange(batch) % (targets + 1)).to(dev)}
    phi = torch.randn(batch, dim, dtype=torch.complex64, generator=g).to(dev).requires_grad_(True)
    phi_true = torch.randn(batch, dim, dtype=torch.complex64, generator=g).to(dev)
    leaves = (tau, f, conf, phi)

    def median_ms(crit, call):
        times = []
        for i in range(warmup + steps):
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            total, _ = call(crit)
            total.backward()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                times.append(time.perf_counter() - t0)
        return round(float(np.median(times)) * 1e3, 4)

    out = {"batch": batch, "targets": targets, "dim": dim, "steps": steps}
    for route in losses.ROUTES:
        anm, pal = losses.BasicANMLoss(), losses.PhiAlignmentLoss()
        anm.route = pal.route = route
        out[f"anm_{route}_ms"] = median_ms(anm, lambda c: c({"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}, truth))
        out[f"phi_{route}_ms"] = median_ms(pal, lambda c: c(phi, phi_true))
    return out


def time_spectral_loss_step(batch=256, targets=3, dim=100, steps=200, warmup=10, repeats=5, seed=0, device="cuda:0"):
    """Device-event time of one forward + backward of ``losses.PhiSpectralLoss`` (default weights plus ``target_weight = 0.5``,
    ``check_status = False``) on ``route = "hip"`` and ``route = "tensor"``: [batch, dim] complex phi on the square grid of
    ``dim`` entries, ``targets`` slots with L_true cycling through 0 .. targets.  ``steps`` forward + backward pairs are enqueued
    between two events; ``repeats`` such windows give the figure (their median) and its range.  Returns a dict of milliseconds."""
    from . import losses
    dev = torch.device(device)
    side = int(round(dim ** 0.5))
    if side * side != dim:
        raise ValueError(f"--dim must be a square for --spectral, got {dim}")
    g = torch.Generator().manual_seed(seed)
    phi = torch.randn(batch, dim, dtype=torch.complex64, generator=g).to(dev).requires_grad_(True)
    phi_true = torch.randn(batch, dim, dtype=torch.complex64, generator=g).to(dev)
    truth = {"tau_true": torch.rand(batch, targets, generator=g).to(dev), "f_true": (torch.rand(batch, targets, generator=g) - 0.5).to(dev),
             "L_true": (torch.arange(batch) % (targets + 1)).to(dev)}
    out = {"batch": batch, "targets": targets, "dim": dim, "steps": steps, "repeats": repeats}
    for route in losses.ROUTES:
        crit = losses.PhiSpectralLoss(side, side, target_weight=0.5)
        crit.route, crit.check_status = route, False

        def window(n):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                phi.grad = None
                crit(phi, phi_true, truth)[0].backward()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / n

        window(warmup)
        times = sorted(window(steps) for _ in range(repeats))
        out[f"spectral_{route}_ms"] = round(times[len(times) // 2], 4)
        out[f"spectral_{route}_range_ms"] = [round(times[0], 4), round(times[-1], 4)]
    return out


def time_set_loss_step(batch=256, targets=3, dim=100, steps=200, warmup=10, repeats=5, seed=0, device="cuda:0"):
    """Device-event time of one forward + backward of ``losses.SetANMLoss`` (``check_status = False``) on ``route = "hip"`` and
    ``route = "tensor"`` (whose assignment is a host loop over the batch), and of ``losses.BasicANMLoss`` on ``route = "hip"`` on
    the same shapes: [batch, targets] head outputs and labels with L_true cycling through 0 .. targets, [batch, dim] complex
    phi.  ``steps`` forward + backward pairs are enqueued between two events; ``repeats`` such windows give the figure (their
    median) and its range.  Returns a dict of milliseconds."""
    from . import losses
    dev = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g).to(dev)
    tau, f, conf = (r(batch, targets).requires_grad_(True) for _ in range(3))
    truth = {"tau_true": r(batch, targets), "f_true": r(batch, targets) - 0.5,
             "L_true": (torch.arange(batch) % (targets + 1)).to(dev)}
    phi = torch.randn(batch, dim, dtype=torch.complex64, generator=g).to(dev).requires_grad_(True)
    outputs = {"tau_est": tau, "f_est": f, "confidences": conf, "phi_final": phi}
    out = {"batch": batch, "targets": targets, "dim": dim, "steps": steps, "repeats": repeats}
    for name, cls, route in (("set_hip", losses.SetANMLoss, "hip"), ("anm_hip", losses.BasicANMLoss, "hip"),
                             ("set_tensor", losses.SetANMLoss, "tensor")):
        crit = cls()
        crit.route, crit.check_status = route, False

        def window(n):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                for t in (tau, f, conf, phi):
                    t.grad = None
                crit(outputs, truth)[0].backward()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / n

        window(warmup)
        times = sorted(window(steps) for _ in range(repeats))
        out[f"{name}_ms"] = round(times[len(times) // 2], 4)
        out[f"{name}_range_ms"] = [round(times[0], 4), round(times[-1], 4)]
    return out


def time_cfar_step(signals=4096, grid=(16, 16), oversample=4, top=16, pfa=1e-4, steps=50, warmup=5, repeats=5, seed=0,
                   device="cuda:0", cancel=None):
    """Device-event time of ``admmnet_cfar_f64`` (both kernels) per method on preallocated buffers: ``signals`` scenes of
    ``make_scenes_device(targets=(1, 3))`` at 15 dB, ``steps`` back-to-back calls between two events; ``repeats`` such windows
    give the figure (their median) and its range.  Returns a dict of milliseconds, and the mean counts of each method.
    ``cancel=(iters, sweeps)`` times ``admmnet_cfar_relax_f64`` with those settings the same way instead, and reports the mean
    ``n_det``, ``maps`` and ``more`` of each method."""
    from . import _lib, detect, ops, synth
    dev = torch.device(device)
    Nb, Nd = grid
    y, b, _, truth = synth.make_scenes_device(signals, Nb, Nd, targets=(1, 3), seed=20260104 + seed, snr_range=(15.0, 15.0), device=dev)
    lib = _lib.load()
    rows = torch.empty(signals, top, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(signals, 2, dtype=torch.int32, device=dev)
    info = torch.empty(signals, 2, dtype=torch.float64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    out = {"signals": signals, "grid": list(grid), "oversample": oversample, "top": top, "pfa": pfa, "steps": steps, "repeats": repeats,
           "lds_bytes": lib.admmnet_cfar_lds_bytes(Nb, Nd, oversample)}
    if cancel is not None:
        iters, sweeps = detect._relax_settings(grid, oversample, *cancel)
        amp = torch.empty(signals, top, dtype=torch.complex128, device=dev)
        counts = torch.empty(signals, 3, dtype=torch.int32, device=dev)
        info = torch.empty(signals, 3, dtype=torch.float64, device=dev)
        out.update(entry="admmnet_cfar_relax_f64", iters=iters, sweeps=sweeps, lds_bytes=lib.admmnet_cfar_relax_lds_bytes(Nb, Nd, oversample))
    for method in ("known", "ca", "os"):
        noise = truth["noise_var"] if method == "known" else None
        _, _, m, phase, r, guard, train, rank, alpha = detect._settings(grid, top, oversample, method, pfa, 1, 2, None, (4, math.pi / 4),
                                                                      noise is not None)

        def window(n):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                if cancel is not None:
                    _lib.check(lib.admmnet_cfar_relax_f64(Nb, Nd, r, top, signals, ops._ptr(y), ops._ptr(b), None, m, phase,
                                                          detect.METHODS[method], guard, train, rank, alpha, ops._ptr(noise), iters, sweeps,
                                                          ops._ptr(rows), ops._ptr(amp), ops._ptr(counts), ops._ptr(info), None,
                                                          ops._ptr(status), ops._stream(dev)), "admmnet_cfar_relax_f64")
                    continue
                _lib.check(lib.admmnet_cfar_f64(Nb, Nd, r, top, signals, ops._ptr(y), ops._ptr(b), None, m, phase, detect.METHODS[method],
                                                guard, train, rank, alpha, ops._ptr(noise), ops._ptr(rows), ops._ptr(counts),
                                                ops._ptr(info), None, ops._ptr(status), ops._stream(dev)), "admmnet_cfar_f64")
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / n

        window(warmup)
        times = sorted(window(steps) for _ in range(repeats))
        out[f"{method}_ms"] = round(times[len(times) // 2], 4)
        out[f"{method}_range_ms"] = [round(times[0], 4), round(times[-1], 4)]
        out[f"{method}_mean_n_det"] = round(counts[:, 0].double().mean().item(), 3)
        if cancel is not None:
            out[f"{method}_mean_more"] = round(counts[:, 1].double().mean().item(), 4)
            out[f"{method}_mean_maps"] = round(counts[:, 2].double().mean().item(), 3)
            continue
        out[f"{method}_mean_n_over"] = round(counts[:, 1].double().mean().item(), 3)
    return out


def _score_case(batch, n_est, n_true, seed, dev):
    """Scenes drawn like ``synth.make_batch`` with estimates = shuffled truth + N(0, 0.03) and strays, as device tensors."""
    rng = np.random.default_rng(seed)
    from .synth import F_RANGE, TAU_RANGE
    tt = rng.uniform(*TAU_RANGE, size=(batch, n_true)).astype(np.float32)
    ft = rng.uniform(*F_RANGE, size=(batch, n_true)).astype(np.float32)
    est = np.stack([rng.uniform(*TAU_RANGE, size=(batch, n_est)), rng.uniform(*F_RANGE, size=(batch, n_est)),
                    rng.uniform(size=(batch, n_est))], axis=2)
    k = min(n_est, n_true)
    est[:, :k, 0] = tt[:, :k] + rng.normal(0, 0.03, size=(batch, k))
    est[:, :k, 1] = ft[:, :k] + rng.normal(0, 0.03, size=(batch, k))
    order = rng.random((batch, n_est)).argsort(axis=1)               # one row order per signal
    est = np.take_along_axis(est, order[:, :, None], axis=1)
    return torch.from_numpy(est).to(dev), torch.from_numpy(tt).to(dev), torch.from_numpy(ft).to(dev)


def time_score_step(steps=50, warmup=5, repeats=5, host_signals=2048, seed=0, device="cuda:0",
                    cases=((65536, 3, 3), (4096, 64, 64)), cutoff=0.1):
    """Median wall time of ``metrics.match_targets`` (each call bracketed by a device synchronisation) at B = 65 536 with three
    estimates and three targets and at B = 4096 with 64 of each, and of the host alternative in the same run: the batch copied to
    the host, then the ``metrics.match_host`` loop -- timed over the first ``host_signals`` signals and reported per signal, the
    copy of the whole batch apart.  ``repeats`` medians of ``steps`` calls each give the figure (their median) and its spread
    (largest less smallest).  Returns a dict."""
    from . import metrics
    dev = torch.device(device)
    out = {"steps": steps, "repeats": repeats, "cutoff": cutoff, "cases": []}
    for batch, n_est, n_true in cases:
        est, tt, ft = _score_case(batch, n_est, n_true, seed, dev)
        medians = []
        for rep in range(repeats):
            times = []
            for i in range(warmup + steps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                metrics.match_targets(est, tt, ft, cutoff=cutoff)
                torch.cuda.synchronize(dev)
                if i >= warmup:
                    times.append(time.perf_counter() - t0)
            medians.append(float(np.median(times)) * 1e3)
        t0 = time.perf_counter()
        h_est, h_tt, h_ft = est.cpu().numpy(), tt.cpu().numpy(), ft.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        n = min(batch, host_signals)
        t0 = time.perf_counter()
        for i in range(n):
            metrics.match_host(h_est[i, :, 0], h_est[i, :, 1], h_tt[i], h_ft[i], cutoff=cutoff)
        host_us = (time.perf_counter() - t0) / n * 1e6
        dev_ms = float(np.median(medians))
        out["cases"].append({"batch": batch, "n_est": n_est, "n_true": n_true, "device_ms": round(dev_ms, 4),
                             "device_ms_spread": round(max(medians) - min(medians), 4),
                             "device_us_per_signal": round(dev_ms * 1e3 / batch, 5), "host_copy_ms": round(copy_ms, 3),
                             "host_signals": n, "host_us_per_signal": round(host_us, 2),
                             "host_ms_whole_batch": round(copy_ms + host_us * batch / 1e3, 1)})
    return out


def evaluate_snr(grid=(NB, ND), layers=10, checkpoint=None, snrs=(5.0, 15.0, 25.0), signals=4096, targets=3, cutoff=1.0,
                 baseline=None, seed=0, device="cuda:0", head=False, cfar=("ca", 1e-4), cancel=None, targets_min=None, min_sep=0.0,
                 order=None, refine=None, crb=False):
    """Detection and accuracy against the noise level: per SNR one batch of ``signals`` scenes at exactly that SNR
    (``synth.make_batch_device(snr_range=(S, S))``), ``model.evaluate`` and ``metrics.summary`` -- scene, forward, peak search and
    score without a host loop.  ``baseline="classical"`` scores the peaks of the classical solver's phi (the generator's labels)
    the same way.  The model is ``PhiEstADMMNet`` at seed 0, or the checkpoint's.  Yields one dict per SNR and method.
    ``crb=True`` adds the root-mean Cramer-Rao bound of the same scenes, pooled over that method's own hits (``metrics.crb``), as
    ``crb_tau`` / ``crb_f``, and the pooled RMSE over it as ``rmse_over_crb_tau`` / ``rmse_over_crb_f``.
    ``refine="given"`` or ``"psk"`` yields, after each method's line, a line ``method + "+refine"``: the same rows fitted to the
    received signal (``refine.refine_targets`` with that symbol mode) and scored the same way, the bound pooled over that line's
    own hits.  The lines without ``+refine`` are those of a run without it.
    ``order=TOP`` (targets .. 16) yields, after those, a line ``method + "+order"``: TOP candidate peaks of the same phi through
    ``order.select_refined`` with the symbol mode of ``refine`` ("given" if that is None), the selected rows scored with
    ``n_est = n_sel``.  The other lines are those of a run without it.
    ``targets_min=LO`` (1 .. targets) and / or ``min_sep=CELLS`` > 0 draw the scenes with ``synth.make_scenes_device``: LO ..
    ``targets`` targets per scene, at least CELLS resolution cells apart.  The ``net`` and ``classical`` lines and their
    ``+refine`` lines are then GIVEN each scene's count (``top_n = n_est = L_true``), the ``+order`` lines are not: they select
    it, and gain ``order_under`` / ``order_exact`` / ``order_over``, the shares of the scenes where ``n_sel`` <, ==, > ``L_true``.
    Every line gains ``targets_min``, ``min_sep``, ``unseparated`` (scenes where a target stayed closer than ``min_sep``) and
    ``ser`` (the mean percentage of symbols decided wrongly); everything is scored against ``L_true``, the bound included.  With
    both at their defaults the scenes, the lines and their keys are those of ``make_batch_device``.
    ``head=True`` yields, after each SNR's other lines, a line ``method = "head"``: the learned head of ``ADMMNet`` (seed 0, or the
    checkpoint's, which is then an ``ADMMNet``'s; the ``net`` lines take its layers) through ``ADMMNet.estimate_head``, scored
    with ``n_est`` = the number of confidences >= 0.5 -- the head is never given a scene's count -- and, on varied scenes, with
    ``order_under`` / ``order_exact`` / ``order_over`` from that ``n_est``.  Without it every line and key is as before.
    ``baseline="periodogram"`` yields, after each SNR's other lines, a line ``method = "periodogram"``: what an OFDM radar
    runs on ``(y, b)`` alone -- ``detect.cfar_targets`` with ``cfar = (method, pfa)``, 16 rows, its other defaults -- scored with
    ``n_est = clamp(n_det, 0, 16)``; the detector is never given a scene's count, and on varied scenes the line gains
    ``order_under`` / ``order_exact`` / ``order_over`` from ``n_det``.  With ``refine`` a line ``periodogram+refine`` follows
    (those rows and that ``n_est`` through ``refine_targets``), with ``order`` a line ``periodogram+order`` (the first ``order``
    CFAR rows through ``order.select_refined`` with ``n_cand = min(n_est, order)``: the selection prunes the sidelobe detections
    of a strong target).  No labels are generated for it, and every other line and key is that of a run without it.  The method
    "known" takes ``truth["noise_var"]``, which only the varied scenes have: it RAISES on the fixed-count kind (pass
    ``targets_min=targets`` for scenes of exactly ``targets`` targets from ``make_scenes_device``).
    ``cancel=(iters, sweeps)``, with ``baseline="periodogram"`` only, yields after the ``periodogram`` lines a line
    ``periodogram+relax``: ``detect.cfar_relax`` with the same ``cfar``, 16 rows, that many Newton steps and re-fitting sweeps,
    scored with ``n_est = n_det`` (and, on varied scenes, ``order_under`` / ``order_exact`` / ``order_over`` from it); with
    ``refine`` a line ``periodogram+relax+refine`` follows.  Every other line is that of a run without it."""
    from . import PhiEstADMMNet, metrics, ops, synth
    from . import order as ordering
    from . import refine as refinement
    if baseline not in (None, "classical", "periodogram"):
        raise ValueError(f"baseline must be None, 'classical' or 'periodogram', got {baseline!r}")
    from . import detect
    try:
        cfar_method, cfar_pfa = cfar
        cfar_pfa = float(cfar_pfa)
    except (TypeError, ValueError):
        raise ValueError(f"cfar must be a pair (method, pfa), got {cfar!r}") from None
    if cfar_method not in detect.METHODS or not 0.0 < cfar_pfa < 1.0:
        raise ValueError(f"cfar must be (one of {sorted(detect.METHODS)}, a rate in (0, 1)), got {cfar!r}")
    if refine is not None and refine not in refinement.MODES:
        raise ValueError(f"refine must be None or one of {sorted(refinement.MODES)}, got {refine!r}")
    if order is not None and (isinstance(order, bool) or int(order) != order or not max(1, targets) <= order <= metrics.MAX_TARGETS):
        raise ValueError(f"order must be None or an int in targets .. {metrics.MAX_TARGETS}, got {order!r}")
    varied = targets_min is not None or min_sep != 0.0
    if targets_min is not None and (isinstance(targets_min, bool) or int(targets_min) != targets_min or not 1 <= targets_min <= targets):
        raise ValueError(f"targets_min must be None or an int in 1 .. targets, got {targets_min!r}")
    if not (min_sep >= 0.0 and math.isfinite(min_sep)):
        raise ValueError(f"min_sep must be finite and >= 0, got {min_sep!r}")
    if baseline == "periodogram" and cfar_method == "known" and not varied:
        raise ValueError("cfar method 'known' takes the scenes' noise_var, which the fixed-count scenes do not have: pass "
                         "targets_min=targets (or min_sep) to draw them with make_scenes_device")
    if cancel is not None:
        if baseline != "periodogram":
            raise ValueError("cancel belongs to baseline='periodogram'")
        try:
            cancel_iters, cancel_sweeps = cancel
        except (TypeError, ValueError):
            raise ValueError(f"cancel must be None or a pair (iters, sweeps), got {cancel!r}") from None
        cancel_iters, cancel_sweeps = detect._relax_settings(grid, 4, cancel_iters, cancel_sweeps)
    dev = torch.device(device)
    M, N = grid
    classical = baseline == "classical"
    torch.manual_seed(seed)
    model = PhiEstADMMNet(num_layers=layers, M=M, N=N, L=targets)
    head_model = None
    if head:
        from . import ADMMNet
        torch.manual_seed(seed)
        head_model = ADMMNet(num_layers=layers, M=M, N=N, L=targets)
        if checkpoint:
            state = load_checkpoint(checkpoint, head_model)["model_state_dict"]
            model.load_state_dict({k: v for k, v in state.items() if k in model.state_dict()})
        head_model.eval()
    elif checkpoint:
        load_checkpoint(checkpoint, model)
    model.eval()
    common = {"grid": [M, N], "layers": layers, "signals": signals, "targets": targets, "cutoff": cutoff}
    if varied:
        common.update(targets_min=targets if targets_min is None else int(targets_min), min_sep=float(min_sep))

    def scored(res, truth, snr, n_sel=None):
        if varied:                                                                     # in summary's one read
            extra = {"unseparated": truth["state"].sum(), "ser": truth["ser"].mean()}
            if n_sel is not None:
                extra["order"] = metrics.order_counts(n_sel, truth["L_true"])
            line = metrics.summary(res, extra=extra)
            line["unseparated"] = int(line["unseparated"])
            if n_sel is not None:
                for name, count in zip(("order_under", "order_exact", "order_over"), line.pop("order")):
                    line[name] = count / signals
        else:
            line = metrics.summary(res)
        if crb:
            c = metrics.crb_summary(metrics.crb(truth["tau"], truth["f"], truth["C"], (M, N), snr_db=snr, L_true=truth.get("L_true"),
                                                match=res.match))
            for axis in ("tau", "f"):
                line[f"crb_{axis}"] = c[f"crb_{axis}_hits"]
                line[f"rmse_over_crb_{axis}"] = line[f"rmse_{axis}"] / c[f"crb_{axis}_hits"]
        return line

    # truth["L_true"]: the count of every scene, which these rows were cut to (None: every scene has ``targets``)
    match = lambda rows, truth: metrics.match_targets(rows, truth["tau"], truth["f"], truth.get("L_true"), truth.get("L_true"),  # noqa: E731
                                                      cutoff=cutoff, scale=(float(N), float(M)), period=(1.0, 1.0))

    def refined(method, rows, y, b, truth, snr):
        fit = refinement.refine_targets(y, b, rows, (M, N), n_est=truth.get("L_true"), symbols=refine)
        return {"snr": snr, "method": method + "+refine", **common, **scored(match(fit.rows, truth), truth, snr)}

    est_opts = {"xstep": 1 / (10 * N), "ystep": 1 / (10 * M), "iter": 3}              # estimate's defaults

    def ordered(method, phi, y, b, truth, snr):
        cand, _ = ops.peak_top(phi, M, N, est_opts, top=int(order))
        sel, _ = ordering.select_refined(y, b, cand, (M, N), symbols=refine or "given")
        res = metrics.match_targets(sel.rows_out, truth["tau"], truth["f"], truth.get("L_true"), n_est=sel.n_sel, cutoff=cutoff,
                                    scale=(float(N), float(M)), period=(1.0, 1.0))
        return {"snr": snr, "method": method + "+order", **common, **scored(res, truth, snr, sel.n_sel)}

    def periodogram(y, b, truth, snr):
        det = detect.cfar_targets(y, b, (M, N), method=cfar_method, pfa=cfar_pfa,
                                  noise_var=truth["noise_var"] if cfar_method == "known" else None)
        n_est = det.n_est
        score = lambda rows, n: metrics.match_targets(rows, truth["tau"], truth["f"], truth.get("L_true"), n_est=n, cutoff=cutoff,  # noqa: E731
                                                      scale=(float(N), float(M)), period=(1.0, 1.0))
        counted = det.n_det if varied else None
        yield {"snr": snr, "method": "periodogram", **common, **scored(score(det.rows, n_est), truth, snr, counted)}
        if refine is not None:
            fit = refinement.refine_targets(y, b, det.rows, (M, N), n_est=n_est, symbols=refine)
            yield {"snr": snr, "method": "periodogram+refine", **common, **scored(score(fit.rows, n_est), truth, snr, counted)}
        if order is not None:
            top = int(order)
            sel, _ = ordering.select_refined(y, b, det.rows[:, :top], (M, N), symbols=refine or "given", n_cand=n_est.clamp(max=top))
            yield {"snr": snr, "method": "periodogram+order", **common, **scored(score(sel.rows_out, sel.n_sel), truth, snr, sel.n_sel)}
        if cancel is not None:
            det = detect.cfar_relax(y, b, (M, N), method=cfar_method, pfa=cfar_pfa, iters=cancel_iters, sweeps=cancel_sweeps,
                                    noise_var=truth["noise_var"] if cfar_method == "known" else None)
            n_est = det.n_est
            counted = det.n_det if varied else None
            yield {"snr": snr, "method": "periodogram+relax", **common, **scored(score(det.rows, n_est), truth, snr, counted)}
            if refine is not None:
                fit = refinement.refine_targets(y, b, det.rows, (M, N), n_est=n_est, symbols=refine)
                yield {"snr": snr, "method": "periodogram+relax+refine", **common,
                       **scored(score(fit.rows, n_est), truth, snr, counted)}

    for i, snr in enumerate(snrs):
        if varied:
            y, b, sigma, truth = synth.make_scenes_device(signals, M, N, targets=(common["targets_min"], targets), min_sep=min_sep,
                                                          seed=20260104 + seed + 7919 * i, snr_range=(snr, snr), device=dev,
                                                          labels=classical)
        else:
            y, b, sigma, truth = synth.make_batch_device(signals, M, N, L=targets, seed=20260104 + seed + 7919 * i, snr_range=(snr, snr),
                                                         device=dev, labels=classical)
        if refine is None and not varied:
            res = model.evaluate(y, b, sigma, truth["tau"], truth["f"], cutoff=cutoff, top=targets)
        else:                                                                          # evaluate, with the rows kept
            rows, _, _ = model._estimate_rows(y, b, sigma, targets, truth.get("L_true"))
            res = match(rows, truth)
        yield {"snr": snr, "method": "net", **common, **scored(res, truth, snr)}
        if refine is not None:
            yield refined("net", rows, y, b, truth, snr)
        if order is not None:
            with torch.no_grad():
                phi, _ = model._run(y, b, sigma, to_caller=False)
            yield ordered("net", phi, y, b, truth, snr)
        if classical:
            opts = {"xstep": 1 / (10 * N), "ystep": 1 / (10 * M), "iter": 3}            # estimate's defaults
            rows, _ = ops.peak_top(truth["phi"], M, N, opts, top=targets, top_n=truth.get("L_true"))
            yield {"snr": snr, "method": "classical", **common, **scored(match(rows, truth), truth, snr)}
            if refine is not None:
                yield refined("classical", rows, y, b, truth, snr)
            if order is not None:
                yield ordered("classical", truth["phi"], y, b, truth, snr)
        if head_model is not None:
            e = head_model._head_rows(y, b, sigma, 0.5)
            res = metrics.match_targets((e.tau, e.f), truth["tau"], truth["f"], truth.get("L_true"), n_est=e.n_est, cutoff=cutoff,
                                        scale=(float(N), float(M)), period=(1.0, 1.0))
            yield {"snr": snr, "method": "head", **common, **scored(res, truth, snr, e.n_est if varied else None)}
        if baseline == "periodogram":
            yield from periodogram(y, b, truth, snr)


def _grid(ap, text):
    try:
        grid = tuple(int(v) for v in text.lower().split("x"))
        assert len(grid) == 2 and min(grid) >= 1
    except (ValueError, AssertionError):
        ap.error(f"--grid must be MxN, got {text!r}")
    return grid


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("time-net")
    a.add_argument("--layers", type=int, default=5)
    a.add_argument("--runs", type=int, default=1000)
    a.add_argument("--out", default=None)
    a.add_argument("--checkpoint", default=None)
    a.add_argument("--seed", type=int, default=0)
    b = sub.add_parser("time-admm")
    b.add_argument("--runs", type=int, default=1000)
    b.add_argument("--out", default=None)
    b.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("train-step")
    c.add_argument("--layers", type=int, default=10)
    c.add_argument("--batch", type=int, default=256)
    c.add_argument("--steps", type=int, default=20)
    c.add_argument("--route", choices=TRAIN_ROUTES, default="tensor")
    c.add_argument("--grid", default=f"{NB}x{ND}", help="MxN")
    c.add_argument("--head", action="store_true", help="time ADMMNet (phi + tau + f loss) instead of PhiEstADMMNet")
    c.add_argument("--warmup", type=int, default=3)
    c.add_argument("--optim", choices=("torch", "hip"), default="torch",
                   help="hip: clipping and AdamW on the kernels of admm_net_amd.optim instead of torch's")
    c.add_argument("--loss", choices=("set", "basic"), default=None,
                   help="with --head: train with SetANMLoss / BasicANMLoss on scenes of --targets-min .. --targets targets")
    c.add_argument("--targets", type=int, default=3)
    c.add_argument("--targets-min", type=int, default=None, metavar="LO")
    c.add_argument("--min-sep", type=float, default=0.0, metavar="CELLS")
    c.add_argument("--save", default=None, metavar="PATH", help="save the model's checkpoint after the last step")
    d = sub.add_parser("loss-step")
    d.add_argument("--batch", type=int, default=256)
    d.add_argument("--targets", type=int, default=3)
    d.add_argument("--dim", type=int, default=100)
    d.add_argument("--steps", type=int, default=200)
    d.add_argument("--spectral", action="store_true",
                   help="time PhiSpectralLoss (device events, median and range of five windows) instead of the two reference losses")
    d.add_argument("--set", action="store_true", dest="set_loss",
                   help="time SetANMLoss on both routes beside BasicANMLoss (device events, median and range of five windows)")
    e = sub.add_parser("score-step")
    e.add_argument("--steps", type=int, default=50)
    e.add_argument("--repeats", type=int, default=5)
    e.add_argument("--host-signals", type=int, default=2048)
    g = sub.add_parser("cfar-step")
    g.add_argument("--signals", type=int, default=4096)
    g.add_argument("--grid", default="16x16", help="MxN")
    g.add_argument("--oversample", type=int, default=4)
    g.add_argument("--steps", type=int, default=50)
    f = sub.add_parser("evaluate")
    for q, what in ((g, "time admmnet_cfar_relax_f64 instead"), (f, "with --baseline periodogram: add the periodogram+relax lines")):
        q.add_argument("--cancel", action="store_true", help=f"successive cancellation with cyclic re-fitting: {what}")
        q.add_argument("--sweeps", type=int, default=2, help="re-fitting sweeps of --cancel")
        q.add_argument("--newton", type=int, default=3, metavar="I", help="Newton steps per fit of --cancel")
    f.add_argument("--grid", default=f"{NB}x{ND}", help="MxN")
    f.add_argument("--layers", type=int, default=10)
    f.add_argument("--checkpoint", default=None)
    f.add_argument("--snr", type=float, nargs="+", default=[5.0, 15.0, 25.0])
    f.add_argument("--signals", type=int, default=4096)
    f.add_argument("--targets", type=int, default=3)
    f.add_argument("--cutoff", type=float, default=1.0, help="in resolution cells")
    f.add_argument("--baseline", choices=("classical", "periodogram"), default=None,
                   help="periodogram: a CFAR detector on the zero-padded periodogram of (y, b), never given a scene's count")
    f.add_argument("--cfar", choices=("ca", "os", "known"), default="ca", help="the noise level of --baseline periodogram")
    f.add_argument("--pfa", type=float, default=1e-4, help="its false-alarm rate per map cell")
    f.add_argument("--refine", choices=("given", "psk"), default=None,
                   help="after each method's line, the same rows fitted to the received signal with these symbols")
    f.add_argument("--crb", action="store_true", help="add the Cramer-Rao bound pooled over each method's hits, and RMSE over it")
    f.add_argument("--targets-min", type=int, default=None, metavar="LO",
                   help="draw LO .. --targets targets per scene; the lines without +order are given each scene's count")
    f.add_argument("--min-sep", type=float, default=0.0, metavar="CELLS",
                   help="keep the targets of a scene at least this many resolution cells apart")
    f.add_argument("--head", action="store_true",
                   help="after each SNR's lines, the learned head of ADMMNet (the checkpoint's), its count from the confidences")
    f.add_argument("--order", type=int, default=None, metavar="TOP",
                   help="after each method's lines, TOP candidate peaks with the number of targets selected against the received signal")
    args = ap.parse_args(argv)
    if args.cmd == "score-step":
        import json
        print(json.dumps(time_score_step(args.steps, repeats=args.repeats, host_signals=args.host_signals)))
        return
    if args.cmd == "cfar-step":
        import json
        extra = {"cancel": (args.newton, args.sweeps)} if args.cancel else {}
        print(json.dumps(time_cfar_step(args.signals, _grid(ap, args.grid), args.oversample, steps=args.steps, **extra)))
        return
    if args.cmd == "evaluate":
        import json
        if args.cancel and args.baseline != "periodogram":
            ap.error("--cancel belongs to --baseline periodogram")
        for line in evaluate_snr(_grid(ap, args.grid), args.layers, args.checkpoint, args.snr, args.signals, args.targets,
                                 args.cutoff, args.baseline, targets_min=args.targets_min, min_sep=args.min_sep,
                                 refine=args.refine, crb=args.crb, order=args.order, head=args.head, cfar=(args.cfar, args.pfa),
                                 cancel=(args.newton, args.sweeps) if args.cancel else None):
            print(json.dumps(line), flush=True)
        return
    if args.cmd == "loss-step":
        import json
        if args.spectral and args.set_loss:
            ap.error("--spectral and --set are two commands")
        step = time_spectral_loss_step if args.spectral else time_set_loss_step if args.set_loss else time_loss_step
        print(json.dumps(step(args.batch, args.targets, args.dim, args.steps)))
        return
    if args.cmd == "train-step":
        import json
        try:
            grid = tuple(int(v) for v in args.grid.lower().split("x"))
            assert len(grid) == 2 and min(grid) >= 1
        except (ValueError, AssertionError):
            ap.error(f"--grid must be MxN, got {args.grid!r}")
        scenes = {}
        if args.loss is not None:
            scenes = dict(loss=args.loss, targets=(args.targets if args.targets_min is None else args.targets_min, args.targets),
                          min_sep=args.min_sep)
        elif args.targets_min is not None or args.min_sep != 0.0 or args.targets != 3:
            ap.error("--targets, --targets-min and --min-sep go with --loss")
        line = time_train_step(args.layers, args.batch, args.steps, warmup=args.warmup, route=args.route, grid=grid, head=args.head,
                               optim=args.optim, checkpoint=args.save, **scenes)
        if line.get("n_ranks", 1) == 1 or torch.distributed.get_rank() == 0:      # one JSON line, rank 0's
            print(json.dumps(line))
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return
    if args.cmd == "time-net":
        from . import PhiEstADMMNet
        torch.manual_seed(0)
        model = PhiEstADMMNet(num_layers=args.layers, M=NB, N=ND, L=3)
        if args.checkpoint:
            load_checkpoint(args.checkpoint, model)
        out = args.out or (f"time_net_{args.layers}.txt" if args.layers != 10 else "time_net.txt")
        t = time_net(model, args.runs, out, args.seed)
    else:
        out = args.out or "time.txt"
        t = time_admm(args.runs, out, args.seed)
    t = np.asarray(t)
    print(f"{out}: {len(t)} runs, mean {t.mean():.6f} s, median {np.median(t):.6f} s, first {t[0]:.6f} s")


if __name__ == "__main__":
    main()
