"""CPU: the training losses of admm_net_amd/losses.py -- the tensor formulation (``TensorLossKernels``, the stand-in for the HIP
kernels of csrc/loss.hip) against the reference's own float32 outputs and gradients (tests/golden/loss_*.npz, written by
tests/golden/make_golden_loss.py) and, in float64, against autograd through a per-sample evaluation written here; the
modules' surface; the opt-in ``loss`` drop-in.

Tolerances (tests/test_gpu_training_fused.py / test_gpu_training_small.py): a reduction within 2e-5 of the sum of the
magnitudes of its terms -- the loss terms are all non-negative, so that sum is the value itself --, an elementwise output
within 1e-6 of the largest entry; float64 against autograd at 1e-12 of the largest entry.
"""
import inspect
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from admm_net_amd import _lib, losses
from admm_net_amd.losses import TensorLossKernels as TLK

import loss_cases as LC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
RED, ELEM, F64 = 2e-5, 1e-6, 1e-12


def _fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z, (lambda k: torch.from_numpy(z[k]))


def _anm_module(route="tensor", **kw):
    m = losses.BasicANMLoss(**kw)
    m.route = route
    return m


def _phi_module(route="tensor", **kw):
    m = losses.PhiAlignmentLoss(**kw)
    m.route = route
    return m


def _anm_call(m, c, leaves=None):
    s = leaves or c
    return m({"tau_est": s["tau"], "f_est": s["f"], "confidences": s["conf"], "phi_final": s["phi"]},
             {"tau_true": c["tau_true"], "f_true": c["f_true"], "L_true": c["L_true"]})


def _leaves(c, keys, dtype=None):
    cast = lambda t: t if dtype is None else t.to(torch.complex128 if t.is_complex() else dtype)
    return {k: cast(c[k]).clone().requires_grad_(True) for k in keys}


def _close_value(got, want, terms, name):
    assert abs(float(got.detach()) - float(want)) <= RED * float(terms), (name, float(got.detach()), float(want))


def _close_elem(got, want, tol, name):
    want = torch.as_tensor(want)
    assert got.shape == want.shape, name
    err = (got - want).abs().max().item()
    assert err <= tol * want.abs().max().item(), f"{name}: {err:.3e} against largest entry {want.abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------------ against the reference, float32
@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_anm_tensor_route_matches_the_reference_fixture(tag):
    z, t = _fixture("loss_anm_b7")
    c = {k: t(k) for k in ("tau", "f", "conf", "tau_true", "f_true", "L_true", "phi")}
    leaves = _leaves(c, ("tau", "f", "conf", "phi"))
    total, d = _anm_call(_anm_module(lambda_reg=float(z["lambda_reg"])), c, leaves)
    assert total is d["total_loss"]
    want = z["out"]
    for i, k in enumerate(("total_loss", "param_loss", "reg_loss")):
        assert d[k].dim() == 0 and d[k].dtype == torch.float32
        _close_value(d[k], want[i], want[i], k)                      # every term of these sums is non-negative
    w = (1.0, 0.0, 0.0) if tag == "g1" else tuple(z["up"])
    sum(wi * d[k] for wi, k in zip(w, ("total_loss", "param_loss", "reg_loss")) if wi != 0.0).backward()
    for k, leaf in leaves.items():
        _close_elem(leaf.grad, z[f"{tag}:{k}"], ELEM, f"{tag}:{k}")
    assert not leaves["phi"].grad[-1].any(), "the gradient of the norm of an all-zero row is 0"
    Lb = c["L_true"].reshape(-1, 1)
    beyond = (torch.arange(3) >= Lb) & (Lb >= 1)
    for k in ("tau", "f", "conf"):
        assert not leaves[k].grad[beyond].any(), k
    assert not leaves["tau"].grad[c["L_true"] == 0].any() and not leaves["f"].grad[c["L_true"] == 0].any()


def test_basic_parameter_loss_matches_the_reference_fixture(monkeypatch):
    z, t = _fixture("loss_anm_b7")
    monkeypatch.setattr(losses.basic_parameter_loss, "route", "tensor")
    got = losses.basic_parameter_loss(t("tau"), t("f"), t("tau_true"), t("f_true"), t("conf"), t("L_true"))
    assert got.dim() == 0
    _close_value(got, z["param_only"], z["param_only"], "basic_parameter_loss")


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_phi_tensor_route_matches_the_reference_fixture(tag):
    z, t = _fixture("loss_phi_b5")
    phi_true, w4 = t("phi_true"), [float(v) for v in z["weights"]]
    LC.check_phase_margin(t("phi"), phi_true)
    phi = t("phi").clone().requires_grad_(True)
    total, d = _phi_module(amplitude_weight=w4[0], phase_weight=w4[1], spectral_weight=w4[2], distribution_weight=w4[3])(phi, phi_true)
    assert total is d["total_loss"]
    want = z["out"]
    for i, k in enumerate(("total_loss", "amplitude_loss", "phase_loss")):
        assert d[k].dim() == 0 and d[k].dtype == torch.float32
        _close_value(d[k], want[i], want[i], k)
    w = (1.0, 0.0, 0.0) if tag == "g1" else tuple(z["up"])
    sum(wi * d[k] for wi, k in zip(w, ("total_loss", "amplitude_loss", "phase_loss")) if wi != 0.0).backward()
    _close_elem(phi.grad, z[f"{tag}:phi"], ELEM, f"{tag}:phi")
    assert (phi.grad[t("phi") == 0] == 0).all() and (t("phi") == 0).any()


# ------------------------------------------------------------------------------------------------ float64 against autograd
def _anm_per_sample(tau, f, conf, tau_true, f_true, L_true, phi, lambda_reg):
    """The definition, one sample at a time, in plain differentiable tensor operations."""
    per = []
    for b in range(tau.shape[0]):
        L = int(L_true[b])
        if L == 0:
            per.append((conf[b] * conf[b]).sum())
        else:
            per.append(((tau[b, :L] - tau_true[b, :L]) ** 2).sum() / L + ((f[b, :L] - f_true[b, :L]) ** 2).sum() / L
                       + 0.1 * ((conf[b, :L] - 1) ** 2).sum() / L)
    param = torch.stack(per).sum() / len(per)
    reg = lambda_reg * torch.stack([torch.linalg.vector_norm(phi[b]) for b in range(phi.shape[0])]).sum() / phi.shape[0]
    return param + reg, param, reg


def _phi_per_entry(phi, phi_true, aw, pw):
    d = torch.angle(phi) - torch.angle(phi_true)
    w = d - 2 * math.pi * torch.floor((d.detach() + math.pi) / (2 * math.pi))      # the floored mod, derivative 1
    amp = ((torch.abs(phi) - torch.abs(phi_true)) ** 2).sum() / phi.numel()
    ph = (w ** 2).sum() / phi.numel()
    return aw * amp + pw * ph, amp, ph


UPS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.7, 0.3, -0.6)]


@pytest.mark.parametrize("up", UPS, ids=["total", "first", "second", "weighted"])
@pytest.mark.parametrize("B,Lmax,D,L", [(7, 3, 20, "mixed"), (1, 1, 1, "all"), (5, 64, 7, "mixed"), (4, 3, 5, "none")])
def test_anm_float64_matches_autograd_per_sample(B, Lmax, D, L, up):
    c = LC.anm_case(B, Lmax, D, seed=B + Lmax + D, L=L)
    keys = ("tau", "f", "conf", "phi")
    a, b = _leaves(c, keys, torch.float64), _leaves(c, keys, torch.float64)
    c64 = {k: (v if k == "L_true" else v.to(torch.complex128 if v.is_complex() else torch.float64)) for k, v in c.items()}
    _, d = _anm_call(_anm_module(lambda_reg=0.37), c64, a)
    got = (d["total_loss"], d["param_loss"], d["reg_loss"])
    want = _anm_per_sample(b["tau"], b["f"], b["conf"], c64["tau_true"], c64["f_true"], c64["L_true"], b["phi"], 0.37)
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and abs(g.item() - w.item()) <= F64 * abs(w.item())
    sum(u * g for u, g in zip(up, got)).backward()
    sum(u * w for u, w in zip(up, want)).backward()
    for k in keys:
        wg = b[k].grad if b[k].grad is not None else torch.zeros_like(b[k])
        assert (a[k].grad - wg).abs().max().item() <= F64 * max(wg.abs().max().item(), 1e-300), k


@pytest.mark.parametrize("up", UPS, ids=["total", "first", "second", "weighted"])
@pytest.mark.parametrize("B,D", [(5, 20), (1, 1), (3, 7)])
def test_phi_float64_matches_autograd_per_entry(B, D, up):
    phi, phi_true = (t.to(torch.complex128) for t in LC.phase_pair(B, D, seed=B + D))
    a, b = phi.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    _, d = _phi_module(amplitude_weight=0.8, phase_weight=0.45)(a, phi_true)
    got = (d["total_loss"], d["amplitude_loss"], d["phase_loss"])
    want = _phi_per_entry(b, phi_true, 0.8, 0.45)
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and abs(g.item() - w.item()) <= F64 * abs(w.item())
    sum(u * g for u, g in zip(up, got)).backward()
    sum(u * w for u, w in zip(up, want)).backward()
    assert (a.grad - b.grad).abs().max().item() <= F64 * b.grad.abs().max().item()
    assert (a.grad[phi == 0] == 0).all()


def test_wrap_semantics():
    """Python's %: a result in [-pi, pi), +pi maps to -pi; on the tensor formulation in float64 only."""
    pi = math.pi
    d = torch.tensor([pi, -pi, 3.5, -3.5, 0.0, 2 * pi, -2 * pi + 0.25], dtype=torch.float64)
    want = torch.tensor([-pi, -pi, 3.5 - 2 * pi, -3.5 + 2 * pi, 0.0, 0.0, 0.25], dtype=torch.float64)
    got = TLK.wrap(d)
    assert (got - want).abs().max().item() <= 1e-15
    assert got[0].item() == -pi and got[1].item() == -pi
    assert all(((x + pi) % (2 * pi) - pi) == g for x, g in zip(d.tolist(), got.tolist()))


# ------------------------------------------------------------------------------------------------ the modules' surface
@pytest.mark.parametrize("bad", [[0, 1, 4, 2, 3, 0, 1], [0, 1, -1, 2, 3, 0, -5]])
def test_L_true_out_of_range_raises(bad):
    c = LC.anm_case(7, 3, 20, seed=1, L=bad)
    m = _anm_module()
    with pytest.raises(ValueError, match="outside"):
        _anm_call(m, c)
    m.check_status = False
    total, _ = _anm_call(m, c)                                   # evaluated with L held to [0, Lmax]
    held = dict(c, L_true=c["L_true"].clamp(0, 3))
    assert torch.equal(total, _anm_call(_anm_module(), held)[0])


def test_targets_that_require_grad_raise():
    c = LC.anm_case(3, 3, 5, seed=2)
    for k in ("tau_true", "f_true"):
        with pytest.raises(ValueError, match="requires grad"):
            _anm_call(_anm_module(), dict(c, **{k: c[k].clone().requires_grad_(True)}))
    phi, phi_true = LC.phase_pair(2, 5, seed=3)
    with pytest.raises(ValueError, match="requires grad"):
        _phi_module()(phi, phi_true.clone().requires_grad_(True))


def test_hip_route_refuses_cpu_tensors_and_unknown_routes():
    c = LC.anm_case(3, 3, 5, seed=2)
    assert losses.BasicANMLoss().route == "hip" and losses.PhiAlignmentLoss().route == "hip" and losses.BasicANMLoss().check_status
    assert losses.basic_parameter_loss.route == "hip"
    with pytest.raises(_lib.AdmmNetError):
        _anm_call(losses.BasicANMLoss(), c)
    phi, phi_true = LC.phase_pair(2, 5, seed=3)
    with pytest.raises(_lib.AdmmNetError):
        losses.PhiAlignmentLoss()(phi, phi_true)
    with pytest.raises(_lib.AdmmNetError):
        losses.basic_parameter_loss(c["tau"], c["f"], c["tau_true"], c["f_true"], c["conf"], c["L_true"])
    with pytest.raises(ValueError, match="route"):
        _anm_call(_anm_module(route="eager"), c)


def test_no_grad_runs_the_forward_only():
    calls = []

    class Spy(TLK):
        @staticmethod
        def anm_bwd(*a):
            calls.append("anm_bwd")
            return TLK.anm_bwd(*a)

    c = LC.anm_case(3, 3, 5, seed=2)
    leaves = _leaves(c, ("tau", "f", "conf", "phi"))
    with torch.no_grad():
        total, d = _anm_call(_anm_module(), c, leaves)
    assert not total.requires_grad and all(not v.requires_grad for v in d.values())
    out = losses._ANMLossFn.apply(leaves["tau"], leaves["f"], leaves["conf"], leaves["phi"], c["tau_true"], c["f_true"], c["L_true"],
                                  1e-4, Spy)
    assert not calls
    out[0].backward()
    assert calls == ["anm_bwd"]


def test_names_match_the_reference():
    for name, cls, fn in (("loss_anm_b7", losses.BasicANMLoss, losses.basic_parameter_loss),
                          ("loss_phi_b5", losses.PhiAlignmentLoss, None)):
        z, _ = _fixture(name)
        want = dict(zip(z["sig_names"].tolist(), z["sig_values"].tolist()))
        assert str(inspect.signature(cls.__init__)) == want["init"]
        assert str(inspect.signature(cls.forward)) == want["forward"]
        if fn is not None:
            assert str(inspect.signature(fn)) == want["function"]
    z, _ = _fixture("loss_anm_b7")
    c = LC.anm_case(3, 3, 5, seed=2)
    assert list(_anm_call(_anm_module(), c)[1].keys()) == z["keys"].tolist()
    z, _ = _fixture("loss_phi_b5")
    assert list(_phi_module()(*LC.phase_pair(2, 5, seed=3))[1].keys()) == z["keys"].tolist()


def test_library_rejects_bad_loss_arguments():
    lib = _lib.load()
    assert lib.admmnet_loss_partials(0, 256) == 64 * 3 and lib.admmnet_loss_partials(1, 5) == 2 * 2
    assert lib.admmnet_loss_partials(2, 5) == -1 and lib.admmnet_loss_partials(0, 0) == -1
    p = lambda n: [None] * n
    for Lmax, D, B in ((0, 4, 4), (65, 4, 4), (3, 0, 4), (3, 4, 0)):
        assert lib.admmnet_loss_anm_f32(Lmax, D, B, *p(7), 0.0, *p(5)) == -1       # (null pointers: rejected before any launch)
    assert lib.admmnet_loss_anm_f32(3, 4, 4, *p(7), 0.0, *p(5)) == -1
    assert b"loss_anm" in lib.admmnet_last_error()
    assert lib.admmnet_loss_anm_bwd_f32(3, 4, 4, *p(9), 0.0, *p(5)) == -1
    assert lib.admmnet_loss_phi_c64(4, 4, None, None, 1.0, 0.5, None, None, None) == -1
    assert lib.admmnet_loss_phi_bwd_c64(4, 4, None, None, None, 1.0, 0.5, None, None) == -1


# ------------------------------------------------------------------------------------------------ the opt-in drop-in
LOSS_PROBE = '''
import json, sys
import loss
from loss import BasicANMLoss, PhiAlignmentLoss, basic_parameter_loss
import admm_net
print(json.dumps({"loss": loss.__file__, "cls": [BasicANMLoss.__module__, PhiAlignmentLoss.__module__, basic_parameter_loss.__module__],
                  "net": admm_net.ADMMNet.__module__, "argv": sys.argv[1:]}))
'''


def _fake_script_tree(tmp_path):
    """A script directory as tests/test_host_logic.py::_fake_reference_tree lays it out, with a loss.py that must lose to the
    shim only when asked."""
    (tmp_path / "utils").mkdir()
    for name, text in (("admm_net.py", "admm_net"), ("admm.py", "admm"), ("utils/peakSearchUtils.py", "peakSearchUtils"),
                       ("utils/mathUtils.py", "mathUtils"), ("loss.py", "loss")):
        (tmp_path / name).write_text(f"raise ImportError('the script directory {text}.py was imported')\n")
    (tmp_path / "utils" / "plotUtils.py").write_text("def plot_predictions_vs_truth(*a, **k):\n    return 'ref plot'\n")
    (tmp_path / "probe.py").write_text(LOSS_PROBE)
    return tmp_path / "probe.py"


def _run(cmd, tmp_path):
    env = {**os.environ, "PYTHONPATH": ROOT, "PYTHONDONTWRITEBYTECODE": "1"}
    return subprocess.run([sys.executable] + cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)


def _assert_shimmed(r, argv):
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["loss"].startswith(os.path.join(ROOT, "admm_net_amd", "dropin", "optional"))
    assert info["cls"] == ["admm_net_amd.losses"] * 3 and info["net"] == "admm_net_amd.modules" and info["argv"] == argv


def test_dropin_leaves_loss_to_the_script_directory_by_default(tmp_path):
    probe = _fake_script_tree(tmp_path)
    r = _run(["-m", "admm_net_amd.dropin", str(probe), "--x", "1"], tmp_path)
    assert r.returncode != 0 and "the script directory loss.py was imported" in r.stderr
    # --hip-loss behind the script name belongs to the script
    r = _run(["-m", "admm_net_amd.dropin", str(probe), "--hip-loss"], tmp_path)
    assert r.returncode != 0 and "the script directory loss.py was imported" in r.stderr


def test_dropin_hip_loss_flag(tmp_path):
    probe = _fake_script_tree(tmp_path)
    _assert_shimmed(_run(["-m", "admm_net_amd.dropin", "--hip-loss", str(probe), "--x", "1", "--hip-loss"], tmp_path),
                    ["--x", "1", "--hip-loss"])


def test_dropin_activate_loss(tmp_path):
    _fake_script_tree(tmp_path)
    (tmp_path / "probe2.py").write_text("from admm_net_amd import dropin\ndropin.activate(loss=True)\n" + LOSS_PROBE)
    _assert_shimmed(_run([str(tmp_path / "probe2.py"), "a"], tmp_path), ["a"])
    (tmp_path / "probe3.py").write_text("import admm_net_amd.dropin.activate_loss\n" + LOSS_PROBE)
    _assert_shimmed(_run([str(tmp_path / "probe3.py")], tmp_path), [])
    # the plain activation keeps its meaning, also in front of the opt-in
    (tmp_path / "probe4.py").write_text("import admm_net_amd.dropin.activate\nimport admm_net_amd.dropin.activate_loss\n" + LOSS_PROBE)
    _assert_shimmed(_run([str(tmp_path / "probe4.py")], tmp_path), [])
    (tmp_path / "probe5.py").write_text("import admm_net_amd.dropin.activate\n" + LOSS_PROBE)
    r = _run([str(tmp_path / "probe5.py")], tmp_path)
    assert r.returncode != 0 and "the script directory loss.py was imported" in r.stderr
