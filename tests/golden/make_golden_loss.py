"""Generate the loss fixtures by IMPORTING the reference's loss.py (build container only; imported, never copied).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss.py
Writes loss_anm_b7.npz and loss_phi_b5.npz next to this file: the inputs (tests/loss_cases.py), the reference's float32
outputs and its float32 gradients -- once for ``total.backward()`` (g1:) and once for a weighted sum of the three dict
entries (g2:, weights in ``up``) -- and the names a drop-in has to match (dict keys, signatures).  Only data is stored.

The reference's BasicANMLoss cannot run its backward in float64 (its ``torch.ones(L)`` is float32), so the fixtures are
float32; the float64 ground truth of the tests is the tensor formulation of admm_net_amd/losses.py.
"""
import inspect
import os
import sys

sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import numpy as np
import torch

import loss as ref_loss   # the reference's loss module (imported, not copied)
from loss_cases import anm_case, phase_pair

UP = (1.7, 0.3, -0.6)     # weights of (total, first part, second part) in the second backward


def names(cls, fn=None):
    out = {"init": str(inspect.signature(cls.__init__)), "forward": str(inspect.signature(cls.forward))}
    if fn is not None:
        out["function"] = str(inspect.signature(fn))
    return out


def save(name, rec):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{name}: {os.path.getsize(path)} bytes")


def grads(leaves, make_loss):
    out = {}
    for tag, w in (("g1", (1.0, 0.0, 0.0)), ("g2", UP)):
        for t in leaves.values():
            t.grad = None
        parts = make_loss()
        sum(wi * p for wi, p in zip(w, parts) if wi != 0.0).backward()
        for k, t in leaves.items():
            out[f"{tag}:{k}"] = t.grad.numpy().copy()
    return out


def anm():
    c = anm_case(7, 3, 20, seed=41)
    assert sorted(set(c["L_true"].tolist())) == [0, 1, 2, 3] and not c["phi"][-1].any()
    crit = ref_loss.BasicANMLoss()
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("tau", "f", "conf", "phi")}

    def run():
        total, d = crit({"tau_est": leaves["tau"], "f_est": leaves["f"], "confidences": leaves["conf"], "phi_final": leaves["phi"]},
                        {"tau_true": c["tau_true"], "f_true": c["f_true"], "L_true": c["L_true"]})
        assert total is d["total_loss"]
        run.keys = list(d.keys())
        return d["total_loss"], d["param_loss"], d["reg_loss"]

    rec = {k: v.numpy() for k, v in c.items()}
    rec["out"] = np.array([float(p.detach()) for p in run()], dtype=np.float32)
    rec["param_only"] = np.float32(ref_loss.basic_parameter_loss(c["tau"], c["f"], c["tau_true"], c["f_true"], c["conf"], c["L_true"]))
    rec.update(grads(leaves, run))
    rec["up"] = np.array(UP)
    rec["lambda_reg"] = np.float64(crit.lambda_reg)
    rec["keys"] = np.array(run.keys)
    sig = names(ref_loss.BasicANMLoss, ref_loss.basic_parameter_loss)
    rec["sig_names"], rec["sig_values"] = np.array(list(sig)), np.array(list(sig.values()))
    save("loss_anm_b7", rec)


def phi():
    p, pt = phase_pair(5, 20, seed=43)
    crit = ref_loss.PhiAlignmentLoss()
    leaves = {"phi": p.clone().requires_grad_(True)}

    def run():
        total, d = crit(leaves["phi"], pt)
        assert total is d["total_loss"]
        run.keys = list(d.keys())
        return d["total_loss"], d["amplitude_loss"], d["phase_loss"]

    rec = {"phi": p.numpy(), "phi_true": pt.numpy()}
    rec["out"] = np.array([float(v.detach()) for v in run()], dtype=np.float32)
    rec.update(grads(leaves, run))
    rec["up"] = np.array(UP)
    rec["weights"] = np.array([crit.amplitude_weight, crit.phase_weight, crit.spectral_weight, crit.distribution_weight])
    rec["keys"] = np.array(run.keys)
    sig = names(ref_loss.PhiAlignmentLoss)
    rec["sig_names"], rec["sig_values"] = np.array(list(sig)), np.array(list(sig.values()))
    save("loss_phi_b5", rec)


if __name__ == "__main__":
    torch.set_num_threads(1)
    anm()
    phi()
