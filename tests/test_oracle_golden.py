"""CPU: the oracle restatement vs the golden vectors generated from the imported reference."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import admm_net_ref as R

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
CASES = [p for p in GOLD if os.path.basename(p).startswith(("phiest_", "admmnet_"))]
TOL_F32 = 2e-5      # oracle fp32 vs reference fp32: same formulas, different BLAS/LAPACK call order
TOL_F64 = 5e-5      # reference fp32 vs ground truth fp64
TRAINED = [p for p in CASES if p.endswith("_trained.npz")]
UNTRAINED = [p for p in CASES if p not in TRAINED]


from golden_util import load_fixture as load   # weights stored, or rebuilt by seed and checksum-verified


def test_depth_fixtures_present():
    """Reference-made fixtures at the depth of the BASELINE configs (K = 8 on 8x16, K = 16 / 32 on 16x16)."""
    names = {os.path.basename(p)[:-4] for p in CASES}
    assert {"phiest_8x16_K8_perturbed", "phiest_16x16_K16_default", "phiest_16x16_K16_perturbed",
            "phiest_16x16_K32_default"} <= names


def test_fixture_inventory():
    assert len(CASES) >= 10
    assert any("16x16" in p for p in CASES) and any("8x16" in p for p in CASES) and any("10x10" in p for p in CASES)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_oracle_matches_reference(path):
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load(path)
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    for dt, tol in (("f32", TOL_F32), ("f64", TOL_F64)):
        tr = []
        out = R.forward(sd, y, b, s, Nb, Nd, K, L, dtype=dt, head=bool(head), trace=tr)
        phi = (out[3] if head else out).numpy()
        ref = z["phi"]
        assert np.abs(phi - ref).max() <= tol * np.abs(ref).max()
        if head:
            for i, key in enumerate(["tau", "f", "conf"]):
                assert np.abs(out[i].numpy() - z[key]).max() <= 1e-5
        if "L0:phi" in z.files:      # per-layer traces for the tiny cases
            for k in range(K):
                for key in ("phi", "h", "G", "Z"):
                    a, r = tr[k][key].numpy(), z[f"L{k}:{key}"]
                    assert np.abs(a - r).max() <= 5e-5 * max(1.0, np.abs(r).max()), (k, key)


@pytest.mark.parametrize("path", UNTRAINED[:4], ids=[os.path.basename(p)[:-4] for p in UNTRAINED[:4]])
def test_dead_tail_is_dead(path):
    """admm_net.py:757-764: the last layer's H/G/Z never reach the output."""
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load(path)
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    a = R.forward(sd, y, b, s, Nb, Nd, K, L)
    c = R.forward(sd, y, b, s, Nb, Nd, K, L, skip_dead_tail=True)
    assert torch.equal(a, c)


def test_batch_mean_couples_signals():
    """splitting the batch changes phi (reference measured 1.2e-4 on this fixture)."""
    p = [q for q in GOLD if "split" in q][0]
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load(p)
    y, b, s = torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"])
    full = R.forward(sd, y, b, s, Nb, Nd, K).numpy()
    split = np.concatenate([R.forward(sd, y[:3], b[:3], s[:3], Nb, Nd, K).numpy(),
                            R.forward(sd, y[3:], b[3:], s[3:], Nb, Nd, K).numpy()])
    assert np.abs(full - z["phi_full"]).max() < 2e-6
    assert np.abs(split - z["phi_split"]).max() < 2e-6
    assert np.abs(full - split).max() > 1e-5


def test_trained_fixtures_present():
    """Weights moved by training (tests/golden/make_golden.py --trained-only) at D = 100, 128 and 256."""
    names = {os.path.basename(p)[:-4] for p in TRAINED}
    assert {"phiest_10x10_K10_trained", "phiest_8x16_K8_trained", "phiest_16x16_K4_trained"} <= names


MIN_SCALAR_MOVE = 1e-2   # |trained - init| of every gLayers.k.threshold and rho that has a gradient
MIN_KINK_MOVE = 1e-2     # max |(-b_j / w_j)_trained - (-b_j / w_j)_init| / max|lambda| over the kinks among the eigenvalues


@pytest.mark.parametrize("path", TRAINED, ids=[os.path.basename(p)[:-4] for p in TRAINED])
def test_trained_fixture_moved_away_from_init(path):
    """A regeneration must not commit near-init weights: the seeded init, rebuilt with the drop-in module (bit-equal to the
    reference's, tests/test_host_logic.py), differs from the stored weights in every G-layer scalar and in the positions of
    value_net's kinks (where f(w) = softplus(w - thr) sigmoid(value_net(|w|)) bends), and the training loss came down.
    Parameters without a gradient are exempt: the G-layer of the last layer (its G never reaches phi, test_dead_tail_is_dead)
    and the rho of layer 0 (Z = 0 there, so A = C - Z / rho is C) only decay; lambda_param never moves, because the reference
    reads it through .item() (admm_net.py:269-271) -- that is checked too."""
    import admm_net_amd as A
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load(path)
    seed, steps, batch, lr, first, last = (float(v) for v in z["train"][:6])
    losses = z["train_loss"]
    assert len(losses) == int(steps) and losses[0] == np.float32(first) and losses[-1] == np.float32(last)
    torch.manual_seed(int(seed))
    init = A.PhiEstADMMNet(M=Nb, N=Nd, L=L, num_layers=K).state_dict()
    assert set(init) == set(sd)
    for k in range(K):
        for name in (f"gLayers.{k}.lambda_param", f"zLayers.{k}.lambda_param"):
            assert torch.equal(sd[name], init[name]), name
    tr = []
    R.forward(sd, torch.from_numpy(z["y"]), torch.from_numpy(z["b"]), torch.from_numpy(z["sigma"]), Nb, Nd, K, L, dtype="f64",
              trace=tr)
    moves, kink_moves = [], []
    for k in range(K - 1):
        for key in ("threshold", "rho") if k else ("threshold",):
            name = f"gLayers.{k}.{key}"
            moves.append((abs(float(sd[name]) - float(init[name])), name))
        # value_net's kinks |w| = -b_j / w_j that can meet an eigenvalue of this layer (|w| within the largest |lambda| of the
        # held-out batch, before or after training): the largest of their moves, relative to that range.  (Not the median: a
        # unit that is never active gets no gradient, and weight decay scales w_j and b_j alike, so its kink stays put.)
        p = f"gLayers.{k}.value_net."
        kinks = [-s[p + "0.bias"].double() / s[p + "0.weight"].double().reshape(-1) for s in (sd, init)]
        top = float(tr[k]["w"].abs().max())
        live = ((kinks[0] >= 0) & (kinks[0] <= top)) | ((kinks[1] >= 0) & (kinks[1] <= top))
        assert live.any(), (k, "no kink of value_net within the eigenvalues")
        kink_moves.append((float((kinks[0] - kinks[1])[live].abs().max()) / top, k))
    print(f"{os.path.basename(path)}: smallest scalar move {min(moves)}, smallest kink move {min(kink_moves)}, "
          f"loss {first:.4f} -> {last:.4f}")
    assert min(moves)[0] >= MIN_SCALAR_MOVE, min(moves)
    assert min(kink_moves)[0] >= MIN_KINK_MOVE, min(kink_moves)
    assert last < first and losses[-10:].mean() < losses[:10].mean(), (first, last)


def test_make_weights_keys_match_reference():
    z, sd, (Nb, Nd, K, B, L, head, s2d) = load([p for p in CASES if "admmnet_10x10" in p][0])
    mine = R.make_weights(Nb, Nd, K, L, seed=1, head=True)
    assert set(mine.keys()) == set(sd.keys())
    for k in sd:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
