"""Host: the float64 statement of the model-order selection (``order.select_host``), the kernel's scalar core under sanitizers
(tests/host_model/order_model.cpp), the selection-and-refinement loop on the mirror, and the refusals and signatures of the new
entry points.  No GPU.

The mirror is what tests/test_gpu_order.py holds the kernel to, so it is itself held to things that do not depend on it: brute
force over subsets, exactly orthogonal atoms, and stand-ins with one defect each.
"""
import inspect
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from admm_net_amd import harness, modules, order

import order_cases as OC
import refine_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "admm_net_amd", "csrc")
HOST = os.path.join(HERE, "host_model")


def _x_and_atoms(c, i):
    s = c.b[i].astype(np.complex128)
    x = c.y[i].astype(np.complex128) * np.conj(s / np.abs(s))
    return x, order.atoms(c.rows[i, :, 0], c.rows[i, :, 1], c.grid)


# ---- 1. the mirror against brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1_of_1_1x12", "L2_of_6_12x1", "L1_of_6_4x6", "L3_of_6_8x8", "pair_0.35_cells", "penalty_0"])
def test_the_greedy_path_has_the_least_squares_residual_of_its_subset(name):
    """RSS_k of the greedy path = the residual of ``lstsq`` on the k rows picked, and no single row would have dropped it more."""
    c = OC.case(name)
    for i, r in enumerate(OC.reference(name)):
        x, A = _x_and_atoms(c, i)
        for k in range(r.ranked + 1):
            cols = A[:, r.perm[:k]]
            res = x - cols @ np.linalg.lstsq(cols, x, rcond=None)[0] if k else x
            assert math.isclose(float((np.abs(res) ** 2).sum()), r.rss[k], rel_tol=1e-10, abs_tol=1e-12 * r.rss[0]), (name, i, k)
            if k < r.ranked:
                for j in r.perm[k + 1:r.ranked]:
                    other = A[:, list(r.perm[:k]) + [j]]
                    rss = float((np.abs(x - other @ np.linalg.lstsq(other, x, rcond=None)[0]) ** 2).sum())
                    assert rss >= r.rss[k + 1] * (1 - 1e-10), (name, i, k, j)
        assert np.all(np.diff(r.rss[:r.ranked + 1]) <= 1e-12 * r.rss[0])


def test_on_orthogonal_atoms_the_greedy_pick_is_the_best_subset_of_every_size():
    c, r = OC.case("orthogonal_on_grid"), OC.reference("orthogonal_on_grid")[0]
    x, A = _x_and_atoms(c, 0)
    gram = A.conj().T @ A
    assert np.allclose(gram, 64 * np.eye(6), atol=1e-11)
    assert r.ranked == 6
    for k in range(1, 7):
        best = min(itertools.combinations(range(6), k),
                   key=lambda s: float((np.abs(x - A[:, s] @ np.linalg.lstsq(A[:, s], x, rcond=None)[0]) ** 2).sum()))
        assert sorted(best) == sorted(int(v) for v in r.perm[:k]), k
    assert r.n_sel == 3 and sorted(r.perm[:3]) == [0, 1, 2]


# ---- 2. the table ---------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    names = [c.name for c in OC.cases()]
    assert len(set(names)) == len(names) >= 20
    assert {c.rows.shape[1] for c in OC.cases()} >= {1, 6, 16}
    assert {c.grid for c in OC.cases()} >= {(1, 12), (12, 1), (4, 6), (8, 8), (16, 16), (13, 262)}
    ref = OC.reference
    assert {r.state for c in OC.cases() for r in ref(c.name)} == {order.RANKED, order.NONFINITE, order.OUTSIDE}
    for c in OC.cases():
        for i, r in enumerate(ref(c.name)):
            assert r.state == c.states[i], (c.name, i, r.state)
            if c.n_sel is not None and c.n_sel[i] is not None:
                assert r.n_sel == c.n_sel[i], (c.name, i, r.n_sel)
            assert sorted(r.perm) == list(range(c.rows.shape[1]))
    margins = {c.name: min(r.margin for r in ref(c.name)) for c in OC.cases()}
    print("the least decision margin per case:", {k: float(f"{v:.2g}") for k, v in margins.items()})
    assert min(margins.values()) > OC.MARGIN                                     # none is dropped
    r = ref("coincident_pair")[0]
    assert r.ranked == 5 and r.perm[-1] == 3 and list(r.perm).index(0) < 5       # the second of the pair is never ranked
    r = ref("pair_0.35_cells")[0]
    assert r.ranked == 6 and r.n_sel >= 3
    r = ref("absent_in_the_middle")[0]
    assert r.ranked == 4 and sorted(r.perm[4:]) == [1, 4]
    assert [q.ranked for q in ref("n_cand")] == [0, 2, 6, 3] and ref("n_cand")[0].rss[0] > 0
    for q in ref("n_held_2_not_the_best"):
        assert list(q.perm[:2]) == [0, 1] and q.n_sel >= 2
        free = OC.host(OC.case("n_held_2_not_the_best"), 0, n_held=None)
        assert list(free.perm[:2]) != [0, 1]                                     # held, not best
    r = ref("exact_tie")[0]
    assert list(r.perm) == [1, 2, 0] and math.isclose(r.rss[0] - r.rss[1], r.rss[1] - r.rss[2], rel_tol=0.2)
    r = ref("noiseless_below_the_floor")[0]
    assert r.rss[1] < order.RSS_FLOOR * r.rss[0] and r.n_sel == 1 and r.ranked == 2
    assert all(q.n_sel == q.ranked == 6 for q in ref("penalty_0"))
    assert [q.n_sel for q in ref("huge_penalty")] == [1, 0]
    assert all(q.ranked == 2 for q in ref("max_order_2"))
    c = OC.case("symbols_given")                                                 # the symbols are used, b is not
    with_b = order.select_host(c.y[0], RC.refine.psk_points(*OC.PSK)[c.symbols[0]], c.rows[0], c.grid)
    assert np.array_equal(with_b.perm, ref("symbols_given")[0].perm) and math.isclose(with_b.cost, ref("symbols_given")[0].cost, rel_tol=1e-6)


# ---- 3. the host model under sanitizers -------------------------------------------------------------------------------------------------
def _num(v):
    return repr(float(v))


def test_order_core_under_sanitizers(tmp_path):
    """tests/host_model/order_model.cpp (its own main, csrc/order_core.h with the workgroup emulated, built with
    -fsanitize=address,undefined) on every scene of the case table, held to ``select_host`` as the kernel is."""
    exe, inp = str(tmp_path / "order_model"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "order_model.cpp"), "-o", exe])
    lines, scenes = [], 0
    for c in OC.cases():
        Le = c.rows.shape[1]
        for i in range(len(c.y)):
            word = lambda v: "none" if v is None else int(v[i])  # noqa: E731
            penalty = order.default_penalty(c.grid) if c.penalty is None else c.penalty
            lines.append(f"{c.grid[0]} {c.grid[1]} {Le} {word(c.n_cand)} {word(c.n_held)} {int(c.symbols is not None)} {OC.PSK[0]} "
                         f"{OC.PSK[1]!r} {penalty!r} {Le if c.max_order is None else c.max_order}")
            lines += [" ".join(_num(v) for v in row) for row in c.rows[i]]
            sym = np.zeros(len(c.y[i]), int) if c.symbols is None else c.symbols[i]
            lines += [f"{_num(a.real)} {_num(a.imag)} {_num(s.real)} {_num(s.imag)} {int(k)}" for a, s, k in zip(c.y[i], c.b[i], sym)]
            scenes += 1
    with open(inp, "w") as fh:
        fh.write(f"{scenes}\n" + "\n".join(lines) + "\n")
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-500:] + p.stderr)[-3000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = iter(p.stdout.split("\n"))
    worst = {}
    for c in OC.cases():
        B, Le = c.rows.shape[:2]
        D = c.y.shape[1]
        perm, n_sel, rss = np.zeros((B, Le), int), np.zeros(B, int), np.zeros((B, Le + 1))
        rows, C, res, info = np.zeros((B, Le, 3)), np.zeros((B, Le), complex), np.zeros((B, D), complex), np.zeros((B, 4))
        for i in range(B):
            state, K, n, cost = next(out).split()
            n_sel[i], info[i] = int(n), [float(cost), float(cost) / D, int(K), int(state)]
            perm[i] = [int(t) for t in next(out).split()]
            rss[i] = [float(t) for t in next(out).split()]
            for j in range(Le):
                v = [float(t) for t in next(out).split()]
                rows[i, j], C[i, j] = v[:3], complex(v[3], v[4])
            for k in range(D):
                v = next(out).split()
                res[i, k] = complex(float(v[0]), float(v[1]))
        worst[c.name] = OC.compare(c.name, perm, n_sel, rss, rows, C, res, info, "host model")
    print("worst (rss / RSS_0, C / max |C|) against the mirror:", {k: (float(f"{a:.2g}"), float(f"{b:.2g}")) for k, (a, b) in worst.items()})
    seen = (max(a for a, _ in worst.values()), max(b for _, b in worst.values()))
    print("the largest:", seen, "recorded:", (OC.RSS_SEEN, OC.C_SEEN))


# ---- 4. one mistake is rejected ---------------------------------------------------------------------------------------------------------
def _same(name, got, i=0):
    r = OC.reference(name)[i]
    return np.array_equal(got.perm, r.perm) and got.n_sel == r.n_sel and got.ranked == r.ranked


def test_one_mistake_is_rejected(monkeypatch):
    """Stand-ins -- the mirror with ONE of its parts replaced by a defective one -- are each rejected by a named case: held to the
    table's reference the way the kernel is, they fail."""
    atoms, pick, held = order.atoms, order.pick_next, order.held_in_order

    def tau_sign(tau, f, grid):
        return atoms(-np.asarray(tau), f, grid)

    def exchanged(tau, f, grid):                         # i = i_d Nb + i_b
        idx = np.arange(grid[0] * grid[1]).reshape(grid).T.reshape(-1)
        return atoms(tau, f, grid)[idx]

    def undivided(gains, norms, eligible, D):            # |a~^H r|^2 instead of |a~^H r|^2 / |a~|^2
        return pick({j: gains[j] * norms[j] for j in gains}, norms, eligible, D)

    def larger_index(gains, norms, eligible, D):         # ties to the LARGER index
        j, gap = pick({-k: v for k, v in gains.items()}, {-k: v for k, v in norms.items()}, [-k for k in reversed(eligible)], D)
        return (None if j is None else -j), gap

    stand_ins = {
        "the sign of tau in the atom": ("atoms", tau_sign, "L3_of_6_8x8"),
        "i_b and i_d exchanged": ("atoms", exchanged, "L1_of_6_4x6"),
        "the gain not divided by |a~|^2": ("pick_next", undivided, "duplicate_before_the_weak_target"),
        "the held rows re-ordered": ("held_in_order", lambda h: list(reversed(h)), "n_held_2_not_the_best"),
        "ties to the larger index": ("pick_next", larger_index, "exact_tie"),
    }
    for what, (name, stand_in, case) in stand_ins.items():
        assert _same(case, OC.host(OC.case(case), 0)), case                  # the mirror itself passes ...
        with monkeypatch.context() as mp:
            mp.setattr(order, name, stand_in)
            rejected = not _same(case, OC.host(OC.case(case), 0))
        print(f"{what}: rejected by {case}")
        assert rejected, what                                                # ... and the stand-in does not
    assert (order.atoms, order.pick_next, order.held_in_order) == (atoms, pick, held)


# ---- 5. the loop on the mirror ----------------------------------------------------------------------------------------------------------
LOOP_DRAWS = 400


def test_a_second_round_selects_better_than_the_first():
    """The 8 x 8 scene at 15 dB, six candidates (order_cases.monte_carlo): the share of draws with exactly the three displaced
    truths selected is larger after the second selection (the first one's rows refined) than after the first, and the share with
    too many rows is smaller.  Measured over 2000 draws: right 0.833 -> 0.9465, too many 0.155 -> 0.033; over the 400 draws used
    here: 0.835 -> 0.9375 and 0.155 -> 0.0375."""
    first, second = OC.mirror_loop(LOOP_DRAWS)
    s1, s2 = OC.shares(first[0]), OC.shares(second[0])
    print(f"{LOOP_DRAWS} draws: (right, too many, other) after round 1 {s1}, after round 2 {s2}")
    assert s2[0] > s1[0] and s2[1] < s1[1]


# ---- 6. arguments and signatures --------------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_statement():
    c = OC.case("L3_of_6_8x8")
    for kw in (dict(psk=(1, 0.0)), dict(psk=(65, 0.0)), dict(psk=(4, math.inf)), dict(psk=4), dict(penalty=-1.0), dict(penalty=math.nan),
               dict(penalty=math.inf), dict(max_order=0), dict(max_order=7), dict(max_order=2.5)):
        with pytest.raises(ValueError):
            order.select_host(c.y[0], c.b[0], c.rows[0], c.grid, **kw)
    for grid in ((8,), (0, 64), (4, 8)):
        with pytest.raises(ValueError):
            order.select_host(c.y[0], c.b[0], c.rows[0], grid)
    with pytest.raises(ValueError):
        order.select_host(c.y[0], c.b[0], np.zeros((17, 3)), c.grid)
    with pytest.raises(TypeError):
        order.select_targets(c.y, c.b, c.rows, c.grid)                # numpy arrays: the device call takes tensors
    import torch
    with pytest.raises(order._lib.AdmmNetError):                       # ... on the device: no CPU fallback
        order.select_targets(torch.from_numpy(c.y), torch.from_numpy(c.b), torch.from_numpy(c.rows), c.grid)
    with pytest.raises(order._lib.AdmmNetError):
        order.select_refined(torch.from_numpy(c.y), torch.from_numpy(c.b), torch.from_numpy(c.rows), c.grid)
    for kw in (dict(symbols="qam"), dict(rounds=-1), dict(grow=1.5)):
        with pytest.raises(ValueError):
            order.select_refined(torch.from_numpy(c.y), torch.from_numpy(c.b), torch.from_numpy(c.rows), c.grid, **kw)


def test_signatures():
    import admm_net_amd
    assert admm_net_amd.order is order and admm_net_amd.select_targets is order.select_targets
    sig = inspect.signature(order.select_targets)
    assert list(sig.parameters) == ["y", "b", "rows", "grid", "n_cand", "n_held", "symbols", "psk", "penalty", "max_order", "out"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[4:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[4:]] == [None, None, None, (4, math.pi / 4), None, None, None]
    assert list(inspect.signature(order.select_host).parameters) == list(sig.parameters)[:-1]
    s = inspect.signature(order.select_refined)
    assert list(s.parameters) == ["y", "b", "rows", "grid", "rounds", "grow", "symbols", "penalty", "peak_opts", "refine_kw"]
    assert [s.parameters[k].default for k in ("rounds", "grow", "symbols", "penalty", "peak_opts")] == [2, 0, "given", None, None]
    assert s.parameters["refine_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert order.OrderResult._fields == ("perm", "n_sel", "rss", "rows_out", "C", "residual", "cost", "noise_var", "ranked", "state",
                                         "status")
    assert order.default_penalty((8, 8)) == 4 * math.log(64) and (order.NONFINITE, order.OUTSIDE) == (3, 4)
    for cls in (modules.PhiEstADMMNet, modules.ADMMNet):
        s = inspect.signature(cls.estimate_selected)
        assert list(s.parameters) == ["self", "y", "b", "sigma", "top", "opts", "rounds", "grow", "symbols", "penalty", "refine_kw"]
        assert all(s.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rounds", "grow", "symbols", "penalty"))
        assert [s.parameters[k].default for k in ("top", "opts", "rounds", "grow", "symbols", "penalty")] == [None, None, 2, 0, "given", None]
    p = inspect.signature(harness.evaluate_snr).parameters
    assert list(p)[-3:] == ["order", "refine", "crb"] and p["order"].default is None


def test_order_on_the_command_line(monkeypatch):
    seen, evaluate_snr = [], harness.evaluate_snr
    monkeypatch.setattr(harness, "evaluate_snr", lambda *a, **kw: seen.append(kw) or iter(()))
    harness.main(["evaluate", "--order", "6", "--refine", "psk"])
    harness.main(["evaluate"])
    assert [(kw["order"], kw["refine"]) for kw in seen] == [(6, "psk"), (None, None)]
    for bad in (0, 17, 2):                                             # 1 .. 16 and at least the targets (3)
        with pytest.raises(ValueError):
            next(evaluate_snr(order=bad))
