"""Host: the float64 statement of successive cancellation on the periodogram (``detect.cfar_relax_host``), the kernel's scalar core
under sanitizers (tests/host_model/relax_model.cpp), stand-ins with one mistake each, the margin on the Monte-Carlo law, and the
refusals, signatures and command line of the new entry points.  No GPU.

The mirror is what tests/test_gpu_relax.py holds the kernel to, so it is itself held to things that do not depend on it: a
brute-force maximum of the matched filter on a fine grid, and what the case table is built to show.
"""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from admm_net_amd import build, detect, harness

import detect_cases as DC
import relax_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "admm_net_amd", "csrc")
HOST = os.path.join(HERE, "host_model")


# ---- 1. the fit against a brute-force maximum -------------------------------------------------------------------------------------------
def test_the_fit_finds_the_maximum_of_the_matched_filter():
    """One target 0.3 map cells off its cell on both axes in noise: eight Newton steps from the cell end, inside the box, within
    1e-6 of a map cell of the best point of a 801 x 801 grid over the box refined twice (to 1.6e-6 of the box), and the gradient
    the steps use vanishes there."""
    grid, r = (8, 8), 2
    rng = np.random.default_rng(5)
    tau0, f0 = RC.on(11, 5)
    y, s, _ = DC.scene(grid, [tau0 + 0.3 / 16], [f0 + 0.3 / 16], [1.0 + 0.5j], 0.05, rng)
    x = y * np.conj(s)
    tau, f, S, margin, not_definite, clamped = detect.fit(x, grid, r, tau0, f0, 8)
    assert not_definite == 0 and margin > 1e-3
    ib, idd = np.divmod(np.arange(64), 8)
    lo_t, hi_t, lo_f, hi_f = tau0 - 0.5 / 16, tau0 + 0.5 / 16, f0 - 0.5 / 16, f0 + 0.5 / 16
    for _ in range(3):
        ts, fs = np.linspace(lo_t, hi_t, 801), np.linspace(lo_f, hi_f, 801)
        A = np.exp(-2j * np.pi * np.multiply.outer(fs, ib)) * x                      # [f, D]
        F = np.abs(A @ np.exp(2j * np.pi * np.multiply.outer(idd, ts))) ** 2         # [f, tau]
        jf, jt = np.unravel_index(F.argmax(), F.shape)
        bt, bf = ts[jt], fs[jf]
        wt, wf = (hi_t - lo_t) / 40, (hi_f - lo_f) / 40
        lo_t, hi_t, lo_f, hi_f = bt - wt, bt + wt, bf - wf, bf + wf
    print("fit", tau, f, "brute force", bt, bf, "in map cells off:", (tau - bt) * 16, (f - bf) * 16)
    assert abs(tau - bt) * 16 < 1e-6 and abs(f - bf) * 16 < 1e-6
    assert math.isclose(abs(S) ** 2, F.max(), rel_tol=1e-9)
    d_tau, d_f, definite, _ = detect.newton_step(detect.moments(x, tau, f, grid), grid)
    assert definite and abs(d_tau) * 16 < 1e-9 and abs(d_f) * 16 < 1e-9
    # iters = 0 leaves the grid point; the amplitude is the least-squares one
    t0, g0, S0, *_ = detect.fit(x, grid, r, tau0, f0, 0)
    assert (t0, g0) == (tau0, f0) and math.isclose(abs(S0 - np.vdot(detect.atom(tau0, f0, grid), x)), 0.0, abs_tol=1e-12)


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    names = [c.name for c in RC.cases()]
    ref = RC.reference
    assert len(set(names)) == len(names)
    shapes = {(c.grid, c.kw["oversample"]) for c in RC.cases()}
    assert shapes >= {((1, 12), 2), ((12, 1), 2), ((4, 6), 3), ((5, 7), 3), ((8, 8), 1), ((8, 8), 2), ((16, 16), 4), ((13, 262), 1)}
    for grid, r in (((16, 16), 4), ((13, 262), 1)):                                  # the two large shapes once each, B = 1
        assert [len(c.y) for c in RC.cases() if (c.grid, c.kw["oversample"]) == (grid, r)] == [1]
    for g in RC.GRIDS:
        assert {c.kw["method"] for c in RC.cases() if (c.grid, c.kw["oversample"]) == (g[0], g[1])} == set(detect.METHODS)
    margins = {}
    for c in RC.cases():
        assert c.exempt == ()
        for i, r in enumerate(ref(c.name)):
            assert r.state == c.states[i], (c.name, i, r.state)
        margins[c.name] = min(r.margin for r in ref(c.name))
    print("the least decision margin per case:", {k: float(f"{v:.2g}") for k, v in margins.items()})
    assert [k for k, v in margins.items() if not v > RC.MARGIN] == []                # the cap on cases left out is 0
    assert {r.state for c in RC.cases() for r in ref(c.name)} == {detect.DONE, detect.NONFINITE, detect.OUTSIDE}
    cell = np.array(RC.on(11, 5))
    r = ref("on_cell")[0]
    assert (r.n_det, r.maps, r.more) == (1, 2, 0) and np.abs(r.rows[0, :2] - cell).max() * 16 < 1e-6
    assert math.isclose(abs(r.amp[0] - (1.0 + 0.5j)), 0.0, abs_tol=1e-6)
    r = ref("half_cell")[0]
    assert r.clamped >= 1 and np.abs(r.rows[0, :2] - cell - 0.5 / 16).max() * 16 < 0.1
    r = ref("near_bound")[0]
    assert r.n_det == 1 and np.abs(r.rows[0, :2] - cell - 0.4 / 16).max() * 16 < 1e-5
    for method in ("ca", "os"):                                                      # both wraps, from cell (0, 0)
        c = RC.case(f"wraps_{method}")
        assert tuple(RC.host(c, 0, iters=0, sweeps=0).rows[0, :2]) == (0.0, -0.5)
        r = ref(c.name)[0]
        assert 1 - 0.5 / 16 <= r.rows[0, 0] < 1 and 0.5 - 0.5 / 16 <= r.rows[0, 1] < 0.5
    assert ref("close_pair_sweeps_0")[0].n_det > 2 and ref("close_pair_sweeps_2")[0].n_det == 2        # what the sweeps are for
    assert np.array_equal(RC.case("close_pair_sweeps_0").y, RC.case("close_pair_sweeps_2").y)
    near = lambda r, tau, f: any(abs(row[0] - tau) * 8 < 0.25 and abs(row[1] - f) * 8 < 0.25 for row in r.rows[:r.n_det])  # noqa: E731
    for tau, f in zip(*RC.CLOSE[:2]):
        assert near(ref("close_pair_sweeps_2")[0], tau, f)
    tau, f, _ = DC.case("masked_pair_ca").truth[0]
    plain = DC.reference("masked_pair_ca")[0]
    assert not any(tuple(row[:2]) == (tau[1], f[1]) for row in plain.rows)           # cfar_targets with "ca" misses the weaker one
    assert near(ref("masked_pair_ca")[0], tau[0], f[0]) and near(ref("masked_pair_ca")[0], tau[1], f[1])
    for name, Le in (("more_than_Le", 1), ("more_than_Le_2", 2)):
        assert (ref(name)[0].n_det, ref(name)[0].more, ref(name)[0].maps, RC.case(name).kw["top"]) == (Le, 1, Le + 1, Le)
    r, first = ref("masked_centre")[0], RC.host(RC.case("masked_centre"), 0, top=1, iters=0, sweeps=0)
    centre = (RC.BLOCK[0][4], RC.BLOCK[1][4])
    P0 = detect.cfar_host(RC.case("masked_centre").y[0], RC.case("masked_centre").b[0], (8, 8), top=6, oversample=2, pfa=1e-3).map
    j, i = np.unravel_index(P0.argmax(), P0.shape)
    assert (i / 16, j / 16 - 0.5) == centre and tuple(first.rows[0, :2]) != centre and r.more == 1   # the highest cell is not over
    assert (ref("Le_1")[0].n_det, ref("Le_1")[0].more) == (1, 0)
    assert all((r.n_det, r.maps) == (0, 1) for r in ref("no_detection") + ref("silence"))
    assert not RC.case("silence").y.any() and ref("silence")[0].resid == 0.0
    k = RC.case("on_grid_clean").kw
    assert (k["iters"], k["sweeps"]) == (0, 0) and RC.case("plain_clean").kw["sweeps"] == 0 and RC.case("plain_clean").kw["iters"] == 3
    r = ref("on_grid_clean")[0]
    assert np.allclose(r.rows[:r.n_det, :2] * 16, np.round(r.rows[:r.n_det, :2] * 16), atol=1e-12)     # grid points
    assert ref("not_definite")[0].not_definite >= 1
    assert max(r.n_det for c in RC.cases() for r in ref(c.name)) >= 5 and any(r.clamped for r in ref("os_5x7_r3"))


# ---- 3. the host model under sanitizers -------------------------------------------------------------------------------------------------
def _num(v):
    return repr(float(v))


def test_relax_core_under_sanitizers(tmp_path):
    """tests/host_model/relax_model.cpp (its own main, csrc/relax_core.h with the workgroup emulated, built with
    -fsanitize=address,undefined) on every scene of the case table, held to ``cfar_relax_host`` as the kernel is."""
    exe, inp = str(tmp_path / "relax_model"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "relax_model.cpp"), "-o", exe])
    lines, scenes = [], 0
    for c in RC.cases():
        k = c.kw
        N = detect.train_count(c.grid, k["guard"], k["train"])
        rank = detect.default_rank(N) if k["rank"] is None else k["rank"]
        alpha = detect.cfar_alpha(k["method"], N, k["pfa"], rank if k["method"] == "os" else None)
        for i in range(len(c.y)):
            noise = "none" if c.noise_var is None else _num(c.noise_var[i])
            lines.append(f"{c.grid[0]} {c.grid[1]} {k['oversample']} {k['top']} {detect.METHODS[k['method']]} {k['guard']} {k['train']} "
                         f"{rank} {alpha!r} {int(c.symbols is not None)} {RC.PSK[0]} {RC.PSK[1]!r} {noise} {k['iters']} {k['sweeps']}")
            sym = np.zeros(len(c.y[i]), int) if c.symbols is None else c.symbols[i]
            lines += [f"{_num(a.real)} {_num(a.imag)} {_num(s.real)} {_num(s.imag)} {int(q)}" for a, s, q in zip(c.y[i], c.b[i], sym)]
            scenes += 1
    with open(inp, "w") as fh:
        fh.write(f"{scenes}\n" + "\n".join(lines) + "\n")
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-500:] + p.stderr)[-3000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    out = iter(p.stdout.split("\n"))
    worst = {}
    for c in RC.cases():
        B, Le = len(c.y), c.kw["top"]
        nf, nt = c.cells
        rows, amp, pmap = np.zeros((B, Le, 3)), np.zeros((B, Le), complex), np.zeros((B, nf, nt))
        n_det, more, maps, state = (np.zeros(B, int) for _ in range(4))
        level, resid = np.zeros(B), np.zeros(B)
        for i in range(B):
            st, nd, mo, mp, lv, rs = next(out).split()
            state[i], n_det[i], more[i], maps[i], level[i], resid[i] = int(st), int(nd), int(mo), int(mp), float(lv), float(rs)
            for j in range(Le):
                v = [float(t) for t in next(out).split()]
                rows[i, j], amp[i, j] = v[:3], complex(v[3], v[4])
            pmap[i] = np.array([float(next(out)) for _ in range(nf * nt)]).reshape(nf, nt)
        worst[c.name] = RC.compare(c.name, rows, amp, n_det, more, maps, level, resid, state, pmap, "host model")
    print("worst (point in resolution cells, power / E, amp / sqrt(E / D)) against the mirror:",
          {k: tuple(float(f"{a:.2g}") for a in v) for k, v in worst.items()})
    print("the largest:", tuple(max(v[k] for v in worst.values()) for k in range(3)), "recorded:",
          (RC.POINT_SEEN, RC.POWER_SEEN, RC.AMP_SEEN))


# ---- 4. one mistake is rejected ---------------------------------------------------------------------------------------------------------
def _same(name, got, i=0):
    c, r = RC.case(name), RC.reference(name)[i]
    if (got.n_det, got.more, got.maps, got.state) != (r.n_det, r.more, r.maps, r.state):
        return False
    d = RC.differences(c, i, r, got.rows, got.amp, got.level, got.resid, got.map)
    return d[0] <= RC.POINT_TOL and d[1] <= RC.POWER_TOL and d[2] <= RC.AMP_TOL


def test_one_mistake_is_rejected(monkeypatch):
    """Stand-ins -- the mirror with ONE of its parts replaced by a defective one -- are each rejected by a named case: held to the
    table's reference the way the kernel is, they fail."""
    parts = ("add_back", "amplitude", "newton_step", "clamp_box", "threshold_map", "candidates", "limit_reached")
    kept = {k: getattr(detect, k) for k in parts}
    step, box = kept["newton_step"], kept["clamp_box"]

    def wrong_sign(mom, grid):
        d_tau, d_f, definite, gap = step(mom, grid)
        return -d_tau, -d_f, definite, gap

    stand_ins = {
        "no add-back in the sweep": ("add_back", lambda x, c, a: x, "close_pair_sweeps_2"),
        "c without / D": ("amplitude", lambda S, D: S, "Le_1"),
        "the Newton step with the wrong sign": ("newton_step", wrong_sign, "near_bound"),
        "the clamp box in resolution cells": ("clamp_box", lambda grid, r: box(grid, 1), "half_cell"),
        "the threshold from the round-0 map": ("threshold_map", lambda P, first: first, "masked_pair_ca"),
        "the global maximum instead of the highest over cell": ("candidates", lambda P, over: P, "masked_centre"),
        "the k == Le test after the fit": ("limit_reached", lambda n, Le, fitted: n == Le and fitted, "more_than_Le"),
    }
    for what, (name, stand_in, case) in stand_ins.items():
        assert _same(case, RC.host(RC.case(case), 0)), case                  # the mirror itself passes ...
        with monkeypatch.context() as mp:
            mp.setattr(detect, name, stand_in)
            rejected = not _same(case, RC.host(RC.case(case), 0))
        print(f"{what}: rejected by {case}")
        assert rejected, what                                                # ... and the stand-in does not
    assert all(getattr(detect, k) is v for k, v in kept.items())


# ---- 5. the margin on the Monte-Carlo law -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targets", [False, True])
def test_the_mirror_holds_the_margin_on_the_monte_carlo_draws(targets):
    """8 x 8, r = 2, 2000 draws, noise only and with 1 .. 3 targets at 15 dB: the share of draws whose decisions all have the
    margin, per method, is at least 99 %."""
    y, b, noise_var = DC.monte_carlo(targets)
    for method in detect.METHODS:
        n_det, more, maps, margin = RC.mc_host(y, b, noise_var, method)
        share = float((margin > RC.MARGIN).mean())
        print(f"targets={targets} {method}: share with the margin {share}, least margin {margin.min():.2g}, mean n_det "
              f"{n_det.mean():.3f}, mean maps {maps.mean():.3f}, more in {int(more.sum())}")
        assert share >= 1 - RC.MC_LEFT_OUT


# ---- 6. arguments and signatures --------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    c = RC.case("ca_8x8_r2")
    y, b = torch.from_numpy(c.y), torch.from_numpy(c.b)
    bad = (dict(top=0), dict(top=17), dict(top=2.0), dict(oversample=0), dict(oversample=9), dict(method="go"), dict(pfa=0.0),
           dict(pfa=1.0), dict(guard=-1), dict(train=0), dict(guard=1, train=3), dict(guard=5, train=4), dict(rank=3),
           dict(method="os", rank=41), dict(noise_var=1.0), dict(method="known"), dict(method="known", noise_var="x"),
           dict(method="known", noise_var=torch.ones(3)), dict(psk=(1, 0.0)), dict(psk=4),
           dict(symbols=torch.zeros(2, 64)), dict(symbols=torch.zeros(2, 63, dtype=torch.int32)),
           dict(iters=-1), dict(iters=17), dict(iters=2.0), dict(iters=True), dict(sweeps=-1), dict(sweeps=9), dict(sweeps=1.5),
           dict(out=torch.zeros(2, 6, 3, dtype=torch.float32)), dict(out=torch.zeros(2, 5, 3, dtype=torch.float64)),
           dict(out=torch.zeros(2, 6, 6, dtype=torch.float64)[:, :, ::2]))
    for kw in bad:
        with pytest.raises(ValueError):
            detect.cfar_relax(y, b, (8, 8), **{**dict(top=6, oversample=2), **kw})
    for grid in ((8,), (0, 64), (4, 8), (64, 64)):
        with pytest.raises(ValueError):
            detect.cfar_relax(y, b, grid, top=6, oversample=1, guard=0, train=1)
    with pytest.raises(ValueError):                                    # 25 x 25 at r = 4 does not fit the LDS
        detect.cfar_relax(torch.zeros(1, 625, dtype=torch.complex64), torch.ones(1, 625, dtype=torch.complex64), (25, 25), oversample=4)
    with pytest.raises(ValueError):
        detect.cfar_relax(y.real, b, (8, 8))
    with pytest.raises(TypeError):
        detect.cfar_relax(c.y, c.b, (8, 8))                            # numpy arrays: the device call takes tensors
    with pytest.raises(detect._lib.AdmmNetError):                      # ... on the device: no CPU fallback
        detect.cfar_relax(y, b, (8, 8), top=6, oversample=2)
    for kw in (dict(top=0), dict(method="known"), dict(iters=17), dict(sweeps=9)):
        with pytest.raises(ValueError):
            detect.cfar_relax_host(c.y[0], c.b[0], (8, 8), **kw)
    with pytest.raises(ValueError):
        detect.cfar_relax_host(c.y[0][:5], c.b[0][:5], (8, 8))
    for kw in (dict(cancel=True), dict(baseline="periodogram", cancel=(17, 2)), dict(baseline="periodogram", cancel=(3, 9)),
               dict(baseline="periodogram", cancel=3), dict(baseline="classical", cancel=(3, 2))):
        with pytest.raises(ValueError):
            next(harness.evaluate_snr(**kw))


def test_signatures():
    import admm_net_amd
    assert admm_net_amd.cfar_relax is detect.cfar_relax and admm_net_amd.cfar_relax_host is detect.cfar_relax_host
    assert {"cfar_relax", "cfar_relax_host"} <= set(admm_net_amd.__all__)
    old = inspect.signature(detect.cfar_targets)
    assert list(old.parameters) == ["y", "b", "grid", "top", "oversample", "method", "pfa", "guard", "train", "rank", "noise_var",
                                    "symbols", "psk", "return_map", "out"]                                  # unchanged
    sig = inspect.signature(detect.cfar_relax)
    assert list(sig.parameters) == list(old.parameters)[:13] + ["iters", "sweeps", "return_map", "out"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [16, 4, "ca", 1e-4, 1, 2, None, None, None,
                                                                            (4, math.pi / 4), 3, 2, False, None]
    host = list(inspect.signature(detect.cfar_relax_host).parameters)
    assert host == list(sig.parameters)[:15] + ["exempt"]
    assert detect.CfarRelaxResult._fields == ("rows", "amp", "n_det", "more", "maps", "level", "resid", "state", "map", "status")
    assert isinstance(detect.CfarRelaxResult.n_est, property)
    assert {"cfar_relax.hip", "cfar.hip"} <= set(build.SOURCES) and {"relax_core.h", "cfar_core.h"} <= set(build.HEADERS)
    assert "cfar_relax_kernel" in open(os.path.join(CSRC, "cfar_relax.hip")).read()
    assert {"admmnet_cfar_relax_lds_bytes", "admmnet_cfar_relax_f64"} <= set(detect._lib.SYMBOLS)
    p = inspect.signature(harness.evaluate_snr).parameters
    assert p["cancel"].default is None and p["cfar"].default == ("ca", 1e-4)
    assert list(p)[:12] == ["grid", "layers", "checkpoint", "snrs", "signals", "targets", "cutoff", "baseline", "seed", "device", "head",
                            "cfar"] and list(p)[12:] == ["cancel", "targets_min", "min_sep", "order", "refine", "crb"]
    for grid, r, want in (((8, 8), 2, 9360), ((16, 16), 4, 63120), ((13, 262), 1, 151664)):             # include/admmnet.h
        assert detect.relax_lds_bytes(grid, r) == want
    assert detect.relax_lds_bytes((13, 262), 1) <= detect.LDS_LIMIT


def test_cancel_on_the_command_line(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "evaluate_snr", lambda *a, **kw: seen.append((a, kw)) or iter(()))
    harness.main(["evaluate", "--baseline", "periodogram", "--cancel", "--sweeps", "1", "--newton", "5", "--cfar", "known"])
    harness.main(["evaluate", "--baseline", "periodogram", "--cancel"])
    harness.main(["evaluate", "--baseline", "periodogram"])
    assert [(a[7], kw["cfar"], kw["cancel"]) for a, kw in seen] == [("periodogram", ("known", 1e-4), (5, 1)),
                                                                    ("periodogram", ("ca", 1e-4), (3, 2)),
                                                                    ("periodogram", ("ca", 1e-4), None)]
    with pytest.raises(SystemExit):
        harness.main(["evaluate", "--cancel"])                          # --cancel belongs to --baseline periodogram
    timed = []
    monkeypatch.setattr(harness, "time_cfar_step", lambda *a, **kw: timed.append(kw) or {})
    harness.main(["cfar-step", "--cancel", "--steps", "2"])
    harness.main(["cfar-step"])
    assert [kw.get("cancel") for kw in timed] == [(3, 2), None]
