"""Host: the float64 statement of the CFAR detector (``detect.cfar_host``), the threshold factors, the false-alarm rate on noise,
the kernel's scalar core under sanitizers (tests/host_model/cfar_model.cpp) and the refusals and signatures of the new entry
points.  No GPU.

The mirror is what tests/test_gpu_detect.py holds the kernel to, so it is itself held to things that do not depend on it: the
definition evaluated by a plain double loop, the false-alarm rate it is designed for, and stand-ins with one defect each.
"""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from admm_net_amd import build, detect, harness

import detect_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "admm_net_amd", "csrc")
HOST = os.path.join(HERE, "host_model")


# ---- 1. the map against the definition ------------------------------------------------------------------------------------------------
def test_the_map_is_the_definition_by_a_plain_double_loop():
    c = DC.case("ca_4x6_r3")
    Nb, Nd, r = 4, 6, 3
    x = c.y[0].astype(np.complex128) * np.conj(c.b[0].astype(np.complex128) / np.abs(c.b[0].astype(np.complex128)))
    P = np.zeros((r * Nb, r * Nd))
    for j in range(r * Nb):
        for i in range(r * Nd):
            f, tau = -0.5 + j / (r * Nb), i / (r * Nd)
            s = sum(x[ib * Nd + idd] * np.exp(-2j * np.pi * (ib * f - idd * tau)) for ib in range(Nb) for idd in range(Nd))
            P[j, i] = abs(s) ** 2 / (Nb * Nd)
    got = DC.reference("ca_4x6_r3")[0].map
    worst = float(np.abs(got - P).max() / P.max())
    print("the map against the double loop, relative to the largest cell:", worst)
    assert worst <= 1e-12


# ---- 2. the factors ---------------------------------------------------------------------------------------------------------------------
def test_cfar_alpha():
    for N in (1, 4, 16, 40, 288):
        for pfa in (1e-2, 1e-4, 1e-8):
            assert math.isclose(detect.cfar_alpha("ca", N, pfa), N * (pfa ** (-1.0 / N) - 1.0), rel_tol=1e-13)
            assert detect.cfar_alpha("known", N, pfa) == -math.log(pfa)
            for k in {1, detect.default_rank(N), N}:
                a = detect.cfar_alpha("os", N, pfa, k)
                assert math.isclose(math.prod((N - m) / (N - m + a) for m in range(k)), pfa, rel_tol=1e-12), (N, k, pfa)
            assert detect.cfar_alpha("os", N, pfa) == detect.cfar_alpha("os", N, pfa, -(-3 * N // 4))
    for pfa in (0.3, 1e-3, 1e-6):
        assert math.isclose(detect.cfar_alpha("os", 1, pfa, 1), detect.cfar_alpha("ca", 1, pfa), rel_tol=1e-12)
    assert detect.default_rank(16) == 12 and detect.default_rank(40) == 30 and detect.default_rank(1) == 1
    for bad in (dict(method="go"), dict(pfa=0.0), dict(pfa=1.0), dict(n_train=0), dict(n_train=2.5), dict(method="os", rank=0),
                dict(method="os", rank=17), dict(method="os", rank=1.5)):
        with pytest.raises(ValueError):
            detect.cfar_alpha(**{**dict(method="ca", n_train=16, pfa=1e-2), **bad})


# ---- 3. the false-alarm rate on noise only ------------------------------------------------------------------------------------------------
FAR_SCENES, FAR_PFA = 2000, 1e-2


@pytest.mark.parametrize("method", ["known", "ca", "os"])
def test_false_alarm_rate_on_noise(method):
    """8 x 8, r = 1, guard = train = 1 (N = 16), pfa = 1e-2, 2000 seeded scenes of unit noise: the share of cells over the
    threshold is within 5 binomial standard errors of pfa.  Measured: known 0.009703, ca 0.009680, os 0.009586, that is -1.07,
    -1.15 and -1.49 standard errors."""
    x = DC.noise_scenes(FAR_SCENES, (8, 8), seed=20260105)
    over = sum(detect.cfar_host(x[i], np.ones(64), (8, 8), oversample=1, method=method, pfa=FAR_PFA, guard=1, train=1,
                                noise_var=1.0 if method == "known" else None).n_over for i in range(FAR_SCENES))
    rate, se = over / (FAR_SCENES * 64), math.sqrt(FAR_PFA * (1 - FAR_PFA) / (FAR_SCENES * 64))
    print(f"{method}: rate {rate:.6f}, {(rate - FAR_PFA) / se:+.2f} standard errors")
    assert abs(rate - FAR_PFA) <= 5 * se


# ---- 4. the table -----------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    names = [c.name for c in DC.cases()]
    assert len(set(names)) == len(names) >= 40
    assert {(c.grid, c.kw["oversample"]) for c in DC.cases()} >= {((1, 12), 2), ((12, 1), 2), ((4, 6), 3), ((5, 7), 3), ((8, 8), 1),
                                                                  ((8, 8), 2), ((16, 16), 4), DC.LARGEST}
    assert {(c.kw["method"], c.kw["top"]) for c in DC.cases()} >= {(m, t) for m in detect.METHODS for t in (1, 6, 16)}
    c = DC.case("ca_4x6_r3")
    assert (c.kw["guard"], c.kw["train"]) == (0, 1)
    # the largest shape admitted: the grid's ceiling, and one row more does not fit the LDS at any oversampling above it
    grid, r = DC.LARGEST
    assert grid[0] * grid[1] == detect.MAX_GRID and detect.lds_bytes(grid, r) <= detect.LDS_LIMIT < detect.lds_bytes(grid, r + 1)
    ref = DC.reference
    assert {r.state for c in DC.cases() for r in ref(c.name)} == {detect.DONE, detect.NONFINITE, detect.OUTSIDE}
    margins = {}
    for c in DC.cases():
        for i, r in enumerate(ref(c.name)):
            assert r.state == c.states[i], (c.name, i, r.state)
        margins[c.name] = min(r.margin for r in ref(c.name))
    print("the least decision margin per case:", {k: float(f"{v:.2g}") for k, v in margins.items()})
    left_out = [k for k, v in margins.items() if not v > DC.MARGIN]
    assert len(left_out) == 0, left_out                                         # the cap on cases left out is 0
    nt = 16
    for method in ("ca", "os"):                                                 # cell (0, 0): tau = 0, f = -1/2
        r = ref(f"cell_0_0_{method}")[0]
        assert tuple(r.rows[0, :2]) == (0.0, -0.5) and r.n_det >= 1
    weak = DC.case("masked_pair_ca").truth[0]
    weak = (weak[0][1], weak[1][1])
    has = lambda r, tf: any(tuple(row[:2]) == tf for row in r.rows)  # noqa: E731
    assert not has(ref("masked_pair_ca")[0], weak) and has(ref("masked_pair_os")[0], weak)     # pins the rank
    strong = (DC.case("masked_pair_os").truth[0][0][0], 0.0)
    assert has(ref("masked_pair_ca")[0], strong) and has(ref("masked_pair_os")[0], strong)
    assert ref("more_than_Le")[0].n_det > 1 and all(r.n_det > 6 for r in ref("noise_many_over"))
    assert all(r.n_det == 0 and r.n_over == 0 for r in ref("no_detection") + ref("silence"))
    r = ref("exact_tie")[0]
    a, b = sorted(DC.case("exact_tie").exempt[0])
    assert a < b and math.isclose(r.map.ravel()[a], r.map.ravel()[b], rel_tol=1e-12) and r.n_det >= 2
    assert [int(round((row[1] + 0.5) * nt)) * nt + int(round(row[0] * nt)) for row in r.rows] == [a, b]
    assert DC.case("rank_1").kw["rank"] == 1 and DC.case("rank_N").kw["rank"] == detect.train_count((8, 8), 1, 2) == 40
    assert DC.case("guard_0").kw["guard"] == 0


# ---- 5. the host model under sanitizers -------------------------------------------------------------------------------------------------
def _num(v):
    return repr(float(v))


def test_cfar_core_under_sanitizers(tmp_path):
    """tests/host_model/cfar_model.cpp (its own main, csrc/cfar_core.h with the workgroup emulated, built with
    -fsanitize=address,undefined) on every scene of the case table, held to ``cfar_host`` as the kernel is."""
    exe, inp = str(tmp_path / "cfar_model"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HOST, "cfar_model.cpp"), "-o", exe])
    lines, scenes = [], 0
    for c in DC.cases():
        k = c.kw
        N = detect.train_count(c.grid, k["guard"], k["train"])
        rank = detect.default_rank(N) if k["rank"] is None else k["rank"]
        alpha = detect.cfar_alpha(k["method"], N, k["pfa"], rank if k["method"] == "os" else None)
        for i in range(len(c.y)):
            noise = "none" if c.noise_var is None else _num(c.noise_var[i])
            lines.append(f"{c.grid[0]} {c.grid[1]} {k['oversample']} {k['top']} {detect.METHODS[k['method']]} {k['guard']} {k['train']} "
                         f"{rank} {alpha!r} {int(c.symbols is not None)} {DC.PSK[0]} {DC.PSK[1]!r} {noise}")
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
    for c in DC.cases():
        B, Le = len(c.y), c.kw["top"]
        nf, nt = c.cells
        rows, pmap = np.zeros((B, Le, 3)), np.zeros((B, nf, nt))
        n_det, n_over, state, level = np.zeros(B, int), np.zeros(B, int), np.zeros(B, int), np.zeros(B)
        for i in range(B):
            st, nd, no, lv = next(out).split()
            state[i], n_det[i], n_over[i], level[i] = int(st), int(nd), int(no), float(lv)
            for j in range(Le):
                rows[i, j] = [float(t) for t in next(out).split()]
            pmap[i] = np.array([float(next(out)) for _ in range(nf * nt)]).reshape(nf, nt)
        worst[c.name] = DC.compare(c.name, rows, n_det, n_over, level, state, pmap, "host model")
    print("worst (map / largest cell, level) against the mirror:", {k: (float(f"{a:.2g}"), float(f"{b:.2g}")) for k, (a, b) in worst.items()})
    seen = (max(a for a, _ in worst.values()), max(b for _, b in worst.values()))
    print("the largest:", seen, "recorded:", (DC.MAP_SEEN, DC.LEVEL_SEEN))


# ---- 6. one mistake is rejected ---------------------------------------------------------------------------------------------------------
def _same(name, got, i=0):
    r = DC.reference(name)[i]
    return (got.n_det, got.n_over, got.state) == (r.n_det, r.n_over, r.state) and np.array_equal(got.rows[:, :2], r.rows[:, :2], equal_nan=True)


def test_one_mistake_is_rejected(monkeypatch):
    """Stand-ins -- the mirror with ONE of its parts replaced by a defective one -- are each rejected by a named case: held to the
    table's reference the way the kernel is, they fail."""
    parts = ("periodogram", "window_offsets", "training_cells", "noise_level", "is_over", "beats")
    kept = {k: getattr(detect, k) for k in parts}
    periodogram, offsets, cells, level, beats = (kept[k] for k in ("periodogram", "window_offsets", "training_cells", "noise_level", "beats"))

    def tau_sign(x, grid, r):
        return np.roll(periodogram(x, grid, r)[:, ::-1], 1, axis=1)            # tau_i -> -tau_i

    def exchanged(x, grid, r):                                                  # i = i_d Nb + i_b
        return periodogram(np.asarray(x).reshape(grid[1], grid[0]).T.reshape(-1), grid, r)

    def f_from_zero(x, grid, r):                                                # f_j = j / n_f
        X = np.asarray(x, dtype=np.complex128).reshape(grid)
        S = np.fft.ifft(np.fft.fft(X, n=r * grid[0], axis=0), n=r * grid[1], axis=1) * (r * grid[1])
        return (S.real ** 2 + S.imag ** 2) / (grid[0] * grid[1])

    def map_cells(P, off, r):                                                   # offsets in map cells
        return cells(P, off, 1)

    def no_guard(grid, guard, train):                                           # the guard cells are training cells too
        return offsets(grid, 0, guard + train)

    def no_wrap(P, off, r):                                                     # cells beyond the edge count as empty
        nf, nt = P.shape
        big = np.zeros((3 * nf, 3 * nt))
        big[nf:2 * nf, nt:2 * nt] = P
        return np.stack([big[nf + p * r:2 * nf + p * r, nt + q * r:2 * nt + q * r] for p, q in off])

    def rank_off(c, method, rank):
        return level(c, method, rank - 1 if rank > 1 else 2)

    def larger_index(Pc, c, Pd, d):
        return beats(Pc, -np.asarray(c), Pd, -np.asarray(d))

    stand_ins = {
        "the sign of tau in the atom": ("periodogram", tau_sign, "known_8x8_r2"),
        "i_b and i_d exchanged": ("periodogram", exchanged, "ca_4x6_r3"),
        "the f axis starting at 0": ("periodogram", f_from_zero, "known_8x8_r2"),
        "training offsets in map cells": ("training_cells", map_cells, "ca_8x8_r2"),
        "guard cells not excluded": ("window_offsets", no_guard, "ca_8x8_r2"),
        "no wrap": ("training_cells", no_wrap, "cell_0_0_ca"),
        "rank off by one": ("noise_level", rank_off, "masked_pair_os"),
        "ties to the larger index": ("beats", larger_index, "exact_tie"),
        ">= instead of > at the threshold": ("is_over", lambda P, t: P >= t, "silence"),
    }
    for what, (name, stand_in, case) in stand_ins.items():
        assert _same(case, DC.host(DC.case(case), 0)), case                  # the mirror itself passes ...
        with monkeypatch.context() as mp:
            mp.setattr(detect, name, stand_in)
            rejected = not _same(case, DC.host(DC.case(case), 0))
        print(f"{what}: rejected by {case}")
        assert rejected, what                                                # ... and the stand-in does not
    assert all(getattr(detect, k) is v for k, v in kept.items())


# ---- 7. the margin on the Monte-Carlo law -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targets", [False, True])
def test_the_mirror_holds_the_margin_on_the_monte_carlo_draws(targets):
    """8 x 8, r = 2, 2000 draws, noise only and with 1 .. 3 targets at 15 dB: the share of draws whose decisions all have the
    margin, per method.  Measured: 1.0 for every method, with and without targets (the least margin over all 12 000 mirror runs
    is 2.2e-6)."""
    y, b, noise_var = DC.monte_carlo(targets)
    for method in detect.METHODS:
        margin = DC.mc_host(y, b, noise_var, method)[2]
        share = float((margin > DC.MARGIN).mean())
        print(f"targets={targets} {method}: share with the margin {share}, least margin {margin.min():.2g}")
        assert share >= 1 - DC.MC_LEFT_OUT


# ---- 8. arguments and signatures --------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    c = DC.case("ca_8x8_r2")
    y, b = torch.from_numpy(c.y), torch.from_numpy(c.b)
    bad = (dict(top=0), dict(top=17), dict(top=2.0), dict(top=True), dict(oversample=0), dict(oversample=9), dict(oversample=1.5),
           dict(method="go"), dict(pfa=0.0), dict(pfa=1.0), dict(pfa=-1.0), dict(guard=-1), dict(guard=1.0), dict(train=0),
           dict(guard=1, train=3),                       # 2 * 4 + 1 = 9 > 8
           dict(guard=5, train=4),                       # beyond the reach
           dict(rank=0), dict(method="os", rank=41), dict(method="os", rank=1.5), dict(rank=3),       # rank belongs to os
           dict(noise_var=1.0),                          # ... and noise_var to known
           dict(method="known"), dict(method="known", noise_var="x"), dict(method="known", noise_var=torch.ones(3)),
           dict(method="known", noise_var=torch.ones(2, dtype=torch.complex64)),
           dict(psk=(1, 0.0)), dict(psk=(65, 0.0)), dict(psk=(4, math.inf)), dict(psk=4),
           dict(symbols=torch.zeros(2, 64)), dict(symbols=torch.zeros(2, 63, dtype=torch.int32)),
           dict(out=torch.zeros(2, 6, 3, dtype=torch.float32)), dict(out=torch.zeros(2, 5, 3, dtype=torch.float64)),
           dict(out=torch.zeros(2, 6, 6, dtype=torch.float64)[:, :, ::2]))
    for kw in bad:
        with pytest.raises(ValueError):
            detect.cfar_targets(y, b, (8, 8), **{**dict(top=6, oversample=2), **kw})
    for grid in ((8,), (0, 64), (4, 8), (64, 64)):
        with pytest.raises(ValueError):
            detect.cfar_targets(y, b, grid, top=6, oversample=1, guard=0, train=1)
    with pytest.raises(ValueError):                                    # 25 x 25 at r = 4 does not fit the LDS
        detect.cfar_targets(torch.zeros(1, 625, dtype=torch.complex64), torch.ones(1, 625, dtype=torch.complex64), (25, 25), oversample=4)
    with pytest.raises(ValueError):
        detect.cfar_targets(y.real, b, (8, 8))
    with pytest.raises(TypeError):
        detect.cfar_targets(c.y, c.b, (8, 8))                          # numpy arrays: the device call takes tensors
    with pytest.raises(detect._lib.AdmmNetError):                      # ... on the device: no CPU fallback
        detect.cfar_targets(y, b, (8, 8), top=6, oversample=2)
    for kw in (dict(top=0), dict(method="known"), dict(guard=1, train=3), dict(method="os", rank=41)):
        with pytest.raises(ValueError):
            detect.cfar_host(c.y[0], c.b[0], (8, 8), **kw)
    with pytest.raises(ValueError):
        detect.cfar_host(c.y[0][:5], c.b[0][:5], (8, 8))
    for kw in (dict(baseline="fft"), dict(baseline="periodogram", cfar=("go", 1e-4)), dict(baseline="periodogram", cfar=("ca", 2.0)),
               dict(baseline="periodogram", cfar="ca"), dict(baseline="periodogram", cfar=("known", 1e-4))):   # known: varied scenes
        with pytest.raises(ValueError):
            next(harness.evaluate_snr(**kw))


def test_signatures():
    import admm_net_amd
    assert admm_net_amd.detect is detect and admm_net_amd.cfar_targets is detect.cfar_targets
    assert admm_net_amd.cfar_alpha is detect.cfar_alpha and admm_net_amd.cfar_host is detect.cfar_host
    sig = inspect.signature(detect.cfar_targets)
    assert list(sig.parameters) == ["y", "b", "grid", "top", "oversample", "method", "pfa", "guard", "train", "rank", "noise_var",
                                    "symbols", "psk", "return_map", "out"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [16, 4, "ca", 1e-4, 1, 2, None, None, None,
                                                                            (4, math.pi / 4), False, None]
    assert list(inspect.signature(detect.cfar_alpha).parameters) == ["method", "n_train", "pfa", "rank"]
    host = list(inspect.signature(detect.cfar_host).parameters)
    assert host[:13] == list(sig.parameters)[:13] and host[13:] == ["exempt"]
    assert detect.CfarResult._fields == ("rows", "n_det", "n_over", "level", "state", "map", "status")
    assert (detect.DONE, detect.NONFINITE, detect.OUTSIDE) == (0, 3, 4)
    assert "cfar.hip" in build.SOURCES and "cfar_core.h" in build.HEADERS
    assert "cfar_kernel" in open(os.path.join(CSRC, "cfar.hip")).read()
    p = inspect.signature(harness.evaluate_snr).parameters
    assert p["baseline"].default is None and p["cfar"].default == ("ca", 1e-4)
    for grid, r, want in (((8, 8), 2, 9712), ((16, 16), 4, 70896), ((13, 262), 1, 154176)):
        assert detect.lds_bytes(grid, r) == want


def test_periodogram_on_the_command_line(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "evaluate_snr", lambda *a, **kw: seen.append((a, kw)) or iter(()))
    harness.main(["evaluate", "--baseline", "periodogram", "--cfar", "os", "--pfa", "1e-3", "--order", "6"])
    harness.main(["evaluate", "--baseline", "periodogram"])
    harness.main(["evaluate"])
    assert [(a[7], kw["cfar"]) for a, kw in seen] == [("periodogram", ("os", 1e-3)), ("periodogram", ("ca", 1e-4)), (None, ("ca", 1e-4))]
