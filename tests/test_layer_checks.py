"""CPU: the per-stage checker (tests/layer_checks.py) on the float32 oracle.

(a) The reference passes: the float32 evaluation of oracle/admm_net_ref.py, driven call by call like the device engine
    (front / back / finish over a state of float32 buffers), passes every check at every case tests/test_gpu_layer_state.py
    runs -- the natural cases, the head cases and the seeded states.
(b) Mutants fail: the same float32 oracle with one stage altered -- the mistakes a kernel could make and the whole-forward
    tolerance would not see -- is rejected by the check of that stage.  This is the evidence that the bounds are tight
    enough to matter.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import layer_checks as LC
from oracle import admm_net_ref as R


# ------------------------------------------------------------------------------------------- the float32 oracle as an engine
def h_layer_variant(sd, k, G, Z, sigma, M, N, tr_abs=False, clamp=True, scale_first=False):
    """oracle h_layer with the switches of the mutants; all off it is R.h_layer to the bit (asserted below)."""
    D = M * N
    p = f"hLayers.{k}."
    rho = F.softplus(sd[p + "rho"])
    T = G[:, :D, :D] + Z[:, :D, :D] / (rho + R.EPS)
    t = torch.diagonal(T, dim1=1, dim2=2).real
    sigma = sigma.to(t.dtype)
    A = 2 * torch.sqrt(torch.tensor(float(M * N), dtype=torch.float32)).to(t.dtype) * sigma + sigma ** 2
    A = A.reshape(-1, 1)
    hid = F.relu(F.linear(t, sd[p + "correction_net.0.weight"], sd[p + "correction_net.0.bias"]))
    corr = torch.tanh(F.linear(hid, sd[p + "correction_net.2.weight"], sd[p + "correction_net.2.bias"]))
    tc = t + 0.1 * corr
    linf = torch.max(torch.abs(tc), dim=1, keepdim=True)[0]
    tr = torch.sum(tc.abs() if tr_abs else tc, dim=1, keepdim=True)
    scale = torch.sigmoid(sd[p + "projection_weight"]) / (A * linf + tr + R.EPS)
    if clamp:
        scale = torch.clamp(scale, max=1.0)
    return t * scale + 0.1 * corr if scale_first else tc * scale


def z_step_variant(sd, k, rn, mean, knorm_layer=None):
    """oracle z_step of layer k with S_KNORM of another layer."""
    kk = k if knorm_layer is None else knorm_layer
    p = f"zLayers.{k}."
    rho = F.softplus(sd[p + "rho"])
    B = rn.shape[0]
    feat = torch.stack([torch.tensor(kk / 10.0, dtype=torch.float32).to(rn.dtype).repeat(B),
                        torch.full((B,), float(rho), dtype=rn.dtype), rn / (mean + R.EPS)], dim=1)
    hid = F.relu(F.linear(feat, sd[p + "residual_scale_net.0.weight"], sd[p + "residual_scale_net.0.bias"]))
    sf = torch.sigmoid(F.linear(hid, sd[p + "residual_scale_net.2.weight"], sd[p + "residual_scale_net.2.bias"]))
    return rho * (0.5 + 1.5 * sf).squeeze(1)


def peak_head_variant(sd, phi, M, N, L, hidden=128, heads=4, drop=None, offset_shift=0):
    """oracle peak_head; ``drop = (head, token)`` leaves that token out of that head's softmax, ``offset_shift`` moves the
    regressor offset t / L to (t + shift) / L.  Without either it is R.peak_head to the bit (asserted below)."""
    p = "peakSearchLayer."
    B = phi.shape[0]
    feat = torch.cat([phi.real, phi.imag], dim=1)
    x = F.relu(F.linear(feat, sd[p + "feature_extractor.0.weight"], sd[p + "feature_extractor.0.bias"]))
    x = F.relu(F.linear(x, sd[p + "feature_extractor.2.weight"], sd[p + "feature_extractor.2.bias"]))
    pos = F.linear(sd[p + "position_encoder"], sd[p + "position_projection.weight"], sd[p + "position_projection.bias"])
    Wi, bi = sd[p + "attention.in_proj_weight"], sd[p + "attention.in_proj_bias"]
    q = F.linear(x, Wi[:hidden], bi[:hidden])
    kk = F.linear(pos, Wi[hidden:2 * hidden], bi[hidden:2 * hidden])
    vv = F.linear(pos, Wi[2 * hidden:], bi[2 * hidden:])
    hd = hidden // heads
    sc = torch.einsum("bhd,thd->bht", q.reshape(B, heads, hd), kk.reshape(-1, heads, hd)) / math.sqrt(hd)
    if drop is not None:
        sc = sc.clone()
        sc[:, drop[0], drop[1]] = -math.inf
    at = torch.softmax(sc, dim=-1)
    ctx = torch.einsum("bht,thd->bhd", at, vv.reshape(-1, heads, hd)).reshape(B, hidden)
    xp = x + F.linear(ctx, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"])
    for i in (0, 2, 4):
        xp = F.relu(F.linear(xp, sd[p + f"peak_extractor.{i}.weight"], sd[p + f"peak_extractor.{i}.bias"]))
    taus, fs, cs = [], [], []
    for t in range(L):
        tf = xp + torch.tensor((t + offset_shift) / L, dtype=torch.float32).to(xp.dtype)
        a = F.relu(F.linear(tf, sd[p + f"tau_regressor.{t}.0.weight"], sd[p + f"tau_regressor.{t}.0.bias"]))
        taus.append(torch.sigmoid(F.linear(a, sd[p + f"tau_regressor.{t}.2.weight"], sd[p + f"tau_regressor.{t}.2.bias"])))
        a = F.relu(F.linear(tf, sd[p + f"f_regressor.{t}.0.weight"], sd[p + f"f_regressor.{t}.0.bias"]))
        fs.append(torch.tanh(F.linear(a, sd[p + f"f_regressor.{t}.2.weight"], sd[p + f"f_regressor.{t}.2.bias"])))
        a = F.relu(F.linear(tf, sd[p + "confidence_net.0.weight"], sd[p + "confidence_net.0.bias"]))
        cs.append(torch.sigmoid(F.linear(a, sd[p + "confidence_net.2.weight"], sd[p + "confidence_net.2.bias"])))
    return torch.cat(taus, 1), torch.cat(fs, 1), torch.cat(cs, 1)


class OracleEngine:
    """The float32 oracle stepped like sharded.HipLayerEngine over a state of float32 buffers (full storage).  ``mut``: the
    altered stage, one of the names test_mutant_is_rejected lists."""

    def __init__(self, sd, y, b, sigma, M, N, K, L=3, mut=None):
        self.sd = R.cast_weights(sd, "f32")
        self.y, self.b, self.sigma = y.to(torch.complex64), b.to(torch.complex64), sigma.float().reshape(-1)
        self.M, self.N, self.K, self.L, self.mut = M, N, K, L, mut
        B, D = self.y.shape
        n = D + 1
        c = lambda *s: torch.zeros(*s, dtype=torch.complex64)
        r = lambda *s: torch.zeros(*s, dtype=torch.float32)
        self.state = LC.snapshot_cpu(c(B, n, n), c(B, n, n), c(B, D), c(B, D), r(B, D), r(B, D), r(B), r(B))

    def snap(self):
        return {key: v.clone() for key, v in self.state.items()}

    def corner_z(self, k):
        return LC.corner(self.sd, f"zLayers.{k}.lambda_param", "f32")

    def front(self, k):
        s, sd, mut = self.state, self.sd, self.mut
        cur, prv = k & 1, (k & 1) ^ 1
        G, Z = s["G"], (torch.zeros_like(s["Z"]) if k <= 1 else s["Z"])
        Zn = Z
        if k >= 1:
            cz = self.corner_z(k if mut == "corner_z_of_layer_k" else k - 1)
            Zn = Z + s["alpha"].reshape(-1, 1, 1) * (G - R.block_matrix(s[f"phi{prv}"], s[f"h{prv}"], cz))
        Zphi = Z if mut == "zeta_before_update" else Zn.conj() if mut == "zeta_conjugated" else Zn
        s[f"phi{cur}"] = R.phi_layer(sd, k, self.y, self.b, G, Zphi)
        if k == self.K - 1:
            return None
        hv = dict(tr_over_abs=dict(tr_abs=True), clamp_dropped=dict(clamp=False), scaled_before_correction=dict(scale_first=True))
        s[f"h{cur}"] = h_layer_variant(sd, k, G, Zn, self.sigma, self.M, self.N, **hv.get(mut, {}))
        if k >= 1:
            s["Z"] = Zn
        s["G"] = R.g_layer(sd, k, s[f"phi{cur}"], s[f"h{cur}"], Zn)
        s["rn"] = torch.linalg.norm(s["G"] - R.block_matrix(s[f"phi{cur}"], s[f"h{cur}"], self.corner_z(k)), dim=(1, 2))
        rn = s["rn"][:-1] if mut == "mean_without_last" else s["rn"]
        self.pair = torch.tensor([float(rn.double().sum()), float(rn.numel())], dtype=torch.float64)
        return torch.tensor([float(s["rn"].double().sum()), float(s["rn"].numel())], dtype=torch.float64)

    def back(self, k, mean):
        mean = float(torch.tensor(float(mean), dtype=torch.float64).float())
        if self.mut == "mean_without_last":
            mean = float(torch.tensor(LC.mean_of_pair(self.pair)).float())
        self.state["alpha"] = z_step_variant(self.sd, k, self.state["rn"], mean,
                                             knorm_layer=k + 1 if self.mut == "knorm_of_next_layer" else None)

    def finish(self):
        phi = self.state[f"phi{(self.K - 1) & 1}"]
        kw = dict(drop_token=dict(drop=(1, phi.shape[1] - 1)), offset_plus_one=dict(offset_shift=1)).get(self.mut, {})
        return torch.stack(peak_head_variant(self.sd, phi, self.M, self.N, self.L, **kw))


def drive(eng, sd, seed=None, g_finite_only=False, seed_after=0):
    """begin / front / back / finish with every check of layer_checks; -> the worst ratio per stage.  ``seed(state, ctx)`` runs
    after back(seed_after); ``g_finite_only``: of the G and rn of the layer behind the seed only finiteness."""
    M, N, K = eng.M, eng.N, eng.K
    res = {}
    for k in range(K):
        before = eng.snap()
        pair = eng.front(k)
        after = eng.snap()
        out = LC.check_front(sd, M, N, K, k, before, after, eng.y, eng.b, eng.sigma, False,
                             eng.corner_z(k - 1) if k else None, pair=pair, g_finite_only=g_finite_only and k == seed_after + 1)
        res[f"scale{k}"] = out.get("scale")
        LC.worst(res, out)
        if k == K - 1:
            break
        before = after
        mean = LC.mean_of_pair(pair)
        eng.back(k, mean)
        LC.worst(res, LC.check_back(sd, k, before, eng.snap(), mean))
        if k == seed_after and seed is not None:
            res["seeded"] = seed(eng.state, dict(sd=sd, sigma=eng.sigma, M=M, N=N, corner_zp=eng.corner_z(0)))
    return res


def strip(res):
    return {key: v for key, v in res.items() if not key.startswith("scale") and key != "seeded"}


def oracle_failed(res):
    """The stages the float32 oracle misses, rn left out.  rn = ||G - C||_F is held to the project's own bound for its kernels
    (1e-5 relative), which float32 LAPACK does not keep: the float32 oracle's rn lies 1.8e-5 (D = 128) to 4e-5 (D = 256, layer 0)
    from float64.  Its figure is printed, not asserted; the bound stays and the device meets it (tests/test_gpu_layer_state.py).
    Every other check, G included, holds for the float32 oracle."""
    return {key: v for key, v in LC.failed(strip(res)).items() if key != "rn"}


@functools.lru_cache(maxsize=None)
def inputs(Nb, Nd, p):
    return LC.case_inputs(Nb, Nd, p)


CASE_IDS = [f"D{a * b}_{a}x{b}_p{p}" for a, b, p in LC.CASES]


# ----------------------------------------------------------------------------------------------------- (a) the reference passes
def test_variants_without_a_switch_are_the_oracle():
    sd, y, b, s = inputs(2, 4, 0.3)
    sd32 = R.cast_weights(LC.case_inputs(2, 4, 0.3, head=True)[0], "f32")
    G, Z = torch.randn(6, 9, 9, dtype=torch.complex64), torch.randn(6, 9, 9, dtype=torch.complex64)
    assert LC.same_bits(h_layer_variant(sd32, 1, G, Z, s, 2, 4), R.h_layer(sd32, 1, G, Z, s, 2, 4))
    rn = torch.rand(6)
    assert LC.same_bits(z_step_variant(sd32, 1, rn, float(rn.mean())), R.z_step(sd32, 1, rn, mean_norm=float(rn.mean())))
    for a, c in zip(peak_head_variant(sd32, y, 2, 4, 3), R.peak_head(sd32, y, 2, 4, 3)):
        assert LC.same_bits(a, c)


@pytest.mark.parametrize("Nb,Nd,p", LC.CASES, ids=CASE_IDS)
def test_float32_oracle_passes_every_stage(Nb, Nd, p):
    sd, y, b, s = inputs(Nb, Nd, p)
    res = drive(OracleEngine(sd, y, b, s, Nb, Nd, LC.K_CASE), sd)
    print("LAYERCHECK f32-oracle", f"D={Nb * Nd} p={p}", {k: f"{v:.3g}" for k, v in strip(res).items()})
    assert not oracle_failed(res), res
    for k in range(1, LC.K_CASE - 1):   # the natural run never clamps at k >= 1
        assert bool((res[f"scale{k}"] < 0.95).all()), res[f"scale{k}"]


@pytest.mark.parametrize("Nb,Nd,p", LC.K4_CASES, ids=[f"D{a * b}" for a, b, _ in LC.K4_CASES])
def test_float32_oracle_passes_with_a_stored_z(Nb, Nd, p):
    sd, y, b, s = LC.case_inputs(Nb, Nd, p, K=4)
    res = drive(OracleEngine(sd, y, b, s, Nb, Nd, 4), sd)
    print("LAYERCHECK f32-oracle K=4", f"D={Nb * Nd} p={p}", {k: f"{v:.3g}" for k, v in strip(res).items()})
    assert not oracle_failed(res), res


def test_float32_oracle_keeps_a_stored_z_where_alpha_is_zero():
    """K = 4 with alpha seeded after back(1): front(2) updates a stored, non-zero Z, and where alpha = 0 it keeps its bits."""
    Nb, Nd, p = LC.K4_CASES[0]
    sd, y, b, s = LC.case_inputs(Nb, Nd, p, K=4)
    eng = OracleEngine(sd, y, b, s, Nb, Nd, 4)
    res = drive(eng, sd, seed=LC.seed_alpha, g_finite_only=True, seed_after=1)
    assert not oracle_failed(res), res
    zero = [i for i, a in enumerate(LC.ALPHA_SEED) if a == 0]
    assert zero and bool((eng.state["Z"][zero].abs().amax(dim=(1, 2)) > 0).all())   # the kept Z is not the trivial zero


# -------------------------------------------------------------------------------------------------- NaN never passes
def test_nan_is_rejected_everywhere():
    """A NaN in a stage's output or inputs fails the stage: in ratio(), through worst() and failed(), and in the drive."""
    nan = float("nan")
    assert LC.worst({}, {"phi": nan})["phi"] != LC.worst({}, {"phi": nan})["phi"]
    assert set(LC.failed(LC.worst({"phi": 0.3, "h": 0.2}, {"phi": nan, "h": 0.1}))) == {"phi"}
    assert set(LC.failed(LC.worst(LC.worst({}, {"phi": nan}), {"phi": 0.5}))) == {"phi"}       # and a later call does not clear it
    assert not LC.passes(nan) and LC.passes(1.0) and not LC.passes(1.0000001)
    one = torch.ones(3)
    assert LC.ratio(torch.tensor([0.0, nan, 0.0]), one) == math.inf and LC.ratio(one * 0.5, torch.tensor([1.0, nan, 1.0])) == math.inf
    assert LC.ratio(torch.tensor([0.0, math.inf, 0.0]), one) == math.inf and LC.ratio(one * 0.5, one) == 0.5
    Nb, Nd, p = 2, 4, 0.3
    sd, y, b, s = inputs(Nb, Nd, p)

    class Poisoned(OracleEngine):      # one NaN element in the phi of layer ``at``
        at = 0

        def front(self, k):
            pair = super().front(k)
            if k == self.at:
                self.state[f"phi{k & 1}"][1, 3] = complex(nan, 0.0)
            return pair

    e = Poisoned(sd, y, b, s, Nb, Nd, LC.K_CASE)
    e.at = LC.K_CASE - 1               # the last layer: nothing downstream reads it
    res = strip(drive(e, sd))
    assert set(LC.failed(res)) == {"phi"}, res
    ratios, _ = LC.check_head(LC.case_inputs(Nb, Nd, 0.5, K=LC.K_HEAD, head=True)[0],
                              torch.full((3, LC.B_CASE, 3), 0.5).index_put((torch.tensor(1), torch.tensor(2), torch.tensor(0)),
                                                                           torch.tensor(nan)), y, Nb, Nd, 3)
    assert not LC.passes(ratios["f"]) and not all(LC.passes(v) for v in ratios.values())


@pytest.mark.parametrize("Nb,Nd", LC.HEAD_GEOMS, ids=[f"D{a * b}" for a, b in LC.HEAD_GEOMS])
@pytest.mark.parametrize("L", LC.HEAD_LS)
def test_float32_oracle_head_passes(Nb, Nd, L):
    sd, y, b, s = LC.case_inputs(Nb, Nd, 0.5, K=LC.K_HEAD, head=True, L=L)
    eng = OracleEngine(sd, y, b, s, Nb, Nd, LC.K_HEAD, L=L)
    drive(eng, sd)
    ratios, yards = LC.check_head(sd, eng.finish(), eng.state[f"phi{(LC.K_HEAD - 1) & 1}"], Nb, Nd, L)
    print("LAYERCHECK f32-oracle head", f"D={Nb * Nd} L={L}", ratios, yards)
    assert all(LC.passes(v) for v in ratios.values()), ratios


@pytest.mark.parametrize("Nb,Nd,p", LC.SEED_CASES, ids=[f"D{a * b}" for a, b, _ in LC.SEED_CASES])
def test_float32_oracle_passes_on_seeded_states(Nb, Nd, p):
    """The seeds reach what the natural inputs do not: the clamp (scale > 1.05 for every signal), a negative cval (a negative,
    unclamped scale) and alpha = 0; the conditioning of the projection holds on each (check_h asserts it)."""
    sd, y, b, s = inputs(Nb, Nd, p)
    for name, seed in (("clamp", LC.seed_clamp), ("neg", LC.seed_negative_cval), ("alpha", LC.seed_alpha)):
        res = drive(OracleEngine(sd, y, b, s, Nb, Nd, LC.K_CASE), sd, seed=seed, g_finite_only=True)
        sc = res["scale1"]
        if name == "clamp":
            assert bool((sc > 1.05).all()), sc
        if name == "neg":
            assert int(res["seeded"].sum()) >= LC.B_CASE - 1 and bool((sc[res["seeded"]] < 0).all()), (res["seeded"], sc)
        print("LAYERCHECK f32-oracle seeded", name, f"D={Nb * Nd}", sc.tolist(), {k: f"{v:.3g}" for k, v in strip(res).items()})
        assert not oracle_failed(res), (name, res)


def test_float32_oracle_alpha_on_seeded_rn():
    sd, y, b, s = inputs(*LC.SEED_CASES[0])
    rn = torch.tensor(LC.RN_SEED, dtype=torch.float32)
    for k in range(LC.K_CASE - 1):
        for mean in LC.MEAN_SEED:
            own = R.z_step(R.cast_weights(sd, "f32"), k, rn, mean_norm=mean)
            r, yard = LC.check_alpha(sd, k, own, rn, mean)
            assert r <= 1.0, (k, mean, r, yard)


# --------------------------------------------------------------------------------------------------------- (b) mutants fail
#   mutant -> (case, the check that must reject it, seed)
MUTANTS = {
    "corner_z_of_layer_k": ((10, 10, 1.0), "Z", None),
    "zeta_before_update": ((10, 10, 1.0), "phi", None),
    "zeta_conjugated": ((10, 10, 1.0), "phi", None),
    "tr_over_abs": ((10, 10, 1.0), "h", None),
    "clamp_dropped": ((10, 10, 1.0), "h", LC.seed_clamp),
    "scaled_before_correction": ((10, 10, 1.0), "h", None),
    "knorm_of_next_layer": ((10, 10, 1.0), "alpha", None),
    "mean_without_last": ((10, 10, 1.0), "alpha", None),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    (Nb, Nd, p), stage, seed = MUTANTS[mut]
    sd, y, b, s = inputs(Nb, Nd, p)
    res = strip(drive(OracleEngine(sd, y, b, s, Nb, Nd, LC.K_CASE, mut=mut), sd, seed=seed, g_finite_only=seed is not None))
    print("LAYERCHECK mutant", mut, {k: f"{v:.3g}" for k, v in res.items()})
    assert res[stage] > 1.0, (mut, res)
    assert set(oracle_failed(res)) == {stage}, (mut, res)   # and only that stage: every other is referred to its own inputs


@pytest.mark.parametrize("mut", ["drop_token", "offset_plus_one"])
def test_head_mutant_is_rejected(mut):
    Nb, Nd, L = 10, 10, 3          # D = 100: not a multiple of the softmax's 64-lane stride; the dropped token is the last
    sd, y, b, s = LC.case_inputs(Nb, Nd, 0.5, K=LC.K_HEAD, head=True, L=L)
    eng = OracleEngine(sd, y, b, s, Nb, Nd, LC.K_HEAD, L=L, mut=mut)
    drive(eng, sd)
    ratios, _ = LC.check_head(sd, eng.finish(), eng.state[f"phi{(LC.K_HEAD - 1) & 1}"], Nb, Nd, L)
    print("LAYERCHECK mutant", mut, ratios)
    assert not all(LC.passes(v) for v in ratios.values()), ratios
