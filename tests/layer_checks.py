"""Per-stage checks of the inference forward against the float64 oracle (tests/test_layer_checks.py on the CPU,
tests/test_gpu_layer_state.py on the device).  Plain torch, no GPU.

Every function takes what a stage produced and the float32-valued inputs that stage actually read, evaluates the oracle's
stage function (oracle/admm_net_ref.py) in float64 on those inputs and returns the worst error / bound ratio: a stage passes
at <= 1.  Because each stage is referred to its own inputs, errors do not compound across layers.

State snapshots are dicts of CPU tensors with the keys of ``KEYS``: ``G``, ``Z`` complex64 [B, n, n], ``phi0``, ``phi1``
complex64 [B, D], ``h0``, ``h1`` float32 [B, D], ``alpha``, ``rn`` float32 [B]; layer k owns ``phi{k & 1}`` / ``h{k & 1}``.
``lower_only``: G and Z hold the lower triangle (row >= column) only.

Bounds, with u = 2^-24 (names as in csrc/prep.hip):
  * Z update  Z_new = Z + alpha (G_prev - C_prev), C_prev from layer k-1's phi, h and corner_z: per element
    |err| <= 4 u (|Z| + |alpha| (|G_prev| + |C_prev|))  (three roundings: difference, product, sum); with alpha_b = 0 the
    stored Z_b keeps its bits.  The Z a layer reads is zero at k <= 1 whatever the buffer holds (PM_FIRST, PM_ZZERO).
  * phi, per real and imaginary part:
    |err| <= 12 u wgt (|y / (b + eps)| + rho |g| + |Z_Di| + |alpha| (|G_Di| + |phi_prev,i|)).  The 12 counts the roundings:
    hypotf, the square, + eps, rho b^2, 1 +, and the quotient in wgt; the Smith division; three in the on-the-fly zeta; rho g;
    two sums; the final product.  zeta is always formed from the Z before the update, as the kernel does (at the last layer it
    never stores Z).
  * h, alpha, head: MLPs whose summation order differs from torch's, so the bound is measured: 3 x yardstick + 4 u, the
    yardstick being the float32 oracle's own distance from float64 for that stage on the same inputs, largest over the
    signals of the case (h: max|dh| / max|h| per signal; alpha: relative; head: absolute, per output kind).  3 x is the
    margin DESIGN.md section 2 gives the reference arithmetic; 4 u keeps a lucky yardstick from setting a bound below one
    rounding of the result.
  * G: max|G - G_ref| <= 2e-5 max|G_ref| over the stored triangle, rn within 1e-5 relative; full storage: G == G^H exactly.
  * (sum, count): count == B, sum within 1e-13 relative of the float64 sum of the rn it was formed from.

Input conditions, asserted on the float64 oracle so that no case passes by sitting on an ill-conditioned point:
  * projection: |cval| >= 0.05 (A linf + sum|tc|);
  * head: tau and confidence in (0.05, 0.95), |f| < 0.9.
"""
import math

import torch
import torch.nn.functional as F

from oracle import admm_net_ref as R

U = 2.0 ** -24
KEYS = ("G", "Z", "phi0", "phi1", "h0", "h1", "alpha", "rn")
TOL_G, TOL_RN, TOL_SUM = 2e-5, 1e-5, 1e-13
COND_PROJ, HEAD_LO, HEAD_HI, HEAD_F = 0.05, 0.05, 0.95, 0.9


# ------------------------------------------------------------------------------------------------------------- helpers
def bits(t):
    """int32 image of a real or complex float32 tensor: equality of bits, NaN and the sign of zero included."""
    t = t.detach().cpu().contiguous()
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def tril_mask(n):
    return torch.tril(torch.ones(n, n, dtype=torch.bool))


def herm_from_lower(X):
    """The Hermitian matrix whose lower triangle (diagonal included, as stored) is X's: what a kernel that reads row >= column
    only sees."""
    return torch.tril(X) + torch.tril(X, -1).transpose(1, 2).conj()


def corner(sd, key, dtype="f64"):
    """1 / (softplus(lambda)^2 + eps) of ``sd[key]`` in the arithmetic of ``dtype``, as a Python float
    (admm_net.py:271 / :426: float32 in the reference, and in the packed weights)."""
    rt, _ = R._dt(dtype)
    lam = F.softplus(sd[key].detach().to(rt))
    return float(1.0 / (lam ** 2 + R.EPS))


def ratio(err, bound):
    """max err / bound; an error where the bound is zero, and a NaN or infinite error or bound, count as infinite."""
    err, bound = err.double(), bound.double()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    r = torch.where(torch.isfinite(err) & torch.isfinite(bound), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def passes(v):
    """A ratio passes at <= 1; NaN does not."""
    return bool(v <= 1.0)


def snapshot_cpu(G, Z, phi0, phi1, h0, h1, alpha, rn):
    return dict(G=G, Z=Z, phi0=phi0, phi1=phi1, h0=h0, h1=h1, alpha=alpha, rn=rn)


def assert_unchanged(before, after, keys, what):
    for key in keys:
        assert same_bits(before[key], after[key]), f"{what}: {key} changed"


# ---------------------------------------------------------------------------------------------------- the inputs of a layer
class Prev:
    """What layer k >= 1 reads of the state layer k-1 left: the Z before the update (zero at k == 1), alpha, G, phi, h and the
    float32 corner_z of layer k-1.  ``as_(dtype)`` gives them in float32 or float64."""

    def __init__(self, k, before, corner_z):
        p = (k - 1) & 1
        self.k = k
        self.Z = torch.zeros_like(before["G"]) if k == 1 else before["Z"]
        self.G, self.alpha = before["G"], before["alpha"]
        self.phi, self.h = before[f"phi{p}"], before[f"h{p}"]
        self.corner_z = float(corner_z)

    def as_(self, dtype):
        rt, ct = R._dt(dtype)
        return self.Z.to(ct), self.alpha.to(rt), self.G.to(ct), self.phi.to(ct), self.h.to(rt)

    def z_update(self, dtype, hermitian):
        """Z + alpha (G - C_prev) in ``dtype``; ``hermitian``: on the Hermitian completion of the lower triangles (what phi, h
        and G of the layer read), else on the stored elements as they are."""
        Z, al, G, phi, h = self.as_(dtype)
        if hermitian:
            Z, G = herm_from_lower(Z), herm_from_lower(G)
        C = R.block_matrix(phi, h, self.corner_z)
        return Z + al.reshape(-1, 1, 1) * (G - C), (Z, al, G, C)


def layer_inputs(prev, B, D, dtype):
    """(G, Z) as phi_layer / h_layer of the oracle take them: zeros at layer 0, else G_prev and the updated Z."""
    _, ct = R._dt(dtype)
    if prev is None:
        z = torch.zeros(B, D + 1, D + 1, dtype=ct)
        return z, z.clone()
    Zn, (_, _, G, _) = prev.z_update(dtype, hermitian=True)
    return G, Zn


# ------------------------------------------------------------------------------------------------------------------ stages
def check_z(Z_out, prev, lower_only):
    """The stored Z after the update against the float64 expression on the stored float32 operands; exact where alpha = 0."""
    ref, (Z, al, G, C) = prev.z_update("f64", hermitian=False)
    bound = 4 * U * (Z.abs() + al.abs().reshape(-1, 1, 1) * (G.abs() + C.abs()))
    n = Z_out.shape[-1]
    mask = tril_mask(n) if lower_only else torch.ones(n, n, dtype=torch.bool)
    err = (Z_out.to(torch.complex128) - ref).abs()
    for i in torch.nonzero(prev.alpha == 0).flatten().tolist():
        assert torch.equal(bits(Z_out[i])[mask], bits(prev.Z[i])[mask]), f"alpha = 0 but Z of signal {i} changed"
    return ratio(err[:, mask], bound[:, mask])


def check_phi(sd, k, phi_out, y, b, prev):
    sd64 = R.cast_weights(sd, "f64")
    B, D = phi_out.shape
    y, b = y.to(torch.complex128), b.to(torch.complex128)
    G, Zn = layer_inputs(prev, B, D, "f64")
    ref = R.phi_layer(sd64, k, y, b, G, Zn)
    rho = F.softplus(sd64[f"phiLayers.{k}.rho"])
    b_sq = b.abs() ** 2 + R.EPS
    wgt = b_sq / (1 + rho * b_sq)
    terms = (y / (b + R.EPS)).abs()
    if prev is not None:
        Z, al, Gp, phip, _ = prev.as_("f64")
        terms = terms + rho * Gp[:, D, :D].abs() + Z[:, D, :D].abs() + al.abs().reshape(-1, 1) * (Gp[:, D, :D].abs() + phip.abs())
    bound = 12 * U * wgt * terms
    d = phi_out.to(torch.complex128) - ref
    return max(ratio(d.real.abs(), bound), ratio(d.imag.abs(), bound))


def projection_parts(sd, k, G, Z, sigma, M, N, with_t=False):
    """cval, A linf + sum|tc| and the unclamped scale of HLayer's projection (oracle h_layer, admm_net.py:176-190), [B] each,
    in the dtype of G."""
    D = M * N
    p = f"hLayers.{k}."
    rho = F.softplus(sd[p + "rho"])
    t = torch.diagonal(G[:, :D, :D] + Z[:, :D, :D] / (rho + R.EPS), dim1=1, dim2=2).real
    sigma = sigma.to(t.dtype).reshape(-1)
    A = 2 * torch.sqrt(torch.tensor(float(D), dtype=torch.float32)).to(t.dtype) * sigma + sigma ** 2
    hid = F.relu(F.linear(t, sd[p + "correction_net.0.weight"], sd[p + "correction_net.0.bias"]))
    tc = t + 0.1 * torch.tanh(F.linear(hid, sd[p + "correction_net.2.weight"], sd[p + "correction_net.2.bias"]))
    linf = tc.abs().max(dim=1).values
    cval = A * linf + tc.sum(dim=1)
    parts = (cval, A * linf + tc.abs().sum(dim=1), torch.sigmoid(sd[p + "projection_weight"]) / (cval + R.EPS))
    return parts + (t, tc) if with_t else parts


def measured_bound(yardstick):
    return 3.0 * yardstick + 4 * U


def check_h(sd, k, h_out, sigma, M, N, prev):
    """-> (ratio, yardstick, unclamped scale [B] of the float64 oracle).  Asserts the conditioning of the projection."""
    B, D = h_out.shape
    sd64, sd32 = R.cast_weights(sd, "f64"), R.cast_weights(sd, "f32")
    G, Zn = layer_inputs(prev, B, D, "f64")
    ref = R.h_layer(sd64, k, G, Zn, sigma.double(), M, N)
    cval, mass, scale = projection_parts(sd64, k, G, Zn, sigma.double(), M, N)
    assert bool((cval.abs() >= COND_PROJ * mass).all()), f"layer {k}: ill-conditioned projection, |cval| / mass = {(cval.abs() / mass).tolist()}"
    G32, Zn32 = layer_inputs(prev, B, D, "f32")
    own = R.h_layer(sd32, k, G32, Zn32, sigma.float(), M, N)
    scale_h = ref.abs().max(dim=1).values
    yard = float(((own.double() - ref).abs().max(dim=1).values / scale_h).max())
    err = (h_out.double() - ref).abs().max(dim=1).values / scale_h
    return float(err.max()) / measured_bound(yard), yard, scale


def mean_of_pair(pair):
    return float(pair[0].double() / pair[1].double())


def check_alpha(sd, k, alpha_out, rn, mean):
    """alpha of layer k from rn and the batch mean (a float: sum / count of the pair in float64, or the float32 mean handed to
    back()).  The float32 oracle takes the mean rounded to float32, as the kernel does.  -> (ratio, yardstick)."""
    sd64, sd32 = R.cast_weights(sd, "f64"), R.cast_weights(sd, "f32")
    ref = R.z_step(sd64, k, rn.double(), mean_norm=float(mean))
    own = R.z_step(sd32, k, rn.float(), mean_norm=float(torch.tensor(float(mean), dtype=torch.float64).float()))
    assert bool(torch.isfinite(ref).all()) and bool((ref != 0).all())
    yard = float(((own.double() - ref).abs() / ref.abs()).max())
    err = float(((alpha_out.double() - ref).abs() / ref.abs()).max())
    return err / measured_bound(yard), yard


def check_head(sd, head_out, phi, M, N, L):
    """head_out float32 [3, B, L] (tau, f, confidence) from phi -> ({kind: ratio}, {kind: yardstick}).  Asserts the head's
    conditioning."""
    sd64, sd32 = R.cast_weights(sd, "f64"), R.cast_weights(sd, "f32")
    ref = R.peak_head(sd64, phi.to(torch.complex128), M, N, L)
    own = R.peak_head(sd32, phi.to(torch.complex64), M, N, L)
    tau, f, conf = ref
    assert bool(((tau > HEAD_LO) & (tau < HEAD_HI)).all()) and bool(((conf > HEAD_LO) & (conf < HEAD_HI)).all()) and \
        bool((f.abs() < HEAD_F).all()), "head outputs of the oracle leave the well-conditioned range"
    ratios, yards = {}, {}
    for i, kind in enumerate(("tau", "f", "conf")):
        yards[kind] = float((own[i].double() - ref[i]).abs().max())
        ratios[kind] = float((head_out[i].double() - ref[i]).abs().max()) / measured_bound(yards[kind])
    return ratios, yards


def check_g(sd, k, G_out, rn_out, phi, h, Z, lower_only):
    """G and rn of layer k from phi, h and the Z the layer used (None: zero, layers 0).  -> (ratio G, ratio rn)."""
    sd64 = R.cast_weights(sd, "f64")
    n = G_out.shape[-1]
    Zh = torch.zeros(G_out.shape, dtype=torch.complex128) if Z is None else herm_from_lower(Z.to(torch.complex128))
    phi, h = phi.to(torch.complex128), h.double()
    ref = R.g_layer(sd64, k, phi, h, Zh)
    rn_ref = torch.linalg.norm(ref - R.block_matrix(phi, h, corner(sd, f"zLayers.{k}.lambda_param")), dim=(1, 2))
    if lower_only:
        mask = tril_mask(n)
    else:
        mask = torch.ones(n, n, dtype=torch.bool)
        assert torch.equal(G_out, G_out.transpose(1, 2).conj()), f"layer {k}: full-storage G is not exactly Hermitian"
    err = (G_out.to(torch.complex128) - ref).abs()[:, mask].max(dim=1).values
    scale = ref.abs()[:, mask].max(dim=1).values
    return float((err / (TOL_G * scale)).max()), float(((rn_out.double() - rn_ref).abs() / (TOL_RN * rn_ref)).max())


def check_pair(pair, rn):
    """The (sum, count) pair of layer_front against the rn it was formed from."""
    assert float(pair[1]) == float(rn.numel()), (float(pair[1]), rn.numel())
    s = float(rn.double().sum())
    return abs(float(pair[0]) - s) / (TOL_SUM * abs(s)) if s != 0 else (0.0 if float(pair[0]) == 0 else math.inf)


# -------------------------------------------------------------------------------------------------------------- the calls
def check_front(sd, M, N, K, k, before, after, y, b, sigma, lower_only, corner_zp, pair=None, g_finite_only=False):
    """Everything layer_front(k) must have done to the state: ``before`` -> ``after``.  ``corner_zp``: the float32 corner_z of
    layer k-1 (None at k = 0); ``pair``: the (sum, count) it wrote.  -> {stage: ratio, 'yard_h': ..., 'scale': [B]}; raises where
    something outside the stage's outputs changed.  ``g_finite_only``: of G and rn only finiteness (seeded states)."""
    cur, prv = k & 1, (k & 1) ^ 1
    B, D = y.shape
    n = D + 1
    last = k == K - 1
    prev = None if k == 0 else Prev(k, before, corner_zp)
    out = {}
    untouched = [f"phi{prv}", f"h{prv}", "alpha"]
    out["phi"] = check_phi(sd, k, after[f"phi{cur}"], y, b, prev)
    if last:   # phi only: zeta on the fly, nothing else written
        assert_unchanged(before, after, untouched + ["G", "Z", f"h{cur}", "rn"], f"front({k})")
        return out
    tri = tril_mask(n)
    if k == 0:
        untouched.append("Z")   # (layer 1 takes it as zero)
    else:
        out["Z"] = check_z(after["Z"], prev, lower_only)
        if lower_only:
            assert torch.equal(bits(after["Z"])[:, ~tri], bits(before["Z"])[:, ~tri]), f"front({k}): upper triangle of Z written"
    if lower_only:
        assert torch.equal(bits(after["G"])[:, ~tri], bits(before["G"])[:, ~tri]), f"front({k}): upper triangle of G written"
    assert_unchanged(before, after, untouched, f"front({k})")
    out["h"], out["yard_h"], out["scale"] = check_h(sd, k, after[f"h{cur}"], sigma, M, N, prev)
    if g_finite_only:
        mask = tri if lower_only else torch.ones(n, n, dtype=torch.bool)
        assert bool(torch.isfinite(torch.view_as_real(after["G"])[:, mask]).all()) and bool(torch.isfinite(after["rn"]).all())
    else:
        out["G"], out["rn"] = check_g(sd, k, after["G"], after["rn"], after[f"phi{cur}"], after[f"h{cur}"],
                                      None if k == 0 else after["Z"], lower_only)
    if pair is not None:
        out["pair"] = check_pair(pair, after["rn"])
    return out


def check_back(sd, k, before, after, mean):
    """layer_back(k): alpha from rn and the mean, nothing else.  -> {'alpha': ratio, 'yard_alpha': ...}"""
    assert_unchanged(before, after, [key for key in KEYS if key != "alpha"], f"back({k})")
    r, yard = check_alpha(sd, k, after["alpha"], before["rn"], mean)
    return {"alpha": r, "yard_alpha": yard}


def worst(acc, new):
    """Fold the ratios and yardsticks of one call into the running maxima of a case.  A NaN stays: Python's max() would drop it."""
    for key, v in new.items():
        if key != "scale":
            old = acc.get(key, 0.0)
            acc[key] = old if (old != old or v <= old) else v
    return acc


def failed(res):
    return {key: v for key, v in res.items() if not key.startswith("yard") and key != "scale" and not passes(v)}


# ------------------------------------------------------------------------------------------------ the cases both suites run
K_CASE, B_CASE = 3, 6
CASES = [   # (Nb, Nd, perturb)
    (1, 1, 0.5),      # n = 2, below the matrix-function route's D >= 8
    (2, 4, 0.3),
    (10, 10, 0.0),
    (10, 10, 1.0),
    (8, 16, 0.5),
    (3, 43, 0.5),     # D = 129: first padded / half-storage size
    (10, 16, 0.5),
    (16, 16, 0.5),
]
# K = 4 on top of the K = 3 every case runs: with K = 3 the only layer that reads a stored, non-zero Z is the last one, which
# forms zeta on the fly and stores nothing; at K = 4 front(2) streams the update of a stored Z (no PM_ZZERO)
K4_CASES = [(10, 10, 1.0), (10, 16, 0.5), (16, 16, 0.5)]
HEAD_GEOMS = [(1, 1), (2, 4), (3, 11), (10, 10), (3, 43), (16, 16)]   # D = 1, 8, 33, 100, 129, 256
HEAD_LS = [1, 3, 5, 16]
K_HEAD = 2
SEED_CASES = [(10, 10, 1.0), (16, 16, 0.5)]   # of CASES: the ones that take the seeded states
ALPHA_SEED = (0.0, 1e-3, 1.0, 2.5, 0.0, 1.0)
RN_SEED = (0.0, 1e-20, 1.0, 1.0, 1e3, 1e30)
MEAN_SEED = (0.0, 0.5, 1e3)


def case_inputs(Nb, Nd, perturb, K=K_CASE, B=B_CASE, head=False, L=3):
    """(sd, y, b, sigma) of a case: R.make_weights(seed=7, perturb) and synth.make_batch(seed=13)."""
    from admm_net_amd import synth
    sd = R.make_weights(Nb, Nd, K, L=L, seed=7, head=head, perturb=perturb)
    y, b, s, _ = synth.make_batch(B, Nb, Nd, seed=13)
    return sd, torch.from_numpy(y), torch.from_numpy(b), torch.from_numpy(s)


# Seeded states: written into the state after back(0) (a dict key -> tensor: CPU snapshots or the device views), before front(1).
# ``ctx``: dict(sd, sigma, M, N, corner_zp) -- the weights, the case's sigma and the float32 corner_z of layer 0.
def _projection_for_diag(state, ctx, gdiag):
    """projection_parts (with t and tc) of layer 1, float64 oracle, on ``state`` with the D x D diagonal of G set to gdiag [B, D]."""
    cpu = {key: v.detach().cpu().clone() for key, v in state.items()}
    B, n = cpu["G"].shape[0], cpu["G"].shape[-1]
    idx = torch.arange(n - 1)
    cpu["G"][:, idx, idx] = gdiag.float().to(torch.complex64)
    G, Zn = layer_inputs(Prev(1, cpu, ctx["corner_zp"]), B, n - 1, "f64")
    return projection_parts(R.cast_weights(ctx["sd"], "f64"), 1, G, Zn, ctx["sigma"].double(), ctx["M"], ctx["N"], with_t=True)


def seed_clamp(state, ctx, shrink=0.2):
    """G and Z a thousand times smaller, then the D x D diagonal of G set so that t cancels all but ``shrink`` of the 0.1 tanh
    correction: tc, and with it cval, is ``shrink`` times what it is at layer 0, the unclamped scale 1 / shrink times -- the
    H-projection clamps -- and |cval| / (A linf + sum|tc|) stays what it is at layer 0.  (The shrinking of G and Z alone does
    not get there: the correction does not shrink with t, the scale stays at 0.2 .. 0.9 on these cases; and lowering the whole
    diagonal by one value makes cval small by cancellation, outside the conditioning.)  t depends on the diagonal through
    t_i = G_ii (1 + alpha / rho) - alpha h_prev,i / rho and the correction on t, so the diagonal is found by fixed-point
    iteration on the float64 oracle."""
    state["G"].mul_(1e-3)
    state["Z"].mul_(1e-3)
    D = state["G"].shape[-1] - 1
    idx = torch.arange(D)
    rho = F.softplus(ctx["sd"]["hLayers.1.rho"].double()) + R.EPS
    slope = 1 + state["alpha"].detach().cpu().double().reshape(-1, 1) / rho      # dt_i / dG_ii
    gd = state["G"].detach().cpu()[:, idx, idx].real.double()
    for _ in range(30):
        _, _, _, t, tc = _projection_for_diag(state, ctx, gd)
        gd = gd + (-(1 - shrink) * (tc - t) - t) / slope
    state["G"][:, idx, idx] = gd.float().to(torch.complex64).to(state["G"].device)


def seed_negative_cval(state, ctx, value=-5.0):
    """A negative diagonal of G's D x D block: t, tr and with them cval turn negative -- a negative scale, which the
    reference leaves unclamped.  With every t_i at -linf, |cval| / (A linf + sum|tc|) is (D - A) / (D + A) at best, A = 2 sqrt(D)
    sigma + sigma^2: a signal whose sigma puts that below 0.1 cannot be seeded inside the conditioning and keeps its G.
    -> the mask [B] of the seeded signals."""
    D = state["G"].shape[-1] - 1
    sg = ctx["sigma"].double().reshape(-1)
    A = 2 * math.sqrt(D) * sg + sg ** 2
    ok = (D - A) / (D + A) >= 0.1
    idx = torch.arange(D)
    rows = torch.nonzero(ok).flatten()
    for i in rows.tolist():
        state["G"][i, idx, idx] = value
    return ok


def seed_alpha(state, ctx=None):
    state["alpha"].copy_(torch.tensor(ALPHA_SEED, dtype=torch.float32).to(state["alpha"].device))


def seed_rn(state, ctx=None):
    state["rn"].copy_(torch.tensor(RN_SEED, dtype=torch.float32).to(state["rn"].device))
