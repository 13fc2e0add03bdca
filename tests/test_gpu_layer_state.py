"""GPU (-m gpu): every stage of the inference forward, layer by layer, against the float64 oracle -- prep_kernel and
half_image_kernel (csrc/prep.hip: the lazy Z update, phi, the H-layer), rn_sum_kernel, the mean kernels and zstep_kernel
(csrc/zstep.hip), headkv_kernel and head_kernel (csrc/head.hip) -- which the rest of the suite sees only through phi after K
layers.

sharded.HipLayerEngine is driven by hand: begin(), per layer front(k) and back_pair(k, pair), finish().  After every call the
state is downloaded through HipLayerEngine.state() and each stage is checked against the device's OWN previous state, its
float32 values evaluated in float64 by the oracle (tests/layer_checks.py states the bounds and how they are derived), so errors
do not compound across layers.  Everything a call is not meant to write must keep its bits.

Cases: K = 3, B = 6, R.make_weights(seed=7, perturb=p), synth.make_batch(seed=13) at D = 1, 8, 100 (p = 0 and 1), 128, 129, 160,
256 (layer_checks.CASES), and K = 4 at D = 100, 160, 256 (the one layer that updates a stored, non-zero Z), under
  * the default route (prep PM_SMALL, the Z update folded into the fused kernel, half_image_kernel for rejected matrices;
    D = 1 lies below the matrix-function route and runs PM_LEAN),
  * Options(spectral=0): PM_LEAN at D <= 128, full storage and the sweep at 129 and 160, PM_HALF with the image at 256,
  * Options(arrow=0) at D = 8, 100, 160: the dense first layer, PM_FIRST with the full image, full storage.
No combination is skipped: route_for reports a route error for none of them.

Seeded states, written through the view after back(0) (layer_checks.seed_*): the clamp branch of the H-projection (unclamped
scale > 1.05 on every signal), a negative cval (negative scale, unclamped), alpha = (0, 1e-3, 1, 2.5, 0, 1) with its exact-zero
case of the Z update (at K = 4 also after back(1), over a stored non-zero Z), and rn = (0, 1e-20, 1, 1, 1e3, 1e30) with chosen means (0 among them) through back(k, mean).

Measured on the MI355X, worst error / bound over all the cases above (1 = the bound), the float32 oracle's figure from
tests/test_layer_checks.py on the CPU beside it, and the largest yardstick of the measured bounds (3 x yardstick + 4 u):
  stage            device   float32 oracle   yardstick (device run / CPU run)
  Z update         0.47     0.50             -- (derived: 4 u)
  phi              0.36     0.29             -- (derived: 12 u)
  h                0.83     0.30             8.1e-7 / 7.9e-7 of max|h| (the clamp seed; 1.5e-7 .. 2.9e-7 on the natural cases)
  alpha            0.34     0.24             1.7e-7 / 1.9e-7 relative
  head tau         0.15     0.15             5.8e-8 / 6.1e-8 absolute
  head f           0.18     0.16             8.0e-8 / 7.2e-8 absolute
  head confidence  0.15     0.14             6.0e-8 / 5.8e-8 absolute
  G                0.87     0.68 (*)         -- (2e-5 max|G_ref|)
  rn               0.092    3.99 (*)         -- (1e-5 relative)
  (sum, count)     0        0                -- (1e-13 relative: every sum came out equal to the float64 sum)
  (*) of layers whose float32 LAPACK result the oracle's own G / rn miss or nearly miss: these two bounds are the project's,
      for its kernels, and tests/test_layer_checks.py does not hold the float32 oracle to them.
The worst h (0.83) is D = 160, layer 1, on all three option sets: 2.6e-7 max|h| against a yardstick of 2.3e-7.  No check failed
on the device and no kernel was changed.
"""
import ctypes

import pytest
import torch

import admm_net_amd as A
from admm_net_amd import _lib, sharded
from admm_net_amd.options import Options
import layer_checks as LC

pytestmark = pytest.mark.gpu

S_CORNER_Z = 7          # slot of corner_z in a layer's packed weights (csrc/common.h)
OPTION_SETS = {"default": None, "spectral0": dict(spectral=0), "arrow0": dict(arrow=0)}
ARROW0_D = (8, 100, 160)


def _id(Nb, Nd, p, opt):
    return f"D{Nb * Nd}_p{p}-{opt}"


NATURAL = [pytest.param(Nb, Nd, p, opt, id=_id(Nb, Nd, p, opt)) for opt in OPTION_SETS for Nb, Nd, p in LC.CASES
           if opt != "arrow0" or Nb * Nd in ARROW0_D]
SEEDED = [pytest.param(Nb, Nd, p, opt, seed, id=_id(Nb, Nd, p, opt) + "-" + seed) for Nb, Nd, p in LC.SEED_CASES
          for opt in ("default", "spectral0") for seed in ("clamp", "negative_cval", "alpha")]
SEEDS = dict(clamp=LC.seed_clamp, negative_cval=LC.seed_negative_cval, alpha=LC.seed_alpha)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def _engine(dev, sd, y, b, s, Nb, Nd, K, opt, head=False, L=3):
    cls = A.ADMMNet if head else A.PhiEstADMMNet
    m = cls(M=Nb, N=Nd, L=L, num_layers=K).eval()
    m.load_state_dict(sd)
    if OPTION_SETS[opt] is not None:
        m.options = Options(**OPTION_SETS[opt])
    return sharded.HipLayerEngine(m, y.to(dev), b.to(dev), s.to(dev))


def _views(eng):
    st = eng.state()
    return dict(G=st.G, Z=st.Z, phi0=st.phi(0), phi1=st.phi(1), h0=st.h(0), h1=st.h(1), alpha=st.alpha, rn=st.rn), st


def _snap(eng):
    torch.cuda.synchronize()
    return {key: v.detach().cpu().clone() for key, v in _views(eng)[0].items()}


def _corner_z(eng, k):
    off = eng.lib.admmnet_layer_weight_offset(ctypes.byref(eng.cfg), k)
    return float(eng.W[off + S_CORNER_Z].item())


def _drive(eng, sd, y, b, s, seed=None, g_finite_only=False, seed_after=0):
    """The whole layer sequence with every check; -> the worst ratio per stage (and 'scale{k}', the oracle's unclamped scales).
    ``seed(views, ctx)`` runs after back(seed_after); ``g_finite_only``: of the G and rn of the layer behind it only finiteness."""
    M, N, K = eng.m.M, eng.m.N, eng.m.num_layers
    lower_only = eng.state().lower_only
    res = {}
    eng.begin()
    for k in range(K):
        before = _snap(eng)
        pair_before = eng.sumcnt.detach().cpu().clone()
        sc = eng.front(k)
        after = _snap(eng)
        pair = sc.detach().cpu().clone()
        last = k == K - 1
        if last:
            assert torch.equal(pair.view(torch.int64), pair_before.view(torch.int64)), "front(K - 1) wrote the pair"
        out = LC.check_front(sd, M, N, K, k, before, after, y, b, s, lower_only, _corner_z(eng, k - 1) if k else None,
                             pair=None if last else pair, g_finite_only=g_finite_only and k == seed_after + 1)
        res[f"scale{k}"] = out.get("scale")
        LC.worst(res, out)
        if last:
            break
        eng.back_pair(k, sc)
        now = _snap(eng)
        LC.worst(res, LC.check_back(sd, k, after, now, LC.mean_of_pair(pair)))
        if k == seed_after and seed is not None:
            views, _ = _views(eng)
            res["seeded"] = seed(views, dict(sd=sd, sigma=s, M=M, N=N, corner_zp=_corner_z(eng, 0)))
    before = _snap(eng)
    phi, head = eng.finish()
    after = _snap(eng)
    LC.assert_unchanged(before, after, LC.KEYS, "finish()")
    assert LC.same_bits(phi.cpu(), after[f"phi{(K - 1) & 1}"]), "finish(): phi_out is not the last layer's phi"
    assert int(eng.status[0].item()) == 0
    return res, head


def _report(what, res):
    show = {key: f"{v:.3g}" for key, v in res.items() if not key.startswith("scale") and key != "seeded"}
    print("LAYERSTATE", what, show)


def _stages(res):
    return {key: v for key, v in res.items() if not key.startswith("scale") and key != "seeded"}


# ----------------------------------------------------------------------------------------------------------- natural cases
@pytest.mark.parametrize("Nb,Nd,p,opt", NATURAL)
def test_every_stage_of_every_layer(dev, Nb, Nd, p, opt):
    sd, y, b, s = LC.case_inputs(Nb, Nd, p)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, LC.K_CASE, opt)
    D = Nb * Nd
    full = opt == "arrow0" or (opt == "spectral0" and 128 < D < 176)
    assert eng.state().lower_only == (not full)
    res, _ = _drive(eng, sd, y, b, s)
    _report(_id(Nb, Nd, p, opt), res)
    assert not LC.failed(_stages(res)), res
    for k in range(1, LC.K_CASE - 1):   # the natural run never clamps at k >= 1 (the seeded states do)
        assert bool((res[f"scale{k}"] < 0.95).all()), res[f"scale{k}"]


K4 = [pytest.param(Nb, Nd, p, opt, id=_id(Nb, Nd, p, opt)) for opt in OPTION_SETS for Nb, Nd, p in LC.K4_CASES
      if opt != "arrow0" or Nb * Nd in ARROW0_D]


@pytest.mark.parametrize("Nb,Nd,p,opt", K4)
def test_update_of_a_stored_z(dev, Nb, Nd, p, opt):
    """K = 4: front(2) is the one call that streams Z <- Z + alpha (G - C_prev) over a stored, non-zero Z (at k = 1 the buffer is
    taken as zero, the last layer forms zeta on the fly) -- in the fused kernel's first sweep, PM_LEAN, PM_HALF or the full
    stream, by the option set."""
    sd, y, b, s = LC.case_inputs(Nb, Nd, p, K=4)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, 4, opt)
    res, _ = _drive(eng, sd, y, b, s)
    _report(_id(Nb, Nd, p, opt) + " K=4", res)
    assert not LC.failed(_stages(res)), res


@pytest.mark.parametrize("Nb,Nd,p,opt", K4)
def test_alpha_zero_keeps_a_stored_z(dev, Nb, Nd, p, opt):
    """K = 4 with alpha = (0, 1e-3, 1, 2.5, 0, 1) written after back(1): front(2) then updates a stored, non-zero Z, and the Z of
    the two signals with alpha = 0 must keep its bits (check_z asserts it; at front(1), where the seeded states run, the Z
    read is zero and the same check only says that zero comes out)."""
    sd, y, b, s = LC.case_inputs(Nb, Nd, p, K=4)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, 4, opt)
    res, _ = _drive(eng, sd, y, b, s, seed=LC.seed_alpha, g_finite_only=True, seed_after=1)
    _report(_id(Nb, Nd, p, opt) + " K=4 seeded alpha", res)
    assert not LC.failed(_stages(res)), res
    torch.cuda.synchronize()
    Z = eng.state().Z.cpu()
    tri = LC.tril_mask(Z.shape[-1])
    zero = [i for i, a in enumerate(LC.ALPHA_SEED) if a == 0]
    assert bool((Z[zero][:, tri].abs().amax(dim=1) > 0).all())   # the Z that was kept is not the trivial zero


# ------------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("L", LC.HEAD_LS)
@pytest.mark.parametrize("Nb,Nd", LC.HEAD_GEOMS, ids=[f"D{a * b}" for a, b in LC.HEAD_GEOMS])
def test_head_from_the_devices_own_phi(dev, Nb, Nd, L):
    """D = 1 .. 256 crosses every stride of the softmax (t = lane; t < D; t += 64) and of the score loop, L = 1 .. 16 every
    regressor slot."""
    sd, y, b, s = LC.case_inputs(Nb, Nd, 0.5, K=LC.K_HEAD, head=True, L=L)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, LC.K_HEAD, "default", head=True, L=L)
    eng.begin()
    eng.back_pair(0, eng.front(0))
    eng.front(1)
    phi, head = eng.finish()
    torch.cuda.synchronize()
    assert head.shape == (3, LC.B_CASE, L)
    ratios, yards = LC.check_head(sd, head.cpu(), phi.cpu(), Nb, Nd, L)
    print("LAYERSTATE head", f"D={Nb * Nd} L={L}", {k: f"{v:.3g}" for k, v in ratios.items()},
          {k: f"{v:.3g}" for k, v in yards.items()})
    assert all(LC.passes(v) for v in ratios.values()), (ratios, yards)


# --------------------------------------------------------------------------------------------------------- seeded states
@pytest.mark.parametrize("Nb,Nd,p,opt,seed", SEEDED)
def test_seeded_state(dev, Nb, Nd, p, opt, seed):
    sd, y, b, s = LC.case_inputs(Nb, Nd, p)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, LC.K_CASE, opt)
    res, _ = _drive(eng, sd, y, b, s, seed=SEEDS[seed], g_finite_only=True)
    _report(_id(Nb, Nd, p, opt) + " seeded " + seed, res)
    sc = res["scale1"]
    if seed == "clamp":
        assert bool((sc > 1.05).all()), sc
    if seed == "negative_cval":
        assert int(res["seeded"].sum()) >= LC.B_CASE - 1 and bool((sc[res["seeded"]] < 0).all()), (res["seeded"], sc)
    assert not LC.failed(_stages(res)), res


@pytest.mark.parametrize("opt", ["default", "spectral0"])
def test_alpha_from_seeded_rn_and_a_chosen_mean(dev, opt):
    """back(k, mean) on rn = (0, 1e-20, 1, 1, 1e3, 1e30) with the means 0, 0.5 and 1e3 against R.z_step(..., mean_norm=mean)."""
    Nb, Nd, p = LC.SEED_CASES[0]
    sd, y, b, s = LC.case_inputs(Nb, Nd, p)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, LC.K_CASE, opt)
    eng.begin()
    eng.front(0)
    worst = {}
    for k in range(LC.K_CASE - 1):
        for mean in LC.MEAN_SEED:
            LC.seed_rn(_views(eng)[0])
            before = _snap(eng)
            eng.back(k, torch.tensor(mean, dtype=torch.float32))
            out = LC.check_back(sd, k, before, _snap(eng), mean)
            assert LC.passes(out["alpha"]), (k, mean, out)
            LC.worst(worst, out)
    _report(f"alpha on seeded rn {opt}", worst)


# ------------------------------------------------------------------------------------------------------- the (sum, count) pair
@pytest.mark.parametrize("B", [1, 1023, 1025, 2500])
def test_pair_at_large_batches(dev, B):
    """The single-trip (B <= 1024) and the strided (B > 1024) path of rn_sum_kernel."""
    Nb, Nd, K = 1, 2, 2
    sd, y, b, s = LC.case_inputs(Nb, Nd, 0.5, K=K, B=B)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, K, "default")
    eng.begin()
    pair = eng.front(0)
    torch.cuda.synchronize()
    rn = eng.state().rn.cpu()
    assert bool(torch.isfinite(rn).all()) and bool((rn > 0).all())
    r = LC.check_pair(pair.cpu(), rn)
    print("LAYERSTATE pair", f"B={B}", f"{r:.3g}")
    assert LC.passes(r), (r, pair.tolist())


# ---------------------------------------------------------------------------------------------------------------- stale state
@pytest.mark.parametrize("Nb,Nd,p", [(10, 10, 1.0), (16, 16, 0.5)], ids=["D100", "D256"])
def test_stale_state_is_never_read(dev, Nb, Nd, p):
    """NaN in every byte of the state before begin() -- only in the spans admmnet_state_layout reports, the chunk buffers
    behind them hold indices -- changes no bit of phi, h, alpha, rn, the stored triangles of G and Z or the outputs against a
    run from a zero-filled workspace; on lower-only storage the other triangle still holds the fill."""
    sd, y, b, s = LC.case_inputs(Nb, Nd, p)
    eng = _engine(dev, sd, y, b, s, Nb, Nd, LC.K_CASE, "default")
    K = LC.K_CASE
    n = Nb * Nd + 1

    def run():
        eng.begin()
        for k in range(K):
            sc = eng.front(k)
            if k < K - 1:
                eng.back_pair(k, sc)
        phi, _ = eng.finish()
        return _snap(eng), phi.cpu().clone(), eng.status.cpu().clone()

    eng.ws.zero_()
    clean, phi_clean, st_clean = run()
    layout = eng.state()
    assert layout.lower_only
    for name, (off, size) in layout.spans.items():
        eng.ws[off:off + size].view(torch.float32).fill_(float("nan"))
    stale, phi_stale, st_stale = run()
    tri = LC.tril_mask(n)
    for key in ("phi0", "phi1", "h0", "h1", "alpha", "rn"):
        assert LC.same_bits(clean[key], stale[key]), key
    for key in ("G", "Z"):
        assert torch.equal(LC.bits(clean[key])[:, tri], LC.bits(stale[key])[:, tri]), key
        assert bool(torch.isnan(torch.view_as_real(stale[key])[:, ~tri]).all()), f"{key}: the upper triangle was written"
        assert bool((torch.view_as_real(clean[key])[:, ~tri] == 0).all()), f"{key}: the upper triangle was written"
    assert LC.same_bits(phi_clean, phi_stale) and torch.equal(st_clean, st_stale)
    assert bool(torch.isfinite(torch.view_as_real(phi_stale)).all())
