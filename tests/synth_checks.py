"""The one comparison of generator outputs with the float64 mirror (tests/synth_mirror.py), and the cases it is run at.

Used by tests/test_synth_mirror.py (CPU: mirror against copies of itself with one mistake each) and by
tests/test_gpu_synth.py (the device kernel against the mirror).  (TEST INFRASTRUCTURE)

Bound per element (real and imaginary part separately):  |got - f32(ref)| <= spacing_f32(ref) + slack, where slack =
64 * 2^-53 * (sum of the magnitudes of the terms the value is built from) covers a few float64 ulps of the device's
sincos / log / atan2 / pow against libm and FMA contraction.  One float32 spacing is what a correctly rounded cast of a
float64 value a few ulps away from the mirror's may differ by; that happens when the float64 value lies within those
few ulps of a float32 rounding boundary, i.e. for about 2^-53 / 2^-24 ~ 1e-8 of the elements.  The cap SHARE_CAP on
the share of elements not bit-equal to the cast mirror is what makes a float32 intermediate fail: it moves most of an
output by about one float32 ulp, which the per-element bound alone allows.
"""
import numpy as np

MARGIN_MIN = 1e-9            # symbols whose demodulated angle is closer than this to a decision boundary are left out
SLACK = 64.0 * 2.0 ** -53
SHARE_CAP = 1e-3
FLOAT_OUTPUTS = ("tau", "f", "C", "b", "y", "sigma", "phi")


def _parts(a):
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=-1) if np.iscomplexobj(a) else a


def symbols_of(b):
    """The QPSK index dd of b = exp(j (2 pi dd / 4 + pi / 4))."""
    return np.round((np.angle(np.asarray(b).astype(np.complex128)) - np.pi / 4) / (np.pi / 2)).astype(np.int64) % 4


def magnitudes(ref):
    """Per output, the magnitude the slack scales with, broadcastable to the output."""
    m = {k: np.abs(ref[k]) for k in ("tau", "f", "C", "b", "sigma")}
    m["y"] = np.abs(ref["C"]).sum(axis=1, keepdims=True) + ref["w_std"] * np.abs(ref["noise_normals"])
    m["phi"] = (1.0 + ref["rho"] * ref["label_iters"]) * np.abs(ref["y"]).max(axis=1, keepdims=True)
    return m


def compare(got, ref):
    """``got``: dict of the outputs as the entry point delivers them (y, b, C, phi complex64; sigma, tau, f float32; phi
    may be missing), for the samples of ``ref`` = a mirror result.  Returns a report: per output the worst
    error / bound (``ratio``) and the share of elements not bit-equal to f32(ref) (``share``), the symbols left out and
    wrong, and ``failures``, a list of sentences that is empty when everything holds."""
    rep = {"ratio": {}, "share": {}, "failures": []}
    keep = ref["margin"] >= MARGIN_MIN
    rep["left_out"] = int((~keep).sum())
    rep["wrong_symbols"] = int((symbols_of(got["b"]) != ref["dd"])[keep].sum())
    if rep["wrong_symbols"]:
        rep["failures"].append("%d decided symbols differ" % rep["wrong_symbols"])
    mag = magnitudes(ref)
    for k in FLOAT_OUTPUTS:
        if k not in got or got[k] is None:
            continue
        cx = np.iscomplexobj(ref[k])
        g = np.asarray(got[k])
        want_t = np.complex64 if cx else np.float32
        if g.dtype != want_t or g.shape != ref[k].shape:
            rep["failures"].append("%s: %s %s, expected %s %s" % (k, g.dtype, g.shape, np.dtype(want_t), ref[k].shape))
            continue
        cast = _parts(ref[k].astype(want_t))
        gp = _parts(g)
        err = np.abs(gp.astype(np.float64) - cast.astype(np.float64))
        m = mag[k][..., None] if cx else mag[k]
        bound = np.spacing(np.abs(cast)).astype(np.float64) + SLACK * m
        with np.errstate(invalid="ignore"):
            ratio = float(np.nan_to_num(err / bound, nan=np.inf).max()) if err.size else 0.0
        share = float((gp.view(np.uint32) != cast.view(np.uint32)).mean()) if err.size else 0.0
        rep["ratio"][k], rep["share"][k] = ratio, share
        if not ratio <= 1.0:
            rep["failures"].append("%s: worst error / bound %.3g" % (k, ratio))
        if not share <= SHARE_CAP:
            rep["failures"].append("%s: %.3g of the elements not bit-equal to the cast mirror" % (k, share))
    return rep


def describe(rep):
    return "left out %d, wrong symbols %d; error/bound %s; not bit-equal %s" % (
        rep["left_out"], rep["wrong_symbols"],
        " ".join("%s %.3g" % kv for kv in rep["ratio"].items()), " ".join("%s %.3g" % kv for kv in rep["share"].items()))


def cast_outputs(ref, labels=True):
    """A mirror result delivered as the entry point would: the float64 values cast to complex64 / float32."""
    out = {k: ref[k].astype(np.complex64 if np.iscomplexobj(ref[k]) else np.float32) for k in FLOAT_OUTPUTS}
    if not labels:
        del out["phi"]
    return out


# ---- the cases of the device test ------------------------------------------------------------------------------------
MAX_D = 3406                 # 48 D + 352 bytes of LDS <= 160 KiB, with equality (csrc/synth.hip, SY_MAX_D)
MAX_D_GRID = (26, 131)       # Nb x Nd = MAX_D
OVER_D_GRID = (1, 3407)      # MAX_D + 1


def case(Nb, Nd, L, B, seed=5, snr_range=(5.0, 25.0), snr_e=7.0, rho=1.0, label_iters=5, samples=None):
    return dict(Nb=Nb, Nd=Nd, L=L, B=B, seed=seed, snr_range=snr_range, snr_e=snr_e, rho=rho, label_iters=label_iters,
                samples=list(range(B)) if samples is None else samples)


# geometries run with rho != 1 so that the label side of every one of them tells 1 + rho Sd from rho + Sd
GEOMETRIES = {"%dx%d_L%d_B%d" % g: case(*g, rho=2.0) for g in
              [(1, 1, 1, 3), (4, 6, 3, 16), (6, 4, 3, 16), (10, 10, 3, 8), (8, 16, 3, 64), (15, 17, 8, 4), (16, 16, 3, 4),
               (1, 257, 2, 3), (24, 32, 3, 2), MAX_D_GRID + (3, 2)]}
SEEDS = {"seed_%d" % s: case(4, 6, 3, 16, seed=s) for s in (0, 5, 2 ** 63 + 12345, 2 ** 64 - 1)}
SNR_RANGES = {"snr_%g_%g" % r: case(4, 6, 3, 16, snr_range=r) for r in ((20.0, 20.0), (5.0, 25.0), (-5.0, 0.0))}
LABELS = {"labels_%dx%d_it%d_rho%g" % (g + (it, rho)): case(*g, 3, 8, seed=11, rho=rho, label_iters=it)
          for g in ((4, 6), (10, 10)) for it in (0, 1, 5, 12) for rho in (0.5, 1.0, 2.0)}
GRID_B = 70000
GRID = {"grid_2x2_B70000": case(2, 2, 1, GRID_B, seed=5, samples=[0, 1, 65535, 65536, 69999])}
CASES = {**GEOMETRIES, **SEEDS, **SNR_RANGES, **LABELS, **GRID}


def mirror_of(c, cls=None):
    from synth_mirror import SynthMirror
    return (cls or SynthMirror)().run(c["samples"], c["Nb"], c["Nd"], c["L"], c["seed"], c["snr_range"], c["snr_e"],
                                      c["rho"], c["label_iters"])
