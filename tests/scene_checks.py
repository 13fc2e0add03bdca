"""The comparison of admmnet_synth_scenes' outputs with the float64 mirror (tests/scene_mirror.py) and the cases it is run at.

Used by tests/test_scene_mirror.py (CPU: the mirror against copies of itself with one mistake each) and by
tests/test_gpu_scenes.py (the device kernel against the mirror).  (TEST INFRASTRUCTURE)

The float outputs the entry shares with admmnet_synth_batch go through synth_checks.compare unchanged.  ``snr_db``, ``noise_var``
(float64) and ``ser`` (float32) are held to the same bound -- one spacing of the output type plus SLACK times the magnitude --
and ``L_true`` and ``state`` to equality.  A scene whose placement came within SEP_MARGIN_MIN of deciding an attempt the other way
would be left out; on every case here the smallest margin is 3.3e-4, so none is, and the callers assert that.
"""
import numpy as np

import synth_checks as SC

SEP_MARGIN_MIN = 1e-9
SCALARS = {"snr_db": np.float64, "noise_var": np.float64, "ser": np.float32}
INTEGERS = {"L_true": np.int64, "state": np.int32}


def compare(got, ref):
    """``got``: the outputs as the entry point delivers them, for the samples of ``ref`` = a SceneMirror result.  The report of
    synth_checks.compare, with the scalar outputs added to ``ratio`` / ``share`` and ``left_out_scenes``."""
    keep = ref["sep_margin"] >= SEP_MARGIN_MIN
    pick = lambda d: {k: (v[keep] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == keep.size else v)  # noqa: E731
                      for k, v in d.items()}
    if not keep.all():
        got, ref = pick(got), pick(ref)
    rep = SC.compare(got, ref)
    rep["left_out_scenes"] = int((~keep).sum())
    for k, want_t in SCALARS.items():
        g = np.asarray(got[k])
        if g.dtype != want_t or g.shape != ref[k].shape:
            rep["failures"].append("%s: %s %s, expected %s %s" % (k, g.dtype, g.shape, np.dtype(want_t), ref[k].shape))
            continue
        cast = ref[k].astype(want_t)
        err = np.abs(g.astype(np.float64) - cast.astype(np.float64))
        bound = np.spacing(np.abs(cast)).astype(np.float64) + SC.SLACK * np.abs(ref[k])
        rep["ratio"][k] = float(np.nan_to_num(err / bound, nan=np.inf).max()) if err.size else 0.0
        rep["share"][k] = float((g != cast).mean()) if err.size else 0.0
        if not rep["ratio"][k] <= 1.0:
            rep["failures"].append("%s: worst error / bound %.3g" % (k, rep["ratio"][k]))
    for k, want_t in INTEGERS.items():
        g = np.asarray(got[k])
        if g.dtype != want_t or g.shape != ref[k].shape:
            rep["failures"].append("%s: %s %s, expected %s %s" % (k, g.dtype, g.shape, np.dtype(want_t), ref[k].shape))
        elif not np.array_equal(g, ref[k]):
            rep["failures"].append("%s: %d scenes differ" % (k, int((g != ref[k]).sum())))
    return rep


def cast_outputs(ref, labels=True):
    """A mirror result delivered as the entry point would."""
    out = SC.cast_outputs(ref, labels)
    out.update({k: ref[k].astype(t) for k, t in {**SCALARS, **INTEGERS}.items()})
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def case(Nb, Nd, targets, min_sep, B, seed=5, snr_range=(5.0, 25.0), rho=1.0, label_iters=5, samples=None):
    return dict(Nb=Nb, Nd=Nd, targets=targets, min_sep=min_sep, B=B, seed=seed, snr_range=snr_range, snr_e=7.0, rho=rho,
                label_iters=label_iters, samples=list(range(B)) if samples is None else samples)


FIRST = (4, 6, (1, 3), 2.0, 16)
CASES = {
    "4x6_1to3_sep2": case(*FIRST),                               # six redraws, one at attempt 23, no state 1
    "4x6_2to3_sep2.5": case(4, 6, (2, 3), 2.5, 16),              # both states, one target accepted at attempt 31
    "6x4_2to3_sep2": case(6, 4, (2, 3), 2.0, 16, seed=11),       # the axes exchanged
    "15x17_1to8_sep1.5": case(15, 17, (1, 8), 1.5, 64),          # every count 1 .. 8
    "1x12_1to3_sep1": case(1, 12, (1, 3), 1.0, 64),              # an axis of length 1
    "1x1_1to1_sep0.5": case(1, 1, (1, 1), 0.5, 3),
    "26x131_2to3_sep8": case(*SC.MAX_D_GRID, (2, 3), 8.0, 2, rho=2.0),      # the largest D, with labels
    "4x6_2to3_sep10": case(4, 6, (2, 3), 10.0, 16),              # infeasible: every scene has state 1
    "grid_2x2_B70000": case(2, 2, (1, 2), 0.5, 70000, samples=[0, 1, 65535, 65536, 69999]),
    **{"seed_%d" % s: case(*FIRST, seed=s) for s in (0, 2 ** 63 + 12345, 2 ** 64 - 1)},
}


def mirror_of(c, cls=None):
    from scene_mirror import SceneMirror
    return (cls or SceneMirror)().run(c["samples"], c["Nb"], c["Nd"], c["targets"], c["seed"], c["snr_range"], c["snr_e"],
                                      c["rho"], c["label_iters"], c["min_sep"])
