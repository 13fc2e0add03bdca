"""Float64 host mirror of the device scene generator with a varying number of targets (scenes_kernel in csrc/synth.hip, behind
admmnet_synth_scenes / synth.make_scenes_device), numpy only (TEST INFRASTRUCTURE).

A subclass of synth_mirror.SynthMirror: the draws, the symbols, the noise and the labels are that mirror's, unchanged.  What
this one restates is the part of the recipe that differs (header comment of admmnet_synth_scenes, include/admmnet.h):

    count      n = lo + min(hi - lo, floor(u (hi - lo + 1))),  u = uniform(bits(seed, s, stream 8, 0))
    positions  target l < n, attempt t = 0 .. 31:  tau = 0.1 + 0.8 uniform(TAU, l + 8 t),  f = -0.4 + 0.8 uniform(F, l + 8 t);
               targets are placed in order; an attempt is accepted when every target j < l already placed is at least
               min_sep away, d^2 = (Nd wrap(dtau))^2 + (Nb wrap(df))^2 >= min_sep^2, wrap(d) = d - round(d);
               min_sep = 0 accepts attempt 0 unseen; after 32 refusals the last attempt stays and the scene's state is 1
    C          of target l as before (stream C, pair l), whatever the attempt
    padding    slots l >= n are exact zeros in tau, f, C and add nothing to psi
    extras     L_true = n, snr_db = the SNR draw, noise_var = w_std^2, ser = 100 #{dd != data} / D, state

Besides those, ``run`` returns per scene ``attempt`` [S, hi] (the attempt each target was accepted at, 32 if none was, -1 past n) and
``sep_margin`` [S]: the smallest |d / min_sep - 1| over every distance it evaluated (inf where it evaluated none) -- how close
the scene came to deciding an attempt the other way, which is what a comparison with another float64 evaluation depends on.
Every step is a method, so that tests/test_scene_mirror.py can derive copies with one mistake each.
"""
import numpy as np

import synth_mirror as SM
from synth_mirror import F, TAU, TWO_PI, uniform

COUNT = 8                    # stream number of the target count
ATTEMPTS = 32
MAXL = 8


class SceneMirror(SM.SynthMirror):
    # ---- pieces of the recipe that a wrong kernel could get wrong ------------------------------------------------
    def count(self, u, lo, hi):
        return lo + np.minimum(hi - lo, np.floor(u * (hi - lo + 1)).astype(np.int64))

    def attempt_index(self, l, t):
        return l + MAXL * t

    def wrap(self, d):
        return d - np.round(d)

    def distance2(self, dtau, df, Nb, Nd):
        """In resolution cells: tau runs along the axis of length Nd, f along the one of length Nb."""
        return (Nd * self.wrap(dtau)) ** 2 + (Nb * self.wrap(df)) ** 2

    def stops(self, accepted):
        """Whether the attempts of a target end here."""
        return accepted

    def pad(self, values, n):
        """Slots l >= n of [S, hi] hold exact zeros."""
        return np.where(np.arange(values.shape[1])[None, :] < n[:, None], values, 0)

    def noise_variance(self, w_std):
        return w_std ** 2

    # ---- the recipe ----------------------------------------------------------------------------------------------
    def counts(self, samples, lo, hi, seed):
        samples = np.asarray(samples, dtype=np.int64).reshape(-1)
        return self.count(uniform(self.bits(seed, samples, COUNT, [0]))[:, 0], lo, hi)

    def place(self, samples, Nb, Nd, n, hi, min_sep, seed):
        """(tau, f [S, hi] unpadded, attempt [S, hi], state [S], sep_margin [S])."""
        S = len(samples)
        idx = np.array([[self.attempt_index(l, t) for t in range(ATTEMPTS)] for l in range(hi)])      # [hi, 32]
        tau_all = (0.1 + 0.8 * uniform(self.bits(seed, samples, TAU, idx.reshape(-1)))).reshape(S, hi, ATTEMPTS)
        f_all = (-0.4 + 0.8 * uniform(self.bits(seed, samples, F, idx.reshape(-1)))).reshape(S, hi, ATTEMPTS)
        tau, f = tau_all[:, :, 0].copy(), f_all[:, :, 0].copy()
        attempt = np.where(np.arange(hi)[None, :] < n[:, None], 0, -1)
        state, margin = np.zeros(S, dtype=np.int64), np.full(S, np.inf)
        if min_sep == 0.0:
            return tau, f, attempt, state, margin
        for s in range(S):
            for l in range(int(n[s])):
                for t in range(ATTEMPTS):
                    tau[s, l], f[s, l], attempt[s, l] = tau_all[s, l, t], f_all[s, l, t], t
                    d2 = self.distance2(tau[s, l] - tau[s, :l], f[s, l] - f[s, :l], Nb, Nd)
                    if l:
                        margin[s] = min(margin[s], float(np.abs(np.sqrt(d2) / min_sep - 1.0).min()))
                    accepted = bool((d2 >= min_sep * min_sep).all())
                    if self.stops(accepted):
                        break
                else:
                    state[s], attempt[s, l] = 1, ATTEMPTS
        return tau, f, attempt, state, margin

    def run(self, samples, Nb, Nd, targets, seed, snr_range=(5.0, 25.0), snr_e=7.0, rho=1.0, label_iters=5, min_sep=0.0):
        samples = np.asarray(samples, dtype=np.int64).reshape(-1)
        lo, hi = (targets, targets) if np.isscalar(targets) else targets
        D = Nb * Nd
        r = super().run(samples, Nb, Nd, hi, seed, snr_range, snr_e, rho, label_iters)   # draws, symbols, b, e, sigma
        n = self.counts(samples, lo, hi, seed)
        tau, f, r["attempt"], r["state"], r["sep_margin"] = self.place(samples, Nb, Nd, n, hi, float(min_sep), seed)
        r["L_true"] = n
        r["tau"], r["f"], r["C"] = self.pad(tau, n), self.pad(f, n), self.pad(r["C"], n)
        ib, idd = self.grid_index(Nb, Nd)
        r["psi"] = (r["C"][:, :, None] * np.exp(1j * TWO_PI * self.phase(ib, idd, r["f"], r["tau"]))).sum(axis=1)
        r["real_y"] = (r["b"] + r["e"]) * r["psi"]
        r["w_std"] = self.noise_std(self.energy(r["real_y"]), r["snr"], D)
        r["y"] = r["real_y"] + r["w_std"] * np.sqrt(0.5) * r["noise_normals"]
        r["phi"] = self.labels(r["y"], r["b"], rho, label_iters)
        r["snr_db"] = r["snr"][:, 0]
        r["noise_var"] = self.noise_variance(r["w_std"][:, 0])
        r["ser"] = 100.0 * (r["dd"] != r["data"]).sum(axis=1) / D
        r["min_sep"] = float(min_sep)
        return r


def pair_distances(tau, f, n, Nb, Nd):
    """[hi, hi] distances in cells between the first n slots of one scene (inf elsewhere and on the diagonal), float64."""
    tau, f = np.asarray(tau, dtype=np.float64), np.asarray(f, dtype=np.float64)
    wrap = lambda d: d - np.round(d)  # noqa: E731
    d = np.sqrt((Nd * wrap(tau[:, None] - tau[None, :])) ** 2 + (Nb * wrap(f[:, None] - f[None, :])) ** 2)
    out = np.full_like(d, np.inf)
    out[:n, :n] = d[:n, :n]
    np.fill_diagonal(out, np.inf)
    return out
