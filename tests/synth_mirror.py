"""Float64 host mirror of the device scene and label generator (csrc/synth.hip), numpy only (TEST INFRASTRUCTURE).

Written from the recipe in the header comment of synth.hip and the reference lines it cites -- generate_data.py:133-221
(_generate_single_sample, _generate_communication_symbols), utils/mathUtils.py:53-111 (pskmod, pskdemod, awgn),
:410-463 / admm.py:77-79 (the phi label) -- as whole-array expressions over (sample, target, symbol), not as the
kernel's loops.  The kernel's generator is counter based, so every draw is a pure function of
(seed, sample index, stream, counter) and the mirror reproduces it exactly:

    bits(seed, s, stream, k) = mix(mix(mix(seed ^ 0xA5A5A5A55A5A5A5A) + s) ^ (stream << 40 | k)),   mix = splitmix64
    uniform(bits)            = ((bits >> 11) + 1/2) 2^-53        in (0, 1]  (the top value rounds to 1 in float64)
    normal pair k            = sqrt(-2 ln u_{2k}) (cos, sin)(2 pi u_{2k+1})                Box-Muller
    streams                    1 tau, 2 f, 3 C, 4 data, 5 demodulation noise, 6 SNR, 7 channel noise

``mirror`` takes explicit sample INDICES, so sample 65536 costs the same as sample 0.  Every step is a method of
``SynthMirror``: tests/test_synth_mirror.py derives copies with one mistake each to show that the comparison of
tests/synth_checks.py notices them.
"""
import numpy as np

U64 = np.uint64
GOLDEN, MUL1, MUL2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)
SEED_MASK = U64(0xA5A5A5A55A5A5A5A)
TAU, F, C, DATA, DEMOD, SNR, NOISE = 1, 2, 3, 4, 5, 6, 7          # stream numbers
TWO_PI = 2.0 * np.pi


def sy_mix(x):
    """splitmix64: the state advances by the golden-ratio increment, the output is its finalizer (mod 2^64)."""
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = x + GOLDEN
        x = (x ^ (x >> U64(30))) * MUL1
        x = (x ^ (x >> U64(27))) * MUL2
    return x ^ (x >> U64(31))


def uniform(bits):
    return ((bits >> U64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def label_recursion(y, b, rho, iters, dtype=np.complex128, denominator=lambda rho, sum_d: 1.0 + rho * sum_d):
    """phi_k = W (y / b + rho phi_{k-1}) from phi_0 = 0, ``iters`` steps, for a batch [S, D].  W = (diag(1 / |b|^2) +
    rho 1 1^T)^-1 applied by Sherman-Morrison: W r = d r - d rho sum(d r) / (1 + rho sum d), d = |b|^2."""
    real = np.float32 if dtype == np.complex64 else np.float64
    y, b, rho = np.asarray(y, dtype=dtype), np.asarray(b, dtype=dtype), real(rho)
    d = (b * np.conj(b)).real
    den = denominator(rho, d.sum(axis=1, keepdims=True)).astype(real)
    phi = np.zeros_like(y)
    for _ in range(iters):
        dr = d * (y / b + rho * phi)
        phi = dr - d * (rho * dr.sum(axis=1, keepdims=True) / den)
    return phi


class SynthMirror:
    noise_stream = NOISE
    second_normal_offset = 1          # the pair k uses the counters 2 k and 2 k + 1
    label_dtype = np.complex128
    extra_label_iters = 0

    # ---- generator ---------------------------------------------------------------------------------------------
    def bits(self, seed, samples, stream, idx):
        """[S, len(idx)] uint64."""
        s = np.asarray(samples, dtype=np.int64).astype(U64)[:, None]
        k = np.asarray(idx, dtype=np.int64).astype(U64)[None, :] & U64(0xFFFFFFFF)
        with np.errstate(over="ignore"):
            per_sample = sy_mix(sy_mix(U64(int(seed) & (2 ** 64 - 1)) ^ SEED_MASK) + s)
        return sy_mix(per_sample ^ ((U64(stream) << U64(40)) | k))

    def normal_pairs(self, seed, samples, stream, n):
        """n complex standard-normal pairs per sample: real and imaginary part are the two Box-Muller normals."""
        k = np.arange(n, dtype=np.int64)
        u1 = uniform(self.bits(seed, samples, stream, 2 * k))
        u2 = uniform(self.bits(seed, samples, stream, 2 * k + self.second_normal_offset))
        return np.sqrt(-2.0 * np.log(u1)) * np.exp(1j * TWO_PI * u2)

    # ---- pieces of the recipe that a wrong kernel could get wrong ------------------------------------------------
    def grid_index(self, Nb, Nd):
        """kr(S, conj D): flat index i = i_b Nd + i_d."""
        i = np.arange(Nb * Nd)
        return i // Nd, i % Nd

    def phase(self, ib, idd, f, tau):
        """[S, L, D] cycles of S[i_b] conj(D[i_d]) per target."""
        return ib[None, None, :] * f[:, :, None] - idd[None, None, :] * tau[:, :, None]

    def demod_noise_scale(self, p_noise):
        return np.sqrt(p_noise / 2.0)                               # awgn: p_noise split over the two components

    def snr_draw(self, seed, samples, D, snr_range):
        u = uniform(self.bits(seed, samples, SNR, [0]))             # one draw per sample, [S, 1]
        return snr_range[0] + (snr_range[1] - snr_range[0]) * u

    def energy(self, real_y):
        return (real_y.real ** 2 + real_y.imag ** 2).sum(axis=1, keepdims=True)

    def noise_std(self, y2, snr_w, D):
        return np.sqrt(y2 / (10.0 ** (snr_w / 10.0) * D))

    def label_denominator(self, rho, sum_d):
        return 1.0 + rho * sum_d

    def labels(self, y, b, rho, iters):
        return label_recursion(y, b, rho, iters + self.extra_label_iters, self.label_dtype,
                               self.label_denominator).astype(np.complex128)

    # ---- the recipe ----------------------------------------------------------------------------------------------
    def run(self, samples, Nb, Nd, L, seed, snr_range=(5.0, 25.0), snr_e=7.0, rho=1.0, label_iters=5):
        samples = np.asarray(samples, dtype=np.int64).reshape(-1)
        D = Nb * Nd
        r = {}
        # raw draws
        r["tau"] = 0.1 + 0.8 * uniform(self.bits(seed, samples, TAU, np.arange(L)))
        r["f"] = -0.4 + 0.8 * uniform(self.bits(seed, samples, F, np.arange(L)))
        r["C"] = 0.7 * self.normal_pairs(seed, samples, C, L)
        r["data"] = (self.bits(seed, samples, DATA, np.arange(D)) >> U64(62)).astype(np.int64)
        r["demod_normals"] = self.normal_pairs(seed, samples, DEMOD, D)
        r["snr"] = self.snr_draw(seed, samples, D, snr_range)
        r["noise_normals"] = self.normal_pairs(seed, samples, self.noise_stream, D)
        # scene
        ib, idd = self.grid_index(Nb, Nd)
        r["psi"] = (r["C"][:, :, None] * np.exp(1j * TWO_PI * self.phase(ib, idd, r["f"], r["tau"]))).sum(axis=1)
        r["sig"] = np.exp(1j * (TWO_PI * r["data"] / 4 + np.pi / 4))                                  # pskmod
        p_noise = 1.0 / 10.0 ** (snr_e / 10.0)                                                        # |sig| = 1
        sig_n = r["sig"] + self.demod_noise_scale(p_noise) * r["demod_normals"]                       # awgn
        ang = np.mod(np.angle(sig_n) - np.pi / 4 + np.pi / 4, TWO_PI)                                 # pskdemod
        q = ang * 4 / TWO_PI
        r["margin"] = np.abs(q - np.round(q))
        r["dd"] = np.floor(q).astype(np.int64) % 4
        r["b"] = np.exp(1j * (TWO_PI * r["dd"] / 4 + np.pi / 4))
        r["e"] = r["sig"] - r["b"]
        r["real_y"] = (r["b"] + r["e"]) * r["psi"]
        r["w_std"] = self.noise_std(self.energy(r["real_y"]), r["snr"], D)
        r["y"] = r["real_y"] + r["w_std"] * np.sqrt(0.5) * r["noise_normals"]
        r["sigma"] = np.sqrt((np.abs(r["e"] / r["b"]) ** 2).sum(axis=1)) + 1.0
        r["phi"] = self.labels(r["y"], r["b"], rho, label_iters)
        r["rho"], r["label_iters"] = float(rho), int(label_iters)
        return r


def mirror(samples, Nb, Nd, L, seed, snr_range=(5.0, 25.0), snr_e=7.0, rho=1.0, label_iters=5):
    """Float64 values of everything the device generator draws, derives and writes, for the given sample indices.

    Raw draws: tau, f [S, L]; C [S, L] complex; data [S, D] in 0..3; demod_normals, noise_normals [S, D] complex
    (real / imaginary part = the two normals of a pair); snr [S, 1] in dB.  Derived: psi, sig, b, dd, e, real_y, y, phi
    [S, D]; w_std [S, 1]; sigma [S]; margin [S, D] = distance of ang 4 / (2 pi) from the nearest integer."""
    return SynthMirror().run(samples, Nb, Nd, L, seed, snr_range, snr_e, rho, label_iters)
