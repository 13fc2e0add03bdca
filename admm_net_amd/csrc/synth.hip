// synth.hip -- batched OFDM-radar scene synthesis + classical-solver labels on the device.
//
// One workgroup per sample restates /root/reference/generate_data.py:133-221 (_generate_single_sample /
// _generate_communication_symbols): L targets tau ~ U(0.1, 0.9), f ~ U(-0.4, 0.4), C ~ N(0, 0.7^2) + j N(0, 0.7^2);
// Psi = kr(S, conj D) C; QPSK symbols, 7 dB demodulation noise, b = mod(demod(.)), e = sig - b; y = diag(b + e) Psi + w
// at snr ~ U(lo, hi) dB; sigma = ||e / b|| + 1; casts to complex64 / float32 (:196-201).  The phi label of
// DatasetGeneratorCreatePhi (:410-463) is admm_for_us(y, b, ...), which as written collapses to the recursion
//   phi_k = W (y / b + rho phi_{k-1}),  W = (diag(1 / |b|^2) + rho 1 1^T)^-1,  stopped at min_iter = 5
// (admm.py:77-79 with the 'rho * np.ones(len)' broadcast) -- O(D) per iteration through
// Sherman-Morrison, evaluated here in float64 like the reference's complex128.
// The reference seeds nothing; the generator here is counter based (splitmix64 of (seed, sample, stream, index)), so a
// batch is reproducible and independent of the launch geometry.  Arithmetic of the scene in float64, as numpy's.
#include "common.h"

namespace admmnet {

constexpr int SY_THREADS = 256;
constexpr int SY_MAXL = 8;
// LDS of one workgroup: three double2 [D] arrays and the 8 block-sum slots (dynamic), the targets and the label
// recursion's sum of d (static).  48 D + 352 bytes <= 160 KiB of a gfx950 CU: D <= SY_MAX_D = 3406 (exactly 160 KiB).
constexpr size_t SY_LDS_LIMIT = 160 * 1024;
constexpr size_t SY_STATIC_LDS = sizeof(double) * (SY_MAXL * 4 + 4);
constexpr size_t sy_dynamic_lds(int64_t D) { return sizeof(double2) * 3 * (size_t)D + sizeof(double) * 8; }
constexpr int64_t SY_MAX_D = (int64_t)((SY_LDS_LIMIT - SY_STATIC_LDS - sizeof(double) * 8) / (sizeof(double2) * 3));
static_assert(sy_dynamic_lds(SY_MAX_D) + SY_STATIC_LDS <= SY_LDS_LIMIT &&
              sy_dynamic_lds(SY_MAX_D + 1) + SY_STATIC_LDS > SY_LDS_LIMIT, "SY_MAX_D is the largest D that fits");

__device__ __forceinline__ unsigned long long sy_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ unsigned long long sy_bits(unsigned long long seed, long long sample, int stream, int idx) {
    return sy_mix(sy_mix(sy_mix(seed ^ 0xA5A5A5A55A5A5A5Aull) + (unsigned long long)sample) ^
                  (((unsigned long long)stream << 40) | (unsigned int)idx));
}
__device__ __forceinline__ double sy_uniform(unsigned long long bits) {   // (0, 1]: the largest draw, 2^53 - 1/2, rounds to 2^53
    return ((double)(bits >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
// two independent standard normals (Box-Muller) from one 64-bit draw + its successor
__device__ __forceinline__ double2 sy_normal2(unsigned long long seed, long long sample, int stream, int idx) {
    const double u1 = sy_uniform(sy_bits(seed, sample, stream, 2 * idx)), u2 = sy_uniform(sy_bits(seed, sample, stream, 2 * idx + 1));
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(2.0 * 3.14159265358979323846 * u2, &s, &c);
    return make_double2(r * c, r * s);
}

enum { SY_TAU = 1, SY_F, SY_C, SY_DATA, SY_DEMOD, SY_SNR, SY_NOISE, SY_COUNT };
constexpr int SY_ATTEMPTS = 32;

// What scenes_kernel draws and reports beyond synth_kernel (admmnet_synth_scenes, include/admmnet.h).
struct SyScene {
    int L_min;                 // the count n is uniform on L_min .. L (= L_max, the stride of tau, f, C)
    double min_sep;            // in resolution cells; 0: no placement loop
    long long *L_true;         // [B] n
    double *snr_db, *noise_var;   // [B] the drawn SNR, w_std^2
    float *ser;                // [B] 100 #{decided symbol != sent symbol} / D
    int *state;                // [B] 1: a target stayed closer than min_sep to an earlier one after SY_ATTEMPTS draws
};

// n = L_min + min(L_max - L_min, floor(u (L_max - L_min + 1))), u in (0, 1]: a pure function of (seed, sample)
__device__ __forceinline__ int sy_count(unsigned long long seed, long long s, int L_min, int L_max) {
    const double u = sy_uniform(sy_bits(seed, s, SY_COUNT, 0));
    return L_min + min(L_max - L_min, (int)floor(u * (double)(L_max - L_min + 1)));
}

// One thread places the n targets of a scene in order: attempt t of target l draws (SY_TAU, SY_F) at index l + SY_MAXL t
// (attempt 0 is synth_kernel's draw) and is accepted when every target j < l lies at least min_sep cells away,
// (Nd wrap(dtau))^2 + (Nb wrap(df))^2 >= min_sep^2 with wrap(d) = d - round(d): the measure of
// match_targets(scale = (Nd, Nb), period = (1, 1)).  The last attempt stays whatever it is; returns 1 if one did.
// At most 8 x 32 attempts against 7 neighbours, done before the first pass over D.
__device__ int sy_place(double (*tgt)[4], int n, int Nb, int Nd, double min_sep, unsigned long long seed, long long s) {
    int unseparated = 0;
    for (int l = 0; l < n; ++l) {
        double ta, fa;
        for (int t = 0;; ++t) {
            ta = 0.1 + 0.8 * sy_uniform(sy_bits(seed, s, SY_TAU, l + SY_MAXL * t));
            fa = -0.4 + 0.8 * sy_uniform(sy_bits(seed, s, SY_F, l + SY_MAXL * t));
            bool apart = true;
            for (int j = 0; j < l && apart; ++j) {
                double dt = ta - tgt[j][0], df = fa - tgt[j][1];
                dt = (double)Nd * (dt - rint(dt));
                df = (double)Nb * (df - rint(df));
                apart = dt * dt + df * df >= min_sep * min_sep;
            }
            if (apart) break;
            if (t == SY_ATTEMPTS - 1) {
                unseparated = 1;
                break;
            }
        }
        tgt[l][0] = ta;
        tgt[l][1] = fa;
    }
    return unseparated;
}

__global__ __launch_bounds__(SY_THREADS) void synth_kernel(int Nb, int Nd, int L, unsigned long long seed, double snr_lo,
                                                           double snr_hi, double snr_e, double rho, int label_iters,
                                                           float2 *__restrict__ y_out, float2 *__restrict__ b_out,
                                                           float *__restrict__ sigma_out, float *__restrict__ tau_out,
                                                           float *__restrict__ f_out, float2 *__restrict__ C_out,
                                                           float2 *__restrict__ phi_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = Nb * Nd;
    double2 *yv = reinterpret_cast<double2 *>(smem);     // [D] y (float64)
    double2 *bv = yv + D;                                // [D] b
    double2 *ph = bv + D;                                // [D] label recursion
    double *red = reinterpret_cast<double *>(ph + D);    // [8]
    __shared__ double tgt[SY_MAXL][4];                   // tau, f, Re C, Im C
    __shared__ double sdw[4];                            // label recursion: sum of d per wave  (both in SY_STATIC_LDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = blockIdx.x;
    if (tid < L) {
        tgt[tid][0] = 0.1 + 0.8 * sy_uniform(sy_bits(seed, s, SY_TAU, tid));     // generate_data.py:30,138
        tgt[tid][1] = -0.4 + 0.8 * sy_uniform(sy_bits(seed, s, SY_F, tid));      // :31,139
        const double2 g = sy_normal2(seed, s, SY_C, tid);                         // :142-144
        tgt[tid][2] = 0.7 * g.x;
        tgt[tid][3] = 0.7 * g.y;
        tau_out[s * L + tid] = (float)tgt[tid][0];
        f_out[s * L + tid] = (float)tgt[tid][1];
        C_out[s * L + tid] = make_float2((float)tgt[tid][2], (float)tgt[tid][3]);
    }
    __syncthreads();
    const double p_noise = 1.0 / pow(10.0, snr_e / 10.0);   // |sig| = 1: awgn(sig, snr_e), mathUtils.py:93-111
    double acc_y2 = 0.0, acc_eb = 0.0;
    for (int i = tid; i < D; i += SY_THREADS) {
        const int ib = i / Nd, id = i - ib * Nd;           // kr(S, conj D): index = i_b * Nd + i_d
        double pr = 0.0, pi = 0.0;
        for (int l = 0; l < L; ++l) {
            double sn, cs;
            sincos(2.0 * 3.14159265358979323846 * ((double)ib * tgt[l][1] - (double)id * tgt[l][0]), &sn, &cs);
            pr += tgt[l][2] * cs - tgt[l][3] * sn;
            pi += tgt[l][2] * sn + tgt[l][3] * cs;
        }
        // QPSK: sig = exp(j (2 pi data / 4 + pi / 4)); demodulate the noisy symbol; b = mod(demod)   (:205-221)
        const int data = (int)(sy_bits(seed, s, SY_DATA, i) >> 62);
        double sgs, sgc;
        sincos(2.0 * 3.14159265358979323846 * data / 4.0 + 3.14159265358979323846 / 4.0, &sgs, &sgc);
        const double2 nz = sy_normal2(seed, s, SY_DEMOD, i);
        const double nr = sgc + sqrt(p_noise / 2.0) * nz.x, ni = sgs + sqrt(p_noise / 2.0) * nz.y;
        double ang = atan2(ni, nr) - 3.14159265358979323846 / 4.0;
        ang = fmod(ang + 3.14159265358979323846 / 4.0, 2.0 * 3.14159265358979323846);
        if (ang < 0.0) ang += 2.0 * 3.14159265358979323846;                       // np.mod: result in [0, 2 pi)
        const int dd = ((int)floor(ang * 4.0 / (2.0 * 3.14159265358979323846))) & 3;
        double bs, bc;
        sincos(2.0 * 3.14159265358979323846 * dd / 4.0 + 3.14159265358979323846 / 4.0, &bs, &bc);
        const double er = sgc - bc, ei = sgs - bs;
        // real_y = (b + e) psi = sig psi
        const double yr = sgc * pr - sgs * pi, yi = sgc * pi + sgs * pr;
        yv[i] = make_double2(yr, yi);
        bv[i] = make_double2(bc, bs);
        acc_y2 += yr * yr + yi * yi;
        acc_eb += er * er + ei * ei;                       // |e / b|^2 = |e|^2 (|b| = 1)
    }
    // block sums
    for (int o = 32; o > 0; o >>= 1) {
        acc_y2 += __shfl_xor(acc_y2, o, 64);
        acc_eb += __shfl_xor(acc_eb, o, 64);
    }
    if (lane == 0) {
        red[wave] = acc_y2;
        red[4 + wave] = acc_eb;
    }
    __syncthreads();
    const double y2 = (red[0] + red[1]) + (red[2] + red[3]), eb = (red[4] + red[5]) + (red[6] + red[7]);
    const double snr_w = snr_lo + (snr_hi - snr_lo) * sy_uniform(sy_bits(seed, s, SY_SNR, 0));   // :164
    const double w_std = sqrt(y2 / (pow(10.0, snr_w / 10.0) * (double)D));                        // :166-169
    for (int i = tid; i < D; i += SY_THREADS) {
        const double2 nz = sy_normal2(seed, s, SY_NOISE, i);
        double2 v = yv[i];
        v.x += w_std * 0.70710678118654752440 * nz.x;
        v.y += w_std * 0.70710678118654752440 * nz.y;
        yv[i] = v;
        y_out[s * D + i] = make_float2((float)v.x, (float)v.y);
        b_out[s * D + i] = make_float2((float)bv[i].x, (float)bv[i].y);
        ph[i] = make_double2(0.0, 0.0);
    }
    if (tid == 0) sigma_out[s] = (float)(sqrt(eb) + 1.0);                                          // :171
    if (phi_out == nullptr) return;   // (uniform)
    // ---- label: phi_k = W (y / b + rho phi_{k-1}),  W r = d r - d (rho sum(d r)) / (1 + rho sum d),  d = |b|^2
    __syncthreads();
    for (int it = 0; it < label_iters; ++it) {
        double sr = 0.0, si = 0.0, sd = 0.0;
        for (int i = tid; i < D; i += SY_THREADS) {
            const double2 bb = bv[i], yy = yv[i], pp = ph[i];
            const double d = bb.x * bb.x + bb.y * bb.y;
            // y / b = y conj(b) / |b|^2
            const double qr = (yy.x * bb.x + yy.y * bb.y) / d + rho * pp.x, qi = (yy.y * bb.x - yy.x * bb.y) / d + rho * pp.y;
            sr += d * qr;
            si += d * qi;
            sd += d;
        }
        for (int o = 32; o > 0; o >>= 1) {
            sr += __shfl_xor(sr, o, 64);
            si += __shfl_xor(si, o, 64);
            sd += __shfl_xor(sd, o, 64);
        }
        __syncthreads();              // the previous iteration's readers of red are done
        if (lane == 0) {
            red[wave] = sr;
            red[4 + wave] = si;
        }
        if (lane == 0) sdw[wave] = sd;
        __syncthreads();
        const double Sr = (red[0] + red[1]) + (red[2] + red[3]), Si = (red[4] + red[5]) + (red[6] + red[7]);
        const double Sd = (sdw[0] + sdw[1]) + (sdw[2] + sdw[3]);
        const double kr = rho * Sr / (1.0 + rho * Sd), ki = rho * Si / (1.0 + rho * Sd);
        for (int i = tid; i < D; i += SY_THREADS) {
            const double2 bb = bv[i], yy = yv[i], pp = ph[i];
            const double d = bb.x * bb.x + bb.y * bb.y;
            const double qr = (yy.x * bb.x + yy.y * bb.y) / d + rho * pp.x, qi = (yy.y * bb.x - yy.x * bb.y) / d + rho * pp.y;
            ph[i] = make_double2(d * qr - d * kr, d * qi - d * ki);
        }
        __syncthreads();
    }
    for (int i = tid; i < D; i += SY_THREADS) phi_out[s * D + i] = make_float2((float)ph[i].x, (float)ph[i].y);
}

// synth_kernel with n = L_min .. L targets per scene (L = L_max, the stride of tau, f, C), kept min_sep apart, and the scene's
// L_true, snr_db, noise_var, ser and state written beside it.  The recipe is synth_kernel's line for line -- with L_min = L and
// min_sep = 0 the shared outputs have its bits -- restated here rather than shared, because instantiating both kernels from one
// body changes synth_kernel's code object, which bench.py's inputs come from.  Same geometry, same LDS to the byte
// (SY_STATIC_LDS + sy_dynamic_lds(D)): the count needs none, the symbol-error count goes through sdw.
__global__ __launch_bounds__(SY_THREADS) void scenes_kernel(int Nb, int Nd, int L, unsigned long long seed, double snr_lo,
                                                            double snr_hi, double snr_e, double rho, int label_iters,
                                                            float2 *__restrict__ y_out, float2 *__restrict__ b_out,
                                                            float *__restrict__ sigma_out, float *__restrict__ tau_out,
                                                            float *__restrict__ f_out, float2 *__restrict__ C_out,
                                                            float2 *__restrict__ phi_out, SyScene sc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = Nb * Nd;
    double2 *yv = reinterpret_cast<double2 *>(smem);     // [D] y (float64)
    double2 *bv = yv + D;                                // [D] b
    double2 *ph = bv + D;                                // [D] label recursion
    double *red = reinterpret_cast<double *>(ph + D);    // [8]
    __shared__ double tgt[SY_MAXL][4];                   // tau, f, Re C, Im C
    __shared__ double sdw[4];                            // label recursion: sum of d per wave  (both in SY_STATIC_LDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = blockIdx.x;
    const int n = sy_count(seed, s, sc.L_min, L);                // every thread evaluates the count itself
    int unseparated = 0;                                          // (thread 0's)
    const bool placed = sc.min_sep > 0.0;
    if (tid < L) {   // C as synth_kernel's, whatever the attempt; slots past n are exact zeros (the reference's padding)
        const bool on = tid < n;
        const double2 g = on ? sy_normal2(seed, s, SY_C, tid) : make_double2(0.0, 0.0);
        tgt[tid][2] = 0.7 * g.x;
        tgt[tid][3] = 0.7 * g.y;
        if (!on || !placed) {
            tgt[tid][0] = on ? 0.1 + 0.8 * sy_uniform(sy_bits(seed, s, SY_TAU, tid)) : 0.0;
            tgt[tid][1] = on ? -0.4 + 0.8 * sy_uniform(sy_bits(seed, s, SY_F, tid)) : 0.0;
        }
    }
    if (placed && tid == 0) unseparated = sy_place(tgt, n, Nb, Nd, sc.min_sep, seed, s);
    __syncthreads();
    if (tid < L) {
        tau_out[s * L + tid] = (float)tgt[tid][0];
        f_out[s * L + tid] = (float)tgt[tid][1];
        C_out[s * L + tid] = make_float2((float)tgt[tid][2], (float)tgt[tid][3]);
    }
    const double p_noise = 1.0 / pow(10.0, snr_e / 10.0);   // |sig| = 1: awgn(sig, snr_e), mathUtils.py:93-111
    double acc_y2 = 0.0, acc_eb = 0.0;
    int errs = 0;                                           // symbols decided wrongly
    for (int i = tid; i < D; i += SY_THREADS) {
        const int ib = i / Nd, id = i - ib * Nd;           // kr(S, conj D): index = i_b * Nd + i_d
        double pr = 0.0, pi = 0.0;
        for (int l = 0; l < n; ++l) {
            double sn, cs;
            sincos(2.0 * 3.14159265358979323846 * ((double)ib * tgt[l][1] - (double)id * tgt[l][0]), &sn, &cs);
            pr += tgt[l][2] * cs - tgt[l][3] * sn;
            pi += tgt[l][2] * sn + tgt[l][3] * cs;
        }
        // QPSK: sig = exp(j (2 pi data / 4 + pi / 4)); demodulate the noisy symbol; b = mod(demod)   (:205-221)
        const int data = (int)(sy_bits(seed, s, SY_DATA, i) >> 62);
        double sgs, sgc;
        sincos(2.0 * 3.14159265358979323846 * data / 4.0 + 3.14159265358979323846 / 4.0, &sgs, &sgc);
        const double2 nz = sy_normal2(seed, s, SY_DEMOD, i);
        const double nr = sgc + sqrt(p_noise / 2.0) * nz.x, ni = sgs + sqrt(p_noise / 2.0) * nz.y;
        double ang = atan2(ni, nr) - 3.14159265358979323846 / 4.0;
        ang = fmod(ang + 3.14159265358979323846 / 4.0, 2.0 * 3.14159265358979323846);
        if (ang < 0.0) ang += 2.0 * 3.14159265358979323846;                       // np.mod: result in [0, 2 pi)
        const int dd = ((int)floor(ang * 4.0 / (2.0 * 3.14159265358979323846))) & 3;
        double bs, bc;
        sincos(2.0 * 3.14159265358979323846 * dd / 4.0 + 3.14159265358979323846 / 4.0, &bs, &bc);
        const double er = sgc - bc, ei = sgs - bs;
        // real_y = (b + e) psi = sig psi
        const double yr = sgc * pr - sgs * pi, yi = sgc * pi + sgs * pr;
        yv[i] = make_double2(yr, yi);
        bv[i] = make_double2(bc, bs);
        acc_y2 += yr * yr + yi * yi;
        acc_eb += er * er + ei * ei;                       // |e / b|^2 = |e|^2 (|b| = 1)
        errs += dd != data;
    }
    // block sums
    for (int o = 32; o > 0; o >>= 1) {
        acc_y2 += __shfl_xor(acc_y2, o, 64);
        acc_eb += __shfl_xor(acc_eb, o, 64);
    }
    if (lane == 0) {
        red[wave] = acc_y2;
        red[4 + wave] = acc_eb;
    }
    for (int o = 32; o > 0; o >>= 1) errs += __shfl_xor(errs, o, 64);
    if (lane == 0) sdw[wave] = (double)errs;   // an exact count in a fixed order, through sdw: idle until the label recursion
    __syncthreads();
    const double y2 = (red[0] + red[1]) + (red[2] + red[3]), eb = (red[4] + red[5]) + (red[6] + red[7]);
    const double snr_w = snr_lo + (snr_hi - snr_lo) * sy_uniform(sy_bits(seed, s, SY_SNR, 0));   // :164
    const double w_std = sqrt(y2 / (pow(10.0, snr_w / 10.0) * (double)D));                        // :166-169
    for (int i = tid; i < D; i += SY_THREADS) {
        const double2 nz = sy_normal2(seed, s, SY_NOISE, i);
        double2 v = yv[i];
        v.x += w_std * 0.70710678118654752440 * nz.x;
        v.y += w_std * 0.70710678118654752440 * nz.y;
        yv[i] = v;
        y_out[s * D + i] = make_float2((float)v.x, (float)v.y);
        b_out[s * D + i] = make_float2((float)bv[i].x, (float)bv[i].y);
        ph[i] = make_double2(0.0, 0.0);
    }
    if (tid == 0) sigma_out[s] = (float)(sqrt(eb) + 1.0);                                          // :171
    if (tid == 0) {
        sc.L_true[s] = n;
        sc.snr_db[s] = snr_w;
        sc.noise_var[s] = w_std * w_std;
        sc.ser[s] = (float)(100.0 * ((sdw[0] + sdw[1]) + (sdw[2] + sdw[3])) / (double)D);   // generate_data.py:219
        sc.state[s] = unseparated;
    }
    if (phi_out == nullptr) return;   // (uniform)
    // ---- label: phi_k = W (y / b + rho phi_{k-1}),  W r = d r - d (rho sum(d r)) / (1 + rho sum d),  d = |b|^2
    __syncthreads();
    for (int it = 0; it < label_iters; ++it) {
        double sr = 0.0, si = 0.0, sd = 0.0;
        for (int i = tid; i < D; i += SY_THREADS) {
            const double2 bb = bv[i], yy = yv[i], pp = ph[i];
            const double d = bb.x * bb.x + bb.y * bb.y;
            // y / b = y conj(b) / |b|^2
            const double qr = (yy.x * bb.x + yy.y * bb.y) / d + rho * pp.x, qi = (yy.y * bb.x - yy.x * bb.y) / d + rho * pp.y;
            sr += d * qr;
            si += d * qi;
            sd += d;
        }
        for (int o = 32; o > 0; o >>= 1) {
            sr += __shfl_xor(sr, o, 64);
            si += __shfl_xor(si, o, 64);
            sd += __shfl_xor(sd, o, 64);
        }
        __syncthreads();              // the previous iteration's readers of red are done
        if (lane == 0) {
            red[wave] = sr;
            red[4 + wave] = si;
        }
        if (lane == 0) sdw[wave] = sd;
        __syncthreads();
        const double Sr = (red[0] + red[1]) + (red[2] + red[3]), Si = (red[4] + red[5]) + (red[6] + red[7]);
        const double Sd = (sdw[0] + sdw[1]) + (sdw[2] + sdw[3]);
        const double kr = rho * Sr / (1.0 + rho * Sd), ki = rho * Si / (1.0 + rho * Sd);
        for (int i = tid; i < D; i += SY_THREADS) {
            const double2 bb = bv[i], yy = yv[i], pp = ph[i];
            const double d = bb.x * bb.x + bb.y * bb.y;
            const double qr = (yy.x * bb.x + yy.y * bb.y) / d + rho * pp.x, qi = (yy.y * bb.x - yy.x * bb.y) / d + rho * pp.y;
            ph[i] = make_double2(d * qr - d * kr, d * qi - d * ki);
        }
        __syncthreads();
    }
    for (int i = tid; i < D; i += SY_THREADS) phi_out[s * D + i] = make_float2((float)ph[i].x, (float)ph[i].y);
}


int64_t synth_max_cells() { return SY_MAX_D; }

int launch_synth(int64_t B, int Nb, int Nd, int L, unsigned long long seed, double snr_lo, double snr_hi, double snr_e,
                 double rho, int label_iters, float2 *y, float2 *b, float *sigma, float *tau, float *f, float2 *C,
                 float2 *phi_label, hipStream_t st) {
    if (B <= 0) return ADMMNET_OK;
    const int64_t D64 = (int64_t)Nb * Nd;
    if (D64 > SY_MAX_D) {
        set_error("synth_batch: Nb * Nd = %lld needs %lld bytes of LDS, the device has %lld (Nb * Nd <= %lld)", (long long)D64,
                  (long long)(sy_dynamic_lds(D64) + SY_STATIC_LDS), (long long)SY_LDS_LIMIT, (long long)SY_MAX_D);
        return ADMMNET_E_ARG;
    }
    const size_t lds = sy_dynamic_lds(D64);
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(synth_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)B), dim3(SY_THREADS), lds, st, Nb, Nd, L, seed, snr_lo, snr_hi, snr_e,
                       rho, label_iters, y, b, sigma, tau, f, C, phi_label);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_synth_scenes(int64_t B, int Nb, int Nd, int L_min, int L_max, double min_sep, unsigned long long seed, double snr_lo,
                        double snr_hi, double snr_e, double rho, int label_iters, float2 *y, float2 *b, float *sigma,
                        float *tau, float *f, float2 *C, float2 *phi_label, int64_t *L_true, double *snr_db,
                        double *noise_var, float *ser, int32_t *state, hipStream_t st) {
    const int64_t D64 = (int64_t)Nb * Nd;
    if (D64 > SY_MAX_D) {
        set_error("synth_scenes: Nb * Nd = %lld needs %lld bytes of LDS, the device has %lld (Nb * Nd <= %lld)", (long long)D64,
                  (long long)(sy_dynamic_lds(D64) + SY_STATIC_LDS), (long long)SY_LDS_LIMIT, (long long)SY_MAX_D);
        return ADMMNET_E_ARG;
    }
    const size_t lds = sy_dynamic_lds(D64);
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scenes_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const SyScene sc{L_min, min_sep, reinterpret_cast<long long *>(L_true), snr_db, noise_var, ser, state};
    hipLaunchKernelGGL(scenes_kernel, dim3((unsigned)B), dim3(SY_THREADS), lds, st, Nb, Nd, L_max, seed, snr_lo, snr_hi, snr_e,
                       rho, label_iters, y, b, sigma, tau, f, C, phi_label, sc);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
