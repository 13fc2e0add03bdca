// loss.hip -- the two training losses of the reference's loss.py, one forward and one hand-written backward kernel each
// (admm_net_amd/losses.py; the tensor stand-in there is the definition the tests hold these kernels to).
//   anm   BasicANMLoss, loss.py:6-60.  Per signal with L = L_true[b] targets out of Lmax slots:
//           L = 0:  loss_b = sum_j conf_j^2 over all Lmax slots
//           L >= 1: loss_b = (sum_{j<L} (tau_j - tau_true_j)^2 + (f_j - f_true_j)^2 + 0.1 (conf_j - 1)^2) / L
//         param = sum_b loss_b / B, reg = lambda_reg sum_b ||phi_b||_2 / B, out = {param + reg, param, reg}
//   phi   PhiAlignmentLoss, loss.py:62-98.  amplitude = mean (|phi| - |phi_true|)^2, phase = mean wrap(arg phi - arg phi_true)^2
//         over all B D entries, wrap(d) = ((d + pi) mod 2 pi) - pi with the floored mod (a result in [-pi, pi): +pi maps to
//         -pi), out = {amplitude_weight amplitude + phase_weight phase, amplitude, phase}
// Backwards take g_out[3], the gradients of the three outputs, on the device, and are elementwise.  Conventions (torch's):
// complex gradients are dL/dRe + i dL/dIm; the gradients of ||phi_b||, |phi| and arg phi are exactly 0 where their argument
// is 0; the wrap has derivative 1; the targets get no gradient.
//
// Launch shape and sums: slab_partials.h, as train_small.hip -- one wave per signal, four signals per workgroup, per-signal
// sums by xor-shuffle butterflies, one row of partials per workgroup, added in float64 by ONE workgroup that also forms the
// three outputs.  No atomics: two runs give the same bits.  Every access is a 4-byte or an 8-byte one.
#include "common.h"
#include "batch_sums.h"

namespace admmnet {

constexpr int LA_ANM_COLS = 3;   // sum_b loss_b, sum_b ||phi_b||, signals whose L_true is outside [0, Lmax]
constexpr int LA_PHI_COLS = 2;   // sum (|phi| - |phi_true|)^2, sum wrap(.)^2
constexpr float LA_PI = 3.14159265358979323846f, LA_2PI = 6.28318530717958647692f;

// ((d + pi) mod 2 pi) - pi, the mod floored (the sign of the divisor): fmod's remainder has the sign of the dividend
__device__ __forceinline__ float la_wrap(float d) {
    float m = fmodf(d + LA_PI, LA_2PI);
    if (m < 0.f) m += LA_2PI;
    return m - LA_PI;
}

// L_true[sig] held to [0, Lmax]: the Python layer raises for a value outside, the kernels only keep their own reads in bounds
__device__ __forceinline__ int la_targets(const int64_t *__restrict__ L_true, int64_t sig, int Lmax, bool *outside) {
    const int64_t raw = L_true[sig];
    *outside = raw < 0 || raw > Lmax;
    return raw < 0 ? 0 : (raw > Lmax ? Lmax : (int)raw);
}

// row slices of the finishing column sum (colsum of batch_sums.h): one thread per column and slice
constexpr int LA_ANM_SLICES = 64, LA_PHI_SLICES = 128;
static_assert(LA_ANM_SLICES * LA_ANM_COLS <= TS_THREADS && LA_PHI_SLICES * LA_PHI_COLS <= TS_THREADS, "one thread per column and slice");

// ---- BasicANMLoss ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void la_anm_kernel(int Lmax, int D, int64_t B, const float *__restrict__ tau,
                                                            const float *__restrict__ f, const float *__restrict__ conf,
                                                            const float *__restrict__ tau_true, const float *__restrict__ f_true,
                                                            const int64_t *__restrict__ L_true, const float2 *__restrict__ phi,
                                                            float *__restrict__ norms, float *__restrict__ part) {
    __shared__ float sh[TS_SLAB * LA_ANM_COLS];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float v[LA_ANM_COLS] = {0.f, 0.f, 0.f};
    if (sig < B) {
        bool outside;
        const int L = la_targets(L_true, sig, Lmax, &outside);
        float t = 0.f;
        if (lane < Lmax) {
            const int64_t e = sig * Lmax + lane;
            const float c = conf[e];
            if (L == 0) {
                t = c * c;
            } else if (lane < L) {
                const float dt = tau[e] - tau_true[e], df = f[e] - f_true[e], dc = c - 1.f;
                t = fmaf(0.1f * dc, dc, fmaf(df, df, dt * dt));
            }
        }
        t = wave_sum(t);
        // ||phi_b||: the squares are exact in float64, so the norm the backward divides by is rounded once
        double ss = 0.0;
        for (int i = lane; i < D; i += 64) {
            const float2 p = phi[sig * D + i];
            ss += (double)p.x * (double)p.x + (double)p.y * (double)p.y;
        }
        const float nrm = (float)sqrt(wave_sum(ss));
        if (lane == 0) norms[sig] = nrm;
        v[0] = L > 0 ? t / (float)L : t;
        v[1] = nrm;
        v[2] = outside ? 1.f : 0.f;
    }
    ts_slab_partials<LA_ANM_COLS>(v, sh, part);
}

__global__ __launch_bounds__(TS_THREADS) void la_anm_finish_kernel(int64_t rows, int64_t B, float lambda_reg,
                                                                   const float *__restrict__ part, float *__restrict__ out,
                                                                   int32_t *__restrict__ status) {
    __shared__ double sh[TS_THREADS];
    colsum<LA_ANM_COLS, LA_ANM_SLICES>(rows, part, sh);
    if (threadIdx.x == 0) {
        const double param = sh[0] / (double)B, reg = (double)lambda_reg * sh[1] / (double)B;
        out[0] = (float)(param + reg);
        out[1] = (float)param;
        out[2] = (float)reg;
        status[0] = (int32_t)fmin(sh[2], 2147483647.0);   // a count of ones, exact in float64; saturates
    }
}

// with cp = g_out[0] + g_out[1] (total and param), cr = g_out[0] + g_out[2] (total and reg):
//   L = 0:  g_conf_j = cp 2 conf_j / B for every slot, g_tau = g_f = 0
//   L >= 1: (g_tau, g_f, g_conf)_j = cp 2 / (L B) (tau_j - tau_true_j, f_j - f_true_j, 0.1 (conf_j - 1)) for j < L, 0 for j >= L
//   g_phi_b = cr lambda_reg / B phi_b / ||phi_b||, 0 where the norm is 0
__global__ __launch_bounds__(TS_THREADS) void la_anm_bwd_kernel(int Lmax, int D, int64_t B, const float *__restrict__ g_out,
                                                                const float *__restrict__ tau, const float *__restrict__ f,
                                                                const float *__restrict__ conf, const float *__restrict__ tau_true,
                                                                const float *__restrict__ f_true, const int64_t *__restrict__ L_true,
                                                                const float2 *__restrict__ phi, const float *__restrict__ norms,
                                                                float lambda_reg, float *__restrict__ g_tau, float *__restrict__ g_f,
                                                                float *__restrict__ g_conf, float2 *__restrict__ g_phi) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const int lane = threadIdx.x & 63;
    const float cp = g_out[0] + g_out[1], cr = g_out[0] + g_out[2], fB = (float)B;
    bool outside;
    const int L = la_targets(L_true, sig, Lmax, &outside);
    if (lane < Lmax) {
        const int64_t e = sig * Lmax + lane;
        float gt = 0.f, gf = 0.f, gc = 0.f;
        if (L == 0) {
            gc = cp * 2.f / fB * conf[e];
        } else if (lane < L) {
            const float s = cp * 2.f / ((float)L * fB);
            gt = s * (tau[e] - tau_true[e]);
            gf = s * (f[e] - f_true[e]);
            gc = s * (0.1f * (conf[e] - 1.f));
        }
        g_tau[e] = gt;
        g_f[e] = gf;
        g_conf[e] = gc;
    }
    const float nrm = norms[sig], s = nrm > 0.f ? cr * lambda_reg / fB / nrm : 0.f;
    for (int i = lane; i < D; i += 64) {
        const int64_t e = sig * D + i;
        const float2 p = phi[e];
        g_phi[e] = nrm > 0.f ? make_float2(s * p.x, s * p.y) : make_float2(0.f, 0.f);
    }
}

// ---- PhiAlignmentLoss --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void la_phi_kernel(int D, int64_t B, const float2 *__restrict__ phi,
                                                            const float2 *__restrict__ phi_true, float *__restrict__ part) {
    __shared__ float sh[TS_SLAB * LA_PHI_COLS];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    float a = 0.f, p = 0.f;
    if (sig < B)
        for (int i = threadIdx.x & 63; i < D; i += 64) {
            const float2 z = phi[sig * D + i], t = phi_true[sig * D + i];
            const float da = hypotf(z.x, z.y) - hypotf(t.x, t.y), w = la_wrap(atan2f(z.y, z.x) - atan2f(t.y, t.x));
            a = fmaf(da, da, a);
            p = fmaf(w, w, p);
        }
    const float v[LA_PHI_COLS] = {wave_sum(a), wave_sum(p)};
    ts_slab_partials<LA_PHI_COLS>(v, sh, part);
}

__global__ __launch_bounds__(TS_THREADS) void la_phi_finish_kernel(int64_t rows, double count, float amplitude_weight,
                                                                   float phase_weight, const float *__restrict__ part,
                                                                   float *__restrict__ out) {
    __shared__ double sh[TS_THREADS];
    colsum<LA_PHI_COLS, LA_PHI_SLICES>(rows, part, sh);
    if (threadIdx.x == 0) {
        const double amp = sh[0] / count, ph = sh[1] / count;
        out[0] = (float)((double)amplitude_weight * amp + (double)phase_weight * ph);
        out[1] = (float)amp;
        out[2] = (float)ph;
    }
}

// for phi = x + i y, r = |phi|, w = wrap(arg phi - arg phi_true), ca = (g_out[0] amplitude_weight + g_out[1]) 2 / (B D),
// cp = (g_out[0] phase_weight + g_out[2]) 2 / (B D):
//   g_phi = ca (r - |phi_true|) (x + i y) / r + cp w (-y + i x) / r^2, 0 where phi = 0
__global__ __launch_bounds__(TS_THREADS) void la_phi_bwd_kernel(int D, int64_t B, float inv_count, const float *__restrict__ g_out,
                                                                const float2 *__restrict__ phi, const float2 *__restrict__ phi_true,
                                                                float amplitude_weight, float phase_weight,
                                                                float2 *__restrict__ g_phi) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const float ca = fmaf(g_out[0], amplitude_weight, g_out[1]) * 2.f * inv_count;
    const float cp = fmaf(g_out[0], phase_weight, g_out[2]) * 2.f * inv_count;
    for (int i = threadIdx.x & 63; i < D; i += 64) {
        const int64_t e = sig * D + i;
        const float2 z = phi[e], t = phi_true[e];
        const float r = hypotf(z.x, z.y);
        float2 g = make_float2(0.f, 0.f);
        if (r > 0.f) {
            const float ux = z.x / r, uy = z.y / r;
            const float ga = ca * (r - hypotf(t.x, t.y)), gp = cp * la_wrap(atan2f(z.y, z.x) - atan2f(t.y, t.x)) / r;
            g = make_float2(fmaf(ga, ux, -gp * uy), fmaf(ga, uy, gp * ux));
        }
        g_phi[e] = g;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t loss_partials(int loss, int64_t B) {
    return train_small_rows(B) * (loss == ADMMNET_LOSS_ANM ? LA_ANM_COLS : LA_PHI_COLS);
}

#define LA_LAUNCH(kernel, grid, ...)                                                                \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(TS_THREADS), 0, st, __VA_ARGS__);       \
    ADMM_HIP(hipGetLastError())

int launch_loss_anm(int Lmax, int D, int64_t B, const float *tau, const float *f, const float *conf, const float *tau_true,
                    const float *f_true, const int64_t *L_true, const float2 *phi, float lambda_reg, float *out, float *norms,
                    int32_t *status, float *part, hipStream_t st) {
    const int64_t rows = train_small_rows(B);
    LA_LAUNCH(la_anm_kernel, rows, Lmax, D, B, tau, f, conf, tau_true, f_true, L_true, phi, norms, part);
    LA_LAUNCH(la_anm_finish_kernel, 1, rows, B, lambda_reg, part, out, status);
    return ADMMNET_OK;
}

int launch_loss_anm_bwd(int Lmax, int D, int64_t B, const float *g_out, const float *tau, const float *f, const float *conf,
                        const float *tau_true, const float *f_true, const int64_t *L_true, const float2 *phi, const float *norms,
                        float lambda_reg, float *g_tau, float *g_f, float *g_conf, float2 *g_phi, hipStream_t st) {
    LA_LAUNCH(la_anm_bwd_kernel, train_small_rows(B), Lmax, D, B, g_out, tau, f, conf, tau_true, f_true, L_true, phi, norms,
              lambda_reg, g_tau, g_f, g_conf, g_phi);
    return ADMMNET_OK;
}

int launch_loss_phi(int D, int64_t B, const float2 *phi, const float2 *phi_true, float amplitude_weight, float phase_weight,
                    float *out, float *part, hipStream_t st) {
    const int64_t rows = train_small_rows(B);
    LA_LAUNCH(la_phi_kernel, rows, D, B, phi, phi_true, part);
    LA_LAUNCH(la_phi_finish_kernel, 1, rows, (double)B * (double)D, amplitude_weight, phase_weight, part, out);
    return ADMMNET_OK;
}

int launch_loss_phi_bwd(int D, int64_t B, const float *g_out, const float2 *phi, const float2 *phi_true, float amplitude_weight,
                        float phase_weight, float2 *g_phi, hipStream_t st) {
    LA_LAUNCH(la_phi_bwd_kernel, train_small_rows(B), D, B, (float)(1.0 / ((double)B * (double)D)), g_out, phi, phi_true,
              amplitude_weight, phase_weight, g_phi);
    return ADMMNET_OK;
}

}  // namespace admmnet
