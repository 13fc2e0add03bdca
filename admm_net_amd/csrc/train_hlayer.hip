// train_hlayer.hip -- the H layer of one TRAINING step with its correction_net inside, one forward and one hand-written backward
// kernel, for train_route = "native" of admm_net_amd/training.py.  It replaces the hinput -> correction_net -> hproject chain
// of train_small.hip (where correction_net is a framework module call) and follows that file's conventions: the kernels read the
// RAW parameters from device memory and the backward returns raw-parameter gradients.
//   forward   t = g_dg + z_dg / (softplus(rho_raw) + eps)                                                            admm_net.py:150-152
//             a1 = relu(W1 t + b1) (W1 [64][D]), m = tanh(W2 a1 + b2) (W2 [D][64]), tc = t + 0.1 m                   :128-133, 156-158
//             c = A max|tc| + sum tc, A = 2 sqrt(D) sigma + sigma^2, s = min(sigmoid(pw) / (c + eps), 1), h = tc s   :160-194
//             t, a1 and m are written out: the backward reads them instead of evaluating the two products again.
//   backward  g_tc from g_h as ts_hproject_bwd_kernel has it (lowest index among ties of max|tc|, the clamp passes the gradient
//             where its argument is <= 1, sigmoid' = e / (1 + e)^2), delta2 = 0.1 g_tc (1 - m^2), g_a1 = W2^T delta2,
//             delta1 = g_a1 [a1 > 0] (relu'(0) = 0), g_t = g_tc + W1^T delta1, g_gdg = g_t, g_zdg = g_t / den,
//             g_rho = -softplus'(rho_raw) / den^2 sum g_t z_dg, g_pw as in hproject.  delta1 [B][64] and delta2 [B][D] are written;
//             gW1 = sum_b delta1_b (x) t_b, gb1 = sum_b delta1_b, gW2 = sum_b delta2_b (x) a1_b, gb2 = sum_b delta2_b
//             come from the batch-reduced product below.
// Launch shape: train_small.hip's, one wave per signal (D <= 256 is four elements per lane), four signals per 256-thread
// workgroup.  The four waves of a workgroup read the same weights, which stay in the L1 / L2; each wave keeps its own vectors
// (t, a1, delta1, delta2) in LDS, where every lane reads the same word at a time (a broadcast, no bank conflict).  In the
// forward a lane owns an OUTPUT and streams its weight row; in the backward the transposed products make the lane index the
// contiguous one, so those loads are coalesced.  Dot products run in four interleaved partial sums.
//
// The weight gradients are two batch-reduced products with their biases as appended columns of ones (bp_kernel of
// batch_product.h over a by-value table of two descriptors); th_sum_kernel adds their slabs and the {g_rho, g_pw} rows.
#include "common.h"
#include "batch_product.h"
#include "slab_partials.h"
#include "train_math.h"

namespace admmnet {

constexpr int TH_PER_LANE = kMaxD / 64;    // elements of one [D] row a lane holds
constexpr int TH_ROWPAR = 2;               // g_rho, g_pw: the partials a workgroup of th_hlayer_bwd_kernel leaves
static_assert(TH_PER_LANE * 64 == kMaxD && kHid == 64, "one wave covers a row of D and the hidden layer");

// One wave's view of the projection: c and the place of max|tc| (lowest index among ties); tc is zero past D
struct ThProj {
    float A, c;
    int imax;
};
__device__ __forceinline__ ThProj th_project(int D, const float (&tc)[TH_PER_LANE], float sigma) {
    ThProj p;
    const int lane = threadIdx.x & 63;
    float mx = -1.f, sm = 0.f;
    int im = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        sm += tc[k];
        if (i < D && fabsf(tc[k]) > mx) mx = fabsf(tc[k]), im = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float omx = __shfl_xor(mx, o, 64);
        const int oim = __shfl_xor(im, o, 64);
        if (omx > mx || (omx == mx && oim < im)) mx = omx, im = oim;
    }
    sm = wave_sum(sm);
    p.A = 2.f * sqrtf((float)D) * sigma + sigma * sigma;
    p.c = p.A * mx + sm;
    p.imax = im;
    return p;
}

__global__ __launch_bounds__(TS_THREADS) void th_hlayer_kernel(int D, int64_t B, const float *__restrict__ gdg,
                                                               const float *__restrict__ zdg, const float *__restrict__ sigma,
                                                               const float *__restrict__ rho_raw, const float *__restrict__ pw_raw,
                                                               const float *__restrict__ W1, const float *__restrict__ b1,
                                                               const float *__restrict__ W2, const float *__restrict__ b2,
                                                               float *__restrict__ h, float *__restrict__ t_out,
                                                               float *__restrict__ a1_out, float *__restrict__ m_out) {
    __shared__ float st[TS_SLAB][kMaxD];
    __shared__ float sa[TS_SLAB][kHid];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + wave;
    const bool live = sig < B;
    const float den = softplus_f(rho_raw[0]) + kEpsRef;
    float t[TH_PER_LANE];
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        const bool on = live && i < D;
        t[k] = on ? gdg[sig * D + i] + zdg[sig * D + i] / den : 0.f;
        st[wave][i] = t[k];
        if (on) t_out[sig * D + i] = t[k];
    }
    __syncthreads();
    const float a = fmaxf(dot4(W1 + (int64_t)lane * D, 1, st[wave], D) + b1[lane], 0.f);
    sa[wave][lane] = a;
    if (live) a1_out[sig * kHid + lane] = a;
    __syncthreads();
    float tc[TH_PER_LANE];
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        tc[k] = 0.f;
        if (live && i < D) {
            const float m = tanhf(dot4(W2 + (int64_t)i * kHid, 1, sa[wave], kHid) + b2[i]);
            m_out[sig * D + i] = m;
            tc[k] = t[k] + 0.1f * m;
        }
    }
    const ThProj p = th_project(D, tc, live ? sigma[sig] : 0.f);
    const float s = fminf(sigmoid_f(pw_raw[0]) / (p.c + kEpsRef), 1.f);
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        if (live && i < D) h[sig * D + i] = tc[k] * s;
    }
}

// part: one row {g_rho, g_pw} per workgroup
__global__ __launch_bounds__(TS_THREADS) void th_hlayer_bwd_kernel(int D, int64_t B, const float *__restrict__ gh,
                                                                   const float *__restrict__ zdg, const float *__restrict__ sigma,
                                                                   const float *__restrict__ rho_raw, const float *__restrict__ pw_raw,
                                                                   const float *__restrict__ W1, const float *__restrict__ W2,
                                                                   const float *__restrict__ t, const float *__restrict__ a1,
                                                                   const float *__restrict__ m, float *__restrict__ ggdg,
                                                                   float *__restrict__ gzdg, float *__restrict__ d1_out,
                                                                   float *__restrict__ d2_out, float *__restrict__ part) {
    __shared__ float sd2[TS_SLAB][kMaxD];
    __shared__ float sd1[TS_SLAB][kHid];
    __shared__ float sh[TS_SLAB * TH_ROWPAR];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + wave;
    const bool live = sig < B;
    const float raw = rho_raw[0], den = softplus_f(raw) + kEpsRef;
    float tc[TH_PER_LANE], mm[TH_PER_LANE], u[TH_PER_LANE], gtc[TH_PER_LANE], gs = 0.f;
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        const bool on = live && i < D;
        mm[k] = on ? m[sig * D + i] : 0.f;
        tc[k] = on ? t[sig * D + i] + 0.1f * mm[k] : 0.f;
        u[k] = on ? gh[sig * D + i] : 0.f;
        gs = fmaf(u[k], tc[k], gs);
    }
    const ThProj p = th_project(D, tc, live ? sigma[sig] : 0.f);
    gs = wave_sum(gs);
    const float sp = sigmoid_f(pw_raw[0]), cden = p.c + kEpsRef, q = sp / cden;
    const bool open = q <= 1.f;
    const float s = open ? q : 1.f, gc = open ? -gs * sp / (cden * cden) : 0.f;
    const float gpw = (live && open) ? gs * dsigmoid_f(pw_raw[0]) / cden : 0.f;
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        const bool on = live && i < D;
        const float sgn = tc[k] > 0.f ? 1.f : (tc[k] < 0.f ? -1.f : 0.f);
        gtc[k] = on ? fmaf(u[k], s, gc * (1.f + (i == p.imax ? p.A * sgn : 0.f))) : 0.f;
        const float d2 = 0.1f * gtc[k] * (1.f - mm[k] * mm[k]);
        sd2[wave][i] = d2;
        if (on) d2_out[sig * D + i] = d2;
    }
    __syncthreads();
    float d1 = dot4(W2 + lane, kHid, sd2[wave], D);
    d1 = (live && a1[sig * kHid + lane] > 0.f) ? d1 : 0.f;
    sd1[wave][lane] = d1;
    if (live) d1_out[sig * kHid + lane] = d1;
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        if (live && i < D) {
            const float gt = gtc[k] + dot4(W1 + i, D, sd1[wave], kHid);
            ggdg[sig * D + i] = gt;
            gzdg[sig * D + i] = gt / den;
            acc = fmaf(gt, zdg[sig * D + i], acc);
        }
    }
    const float v[TH_ROWPAR] = {-wave_sum(acc) * dsoftplus_f(raw) / (den * den), gpw};
    ts_slab_partials<TH_ROWPAR>(v, sh, part);
}

// ---- the parameter gradients -------------------------------------------------------------------------------------------------
struct ThTable {   // gW1 with gb1, gW2 with gb2
    BpDesc d[2];
    __host__ __device__ int count() const { return 2; }
    __host__ __device__ BpDesc desc(int i) const { return d[i]; }
};

// workgroups 1 ..: out[npar + e] = the slabs' sums of the products (bp_sum_regions); workgroup 0 adds the `rows` rows of the npar
// (<= 4) per-workgroup partials, one wave per column: lane l the rows l, l + 64, ..., then a butterfly
__global__ __launch_bounds__(TS_THREADS) void th_sum_kernel(int npar, int64_t rows, const float *__restrict__ rowpart, BpRegion r,
                                                            float *__restrict__ out) {
    if (blockIdx.x == 0) {
        const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (c >= npar) return;
        double a = 0.0;
        for (int64_t i = lane; i < rows; i += 64) a += (double)rowpart[i * npar + c];
        a = wave_sum(a);
        if (lane == 0) out[c] = (float)a;
        return;
    }
    bp_sum_regions((int64_t)(blockIdx.x - 1) * TS_THREADS + threadIdx.x, r, BpRegion{nullptr, 0, 0, 0, 0, 0}, out);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static int64_t hlayer_total(int D) { return (int64_t)2 * kHid * D + kHid + D; }   // gW1, gb1, gW2, gb2

// floats: the {g_rho, g_pw} rows of the slabs of four signals, then [batch slabs][gW1, gb1, gW2, gb2]
int64_t train_hlayer_workspace_floats(int D, int64_t B) { return TH_ROWPAR * train_small_rows(B) + bp_slabs(B) * hlayer_total(D); }

int launch_train_hlayer(int D, int64_t B, const float *gdg, const float *zdg, const float *sigma, const float *rho_raw,
                        const float *pw_raw, const float *W1, const float *b1, const float *W2, const float *b2, float *h, float *t,
                        float *a1, float *m, hipStream_t st) {
    hipLaunchKernelGGL(th_hlayer_kernel, dim3((unsigned)train_small_rows(B)), dim3(TS_THREADS), 0, st, D, B, gdg, zdg, sigma,
                       rho_raw, pw_raw, W1, b1, W2, b2, h, t, a1, m);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// gpar: g_rho, g_pw, gW1 [64][D], gb1 [64], gW2 [D][64], gb2 [D]
int launch_train_hlayer_bwd(int D, int64_t B, const float *gh, const float *zdg, const float *sigma, const float *rho_raw,
                            const float *pw_raw, const float *W1, const float *W2, const float *t, const float *a1, const float *m,
                            float *ggdg, float *gzdg, float *d1, float *d2, float *gpar, float *work, hipStream_t st) {
    const int64_t rows = train_small_rows(B), slabs = bp_slabs(B), total = hlayer_total(D);
    float *rowpart = work, *part = work + TH_ROWPAR * rows;
    hipLaunchKernelGGL(th_hlayer_bwd_kernel, dim3((unsigned)rows), dim3(TS_THREADS), 0, st, D, B, gh, zdg, sigma, rho_raw, pw_raw,
                       W1, W2, t, a1, m, ggdg, gzdg, d1, d2, rowpart);
    ADMM_HIP(hipGetLastError());
    const int64_t oW2 = (int64_t)kHid * D + kHid;
    ThTable tab;
    tab.d[0] = {d1, t, kHid, D, kHid, D, 1, D, B, 0, (int64_t)kHid * D, part, total};          // gW1 [64][D], gb1
    tab.d[1] = {d2, a1, D, kHid, D, kHid, 1, kHid, B, oW2, oW2 + (int64_t)D * kHid, part, total};   // gW2 [D][64], gb2
    hipLaunchKernelGGL(bp_kernel<ThTable>, dim3((unsigned)bp_tiles(tab), (unsigned)slabs), dim3(64), 0, st, tab);
    ADMM_HIP(hipGetLastError());
    const BpRegion r{part, total, slabs, TH_ROWPAR, total, 0};   // the products follow g_rho, g_pw in gpar
    hipLaunchKernelGGL(th_sum_kernel, dim3((unsigned)(1 + (total + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, TH_ROWPAR,
                       rows, rowpart, r, gpar);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
