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
// Batch-reduced product  C[m][n] = sum_b A[b][m] Bm[b][n]  (bp_kernel): the batch index is the k dimension of
// v_mfma_f32_32x32x2_f32, whose A operand is A[i = lane & 31][k = lane >> 5] and B operand B[k = lane >> 5][j = lane & 31]: with
// the batch as k both are read straight from the [B][M] / [B][N] tensors, 128 contiguous bytes per lane half, no LDS.  One
// grouped launch over a descriptor table handed over by value: one wave per (32 x 32 tile, slab of BP_SLAB signals).  Rows past
// B (B odd, B = 1, a ragged last slab) and rows / columns past M / N enter as zeros.  Bm = nullptr stands for a column of ones
// (N = 1): the column sums for the biases.  Within a slab the sum runs in float32 in the matrix core's fixed k order; bp_sum_kernel
// adds the slabs in ascending order in float64.  The slab length is a constant, so neither the grid nor the run changes a bit.
#include "common.h"
#include "slab_partials.h"

namespace admmnet {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int TH_PER_LANE = kMaxD / 64;    // elements of one [D] row a lane holds
constexpr int BP_SLAB = 128;               // signals summed in float32 by one wave of bp_kernel
constexpr int BP_MAX_DESC = 4;
constexpr int BP_UNROLL = 8;              // k steps (pairs of signals) whose operands bp_kernel loads ahead of their MFMAs
static_assert(TH_PER_LANE * 64 == kMaxD && kHid == 64, "one wave covers a row of D and the hidden layer");

__device__ __forceinline__ float th_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float th_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float th_dsoftplus(float x) { return x > 20.f ? 1.f : th_sigmoid(x); }
__device__ __forceinline__ float th_dsigmoid(float x) {
    const float e = expf(-fabsf(x)), d = 1.f + e;
    return e / (d * d);
}

// sum_{i < len} w[i * stride] * x[i], x in LDS, four interleaved partial sums
__device__ __forceinline__ float th_dot(const float *__restrict__ w, int stride, const float *x, int len) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 3 < len; i += 4) {
        a0 = fmaf(w[(int64_t)i * stride], x[i], a0);
        a1 = fmaf(w[(int64_t)(i + 1) * stride], x[i + 1], a1);
        a2 = fmaf(w[(int64_t)(i + 2) * stride], x[i + 2], a2);
        a3 = fmaf(w[(int64_t)(i + 3) * stride], x[i + 3], a3);
    }
    for (; i < len; ++i) a0 = fmaf(w[(int64_t)i * stride], x[i], a0);
    return (a0 + a1) + (a2 + a3);
}

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
    const float den = th_softplus(rho_raw[0]) + kEpsRef;
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
    const float a = fmaxf(th_dot(W1 + (int64_t)lane * D, 1, st[wave], D) + b1[lane], 0.f);
    sa[wave][lane] = a;
    if (live) a1_out[sig * kHid + lane] = a;
    __syncthreads();
    float tc[TH_PER_LANE];
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        tc[k] = 0.f;
        if (live && i < D) {
            const float m = tanhf(th_dot(W2 + (int64_t)i * kHid, 1, sa[wave], kHid) + b2[i]);
            m_out[sig * D + i] = m;
            tc[k] = t[k] + 0.1f * m;
        }
    }
    const ThProj p = th_project(D, tc, live ? sigma[sig] : 0.f);
    const float s = fminf(th_sigmoid(pw_raw[0]) / (p.c + kEpsRef), 1.f);
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
    __shared__ float sh[TS_SLAB * 2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + wave;
    const bool live = sig < B;
    const float raw = rho_raw[0], den = th_softplus(raw) + kEpsRef;
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
    const float sp = th_sigmoid(pw_raw[0]), cden = p.c + kEpsRef, q = sp / cden;
    const bool open = q <= 1.f;
    const float s = open ? q : 1.f, gc = open ? -gs * sp / (cden * cden) : 0.f;
    const float gpw = (live && open) ? gs * th_dsigmoid(pw_raw[0]) / cden : 0.f;
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
    float d1 = th_dot(W2 + lane, kHid, sd2[wave], D);
    d1 = (live && a1[sig * kHid + lane] > 0.f) ? d1 : 0.f;
    sd1[wave][lane] = d1;
    if (live) d1_out[sig * kHid + lane] = d1;
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < TH_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        if (live && i < D) {
            const float gt = gtc[k] + th_dot(W1 + i, D, sd1[wave], kHid);
            ggdg[sig * D + i] = gt;
            gzdg[sig * D + i] = gt / den;
            acc = fmaf(gt, zdg[sig * D + i], acc);
        }
    }
    const float v[2] = {-wave_sum(acc) * th_dsoftplus(raw) / (den * den), gpw};
    ts_slab_partials<2>(v, sh, part);
}

// ---- batch-reduced product ---------------------------------------------------------------------------------------------------
struct BpDesc {
    const float *A;    // [B][M]
    const float *Bm;   // [B][N]; nullptr: a column of ones, N = 1
    int M, N;
    int tile0, tn;     // first tile of this product in the launch, tiles along n
    int64_t off;       // offset of C [M][N] in a row of partials and in the output
};
struct BpTable {
    int count;
    BpDesc d[BP_MAX_DESC];
};

// part: [slabs][total] float; grid (tiles, slabs), one wave each
__global__ __launch_bounds__(64) void bp_kernel(BpTable tab, int64_t B, int64_t total, float *__restrict__ part) {
    int di = 0;
    for (int k = 1; k < tab.count; ++k)
        if ((int)blockIdx.x >= tab.d[k].tile0) di = k;
    const BpDesc d = tab.d[di];
    const int tile = blockIdx.x - d.tile0, m0 = 32 * (tile / d.tn), n0 = 32 * (tile % d.tn);
    const int lane = threadIdx.x, r32 = lane & 31, kh = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.y * BP_SLAB, b1 = b0 + BP_SLAB < B ? b0 + BP_SLAB : B;
    const bool mv = m0 + r32 < d.M, nv = n0 + r32 < d.N;
    const float *ap = d.A + (mv ? m0 + r32 : 0);
    const float *bp = d.Bm ? d.Bm + (nv ? n0 + r32 : 0) : nullptr;
    f32x16 acc = {0};
    // BP_UNROLL k steps at a time: their loads are in flight together, the products still accumulate in ascending k order (a
    // k step past the slab's end adds an exact zero)
    const int len = (int)(b1 - b0);
    for (int k0 = 0; k0 < len; k0 += 2 * BP_UNROLL) {
        float x[BP_UNROLL], y[BP_UNROLL];
#pragma unroll
        for (int u = 0; u < BP_UNROLL; ++u) {
            const int64_t b = b0 + k0 + 2 * u + kh;
            const bool bv = b < b1;
            const int64_t bb = bv ? b : b0;
            x[u] = ap[bb * d.M];
            y[u] = bp ? bp[bb * d.N] : 1.f;
            if (!(bv && mv)) x[u] = 0.f;
            if (!(bv && nv)) y[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < BP_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], y[u], acc, 0, 0, 0);
    }
    // C/D layout: column = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
    float *out = part + (int64_t)blockIdx.y * total + d.off;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int gm = m0 + (q & 3) + 8 * (q >> 2) + 4 * kh, gn = n0 + r32;
        if (gm < d.M && gn < d.N) out[(int64_t)gm * d.N + gn] = acc[q];
    }
}

// out[npar + e] = sum over slabs of part[slab][e] in ascending order in float64 (workgroups 1 ..); workgroup 0 adds the `rows`
// rows of the npar (<= 4) per-workgroup partials, one wave per column: lane l the rows l, l + 64, ..., then a butterfly
__global__ __launch_bounds__(TS_THREADS) void bp_sum_kernel(int npar, int64_t rows, const float *__restrict__ rowpart,
                                                            int64_t slabs, int64_t total, const float *__restrict__ part,
                                                            float *__restrict__ out) {
    if (blockIdx.x == 0) {
        const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (c >= npar) return;
        double a = 0.0;
        for (int64_t r = lane; r < rows; r += 64) a += (double)rowpart[r * npar + c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) out[c] = (float)a;
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - 1) * TS_THREADS + threadIdx.x;
    if (e >= total) return;
    double a = 0.0;
    for (int64_t s = 0; s < slabs; ++s) a += (double)part[s * total + e];
    out[npar + e] = (float)a;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static int64_t bp_slabs(int64_t B) { return (B + BP_SLAB - 1) / BP_SLAB; }
static int64_t hlayer_total(int D) { return (int64_t)2 * kHid * D + kHid + D; }   // gW1, gb1, gW2, gb2

// floats: the {g_rho, g_pw} rows of the slabs of four signals, then [batch slabs][gW1, gb1, gW2, gb2]
int64_t train_hlayer_workspace_floats(int D, int64_t B) { return 2 * train_small_rows(B) + bp_slabs(B) * hlayer_total(D); }

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
    float *rowpart = work, *part = work + 2 * rows;
    hipLaunchKernelGGL(th_hlayer_bwd_kernel, dim3((unsigned)rows), dim3(TS_THREADS), 0, st, D, B, gh, zdg, sigma, rho_raw, pw_raw,
                       W1, W2, t, a1, m, ggdg, gzdg, d1, d2, rowpart);
    ADMM_HIP(hipGetLastError());
    const int td = (D + 31) / 32, th = kHid / 32;
    BpTable tab;
    tab.count = 4;
    tab.d[0] = {d1, t, kHid, D, 0, td, 0};                                                   // gW1
    tab.d[1] = {d1, nullptr, kHid, 1, th * td, 1, (int64_t)kHid * D};                        // gb1
    tab.d[2] = {d2, a1, D, kHid, th * td + th, th, (int64_t)kHid * D + kHid};                // gW2
    tab.d[3] = {d2, nullptr, D, 1, 2 * th * td + th, 1, (int64_t)2 * kHid * D + kHid};       // gb2
    const int tiles = 2 * th * td + th + td;
    hipLaunchKernelGGL(bp_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(64), 0, st, tab, B, total, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(bp_sum_kernel, dim3((unsigned)(1 + (total + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, 2, rows,
                       rowpart, slabs, total, part, gpar);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
