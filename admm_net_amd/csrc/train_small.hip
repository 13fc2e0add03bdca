// train_small.hip -- the O(B D)-sized steps of one TRAINING layer, one forward and one hand-written backward kernel each, for
// train_route = "full" of admm_net_amd/training.py (the n^2-sized steps are train_layer.hip's).  Every kernel reads the RAW
// parameters from device memory and applies softplus / sigmoid itself; every backward returns gradients for the raw parameters.
//   phi       phi = bs / (1 + rho bs) (y / (b + eps) + rho g_col + z_col), rho = softplus(rho_raw), bs = |b|^2 + eps   admm_net.py:79-105
//   hinput    t = g_dg + z_dg / (softplus(rho_raw) + eps)                                                               :150-152
//   hproject  tc = t + 0.1 m, c = A max|tc| + sum tc, A = 2 sqrt(D) sigma + sigma^2, s = min(sigmoid(pw) / (c + eps), 1),
//             h = tc s (m = correction_net(t), a framework module call between hinput and hproject)                     :160-194
//   eigmap    wp = softplus(w - sigmoid(thr)) sigmoid(W2 relu(W1 |w| + b1) + b2), one 1 -> 16 -> 1 network per eigenvalue :310-334
//   stepsize  u_b = rn_b / (mean_g rn + eps), step_b = rho (0.5 + 1.5 sigmoid(W2 relu(W1 [k/10, rho, u_b] + b1) + b2));
//             the rho FEATURE is a constant (the reference's .item()), the leading rho is not                           :440-474
// Conventions (torch's): relu'(0) = 0, d|x|/dx = 0 at 0, clamp(max = 1) passes the gradient where its argument is <= 1, the
// gradient of max|tc| goes to the lowest index among ties, softplus has beta = 1 and is linear above 20.
//
// Launch shapes.  D <= 256 is at most four elements per lane of one wave, so phi / hinput / hproject / eigmap give every signal
// ONE WAVE and a workgroup a slab of four consecutive signals: the per-signal reductions (max, sum, dot products) are xor-shuffle
// butterflies and need neither LDS nor a barrier.  stepsize couples the signals of a group through their mean: one 256-thread
// workgroup per group (one for the whole call without sub-batches).  The `pair` forms take the mean from outside (the sum over
// the ranks of a sharded batch): slabs of 256 signals, one thread each.
// Sums over the batch (the parameter gradients) run in a fixed order without atomics: per lane serially, across the wave by
// the butterfly, across the slab's four waves serially from LDS into one row of `partials` per workgroup; ts_colsum_kernel (one
// workgroup) then adds the rows in float64 in colsum's order (batch_sums.h).  Two runs give the same bits.
// Every access is a 4-byte (float) or 8-byte (float2) one: the [B, D] tensors need no more than their natural alignment.
#include "common.h"
#include "batch_sums.h"
#include "train_math.h"

namespace admmnet {

constexpr int TS_PER_LANE = 5;             // ceil((kMaxD + 1) / 64): elements of one row a lane visits
constexpr int TS_EIG_PAR = 50;             // g_thr, gW1[16], gb1[16], gW2[16], gb2
constexpr int TS_STEP_PAR = 162;           // g_rho, gW1[32][3], gb1[32], gW2[32], gb2
static_assert(TS_PER_LANE * 64 >= kMaxD + 1, "a wave must cover one row");

// out[c] = sum over rows of part[row][c] in float64 in colsum's fixed order (batch_sums.h), ns slices (count <= 256; one workgroup)
__global__ __launch_bounds__(TS_THREADS) void ts_colsum_kernel(int count, int ns, int64_t rows, const float *__restrict__ part,
                                                               float *__restrict__ out) {
    __shared__ double sh[TS_THREADS];
    colsum(count, ns, rows, count, part, sh);
    if ((int)threadIdx.x < count) out[threadIdx.x] = (float)sh[threadIdx.x];
}

static int ts_colsum(int count, int64_t rows, const float *part, float *out, hipStream_t st) {
    int ns = 1;
    while (2 * ns * count <= TS_THREADS) ns *= 2;
    hipLaunchKernelGGL(ts_colsum_kernel, dim3(1), dim3(TS_THREADS), 0, st, count, ns, rows, part, out);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// ---- phi ---------------------------------------------------------------------------------------------------------------------
struct TsPhi {
    float coef, dcoef;   // bs / (1 + rho bs) and its derivative by rho, -coef^2
    float2 inner;        // y / (b + eps) + rho g + z
};
__device__ __forceinline__ TsPhi ts_phi_at(float2 y, float2 b, float2 g, float2 z, float rho) {
    TsPhi p;
    const float bs = b.x * b.x + b.y * b.y + kEpsRef;
    p.coef = bs / (1.f + rho * bs);
    p.dcoef = -p.coef * p.coef;
    const float dx = b.x + kEpsRef, dy = b.y, dd = dx * dx + dy * dy;
    const float qx = (y.x * dx + y.y * dy) / dd, qy = (y.y * dx - y.x * dy) / dd;
    p.inner = make_float2(qx + rho * g.x + z.x, qy + rho * g.y + z.y);
    return p;
}

__global__ __launch_bounds__(TS_THREADS) void ts_phi_kernel(int D, int64_t B, const float2 *__restrict__ y,
                                                            const float2 *__restrict__ b, const float2 *__restrict__ gcol,
                                                            const float2 *__restrict__ zcol, const float *__restrict__ rho_raw,
                                                            float2 *__restrict__ phi) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const float rho = softplus_f(rho_raw[0]);
    for (int i = threadIdx.x & 63; i < D; i += 64) {
        const int64_t e = sig * D + i;
        const TsPhi p = ts_phi_at(y[e], b[e], gcol[e], zcol[e], rho);
        phi[e] = make_float2(p.coef * p.inner.x, p.coef * p.inner.y);
    }
}

// g_gcol = coef rho g_phi, g_zcol = coef g_phi, g_rho_raw = softplus'(rho_raw) sum Re(conj(g_phi) (coef g + dcoef inner))
__global__ __launch_bounds__(TS_THREADS) void ts_phi_bwd_kernel(int D, int64_t B, const float2 *__restrict__ gphi,
                                                                const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                                const float2 *__restrict__ gcol, const float2 *__restrict__ zcol,
                                                                const float *__restrict__ rho_raw, float2 *__restrict__ ggcol,
                                                                float2 *__restrict__ gzcol, float *__restrict__ part) {
    __shared__ float sh[TS_SLAB];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const float raw = rho_raw[0], rho = softplus_f(raw);
    float acc = 0.f;
    if (sig < B)
        for (int i = threadIdx.x & 63; i < D; i += 64) {
            const int64_t e = sig * D + i;
            const float2 g = gcol[e], u = gphi[e];
            const TsPhi p = ts_phi_at(y[e], b[e], g, zcol[e], rho);
            ggcol[e] = make_float2(p.coef * rho * u.x, p.coef * rho * u.y);
            gzcol[e] = make_float2(p.coef * u.x, p.coef * u.y);
            const float dx = p.coef * g.x + p.dcoef * p.inner.x, dy = p.coef * g.y + p.dcoef * p.inner.y;
            acc = fmaf(u.x, dx, fmaf(u.y, dy, acc));
        }
    const float v[1] = {wave_sum(acc) * dsoftplus_f(raw)};
    ts_slab_partials<1>(v, sh, part);
}

// ---- H input -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void ts_hinput_kernel(int D, int64_t B, const float *__restrict__ gdg,
                                                               const float *__restrict__ zdg, const float *__restrict__ rho_raw,
                                                               float *__restrict__ t) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const float den = softplus_f(rho_raw[0]) + kEpsRef;
    for (int i = threadIdx.x & 63; i < D; i += 64) {
        const int64_t e = sig * D + i;
        t[e] = gdg[e] + zdg[e] / den;
    }
}

// g_gdg = g_t, g_zdg = g_t / den, g_rho_raw = -softplus'(rho_raw) / den^2 sum g_t z_dg, den = softplus(rho_raw) + eps
__global__ __launch_bounds__(TS_THREADS) void ts_hinput_bwd_kernel(int D, int64_t B, const float *__restrict__ gt,
                                                                   const float *__restrict__ zdg, const float *__restrict__ rho_raw,
                                                                   float *__restrict__ ggdg, float *__restrict__ gzdg,
                                                                   float *__restrict__ part) {
    __shared__ float sh[TS_SLAB];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const float raw = rho_raw[0], den = softplus_f(raw) + kEpsRef;
    float acc = 0.f;
    if (sig < B)
        for (int i = threadIdx.x & 63; i < D; i += 64) {
            const int64_t e = sig * D + i;
            const float u = gt[e];
            ggdg[e] = u;
            gzdg[e] = u / den;
            acc = fmaf(u, zdg[e], acc);
        }
    const float v[1] = {-wave_sum(acc) * dsoftplus_f(raw) / (den * den)};
    ts_slab_partials<1>(v, sh, part);
}

// ---- H projection ------------------------------------------------------------------------------------------------------------
// One wave's view of a signal: its tc values, c and the place of max|tc| (lowest index among ties)
struct TsProj {
    float tc[TS_PER_LANE - 1];
    float A, c;
    int imax;
};
__device__ __forceinline__ TsProj ts_project(int D, const float *__restrict__ t, const float *__restrict__ m, float sigma) {
    TsProj p;
    const int lane = threadIdx.x & 63;
    float mx = -1.f, sm = 0.f;
    int im = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < TS_PER_LANE - 1; ++k) {
        const int i = lane + 64 * k;
        p.tc[k] = i < D ? t[i] + 0.1f * m[i] : 0.f;
        sm += p.tc[k];
        if (i < D && fabsf(p.tc[k]) > mx) mx = fabsf(p.tc[k]), im = i;
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

__global__ __launch_bounds__(TS_THREADS) void ts_hproject_kernel(int D, int64_t B, const float *__restrict__ t,
                                                                 const float *__restrict__ m, const float *__restrict__ sigma,
                                                                 const float *__restrict__ pw_raw, float *__restrict__ h) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const TsProj p = ts_project(D, t + sig * D, m + sig * D, sigma[sig]);
    const float s = fminf(sigmoid_f(pw_raw[0]) / (p.c + kEpsRef), 1.f);
#pragma unroll
    for (int k = 0; k < TS_PER_LANE - 1; ++k) {
        const int i = (threadIdx.x & 63) + 64 * k;
        if (i < D) h[sig * D + i] = p.tc[k] * s;
    }
}

// with sp = sigmoid(pw), q = sp / (c + eps), g_s = sum_i g_h[i] tc[i]:
//   q <= 1:  g_c = -g_s sp / (c + eps)^2,  g_tc[i] = g_h[i] q + g_c (1 + [i = imax] A sign(tc[i])),  g_pw += g_s sp (1 - sp) / (c + eps)
//   q >  1:  g_tc = g_h (the clamp holds s at 1 and passes nothing)
// g_t = g_tc, g_m = 0.1 g_tc
__global__ __launch_bounds__(TS_THREADS) void ts_hproject_bwd_kernel(int D, int64_t B, const float *__restrict__ gh,
                                                                     const float *__restrict__ t, const float *__restrict__ m,
                                                                     const float *__restrict__ sigma,
                                                                     const float *__restrict__ pw_raw, float *__restrict__ gt,
                                                                     float *__restrict__ gm, float *__restrict__ part) {
    __shared__ float sh[TS_SLAB];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float gpw = 0.f;
    if (sig < B) {
        const TsProj p = ts_project(D, t + sig * D, m + sig * D, sigma[sig]);
        const float sp = sigmoid_f(pw_raw[0]), den = p.c + kEpsRef, q = sp / den;
        float u[TS_PER_LANE - 1], gs = 0.f;
#pragma unroll
        for (int k = 0; k < TS_PER_LANE - 1; ++k) {
            const int i = lane + 64 * k;
            u[k] = i < D ? gh[sig * D + i] : 0.f;
            gs = fmaf(u[k], p.tc[k], gs);
        }
        gs = wave_sum(gs);
        const bool open = q <= 1.f;
        const float s = open ? q : 1.f, gc = open ? -gs * sp / (den * den) : 0.f;
        if (open) gpw = gs * dsigmoid_f(pw_raw[0]) / den;
#pragma unroll
        for (int k = 0; k < TS_PER_LANE - 1; ++k) {
            const int i = lane + 64 * k;
            if (i >= D) continue;
            const float sgn = p.tc[k] > 0.f ? 1.f : (p.tc[k] < 0.f ? -1.f : 0.f);
            const float gtc = fmaf(u[k], s, gc * (1.f + (i == p.imax ? p.A * sgn : 0.f)));
            gt[sig * D + i] = gtc;
            gm[sig * D + i] = 0.1f * gtc;
        }
    }
    const float v[1] = {gpw};
    ts_slab_partials<1>(v, sh, part);
}

// ---- eigenvalue map ----------------------------------------------------------------------------------------------------------
struct TsValueNet {   // value_net: Linear(1, 16), ReLU, Linear(16, 1), Sigmoid
    float W1[16], b1[16], W2[16], b2, st;   // st = sigmoid(threshold_raw)
};
__device__ __forceinline__ TsValueNet ts_load_value_net(const float *__restrict__ thr, const float *__restrict__ W1,
                                                        const float *__restrict__ b1, const float *__restrict__ W2,
                                                        const float *__restrict__ b2) {
    TsValueNet p;
#pragma unroll
    for (int j = 0; j < 16; ++j) p.W1[j] = W1[j], p.b1[j] = b1[j], p.W2[j] = W2[j];
    p.b2 = b2[0];
    p.st = sigmoid_f(thr[0]);
    return p;
}

__global__ __launch_bounds__(TS_THREADS) void ts_eigmap_kernel(int n, int64_t B, const float *__restrict__ w,
                                                               const float *__restrict__ thr, const float *__restrict__ W1,
                                                               const float *__restrict__ b1, const float *__restrict__ W2,
                                                               const float *__restrict__ b2, float *__restrict__ wp) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const TsValueNet p = ts_load_value_net(thr, W1, b1, W2, b2);
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        const float x = w[sig * n + i], ax = fabsf(x);
        float o = p.b2;
#pragma unroll
        for (int j = 0; j < 16; ++j) o = fmaf(p.W2[j], fmaxf(fmaf(p.W1[j], ax, p.b1[j]), 0.f), o);
        wp[sig * n + i] = softplus_f(x - p.st) * sigmoid_f(o);
    }
}

// with a = softplus(w - st), v = sigmoid(o), g_a = g v, g_o = g a v (1 - v), dh_j = g_o W2_j [pre_j > 0]:
//   g_w = g_a sigmoid(w - st) + sign(w) sum_j dh_j W1_j
//   g_thr_raw = -st (1 - st) sum g_a sigmoid(w - st);  gW1_j = sum dh_j |w|;  gb1_j = sum dh_j;  gW2_j = sum g_o relu(pre_j);  gb2 = sum g_o
__global__ __launch_bounds__(TS_THREADS) void ts_eigmap_bwd_kernel(int n, int64_t B, const float *__restrict__ gwp,
                                                                   const float *__restrict__ w, const float *__restrict__ thr,
                                                                   const float *__restrict__ W1, const float *__restrict__ b1,
                                                                   const float *__restrict__ W2, const float *__restrict__ b2,
                                                                   float *__restrict__ gw, float *__restrict__ part) {
    __shared__ float sh[TS_SLAB * TS_EIG_PAR];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const TsValueNet p = ts_load_value_net(thr, W1, b1, W2, b2);
    float acc[TS_EIG_PAR];
#pragma unroll
    for (int c = 0; c < TS_EIG_PAR; ++c) acc[c] = 0.f;
    if (sig < B)
        for (int i = threadIdx.x & 63; i < n; i += 64) {
            const float x = w[sig * n + i], ax = fabsf(x), g = gwp[sig * n + i];
            float pre[16], o = p.b2;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                pre[j] = fmaf(p.W1[j], ax, p.b1[j]);
                o = fmaf(p.W2[j], fmaxf(pre[j], 0.f), o);
            }
            const float a = softplus_f(x - p.st), da = dsoftplus_f(x - p.st), v = sigmoid_f(o);
            const float ga = g * v, go = g * a * dsigmoid_f(o);
            float gax = 0.f;
            acc[0] = fmaf(ga, da, acc[0]);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float dh = pre[j] > 0.f ? go * p.W2[j] : 0.f;
                acc[1 + j] = fmaf(dh, ax, acc[1 + j]);
                acc[17 + j] += dh;
                acc[33 + j] = fmaf(go, fmaxf(pre[j], 0.f), acc[33 + j]);
                gax = fmaf(dh, p.W1[j], gax);
            }
            acc[49] += go;
            const float sgn = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
            gw[sig * n + i] = fmaf(ga, da, sgn * gax);
        }
#pragma unroll
    for (int c = 0; c < TS_EIG_PAR; ++c) acc[c] = wave_sum(acc[c]);
    acc[0] *= -dsigmoid_f(thr[0]);
    ts_slab_partials<TS_EIG_PAR>(acc, sh, part);
}

// ---- step size ---------------------------------------------------------------------------------------------------------------
// residual_scale_net: Linear(3, 32) (W1 [32][3] row-major), ReLU, Linear(32, 1), Sigmoid.  Group gi of a call with
// sub_batch = g is the signals [gi g, min((gi + 1) g, B)); g = 0: the call is one group.
__device__ __forceinline__ float ts_step_pre(const float *__restrict__ W1, const float *__restrict__ b1, int j, float f0, float f1,
                                             float u) {
    return fmaf(W1[3 * j + 2], u, fmaf(W1[3 * j + 1], f1, fmaf(W1[3 * j], f0, b1[j])));
}

// sum of the group's rn in float64: colsum's order with one column and a slice per thread
__device__ __forceinline__ double ts_group_sum(const float *__restrict__ rn, int64_t r, double *sh) {
    colsum<1, TS_THREADS>(r, rn, sh);
    return sh[0];
}
__device__ __forceinline__ float ts_group_mean(const float *__restrict__ rn, int64_t r, double *sh) {
    return (float)(ts_group_sum(rn, r, sh) / (double)r);
}

// the output layer's pre-activation o = W2 relu(W1 [f0, f1, u] + b1) + b2
__device__ __forceinline__ float ts_step_o(const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2,
                                           const float *__restrict__ b2, float f0, float f1, float u) {
    float o = b2[0];
#pragma unroll
    for (int j = 0; j < 32; ++j) o = fmaf(W2[j], fmaxf(ts_step_pre(W1, b1, j, f0, f1, u), 0.f), o);
    return o;
}
// g_u = sum_j dy W2_j [pre_j > 0] W1[j][2]
__device__ __forceinline__ float ts_step_gu(const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2,
                                            float f0, float f1, float u, float dy) {
    float gu = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (ts_step_pre(W1, b1, j, f0, f1, u) > 0.f) gu = fmaf(dy * W2[j], W1[3 * j + 2], gu);
    return gu;
}

__global__ __launch_bounds__(TS_THREADS) void ts_stepsize_kernel(int64_t B, int64_t g, float knorm, const float *__restrict__ rng,
                                                                 const float *__restrict__ rho_raw, const float *__restrict__ W1,
                                                                 const float *__restrict__ b1, const float *__restrict__ W2,
                                                                 const float *__restrict__ b2, float *__restrict__ stepg) {
    __shared__ double shd[TS_THREADS];
    const int64_t s0 = g ? (int64_t)blockIdx.x * g : 0, r = g ? (B - s0 < g ? B - s0 : g) : B;
    const float *rn = rng + s0;
    const float den = ts_group_mean(rn, r, shd) + kEpsRef, rho = softplus_f(rho_raw[0]);
    for (int64_t i = threadIdx.x; i < r; i += TS_THREADS) {
        const float o = ts_step_o(W1, b1, W2, b2, knorm, rho, rn[i] / den);
        stepg[s0 + i] = rho * (0.5f + 1.5f * sigmoid_f(o));
    }
}

// Pass 2 of the step-size backward over the r signals a workgroup holds: thread (j, q) = (t / 8, t % 8) takes the sums of hidden
// unit j over the signals q, q + 8, ..., joined over q by a butterfly, and thread (j, 0) writes gW1[j], gb1[j], gW2[j] into row.
// at(i) gives signal i's (dy, u).
template <typename Index, class At>
__device__ __forceinline__ void ts_step_hidden_sums(Index r, float knorm, float rho, const float *__restrict__ W1,
                                                    const float *__restrict__ b1, const float *__restrict__ W2, float *row, At at) {
    const int j = threadIdx.x >> 3, q = threadIdx.x & 7;
    const float w2 = W2[j];
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (Index i = q; i < r; i += 8) {
        const float2 v = at(i);
        const float dy = v.x, u = v.y, pre = ts_step_pre(W1, b1, j, knorm, rho, u);
        const float dh = pre > 0.f ? dy * w2 : 0.f;
        s1 += dh;
        s2 = fmaf(dy, fmaxf(pre, 0.f), s2);
        s3 = fmaf(dh, u, s3);
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
        s3 += __shfl_xor(s3, o, 64);
    }
    if (q == 0) {
        row[1 + 3 * j] = knorm * s1;
        row[2 + 3 * j] = rho * s1;
        row[3 + 3 * j] = s3;
        row[97 + j] = s1;
        row[129 + j] = s2;
    }
}

// from g_step [B], with sg_b = sigmoid(o_b), dy_b = g_step_b rho 1.5 sg_b (1 - sg_b), dh_bj = dy_b W2_j [pre_bj > 0],
// g_u_b = sum_j dh_bj W1[j][2], den = mean + eps, r the group's size:
//   g_rn_b = ((g_u_b mean - (sum_b' g_u_b' rn_b') / r) + g_u_b eps) / den^2                (= g_u_b / den - mean(g_u rn) / den^2, the
//            coupling through the mean; in a group of ONE signal the two parts cancel to g_u eps / den^2, which this form keeps --
//            the two products are rounded separately, so their difference is then an exact zero)
//   g_rho_raw = softplus'(rho_raw) sum_b g_step_b (0.5 + 1.5 sg_b)                         (leading factor only)
//   gW2_j = sum_b dy_b relu(pre_bj), gb2 = sum_b dy_b, gb1_j = sum_b dh_bj, gW1[j] = (k/10 gb1_j, rho gb1_j, sum_b dh_bj u_b)
// Pass 1 gives a thread the signals t, t + 256, ... and leaves dy_b in tmp and g_u_b in g_rn; pass 2 gives thread (j, q) =
// (t / 8, t % 8) the sums of hidden unit j over the signals q, q + 8, ..., joined over q by a butterfly; pass 3 finishes g_rn.
// One row of TS_STEP_PAR partials per group.
__global__ __launch_bounds__(TS_THREADS) void ts_stepsize_bwd_kernel(int64_t B, int64_t g, float knorm, const float *__restrict__ gstepg,
                                                                     const float *__restrict__ rng, const float *__restrict__ rho_raw,
                                                                     const float *__restrict__ W1, const float *__restrict__ b1,
                                                                     const float *__restrict__ W2, const float *__restrict__ b2,
                                                                     float *grng, float *tmpg, float *__restrict__ part) {
    __shared__ double shd[TS_THREADS];
    __shared__ float sh[TS_SLAB];
    const int64_t s0 = g ? (int64_t)blockIdx.x * g : 0, r = g ? (B - s0 < g ? B - s0 : g) : B;
    const float *rn = rng + s0, *gstep = gstepg + s0;
    float *grn = grng + s0, *tmp = tmpg + s0;
    const float mean = ts_group_mean(rn, r, shd), den = mean + kEpsRef, raw = rho_raw[0], rho = softplus_f(raw);
    float a_rho = 0.f, a_b2 = 0.f, a_gm = 0.f;
    for (int64_t i = threadIdx.x; i < r; i += TS_THREADS) {
        const float x = rn[i], u = x / den, gs = gstep[i];
        const float o = ts_step_o(W1, b1, W2, b2, knorm, rho, u);
        const float sg = sigmoid_f(o), dy = gs * rho * 1.5f * dsigmoid_f(o);
        const float gu = ts_step_gu(W1, b1, W2, knorm, rho, u, dy);
        a_rho = fmaf(gs, 0.5f + 1.5f * sg, a_rho);
        a_b2 += dy;
        a_gm += __fmul_rn(gu, x);
        tmp[i] = dy;
        grn[i] = gu;
    }
    a_rho = block_sum<TS_SLAB, true>(a_rho, sh);
    a_b2 = block_sum<TS_SLAB, true>(a_b2, sh);
    a_gm = block_sum<TS_SLAB, true>(a_gm, sh);   // (its barriers also order the writes of tmp before pass 2)
    float *row = part + (int64_t)blockIdx.x * TS_STEP_PAR;
    ts_step_hidden_sums(r, knorm, rho, W1, b1, W2, row, [&](int64_t i) { return make_float2(tmp[i], rn[i] / den); });
    if (threadIdx.x == 0) {
        row[0] = a_rho * dsoftplus_f(raw);
        row[161] = a_b2;
    }
    const float gmean = a_gm / (float)r;
    for (int64_t i = threadIdx.x; i < r; i += TS_THREADS) {
        const float gu = grn[i];
        grn[i] = (__fsub_rn(__fmul_rn(gu, mean), gmean) + gu * kEpsRef) / (den * den);
    }
}

// ---- step size from an OUTSIDE mean ------------------------------------------------------------------------------------------
// The batch-sharded training (admm_net_amd/sharded.py) takes the mean over the signals of all ranks: `pair` = (sum of rn, number
// of signals) of the whole batch in float64, all-reduced between ts_rnsum_kernel and the kernels below.  With the mean given no
// reduction is left in the forward: a workgroup takes a slab of TS_THREADS consecutive signals, one per thread.  The backward is
// two kernels around the second all-reduce: `front` leaves g_u_b and this call's share of sum_b g_u_b rn_b, `back` finishes g_rn
// from the sum over all ranks.
__device__ __forceinline__ float ts_pair_mean(const double *__restrict__ pair) { return (float)(pair[0] / pair[1]); }

__global__ __launch_bounds__(TS_THREADS) void ts_rnsum_kernel(int64_t B, const float *__restrict__ rn, double *__restrict__ pair) {
    __shared__ double shd[TS_THREADS];
    const double s = ts_group_sum(rn, B, shd);
    if (threadIdx.x == 0) pair[0] = s, pair[1] = (double)B;
}

__global__ __launch_bounds__(TS_THREADS) void ts_stepsize_pair_kernel(int64_t B, float knorm, const float *__restrict__ rn,
                                                                      const double *__restrict__ pair, const float *__restrict__ rho_raw,
                                                                      const float *__restrict__ W1, const float *__restrict__ b1,
                                                                      const float *__restrict__ W2, const float *__restrict__ b2,
                                                                      float *__restrict__ step) {
    const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= B) return;
    const float den = ts_pair_mean(pair) + kEpsRef, rho = softplus_f(rho_raw[0]);
    const float o = ts_step_o(W1, b1, W2, b2, knorm, rho, rn[i] / den);
    step[i] = rho * (0.5f + 1.5f * sigmoid_f(o));
}

// block_sum<TS_SLAB, true> in float64.  The butterfly stays written out: ts_stepsize_bwd_pair_front_kernel sits at the SGPR ceiling,
// and with a call of wave_sum here the compiler spills 20 SGPRs instead of 10 and gives the kernel a 36-byte private segment.
__device__ __forceinline__ double ts_block_sum_f64(double x, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < TS_SLAB; ++w) s += sh[w];
    return s;
}

// ts_stepsize_bwd_kernel's passes 1 and 2 on one slab, dy_b and u_b of the slab in LDS: g_u_b to gu, one row of TS_STEP_PAR
// partials and one double, sum_b g_u_b rn_b with products and sums in float64, per slab.
__global__ __launch_bounds__(TS_THREADS) void ts_stepsize_bwd_pair_front_kernel(
    int64_t B, float knorm, const float *__restrict__ gstep, const float *__restrict__ rn, const double *__restrict__ pair,
    const float *__restrict__ rho_raw, const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2,
    const float *__restrict__ b2, float *__restrict__ gu_out, double *__restrict__ part_gm, float *__restrict__ part) {
    __shared__ double shd[TS_SLAB];
    __shared__ float sh[TS_SLAB], s_dy[TS_THREADS], s_u[TS_THREADS];
    const int64_t s0 = (int64_t)blockIdx.x * TS_THREADS;
    const int r = B - s0 < TS_THREADS ? (int)(B - s0) : TS_THREADS, t = threadIdx.x;
    const float den = ts_pair_mean(pair) + kEpsRef, raw = rho_raw[0], rho = softplus_f(raw);
    float a_rho = 0.f, dy = 0.f, u = 0.f;
    double a_gm = 0.0;
    if (t < r) {
        const float x = rn[s0 + t], gs = gstep[s0 + t];
        u = x / den;
        const float o = ts_step_o(W1, b1, W2, b2, knorm, rho, u);
        dy = gs * rho * 1.5f * dsigmoid_f(o);
        const float gu = ts_step_gu(W1, b1, W2, knorm, rho, u, dy);
        a_rho = gs * (0.5f + 1.5f * sigmoid_f(o));
        a_gm = (double)gu * (double)x;
        gu_out[s0 + t] = gu;
    }
    s_dy[t] = dy;
    s_u[t] = u;
    a_rho = block_sum<TS_SLAB, true>(a_rho, sh);            // (its barriers also order the writes of s_dy, s_u before pass 2)
    const float a_b2 = block_sum<TS_SLAB, true>(dy, sh);
    a_gm = ts_block_sum_f64(a_gm, shd);
    float *row = part + (int64_t)blockIdx.x * TS_STEP_PAR;
    ts_step_hidden_sums(r, knorm, rho, W1, b1, W2, row, [&](int i) { return make_float2(s_dy[i], s_u[i]); });
    if (t == 0) {
        row[0] = a_rho * dsoftplus_f(raw);
        row[161] = a_b2;
        part_gm[blockIdx.x] = a_gm;
    }
}

// the slabs' rows added in ascending order in float64, one thread per column; thread TS_STEP_PAR adds the slabs' doubles
__global__ __launch_bounds__(TS_THREADS) void ts_pair_finish_kernel(int64_t rows, const double *__restrict__ part_gm,
                                                                    const float *__restrict__ part, float *__restrict__ gpar,
                                                                    double *__restrict__ total) {
    const int c = threadIdx.x;
    double a = 0.0;
    if (c < TS_STEP_PAR) {
        for (int64_t r = 0; r < rows; ++r) a += (double)part[r * TS_STEP_PAR + c];
        gpar[c] = (float)a;
    } else if (c == TS_STEP_PAR) {
        for (int64_t r = 0; r < rows; ++r) a += part_gm[r];
        total[0] = a;
    }
}

// g_rn_b = ((g_u_b mean - total / count) + g_u_b eps) / den^2.  The product and the difference in float64: a float product is exact
// there, so with a pair of ONE signal (mean = rn, total = g_u rn) the difference is an exact zero and g_u eps / den^2 remains.
// gu and grn may be the same buffer.
__global__ __launch_bounds__(TS_THREADS) void ts_stepsize_bwd_pair_back_kernel(int64_t B, const float *gu, const double *__restrict__ pair,
                                                                               const double *__restrict__ total, float *grn) {
    const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= B) return;
    const float mean = ts_pair_mean(pair), den = mean + kEpsRef, g = gu[i];
    const float diff = (float)((double)g * (double)mean - total[0] / pair[1]);
    grn[i] = (diff + g * kEpsRef) / (den * den);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t train_small_rows(int64_t B) { return (B + TS_SLAB - 1) / TS_SLAB; }
int64_t train_small_groups(int64_t B, int64_t g) { return g > 0 ? (B + g - 1) / g : 1; }

#define TS_LAUNCH(kernel, grid, ...)                                                                \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(TS_THREADS), 0, st, __VA_ARGS__);       \
    ADMM_HIP(hipGetLastError())

int launch_train_phi(int D, int64_t B, const float2 *y, const float2 *b, const float2 *gcol, const float2 *zcol,
                     const float *rho_raw, float2 *phi, hipStream_t st) {
    TS_LAUNCH(ts_phi_kernel, train_small_rows(B), D, B, y, b, gcol, zcol, rho_raw, phi);
    return ADMMNET_OK;
}

int launch_train_phi_bwd(int D, int64_t B, const float2 *gphi, const float2 *y, const float2 *b, const float2 *gcol,
                         const float2 *zcol, const float *rho_raw, float2 *ggcol, float2 *gzcol, float *grho, float *part,
                         hipStream_t st) {
    TS_LAUNCH(ts_phi_bwd_kernel, train_small_rows(B), D, B, gphi, y, b, gcol, zcol, rho_raw, ggcol, gzcol, part);
    return ts_colsum(1, train_small_rows(B), part, grho, st);
}

int launch_train_hinput(int D, int64_t B, const float *gdg, const float *zdg, const float *rho_raw, float *t, hipStream_t st) {
    TS_LAUNCH(ts_hinput_kernel, train_small_rows(B), D, B, gdg, zdg, rho_raw, t);
    return ADMMNET_OK;
}

int launch_train_hinput_bwd(int D, int64_t B, const float *gt, const float *zdg, const float *rho_raw, float *ggdg, float *gzdg,
                            float *grho, float *part, hipStream_t st) {
    TS_LAUNCH(ts_hinput_bwd_kernel, train_small_rows(B), D, B, gt, zdg, rho_raw, ggdg, gzdg, part);
    return ts_colsum(1, train_small_rows(B), part, grho, st);
}

int launch_train_hproject(int D, int64_t B, const float *t, const float *m, const float *sigma, const float *pw_raw, float *h,
                          hipStream_t st) {
    TS_LAUNCH(ts_hproject_kernel, train_small_rows(B), D, B, t, m, sigma, pw_raw, h);
    return ADMMNET_OK;
}

int launch_train_hproject_bwd(int D, int64_t B, const float *gh, const float *t, const float *m, const float *sigma,
                              const float *pw_raw, float *gt, float *gm, float *gpw, float *part, hipStream_t st) {
    TS_LAUNCH(ts_hproject_bwd_kernel, train_small_rows(B), D, B, gh, t, m, sigma, pw_raw, gt, gm, part);
    return ts_colsum(1, train_small_rows(B), part, gpw, st);
}

int launch_train_eigmap(int n, int64_t B, const float *w, const float *thr, const float *W1, const float *b1, const float *W2,
                        const float *b2, float *wp, hipStream_t st) {
    TS_LAUNCH(ts_eigmap_kernel, train_small_rows(B), n, B, w, thr, W1, b1, W2, b2, wp);
    return ADMMNET_OK;
}

int launch_train_eigmap_bwd(int n, int64_t B, const float *gwp, const float *w, const float *thr, const float *W1, const float *b1,
                            const float *W2, const float *b2, float *gw, float *gpar, float *part, hipStream_t st) {
    TS_LAUNCH(ts_eigmap_bwd_kernel, train_small_rows(B), n, B, gwp, w, thr, W1, b1, W2, b2, gw, part);
    return ts_colsum(TS_EIG_PAR, train_small_rows(B), part, gpar, st);
}

int launch_train_stepsize(int64_t B, int64_t g, float knorm, const float *rn, const float *rho_raw, const float *W1,
                          const float *b1, const float *W2, const float *b2, float *step, hipStream_t st) {
    TS_LAUNCH(ts_stepsize_kernel, train_small_groups(B, g), B, g, knorm, rn, rho_raw, W1, b1, W2, b2, step);
    return ADMMNET_OK;
}

// part: [groups][TS_STEP_PAR] rows, then B floats for dy
int launch_train_stepsize_bwd(int64_t B, int64_t g, float knorm, const float *gstep, const float *rn, const float *rho_raw,
                              const float *W1, const float *b1, const float *W2, const float *b2, float *grn, float *gpar,
                              float *part, hipStream_t st) {
    const int64_t groups = train_small_groups(B, g);
    TS_LAUNCH(ts_stepsize_bwd_kernel, groups, B, g, knorm, gstep, rn, rho_raw, W1, b1, W2, b2, grn, part + groups * TS_STEP_PAR,
              part);
    return ts_colsum(TS_STEP_PAR, groups, part, gpar, st);
}

int64_t train_pair_rows(int64_t B) { return (B + TS_THREADS - 1) / TS_THREADS; }
int64_t train_pair_partials(int64_t B) { return train_pair_rows(B) * (2 + TS_STEP_PAR); }

int launch_train_rnsum(int64_t B, const float *rn, double *pair, hipStream_t st) {
    TS_LAUNCH(ts_rnsum_kernel, 1, B, rn, pair);
    return ADMMNET_OK;
}

int launch_train_stepsize_pair(int64_t B, float knorm, const float *rn, const double *pair, const float *rho_raw, const float *W1,
                               const float *b1, const float *W2, const float *b2, float *step, hipStream_t st) {
    TS_LAUNCH(ts_stepsize_pair_kernel, train_pair_rows(B), B, knorm, rn, pair, rho_raw, W1, b1, W2, b2, step);
    return ADMMNET_OK;
}

// part: [slabs] doubles, then [slabs][TS_STEP_PAR] floats
int launch_train_stepsize_bwd_pair_front(int64_t B, float knorm, const float *gstep, const float *rn, const double *pair,
                                         const float *rho_raw, const float *W1, const float *b1, const float *W2, const float *b2,
                                         float *gu, float *gpar, double *total, float *part, hipStream_t st) {
    const int64_t rows = train_pair_rows(B);
    double *part_gm = reinterpret_cast<double *>(part);
    float *rowsf = part + 2 * rows;
    TS_LAUNCH(ts_stepsize_bwd_pair_front_kernel, rows, B, knorm, gstep, rn, pair, rho_raw, W1, b1, W2, b2, gu, part_gm, rowsf);
    TS_LAUNCH(ts_pair_finish_kernel, 1, rows, part_gm, rowsf, gpar, total);
    return ADMMNET_OK;
}

int launch_train_stepsize_bwd_pair_back(int64_t B, const float *gu, const double *pair, const double *total, float *grn,
                                        hipStream_t st) {
    TS_LAUNCH(ts_stepsize_bwd_pair_back_kernel, train_pair_rows(B), B, gu, pair, total, grn);
    return ADMMNET_OK;
}

}  // namespace admmnet
