// rebuild_core.h -- what every G-layer route ends in, defined once: the learned eigenvalue map, the lower-triangle tile
// decode, and (device only) the f-table fill, the complex tile store and the arrow-row / corner / ||G - C||_F tail of
//   G = V f(Lambda) V^H,  r = ||G - [[diag h, phi], [phi^H, corner_z]]||_F     (the reference's admm_net.py:310-354, 400-403, 454)
// Users: rebuild.hip, rebuild_big.hip, rebuild_lds.h (backrebuild.hip, arrow.hip), arrow.hip's fused tail; the map in double
// and the decode also spectral.hip, spectral_fused.hip, vdvh.hip, train_layer.hip.  tests/test_gpu_variants.py demands the
// same phi from every route, so a change to the map or to the norm is made here and nowhere else.
//
// The residual is summed in one fixed order on every route: a lane's tiles in the order it holds them, entries q = 0 .. 15,
// then its arrow-row entries, then the corner in lane 0 of the corner wave; wave_sum; the waves in ascending order.
// arrow.hip's fused tile loop is not rebuild_tile_store: it turns each real accumulator entry into a complex one first
// (arrow_phase_entry) and holds one accumulator per tile, not two; it shares the tail.
#pragma once
#include "eig_core.h"

namespace admmnet {

// f(lambda) = softplus(lambda - sigmoid(thr)) * sigmoid(value_net(|lambda|))   (admm_net.py:310-334)
// vn: w1[16] b1[16] w2[16] b2[1]; thr already sigmoid-ed
HD float eig_map(float w, float thr, const float *vn) {
    const float base = softplus_f(w - thr);
    const float a = fabsf(w);
    float acc = vn[48];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = fmaf(vn[32 + j], fmaxf(fmaf(vn[j], a, vn[16 + j]), 0.f), acc);
    return base * sigmoid_f(acc);
}

HD double eig_map_f64(double w, double thr, const float *vn) {
    const double x = w - thr;
    const double base = x > 20.0 ? x : log1p(exp(x));
    const double a = fabs(w);
    double acc = vn[48];
    for (int j = 0; j < 16; ++j) {
        const double pre = (double)vn[j] * a + (double)vn[16 + j];
        acc += (double)vn[32 + j] * (pre > 0.0 ? pre : 0.0);
    }
    return base / (1.0 + exp(-acc));
}

// tile t of a lower triangle numbered row by row -> (I, J), I >= J
HD void tri_tile(int t, int &I, int &J) {
    I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    J = t - I * (I + 1) / 2;
}

}  // namespace admmnet

#if defined(__HIPCC__)
#include "common.h"

namespace admmnet {

// fs[c] = f(lambda_c), w0f[c] = w0_c f_c, z0s[c] = w0_c for c < n and zeros for n <= c < count (the k-loops read past n
// unpredicated); wv / w0v: this matrix' eigenvalues and arrow-row entries of V.  The caller's barrier follows.
template <int THREADS>
__device__ __forceinline__ void rebuild_fill_f(int n, int count, const float *wv, const float *w0v,
                                               float thr, const float *vn, float *fs, float *w0f, float *z0s) {
    for (int c = threadIdx.x; c < count; c += THREADS) {
        float f = 0.f, z0 = 0.f;
        if (c < n) {
            f = eig_map(wv[c], thr, vn);
            z0 = w0v[c];
        }
        fs[c] = f;
        w0f[c] = z0 * f;
        z0s[c] = z0;
    }
}

// One 32 x 32 tile with origin (i0, j0), i0 >= j0, out of its two matrix-core accumulators (C/D layout: column = lane & 31,
// row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)): the entries on and below the diagonal inside Da x Da go to Gb (pitch na),
// their conjugates to the upper triangle unless lower_only (state kept as lower triangle), the diagonal exactly real.
// Returns acc2 plus this lane's terms of ||G - C||^2: (re - h)^2 on the diagonal, 2 |g|^2 below it (C is zero there).
__device__ __forceinline__ float rebuild_tile_store(const f32x16 &aRe, const f32x16 &aIm, int i0, int j0, int Da, int na,
                                                    float2 *Gb, const float *hb, int lower_only, float acc2) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int gi = i0 + (q & 3) + 8 * (q >> 2) + 4 * kh;
        const int gj = j0 + l32;
        if (gi < Da && gj < Da && gi >= gj) {
            const float re = aRe[q], im = aIm[q];
            if (gi == gj) {
                Gb[(int64_t)gi * na + gj] = make_float2(re, 0.f);
                const float d = re - hb[gi];
                acc2 += d * d;
            } else {
                Gb[(int64_t)gi * na + gj] = make_float2(re, im);
                if (!lower_only) Gb[(int64_t)gj * na + gi] = make_float2(re, -im);
                acc2 += 2.f * (re * re + im * im);
            }
        }
    }
    return acc2;
}

// The tail of a workgroup of NW waves: arrow row G[Da][o] = row(o) against C[Da][o] = conj(phi_o), the corner
// G[Da][Da] = sum_{c < n} w0f[c] z0s[c] against corner_z in lane 0 of wave corner_wave, and rn = sqrt of the sum.
// acc2: the lane's tile terms.  row(o, re, im) yields entry o for the thread that asks (o = tid, tid + 64 NW, ..).
// redb: NW floats of LDS.  All threads must call it.
template <int NW, class Row>
__device__ __forceinline__ void rebuild_tail(float acc2, int corner_wave, int n, int Da, float2 *Gb,
                                             const float2 *phib, float corner_z, const float *w0f,
                                             const float *z0s, float *redb, float *rnb, int lower_only, Row row) {
    const int na = Da + 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int o = tid; o < Da; o += 64 * NW) {
        float gr, gim;
        row(o, gr, gim);
        Gb[(int64_t)Da * na + o] = make_float2(gr, gim);
        if (!lower_only) Gb[(int64_t)o * na + Da] = make_float2(gr, -gim);
        const float2 p = phib[o];
        const float dr = gr - p.x, di = gim + p.y;
        acc2 += 2.f * (dr * dr + di * di);
    }
    if (wave == corner_wave) {
        float g00 = 0.f;
        for (int c = lane; c < n; c += 64) g00 = fmaf(w0f[c], z0s[c], g00);
        g00 = wave_sum(g00);
        if (lane == 0) {
            Gb[(int64_t)Da * na + Da] = make_float2(g00, 0.f);
            const float d = g00 - corner_z;
            acc2 += d * d;
        }
    }
    acc2 = wave_sum(acc2);
    if (lane == 0) redb[wave] = acc2;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < NW; ++i) s += redb[i];
        *rnb = sqrtf(s);
    }
}

}  // namespace admmnet
#endif
