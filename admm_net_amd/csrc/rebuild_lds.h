// rebuild_lds.h -- G = V f(Lambda) V^H, arrow row, corner and ||G - C||_F with V resident in LDS.
// Shared tail of backrebuild.hip (V from the back-transform) and arrow.hip (V from the arrowhead
// solver); same arithmetic as rebuild.hip (/root/reference/admm_net.py:336-354, 400-403, 454).
//
// LDS inputs (all written before the call, followed by a barrier):
//   VTl[c][rho'] (pitch VP): eigenvector c, rho' = row index in the real plane | Dp + row index in
//                the imaginary plane, planes padded to Dp = 32 ceil(D / 32) with zeros
//   fs[c] = f(lambda_c) with fs[n] = 0, w0f[c] = w0_c f_c, z0s[c] = w0_c (w0 = arrow-row entries of V)
#pragma once
#include "common.h"
#include "rebuild_core.h"

namespace admmnet {

struct BrGeom {
    int D, n, NT, Dp, BP, VP;
    __host__ __device__ explicit BrGeom(int D_) : D(D_), n(D_ + 1), NT((D_ + 31) / 32), Dp(32 * ((D_ + 31) / 32)) {
        BP = 2 * Dp;       // slab B row pitch: real plane | imaginary plane, each padded to 32
        VP = 2 * Dp + 4;   // VT row pitch in LDS
    }
    __host__ __device__ size_t vt_floats() const { return (size_t)n * VP; }
    // fs, w0f, z0s, rowb, redb
    __host__ __device__ size_t small_floats() const { return (size_t)3 * ((n + 4) & ~3) + 2 * Dp + 8; }
};

template <class Mark>
__device__ __forceinline__ void rebuild_from_lds(const BrGeom &g, int64_t b, const float *__restrict__ lw,
                                                 const float *VTl, const float *fs, const float *w0f,
                                                 const float *z0s, float *rowb, float *redb,
                                                 const float2 *__restrict__ phi, const float *__restrict__ h,
                                                 float2 *__restrict__ G, float *__restrict__ rn, Mark mark,
                                                 int lower_only = 0) {
    constexpr int BR_THREADS = 256;
    const int D = g.D, n = g.n, NT = g.NT, Dp = g.Dp, VP = g.VP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, kh = lane >> 5;
    // ---------------- phase C: G = V f V^H, lower-triangle tiles, operands from LDS -------------------
    float2 *Gb = G + b * (int64_t)n * n;
    float acc2 = 0.f;
    const int ntiles = NT * (NT + 1) / 2;
    for (int t = wave; t < ntiles; t += BR_THREADS / 64) {
        int I, J;
        tri_tile(t, I, J);
        const int i0 = 32 * I, j0 = 32 * J;
        f32x16 aRe = {0}, aIm = {0};
        // K-steps in groups of 4, software pipelined: the 20 LDS reads of group g + 1 are issued before
        // the 16 MFMAs of group g.  No predicates: f(lambda) is zero-padded (fs[n] = 0) and the row index
        // is clamped, so the steps beyond n contribute exact zeros.
        constexpr int U = 4;
        const int nks = (n + 1) / 2;
        float fx[U], xr[U], xi[U], yr[U], yi[U];
        // u in [U0, U1) of one group of 4 K-steps
        auto lds_part = [&](int ks0, int U0, int U1, float (&f_)[U], float (&xr_)[U], float (&xi_)[U],
                            float (&yr_)[U], float (&yi_)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < U0 || u >= U1) continue;
                const int c = min(2 * (ks0 + u) + kh, n);
                const float *row = VTl + min(c, n - 1) * VP + l32;
                f_[u] = fs[c];
                xr_[u] = row[i0];
                xi_[u] = row[Dp + i0];
                yr_[u] = row[j0];
                yi_[u] = row[Dp + j0];
            }
        };
        auto mfma_part = [&](int U0, int U1, const float (&f_)[U], const float (&xr_)[U], const float (&xi_)[U],
                             const float (&yr_)[U], const float (&yi_)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < U0 || u >= U1) continue;
                const float ar = xr_[u] * f_[u], ai = xi_[u] * f_[u];
                aRe = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, yr_[u], aRe, 0, 0, 0);
                aIm = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, yr_[u], aIm, 0, 0, 0);
                aRe = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, yi_[u], aRe, 0, 0, 0);
                aIm = __builtin_amdgcn_mfma_f32_32x32x2f32(-ar, yi_[u], aIm, 0, 0, 0);
            }
        };
        // Two register sets in ping-pong, no copies.  The reads of the NEXT group are issued ahead of the MFMAs
        // of the current one, ten at a time: lgkmcnt is a 4-bit counter, so with more than 15 younger reads in
        // flight "wait for the older ones" is not expressible and the compiler falls back to lgkmcnt(0) -- a
        // full LDS round trip in front of every group.  sched_barrier pins the order.
        float fb[U], xrb[U], xib[U], yrb[U], yib[U];
        const int ngrp = (nks + U - 1) / U;
        lds_part(0, 0, U, fx, xr, xi, yr, yi);
        int gq = 0;
        for (; gq + 1 < ngrp; gq += 2) {
            lds_part((gq + 1) * U, 0, 2, fb, xrb, xib, yrb, yib);
            __builtin_amdgcn_sched_barrier(0);
            mfma_part(0, 2, fx, xr, xi, yr, yi);
            __builtin_amdgcn_sched_barrier(0);
            lds_part((gq + 1) * U, 2, 4, fb, xrb, xib, yrb, yib);
            __builtin_amdgcn_sched_barrier(0);
            mfma_part(2, 4, fx, xr, xi, yr, yi);
            __builtin_amdgcn_sched_barrier(0);
            lds_part((gq + 2) * U, 0, 2, fx, xr, xi, yr, yi);   // (past the end: clamped, exact zeros, unused)
            __builtin_amdgcn_sched_barrier(0);
            mfma_part(0, 2, fb, xrb, xib, yrb, yib);
            __builtin_amdgcn_sched_barrier(0);
            lds_part((gq + 2) * U, 2, 4, fx, xr, xi, yr, yi);
            __builtin_amdgcn_sched_barrier(0);
            mfma_part(2, 4, fb, xrb, xib, yrb, yib);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (gq < ngrp) mfma_part(0, U, fx, xr, xi, yr, yi);
        acc2 = rebuild_tile_store(aRe, aIm, i0, j0, D, n, Gb, h + b * D, lower_only, acc2);
    }

    mark(4);
    // ---------------- arrow row (perm row 0 = original row D): G'[0][j] = sum_c w0_c f_c conj(V[j][c])
    //   When the tiles do not divide evenly over the four waves (10 tiles at NT = 4: 3, 3, 2, 2) the waves with
    //   one tile fewer take this row, while the others are still in their last tile.
    {
        const int heavy = ntiles & 3;                                   // waves [0, heavy) had one tile more
        const int first = heavy ? heavy : 0, nl = BR_THREADS / 64 - first;
        if (wave >= first) {
            for (int rp = tid - 64 * first; rp < 2 * Dp; rp += 64 * nl) {
                float a = 0.f;
#pragma unroll 8
                for (int c = 0; c < n; ++c) a = fmaf(w0f[c], VTl[c * VP + rp], a);
                rowb[rp] = a;
            }
        }
    }
    __syncthreads();
    rebuild_tail<BR_THREADS / 64>(acc2, 0, n, D, Gb, phi + b * D, lw[S_CORNER_Z], w0f, z0s, redb, rn + b, lower_only,
                                  [&](int o, float &gr, float &gim) {   // G[D][o]
                                      gr = rowb[o];
                                      gim = -rowb[Dp + o];
                                  });
    mark(5);
}

}  // namespace admmnet
