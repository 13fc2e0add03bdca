// train_layer.hip -- the n^2-sized steps of one TRAINING layer as streaming kernels (forward and hand-written backward),
// for the differentiable route of admm_net_amd/training.py.  With C(phi, h, c) = [[diag h, phi], [phi^H, c]] (never
// materialised: it differs from zero only on the diagonal, the border row / column and the corner, handled by index),
// herm(X) = (X + X^H) / 2 and <X, Y> = Re sum conj(X_ij) Y_ij:
//   matrix   A  = herm(C(phi, h, c_g) - r Z)        GLayer, admm_net.py:262-300 (block matrix, - Z / rho,
//                                                    symmetrisation); A is what the eigensolver reads
//   resnorm  rn = ||G - C(phi, h, c_z)||_F           ZLayer, admm_net.py:428-459 (block matrix, residual, its norm)
//   zupdate  Z' = Z + s (G - C(phi, h, c_z))         ZLayer, admm_net.py:460-474
//   gather   X[:, :D, D], Re diag X[:, :D]           what PhiLayer (admm_net.py:98-99) and HLayer (:150-152) read of G and Z
// and their backwards (formulas at each kernel).  The residual R = G - C is recomputed where it is needed and never stored.
//
// Two kernel shapes:
//   * matrix / matrix_bwd need X and X^H: one 256-thread workgroup per (signal, pair of 32 x 32 tiles (I, J), I >= J).  Both
//     tiles are read row-wise (a lane per column: 256 B per row segment), transposed through LDS, and both result tiles are
//     written row-wise.  A(i, j) = (p_ij + conj p_ji) / 2 with p evaluated by the same instruction sequence at both
//     places, so A(j, i) is conj A(i, j) bit for bit and the diagonal's imaginary part is an exact zero.
//   * resnorm / resnorm_bwd / zupdate / zupdate_bwd read the matrix as a flat stream: one 1024-thread workgroup per signal
//     (16 waves per CU keep enough loads in flight once B reaches the CU count; a smaller batch is a small problem).  n is
//     odd at every tuned geometry, so a matrix starts 8-byte aligned only: the stream is peeled by one element where the
//     matrix starts on an odd element, and the body moves 16 bytes (two complex numbers) per lane.
// Every sum runs in a fixed order -- per thread serially, across a wave by xor-shuffles, across the waves serially from
// LDS -- and the sum over the batch (g_r) in float64 by one workgroup (colsum of batch_sums.h).  No atomics.
#include "common.h"
#include "batch_sums.h"
#include "rebuild_core.h"

namespace admmnet {

constexpr int TL_TILE = 32;
constexpr int TL_PAIR_THREADS = 256;
constexpr int TL_STREAM_THREADS = 1024;

// C(phi, h, c)(i, j); D = n - 1 is the border index
__device__ __forceinline__ float2 tl_c(int i, int j, int D, const float2 *__restrict__ phi, const float *__restrict__ h,
                                       float corner) {
    if (i == j) return make_float2(i == D ? corner : h[i], 0.f);
    if (j == D) return phi[i];
    if (i == D) {
        const float2 p = phi[j];
        return make_float2(p.x, -p.y);
    }
    return make_float2(0.f, 0.f);
}

// ---- matrix: A = herm(C - r Z) -------------------------------------------------------------------------------------------
// LDS tile T[r][c] with one column of padding
struct TlTiles {
    float2 a[TL_TILE][TL_TILE + 1];   // X[32 I + r][32 J + c]
    float2 b[TL_TILE][TL_TILE + 1];   // X[32 J + r][32 I + c]
};

__device__ __forceinline__ void tl_load_tiles(TlTiles &T, const float2 *__restrict__ X, int n, int I, int J) {
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int r = r0; r < TL_TILE; r += TL_PAIR_THREADS / 32) {
        const int ia = TL_TILE * I + r, ja = TL_TILE * J + c;
        T.a[r][c] = (ia < n && ja < n) ? X[(int64_t)ia * n + ja] : make_float2(0.f, 0.f);
        if (I != J) {
            const int ib = TL_TILE * J + r, jb = TL_TILE * I + c;
            T.b[r][c] = (ib < n && jb < n) ? X[(int64_t)ib * n + jb] : make_float2(0.f, 0.f);
        }
    }
}

__global__ __launch_bounds__(TL_PAIR_THREADS) void tl_matrix_kernel(int n, int npairs, const float2 *__restrict__ phig,
                                                                    const float *__restrict__ hg, const float2 *__restrict__ Zg,
                                                                    const float *__restrict__ rp, float corner,
                                                                    float2 *__restrict__ Ag) {
    __shared__ TlTiles T;
    const int64_t b = blockIdx.x / npairs;
    int I, J;
    tri_tile((int)(blockIdx.x - b * npairs), I, J);
    const int D = n - 1;
    const float2 *phi = phig + b * D, *Z = Zg + b * (int64_t)n * n;
    const float *h = hg + b * D;
    float2 *A = Ag + b * (int64_t)n * n;
    const float r = rp[0];
    tl_load_tiles(T, Z, n, I, J);
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int half = 0; half < (I == J ? 1 : 2); ++half) {
        // half 0 writes tile (I, J) from a and b^T, half 1 tile (J, I) from b and a^T
        const int Ti = half ? J : I, Tj = half ? I : J;
        for (int rr = r0; rr < TL_TILE; rr += TL_PAIR_THREADS / 32) {
            const int i = TL_TILE * Ti + rr, j = TL_TILE * Tj + c;
            if (i >= n || j >= n) continue;
            const float2 x = half ? T.b[rr][c] : T.a[rr][c];
            const float2 y = (I == J) ? T.a[c][rr] : (half ? T.a[c][rr] : T.b[c][rr]);
            const float2 cij = tl_c(i, j, D, phi, h, corner), cji = tl_c(j, i, D, phi, h, corner);
            const float px = fmaf(-r, x.x, cij.x), py = fmaf(-r, x.y, cij.y);     // p_ij
            const float qx = fmaf(-r, y.x, cji.x), qy = fmaf(-r, y.y, cji.y);     // p_ji
            A[(int64_t)i * n + j] = make_float2(0.5f * (px + qx), 0.5f * (py - qy));
        }
    }
}

// backward of matrix from gA, with S = herm(gA):
//   gZ = -r S,  g_phi[i] = 2 S[i, D],  g_h[i] = Re S[i, i],  part[b][pair] = <S, Z> over the pair's elements
// (g_r = -sum of all parts, tl_negsum_kernel).
__global__ __launch_bounds__(TL_PAIR_THREADS) void tl_matrix_bwd_kernel(int n, int npairs, const float2 *__restrict__ gAg,
                                                                        const float2 *__restrict__ Zg,
                                                                        const float *__restrict__ rp, float2 *__restrict__ gZg,
                                                                        float2 *__restrict__ gphig, float *__restrict__ ghg,
                                                                        float *__restrict__ part) {
    __shared__ TlTiles T;
    __shared__ float sh[TL_PAIR_THREADS / 64];
    const int64_t b = blockIdx.x / npairs;
    int I, J;
    tri_tile((int)(blockIdx.x - b * npairs), I, J);
    const int D = n - 1;
    const float2 *gA = gAg + b * (int64_t)n * n, *Z = Zg + b * (int64_t)n * n;
    float2 *gZ = gZg + b * (int64_t)n * n, *gphi = gphig + b * D;
    float *gh = ghg + b * D;
    const float r = rp[0];
    tl_load_tiles(T, gA, n, I, J);
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    float acc = 0.f;
    for (int half = 0; half < (I == J ? 1 : 2); ++half) {
        const int Ti = half ? J : I, Tj = half ? I : J;
        for (int rr = r0; rr < TL_TILE; rr += TL_PAIR_THREADS / 32) {
            const int i = TL_TILE * Ti + rr, j = TL_TILE * Tj + c;
            if (i >= n || j >= n) continue;
            const float2 x = half ? T.b[rr][c] : T.a[rr][c];
            const float2 y = (I == J) ? T.a[c][rr] : (half ? T.a[c][rr] : T.b[c][rr]);
            const float sx = 0.5f * (x.x + y.x), sy = 0.5f * (x.y - y.y);
            const float2 z = Z[(int64_t)i * n + j];
            acc = fmaf(sx, z.x, fmaf(sy, z.y, acc));
            gZ[(int64_t)i * n + j] = make_float2(-r * sx, -r * sy);
            if (j == D && i < D) gphi[i] = make_float2(2.f * sx, 2.f * sy);
            if (i == j && i < D) gh[i] = sx;
        }
    }
    const float s = block_sum<TL_PAIR_THREADS / 64, false>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[0] = -(sum of part[0 .. count)) in float64, fixed order (one workgroup)
__global__ __launch_bounds__(1024) void tl_negsum_kernel(int64_t count, const float *__restrict__ part, float *__restrict__ out) {
    __shared__ double sh[1024];
    colsum<1, 1024>(count, part, sh);
    if (threadIdx.x == 0) out[0] = (float)(-sh[0]);
}

// ---- flat streams ----------------------------------------------------------------------------------------------------------
// Element e of matrix b sits at complex index b n^2 + e.  With `vec` (every base pointer 16-byte aligned) the elements
// [head, head + 2 npair) are visited as 16-byte pairs, head = (b n^2) & 1, and the at most two leftover elements singly;
// without it every element singly.  f(e, i, j) is called once per element; a pair calls it for e and e + 1.
struct TlSpan {
    int head, npair, total;
};
__device__ __forceinline__ TlSpan tl_span(int64_t b, int n, bool vec) {
    TlSpan s;
    s.total = n * n;
    s.head = vec ? (int)((b * (int64_t)s.total) & 1) : 0;
    s.npair = vec ? (s.total - s.head) / 2 : 0;
    return s;
}

// rn[b] = ||G_b - C||_F
__global__ __launch_bounds__(TL_STREAM_THREADS) void tl_resnorm_kernel(int n, bool vec, const float2 *__restrict__ Gg,
                                                                       const float2 *__restrict__ phig,
                                                                       const float *__restrict__ hg, float corner,
                                                                       float *__restrict__ rn) {
    __shared__ float sh[TL_STREAM_THREADS / 64];
    const int64_t b = blockIdx.x;
    const int D = n - 1;
    const float2 *G = Gg + b * (int64_t)n * n, *phi = phig + b * D;
    const float *h = hg + b * D;
    const TlSpan sp = tl_span(b, n, vec);
    float acc = 0.f;
    auto one = [&](int e, float2 g) {
        const int i = e / n, j = e - i * n;
        const float2 c = tl_c(i, j, D, phi, h, corner);
        const float rx = g.x - c.x, ry = g.y - c.y;
        acc = fmaf(rx, rx, fmaf(ry, ry, acc));
    };
    for (int p = threadIdx.x; p < sp.npair; p += TL_STREAM_THREADS) {
        const int e = sp.head + 2 * p;
        const float4 g = *reinterpret_cast<const float4 *>(G + e);
        one(e, make_float2(g.x, g.y));
        one(e + 1, make_float2(g.z, g.w));
    }
    // leftovers: element 0 when head = 1, and everything behind the last pair
    for (int e = sp.head + 2 * sp.npair + threadIdx.x; e < sp.total; e += TL_STREAM_THREADS) one(e, G[e]);
    if (sp.head && threadIdx.x == TL_STREAM_THREADS - 1) one(0, G[0]);
    const float s = block_sum<TL_STREAM_THREADS / 64, false>(acc, sh);
    if (threadIdx.x == 0) rn[b] = sqrtf(s);
}

// backward of resnorm from g_rn, with q = g_rn / rn:
//   gG = q R,  g_phi[i] = -q (R[i, D] + conj R[D, i]),  g_h[i] = -q Re R[i, i]
__global__ __launch_bounds__(TL_STREAM_THREADS) void tl_resnorm_bwd_kernel(int n, bool vec, const float *__restrict__ grn,
                                                                           const float *__restrict__ rn,
                                                                           const float2 *__restrict__ Gg,
                                                                           const float2 *__restrict__ phig,
                                                                           const float *__restrict__ hg, float corner,
                                                                           float2 *__restrict__ gGg, float2 *__restrict__ gphig,
                                                                           float *__restrict__ ghg) {
    const int64_t b = blockIdx.x;
    const int D = n - 1;
    const float2 *G = Gg + b * (int64_t)n * n, *phi = phig + b * D;
    const float *h = hg + b * D;
    float2 *gG = gGg + b * (int64_t)n * n, *gphi = gphig + b * D;
    float *gh = ghg + b * D;
    const float q = grn[b] / rn[b];
    const TlSpan sp = tl_span(b, n, vec);
    auto one = [&](int e, float2 g) {
        const int i = e / n, j = e - i * n;
        const float2 c = tl_c(i, j, D, phi, h, corner);
        return make_float2(q * (g.x - c.x), q * (g.y - c.y));
    };
    for (int p = threadIdx.x; p < sp.npair; p += TL_STREAM_THREADS) {
        const int e = sp.head + 2 * p;
        const float4 g = *reinterpret_cast<const float4 *>(G + e);
        const float2 u = one(e, make_float2(g.x, g.y)), v = one(e + 1, make_float2(g.z, g.w));
        *reinterpret_cast<float4 *>(gG + e) = make_float4(u.x, u.y, v.x, v.y);
    }
    for (int e = sp.head + 2 * sp.npair + threadIdx.x; e < sp.total; e += TL_STREAM_THREADS) gG[e] = one(e, G[e]);
    if (sp.head && threadIdx.x == TL_STREAM_THREADS - 1) gG[0] = one(0, G[0]);
    for (int i = threadIdx.x; i < D; i += TL_STREAM_THREADS) {
        const float2 p = phi[i], col = G[(int64_t)i * n + D], row = G[(int64_t)D * n + i];
        // R[i, D] = col - phi_i,  conj R[D, i] = conj(row - conj phi_i) = conj(row) - phi_i
        gphi[i] = make_float2(-q * ((col.x - p.x) + (row.x - p.x)), -q * ((col.y - p.y) + (-row.y - p.y)));
        gh[i] = -q * (G[(int64_t)i * n + i].x - h[i]);
    }
}

// Zn = Z + s (G - C)
__global__ __launch_bounds__(TL_STREAM_THREADS) void tl_zupdate_kernel(int n, bool vec, const float2 *__restrict__ Zg,
                                                                       const float2 *__restrict__ Gg,
                                                                       const float2 *__restrict__ phig,
                                                                       const float *__restrict__ hg, const float *__restrict__ sg,
                                                                       float corner, float2 *__restrict__ Zng) {
    const int64_t b = blockIdx.x;
    const int D = n - 1;
    const float2 *Z = Zg + b * (int64_t)n * n, *G = Gg + b * (int64_t)n * n, *phi = phig + b * D;
    const float *h = hg + b * D;
    float2 *Zn = Zng + b * (int64_t)n * n;
    const float s = sg[b];
    const TlSpan sp = tl_span(b, n, vec);
    auto one = [&](int e, float2 z, float2 g) {
        const int i = e / n, j = e - i * n;
        const float2 c = tl_c(i, j, D, phi, h, corner);
        return make_float2(fmaf(s, g.x - c.x, z.x), fmaf(s, g.y - c.y, z.y));
    };
    for (int p = threadIdx.x; p < sp.npair; p += TL_STREAM_THREADS) {
        const int e = sp.head + 2 * p;
        const float4 z = *reinterpret_cast<const float4 *>(Z + e), g = *reinterpret_cast<const float4 *>(G + e);
        const float2 u = one(e, make_float2(z.x, z.y), make_float2(g.x, g.y));
        const float2 v = one(e + 1, make_float2(z.z, z.w), make_float2(g.z, g.w));
        *reinterpret_cast<float4 *>(Zn + e) = make_float4(u.x, u.y, v.x, v.y);
    }
    for (int e = sp.head + 2 * sp.npair + threadIdx.x; e < sp.total; e += TL_STREAM_THREADS) Zn[e] = one(e, Z[e], G[e]);
    if (sp.head && threadIdx.x == TL_STREAM_THREADS - 1) Zn[0] = one(0, Z[0], G[0]);
}

// backward of zupdate from g (gZ is g itself and needs no kernel):
//   gG = s g,  g_s[b] = <R_b, g_b>,  g_phi[i] = -s (g[i, D] + conj g[D, i]),  g_h[i] = -s Re g[i, i]
__global__ __launch_bounds__(TL_STREAM_THREADS) void tl_zupdate_bwd_kernel(int n, bool vec, const float2 *__restrict__ gg,
                                                                           const float2 *__restrict__ Gg,
                                                                           const float2 *__restrict__ phig,
                                                                           const float *__restrict__ hg, const float *__restrict__ sg,
                                                                           float corner, float2 *__restrict__ gGg,
                                                                           float2 *__restrict__ gphig, float *__restrict__ ghg,
                                                                           float *__restrict__ gsg) {
    __shared__ float sh[TL_STREAM_THREADS / 64];
    const int64_t b = blockIdx.x;
    const int D = n - 1;
    const float2 *gin = gg + b * (int64_t)n * n, *G = Gg + b * (int64_t)n * n, *phi = phig + b * D;
    const float *h = hg + b * D;
    float2 *gG = gGg + b * (int64_t)n * n, *gphi = gphig + b * D;
    float *gh = ghg + b * D;
    const float s = sg[b];
    const TlSpan sp = tl_span(b, n, vec);
    float acc = 0.f;
    auto one = [&](int e, float2 u, float2 g) {
        const int i = e / n, j = e - i * n;
        const float2 c = tl_c(i, j, D, phi, h, corner);
        acc = fmaf(g.x - c.x, u.x, fmaf(g.y - c.y, u.y, acc));
        return make_float2(s * u.x, s * u.y);
    };
    for (int p = threadIdx.x; p < sp.npair; p += TL_STREAM_THREADS) {
        const int e = sp.head + 2 * p;
        const float4 u = *reinterpret_cast<const float4 *>(gin + e), g = *reinterpret_cast<const float4 *>(G + e);
        const float2 o0 = one(e, make_float2(u.x, u.y), make_float2(g.x, g.y));
        const float2 o1 = one(e + 1, make_float2(u.z, u.w), make_float2(g.z, g.w));
        *reinterpret_cast<float4 *>(gG + e) = make_float4(o0.x, o0.y, o1.x, o1.y);
    }
    for (int e = sp.head + 2 * sp.npair + threadIdx.x; e < sp.total; e += TL_STREAM_THREADS) gG[e] = one(e, gin[e], G[e]);
    if (sp.head && threadIdx.x == TL_STREAM_THREADS - 1) gG[0] = one(0, gin[0], G[0]);
    for (int i = threadIdx.x; i < D; i += TL_STREAM_THREADS) {
        const float2 col = gin[(int64_t)i * n + D], row = gin[(int64_t)D * n + i];
        gphi[i] = make_float2(-s * (col.x + row.x), -s * (col.y - row.y));
        gh[i] = -s * gin[(int64_t)i * n + i].x;
    }
    const float t = block_sum<TL_STREAM_THREADS / 64, false>(acc, sh);
    if (threadIdx.x == 0) gsg[b] = t;
}

// ---- border column and diagonal: what the phi layer and the H layer read of G and Z ---------------------------------------------
// gather: col[b][i] = X[b][i][D], dg[b][i] = Re X[b][i][i], i < D (admm_net.py:98-99 and :150-152 slice these out of the
// dense matrices; autograd answers every such slice with a zero-filled dense tensor).
__global__ __launch_bounds__(256) void tl_gather_kernel(int n, int64_t total, const float2 *__restrict__ Xg,
                                                        float2 *__restrict__ col, float *__restrict__ dg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int D = n - 1;
    const int64_t b = t / D;
    const int i = (int)(t - b * D);
    const float2 *X = Xg + b * (int64_t)n * n;
    col[t] = X[(int64_t)i * n + D];
    dg[t] = X[(int64_t)i * n + i].x;
}

// E(col, dg)(i, j): col[i] at (i, D), dg[i] at (i, i), i < D; zero elsewhere.  This is the gradient of the gather.
__device__ __forceinline__ float2 tl_e(int i, int j, int D, const float2 *__restrict__ col, const float *__restrict__ dg) {
    if (i < D && j == D) return col[i];
    if (i == j && i < D) return make_float2(dg[i], 0.f);
    return make_float2(0.f, 0.f);
}

// backward of gather: gX = E(g_col, g_dg), written as one stream (no separate zero fill)
__global__ __launch_bounds__(TL_STREAM_THREADS) void tl_scatter_kernel(int n, bool vec, const float2 *__restrict__ gcolg,
                                                                       const float *__restrict__ gdgg, float2 *__restrict__ gXg) {
    const int64_t b = blockIdx.x;
    const int D = n - 1;
    const float2 *gcol = gcolg + b * D;
    const float *gdg = gdgg + b * D;
    float2 *gX = gXg + b * (int64_t)n * n;
    const TlSpan sp = tl_span(b, n, vec);
    auto one = [&](int e) {
        const int i = e / n, j = e - i * n;
        return tl_e(i, j, D, gcol, gdg);
    };
    for (int p = threadIdx.x; p < sp.npair; p += TL_STREAM_THREADS) {
        const int e = sp.head + 2 * p;
        const float2 u = one(e), v = one(e + 1);
        *reinterpret_cast<float4 *>(gX + e) = make_float4(u.x, u.y, v.x, v.y);
    }
    for (int e = sp.head + 2 * sp.npair + threadIdx.x; e < sp.total; e += TL_STREAM_THREADS) gX[e] = one(e);
    if (sp.head && threadIdx.x == TL_STREAM_THREADS - 1) gX[0] = one(0);
}

// S = herm(g + E(g_col, g_dg)), exactly Hermitian: what the rebuild's backward hands to vhsv_kernel when G's border column
// and diagonal left the rebuild as outputs of their own (g_col / g_dg null: S = herm(g)).
__global__ __launch_bounds__(TL_PAIR_THREADS) void tl_herm_kernel(int n, int npairs, const float2 *__restrict__ gg,
                                                                  const float2 *__restrict__ gcolg, const float *__restrict__ gdgg,
                                                                  float2 *__restrict__ Sg) {
    __shared__ TlTiles T;
    const int64_t b = blockIdx.x / npairs;
    int I, J;
    tri_tile((int)(blockIdx.x - b * npairs), I, J);
    const int D = n - 1;
    const bool sc = gcolg != nullptr;
    const float2 *g = gg + b * (int64_t)n * n, *gcol = sc ? gcolg + b * D : nullptr;
    const float *gdg = sc ? gdgg + b * D : nullptr;
    float2 *S = Sg + b * (int64_t)n * n;
    tl_load_tiles(T, g, n, I, J);
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int half = 0; half < (I == J ? 1 : 2); ++half) {
        const int Ti = half ? J : I, Tj = half ? I : J;
        for (int rr = r0; rr < TL_TILE; rr += TL_PAIR_THREADS / 32) {
            const int i = TL_TILE * Ti + rr, j = TL_TILE * Tj + c;
            if (i >= n || j >= n) continue;
            float2 x = half ? T.b[rr][c] : T.a[rr][c];
            float2 y = (I == J) ? T.a[c][rr] : (half ? T.a[c][rr] : T.b[c][rr]);
            if (sc) {
                const float2 ex = tl_e(i, j, D, gcol, gdg), ey = tl_e(j, i, D, gcol, gdg);
                x.x += ex.x, x.y += ex.y, y.x += ey.x, y.y += ey.y;
            }
            S[(int64_t)i * n + j] = make_float2(0.5f * (x.x + y.x), 0.5f * (x.y - y.y));
        }
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
static bool tl_aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

int train_tile_pairs(int n) {
    const int nt = (n + TL_TILE - 1) / TL_TILE;
    return nt * (nt + 1) / 2;
}

int launch_train_matrix(int n, int64_t B, const float2 *phi, const float *h, const float2 *Z, const float *r, float corner,
                        float2 *A, hipStream_t st) {
    const int np = train_tile_pairs(n);
    hipLaunchKernelGGL(tl_matrix_kernel, dim3((unsigned)(B * np)), dim3(TL_PAIR_THREADS), 0, st, n, np, phi, h, Z, r, corner, A);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_matrix_bwd(int n, int64_t B, const float2 *gA, const float2 *Z, const float *r, float2 *gZ, float2 *gphi,
                            float *gh, float *gr, float *part, hipStream_t st) {
    const int np = train_tile_pairs(n);
    hipLaunchKernelGGL(tl_matrix_bwd_kernel, dim3((unsigned)(B * np)), dim3(TL_PAIR_THREADS), 0, st, n, np, gA, Z, r, gZ, gphi,
                       gh, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(tl_negsum_kernel, dim3(1), dim3(1024), 0, st, B * np, part, gr);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_resnorm(int n, int64_t B, const float2 *G, const float2 *phi, const float *h, float corner, float *rn,
                         hipStream_t st) {
    hipLaunchKernelGGL(tl_resnorm_kernel, dim3((unsigned)B), dim3(TL_STREAM_THREADS), 0, st, n, tl_aligned16(G), G, phi, h,
                       corner, rn);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_resnorm_bwd(int n, int64_t B, const float *grn, const float *rn, const float2 *G, const float2 *phi,
                             const float *h, float corner, float2 *gG, float2 *gphi, float *gh, hipStream_t st) {
    hipLaunchKernelGGL(tl_resnorm_bwd_kernel, dim3((unsigned)B), dim3(TL_STREAM_THREADS), 0, st, n, tl_aligned16(G, gG), grn, rn,
                       G, phi, h, corner, gG, gphi, gh);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_zupdate(int n, int64_t B, const float2 *Z, const float2 *G, const float2 *phi, const float *h, const float *s,
                         float corner, float2 *Zn, hipStream_t st) {
    hipLaunchKernelGGL(tl_zupdate_kernel, dim3((unsigned)B), dim3(TL_STREAM_THREADS), 0, st, n, tl_aligned16(Z, G, Zn), Z, G, phi,
                       h, s, corner, Zn);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_zupdate_bwd(int n, int64_t B, const float2 *g, const float2 *G, const float2 *phi, const float *h,
                             const float *s, float corner, float2 *gG, float2 *gphi, float *gh, float *gs, hipStream_t st) {
    hipLaunchKernelGGL(tl_zupdate_bwd_kernel, dim3((unsigned)B), dim3(TL_STREAM_THREADS), 0, st, n, tl_aligned16(g, G, gG), g, G,
                       phi, h, s, corner, gG, gphi, gh, gs);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_gather(int n, int64_t B, const float2 *X, float2 *col, float *dg, hipStream_t st) {
    const int64_t total = B * (n - 1);
    hipLaunchKernelGGL(tl_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n, total, X, col, dg);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_scatter(int n, int64_t B, const float2 *gcol, const float *gdg, float2 *gX, hipStream_t st) {
    hipLaunchKernelGGL(tl_scatter_kernel, dim3((unsigned)B), dim3(TL_STREAM_THREADS), 0, st, n, tl_aligned16(gX), gcol, gdg, gX);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_herm(int n, int64_t B, const float2 *g, const float2 *gcol, const float *gdg, float2 *S, hipStream_t st) {
    const int np = train_tile_pairs(n);
    hipLaunchKernelGGL(tl_herm_kernel, dim3((unsigned)(B * np)), dim3(TL_PAIR_THREADS), 0, st, n, np, g, gcol, gdg, S);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
