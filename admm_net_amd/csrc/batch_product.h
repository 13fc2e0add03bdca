// batch_product.h -- the batch-reduced product C[m][n] = sum_b A[b][m] Bm[b][n] of the training backwards (train_hlayer.hip,
// train_head.hip): every weight gradient is one, with a column of ones appended to Bm for the bias.  The batch index is the k
// dimension of v_mfma_f32_32x32x2_f32, whose A operand is A[i = lane & 31][k = lane >> 5] and B operand B[k = lane >> 5][j = lane & 31]:
// with the batch as k both are read straight from the [nb][M] / [nb][N] tensors, no LDS.  One grouped launch over a table of
// descriptors, one wave per (32 x 32 tile, slab of BP_SLAB rows of the batch).  Rows past nb (nb odd, nb = 1, a ragged last slab)
// and rows / columns past M / N enter as zeros.  An output element accumulates only its own row of A and column of Bm, in k order:
// float32 within a slab in the matrix core's fixed order, then bp_sum_regions adds the slabs in ascending order in float64.  The
// slab length is a constant, so neither the grid, the tiling nor the run changes a bit.  No atomics.
// The sources are separate translation units without relocatable device code, so the product is a kernel TEMPLATE over the
// caller's table type: count() descriptors, desc(i) the i-th, both usable on the host (to count tiles) and in the wave.
#pragma once
#include "common.h"

namespace admmnet {

constexpr int BP_SLAB = 128;              // rows of the batch summed in float32 by one wave
constexpr int BP_UNROLL = 8;              // k steps (pairs of rows) whose operands are loaded ahead of their MFMAs

__host__ __device__ inline int64_t bp_slabs(int64_t nb) { return (nb + BP_SLAB - 1) / BP_SLAB; }

struct BpDesc {
    const float *A, *Bm;     // A[b * lda + m], Bm[b * ldb + n * cs]
    int M, N, lda, ldb, cs, ldc;
    int64_t nb;              // rows of the batch
    int64_t off, boff;       // C [M][ldc] and the bias [M] (column N, a column of ones; boff < 0: none) in a partial row
    float *part;             // [bp_slabs(nb)][pstride]
    int64_t pstride;
    __host__ __device__ int tiles() const { return ((M + 31) / 32) * ((N + (boff >= 0 ? 1 : 0) + 31) / 32); }
};

template <class Table>
static int64_t bp_tiles(const Table &tab) {
    int64_t n = 0;
    for (int i = 0; i < tab.count(); ++i) n += tab.desc(i).tiles();
    return n;
}

// grid (bp_tiles, slabs of the longest batch), one wave each
template <class Table>
__global__ __launch_bounds__(64) void bp_kernel(Table tab) {
    int tile = blockIdx.x, i = 0;
    const int n = tab.count();
    BpDesc d = tab.desc(0);
    for (; i + 1 < n && tile >= d.tiles(); d = tab.desc(i)) tile -= d.tiles(), ++i;
    const int64_t b0 = (int64_t)blockIdx.y * BP_SLAB;
    if (b0 >= d.nb) return;
    const int64_t b1 = b0 + BP_SLAB < d.nb ? b0 + BP_SLAB : d.nb;
    const int ne = d.N + (d.boff >= 0 ? 1 : 0), tn = (ne + 31) / 32;
    const int m0 = 32 * (tile / tn), n0 = 32 * (tile % tn);
    const int lane = threadIdx.x, r32 = lane & 31, kh = lane >> 5;
    const bool mv = m0 + r32 < d.M, nv = n0 + r32 < d.N, ones = d.boff >= 0 && n0 + r32 == d.N;
    const float *ap = d.A + (mv ? m0 + r32 : 0);
    const float *bp = d.Bm + (nv ? (int64_t)(n0 + r32) * d.cs : 0);
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
            x[u] = ap[bb * d.lda];
            y[u] = bp[bb * d.ldb];
            if (!(bv && mv)) x[u] = 0.f;
            if (ones) y[u] = 1.f;
            if (!(bv && (nv || ones))) y[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < BP_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], y[u], acc, 0, 0, 0);
    }
    // C/D layout: column = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
    float *out = d.part + (int64_t)blockIdx.y * d.pstride;
    const int gn = n0 + r32;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int gm = m0 + (q & 3) + 8 * (q >> 2) + 4 * kh;
        if (gm >= d.M) continue;
        if (gn < d.N) out[d.off + (int64_t)gm * d.ldc + gn] = acc[q];
        else if (gn == d.N && d.boff >= 0) out[d.boff + gm] = acc[q];
    }
}

// out[o0 + e (+ shift where e >= cut)] = sum over the slabs of part[slab][e], ascending, in float64; e counts through r0, then r1
// (total = 0: no such region).  The caller's kernel gives thread e; TS_THREADS elements per workgroup.
struct BpRegion {
    const float *part;
    int64_t total, slabs, o0, cut, shift;
};
__device__ __forceinline__ void bp_sum_regions(int64_t e, const BpRegion &r0, const BpRegion &r1, float *__restrict__ out) {
    BpRegion r = r0;
    if (e >= r0.total) e -= r0.total, r = r1;
    if (e >= r.total) return;
    double a = 0.0;
    for (int64_t s = 0; s < r.slabs; ++s) a += (double)r.part[s * r.total + e];
    out[r.o0 + e + (e >= r.cut ? r.shift : 0)] = (float)a;
}

}  // namespace admmnet
