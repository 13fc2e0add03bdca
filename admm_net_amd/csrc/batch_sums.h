// batch_sums.h -- float64 sums over a batch in a fixed order, without atomics (score.hip, crb.hip): every workgroup leaves one row
// of partial sums, ONE workgroup adds the rows, so two runs give the same bits whatever the scheduling.
#pragma once
#include "common.h"
#include "slab_partials.h"

namespace admmnet {

constexpr int SC_FIN_THREADS = 1024;
constexpr int SC_FIN_SLICES = 64;             // row slices of the finishing sum per column

__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ts_slab_partials in float64
template <int COUNT>
__device__ __forceinline__ void sc_slab_partials(const double (&v)[COUNT], double *sh, double *__restrict__ part) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < COUNT; ++c) sh[wave * COUNT + c] = v[c];
    }
    __syncthreads();
    if ((int)threadIdx.x < COUNT) {
        double s = 0.0;
        for (int w = 0; w < TS_SLAB; ++w) s += sh[w * COUNT + threadIdx.x];
        part[(int64_t)blockIdx.x * COUNT + threadIdx.x] = s;
    }
}

// column sums of part [rows][COLS], fixed order (la_colsum's scheme): thread (c, s) adds the rows s, s + NS, ..., a tree halves
// the NS slices; the sums are left in sh[0 .. COLS).  One workgroup, every thread calls it.
template <int COLS>
__device__ __forceinline__ void sc_colsum(int64_t rows, const double *__restrict__ part, double *sh) {
    constexpr int NS = SC_FIN_SLICES;
    const int c = threadIdx.x % COLS, s = threadIdx.x / COLS;
    const bool live = s < NS;
    double a = 0.0;
    if (live)
        for (int64_t r = s; r < rows; r += NS) a += part[r * COLS + c];
    if (live) sh[s * COLS + c] = a;
    __syncthreads();
    for (int o = NS >> 1; o > 0; o >>= 1) {
        if (live && s < o) sh[s * COLS + c] += sh[(s + o) * COLS + c];
        __syncthreads();
    }
}

__device__ __forceinline__ int32_t sc_count(double v) { return (int32_t)fmin(v, 2147483647.0); }   // exact in float64; saturates

}  // namespace admmnet
