// batch_sums.h -- sums over a batch in a fixed order, without atomics, for the training and evaluation kernels: every workgroup
// leaves one row of partial sums, ONE workgroup adds the rows in float64 (colsum), so two runs give the same bits whatever the
// scheduling.  The order of the additions is fixed by what each caller chooses: its slice count NS, its workgroup size and the
// epilogue it applies to the sums.
#pragma once
#include "common.h"
#include "slab_partials.h"

namespace admmnet {

constexpr int SC_FIN_THREADS = 1024;
constexpr int SC_FIN_SLICES = 64;             // row slices of the finishing sum per column (score.hip, crb.hip, loss_set.hip)

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

// THE fixed-order column sum: sh[c] = sum over r < rows of part[r * stride + c] in float64, c < cols.  Thread (c, s) =
// (t % cols, t / cols) adds the rows s, s + ns, ... from 0.0, then a tree halves the ns slices (ns a power of two, cols ns <= the
// workgroup's size, sh holds cols ns doubles).  One workgroup, every thread calls it; every thread may read sh[0 .. cols) after it.
template <typename T>
__device__ __forceinline__ void colsum(int cols, int ns, int64_t rows, int64_t stride, const T *__restrict__ part, double *sh) {
    const int c = threadIdx.x % cols, s = threadIdx.x / cols;
    const bool live = s < ns;
    double a = 0.0;
    if (live)
        for (int64_t r = s; r < rows; r += ns) a += (double)part[r * stride + c];
    if (live) sh[s * cols + c] = a;
    __syncthreads();
    for (int o = ns >> 1; o > 0; o >>= 1) {
        if (live && s < o) sh[s * cols + c] += sh[(s + o) * cols + c];
        __syncthreads();
    }
}
// the same with the counts known to the compiler and dense rows; COLS = 1, NS = the workgroup's size sums one array
template <int COLS, int NS, typename T>
__device__ __forceinline__ void colsum(int64_t rows, const T *__restrict__ part, double *sh) {
    static_assert(NS > 0 && (NS & (NS - 1)) == 0, "the tree halves the slices");
    colsum(COLS, NS, rows, COLS, part, sh);
}

// sum over the workgroup's WAVES waves in a fixed order: the butterfly, then the waves' sums serially from sh [WAVES].  Every
// thread must call it; the result is valid in thread 0, with ALL in every thread.
template <int WAVES, bool ALL>
__device__ __forceinline__ float block_sum(float x, float *sh) {
    x = wave_sum(x);
    __syncthreads();   // (sh may still be read from a previous sum)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    float s = 0.f;
    if (ALL || threadIdx.x == 0)
        for (int w = 0; w < WAVES; ++w) s += sh[w];
    return s;
}

__device__ __forceinline__ int32_t sc_count(double v) { return (int32_t)fmin(v, 2147483647.0); }   // exact in float64; saturates

}  // namespace admmnet
