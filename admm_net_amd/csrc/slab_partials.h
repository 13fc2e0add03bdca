// slab_partials.h -- the launch shape of the per-signal training kernels (train_small.hip, loss.hip): one wave per signal, a
// 256-thread workgroup takes a slab of four consecutive signals and leaves one row of partial sums for the batch.
#pragma once
#include "common.h"

namespace admmnet {

constexpr int TS_THREADS = 256;
constexpr int TS_SLAB = TS_THREADS / 64;   // signals per workgroup, one per wave

// v[0 .. COUNT) hold wave sums (the same value in every lane): adds the slab's waves in wave order into row blockIdx.x of part.
// Every thread of the workgroup must call it.
template <int COUNT>
__device__ __forceinline__ void ts_slab_partials(const float (&v)[COUNT], float *sh, float *__restrict__ part) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < COUNT; ++c) sh[wave * COUNT + c] = v[c];
    }
    __syncthreads();
    if ((int)threadIdx.x < COUNT) {
        float s = 0.f;
        for (int w = 0; w < TS_SLAB; ++w) s += sh[w * COUNT + threadIdx.x];
        part[(int64_t)blockIdx.x * COUNT + threadIdx.x] = s;
    }
}

}  // namespace admmnet
