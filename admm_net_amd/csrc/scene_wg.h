// scene_wg.h -- the workgroup plumbing of the "one scene per workgroup" float64 kernels (refine.hip, order.hip, cfar.hip,
// cfar_relax.hip), each defined ONCE:
//     ScenePar                  how a workgroup shares a loop -- the `Par` the *_core.h scene loops are written over.  The order
//                               of its sums is what "a scene's bits depend on neither B, nor its place, nor its neighbours" rests
//                               on; tests/host_model/host_par.h is the same order on the host
//     LdsCarver                 the dynamic LDS of a scene laid out array by array: a kernel file names its arrays once, in a
//                               *_carve function that serves the kernel (the pointers) and the host (the byte count)
//     scene_state_counts_kernel the batch counts of `status`, added from the state column of `info` by one workgroup
//     launch_scenes             B workgroups of a scene kernel, then the counts
#pragma once
#include "common.h"
#include "batch_sums.h"

namespace admmnet {

constexpr int64_t SCENE_LDS_LIMIT = 160 * 1024;

// each: items dealt to the threads with a barrier behind them.  sum: a thread adds its items in index order, a butterfly adds the
// lanes of a wave, the waves are added in wave order.  sums<N>: N such sums in one pass and one barrier pair.  best: the item of
// greatest value -- a thread keeps its best in index order, a butterfly takes the better of two lanes, the waves are compared in
// wave order; a tie goes to the smaller index at every stage.  No atomics.
template <int THREADS, int MAXSUMS = 1>
struct ScenePar {
    static constexpr int WAVES = THREADS / 64;
    double *red;   // [WAVES * MAXSUMS]
    int *arg;      // [WAVES]; null in a kernel without best

    template <class F>
    __device__ __forceinline__ void each(int count, F fn) {
        for (int item = threadIdx.x; item < count; item += THREADS) fn(item);
        __syncthreads();
    }

    template <class F>
    __device__ __forceinline__ double sum(int count, F fn) {
        double v = 0.0;
        for (int item = threadIdx.x; item < count; item += THREADS) v += fn(item);
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double total = red[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) total += red[w];
        __syncthreads();
        return total;
    }

    template <int N, class F>
    __device__ __forceinline__ void sums(int count, F fn, double (&out)[N]) {
        static_assert(N <= MAXSUMS, "red holds MAXSUMS sums per wave");
        double v[N];
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = 0.0;
        for (int item = threadIdx.x; item < count; item += THREADS) fn(item, v);
#pragma unroll
        for (int n = 0; n < N; ++n) {
            v[n] = wave_sum(v[n]);
            if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * N + n] = v[n];
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < N; ++n) {
            double total = red[n];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) total += red[w * N + n];
            out[n] = total;
        }
        __syncthreads();
    }

    // (value, item) `o` is better than `b`: higher, or as high with the smaller item
    static __device__ __forceinline__ bool better(double ov, int oi, double bv, int bi) { return ov > bv || (ov == bv && oi < bi); }

    template <class F>
    __device__ __forceinline__ int best(int count, F fn) {
        double bv = -1.0;
        int bi = -1;
        for (int item = threadIdx.x; item < count; item += THREADS) {
            const double v = fn(item);
            if (v > bv) {
                bv = v;
                bi = item;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6] = bv;
            arg[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        bv = red[0];
        bi = arg[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
            if (better(red[w], arg[w], bv, bi)) {
                bv = red[w];
                bi = arg[w];
            }
        __syncthreads();
        return bv >= 0.0 ? bi : -1;
    }
};

// The arrays of a scene behind one another in its dynamic LDS, each 16-byte aligned.  In the kernel `base` is the extern __shared__
// array; on the host it is null, every pointer is its offset and only `at`, the bytes taken, is read.
struct LdsCarver {
    char *base;
    size_t at = 0;
    template <class T>
    __host__ __device__ T *take(size_t count) {
        T *p = reinterpret_cast<T *>(base + at);
        at += (count * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
};

// the states counted into status[0 .. STATES), passed by value
template <int STATES>
struct SceneStates {
    int state[STATES];
};

// status[c] = the scenes whose info[col] is states.state[c]; the counts are whole numbers, exact in float64 in any order
template <int STATES>
__global__ __launch_bounds__(SC_FIN_THREADS) void scene_state_counts_kernel(int64_t B, const double *__restrict__ info, int stride,
                                                                            int col, SceneStates<STATES> states,
                                                                            int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_THREADS];
    for (int c = 0; c < STATES; ++c) {
        double n = 0.0;
        for (int64_t r = threadIdx.x; r < B; r += SC_FIN_THREADS) n += info[r * stride + col] == (double)states.state[c] ? 1.0 : 0.0;
        sh[threadIdx.x] = n;
        __syncthreads();
        for (int o = SC_FIN_THREADS >> 1; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) status[c] = sc_count(sh[0]);
        __syncthreads();
    }
}

template <int STATES>
int launch_scene_state_counts(int64_t B, const double *info, int stride, int col, SceneStates<STATES> states, int32_t *status,
                              hipStream_t st) {
    hipLaunchKernelGGL(scene_state_counts_kernel<STATES>, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, info, stride, col, states, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// B workgroups of THREADS run `kernel(args...)`, a scene each, on `lds` bytes of dynamic LDS (allowed above 64 KiB first); then the
// states of column `col` of their `info` rows of `stride` are counted into `status`
template <int THREADS, int STATES, class... Params, class... Args>
int launch_scenes(void (*kernel)(Params...), size_t lds, int64_t B, hipStream_t st, const double *info, int stride, int col,
                  SceneStates<STATES> states, int32_t *status, Args... args) {
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(THREADS), lds, st, args...);
    ADMM_HIP(hipGetLastError());
    return launch_scene_state_counts(B, info, stride, col, states, status, st);
}

}  // namespace admmnet
