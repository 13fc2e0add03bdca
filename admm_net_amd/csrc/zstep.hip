// zstep.hip -- K5: batch-coupled adaptive dual step of the Z layer.
//   r_b / (mean_b r + eps) -> MLP 3 -> 32 -> 1 -> sigmoid -> 0.5 + 1.5 s -> * softplus(rho)
//   /root/reference/admm_net.py:443-474 (ZLayer._compute_adaptive_step).
// The batch mean is the only cross-signal (and cross-GPU) coupling of the whole
// forward: the local sum is produced in fp64 by one deterministic workgroup and
// the caller may all-reduce it before the step kernel runs.
#include "common.h"
#include "batch_sums.h"

namespace admmnet {

__global__ __launch_bounds__(1024) void rn_sum_kernel(int64_t B, const float *__restrict__ rn,
                                                      double *__restrict__ sum) {
    __shared__ double sh[1024];
    colsum<1, 1024>(B, rn, sh);
    if (threadIdx.x == 0) {
        sum[0] = sh[0];
        sum[1] = (double)B;   // (the pair the sharded protocol all-reduces: local sum, local count)
    }
}

__global__ void mean_kernel(const double *__restrict__ sum, int64_t B, float *__restrict__ mean) {
    if (threadIdx.x == 0 && blockIdx.x == 0) mean[0] = (float)(sum[0] / (double)B);
}

// alpha[i] from signal i's rn and the mean of its group: the one body of zstep_kernel and zstep_group_kernel
__device__ __forceinline__ void zstep_at(int D, int64_t i, const float *__restrict__ lw, const float *__restrict__ rn, float mean,
                                         float *__restrict__ alpha) {
    const LayerLayout L{D};
    const float *rs = lw + L.off_rs();   // W1[32][3] b1[32] w2[32] b2[1]
    const float rho = lw[S_RHO_Z];
    const float f0 = lw[S_KNORM], f1 = rho, f2 = rn[i] / (mean + kEpsRef);
    float acc = rs[160];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        float hj = rs[96 + j];
        hj = fmaf(rs[3 * j + 0], f0, hj);
        hj = fmaf(rs[3 * j + 1], f1, hj);
        hj = fmaf(rs[3 * j + 2], f2, hj);
        acc = fmaf(rs[128 + j], fmaxf(hj, 0.f), acc);
    }
    const float sf = 0.5f + 1.5f * sigmoid_f(acc);
    alpha[i] = rho * sf;
}

__global__ __launch_bounds__(256) void zstep_kernel(int D, int64_t B, const float *__restrict__ lw,
                                                    const float *__restrict__ rn,
                                                    const float *__restrict__ mean,
                                                    float *__restrict__ alpha) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < B) zstep_at(D, i, lw, rn, mean[0], alpha);
}

int launch_rn_sum(int64_t B, const float *rn, double *sum, hipStream_t st) {
    hipLaunchKernelGGL(rn_sum_kernel, dim3(1), dim3(1024), 0, st, B, rn, sum);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

__global__ void mean_pair_kernel(const double *__restrict__ sc, float *__restrict__ mean) {
    if (threadIdx.x == 0 && blockIdx.x == 0) mean[0] = (float)(sc[0] / sc[1]);
}

int launch_mean_from_pair(const double *sum_count, float *mean, hipStream_t st) {
    hipLaunchKernelGGL(mean_pair_kernel, dim3(1), dim3(64), 0, st, sum_count, mean);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_mean_from_sum(const double *sum, int64_t B, float *mean, hipStream_t st) {
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(64), 0, st, sum, B, mean);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_zstep(const float *lw, int D, int64_t B, const float *rn, const float *mean, float *alpha,
                 hipStream_t st) {
    ProfScope _prof(KC_ZSTEP, st);
    if (B <= 0) return ADMMNET_OK;
    hipLaunchKernelGGL(zstep_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, D, B, lw, rn, mean,
                       alpha);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// ---- sub-batches (admmnet_cfg.sub_batch = g > 0) ----------------------------------------------------------------------
// Group j is the signals [j g, min((j + 1) g, B)) and steps with its own mean.  Its (sum, count) pair must carry the bits
// that rn_sum_kernel gives a separate call of that group: thread t sums rn[t], rn[t + 1024], ... from 0.0, then a tree
// halves 1024 slots.  For a group of r <= P <= 1024 signals (P a power of two) the slots t >= r hold 0.0 and rn >= 0, so
// every tree level above P adds exact zeros: a P-slot tree in the same pairing order gives the same bits.  Groups of more
// than 1024 signals take P = 1024 with rn_sum_kernel's stride.  No atomics; blockDim / P groups per workgroup.
__global__ __launch_bounds__(1024) void rn_group_sum_kernel(int64_t B, int64_t g, int P, int64_t ngroups,
                                                            const float *__restrict__ rn, double *__restrict__ pairs) {
    __shared__ double sh[1024];
    const int t = threadIdx.x, lane = t & (P - 1);
    const int64_t j = (int64_t)blockIdx.x * (blockDim.x / P) + t / P, s = j * g;
    const int64_t r = j < ngroups ? ((B - s < g) ? B - s : g) : 0;
    double a = 0.0;
    for (int64_t i = lane; i < r; i += P) a += (double)rn[s + i];
    sh[t] = a;
    __syncthreads();
    for (int o = P >> 1; o > 0; o >>= 1) {
        if (lane < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (lane == 0 && j < ngroups) {
        pairs[2 * j] = sh[t];
        pairs[2 * j + 1] = (double)r;
    }
}

int launch_rn_group_sum(int64_t B, int64_t g, const float *rn, double *pairs, hipStream_t st) {
    const int64_t ngroups = (B + g - 1) / g;
    int P = 1;
    while (P < 1024 && P < g) P <<= 1;
    const int threads = P > 256 ? P : 256;
    const int64_t blocks = (ngroups + threads / P - 1) / (threads / P);
    hipLaunchKernelGGL(rn_group_sum_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, B, g, P, ngroups, rn, pairs);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// mean[j] = pairs[2j] / pairs[2j + 1]: mean_pair_kernel for every group
__global__ void mean_pairs_kernel(const double *__restrict__ sc, int64_t ngroups, float *__restrict__ mean) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ngroups) mean[j] = (float)(sc[2 * j] / sc[2 * j + 1]);
}

int launch_mean_from_pairs(const double *pairs, int64_t ngroups, float *mean, hipStream_t st) {
    hipLaunchKernelGGL(mean_pairs_kernel, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, st, pairs, ngroups, mean);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

// zstep_kernel with the mean of signal i's group; a call without sub-batches keeps zstep_kernel, which reads mean[0] and divides
// nothing
__global__ __launch_bounds__(256) void zstep_group_kernel(int D, int64_t B, int64_t g, const float *__restrict__ lw,
                                                          const float *__restrict__ rn, const float *__restrict__ mean,
                                                          float *__restrict__ alpha) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < B) zstep_at(D, i, lw, rn, mean[i / g], alpha);
}

int launch_zstep_groups(const float *lw, int D, int64_t B, int64_t g, const float *rn, const float *mean, float *alpha,
                        hipStream_t st) {
    ProfScope _prof(KC_ZSTEP, st);
    if (B <= 0) return ADMMNET_OK;
    hipLaunchKernelGGL(zstep_group_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, D, B, g, lw, rn, mean,
                       alpha);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
