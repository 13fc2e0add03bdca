// optim.hip -- AdamW and gradient-norm clipping over a LIST of float32 tensors (admm_net_amd/optim.py; the tensor stand-in there
// is the definition the tests hold these kernels to).  What a training loop writes as
//     torch.nn.utils.clip_grad_norm_(params, max_norm);  optimizer.step()          # optim.AdamW
// is here  op_sqnorm_kernel -> op_finish_kernel -> op_adamw_kernel (or op_scale_kernel when the clipping stands alone).
//
// Tensor list.  A launch carries its part of the list BY VALUE in the kernel arguments (as train_head.hip carries HeadPtrs): base
// pointers, the running count of blocks and the size of each tensor's last block.  Nothing lives in a device-side table, so no
// host buffer has a lifetime.  The host cuts a longer list into consecutive launches of OP_LIST_T (norm, scale), OP_ADAM_T
// (update) or OP_BUCKET_T (pack, unpack: a tensor takes two of the OP_LIST_T pointers) list positions.
//
// Work.  A block is OP_BLOCK consecutive elements of ONE tensor, one workgroup of OP_THREADS threads, thread t owning the elements
// 4 t .. 4 t + 3 of the block.  A tensor of n elements has ceil(n / OP_BLOCK) blocks (none for n = 0: such a tensor only takes a
// list position) and the blocks of the list are numbered in list order, so the partition -- and with it the order of every sum
// -- depends on the list alone, never on where it was cut into launches.  A workgroup finds its tensor by a binary search of
// the running block counts (uniform: scalar loads from the argument segment).
//
// Accesses.  One 16-byte access per thread where every pointer of the tensor is 16-byte aligned and its element count is a
// multiple of four; four 4-byte accesses of the same elements otherwise (views at odd offsets).  The same thread owns the same
// elements either way, so the bits of the norm do not depend on the alignment.
//
// Sums.  Squares and sums in float64: in-lane in element order, the xor butterfly across the wave (offsets 32 .. 1, the float64
// wave_sum of common.h), the four waves serially from LDS, one double per block; op_finish_kernel (one workgroup) adds the blocks
// in the fixed order of colsum (batch_sums.h).  No atomics: every run gives the same bits.
//
// Rounding.  The file is compiled with floating-point contraction OFF (the pragma below): every product, sum, quotient and root
// is rounded to its type on its own, and a multiply-add is fused only where fmaf is written.  (The __fmul_rn family is no tool
// for this here: the toolchain's headers define __fmul_rn(x, y) as x * y, which the default contraction mode may still fuse
// into a following sum, and __fsqrt_rn as the native, not correctly rounded, root.)  sqrtf and / are the compiler's correctly
// rounded defaults; no fast-math flag is given.
#include "common.h"
#include "batch_sums.h"

#pragma clang fp contract(off)

namespace admmnet {

constexpr int OP_BLOCK = 1024, OP_THREADS = 256, OP_WAVES = OP_THREADS / 64;
constexpr int OP_LIST_T = 256;    // list positions per launch of the norm and scale passes
constexpr int OP_ADAM_T = 64;     // ... of the update
constexpr int OP_HYPER = 8;       // hyper-parameter sets per launch of the update
constexpr unsigned OP_VEC = 0x8000u;   // tail bit: the 16-byte path
static_assert(OP_BLOCK == 4 * OP_THREADS, "a thread owns four consecutive elements");
static_assert(OP_BLOCK < (int)OP_VEC, "the last block's size shares 16 bits with the vector flag");

// end[i]: blocks of the launch's tensors 0 .. i; tail[i]: elements of tensor i's last block (1 .. OP_BLOCK) | OP_VEC
struct OpListArgs {
    float *g[OP_LIST_T];
    uint32_t end[OP_LIST_T];
    uint16_t tail[OP_LIST_T];
    double *partials;      // sqnorm: one double per block of this launch
    const float *coef;     // scale
    int32_t count;
};
static_assert(sizeof(OpListArgs) <= 4096, "the kernel argument segment holds 4 KiB");

struct OpHyper {
    float decay, omb1, beta2, omb2, step_size, bc2s, eps;   // 1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t)
};

struct OpAdamArgs {
    float *p[OP_ADAM_T];
    const float *g[OP_ADAM_T];
    float *m[OP_ADAM_T];
    float *v[OP_ADAM_T];
    uint32_t end[OP_ADAM_T];
    uint16_t tail[OP_ADAM_T];
    uint8_t hyper[OP_ADAM_T];
    OpHyper h[OP_HYPER];
    const float *coef;     // nullptr: the gradients are used as they are
    int32_t count;
};
static_assert(sizeof(OpAdamArgs) <= 4096, "the kernel argument segment holds 4 KiB");

// the tensor of block blk (the first i with end[i] > blk), the block's offset in it and its element count
struct OpSpan {
    int i, cnt;
    int64_t off;
    bool vec;
};
__device__ __forceinline__ OpSpan op_locate(const uint32_t *end, const uint16_t *tail, int count, uint32_t blk) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (end[mid] > blk) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t first = lo > 0 ? end[lo - 1] : 0u, t = tail[lo];
    OpSpan s;
    s.i = lo;
    s.off = (int64_t)(blk - first) * OP_BLOCK;
    s.cnt = blk + 1 == end[lo] ? (int)(t & (OP_VEC - 1)) : OP_BLOCK;
    s.vec = (t & OP_VEC) != 0;
    return s;
}

// a thread's four elements (zeros past the block's end) and back
__device__ __forceinline__ void op_load4(const float *__restrict__ x, int e, const OpSpan &s, float (&r)[4]) {
    if (s.vec) {
        const float4 q = e < s.cnt ? *reinterpret_cast<const float4 *>(x + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = e + j < s.cnt ? x[e + j] : 0.f;
    }
}
__device__ __forceinline__ void op_store4(float *__restrict__ x, int e, const OpSpan &s, const float (&r)[4]) {
    if (s.vec) {
        if (e < s.cnt) *reinterpret_cast<float4 *>(x + e) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < s.cnt) x[e + j] = r[j];
    }
}

// ---- the norm ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OP_THREADS) void op_sqnorm_kernel(OpListArgs a) {
    __shared__ double sh[OP_WAVES];
    const OpSpan s = op_locate(a.end, a.tail, a.count, blockIdx.x);
    float x[4];
    op_load4(a.g[s.i] + s.off, 4 * (int)threadIdx.x, s, x);
    double acc = (double)x[0] * (double)x[0];                 // (a float's square is exact in float64)
#pragma unroll
    for (int j = 1; j < 4; ++j) acc += (double)x[j] * (double)x[j];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
#pragma unroll
        for (int w = 1; w < OP_WAVES; ++w) t += sh[w];
        a.partials[blockIdx.x] = t;
    }
}

// sumsq = the blocks' sums added in a fixed order (colsum of batch_sums.h: one column, a slice per thread);
// total_norm = (float) sqrt(sumsq); coef = clamp(max_norm / (total_norm + 1e-6), max = 1) as torch evaluates it in float32:
// `number / tensor` is reciprocal(tensor) * number there, and clamp keeps a NaN (an infinite norm gives 1 / inf = 0)
__global__ __launch_bounds__(OP_THREADS) void op_finish_kernel(int64_t rows, const double *__restrict__ partials, float max_norm,
                                                               double *__restrict__ sumsq, float *__restrict__ total_norm,
                                                               float *__restrict__ coef) {
    __shared__ double sh[OP_THREADS];
    colsum<1, OP_THREADS>(rows, partials, sh);
    if (threadIdx.x == 0) {
        const double ss = sh[0];
        const float nrm = (float)sqrt(ss);
        const float c = (1.f / (nrm + 1e-6f)) * max_norm;
        sumsq[0] = ss;
        total_norm[0] = nrm;
        coef[0] = c > 1.f ? 1.f : c;
    }
}

// g <- g coef, always (torch multiplies by a coefficient of 1 too)
__global__ __launch_bounds__(OP_THREADS) void op_scale_kernel(OpListArgs a) {
    const OpSpan s = op_locate(a.end, a.tail, a.count, blockIdx.x);
    const float c = a.coef[0];
    const int e = 4 * (int)threadIdx.x;
    float *g = a.g[s.i] + s.off;
    float x[4];
    op_load4(g, e, s, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = x[j] * c;
    op_store4(g, e, s, x);
}

// ---- the bucket --------------------------------------------------------------------------------------------------------------
// pack / unpack: the list's tensors, in list order, to and from ONE contiguous buffer (the bucket of a gradient all-reduce or a
// parameter broadcast).  A launch carries OP_BUCKET_T tensors in the same by-value list: g[i] the tensor, g[OP_BUCKET_T + i] its
// place in the flat buffer; the vector flag asks both to be 16-byte aligned.
constexpr int OP_BUCKET_T = OP_LIST_T / 2;

template <bool TO_FLAT>
__global__ __launch_bounds__(OP_THREADS) void op_bucket_kernel(OpListArgs a) {
    const OpSpan s = op_locate(a.end, a.tail, a.count, blockIdx.x);
    const int e = 4 * (int)threadIdx.x;
    float *t = a.g[s.i] + s.off, *f = a.g[OP_BUCKET_T + s.i] + s.off;
    float x[4];
    op_load4(TO_FLAT ? t : f, e, s, x);
    op_store4(TO_FLAT ? f : t, e, s, x);
}

// ---- the update --------------------------------------------------------------------------------------------------------------
// torch.optim.adam._single_tensor_adam (decoupled weight decay, not capturable), every operation rounded to float32 on its own
// except the three multiply-adds marked fma:
//   p <- p (1 - lr wd);  m <- m + (g - m)(1 - beta1)  [fma];  v <- beta2 v + ((1 - beta2) g) g  [fma];
//   denom = sqrt(v) / bc2s + eps;  p <- p - step_size (m / denom)  [fma]
// with g <- g coef rounded first when a coefficient is given: op_scale_kernel followed by this kernel without one gives the same bits.
__global__ __launch_bounds__(OP_THREADS) void op_adamw_kernel(OpAdamArgs a) {
    const OpSpan s = op_locate(a.end, a.tail, a.count, blockIdx.x);
    const OpHyper h = a.h[a.hyper[s.i]];
    const bool clip = a.coef != nullptr;
    const float c = clip ? a.coef[0] : 1.f;
    const int e = 4 * (int)threadIdx.x;
    float *pp = a.p[s.i] + s.off, *pm = a.m[s.i] + s.off, *pv = a.v[s.i] + s.off;
    float p[4], g[4], m[4], v[4];
    op_load4(pp, e, s, p);
    op_load4(a.g[s.i] + s.off, e, s, g);
    op_load4(pm, e, s, m);
    op_load4(pv, e, s, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gs = clip ? g[j] * c : g[j];      // rounded here: contraction is off
        const float pd = p[j] * h.decay;
        m[j] = fmaf(gs - m[j], h.omb1, m[j]);
        v[j] = fmaf(h.omb2 * gs, gs, h.beta2 * v[j]);
        const float denom = sqrtf(v[j]) / h.bc2s + h.eps;
        p[j] = fmaf(-h.step_size, m[j] / denom, pd);
    }
    op_store4(pp, e, s, p);
    op_store4(pm, e, s, m);
    op_store4(pv, e, s, v);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static inline int64_t op_blocks(int64_t n) { return (n + OP_BLOCK - 1) / OP_BLOCK; }

// the blocks of the whole list, or -1 when a count is negative or the total passes 2^31 - 1
int64_t optim_blocks(int count, const int64_t *numel) {
    int64_t total = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] < 0 || numel[i] > (int64_t)0x7fffffff * OP_BLOCK) return -1;
        total += op_blocks(numel[i]);
        if (total > 0x7fffffffLL) return -1;
    }
    return total;
}

static inline uint16_t op_tail(int64_t n, bool vec) {
    return (uint16_t)((n > 0 ? (unsigned)(n - (op_blocks(n) - 1) * OP_BLOCK) : 0u) | (vec && n % 4 == 0 ? OP_VEC : 0u));
}
static inline bool op_aligned(const void *p) { return ((uintptr_t)p & 15u) == 0; }

#define OP_LAUNCH(kernel, grid, ...)                                                                \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(OP_THREADS), 0, st, __VA_ARGS__);       \
    ADMM_HIP(hipGetLastError())

// the list in launches of OP_LIST_T positions: the norm's partials when `partials`, the scaling otherwise
static int op_list_pass(int count, float *const *grads, const int64_t *numel, double *partials, const float *coef, hipStream_t st) {
    int64_t base = 0;
    for (int first = 0; first < count; first += OP_LIST_T) {
        OpListArgs a = {};
        a.count = count - first < OP_LIST_T ? count - first : OP_LIST_T;
        uint32_t blocks = 0;
        for (int i = 0; i < a.count; ++i) {
            const int64_t n = numel[first + i];
            a.g[i] = grads[first + i];
            blocks += (uint32_t)op_blocks(n);
            a.end[i] = blocks;
            a.tail[i] = op_tail(n, op_aligned(a.g[i]));
        }
        a.partials = partials ? partials + base : nullptr;
        a.coef = coef;
        base += blocks;
        if (!blocks) continue;
        if (partials) {
            OP_LAUNCH(op_sqnorm_kernel, blocks, a);
        } else {
            OP_LAUNCH(op_scale_kernel, blocks, a);
        }
    }
    return ADMMNET_OK;
}

int launch_optim_gradnorm(int count, const float *const *grads, const int64_t *numel, float max_norm, double *partials,
                          double *sumsq, float *total_norm, float *coef, hipStream_t st) {
    if (int rc = op_list_pass(count, const_cast<float *const *>(grads), numel, partials, nullptr, st)) return rc;
    OP_LAUNCH(op_finish_kernel, 1, optim_blocks(count, numel), partials, max_norm, sumsq, total_norm, coef);
    return ADMMNET_OK;
}

int launch_optim_scale(int count, float *const *grads, const int64_t *numel, const float *coef, hipStream_t st) {
    return op_list_pass(count, grads, numel, nullptr, coef, st);
}

int launch_optim_bucket(int count, float *const *tensors, const int64_t *numel, float *flat, bool to_flat, hipStream_t st) {
    int64_t off = 0;
    for (int first = 0; first < count; first += OP_BUCKET_T) {
        OpListArgs a = {};
        a.count = count - first < OP_BUCKET_T ? count - first : OP_BUCKET_T;
        uint32_t blocks = 0;
        for (int i = 0; i < a.count; ++i) {
            const int64_t n = numel[first + i];
            a.g[i] = tensors[first + i];
            a.g[OP_BUCKET_T + i] = flat + off;
            blocks += (uint32_t)op_blocks(n);
            a.end[i] = blocks;
            a.tail[i] = op_tail(n, op_aligned(a.g[i]) && op_aligned(flat + off));
            off += n;
        }
        if (!blocks) continue;
        if (to_flat) {
            OP_LAUNCH(op_bucket_kernel<true>, blocks, a);
        } else {
            OP_LAUNCH(op_bucket_kernel<false>, blocks, a);
        }
    }
    return ADMMNET_OK;
}

// a launch ends after OP_ADAM_T list positions or before the tensor that would need a ninth hyper-parameter set
int launch_optim_adamw(int count, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                       const int64_t *numel, const int32_t *hyper_index, const admmnet_adamw_hyper *hyper, const float *coef,
                       hipStream_t st) {
    int first = 0;
    while (first < count) {
        OpAdamArgs a = {};
        int32_t set[OP_HYPER];
        int nset = 0, n = 0;
        uint32_t blocks = 0;
        for (; first + n < count && n < OP_ADAM_T; ++n) {
            const int t = first + n;
            int k = 0;
            while (k < nset && set[k] != hyper_index[t]) ++k;
            if (k == nset) {
                if (nset == OP_HYPER) break;
                const admmnet_adamw_hyper &src = hyper[hyper_index[t]];
                set[nset++] = hyper_index[t];
                a.h[k] = OpHyper{(float)src.decay, (float)src.one_minus_beta1, (float)src.beta2, (float)src.one_minus_beta2,
                                 (float)src.step_size, (float)src.bias_correction2_sqrt, (float)src.eps};
            }
            a.p[n] = params[t], a.g[n] = grads[t], a.m[n] = exp_avg[t], a.v[n] = exp_avg_sq[t];
            a.hyper[n] = (uint8_t)k;
            blocks += (uint32_t)op_blocks(numel[t]);
            a.end[n] = blocks;
            a.tail[n] = op_tail(numel[t], op_aligned(a.p[n]) && op_aligned(a.g[n]) && op_aligned(a.m[n]) && op_aligned(a.v[n]));
        }
        a.count = n;
        a.coef = coef;
        first += n;
        if (blocks) {
            OP_LAUNCH(op_adamw_kernel, blocks, a);
        }
    }
    return ADMMNET_OK;
}

}  // namespace admmnet
