// cfar_relax.hip -- successive cancellation with cyclic re-fitting on the periodogram of every scene (admm_net_amd/detect.py:
// cfar_relax; the definition is with admmnet_cfar_relax_f64 in include/admmnet.h, the float64 host statement is
// detect.cfar_relax_host).
//
// One scene per workgroup of CFAR_THREADS threads, one launch for the batch, as cfar.hip.  relax_core.h has the scene loop, written
// over cfar.hip's two ways a workgroup shares a loop and two more: N sums in one pass (the six complex moments of a Newton step:
// one pass over D and one barrier pair, not six), and the item of greatest value (the highest cell over the threshold) -- a thread
// keeps its best in index order, a butterfly takes the better of two lanes, the waves are compared in wave order; a tie goes to
// the smaller index at every stage.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.  y and b are
// read from HBM once; the residual, the intermediate image, the map, the tables and the targets stay in LDS (relax_layout).  The
// map is recomputed from the residual every round.  The batch counts of `status` are added from the state column of `info` by one
// workgroup in a second, tiny launch.
#include "common.h"
#include "batch_sums.h"
#include "relax_core.h"

namespace admmnet {

constexpr int64_t RELAX_LDS_LIMIT = 160 * 1024;
constexpr int RELAX_WAVES = CFAR_THREADS / 64;

struct RelaxPar {
    double *red;   // [RELAX_WAVES * RELAX_SUMS]
    int *arg;      // [RELAX_WAVES]

    template <class F>
    __device__ __forceinline__ void each(int count, F fn) {
        for (int item = threadIdx.x; item < count; item += CFAR_THREADS) fn(item);
        __syncthreads();
    }

    template <class F>
    __device__ __forceinline__ double sum(int count, F fn) {
        double v = 0.0;
        for (int item = threadIdx.x; item < count; item += CFAR_THREADS) v += fn(item);
        v = sc_wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double total = red[0];
#pragma unroll
        for (int w = 1; w < RELAX_WAVES; ++w) total += red[w];
        __syncthreads();
        return total;
    }

    template <int N, class F>
    __device__ __forceinline__ void sums(int count, F fn, double (&out)[N]) {
        static_assert(N <= RELAX_SUMS, "red holds RELAX_SUMS sums per wave");
        double v[N];
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = 0.0;
        for (int item = threadIdx.x; item < count; item += CFAR_THREADS) fn(item, v);
#pragma unroll
        for (int n = 0; n < N; ++n) {
            v[n] = sc_wave_sum(v[n]);
            if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * N + n] = v[n];
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < N; ++n) {
            double total = red[n];
#pragma unroll
            for (int w = 1; w < RELAX_WAVES; ++w) total += red[w * N + n];
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
        for (int item = threadIdx.x; item < count; item += CFAR_THREADS) {
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
        for (int w = 1; w < RELAX_WAVES; ++w)
            if (better(red[w], arg[w], bv, bi)) {
                bv = red[w];
                bi = arg[w];
            }
        __syncthreads();
        return bv >= 0.0 ? bi : -1;
    }
};

// the dynamic LDS of a scene: byte offsets of the arrays of RelaxMem, each 16-byte aligned
struct RelaxLayout {
    size_t x, img, map, tf, tt, pt, off, flag, u, v, tg, red, arg, total;
};

static __host__ __device__ RelaxLayout relax_layout(int Nb, int Nd, int r) {
    const size_t D = (size_t)Nb * (size_t)Nd, nf = (size_t)r * Nb, nt = (size_t)r * Nd, cells = nf * nt;
    RelaxLayout o;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    };
    o.x = take(D * sizeof(RfC));
    o.img = take(nf * (size_t)Nd * sizeof(RfC));
    o.map = take(cells * sizeof(double));
    o.tf = take(nf * sizeof(RfC));
    o.tt = take(nt * sizeof(RfC));
    o.pt = take(REFINE_MAX_M * sizeof(RfC));
    o.off = take(CFAR_MAX_TRAIN * sizeof(int));
    o.flag = take(cells * sizeof(uint8_t));
    o.u = take((size_t)Nb * sizeof(RfC));
    o.v = take((size_t)Nd * sizeof(RfC));
    o.tg = take(CRB_MAXL * sizeof(RelaxTarget));
    o.red = take(RELAX_WAVES * RELAX_SUMS * sizeof(double));
    o.arg = take(RELAX_WAVES * sizeof(int));
    o.total = at;
    return o;
}

__global__ __launch_bounds__(CFAR_THREADS) void cfar_relax_kernel(RelaxArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                                  const int32_t *__restrict__ symbols,
                                                                  const double *__restrict__ noise_var, double *__restrict__ rows,
                                                                  double *__restrict__ amp, int32_t *__restrict__ counts,
                                                                  double *__restrict__ info, double *__restrict__ map_out) {
    extern __shared__ __attribute__((aligned(16))) char relax_lds[];
    const RelaxLayout o = relax_layout(a.c.Nb, a.c.Nd, a.c.r);
    char *p = relax_lds;
    RelaxMem m;
    m.c.x = reinterpret_cast<RfC *>(p + o.x);
    m.c.img = reinterpret_cast<RfC *>(p + o.img);
    m.c.map = reinterpret_cast<double *>(p + o.map);
    m.c.tf = reinterpret_cast<RfC *>(p + o.tf);
    m.c.tt = reinterpret_cast<RfC *>(p + o.tt);
    m.c.pt = reinterpret_cast<RfC *>(p + o.pt);
    m.c.off = reinterpret_cast<int *>(p + o.off);
    m.c.flag = reinterpret_cast<uint8_t *>(p + o.flag);
    m.c.list = nullptr;
    m.c.chunk = nullptr;
    m.c.slot = nullptr;
    m.u = reinterpret_cast<RfC *>(p + o.u);
    m.v = reinterpret_cast<RfC *>(p + o.v);
    m.tg = reinterpret_cast<RelaxTarget *>(p + o.tg);
    RelaxPar par = {reinterpret_cast<double *>(p + o.red), reinterpret_cast<int *>(p + o.arg)};
    const int64_t sig = blockIdx.x, D = (int64_t)a.c.Nb * a.c.Nd, cells = D * a.c.r * a.c.r;
    relax_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                symbols ? symbols + sig * D : nullptr, noise_var ? noise_var + sig : nullptr, rows + sig * a.c.Le * 3,
                amp + sig * a.c.Le * 2, counts + sig * RELAX_COUNTS, info + sig * RELAX_INFO, map_out ? map_out + sig * cells : nullptr);
}

// cfar.hip's cfar_finish_kernel on the state column of this entry's `info`
__global__ __launch_bounds__(SC_FIN_THREADS) void cfar_relax_finish_kernel(int64_t B, const double *__restrict__ info,
                                                                           int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_THREADS];
    constexpr int slot_state[CFAR_STATUS] = {CF_NONFINITE, CF_OUTSIDE};
    for (int c = 0; c < CFAR_STATUS; ++c) {
        double n = 0.0;
        for (int64_t r = threadIdx.x; r < B; r += SC_FIN_THREADS)
            n += info[r * RELAX_INFO + 2] == (double)slot_state[c] ? 1.0 : 0.0;
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

int64_t cfar_relax_lds_bytes(int Nb, int Nd, int r) { return (int64_t)relax_layout(Nb, Nd, r).total; }
int64_t cfar_relax_lds_limit() { return RELAX_LDS_LIMIT; }

int launch_cfar_relax(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                      double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, int iters,
                      int sweeps, double *rows, double *amp, int32_t *counts, double *info, double *map_out, int32_t *status,
                      hipStream_t st) {
    const size_t lds = relax_layout(Nb, Nd, r).total;
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cfar_relax_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    const RelaxArgs a = {{Nb, Nd, r, Le, method, guard, train, rank, psk_m, psk_phase, alpha}, iters, sweeps};
    hipLaunchKernelGGL(cfar_relax_kernel, dim3((unsigned)B), dim3(CFAR_THREADS), lds, st, a, y, b, symbols, noise_var, rows, amp,
                       counts, info, map_out);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(cfar_relax_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, info, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
