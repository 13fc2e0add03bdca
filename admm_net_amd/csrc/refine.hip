// refine.hip -- target estimates refined against the received signal on the device (admm_net_amd/refine.py: refine_targets; the
// definition is with admmnet_refine_f64 in include/admmnet.h, the float64 host statement is refine.refine_host).
//
// One scene per workgroup of REFINE_THREADS threads, one launch for the batch; every iteration of a scene runs inside it.
// refine_core.h has the scene loop, written over the two ways a workgroup shares a loop (WgPar below): items dealt to the threads
// with a barrier behind them, and a sum in a fixed order -- a thread adds its items in index order, a butterfly adds the lanes of a
// wave, the waves are added in wave order.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.
// y and b are read from HBM once; x, the P x P matrix and the per-target twiddle tables stay in LDS (refine_layout).  The batch
// counts of `status` are added from the state column of `info` by one workgroup in a second, tiny launch.
#include "common.h"
#include "batch_sums.h"
#include "refine_core.h"

namespace admmnet {

constexpr int64_t REFINE_LDS_LIMIT = 160 * 1024;
constexpr int REFINE_WAVES = REFINE_THREADS / 64;
static_assert(CRB_MAXP <= REFINE_THREADS, "one thread per parameter");

struct WgPar {
    double *red;   // [REFINE_WAVES]

    template <class F>
    __device__ __forceinline__ void each(int count, F fn) {
        for (int item = threadIdx.x; item < count; item += REFINE_THREADS) fn(item);
        __syncthreads();
    }

    template <class F>
    __device__ __forceinline__ double sum(int count, F fn) {
        double v = 0.0;
        for (int item = threadIdx.x; item < count; item += REFINE_THREADS) v += fn(item);
        v = sc_wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double total = red[0];
#pragma unroll
        for (int w = 1; w < REFINE_WAVES; ++w) total += red[w];
        __syncthreads();
        return total;
    }
};

// the dynamic LDS of a scene: byte offsets of the arrays of RefineMem, each 16-byte aligned
struct RefineLayout {
    size_t z, k, k0, pt, A, tab, rs, cont, tg, trial, g, dsc, step, col, idx, red, total;
};

static __host__ __device__ RefineLayout refine_layout(int Nb, int Nd, int Le) {
    const size_t D = (size_t)Nb * (size_t)Nd, P = (size_t)rf_pmax(Nb, Nd, Le);
    RefineLayout o;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    };
    o.z = take(D * sizeof(RfC));
    o.k = take(D);
    o.k0 = take(D);
    o.pt = take(REFINE_MAX_M * sizeof(RfC));
    o.A = take(P * P * sizeof(double));
    o.tab = take((size_t)rf_tab_count(Nb, Nd, Le) * sizeof(RfC));
    o.rs = take((size_t)rf_rows_count(Nb, Le) * sizeof(RfC));
    o.cont = take(RF_CONT * sizeof(RfC));
    o.tg = take(CRB_MAXL * sizeof(CrbTarget));
    o.trial = take(CRB_MAXL * sizeof(CrbTarget));
    o.g = take(CRB_MAXP * sizeof(double));
    o.dsc = take(CRB_MAXP * sizeof(double));
    o.step = take(CRB_MAXP * sizeof(double));
    o.col = take(CRB_MAXP * sizeof(double));
    o.idx = take(RF_IDX * sizeof(int));
    o.red = take(REFINE_WAVES * sizeof(double));
    o.total = at;
    return o;
}

__global__ __launch_bounds__(REFINE_THREADS) void refine_kernel(RefineArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                                const double *__restrict__ rows_in, const int32_t *__restrict__ n_est,
                                                                double *__restrict__ rows_out, double2 *__restrict__ C_out,
                                                                double *__restrict__ info, int32_t *__restrict__ symbols_out) {
    extern __shared__ __attribute__((aligned(16))) char refine_lds[];
    const RefineLayout o = refine_layout(a.Nb, a.Nd, a.Le);
    char *p = refine_lds;
    RefineMem m;
    m.z = reinterpret_cast<RfC *>(p + o.z);
    m.k = reinterpret_cast<uint8_t *>(p + o.k);
    m.k0 = reinterpret_cast<uint8_t *>(p + o.k0);
    m.pt = reinterpret_cast<RfC *>(p + o.pt);
    m.A = reinterpret_cast<double *>(p + o.A);
    m.tab = reinterpret_cast<RfC *>(p + o.tab);
    m.rs = reinterpret_cast<RfC *>(p + o.rs);
    m.cont = reinterpret_cast<RfC *>(p + o.cont);
    m.tg = reinterpret_cast<CrbTarget *>(p + o.tg);
    m.trial = reinterpret_cast<CrbTarget *>(p + o.trial);
    m.g = reinterpret_cast<double *>(p + o.g);
    m.dsc = reinterpret_cast<double *>(p + o.dsc);
    m.step = reinterpret_cast<double *>(p + o.step);
    m.col = reinterpret_cast<double *>(p + o.col);
    m.idx = reinterpret_cast<int *>(p + o.idx);
    WgPar par = {reinterpret_cast<double *>(p + o.red)};
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd;
    refine_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                 rows_in + sig * a.Le * 3, n_est ? n_est + sig : nullptr, rows_out + sig * a.Le * 3,
                 reinterpret_cast<double *>(C_out + sig * a.Le), info + sig * REFINE_INFO,
                 symbols_out ? symbols_out + sig * D : nullptr);
}

// status[c] = the scenes in state c's slot; the counts are whole numbers, exact in float64 in any order
__global__ __launch_bounds__(SC_FIN_THREADS) void refine_finish_kernel(int64_t B, const double *__restrict__ info,
                                                                       int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_THREADS];
    constexpr int slot_state[REFINE_STATUS] = {RF_OUTSIDE, RF_NONFINITE, RF_GAVE_UP, RF_LIMIT};
    for (int c = 0; c < REFINE_STATUS; ++c) {
        double n = 0.0;
        for (int64_t r = threadIdx.x; r < B; r += SC_FIN_THREADS) n += info[r * REFINE_INFO + 4] == (double)slot_state[c] ? 1.0 : 0.0;
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

int64_t refine_lds_bytes(int Nb, int Nd, int Le) { return (int64_t)refine_layout(Nb, Nd, Le).total; }
int64_t refine_lds_limit() { return REFINE_LDS_LIMIT; }

int launch_refine(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_est,
                  int mode, int psk_m, double psk_phase, int iters, double tol, double *rows_out, double2 *C_out, double *info,
                  int32_t *symbols_out, int32_t *status, hipStream_t st) {
    const size_t lds = refine_layout(Nb, Nd, Le).total;
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(refine_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    const RefineArgs a = {Nb, Nd, Le, mode, psk_m, psk_phase, iters, tol};
    hipLaunchKernelGGL(refine_kernel, dim3((unsigned)B), dim3(REFINE_THREADS), lds, st, a, y, b, rows_in, n_est, rows_out, C_out, info,
                       symbols_out);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(refine_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, info, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
