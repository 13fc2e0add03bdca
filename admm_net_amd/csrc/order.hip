// order.hip -- the number of targets of every scene selected on the device (admm_net_amd/order.py: select_targets; the definition
// is with admmnet_order_f64 in include/admmnet.h, the float64 host statement is order.select_host).
//
// One scene per workgroup of ORDER_THREADS threads, one launch for the batch.  order_core.h has the scene loop, written over the
// two ways a workgroup shares a loop (refine.hip's, repeated below as OrderPar): items dealt to the threads with a barrier behind
// them, and a sum in a fixed order -- a thread adds its items in index order, a butterfly adds the lanes of a wave, the waves are
// added in wave order.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.  y and b are read from
// HBM once; x, the twiddle tables of the rows, the Gram matrix and the Cholesky factor stay in LDS (order_layout).  The batch
// counts of `status` are added from the state column of `info` by one workgroup in a second, tiny launch.
#include "common.h"
#include "batch_sums.h"
#include "order_core.h"

namespace admmnet {

constexpr int64_t ORDER_LDS_LIMIT = 160 * 1024;
constexpr int ORDER_WAVES = ORDER_THREADS / 64;
static_assert(CRB_MAXL * (CRB_MAXL + 1) / 2 <= ORDER_THREADS, "one thread per pair of rows");
static_assert(CRB_MAXL <= 32, "the rows taken are kept in a 32-bit mask");

struct OrderPar {
    double *red;   // [ORDER_WAVES]

    template <class F>
    __device__ __forceinline__ void each(int count, F fn) {
        for (int item = threadIdx.x; item < count; item += ORDER_THREADS) fn(item);
        __syncthreads();
    }

    template <class F>
    __device__ __forceinline__ double sum(int count, F fn) {
        double v = 0.0;
        for (int item = threadIdx.x; item < count; item += ORDER_THREADS) v += fn(item);
        v = sc_wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double total = red[0];
#pragma unroll
        for (int w = 1; w < ORDER_WAVES; ++w) total += red[w];
        __syncthreads();
        return total;
    }
};

// the dynamic LDS of a scene: byte offsets of the arrays of OrderMem, each 16-byte aligned
struct OrderLayout {
    size_t x, pt, tab, rs, G, F, c, d, w, C, tau, f, rss, idx, pick, perm, meta, red, total;
};

static __host__ __device__ OrderLayout order_layout(int Nb, int Nd, int Le) {
    const size_t D = (size_t)Nb * (size_t)Nd, L = (size_t)Le;
    OrderLayout o;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    };
    o.x = take(D * sizeof(RfC));
    o.pt = take(REFINE_MAX_M * sizeof(RfC));
    o.tab = take((size_t)od_tab_count(Nb, Nd, Le) * sizeof(RfC));
    o.rs = take(L * (size_t)Nb * sizeof(RfC));
    o.G = take(L * L * sizeof(RfC));
    o.F = take(L * L * sizeof(RfC));
    o.c = take((L + 1) * L * sizeof(RfC));
    o.d = take((L + 1) * L * sizeof(double));
    o.w = take(L * sizeof(RfC));
    o.C = take(L * sizeof(RfC));
    o.tau = take(L * sizeof(double));
    o.f = take(L * sizeof(double));
    o.rss = take((L + 1) * sizeof(double));
    o.idx = take(L * sizeof(int));
    o.pick = take(L * sizeof(int));
    o.perm = take(L * sizeof(int));
    o.meta = take(OD_META * sizeof(int));
    o.red = take(ORDER_WAVES * sizeof(double));
    o.total = at;
    return o;
}

__global__ __launch_bounds__(ORDER_THREADS) void order_kernel(OrderArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                              const double *__restrict__ rows_in, const int32_t *__restrict__ n_cand,
                                                              const int32_t *__restrict__ n_held, const int32_t *__restrict__ symbols,
                                                              int32_t *__restrict__ perm, int32_t *__restrict__ n_sel,
                                                              double *__restrict__ rss, double *__restrict__ rows_out,
                                                              double2 *__restrict__ C_out, float2 *__restrict__ residual,
                                                              double *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) char order_lds[];
    const OrderLayout o = order_layout(a.Nb, a.Nd, a.Le);
    char *p = order_lds;
    OrderMem m;
    m.x = reinterpret_cast<RfC *>(p + o.x);
    m.pt = reinterpret_cast<RfC *>(p + o.pt);
    m.tab = reinterpret_cast<RfC *>(p + o.tab);
    m.rs = reinterpret_cast<RfC *>(p + o.rs);
    m.G = reinterpret_cast<RfC *>(p + o.G);
    m.F = reinterpret_cast<RfC *>(p + o.F);
    m.c = reinterpret_cast<RfC *>(p + o.c);
    m.d = reinterpret_cast<double *>(p + o.d);
    m.w = reinterpret_cast<RfC *>(p + o.w);
    m.C = reinterpret_cast<RfC *>(p + o.C);
    m.tau = reinterpret_cast<double *>(p + o.tau);
    m.f = reinterpret_cast<double *>(p + o.f);
    m.rss = reinterpret_cast<double *>(p + o.rss);
    m.idx = reinterpret_cast<int *>(p + o.idx);
    m.pick = reinterpret_cast<int *>(p + o.pick);
    m.perm = reinterpret_cast<int *>(p + o.perm);
    m.meta = reinterpret_cast<int *>(p + o.meta);
    OrderPar par = {reinterpret_cast<double *>(p + o.red)};
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd;
    order_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                rows_in + sig * a.Le * 3, n_cand ? n_cand + sig : nullptr, n_held ? n_held + sig : nullptr,
                symbols ? symbols + sig * D : nullptr, perm + sig * a.Le, n_sel + sig, rss + sig * (a.Le + 1),
                rows_out + sig * a.Le * 3, reinterpret_cast<double *>(C_out + sig * a.Le),
                reinterpret_cast<float *>(residual + sig * D), info + sig * ORDER_INFO);
}

// status[c] = the scenes in state c's slot; the counts are whole numbers, exact in float64 in any order
__global__ __launch_bounds__(SC_FIN_THREADS) void order_finish_kernel(int64_t B, const double *__restrict__ info,
                                                                      int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_THREADS];
    constexpr int slot_state[ORDER_STATUS] = {OD_NONFINITE, OD_OUTSIDE};
    for (int c = 0; c < ORDER_STATUS; ++c) {
        double n = 0.0;
        for (int64_t r = threadIdx.x; r < B; r += SC_FIN_THREADS)
            n += info[r * ORDER_INFO + 3] == (double)slot_state[c] ? 1.0 : 0.0;
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

int64_t order_lds_bytes(int Nb, int Nd, int Le) { return (int64_t)order_layout(Nb, Nd, Le).total; }
int64_t order_lds_limit() { return ORDER_LDS_LIMIT; }

int launch_order(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_cand,
                 const int32_t *n_held, const int32_t *symbols, int psk_m, double psk_phase, double penalty, int max_order,
                 int32_t *perm, int32_t *n_sel, double *rss, double *rows_out, double2 *C_out, float2 *residual, double *info,
                 int32_t *status, hipStream_t st) {
    const size_t lds = order_layout(Nb, Nd, Le).total;
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    const OrderArgs a = {Nb, Nd, Le, psk_m, psk_phase, penalty, max_order};
    hipLaunchKernelGGL(order_kernel, dim3((unsigned)B), dim3(ORDER_THREADS), lds, st, a, y, b, rows_in, n_cand, n_held, symbols, perm,
                       n_sel, rss, rows_out, C_out, residual, info);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(order_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, info, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
