// order.hip -- the number of targets of every scene selected on the device (admm_net_amd/order.py: select_targets; the definition
// is with admmnet_order_f64 in include/admmnet.h, the float64 host statement is order.select_host).
//
// One scene per workgroup of ORDER_THREADS threads, one launch for the batch.  order_core.h has the scene loop, written over the
// ways a workgroup shares a loop (scene_wg.h's ScenePar): items dealt to the threads with a barrier behind them, and a sum in a
// fixed order.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.  y and b are read from HBM
// once; x, the twiddle tables of the rows, the Gram matrix and the Cholesky factor stay in LDS (order_carve).  The batch counts of
// `status` are added from the state column of `info` by scene_wg.h's second, tiny launch.
#include "common.h"
#include "order_core.h"
#include "scene_wg.h"

namespace admmnet {

static_assert(CRB_MAXL * (CRB_MAXL + 1) / 2 <= ORDER_THREADS, "one thread per pair of rows");
static_assert(CRB_MAXL <= 32, "the rows taken are kept in a 32-bit mask");

using OrderPar = ScenePar<ORDER_THREADS>;

// the dynamic LDS of a scene: the arrays of OrderMem, then the scratch of the sums
static __host__ __device__ void order_carve(LdsCarver &c, int Nb, int Nd, int Le, OrderMem &m, OrderPar &par) {
    const size_t D = (size_t)Nb * (size_t)Nd, L = (size_t)Le;
    m.x = c.take<RfC>(D);
    m.pt = c.take<RfC>(REFINE_MAX_M);
    m.tab = c.take<RfC>((size_t)od_tab_count(Nb, Nd, Le));
    m.rs = c.take<RfC>(L * (size_t)Nb);
    m.G = c.take<RfC>(L * L);
    m.F = c.take<RfC>(L * L);
    m.c = c.take<RfC>((L + 1) * L);
    m.d = c.take<double>((L + 1) * L);
    m.w = c.take<RfC>(L);
    m.C = c.take<RfC>(L);
    m.tau = c.take<double>(L);
    m.f = c.take<double>(L);
    m.rss = c.take<double>(L + 1);
    m.idx = c.take<int>(L);
    m.pick = c.take<int>(L);
    m.perm = c.take<int>(L);
    m.meta = c.take<int>(OD_META);
    par.red = c.take<double>(OrderPar::WAVES);
    par.arg = nullptr;
}

__global__ __launch_bounds__(ORDER_THREADS) void order_kernel(OrderArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                              const double *__restrict__ rows_in, const int32_t *__restrict__ n_cand,
                                                              const int32_t *__restrict__ n_held, const int32_t *__restrict__ symbols,
                                                              int32_t *__restrict__ perm, int32_t *__restrict__ n_sel,
                                                              double *__restrict__ rss, double *__restrict__ rows_out,
                                                              double2 *__restrict__ C_out, float2 *__restrict__ residual,
                                                              double *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) char order_lds[];
    LdsCarver c{order_lds};
    OrderMem m;
    OrderPar par;
    order_carve(c, a.Nb, a.Nd, a.Le, m, par);
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd;
    order_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                rows_in + sig * a.Le * 3, n_cand ? n_cand + sig : nullptr, n_held ? n_held + sig : nullptr,
                symbols ? symbols + sig * D : nullptr, perm + sig * a.Le, n_sel + sig, rss + sig * (a.Le + 1),
                rows_out + sig * a.Le * 3, reinterpret_cast<double *>(C_out + sig * a.Le),
                reinterpret_cast<float *>(residual + sig * D), info + sig * ORDER_INFO);
}

int64_t order_lds_bytes(int Nb, int Nd, int Le) {
    LdsCarver c{nullptr};
    OrderMem m;
    OrderPar par;
    order_carve(c, Nb, Nd, Le, m, par);
    return (int64_t)c.at;
}
int64_t order_lds_limit() { return SCENE_LDS_LIMIT; }

int launch_order(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_cand,
                 const int32_t *n_held, const int32_t *symbols, int psk_m, double psk_phase, double penalty, int max_order,
                 int32_t *perm, int32_t *n_sel, double *rss, double *rows_out, double2 *C_out, float2 *residual, double *info,
                 int32_t *status, hipStream_t st) {
    const OrderArgs a = {Nb, Nd, Le, psk_m, psk_phase, penalty, max_order};
    const SceneStates<ORDER_STATUS> states = {{OD_NONFINITE, OD_OUTSIDE}};
    return launch_scenes<ORDER_THREADS>(order_kernel, (size_t)order_lds_bytes(Nb, Nd, Le), B, st, info, ORDER_INFO, ORDER_INFO_STATE,
                                        states, status, a, y, b, rows_in, n_cand, n_held, symbols, perm, n_sel, rss, rows_out, C_out,
                                        residual, info);
}

}  // namespace admmnet
