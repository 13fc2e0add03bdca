// refine.hip -- target estimates refined against the received signal on the device (admm_net_amd/refine.py: refine_targets; the
// definition is with admmnet_refine_f64 in include/admmnet.h, the float64 host statement is refine.refine_host).
//
// One scene per workgroup of REFINE_THREADS threads, one launch for the batch; every iteration of a scene runs inside it.
// refine_core.h has the scene loop, written over the ways a workgroup shares a loop (scene_wg.h's ScenePar): items dealt to the
// threads with a barrier behind them, and a sum in a fixed order.  No atomics: a scene's bits depend on neither B, nor its place,
// nor its neighbours.  y and b are read from HBM once; x, the P x P matrix and the per-target twiddle tables stay in LDS
// (refine_carve).  The batch counts of `status` are added from the state column of `info` by scene_wg.h's second, tiny launch.
#include "common.h"
#include "refine_core.h"
#include "scene_wg.h"

namespace admmnet {

static_assert(CRB_MAXP <= REFINE_THREADS, "one thread per parameter");

using RefinePar = ScenePar<REFINE_THREADS>;

// the dynamic LDS of a scene: the arrays of RefineMem, then the scratch of the sums
static __host__ __device__ void refine_carve(LdsCarver &c, int Nb, int Nd, int Le, RefineMem &m, RefinePar &par) {
    const size_t D = (size_t)Nb * (size_t)Nd, P = (size_t)rf_pmax(Nb, Nd, Le);
    m.z = c.take<RfC>(D);
    m.k = c.take<uint8_t>(D);
    m.k0 = c.take<uint8_t>(D);
    m.pt = c.take<RfC>(REFINE_MAX_M);
    m.A = c.take<double>(P * P);
    m.tab = c.take<RfC>((size_t)rf_tab_count(Nb, Nd, Le));
    m.rs = c.take<RfC>((size_t)rf_rows_count(Nb, Le));
    m.cont = c.take<RfC>(RF_CONT);
    m.tg = c.take<CrbTarget>(CRB_MAXL);
    m.trial = c.take<CrbTarget>(CRB_MAXL);
    m.g = c.take<double>(CRB_MAXP);
    m.dsc = c.take<double>(CRB_MAXP);
    m.step = c.take<double>(CRB_MAXP);
    m.col = c.take<double>(CRB_MAXP);
    m.idx = c.take<int>(RF_IDX);
    par.red = c.take<double>(RefinePar::WAVES);
    par.arg = nullptr;
}

__global__ __launch_bounds__(REFINE_THREADS) void refine_kernel(RefineArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                                const double *__restrict__ rows_in, const int32_t *__restrict__ n_est,
                                                                double *__restrict__ rows_out, double2 *__restrict__ C_out,
                                                                double *__restrict__ info, int32_t *__restrict__ symbols_out) {
    extern __shared__ __attribute__((aligned(16))) char refine_lds[];
    LdsCarver c{refine_lds};
    RefineMem m;
    RefinePar par;
    refine_carve(c, a.Nb, a.Nd, a.Le, m, par);
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd;
    refine_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                 rows_in + sig * a.Le * 3, n_est ? n_est + sig : nullptr, rows_out + sig * a.Le * 3,
                 reinterpret_cast<double *>(C_out + sig * a.Le), info + sig * REFINE_INFO,
                 symbols_out ? symbols_out + sig * D : nullptr);
}

int64_t refine_lds_bytes(int Nb, int Nd, int Le) {
    LdsCarver c{nullptr};
    RefineMem m;
    RefinePar par;
    refine_carve(c, Nb, Nd, Le, m, par);
    return (int64_t)c.at;
}
int64_t refine_lds_limit() { return SCENE_LDS_LIMIT; }

int launch_refine(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_est,
                  int mode, int psk_m, double psk_phase, int iters, double tol, double *rows_out, double2 *C_out, double *info,
                  int32_t *symbols_out, int32_t *status, hipStream_t st) {
    const RefineArgs a = {Nb, Nd, Le, mode, psk_m, psk_phase, iters, tol};
    const SceneStates<REFINE_STATUS> states = {{RF_OUTSIDE, RF_NONFINITE, RF_GAVE_UP, RF_LIMIT}};
    return launch_scenes<REFINE_THREADS>(refine_kernel, (size_t)refine_lds_bytes(Nb, Nd, Le), B, st, info, REFINE_INFO,
                                         REFINE_INFO_STATE, states, status, a, y, b, rows_in, n_est, rows_out, C_out, info, symbols_out);
}

}  // namespace admmnet
