// cfar_relax.hip -- successive cancellation with cyclic re-fitting on the periodogram of every scene (admm_net_amd/detect.py:
// cfar_relax; the definition is with admmnet_cfar_relax_f64 in include/admmnet.h, the float64 host statement is
// detect.cfar_relax_host).
//
// One scene per workgroup of CFAR_THREADS threads, one launch for the batch, as cfar.hip.  relax_core.h has the scene loop, written
// over all four ways a workgroup shares a loop (scene_wg.h's ScenePar): cfar.hip's two, N sums in one pass (the six complex moments
// of a Newton step: one pass over D and one barrier pair, not six), and the item of greatest value (the highest cell over the
// threshold), a tie going to the smaller index at every stage.  No atomics: a scene's bits depend on neither B, nor its place, nor
// its neighbours.  y and b are read from HBM once; the residual, the intermediate image, the map, the tables and the targets stay
// in LDS (relax_carve).  The map is recomputed from the residual every round.  The batch counts of `status` are added from the
// state column of `info` by scene_wg.h's second, tiny launch.
#include "common.h"
#include "relax_core.h"
#include "scene_wg.h"

namespace admmnet {

using RelaxPar = ScenePar<CFAR_THREADS, RELAX_SUMS>;

// the dynamic LDS of a scene: the arrays of RelaxMem (its CfarMem without the list of detections), then the scratch of the sums
// and of the best item
static __host__ __device__ void relax_carve(LdsCarver &c, int Nb, int Nd, int r, RelaxMem &m, RelaxPar &par) {
    const size_t D = (size_t)Nb * (size_t)Nd, nf = (size_t)r * Nb, nt = (size_t)r * Nd, cells = nf * nt;
    m.c.x = c.take<RfC>(D);
    m.c.img = c.take<RfC>(nf * (size_t)Nd);
    m.c.map = c.take<double>(cells);
    m.c.tf = c.take<RfC>(nf);
    m.c.tt = c.take<RfC>(nt);
    m.c.pt = c.take<RfC>(REFINE_MAX_M);
    m.c.off = c.take<int>(CFAR_MAX_TRAIN);
    m.c.flag = c.take<uint8_t>(cells);
    m.c.list = nullptr;
    m.c.chunk = nullptr;
    m.c.slot = nullptr;
    m.u = c.take<RfC>((size_t)Nb);
    m.v = c.take<RfC>((size_t)Nd);
    m.tg = c.take<RelaxTarget>(CRB_MAXL);
    par.red = c.take<double>(RelaxPar::WAVES * RELAX_SUMS);
    par.arg = c.take<int>(RelaxPar::WAVES);
}

__global__ __launch_bounds__(CFAR_THREADS) void cfar_relax_kernel(RelaxArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                                  const int32_t *__restrict__ symbols,
                                                                  const double *__restrict__ noise_var, double *__restrict__ rows,
                                                                  double *__restrict__ amp, int32_t *__restrict__ counts,
                                                                  double *__restrict__ info, double *__restrict__ map_out) {
    extern __shared__ __attribute__((aligned(16))) char relax_lds[];
    LdsCarver c{relax_lds};
    RelaxMem m;
    RelaxPar par;
    relax_carve(c, a.c.Nb, a.c.Nd, a.c.r, m, par);
    const int64_t sig = blockIdx.x, D = (int64_t)a.c.Nb * a.c.Nd, cells = D * a.c.r * a.c.r;
    relax_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
                symbols ? symbols + sig * D : nullptr, noise_var ? noise_var + sig : nullptr, rows + sig * a.c.Le * 3,
                amp + sig * a.c.Le * 2, counts + sig * RELAX_COUNTS, info + sig * RELAX_INFO, map_out ? map_out + sig * cells : nullptr);
}

int64_t cfar_relax_lds_bytes(int Nb, int Nd, int r) {
    LdsCarver c{nullptr};
    RelaxMem m;
    RelaxPar par;
    relax_carve(c, Nb, Nd, r, m, par);
    return (int64_t)c.at;
}
int64_t cfar_relax_lds_limit() { return SCENE_LDS_LIMIT; }

int launch_cfar_relax(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                      double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, int iters,
                      int sweeps, double *rows, double *amp, int32_t *counts, double *info, double *map_out, int32_t *status,
                      hipStream_t st) {
    const RelaxArgs a = {{Nb, Nd, r, Le, method, guard, train, rank, psk_m, psk_phase, alpha}, iters, sweeps};
    const SceneStates<CFAR_STATUS> states = {{CF_NONFINITE, CF_OUTSIDE}};
    return launch_scenes<CFAR_THREADS>(cfar_relax_kernel, (size_t)cfar_relax_lds_bytes(Nb, Nd, r), B, st, info, RELAX_INFO,
                                       RELAX_INFO_STATE, states, status, a, y, b, symbols, noise_var, rows, amp, counts, info, map_out);
}

}  // namespace admmnet
