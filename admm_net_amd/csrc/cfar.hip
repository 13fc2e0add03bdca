// cfar.hip -- a CFAR detector on the zero-padded 2-D periodogram of every scene (admm_net_amd/detect.py: cfar_targets; the
// definition is with admmnet_cfar_f64 in include/admmnet.h, the float64 host statement is detect.cfar_host).
//
// One scene per workgroup of CFAR_THREADS threads, one launch for the batch.  cfar_core.h has the scene loop, written over the ways
// a workgroup shares a loop (scene_wg.h's ScenePar): items dealt to the threads with a barrier behind them, and a sum in a fixed
// order.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.  y and b are read from HBM once; x,
// the intermediate image, the map, the twiddle tables and the list of detections stay in LDS (cfar_carve).  The batch counts of
// `status` are added from the state column of `info` by scene_wg.h's second, tiny launch.
#include "common.h"
#include "cfar_core.h"
#include "scene_wg.h"

namespace admmnet {

using CfarPar = ScenePar<CFAR_THREADS>;

// the dynamic LDS of a scene: the arrays of CfarMem, then the scratch of the sums
static __host__ __device__ void cfar_carve(LdsCarver &c, int Nb, int Nd, int r, CfarMem &m, CfarPar &par) {
    const size_t D = (size_t)Nb * (size_t)Nd, nf = (size_t)r * Nb, nt = (size_t)r * Nd, cells = nf * nt;
    m.x = c.take<RfC>(D);
    m.img = c.take<RfC>(nf * (size_t)Nd);
    m.map = c.take<double>(cells);
    m.tf = c.take<RfC>(nf);
    m.tt = c.take<RfC>(nt);
    m.pt = c.take<RfC>(REFINE_MAX_M);
    m.off = c.take<int>(CFAR_MAX_TRAIN);
    m.flag = c.take<uint8_t>(cells);
    m.list = c.take<uint16_t>(cells);
    m.chunk = c.take<int>(CFAR_THREADS + 1);
    m.slot = c.take<int>(CRB_MAXL);
    par.red = c.take<double>(CfarPar::WAVES);
    par.arg = nullptr;
}

__global__ __launch_bounds__(CFAR_THREADS) void cfar_kernel(CfarArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                            const int32_t *__restrict__ symbols, const double *__restrict__ noise_var,
                                                            double *__restrict__ rows, int32_t *__restrict__ counts,
                                                            double *__restrict__ info, double *__restrict__ map_out) {
    extern __shared__ __attribute__((aligned(16))) char cfar_lds[];
    LdsCarver c{cfar_lds};
    CfarMem m;
    CfarPar par;
    cfar_carve(c, a.Nb, a.Nd, a.r, m, par);
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd, cells = D * a.r * a.r;
    cfar_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
               symbols ? symbols + sig * D : nullptr, noise_var ? noise_var + sig : nullptr, rows + sig * a.Le * 3,
               counts + sig * CFAR_COUNTS, info + sig * CFAR_INFO, map_out ? map_out + sig * cells : nullptr);
}

int64_t cfar_lds_bytes(int Nb, int Nd, int r) {
    LdsCarver c{nullptr};
    CfarMem m;
    CfarPar par;
    cfar_carve(c, Nb, Nd, r, m, par);
    return (int64_t)c.at;
}
int64_t cfar_lds_limit() { return SCENE_LDS_LIMIT; }

int launch_cfar(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, double *rows,
                int32_t *counts, double *info, double *map_out, int32_t *status, hipStream_t st) {
    const CfarArgs a = {Nb, Nd, r, Le, method, guard, train, rank, psk_m, psk_phase, alpha};
    const SceneStates<CFAR_STATUS> states = {{CF_NONFINITE, CF_OUTSIDE}};
    return launch_scenes<CFAR_THREADS>(cfar_kernel, (size_t)cfar_lds_bytes(Nb, Nd, r), B, st, info, CFAR_INFO, CFAR_INFO_STATE, states,
                                       status, a, y, b, symbols, noise_var, rows, counts, info, map_out);
}

}  // namespace admmnet
