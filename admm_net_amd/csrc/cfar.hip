// cfar.hip -- a CFAR detector on the zero-padded 2-D periodogram of every scene (admm_net_amd/detect.py: cfar_targets; the
// definition is with admmnet_cfar_f64 in include/admmnet.h, the float64 host statement is detect.cfar_host).
//
// One scene per workgroup of CFAR_THREADS threads, one launch for the batch.  cfar_core.h has the scene loop, written over the two
// ways a workgroup shares a loop (refine.hip's, repeated below as CfarPar): items dealt to the threads with a barrier behind them,
// and a sum in a fixed order -- a thread adds its items in index order, a butterfly adds the lanes of a wave, the waves are added
// in wave order.  No atomics: a scene's bits depend on neither B, nor its place, nor its neighbours.  y and b are read from HBM
// once; x, the intermediate image, the map, the twiddle tables and the list of detections stay in LDS (cfar_layout).  The batch
// counts of `status` are added from the state column of `info` by one workgroup in a second, tiny launch.
#include "common.h"
#include "batch_sums.h"
#include "cfar_core.h"

namespace admmnet {

constexpr int64_t CFAR_LDS_LIMIT = 160 * 1024;
constexpr int CFAR_WAVES = CFAR_THREADS / 64;

struct CfarPar {
    double *red;   // [CFAR_WAVES]

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
        for (int w = 1; w < CFAR_WAVES; ++w) total += red[w];
        __syncthreads();
        return total;
    }
};

// the dynamic LDS of a scene: byte offsets of the arrays of CfarMem, each 16-byte aligned
struct CfarLayout {
    size_t x, img, map, tf, tt, pt, off, flag, list, chunk, slot, red, total;
};

static __host__ __device__ CfarLayout cfar_layout(int Nb, int Nd, int r) {
    const size_t D = (size_t)Nb * (size_t)Nd, nf = (size_t)r * Nb, nt = (size_t)r * Nd, cells = nf * nt;
    CfarLayout o;
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
    o.list = take(cells * sizeof(uint16_t));
    o.chunk = take((CFAR_THREADS + 1) * sizeof(int));
    o.slot = take(CRB_MAXL * sizeof(int));
    o.red = take(CFAR_WAVES * sizeof(double));
    o.total = at;
    return o;
}

__global__ __launch_bounds__(CFAR_THREADS) void cfar_kernel(CfarArgs a, const float2 *__restrict__ y, const float2 *__restrict__ b,
                                                            const int32_t *__restrict__ symbols, const double *__restrict__ noise_var,
                                                            double *__restrict__ rows, int32_t *__restrict__ counts,
                                                            double *__restrict__ info, double *__restrict__ map_out) {
    extern __shared__ __attribute__((aligned(16))) char cfar_lds[];
    const CfarLayout o = cfar_layout(a.Nb, a.Nd, a.r);
    char *p = cfar_lds;
    CfarMem m;
    m.x = reinterpret_cast<RfC *>(p + o.x);
    m.img = reinterpret_cast<RfC *>(p + o.img);
    m.map = reinterpret_cast<double *>(p + o.map);
    m.tf = reinterpret_cast<RfC *>(p + o.tf);
    m.tt = reinterpret_cast<RfC *>(p + o.tt);
    m.pt = reinterpret_cast<RfC *>(p + o.pt);
    m.off = reinterpret_cast<int *>(p + o.off);
    m.flag = reinterpret_cast<uint8_t *>(p + o.flag);
    m.list = reinterpret_cast<uint16_t *>(p + o.list);
    m.chunk = reinterpret_cast<int *>(p + o.chunk);
    m.slot = reinterpret_cast<int *>(p + o.slot);
    CfarPar par = {reinterpret_cast<double *>(p + o.red)};
    const int64_t sig = blockIdx.x, D = (int64_t)a.Nb * a.Nd, cells = D * a.r * a.r;
    cfar_scene(par, a, m, reinterpret_cast<const float *>(y + sig * D), reinterpret_cast<const float *>(b + sig * D),
               symbols ? symbols + sig * D : nullptr, noise_var ? noise_var + sig : nullptr, rows + sig * a.Le * 3,
               counts + sig * CFAR_COUNTS, info + sig * CFAR_INFO, map_out ? map_out + sig * cells : nullptr);
}

// status[c] = the scenes in state c's slot; the counts are whole numbers, exact in float64 in any order
__global__ __launch_bounds__(SC_FIN_THREADS) void cfar_finish_kernel(int64_t B, const double *__restrict__ info,
                                                                     int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_THREADS];
    constexpr int slot_state[CFAR_STATUS] = {CF_NONFINITE, CF_OUTSIDE};
    for (int c = 0; c < CFAR_STATUS; ++c) {
        double n = 0.0;
        for (int64_t r = threadIdx.x; r < B; r += SC_FIN_THREADS)
            n += info[r * CFAR_INFO + 1] == (double)slot_state[c] ? 1.0 : 0.0;
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

int64_t cfar_lds_bytes(int Nb, int Nd, int r) { return (int64_t)cfar_layout(Nb, Nd, r).total; }
int64_t cfar_lds_limit() { return CFAR_LDS_LIMIT; }

int launch_cfar(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, double *rows,
                int32_t *counts, double *info, double *map_out, int32_t *status, hipStream_t st) {
    const size_t lds = cfar_layout(Nb, Nd, r).total;
    if (lds > 64 * 1024)
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cfar_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    const CfarArgs a = {Nb, Nd, r, Le, method, guard, train, rank, psk_m, psk_phase, alpha};
    hipLaunchKernelGGL(cfar_kernel, dim3((unsigned)B), dim3(CFAR_THREADS), lds, st, a, y, b, symbols, noise_var, rows, counts, info,
                       map_out);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(cfar_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, info, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
