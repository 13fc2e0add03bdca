// estimate.hip -- batched top-L target estimation: spectrum -> regional maxima -> refinement rounds -> selection of
// the L highest refined peaks, one workgroup per signal, nothing but L rows and one count per signal written.
//   utils/peakSearchUtils.py:63-173 (alt_peak_search) followed by the two lines both inference callers add
//   (main_for_net.py:117-126, test/test_model_peaksearch.py:85-96): sort the rows by refined height, descending and
//   stable, and keep the first L.
// The stages are the shared bodies of spectrum_kernel and peaks_kernel (peak_core.h), so image, maxima and refined
// rows are bit for bit those of admmnet_peak_search_f64; the coarse image lives in LDS only and there is no peak
// list: every regional maximum takes part, whatever their number.
//
// Selection: peak k (np.where order) has rank(k) = #{j : h_j > h_k} + #{j < k : h_j == h_k}; output row r is the peak
// of rank r.  Wave w refines the peaks k = w (mod 4) in ascending k and keeps its own L best in registers, lane r
// holding its r-th; the four lists (4 L <= 256 candidates, one per thread) are ranked against each other at the end.
//
// LDS: img [ny][nx] f64 | ph [D] double2 | tail, used twice:
//   while the image is evaluated   U [ybase][64] double2 (staging of sp_image)
//   afterwards                     mh, mx, my [4 L] f64, mk [4 L] i32 (the four lists), scan [257] i32,
//                                  tile [256] i32 (pixel of peak t0 + i of the current tile), cand [2][npix] u8
#include "common.h"
#include "peak_core.h"

namespace admmnet {

constexpr int EST_WAVES = PK_THREADS / 64;
constexpr int EST_TILE = 256;   // peaks numbered per pass over the mask; a multiple of EST_WAVES
constexpr int EST_LMAX = 64;    // one list entry per lane

static size_t est_tail_bytes(int npix, int ybase, int L) {
    const size_t stage = sizeof(double2) * (size_t)ybase * SP_XCHUNK;
    const size_t search = (size_t)EST_WAVES * L * (3 * sizeof(double) + sizeof(int)) +
                          sizeof(int) * (PK_THREADS + 1 + EST_TILE) + 2 * (size_t)npix;
    return stage > search ? stage : search;
}

size_t estimate_lds_bytes(int npix, int D, int ybase, int L) {
    return sizeof(double) * (size_t)npix + sizeof(double2) * (size_t)D + est_tail_bytes(npix, ybase, L) + 16;
}

__global__ __launch_bounds__(PK_THREADS) void estimate_kernel(const float2 *__restrict__ phi, int xbase, int ybase,
                                                              const double2 *__restrict__ tabD, int nx,
                                                              const double2 *__restrict__ tabS, int ny,
                                                              const double *__restrict__ axis_x,
                                                              const double *__restrict__ axis_y, PeakOpts o, int L,
                                                              const int32_t *__restrict__ top_n,
                                                              double *__restrict__ top, int32_t *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int npix = nx * ny, D = xbase * ybase;
    double *img = reinterpret_cast<double *>(smem);                 // [ny][nx]
    double2 *ph = reinterpret_cast<double2 *>(img + npix);          // [D]
    double2 *U = ph + D;                                            // tail, first use
    double *mh = reinterpret_cast<double *>(ph + D);                // tail, second use
    double *mx = mh + EST_WAVES * L, *my = mx + EST_WAVES * L;
    int *mk = reinterpret_cast<int *>(my + EST_WAVES * L);
    int *scan = mk + EST_WAVES * L;                                 // [PK_THREADS + 1]
    int *tile = scan + PK_THREADS + 1;                              // [EST_TILE]
    unsigned char *cand = reinterpret_cast<unsigned char *>(tile + EST_TILE);   // [2][npix]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    double *out = top + b * (int64_t)L * 3;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = tid; i < 3 * L; i += PK_THREADS) out[i] = nan;     // rows no peak claims below stay NaN
    for (int i = tid; i < D; i += PK_THREADS) {
        const float2 p = phi[b * D + i];
        ph[i] = make_double2((double)p.x, (double)p.y);
    }
    __syncthreads();
    sp_image(ph, xbase, ybase, tabD, nx, tabS, ny, U, img);         // ends with a barrier: U is free from here on
    const unsigned char *cur = pk_maxima(img, nx, ny, cand);
    int i0, i1;
    const int total = pk_number(cur, npix, scan, i0, i1);
    if (tid == 0) counts[b] = total;
    // ---- refinement, one wave per peak, and the wave's running top L: lane r holds (eh, ex, ey, ek) of its r-th best
    double eh = 0.0, ex = 0.0, ey = 0.0;
    int ek = -1;                                                    // -1: empty (the empty entries are the last ones)
    for (int t0 = 0; t0 < total; t0 += EST_TILE) {
        int pos = scan[tid];
        for (int i = i0; i < i1; ++i)
            if (cur[i]) {
                if (pos >= t0 && pos < t0 + EST_TILE) tile[pos - t0] = i;
                ++pos;
            }
        __syncthreads();
        const int nk = min(EST_TILE, total - t0);
        for (int kk = wave; kk < nk; kk += EST_WAVES) {
            const int pix = tile[kk];
            const int r = pix / nx, c = pix - r * nx;
            double px = axis_x[c], py = axis_y[r], height;
            pk_refine(ph, xbase, ybase, o, px, py, height);
            // insert: a wave meets its peaks in ascending k, so a new peak goes behind every entry of equal height
            const int beaten = (ek < 0 || height > eh) ? 1 : 0;
            const double uh = __shfl_up(eh, 1, 64), ux = __shfl_up(ex, 1, 64), uy = __shfl_up(ey, 1, 64);
            const int uk = __shfl_up(ek, 1, 64);
            int ubeaten = __shfl_up(beaten, 1, 64);   // (every lane takes part in the shuffle; lane 0 has no lane above)
            if (lane == 0) ubeaten = 0;
            if (beaten) {
                eh = ubeaten ? uh : height;
                ex = ubeaten ? ux : px;
                ey = ubeaten ? uy : py;
                ek = ubeaten ? uk : t0 + kk;
            }
        }
        __syncthreads();
    }
    // ---- merge the four lists: candidate c = thread c, its rank among all of them is its rank among all peaks
    const int nc = EST_WAVES * L;
    if (lane < L) {
        mh[wave * L + lane] = eh;
        mx[wave * L + lane] = ex;
        my[wave * L + lane] = ey;
        mk[wave * L + lane] = ek;
    }
    __syncthreads();
    int Lb = L;
    if (top_n) Lb = min(max(top_n[b], 0), L);
    if (tid < nc && mk[tid] >= 0) {
        const double h = mh[tid];
        const int k = mk[tid];
        int rank = 0;
        for (int j = 0; j < nc; ++j) rank += (mk[j] >= 0 && (mh[j] > h || (mh[j] == h && mk[j] < k))) ? 1 : 0;
        if (rank < Lb) {
            out[3 * rank + 0] = mx[tid];
            out[3 * rank + 1] = my[tid];
            out[3 * rank + 2] = h;
        }
    }
}

int launch_estimate(const float2 *phi, int64_t B, int xbase, int ybase, const double2 *tabD, int nx,
                    const double2 *tabS, int ny, const double *axis_x, const double *axis_y, const double *opt7,
                    int iters, int L, const int32_t *top_n, double *top, int32_t *counts, hipStream_t st) {
    ProfScope _prof(KC_SPECTRUM, st);   // (bench accounting: with the spectrum and the peak search it replaces)
    if (B <= 0) return ADMMNET_OK;
    static_assert(EST_TILE % EST_WAVES == 0 && EST_WAVES * EST_LMAX <= PK_THREADS, "one merge candidate per thread");
    const size_t lds = estimate_lds_bytes(nx * ny, xbase * ybase, ybase, L);
    if (lds > 160 * 1024) {
        set_error("peak top: grid %d x %d does not fit the LDS", nx, ny);
        return ADMMNET_E_ARG;
    }
    PeakOpts o{opt7[0], opt7[1], opt7[2], opt7[3], opt7[4], opt7[5], opt7[6], iters, 0};
    ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(estimate_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(estimate_kernel, dim3((unsigned)B), dim3(PK_THREADS), lds, st, phi, xbase, ybase, tabD, nx,
                       tabS, ny, axis_x, axis_y, o, L, top_n, top, counts);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
