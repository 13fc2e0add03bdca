// peaks.hip -- batched grid peak search on the delay-Doppler spectrum of phi: regional maxima of the
// coarse grid + local refinement rounds, one workgroup per signal.
//   /root/reference/utils/peakSearchUtils.py:63-173 (alt_peak_search): coarse grid -> skimage
//   local_maxima(connectivity=2) (:118) -> coordinates in np.where row-major order (:119-126) -> `iter`
//   refinement rounds (:136-171): step *= reducefactor, window +-step clipped to [min, max - step],
//   np.arange grid, first arg-max in row-major order.  Rows of the result: (x = tau, y = f, height).
// The coarse spectrum comes from spectrum.hip (float64, same arithmetic as the local evaluations here);
// this kernel is O(grid) integer / compare work per signal plus a handful of D-term inner products per peak.
#include "common.h"
#include "peak_core.h"

// numpy evaluates start + i * delta, k * step, ... with one rounding per operation: no FMA contraction in this
// file, so that grid coordinates (and hence the returned peak positions) are bit-identical to the reference's
#pragma clang fp contract(off)

namespace admmnet {

__global__ __launch_bounds__(PK_THREADS) void peaks_kernel(const float2 *__restrict__ phi, int xbase, int ybase,
                                                           const double *__restrict__ Z, int nx, int ny,
                                                           const double *__restrict__ axis_x,
                                                           const double *__restrict__ axis_y, PeakOpts o,
                                                           double *__restrict__ peaks, int32_t *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int npix = nx * ny, D = xbase * ybase;
    double *img = reinterpret_cast<double *>(smem);                 // [ny][nx]
    double2 *ph = reinterpret_cast<double2 *>(img + npix);          // [D]
    int *plist = reinterpret_cast<int *>(ph + D);                   // [max_peaks] pixel index of peak k
    int *scan = plist + o.max_peaks;                                // [PK_THREADS + 1]
    unsigned char *cand = reinterpret_cast<unsigned char *>(scan + PK_THREADS + 1);   // [2][npix]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const double *Zb = Z + b * (int64_t)npix;
    for (int i = tid; i < npix; i += PK_THREADS) img[i] = Zb[i];
    for (int i = tid; i < D; i += PK_THREADS) {   // (phi == nullptr: maxima of a caller-supplied image, no refinement)
        const float2 p = phi ? phi[b * D + i] : make_float2(0.f, 0.f);
        ph[i] = make_double2((double)p.x, (double)p.y);
    }
    __syncthreads();
    // ---- regional maxima, then the peaks in row-major order (np.where): each thread owns a contiguous run of pixels
    const unsigned char *cur = pk_maxima(img, nx, ny, cand);
    int i0, i1;
    const int total = pk_number(cur, npix, scan, i0, i1);
    {
        int pos = scan[tid];
        for (int i = i0; i < i1; ++i)
            if (cur[i]) {
                if (pos < o.max_peaks) plist[pos] = i;
                ++pos;
            }
    }
    if (tid == 0) counts[b] = total;
    __syncthreads();
    // ---- refinement: one wave per peak, lanes over the points of the local grid
    const int npk = min(total, o.max_peaks);
    double *out = peaks + b * (int64_t)o.max_peaks * 3;
    for (int k = wave; k < npk; k += PK_THREADS / 64) {
        const int pix = plist[k];
        const int r = pix / nx, c = pix - r * nx;
        double px = axis_x ? axis_x[c] : (double)c, py = axis_y ? axis_y[r] : (double)r, height;
        pk_refine(ph, xbase, ybase, o, px, py, height);
        if (lane == 0) {
            out[3 * k + 0] = px;
            out[3 * k + 1] = py;
            out[3 * k + 2] = height;
        }
    }
}

size_t peaks_lds_bytes(int npix, int D, int max_peaks) {
    return sizeof(double) * npix + sizeof(double2) * D + sizeof(int) * (max_peaks + PK_THREADS + 1) + 2 * (size_t)npix + 16;
}

int launch_peaks(const float2 *phi, int64_t B, int xbase, int ybase, const double *Z, int nx, int ny,
                 const double *axis_x, const double *axis_y, const double *opt7, int iters, int max_peaks,
                 double *peaks, int32_t *counts, hipStream_t st) {
    ProfScope _prof(KC_SPECTRUM, st);   // (bench accounting: the post-processing of cfg5 belongs to the "spectrum" class)
    if (B <= 0) return ADMMNET_OK;
    const size_t lds = peaks_lds_bytes(nx * ny, xbase * ybase, max_peaks);
    if (lds > 160 * 1024) {
        set_error("peak search: grid %d x %d (+ %d peaks) does not fit the LDS", nx, ny, max_peaks);
        return ADMMNET_E_ARG;
    }
    PeakOpts o{opt7[0], opt7[1], opt7[2], opt7[3], opt7[4], opt7[5], opt7[6], iters, max_peaks};
    ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(peaks_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(peaks_kernel, dim3((unsigned)B), dim3(PK_THREADS), lds, st, phi, xbase, ybase, Z, nx, ny,
                       axis_x, axis_y, o, peaks, counts);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
