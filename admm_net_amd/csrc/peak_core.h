// peak_core.h -- the per-signal bodies of the delay-Doppler spectrum (spectrum.hip) and of the grid peak search
// (peaks.hip) as __device__ functions, shared with the fused estimator (estimate.hip) so that the three kernels
// compute the same bits by construction.
//
// Every function here fixes its own floating-point contraction with `#pragma clang fp contract(off)` at the start
// of its body, so what it computes does not depend on the file or the kernel it is inlined into:
//   * sp_image writes the fused multiply-adds OUT: fma() where spectrum_kernel's ISA has v_fma_f64 / v_fmac_f64
//     (the compiler's choice while that kernel was free to contract, read from its gfx950 assembly), a separate
//     multiply and add where it has not.  The image is therefore the one spectrum_kernel has always written;
//   * the peak-search functions use no fused operation at all: numpy evaluates start + i * delta, k * step, ...
//     with one rounding per operation, and the grid coordinates (hence the returned positions) must be bit-identical
//     to the reference's.
#pragma once
#include "common.h"

namespace admmnet {

constexpr int SP_THREADS = 256;
constexpr int SP_XCHUNK = 64;
constexpr int PK_THREADS = 256;

// |phi^H kron(s(f), conj d(tau))|^2 of one signal on the whole grid, by a workgroup of SP_THREADS threads:
//   U[ks][ix] = sum_kd conj(phi[ks][kd]) conj(d_ix[kd]),  z[iy][ix] = sum_ks s_iy[ks] U[ks][ix],  out[iy][ix] = |z|^2
// ph: LDS [ybase * xbase] (phi in double), U: LDS staging [ybase][SP_XCHUNK], out: [ny][nx] in global memory or LDS.
// ph must be visible on entry; out is visible to the whole workgroup on return (the loop ends with a barrier).
__device__ __forceinline__ void sp_image(const double2 *ph, int xbase, int ybase, const double2 *__restrict__ tabD,
                                         int nx, const double2 *__restrict__ tabS, int ny, double2 *U, double *out) {
#pragma clang fp contract(off)
    for (int x0 = 0; x0 < nx; x0 += SP_XCHUNK) {
        const int xw = min(SP_XCHUNK, nx - x0);
        for (int p = threadIdx.x; p < ybase * xw; p += SP_THREADS) {
            const int ks = p / xw, xl = p - ks * xw;
            const double2 *d = tabD + (int64_t)(x0 + xl) * xbase;
            double ur = 0.0, ui = 0.0;
            for (int kd = 0; kd < xbase; ++kd) {
                // conj(phi) * conj(d) = conj(phi * d)
                const double2 a = ph[ks * xbase + kd], e = d[kd];
                ur = ur + fma(a.x, e.x, -(a.y * e.y));
                ui = ui - fma(a.y, e.x, a.x * e.y);
            }
            U[ks * SP_XCHUNK + xl] = make_double2(ur, ui);
        }
        __syncthreads();
        for (int p = threadIdx.x; p < ny * xw; p += SP_THREADS) {
            const int iy = p / xw, xl = p - iy * xw;
            const double2 *s = tabS + (int64_t)iy * ybase;
            double zr = 0.0, zi = 0.0;
            for (int ks = 0; ks < ybase; ++ks) {
                const double2 a = s[ks], u = U[ks * SP_XCHUNK + xl];
                zr = zr + fma(a.x, u.x, -(a.y * u.y));
                zi = zi + fma(a.y, u.x, a.x * u.y);
            }
            out[iy * (int64_t)nx + x0 + xl] = fma(zr, zr, zi * zi);
        }
        __syncthreads();
    }
}

// exp(j 2 pi fre_k), fre = numpy.linspace(0, (base - 1) x, base)[k]  (utils/mathUtils.py:4-21); the same
// expression as steer_table_kernel in spectrum.hip
__device__ __forceinline__ double2 pk_steer(double x, int k, int base) {
#pragma clang fp contract(off)
    const double stop = (double)(base - 1) * x;
    double fre = (base > 1) ? (double)k * (stop / (double)(base - 1)) : 0.0;
    if (base > 1 && k == base - 1) fre = stop;
    double s, c;
    sincos(2.0 * 3.14159265358979323846 * fre, &s, &c);
    return make_double2(c, s);
}

// |phi^H kron(s(y), conj d(x))|^2 at one point, separable form of sp_image.  The delay steering vector
// is evaluated once per point when it fits 16 registers pairs (every geometry of the reference), else per use.
__device__ inline double pk_point(const double2 *ph, int xbase, int ybase, double x, double y) {
#pragma clang fp contract(off)
    double2 e[16];
    const bool cached = xbase <= 16;
    if (cached) {
#pragma unroll
        for (int kd = 0; kd < 16; ++kd) e[kd] = (kd < xbase) ? pk_steer(x, kd, xbase) : make_double2(0.0, 0.0);
    }
    double zr = 0.0, zi = 0.0;
    for (int ks = 0; ks < ybase; ++ks) {
        double ur = 0.0, ui = 0.0;
        if (cached) {
#pragma unroll
            for (int kd = 0; kd < 16; ++kd) {
                if (kd < xbase) {
                    const double2 a = ph[ks * xbase + kd];
                    ur += a.x * e[kd].x - a.y * e[kd].y;
                    ui -= a.x * e[kd].y + a.y * e[kd].x;
                }
            }
        } else {
            for (int kd = 0; kd < xbase; ++kd) {
                const double2 a = ph[ks * xbase + kd], ee = pk_steer(x, kd, xbase);
                ur += a.x * ee.x - a.y * ee.y;
                ui -= a.x * ee.y + a.y * ee.x;
            }
        }
        const double2 s = pk_steer(y, ks, ybase);
        zr += s.x * ur - s.y * ui;
        zi += s.x * ui + s.y * ur;
    }
    return zr * zr + zi * zi;
}

struct PeakOpts {
    double xmin, xmax, xstep, ymin, ymax, ystep, reduce;
    int iters, max_peaks;
};

// Regional maxima of img [ny][nx] (LDS, visible on entry), 8-connected, plateau aware (skimage
// local_maxima(connectivity=2)): a pixel is a candidate if no neighbour is larger; a plateau survives only if all of
// its pixels do.  cand: LDS [2][nx * ny]; returns the half that holds the mask, visible to the whole workgroup.
__device__ __forceinline__ unsigned char *pk_maxima(const double *img, int nx, int ny, unsigned char *cand) {
    const int npix = nx * ny, tid = threadIdx.x;
    const double v0 = img[0];
    int notflat = 0;
    for (int i = tid; i < npix; i += PK_THREADS) notflat |= (img[i] != v0);
    const int any_diff = __syncthreads_or(notflat);
    unsigned char *cur = cand, *nxt = cand + npix;
    for (int i = tid; i < npix; i += PK_THREADS) {
        const int r = i / nx, c = i - r * nx;
        const double v = img[i];
        bool ok = any_diff != 0;   // a constant image has no regional maximum
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if ((dr | dc) == 0 || rr < 0 || rr >= ny || cc < 0 || cc >= nx) continue;
                ok = ok && (v >= img[rr * nx + cc]);
            }
        cur[i] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int guard = 0; guard < npix; ++guard) {   // rejection spreads over plateaus until nothing changes
        int changed = 0;
        for (int i = tid; i < npix; i += PK_THREADS) {
            unsigned char keep = cur[i];
            if (keep) {
                const int r = i / nx, c = i - r * nx;
                const double v = img[i];
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc) {
                        const int rr = r + dr, cc = c + dc;
                        if ((dr | dc) == 0 || rr < 0 || rr >= ny || cc < 0 || cc >= nx) continue;
                        const int q = rr * nx + cc;
                        if (img[q] == v && !cur[q]) keep = 0;
                    }
                changed |= !keep;
            }
            nxt[i] = keep;
        }
        unsigned char *t = cur;
        cur = nxt;
        nxt = t;
        if (!__syncthreads_or(changed)) break;
    }
    return cur;
}

// Row-major (np.where) numbering of the maxima: thread t owns the contiguous pixel run [i0, i1) and its first
// maximum has list position scan[t] on return; returns the number of maxima.  scan: LDS [PK_THREADS + 1].
__device__ __forceinline__ int pk_number(const unsigned char *cur, int npix, int *scan, int &i0, int &i1) {
    const int tid = threadIdx.x;
    const int per = (npix + PK_THREADS - 1) / PK_THREADS;
    i0 = min(tid * per, npix);
    i1 = min(i0 + per, npix);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += cur[i];
    scan[tid + 1] = mine;
    if (tid == 0) scan[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int t = 1; t <= PK_THREADS; ++t) scan[t] += scan[t - 1];
    __syncthreads();
    return scan[PK_THREADS];
}

// The refinement rounds of one peak (peakSearchUtils.py:136-171) by one whole wave, lanes over the points of the
// local grid.  (px, py): in, the coarse position; out, the refined one.  height: the value after the last round that
// ran, 0.0 if none did.  All lanes return the same values.
__device__ __forceinline__ void pk_refine(const double2 *ph, int xbase, int ybase, const PeakOpts &o, double &px,
                                          double &py, double &height) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    height = 0.0;
    double lx = o.xstep, ly = o.ystep;
    for (int it = 0; it < o.iters; ++it) {
        lx = o.reduce * lx;
        ly = o.reduce * ly;
        const double x0 = fmax(o.xmin, px - lx), x1 = fmin(o.xmax - lx, px + lx);
        const double y0 = fmax(o.ymin, py - ly), y1 = fmin(o.ymax - ly, py + ly);
        if (x0 >= x1 || y0 >= y1) continue;
        // numpy.arange(start, stop, step): len = ceil((stop - start) / step), values start + i * ((start + step) - start)
        const int nxl = (int)ceil((x1 - x0) / lx), nyl = (int)ceil((y1 - y0) / ly);
        if (nxl <= 0 || nyl <= 0) continue;
        const double dx = (x0 + lx) - x0, dy = (y0 + ly) - y0;
        double best = -1.0;
        int bidx = 0x7fffffff;
        for (int p = lane; p < nxl * nyl; p += 64) {
            const int pr = p / nxl, pc = p - pr * nxl;
            const double z = pk_point(ph, xbase, ybase, x0 + pc * dx, y0 + pr * dy);
            if (z > best) {   // first arg-max in row-major order: strictly greater replaces, ties keep the lower index
                best = z;
                bidx = p;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (ob > best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        const int pr = bidx / nxl, pc = bidx - pr * nxl;
        px = x0 + pc * dx;
        py = y0 + pr * dy;
        height = best;
    }
}

}  // namespace admmnet
