// loss_spectrum.hip -- the terms of the phi loss that are defined on the delay-Doppler spectrum (admm_net_amd/losses.py,
// PhiSpectralLoss; the tensor stand-in there is the definition the tests hold these kernels to).  With the atom
// a(tau, f)[ks xbase + kd] = exp(j 2 pi (ks f - kd tau)), z(tau, f) = sum_i conj(phi[i]) a(tau, f)[i], S = |z|^2 (the image of
// spectrum.hip) on the uniform full-period grid of G = nx ny points, m = mean_grid S, and S*, z*, m* the same of phi_true:
//   spectral_b     = mean_grid (S / m - S* / m*)^2
//   distribution_b = 1 - sum_grid |z| |z*| / sqrt(sum_grid S  sum_grid S*)
//   target_b       = mean_{l<L} (1 - rho_l),  rho_l = |z(tau_l, f_l)|^2 / (D ||phi||^2),  0 for L = 0
// and out = {ws spectral + wd distribution + wt target, spectral, distribution, target}, each term its mean over the batch.
//
// One workgroup per signal, float64.  Forward: phi and phi_true go to LDS once; z and z* come from the separable contraction
// of sp_image (peak_core.h) chunk by chunk; z and S* are SAVED in the workspace (m has to be known before the spectral sum
// can be formed, so the forward reads them a second time anyway, and the backward is spared the whole contraction); the L
// point values take one wave each.  A finish kernel adds the per-signal rows over the batch (la_phi_finish_kernel's scheme).
// Backward: C = c conj(z) over the grid in LDS, c = d total / d S, contracted back through the two tables,
//   g[ks][kd] = 2 sum_q s_q[ks] sum_p C[q][p] conj(d_p[kd]),
// plus the target rows 2 c_l conj(z_l) a_l and the derivative of ||phi||^2.  Every sum has a fixed order (a thread's own
// strided terms, a xor butterfly, the four waves in order): a signal's figures depend on neither B nor its place.
#include "common.h"
#include "batch_sums.h"

namespace admmnet {

constexpr int LS_THREADS = 256, LS_WAVES = LS_THREADS / 64, LS_XCHUNK = 64;
constexpr int LS_ROW = 48;    // doubles per signal in the workspace: the six summed columns, the scalars of the backward, z_l
constexpr int LS_COLS = 6;    // spectral, distribution, target, L_true outside [0, Lmax], zero phi row, zero phi_true row
enum { LS_SPEC = 0, LS_DIST, LS_TARG, LS_OUTSIDE, LS_ZERO, LS_ZERO_TRUE, LS_M, LS_MT, LS_H, LS_E, LS_N2, LS_LIVE, LS_L, LS_GRID, LS_Z = 16 };
static_assert(LS_Z + 2 * LS_MAX_TARGETS <= LS_ROW, "a row holds every z_l");
constexpr size_t LS_LDS_MAX = 150 * 1024;

static int64_t ls_align(int64_t v) { return (v + 255) / 256 * 256; }

struct LsLayout {   // byte offsets into the workspace
    int nx, ny;
    int64_t G, tabD, tabS, axes, rows, z, st, bytes;
};

static LsLayout ls_layout(int xbase, int ybase, int r, int64_t B) {
    LsLayout w;
    w.nx = xbase > 1 ? r * xbase : 1;
    w.ny = ybase > 1 ? r * ybase : 1;
    w.G = (int64_t)w.nx * w.ny;
    w.tabD = 0;
    w.tabS = w.tabD + ls_align((int64_t)sizeof(double2) * w.nx * xbase);
    w.axes = w.tabS + ls_align((int64_t)sizeof(double2) * w.ny * ybase);
    w.rows = w.axes + ls_align((int64_t)sizeof(double) * (w.nx + w.ny));
    w.z = w.rows + ls_align((int64_t)sizeof(double) * LS_ROW * B);
    w.st = w.z + ls_align((int64_t)sizeof(double2) * w.G * B);
    w.bytes = w.st + ls_align((int64_t)sizeof(double) * w.G * B);
    return w;
}

// LDS of the two kernels, in bytes; every carve is a multiple of 16
static size_t ls_lds_fwd(int xbase, int ybase, int Lmax) {
    return sizeof(double2) * ((size_t)2 * xbase * ybase + (size_t)2 * ybase * LS_XCHUNK + (size_t)Lmax * (xbase + ybase) +
                              LS_MAX_TARGETS + 2 * LS_WAVES);
}
static size_t ls_lds_bwd(int xbase, int ybase, int nx, int ny, int Lmax) {
    return sizeof(double2) * ((size_t)xbase * ybase + (size_t)nx * ny + (size_t)ny * xbase + (size_t)Lmax * (xbase + ybase));
}

// the sums of K per-thread values over the workgroup, in every thread; red: LDS [LS_WAVES * K], free again on return
template <int K>
__device__ __forceinline__ void ls_block_sum(double (&v)[K], double *red) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
    __syncthreads();
}
static_assert(LS_WAVES == 4, "ls_block_sum adds four waves");

// exp(j 2 pi t), the argument reduced to a fraction of a turn (rf_turn of refine_core.h)
__device__ __forceinline__ double2 ls_turn(double t) {
    double s, c;
    sincospi(2.0 * (t - rint(t)), &s, &c);
    return make_double2(c, s);
}

// the twiddles of the first L target rows: tw[l][k] = exp(j 2 pi k f_l) for k < ybase, exp(-j 2 pi (k - ybase) tau_l) above
__device__ __forceinline__ void ls_twiddles(int xbase, int ybase, int L, const float *__restrict__ tau, const float *__restrict__ f,
                                            double2 *tw) {
    const int span = xbase + ybase;
    for (int item = threadIdx.x; item < L * span; item += LS_THREADS) {
        const int l = item / span, k = item - l * span;
        tw[item] = k < ybase ? ls_turn((double)k * (double)f[l]) : ls_turn(-((double)(k - ybase) * (double)tau[l]));
    }
}

__device__ __forceinline__ int ls_targets(const int64_t *__restrict__ L_true, int64_t sig, int Lmax, bool *outside) {
    const int64_t raw = L_true[sig];
    *outside = raw < 0 || raw > Lmax;
    return raw < 0 ? 0 : (raw > Lmax ? Lmax : (int)raw);
}

__global__ void ls_axes_kernel(int nx, int ny, double *__restrict__ axes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nx) axes[i] = (double)i / (double)nx;
    else if (i < nx + ny) axes[i] = -0.5 + (double)(i - nx) / (double)ny;
}

__global__ __launch_bounds__(LS_THREADS) void ls_fwd_kernel(int xbase, int ybase, int nx, int ny, int Lmax,
                                                            const float2 *__restrict__ phi, const float2 *__restrict__ phi_true,
                                                            const float *__restrict__ tau_true, const float *__restrict__ f_true,
                                                            const int64_t *__restrict__ L_true, const double2 *__restrict__ tabD,
                                                            const double2 *__restrict__ tabS, double *__restrict__ rows,
                                                            double2 *__restrict__ zws, double *__restrict__ sws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = xbase * ybase, tid = threadIdx.x;
    const int64_t b = blockIdx.x, G = (int64_t)nx * ny;
    double2 *ph = reinterpret_cast<double2 *>(smem);   // [D]
    double2 *pt = ph + D;                              // [D]
    double2 *U = pt + D;                               // [ybase][LS_XCHUNK]
    double2 *Ut = U + ybase * LS_XCHUNK;               // [ybase][LS_XCHUNK]
    double2 *tw = Ut + ybase * LS_XCHUNK;              // [Lmax][xbase + ybase]
    double2 *zl = tw + Lmax * (xbase + ybase);         // [LS_MAX_TARGETS]
    double *red = reinterpret_cast<double *>(zl + LS_MAX_TARGETS);   // [4 LS_WAVES]
    const bool grid = phi_true != nullptr, targ = L_true != nullptr;

    double n[2] = {0.0, 0.0};
    for (int i = tid; i < D; i += LS_THREADS) {
        const float2 p = phi[b * D + i];
        ph[i] = make_double2((double)p.x, (double)p.y);
        n[0] += (double)p.x * (double)p.x + (double)p.y * (double)p.y;
        if (grid) {
            const float2 t = phi_true[b * D + i];
            pt[i] = make_double2((double)t.x, (double)t.y);
            n[1] += (double)t.x * (double)t.x + (double)t.y * (double)t.y;
        }
    }
    ls_block_sum<2>(n, red);                           // (its barriers make ph and pt visible)
    const double n2 = n[0];
    const bool live = n2 > 0.0 && (!grid || n[1] > 0.0);
    double spec = 0.0, dist = 0.0, target = 0.0, m = 0.0, mt = 0.0, H = 0.0, E = 0.0;

    if (grid && live) {
        double2 *zb = zws + b * G;
        double *sb = sws + b * G;
        double acc[3] = {0.0, 0.0, 0.0};               // sum S, sum S*, sum |z| |z*|
        for (int x0 = 0; x0 < nx; x0 += LS_XCHUNK) {
            const int xw = min(LS_XCHUNK, nx - x0);
            for (int p = tid; p < ybase * xw; p += LS_THREADS) {
                const int ks = p / xw, xl = p - ks * xw;
                const double2 *d = tabD + (int64_t)(x0 + xl) * xbase;
                double ur = 0.0, ui = 0.0, vr = 0.0, vi = 0.0;
                for (int kd = 0; kd < xbase; ++kd) {   // conj(phi) conj(d) = conj(phi d)
                    const double2 a = ph[ks * xbase + kd], t = pt[ks * xbase + kd], e = d[kd];
                    ur += a.x * e.x - a.y * e.y;
                    ui -= a.y * e.x + a.x * e.y;
                    vr += t.x * e.x - t.y * e.y;
                    vi -= t.y * e.x + t.x * e.y;
                }
                U[ks * LS_XCHUNK + xl] = make_double2(ur, ui);
                Ut[ks * LS_XCHUNK + xl] = make_double2(vr, vi);
            }
            __syncthreads();
            for (int p = tid; p < ny * xw; p += LS_THREADS) {
                const int iy = p / xw, xl = p - iy * xw;
                const double2 *s = tabS + (int64_t)iy * ybase;
                double zr = 0.0, zi = 0.0, tr = 0.0, ti = 0.0;
                for (int ks = 0; ks < ybase; ++ks) {
                    const double2 a = s[ks], u = U[ks * LS_XCHUNK + xl], v = Ut[ks * LS_XCHUNK + xl];
                    zr += a.x * u.x - a.y * u.y;
                    zi += a.y * u.x + a.x * u.y;
                    tr += a.x * v.x - a.y * v.y;
                    ti += a.y * v.x + a.x * v.y;
                }
                const double S = zr * zr + zi * zi, St = tr * tr + ti * ti;
                const int64_t k = (int64_t)iy * nx + x0 + xl;
                zb[k] = make_double2(zr, zi);
                sb[k] = St;
                acc[0] += S;
                acc[1] += St;
                acc[2] += sqrt(S * St);
            }
            __syncthreads();                           // (also: zb and sb are visible to the workgroup)
        }
        ls_block_sum<3>(acc, red);
        H = acc[2];
        m = acc[0] / (double)G;
        mt = acc[1] / (double)G;
        double q[2] = {0.0, 0.0};                      // sum (u - v)^2, sum (u - v) u
        for (int64_t k = tid; k < G; k += LS_THREADS) {
            const double2 z = zb[k];
            const double u = (z.x * z.x + z.y * z.y) / m, d = u - sb[k] / mt;
            q[0] += d * d;
            q[1] += d * u;
        }
        ls_block_sum<2>(q, red);
        spec = q[0] / (double)G;
        E = q[1] / (double)G;
        dist = 1.0 - H / sqrt(acc[0] * acc[1]);
    }

    bool outside = false;
    int L = 0;
    if (targ) L = ls_targets(L_true, b, Lmax, &outside);
    if (tid < LS_MAX_TARGETS) zl[tid] = make_double2(0.0, 0.0);
    if (targ && live && L > 0) {
        ls_twiddles(xbase, ybase, L, tau_true + b * Lmax, f_true + b * Lmax, tw);
        __syncthreads();
        const int lane = tid & 63, span = xbase + ybase;
        for (int l = tid >> 6; l < L; l += LS_WAVES) {  // one wave per target row
            double zr = 0.0, zi = 0.0;
            for (int i = lane; i < D; i += 64) {
                const int ks = i / xbase, kd = i - ks * xbase;
                const double2 a = ph[i], ef = tw[l * span + ks], et = tw[l * span + ybase + kd];
                const double er = ef.x * et.x - ef.y * et.y, ei = ef.x * et.y + ef.y * et.x;
                zr += a.x * er + a.y * ei;             // conj(phi) a
                zi += a.x * ei - a.y * er;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                zr += __shfl_xor(zr, o, 64);
                zi += __shfl_xor(zi, o, 64);
            }
            if (lane == 0) zl[l] = make_double2(zr, zi);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (targ && live && L > 0) {
            double s = 0.0;
            for (int l = 0; l < L; ++l) s += 1.0 - (zl[l].x * zl[l].x + zl[l].y * zl[l].y) / ((double)D * n2);
            target = s / (double)L;
        }
        double *row = rows + b * LS_ROW;
        row[LS_SPEC] = spec;
        row[LS_DIST] = dist;
        row[LS_TARG] = target;
        row[LS_OUTSIDE] = outside ? 1.0 : 0.0;
        row[LS_ZERO] = n2 > 0.0 ? 0.0 : 1.0;
        row[LS_ZERO_TRUE] = grid && !(n[1] > 0.0) ? 1.0 : 0.0;
        row[LS_M] = m;
        row[LS_MT] = mt;
        row[LS_H] = H;
        row[LS_E] = E;
        row[LS_N2] = n2;
        row[LS_LIVE] = live ? 1.0 : 0.0;
        row[LS_L] = (double)L;
        row[LS_GRID] = grid ? 1.0 : 0.0;               // (the backward reads z and S* only where the forward wrote them)
        for (int k = LS_GRID + 1; k < LS_Z; ++k) row[k] = 0.0;
        for (int l = 0; l < LS_MAX_TARGETS; ++l) {
            row[LS_Z + 2 * l] = zl[l].x;
            row[LS_Z + 2 * l + 1] = zl[l].y;
        }
    }
}

// the six columns of rows [B][LS_ROW] added in float64 in a fixed order (colsum of batch_sums.h over LS_ROW-strided rows)
__global__ __launch_bounds__(LS_THREADS) void ls_finish_kernel(int64_t B, const double *__restrict__ rows, float spectral_weight,
                                                               float distribution_weight, float target_weight,
                                                               float *__restrict__ out, int32_t *__restrict__ status) {
    constexpr int NS = 32;
    static_assert(NS * LS_COLS <= LS_THREADS, "one thread per column and slice");
    __shared__ double sh[NS * LS_COLS];
    colsum(LS_COLS, NS, B, LS_ROW, rows, sh);
    if (threadIdx.x == 0) {
        const double spec = sh[LS_SPEC] / (double)B, dist = sh[LS_DIST] / (double)B, targ = sh[LS_TARG] / (double)B;
        out[0] = (float)((double)spectral_weight * spec + (double)distribution_weight * dist + (double)target_weight * targ);
        out[1] = (float)spec;
        out[2] = (float)dist;
        out[3] = (float)targ;
        for (int k = 0; k < 3; ++k) status[k] = (int32_t)fmin(sh[LS_OUTSIDE + k], 2147483647.0);   // counts of ones; saturates
    }
}

// with cs = (g_out[0] ws + g_out[1]) / B, cd = (g_out[0] wd + g_out[2]) / B, ct = (g_out[0] wt + g_out[3]) / B, u = S / m,
// v = S* / m*, E = mean_grid (u - v) u, A = sum S, A* = sum S*, H = sum |z| |z*|:
//   c = cs 2 / (G m) ((u - v) - E) - cd / (2 sqrt(A A*)) (|z*| / |z| - H / A)          (the ratio taken as 0 where z = 0)
//   g_phi[i] = 2 sum_grid c conj(z) a[i] - 2 ct / L sum_{l<L} (conj(z_l) a_l[i] / (D n2) - rho_l phi[i] / n2)
__global__ __launch_bounds__(LS_THREADS) void ls_bwd_kernel(int xbase, int ybase, int nx, int ny, int Lmax, double inv_B,
                                                            const float *__restrict__ g_out, const float2 *__restrict__ phi,
                                                            const float *__restrict__ tau_true, const float *__restrict__ f_true,
                                                            float spectral_weight, float distribution_weight, float target_weight,
                                                            int skip, const double2 *__restrict__ tabD,
                                                            const double2 *__restrict__ tabS, const double *__restrict__ rows,
                                                            const double2 *__restrict__ zws, const double *__restrict__ sws,
                                                            float2 *__restrict__ g_phi) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = xbase * ybase, tid = threadIdx.x, span = xbase + ybase;
    const int64_t b = blockIdx.x, G = (int64_t)nx * ny;
    double2 *ph = reinterpret_cast<double2 *>(smem);   // [D]
    double2 *C = ph + D;                               // [ny][nx]
    double2 *V = C + G;                                // [ny][xbase]
    double2 *tw = V + ny * xbase;                      // [Lmax][xbase + ybase]
    const double *row = rows + b * LS_ROW;
    if (row[LS_LIVE] == 0.0) {                         // (the same for every thread of the workgroup)
        for (int i = tid; i < D; i += LS_THREADS) g_phi[b * D + i] = make_float2(0.f, 0.f);
        return;
    }
    const double g0 = (double)g_out[0];
    const double cs = (skip & ADMMNET_LOSS_SPECTRUM_SKIP_SPECTRAL) ? 0.0 : (g0 * (double)spectral_weight + (double)g_out[1]) * inv_B;
    const double cd = (skip & ADMMNET_LOSS_SPECTRUM_SKIP_DISTRIBUTION) ? 0.0
                                                                       : (g0 * (double)distribution_weight + (double)g_out[2]) * inv_B;
    const double ct = (skip & ADMMNET_LOSS_SPECTRUM_SKIP_TARGET) ? 0.0 : (g0 * (double)target_weight + (double)g_out[3]) * inv_B;
    const bool grid = row[LS_GRID] != 0.0 &&           // (a forward without phi_true left no z: its grid terms are constants)
                      (skip & (ADMMNET_LOSS_SPECTRUM_SKIP_SPECTRAL | ADMMNET_LOSS_SPECTRUM_SKIP_DISTRIBUTION)) !=
                          (ADMMNET_LOSS_SPECTRUM_SKIP_SPECTRAL | ADMMNET_LOSS_SPECTRUM_SKIP_DISTRIBUTION);
    const int L = (skip & ADMMNET_LOSS_SPECTRUM_SKIP_TARGET) ? 0 : min((int)row[LS_L], Lmax);
    const double n2 = row[LS_N2];

    for (int i = tid; i < D; i += LS_THREADS) {
        const float2 p = phi[b * D + i];
        ph[i] = make_double2((double)p.x, (double)p.y);
    }
    if (L > 0) ls_twiddles(xbase, ybase, L, tau_true + b * Lmax, f_true + b * Lmax, tw);
    if (grid) {
        const double m = row[LS_M], mt = row[LS_MT], H = row[LS_H], E = row[LS_E];
        const double A = m * (double)G, At = mt * (double)G;
        const double ks_ = cs * 2.0 / ((double)G * m), kd_ = -cd / (2.0 * sqrt(A * At)), HA = H / A;
        const double2 *zb = zws + b * G;
        const double *sb = sws + b * G;
        for (int64_t k = tid; k < G; k += LS_THREADS) {
            const double2 z = zb[k];
            const double St = sb[k], S = z.x * z.x + z.y * z.y;
            double c = ks_ * ((S / m - St / mt) - E);
            if (S > 0.0) c += kd_ * (sqrt(St / S) - HA);
            C[k] = make_double2(c * z.x, -(c * z.y));
        }
        __syncthreads();
        for (int o = tid; o < ny * xbase; o += LS_THREADS) {   // V[q][kd] = sum_p C[q][p] conj(d_p[kd])
            const int q = o / xbase, kd = o - q * xbase;
            double vr = 0.0, vi = 0.0;
            for (int p = 0; p < nx; ++p) {
                const double2 c = C[q * nx + p], e = tabD[(int64_t)p * xbase + kd];
                vr += c.x * e.x + c.y * e.y;
                vi += c.y * e.x - c.x * e.y;
            }
            V[o] = make_double2(vr, vi);
        }
    }
    __syncthreads();                                   // ph, tw and V are visible
    for (int i = tid; i < D; i += LS_THREADS) {
        const int ks = i / xbase, kd = i - ks * xbase;
        double gr = 0.0, gi = 0.0;
        if (grid) {
            for (int q = 0; q < ny; ++q) {             // 2 sum_q s_q[ks] V[q][kd]
                const double2 s = tabS[(int64_t)q * ybase + ks], v = V[q * xbase + kd];
                gr += s.x * v.x - s.y * v.y;
                gi += s.x * v.y + s.y * v.x;
            }
            gr *= 2.0;
            gi *= 2.0;
        }
        if (L > 0) {
            double tr = 0.0, ti = 0.0;
            const double dn = (double)D * n2;
            for (int l = 0; l < L; ++l) {
                const double zr = row[LS_Z + 2 * l], zi = row[LS_Z + 2 * l + 1], rho = (zr * zr + zi * zi) / dn;
                const double2 ef = tw[l * span + ks], et = tw[l * span + ybase + kd];
                const double er = ef.x * et.x - ef.y * et.y, ei = ef.x * et.y + ef.y * et.x;
                tr += (zr * er + zi * ei) / dn - rho * ph[i].x / n2;   // conj(z_l) a_l
                ti += (zr * ei - zi * er) / dn - rho * ph[i].y / n2;
            }
            const double k = -2.0 * ct / (double)L;
            gr += k * tr;
            gi += k * ti;
        }
        g_phi[b * D + i] = make_float2((float)gr, (float)gi);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t loss_spectrum_workspace_bytes(int xbase, int ybase, int oversample, int64_t B) {
    const LsLayout w = ls_layout(xbase, ybase, oversample, B);
    if (ls_lds_fwd(xbase, ybase, LS_MAX_TARGETS) > LS_LDS_MAX || ls_lds_bwd(xbase, ybase, w.nx, w.ny, LS_MAX_TARGETS) > LS_LDS_MAX)
        return -1;
    return w.bytes;
}

int launch_loss_spectrum(int xbase, int ybase, int oversample, int Lmax, int64_t B, const float2 *phi, const float2 *phi_true,
                         const float *tau_true, const float *f_true, const int64_t *L_true, float spectral_weight,
                         float distribution_weight, float target_weight, float *out, int32_t *status, void *workspace,
                         hipStream_t st) {
    const LsLayout w = ls_layout(xbase, ybase, oversample, B);
    char *base = (char *)workspace;
    double2 *tabD = (double2 *)(base + w.tabD), *tabS = (double2 *)(base + w.tabS);
    double *axes = (double *)(base + w.axes), *rows = (double *)(base + w.rows);
    hipLaunchKernelGGL(ls_axes_kernel, dim3((w.nx + w.ny + 255) / 256), dim3(256), 0, st, w.nx, w.ny, axes);
    ADMM_HIP(hipGetLastError());
    if (int rc = launch_spectrum_tables(axes, w.nx, xbase, axes + w.nx, w.ny, ybase, tabD, tabS, st)) return rc;
    const size_t lds = ls_lds_fwd(xbase, ybase, Lmax);
    ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ls_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ls_fwd_kernel, dim3((unsigned)B), dim3(LS_THREADS), lds, st, xbase, ybase, w.nx, w.ny, Lmax, phi, phi_true,
                       tau_true, f_true, L_true, tabD, tabS, rows, (double2 *)(base + w.z), (double *)(base + w.st));
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ls_finish_kernel, dim3(1), dim3(LS_THREADS), 0, st, B, rows, spectral_weight, distribution_weight,
                       target_weight, out, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_loss_spectrum_bwd(int xbase, int ybase, int oversample, int Lmax, int64_t B, const float *g_out, const float2 *phi,
                             const float *tau_true, const float *f_true, const int64_t *L_true, float spectral_weight,
                             float distribution_weight, float target_weight, int skip, const void *workspace, float2 *g_phi,
                             hipStream_t st) {
    (void)L_true;                                      // (the forward left L, held to [0, Lmax], in the signal's row)
    const LsLayout w = ls_layout(xbase, ybase, oversample, B);
    const char *base = (const char *)workspace;
    const size_t lds = ls_lds_bwd(xbase, ybase, w.nx, w.ny, Lmax);
    ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ls_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ls_bwd_kernel, dim3((unsigned)B), dim3(LS_THREADS), lds, st, xbase, ybase, w.nx, w.ny, Lmax, 1.0 / (double)B,
                       g_out, phi, tau_true, f_true, spectral_weight, distribution_weight, target_weight, skip,
                       (const double2 *)(base + w.tabD), (const double2 *)(base + w.tabS), (const double *)(base + w.rows),
                       (const double2 *)(base + w.z), (const double *)(base + w.st), g_phi);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
