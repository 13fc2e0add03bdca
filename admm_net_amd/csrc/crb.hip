// crb.hip -- the Cramer-Rao bound of a scene's targets on the device (admm_net_amd/metrics.py: crb; the definition is with
// admmnet_crb_f64 in include/admmnet.h, the float64 host statement is metrics.crb_host).
//
// One wave per scene, one scene per workgroup; crb_core.h has one lane's share of every step.  The lanes are spread over the target
// pairs l <= m for the power sums (a serial loop over k < max(Nb, Nd) each), then lane i owns row i of the unit-diagonal matrix,
// which stays in LDS (P x P float64, P <= 64: at most 32 KiB): one pivot broadcast with __shfl and one barrier per column of the
// Cholesky factor, then lane c inverts its column of the trailing (tau, f) block.  Sums over the batch: batch_sums.h, one row of
// float64 partials per scene added in a fixed order by ONE workgroup -- no atomics, two runs give the same bits.
#include "common.h"
#include "batch_sums.h"
#include "crb_core.h"
#include "score_core.h"

namespace admmnet {

constexpr int CRB_THREADS = 64;
static_assert(SC_FIN_SLICES * CRB_COLS <= SC_FIN_THREADS, "one thread per column and slice");
static_assert(CRB_MAXP <= CRB_THREADS, "one lane per parameter");

__global__ __launch_bounds__(CRB_THREADS) void crb_kernel(int Nb, int Nd, int Lt, const float *__restrict__ tau_true,
                                                          const float *__restrict__ f_true, const float2 *__restrict__ C,
                                                          const int64_t *__restrict__ L_true, const int32_t *__restrict__ match,
                                                          const double *__restrict__ noise, int noise_is_snr,
                                                          double *__restrict__ bound, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char crb_lds[];
    double *A = reinterpret_cast<double *>(crb_lds);   // [(4 Lt)^2]
    __shared__ CrbTarget tg[CRB_MAXL];
    __shared__ double dsc[CRB_MAXP];
    const int64_t sig = blockIdx.x;
    const int lane = threadIdx.x;
    bool outside = false;
    const int nt = sc_clamp_count(L_true ? L_true[sig] : (int64_t)Lt, Lt, &outside);
    const bool live = !outside && lane < nt;
    CrbTarget t = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        const float2 c = C[sig * Lt + lane];
        t.tau = (double)tau_true[sig * Lt + lane];
        t.f = (double)f_true[sig * Lt + lane];
        t.cr = (double)c.x;
        t.ci = (double)c.y;
    }
    const double nz = noise[sig];
    const bool nonfinite = !sc_finite(nz) || (!noise_is_snr && !(nz > 0.0)) ||
                           __ballot(live && !(sc_finite(t.tau) && sc_finite(t.f) && sc_finite(t.cr) && sc_finite(t.ci))) != 0ull;
    int state = outside ? 0 : (nonfinite ? 1 : -1);   // the column of status this scene is counted in, -1: none
    double b_tau = NAN, b_f = NAN;
    if (state < 0 && nt > 0) {   // (uniform over the workgroup, as every branch around a barrier below)
        const bool has_tau = Nd > 1, has_f = Nb > 1;
        const int P = crb_params(nt, has_tau, has_f), ld = P, first = 2 * nt;
        if (live) tg[lane] = t;
        __syncthreads();
        double e = 0.0;
        for (int pr = lane; pr < nt * (nt + 1) / 2; pr += CRB_THREADS) {
            int l, m;
            crb_pair_decode(pr, &l, &m);
            e += crb_pair_fill(l, m, nt, Nb, Nd, tg, A, ld);
        }
        const double v = crb_noise_var(noise_is_snr != 0, nz, wave_sum(e), (double)Nb * (double)Nd);
        __syncthreads();
        if (!(v > 0.0 && sc_finite(v))) {
            state = 1;
        } else {
            bool diag_ok = true;
            if (lane < P) {
                const double g = A[lane * ld + lane];
                diag_ok = g > 0.0 && sc_finite(g);
                dsc[lane] = 1.0 / sqrt(g);
            }
            bool pd = __ballot(!diag_ok) == 0ull;
            __syncthreads();
            if (pd) {
                if (lane < P) crb_scale_row(lane, A, ld, dsc);
                __syncthreads();
                for (int j = 0; j < P; ++j) {
                    const bool mine = lane >= j && lane < P;
                    const double s = mine ? crb_chol_dot(lane, j, A, ld) : 0.0;
                    const double pivot = __shfl(s, j, 64);
                    if (!(pivot >= CRB_PIVOT_MIN)) {
                        pd = false;
                        break;
                    }
                    const double ljj = sqrt(pivot);
                    if (mine) A[j * ld + lane] = lane == j ? ljj : s / ljj;
                    __syncthreads();
                }
            }
            if (!pd) {
                state = 2;
            } else {
                double inv = 0.0;
                if (first + lane < P) {
                    const double d = dsc[first + lane];
                    inv = 0.5 * v * (d * d * crb_inv_diag(first + lane, P, A, ld));
                }
                const int slot = lane < nt ? lane : 0;
                const double vt = __shfl(inv, slot, 64), vf = __shfl(inv, (has_tau ? nt : 0) + slot, 64);
                if (live) {
                    b_tau = has_tau ? vt : INFINITY;
                    b_f = has_f ? vf : INFINITY;
                }
            }
        }
    }
    if (lane < Lt) {
        bound[(sig * Lt + lane) * 2] = b_tau;
        bound[(sig * Lt + lane) * 2 + 1] = b_f;
    }
    const bool hit = live && match != nullptr && match[sig * Lt + lane] >= 0;
    const bool in_tau = live && sc_finite(b_tau), in_f = live && sc_finite(b_f);   // neither NaN nor the inf of an absent axis
    double acc[CRB_COLS];
    acc[0] = wave_sum(in_tau ? b_tau : 0.0);
    acc[1] = wave_sum(in_f ? b_f : 0.0);
    acc[2] = wave_sum(in_tau ? 1.0 : 0.0);
    acc[3] = wave_sum(in_f ? 1.0 : 0.0);
    acc[4] = wave_sum(in_tau && hit ? b_tau : 0.0);
    acc[5] = wave_sum(in_f && hit ? b_f : 0.0);
    acc[6] = wave_sum(in_tau && hit ? 1.0 : 0.0);
    acc[7] = wave_sum(in_f && hit ? 1.0 : 0.0);
#pragma unroll
    for (int c = 0; c < CRB_STATUS; ++c) acc[CRB_TOTALS + c] = state == c ? 1.0 : 0.0;
    if (lane < CRB_COLS) {
        double mine = acc[0];
#pragma unroll
        for (int c = 1; c < CRB_COLS; ++c) mine = lane == c ? acc[c] : mine;
        part[sig * CRB_COLS + lane] = mine;
    }
}

__global__ __launch_bounds__(SC_FIN_THREADS) void crb_finish_kernel(int64_t rows, const double *__restrict__ part,
                                                                    double *__restrict__ totals, int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_SLICES * CRB_COLS];
    colsum<CRB_COLS, SC_FIN_SLICES>(rows, part, sh);
    if ((int)threadIdx.x < CRB_TOTALS) totals[threadIdx.x] = sh[threadIdx.x];
    if ((int)threadIdx.x < CRB_STATUS) status[threadIdx.x] = sc_count(sh[CRB_TOTALS + threadIdx.x]);
}

int64_t crb_partials(int64_t B) { return B * CRB_COLS; }   // doubles: one row per scene

int launch_crb(int Nb, int Nd, int Lt, int64_t B, const float *tau_true, const float *f_true, const float2 *C,
               const int64_t *L_true, const int32_t *match, const double *noise, int noise_is_snr, double *bound, double *totals,
               int32_t *status, double *part, hipStream_t st) {
    const size_t lds = sizeof(double) * (size_t)(4 * Lt) * (size_t)(4 * Lt);
    hipLaunchKernelGGL(crb_kernel, dim3((unsigned)B), dim3(CRB_THREADS), lds, st, Nb, Nd, Lt, tau_true, f_true, C, L_true, match,
                       noise, noise_is_snr, bound, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(crb_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, part, totals, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
