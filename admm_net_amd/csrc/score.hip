// score.hip -- target estimates scored against ground truth on the device (admm_net_amd/metrics.py; the definitions are
// with admmnet_score_match_f64 / admmnet_score_ordered_f32 in include/admmnet.h, the float64 host statement is
// metrics.match_host).
//   match     one optimal assignment per signal under the truncated cost min(d^2, c^2), the GOSPA assignment: the reference's
//             test/test_model_peaksearch.py:85-97 sorts and cuts both peak lists and prints them, the comparison itself was
//             never written (peak-search rows come in height order, not truth order)
//   ordered   the validation / test RMSE of train.py:262-274, 388-408, slot j against slot j
//
// Launch shape and sums: slab_partials.h, as loss.hip -- one wave per signal, four signals per workgroup; lane j owns column j of
// the assignment and row j's potential (score_core.h has the search, one lane's share of every step).  What the wave adds here:
// the row the path reached is broadcast with __shfl, the free column of least distance is ONE xor-butterfly argmin per step
// under the total order (distance, lane), so every lane holds the same winner and two runs give the same bits, and the path is
// flipped by a walk of __shfl reads.  No LDS or HBM cost matrix, no atomics.  Sums over the batch: one row of float64 partials
// per workgroup, added in a fixed order by ONE workgroup.
#include "common.h"
#include "score_core.h"
#include "batch_sums.h"

namespace admmnet {

constexpr int SC_MATCH_COLS = SC_STATS + 2;   // the stats, then signals whose L_true was outside, signals with a non-finite truth
constexpr int SC_ORD_COLS = 4;                // sum rmse_tau, sum rmse_f, signals with L > 0, signals whose L_true was outside
static_assert(SC_FIN_SLICES * SC_MATCH_COLS <= SC_FIN_THREADS, "one thread per column and slice");
constexpr int SC_STEPS = SC_MAX + 1;          // no search and no path is longer than the columns there are

// ---- the assignment ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void sc_match_kernel(int Le, int Lt, int64_t B, const double *__restrict__ est,
                                                              const int32_t *__restrict__ n_est, const float *__restrict__ tau_true,
                                                              const float *__restrict__ f_true, const int64_t *__restrict__ L_true,
                                                              ScoreOpt o, int32_t *__restrict__ match, double *__restrict__ stats,
                                                              double *__restrict__ part) {
    __shared__ double sh[TS_SLAB * SC_MATCH_COLS];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    double acc[SC_MATCH_COLS];
#pragma unroll
    for (int c = 0; c < SC_MATCH_COLS; ++c) acc[c] = 0.0;
    if (sig < B) {
        bool outside = false;
        const int nt = sc_clamp_count(L_true ? L_true[sig] : (int64_t)Lt, Lt, &outside);
        const bool t_live = !outside && lane < nt;
        double t_tau = 0.0, t_f = 0.0;
        if (t_live) {
            t_tau = (double)tau_true[sig * Lt + lane];
            t_f = (double)f_true[sig * Lt + lane];
        }
        const bool nonfinite = __ballot(t_live && !(sc_finite(t_tau) && sc_finite(t_f))) != 0ull;
        int m = -1;
        if (outside || nonfinite) {
            if (lane < SC_STATS) stats[sig * SC_STATS + lane] = NAN;
            acc[SC_STATS] = outside ? 1.0 : 0.0;
            acc[SC_STATS + 1] = outside ? 0.0 : 1.0;
        } else {
            bool cap_outside;
            const int ne_cap = sc_clamp_count(n_est ? (int64_t)n_est[sig] : (int64_t)Le, Le, &cap_outside);
            double e_tau = 0.0, e_f = 0.0;
            bool e_live = false;
            if (lane < ne_cap) {
                e_tau = est[(sig * Le + lane) * 3];
                e_f = est[(sig * Le + lane) * 3 + 1];
                e_live = sc_finite(e_tau) && sc_finite(e_f);
            }
            const unsigned long long e_mask = __ballot(e_live);
            const int ne = __popcll(e_mask);
            // rows are the smaller side (on a tie the estimates): lane j is column j of the other side and keeps row j's potential
            const bool rows_est = ne <= nt;
            const double r_tau = rows_est ? e_tau : t_tau, r_f = rows_est ? e_f : t_f;
            unsigned long long rows = rows_est ? e_mask : (nt >= 64 ? ~0ull : ((1ull << nt) - 1ull));
            ScCol col;
            sc_col_init(col, rows_est ? t_tau : e_tau, rows_est ? t_f : e_f, rows_est ? t_live : e_live);
            double u = 0.0;
            while (rows) {
                const int root = __ffsll((long long)rows) - 1;
                rows &= rows - 1ull;
                sc_col_begin(col);
                bool in_tree = lane == root;
                int cur = root, j0 = -1;
                for (int step = 0; step < SC_STEPS; ++step) {
                    sc_relax(col, __shfl(r_tau, cur, 64), __shfl(r_f, cur, 64), __shfl(u, cur, 64), j0, o);
                    double key = sc_key(col);
                    int arg = lane;
#pragma unroll
                    for (int x = 32; x > 0; x >>= 1) {
                        const double k2 = __shfl_xor(key, x, 64);
                        const int a2 = __shfl_xor(arg, x, 64);
                        if (sc_better(key, arg, k2, a2)) {
                            key = k2;
                            arg = a2;
                        }
                    }
                    sc_shift(col, u, in_tree, key);
                    col.used = col.used || lane == arg;
                    j0 = arg;
                    cur = __shfl(col.p, arg, 64);
                    if (cur < 0) break;
                    in_tree = in_tree || lane == cur;
                }
                // flip the path: every column on it takes the row of the column before it, the first one the root
                for (int step = 0; step < SC_STEPS && j0 >= 0; ++step) {
                    const int before = __shfl(col.way, j0, 64);
                    const int row = __shfl(col.p, before < 0 ? 0 : before, 64);
                    if (lane == j0) col.p = before < 0 ? root : row;
                    j0 = before;
                }
            }
            // the pairs, seen from the columns
            const int src = col.p < 0 ? 0 : col.p;
            const ScDelta d = sc_delta(__shfl(r_tau, src, 64), __shfl(r_f, src, 64), col.tau, col.f, o);   // as sc_relax saw it
            const bool hit = col.live && col.p >= 0 && sc_hit(d.d2, o.c2);
            const double n_hit = wave_sum(hit ? 1.0 : 0.0), s_tau = wave_sum(hit ? d.dtau * d.dtau : 0.0),
                         s_f = wave_sum(hit ? d.df * d.df : 0.0), s_d2 = wave_sum(hit ? d.d2 : 0.0);
            if (rows_est) {
                m = hit ? col.p : -1;                       // lane = truth, p = its estimate
            } else {
                for (int e = 0; e < Le; ++e) {               // lane = estimate, p = its truth: hand e to that lane
                    const int t = __shfl(col.p, e, 64);
                    const bool h = __shfl((int)hit, e, 64) != 0;
                    if (h && lane == t) m = e;
                }
            }
            sc_stats(ne, nt, n_hit, s_tau, s_f, s_d2, o.c2, acc);
            if (lane < SC_STATS) {
                double mine = acc[0];
#pragma unroll
                for (int c = 1; c < SC_STATS; ++c) mine = lane == c ? acc[c] : mine;
                stats[sig * SC_STATS + lane] = mine;
            }
        }
        if (lane < Lt) match[sig * Lt + lane] = m;
    }
    sc_slab_partials<SC_MATCH_COLS>(acc, sh, part);
}

__global__ __launch_bounds__(SC_FIN_THREADS) void sc_match_finish_kernel(int64_t rows, const double *__restrict__ part,
                                                                         double *__restrict__ totals, int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_SLICES * SC_MATCH_COLS];
    colsum<SC_MATCH_COLS, SC_FIN_SLICES>(rows, part, sh);
    if ((int)threadIdx.x < SC_STATS) totals[threadIdx.x] = sh[threadIdx.x];
    if (threadIdx.x == 0) {
        status[0] = sc_count(sh[SC_STATS]);
        status[1] = sc_count(sh[SC_STATS + 1]);
    }
}

// ---- the ordered RMSE --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void sc_ordered_kernel(int Lmax, int64_t B, const float *__restrict__ tau_est,
                                                                const float *__restrict__ f_est, const float *__restrict__ tau_true,
                                                                const float *__restrict__ f_true, const int64_t *__restrict__ L_true,
                                                                double *__restrict__ per_sample, double *__restrict__ part) {
    __shared__ double sh[TS_SLAB * SC_ORD_COLS];
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    double acc[SC_ORD_COLS] = {0.0, 0.0, 0.0, 0.0};
    if (sig < B) {
        bool outside;
        const int L = sc_clamp_count(L_true[sig], Lmax, &outside);
        double dt = 0.0, df = 0.0;
        if (lane < L) {
            const int64_t e = sig * Lmax + lane;
            dt = (double)tau_est[e] - (double)tau_true[e];
            df = (double)f_est[e] - (double)f_true[e];
        }
        const double st = wave_sum(dt * dt), sf = wave_sum(df * df);
        const double rt = L > 0 ? sqrt(st / (double)L) : NAN, rf = L > 0 ? sqrt(sf / (double)L) : NAN;
        if (lane < 2) per_sample[sig * 2 + lane] = lane == 0 ? rt : rf;
        if (L > 0) {
            acc[0] = rt;
            acc[1] = rf;
            acc[2] = 1.0;
        }
        acc[3] = outside ? 1.0 : 0.0;
    }
    sc_slab_partials<SC_ORD_COLS>(acc, sh, part);
}

__global__ __launch_bounds__(SC_FIN_THREADS) void sc_ordered_finish_kernel(int64_t rows, const double *__restrict__ part,
                                                                           double *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_SLICES * SC_ORD_COLS];
    colsum<SC_ORD_COLS, SC_FIN_SLICES>(rows, part, sh);
    if (threadIdx.x == 0) {
        const double count = sh[2];
        out[0] = count > 0.0 ? sh[0] / count : 0.0;
        out[1] = count > 0.0 ? sh[1] / count : 0.0;
        out[2] = count;
        status[0] = sc_count(sh[3]);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t score_partials(int64_t B) { return train_small_rows(B) * SC_MATCH_COLS; }   // doubles; the ordered sum uses fewer

int launch_score_match(int Le, int Lt, int64_t B, const double *est, const int32_t *n_est, const float *tau_true,
                       const float *f_true, const int64_t *L_true, const double *opts, int32_t *match, double *stats, double *totals,
                       int32_t *status, double *part, hipStream_t st) {
    const ScoreOpt o = {opts[0], opts[1], opts[2] * opts[2], opts[3], opts[4]};
    const int64_t rows = train_small_rows(B);
    hipLaunchKernelGGL(sc_match_kernel, dim3((unsigned)rows), dim3(TS_THREADS), 0, st, Le, Lt, B, est, n_est, tau_true, f_true,
                       L_true, o, match, stats, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_match_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, rows, part, totals, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_score_ordered(int Lmax, int64_t B, const float *tau_est, const float *f_est, const float *tau_true, const float *f_true,
                         const int64_t *L_true, double *per_sample, double *out, int32_t *status, double *part, hipStream_t st) {
    const int64_t rows = train_small_rows(B);
    hipLaunchKernelGGL(sc_ordered_kernel, dim3((unsigned)rows), dim3(TS_THREADS), 0, st, Lmax, B, tau_est, f_est, tau_true, f_true,
                       L_true, per_sample, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_ordered_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, rows, part, out, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
