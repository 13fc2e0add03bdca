// loss_set.hip -- the assignment loss of the head (admm_net_amd/losses.py: SetANMLoss; the definition is with
// admmnet_loss_set_f32 in include/admmnet.h, the float64 host statement is losses.set_assign_host plus the tensor stand-in).
// A permutation-invariant loss: the Lmax slots of a signal are matched to its first n targets by the assignment that minimises
// the loss itself; matched slots learn tau, f and conf -> 1, the others conf -> 0.
//
// Launch shape: score.hip's -- one wave per signal, four signals per workgroup; lane j owns column j of the assignment and row
// j's potential.  The search is score_core.h's with the relaxation of set_core.h (the cost c_ij = d2_ij / n + wl (1 - 2 conf_i) is
// recomputed from the coordinates, no cost matrix); the row the path reached is broadcast with __shfl, the free column of least
// distance is one xor-butterfly argmin per step under the total order (distance, lane), the path is flipped by a walk of __shfl
// reads.  Every signal leaves ONE row of SET_COLS float64 values of its own, so its bits depend on neither B, nor its place,
// nor its neighbours; ONE workgroup adds the rows in a fixed order (batch_sums.h) and forms the outputs.  No LDS in the
// forward, no atomics.  The backward is one elementwise launch from the saved assignment and norms.
#include "common.h"
#include "set_core.h"
#include "batch_sums.h"

namespace admmnet {

static_assert(SC_FIN_SLICES * SET_COLS <= SC_FIN_THREADS, "one thread per column and slice");
constexpr int SET_STEPS = SC_MAX + 1;   // no search and no path is longer than the columns there are

struct SetOpt {
    ScoreOpt sc;
    double w_conf, lambda_reg;
};

// what both kernels read of a signal: the slots, the first n targets, and whether any of those values is no number
struct SetSignal {
    double s_tau, s_f, s_conf, t_tau, t_f;
    int n;
    bool outside, nonfinite;
};

__device__ __forceinline__ SetSignal set_load(int Lmax, int Lt, int64_t sig, int lane, const float *__restrict__ tau,
                                              const float *__restrict__ f, const float *__restrict__ conf,
                                              const float *__restrict__ tau_true, const float *__restrict__ f_true,
                                              const int64_t *__restrict__ L_true) {
    SetSignal s;
    s.n = sc_clamp_count(L_true[sig], Lt, &s.outside);
    s.s_tau = s.s_f = s.s_conf = s.t_tau = s.t_f = 0.0;
    if (lane < Lmax) {
        const int64_t e = sig * Lmax + lane;
        s.s_tau = (double)tau[e];
        s.s_f = (double)f[e];
        s.s_conf = (double)conf[e];
    }
    if (lane < s.n) {
        const int64_t e = sig * Lt + lane;
        s.t_tau = (double)tau_true[e];
        s.t_f = (double)f_true[e];
    }
    // (lanes past a side hold zeros, which are finite)
    s.nonfinite = __ballot(!(sc_finite(s.s_tau) && sc_finite(s.s_f) && sc_finite(s.s_conf) && sc_finite(s.t_tau) &&
                             sc_finite(s.t_f))) != 0ull;
    return s;
}

__global__ __launch_bounds__(TS_THREADS) void ls_set_kernel(int Lmax, int Lt, int D, int64_t B, const float *__restrict__ tau,
                                                            const float *__restrict__ f, const float *__restrict__ conf,
                                                            const float *__restrict__ tau_true, const float *__restrict__ f_true,
                                                            const int64_t *__restrict__ L_true, const float2 *__restrict__ phi,
                                                            SetOpt o, int32_t *__restrict__ assign, float *__restrict__ norms,
                                                            double *__restrict__ rows_out) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;   // (no barrier below)
    const int lane = threadIdx.x & 63;
    const SetSignal s = set_load(Lmax, Lt, sig, lane, tau, f, conf, tau_true, f_true, L_true);
    const int n = s.n;
    // ||phi_b||: the squares are exact in float64, so the norm the backward divides by is rounded once (as la_anm_kernel)
    double ss = 0.0;
    for (int i = lane; i < D; i += 64) {
        const float2 p = phi[sig * D + i];
        ss += (double)p.x * (double)p.x + (double)p.y * (double)p.y;
    }
    const float nrm = (float)sqrt(wave_sum(ss));
    if (lane == 0) norms[sig] = nrm;
    double v[SET_COLS] = {0.0, 0.0, 0.0, 0.0, s.outside ? 1.0 : 0.0, s.nonfinite ? 1.0 : 0.0};
    int a = -1;
    if (!s.nonfinite) {
        const bool slot_live = lane < Lmax, t_live = lane < n;
        const double wl = o.w_conf / (double)Lmax, term = set_term(wl, s.s_conf);
        // rows are the smaller side (on a tie the slots): lane j is column j of the other side and keeps row j's potential
        const bool rows_slots = Lmax <= n;
        const double r_tau = rows_slots ? s.s_tau : s.t_tau, r_f = rows_slots ? s.s_f : s.t_f;
        const int nrows = rows_slots ? Lmax : n;
        unsigned long long rows = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
        ScCol col;
        sc_col_init(col, rows_slots ? s.t_tau : s.s_tau, rows_slots ? s.t_f : s.s_f, rows_slots ? t_live : slot_live);
        double u = 0.0;
        while (rows) {
            const int root = __ffsll((long long)rows) - 1;
            rows &= rows - 1ull;
            sc_col_begin(col);
            bool in_tree = lane == root;
            int cur = root, j0 = -1;
            for (int step = 0; step < SET_STEPS; ++step) {
                const double row_term = __shfl(term, cur, 64);
                set_relax(col, rows_slots, __shfl(r_tau, cur, 64), __shfl(r_f, cur, 64), __shfl(u, cur, 64), j0,
                          rows_slots ? row_term : term, n, o.sc);
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
            for (int step = 0; step < SET_STEPS && j0 >= 0; ++step) {
                const int before = __shfl(col.way, j0, 64);
                const int row = __shfl(col.p, before < 0 ? 0 : before, 64);
                if (lane == j0) col.p = before < 0 ? root : row;
                j0 = before;
            }
        }
        // the target of every slot
        if (rows_slots) {
            for (int t = 0; t < n; ++t) {                // lane = target, p = its slot: hand t to that lane
                const int slot = __shfl(col.p, t, 64);
                if (lane == slot) a = t;
            }
        } else {
            a = slot_live ? col.p : -1;                  // lane = slot, p = its target
        }
        const int src = a < 0 ? 0 : a;
        const ScDelta d = sc_delta(s.s_tau, s.s_f, __shfl(s.t_tau, src, 64), __shfl(s.t_f, src, 64), o.sc);   // as set_relax saw it
        const double sum_d2 = wave_sum(a >= 0 ? d.d2 : 0.0);
        const double sum_c = wave_sum(slot_live ? set_conf_sq(s.s_conf, a >= 0) : 0.0);
        set_values(sum_d2, sum_c, n, Lmax, o.w_conf, v);
        v[3] = (double)nrm;
    }
    if (lane < Lmax) assign[sig * Lmax + lane] = a;
    if (lane < SET_COLS) {
        double mine = v[0];
#pragma unroll
        for (int c = 1; c < SET_COLS; ++c) mine = lane == c ? v[c] : mine;
        rows_out[sig * SET_COLS + lane] = mine;
    }
}

__global__ __launch_bounds__(SC_FIN_THREADS) void ls_set_finish_kernel(int64_t B, double w_conf, double lambda_reg,
                                                                       const double *__restrict__ rows, float *__restrict__ out,
                                                                       int32_t *__restrict__ status) {
    __shared__ double sh[SC_FIN_SLICES * SET_COLS];
    colsum<SET_COLS, SC_FIN_SLICES>(B, rows, sh);
    if (threadIdx.x == 0) {
        const double match = sh[1] / (double)B, cf = sh[2] / (double)B, reg = lambda_reg * sh[3] / (double)B;
        out[0] = (float)(match + w_conf * cf + reg);
        out[1] = (float)match;
        out[2] = (float)cf;
        out[3] = (float)reg;
        status[0] = sc_count(sh[4]);
        status[1] = sc_count(sh[5]);
    }
}

// with cm = g_out[0] + g_out[1], cc = g_out[0] w_conf + g_out[2], cr = g_out[0] + g_out[3] and j = assign_i:
//   g_tau_i = cm 2 sx^2 wrap(tau_i - tau_true_j) / (n B) on a matched slot, exactly 0 elsewhere; g_f_i the same with sy and f
//   g_conf_i = cc 2 (conf_i - t_i) / (Lmax B)
//   g_phi_b = cr lambda_reg / B phi_b / ||phi_b||, 0 where the norm is 0 (la_anm_bwd_kernel's)
// a signal with a non-finite value gets zeros throughout
__global__ __launch_bounds__(TS_THREADS) void ls_set_bwd_kernel(int Lmax, int Lt, int D, int64_t B, const float *__restrict__ g_out,
                                                                const float *__restrict__ tau, const float *__restrict__ f,
                                                                const float *__restrict__ conf, const float *__restrict__ tau_true,
                                                                const float *__restrict__ f_true, const int64_t *__restrict__ L_true,
                                                                const float2 *__restrict__ phi, const int32_t *__restrict__ assign,
                                                                const float *__restrict__ norms, SetOpt o, float *__restrict__ g_tau,
                                                                float *__restrict__ g_f, float *__restrict__ g_conf,
                                                                float2 *__restrict__ g_phi) {
    const int64_t sig = (int64_t)blockIdx.x * TS_SLAB + (threadIdx.x >> 6);
    if (sig >= B) return;
    const int lane = threadIdx.x & 63;
    const SetSignal s = set_load(Lmax, Lt, sig, lane, tau, f, conf, tau_true, f_true, L_true);
    const double cm = (double)g_out[0] + (double)g_out[1], cc = (double)g_out[0] * o.w_conf + (double)g_out[2];
    const float cr = g_out[0] + g_out[3], fB = (float)B;
    if (lane < Lmax) {
        const int64_t e = sig * Lmax + lane;
        const int j = assign[e];
        const bool matched = !s.nonfinite && j >= 0 && j < s.n;   // (j < n: a foreign assign reads nothing out of bounds)
        float gt = 0.f, gf = 0.f, gc = 0.f;
        if (matched) {
            const ScDelta d = sc_delta(s.s_tau, s.s_f, (double)tau_true[sig * Lt + j], (double)f_true[sig * Lt + j], o.sc);
            gt = (float)set_grad_coord(cm, o.sc.sx, d.dtau, s.n, B);
            gf = (float)set_grad_coord(cm, o.sc.sy, d.df, s.n, B);
        }
        if (!s.nonfinite) gc = (float)set_grad_conf(cc, s.s_conf, matched, Lmax, B);
        g_tau[e] = gt;
        g_f[e] = gf;
        g_conf[e] = gc;
    }
    const float nrm = norms[sig];
    const bool live = nrm > 0.f && !s.nonfinite;
    const float sc = live ? cr * (float)o.lambda_reg / fB / nrm : 0.f;
    for (int i = lane; i < D; i += 64) {
        const int64_t e = sig * D + i;
        const float2 p = phi[e];
        g_phi[e] = live ? make_float2(sc * p.x, sc * p.y) : make_float2(0.f, 0.f);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t loss_set_partials(int64_t B) { return B * SET_COLS; }   // doubles: one row per signal

int launch_loss_set(int Lmax, int Lt, int D, int64_t B, const float *tau, const float *f, const float *conf, const float *tau_true,
                    const float *f_true, const int64_t *L_true, const float2 *phi, const double *opts, float *out, int32_t *assign,
                    float *norms, int32_t *status, double *part, hipStream_t st) {
    const SetOpt o = {set_score_opt(opts), opts[4], opts[5]};
    hipLaunchKernelGGL(ls_set_kernel, dim3((unsigned)train_small_rows(B)), dim3(TS_THREADS), 0, st, Lmax, Lt, D, B, tau, f, conf,
                       tau_true, f_true, L_true, phi, o, assign, norms, part);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ls_set_finish_kernel, dim3(1), dim3(SC_FIN_THREADS), 0, st, B, o.w_conf, o.lambda_reg, part, out, status);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_loss_set_bwd(int Lmax, int Lt, int D, int64_t B, const float *g_out, const float *tau, const float *f, const float *conf,
                        const float *tau_true, const float *f_true, const int64_t *L_true, const float2 *phi, const int32_t *assign,
                        const float *norms, const double *opts, float *g_tau, float *g_f, float *g_conf, float2 *g_phi,
                        hipStream_t st) {
    const SetOpt o = {set_score_opt(opts), opts[4], opts[5]};
    hipLaunchKernelGGL(ls_set_bwd_kernel, dim3((unsigned)train_small_rows(B)), dim3(TS_THREADS), 0, st, Lmax, Lt, D, B, g_out, tau,
                       f, conf, tau_true, f_true, L_true, phi, assign, norms, o, g_tau, g_f, g_conf, g_phi);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
