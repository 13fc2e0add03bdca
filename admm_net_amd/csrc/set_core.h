// set_core.h -- the scalar core of the assignment loss of the head (loss_set.hip): everything one lane computes, without a wave in
// it, so that tests/host_model/set_model.cpp runs the same arithmetic with the lane loop emulated.
//
// The loss (admmnet_loss_set_f32 in include/admmnet.h has the definition).  Per signal, Lmax slots (tau, f, conf) and the first n
// targets; with wl = w_conf / Lmax the search minimises sum over the matched pairs (slot i, target j) of
//     c_ij = d2_ij / n + wl (1 - 2 conf_i),      d2_ij = (sx wrap(tau_i - tau_true_j))^2 + (sy wrap(f_i - f_true_j))^2,
// a linear assignment with a per-slot term; loss_b = wl sum_i conf_i^2 + that minimum.  The search is score_core.h's (ScCol,
// sc_col_init, sc_col_begin, sc_key, sc_better, sc_shift; rows = the smaller side, lane j = column j): only the relaxation
// differs, it sees c_ij in place of the truncated distance.  d2 is always formed slot minus target (sc_delta), whichever side
// the rows are, so the search, the values and the backward see one number per pair.
#pragma once
#include "score_core.h"

namespace admmnet {

constexpr int SET_OPTS = 6;   // sx, sy, period_tau, period_f, w_conf, lambda_reg
constexpr int SET_COLS = 6;   // per-signal row: loss_b, match_b, conf_b, ||phi_b||, L_true outside [0, Lt], a non-finite value

// scales > 0, periods >= 0, w_conf >= 0, lambda_reg >= 0, all finite
SC_HD bool set_opts_ok(const double *o) {
    return o[0] > 0.0 && sc_finite(o[0]) && o[1] > 0.0 && sc_finite(o[1]) && o[2] >= 0.0 && sc_finite(o[2]) && o[3] >= 0.0 &&
           sc_finite(o[3]) && o[4] >= 0.0 && sc_finite(o[4]) && o[5] >= 0.0 && sc_finite(o[5]);
}

SC_HD ScoreOpt set_score_opt(const double *o) { return ScoreOpt{o[0], o[1], INFINITY, o[2], o[3]}; }

// the per-slot term of c_ij
SC_HD double set_term(double wl, double conf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t = 2.0 * conf;
    return wl * (1.0 - t);
}

// c_ij from d2_ij, n >= 1 and the slot's term
SC_HD double set_cost(double d2, int n, double term) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = d2 / (double)n;
    return q + term;
}

// sc_relax under c_ij.  `rows_slots`: the rows are the slots and column c is a target, else the other way round; `term` is the
// term of the slot of the pair (the row's or the column's own).
SC_HD void set_relax(ScCol &c, bool rows_slots, double row_tau, double row_f, double u, int from, double term, int n,
                     const ScoreOpt &o) {
    if (!c.live || c.used) return;
    const ScDelta d = rows_slots ? sc_delta(row_tau, row_f, c.tau, c.f, o) : sc_delta(c.tau, c.f, row_tau, row_f, o);
    const double cur = set_cost(d.d2, n, term) - u - c.v;
    if (cur < c.minv) {
        c.minv = cur;
        c.way = from;
    }
}

// (conf_i - t_i)^2, t_i = 1 on a matched slot
SC_HD double set_conf_sq(double conf, bool matched) {
    const double e = conf - (matched ? 1.0 : 0.0);
    return e * e;
}

// a signal's values from its three wave sums: out[0 .. 3) = loss_b, match_b, conf_b
SC_HD void set_values(double sum_d2, double sum_conf_sq, int n, int Lmax, double w_conf, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double m = sum_d2 / (double)(n > 1 ? n : 1), c = sum_conf_sq / (double)Lmax;
    const double wc = w_conf * c;
    out[0] = m + wc;
    out[1] = m;
    out[2] = c;
}

// g_tau_i (scale = sx, d = wrap(dtau)) or g_f_i on a matched slot: cm 2 scale^2 d / (n B)
SC_HD double set_grad_coord(double cm, double scale, double d, int n, int64_t B) {
    return cm * 2.0 * scale * scale * d / ((double)n * (double)B);
}

// g_conf_i: cc 2 (conf_i - t_i) / (Lmax B)
SC_HD double set_grad_conf(double cc, double conf, bool matched, int Lmax, int64_t B) {
    return cc * 2.0 * (conf - (matched ? 1.0 : 0.0)) / ((double)Lmax * (double)B);
}

}  // namespace admmnet
