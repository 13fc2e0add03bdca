// score_core.h -- the scalar core of the scoring kernels (score.hip): everything one lane computes, without a wave in it, so
// that tests/host_model/score_model.cpp runs the same arithmetic with the lane loop emulated.
//
// The assignment (admmnet_score_match_f64 in include/admmnet.h has the definition).  Rows are the smaller side, columns the
// larger, lane j owns column j (ScCol) and, as a row, the potential u of row j.  For each row i in index order one
// shortest-augmenting-path search in the reduced costs cost(i, j) - u_i - v_j (Jonker-Volgenant / the Hungarian method with
// potentials), every step of it
//     relax     each free column from the row the path reached               sc_relax     (a lane)
//     choose    the free column of least distance, lowest lane on ties       sc_better    (the order of the wave's argmin)
//     shift     the potentials of the tree and the distances of the rest     sc_shift     (a lane)
// until the chosen column has no row; then the path is flipped from that column back to row i.  Costs are recomputed from the
// coordinates (sc_delta, sc_cost): there is no cost matrix.  The truncation min(d^2, c^2) is inside the cost the search sees.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SC_HD __host__ __device__ __forceinline__
#else
#define SC_HD inline
#endif

namespace admmnet {

constexpr int SC_MAX = 64;     // most rows of estimates and of targets per signal: one lane each
constexpr int SC_STATS = 8;    // n_hit, n_miss, n_false, sum dtau^2, sum df^2, sum d^2, gospa^2, optimal truncated cost
constexpr int SC_OPTS = 5;     // sx, sy, cutoff, period_tau, period_f

struct ScoreOpt {
    double sx, sy, c2, period_tau, period_f;   // c2 = cutoff^2
};

// neither an infinity nor a NaN (a comparison with a NaN is false)
SC_HD bool sc_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

SC_HD bool sc_opts_ok(const double *o) {
    return o[0] > 0.0 && sc_finite(o[0]) && o[1] > 0.0 && sc_finite(o[1]) && o[2] > 0.0 && sc_finite(o[2]) && o[3] >= 0.0 &&
           sc_finite(o[3]) && o[4] >= 0.0 && sc_finite(o[4]);
}

// a count held to [0, cap]; *outside: the raw value was not in it
SC_HD int sc_clamp_count(int64_t raw, int cap, bool *outside) {
    *outside = raw < 0 || raw > cap;
    return raw < 0 ? 0 : (raw > cap ? cap : (int)raw);
}

// d into [-P / 2, P / 2) for a period P > 0; P = 0: d itself
SC_HD double sc_wrap(double d, double P) { return P > 0.0 ? d - P * floor(d / P + 0.5) : d; }

struct ScDelta {
    double dtau, df, d2;
};

// (tau, f) of a minus (tau, f) of b, wrapped, and d^2 = (sx dtau)^2 + (sy df)^2.  Every product is rounded on its own (no fused
// multiply-add), so the host's float64 gives the same bits.
SC_HD ScDelta sc_delta(double tau_a, double f_a, double tau_b, double f_b, const ScoreOpt &o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    ScDelta r;
    r.dtau = sc_wrap(tau_a - tau_b, o.period_tau);
    r.df = sc_wrap(f_a - f_b, o.period_f);
    const double a = o.sx * r.dtau, b = o.sy * r.df;
    const double aa = a * a, bb = b * b;
    r.d2 = aa + bb;
    return r;
}

// min(d^2, c^2); a d^2 that is no number (differences of huge finite coordinates) costs c^2 and is no hit
SC_HD double sc_cost(double d2, double c2) { return d2 < c2 ? d2 : c2; }
SC_HD bool sc_hit(double d2, double c2) { return d2 < c2; }

// one column of the assignment, as its lane holds it
struct ScCol {
    double tau, f;   // coordinates
    double v;        // potential
    double minv;     // least reduced cost of a path from the root row to this column, while it is free
    int p;           // the row assigned to it, -1: none
    int way;         // the column before it on that path, -1: the root row itself
    bool live;       // takes part (a lane at or past the side's count, or an absent row of estimates, does not)
    bool used;       // in the tree of the current search
};

SC_HD void sc_col_init(ScCol &c, double tau, double f, bool live) {
    c.tau = tau;
    c.f = f;
    c.v = 0.0;
    c.minv = INFINITY;
    c.p = -1;
    c.way = -1;
    c.live = live;
    c.used = false;
}

SC_HD void sc_col_begin(ScCol &c) {   // a new search
    c.minv = INFINITY;
    c.used = false;
}

// relax column c from the row at (row_tau, row_f) with potential u, reached through column `from` (-1: it is the root)
SC_HD void sc_relax(ScCol &c, double row_tau, double row_f, double u, int from, const ScoreOpt &o) {
    if (!c.live || c.used) return;
    const double cur = sc_cost(sc_delta(row_tau, row_f, c.tau, c.f, o).d2, o.c2) - u - c.v;
    if (cur < c.minv) {
        c.minv = cur;
        c.way = from;
    }
}

// what a column offers to the argmin: its distance while it is free, +inf otherwise
SC_HD double sc_key(const ScCol &c) { return c.live && !c.used ? c.minv : INFINITY; }

// (key_b, lane_b) before (key_a, lane_a): a smaller key, the lower lane on equal keys
SC_HD bool sc_better(double key_a, int lane_a, double key_b, int lane_b) {
    return key_b < key_a || (key_b == key_a && lane_b < lane_a);
}

// after the argmin found `delta`: the lane's column, and the row potential u of the lane when that row is in the tree
SC_HD void sc_shift(ScCol &c, double &u, bool row_in_tree, double delta) {
    if (row_in_tree) u += delta;
    if (c.used)
        c.v -= delta;
    else
        c.minv -= delta;
}

// stats[SC_STATS] of one signal from its counts and the three sums over its hits
SC_HD void sc_stats(int n_est, int n_true, double n_hit, double s_tau, double s_f, double s_d2, double c2, double *out) {
    const int k = n_est < n_true ? n_est : n_true;
    const double miss = (double)n_true - n_hit, fa = (double)n_est - n_hit;
    out[0] = n_hit;
    out[1] = miss;
    out[2] = fa;
    out[3] = s_tau;
    out[4] = s_f;
    out[5] = s_d2;
    out[6] = s_d2 + 0.5 * c2 * (miss + fa);
    out[7] = s_d2 + c2 * ((double)k - n_hit);
}

}  // namespace admmnet
