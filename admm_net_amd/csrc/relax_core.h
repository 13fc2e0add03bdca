// relax_core.h -- the scene loop of successive cancellation on the periodogram (cfar_relax.hip): the CFAR detector of cfar_core.h
// run round after round on a residual, the highest cell over the threshold fitted off the grid by Newton steps on the matched
// filter, subtracted, and every target found so far re-fitted cyclically (RELAX) -- admmnet_cfar_relax_f64 in include/admmnet.h has
// the definition.  Written ONCE over the `Par` of refine_core.h, with two more ways for a workgroup to share a loop, so that
// tests/host_model/relax_model.cpp runs the same arithmetic with the threads emulated:
//     par.sums<N>(count, fn, out)   out[n] = the sum of what fn(item, v) adds to v[n], N sums in ONE pass, each in par.sum's order
//     par.best(count, fn)           the item of greatest fn(item) >= 0, ties to the smaller item; -1 where no item has one.  A thread
//                                   keeps its best in index order, then the lanes of a wave, then the waves: no atomics
// Everything between two such calls is computed by every thread from what the last one left in memory, so every branch around
// them is uniform.  The pieces:
//     map, level   cf_tables, cf_map, cf_window, cf_level of cfar_core.h on the residual m.c.x: round 0's map is cfar_targets'
//     moments      S_w = sum_i x_i w_i exp(-j 2 pi (i_b f - i_d tau)) for w = 1, i_b, i_d, i_b^2, i_d^2, i_b i_d: one pass over D with
//                  u[i_b] = exp(-j 2 pi i_b f) and v[i_d] = exp(+j 2 pi i_d tau) from tables, each from sincospi            rx_moments
//     fit          Newton steps on |S|^2 where its Hessian is negative definite, clamped to half a map cell round the start  rx_fit
//     cancel       x_i -= c conj(u[i_b] v[i_d]) with the tables of the last pass, c = S / D                                  rx_axpy
#pragma once
#include "cfar_core.h"

namespace admmnet {

constexpr int RELAX_INFO = 3;              // level, resid, state
constexpr int RELAX_INFO_STATE = 2;        // the column of the state
constexpr int RELAX_COUNTS = 3;            // n_det, more, maps
constexpr int RELAX_SUMS = 12;             // six complex moments
constexpr int RELAX_MAX_ITERS = 16;
constexpr int RELAX_MAX_SWEEPS = 8;

struct RelaxArgs {
    CfarArgs c;
    int iters, sweeps;
};

struct RelaxTarget {
    double tau, f, cr, ci, height;         // c = S / D, height = |S|^2 / D = |c|^2 D
};

struct RelaxMem {
    CfarMem c;           // x is the residual; list, chunk and slot are not used
    RfC *u, *v;          // [Nb], [Nd]
    RelaxTarget *tg;     // [CRB_MAXL]
};

template <class Par>
CRB_HD void rx_tables(Par &par, int Nb, int Nd, double tau, double f, const RelaxMem &m) {
    par.each(Nb + Nd, [&](int k) {
        if (k < Nb)
            m.u[k] = rf_turn(-((double)k * f));
        else
            m.v[k - Nb] = rf_turn((double)(k - Nb) * tau);
    });
}

// s[2 w], s[2 w + 1] = Re, Im of the moment of weight w = 1, i_b, i_d, i_b^2, i_d^2, i_b i_d at the point of the tables
template <class Par>
CRB_HD void rx_moments(Par &par, int Nb, int Nd, const RelaxMem &m, double (&s)[RELAX_SUMS]) {
    par.template sums<RELAX_SUMS>(Nb * Nd, [&](int i, double (&acc)[RELAX_SUMS]) {
        const int ib = i / Nd, id = i - ib * Nd;
        const RfC p = rf_mul(rf_mul(m.c.x[i], m.u[ib]), m.v[id]);
        const double wb = (double)ib, wd = (double)id;
        const double w[6] = {1.0, wb, wd, wb * wb, wd * wd, wb * wd};
        for (int k = 0; k < 6; ++k) {
            acc[2 * k] += w[k] * p.re;
            acc[2 * k + 1] += w[k] * p.im;
        }
    }, s);
}

// x += sign c a(tau, f) with the tables of (tau, f)
template <class Par>
CRB_HD void rx_axpy(Par &par, int Nb, int Nd, const RelaxMem &m, const RelaxTarget &t, double sign) {
    par.each(Nb * Nd, [&](int i) {
        const int ib = i / Nd, id = i - ib * Nd;
        const RfC uv = rf_mul(m.u[ib], m.v[id]), ca = rf_mul_conj({t.cr, t.ci}, uv);
        m.c.x[i].re += sign * ca.re;
        m.c.x[i].im += sign * ca.im;
    });
}

CRB_HD double rx_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// At most `iters` Newton steps on |S(tau, f)|^2 from (tau0, f0); the tables are left at the point returned.  g and H below are
// the gradient and the Hessian of F = |S|^2 / D over 4 pi / D, which a Newton step does not see.
template <class Par>
CRB_HD RelaxTarget rx_fit(Par &par, const RelaxArgs &a, const RelaxMem &m, double tau0, double f0) {
    const int Nb = a.c.Nb, Nd = a.c.Nd;
    const double D = (double)(Nb * Nd), half_f = 0.5 / (double)(a.c.r * Nb), half_tau = 0.5 / (double)(a.c.r * Nd);
    const bool has_tau = Nd > 1, has_f = Nb > 1;
    double tau = tau0, f = f0;
    RelaxTarget t;
    for (int step = 0;; ++step) {
        rx_tables(par, Nb, Nd, tau, f, m);
        double s[RELAX_SUMS];
        rx_moments(par, Nb, Nd, m, s);
        const RfC S = {s[0], s[1]}, Sb = {s[2], s[3]}, Sd = {s[4], s[5]}, Sbb = {s[6], s[7]}, Sdd = {s[8], s[9]}, Sbd = {s[10], s[11]};
        t = {tau, f, S.re / D, S.im / D, (S.re * S.re + S.im * S.im) / D};
        if (step == a.iters || !(has_tau || has_f)) break;
        const double g_tau = -(S.re * Sd.im - S.im * Sd.re), g_f = S.re * Sb.im - S.im * Sb.re;
        const double h_tt = CRB_TWO_PI * ((Sd.re * Sd.re + Sd.im * Sd.im) - (S.re * Sdd.re + S.im * Sdd.im));
        const double h_ff = CRB_TWO_PI * ((Sb.re * Sb.re + Sb.im * Sb.im) - (S.re * Sbb.re + S.im * Sbb.im));
        const double h_tf = CRB_TWO_PI * ((S.re * Sbd.re + S.im * Sbd.im) - (Sd.re * Sb.re + Sd.im * Sb.im));
        double d_tau = 0.0, d_f = 0.0;
        if (has_tau && has_f) {
            const double det = h_tt * h_ff - h_tf * h_tf;
            if (!(h_tt < 0.0 && det > 0.0)) break;
            d_tau = -(h_ff * g_tau - h_tf * g_f) / det;
            d_f = -(h_tt * g_f - h_tf * g_tau) / det;
        } else if (has_tau) {
            if (!(h_tt < 0.0)) break;
            d_tau = -g_tau / h_tt;
        } else {
            if (!(h_ff < 0.0)) break;
            d_f = -g_f / h_ff;
        }
        tau = rx_clamp(tau + d_tau, tau0 - half_tau, tau0 + half_tau);
        f = rx_clamp(f + d_f, f0 - half_f, f0 + half_f);
    }
    return t;
}

// With iters = 0 a NEW detection needs no moment: c is the map's own sum at the cell, taken from the row of img and the table the
// map was made of (both still in memory), in the map's order -- so on-grid cancellation costs no pass over D and its heights are
// cells of the map, bit for bit.  The tables are left at the cell for rx_axpy.
template <class Par>
CRB_HD RelaxTarget rx_cell(Par &par, const RelaxArgs &a, const RelaxMem &m, int j, int i, int nf, int nt) {
    const int Nb = a.c.Nb, Nd = a.c.Nd;
    const double D = (double)(Nb * Nd), tau = (double)i / (double)nt, f = (double)j / (double)nf - 0.5;
    rx_tables(par, Nb, Nd, tau, f, m);
    RfC s = {0.0, 0.0};
    for (int id = 0, k = 0; id < Nd; ++id) {                 // cf_map's second sum
        const RfC p = rf_mul(m.c.img[j * Nd + id], m.c.tt[k]);
        s.re += p.re;
        s.im += p.im;
        k = k + i >= nt ? k + i - nt : k + i;
    }
    return {tau, f, s.re / D, s.im / D, (s.re * s.re + s.im * s.im) / D};
}

// One scene.  y, b, sym, noise_var, map_out as cfar_scene; rows: Le rows of 3; amp: Le pairs; counts: RELAX_COUNTS; info: RELAX_INFO.
template <class Par>
CRB_HD void relax_scene(Par &par, const RelaxArgs &ra, const RelaxMem &rm, const float *y, const float *b, const int32_t *sym,
                        const double *noise_var, double *rows, double *amp, int32_t *counts, double *info, double *map_out) {
    const CfarArgs &a = ra.c;
    const CfarMem &m = rm.c;
    const int Nb = a.Nb, Nd = a.Nd, Le = a.Le, D = Nb * Nd, nf = a.r * Nb, nt = a.r * Nd, cells = nf * nt;
    // the symbols and the states of cfar_scene
    const double known = a.method == CF_KNOWN ? *noise_var : 1.0;
    int state = a.method == CF_KNOWN && known <= 0.0 ? CF_OUTSIDE : CF_DONE;
    if (state == CF_DONE && sym) {
        const double bad = par.sum(D, [&](int i) { return sym[i] >= 0 && sym[i] < a.psk_m ? 0.0 : 1.0; });
        if (bad > 0.0) state = CF_OUTSIDE;
    }
    if (state == CF_DONE && !sc_finite(known)) state = CF_NONFINITE;
    if (state == CF_DONE) {
        par.each(a.psk_m, [&](int k) { m.pt[k] = rf_turn((double)k / (double)a.psk_m + a.psk_phase / CRB_TWO_PI); });
        const double bad = par.sum(D, [&](int i) {
            const RfC yi = {(double)y[2 * i], (double)y[2 * i + 1]}, bi = {(double)b[2 * i], (double)b[2 * i + 1]};
            const bool ok = sc_finite(yi.re) && sc_finite(yi.im) && sc_finite(bi.re) && sc_finite(bi.im) &&
                            (sym || bi.re != 0.0 || bi.im != 0.0);
            if (sym) {
                m.x[i] = rf_mul_conj(yi, m.pt[sym[i]]);
            } else {
                const double mag = sqrt(bi.re * bi.re + bi.im * bi.im);
                m.x[i] = rf_mul_conj(yi, {bi.re / mag, bi.im / mag});
            }
            return ok ? 0.0 : 1.0;
        });
        if (bad > 0.0) state = CF_NONFINITE;
    }
    if (state != CF_DONE) {   // no map
        par.each(Le, [&](int l) {
            rows[3 * l] = rows[3 * l + 1] = rows[3 * l + 2] = NAN;
            amp[2 * l] = amp[2 * l + 1] = NAN;
        });
        if (map_out) par.each(cells, [&](int c) { map_out[c] = NAN; });
        par.each(1, [&](int) {
            counts[0] = counts[1] = counts[2] = 0;
            info[0] = info[1] = NAN;
            info[2] = (double)state;
        });
        return;
    }
    cf_tables(par, nf, nt, m);
    if (a.method != CF_KNOWN) cf_window(par, a, m);
    const int N = a.method != CF_KNOWN ? cf_train_count(Nb, Nd, a.guard, a.train) : 0;
    int n = 0, more = 0, maps = 0;
    double zsum = 0.0;
    for (;;) {   // at most Le + 1 rounds
        cf_map(par, Nb, Nd, nf, nt, m);
        ++maps;
        zsum = par.sum(cells, [&](int c) {
            const double Z = cf_level(c, a, N, nf, nt, known, m);
            m.flag[c] = m.map[c] > a.alpha * Z ? 1 : 0;
            return Z;
        });
        const int top = par.best(cells, [&](int c) { return m.flag[c] ? m.map[c] : -1.0; });
        if (top < 0) break;
        if (n == Le) {
            more = 1;
            break;
        }
        const int j = top / nt, i = top - j * nt;
        RelaxTarget t = ra.iters == 0 ? rx_cell(par, ra, rm, j, i, nf, nt)
                                      : rx_fit(par, ra, rm, (double)i / (double)nt, (double)j / (double)nf - 0.5);
        rx_axpy(par, Nb, Nd, rm, t, -1.0);
        par.each(1, [&](int) { rm.tg[n] = t; });
        ++n;
        for (int sweep = 0; n >= 2 && sweep < ra.sweeps; ++sweep)
            for (int l = 0; l < n; ++l) {
                t = rm.tg[l];
                rx_tables(par, Nb, Nd, t.tau, t.f, rm);
                rx_axpy(par, Nb, Nd, rm, t, 1.0);
                t = rx_fit(par, ra, rm, t.tau, t.f);
                rx_axpy(par, Nb, Nd, rm, t, -1.0);
                par.each(1, [&](int) { rm.tg[l] = t; });
            }
    }
    const double rsum = par.sum(D, [&](int i) { return m.x[i].re * m.x[i].re + m.x[i].im * m.x[i].im; });
    par.each(Le, [&](int l) {
        if (l < n) {
            const RelaxTarget t = rm.tg[l];
            double tau = t.tau, f = t.f;
            if (tau < 0.0 || tau >= 1.0) {                   // a point the fit left on the grid keeps its bits
                tau -= floor(tau);
                tau = tau >= 1.0 ? 0.0 : tau;
            }
            if (f < -0.5 || f >= 0.5) {
                f -= floor(f + 0.5);
                f = f >= 0.5 ? -0.5 : f;
            }
            rows[3 * l] = tau;
            rows[3 * l + 1] = f;
            rows[3 * l + 2] = t.height;
            amp[2 * l] = t.cr;
            amp[2 * l + 1] = t.ci;
        } else {
            rows[3 * l] = rows[3 * l + 1] = rows[3 * l + 2] = NAN;
            amp[2 * l] = amp[2 * l + 1] = NAN;
        }
    });
    if (map_out) par.each(cells, [&](int c) { map_out[c] = m.map[c]; });
    par.each(1, [&](int) {
        counts[0] = n;
        counts[1] = more;
        counts[2] = maps;
        info[0] = a.method == CF_KNOWN ? known : zsum / (double)cells;
        info[1] = rsum / (double)D;
        info[2] = (double)state;
    });
}

}  // namespace admmnet
