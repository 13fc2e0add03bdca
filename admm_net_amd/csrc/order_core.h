// order_core.h -- the scene loop of the model-order kernel (order.hip): the candidate rows of a scene ranked by greedy orthogonal
// least squares against the received signal, and the number of targets chosen by a penalised log residual (admmnet_order_f64 in
// include/admmnet.h has the definition).  Written ONCE over the `Par` of refine_core.h (par.each, par.sum), so that
// tests/host_model/order_model.cpp runs the same arithmetic with the threads emulated.  Everything between two such calls is
// computed by every thread from what the last one left in memory, so every branch around them is uniform.  The pieces:
//     tables     u_l^k = exp(j 2 pi k f_l), k < Nb, and v_l^k = exp(-j 2 pi k tau_l), k < Nd, of every present row, each from
//                sincospi of the argument reduced to a fraction of a turn -- never from a recurrence                  od_tables
//     Gram       G[p][q] = a_p^H a_q = (sum_ib conj(u_p) u_q) (sum_id conj(v_p) v_q), a thread per pair p <= q         od_gram
//     data       c[p] = a_p^H x, first over i_d (a thread per (p, i_b)), then over i_b                                od_contract
//     ranking    a pivoted Cholesky of G: with q_k the unit vector of the k-th pick, F[p][k] = a_p^H q_k, w[k] = q_k^H x,
//                d[p] = |a_p|^2 - sum_k |F[p][k]|^2 and c[p] = a_p^H r are downdated per pick (a thread per row; step k reads
//                version k of d and c and writes version k + 1, so no thread reads what another is writing)              od_rank
//     order      the smallest k that minimises D ln(RSS_k / D) + penalty k; R C = w by back substitution, R = F^H of the picks
//     residual   x_i - sum_l C_l a_l(i) evaluated entry by entry, its squares added in float64 before the rounding   od_residual
#pragma once
#include "refine_core.h"

namespace admmnet {

constexpr int ORDER_THREADS = REFINE_THREADS;
constexpr int ORDER_INFO = 4;             // cost, cost / D, rows ranked, state
constexpr int ORDER_INFO_STATE = 3;       // the column of the state
constexpr int ORDER_STATUS = 2;           // scenes non-finite, scenes outside
constexpr double ORDER_COINCIDENT = CRB_PIVOT_MIN;                       // times D: |a~_j|^2 below it, the row is never taken
constexpr double ORDER_RSS_FLOOR = CRB_PIVOT_MIN * CRB_PIVOT_MIN;        // 2^-80, times |x|^2

enum { OD_RANKED = 0, OD_NONFINITE = RF_NONFINITE, OD_OUTSIDE = RF_OUTSIDE };
enum { OD_N = 0, OD_K = 1, OD_HELD = 2, OD_NSEL = 3, OD_META = 4 };

struct OrderArgs {
    int Nb, Nd, Le, psk_m;
    double psk_phase, penalty;
    int max_order;
};

CRB_HD int od_tab_count(int Nb, int Nd, int Le) { return Le * (Nb + Nd); }

struct OrderMem {
    RfC *x;              // [D] y conj(s)
    RfC *pt;             // [REFINE_MAX_M] the constellation
    RfC *tab;            // [Le (Nb + Nd)] per present row u^k, k < Nb, then v^k, k < Nd
    RfC *rs;             // [Le Nb] per (row, i_b): the sum over i_d
    RfC *G;              // [Le * Le] row-major, Hermitian
    RfC *F;              // [Le * Le] F[p * Le + k]
    RfC *c;              // [(Le + 1) * Le] version k of a_p^H r at [k * Le + p]
    double *d;           // [(Le + 1) * Le] version k of |a~_p|^2
    RfC *w, *C;          // [Le]
    double *tau, *f;     // [Le] of the present rows
    double *rss;         // [Le + 1]
    int *idx;            // [Le] the input row of every present row
    int *pick;           // [Le] the present row taken at every step
    int *perm;           // [Le]
    int *meta;           // [OD_META]
};

template <class Par>
CRB_HD void od_tables(Par &par, int Nb, int Nd, int n, const OrderMem &m) {
    par.each(n * (Nb + Nd), [&](int item) {
        const int l = item / (Nb + Nd), k = item - l * (Nb + Nd);
        m.tab[item] = k < Nb ? rf_turn((double)k * m.f[l]) : rf_turn(-((double)(k - Nb) * m.tau[l]));
    });
}

template <class Par>
CRB_HD void od_gram(Par &par, int Nb, int Nd, int Le, int n, const OrderMem &m) {
    par.each(n * (n + 1) / 2, [&](int pr) {
        int p, q;
        crb_pair_decode(pr, &p, &q);                       // p <= q
        const RfC *tp = m.tab + p * (Nb + Nd), *tq = m.tab + q * (Nb + Nd);
        RfC sb = {0.0, 0.0}, sd = {0.0, 0.0};
        for (int k = 0; k < Nb; ++k) {
            const RfC t = rf_mul_conj(tq[k], tp[k]);
            sb.re += t.re;
            sb.im += t.im;
        }
        for (int k = 0; k < Nd; ++k) {
            const RfC t = rf_mul_conj(tq[Nb + k], tp[Nb + k]);
            sd.re += t.re;
            sd.im += t.im;
        }
        const RfC g = rf_mul(sb, sd);
        if (p == q) {
            m.G[p * Le + p] = {g.re, 0.0};
        } else {
            m.G[p * Le + q] = g;
            m.G[q * Le + p] = {g.re, -g.im};
        }
    });
}

// version 0 of c: c[p] = sum_i conj(a_p(i)) x_i
template <class Par>
CRB_HD void od_contract(Par &par, int Nb, int Nd, int n, const OrderMem &m) {
    par.each(n * Nb, [&](int item) {
        const int l = item / Nb, ib = item - l * Nb;
        const RfC *v = m.tab + l * (Nb + Nd) + Nb;
        RfC s = {0.0, 0.0};
        for (int id = 0; id < Nd; ++id) {
            const RfC p = rf_mul_conj(m.x[ib * Nd + id], v[id]);
            s.re += p.re;
            s.im += p.im;
        }
        m.rs[item] = s;
    });
    par.each(n, [&](int l) {
        const RfC *u = m.tab + l * (Nb + Nd);
        RfC s = {0.0, 0.0};
        for (int ib = 0; ib < Nb; ++ib) {
            const RfC p = rf_mul_conj(m.rs[l * Nb + ib], u[ib]);
            s.re += p.re;
            s.im += p.im;
        }
        m.c[l] = s;
    });
}

// The picks in order; leaves pick, w, F, rss and meta[OD_K], meta[OD_HELD].  held: the present rows p < held are taken first.
template <class Par>
CRB_HD void od_rank(Par &par, int Le, int n, int held, int max_order, double D, double energy, const OrderMem &m) {
    const double floor_d = ORDER_COINCIDENT * D;
    par.each(n, [&](int p) { m.d[p] = m.G[p * Le + p].re; });
    int K = 0, hp = 0, h = 0;
    uint32_t taken = 0;
    double rss = energy;
    while (K < max_order) {
        const double *d = m.d + K * Le;
        const RfC *c = m.c + K * Le;
        int j = -1;
        while (hp < held && j < 0) {
            if (d[hp] >= floor_d) j = hp;
            ++hp;
        }
        const bool is_held = j >= 0;
        if (j < 0) {
            double top = -1.0;
            for (int p = 0; p < n; ++p) {
                if ((taken >> p & 1u) || !(d[p] >= floor_d)) continue;
                const double gain = (c[p].re * c[p].re + c[p].im * c[p].im) / d[p];
                if (gain > top) {
                    top = gain;
                    j = p;
                }
            }
        }
        if (j < 0) break;
        const double dj = d[j], root = sqrt(dj);
        const RfC wk = {c[j].re / root, c[j].im / root};
        const double gain = (c[j].re * c[j].re + c[j].im * c[j].im) / dj;
        rss -= gain;
        const int k = K;
        par.each(n, [&](int p) {
            RfC s = m.G[p * Le + j];                        // a_p^H a_j less what the earlier picks span
            for (int q = 0; q < k; ++q) {
                const RfC t = rf_mul_conj(m.F[p * Le + q], m.F[j * Le + q]);
                s.re -= t.re;
                s.im -= t.im;
            }
            const RfC fk = {s.re / root, s.im / root};
            m.F[p * Le + k] = fk;
            const RfC t = rf_mul(fk, wk);
            m.c[(k + 1) * Le + p] = {m.c[k * Le + p].re - t.re, m.c[k * Le + p].im - t.im};
            m.d[(k + 1) * Le + p] = m.d[k * Le + p] - (fk.re * fk.re + fk.im * fk.im);
            if (p == 0) {
                m.pick[k] = j;
                m.w[k] = wk;
                m.rss[k + 1] = rss;
            }
        });
        taken |= 1u << j;
        h += is_held ? 1 : 0;
        ++K;
    }
    par.each(1, [&](int) {
        m.meta[OD_K] = K;
        m.meta[OD_HELD] = h;
    });
}

CRB_HD RfC od_model(int i, int Nb, int Nd, int n_sel, const OrderMem &m) {
    const int ib = i / Nd, id = i - ib * Nd;
    RfC mu = {0.0, 0.0};
    for (int l = 0; l < n_sel; ++l) {
        const RfC *t = m.tab + m.pick[l] * (Nb + Nd);
        const RfC s = rf_mul(m.C[l], rf_mul(t[ib], t[Nb + id]));
        mu.re += s.re;
        mu.im += s.im;
    }
    return mu;
}

// One scene.  y, b: D pairs (re, im) of float; rows_in, rows_out: Le rows of 3; n_cand, n_held, sym: null or the scene's; perm: Le;
// n_sel: 1; rss: Le + 1; C_out: Le pairs; residual: D pairs of float; info: ORDER_INFO.
template <class Par>
CRB_HD void order_scene(Par &par, const OrderArgs &a, const OrderMem &m, const float *y, const float *b, const double *rows_in,
                        const int32_t *n_cand, const int32_t *n_held, const int32_t *sym, int32_t *perm, int32_t *n_sel_out,
                        double *rss_out, double *rows_out, double *C_out, float *residual, double *info) {
    const int Nb = a.Nb, Nd = a.Nd, Le = a.Le, D = Nb * Nd;
    bool outside = false, held_outside = false;
    const int count = sc_clamp_count(n_cand ? (int64_t)*n_cand : (int64_t)Le, Le, &outside);
    const int held_rows = sc_clamp_count(n_held ? (int64_t)*n_held : 0, count, &held_outside);
    int state = outside || held_outside ? OD_OUTSIDE : OD_RANKED;
    if (state == OD_RANKED && sym) {
        const double bad = par.sum(D, [&](int i) { return sym[i] >= 0 && sym[i] < a.psk_m ? 0.0 : 1.0; });
        if (bad > 0.0) state = OD_OUTSIDE;
    }
    if (state == OD_RANKED) {
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
        if (bad > 0.0) state = OD_NONFINITE;
    }
    if (state != OD_RANKED) {   // not ranked
        par.each(Le, [&](int j) {
            perm[j] = j;
            rows_out[3 * j] = rows_out[3 * j + 1] = rows_out[3 * j + 2] = NAN;
            C_out[2 * j] = C_out[2 * j + 1] = NAN;
        });
        par.each(Le + 1, [&](int k) { rss_out[k] = NAN; });
        par.each(D, [&](int i) { residual[2 * i] = residual[2 * i + 1] = NAN; });
        par.each(1, [&](int) {
            *n_sel_out = 0;
            info[0] = info[1] = NAN;
            info[2] = 0.0;
            info[3] = (double)state;
        });
        return;
    }
    par.each(1, [&](int) {
        int n = 0, held = 0;
        for (int j = 0; j < count; ++j) {
            const double tau = rows_in[3 * j], f = rows_in[3 * j + 1];
            if (!(sc_finite(tau) && sc_finite(f))) continue;
            m.idx[n] = j;
            m.tau[n] = tau;
            m.f[n] = f;
            held += j < held_rows ? 1 : 0;
            ++n;
        }
        m.meta[OD_N] = n;
        m.meta[OD_HELD] = held;
    });
    const int n = m.meta[OD_N], held = m.meta[OD_HELD];
    const double energy = par.sum(D, [&](int i) { return m.x[i].re * m.x[i].re + m.x[i].im * m.x[i].im; });
    par.each(1, [&](int) { m.rss[0] = energy; });
    od_tables(par, Nb, Nd, n, m);
    od_gram(par, Nb, Nd, Le, n, m);
    od_contract(par, Nb, Nd, n, m);
    od_rank(par, Le, n, held, a.max_order < Le ? a.max_order : Le, (double)D, energy, m);
    const int K = m.meta[OD_K], h = m.meta[OD_HELD];
    // the order: the smallest k in h .. K of the least criterion
    int n_sel = h;
    double least = 0.0;
    for (int k = h; k <= K; ++k) {
        const double r = m.rss[k], lo = ORDER_RSS_FLOOR * energy;
        const double crit = (double)D * log((r > lo ? r : lo) / (double)D) + a.penalty * (double)k;
        if (k == h || crit < least) {
            least = crit;
            n_sel = k;
        }
    }
    // R C = w on the selected picks: R[k][l] = conj(F[pick_l][k]), k <= l
    par.each(1, [&](int) {
        for (int l = n_sel - 1; l >= 0; --l) {
            RfC s = m.w[l];
            for (int q = l + 1; q < n_sel; ++q) {
                const RfC r = {m.F[m.pick[q] * Le + l].re, -m.F[m.pick[q] * Le + l].im};
                const RfC t = rf_mul(r, m.C[q]);
                s.re -= t.re;
                s.im -= t.im;
            }
            const double rll = m.F[m.pick[l] * Le + l].re;
            m.C[l] = {s.re / rll, s.im / rll};
        }
        uint32_t ranked = 0;
        for (int k = 0; k < K; ++k) {
            m.perm[k] = m.idx[m.pick[k]];
            ranked |= 1u << m.perm[k];
        }
        int at = K;
        for (int j = 0; j < Le; ++j)
            if (!(ranked >> j & 1u)) m.perm[at++] = j;
    });
    const double cost = par.sum(D, [&](int i) {
        const RfC mu = od_model(i, Nb, Nd, n_sel, m);
        const double dr = m.x[i].re - mu.re, di = m.x[i].im - mu.im;
        residual[2 * i] = (float)dr;
        residual[2 * i + 1] = (float)di;
        return dr * dr + di * di;
    });
    par.each(Le, [&](int j) {
        const int from = m.perm[j];
        perm[j] = from;
        rows_out[3 * j] = rows_in[3 * from];
        rows_out[3 * j + 1] = rows_in[3 * from + 1];
        rows_out[3 * j + 2] = j < n_sel ? sqrt(m.C[j].re * m.C[j].re + m.C[j].im * m.C[j].im) : NAN;
        C_out[2 * j] = j < n_sel ? m.C[j].re : NAN;
        C_out[2 * j + 1] = j < n_sel ? m.C[j].im : NAN;
    });
    par.each(Le + 1, [&](int k) { rss_out[k] = k <= K ? m.rss[k] : NAN; });
    par.each(1, [&](int) {
        *n_sel_out = n_sel;
        info[0] = cost;
        info[1] = cost / (double)D;
        info[2] = (double)K;
        info[3] = (double)state;
    });
}

}  // namespace admmnet
