// refine_core.h -- the scene loop of the refinement kernel (refine.hip): a local maximum-likelihood fit of a scene's targets to the
// received signal, started at the rows of a peak search (admmnet_refine_f64 in include/admmnet.h has the definition).  It is
// written ONCE over a `Par` that says how a workgroup shares a loop, so that tests/host_model/refine_model.cpp runs the same
// arithmetic with the threads emulated:
//     par.each(count, fn)   fn(item) for every item < count, the items dealt to the threads; a barrier behind it
//     par.sum(count, fn)    the sum of fn(item) in a fixed order, known to every thread
// Everything between two such calls is computed by every thread from what the last one left in memory, so every branch around
// them is uniform.  The pieces, per linearisation at theta = (Re C, Im C, tau, f) (crb_core.h's order and its 4 x 4 pair blocks):
//     tables     u_l^k = exp(j 2 pi k f_l), k < Nb, and v_l^k = exp(-j 2 pi k tau_l), k < Nd, each from sincospi of the argument
//                reduced to a fraction of a turn -- never from a recurrence                                         rf_tables
//     data       sum_i conj(a_li) x_i {1, i_b, i_d} per target, first over i_d (a thread per (l, i_b)), then over i_b  rf_contract
//     G          Re(J^H J) from the power sums, crb_pair_fill (a thread per pair); it does not depend on x as |s| = 1
//     g          Re(J^H x) - G[:, C] c: J^H mu is a combination of G's columns of Re C and Im C
//     solve      A = D G D kept in the upper triangle, (A + lambda I) factored in the lower (crb_chol_dot), two triangular solves
//     Q          sum_i |x_i - mu_i|^2 evaluated entry by entry at the trial theta (the closed form in c cancels)    rf_cost
//     symbols    the constellation point nearest to y_i conj(mu_i), mode "psk"                                      rf_decide
#pragma once
#include "crb_core.h"
#include "score_core.h"

namespace admmnet {

constexpr int REFINE_MAX_M = 64;          // most constellation points
constexpr int REFINE_MAX_ITERS = 64;
constexpr int REFINE_THREADS = 256;       // of a workgroup; the host model emulates as many
constexpr int REFINE_INFO = 5;            // Q, Q / D, linearisations used, flips, state
constexpr int REFINE_INFO_STATE = 4;      // the column of the state
constexpr int REFINE_STATUS = 4;          // scenes outside, non-finite, gave up, limit reached
constexpr double REFINE_LAMBDA_START = 1e-4;
constexpr double REFINE_LAMBDA_MAX = 1e8;
constexpr double REFINE_MAX_MOVE = 0.5;   // cells per step

enum { RF_CONVERGED = 0, RF_LIMIT = 1, RF_GAVE_UP = 2, RF_NONFINITE = 3, RF_OUTSIDE = 4 };

struct RfC {
    double re, im;
};

struct RefineArgs {
    int Nb, Nd, Le, mode, psk_m;
    double psk_phase;
    int iters;
    double tol;
};

// entries of each array of a scene (RefineMem), from the sizes of the call
CRB_HD int rf_pmax(int Nb, int Nd, int Le) { return crb_params(Le, Nd > 1, Nb > 1); }
CRB_HD int rf_tab_count(int Nb, int Nd, int Le) { return Le * (Nb + Nd); }
CRB_HD int rf_rows_count(int Nb, int Le) { return 2 * Le * Nb; }
constexpr int RF_CONT = 3 * CRB_MAXL;     // per target: the sums with 1, i_b, i_d
constexpr int RF_IDX = CRB_MAXL + 1;      // the input row of every present target, then their number

struct RefineMem {
    RfC *z;              // [D] x = y conj(s) in mode 0, y in mode 1 (x = z conj(pt[k]))
    uint8_t *k, *k0;     // [D] the symbol of every entry now and at the start
    RfC *pt;             // [psk_m] the constellation
    double *A;           // [P * P] column-major: the lower triangle is worked on, the upper keeps the unit-diagonal matrix
    RfC *tab;            // [Le (Nb + Nd)] per target u^k, k < Nb, then v^k, k < Nd
    RfC *rs;             // [2 Le Nb] per (target, i_b): the sums over i_d with 1 and with i_d
    RfC *cont;           // [RF_CONT]
    CrbTarget *tg, *trial;   // [CRB_MAXL]
    double *g, *dsc, *step, *col;   // [CRB_MAXP]
    int *idx;            // [RF_IDX]
};

CRB_HD RfC rf_mul(RfC a, RfC b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
CRB_HD RfC rf_mul_conj(RfC a, RfC b) { return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }   // a conj(b)

// exp(j 2 pi t)
CRB_HD RfC rf_turn(double t) {
    RfC r;
    crb_sincos_turns(t - rint(t), &r.im, &r.re);
    return r;
}

// the k of greatest Re(w conj(p_k)), the smaller k on ties
CRB_HD int rf_nearest(RfC w, const RfC *pt, int m) {
    int best = 0;
    double top = w.re * pt[0].re + w.im * pt[0].im;
    for (int k = 1; k < m; ++k) {
        const double v = w.re * pt[k].re + w.im * pt[k].im;
        if (v > top) {
            top = v;
            best = k;
        }
    }
    return best;
}

CRB_HD RfC rf_x(int i, const RefineMem &m, bool psk) { return psk ? rf_mul_conj(m.z[i], m.pt[m.k[i]]) : m.z[i]; }

CRB_HD RfC rf_mu(int i, int Nb, int Nd, int n, const CrbTarget *tg, const RfC *tab) {
    const int ib = i / Nd, id = i - ib * Nd;
    RfC mu = {0.0, 0.0};
    for (int l = 0; l < n; ++l) {
        const RfC *t = tab + l * (Nb + Nd);
        const RfC a = rf_mul(t[ib], t[Nb + id]), c = rf_mul({tg[l].cr, tg[l].ci}, a);
        mu.re += c.re;
        mu.im += c.im;
    }
    return mu;
}

template <class Par>
CRB_HD void rf_tables(Par &par, int Nb, int Nd, int n, const CrbTarget *tg, RfC *tab) {
    par.each(n * (Nb + Nd), [&](int item) {
        const int l = item / (Nb + Nd), k = item - l * (Nb + Nd);
        tab[item] = k < Nb ? rf_turn((double)k * tg[l].f) : rf_turn(-((double)(k - Nb) * tg[l].tau));
    });
}

template <class Par>
CRB_HD double rf_cost(Par &par, int Nb, int Nd, int n, const CrbTarget *tg, const RefineMem &m, bool psk) {
    return par.sum(Nb * Nd, [&](int i) {
        const RfC x = rf_x(i, m, psk), mu = rf_mu(i, Nb, Nd, n, tg, m.tab);
        const double dr = x.re - mu.re, di = x.im - mu.im;
        return dr * dr + di * di;
    });
}

template <class Par>
CRB_HD void rf_decide(Par &par, int Nb, int Nd, int n, int psk_m, const RefineMem &m) {
    par.each(Nb * Nd, [&](int i) { m.k[i] = (uint8_t)rf_nearest(rf_mul_conj(m.z[i], rf_mu(i, Nb, Nd, n, m.tg, m.tab)), m.pt, psk_m); });
}

// cont[3 l + {0, 1, 2}] = sum_i conj(a_li) x_i {1, i_b, i_d}
template <class Par>
CRB_HD void rf_contract(Par &par, int Nb, int Nd, int n, const RefineMem &m, bool psk) {
    par.each(n * Nb, [&](int item) {
        const int l = item / Nb, ib = item - l * Nb;
        const RfC *v = m.tab + l * (Nb + Nd) + Nb;
        RfC s0 = {0.0, 0.0}, s1 = {0.0, 0.0};
        for (int id = 0; id < Nd; ++id) {
            const RfC p = rf_mul_conj(rf_x(ib * Nd + id, m, psk), v[id]);
            s0.re += p.re;
            s0.im += p.im;
            s1.re += (double)id * p.re;
            s1.im += (double)id * p.im;
        }
        m.rs[2 * item] = s0;
        m.rs[2 * item + 1] = s1;
    });
    par.each(n, [&](int l) {
        const RfC *u = m.tab + l * (Nb + Nd);
        RfC c0 = {0.0, 0.0}, cb = {0.0, 0.0}, cd = {0.0, 0.0};
        for (int ib = 0; ib < Nb; ++ib) {
            const RfC p = rf_mul_conj(m.rs[2 * (l * Nb + ib)], u[ib]), q = rf_mul_conj(m.rs[2 * (l * Nb + ib) + 1], u[ib]);
            c0.re += p.re;
            c0.im += p.im;
            cb.re += (double)ib * p.re;
            cb.im += (double)ib * p.im;
            cd.re += q.re;
            cd.im += q.im;
        }
        m.cont[3 * l] = c0;
        m.cont[3 * l + 1] = cb;
        m.cont[3 * l + 2] = cd;
    });
}

// Re(J_p^H x) for the parameter `kind` of target l: the column is coef * i^p * a_l
CRB_HD double rf_jhx(int kind, int l, const RefineMem &m) {
    double cr, ci;
    crb_coef(kind, m.tg[l], &cr, &ci);
    const RfC s = m.cont[3 * l + (kind == CRB_F ? 1 : (kind == CRB_TAU ? 2 : 0))];
    return cr * s.re + ci * s.im;
}

// the kind and the target of parameter p among those of n targets (the inverse of crb_index)
CRB_HD void rf_param(int p, int n, bool has_tau, int *kind, int *l) {
    const int block = p / n;
    *l = p - block * n;
    *kind = block < 2 ? block : (block == 2 && has_tau ? CRB_TAU : CRB_F);
}

CRB_HD double rf_sym(const double *A, int ld, int i, int j) { return i >= j ? A[j * ld + i] : A[i * ld + j]; }   // of the lower triangle

// rows i < Pn of the lower triangle scaled to unit diagonal and kept in the upper triangle
template <class Par>
CRB_HD void rf_scale(Par &par, int Pn, int ld, const RefineMem &m) {
    par.each(Pn, [&](int i) {
        crb_scale_row(i, m.A, ld, m.dsc);
        for (int k = 0; k < i; ++k) m.A[i * ld + k] = m.A[k * ld + i];
    });
}

// the leading Pn x Pn block of (kept matrix + lambda I) factored in the lower triangle; false: a pivot below the floor
template <class Par>
CRB_HD bool rf_factor(Par &par, int Pn, int ld, double lambda, const RefineMem &m) {
    par.each(Pn, [&](int i) {
        for (int k = 0; k < i; ++k) m.A[k * ld + i] = m.A[i * ld + k];
        m.A[i * ld + i] = 1.0 + lambda;
    });
    for (int j = 0; j < Pn; ++j) {
        par.each(Pn - j, [&](int r) { m.col[j + r] = crb_chol_dot(j + r, j, m.A, ld); });
        const double pivot = m.col[j];
        if (!(pivot >= CRB_PIVOT_MIN)) return false;
        const double ljj = sqrt(pivot);
        par.each(Pn - j, [&](int r) { m.A[j * ld + j + r] = r == 0 ? ljj : m.col[j + r] / ljj; });
    }
    return true;
}

// step <- D (L L^T)^-1 step for the factor of rf_factor: the solution in the unscaled parameters
template <class Par>
CRB_HD void rf_solve(Par &par, int Pn, int ld, const RefineMem &m) {
    par.each(1, [&](int) {
        double *w = m.step;
        for (int i = 0; i < Pn; ++i) {
            double s = w[i];
            for (int k = 0; k < i; ++k) s -= m.A[k * ld + i] * w[k];
            w[i] = s / m.A[i * ld + i];
        }
        for (int i = Pn - 1; i >= 0; --i) {
            double s = w[i];
            for (int k = i + 1; k < Pn; ++k) s -= m.A[i * ld + k] * w[k];
            w[i] = s / m.A[i * ld + i];
        }
        for (int i = 0; i < Pn; ++i) w[i] *= m.dsc[i];
    });
}

// One scene.  y, b: D pairs (re, im) of float; rows_in, rows_out: Le rows of 3; C_out: Le pairs; info: REFINE_INFO; sym: D or null.
template <class Par>
CRB_HD void refine_scene(Par &par, const RefineArgs &a, const RefineMem &m, const float *y, const float *b, const double *rows_in,
                         const int32_t *n_est, double *rows_out, double *C_out, double *info, int32_t *sym) {
    const int Nb = a.Nb, Nd = a.Nd, Le = a.Le, D = Nb * Nd;
    const bool has_tau = Nd > 1, has_f = Nb > 1, psk = a.mode == 1;
    bool outside = false;
    const int count = sc_clamp_count(n_est ? (int64_t)*n_est : (int64_t)Le, Le, &outside);
    int state = outside ? RF_OUTSIDE : RF_CONVERGED;
    if (!outside) {
        par.each(a.psk_m, [&](int k) { m.pt[k] = rf_turn((double)k / (double)a.psk_m + a.psk_phase / CRB_TWO_PI); });
        const double bad = par.sum(D, [&](int i) {
            const RfC yi = {(double)y[2 * i], (double)y[2 * i + 1]}, bi = {(double)b[2 * i], (double)b[2 * i + 1]};
            const bool ok = sc_finite(yi.re) && sc_finite(yi.im) && sc_finite(bi.re) && sc_finite(bi.im) &&
                            (psk || bi.re != 0.0 || bi.im != 0.0);
            m.k[i] = m.k0[i] = (uint8_t)rf_nearest(bi, m.pt, a.psk_m);
            if (psk) {
                m.z[i] = yi;
            } else {
                const double mag = sqrt(bi.re * bi.re + bi.im * bi.im);
                m.z[i] = rf_mul_conj(yi, {bi.re / mag, bi.im / mag});
            }
            return ok ? 0.0 : 1.0;
        });
        if (bad > 0.0) state = RF_NONFINITE;
    }
    if (state != RF_CONVERGED) {   // not fitted
        par.each(Le, [&](int j) {
            rows_out[3 * j] = rows_out[3 * j + 1] = rows_out[3 * j + 2] = NAN;
            C_out[2 * j] = C_out[2 * j + 1] = NAN;
        });
        if (sym) par.each(D, [&](int i) { sym[i] = -1; });
        par.each(1, [&](int) {
            info[0] = info[1] = NAN;
            info[2] = info[3] = 0.0;
            info[4] = (double)state;
        });
        return;
    }
    par.each(1, [&](int) {
        int n = 0;
        for (int j = 0; j < count; ++j) {
            const double tau = rows_in[3 * j], f = rows_in[3 * j + 1];
            if (!(sc_finite(tau) && sc_finite(f))) continue;
            m.idx[n] = j;
            m.tg[n] = {tau, f, 0.0, 0.0};
            ++n;
        }
        m.idx[CRB_MAXL] = n;
    });
    const int n = m.idx[CRB_MAXL];
    const int P = crb_params(n, has_tau, has_f), ld = P, first = 2 * n;
    double Q = NAN;
    int used = 0;
    auto fill = [&]() {
        par.each(n * (n + 1) / 2, [&](int pr) {
            int l, mm;
            crb_pair_decode(pr, &l, &mm);
            crb_pair_fill(l, mm, n, Nb, Nd, m.tg, m.A, ld);
        });
    };
    if (n == 0) {
        Q = par.sum(D, [&](int i) { return m.z[i].re * m.z[i].re + m.z[i].im * m.z[i].im; });
    } else {
        // the starting C: least squares at the starting (tau, f), on the unit-diagonal C-block (the leading 2 n parameters)
        rf_tables(par, Nb, Nd, n, m.tg, m.tab);
        rf_contract(par, Nb, Nd, n, m, psk);
        fill();
        double bad = par.sum(first, [&](int p) {
            const double gpp = m.A[p * ld + p];
            m.dsc[p] = 1.0 / sqrt(gpp);
            m.step[p] = m.dsc[p] * (p < n ? m.cont[3 * p].re : m.cont[3 * (p - n)].im);
            return gpp > 0.0 && sc_finite(gpp) ? 0.0 : 1.0;
        });
        bool ok = !(bad > 0.0);
        if (ok) {
            rf_scale(par, first, ld, m);
            ok = rf_factor(par, first, ld, 0.0, m);
        }
        if (!ok) {
            state = RF_GAVE_UP;
            par.each(n, [&](int l) { m.tg[l].cr = m.tg[l].ci = NAN; });
        } else {
            rf_solve(par, first, ld, m);
            par.each(n, [&](int l) {
                m.tg[l].cr = m.step[l];
                m.tg[l].ci = m.step[n + l];
            });
            Q = rf_cost(par, Nb, Nd, n, m.tg, m, psk);
            double lambda = REFINE_LAMBDA_START;
            for (bool done = false; !done;) {
                if (used == a.iters) {
                    state = RF_LIMIT;
                    break;
                }
                ++used;
                if (psk) {
                    rf_decide(par, Nb, Nd, n, a.psk_m, m);
                    Q = rf_cost(par, Nb, Nd, n, m.tg, m, psk);
                }
                rf_contract(par, Nb, Nd, n, m, psk);
                fill();
                bad = par.sum(P, [&](int p) {
                    int kind, l;
                    rf_param(p, n, has_tau, &kind, &l);
                    double s = rf_jhx(kind, l, m);
                    for (int q = 0; q < n; ++q) s -= rf_sym(m.A, ld, p, q) * m.tg[q].cr + rf_sym(m.A, ld, p, n + q) * m.tg[q].ci;
                    const double gpp = m.A[p * ld + p];
                    m.g[p] = s;
                    m.dsc[p] = 1.0 / sqrt(gpp);
                    return gpp > 0.0 && sc_finite(gpp) ? 0.0 : 1.0;
                });
                if (bad > 0.0) {
                    state = RF_GAVE_UP;
                    break;
                }
                rf_scale(par, P, ld, m);
                for (;;) {
                    double moved = INFINITY, Qt = NAN;
                    if (rf_factor(par, P, ld, lambda, m)) {
                        par.each(P, [&](int p) { m.step[p] = m.dsc[p] * m.g[p]; });
                        rf_solve(par, P, ld, m);
                        double mv = 0.0;
                        bool nan = false;
                        for (int l = 0; l < n; ++l) {
                            const double dt = has_tau ? fabs(m.step[first + l]) * (double)Nd : 0.0;
                            const double df = has_f ? fabs(m.step[first + (has_tau ? n : 0) + l]) * (double)Nb : 0.0;
                            nan = nan || dt != dt || df != df;
                            mv = dt > mv ? dt : mv;
                            mv = df > mv ? df : mv;
                        }
                        const double scale = mv > REFINE_MAX_MOVE ? REFINE_MAX_MOVE / mv : 1.0;
                        moved = nan ? NAN : mv * scale;
                        par.each(n, [&](int l) {
                            CrbTarget t = m.tg[l];
                            t.cr += scale * m.step[l];
                            t.ci += scale * m.step[n + l];
                            if (has_tau) t.tau += scale * m.step[first + l];
                            if (has_f) t.f += scale * m.step[first + (has_tau ? n : 0) + l];
                            m.trial[l] = t;
                        });
                        rf_tables(par, Nb, Nd, n, m.trial, m.tab);
                        Qt = rf_cost(par, Nb, Nd, n, m.trial, m, psk);
                    }
                    if (Qt <= Q) {
                        par.each(n, [&](int l) { m.tg[l] = m.trial[l]; });
                        Q = Qt;
                        lambda /= 10.0;
                        done = moved <= a.tol;
                        break;
                    }
                    lambda *= 10.0;
                    if (moved <= a.tol || lambda > REFINE_LAMBDA_MAX) {
                        if (!(moved <= a.tol)) state = RF_GAVE_UP;
                        done = true;
                        break;
                    }
                }
            }
        }
    }
    const double flips = par.sum(D, [&](int i) { return m.k[i] != m.k0[i] ? 1.0 : 0.0; });
    par.each(Le, [&](int j) {
        rows_out[3 * j] = rows_out[3 * j + 1] = rows_out[3 * j + 2] = NAN;
        C_out[2 * j] = C_out[2 * j + 1] = NAN;
    });
    par.each(n, [&](int l) {
        const int j = m.idx[l];
        const CrbTarget t = m.tg[l];
        rows_out[3 * j] = t.tau;
        rows_out[3 * j + 1] = t.f;
        rows_out[3 * j + 2] = sqrt(t.cr * t.cr + t.ci * t.ci);
        C_out[2 * j] = t.cr;
        C_out[2 * j + 1] = t.ci;
    });
    if (sym) par.each(D, [&](int i) { sym[i] = (int32_t)m.k[i]; });
    par.each(1, [&](int) {
        info[0] = Q;
        info[1] = Q / (double)D;
        info[2] = (double)used;
        info[3] = flips;
        info[4] = (double)state;
    });
}

}  // namespace admmnet
