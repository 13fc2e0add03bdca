// cfar_core.h -- the scene loop of the CFAR detector (cfar.hip): the zero-padded 2-D periodogram of x = y conj(s), thresholded at a
// constant false-alarm rate against a known or an estimated noise level, its local maxima returned as rows (admmnet_cfar_f64 in
// include/admmnet.h has the definition).  Written ONCE over the `Par` of refine_core.h (par.each, par.sum), so that
// tests/host_model/cfar_model.cpp runs the same arithmetic with the threads emulated.  Everything between two such calls is
// computed by every thread from what the last one left in memory, so every branch around them is uniform.  The pieces:
//     tables     exp(-j 2 pi k / n_f), k < n_f, and exp(+j 2 pi k / n_tau), k < n_tau, each from sincospi of k / n; a product
//                i_b j or i_d i is reduced modulo n in integer arithmetic and looked up -- never a recurrence          cf_tables
//     map        img[j][i_d] = sum_ib x[i_b][i_d] (-1)^i_b tf[(i_b j) mod n_f]  (the -1/2 of f_j is the sign), then
//                P[j][i] = |sum_id img[j][i_d] tt[(i_d i) mod n_tau]|^2 / D, both sums in index order                   cf_map
//     window     the offsets (p, q) of the training cells in resolution cells, p outer and q inner, both ascending       cf_window
//     level      Z of a cell: the given value, the mean of the training cells added in window order, or the k-th smallest of
//                them found by counting against a pivot (cf_kth: no storage, about 2 N ln N reads, and the value does not
//                depend on how ties are ordered)                                                                      cf_level
//     detections a cell over the threshold that beats its 8 torus neighbours; contiguous chunks of cells are counted, the counts
//                are prefixed by one thread, every chunk writes its detections behind its prefix: the list is in index order
//     order      the place of a detection = the number of detections that beat it (O(n_det^2 / threads)); the first Le are rows
#pragma once
#include "refine_core.h"

namespace admmnet {

constexpr int CFAR_THREADS = REFINE_THREADS;
constexpr int CFAR_INFO = 2;               // level, state
constexpr int CFAR_INFO_STATE = 1;         // the column of the state
constexpr int CFAR_COUNTS = 2;             // n_det, n_over
constexpr int CFAR_STATUS = 2;             // scenes non-finite, scenes outside
constexpr int CFAR_MAX_OVERSAMPLE = 8;
constexpr int CFAR_MAX_REACH = 8;          // guard + train at most
constexpr int CFAR_MAX_TRAIN = (2 * CFAR_MAX_REACH + 1) * (2 * CFAR_MAX_REACH + 1) - 1;   // N <= 288 training cells
constexpr int CFAR_OFF_BIAS = CFAR_MAX_REACH * CFAR_MAX_OVERSAMPLE;   // makes an offset in map cells non-negative
constexpr int CFAR_MAX_CELLS = 65535;      // a detection is listed by a 16-bit cell index (160 KiB of LDS end far below)

enum { CF_KNOWN = 0, CF_CA = 1, CF_OS = 2 };
enum { CF_DONE = 0, CF_NONFINITE = RF_NONFINITE, CF_OUTSIDE = RF_OUTSIDE };

struct CfarArgs {
    int Nb, Nd, r, Le, method, guard, train, rank, psk_m;
    double psk_phase, alpha;
};

// the reach of the window on an axis of length n: 0 where the axis has one sample
CRB_HD int cf_reach(int n, int cells) { return n > 1 ? cells : 0; }

// N = |Omega|
CRB_HD int cf_train_count(int Nb, int Nd, int guard, int train) {
    const int Wb = cf_reach(Nb, guard + train), Wd = cf_reach(Nd, guard + train), Gb = cf_reach(Nb, guard), Gd = cf_reach(Nd, guard);
    return (2 * Wb + 1) * (2 * Wd + 1) - (2 * Gb + 1) * (2 * Gd + 1);
}

struct CfarMem {
    RfC *x;              // [D] y conj(s)
    RfC *img;            // [n_f Nd]
    double *map;         // [n_f n_tau]
    RfC *tf, *tt;        // [n_f], [n_tau]
    RfC *pt;             // [REFINE_MAX_M] the constellation
    int *off;            // [CFAR_MAX_TRAIN] the first N: the training offsets in map cells, p r in the high 16 bits and q r in the low ones, each plus CFAR_OFF_BIAS
    uint8_t *flag;       // [n_f n_tau] bit 0 over, bit 1 detection
    uint16_t *list;      // [n_f n_tau] the detections in index order
    int *chunk;          // [CFAR_THREADS + 1] detections per chunk of cells, then their exclusive prefix; the last is n_det
    int *slot;           // [CRB_MAXL] the cell of every row, -1: none
};

template <class Par>
CRB_HD void cf_tables(Par &par, int nf, int nt, const CfarMem &m) {
    par.each(nf + nt, [&](int item) {
        if (item < nf)
            m.tf[item] = rf_turn(-((double)item / (double)nf));
        else
            m.tt[item - nf] = rf_turn((double)(item - nf) / (double)nt);
    });
}

template <class Par>
CRB_HD void cf_map(Par &par, int Nb, int Nd, int nf, int nt, const CfarMem &m) {
    par.each(nf * Nd, [&](int item) {
        const int j = item / Nd, id = item - j * Nd;
        RfC s = {0.0, 0.0};
        for (int ib = 0, k = 0; ib < Nb; ++ib) {             // k = (i_b j) mod n_f, exact in integers
            const RfC t = rf_mul(m.x[ib * Nd + id], m.tf[k]);
            s.re += (ib & 1) ? -t.re : t.re;
            s.im += (ib & 1) ? -t.im : t.im;
            k = k + j >= nf ? k + j - nf : k + j;
        }
        m.img[item] = s;
    });
    const double D = (double)(Nb * Nd);
    par.each(nf * nt, [&](int c) {
        const int j = c / nt, i = c - j * nt;
        RfC s = {0.0, 0.0};
        for (int id = 0, k = 0; id < Nd; ++id) {             // k = (i_d i) mod n_tau
            const RfC t = rf_mul(m.img[j * Nd + id], m.tt[k]);
            s.re += t.re;
            s.im += t.im;
            k = k + i >= nt ? k + i - nt : k + i;
        }
        m.map[c] = (s.re * s.re + s.im * s.im) / D;
    });
}

template <class Par>
CRB_HD void cf_window(Par &par, const CfarArgs &a, const CfarMem &m) {
    par.each(1, [&](int) {
        const int Wb = cf_reach(a.Nb, a.guard + a.train), Wd = cf_reach(a.Nd, a.guard + a.train);
        const int Gb = cf_reach(a.Nb, a.guard), Gd = cf_reach(a.Nd, a.guard);
        int n = 0;
        for (int p = -Wb; p <= Wb; ++p)
            for (int q = -Wd; q <= Wd; ++q) {
                if (p >= -Gb && p <= Gb && q >= -Gd && q <= Gd) continue;
                m.off[n++] = (p * a.r + CFAR_OFF_BIAS) << 16 | (q * a.r + CFAR_OFF_BIAS);
            }
    });
}

// the training cell `n` of the cell (j, i): r map cells per resolution cell, round the torus (|p| r <= n_f / 2)
CRB_HD double cf_train_cell(int n, int j, int i, int nf, int nt, const CfarMem &m) {
    const int o = m.off[n];
    int jj = j + (o >> 16) - CFAR_OFF_BIAS, ii = i + (o & 0xffff) - CFAR_OFF_BIAS;
    jj = jj < 0 ? jj + nf : (jj >= nf ? jj - nf : jj);
    ii = ii < 0 ? ii + nt : (ii >= nt ? ii - nt : ii);
    return m.map[jj * nt + ii];
}

// The k-th smallest of the N training cells of (j, i), without storage: a pivot v is the answer iff fewer than k cells are below it
// and at least k are not above it; otherwise the answer lies strictly on one side of v, and the pass that counted has also kept the
// first cell (in window order) on either side within the bounds known so far, which is the next pivot.  The first pivot is cell 0.
// A pass is N reads; the bounds shrink as in a quickselect, about 2 ln N passes for cells in no particular order, N at worst.
CRB_HD double cf_kth(int k, int N, int j, int i, int nf, int nt, const CfarMem &m) {
    double lo = -INFINITY, hi = INFINITY, v = cf_train_cell(0, j, i, nf, nt, m);
    for (int pass = 0; pass < N; ++pass) {
        int below = 0, not_above = 0;
        double next_lo = NAN, next_hi = NAN;
        for (int n = 0; n < N; ++n) {
            const double w = cf_train_cell(n, j, i, nf, nt, m);
            below += w < v ? 1 : 0;
            not_above += w <= v ? 1 : 0;
            if (w > lo && w < v && next_lo != next_lo) next_lo = w;
            if (w > v && w < hi && next_hi != next_hi) next_hi = w;
        }
        if (below < k && k <= not_above) return v;
        if (k <= below) {
            hi = v;
            v = next_lo;
        } else {
            lo = v;
            v = next_hi;
        }
    }
    return v;   // not reached: every pass rules its pivot out, and the map is finite
}

CRB_HD double cf_level(int c, const CfarArgs &a, int N, int nf, int nt, double known, const CfarMem &m) {
    if (a.method == CF_KNOWN) return known;
    const int j = c / nt, i = c - j * nt;
    if (a.method == CF_OS) return cf_kth(a.rank, N, j, i, nf, nt, m);
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += cf_train_cell(n, j, i, nf, nt, m);
    return s / (double)N;
}

// cell c beats cell d
CRB_HD bool cf_beats(int c, int d, const double *map) { return map[c] > map[d] || (map[c] == map[d] && c < d); }

CRB_HD bool cf_is_peak(int c, int nf, int nt, const double *map) {
    const int j = c / nt, i = c - j * nt;
    for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
            const int jj = (j + dj + nf) % nf, ii = (i + di + nt) % nt, d = jj * nt + ii;
            if (d != c && !cf_beats(c, d, map)) return false;
        }
    return true;
}

// One scene.  y, b: D pairs (re, im) of float; sym: null or D; noise_var: null or the scene's; rows: Le rows of 3; counts:
// CFAR_COUNTS; info: CFAR_INFO; map_out: null or n_f n_tau.
template <class Par>
CRB_HD void cfar_scene(Par &par, const CfarArgs &a, const CfarMem &m, const float *y, const float *b, const int32_t *sym,
                       const double *noise_var, double *rows, int32_t *counts, double *info, double *map_out) {
    const int Nb = a.Nb, Nd = a.Nd, Le = a.Le, D = Nb * Nd, nf = a.r * Nb, nt = a.r * Nd, cells = nf * nt;
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
        par.each(3 * Le, [&](int k) { rows[k] = NAN; });
        if (map_out) par.each(cells, [&](int c) { map_out[c] = NAN; });
        par.each(1, [&](int) {
            counts[0] = counts[1] = 0;
            info[0] = NAN;
            info[1] = (double)state;
        });
        return;
    }
    cf_tables(par, nf, nt, m);
    cf_map(par, Nb, Nd, nf, nt, m);
    if (a.method != CF_KNOWN) cf_window(par, a, m);
    const int N = a.method != CF_KNOWN ? cf_train_count(Nb, Nd, a.guard, a.train) : 0;
    const double zsum = par.sum(cells, [&](int c) {
        const double Z = cf_level(c, a, N, nf, nt, known, m);
        m.flag[c] = m.map[c] > a.alpha * Z ? 1 : 0;
        return Z;
    });
    const double n_over = par.sum(cells, [&](int c) { return (double)m.flag[c]; });
    const int per = (cells + CFAR_THREADS - 1) / CFAR_THREADS;
    par.each(CFAR_THREADS, [&](int t) {
        int n = 0;
        for (int c = t * per; c < (t + 1) * per && c < cells; ++c) {
            const bool det = (m.flag[c] & 1) && cf_is_peak(c, nf, nt, m.map);
            if (det) m.flag[c] |= 2;
            n += det ? 1 : 0;
        }
        m.chunk[t] = n;
    });
    par.each(1, [&](int) {
        int at = 0;
        for (int t = 0; t < CFAR_THREADS; ++t) {
            const int n = m.chunk[t];
            m.chunk[t] = at;
            at += n;
        }
        m.chunk[CFAR_THREADS] = at;
    });
    par.each(CFAR_THREADS, [&](int t) {
        int at = m.chunk[t];
        for (int c = t * per; c < (t + 1) * per && c < cells; ++c)
            if (m.flag[c] & 2) m.list[at++] = (uint16_t)c;
        if (t < Le) m.slot[t] = -1;
    });
    const int n_det = m.chunk[CFAR_THREADS];
    par.each(n_det, [&](int e) {
        const int c = m.list[e];
        int place = 0;
        for (int k = 0; k < n_det && place < Le; ++k) place += k != e && cf_beats(m.list[k], c, m.map) ? 1 : 0;
        if (place < Le) m.slot[place] = c;
    });
    par.each(Le, [&](int l) {
        const int c = m.slot[l];
        const int j = c < 0 ? 0 : c / nt, i = c < 0 ? 0 : c - j * nt;
        rows[3 * l] = c < 0 ? NAN : (double)i / (double)nt;
        rows[3 * l + 1] = c < 0 ? NAN : (double)j / (double)nf - 0.5;
        rows[3 * l + 2] = c < 0 ? NAN : m.map[c];
    });
    if (map_out) par.each(cells, [&](int c) { map_out[c] = m.map[c]; });
    par.each(1, [&](int) {
        counts[0] = n_det;
        counts[1] = (int32_t)n_over;
        info[0] = a.method == CF_KNOWN ? known : zsum / (double)cells;
        info[1] = (double)state;
    });
}

}  // namespace admmnet
