// crb_core.h -- the scalar core of the Cramer-Rao bound kernel (crb.hip): everything one lane computes, without a wave in it, so
// that tests/host_model/crb_model.cpp runs the same arithmetic with the lane loop emulated.
//
// The bound (admmnet_crb_f64 in include/admmnet.h has the definition).  With G = Re(J^H J), J = d mu / d theta, the information
// matrix is F = (2 / v) G and the bound of parameter i is (v / 2) [G^-1]_ii.  Every entry of J^H J for the targets (l, m) is a
// constant times S_p(f_m - f_l; Nb) S_q(-(tau_m - tau_l); Nd), S_p(x; N) = sum_{k<N} k^p exp(j 2 pi k x): O(Nb + Nd) per pair.
//     fill      the 4 x 4 block of one target pair l <= m, and its share of sum |mu|^2       crb_pair_fill    (a lane per pair)
//     scale     A = D G D with D = diag(G)^-1/2, so the tau, f and C blocks are comparable   crb_scale_row    (a lane per row)
//     factor    A = L L^T by columns, lane i owns row i                                       crb_chol_dot
//     invert    [A^-1]_ii of the trailing (tau, f) block from the columns of L22^-1           crb_inv_diag     (a lane per column)
// Inside the kernel theta is ordered (Re C, Im C, tau, f): the parameters that are bounded come last, so [A^-1] on them is the
// inverse of the trailing Cholesky block alone.  A is column-major in the lower triangle, A(i, k) at k * ld + i for i >= k; the
// upper triangle of the trailing block takes L22^-1.  An axis of length 1 carries no information about its parameter, which then
// leaves theta.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CRB_HD __host__ __device__ __forceinline__
#else
#define CRB_HD inline
#endif

namespace admmnet {

constexpr int CRB_MAXL = 16;              // most targets of a scene
constexpr int CRB_MAXP = 4 * CRB_MAXL;    // most parameters: one lane each
constexpr int CRB_TOTALS = 8;             // sum tau, sum f, count tau, count f over j < L_true; the same over the hits
constexpr int CRB_STATUS = 3;             // scenes with L_true outside, with a non-finite input or noise, not positive definite
constexpr int CRB_COLS = CRB_TOTALS + CRB_STATUS;
constexpr double CRB_PIVOT_MIN = 1.0 / 1099511627776.0;   // 2^-40, on the unit-diagonal matrix
constexpr double CRB_TWO_PI = 6.283185307179586476925286766559;

enum { CRB_RE = 0, CRB_IM = 1, CRB_TAU = 2, CRB_F = 3 };

struct CrbTarget {
    double tau, f, cr, ci;
};

CRB_HD int crb_params(int L, bool has_tau, bool has_f) { return L * (2 + (has_tau ? 1 : 0) + (has_f ? 1 : 0)); }

// the place of parameter `kind` of target l among the parameters of L targets; -1: it left theta
CRB_HD int crb_index(int kind, int l, int L, bool has_tau, bool has_f) {
    if (kind == CRB_RE) return l;
    if (kind == CRB_IM) return L + l;
    if (kind == CRB_TAU) return has_tau ? 2 * L + l : -1;
    return has_f ? 2 * L + (has_tau ? L : 0) + l : -1;
}

// pair number pr = m (m + 1) / 2 + l with l <= m
CRB_HD void crb_pair_decode(int pr, int *l, int *m) {
    int row = 0;
    while ((row + 1) * (row + 2) / 2 <= pr) ++row;
    *m = row;
    *l = pr - row * (row + 1) / 2;
}

// sin and cos of t turns, |t| <= 1 / 2
CRB_HD void crb_sincos_turns(double t, double *s, double *c) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * t, s, c);
#else
    *s = sin(CRB_TWO_PI * t);
    *c = cos(CRB_TWO_PI * t);
#endif
}

// S_p(x; N) = sum_{k<N} k^p exp(j 2 pi k x), p = 0, 1, 2; the argument is reduced as a fraction of a turn
CRB_HD void crb_power_sums(double x, int N, double *re, double *im) {
    re[0] = re[1] = re[2] = im[0] = im[1] = im[2] = 0.0;
    for (int k = 0; k < N; ++k) {
        const double kd = (double)k, t = kd * x;
        double s, c;
        crb_sincos_turns(t - rint(t), &s, &c);
        re[0] += c;
        im[0] += s;
        re[1] += kd * c;
        im[1] += kd * s;
        re[2] += kd * kd * c;
        im[2] += kd * kd * s;
    }
}

// d mu / d theta = coef * i_b^pb * i_d^pd * exp(j 2 pi (i_b f - i_d tau)):  Re C: 1,  Im C: j,  tau: -j 2 pi C i_d,  f: j 2 pi C i_b
CRB_HD void crb_coef(int kind, const CrbTarget &t, double *cr, double *ci) {
    if (kind == CRB_RE) {
        *cr = 1.0;
        *ci = 0.0;
    } else if (kind == CRB_IM) {
        *cr = 0.0;
        *ci = 1.0;
    } else if (kind == CRB_TAU) {
        *cr = CRB_TWO_PI * t.ci;
        *ci = -CRB_TWO_PI * t.cr;
    } else {
        *cr = -CRB_TWO_PI * t.ci;
        *ci = CRB_TWO_PI * t.cr;
    }
}

// Re(conj(a) b z)
CRB_HD double crb_re_abz(double ar, double ai, double br, double bi, double zr, double zi) {
    return (ar * br + ai * bi) * zr - (ar * bi - ai * br) * zi;
}

// The block of the pair l <= m of L targets into the lower triangle of A, and the pair's share of sum |mu|^2.
CRB_HD double crb_pair_fill(int l, int m, int L, int Nb, int Nd, const CrbTarget *tg, double *A, int ld) {
    const bool has_tau = Nd > 1, has_f = Nb > 1;
    double fr[3], fi[3], tr[3], ti[3];
    crb_power_sums(tg[m].f - tg[l].f, Nb, fr, fi);
    crb_power_sums(-(tg[m].tau - tg[l].tau), Nd, tr, ti);
    for (int a = 0; a < 4; ++a) {
        const int ia = crb_index(a, l, L, has_tau, has_f);
        double ar, ai;
        crb_coef(a, tg[l], &ar, &ai);
        for (int b = 0; b < 4; ++b) {
            const int ib = crb_index(b, m, L, has_tau, has_f);
            if (ia < 0 || ib < 0 || (l == m && a > b)) continue;
            double br, bi;
            crb_coef(b, tg[m], &br, &bi);
            const int p = (a == CRB_F ? 1 : 0) + (b == CRB_F ? 1 : 0), q = (a == CRB_TAU ? 1 : 0) + (b == CRB_TAU ? 1 : 0);
            const double zr = fr[p] * tr[q] - fi[p] * ti[q], zi = fr[p] * ti[q] + fi[p] * tr[q];
            const int hi = ia > ib ? ia : ib, lo = ia > ib ? ib : ia;
            A[lo * ld + hi] = crb_re_abz(ar, ai, br, bi, zr, zi);
        }
    }
    const double zr = fr[0] * tr[0] - fi[0] * ti[0], zi = fr[0] * ti[0] + fi[0] * tr[0];
    const double e = crb_re_abz(tg[l].cr, tg[l].ci, tg[m].cr, tg[m].ci, zr, zi);
    return l == m ? e : 2.0 * e;
}

// the noise variance: given, or from the SNR in the generator's definition, v = sum |mu|^2 / (10^(snr / 10) D)
CRB_HD double crb_noise_var(bool is_snr, double noise, double energy, double D) {
    return is_snr ? energy / (pow(10.0, noise / 10.0) * D) : noise;
}

// row i of A = D G D, unit diagonal; d[k] = G_kk^-1/2
CRB_HD void crb_scale_row(int i, double *A, int ld, const double *d) {
    for (int k = 0; k < i; ++k) A[k * ld + i] *= d[i] * d[k];
    A[i * ld + i] = 1.0;
}

// row i >= j of column j before the division: A_ij - sum_{k<j} L_ik L_jk (i = j: the pivot)
CRB_HD double crb_chol_dot(int i, int j, const double *A, int ld) {
    double s = A[j * ld + i];
    for (int k = 0; k < j; ++k) s -= A[k * ld + i] * A[k * ld + j];
    return s;
}

// [A^-1]_cc for column c >= n1 of a factored P x P matrix whose parameters of interest are n1 .. P - 1: the squared norm of
// column c of L22^-1, which is left in row c of the upper triangle.
CRB_HD double crb_inv_diag(int c, int P, double *A, int ld) {
    const double ycc = 1.0 / A[c * ld + c];
    double sum = ycc * ycc;
    for (int i = c + 1; i < P; ++i) {
        double s = A[c * ld + i] * ycc;
        for (int k = c + 1; k < i; ++k) s += A[k * ld + i] * A[k * ld + c];
        const double y = -s / A[i * ld + i];
        A[i * ld + c] = y;
        sum += y * y;
    }
    return sum;
}

}  // namespace admmnet
