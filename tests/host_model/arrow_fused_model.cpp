// Host (CPU) model of the fused first G-layer at D > 128 -- TEST HARNESS.
// The solver phases of tests/host_model/arrow_model.cpp (the cores of admm_net_amd/csrc/arrow_core.h and dc_core.h, run
// sequentially), then the formulas of arrow.hip's arrow_fused_tail in the order the kernel applies them: the REAL
// eigenvector matrix X entry by entry (arrow_vec_entry), the deflation rotations undone row by row, S = X^T diag(f) X
// as one float fma chain per entry over the eigenvector index (what v_mfma_f32_32x32x2_f32 computes), the phases
// (arrow_phase_entry), the arrow row and the corner.
//   g++ -O2 -shared -fPIC -I admm_net_amd/csrc tests/host_model/arrow_fused_model.cpp -o tests/host_model/libarrow_fused_model.so
#include <algorithm>
#include <cmath>
#include <vector>

#include "arrow_core.h"

using namespace admmnet;

extern "C" {

// C = [[diag h, z], [z^H, alpha]] (the layer's index order: arrow last), z[D] interleaved complex.
// lam_out[n]: eigenvalues ascending.  f == nullptr: eigenvalues only.  Otherwise f[n] = map values in ascending
// eigenvalue order and G_ri[n * n] (interleaved complex, row-major) = V diag(f) V^H.
// stats[4] = {k, deflated, rotations, max secular iterations}.
int arrow_fused_g(int D, float alpha, const float *z_ri, const float *h, const float *f, float *lam_out, float *G_ri,
                  int *stats) {
    const int n = D + 1;
    std::vector<float> zeta(D), phr(D), phim(D);
    for (int i = 0; i < D; ++i) {
        const float re = z_ri[2 * i], im = z_ri[2 * i + 1];
        const float a = std::sqrt(re * re + im * im);
        zeta[i] = a;
        phr[i] = a > 0.f ? re / a : 1.f;
        phim[i] = a > 0.f ? im / a : 0.f;
    }
    // P1: sort h ascending (stable rank counting)
    std::vector<int> perm(D), ipos(D);
    for (int i = 0; i < D; ++i) {
        int r = 0;
        for (int q = 0; q < D; ++q) r += (h[q] < h[i]) || (h[q] == h[i] && q < i);
        perm[r] = i;
        ipos[i] = r;
    }
    // P2: deflation
    std::vector<float> ds(D), zs(D), dl(D), zl(D);
    std::vector<int> src(D);
    std::vector<DcRot> rot(D);
    float dmax = std::fabs(alpha), zmax = 0.f;
    for (int p = 0; p < D; ++p) {
        ds[p] = h[perm[p]];
        zs[p] = zeta[perm[p]];
        dmax = std::max(dmax, std::fabs(ds[p]));
        zmax = std::max(zmax, zs[p]);
    }
    int k = 0, nrot = 0;
    deflate_scan_tol(D, 1.0f, dmax, zmax, ds.data(), zs.data(), dl.data(), zl.data(), src.data(), rot.data(), k, nrot);
    std::vector<int> kidx(D);
    for (int p = 0; p < D; ++p) kidx[src[p]] = (p < k) ? p : -(p + 1) - 1;
    // P4: roots
    std::vector<int> org(k + 1);
    std::vector<float> tau(k + 1), lamd(k + 1), vals(n);
    float zn2 = 0.f;
    for (int i = 0; i < k; ++i) zn2 += zl[i] * zl[i];
    const float znorm = std::sqrt(zn2);
    int itmax = 0;
    if (k == 0) {
        vals[0] = alpha;
    } else {
        for (int j = 0; j <= k; ++j) {
            int nit = 0;
            arrow_root(k, j, alpha, znorm, dl.data(), zl.data(), org[j], tau[j], &nit);
            itmax = std::max(itmax, nit);
            lamd[j] = dl[org[j]];
            vals[j] = lamd[j] + tau[j];
        }
    }
    for (int p = k; p < D; ++p) vals[p + 1] = dl[p];
    // P5: zeta-hat, final positions
    std::vector<float> zh(k);
    for (int i = 0; i < k; ++i) zh[i] = arrow_zhat(k, i, dl.data(), lamd.data(), tau.data());
    std::vector<int> rnk(n);
    for (int s = 0; s < n; ++s) {
        int r = 0;
        for (int q = 0; q < n; ++q) r += (vals[q] < vals[s]) || (vals[q] == vals[s] && q < s);
        rnk[s] = r;
    }
    // P6: norms; everything the slabs need in FINAL order c
    std::vector<float> x0c(n), lamc(n), tauc(n);
    for (int s = 0; s < n; ++s) {
        float xa = 0.f;
        if (s <= k) {
            float nrm = 1.f;
            for (int i = 0; i < k; ++i) {
                const float v = fdiv_fast(zh[i], (lamd[s] - dl[i]) + tau[s]);
                nrm = std::fma(v, v, nrm);
            }
            xa = 1.0f / std::sqrt(nrm);
        }
        const int c = rnk[s];
        const bool root = s <= k && k > 0;
        x0c[c] = xa;
        lamc[c] = root ? lamd[s] : 3.0e38f;
        tauc[c] = root ? tau[s] : 0.f;
        lam_out[c] = vals[s];
    }
    if (stats) {
        stats[0] = k;
        stats[1] = D - k;
        stats[2] = nrot;
        stats[3] = itmax;
    }
    if (!f) return 0;
    // X[c][i], i = ORIGINAL index: what the kernel's thread i writes into row c of a slab
    std::vector<float> X((size_t)n * D);
    for (int i = 0; i < D; ++i) {
        const int kd = kidx[ipos[i]];
        for (int c = 0; c < n; ++c) {
            float v;
            if (kd >= 0) v = arrow_vec_entry(zh[kd], dl[kd], lamc[c], tauc[c], x0c[c]);
            else v = (c == rnk[-kd - 1]) ? 1.f : 0.f;
            X[(size_t)c * D + i] = v;
        }
    }
    // deflation rotations undone (reverse order), row by row
    for (int c = 0; c < n; ++c) {
        float *row = &X[(size_t)c * D];
        for (int q = nrot - 1; q >= 0; --q) {
            const int ia = perm[rot[q].pa], ib = perm[rot[q].pb];
            const float a = row[ia], bb = row[ib];
            row[ia] = rot[q].c * a - rot[q].s * bb;
            row[ib] = rot[q].s * a + rot[q].c * bb;
        }
    }
    auto put = [&](int i, int j, float re, float im) {
        G_ri[2 * ((size_t)i * n + j)] = re;
        G_ri[2 * ((size_t)i * n + j) + 1] = im;
    };
    // S_ij = sum_c (f_c X[c][i]) X[c][j], lower triangle; phases; the mirrored half is the exact conjugate
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            float S = 0.f;
            for (int c = 0; c < n; ++c) S = std::fma(X[(size_t)c * D + i] * f[c], X[(size_t)c * D + j], S);
            if (i == j) {
                put(i, i, S, 0.f);
            } else {
                float re, im;
                arrow_phase_entry(S, phr[i], phim[i], phr[j], phim[j], re, im);
                put(i, j, re, im);
                put(j, i, re, -im);
            }
        }
    // arrow row G[D][o] = (sum_c f_c x0_c X[c][o]) conj(p_o), corner sum_c f_c x0_c^2
    float g00 = 0.f;
    for (int c = 0; c < n; ++c) g00 = std::fma(x0c[c] * f[c], x0c[c], g00);
    put(D, D, g00, 0.f);
    for (int o = 0; o < D; ++o) {
        float arow = 0.f;
        for (int c = 0; c < n; ++c) arow = std::fma(x0c[c] * f[c], X[(size_t)c * D + o], arow);
        const float gr = arow * phr[o], gim = -(arow * phim[o]);
        put(D, o, gr, gim);
        put(o, D, gr, -gim);
    }
    return 0;
}
}
