// crb_model.cpp -- csrc/crb_core.h on the host, with the wave of csrc/crb.hip emulated: the lanes are loops, a __shfl is a plain
// index, a wave sum adds the lanes' values in the butterfly's pairing.  A stand-alone program (its own main): tests/test_crb.py
// builds it with -fsanitize=address,undefined, feeds it the case table and holds its bounds to metrics.crb_host.
//
//   input   (the file named by argv[1])  the number of scenes, then per scene "Nb Nd L is_snr noise" and L lines "tau f Re(C) Im(C)"
//   output  per scene "state v" (state: -1 bounded, 1 non-finite input or noise, 2 not positive definite) and L lines "b_tau b_f"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "crb_core.h"
#include "score_core.h"

using namespace admmnet;

static double wave_sum(const double *lane) {   // wave_sum (float64): xor-butterfly over 64 lanes, as lane 0 sees it
    double v[64];
    for (int i = 0; i < 64; ++i) v[i] = lane[i];
    for (int o = 32; o > 0; o >>= 1)
        for (int i = 0; i < o; ++i) v[i] += v[i + o];
    return v[0];
}

// the body of crb_kernel for one scene whose L_true = L lies inside
static int scene(int Nb, int Nd, int L, bool is_snr, double nz, const std::vector<CrbTarget> &tg, double *v_out,
                 std::vector<double> &b_tau, std::vector<double> &b_f) {
    b_tau.assign(L, NAN);
    b_f.assign(L, NAN);
    *v_out = NAN;
    bool bad = !sc_finite(nz) || (!is_snr && !(nz > 0.0));
    for (int l = 0; l < L; ++l) bad = bad || !(sc_finite(tg[l].tau) && sc_finite(tg[l].f) && sc_finite(tg[l].cr) && sc_finite(tg[l].ci));
    if (bad) return 1;
    if (L == 0) return -1;
    const bool has_tau = Nd > 1, has_f = Nb > 1;
    const int P = crb_params(L, has_tau, has_f), ld = P, first = 2 * L;
    std::vector<double> A((size_t)P * P, NAN), dsc(P);   // exactly the scene's P x P: the sanitizer sees any index outside it
    double e[64] = {};
    for (int lane = 0; lane < 64; ++lane)
        for (int pr = lane; pr < L * (L + 1) / 2; pr += 64) {
            int l, m;
            crb_pair_decode(pr, &l, &m);
            e[lane] += crb_pair_fill(l, m, L, Nb, Nd, tg.data(), A.data(), ld);
        }
    const double v = crb_noise_var(is_snr, nz, wave_sum(e), (double)Nb * (double)Nd);
    *v_out = v;
    if (!(v > 0.0 && sc_finite(v))) return 1;
    bool pd = true;
    for (int lane = 0; lane < P; ++lane) {
        const double g = A[lane * ld + lane];
        pd = pd && g > 0.0 && sc_finite(g);
        dsc[lane] = 1.0 / sqrt(g);
    }
    if (!pd) return 2;
    for (int lane = 0; lane < P; ++lane) crb_scale_row(lane, A.data(), ld, dsc.data());
    for (int j = 0; j < P; ++j) {
        double s[CRB_MAXP];
        for (int lane = j; lane < P; ++lane) s[lane] = crb_chol_dot(lane, j, A.data(), ld);
        const double pivot = s[j];
        if (!(pivot >= CRB_PIVOT_MIN)) return 2;
        const double ljj = sqrt(pivot);
        for (int lane = j; lane < P; ++lane) A[j * ld + lane] = lane == j ? ljj : s[lane] / ljj;
    }
    double inv[64] = {};
    for (int lane = 0; first + lane < P; ++lane) {
        const double d = dsc[first + lane];
        inv[lane] = 0.5 * v * (d * d * crb_inv_diag(first + lane, P, A.data(), ld));
    }
    for (int l = 0; l < L; ++l) {
        b_tau[l] = has_tau ? inv[l] : INFINITY;
        b_f[l] = has_f ? inv[(has_tau ? L : 0) + l] : INFINITY;
    }
    return -1;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: crb_model CASES\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r");
    int scenes = 0;
    if (!in || std::fscanf(in, "%d", &scenes) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    // the pair numbering covers every l <= m exactly once
    for (int L = 1; L <= CRB_MAXL; ++L) {
        std::vector<int> seen(L * L, 0);
        for (int pr = 0; pr < L * (L + 1) / 2; ++pr) {
            int l, m;
            crb_pair_decode(pr, &l, &m);
            if (!(0 <= l && l <= m && m < L) || seen[m * L + l]++) {
                std::fprintf(stderr, "FAILED pair %d of %d -> (%d, %d)\n", pr, L, l, m);
                return 1;
            }
        }
    }
    for (int s = 0; s < scenes; ++s) {
        int Nb, Nd, L, is_snr;
        double nz;
        if (std::fscanf(in, "%d %d %d %d %lf", &Nb, &Nd, &L, &is_snr, &nz) != 5 || L < 0 || L > CRB_MAXL || Nb < 1 || Nd < 1) {
            std::fprintf(stderr, "bad scene %d\n", s);
            return 2;
        }
        std::vector<CrbTarget> tg(L);
        for (int l = 0; l < L; ++l)
            if (std::fscanf(in, "%lf %lf %lf %lf", &tg[l].tau, &tg[l].f, &tg[l].cr, &tg[l].ci) != 4) {
                std::fprintf(stderr, "bad target %d of scene %d\n", l, s);
                return 2;
            }
        std::vector<double> b_tau, b_f;
        double v;
        const int state = scene(Nb, Nd, L, is_snr != 0, nz, tg, &v, b_tau, b_f);
        std::printf("%d %.17g\n", state, v);
        for (int l = 0; l < L; ++l) std::printf("%.17g %.17g\n", b_tau[l], b_f[l]);
    }
    std::fclose(in);
    return 0;
}
