// refine_model.cpp -- csrc/refine_core.h on the host, with the workgroup of csrc/refine.hip emulated by host_par.h's HostPar<REFINE_THREADS>,
// which states the order of every shared loop and sum once for the four scene models.  A stand-alone program (its own main):
// tests/test_refine.py builds it with -fsanitize=address,undefined, feeds it the case table and holds its results to
// refine.refine_host.  Every array has exactly the entries the kernel's LDS layout gives it, so the sanitizer sees any index
// outside.
//
//   input   (the file named by argv[1])  the number of scenes, then per scene "Nb Nd Le n_est mode psk_m psk_phase iters tol"
//           (n_est: "none" or a number), Le lines "tau f height" and D lines "Re(y) Im(y) Re(b) Im(b)"
//   output  per scene "state iterations flips Q", Le lines "tau f |C| Re(C) Im(C)" and one line of the D symbols
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_par.h"
#include "refine_core.h"

using namespace admmnet;

static double number(const char *s) { return std::strtod(s, nullptr); }   // reads nan and inf too

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: refine_model CASES\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r");
    int scenes = 0;
    if (!in || std::fscanf(in, "%d", &scenes) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    // rf_param is the inverse of crb_index
    for (int n = 1; n <= CRB_MAXL; ++n)
        for (int axes = 0; axes < 4; ++axes) {
            const bool has_tau = axes & 1, has_f = axes & 2;
            for (int p = 0; p < crb_params(n, has_tau, has_f); ++p) {
                int kind, l;
                rf_param(p, n, has_tau, &kind, &l);
                if (crb_index(kind, l, n, has_tau, has_f) != p) {
                    std::fprintf(stderr, "FAILED parameter %d of %d targets -> (%d, %d)\n", p, n, kind, l);
                    return 1;
                }
            }
        }
    char w[9][64];
    for (int s = 0; s < scenes; ++s) {
        if (std::fscanf(in, "%63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]) != 9) {
            std::fprintf(stderr, "bad scene %d\n", s);
            return 2;
        }
        RefineArgs a = {std::atoi(w[0]), std::atoi(w[1]), std::atoi(w[2]), std::atoi(w[4]), std::atoi(w[5]), number(w[6]),
                        std::atoi(w[7]), number(w[8])};
        const bool has_n = std::strcmp(w[3], "none") != 0;
        const int32_t n_est = has_n ? std::atoi(w[3]) : 0;
        if (a.Nb < 1 || a.Nd < 1 || a.Le < 1 || a.Le > CRB_MAXL || a.psk_m < 2 || a.psk_m > REFINE_MAX_M || a.iters < 1 ||
            a.iters > REFINE_MAX_ITERS) {
            std::fprintf(stderr, "bad sizes in scene %d\n", s);
            return 2;
        }
        const int D = a.Nb * a.Nd, P = rf_pmax(a.Nb, a.Nd, a.Le);
        std::vector<double> rows(3 * a.Le), rows_out(3 * a.Le), C_out(2 * a.Le), info(REFINE_INFO);
        std::vector<float> y(2 * D), b(2 * D);
        std::vector<int32_t> sym(D);
        char v[4][64];
        for (int j = 0; j < a.Le; ++j) {
            if (std::fscanf(in, "%63s %63s %63s", v[0], v[1], v[2]) != 3) return 2;
            for (int c = 0; c < 3; ++c) rows[3 * j + c] = number(v[c]);
        }
        for (int i = 0; i < D; ++i) {
            if (std::fscanf(in, "%63s %63s %63s %63s", v[0], v[1], v[2], v[3]) != 4) return 2;
            y[2 * i] = (float)number(v[0]);
            y[2 * i + 1] = (float)number(v[1]);
            b[2 * i] = (float)number(v[2]);
            b[2 * i + 1] = (float)number(v[3]);
        }
        std::vector<RfC> z(D), pt(a.psk_m), tab(rf_tab_count(a.Nb, a.Nd, a.Le)), rs(rf_rows_count(a.Nb, a.Le)), cont(RF_CONT);
        std::vector<uint8_t> k(D), k0(D);
        std::vector<double> A((size_t)P * P, NAN), g(P), dsc(P), step(P), col(P);
        std::vector<CrbTarget> tg(a.Le), trial(a.Le);
        std::vector<int> idx(RF_IDX);
        RefineMem m = {z.data(), k.data(), k0.data(), pt.data(), A.data(), tab.data(), rs.data(), cont.data(), tg.data(), trial.data(),
                       g.data(), dsc.data(), step.data(), col.data(), idx.data()};
        HostPar<REFINE_THREADS> par;
        refine_scene(par, a, m, y.data(), b.data(), rows.data(), has_n ? &n_est : nullptr, rows_out.data(), C_out.data(), info.data(),
                     sym.data());
        std::printf("%d %d %d %.17g\n", (int)info[4], (int)info[2], (int)info[3], info[0]);
        for (int j = 0; j < a.Le; ++j)
            std::printf("%.17g %.17g %.17g %.17g %.17g\n", rows_out[3 * j], rows_out[3 * j + 1], rows_out[3 * j + 2], C_out[2 * j],
                        C_out[2 * j + 1]);
        for (int i = 0; i < D; ++i) std::printf(i + 1 < D ? "%d " : "%d\n", sym[i]);
    }
    std::fclose(in);
    return 0;
}
