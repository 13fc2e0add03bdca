// order_model.cpp -- csrc/order_core.h on the host, with the workgroup of csrc/order.hip emulated by host_par.h's HostPar<ORDER_THREADS>,
// which states the order of every shared loop and sum once for the four scene models.  A stand-alone program (its own main):
// tests/test_order.py builds it with -fsanitize=address,undefined, feeds it the case table and holds its results to
// order.select_host.  Every array has exactly the entries the kernel's LDS layout gives it, so the sanitizer sees any index
// outside.
//
//   input   (the file named by argv[1])  the number of scenes, then per scene "Nb Nd Le n_cand n_held symbols psk_m psk_phase
//           penalty max_order" (n_cand, n_held: "none" or a number; symbols: 0 or 1), Le lines "tau f height" and D lines
//           "Re(y) Im(y) Re(b) Im(b) k"
//   output  per scene "state K n_sel cost", one line of perm, one of rss, Le lines "tau f |C| Re(C) Im(C)" and D lines of the residual
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_par.h"
#include "order_core.h"

using namespace admmnet;

static double number(const char *s) { return std::strtod(s, nullptr); }   // reads nan and inf too

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: order_model CASES\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r");
    int scenes = 0;
    if (!in || std::fscanf(in, "%d", &scenes) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    char w[10][64];
    for (int s = 0; s < scenes; ++s) {
        if (std::fscanf(in, "%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8],
                        w[9]) != 10) {
            std::fprintf(stderr, "bad scene %d\n", s);
            return 2;
        }
        OrderArgs a = {std::atoi(w[0]), std::atoi(w[1]), std::atoi(w[2]), std::atoi(w[6]), number(w[7]), number(w[8]), std::atoi(w[9])};
        const bool has_cand = std::strcmp(w[3], "none") != 0, has_held = std::strcmp(w[4], "none") != 0, has_sym = std::atoi(w[5]) != 0;
        const int32_t n_cand = has_cand ? std::atoi(w[3]) : 0, n_held = has_held ? std::atoi(w[4]) : 0;
        if (a.Nb < 1 || a.Nd < 1 || a.Le < 1 || a.Le > CRB_MAXL || a.psk_m < 2 || a.psk_m > REFINE_MAX_M || a.max_order < 1 ||
            a.max_order > a.Le || !(a.penalty >= 0.0)) {
            std::fprintf(stderr, "bad sizes in scene %d\n", s);
            return 2;
        }
        const int D = a.Nb * a.Nd, Le = a.Le;
        std::vector<double> rows(3 * Le), rows_out(3 * Le), C_out(2 * Le), info(ORDER_INFO), rss_out(Le + 1);
        std::vector<float> y(2 * D), b(2 * D), residual(2 * D);
        std::vector<int32_t> sym(D), perm(Le);
        int32_t n_sel = -1;
        char v[5][64];
        for (int j = 0; j < Le; ++j) {
            if (std::fscanf(in, "%63s %63s %63s", v[0], v[1], v[2]) != 3) return 2;
            for (int c = 0; c < 3; ++c) rows[3 * j + c] = number(v[c]);
        }
        for (int i = 0; i < D; ++i) {
            if (std::fscanf(in, "%63s %63s %63s %63s %63s", v[0], v[1], v[2], v[3], v[4]) != 5) return 2;
            y[2 * i] = (float)number(v[0]);
            y[2 * i + 1] = (float)number(v[1]);
            b[2 * i] = (float)number(v[2]);
            b[2 * i + 1] = (float)number(v[3]);
            sym[i] = std::atoi(v[4]);
        }
        std::vector<RfC> x(D), pt(REFINE_MAX_M), tab(od_tab_count(a.Nb, a.Nd, Le)), rs(Le * a.Nb), G(Le * Le), F(Le * Le),
            c((Le + 1) * Le), wv(Le), C(Le);
        std::vector<double> d((Le + 1) * Le), tau(Le), f(Le), rss(Le + 1);
        std::vector<int> idx(Le), pick(Le), pm(Le), meta(OD_META);
        OrderMem m = {x.data(), pt.data(), tab.data(), rs.data(), G.data(), F.data(), c.data(), d.data(), wv.data(), C.data(),
                      tau.data(), f.data(), rss.data(), idx.data(), pick.data(), pm.data(), meta.data()};
        HostPar<ORDER_THREADS> par;
        order_scene(par, a, m, y.data(), b.data(), rows.data(), has_cand ? &n_cand : nullptr, has_held ? &n_held : nullptr,
                    has_sym ? sym.data() : nullptr, perm.data(), &n_sel, rss_out.data(), rows_out.data(), C_out.data(),
                    residual.data(), info.data());
        std::printf("%d %d %d %.17g\n", (int)info[3], (int)info[2], (int)n_sel, info[0]);
        for (int j = 0; j < Le; ++j) std::printf(j + 1 < Le ? "%d " : "%d\n", perm[j]);
        for (int k = 0; k <= Le; ++k) std::printf(k < Le ? "%.17g " : "%.17g\n", rss_out[k]);
        for (int j = 0; j < Le; ++j)
            std::printf("%.17g %.17g %.17g %.17g %.17g\n", rows_out[3 * j], rows_out[3 * j + 1], rows_out[3 * j + 2], C_out[2 * j],
                        C_out[2 * j + 1]);
        for (int i = 0; i < D; ++i) std::printf("%.9g %.9g\n", residual[2 * i], residual[2 * i + 1]);
    }
    std::fclose(in);
    return 0;
}
