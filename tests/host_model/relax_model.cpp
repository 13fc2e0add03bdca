// relax_model.cpp -- csrc/relax_core.h on the host, with the workgroup of csrc/cfar_relax.hip emulated by host_par.h's HostPar<CFAR_THREADS>,
// which states the order of every shared loop and sum once for the four scene models.  A stand-alone program (its own main):
// tests/test_relax.py builds it with -fsanitize=address,undefined, feeds it the case table and holds its results to
// detect.cfar_relax_host.  Every array has exactly the entries the kernel's LDS layout gives it, so the sanitizer sees any index
// outside.
//
//   input   (the file named by argv[1])  the number of scenes, then per scene "Nb Nd r Le method guard train rank alpha symbols
//           psk_m psk_phase noise_var iters sweeps" (symbols: 0 or 1; noise_var: "none" or a number) and D lines
//           "Re(y) Im(y) Re(b) Im(b) k"
//   output  per scene "state n_det more maps level resid", Le lines "tau f height Re(c) Im(c)" and n_f n_tau lines of the last map
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_par.h"
#include "relax_core.h"

using namespace admmnet;

static double number(const char *s) { return std::strtod(s, nullptr); }   // reads nan and inf too

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: relax_model CASES\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r");
    int scenes = 0;
    if (!in || std::fscanf(in, "%d", &scenes) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    char w[15][64];
    for (int s = 0; s < scenes; ++s) {
        for (int k = 0; k < 15; ++k)
            if (std::fscanf(in, "%63s", w[k]) != 1) {
                std::fprintf(stderr, "bad scene %d\n", s);
                return 2;
            }
        RelaxArgs ra = {{std::atoi(w[0]), std::atoi(w[1]), std::atoi(w[2]), std::atoi(w[3]), std::atoi(w[4]), std::atoi(w[5]),
                         std::atoi(w[6]), std::atoi(w[7]), std::atoi(w[10]), number(w[11]), number(w[8])},
                        std::atoi(w[13]), std::atoi(w[14])};
        const CfarArgs &a = ra.c;
        const bool has_sym = std::atoi(w[9]) != 0, has_noise = std::strcmp(w[12], "none") != 0;
        const double noise = has_noise ? number(w[12]) : 0.0;
        const bool known = a.method == CF_KNOWN;
        const int W = a.guard + a.train;
        if (a.Nb < 1 || a.Nd < 1 || a.r < 1 || a.r > CFAR_MAX_OVERSAMPLE || a.Nb * a.Nd * a.r * a.r > CFAR_MAX_CELLS || a.Le < 1 ||
            a.Le > CRB_MAXL || a.psk_m < 2 || a.psk_m > REFINE_MAX_M || a.method < 0 || a.method > 2 || known != has_noise ||
            (!known && (a.guard < 0 || a.train < 1 || W > CFAR_MAX_REACH || (a.Nb > 1 && 2 * W + 1 > a.Nb) ||
                        (a.Nd > 1 && 2 * W + 1 > a.Nd) || cf_train_count(a.Nb, a.Nd, a.guard, a.train) < 1)) ||
            (a.method == CF_OS && (a.rank < 1 || a.rank > cf_train_count(a.Nb, a.Nd, a.guard, a.train))) || ra.iters < 0 ||
            ra.iters > RELAX_MAX_ITERS || ra.sweeps < 0 || ra.sweeps > RELAX_MAX_SWEEPS) {
            std::fprintf(stderr, "bad sizes in scene %d\n", s);
            return 2;
        }
        const int D = a.Nb * a.Nd, Le = a.Le, nf = a.r * a.Nb, nt = a.r * a.Nd, cells = nf * nt;
        std::vector<float> y(2 * D), b(2 * D);
        std::vector<int32_t> sym(D);
        char v[5][64];
        for (int i = 0; i < D; ++i) {
            if (std::fscanf(in, "%63s %63s %63s %63s %63s", v[0], v[1], v[2], v[3], v[4]) != 5) return 2;
            y[2 * i] = (float)number(v[0]);
            y[2 * i + 1] = (float)number(v[1]);
            b[2 * i] = (float)number(v[2]);
            b[2 * i + 1] = (float)number(v[3]);
            sym[i] = std::atoi(v[4]);
        }
        std::vector<RfC> x(D), img(nf * a.Nd), tf(nf), tt(nt), pt(REFINE_MAX_M), u(a.Nb), vd(a.Nd);
        std::vector<double> map(cells), rows(3 * Le), amp(2 * Le), info(RELAX_INFO), map_out(cells);
        std::vector<int> off(known ? 0 : cf_train_count(a.Nb, a.Nd, a.guard, a.train));
        std::vector<uint8_t> flag(cells);
        std::vector<RelaxTarget> tg(CRB_MAXL);
        std::vector<int32_t> counts(RELAX_COUNTS, -1);
        RelaxMem m = {{x.data(), img.data(), map.data(), tf.data(), tt.data(), pt.data(), off.data(), flag.data(), nullptr, nullptr,
                       nullptr},
                      u.data(), vd.data(), tg.data()};
        HostPar<CFAR_THREADS> par;
        relax_scene(par, ra, m, y.data(), b.data(), has_sym ? sym.data() : nullptr, has_noise ? &noise : nullptr, rows.data(),
                    amp.data(), counts.data(), info.data(), map_out.data());
        std::printf("%d %d %d %d %.17g %.17g\n", (int)info[2], (int)counts[0], (int)counts[1], (int)counts[2], info[0], info[1]);
        for (int j = 0; j < Le; ++j)
            std::printf("%.17g %.17g %.17g %.17g %.17g\n", rows[3 * j], rows[3 * j + 1], rows[3 * j + 2], amp[2 * j], amp[2 * j + 1]);
        for (int c = 0; c < cells; ++c) std::printf("%.17g\n", map_out[c]);
    }
    std::fclose(in);
    return 0;
}
