// cfar_model.cpp -- csrc/cfar_core.h on the host, with the workgroup of csrc/cfar.hip emulated by host_par.h's HostPar<CFAR_THREADS>,
// which states the order of every shared loop and sum once for the four scene models.  A stand-alone program (its own main):
// tests/test_detect.py builds it with -fsanitize=address,undefined, feeds it the case table and holds its results to
// detect.cfar_host.  Every array has exactly the entries the kernel's LDS layout gives it, so the sanitizer sees any index
// outside.
//
//   input   (the file named by argv[1])  the number of scenes, then per scene "Nb Nd r Le method guard train rank alpha symbols
//           psk_m psk_phase noise_var" (symbols: 0 or 1; noise_var: "none" or a number) and D lines "Re(y) Im(y) Re(b) Im(b) k"
//   output  per scene "state n_det n_over level", Le lines "tau f P" and n_f n_tau lines of the map
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_par.h"
#include "cfar_core.h"

using namespace admmnet;

static double number(const char *s) { return std::strtod(s, nullptr); }   // reads nan and inf too

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: cfar_model CASES\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r");
    int scenes = 0;
    if (!in || std::fscanf(in, "%d", &scenes) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    char w[13][64];
    for (int s = 0; s < scenes; ++s) {
        if (std::fscanf(in, "%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6],
                        w[7], w[8], w[9], w[10], w[11], w[12]) != 13) {
            std::fprintf(stderr, "bad scene %d\n", s);
            return 2;
        }
        CfarArgs a = {std::atoi(w[0]), std::atoi(w[1]), std::atoi(w[2]), std::atoi(w[3]), std::atoi(w[4]), std::atoi(w[5]),
                      std::atoi(w[6]), std::atoi(w[7]), std::atoi(w[10]), number(w[11]), number(w[8])};
        const bool has_sym = std::atoi(w[9]) != 0, has_noise = std::strcmp(w[12], "none") != 0;
        const double noise = has_noise ? number(w[12]) : 0.0;
        const bool known = a.method == CF_KNOWN;
        const int W = a.guard + a.train;
        if (a.Nb < 1 || a.Nd < 1 || a.r < 1 || a.r > CFAR_MAX_OVERSAMPLE || a.Nb * a.Nd * a.r * a.r > CFAR_MAX_CELLS || a.Le < 1 ||
            a.Le > CRB_MAXL || a.psk_m < 2 || a.psk_m > REFINE_MAX_M || a.method < 0 || a.method > 2 || known != has_noise ||
            (!known && (a.guard < 0 || a.train < 1 || W > CFAR_MAX_REACH || (a.Nb > 1 && 2 * W + 1 > a.Nb) ||
                        (a.Nd > 1 && 2 * W + 1 > a.Nd) || cf_train_count(a.Nb, a.Nd, a.guard, a.train) < 1)) ||
            (a.method == CF_OS && (a.rank < 1 || a.rank > cf_train_count(a.Nb, a.Nd, a.guard, a.train)))) {
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
        std::vector<RfC> x(D), img(nf * a.Nd), tf(nf), tt(nt), pt(REFINE_MAX_M);
        std::vector<double> map(cells), rows(3 * Le), info(CFAR_INFO), map_out(cells);
        std::vector<int> off(known ? 0 : cf_train_count(a.Nb, a.Nd, a.guard, a.train)), chunk(CFAR_THREADS + 1), slot(CRB_MAXL);
        std::vector<uint8_t> flag(cells);
        std::vector<uint16_t> list(cells);
        std::vector<int32_t> counts(CFAR_COUNTS, -1);
        CfarMem m = {x.data(), img.data(), map.data(), tf.data(), tt.data(), pt.data(), off.data(), flag.data(), list.data(),
                     chunk.data(), slot.data()};
        HostPar<CFAR_THREADS> par;
        cfar_scene(par, a, m, y.data(), b.data(), has_sym ? sym.data() : nullptr, has_noise ? &noise : nullptr, rows.data(),
                   counts.data(), info.data(), map_out.data());
        std::printf("%d %d %d %.17g\n", (int)info[1], (int)counts[0], (int)counts[1], info[0]);
        for (int j = 0; j < Le; ++j) std::printf("%.17g %.17g %.17g\n", rows[3 * j], rows[3 * j + 1], rows[3 * j + 2]);
        for (int c = 0; c < cells; ++c) std::printf("%.17g\n", map_out[c]);
    }
    std::fclose(in);
    return 0;
}
