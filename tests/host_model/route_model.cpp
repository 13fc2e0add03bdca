// Host model of csrc/route.h for tests/test_route_host.py (plain g++, no HIP).
//   route_model switches          the Switches parsed from this process's environment, one "field value" per line
//   route_model routes D [D ...]  route_for(D, switches()), one line of "field=value" per D
//   route_model sweep             every D in 1 .. 256 x every on/off combination of the twelve route switches (bit i of the
//                                 combination = switch i of SWEEP_ORDER in the test off its default), as 4096 x 256 packed uint32
#include <stdio.h>

#include <vector>

#include "route.h"

using namespace admmnet;

static const char *const kStorage[] = {"full", "lean", "half"};
static const char *const kFirst[] = {"AR_LDS", "AR_GLOBAL", "AR_FUSED", "dense"};
static const char *const kTridiag[] = {"reg", "lds", "sweep", "panel"};
static const char *const kBack[] = {"in_rebuild", "vgemm", "vgemm_big", "wy_apply", "rotation"};
static const char *const kRebuild[] = {"back_rebuild", "rebuild_big", "rebuild"};
static const char *const kMatFun[] = {"off", "fused", "kernels"};
static const char *const kError[] = {"none", "tiles_skip", "lean_loader", "kernels_fold"};

static uint32_t pack(int D, const Route &r) {   // field widths: see unpack() in the test
    return (uint32_t)(r.eig_dim != D) | r.storage << 1 | r.first << 3 | r.first_rebuild << 5 | r.tridiag << 7 | r.explicit_q << 9 |
           r.dc << 10 | r.back << 11 | r.rebuild << 14 | r.matfun << 16 | r.late_image << 18 | r.fold << 19 | r.buffers << 20 |
           r.error << 25 | (uint32_t)(r.eig_dim == 256) << 27;
}

int main(int argc, char **argv) {
    const char *cmd = argc > 1 ? argv[1] : "";
    const Switches &s = switches();
    if (!strcmp(cmd, "switches")) {
        printf("ADMMNET_SPECTRAL %d\nADMMNET_SPECTRAL_FUSED %d\nADMMNET_SPECTRAL_TOL %.9g\nADMMNET_SPECTRAL_ITERS %d\n", s.spectral,
               s.spectral_fused, s.spectral_tol, s.spectral_iters);
        printf("ADMMNET_SF_FOLD %d\nADMMNET_SF_SMALLWG %d\nADMMNET_SF_TIMING %d\nADMMNET_EIG %d\n", s.sf_fold, s.sf_smallwg,
               s.sf_timing, s.eig_ql);
        printf("ADMMNET_ARROW %d\nADMMNET_ARROW_FUSED %d\nADMMNET_AR_TIMING %d\nADMMNET_LEAN %d\nADMMNET_FUSE_BACK %d\n", s.arrow,
               s.arrow_fused, s.ar_timing, s.lean, s.fuse_back);
        printf("ADMMNET_BR_TIMING %d\nADMMNET_TRIDIAG %d\nADMMNET_TRIDIAG_BIG %d\nADMMNET_BACK %d\nADMMNET_REBUILD %d\n", s.br_timing,
               s.tridiag_lds, s.tridiag_sweep, s.back_q, s.rebuild_tiles);
        printf("ADMMNET_PAD_MIN %d\nADMMNET_STREAMS %d\nADMMNET_TR_OCC %d\nADMMNET_TR_PAD_LDS %d\nADMMNET_PN_SPLIT %d\n",
               s.pad_min_set ? s.pad_min : -1000, s.two_streams, s.tr_occ3, s.tr_pad_lds, s.pn_split);
        printf("ADMMNET_PN_TIMING %d\nADMMNET_DC_OCC %d\nADMMNET_DC_BLOCKS %d\nADMMNET_DC_POISON %d\nADMMNET_DC_TIMING %d\n", s.pn_timing,
               s.dc_occ, s.dc_blocks, s.dc_poison, s.dc_timing);
        return 0;
    }
    if (!strcmp(cmd, "routes")) {
        for (int i = 2; i < argc; ++i) {
            const int D = atoi(argv[i]);
            const Route r = route_for(D, s);
            printf("D=%d eig_dim=%d storage=%s first=%s first_rebuild=%s tridiag=%s explicit_q=%d dc=%d rowmajor=%d colmap=%d back=%s "
                   "back_v=%s rebuild=%s matfun=%s late_image=%d fold=%d buffers=%u error=%s\n",
                   D, r.eig_dim, kStorage[r.storage], kFirst[r.first], kRebuild[r.first_rebuild], kTridiag[r.tridiag], r.explicit_q,
                   r.dc, r.dc && Route::dc_rowmajor(r.back), r.dc && Route::dc_colmap(r.back), kBack[r.back], kBack[r.back_v()],
                   kRebuild[r.rebuild], kMatFun[r.matfun], r.late_image, r.fold, r.buffers, kError[r.error]);
        }
        return 0;
    }
    if (!strcmp(cmd, "sweep")) {
        std::vector<uint32_t> out;
        for (int m = 0; m < 4096; ++m) {
            Switches t = s;   // (the test runs this with no ADMMNET_* variable set: the defaults)
            t.eig_ql = m & 1, t.spectral = !(m & 2), t.spectral_fused = !(m & 4), t.sf_fold = !(m & 8), t.arrow = !(m & 16);
            t.arrow_fused = !(m & 32), t.lean = !(m & 64), t.fuse_back = !(m & 128), t.tridiag_lds = m & 256;
            t.tridiag_sweep = m & 512, t.back_q = m & 1024, t.rebuild_tiles = m & 2048;
            for (int D = 1; D <= 256; ++D) out.push_back(pack(D, route_for(D, t)));
        }
        return fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) == out.size() ? 0 : 1;
    }
    fprintf(stderr, "usage: route_model switches | routes D ... | sweep\n");
    return 2;
}
