// route.h -- the one place that parses the ADMMNET_* switches (Switches: the environment gives the process defaults, an option
// set of options.h overrides them per model) and decides which kernels run for a geometry (Route): api.hip resolves the Switches
// of a call from its cfg, carves and enqueues from the Route, the launchers receive the chosen form and choose nothing.
// Plain C++17 without a HIP include: tests/host_model/route_model.cpp compiles it with g++ (tests/test_route_host.py).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace admmnet {

struct Switches {   // (INTEGRATION.md section 6 is the user-facing table of these)
    // ADMMNET_SPECTRAL=0: every G-layer through the eigensolver pipeline (default: as a matrix function wherever the per-matrix
    // checks allow it, the eigen-pipeline then only runs the matrices it flagged)
    bool spectral;
    bool spectral_fused;   // ADMMNET_SPECTRAL_FUSED=0: the matrix function as five kernels (spectral.hip) instead of sp_fused_kernel
    // ADMMNET_SPECTRAL_TOL: model tolerance of the matrix-function checks.  The quadratic may miss f on the bulk by 1e-6 of the
    // result's scale -- below the eigensolver route's own rounding per layer (~2e-6) and without effect on the distance to the
    // float64 oracle (3e-7, 1e-6 and 3e-6 measured the same: tests/gpu_spectral_check.py); at K = 32 the tighter 3e-7 rejected
    // 3.0 % of the matrix-layers, this one 0.4 %
    float spectral_tol;
    int spectral_iters;    // ADMMNET_SPECTRAL_ITERS: upper bound of the subspace passes (default 5)
    // ADMMNET_SF_FOLD=0: the lazy Z update of the previous layer streamed by prep_kernel (default: it rides the first sweep of the
    // fused kernel, prep then only computes phi and h)
    bool sf_fold;
    // ADMMNET_SF_FOLD=2: the fold as by default, but prep_kernel gathers the diagonals of G and Z from the matrices in every layer
    // (default: from layer 2 on it reads the compact pairs the fused kernel left in G, common.h diag_pairs) -- for A/B runs and tests
    bool prep_gather;
    bool sf_smallwg;       // ADMMNET_SF_SMALLWG=0: never the 4-wave shape of the fused kernel (spectral_waves)
    bool sf_timing;        // ADMMNET_SF_TIMING: developer phase timer of sp_fused_kernel (this and the other *_TIMING: never on by default)
    bool eig_ql;           // ADMMNET_EIG=ql: tridiagonal eigensolver = QL + rotation replay (default: divide & conquer)
    // ADMMNET_ARROW=0: the first G-layer down the dense path like every other (default: Z = 0 gives a plain arrowhead matrix,
    // which arrow.hip solves directly in O(n^2))
    bool arrow;
    bool arrow_fused;      // ADMMNET_ARROW_FUSED=0, D > 128: arrowhead eigenvectors to the global image + rebuild, not the slab form
    // ADMMNET_ARROW_FUSED=2, D > 128: the slab form as ONE kernel (default: a solver kernel at its own occupancy, then the tail
    // kernel, arrow.hip) -- the same bits, for A/B runs and tests
    bool arrow_onekernel;
    bool ar_timing;        // ADMMNET_AR_TIMING: developer phase timer of arrow_rebuild_kernel
    // ADMMNET_LEAN=0: G / Z in full storage + the image written by prep (default: G and Z kept as lower triangles; D <= 128: the
    // tridiagonalisation forms A = C - Z / rho itself, prep only streams the lazy Z update; D > 128: "half image", prep.hip PM_HALF)
    bool lean;
    // ADMMNET_FUSE_BACK=0: separate back-transform and rebuild kernels (default, D <= 128 on D&C: V = Q W inside the rebuild
    // kernel, backrebuild.hip -- the eigen-solve stops at (Q, W) and V never goes through memory)
    bool fuse_back;
    bool br_timing;        // ADMMNET_BR_TIMING: developer phase timer of back_rebuild_kernel
    bool tridiag_lds;      // ADMMNET_TRIDIAG=lds: the LDS-resident tridiagonalisation (tridiag.hip), kept for A/B runs
    bool tridiag_sweep;    // ADMMNET_TRIDIAG_BIG=sweep, D > 128: per-reflector register sweep instead of the panel kernel
    bool back_q;           // ADMMNET_BACK=q: explicit Q (ungtr_big_kernel) + vgemm_big_kernel instead of the block reflectors
    bool rebuild_tiles;    // ADMMNET_REBUILD=tiles: rebuild_kernel also at D = 256 (default there: rebuild_big_kernel)
    // ADMMNET_PAD_MIN: smallest D above 128 that runs in the D = 256 pipeline (Route::eig_dim).  Unset: 129 with the matrix-function
    // route on -- the eigen-pipeline then only sees the matrices it rejects, and the route needs the lower-triangle state of the
    // padded pipeline -- else 176, below which the sweep at the geometry's own size is faster than 256-sized work (measured on
    // MI355X, K = 16, 4096 signals, padded vs sweep per forward: D = 160 306 vs 280 ms, D = 176 312 vs 368 ms, D = 192 319 vs 396 ms)
    bool pad_min_set; int pad_min;
    bool two_streams;      // ADMMNET_STREAMS=2: two chunks in flight on two internal streams (api.hip)
    // ADMMNET_STREAMS=1: everything on the caller's stream (default: the eigensolver fallback of a chunk runs on a side stream
    // beside the next chunk's matrix-function kernel, api.hip)
    bool one_stream;
    bool tr_occ3;          // ADMMNET_TR_OCC=2 clears it: the two-workgroup build of tridiag_reg_kernel<7> for A/B runs
    int tr_pad_lds;        // ADMMNET_TR_PAD_LDS=<bytes> of unused dynamic LDS per tridiag_reg workgroup (developer knob)
    int pn_split;          // ADMMNET_PN_SPLIT: stages of the panel tridiagonalisation -- "0" one (0), "8" two (8), else three (84)
    bool pn_timing;        // ADMMNET_PN_TIMING: developer phase timer of tridiag_panel_kernel
    int dc_occ;            // ADMMNET_DC_OCC: waves per SIMD the D&C kernel is compiled for (0 = its own default; tuning knob)
    bool dc_blocks;        // ADMMNET_DC_BLOCKS=0: the plain D&C variant at n > 129 instead of the block-structured one
    bool dc_poison;        // ADMMNET_DC_POISON: tests -- NaN in every never-written element of the D&C buffers
    bool dc_timing;        // ADMMNET_DC_TIMING: developer phase timer of dc_kernel
};

// the built-in defaults: what every switch is with nothing set anywhere
inline Switches builtin_switches() {
    Switches s;
    s.spectral = s.spectral_fused = s.sf_fold = s.sf_smallwg = s.arrow = s.arrow_fused = s.lean = s.fuse_back = true;
    s.spectral_tol = 1e-6f;
    s.spectral_iters = 5;
    s.sf_timing = s.ar_timing = s.br_timing = s.pn_timing = s.dc_timing = s.dc_poison = false;
    s.eig_ql = s.tridiag_lds = s.tridiag_sweep = s.back_q = s.rebuild_tiles = s.two_streams = s.one_stream = s.prep_gather = s.arrow_onekernel = false;
    s.pad_min_set = false;
    s.pad_min = 0;
    s.tr_occ3 = true;
    s.tr_pad_lds = 0;
    s.pn_split = 84;
    s.dc_occ = 0;
    s.dc_blocks = true;
    return s;
}

// The one parser: `base` with every name that `env` has a value for (env(name) -> its string, or nullptr: keep base's) read in
// the environment's syntax.  The process defaults are the environment over builtin_switches() (switches()), an option set is
// the caller's (name, value) pairs over the process defaults (options.h): the names and spellings of both are these lines.
template <class Lookup>
inline Switches switches_from_env(const Switches &base, const Lookup &env) {
    const auto is = [&](const char *name, const char *word, bool b) { return env(name) ? !strcmp(env(name), word) : b; };
    const auto on = [&](const char *name, bool b) { return env(name) ? atoi(env(name)) != 0 : b; };   // "=0" (anything atoi reads as 0) turns off
    const auto set = [&](const char *name, bool b) { return env(name) != nullptr || b; };             // present, whatever the value
    const auto num = [&](const char *name, int b) { return env(name) ? atoi(env(name)) : b; };
    Switches s = base;
    s.spectral = on("ADMMNET_SPECTRAL", base.spectral);
    s.spectral_fused = on("ADMMNET_SPECTRAL_FUSED", base.spectral_fused);
    s.spectral_tol = env("ADMMNET_SPECTRAL_TOL") ? (float)atof(env("ADMMNET_SPECTRAL_TOL")) : base.spectral_tol;
    s.spectral_iters = num("ADMMNET_SPECTRAL_ITERS", base.spectral_iters);
    s.sf_fold = on("ADMMNET_SF_FOLD", base.sf_fold);
    s.prep_gather = env("ADMMNET_SF_FOLD") ? atoi(env("ADMMNET_SF_FOLD")) == 2 : base.prep_gather;
    s.sf_smallwg = on("ADMMNET_SF_SMALLWG", base.sf_smallwg);
    s.sf_timing = set("ADMMNET_SF_TIMING", base.sf_timing);
    s.eig_ql = is("ADMMNET_EIG", "ql", base.eig_ql);
    s.arrow = on("ADMMNET_ARROW", base.arrow);
    s.arrow_fused = on("ADMMNET_ARROW_FUSED", base.arrow_fused);
    s.arrow_onekernel = env("ADMMNET_ARROW_FUSED") ? atoi(env("ADMMNET_ARROW_FUSED")) == 2 : base.arrow_onekernel;
    s.ar_timing = set("ADMMNET_AR_TIMING", base.ar_timing);
    s.lean = on("ADMMNET_LEAN", base.lean);
    s.fuse_back = on("ADMMNET_FUSE_BACK", base.fuse_back);
    s.br_timing = set("ADMMNET_BR_TIMING", base.br_timing);
    s.tridiag_lds = is("ADMMNET_TRIDIAG", "lds", base.tridiag_lds);
    s.tridiag_sweep = is("ADMMNET_TRIDIAG_BIG", "sweep", base.tridiag_sweep);
    s.back_q = is("ADMMNET_BACK", "q", base.back_q);
    s.rebuild_tiles = is("ADMMNET_REBUILD", "tiles", base.rebuild_tiles);
    s.pad_min_set = set("ADMMNET_PAD_MIN", base.pad_min_set);
    s.pad_min = num("ADMMNET_PAD_MIN", base.pad_min);
    s.two_streams = env("ADMMNET_STREAMS") ? atoi(env("ADMMNET_STREAMS")) == 2 : base.two_streams;
    s.one_stream = env("ADMMNET_STREAMS") ? atoi(env("ADMMNET_STREAMS")) == 1 : base.one_stream;
    s.tr_occ3 = env("ADMMNET_TR_OCC") ? atoi(env("ADMMNET_TR_OCC")) != 2 : base.tr_occ3;
    s.tr_pad_lds = num("ADMMNET_TR_PAD_LDS", base.tr_pad_lds);
    s.pn_split = !env("ADMMNET_PN_SPLIT") ? base.pn_split : is("ADMMNET_PN_SPLIT", "0", false) ? 0 : is("ADMMNET_PN_SPLIT", "8", false) ? 8 : 84;
    s.pn_timing = set("ADMMNET_PN_TIMING", base.pn_timing);
    s.dc_occ = num("ADMMNET_DC_OCC", base.dc_occ);
    s.dc_blocks = !is("ADMMNET_DC_BLOCKS", "0", !base.dc_blocks);
    s.dc_poison = set("ADMMNET_DC_POISON", base.dc_poison);
    s.dc_timing = set("ADMMNET_DC_TIMING", base.dc_timing);
    return s;
}

// The process defaults: the environment over the built-in values, read once per process (the
// child-process tests rely on it).  The only reader of the environment in csrc/, and referenced only where the option handle 0
// is resolved (options.h): everything else receives the Switches of its call.
inline const Switches &switches() {
    static const Switches s = switches_from_env(builtin_switches(), [](const char *name) -> const char * { return getenv(name); });
    return s;
}

// ---- the route of a geometry --------------------------------------------------------------------------------------------------
enum Storage { ST_FULL, ST_LEAN, ST_HALF };   // G / Z: full | lower triangles, A from the tridiagonalisation's loader | lower triangles + half image
enum ArMode { AR_LDS = 0, AR_GLOBAL = 1, AR_FUSED = 2, AR_NONE = 3 };   // first layer's arrowhead eigenvectors: LDS image, global image (+ rebuild), slabs; dense path
enum Tridiag { TD_REG, TD_LDS, TD_SWEEP, TD_PANEL };   // tridiag_reg.hip | tridiag.hip | tridiag_big.hip | tridiag_panel.hip
enum Back { BK_IN_REBUILD, BK_VGEMM, BK_VGEMM_BIG, BK_WY, BK_ROTATION };   // V = Q W: backrebuild.hip | dc.hip | vgemm_big.hip | wy_apply.hip | rotapply.hip
enum Rebuild { RB_BACK, RB_BIG, RB_TILES };            // backrebuild.hip | rebuild_big.hip | rebuild.hip
enum MatFun { MF_OFF, MF_FUSED, MF_KERNELS };          // the G-layer as a matrix function: not at this D | spectral_fused.hip | spectral.hip
enum Buffer { BUF_WDC = 1, BUF_LOG = 2, BUF_PANEL = 4 /* Tfac, Tail, Wmap */, BUF_SPEC_MAT = 8 /* spec_mat, spec_vec, spec_val */, BUF_SPEC_FLAG = 16 };
// combinations a kernel cannot serve: the API entry point refuses them (ADMMNET_E_ARG) before it enqueues anything
enum RouteError { RE_NONE, RE_TILES_SKIP, RE_LEAN_LOADER, RE_KERNELS_FOLD };

struct Route {
    // Dimension the eigen-pipeline works in, and every chunk buffer is laid out for.  128 < D < 256 from pad_min up ("padded route"):
    // the layer matrix is embedded in the D = 256 pipeline as A' = diag(A, 0) -- arrow-first order puts the padding behind the last
    // row of the D x D block.  The reflectors of A have exact zeros in the padded rows, the padded columns reduce to identity
    // reflectors (tau = 0), so T' = diag(T, 0) exactly; the padded poles deflate (z = 0) with unit eigenvectors, the block
    // reflectors leave those alone, and G' = V' f(L') V'^H = diag(G, f(0) I): the rebuild stores the leading block.  Costs the
    // D = 256 flops whatever D is, still several times faster than the per-reflector sweep it replaces; any switch that leaves
    // the panel / D&C / block-reflector route also leaves the padding.
    int D, eig_dim;
    Storage storage;
    ArMode first;            // the first G-layer (Z = 0); AR_GLOBAL is followed by first_rebuild
    Rebuild first_rebuild;
    Tridiag tridiag;
    bool explicit_q;         // Q is formed (false: the back-transform applies the panel kernel's block reflectors itself)
    bool dc;                 // tridiagonal solver: divide & conquer, else QL with its rotation log
    Back back;               // for the G-layer; back_v() where the caller wants V itself (admmnet_eigh_c64)
    Rebuild rebuild;
    MatFun matfun;           // when on, the eigen-pipeline kernels carry the per-matrix skip filter
    bool late_image;         // D > 128: prep writes no image, launch_half_image builds it for the flagged matrices only
    bool fold;               // layers k >= 1: the lazy Z update rides the fused kernel's first sweep, prep computes phi and h only
    unsigned buffers;        // Buffer bits: what carve_chunk lays out besides the buffers every route has
    RouteError error;

    bool lean() const { return storage != ST_FULL; }
    Back back_v() const { return back == BK_IN_REBUILD ? BK_VGEMM : back; }
    static bool dc_rowmajor(Back b) { return b == BK_VGEMM; }   // (the fused consumer and the large back-transforms read the transposed image)
    static bool dc_colmap(Back b) { return b == BK_WY; }        // (the block reflectors read W through the top-level merge's column map)
};

inline Route route_for(int D, const Switches &s) {
    Route r;
    r.D = D;
    const bool big = D > 128;
    // block reflectors need the T factors of the panel kernel and the D&C column map: every switch that takes the tridiagonalisation
    // or the tridiagonal solver off that route turns them off
    const bool wy = !s.back_q && !s.tridiag_sweep && !s.tridiag_lds && !s.eig_ql;
    const int pad_min = s.pad_min_set ? s.pad_min : (s.spectral ? 129 : 176);
    r.eig_dim = (big && D >= pad_min && D < 256 && wy) ? 256 : D;
    const int E = r.eig_dim;
    r.dc = !s.eig_ql;
    r.tridiag = s.tridiag_lds ? TD_LDS : E <= 128 ? TD_REG : (E == 256 && !s.tridiag_sweep) ? TD_PANEL : TD_SWEEP;
    r.explicit_q = !(r.tridiag == TD_PANEL && wy);
    // lean needs the arrowhead first layer and a tridiagonalisation that reads the lower triangle: tridiag_reg's own loader, or the
    // tiles tridiag_panel_kernel loads
    const bool lean = s.lean && s.arrow && (big ? r.dc && r.tridiag == TD_PANEL : r.tridiag == TD_REG);
    r.storage = !lean ? ST_FULL : big ? ST_HALF : ST_LEAN;
    r.first = !s.arrow ? AR_NONE : !big ? AR_LDS : s.arrow_fused ? AR_FUSED : AR_GLOBAL;
    r.first_rebuild = (D == 256 && !s.rebuild_tiles) ? RB_BIG : RB_TILES;   // (AR_GLOBAL lays the image out for D itself)
    const bool fused = s.fuse_back && r.dc && !big;
    r.back = fused ? BK_IN_REBUILD : !r.dc ? BK_ROTATION : !r.explicit_q ? BK_WY : E > 128 ? BK_VGEMM_BIG : BK_VGEMM;
    r.rebuild = fused ? RB_BACK : (E == 256 && (!s.rebuild_tiles || E != D)) ? RB_BIG : RB_TILES;
    // G as a matrix function where the spectrum allows it (checked per matrix), from the lower-triangle state
    const bool spec = s.spectral && lean && D >= 8 && (big || fused);
    r.matfun = !spec ? MF_OFF : s.spectral_fused ? MF_FUSED : MF_KERNELS;
    r.late_image = r.matfun == MF_FUSED && big;
    r.fold = r.matfun == MF_FUSED && s.sf_fold;
    // (the matrix-function buffers follow the switch, not the geometry: one workspace layout per environment)
    r.buffers = (r.dc ? BUF_WDC : BUF_LOG) | (r.dc && E == 256 ? BUF_PANEL : 0) | (s.spectral ? BUF_SPEC_FLAG : 0) |
                (s.spectral && !s.spectral_fused ? BUF_SPEC_MAT : 0);
    r.error = (r.matfun != MF_OFF && r.rebuild == RB_TILES) ? RE_TILES_SKIP
              : (r.storage == ST_LEAN && r.tridiag != TD_REG) || (r.storage == ST_HALF && r.tridiag != TD_PANEL) ? RE_LEAN_LOADER
              : (r.fold && r.matfun != MF_FUSED) ? RE_KERNELS_FOLD : RE_NONE;
    return r;
}

inline constexpr const char *kRouteErrorText[] = {   // by RouteError
    "", "rebuild: the per-tile kernel has no per-matrix filter (ADMMNET_SPECTRAL=1 with ADMMNET_REBUILD=tiles)",
    "tridiag: the lean loader exists for the register-resident kernel only (D <= 128)",
    "spectral: the multi-kernel form does not apply the Z update"};

// The workgroup shape of the fused matrix-function kernel (4 or 12 waves per matrix), chosen once per CALL from the call's batch
// size B -- never from a chunk's size: the two shapes sum in different orders, and the bits of a signal must not depend on
// cfg.chunk.  256 threads per matrix, three matrices per CU, once there are more than two matrices per CU to overlap (measured at
// 10 x 10, K = 10: 1024 signals 3.45 vs 3.63 ms per forward, 4096 signals 8.3 vs 10.4 ms; but 256 signals 2.42 vs 2.03 ms and a
// single signal 0.64 vs 0.53 ms: a lone matrix is served faster by twelve waves).
inline int spectral_waves(int D, int64_t B, const Switches &s) { return (D <= 128 && s.sf_smallwg && B > 512) ? 4 : 12; }

}  // namespace admmnet
