// api.hip -- the extern "C" boundary declared in include/admmnet.h: host-side
// weight packing, workspace carving and the per-layer launch sequence.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "common.h"
#include "options.h"
#include "score_core.h"
#include "set_core.h"
#include "crb_core.h"
#include "refine_core.h"
#include "cfar_core.h"
#include "relax_core.h"

namespace admmnet {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- profiler -------------------------------------------------------------------
// Event pairs live in a pool that grows with the number of scopes recorded since the last read (the bench records
// ~600 scopes per cfg3 step; an earlier fixed pool of 8192 silently dropped everything after step 13).  A scope is
// only ever dropped when an event cannot be created; drops are counted and reported by admmnet_profile_dropped().
struct ProfState {
    std::mutex mu;
    bool on = false;
    std::vector<hipEvent_t> ev0, ev1;   // created events (reused across reads)
    std::vector<int> kclass;            // class of the scopes recorded since the last read
    int64_t dropped = 0;
};
static ProfState &prof() {
    static ProfState p;
    return p;
}
static const size_t kProfHardCap = (size_t)1 << 22;   // 4 M scopes between two reads: a runaway guard, not a budget

ProfScope::ProfScope(int kclass, hipStream_t s) : slot(-1), st(s) {
    ProfState &p = prof();
    if (!p.on) return;
    std::lock_guard<std::mutex> lk(p.mu);
    const size_t i = p.kclass.size();
    if (i >= p.ev0.size()) {
        hipEvent_t a, b;
        if (i >= kProfHardCap || hipEventCreate(&a) != hipSuccess) {
            ++p.dropped;
            return;
        }
        if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);
            ++p.dropped;
            return;
        }
        p.ev0.push_back(a);
        p.ev1.push_back(b);
    }
    p.kclass.push_back(kclass);
    slot = (int)i;
    (void)hipEventRecord(p.ev0[i], st);
}
ProfScope::~ProfScope() {
    if (slot < 0) return;
    ProfState &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    (void)hipEventRecord(p.ev1[slot], st);
}

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

static int check_cfg(const admmnet_cfg *cfg) {
    if (!cfg) {
        set_error("cfg is NULL");
        return ADMMNET_E_ARG;
    }
    const int64_t D = (int64_t)cfg->M * cfg->N;
    if (cfg->M < 1 || cfg->N < 1 || D < 1 || D > kMaxD) {
        set_error("unsupported geometry M=%d N=%d (need 1 <= M*N <= %d)", cfg->M, cfg->N, kMaxD);
        return ADMMNET_E_ARG;
    }
    if (cfg->K < 1 || cfg->K > 1024) {
        set_error("unsupported num_layers K=%d", cfg->K);
        return ADMMNET_E_ARG;
    }
    if (cfg->has_head && (cfg->L < 1 || cfg->L > 16)) {
        set_error("unsupported L=%d", cfg->L);
        return ADMMNET_E_ARG;
    }
    if (cfg->sub_batch < 0) {
        set_error("sub_batch=%d (need 0 = one batch, or >= 1 signals per sub-batch)", cfg->sub_batch);
        return ADMMNET_E_ARG;
    }
    if (!options_resolve(cfg->reserved[0])) {
        set_error("cfg.reserved[0] = %d is not an option handle admmnet_options_intern has issued (0 = the process defaults)",
                  cfg->reserved[0]);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

// The Switches of a call: the option set its cfg names (options.h; handle 0 = the process defaults).  Behind check_cfg.
static const Switches &cfg_switches(const admmnet_cfg *cfg) { return *options_resolve(cfg->reserved[0]); }

// Sub-batches (cfg->sub_batch = g > 0): the signals [j g, min((j + 1) g, B)) form group j, which takes its own batch mean.
// group_size() is g capped at B (g >= B is one group); without sub-batches the whole call is one group of B.
static int64_t group_size(const admmnet_cfg *cfg, int64_t B) {
    return (cfg->sub_batch > 0 && cfg->sub_batch < B) ? cfg->sub_batch : B;
}
static int64_t group_count(const admmnet_cfg *cfg, int64_t B) {
    const int64_t g = group_size(cfg, B);
    return g > 0 ? (B + g - 1) / g : 1;
}

static int64_t pick_chunk(const admmnet_cfg *cfg, int64_t B) {
    int64_t c = cfg->chunk > 0 ? cfg->chunk : 8192;
    if (c > B) c = B;
    if (c < 1) c = 1;
    return c;
}

// carve helper
struct Carver {
    char *base;
    int64_t off = 0;
    template <class T>
    T *take(int64_t count) {
        T *p = reinterpret_cast<T *>(base + off);
        off = align_up(off + (int64_t)sizeof(T) * count, 256);
        return p;
    }
};

// lays out exactly r.buffers behind the buffers every route has, all for r.eig_dim
static void carve_chunk(Carver &c, const Route &r, int64_t chunk, Ws *ws) {
    const int D = r.eig_dim;
    const int64_t n = D + 1, na = r.D + 1;
    ws->chunk = chunk;
    ws->cap = ((int64_t)kLogCapMul * n * n + 64 * n + 64 + 7) & ~(int64_t)7;   // whole 64-byte groups
    ws->Mbuf = c.take<float2>(chunk * ((int64_t)D * D + D + 1));
    ws->QV = c.take<float>(chunk * n * 2 * D);
    const int64_t groups = (chunk + 63) / 64;
    ws->dT = c.take<float>(groups * n * 64);
    ws->eT = c.take<float>(groups * n * 64);
    ws->w = c.take<float>(chunk * n);
    ws->w0 = c.take<float>(chunk * n);
    ws->logn = c.take<int>(chunk * 2);
    const auto has = [&](Buffer b) { return (r.buffers & b) != 0; };
    ws->Wdc = has(BUF_WDC) ? c.take<float>(chunk * 3 * n * n) : nullptr;
    ws->VT = has(BUF_WDC) ? c.take<float>(chunk * n * 2 * D) : ws->QV;   // (the rotation replay works in place)
    ws->Tfac = has(BUF_PANEL) ? c.take<float2>(chunk * 17 * 256) : nullptr;
    ws->Tail = has(BUF_PANEL) ? c.take<float2>(chunk * tridiag_panel_tail_elems()) : nullptr;
    ws->Wmap = has(BUF_PANEL) ? c.take<int2>(chunk * n) : nullptr;
    ws->log = has(BUF_LOG) ? c.take<LogRec>(chunk * ws->cap) : nullptr;
    // (in the layer's own dimension: the fast path never sees the padded image; the multi-kernel form keeps A / E and E^2 in memory)
    ws->spec_mat = has(BUF_SPEC_MAT) ? c.take<float2>(2 * chunk * na * na) : nullptr;
    ws->spec_vec = has(BUF_SPEC_MAT) ? c.take<float2>(chunk * 2 * na) : nullptr;
    ws->spec_val = has(BUF_SPEC_MAT) ? c.take<double>(chunk * 8) : nullptr;
    ws->spec_flag = has(BUF_SPEC_FLAG) ? c.take<int>(chunk) : nullptr;
    ws->skip = nullptr;
}

// Two chunks in flight (ADMMNET_STREAMS=2): the per-chunk kernel sequence prep -> tridiagonalisation -> D&C -> back-transform ->
// rebuild of consecutive chunks alternates between two internal streams and two sets of chunk buffers, so that the
// vector-ALU-bound kernels of one chunk and the matrix-core-bound kernels of the other can share the CUs wherever their
// registers and LDS admit both.  Only for batches of at least two chunks; the state (G, Z, phi, h, rn) is shared -- the
// chunks touch disjoint slices of it.
struct ChunkStreams {   // per device, created on first use (non-blocking streams: they order against the caller's by events)
    std::mutex mu;
    hipStream_t s[2] = {nullptr, nullptr};
    int dev = -1;
};
static int chunk_streams(hipStream_t out[2]) {
    static ChunkStreams cs[16];
    int dev = 0;
    ADMM_HIP(hipGetDevice(&dev));
    ChunkStreams &c = cs[dev & 15];
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.s[0] == nullptr || c.dev != dev) {
        ADMM_HIP(hipStreamCreateWithFlags(&c.s[0], hipStreamNonBlocking));
        ADMM_HIP(hipStreamCreateWithFlags(&c.s[1], hipStreamNonBlocking));
        c.dev = dev;
    }
    out[0] = c.s[0];
    out[1] = c.s[1];
    return ADMMNET_OK;
}

// The eigensolver fallback beside the next chunk (default; ADMMNET_STREAMS=1 turns it off): behind the matrix-function kernel of a
// chunk the eigen-pipeline only runs the few matrices that kernel flagged -- one workgroup per flagged matrix in eight dependent
// kernels, each with a tail of its own, during which most of the chip idles.  It depends on its own chunk alone (reads the
// chunk's flags, Z, phi and h, writes the flagged matrices' G and rn), so admmnet_layer_front enqueues it on a side stream while
// the caller's stream goes on with prep_kernel and sp_fused_kernel of the next chunk.  One side stream per device (non-blocking,
// the higher of the device's priorities: the handful of fallback workgroups are placed as CUs come free), created on first
// use; the events that order it against the caller's stream come from a per-device pool.  A call leases three events
// (one fork, two alternating "fallback done") for its duration; concurrent calls share the stream, never an event.
struct SideStream {
    std::mutex mu;
    hipStream_t s = nullptr;
    int dev = -1;
    std::vector<hipEvent_t> idle;   // created events no call holds
};
struct SideLease {
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // [0], [1]: fallback of an even / odd chunk done; [2]: fork and join
    SideStream *from = nullptr;
};
static void side_release(SideLease *l) {
    if (!l->from) return;
    std::lock_guard<std::mutex> lk(l->from->mu);
    for (hipEvent_t &e : l->ev)
        if (e) l->from->idle.push_back(e), e = nullptr;
    l->from = nullptr;
}
static int side_acquire(SideLease *l) {
    static SideStream ss[16];
    int dev = 0;
    ADMM_HIP(hipGetDevice(&dev));
    SideStream &c = ss[dev & 15];
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.s == nullptr || c.dev != dev) {
        int least = 0, greatest = 0;
        ADMM_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        hipStream_t s;
        ADMM_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
        c.s = s;
        c.dev = dev;
        c.idle.clear();   // (events of another device: never reused here)
    }
    hipEvent_t got[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        if (!c.idle.empty()) {
            got[i] = c.idle.back();
            c.idle.pop_back();
            continue;
        }
        const hipError_t e = hipEventCreateWithFlags(&got[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            for (int j = 0; j < i; ++j) c.idle.push_back(got[j]);
            set_error("hipEventCreateWithFlags failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
            return ADMMNET_E_HIP;
        }
    }
    l->s = c.s;
    for (int i = 0; i < 3; ++i) l->ev[i] = got[i];
    l->from = &c;
    return ADMMNET_OK;
}
// the caller's stream continues behind everything the side stream holds
static int side_join(const SideLease &l, hipStream_t st) {
    ADMM_HIP(hipEventRecord(l.ev[2], l.s));
    ADMM_HIP(hipStreamWaitEvent(st, l.ev[2], 0));
    return ADMMNET_OK;
}

static int carve_workspace(const admmnet_cfg *cfg, int64_t B, void *base, int64_t bytes, Ws *ws, bool state) {
    const int D = cfg->M * cfg->N;
    const int64_t n = D + 1;
    Carver c{reinterpret_cast<char *>(base)};
    memset(ws, 0, sizeof(*ws));
    const Switches &sw = cfg_switches(cfg);
    const Route r = route_for(D, sw);
    if (state) {
        ws->G = c.take<float2>(B * n * n);
        ws->Z = c.take<float2>(B * n * n);
        for (int i = 0; i < 2; ++i) ws->phi[i] = c.take<float2>(B * D);
        for (int i = 0; i < 2; ++i) ws->h[i] = c.take<float>(B * D);
        ws->alpha = c.take<float>(B);
        ws->rn = c.take<float>(B);
        const int64_t ng = group_count(cfg, B);   // (1 without sub-batches: the layout of a plain call)
        ws->sum = c.take<double>(2 * ng);
        ws->mean = c.take<float>(ng > 4 ? ng : 4);
        ws->headkv = c.take<float>((int64_t)2 * D * 128);
        // The compact diagonals (common.h), behind everything admmnet_state_layout reports.  Written by the fused matrix-function
        // kernel of a layer k >= 1 whose update is folded, read by prep_kernel of layer k + 1 <= K - 2 (the last layer forms
        // phi alone): a model of fewer than four layers has no reader and no buffers.
        if (r.fold && cfg->K >= 4) {
            ws->diag = c.take<float>(B * 2 * D);
            ws->diag_ok = c.take<int>(B);
        }
    }
    carve_chunk(c, r, pick_chunk(cfg, B), ws);
    ws->set2_offset = 0;
    if (state && sw.two_streams && B > ws->chunk) {   // room for a second chunk in flight: a second set, same layout
        ws->set2_offset = c.off;
        Ws tmp;
        carve_chunk(c, r, ws->chunk, &tmp);
    }
    ws->total_bytes = c.off;
    if (base && bytes < c.off) {
        set_error("workspace too small: %lld < %lld bytes", (long long)bytes, (long long)c.off);
        return ADMMNET_E_WORKSPACE;
    }
    return ADMMNET_OK;
}

// What the G-layer of a chunk reads and writes (Zlow: the lower-triangle Z of ST_LEAN storage, for the tridiagonalisation's loader)
struct GLayerIO {
    const float *lw = nullptr;
    const float2 *phi = nullptr;
    const float *h = nullptr;
    const float2 *Zlow = nullptr;
    float2 *G = nullptr;
    float *rn = nullptr, *w_out = nullptr;
    bool lower_only = false;
};

// The eigen-pipeline of a chunk whose image is built (ws.skip: its per-matrix filter), then the rebuild of G.  io == nullptr:
// eigenvalues and the explicit eigenvector image only (admmnet_eigh_c64).
static int eig_chunk(const Route &r, const Switches &sw, int64_t nb, const Ws &ws, int32_t *status, hipStream_t st,
                     const GLayerIO *io) {
    const int D = r.D, E = r.eig_dim;   // (the image, T, W and the eigenvector image are all of dimension E)
    const Back back = io ? r.back : r.back_v();
    const GLayerIO g = io ? *io : GLayerIO{};
    int rc;
    if ((rc = launch_tridiag(r, sw, nb, ws, st, g.Zlow, g.phi, g.h, g.lw))) return rc;
    if (r.dc) rc = launch_dc(sw, E + 1, nb, ws, status, st, Route::dc_rowmajor(back), Route::dc_colmap(back));
    else rc = launch_tql(E + 1, nb, ws, status, st);
    if (rc) return rc;
    switch (back) {
        case BK_IN_REBUILD: break;
        case BK_VGEMM: rc = launch_vgemm(E, nb, ws, st); break;            // V = Q W on the matrix cores
        case BK_VGEMM_BIG: rc = launch_vgemm_big(E, nb, ws, st); break;
        case BK_WY: rc = launch_wy_apply(E, nb, ws, st); break;            // block reflectors applied to W: no explicit Q
        case BK_ROTATION: rc = launch_rotapply(E, nb, ws, st); break;
    }
    if (rc || !io) return rc;
    if (r.rebuild == RB_BACK) return launch_back_rebuild(sw, D, nb, g.lw, g.phi, g.h, g.G, g.rn, g.w_out, ws, st, g.lower_only);
    return launch_rebuild(D, nb, g.lw, g.phi, g.h, g.G, g.rn, g.w_out, ws, st, g.lower_only, r.rebuild, E);
}

}  // namespace admmnet

using namespace admmnet;

extern "C" {

int admmnet_abi_version(void) { return ADMMNET_ABI_VERSION; }
const char *admmnet_last_error(void) { return g_err; }

int32_t admmnet_options_intern(const char *const *names, const char *const *values, int32_t count) {
    char err[sizeof(g_err)];
    const int32_t h = options_intern(names, values, count, err, sizeof(err));
    if (h >= 0) return h;
    set_error("%s", err);
    return ADMMNET_E_ARG;
}

int64_t admmnet_options_describe(int32_t handle, char *buf, int64_t len) {
    const Switches *sw = options_resolve(handle);
    if (!sw || !buf || len < 1) {
        set_error("options_describe: %s (handle %d)", sw ? "no buffer" : "not an option handle admmnet_options_intern has issued", handle);
        return ADMMNET_E_ARG;
    }
    return options_describe(*sw, buf, (size_t)len);
}

int64_t admmnet_raw_weight_count(const admmnet_cfg *cfg) {
    if (check_cfg(cfg)) return -1;
    const int64_t D = (int64_t)cfg->M * cfg->N;
    const int64_t per_layer = 1 + 2 + 64 * D + 64 + D * 64 + D + 3 + 49 + 2 + 161;
    int64_t total = per_layer * cfg->K;
    if (cfg->has_head) {
        const int64_t L = cfg->L;
        total += 2 * D + 128 * 2 * D + 128 + 128 * 128 + 128 + 256 + 128 + 384 * 128 + 384 + 128 * 128 + 128 +
                 64 * 128 + 64 + 32 * 64 + 32 + 16 * 32 + 16 + L * 2 * (32 * 16 + 32 + 32 + 1) +
                 16 * 16 + 16 + 16 + 1;
    }
    return total;
}

int64_t admmnet_layer_weight_offset(const admmnet_cfg *cfg, int32_t k) {
    if (check_cfg(cfg)) return -1;
    const LayerLayout L{cfg->M * cfg->N};
    return (int64_t)k * L.size();
}

int64_t admmnet_packed_weight_count(const admmnet_cfg *cfg) {
    if (check_cfg(cfg)) return -1;
    const int D = cfg->M * cfg->N;
    const LayerLayout L{D};
    int64_t total = (int64_t)cfg->K * L.size();
    if (cfg->has_head) total += HeadLayout{D, cfg->L}.size();
    return total;
}

// transpose src[rows][cols] -> dst[cols][rows]
static void tr(const float *src, int rows, int cols, float *dst) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
}

int admmnet_pack_weights(const admmnet_cfg *cfg, const float *raw, float *out) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!raw || !out) {
        set_error("pack_weights: NULL buffer");
        return ADMMNET_E_ARG;
    }
    const int D = cfg->M * cfg->N;
    const LayerLayout L{D};
    memset(out, 0, sizeof(float) * (size_t)admmnet_packed_weight_count(cfg));
    const float *p = raw;
    for (int k = 0; k < cfg->K; ++k) {
        float *o = out + (size_t)k * L.size();
        const float rho_phi = *p++;
        const float rho_h = *p++, pw = *p++;
        const float *w1 = p; p += 64 * D;
        const float *b1 = p; p += 64;
        const float *w2 = p; p += D * 64;
        const float *b2 = p; p += D;
        const float lam_g = *p++, rho_g = *p++, thr = *p++;
        const float *vn = p; p += 49;
        const float rho_z = *p++, lam_z = *p++;
        const float *rs = p; p += 161;
        // fp32 arithmetic, mirroring the reference tensors (admm_net.py:97,148,188,269-271,287-288,321,406,424-426,457)
        o[S_RHO_PHI] = softplus_f(rho_phi);
        o[S_RHO_H_EPS] = softplus_f(rho_h) + kEpsRef;
        o[S_SIG_PW] = sigmoid_f(pw);
        {
            const float lv = softplus_f(lam_g);
            o[S_CORNER_G] = 1.0f / (lv * lv + kEpsRef);
        }
        o[S_INV_RHO_G] = 1.0f / (softplus_f(rho_g) + kEpsRef);
        o[S_THR] = sigmoid_f(thr);
        o[S_RHO_Z] = softplus_f(rho_z);
        {
            const float lv = softplus_f(lam_z);
            o[S_CORNER_Z] = 1.0f / (lv * lv + kEpsRef);
        }
        o[S_KNORM] = (float)((double)k / 10.0);
        o[S_A_COEF] = 2.0f * sqrtf((float)D);
        tr(w1, 64, D, o + L.off_w1t());           // [64][D] -> [D][64]
        memcpy(o + L.off_b1(), b1, sizeof(float) * 64);
        tr(w2, D, 64, o + L.off_w2t());           // [D][64] -> [64][D]
        memcpy(o + L.off_b2(), b2, sizeof(float) * D);
        memcpy(o + L.off_vn(), vn, sizeof(float) * 49);
        memcpy(o + L.off_rs(), rs, sizeof(float) * 161);
    }
    if (cfg->has_head) {
        const HeadLayout H{D, cfg->L};
        float *o = out + (size_t)cfg->K * L.size();
        memcpy(o + H.off_pos(), p, sizeof(float) * 2 * D); p += 2 * D;
        tr(p, 128, 2 * D, o + H.off_fe0w()); p += 128 * 2 * D;
        memcpy(o + H.off_fe0b(), p, sizeof(float) * 128); p += 128;
        tr(p, 128, 128, o + H.off_fe2w()); p += 128 * 128;
        memcpy(o + H.off_fe2b(), p, sizeof(float) * 128); p += 128;
        memcpy(o + H.off_ppw(), p, sizeof(float) * 256); p += 256;
        memcpy(o + H.off_ppb(), p, sizeof(float) * 128); p += 128;
        tr(p, 384, 128, o + H.off_inw()); p += 384 * 128;
        memcpy(o + H.off_inb(), p, sizeof(float) * 384); p += 384;
        tr(p, 128, 128, o + H.off_outw()); p += 128 * 128;
        memcpy(o + H.off_outb(), p, sizeof(float) * 128); p += 128;
        tr(p, 64, 128, o + H.off_pe0w()); p += 64 * 128;
        memcpy(o + H.off_pe0b(), p, sizeof(float) * 64); p += 64;
        tr(p, 32, 64, o + H.off_pe2w()); p += 32 * 64;
        memcpy(o + H.off_pe2b(), p, sizeof(float) * 32); p += 32;
        tr(p, 16, 32, o + H.off_pe4w()); p += 16 * 32;
        memcpy(o + H.off_pe4b(), p, sizeof(float) * 16); p += 16;
        for (int t = 0; t < cfg->L; ++t) {
            float *r = o + H.off_reg(t);
            for (int q = 0; q < 2; ++q) {      // tau then f
                tr(p, 32, 16, r); p += 32 * 16;                     // [32][16] -> [16][32]
                memcpy(r + 512, p, sizeof(float) * 32); p += 32;    // b1
                memcpy(r + 544, p, sizeof(float) * 32); p += 32;    // w2
                r[576] = *p++;                                      // b2
                r += 577;
            }
        }
        float *c = o + H.off_conf();
        tr(p, 16, 16, c); p += 256;
        memcpy(c + 256, p, sizeof(float) * 16); p += 16;
        memcpy(c + 272, p, sizeof(float) * 16); p += 16;
        c[288] = *p++;
    }
    if (p - raw != admmnet_raw_weight_count(cfg)) {
        set_error("pack_weights: internal count mismatch %lld vs %lld", (long long)(p - raw),
                  (long long)admmnet_raw_weight_count(cfg));
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_workspace_bytes(const admmnet_cfg *cfg, int64_t B) {
    if (check_cfg(cfg) || B < 1) return -1;
    Ws ws;
    carve_workspace(cfg, B, nullptr, 0, &ws, true);
    return ws.total_bytes;
}

int admmnet_state_layout(const admmnet_cfg *cfg, int64_t B, int64_t offsets[ADMMNET_STATE_SPANS + 1], int32_t *lower_only) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (B < 1 || !offsets) {
        set_error("state_layout: bad B or offsets");
        return ADMMNET_E_ARG;
    }
    Ws ws;
    carve_workspace(cfg, B, nullptr, 0, &ws, true);   // null base: every pointer is its offset
    const void *spans[ADMMNET_STATE_SPANS + 1] = {ws.G, ws.Z, ws.phi[0], ws.phi[1], ws.h[0], ws.h[1], ws.alpha, ws.rn, ws.sum};
    for (int i = 0; i <= ADMMNET_STATE_SPANS; ++i) offsets[i] = (int64_t)reinterpret_cast<intptr_t>(spans[i]);
    if (lower_only) *lower_only = route_for(cfg->M * cfg->N, cfg_switches(cfg)).lean() ? 1 : 0;
    return ADMMNET_OK;
}

int admmnet_begin(const admmnet_cfg *cfg, int64_t B, void *workspace, int64_t workspace_bytes,
                  int32_t *status, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (B < 1 || !workspace) {
        set_error("begin: bad B or workspace");
        return ADMMNET_E_ARG;
    }
    // a combination no kernel serves is refused here, before the forward enqueues anything (admmnet_layer_front refuses it too):
    // the dense G-layers are k = 1 .. K - 2, and k = 0 where the arrowhead solver is off
    const Route r = route_for(cfg->M * cfg->N, cfg_switches(cfg));
    if (r.error != RE_NONE && (cfg->K >= 3 || (cfg->K == 2 && r.first == AR_NONE))) {
        set_error("%s", kRouteErrorText[r.error]);
        return ADMMNET_E_ARG;
    }
    Ws ws;
    if ((rc = carve_workspace(cfg, B, workspace, workspace_bytes, &ws, true))) return rc;
    if (status) ADMM_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), (hipStream_t)stream));
    // (no row of the compact diagonals describes the state this forward starts from, whatever the workspace held before)
    if (ws.diag_ok) ADMM_HIP(hipMemsetAsync(ws.diag_ok, 0, sizeof(int) * (size_t)B, (hipStream_t)stream));
    return ADMMNET_OK;
}

int admmnet_layer_front(const admmnet_cfg *cfg, const float *W, int32_t k, const void *y, const void *b,
                        const float *sigma, int64_t B, void *workspace, double *sum_out, int32_t *status,
                        void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (k < 0 || k >= cfg->K || B < 1 || !W || !y || !b || !sigma || !workspace) {
        set_error("layer_front: bad argument");
        return ADMMNET_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    Ws ws;
    carve_workspace(cfg, B, workspace, INT64_MAX, &ws, true);
    const int D = cfg->M * cfg->N;
    const int64_t n = D + 1;
    const LayerLayout L{D};
    const float2 *yy = (const float2 *)y, *bb = (const float2 *)b;
    const Switches &sw = cfg_switches(cfg);
    const Route r = route_for(D, sw);
    if (k == cfg->K - 1) return launch_prep(cfg, W, k, yy, bb, sigma, 0, B, ws, PM_PHI_ONLY, r.eig_dim, st);
    const bool arrow = k == 0 && r.first != AR_NONE;   // Z = 0: arrowhead, no matrix is ever formed
    if (!arrow && r.error != RE_NONE) {
        set_error("%s", kRouteErrorText[r.error]);
        return ADMMNET_E_ARG;
    }
    // status[1] of a forward = the matrix-layers that went through the eigensolver (include/admmnet.h).  One writer per call:
    // with the matrix-function route on (r.matfun), its kernel counts the matrices it hands over and nothing is written here;
    // with the route off for this call every matrix of a dense layer goes there and no kernel counts, so the word is set here
    // to the dense matrix-layers up to and including layer k (the arrowhead layer is not one of them), saturating at INT32_MAX
    if (!arrow && r.matfun == MF_OFF && status) {
        const int64_t dense = B * (int64_t)(k + 1 - (r.first != AR_NONE ? 1 : 0));
        ADMM_HIP(hipMemsetD32Async((hipDeviceptr_t)(status + 1), (int)(dense > INT32_MAX ? INT32_MAX : dense), 1, st));
    }
    const float *lw = W + (int64_t)k * L.size();
    const int cur = k & 1;
    // chunk buffers and streams: one set on the caller's stream, or two sets on two internal streams (ADMMNET_STREAMS=2)
    Ws sets[2] = {ws, ws};
    hipStream_t ss[2] = {st, st};
    const bool dual = ws.set2_offset != 0;
    if (dual) {
        Carver c2{reinterpret_cast<char *>(workspace) + ws.set2_offset};
        carve_chunk(c2, r, ws.chunk, &sets[1]);
        if ((rc = chunk_streams(ss))) return rc;
        hipEvent_t e0;
        ADMM_HIP(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
        ADMM_HIP(hipEventRecord(e0, st));                  // everything the caller has enqueued so far ...
        ADMM_HIP(hipStreamWaitEvent(ss[0], e0, 0));        // ... happens before the chunks
        ADMM_HIP(hipStreamWaitEvent(ss[1], e0, 0));
        ADMM_HIP(hipEventDestroy(e0));
    }
    // The eigensolver fallback of chunk c on the side stream, beside prep and the matrix-function kernel of chunk c + 1 (SideStream
    // above).  Only where the fallback touches nothing the caller's stream touches meanwhile: the fused matrix function (prep then
    // writes no image, the chunk buffers belong to the eigen-pipeline alone), a dense layer, several chunks.  With the event
    // profiler on the call stays on one stream -- its per-class times are serial times (bench.py --full) -- and so it does with a
    // developer phase timer on, with ADMMNET_STREAMS=2 and with ADMMNET_STREAMS=1.
    // Flags: sp_fused_kernel of chunk c + 1 must not overwrite the flags the fallback of chunk c still reads, so consecutive chunks
    // alternate between ws.spec_flag and a second buffer, and the kernel of chunk c + 2 waits for the fallback of chunk c.  The
    // second buffer is ws.headkv read as int[256 D]: the head's K / V projections, which launch_head (admmnet_finish) writes
    // and then reads in one call, behind every layer -- nothing lives there while a layer runs, and this call joins the side
    // stream before it returns.  A chunk whose flags do not fit there stays on one stream.
    // The compact diagonals (common.h, Ws::diag) need no event of their own: sp_fused_kernel writes its chunk's slice on the stream
    // that launched it (the caller's, or a chunk stream of ADMMNET_STREAMS=2, joined before the layer ends), the fallback on the
    // side stream touches neither buffer, and their reader is prep_kernel of the NEXT layer, behind the join.
    const bool timers = sw.sf_timing || sw.pn_timing || sw.dc_timing || sw.br_timing;
    const bool fork = r.matfun == MF_FUSED && !arrow && B > ws.chunk && !sw.two_streams && !sw.one_stream && !prof().on && !timers &&
                      ws.spec_flag && ws.chunk <= (int64_t)256 * D;
    SideLease side;
    if (fork && (rc = side_acquire(&side))) return rc;
    int *const flags[2] = {ws.spec_flag, reinterpret_cast<int *>(ws.headkv)};   // (fork only)
    // The matrix-function kernel's shape follows the size of the matrix's group, as a separate call of that group would
    // choose it (spectral_waves).  Full groups of g and a short last group may take different shapes: no chunk then
    // straddles the start of the last group.  Without sub-batches both are spectral_waves(D, B) and nothing splits.
    const int64_t gsz = group_size(cfg, B), last0 = (group_count(cfg, B) - 1) * gsz;
    const int waves_full = spectral_waves(D, gsz, sw), waves_last = spectral_waves(D, B - last0, sw);
    const auto run_chunks = [&]() -> int {
        int rc, ci = 0;
        int64_t nb = 0;
        for (int64_t b0 = 0; b0 < B; b0 += nb, ++ci) {
            nb = (B - b0 < ws.chunk) ? (B - b0) : ws.chunk;
            if (waves_full != waves_last && b0 < last0 && b0 + nb > last0) nb = last0 - b0;
            const int waves = b0 >= last0 ? waves_last : waves_full;
            Ws wc = sets[ci & 1];
            if (fork) wc.spec_flag = flags[ci & 1];
            hipStream_t sc = ss[ci & 1];
            float2 *Zk = ws.Z + b0 * n * n;
            GLayerIO io{lw, ws.phi[cur] + b0 * D, ws.h[cur] + b0 * D, r.storage == ST_LEAN ? Zk : nullptr, ws.G + b0 * n * n,
                        ws.rn + b0, nullptr, r.lean()};
            if (arrow) {
                if ((rc = launch_prep(cfg, W, k, yy, bb, sigma, b0, nb, wc, PM_NO_MATRIX, r.eig_dim, sc))) return rc;
                if ((rc = launch_arrow_rebuild(r, sw, nb, io.lw, io.phi, io.h, io.G, io.rn, io.w_out, status, wc, sc, io.lower_only)))
                    return rc;
                continue;
            }
            // the lazy Z update of the previous layer rides the first sweep of the fused kernel: prep then only computes phi and h
            const bool fold = r.fold && k >= 1;
            const int mode = (r.storage == ST_HALF ? PM_HALF : r.storage == ST_LEAN ? PM_LEAN : 0) | (r.late_image ? PM_NOIMG : 0) |
                             (fold ? PM_SMALL : 0) | (fold && !sw.prep_gather ? PM_DIAG : 0);
            if ((rc = launch_prep(cfg, W, k, yy, bb, sigma, b0, nb, wc, mode, r.eig_dim, sc))) return rc;
            Ws wf = wc;
            // G as a matrix function where the spectrum allows it (checked per matrix, spectral.hip); the eigen-pipeline below then
            // only runs the matrices it flagged
            if (r.matfun != MF_OFF) {
                const int prv = cur ^ 1;
                const float *lwp = k >= 1 ? W + (int64_t)(k - 1) * L.size() : lw;
                // (these flags were chunk ci - 2's: its fallback has read them.  The side stream runs the fallbacks in order, so
                //  this also puts the fallback of chunk ci - 1 at most one chunk behind)
                if (fork && ci >= 2) ADMM_HIP(hipStreamWaitEvent(st, side.ev[ci & 1], 0));
                if ((rc = launch_spectral(sw, D, nb, lw, io.phi, io.h, Zk, io.G, io.rn, wc, status, sc, r.matfun, waves,
                                          fold ? ws.alpha + b0 : nullptr, fold ? ws.phi[prv] + b0 * D : nullptr,
                                          fold ? ws.h[prv] + b0 * D : nullptr, fold ? lwp : nullptr, fold ? (k == 1 ? 2 : 1) : 0, ws.diag ? ws.diag + b0 * 2 * D : nullptr,
                                          ws.diag ? ws.diag_ok + b0 : nullptr)))
                    return rc;
                wf.skip = wc.spec_flag;
                if (fork) {   // the rest of this chunk on the side stream, behind its matrix-function kernel
                    ADMM_HIP(hipEventRecord(side.ev[2], st));
                    ADMM_HIP(hipStreamWaitEvent(side.s, side.ev[2], 0));
                    sc = side.s;
                }
                // (the image only for the flagged matrices, afterwards)
                if (r.late_image && (rc = launch_half_image(D, nb, lw, io.phi, io.h, Zk, wf, r.eig_dim, sc))) return rc;
            }
            // (ST_LEAN: the tridiagonalisation's own loader forms A from the lower triangle of Z; ST_HALF reads the half image)
            if ((rc = eig_chunk(r, sw, nb, wf, status, sc, &io))) return rc;
            if (fork) ADMM_HIP(hipEventRecord(side.ev[ci & 1], side.s));
        }
        return ADMMNET_OK;
    };
    rc = run_chunks();
    if (fork) {   // the batch sums below read every chunk's rn; a launch that failed above leaves nothing running beside the caller either
        const int jrc = side_join(side, st);
        side_release(&side);
        if (!rc) rc = jrc;
    }
    if (rc) return rc;
    if (dual) {   // the caller's stream continues behind both chunk streams
        for (int q = 0; q < 2; ++q) {
            hipEvent_t e1;
            ADMM_HIP(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
            ADMM_HIP(hipEventRecord(e1, ss[q]));
            ADMM_HIP(hipStreamWaitEvent(st, e1, 0));
            ADMM_HIP(hipEventDestroy(e1));
        }
    }
    if (cfg->sub_batch > 0) return launch_rn_group_sum(B, gsz, ws.rn, sum_out ? sum_out : ws.sum, st);
    return launch_rn_sum(B, ws.rn, sum_out ? sum_out : ws.sum, st);
}

int admmnet_layer_back(const admmnet_cfg *cfg, const float *W, int32_t k, int64_t B, void *workspace,
                       const float *mean_dev, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (k < 0 || k >= cfg->K - 1 || !mean_dev) {
        set_error("layer_back: bad argument (k=%d)", k);
        return ADMMNET_E_ARG;
    }
    Ws ws;
    carve_workspace(cfg, B, workspace, INT64_MAX, &ws, true);
    const int D = cfg->M * cfg->N;
    const LayerLayout L{D};
    if (cfg->sub_batch > 0)   // mean_dev: one mean per group
        return launch_zstep_groups(W + (int64_t)k * L.size(), D, B, group_size(cfg, B), ws.rn, mean_dev, ws.alpha,
                                   (hipStream_t)stream);
    return launch_zstep(W + (int64_t)k * L.size(), D, B, ws.rn, mean_dev, ws.alpha, (hipStream_t)stream);
}

int admmnet_layer_back_pair(const admmnet_cfg *cfg, const float *W, int32_t k, int64_t B, void *workspace,
                            const double *sum_count_dev, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (k < 0 || k >= cfg->K - 1 || !sum_count_dev) {
        set_error("layer_back_pair: bad argument (k=%d)", k);
        return ADMMNET_E_ARG;
    }
    Ws ws;
    carve_workspace(cfg, B, workspace, INT64_MAX, &ws, true);
    const int D = cfg->M * cfg->N;
    const LayerLayout L{D};
    if (cfg->sub_batch > 0) {   // sum_count_dev: one pair per group
        if ((rc = launch_mean_from_pairs(sum_count_dev, group_count(cfg, B), ws.mean, (hipStream_t)stream))) return rc;
        return launch_zstep_groups(W + (int64_t)k * L.size(), D, B, group_size(cfg, B), ws.rn, ws.mean, ws.alpha,
                                   (hipStream_t)stream);
    }
    if ((rc = launch_mean_from_pair(sum_count_dev, ws.mean, (hipStream_t)stream))) return rc;
    return launch_zstep(W + (int64_t)k * L.size(), D, B, ws.rn, ws.mean, ws.alpha, (hipStream_t)stream);
}

int admmnet_finish(const admmnet_cfg *cfg, const float *W, int64_t B, void *workspace, void *phi_out,
                   float *head_out, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    Ws ws;
    carve_workspace(cfg, B, workspace, INT64_MAX, &ws, true);
    const int D = cfg->M * cfg->N;
    const float2 *phi = ws.phi[(cfg->K - 1) & 1];
    if (phi_out)
        ADMM_HIP(hipMemcpyAsync(phi_out, phi, sizeof(float2) * B * D, hipMemcpyDeviceToDevice, st));
    if (head_out) {
        if (!cfg->has_head) {
            set_error("finish: head_out given but cfg.has_head == 0");
            return ADMMNET_E_ARG;
        }
        const LayerLayout L{D};
        return launch_head(cfg, W + (int64_t)cfg->K * L.size(), B, phi, ws.headkv, head_out, st);
    }
    return ADMMNET_OK;
}

int admmnet_forward_f32(const admmnet_cfg *cfg, const float *W, const void *y, const void *b,
                        const float *sigma, int64_t B, void *phi_out, float *head_out, void *workspace,
                        int64_t workspace_bytes, int32_t *status, void *stream) {
    int rc;
    if ((rc = admmnet_begin(cfg, B, workspace, workspace_bytes, status, stream))) return rc;
    Ws ws;
    carve_workspace(cfg, B, workspace, workspace_bytes, &ws, true);
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < cfg->K; ++k) {
        if ((rc = admmnet_layer_front(cfg, W, k, y, b, sigma, B, workspace, ws.sum, status, stream))) return rc;
        if (k < cfg->K - 1) {
            if (cfg->sub_batch > 0) {   // ws.sum holds one pair per group
                if ((rc = admmnet_layer_back_pair(cfg, W, k, B, workspace, ws.sum, stream))) return rc;
                continue;
            }
            if ((rc = launch_mean_from_sum(ws.sum, B, ws.mean, st))) return rc;
            if ((rc = admmnet_layer_back(cfg, W, k, B, workspace, ws.mean, stream))) return rc;
        }
    }
    return admmnet_finish(cfg, W, B, workspace, phi_out, head_out, stream);
}

int admmnet_glayer_f32(const admmnet_cfg *cfg, const float *lw, const void *phi, const float *h,
                       const void *Z, int64_t B, void *G_out, float *w_out, float *rn_out, void *workspace,
                       int64_t workspace_bytes, int32_t *status, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (B < 1 || !lw || !phi || !h || !G_out || !workspace) {
        set_error("glayer: bad argument");
        return ADMMNET_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const int D = cfg->M * cfg->N;
    const int64_t n = D + 1;
    // workspace: [rn scratch B floats | chunk buffers]; weights scalars are needed on the host
    float sc[S_COUNT];
    ADMM_HIP(hipMemcpyAsync(sc, lw, sizeof(sc), hipMemcpyDeviceToHost, st));
    ADMM_HIP(hipStreamSynchronize(st));   // test/utility entry point only
    admmnet_cfg c2 = *cfg;
    Ws ws;
    char *base = (char *)workspace;
    const int64_t rn_bytes = align_up(sizeof(float) * B, 256);
    if ((rc = carve_workspace(&c2, B, base + rn_bytes, workspace_bytes - rn_bytes, &ws, false))) return rc;
    float *rn_tmp = (float *)base;
    if (status) ADMM_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st));
    const Switches &sw = cfg_switches(cfg);
    const Route r = route_for(D, sw);
    for (int64_t b0 = 0; b0 < B; b0 += ws.chunk) {
        const int64_t nb = (B - b0 < ws.chunk) ? (B - b0) : ws.chunk;
        const float2 *Zc = Z ? (const float2 *)Z + b0 * n * n : nullptr;
        const GLayerIO io{lw, (const float2 *)phi + b0 * D, h + b0 * D, nullptr, (float2 *)G_out + b0 * n * n,
                          rn_out ? rn_out + b0 : rn_tmp + b0, w_out ? w_out + b0 * n : nullptr, false};
        if (!Zc && r.first != AR_NONE) {
            if ((rc = launch_arrow_rebuild(r, sw, nb, io.lw, io.phi, io.h, io.G, io.rn, io.w_out, status, ws, st, io.lower_only)))
                return rc;
            continue;
        }
        if ((rc = launch_build_block(D, nb, sc[S_CORNER_G], sc[S_INV_RHO_G], io.phi, io.h, Zc, ws, r.eig_dim, st))) return rc;
        if ((rc = eig_chunk(r, sw, nb, ws, status, st, &io))) return rc;
    }
    return ADMMNET_OK;
}

int admmnet_glayer_spectral_f32(const admmnet_cfg *cfg, const float *layer_weights, const void *phi, const float *h,
                                void *Z, int32_t mode, const float *prev_layer_weights, const float *alpha,
                                const void *phi_prev, const float *h_prev, int64_t B, void *G, float *rn_out,
                                int32_t *flag, int32_t *status, int32_t waves, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    const int D = cfg->M * cfg->N;
    if (D < 8 || B < 1 || !layer_weights || !phi || !h || !Z || !G || !rn_out || !flag || !status || mode < 0 || mode > 2 ||
        (mode && (!prev_layer_weights || !alpha || !phi_prev || !h_prev)) || !(waves == 0 || waves == 4 || waves == 12)) {
        set_error("glayer_spectral: bad argument (D=%d, mode=%d, waves=%d)", D, mode, waves);
        return ADMMNET_E_ARG;
    }
    if (waves == 4 && D > 128) {
        set_error("glayer_spectral: the 4-wave shape needs D <= 128 (D=%d)", D);
        return ADMMNET_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    ADMM_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st));
    const Switches &sw = cfg_switches(cfg);
    return launch_spectral_fused(sw, D, B, layer_weights, (const float2 *)phi, h, (float2 *)Z, (float2 *)G, rn_out, flag, status,
                                 mode ? alpha : nullptr, mode ? (const float2 *)phi_prev : nullptr,
                                 mode ? h_prev : nullptr, mode ? prev_layer_weights : nullptr, mode,
                                 waves ? waves : spectral_waves(D, B, sw), /* no compact diagonals */ nullptr, nullptr, st);
}

int64_t admmnet_eigh_workspace_bytes(int32_t n, int64_t B) { return admmnet_eigh_workspace_bytes_o(n, B, 0); }

int64_t admmnet_eigh_workspace_bytes_o(int32_t n, int64_t B, int32_t options) {
    if (n < 2 || n - 1 > kMaxD || B < 1) return -1;
    admmnet_cfg cfg = {n - 1, 1, 3, 1, 0, 0, 0, {options}};
    if (check_cfg(&cfg)) return -1;
    Ws ws;
    carve_workspace(&cfg, B, nullptr, 0, &ws, false);
    return ws.total_bytes;
}

int64_t admmnet_glayer_workspace_bytes(const admmnet_cfg *cfg, int64_t B) {
    if (check_cfg(cfg) || B < 1) return -1;
    Ws ws;
    carve_workspace(cfg, B, nullptr, 0, &ws, false);
    return ws.total_bytes + align_up(sizeof(float) * B, 256);
}

int admmnet_eigh_c64(int32_t n, int64_t B, const void *A, float *w, void *V, void *workspace,
                     int64_t workspace_bytes, int32_t *status, void *stream) {
    return admmnet_eigh_c64_o(n, B, A, w, V, workspace, workspace_bytes, status, stream, 0);
}

int admmnet_eigh_c64_o(int32_t n, int64_t B, const void *A, float *w, void *V, void *workspace,
                       int64_t workspace_bytes, int32_t *status, void *stream, int32_t options) {
    if (n < 2 || n - 1 > kMaxD || B < 1 || !A || !w || !V || !workspace) {
        set_error("eigh: bad argument (n=%d)", n);
        return ADMMNET_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    admmnet_cfg cfg = {n - 1, 1, 3, 1, 0, 0, 0, {options}};
    Ws ws;
    int rc;
    if ((rc = check_cfg(&cfg))) return rc;
    if ((rc = carve_workspace(&cfg, B, workspace, workspace_bytes, &ws, false))) return rc;
    if (status) ADMM_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st));
    const int D = n - 1;
    const Switches &sw = cfg_switches(&cfg);
    const Route r = route_for(D, sw);
    for (int64_t b0 = 0; b0 < B; b0 += ws.chunk) {
        const int64_t nb = (B - b0 < ws.chunk) ? (B - b0) : ws.chunk;
        if ((rc = launch_build_generic(n, nb, (const float2 *)A + b0 * n * n, ws, r.eig_dim, st))) return rc;
        if ((rc = eig_chunk(r, sw, nb, ws, status, st, nullptr))) return rc;
        if ((rc = launch_vout(n, nb, (float2 *)V + b0 * (int64_t)n * n, w + b0 * n, ws, r.eig_dim, st))) return rc;
    }
    return ADMMNET_OK;
}

int admmnet_vdvh_c64(int32_t n, int64_t B, const void *V, const float *d, void *out, void *stream) {
    if (n < 1 || n - 1 > kMaxD || B < 1 || !V || !d || !out) {
        set_error("vdvh: bad argument (n=%d)", n);
        return ADMMNET_E_ARG;
    }
    return launch_vdvh(n, B, (const float2 *)V, d, (float2 *)out, (hipStream_t)stream);
}

int admmnet_vhsv_f32(int32_t n, int64_t B, const void *V, const void *S, float *q, void *stream) {
    if (n < 1 || n - 1 > kMaxD || B < 1 || !V || !S || !q) {
        set_error("vhsv: bad argument (n=%d)", n);
        return ADMMNET_E_ARG;
    }
    return launch_vhsv(n, B, (const float2 *)V, (const float2 *)S, q, (hipStream_t)stream);
}

// ---- training route: the n^2-sized steps of a layer (train_layer.hip) ------------------------------------------------------
// n as admmnet_eigh_c64 takes it; the tile-pair grid B * pairs(n) must fit a 31-bit grid
static int train_args_ok(const char *what, int32_t n, int64_t B, bool ptrs) {
    if (n < 2 || n - 1 > kMaxD || B < 1 || B * (int64_t)train_tile_pairs(n) > 0x7fffffffLL || !ptrs) {
        set_error("%s: bad argument (n=%d, B=%lld)", what, n, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_train_partials(int32_t n, int64_t B) {
    if (n < 2 || n - 1 > kMaxD || B < 1) return -1;
    return B * (int64_t)train_tile_pairs(n);
}

int admmnet_train_matrix_f32(int32_t n, int64_t B, const void *phi, const float *h, const void *Z, const float *r, float corner,
                             void *A, void *stream) {
    if (int rc = train_args_ok("train_matrix", n, B, phi && h && Z && r && A)) return rc;
    return launch_train_matrix(n, B, (const float2 *)phi, h, (const float2 *)Z, r, corner, (float2 *)A, (hipStream_t)stream);
}

int admmnet_train_matrix_bwd_f32(int32_t n, int64_t B, const void *gA, const void *Z, const float *r, void *gZ, void *g_phi,
                                 float *g_h, float *g_r, float *partials, void *stream) {
    if (int rc = train_args_ok("train_matrix_bwd", n, B, gA && Z && r && gZ && g_phi && g_h && g_r && partials)) return rc;
    return launch_train_matrix_bwd(n, B, (const float2 *)gA, (const float2 *)Z, r, (float2 *)gZ, (float2 *)g_phi, g_h, g_r,
                                   partials, (hipStream_t)stream);
}

int admmnet_train_resnorm_f32(int32_t n, int64_t B, const void *G, const void *phi, const float *h, float corner, float *rn,
                              void *stream) {
    if (int rc = train_args_ok("train_resnorm", n, B, G && phi && h && rn)) return rc;
    return launch_train_resnorm(n, B, (const float2 *)G, (const float2 *)phi, h, corner, rn, (hipStream_t)stream);
}

int admmnet_train_resnorm_bwd_f32(int32_t n, int64_t B, const float *g_rn, const float *rn, const void *G, const void *phi,
                                  const float *h, float corner, void *gG, void *g_phi, float *g_h, void *stream) {
    if (int rc = train_args_ok("train_resnorm_bwd", n, B, g_rn && rn && G && phi && h && gG && g_phi && g_h)) return rc;
    return launch_train_resnorm_bwd(n, B, g_rn, rn, (const float2 *)G, (const float2 *)phi, h, corner, (float2 *)gG,
                                    (float2 *)g_phi, g_h, (hipStream_t)stream);
}

int admmnet_train_zupdate_c64(int32_t n, int64_t B, const void *Z, const void *G, const void *phi, const float *h,
                              const float *s, float corner, void *Z_new, void *stream) {
    if (int rc = train_args_ok("train_zupdate", n, B, Z && G && phi && h && s && Z_new)) return rc;
    return launch_train_zupdate(n, B, (const float2 *)Z, (const float2 *)G, (const float2 *)phi, h, s, corner, (float2 *)Z_new,
                                (hipStream_t)stream);
}

int admmnet_train_zupdate_bwd_c64(int32_t n, int64_t B, const void *g, const void *G, const void *phi, const float *h,
                                  const float *s, float corner, void *gG, void *g_phi, float *g_h, float *g_s, void *stream) {
    if (int rc = train_args_ok("train_zupdate_bwd", n, B, g && G && phi && h && s && gG && g_phi && g_h && g_s)) return rc;
    return launch_train_zupdate_bwd(n, B, (const float2 *)g, (const float2 *)G, (const float2 *)phi, h, s, corner, (float2 *)gG,
                                    (float2 *)g_phi, g_h, g_s, (hipStream_t)stream);
}

int admmnet_train_gather_c64(int32_t n, int64_t B, const void *X, void *col, float *diag, void *stream) {
    if (int rc = train_args_ok("train_gather", n, B, X && col && diag)) return rc;
    return launch_train_gather(n, B, (const float2 *)X, (float2 *)col, diag, (hipStream_t)stream);
}

int admmnet_train_scatter_c64(int32_t n, int64_t B, const void *g_col, const float *g_diag, void *gX, void *stream) {
    if (int rc = train_args_ok("train_scatter", n, B, g_col && g_diag && gX)) return rc;
    return launch_train_scatter(n, B, (const float2 *)g_col, g_diag, (float2 *)gX, (hipStream_t)stream);
}

int admmnet_train_herm_c64(int32_t n, int64_t B, const void *g, const void *g_col, const float *g_diag, void *S, void *stream) {
    if (int rc = train_args_ok("train_herm", n, B, g && S && (!g_col == !g_diag))) return rc;
    return launch_train_herm(n, B, (const float2 *)g, (const float2 *)g_col, g_diag, (float2 *)S, (hipStream_t)stream);
}

// ---- training route "full": the O(B D)-sized steps of a layer (train_small.hip) -----------------------------------------------
// D = M N for phi / hinput / hproject, n = D + 1 for eigmap; the slab grid must fit 31 bits
static int train_small_args_ok(const char *what, int32_t d, int32_t dmin, int32_t dmax, int64_t B, bool ptrs) {
    if (d < dmin || d > dmax || B < 1 || train_small_rows(B) > 0x7fffffffLL || !ptrs) {
        set_error("%s: bad argument (size=%d, B=%lld)", what, d, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

static int train_step_args_ok(const char *what, int64_t B, int64_t g, bool ptrs) {
    if (B < 1 || g < 0 || train_small_groups(B, g) > 0x7fffffffLL || !ptrs) {
        set_error("%s: bad argument (B=%lld, sub_batch=%lld)", what, (long long)B, (long long)g);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_train_small_partials(int32_t step, int64_t B, int64_t sub_batch) {
    if (B < 1 || sub_batch < 0) return -1;
    switch (step) {
    case ADMMNET_TRAIN_PHI:
    case ADMMNET_TRAIN_HINPUT:
    case ADMMNET_TRAIN_HPROJECT: return train_small_rows(B);
    case ADMMNET_TRAIN_EIGMAP: return train_small_rows(B) * ADMMNET_TRAIN_EIGMAP_GRADS;
    case ADMMNET_TRAIN_STEPSIZE: return train_small_groups(B, sub_batch) * ADMMNET_TRAIN_STEPSIZE_GRADS + B;
    }
    return -1;
}

int admmnet_train_phi_c64(int32_t D, int64_t B, const void *y, const void *b, const void *g_col, const void *z_col,
                          const float *rho, void *phi, void *stream) {
    if (int rc = train_small_args_ok("train_phi", D, 1, kMaxD, B, y && b && g_col && z_col && rho && phi)) return rc;
    return launch_train_phi(D, B, (const float2 *)y, (const float2 *)b, (const float2 *)g_col, (const float2 *)z_col, rho,
                            (float2 *)phi, (hipStream_t)stream);
}

int admmnet_train_phi_bwd_c64(int32_t D, int64_t B, const void *g_phi, const void *y, const void *b, const void *g_col,
                              const void *z_col, const float *rho, void *g_gcol, void *g_zcol, float *g_rho, float *partials,
                              void *stream) {
    if (int rc = train_small_args_ok("train_phi_bwd", D, 1, kMaxD, B,
                                     g_phi && y && b && g_col && z_col && rho && g_gcol && g_zcol && g_rho && partials))
        return rc;
    return launch_train_phi_bwd(D, B, (const float2 *)g_phi, (const float2 *)y, (const float2 *)b, (const float2 *)g_col,
                                (const float2 *)z_col, rho, (float2 *)g_gcol, (float2 *)g_zcol, g_rho, partials,
                                (hipStream_t)stream);
}

int admmnet_train_hinput_f32(int32_t D, int64_t B, const float *g_dg, const float *z_dg, const float *rho, float *t,
                             void *stream) {
    if (int rc = train_small_args_ok("train_hinput", D, 1, kMaxD, B, g_dg && z_dg && rho && t)) return rc;
    return launch_train_hinput(D, B, g_dg, z_dg, rho, t, (hipStream_t)stream);
}

int admmnet_train_hinput_bwd_f32(int32_t D, int64_t B, const float *g_t, const float *z_dg, const float *rho, float *g_gdg,
                                 float *g_zdg, float *g_rho, float *partials, void *stream) {
    if (int rc = train_small_args_ok("train_hinput_bwd", D, 1, kMaxD, B, g_t && z_dg && rho && g_gdg && g_zdg && g_rho && partials))
        return rc;
    return launch_train_hinput_bwd(D, B, g_t, z_dg, rho, g_gdg, g_zdg, g_rho, partials, (hipStream_t)stream);
}

int admmnet_train_hproject_f32(int32_t D, int64_t B, const float *t, const float *m, const float *sigma,
                               const float *projection_weight, float *h, void *stream) {
    if (int rc = train_small_args_ok("train_hproject", D, 1, kMaxD, B, t && m && sigma && projection_weight && h)) return rc;
    return launch_train_hproject(D, B, t, m, sigma, projection_weight, h, (hipStream_t)stream);
}

int admmnet_train_hproject_bwd_f32(int32_t D, int64_t B, const float *g_h, const float *t, const float *m, const float *sigma,
                                   const float *projection_weight, float *g_t, float *g_m, float *g_pw, float *partials,
                                   void *stream) {
    if (int rc = train_small_args_ok("train_hproject_bwd", D, 1, kMaxD, B,
                                     g_h && t && m && sigma && projection_weight && g_t && g_m && g_pw && partials))
        return rc;
    return launch_train_hproject_bwd(D, B, g_h, t, m, sigma, projection_weight, g_t, g_m, g_pw, partials, (hipStream_t)stream);
}

// ---- training route "native": the H layer with correction_net inside (train_hlayer.hip) ------------------------------------------
// the batch-slab grid of the weight-gradient product is the launch's y dimension
static int train_hlayer_args_ok(const char *what, int32_t D, int64_t B, bool ptrs) {
    if (int rc = train_small_args_ok(what, D, 1, kMaxD, B, ptrs)) return rc;
    if (B > (int64_t)65535 * 128) {
        set_error("%s: bad argument (B=%lld)", what, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_train_hlayer_workspace(int32_t D, int64_t B) {
    if (D < 1 || D > kMaxD || B < 1 || B > (int64_t)65535 * 128) return -1;
    return train_hlayer_workspace_floats(D, B) * (int64_t)sizeof(float);
}

int admmnet_train_hlayer_f32(int32_t D, int64_t B, const float *g_dg, const float *z_dg, const float *sigma, const float *rho,
                             const float *projection_weight, const float *W1, const float *b1, const float *W2, const float *b2,
                             float *h, float *t, float *a1, float *m, void *stream) {
    if (int rc = train_hlayer_args_ok("train_hlayer", D, B,
                                      g_dg && z_dg && sigma && rho && projection_weight && W1 && b1 && W2 && b2 && h && t && a1 && m))
        return rc;
    return launch_train_hlayer(D, B, g_dg, z_dg, sigma, rho, projection_weight, W1, b1, W2, b2, h, t, a1, m, (hipStream_t)stream);
}

int admmnet_train_hlayer_bwd_f32(int32_t D, int64_t B, const float *g_h, const float *z_dg, const float *sigma, const float *rho,
                                 const float *projection_weight, const float *W1, const float *W2, const float *t, const float *a1,
                                 const float *m, float *g_gdg, float *g_zdg, float *delta1, float *delta2, float *g_params,
                                 void *workspace, void *stream) {
    if (int rc = train_hlayer_args_ok("train_hlayer_bwd", D, B,
                                      g_h && z_dg && sigma && rho && projection_weight && W1 && W2 && t && a1 && m && g_gdg &&
                                          g_zdg && delta1 && delta2 && g_params && workspace))
        return rc;
    return launch_train_hlayer_bwd(D, B, g_h, z_dg, sigma, rho, projection_weight, W1, W2, t, a1, m, g_gdg, g_zdg, delta1, delta2,
                                   g_params, (float *)workspace, (hipStream_t)stream);
}

// ---- training route "native": the PeakSearchLayer head (train_head.hip) ---------------------------------------------------------
// the slabs of the (signal, target) pairs are the product launch's y dimension
static int train_head_args_ok(const char *what, int32_t D, int32_t L, int64_t B, const void *const *params, const void *keep, float p,
                              bool ptrs) {
    bool ok = D >= 1 && D <= kMaxD && L >= 1 && L <= 16 && B >= 1 && B * L <= (int64_t)65535 * 128 && ptrs && params;
    ok = ok && (!keep || (p >= 0.f && p < 1.f));
    for (int i = 0; ok && i < 21 + 8 * L; ++i) ok = params[i] != nullptr;
    if (!ok) {
        set_error("%s: bad argument (D=%d, L=%d, B=%lld, p=%g)", what, D, L, (long long)B, (double)p);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_train_head_workspace(int32_t D, int32_t L, int64_t B, int32_t part) {
    if (D < 1 || D > kMaxD || L < 1 || L > 16 || B < 1 || B * L > (int64_t)65535 * 128) return -1;
    switch (part) {
    case ADMMNET_TRAIN_HEAD_SAVED: return train_head_saved_floats(D, L, B) * (int64_t)sizeof(float);
    case ADMMNET_TRAIN_HEAD_WORK: return train_head_work_floats(D, L, B) * (int64_t)sizeof(float);
    case ADMMNET_TRAIN_HEAD_GRADS: return train_head_grad_floats(D, L) * (int64_t)sizeof(float);
    }
    return -1;
}

int admmnet_train_head_f32(int32_t D, int32_t L, int64_t B, const void *phi, const void *const *params, const uint8_t *keep, float p,
                           float *tau, float *f, float *conf, void *saved, void *stream) {
    if (int rc = train_head_args_ok("train_head", D, L, B, phi ? params : nullptr, keep, p, phi && tau && f && conf && saved))
        return rc;
    return launch_train_head(D, L, B, (const float2 *)phi, (const float *const *)params, keep, keep ? p : 0.f, tau, f, conf,
                             (float *)saved, (hipStream_t)stream);
}

int admmnet_train_head_bwd_f32(int32_t D, int32_t L, int64_t B, const float *g_tau, const float *g_f, const float *g_conf,
                               const void *phi, const void *const *params, const uint8_t *keep, float p, const float *tau,
                               const float *f, const float *conf, void *saved, void *g_phi, float *g_params, void *workspace,
                               void *stream) {
    const bool ptrs = g_tau && g_f && g_conf && phi && tau && f && conf && saved && g_phi && g_params && workspace;
    if (int rc = train_head_args_ok("train_head_bwd", D, L, B, ptrs ? params : nullptr, keep, p, ptrs)) return rc;
    return launch_train_head_bwd(D, L, B, g_tau, g_f, g_conf, (const float2 *)phi, (const float *const *)params, keep,
                                 keep ? p : 0.f, tau, f, conf, (float *)saved, (float2 *)g_phi, g_params, (float *)workspace,
                                 (hipStream_t)stream);
}

int admmnet_train_eigmap_f32(int32_t n, int64_t B, const float *w, const float *threshold, const float *W1, const float *b1,
                             const float *W2, const float *b2, float *wp, void *stream) {
    if (int rc = train_small_args_ok("train_eigmap", n, 2, kMaxD + 1, B, w && threshold && W1 && b1 && W2 && b2 && wp)) return rc;
    return launch_train_eigmap(n, B, w, threshold, W1, b1, W2, b2, wp, (hipStream_t)stream);
}

int admmnet_train_eigmap_bwd_f32(int32_t n, int64_t B, const float *g_wp, const float *w, const float *threshold, const float *W1,
                                 const float *b1, const float *W2, const float *b2, float *g_w, float *g_params, float *partials,
                                 void *stream) {
    if (int rc = train_small_args_ok("train_eigmap_bwd", n, 2, kMaxD + 1, B,
                                     g_wp && w && threshold && W1 && b1 && W2 && b2 && g_w && g_params && partials))
        return rc;
    return launch_train_eigmap_bwd(n, B, g_wp, w, threshold, W1, b1, W2, b2, g_w, g_params, partials, (hipStream_t)stream);
}

int admmnet_train_stepsize_f32(int64_t B, int64_t sub_batch, float knorm, const float *rn, const float *rho, const float *W1,
                               const float *b1, const float *W2, const float *b2, float *step, void *stream) {
    if (int rc = train_step_args_ok("train_stepsize", B, sub_batch, rn && rho && W1 && b1 && W2 && b2 && step)) return rc;
    return launch_train_stepsize(B, sub_batch, knorm, rn, rho, W1, b1, W2, b2, step, (hipStream_t)stream);
}

int admmnet_train_stepsize_bwd_f32(int64_t B, int64_t sub_batch, float knorm, const float *g_step, const float *rn,
                                   const float *rho, const float *W1, const float *b1, const float *W2, const float *b2,
                                   float *g_rn, float *g_params, float *partials, void *stream) {
    if (int rc = train_step_args_ok("train_stepsize_bwd", B, sub_batch,
                                    g_step && rn && rho && W1 && b1 && W2 && b2 && g_rn && g_params && partials))
        return rc;
    return launch_train_stepsize_bwd(B, sub_batch, knorm, g_step, rn, rho, W1, b1, W2, b2, g_rn, g_params, partials,
                                     (hipStream_t)stream);
}

// the step size from an outside (sum, count) pair; the doubles need their natural alignment
static int train_pair_args_ok(const char *what, int64_t B, bool ptrs, const void *d0, const void *d1, const void *d2) {
    const bool aligned = (((uintptr_t)d0 | (uintptr_t)d1 | (uintptr_t)d2) & 7u) == 0;
    if (B < 1 || train_pair_rows(B) > 0x7fffffffLL || !ptrs || !aligned) {
        set_error("%s: bad argument (B=%lld, a null pointer, or float64 data that is not 8-byte aligned)", what, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_train_stepsize_pair_partials(int64_t B) { return B < 1 ? -1 : train_pair_partials(B); }

int admmnet_train_rnsum_f64(int64_t B, const float *rn, double *pair, void *stream) {
    if (int rc = train_pair_args_ok("train_rnsum", B, rn && pair, pair, nullptr, nullptr)) return rc;
    return launch_train_rnsum(B, rn, pair, (hipStream_t)stream);
}

int admmnet_train_stepsize_pair_f32(int64_t B, float knorm, const float *rn, const double *pair, const float *rho, const float *W1,
                                    const float *b1, const float *W2, const float *b2, float *step, void *stream) {
    if (int rc = train_pair_args_ok("train_stepsize_pair", B, rn && pair && rho && W1 && b1 && W2 && b2 && step, pair, nullptr, nullptr))
        return rc;
    return launch_train_stepsize_pair(B, knorm, rn, pair, rho, W1, b1, W2, b2, step, (hipStream_t)stream);
}

int admmnet_train_stepsize_bwd_pair_front_f32(int64_t B, float knorm, const float *g_step, const float *rn, const double *pair,
                                              const float *rho, const float *W1, const float *b1, const float *W2, const float *b2,
                                              float *g_u, float *g_params, double *total, float *partials, void *stream) {
    if (int rc = train_pair_args_ok("train_stepsize_bwd_pair_front", B,
                                    g_step && rn && pair && rho && W1 && b1 && W2 && b2 && g_u && g_params && total && partials, pair,
                                    total, partials))
        return rc;
    return launch_train_stepsize_bwd_pair_front(B, knorm, g_step, rn, pair, rho, W1, b1, W2, b2, g_u, g_params, total, partials,
                                                (hipStream_t)stream);
}

int admmnet_train_stepsize_bwd_pair_back_f32(int64_t B, const float *g_u, const double *pair, const double *total, float *g_rn,
                                             void *stream) {
    if (int rc = train_pair_args_ok("train_stepsize_bwd_pair_back", B, g_u && pair && total && g_rn, pair, total, nullptr)) return rc;
    return launch_train_stepsize_bwd_pair_back(B, g_u, pair, total, g_rn, (hipStream_t)stream);
}

// ---- the training losses (loss.hip) ------------------------------------------------------------------------------------------
// one lane per target slot (Lmax <= 64); the slab grid must fit 31 bits
static int loss_args_ok(const char *what, int32_t Lmax, int32_t D, int64_t B, bool ptrs) {
    if (Lmax < 1 || Lmax > 64 || D < 1 || B < 1 || train_small_rows(B) > 0x7fffffffLL || !ptrs) {
        set_error("%s: bad argument (Lmax=%d, D=%d, B=%lld)", what, Lmax, D, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_loss_partials(int32_t loss, int64_t B) {
    if (B < 1 || (loss != ADMMNET_LOSS_ANM && loss != ADMMNET_LOSS_PHI)) return -1;
    return loss_partials(loss, B);
}

int admmnet_loss_anm_f32(int32_t Lmax, int32_t D, int64_t B, const float *tau, const float *f, const float *conf,
                         const float *tau_true, const float *f_true, const int64_t *L_true, const void *phi, float lambda_reg,
                         float *out, float *norms, int32_t *status, float *partials, void *stream) {
    if (int rc = loss_args_ok("loss_anm", Lmax, D, B,
                              tau && f && conf && tau_true && f_true && L_true && phi && out && norms && status && partials))
        return rc;
    return launch_loss_anm(Lmax, D, B, tau, f, conf, tau_true, f_true, L_true, (const float2 *)phi, lambda_reg, out, norms,
                           status, partials, (hipStream_t)stream);
}

int admmnet_loss_anm_bwd_f32(int32_t Lmax, int32_t D, int64_t B, const float *g_out, const float *tau, const float *f,
                             const float *conf, const float *tau_true, const float *f_true, const int64_t *L_true,
                             const void *phi, const float *norms, float lambda_reg, float *g_tau, float *g_f, float *g_conf,
                             void *g_phi, void *stream) {
    if (int rc = loss_args_ok("loss_anm_bwd", Lmax, D, B,
                              g_out && tau && f && conf && tau_true && f_true && L_true && phi && norms && g_tau && g_f &&
                                  g_conf && g_phi))
        return rc;
    return launch_loss_anm_bwd(Lmax, D, B, g_out, tau, f, conf, tau_true, f_true, L_true, (const float2 *)phi, norms,
                               lambda_reg, g_tau, g_f, g_conf, (float2 *)g_phi, (hipStream_t)stream);
}

int admmnet_loss_phi_c64(int32_t D, int64_t B, const void *phi, const void *phi_true, float amplitude_weight,
                         float phase_weight, float *out, float *partials, void *stream) {
    if (int rc = loss_args_ok("loss_phi", 1, D, B, phi && phi_true && out && partials)) return rc;
    return launch_loss_phi(D, B, (const float2 *)phi, (const float2 *)phi_true, amplitude_weight, phase_weight, out, partials,
                           (hipStream_t)stream);
}

int admmnet_loss_phi_bwd_c64(int32_t D, int64_t B, const float *g_out, const void *phi, const void *phi_true,
                             float amplitude_weight, float phase_weight, void *g_phi, void *stream) {
    if (int rc = loss_args_ok("loss_phi_bwd", 1, D, B, g_out && phi && phi_true && g_phi)) return rc;
    return launch_loss_phi_bwd(D, B, g_out, (const float2 *)phi, (const float2 *)phi_true, amplitude_weight, phase_weight,
                               (float2 *)g_phi, (hipStream_t)stream);
}

// ---- the spectral terms of the phi loss (loss_spectrum.hip) ------------------------------------------------------------------
// bases of at most 1024 keep every index product inside 31 bits; the LDS limit (workspace_bytes < 0) is far below that
static int64_t loss_spectrum_need(int32_t xbase, int32_t ybase, int32_t oversample, int64_t B) {
    if (xbase < 1 || ybase < 1 || xbase > 1024 || ybase > 1024 || oversample < 1 || oversample > LS_MAX_OVERSAMPLE || B < 1 ||
        B > 0x7fffffffLL)
        return -1;
    return loss_spectrum_workspace_bytes(xbase, ybase, oversample, B);
}

int64_t admmnet_loss_spectrum_workspace_bytes(int32_t xbase, int32_t ybase, int32_t oversample, int64_t B) {
    return loss_spectrum_need(xbase, ybase, oversample, B);
}

static int loss_spectrum_args_ok(const char *what, int32_t xbase, int32_t ybase, int32_t oversample, int32_t Lmax, int64_t B,
                                 bool ptrs, bool target, const void *workspace, int64_t workspace_bytes) {
    const int64_t need = loss_spectrum_need(xbase, ybase, oversample, B);
    if (need < 0 || Lmax < 0 || Lmax > LS_MAX_TARGETS || (target && Lmax < 1) || !ptrs || !workspace) {
        set_error("%s: bad argument (xbase=%d, ybase=%d, oversample=%d, Lmax=%d, B=%lld, a null pointer, or a grid beyond the LDS)",
                  what, xbase, ybase, oversample, Lmax, (long long)B);
        return ADMMNET_E_ARG;
    }
    if (workspace_bytes < need) {
        set_error("%s: workspace too small (%lld < %lld bytes)", what, (long long)workspace_bytes, (long long)need);
        return ADMMNET_E_WORKSPACE;
    }
    return ADMMNET_OK;
}

int admmnet_loss_spectrum_f64(int32_t xbase, int32_t ybase, int32_t oversample, int32_t Lmax, int64_t B, const void *phi,
                              const void *phi_true, const float *tau_true, const float *f_true, const int64_t *L_true,
                              float spectral_weight, float distribution_weight, float target_weight, float *out,
                              int32_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
    const bool target = L_true != nullptr;
    if (int rc = loss_spectrum_args_ok("loss_spectrum", xbase, ybase, oversample, Lmax, B,
                                       phi && out && status && (phi_true || target) && (!target || (tau_true && f_true)), target,
                                       workspace, workspace_bytes))
        return rc;
    return launch_loss_spectrum(xbase, ybase, oversample, Lmax, B, (const float2 *)phi, (const float2 *)phi_true, tau_true, f_true,
                                L_true, spectral_weight, distribution_weight, target_weight, out, status, workspace,
                                (hipStream_t)stream);
}

int admmnet_loss_spectrum_bwd_f64(int32_t xbase, int32_t ybase, int32_t oversample, int32_t Lmax, int64_t B, const float *g_out,
                                  const void *phi, const float *tau_true, const float *f_true, const int64_t *L_true,
                                  float spectral_weight, float distribution_weight, float target_weight, int32_t skip,
                                  const void *workspace, int64_t workspace_bytes, void *g_phi, void *stream) {
    const bool target = !(skip & ADMMNET_LOSS_SPECTRUM_SKIP_TARGET);
    if (int rc = loss_spectrum_args_ok("loss_spectrum_bwd", xbase, ybase, oversample, Lmax, B,
                                       g_out && phi && g_phi && skip >= 0 && skip < 8 && (!target || (tau_true && f_true && L_true)),
                                       target, workspace, workspace_bytes))
        return rc;
    return launch_loss_spectrum_bwd(xbase, ybase, oversample, Lmax, B, g_out, (const float2 *)phi, tau_true, f_true, L_true,
                                    spectral_weight, distribution_weight, target_weight, skip, workspace, (float2 *)g_phi,
                                    (hipStream_t)stream);
}

// ---- the assignment loss of the head (loss_set.hip) ---------------------------------------------------------------------------
// one lane per slot and per target (<= 64 each); the slab grid must fit 31 bits
static int loss_set_args_ok(const char *what, int32_t Lmax, int32_t Lt, int32_t D, int64_t B, bool ptrs, const double *opts) {
    if (Lmax < 1 || Lmax > SC_MAX || Lt < 1 || Lt > SC_MAX || D < 1 || B < 1 || train_small_rows(B) > 0x7fffffffLL || !ptrs || !opts) {
        set_error("%s: bad argument (Lmax=%d, Lt=%d, D=%d, B=%lld, or a null pointer)", what, Lmax, Lt, D, (long long)B);
        return ADMMNET_E_ARG;
    }
    if (!set_opts_ok(opts)) {
        set_error("%s: bad options (sx=%g, sy=%g must be > 0, periods %g, %g >= 0, w_conf=%g >= 0, lambda_reg=%g >= 0, all finite)",
                  what, opts[0], opts[1], opts[2], opts[3], opts[4], opts[5]);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_loss_set_partials(int64_t B) {
    if (B < 1 || train_small_rows(B) > 0x7fffffffLL) return -1;
    return loss_set_partials(B);
}

int admmnet_loss_set_f32(int32_t Lmax, int32_t Lt, int32_t D, int64_t B, const float *tau, const float *f, const float *conf,
                         const float *tau_true, const float *f_true, const int64_t *L_true, const void *phi, const double *opts,
                         float *out, int32_t *assign, float *norms, int32_t *status, double *partials, void *stream) {
    if (int rc = loss_set_args_ok("loss_set", Lmax, Lt, D, B,
                                  tau && f && conf && tau_true && f_true && L_true && phi && out && assign && norms && status &&
                                      partials,
                                  opts))
        return rc;
    return launch_loss_set(Lmax, Lt, D, B, tau, f, conf, tau_true, f_true, L_true, (const float2 *)phi, opts, out, assign, norms,
                           status, partials, (hipStream_t)stream);
}

int admmnet_loss_set_bwd_f32(int32_t Lmax, int32_t Lt, int32_t D, int64_t B, const float *g_out, const float *tau, const float *f,
                             const float *conf, const float *tau_true, const float *f_true, const int64_t *L_true,
                             const void *phi, const int32_t *assign, const float *norms, const double *opts, float *g_tau,
                             float *g_f, float *g_conf, void *g_phi, void *stream) {
    if (int rc = loss_set_args_ok("loss_set_bwd", Lmax, Lt, D, B,
                                  g_out && tau && f && conf && tau_true && f_true && L_true && phi && assign && norms && g_tau &&
                                      g_f && g_conf && g_phi,
                                  opts))
        return rc;
    return launch_loss_set_bwd(Lmax, Lt, D, B, g_out, tau, f, conf, tau_true, f_true, L_true, (const float2 *)phi, assign, norms,
                               opts, g_tau, g_f, g_conf, (float2 *)g_phi, (hipStream_t)stream);
}

// ---- estimates against ground truth (score.hip) ------------------------------------------------------------------------------
// one lane per estimate and per target (<= 64 each); the slab grid must fit 31 bits
static int score_args_ok(const char *what, int32_t Le, int32_t Lt, int64_t B, bool ptrs) {
    if (Le < 1 || Le > SC_MAX || Lt < 1 || Lt > SC_MAX || B < 1 || train_small_rows(B) > 0x7fffffffLL || !ptrs) {
        set_error("%s: bad argument (Le=%d, Lt=%d, B=%lld, or a null pointer)", what, Le, Lt, (long long)B);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int64_t admmnet_score_partials(int64_t B) {
    if (B < 1) return -1;
    return score_partials(B);
}

int admmnet_score_match_f64(int32_t Le, int32_t Lt, int64_t B, const double *est, const int32_t *n_est, const float *tau_true,
                            const float *f_true, const int64_t *L_true, const double *opts, int32_t *match, double *stats,
                            double *totals, int32_t *status, double *partials, void *stream) {
    if (int rc = score_args_ok("score_match", Le, Lt, B, est && tau_true && f_true && opts && match && stats && totals && status && partials))
        return rc;
    if (!sc_opts_ok(opts) || !sc_finite(opts[2] * opts[2])) {
        set_error("score_match: bad options (sx=%g, sy=%g must be > 0, cutoff=%g > 0 with a finite square, periods %g, %g >= 0)",
                  opts[0], opts[1], opts[2], opts[3], opts[4]);
        return ADMMNET_E_ARG;
    }
    return launch_score_match(Le, Lt, B, est, n_est, tau_true, f_true, L_true, opts, match, stats, totals, status, partials,
                              (hipStream_t)stream);
}

int admmnet_score_ordered_f32(int32_t Lmax, int64_t B, const float *tau_est, const float *f_est, const float *tau_true,
                              const float *f_true, const int64_t *L_true, double *per_sample, double *out, int32_t *status,
                              double *partials, void *stream) {
    if (int rc = score_args_ok("score_ordered", Lmax, Lmax, B,
                               tau_est && f_est && tau_true && f_true && L_true && per_sample && out && status && partials))
        return rc;
    return launch_score_ordered(Lmax, B, tau_est, f_est, tau_true, f_true, L_true, per_sample, out, status, partials,
                                (hipStream_t)stream);
}

// ---- the Cramer-Rao bound of a scene's targets (crb.hip) ----------------------------------------------------------------------
// one lane per parameter (4 Lt <= 64); the scenes are those the generator makes (synth.hip's ceiling on Nb * Nd)
int64_t admmnet_crb_partials(int64_t B) {
    if (B < 1 || B > 2147483647) return -1;
    return crb_partials(B);
}

int admmnet_crb_f64(int32_t Nb, int32_t Nd, int32_t Lt, int64_t B, const float *tau_true, const float *f_true, const void *C,
                    const int64_t *L_true, const int32_t *match, const double *noise, int32_t noise_is_snr, double *bound,
                    double *totals, int32_t *status, double *partials, void *stream) {
    if (Lt < 1 || Lt > CRB_MAXL || B < 1 || B > 2147483647 || Nb < 1 || Nd < 1 || (int64_t)Nb * Nd > synth_max_cells() ||
        (noise_is_snr != 0 && noise_is_snr != 1) || !tau_true || !f_true || !C || !noise || !bound || !totals || !status ||
        !partials) {
        set_error("crb: bad argument (Nb=%d, Nd=%d with Nb * Nd <= %lld, Lt=%d in 1 .. %d, B=%lld, noise_is_snr=%d, or a null pointer)",
                  Nb, Nd, (long long)synth_max_cells(), Lt, CRB_MAXL, (long long)B, noise_is_snr);
        return ADMMNET_E_ARG;
    }
    return launch_crb(Nb, Nd, Lt, B, tau_true, f_true, (const float2 *)C, L_true, match, noise, noise_is_snr, bound, totals, status,
                      partials, (hipStream_t)stream);
}

// ---- target estimates refined against the received signal (refine.hip) -------------------------------------------------------
// one lane per parameter (4 Le <= 64); x, the matrix and the twiddle tables of a scene stay in the LDS of its workgroup
static bool refine_sizes_ok(int32_t Nb, int32_t Nd, int32_t Le) {
    return Le >= 1 && Le <= CRB_MAXL && Nb >= 1 && Nd >= 1 && (int64_t)Nb * Nd <= synth_max_cells();
}

// the scene kernels (scene_wg.h) keep a scene in the LDS of its workgroup: one that does not fit is refused, `before third after`
// saying which third size goes with the grid
static int scene_lds_ok(const char *what, int32_t Nb, int32_t Nd, const char *before, int32_t third, const char *after, int64_t need,
                        int64_t limit) {
    if (need <= limit) return ADMMNET_OK;
    set_error("%s: a %d x %d grid %s%d%s needs %lld bytes of LDS, a workgroup has %lld", what, Nb, Nd, before, third, after,
              (long long)need, (long long)limit);
    return ADMMNET_E_ARG;
}

int64_t admmnet_refine_lds_bytes(int32_t Nb, int32_t Nd, int32_t Le) {
    return refine_sizes_ok(Nb, Nd, Le) ? refine_lds_bytes(Nb, Nd, Le) : -1;
}

int admmnet_refine_f64(int32_t Nb, int32_t Nd, int32_t Le, int64_t B, const void *y, const void *b, const double *rows_in,
                       const int32_t *n_est, int32_t mode, int32_t psk_m, double psk_phase, int32_t iters, double tol,
                       double *rows_out, void *C_out, double *info, int32_t *symbols_out, int32_t *status, void *stream) {
    if (!refine_sizes_ok(Nb, Nd, Le) || B < 1 || B > 2147483647 || (mode != 0 && mode != 1) || psk_m < 2 || psk_m > REFINE_MAX_M ||
        !sc_finite(psk_phase) || iters < 1 || iters > REFINE_MAX_ITERS || !(tol > 0.0) || !sc_finite(tol) || !y || !b || !rows_in ||
        !rows_out || !C_out || !info || !status) {
        set_error("refine: bad argument (Nb=%d, Nd=%d with Nb * Nd <= %lld, Le=%d in 1 .. %d, B=%lld, mode=%d, psk_m=%d in 2 .. %d, "
                  "psk_phase=%g, iters=%d in 1 .. %d, tol=%g > 0, or a null pointer)",
                  Nb, Nd, (long long)synth_max_cells(), Le, CRB_MAXL, (long long)B, mode, psk_m, REFINE_MAX_M, psk_phase, iters,
                  REFINE_MAX_ITERS, tol);
        return ADMMNET_E_ARG;
    }
    if (int rc = scene_lds_ok("refine", Nb, Nd, "with Le=", Le, "", refine_lds_bytes(Nb, Nd, Le), refine_lds_limit())) return rc;
    return launch_refine(Nb, Nd, Le, B, (const float2 *)y, (const float2 *)b, rows_in, n_est, mode, psk_m, psk_phase, iters, tol,
                         rows_out, (double2 *)C_out, info, symbols_out, status, (hipStream_t)stream);
}

// ---- the number of targets of a scene selected among candidate rows (order.hip) ----------------------------------------------
// the sizes of the refinement; a thread per pair of rows, the rows taken in a 32-bit mask
int64_t admmnet_order_lds_bytes(int32_t Nb, int32_t Nd, int32_t Le) {
    if (!refine_sizes_ok(Nb, Nd, Le)) return -1;
    return order_lds_bytes(Nb, Nd, Le) <= order_lds_limit() ? order_lds_bytes(Nb, Nd, Le) : -1;
}

int admmnet_order_f64(int32_t Nb, int32_t Nd, int32_t Le, int64_t B, const void *y, const void *b, const double *rows_in,
                      const int32_t *n_cand, const int32_t *n_held, const int32_t *symbols, int32_t psk_m, double psk_phase,
                      double penalty, int32_t max_order, int32_t *perm, int32_t *n_sel, double *rss, double *rows_out, void *C_out,
                      void *residual, double *info, int32_t *status, void *stream) {
    if (!refine_sizes_ok(Nb, Nd, Le) || B < 1 || B > 2147483647 || psk_m < 2 || psk_m > REFINE_MAX_M || !sc_finite(psk_phase) ||
        !(penalty >= 0.0) || !sc_finite(penalty) || max_order < 1 || max_order > Le || !y || !b || !rows_in || !perm || !n_sel ||
        !rss || !rows_out || !C_out || !residual || !info || !status || rows_out == rows_in) {
        set_error("order: bad argument (Nb=%d, Nd=%d with Nb * Nd <= %lld, Le=%d in 1 .. %d, B=%lld, psk_m=%d in 2 .. %d, "
                  "psk_phase=%g, penalty=%g >= 0, max_order=%d in 1 .. Le, a null pointer, or rows_out = rows_in)",
                  Nb, Nd, (long long)synth_max_cells(), Le, CRB_MAXL, (long long)B, psk_m, REFINE_MAX_M, psk_phase, penalty,
                  max_order);
        return ADMMNET_E_ARG;
    }
    if (int rc = scene_lds_ok("order", Nb, Nd, "with Le=", Le, "", order_lds_bytes(Nb, Nd, Le), order_lds_limit())) return rc;
    return launch_order(Nb, Nd, Le, B, (const float2 *)y, (const float2 *)b, rows_in, n_cand, n_held, symbols, psk_m, psk_phase,
                        penalty, max_order, perm, n_sel, rss, rows_out, (double2 *)C_out, (float2 *)residual, info, status,
                        (hipStream_t)stream);
}

// ---- a CFAR detector on the periodogram of a scene (cfar.hip) --------------------------------------------------------------------
static bool cfar_sizes_ok(int32_t Nb, int32_t Nd, int32_t r) {
    return Nb >= 1 && Nd >= 1 && (int64_t)Nb * Nd <= synth_max_cells() && r >= 1 && r <= CFAR_MAX_OVERSAMPLE &&
           (int64_t)Nb * Nd * r * r <= CFAR_MAX_CELLS;
}

int64_t admmnet_cfar_lds_bytes(int32_t Nb, int32_t Nd, int32_t r) {
    if (!cfar_sizes_ok(Nb, Nd, r)) return -1;
    return cfar_lds_bytes(Nb, Nd, r) <= cfar_lds_limit() ? cfar_lds_bytes(Nb, Nd, r) : -1;
}

// the window fits its axis without a training cell counted twice, and holds at least one cell
static bool cfar_window_ok(int32_t Nb, int32_t Nd, int32_t guard, int32_t train) {
    if (guard < 0 || train < 1 || (int64_t)guard + train > CFAR_MAX_REACH) return false;
    const int W = guard + train;
    if ((Nb > 1 && 2 * W + 1 > Nb) || (Nd > 1 && 2 * W + 1 > Nd)) return false;
    return cf_train_count(Nb, Nd, guard, train) >= 1;
}

// what admmnet_cfar_f64 and admmnet_cfar_relax_f64 ask of the arguments they share.  `rest_ok` and `rest` are the checks the entry
// adds (its own values, its pointers) and the text of those values
static int cfar_args_ok(const char *what, int32_t Nb, int32_t Nd, int32_t r, int32_t Le, int64_t B, int32_t psk_m, double psk_phase,
                        int32_t method, int32_t guard, int32_t train, int32_t rank, double alpha, const double *noise_var,
                        bool rest_ok, const char *rest) {
    const bool sizes = cfar_sizes_ok(Nb, Nd, r) && Le >= 1 && Le <= CRB_MAXL;
    const bool method_ok = method == CF_KNOWN || method == CF_CA || method == CF_OS;
    const bool window = sizes && method_ok && (method == CF_KNOWN || cfar_window_ok(Nb, Nd, guard, train));
    const bool rank_ok = window && (method != CF_OS || (rank >= 1 && rank <= cf_train_count(Nb, Nd, guard, train)));
    if (!rank_ok || B < 1 || B > 2147483647 || psk_m < 2 || psk_m > REFINE_MAX_M || !sc_finite(psk_phase) || !(alpha > 0.0) ||
        !sc_finite(alpha) || (method == CF_KNOWN) != (noise_var != nullptr) || !rest_ok) {
        set_error("%s: bad argument (Nb=%d, Nd=%d with Nb * Nd <= %lld, r=%d in 1 .. %d with at most %d map cells, Le=%d in 1 .. %d, "
                  "B=%lld, psk_m=%d in 2 .. %d, psk_phase=%g, method=%d in 0 .. 2, guard=%d >= 0, train=%d >= 1 with guard + train "
                  "<= %d and 2 (guard + train) + 1 <= every axis longer than 1, rank=%d in 1 .. N, alpha=%g > 0, noise_var given "
                  "exactly in method 0, %sor a null pointer)",
                  what, Nb, Nd, (long long)synth_max_cells(), r, CFAR_MAX_OVERSAMPLE, CFAR_MAX_CELLS, Le, CRB_MAXL, (long long)B, psk_m,
                  REFINE_MAX_M, psk_phase, method, guard, train, CFAR_MAX_REACH, rank, alpha, rest);
        return ADMMNET_E_ARG;
    }
    return ADMMNET_OK;
}

int admmnet_cfar_f64(int32_t Nb, int32_t Nd, int32_t r, int32_t Le, int64_t B, const void *y, const void *b, const int32_t *symbols,
                     int32_t psk_m, double psk_phase, int32_t method, int32_t guard, int32_t train, int32_t rank, double alpha,
                     const double *noise_var, double *rows, int32_t *counts, double *info, double *map_out, int32_t *status,
                     void *stream) {
    if (int rc = cfar_args_ok("cfar", Nb, Nd, r, Le, B, psk_m, psk_phase, method, guard, train, rank, alpha, noise_var,
                              y && b && rows && counts && info && status, ""))
        return rc;
    if (int rc = scene_lds_ok("cfar", Nb, Nd, "oversampled ", r, " times", cfar_lds_bytes(Nb, Nd, r), cfar_lds_limit())) return rc;
    return launch_cfar(Nb, Nd, r, Le, B, (const float2 *)y, (const float2 *)b, symbols, psk_m, psk_phase, method, guard, train, rank,
                       alpha, noise_var, rows, counts, info, map_out, status, (hipStream_t)stream);
}

// ---- successive cancellation with cyclic re-fitting on that periodogram (cfar_relax.hip) --------------------------------------------
int64_t admmnet_cfar_relax_lds_bytes(int32_t Nb, int32_t Nd, int32_t r) {
    if (!cfar_sizes_ok(Nb, Nd, r)) return -1;
    return cfar_relax_lds_bytes(Nb, Nd, r) <= cfar_relax_lds_limit() ? cfar_relax_lds_bytes(Nb, Nd, r) : -1;
}

int admmnet_cfar_relax_f64(int32_t Nb, int32_t Nd, int32_t r, int32_t Le, int64_t B, const void *y, const void *b,
                           const int32_t *symbols, int32_t psk_m, double psk_phase, int32_t method, int32_t guard, int32_t train,
                           int32_t rank, double alpha, const double *noise_var, int32_t iters, int32_t sweeps, double *rows, void *amp,
                           int32_t *counts, double *info, double *map_out, int32_t *status, void *stream) {
    char rest[96];
    snprintf(rest, sizeof(rest), "iters=%d in 0 .. %d, sweeps=%d in 0 .. %d, ", iters, RELAX_MAX_ITERS, sweeps, RELAX_MAX_SWEEPS);
    const bool rest_ok = iters >= 0 && iters <= RELAX_MAX_ITERS && sweeps >= 0 && sweeps <= RELAX_MAX_SWEEPS && y && b && rows && amp &&
                         counts && info && status;
    if (int rc = cfar_args_ok("cfar_relax", Nb, Nd, r, Le, B, psk_m, psk_phase, method, guard, train, rank, alpha, noise_var, rest_ok,
                              rest))
        return rc;
    if (int rc = scene_lds_ok("cfar_relax", Nb, Nd, "oversampled ", r, " times", cfar_relax_lds_bytes(Nb, Nd, r), cfar_relax_lds_limit()))
        return rc;
    return launch_cfar_relax(Nb, Nd, r, Le, B, (const float2 *)y, (const float2 *)b, symbols, psk_m, psk_phase, method, guard, train,
                             rank, alpha, noise_var, iters, sweeps, rows, (double *)amp, counts, info, map_out, status,
                             (hipStream_t)stream);
}

// ---- AdamW and gradient-norm clipping over a tensor list (optim.hip) ---------------------------------------------------------
// a pointer may be null only where its tensor has no element
static int optim_args_ok(const char *what, int32_t count, const int64_t *numel, bool ptrs, const void *const *const *lists, int nlists) {
    if (count < 0 || (count > 0 && (!numel || !ptrs))) {
        set_error("%s: bad argument (count=%d, or a null pointer)", what, count);
        return ADMMNET_E_ARG;
    }
    for (int l = 0; l < nlists && count > 0; ++l)
        if (!lists[l]) {
            set_error("%s: pointer list %d is null", what, l);
            return ADMMNET_E_ARG;
        }
    if (optim_blocks(count, numel) < 0) {
        set_error("%s: a negative element count, or more than 2^31 - 1 blocks of 1024 elements in the list", what);
        return ADMMNET_E_ARG;
    }
    for (int i = 0; i < count; ++i)
        for (int l = 0; l < nlists; ++l)
            if (numel[i] > 0 && !lists[l][i]) {
                set_error("%s: tensor %d of pointer list %d is null and has %lld elements", what, i, l, (long long)numel[i]);
                return ADMMNET_E_ARG;
            }
    return ADMMNET_OK;
}

int64_t admmnet_optim_partials(int32_t count, const int64_t *numel) {
    if (count < 0 || (count > 0 && !numel)) return -1;
    return optim_blocks(count, numel);
}

int admmnet_optim_gradnorm_f32(int32_t count, const float *const *grads, const int64_t *numel, float max_norm, double *partials,
                               double *sumsq, float *total_norm, float *coef, void *stream) {
    const void *const *lists[] = {(const void *const *)grads};
    if (int rc = optim_args_ok("optim_gradnorm", count, numel, partials && sumsq && total_norm && coef, lists, 1)) return rc;
    if (count == 0) return ADMMNET_OK;
    return launch_optim_gradnorm(count, grads, numel, max_norm, partials, sumsq, total_norm, coef, (hipStream_t)stream);
}

int admmnet_optim_scale_f32(int32_t count, float *const *grads, const int64_t *numel, const float *coef, void *stream) {
    const void *const *lists[] = {(const void *const *)grads};
    if (int rc = optim_args_ok("optim_scale", count, numel, coef != nullptr, lists, 1)) return rc;
    if (count == 0) return ADMMNET_OK;
    return launch_optim_scale(count, grads, numel, coef, (hipStream_t)stream);
}

int admmnet_optim_adamw_f32(int32_t count, float *const *params, const float *const *grads, float *const *exp_avg,
                            float *const *exp_avg_sq, const int64_t *numel, const int32_t *hyper_index, int32_t nhyper,
                            const admmnet_adamw_hyper *hyper, const float *coef_or_null, void *stream) {
    const void *const *lists[] = {(const void *const *)params, (const void *const *)grads, (const void *const *)exp_avg,
                                  (const void *const *)exp_avg_sq};
    if (int rc = optim_args_ok("optim_adamw", count, numel, hyper_index && hyper && nhyper >= 1, lists, 4)) return rc;
    for (int i = 0; i < count; ++i)
        if (hyper_index[i] < 0 || hyper_index[i] >= nhyper) {
            set_error("optim_adamw: hyper_index[%d] = %d is outside [0, %d)", i, hyper_index[i], nhyper);
            return ADMMNET_E_ARG;
        }
    if (count == 0) return ADMMNET_OK;
    return launch_optim_adamw(count, params, grads, exp_avg, exp_avg_sq, numel, hyper_index, hyper, coef_or_null,
                              (hipStream_t)stream);
}

int admmnet_optim_pack_f32(int32_t count, const float *const *tensors, const int64_t *numel, float *flat, void *stream) {
    const void *const *lists[] = {(const void *const *)tensors};
    if (int rc = optim_args_ok("optim_pack", count, numel, flat != nullptr, lists, 1)) return rc;
    if (count == 0) return ADMMNET_OK;
    return launch_optim_bucket(count, const_cast<float *const *>(tensors), numel, flat, true, (hipStream_t)stream);
}

int admmnet_optim_unpack_f32(int32_t count, float *const *tensors, const int64_t *numel, const float *flat, void *stream) {
    const void *const *lists[] = {(const void *const *)tensors};
    if (int rc = optim_args_ok("optim_unpack", count, numel, flat != nullptr, lists, 1)) return rc;
    if (count == 0) return ADMMNET_OK;
    return launch_optim_bucket(count, tensors, numel, const_cast<float *>(flat), false, (hipStream_t)stream);
}

int admmnet_profile_enable(int32_t on) {
    ProfState &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    p.on = on != 0;
    p.kclass.clear();
    p.dropped = 0;
    return ADMMNET_OK;
}

int64_t admmnet_profile_dropped(void) {
    ProfState &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    return p.dropped;
}

int admmnet_profile_read(double *ms_total, int64_t *launches, int32_t nclasses) {
    if (!ms_total || !launches || nclasses < KC_COUNT) {
        set_error("profile_read: need %d classes", (int)KC_COUNT);
        return ADMMNET_E_ARG;
    }
    for (int i = 0; i < nclasses; ++i) { ms_total[i] = 0.0; launches[i] = 0; }
    ProfState &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    for (size_t i = 0; i < p.kclass.size(); ++i) {
        ADMM_HIP(hipEventSynchronize(p.ev1[i]));
        float ms = 0.f;
        ADMM_HIP(hipEventElapsedTime(&ms, p.ev0[i], p.ev1[i]));
        ms_total[p.kclass[i]] += ms;
        launches[p.kclass[i]] += 1;
    }
    p.kclass.clear();
    return ADMMNET_OK;
}

int64_t admmnet_spectrum_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny) {
    if (xbase < 1 || ybase < 1 || nx < 1 || ny < 1) return -1;
    return align_up(sizeof(double2) * (int64_t)nx * xbase, 256) + align_up(sizeof(double2) * (int64_t)ny * ybase, 256);
}

int admmnet_spectrum_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase, const double *taus,
                         int32_t nx, const double *fs, int32_t ny, double *out, void *workspace,
                         int64_t workspace_bytes, void *stream) {
    const int64_t need = admmnet_spectrum_workspace_bytes(xbase, ybase, nx, ny);
    if (need < 0 || B < 1 || !phi || !taus || !fs || !out || !workspace) {
        set_error("spectrum: bad argument");
        return ADMMNET_E_ARG;
    }
    if (workspace_bytes < need) {
        set_error("spectrum: workspace too small");
        return ADMMNET_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double2 *tabD = (double2 *)workspace;
    double2 *tabS = (double2 *)((char *)workspace + align_up(sizeof(double2) * (int64_t)nx * xbase, 256));
    int rc;
    if ((rc = launch_spectrum_tables(taus, nx, xbase, fs, ny, ybase, tabD, tabS, st))) return rc;
    return launch_spectrum_main((const float2 *)phi, B, xbase, ybase, tabD, nx, tabS, ny, out, st);
}

int64_t admmnet_peak_search_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny, int64_t B) {
    const int64_t t = admmnet_spectrum_workspace_bytes(xbase, ybase, nx, ny);
    if (t < 0 || B < 1) return -1;
    return align_up(t, 256) + align_up((int64_t)sizeof(double) * B * nx * ny, 256);
}

int admmnet_peak_search_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase, const double *axis_x,
                            int32_t nx, const double *axis_y, int32_t ny, const double *opts7, int32_t iters,
                            int32_t max_peaks, double *peaks, int32_t *counts, void *workspace,
                            int64_t workspace_bytes, void *stream) {
    const int64_t need = admmnet_peak_search_workspace_bytes(xbase, ybase, nx, ny, B);
    if (need < 0 || !phi || !axis_x || !axis_y || !opts7 || !peaks || !counts || !workspace || nx < 1 || ny < 1 ||
        iters < 0 || max_peaks < 1) {
        set_error("peak search: bad argument");
        return ADMMNET_E_ARG;
    }
    if (workspace_bytes < need) {
        set_error("peak search: workspace too small");
        return ADMMNET_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t tb = align_up(admmnet_spectrum_workspace_bytes(xbase, ybase, nx, ny), 256);
    double *Z = (double *)((char *)workspace + tb);
    int rc;
    if ((rc = admmnet_spectrum_f64(phi, B, xbase, ybase, axis_x, nx, axis_y, ny, Z, workspace, tb, stream))) return rc;
    return launch_peaks((const float2 *)phi, B, xbase, ybase, Z, nx, ny, axis_x, axis_y, opts7, iters, max_peaks,
                        peaks, counts, st);
}

int64_t admmnet_peak_top_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny) {
    return admmnet_spectrum_workspace_bytes(xbase, ybase, nx, ny);   // the two steering tables
}

int admmnet_peak_top_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase, const double *axis_x, int32_t nx,
                         const double *axis_y, int32_t ny, const double *opts7, int32_t iters, int32_t L,
                         const int32_t *top_n, double *top, int32_t *counts, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    const int64_t need = admmnet_peak_top_workspace_bytes(xbase, ybase, nx, ny);
    if (need < 0 || B < 0 || !phi || !axis_x || !axis_y || !opts7 || !top || !counts || !workspace || nx < 1 || ny < 1 ||
        iters < 0 || L < 1 || L > 64) {
        set_error("peak top: bad argument");
        return ADMMNET_E_ARG;
    }
    if (workspace_bytes < need) {
        set_error("peak top: workspace too small");
        return ADMMNET_E_WORKSPACE;
    }
    // image + phi in double must fit one workgroup's LDS (checked here in 64 bits, exactly in launch_estimate)
    if ((int64_t)nx * ny + 2 * (int64_t)xbase * ybase > 160 * 1024 / 8) {
        set_error("peak top: grid %d x %d (phi %d x %d) does not fit the LDS", nx, ny, xbase, ybase);
        return ADMMNET_E_ARG;
    }
    if (B == 0) return ADMMNET_OK;
    hipStream_t st = (hipStream_t)stream;
    double2 *tabD = (double2 *)workspace;
    double2 *tabS = (double2 *)((char *)workspace + align_up(sizeof(double2) * (int64_t)nx * xbase, 256));
    int rc;
    if ((rc = launch_spectrum_tables(axis_x, nx, xbase, axis_y, ny, ybase, tabD, tabS, st))) return rc;
    return launch_estimate((const float2 *)phi, B, xbase, ybase, tabD, nx, tabS, ny, axis_x, axis_y, opts7, iters, L,
                           top_n, top, counts, st);
}

int admmnet_regional_maxima_f64(const double *Z, int64_t B, int32_t nx, int32_t ny, int32_t max_peaks,
                                double *peaks, int32_t *counts, void *stream) {
    if (!Z || B < 1 || nx < 1 || ny < 1 || max_peaks < 1 || !peaks || !counts) {
        set_error("regional maxima: bad argument");
        return ADMMNET_E_ARG;
    }
    const double o7[7] = {0, 0, 0, 0, 0, 0, 0};
    // the maxima stage of the peak-search kernel alone: no phi, no axes (positions = pixel column / row), no rounds
    return launch_peaks(nullptr, B, 1, 1, Z, nx, ny, nullptr, nullptr, o7, 0, max_peaks, peaks, counts,
                        (hipStream_t)stream);
}

int admmnet_synth_batch(int64_t B, int32_t Nb, int32_t Nd, int32_t L, uint64_t seed, double snr_lo, double snr_hi,
                        double snr_e, double rho, int32_t label_iters, void *y, void *b, float *sigma, float *tau, float *f,
                        void *C, void *phi_label, void *stream) {
    // (launch_synth refuses an Nb * Nd whose three float64 arrays do not fit the LDS)
    if (B < 1 || B > 2147483647 || Nb < 1 || Nd < 1 || L < 1 || L > 8 || !y || !b || !sigma || !tau || !f || !C ||
        label_iters < 0) {
        set_error("synth_batch: bad argument");
        return ADMMNET_E_ARG;
    }
    return launch_synth(B, Nb, Nd, L, seed, snr_lo, snr_hi, snr_e, rho, label_iters, (float2 *)y, (float2 *)b, sigma, tau,
                        f, (float2 *)C, (float2 *)phi_label, (hipStream_t)stream);
}

int admmnet_synth_scenes(int64_t B, int32_t Nb, int32_t Nd, int32_t L_min, int32_t L_max, double min_sep, uint64_t seed,
                         double snr_lo, double snr_hi, double snr_e, double rho, int32_t label_iters, void *y, void *b,
                         float *sigma, float *tau, float *f, void *C, void *phi_label, int64_t *L_true, double *snr_db,
                         double *noise_var, float *ser, int32_t *state, void *stream) {
    // (launch_synth_scenes refuses an Nb * Nd whose three float64 arrays do not fit the LDS)
    if (B < 1 || B > 2147483647 || Nb < 1 || Nd < 1 || L_min < 1 || L_max > 8 || L_min > L_max || !(min_sep >= 0.0) ||
        !__builtin_isfinite(min_sep) || label_iters < 0 || !y || !b || !sigma || !tau || !f || !C || !L_true || !snr_db ||
        !noise_var || !ser || !state) {
        set_error("synth_scenes: needs 1 <= B < 2^31, Nb, Nd >= 1, 1 <= L_min <= L_max <= 8, a finite min_sep >= 0, label_iters "
                  ">= 0 and every output but phi_label (got B %lld, grid %d x %d, targets %d .. %d, min_sep %g, label_iters %d)",
                  (long long)B, Nb, Nd, L_min, L_max, min_sep, label_iters);
        return ADMMNET_E_ARG;
    }
    return launch_synth_scenes(B, Nb, Nd, L_min, L_max, min_sep, seed, snr_lo, snr_hi, snr_e, rho, label_iters, (float2 *)y,
                               (float2 *)b, sigma, tau, f, (float2 *)C, (float2 *)phi_label, L_true, snr_db, noise_var, ser,
                               state, (hipStream_t)stream);
}

}  // extern "C"
