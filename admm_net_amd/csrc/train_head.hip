// train_head.hip -- the PeakSearchLayer head of one TRAINING step, forward and hand-written backward, for train_route = "native" of
// admm_net_amd/training.py (admm_net.py:570-630; head.hip is the same forward for inference on packed weights).  The kernels read
// the RAW parameters through a pointer table (HeadPtrs, the order of training._head_params) and return raw-parameter gradients.
//   forward   hd_kv_kernel     the batch-independent position tokens P = position_projection(position_encoder) [D][128] and their
//                              K / V projections (the K and V slices of in_proj), one workgroup per token;
//             hd_fwd_kernel    one 128-thread workgroup per signal: feature_extractor, q = (Wq x + bq) / sqrt(32) (scaled before
//                              the product, as torch does), four heads' softmax over the D tokens, the optional keep mask
//                              a <- a keep / (1 - p) between the softmax and the value product, out_proj, the residual,
//                              peak_extractor, and per target t the two regressors and confidence_net on xp + t / L (a float32
//                              constant).  It saves x1, x, q, a (before the mask), ctx, xf, u0, u1, xp and the regressors' hidden
//                              layers: 4 D + 752 + 80 L floats per signal.
//   backward  hd_bwd_kernel    per signal: g_phi and the pre-activation delta of every linear layer (relu'(0) = 0), the masked
//                              weights a' and the score gradients g_s;
//             bp_kernel        every weight gradient as a batch-reduced product C[m][n] = sum_b A[b][m] Bm[b][n] with a ones
//                              column appended for the bias (batch_product.h: the MFMA loop, the slabs and their float64 sums
//                              are defined there); the token side's gV_h[d] = sum_b a'_bhd g_ctx_bh and gK_h[d] = sum_b g_s_bhd q_bh
//                              are products of the same launch.  hb_sum_kernel adds the slabs.  confidence_net is shared over
//                              t: its batch is the B L (signal, target) pairs.
//             hd_token_kernel  gK, gV [D][128] through the K and V slices of in_proj to g_P, and g_P through position_projection
//                              to the gradient of the position_encoder parameter; a second bp_kernel launch with the D tokens as
//                              the batch gives gWk, gbk (= sum_d gK), gWv, gbv, gWp, gbp.
// The descriptors of the products are not stored: hb_desc evaluates descriptor i from the sizes and the buffers' base pointers,
// on the host to count tiles and in every wave to find its own.
#include "common.h"
#include "batch_product.h"
#include "slab_partials.h"
#include "train_math.h"

namespace admmnet {

constexpr int HDIM = 128;             // hidden_dim = threads of the per-signal workgroup
constexpr int HD_HEADS = 4;
constexpr int HD_DH = 32;           // head dim
constexpr int HD_MAXL = 16;
constexpr int HD_RH = 80;           // hidden units of one target: 32 tau, 32 f, 16 confidence
constexpr float HD_SCALE = 0.17677669529663687f;   // 1 / sqrt(32)

enum { P_POS = 0, P_FE0W, P_FE0B, P_FE2W, P_FE2B, P_PPW, P_PPB, P_INW, P_INB, P_OUTW, P_OUTB, P_PE0W, P_PE0B, P_PE2W, P_PE2B,
       P_PE4W, P_PE4B, P_C0W, P_C0B, P_C2W, P_C2B, P_REG };   // then per target: tau w0, b0, w2, b2, f w0, b0, w2, b2

struct HeadPtrs {
    const float *p[P_REG + 8 * HD_MAXL];
};

// the saved activations of the forward
struct HeadSaved {
    float *x1, *x, *q, *a, *ctx, *xf, *u0, *u1, *xp, *hid, *P, *K, *V;
    __host__ __device__ HeadSaved(float *c, int D, int L, int64_t B) {
        x1 = c, c += B * HDIM;
        x = c, c += B * HDIM;
        q = c, c += B * HDIM;
        ctx = c, c += B * HDIM;
        xf = c, c += B * HDIM;
        u0 = c, c += B * 64;
        u1 = c, c += B * 32;
        xp = c, c += B * 16;
        a = c, c += B * HD_HEADS * D;
        hid = c, c += B * L * HD_RH;
        P = c, c += (int64_t)D * HDIM;
        K = c, c += (int64_t)D * HDIM;
        V = c;
    }
    static __host__ __device__ int64_t floats(int D, int L, int64_t B) {
        return B * (4 * D + 752 + HD_RH * L) + (int64_t)3 * D * HDIM;
    }
};

// the gradient buffer: [confidence_net | region A | Wk Wv | bq bk bv | ppw ppb | position_encoder].  Region A's partial row ends
// with Wq and bq; the sum moves bq behind Wv so that in_proj_weight and in_proj_bias come out contiguous.
struct HeadGrad {
    int64_t fe0w, fe0b, fe2w, fe2b, outw, outb, pe0w, pe0b, pe2w, pe2b, pe4w, pe4b, reg, gk, gv, wq, bq;   // within region A
    int64_t TA, TB, TC, oA, oC, opos, total;
    __host__ __device__ HeadGrad(int D, int L) {
        int64_t e = 0;
        fe0w = e, e += (int64_t)HDIM * 2 * D;
        fe0b = e, e += HDIM;
        fe2w = e, e += HDIM * HDIM;
        fe2b = e, e += HDIM;
        outw = e, e += HDIM * HDIM;
        outb = e, e += HDIM;
        pe0w = e, e += 64 * HDIM;
        pe0b = e, e += 64;
        pe2w = e, e += 32 * 64;
        pe2b = e, e += 32;
        pe4w = e, e += 16 * 32;
        pe4b = e, e += 16;
        reg = e, e += (int64_t)1154 * L;   // per target: [tau w0 | f w0] 1024, [tau b0 | f b0] 64, tau w2 32, b2 1, f w2 32, b2 1
        gk = e, e += (int64_t)D * HDIM;
        gv = e, e += (int64_t)D * HDIM;
        wq = e, e += HDIM * HDIM;
        bq = e, e += HDIM;
        TA = e;
        TB = 289;                          // c0w 256, c0b 16, c2w 16, c2b 1
        TC = 2 * HDIM * HDIM + 2 * HDIM + 2 * HDIM + HDIM;   // Wk, Wv, bk, bv, ppw, ppb
        oA = TB;
        oC = oA + bq;                      // Wk follows Wq
        opos = oC + TC + HDIM;
        total = opos + 2 * D;
    }
};

// the backward's scratch: deltas per signal, g_P, the slab partials
struct HeadWork {
    float *dhid, *dout, *z, *d4, *d2, *d0, *gxf, *gctx, *am, *gs, *dq, *dp2, *dp1, *gP, *partA, *partB, *partC;
    static __host__ __device__ int64_t slabs(int64_t nb) { return bp_slabs(nb); }
    __host__ __device__ HeadWork(float *c, int D, int L, int64_t B) {
        const HeadGrad G(D, L);
        dhid = c, c += B * L * HD_RH;
        dout = c, c += B * L * 3;
        z = c, c += B * L * 16;
        d4 = c, c += B * 16;
        d2 = c, c += B * 32;
        d0 = c, c += B * 64;
        gxf = c, c += B * HDIM;
        gctx = c, c += B * HDIM;
        dq = c, c += B * HDIM;
        dp2 = c, c += B * HDIM;
        dp1 = c, c += B * HDIM;
        am = c, c += B * HD_HEADS * D;
        gs = c, c += B * HD_HEADS * D;
        gP = c, c += (int64_t)D * HDIM;
        partA = c, c += slabs(B) * G.TA;
        partB = c, c += slabs(B * L) * G.TB;
        partC = c, c += slabs(D) * G.TC;
        end = c;
    }
    float *end;
    static __host__ int64_t floats(int D, int L, int64_t B) {
        float *const base = reinterpret_cast<float *>(uintptr_t(4096));   // only the distances matter
        return (int64_t)(HeadWork(base, D, L, B).end - base);
    }
};

__device__ __forceinline__ float hd_offset(int t, int L) { return (float)((double)t / (double)L); }

// ---- forward -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HDIM) void hd_kv_kernel(int D, int L, int64_t B, HeadPtrs hp, float *saved) {
    __shared__ float pos[HDIM];
    const HeadSaved S(saved, D, L, B);
    const int t = blockIdx.x, o = threadIdx.x;
    const float p0 = hp.p[P_POS][2 * t], p1 = hp.p[P_POS][2 * t + 1];
    const float v = fmaf(hp.p[P_PPW][2 * o], p0, fmaf(hp.p[P_PPW][2 * o + 1], p1, hp.p[P_PPB][o]));
    pos[o] = v;
    S.P[(int64_t)t * HDIM + o] = v;
    __syncthreads();
    const float *inw = hp.p[P_INW], *inb = hp.p[P_INB];
    S.K[(int64_t)t * HDIM + o] = dot4(inw + (int64_t)(HDIM + o) * HDIM, 1, pos, HDIM) + inb[HDIM + o];
    S.V[(int64_t)t * HDIM + o] = dot4(inw + (int64_t)(2 * HDIM + o) * HDIM, 1, pos, HDIM) + inb[2 * HDIM + o];
}

// keep: [B][4][D] bytes or nullptr; inv = 1 / (1 - p)
__global__ __launch_bounds__(HDIM) void hd_fwd_kernel(int D, int L, int64_t B, HeadPtrs hp, const float2 *__restrict__ phi,
                                                    const unsigned char *__restrict__ keep, float inv, float *saved,
                                                    float *__restrict__ tau, float *__restrict__ f, float *__restrict__ conf) {
    __shared__ float feat[2 * kMaxD], sc[HD_HEADS * kMaxD], va[HDIM], vb[HDIM], red[HD_HEADS], hid[HD_RH];
    const HeadSaved S(saved, D, L, B);
    const int o = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = o; i < D; i += HDIM) {
        const float2 p = phi[b * D + i];
        feat[i] = p.x;
        feat[D + i] = p.y;
    }
    __syncthreads();
    const float x1 = fmaxf(dot4(hp.p[P_FE0W] + (int64_t)o * 2 * D, 1, feat, 2 * D) + hp.p[P_FE0B][o], 0.f);
    va[o] = x1;
    S.x1[b * HDIM + o] = x1;
    __syncthreads();
    const float x = fmaxf(dot4(hp.p[P_FE2W] + (int64_t)o * HDIM, 1, va, HDIM) + hp.p[P_FE2B][o], 0.f);
    vb[o] = x;
    S.x[b * HDIM + o] = x;
    __syncthreads();
    const float q = (dot4(hp.p[P_INW] + (int64_t)o * HDIM, 1, vb, HDIM) + hp.p[P_INB][o]) * HD_SCALE;
    va[o] = q;
    S.q[b * HDIM + o] = q;
    __syncthreads();
    for (int p = o; p < HD_HEADS * D; p += HDIM) {
        const int hh = p / D, t = p - hh * D;
        const float *kr = S.K + (int64_t)t * HDIM + hh * HD_DH;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < HD_DH; ++j) a = fmaf(va[hh * HD_DH + j], kr[j], a);
        sc[p] = a;
    }
    __syncthreads();
    {   // softmax per head: wave w takes the heads w, w + 2
        const int lane = o & 63, wave = o >> 6;
        for (int hh = wave; hh < HD_HEADS; hh += HDIM / 64) {
            float m = -INFINITY;
            for (int t = lane; t < D; t += 64) m = fmaxf(m, sc[hh * D + t]);
            m = wave_max(m);
            float ssum = 0.f;
            for (int t = lane; t < D; t += 64) {
                const float e = expf(sc[hh * D + t] - m);
                sc[hh * D + t] = e;
                ssum += e;
            }
            ssum = wave_sum(ssum);
            if (lane == 0) red[hh] = ssum;
        }
    }
    __syncthreads();
    for (int p = o; p < HD_HEADS * D; p += HDIM) {
        const float a = sc[p] / red[p / D];
        S.a[b * HD_HEADS * D + p] = a;
        sc[p] = keep ? (keep[b * HD_HEADS * D + p] ? a * inv : 0.f) : a;
    }
    __syncthreads();
    {
        const int hh = o / HD_DH;
        float a = 0.f;
        for (int t = 0; t < D; ++t) a = fmaf(sc[hh * D + t], S.V[(int64_t)t * HDIM + o], a);
        va[o] = a;
        S.ctx[b * HDIM + o] = a;
    }
    __syncthreads();
    const float xf = x + (dot4(hp.p[P_OUTW] + (int64_t)o * HDIM, 1, va, HDIM) + hp.p[P_OUTB][o]);
    vb[o] = xf;
    S.xf[b * HDIM + o] = xf;
    __syncthreads();
    if (o < 64) {
        const float u = fmaxf(dot4(hp.p[P_PE0W] + (int64_t)o * HDIM, 1, vb, HDIM) + hp.p[P_PE0B][o], 0.f);
        va[o] = u;
        S.u0[b * 64 + o] = u;
    }
    __syncthreads();
    if (o < 32) {
        const float u = fmaxf(dot4(hp.p[P_PE2W] + (int64_t)o * 64, 1, va, 64) + hp.p[P_PE2B][o], 0.f);
        vb[o] = u;
        S.u1[b * 32 + o] = u;
    }
    __syncthreads();
    if (o < 16) {
        const float u = fmaxf(dot4(hp.p[P_PE4W] + (int64_t)o * 32, 1, vb, 32) + hp.p[P_PE4B][o], 0.f);
        va[o] = u;   // xp
        S.xp[b * 16 + o] = u;
    }
    __syncthreads();
    for (int t = 0; t < L; ++t) {
        const float off = hd_offset(t, L);
        const int r = P_REG + 8 * t;
        if (o < HD_RH) {   // hidden layers on z = xp + t / L: threads 0 .. 31 tau, 32 .. 63 f, 64 .. 79 confidence
            const float *w = o < 32 ? hp.p[r] + o * 16 : (o < 64 ? hp.p[r + 4] + (o - 32) * 16 : hp.p[P_C0W] + (o - 64) * 16);
            float a = o < 32 ? hp.p[r + 1][o] : (o < 64 ? hp.p[r + 5][o - 32] : hp.p[P_C0B][o - 64]);
#pragma unroll
            for (int i = 0; i < 16; ++i) a = fmaf(w[i], va[i] + off, a);
            a = fmaxf(a, 0.f);
            hid[o] = a;
            S.hid[(b * L + t) * HD_RH + o] = a;
        }
        __syncthreads();
        if (o < 3) {
            const float *w2 = o == 0 ? hp.p[r + 2] : (o == 1 ? hp.p[r + 6] : hp.p[P_C2W]);
            const float *hs = hid + 32 * o;
            const int nh = o < 2 ? 32 : 16;
            float a = o == 0 ? hp.p[r + 3][0] : (o == 1 ? hp.p[r + 7][0] : hp.p[P_C2B][0]);
            for (int j = 0; j < nh; ++j) a = fmaf(w2[j], hs[j], a);
            if (o == 0) tau[b * L + t] = sigmoid_f(a);
            else if (o == 1) f[b * L + t] = tanhf(a);
            else conf[b * L + t] = sigmoid_f(a);
        }
        __syncthreads();
    }
}

// ---- backward, per signal ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HDIM) void hd_bwd_kernel(int D, int L, int64_t B, HeadPtrs hp, const float *__restrict__ gtau,
                                                    const float *__restrict__ gf, const float *__restrict__ gconf,
                                                    const float *__restrict__ tau, const float *__restrict__ f,
                                                    const float *__restrict__ conf, const unsigned char *__restrict__ keep,
                                                    float inv, float *saved, float *work, float2 *__restrict__ gphi) {
    __shared__ float sa[HD_HEADS * kMaxD], sg[HD_HEADS * kMaxD], va[HDIM], vb[HDIM], vc[HDIM], red[HD_HEADS], dh[HD_RH], dd[4], xp[16];
    const HeadSaved S(saved, D, L, B);
    const HeadWork W(work, D, L, B);
    const int o = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (o < 16) xp[o] = S.xp[b * 16 + o];
    __syncthreads();
    // the regressors and confidence_net of every target: deltas of their two layers, g_xp summed over the targets
    float gxp = 0.f;
    for (int t = 0; t < L; ++t) {
        const int r = P_REG + 8 * t;
        const int64_t bt = b * L + t;
        if (o < 3) {
            float d;
            if (o == 0) { const float v = tau[bt]; d = gtau[bt] * v * (1.f - v); }
            else if (o == 1) { const float v = f[bt]; d = gf[bt] * (1.f - v * v); }
            else { const float v = conf[bt]; d = gconf[bt] * v * (1.f - v); }
            dd[o] = d;
            W.dout[bt * 3 + o] = d;
        }
        if (o < 16) W.z[bt * 16 + o] = xp[o] + hd_offset(t, L);
        __syncthreads();
        if (o < HD_RH) {
            const float w2 = o < 32 ? hp.p[r + 2][o] : (o < 64 ? hp.p[r + 6][o - 32] : hp.p[P_C2W][o - 64]);
            const float d = S.hid[bt * HD_RH + o] > 0.f ? dd[o < 32 ? 0 : (o < 64 ? 1 : 2)] * w2 : 0.f;
            dh[o] = d;
            W.dhid[bt * HD_RH + o] = d;
        }
        __syncthreads();
        if (o < 16)
            gxp += dot4(hp.p[r] + o, 16, dh, 32) + dot4(hp.p[r + 4] + o, 16, dh + 32, 32) + dot4(hp.p[P_C0W] + o, 16, dh + 64, 16);
        __syncthreads();
    }
    // peak_extractor
    if (o < 16) {
        const float d = xp[o] > 0.f ? gxp : 0.f;
        va[o] = d;
        W.d4[b * 16 + o] = d;
    }
    __syncthreads();
    if (o < 32) {
        const float d = S.u1[b * 32 + o] > 0.f ? dot4(hp.p[P_PE4W] + o, 32, va, 16) : 0.f;
        vb[o] = d;
        W.d2[b * 32 + o] = d;
    }
    __syncthreads();
    if (o < 64) {
        const float d = S.u0[b * 64 + o] > 0.f ? dot4(hp.p[P_PE2W] + o, 64, vb, 32) : 0.f;
        va[o] = d;
        W.d0[b * 64 + o] = d;
    }
    __syncthreads();
    const float gxf = dot4(hp.p[P_PE0W] + o, HDIM, va, 64);   // also the delta of out_proj and the residual's gradient of x
    vc[o] = gxf;
    W.gxf[b * HDIM + o] = gxf;
    __syncthreads();
    const float gctx = dot4(hp.p[P_OUTW] + o, HDIM, vc, HDIM);
    vb[o] = gctx;
    W.gctx[b * HDIM + o] = gctx;
    __syncthreads();
    // the value product, the mask and the softmax
    for (int p = o; p < HD_HEADS * D; p += HDIM) {
        const int hh = p / D, t = p - hh * D;
        const float *vr = S.V + (int64_t)t * HDIM + hh * HD_DH;
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < HD_DH; ++j) g = fmaf(vb[hh * HD_DH + j], vr[j], g);
        const float a = S.a[b * HD_HEADS * D + p];
        const float km = keep ? (keep[b * HD_HEADS * D + p] ? inv : 0.f) : 1.f;
        W.am[b * HD_HEADS * D + p] = a * km;
        sa[p] = a;
        sg[p] = g * km;
    }
    __syncthreads();
    {
        const int lane = o & 63, wave = o >> 6;
        for (int hh = wave; hh < HD_HEADS; hh += HDIM / 64) {
            float s = 0.f;
            for (int t = lane; t < D; t += 64) s = fmaf(sa[hh * D + t], sg[hh * D + t], s);
            s = wave_sum(s);
            if (lane == 0) red[hh] = s;
        }
    }
    __syncthreads();
    for (int p = o; p < HD_HEADS * D; p += HDIM) {
        const float g = sa[p] * (sg[p] - red[p / D]);
        sg[p] = g;
        W.gs[b * HD_HEADS * D + p] = g;
    }
    __syncthreads();
    {
        const int hh = o / HD_DH;
        float a = 0.f;
        for (int t = 0; t < D; ++t) a = fmaf(sg[hh * D + t], S.K[(int64_t)t * HDIM + o], a);
        a *= HD_SCALE;
        va[o] = a;
        W.dq[b * HDIM + o] = a;
    }
    __syncthreads();
    // q, the residual and feature_extractor
    const float gx = gxf + dot4(hp.p[P_INW] + o, HDIM, va, HDIM);
    const float dp2 = S.x[b * HDIM + o] > 0.f ? gx : 0.f;
    vb[o] = dp2;
    W.dp2[b * HDIM + o] = dp2;
    __syncthreads();
    const float dp1 = S.x1[b * HDIM + o] > 0.f ? dot4(hp.p[P_FE2W] + o, HDIM, vb, HDIM) : 0.f;
    vc[o] = dp1;
    W.dp1[b * HDIM + o] = dp1;
    __syncthreads();
    for (int i = o; i < D; i += HDIM)
        gphi[b * D + i] = make_float2(dot4(hp.p[P_FE0W] + i, 2 * D, vc, HDIM), dot4(hp.p[P_FE0W] + D + i, 2 * D, vc, HDIM));
}

// g_P[d] = gK[d] Wk + gV[d] Wv, g_pos[d] = g_P[d] Wp; one workgroup per token.  g: the gradient buffer (gK, gV summed in it)
__global__ __launch_bounds__(HDIM) void hd_token_kernel(int D, int L, int64_t B, HeadPtrs hp, float *work, float *g) {
    __shared__ float sk[HDIM], sv[HDIM], sp[HDIM];
    const HeadWork W(work, D, L, B);
    const HeadGrad G(D, L);
    const int d = blockIdx.x, o = threadIdx.x;
    sk[o] = g[G.oA + G.gk + (int64_t)d * HDIM + o];
    sv[o] = g[G.oA + G.gv + (int64_t)d * HDIM + o];
    __syncthreads();
    const float *inw = hp.p[P_INW];
    const float gp = dot4(inw + (int64_t)HDIM * HDIM + o, HDIM, sk, HDIM) + dot4(inw + (int64_t)2 * HDIM * HDIM + o, HDIM, sv, HDIM);
    sp[o] = gp;
    W.gP[(int64_t)d * HDIM + o] = gp;
    __syncthreads();
    if (o < 2) g[G.opos + 2 * d + o] = dot4(hp.p[P_PPW] + o, 2, sp, HDIM);
}

// ---- batch-reduced products --------------------------------------------------------------------------------------------------
struct HbCtx {
    int D, L;
    int64_t B;
    const float *phi, *pos;
    float *saved, *work, *g;
};

// phase 0: the batch sums over the signals (and the (signal, target) pairs); phase 1: over the tokens
__host__ __device__ inline int hb_count(const HbCtx &c, int phase) { return phase == 0 ? 16 + 3 * c.L + 2 : 3; }

__host__ __device__ inline BpDesc hb_desc(const HbCtx &c, int phase, int i) {
    const HeadSaved S(c.saved, c.D, c.L, c.B);
    const HeadWork W(c.work, c.D, c.L, c.B);
    const HeadGrad G(c.D, c.L);
    const int D = c.D, L = c.L;
    BpDesc d;
    d.cs = 1, d.nb = c.B, d.part = W.partA, d.pstride = G.TA, d.boff = -1;
    auto set = [&](const float *A, int M, int lda, const float *Bm, int N, int ldb, int64_t off, int64_t boff) {
        d.A = A, d.M = M, d.lda = lda, d.Bm = Bm, d.N = N, d.ldb = ldb, d.ldc = N, d.off = off, d.boff = boff;
    };
    if (phase == 1) {
        d.nb = D, d.part = W.partC, d.pstride = G.TC;
        if (i == 0) set(c.g + G.oA + G.gk, HDIM, HDIM, S.P, HDIM, HDIM, 0, 2 * HDIM * HDIM);
        else if (i == 1) set(c.g + G.oA + G.gv, HDIM, HDIM, S.P, HDIM, HDIM, HDIM * HDIM, 2 * HDIM * HDIM + HDIM);
        else set(W.gP, HDIM, HDIM, c.pos, 2, 2, 2 * HDIM * HDIM + 2 * HDIM, 2 * HDIM * HDIM + 4 * HDIM);
        return d;
    }
    if (i == 0) {
        set(W.dp1, HDIM, HDIM, c.phi, D, 2 * D, G.fe0w, G.fe0b);          // real parts: columns 0 .. D - 1 of fe0w
        d.cs = 2, d.ldc = 2 * D;
    } else if (i == 1) {
        set(W.dp1, HDIM, HDIM, c.phi + 1, D, 2 * D, G.fe0w + D, -1);      // imaginary parts: columns D .. 2 D - 1
        d.cs = 2, d.ldc = 2 * D;
    } else if (i == 2) set(W.dp2, HDIM, HDIM, S.x1, HDIM, HDIM, G.fe2w, G.fe2b);
    else if (i == 3) set(W.gxf, HDIM, HDIM, S.ctx, HDIM, HDIM, G.outw, G.outb);
    else if (i == 4) set(W.d0, 64, 64, S.xf, HDIM, HDIM, G.pe0w, G.pe0b);
    else if (i == 5) set(W.d2, 32, 32, S.u0, 64, 64, G.pe2w, G.pe2b);
    else if (i == 6) set(W.d4, 16, 16, S.u1, 32, 32, G.pe4w, G.pe4b);
    else if (i == 7) set(W.dq, HDIM, HDIM, S.x, HDIM, HDIM, G.wq, G.bq);
    else if (i < 12) {
        const int h = i - 8;                                          // gK_h[d] = sum_b g_s_bhd q_bh (q carries 1 / sqrt(32))
        set(W.gs + h * D, D, HD_HEADS * D, S.q + HD_DH * h, HD_DH, HDIM, G.gk + HD_DH * h, -1);
        d.ldc = HDIM;
    } else if (i < 16) {
        const int h = i - 12;                                         // gV_h[d] = sum_b a'_bhd g_ctx_bh
        set(W.am + h * D, D, HD_HEADS * D, W.gctx + HD_DH * h, HD_DH, HDIM, G.gv + HD_DH * h, -1);
        d.ldc = HDIM;
    } else if (i < 16 + 3 * L) {
        const int t = (i - 16) / 3, k = (i - 16) % 3;
        const int64_t r = G.reg + (int64_t)1154 * t;
        if (k == 0) set(W.dhid + HD_RH * t, 64, HD_RH * L, W.z + 16 * t, 16, 16 * L, r, r + 1024);
        else if (k == 1) set(W.dout + 3 * t, 1, 3 * L, S.hid + HD_RH * t, 32, HD_RH * L, r + 1088, r + 1120);
        else set(W.dout + 3 * t + 1, 1, 3 * L, S.hid + HD_RH * t + 32, 32, HD_RH * L, r + 1121, r + 1153);
    } else {
        d.nb = c.B * L, d.part = W.partB, d.pstride = G.TB;           // confidence_net: summed over the targets as well
        if (i == 16 + 3 * L) set(W.dhid + 64, 16, HD_RH, W.z, 16, 16, 0, 256);
        else set(W.dout + 2, 1, 3, S.hid + 64, 16, HD_RH, 272, 288);
    }
    return d;
}

struct HbTable {
    HbCtx c;
    int phase;
    __host__ __device__ int count() const { return hb_count(c, phase); }
    __host__ __device__ BpDesc desc(int i) const { return hb_desc(c, phase, i); }
};

// up to two regions of slab sums per launch
__global__ __launch_bounds__(TS_THREADS) void hb_sum_kernel(BpRegion r0, BpRegion r1, float *__restrict__ out) {
    bp_sum_regions((int64_t)blockIdx.x * TS_THREADS + threadIdx.x, r0, r1, out);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int64_t train_head_saved_floats(int D, int L, int64_t B) { return HeadSaved::floats(D, L, B); }
int64_t train_head_work_floats(int D, int L, int64_t B) { return HeadWork::floats(D, L, B); }
int64_t train_head_grad_floats(int D, int L) { return HeadGrad(D, L).total; }

static HeadPtrs head_ptrs(int L, const float *const *params) {
    HeadPtrs hp;
    for (int i = 0; i < P_REG + 8 * HD_MAXL; ++i) hp.p[i] = i < P_REG + 8 * L ? params[i] : nullptr;
    return hp;
}

int launch_train_head(int D, int L, int64_t B, const float2 *phi, const float *const *params, const unsigned char *keep, float p,
                      float *tau, float *f, float *conf, float *saved, hipStream_t st) {
    const HeadPtrs hp = head_ptrs(L, params);
    hipLaunchKernelGGL(hd_kv_kernel, dim3(D), dim3(HDIM), 0, st, D, L, B, hp, saved);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(hd_fwd_kernel, dim3((unsigned)B), dim3(HDIM), 0, st, D, L, B, hp, phi, keep, 1.f / (1.f - p), saved, tau, f,
                       conf);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

int launch_train_head_bwd(int D, int L, int64_t B, const float *gtau, const float *gf, const float *gconf, const float2 *phi,
                          const float *const *params, const unsigned char *keep, float p, const float *tau, const float *f,
                          const float *conf, float *saved, float2 *gphi, float *g, float *work, hipStream_t st) {
    const HeadPtrs hp = head_ptrs(L, params);
    const HeadGrad G(D, L);
    const HeadWork W(work, D, L, B);
    hipLaunchKernelGGL(hd_bwd_kernel, dim3((unsigned)B), dim3(HDIM), 0, st, D, L, B, hp, gtau, gf, gconf, tau, f, conf, keep,
                       1.f / (1.f - p), saved, work, gphi);
    ADMM_HIP(hipGetLastError());
    const HbCtx c{D, L, B, reinterpret_cast<const float *>(phi), params[P_POS], saved, work, g};
    const HbTable tab0{c, 0}, tab1{c, 1};
    hipLaunchKernelGGL(bp_kernel<HbTable>, dim3((unsigned)bp_tiles(tab0), (unsigned)HeadWork::slabs(B * L)), dim3(64), 0, st, tab0);
    ADMM_HIP(hipGetLastError());
    const BpRegion rB{W.partB, G.TB, HeadWork::slabs(B * L), 0, G.TB, 0};
    const BpRegion rA{W.partA, G.TA, HeadWork::slabs(B), G.oA, G.bq, 2 * HDIM * HDIM};   // bq goes behind Wk and Wv
    hipLaunchKernelGGL(hb_sum_kernel, dim3((unsigned)((G.TA + G.TB + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, rB, rA,
                       g);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(hd_token_kernel, dim3(D), dim3(HDIM), 0, st, D, L, B, hp, work, g);
    ADMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(bp_kernel<HbTable>, dim3((unsigned)bp_tiles(tab1), (unsigned)HeadWork::slabs(D)), dim3(64), 0, st, tab1);
    ADMM_HIP(hipGetLastError());
    const BpRegion rC{W.partC, G.TC, HeadWork::slabs(D), G.oC, 2 * HDIM * HDIM, HDIM};     // bk, bv follow bq
    const BpRegion none{nullptr, 0, 0, 0, 0, 0};
    hipLaunchKernelGGL(hb_sum_kernel, dim3((unsigned)((G.TC + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, rC, none, g);
    ADMM_HIP(hipGetLastError());
    return ADMMNET_OK;
}

}  // namespace admmnet
