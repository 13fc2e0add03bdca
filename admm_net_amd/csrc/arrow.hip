// arrow.hip -- first G-layer (Z = 0): direct eigensolver for the Hermitian arrowhead
//     A = C = [[diag h, phi], [phi^H, corner]]          (/root/reference/admm_net.py:273-288)
// fused with the rebuild G = V f(Lambda) V^H + ||G - C||_F (admm_net.py:303-354, 400-403, 454), D <= 128.
//
// The dense path (tridiagonalise, divide & conquer, back-transform) costs O(n^3) per matrix; an
// arrowhead's eigenpairs follow from one secular equation in O(n^2) (arrow_core.h).  One 256-thread
// workgroup per matrix:
//   P1 sort h (rank counting), |phi| and phases          P5 zeta-hat (Loewner), ranks of all eigenvalues
//   P2 deflation scan (one thread, as in the D&C merge)  P6 norms, eigenvalue map f(lambda)
//   P4 secular roots, one thread per root                P7 eigenvectors written straight into LDS as VT[c][rho]
//   P8 deflation rotations undone, phases applied        then rebuild_from_lds (shared with backrebuild.hip)
// V never exists in memory; the only HBM traffic is phi, h in and G out.
//
// 128 < D <= 256 (AR_FUSED): the image does not fit the LDS, and it is not needed.  With p_i = phi_i / |phi_i| every
// eigenvector is V[i][c] = p_i X[c][i] with X REAL, so G_ij = p_i conj(p_j) S_ij with S = X^T diag(f) X real symmetric.
// After P6 the kernel generates X in slabs of AF_KS eigenvectors straight into LDS (one fast division per entry, from
// O(n) data already there), accumulates all 36 lower 32 x 32 tiles of S as resident f32 matrix-core accumulators and
// applies the phases in the epilogue (arrow_fused_tail below).  By default that is two launches: the solver phases P0 - P6 as
// arrow_rebuild_kernel<AR_SOLVE> (63 VGPRs, seven workgroups per CU -- inside one kernel they ran at the occupancy of the tail's
// nine accumulator tiles), a record per matrix in the chunk's VT buffer (ArRecord), and arrow_tail_kernel, which loads the record
// into LDS and runs the same arrow_fused_tail.  ADMMNET_ARROW_FUSED=2 keeps both in one kernel (arrow_rebuild_kernel<AR_FUSED>),
// for A/B runs: the same bits.  ADMMNET_ARROW_FUSED=0 keeps the former pair: this kernel writing the image to the global VT
// buffer (AR_GLOBAL), then rebuild.hip's kernel.
// In every form the roots of P4 read their poles from plain LDS arrays, direct or reflected (arrow_core.h ArrowPoles).
#include <cstdio>
#include <cstdlib>

#include "common.h"

#include "arrow_core.h"
#include "lane_reduce.h"
#include "rebuild_lds.h"

namespace admmnet {

constexpr int AR_THREADS = 256;
// (ArMode, route.h: where the eigenvectors go -- AR_LDS image in LDS, AR_GLOBAL image in global memory, AR_FUSED slabs)
constexpr int AF_KS = 16;     // eigenvectors per slab of the fused form
constexpr int AF_W = kMaxD;   // slab row: one float per original index
static_assert(AR_THREADS == AF_W, "the fused tail gives every thread one column of X");

struct ArShared {
    int k, nrot, conf;
    int mx[2];
    float znorm;
};

__host__ __device__ inline size_t ar_np(int D) { return (size_t)((D + 1 + 3) & ~3); }
// float arrays of length NP: hraw zraw phr phim ds zs dl zl tau zh vals x0 (12) ; int arrays: perm src org rnk kidx (5)
__host__ __device__ inline size_t ar_lds_bytes(const BrGeom &g) {
    const size_t NP = ar_np(g.D);
    return sizeof(float) * (g.vt_floats() + g.small_floats() + 12 * NP) + sizeof(int) * 5 * NP + sizeof(DcRot) * NP;
}
// the solver kernel of the split form: no image, no rowb, and hraw / zraw / src / org share other arrays' memory (the kernel's carve)
__host__ __device__ inline size_t ar_solve_lds_bytes(const BrGeom &g) {
    return ar_lds_bytes(g) - sizeof(float) * (g.vt_floats() + 2 * g.Dp + 4 * ar_np(g.D));
}

// The split form of AR_FUSED (the default at 128 < D <= 256): arrow_rebuild_kernel<AR_SOLVE> runs the solver phases at its own
// occupancy and leaves, per matrix, the record below (4-byte words) in the chunk's eigenvector-image buffer ws.VT, which nothing
// else uses while the first layer runs; arrow_tail_kernel reads it back and runs arrow_fused_tail.  Word 0: 1, or 0 = non-finite
// input, nothing else written and nothing to do; word 1: the number of rotations (only those are copied).
constexpr int AR_SOLVE = 4;   // (a mode of the kernel template only: the route stays AR_FUSED)
struct ArRecord {
    int F, fs, phr, lamc, tauc, zh, dl, kidx, perm, rnk, rot, words;
    __host__ __device__ explicit ArRecord(int D) {
        const int NP = (int)ar_np(D);
        F = (D + 1 + 4) & ~3;        // fs / w0f / z0s: n + 1 entries each
        fs = 4;
        phr = fs + 3 * F;            // phr, phim
        lamc = phr + 2 * NP;
        tauc = lamc + NP;
        zh = tauc + NP;
        dl = zh + NP;
        kidx = dl + NP;
        perm = kidx + NP;
        rnk = perm + NP;
        rot = rnk + NP;              // DcRot: four words each
        words = rot + 4 * NP;
    }
};
static_assert(sizeof(DcRot) == 16, "ArRecord counts a rotation as four words");
__host__ __device__ inline int ar_rec_words(int D) { return ArRecord(D).words; }

// ---- fused tail (AR_FUSED, 128 < D <= 256): S = X^T diag(f) X on the matrix cores, X generated slab by slab in LDS ----
// In: the solver's LDS arrays after P6 -- fs / w0f / z0s / lamc / tauc in FINAL eigenvalue order c, zh / dl per surviving
// pole, kidx / perm / rnk / rot of the deflation.  Thread t owns column t of X (original index): entry [c][t] is
// arrow_vec_entry for a surviving pole, a unit entry in row rnk[slot] for a deflated one.  Rotations (rare) are undone
// row by row in the slab.  Four waves; wave w holds block rows 7 - w and w of the lower triangle: slot q <= 7 - w is
// tile (7 - w, q), slot q > 7 - w is tile (w, 8 - q) -- nine 32 x 32 accumulators, the column block of every slot static.
template <class Mark>
__device__ __forceinline__ void arrow_fused_tail(int D, int nrot, int64_t b, const float *__restrict__ lw, float *slab,
                                                 const float *fs, const float *w0f, const float *z0s, const float *lamc,
                                                 const float *tauc, const float *phr, const float *phim, const float *zh,
                                                 const float *dl, const int *kidx, int *ipos, const int *perm,
                                                 const int *rnk, const DcRot *rot, float *redb,
                                                 const float2 *__restrict__ phi, const float *__restrict__ h,
                                                 float2 *__restrict__ G, float *__restrict__ rn, int lower_only, Mark mark) {
    const int n = D + 1, NT = (D + 31) >> 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, kh = lane >> 5;
    const int Ihi = 7 - wave, Ilo = wave;
    for (int p = tid; p < D; p += AR_THREADS) ipos[perm[p]] = p;   // inverse permutation
    __syncthreads();
    float zi = 0.f, di = 0.f;
    int cdef = -1;   // deflated pole: the row of its unit entry
    bool surv = false;
    if (tid < D) {
        const int kd = kidx[ipos[tid]];
        if (kd >= 0) {
            surv = true;
            zi = zh[kd];
            di = dl[kd];
        } else {
            cdef = rnk[-kd - 1];
        }
    }
    auto gen = [&](int sl, int buf) {   // rows beyond n and columns beyond D: zeros
        float *dst = slab + buf * (AF_KS * AF_W) + tid;
        const int c0 = sl * AF_KS;
#pragma unroll
        for (int r = 0; r < AF_KS; ++r) {
            const int c = c0 + r, cc = min(c, n - 1);
            const float v = surv ? arrow_vec_entry(zi, di, lamc[cc], tauc[cc], z0s[cc]) : (c == cdef ? 1.f : 0.f);
            dst[r * AF_W] = (c < n) ? v : 0.f;
        }
    };
    // deflation rotations undone (reverse order, v = G^T v'), one thread per row of the slab -- arrow.hip P8
    auto unrotate = [&](int sl, int buf) {
        const int r = tid >> 4;
        if ((tid & 15) == 0 && sl * AF_KS + r < n) {
            float *row = slab + (buf * AF_KS + r) * AF_W;
            for (int q = nrot - 1; q >= 0; --q) {
                const DcRot rr = rot[q];
                const int ia = perm[rr.pa], ib = perm[rr.pb];
                const float a = row[ia], bb = row[ib];
                row[ia] = rr.c * a - rr.s * bb;
                row[ib] = rr.s * a + rr.c * bb;
            }
        }
    };
    // slot -> tile.  Slots 0 .. 4 are always (Ihi, q) and slot 8 is (Ilo, 0); slots 5 .. 7 depend on the wave.
    const bool hi5 = 5 <= Ihi, hi6 = 6 <= Ihi, hi7 = 7 <= Ihi;
    const int J5 = hi5 ? 5 : 3, J6 = hi6 ? 6 : 2, J7 = hi7 ? 7 : 1;
    // D < 256: block rows >= NT are not computed (their slab columns hold zeros)
    const bool en_hi = Ihi < NT, en_lo = Ilo < NT;
    const bool en5 = hi5 ? en_hi : en_lo, en6 = hi6 ? en_hi : en_lo, en7 = hi7 ? en_hi : en_lo;
    f32x16 acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] = f32x16{0};
    float arow = 0.f;   // sum_c f_c x0_c X[c][tid]
    const int nslab = (n + AF_KS - 1) / AF_KS;
    gen(0, 0);
    __syncthreads();
    if (nrot > 0) {   // (uniform; the usual case has none)
        unrotate(0, 0);
        __syncthreads();
    }
    mark(3);
    // one slab: arrow row, then k-steps of two eigenvectors (lane half kh takes eigenvector c0 + kk + kh)
    auto consume = [&](int sl) {
        const int c0 = sl * AF_KS;
        const float *sb = slab + (sl & 1) * (AF_KS * AF_W);
#pragma unroll
        for (int r = 0; r < AF_KS; ++r) arow = fmaf(w0f[min(c0 + r, n)], sb[r * AF_W + tid], arow);   // (w0f[n] = 0)
        // operands of one k-step, read one step ahead of the MFMAs that use them (sched_barrier pins that order: left
        // alone, the scheduler hoists every read of the slab to the top and spills the accumulators)
        struct Step { float x0, x1, x2, x3, x4, x5, x6, x7, ahi, alo; };
        auto load = [&](int kk) {
            const float fc = fs[min(c0 + kk + kh, n)];   // (fs[n] = 0; rows beyond n hold zeros)
            const float *row = sb + (kk + kh) * AF_W + r32;
            return Step{row[0], row[32], row[64], row[96], row[128], row[32 * J5], row[32 * J6], row[32 * J7],
                        row[32 * Ihi] * fc, row[32 * Ilo] * fc};
        };
        Step cur = load(0);
#pragma unroll
        for (int kk = 0; kk < AF_KS; kk += 2) {
            Step nxt = cur;
            if (kk + 2 < AF_KS) nxt = load(kk + 2);
            __builtin_amdgcn_sched_barrier(0);
            if (c0 + kk < n) {   // (uniform) the last slab is short
                const float a5 = hi5 ? cur.ahi : cur.alo, a6 = hi6 ? cur.ahi : cur.alo, a7 = hi7 ? cur.ahi : cur.alo;
                if (en_hi) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ahi, cur.x0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ahi, cur.x1, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ahi, cur.x2, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ahi, cur.x3, acc[3], 0, 0, 0);
                    acc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ahi, cur.x4, acc[4], 0, 0, 0);
                }
                if (en5) acc[5] = __builtin_amdgcn_mfma_f32_32x32x2f32(a5, cur.x5, acc[5], 0, 0, 0);
                if (en6) acc[6] = __builtin_amdgcn_mfma_f32_32x32x2f32(a6, cur.x6, acc[6], 0, 0, 0);
                if (en7) acc[7] = __builtin_amdgcn_mfma_f32_32x32x2f32(a7, cur.x7, acc[7], 0, 0, 0);
                if (en_lo) acc[8] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.alo, cur.x0, acc[8], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
    };
    for (int sl = 0; sl < nslab; ++sl) {
        if (sl + 1 < nslab) gen(sl + 1, (sl & 1) ^ 1);
        consume(sl);
        __syncthreads();
        if (nrot > 0 && sl + 1 < nslab) {
            unrotate(sl + 1, (sl & 1) ^ 1);
            __syncthreads();
        }
    }
    mark(4);
    // ---- epilogue: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float2 *Gb = G + b * (int64_t)n * n;
    float acc2 = 0.f;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const bool hi = q <= 4 || (q == 5 && hi5) || (q == 6 && hi6) || (q == 7 && hi7);
        const int I = hi ? Ihi : Ilo, J = hi ? q : 8 - q;
        if (I < NT) {
            const int gj = 32 * J + r32;
            const float prj = phr[min(gj, D - 1)], pij = phim[min(gj, D - 1)];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int gi = 32 * I + (e & 3) + 8 * (e >> 2) + 4 * kh;
                if (gi >= gj && gi < D) {
                    const float S = acc[q][e];
                    if (gi == gj) {
                        Gb[(int64_t)gi * n + gj] = make_float2(S, 0.f);
                        const float d = S - h[b * D + gi];
                        acc2 += d * d;
                    } else {
                        float re, im;
                        arrow_phase_entry(S, phr[gi], phim[gi], prj, pij, re, im);
                        Gb[(int64_t)gi * n + gj] = make_float2(re, im);
                        if (!lower_only) Gb[(int64_t)gj * n + gi] = make_float2(re, -im);
                        acc2 += 2.f * (re * re + im * im);
                    }
                }
            }
        }
    }
    // arrow row G[D][o] = arow conj(p_o): thread o holds its own arow (D <= AR_THREADS)
    rebuild_tail<AR_THREADS / 64>(acc2, 0, n, D, Gb, phi + b * D, lw[S_CORNER_Z], w0f, z0s, redb, rn + b, lower_only,
                                  [&](int o, float &gr, float &gim) {
                                      gr = arow * phr[o];
                                      gim = -(arow * phim[o]);
                                  });
    mark(5);
}

// BIG (AR_GLOBAL, 128 < D <= 256 with ADMMNET_ARROW_FUSED=0): the eigenvector image does not fit the LDS; it is built
// in the global VT buffer of the dense path (rows c, planes at 0 / D, pitch 2 D) together with w and w0, and rebuild.hip's
// kernel consumes it.
template <int MODE>
__global__ __launch_bounds__(AR_THREADS, MODE == AR_FUSED ? 2 : MODE == AR_SOLVE ? 7 : 1) void arrow_rebuild_kernel(
    int D, const float *__restrict__ lw, const float2 *__restrict__ phi, const float *__restrict__ h,
    float2 *__restrict__ G, float *__restrict__ rn, float *__restrict__ w_out, int32_t *__restrict__ status,
    unsigned long long *__restrict__ ptime, int lower_only, float *VTg, float *__restrict__ w0g) {
    constexpr bool BIG = MODE == AR_GLOBAL, SOLVE = MODE == AR_SOLVE, FUSED = MODE == AR_FUSED || SOLVE;   // (FUSED: what the tail reads)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ ArShared sh;
    // developer phase timer (ADMMNET_AR_TIMING=1): cycles of thread 0 between marks
    long long t_prev = ptime ? clock64() : 0;
    auto mark = [&](int id) {
        if (ptime && threadIdx.x == 0) {
            const long long t_now = clock64();
            atomicAdd(&ptime[id], (unsigned long long)(t_now - t_prev));
            t_prev = t_now;
        }
    };
    const BrGeom g(D);
    const int n = g.n;
    const int Dp = BIG ? D : g.Dp, VP = BIG ? 2 * D : g.VP;   // plane width / row pitch of the eigenvector image
    const int NP = (int)ar_np(D);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float alpha = lw[S_CORNER_G];   // corner of C = 1 / (lambda^2 + eps), admm_net.py:271
    float *VTl = BIG ? VTg + b * ((int64_t)n * 2 * D) : reinterpret_cast<float *>(smem);
    float *fs = reinterpret_cast<float *>(smem) + (BIG || FUSED ? 0 : g.vt_floats());
    float *w0f = fs + ((n + 4) & ~3);
    float *z0s = w0f + ((n + 4) & ~3);
    float *rowb = z0s + ((n + 4) & ~3);
    float *redb = rowb + (SOLVE ? 0 : 2 * Dp);   // (SOLVE: no rowb -- and no hraw / zraw / src / org of its own, see below)
    float *own = redb + 8;
    float *phr = own + (SOLVE ? 0 : 2 * NP);
    float *phim = phr + NP;
    float *ds = phim + NP;
    float *zs = ds + NP;
    float *dl = zs + NP;
    float *zl = dl + NP;
    float *tau = zl + NP;
    float *zh = tau + NP;
    float *vals = zh + NP;
    float *x0 = vals + NP;
    float *lamd = zs;   // (after the deflation scan) d[org_j]: origin pole value of root j
    int *perm = reinterpret_cast<int *>(x0 + NP);
    int *own_i = perm + NP;
    int *rnk = own_i + (SOLVE ? 0 : 2 * NP);
    int *kidx = rnk + NP;
    // SOLVE keeps its LDS small enough for seven workgroups per CU: arrays whose lives do not meet share memory.  hraw / zraw
    // die with P1, before the deflation first writes tau / zh; src dies with kidx and org with the deflation, both before P6
    // writes w0f / z0s.
    float *hraw = SOLVE ? tau : own, *zraw = SOLVE ? zh : own + NP;
    int *src = SOLVE ? reinterpret_cast<int *>(w0f) : own_i, *org = SOLVE ? reinterpret_cast<int *>(z0s) : own_i + NP;
    // the poles as the root solver reads them (arrow_core.h ArrowPoles), alive from the deflation to the end of P4: in ds (read
    // last by the deflation, lamc from P6), x0 (written in P6) and rnk (written in P5, behind the barrier that ends P4)
    float *zz = reinterpret_cast<float *>(rnk), *dR = ds, *zzR = x0;
    DcRot *rot = reinterpret_cast<DcRot *>(kidx + NP);
    float *lamc = ds, *tauc = zl;   // (FUSED, after P6) origin pole value and tau of the root in final position c

    // ---- P0: load, moduli and phases
    if (tid == 0) {
        sh.mx[0] = __float_as_int(fabsf(alpha));
        sh.mx[1] = 0;
    }
    int bad = 0;   // non-finite input or eigenvalue: reported through status[0] (torch.linalg.eigh raises on such input)
    for (int i = tid; i < D; i += AR_THREADS) {
        const float2 z = phi[b * D + i];
        const float a = sqrtf(z.x * z.x + z.y * z.y);
        const float ia = a > 0.f ? 1.0f / a : 0.f;
        hraw[i] = h[b * D + i];
        bad |= !(isfinite(a) && isfinite(hraw[i]));
        zraw[i] = a;
        phr[i] = a > 0.f ? z.x * ia : 1.f;
        phim[i] = a > 0.f ? z.y * ia : 0.f;
    }
    if (__syncthreads_or(bad)) {   // NaN / Inf input: the rank sort below would leave permutation slots unwritten
        if (tid == 0 && status) atomicAdd(status, 1);
        if (SOLVE && tid == 0) reinterpret_cast<int *>(VTg + b * (int64_t)ar_rec_words(D))[0] = 0;   // the tail leaves at once
        return;
    }
    // ---- P1: sort h ascending (stable rank counting)
    for (int i = tid; i < D; i += AR_THREADS) {
        const float v = hraw[i];
        int r = 0;
#pragma unroll 8
        for (int q = 0; q < D; ++q) {
            const float u = hraw[q];
            r += (u < v) || (u == v && q < i);
        }
        perm[r] = i;
        ds[r] = v;
        zs[r] = zraw[i];
        atomicMax(&sh.mx[0], __float_as_int(fabsf(v)));
        atomicMax(&sh.mx[1], __float_as_int(zraw[i]));
    }
    __syncthreads();
    // ---- P2: deflation.  Usual case: nothing deflates (distinct h, non-zero phi) -- checked in parallel;
    //      otherwise the serial scan of the D&C merge (one thread)
    {
        const float dmax = __int_as_float(sh.mx[0]), zmax = __int_as_float(sh.mx[1]);
        int trig = 0;
        for (int p = tid; p < D; p += AR_THREADS) trig |= deflate_triggers(p, 1.0f, dmax, zmax, ds, zs) ? 1 : 0;
        if (__syncthreads_or(trig)) {   // team form of the scan (dc_core.h), later phases' arrays as scratch
            const float tol = 8.0f * kEps32 * fmaxf(dmax, zmax);
            float *dde = reinterpret_cast<float *>(kidx);
            defl_par_flags(tid, AR_THREADS, D, 1.0f, tol, ds, zs, org, rnk, tau, zh);
            if (tid == 0) sh.conf = 0;
            __syncthreads();
            defl_par_walk(tid, AR_THREADS, D, tol, ds, zs, org, rnk, tau, zh, vals, x0, dde, &sh.conf);
            __syncthreads();
            if (sh.conf) {   // a rotation chain grew into the next run of candidates: serial scan
                if (tid == 0) {
                    int k = 0, nr = 0;
                    deflate_scan_tol(D, 1.0f, dmax, zmax, ds, zs, dl, zl, src, rot, k, nr);
                    sh.k = k;
                    sh.nrot = nr;
                }
            } else {
                defl_par_emit(tid, AR_THREADS, D, ds, org, rnk, tau, zh, vals, x0, dde, dl, zl, src, rot, &sh.k, &sh.nrot);
            }
        } else {
            for (int p = tid; p < D; p += AR_THREADS) {
                dl[p] = ds[p];
                zl[p] = zs[p];
                src[p] = p;
            }
            if (tid == 0) {
                sh.k = D;
                sh.nrot = 0;
            }
        }
    }
    __syncthreads();
    mark(0);
    const int k = sh.k, nrot = sh.nrot;
    // slots: 0..k roots, p + 1 for the deflated pole at scan position p in [k, D)
    for (int p = k + tid; p < D; p += AR_THREADS) vals[p + 1] = dl[p];
    for (int p = tid; p < D; p += AR_THREADS) kidx[src[p]] = (p < k) ? p : -(p + 1) - 1;   // sorted position -> pole / slot
    for (int i = tid; i < k; i += AR_THREADS) arrow_poles_fill(k, i, dl, zl, zz, dR, zzR);
    if (tid < 64) {   // ||zeta|| of the surviving poles
        float s = 0.f;
        for (int i = tid; i < k; i += 64) s = fmaf(zl[i], zl[i], s);
        s = wave_sum(s);
        if (tid == 0) sh.znorm = sqrtf(s);
    }
    __syncthreads();
    // ---- P4: secular roots
    if (k == 0) {
        if (tid == 0) vals[0] = alpha;
    } else {
        const float znorm = sh.znorm;
        const ArrowPoles poles{dl, zz, dR, zzR};
        auto put = [&](int jr, int o, float t) {
            tau[jr] = t;
            lamd[jr] = dl[o];
            vals[jr] = dl[o] + t;
        };
        // Lanes per root: two adjacent lanes (each sums every other pole) while the roots fit, one otherwise; roots
        // beyond the lanes' first pass -- root 128 of D = 128, root 256 of D = 256 -- are solved by the whole of
        // wave 0 (each lane two to four poles) instead of a second, nearly empty pass.
        const int first = (k + 1 <= AR_THREADS / 2 + 1) ? min(k + 1, AR_THREADS / 2) : min(k + 1, AR_THREADS);
        if (first <= AR_THREADS / 2) {
            const int jr = tid >> 1, sub = tid & 1;
            if (jr < first) {
                int o;
                float t;
                arrow_root(k, jr, alpha, znorm, poles, o, t, nullptr, sub, 2, [](float x) {
                    return pair_sum(x);
                });
                if (sub == 0) put(jr, o, t);
            }
        } else if (tid < first) {
            int o;
            float t;
            arrow_root(k, tid, alpha, znorm, poles, o, t);
            put(tid, o, t);
        }
        if (tid < 64) {
            for (int jr = first; jr <= k; ++jr) {
                int o;
                float t;
                arrow_root(k, jr, alpha, znorm, poles, o, t, nullptr, tid, 64, [](float x) { return wave_sum(x); });
                if (tid == 0) put(jr, o, t);
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < n; p += AR_THREADS) bad |= !isfinite(vals[p]);
    mark(1);
    // ---- P5: zeta-hat, final (ascending, stable) positions of all n eigenvalues
    {   // two adjacent lanes per pole (k <= 128): half of the serial product each
        const int G = (2 * k <= AR_THREADS) ? 2 : 1;
        const int sub = (G == 2) ? (tid & 1) : 0;
        auto redm = [G](float x) {
            const float y = pair_get(x);
            return G == 2 ? x * y : x;
        };
        for (int i = (G == 2) ? (tid >> 1) : tid; i < k; i += AR_THREADS / G) {
            const float v = arrow_zhat(k, i, dl, lamd, tau, sub, G, redm);
            if (sub == 0) zh[i] = v;
        }
    }
    for (int s = tid; s < n; s += AR_THREADS) {
        const float v = vals[s];
        int r = 0;
#pragma unroll 8
        for (int q = 0; q < n; ++q) {
            const float u = vals[q];
            r += (u < v) || (u == v && q < s);
        }
        rnk[s] = r;
    }
    __syncthreads();
    // ---- P6: norms; eigenvalue map and arrow-row entries in final order
    {
        const LayerLayout L{D};
        const float thr = lw[S_THR];
        const float *vn = lw + L.off_vn();
        for (int s = tid; s < n; s += AR_THREADS) {
            float xa = 0.f;   // arrow component of eigenvector s
            if (s <= k) {
                float nrm = 1.f;
                if (k > 0) {
                    const float dorg = lamd[s], ts = tau[s];
#pragma unroll 4
                    for (int i = 0; i < k; ++i) {
                        const float v = fdiv_fast(zh[i], (dorg - dl[i]) + ts);   // zhat_i / (lam_s - d_i)
                        nrm = fmaf(v, v, nrm);
                    }
                }
                xa = 1.0f / sqrtf(nrm);
            }
            x0[s] = xa;
            const int c = rnk[s];
            const float lam = vals[s];
            const float f = eig_map(lam, thr, vn);
            fs[c] = f;
            w0f[c] = xa * f;
            z0s[c] = xa;
            if (w_out) w_out[b * n + c] = lam;
            if (BIG) w0g[b * n + c] = xa;
            if (FUSED) {   // (deflated slots: a divisor no pole value reaches; their x0 = 0 makes the entry an exact zero)
                const bool root = s <= k && k > 0;
                lamc[c] = root ? lamd[s] : 3.0e38f;
                tauc[c] = root ? tau[s] : 0.f;
            }
        }
        if (tid == 0) {
            fs[n] = 0.f;
            w0f[n] = 0.f;
            z0s[n] = 0.f;
        }
    }
    __syncthreads();
    if constexpr (SOLVE) {   // the record of this matrix for arrow_tail_kernel (ArRecord), in the chunk's image buffer
        if (__syncthreads_or(bad) && tid == 0 && status) atomicAdd(status, 1);
        const ArRecord R(D);
        float *rec = VTg + b * (int64_t)R.words;
        const auto put = [&](int off, const void *src_, int cnt) {
            const float *sp = static_cast<const float *>(src_);
            for (int i = tid; i < cnt; i += AR_THREADS) rec[off + i] = sp[i];
        };
        if (tid == 0) {
            reinterpret_cast<int *>(rec)[0] = 1;
            reinterpret_cast<int *>(rec)[1] = nrot;
        }
        put(R.fs, fs, 3 * R.F);   // fs, w0f, z0s
        put(R.phr, phr, 2 * NP);  // phr, phim
        put(R.lamc, lamc, NP);
        put(R.tauc, tauc, NP);
        put(R.zh, zh, NP);
        put(R.dl, dl, NP);
        put(R.kidx, kidx, NP);
        put(R.perm, perm, NP);
        put(R.rnk, rnk, NP);
        put(R.rot, rot, 4 * nrot);
        mark(2);
        return;
    }
    mark(2);
    if constexpr (MODE == AR_FUSED) {
        if (__syncthreads_or(bad) && tid == 0 && status) atomicAdd(status, 1);
        arrow_fused_tail(D, nrot, b, lw, reinterpret_cast<float *>(rot + NP), fs, w0f, z0s, lamc, tauc, phr, phim, zh, dl,
                         kidx, reinterpret_cast<int *>(hraw), perm, rnk, rot, redb, phi, h, G, rn, lower_only,
                         [&](int id) { mark(id); });
        return;
    }
    // ---- P7: eigenvectors in the rotated real basis, straight into VT[c][column of ORIGINAL index]
    //      thread = original index i (both planes' padding columns are zeroed as well)
    int *ipos = reinterpret_cast<int *>(hraw);   // inverse permutation (hraw is dead since P1)
    for (int p = tid; p < D; p += AR_THREADS) ipos[perm[p]] = p;
    __syncthreads();
    // (when the plane is narrower than the workgroup, AR_THREADS / Dp threads share a column and split its
    //  entries s: at D = 128 two threads per column instead of 128 idle ones)
    const int nparts = (AR_THREADS / Dp > 0) ? AR_THREADS / Dp : 1;
    const int sper = (n + nparts - 1) / nparts;
    for (int it = tid; it < Dp * nparts; it += AR_THREADS) {
        const int i = it % Dp, part = it / Dp;
        const int s0 = part * sper, s1 = min(n, s0 + sper);
        float *colr = VTl + i, *coli = VTl + Dp + i;
        if (i >= D) {
            for (int c = s0; c < s1; ++c) {
                colr[c * VP] = 0.f;
                coli[c * VP] = 0.f;
            }
            continue;
        }
        const int kd = kidx[ipos[i]];
        if (kd >= 0) {   // surviving pole kd: component zhat x0_s / (lam_s - d) in every root's eigenvector
            const float zi = zh[kd], di = dl[kd];
#pragma unroll 4
            for (int s = s0; s < min(s1, k + 1); ++s) {
                const float v = fdiv_fast(zi, (lamd[s] - di) + tau[s]) * x0[s];
                colr[rnk[s] * VP] = v;
            }
            for (int s = max(s0, k + 1); s < s1; ++s) colr[rnk[s] * VP] = 0.f;
        } else {         // deflated pole: unit vector of slot -(kd) - 1
            const int slot = -kd - 1;
#pragma unroll 4
            for (int s = s0; s < s1; ++s) colr[rnk[s] * VP] = (s == slot) ? 1.f : 0.f;
        }
    }
    __syncthreads();
    // ---- P8: undo the deflation rotations (reverse order, v = G^T v'), thread = eigenvector row c
    for (int c = tid; c < n; c += AR_THREADS) {
        float *row = VTl + c * VP;
        for (int r = nrot - 1; r >= 0; --r) {
            const DcRot rr = rot[r];
            const int ia = perm[rr.pa], ib = perm[rr.pb];
            const float a = row[ia], bb = row[ib];
            row[ia] = rr.c * a - rr.s * bb;
            row[ib] = rr.s * a + rr.c * bb;
        }
    }
    __syncthreads();
    // phases: (re, im) planes
    for (int it = tid; it < Dp * nparts; it += AR_THREADS) {
        const int i = it % Dp, part = it / Dp;
        if (i >= D) continue;
        float *colr = VTl + i, *coli = VTl + Dp + i;
        const float pr = phr[i], pi = phim[i];
#pragma unroll 8
        for (int c = part * sper; c < min(n, (part + 1) * sper); ++c) {
            const float x = colr[c * VP];
            colr[c * VP] = x * pr;
            coli[c * VP] = x * pi;
        }
    }
    __syncthreads();
    mark(3);
    if (__syncthreads_or(bad) && tid == 0 && status) atomicAdd(status, 1);
    if constexpr (BIG) return;
    else rebuild_from_lds(g, b, lw, VTl, fs, w0f, z0s, rowb, redb, phi, h, G, rn, [&](int id) { mark(id); }, lower_only);
}

// Second kernel of the split first layer: the record into LDS (one linear copy: it is laid out as the tail reads it), then the
// tail as the one-kernel form runs it.
__global__ __launch_bounds__(AR_THREADS, 2) void arrow_tail_kernel(int D, const float *__restrict__ lw,
                                                                   const float2 *__restrict__ phi, const float *__restrict__ h,
                                                                   float2 *__restrict__ G, float *__restrict__ rn,
                                                                   unsigned long long *__restrict__ ptime, int lower_only,
                                                                   const float *__restrict__ recs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long t_prev = ptime ? clock64() : 0;
    auto mark = [&](int id) {
        if (ptime && threadIdx.x == 0) {
            const long long t_now = clock64();
            atomicAdd(&ptime[id], (unsigned long long)(t_now - t_prev));
            t_prev = t_now;
        }
    };
    const ArRecord R(D);
    const int NP = (int)ar_np(D);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float *rec = recs + b * (int64_t)R.words;
    const int ok = reinterpret_cast<const int *>(rec)[0], nrot = reinterpret_cast<const int *>(rec)[1];   // (uniform)
    if (!ok) return;   // non-finite input: counted by the solver kernel, nothing is written
    float *l = reinterpret_cast<float *>(smem);
    const int nw = R.rot + 4 * nrot;   // (a multiple of 4, as the record's stride is)
    for (int i = 4 * tid; i < nw; i += 4 * AR_THREADS)
        *reinterpret_cast<float4 *>(l + i) = *reinterpret_cast<const float4 *>(rec + i);
    int *ipos = reinterpret_cast<int *>(l + R.words);
    float *redb = reinterpret_cast<float *>(ipos + NP);
    float *slab = redb + 8;
    __syncthreads();
    arrow_fused_tail(D, nrot, b, lw, slab, l + R.fs, l + R.fs + R.F, l + R.fs + 2 * R.F, l + R.lamc, l + R.tauc, l + R.phr,
                     l + R.phr + NP, l + R.zh, l + R.dl, reinterpret_cast<const int *>(l + R.kidx), ipos,
                     reinterpret_cast<const int *>(l + R.perm), reinterpret_cast<const int *>(l + R.rnk),
                     reinterpret_cast<const DcRot *>(l + R.rot), redb, phi, h, G, rn, lower_only, [&](int id) { mark(id); });
}
static size_t ar_tail_lds_bytes(int D) {
    return sizeof(float) * ((size_t)ArRecord(D).words + ar_np(D) + 8 + 2 * AF_KS * AF_W);
}

bool arrow_rebuild_supported(int D) { return D >= 1 && D <= 256; }

// developer phase timer (ADMMNET_AR_TIMING=1): mean cycles of thread 0 per phase, printed after the launch
static int ar_timing_end(PhaseTimer &tm, hipStream_t st, int D, int64_t nb, const char *const (&nm)[6]) {
    if (!tm.dev) return ADMMNET_OK;
    unsigned long long hb[16];
    if (int rc = tm.end(st, hb)) return rc;
    fprintf(stderr, "[arrow_rebuild timing] D=%d nb=%lld  mean cycles per workgroup:\n", D, (long long)nb);
    for (int i = 0; i < 6; ++i) fprintf(stderr, "   %-14s %10.0f\n", nm[i], (double)hb[i] / (double)nb);
    return ADMMNET_OK;
}

int launch_arrow_rebuild(const Route &r, const Switches &sw, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *G, float *rn,
                         float *w_out, int32_t *status, const Ws &ws, hipStream_t st, bool lower_only) {
    const int D = r.D;
    if (nb <= 0) return ADMMNET_OK;
    if (!arrow_rebuild_supported(D)) {
        set_error("arrow_rebuild: D=%d unsupported", D);
        return ADMMNET_E_ARG;
    }
    const BrGeom g(D);
    int rc;
    // D > 128: X in LDS slabs and real S on the matrix cores (AR_FUSED) -- as solver kernel + tail kernel, or behind
    // ADMMNET_ARROW_FUSED=2 as the one kernel it was -- or the image in global memory and the dense path's rebuild (AR_GLOBAL)
    static const char *const nm_fused[6] = {"sort+deflate", "roots", "zhat+rank+norm", "first slab", "slabs + S", "epilogue"};
    if (r.first == AR_FUSED && !sw.arrow_onekernel) {
        if (!ws.VT) {
            set_error("arrow_rebuild: the split first layer needs the chunk's image buffer");
            return ADMMNET_E_ARG;
        }
        ProfScope _prof(KC_REBUILD, st);
        const size_t lds = ar_solve_lds_bytes(g), lds_tail = ar_tail_lds_bytes(D);
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(arrow_rebuild_kernel<AR_SOLVE>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(arrow_tail_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_tail));
        PhaseTimer tm;
        if ((rc = tm.begin(sw.ar_timing, st, 16))) return rc;
        hipLaunchKernelGGL(arrow_rebuild_kernel<AR_SOLVE>, dim3((unsigned)nb), dim3(AR_THREADS), lds, st, D, lw, phi, h, G,
                           rn, w_out, status, tm.dev, lower_only ? 1 : 0, ws.VT, (float *)nullptr);
        ADMM_HIP(hipGetLastError());
        hipLaunchKernelGGL(arrow_tail_kernel, dim3((unsigned)nb), dim3(AR_THREADS), lds_tail, st, D, lw, phi, h, G, rn, tm.dev,
                           lower_only ? 1 : 0, ws.VT);
        ADMM_HIP(hipGetLastError());
        return ar_timing_end(tm, st, D, nb, nm_fused);
    }
    if (r.first == AR_FUSED) {
        ProfScope _prof(KC_REBUILD, st);
        const size_t lds = ar_lds_bytes(g) - sizeof(float) * g.vt_floats() + sizeof(float) * 2 * AF_KS * AF_W;
        ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(arrow_rebuild_kernel<AR_FUSED>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PhaseTimer tm;
        if ((rc = tm.begin(sw.ar_timing, st, 16))) return rc;
        hipLaunchKernelGGL(arrow_rebuild_kernel<AR_FUSED>, dim3((unsigned)nb), dim3(AR_THREADS), lds, st, D, lw, phi, h, G,
                           rn, w_out, status, tm.dev, lower_only ? 1 : 0, (float *)nullptr, (float *)nullptr);
        ADMM_HIP(hipGetLastError());
        return ar_timing_end(tm, st, D, nb, nm_fused);
    }
    if (r.first == AR_GLOBAL) {   // eigenvectors to the global image, then the dense path's rebuild kernel
        {
            ProfScope _prof(KC_REBUILD, st);
            const size_t lds = ar_lds_bytes(g) - sizeof(float) * g.vt_floats();
            ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(arrow_rebuild_kernel<AR_GLOBAL>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(arrow_rebuild_kernel<AR_GLOBAL>, dim3((unsigned)nb), dim3(AR_THREADS), lds, st, D, lw, phi, h,
                               G, rn, ws.w, status, (unsigned long long *)nullptr, lower_only ? 1 : 0, ws.VT, ws.w0);
            ADMM_HIP(hipGetLastError());
        }
        return launch_rebuild(D, nb, lw, phi, h, G, rn, w_out, ws, st, lower_only, r.first_rebuild, D);   // (image laid out for D itself)
    }
    ProfScope _prof(KC_REBUILD, st);
    const size_t lds = ar_lds_bytes(g);
    ADMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(arrow_rebuild_kernel<AR_LDS>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PhaseTimer tm;
    if ((rc = tm.begin(sw.ar_timing, st, 16))) return rc;
    hipLaunchKernelGGL(arrow_rebuild_kernel<AR_LDS>, dim3((unsigned)nb), dim3(AR_THREADS), lds, st, D, lw, phi, h, G, rn,
                       w_out, status, tm.dev, lower_only ? 1 : 0, (float *)nullptr, (float *)nullptr);
    ADMM_HIP(hipGetLastError());
    static const char *const nm[6] = {"sort+deflate", "roots", "zhat+rank+norm", "vectors", "G tiles", "arrow+norm"};
    return ar_timing_end(tm, st, D, nb, nm);
}

}  // namespace admmnet
