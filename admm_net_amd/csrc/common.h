// common.h -- shared host/device declarations of the gfx950 ADMM-Net library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/admmnet.h"
#include "eig_core.h"
#include "route.h"

namespace admmnet {

constexpr float kEpsRef = 1e-8f;   // epsilon of every reference layer (admm_net.py:74,114,211,360)
constexpr int kHid = 64;           // HLayer.correction_net hidden width (admm_net.py:128)
constexpr int kMaxD = 256;         // largest supported signal length D = M*N
constexpr int kLogCapMul = 3;      // rotation-log capacity = kLogCapMul * n * n records per matrix

void set_error(const char *fmt, ...);
#define ADMM_HIP(call)                                                              \
    do {                                                                            \
        hipError_t _e = (call);                                                     \
        if (_e != hipSuccess) {                                                     \
            admmnet::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                               __FILE__, __LINE__);                                 \
            return ADMMNET_E_HIP;                                                   \
        }                                                                           \
    } while (0)

// ---- packed per-layer weights (floats) -------------------------------------
// scalars, resolved on the host by admmnet_pack_weights
enum LayerScalar {
    S_RHO_PHI = 0,    // softplus(phiLayers.k.rho)                      admm_net.py:97
    S_RHO_H_EPS = 1,  // softplus(hLayers.k.rho) + eps                  admm_net.py:148,151
    S_SIG_PW = 2,     // sigmoid(hLayers.k.projection_weight)          admm_net.py:188
    S_CORNER_G = 3,   // 1 / (softplus(gLayers.k.lambda_param)^2 + eps) admm_net.py:269-271
    S_INV_RHO_G = 4,  // 1 / (softplus(gLayers.k.rho) + eps)            admm_net.py:287-288
    S_THR = 5,        // sigmoid(gLayers.k.threshold)                  admm_net.py:321
    S_RHO_Z = 6,      // softplus(zLayers.k.rho)                        admm_net.py:406
    S_CORNER_Z = 7,   // 1 / (softplus(zLayers.k.lambda_param)^2 + eps) admm_net.py:424-426
    S_KNORM = 8,      // (float)(k / 10.0)                              admm_net.py:457
    S_A_COEF = 9,     // 2 * sqrtf((float)(M*N))                        admm_net.py:159
    S_COUNT = 16
};

struct LayerLayout {
    int D;
    __host__ __device__ int off_scal() const { return 0; }
    __host__ __device__ int off_w1t() const { return S_COUNT; }               // [D][64]  (transposed correction_net.0.weight)
    __host__ __device__ int off_b1() const { return off_w1t() + D * kHid; }   // [64]
    __host__ __device__ int off_w2t() const { return off_b1() + kHid; }       // [64][D]  (transposed correction_net.2.weight)
    __host__ __device__ int off_b2() const { return off_w2t() + kHid * D; }   // [D]
    __host__ __device__ int off_vn() const { return off_b2() + D; }           // value_net: w1[16] b1[16] w2[16] b2[1]
    __host__ __device__ int off_rs() const { return off_vn() + 49; }          // residual_scale_net: W1[32][3] b1[32] w2[32] b2[1]
    __host__ __device__ int size() const { return (off_rs() + 161 + 3) & ~3; }
};

// head (PeakSearchLayer) packed layout, hidden = 128, heads = 4
struct HeadLayout {
    int D, L;
    __host__ __device__ int off_pos() const { return 0; }                          // position_encoder [D][2]
    __host__ __device__ int off_fe0w() const { return off_pos() + 2 * D; }         // [2D][128] transposed
    __host__ __device__ int off_fe0b() const { return off_fe0w() + 2 * D * 128; }
    __host__ __device__ int off_fe2w() const { return off_fe0b() + 128; }          // [128][128] transposed
    __host__ __device__ int off_fe2b() const { return off_fe2w() + 128 * 128; }
    __host__ __device__ int off_ppw() const { return off_fe2b() + 128; }           // position_projection.weight [128][2]
    __host__ __device__ int off_ppb() const { return off_ppw() + 256; }
    __host__ __device__ int off_inw() const { return off_ppb() + 128; }            // in_proj_weight [384][128] -> stored transposed [128][384]
    __host__ __device__ int off_inb() const { return off_inw() + 384 * 128; }
    __host__ __device__ int off_outw() const { return off_inb() + 384; }           // out_proj.weight transposed [128][128]
    __host__ __device__ int off_outb() const { return off_outw() + 128 * 128; }
    __host__ __device__ int off_pe0w() const { return off_outb() + 128; }          // [128][64] transposed
    __host__ __device__ int off_pe0b() const { return off_pe0w() + 128 * 64; }
    __host__ __device__ int off_pe2w() const { return off_pe0b() + 64; }           // [64][32] transposed
    __host__ __device__ int off_pe2b() const { return off_pe2w() + 64 * 32; }
    __host__ __device__ int off_pe4w() const { return off_pe2b() + 32; }           // [32][16] transposed
    __host__ __device__ int off_pe4b() const { return off_pe4w() + 32 * 16; }
    // per target t: tau.0 w[16][32]T b[32], tau.2 w[32] b[1], f.0 w[16][32]T b[32], f.2 w[32] b[1]
    __host__ __device__ int off_reg(int t) const { return off_pe4b() + 16 + t * reg_size(); }
    __host__ __device__ int reg_size() const { return 2 * (16 * 32 + 32 + 32 + 1); }
    __host__ __device__ int off_conf() const { return off_reg(L); }                // c.0 w[16][16]T b[16], c.2 w[16] b[1]
    __host__ __device__ int size() const { return (off_conf() + 16 * 16 + 16 + 16 + 1 + 3) & ~3; }
};

// ---- workspace carve (all offsets in bytes, 256-byte aligned) ------------
struct Ws {
    float2 *G, *Z;            // [B][n][n] state, original index order, full storage
    float2 *phi[2];           // [B][D] double buffered (layer k uses k&1)
    float *h[2];              // [B][D]
    float *alpha;             // [B] adaptive step of the previous layer
    float *rn;                // [B] ||G - C||_F of the current layer
    double *sum;              // [2] scratch for the batch sum ([ngroups][2] with sub-batches)
    float *mean;              // [1] batch mean (single-rank path; [ngroups] with sub-batches)
    float *headkv;            // [2][D][128] batch independent K / V projections of the head
    // The compact diagonals (null where no layer reads them: carve_workspace).  prep_kernel needs Re G_ii and Re Z_ii, i < D: 2 D floats
    // out of 2 D cache lines when it gathers them from the matrices.  sp_fused_kernel holds both while it writes G, so it leaves
    // them as two rows for the next layer's prep_kernel.  A matrix that kernel rejects gets its G from the eigen-pipeline, which
    // writes no row: diag_ok is 0 there and prep_kernel gathers as it always did.
    float *diag;              // [B][2][D]: row 0 = Re G_ii, row 1 = Re Z_ii -- the floats stored at G[i][i].x and Z[i][i].x
    int *diag_ok;             // [B] 1 = sp_fused_kernel wrote this matrix's G and its rows in its last launch, 0 = it rejected the matrix
    // chunk-sized eigensolver buffers
    float2 *Mbuf;             // [chunk][D*D + D + 1]: M row-major, arrow a[D], corner (re only)
    float *QV;                // [chunk][n][2D] planar transposed: QT (D columns) then VT (n columns)
    float *dT, *eT;           // [chunk][n] tridiagonal (diagonal, off-diagonal)
    float *w, *w0;            // [chunk][n] eigenvalues, first row of W
    float *Wdc;               // [chunk][3][n][n] divide & conquer: two WT ping-pong buffers + U (null: QL path)
    int2 *Wmap;               // [chunk][n] D = 256 path: where eigenvector j of T lives after the top-level merge (float offset
                              // into the matrix' Wdc block, valid rows lo | hi << 16) -- deflated columns are not copied there
    float *VT;                // [chunk][n][2D] eigenvectors for the rebuild (= QV on the QL path)
    float2 *Tfac;             // [chunk][17][16][16] T factors of the panel block reflectors (D = 256 path, else null)
    float2 *Tail;             // [chunk][36][4][64] trailing 128 x 128 tile set between the stages of tridiag_panel
    LogRec *log;              // [chunk][cap], 64-byte groups (eig_core.h)
    int *logn;                // [chunk][2]: records, status
    int64_t chunk;            // signals per chunk
    int64_t cap;              // log records per matrix (multiple of 8)
    int64_t total_bytes;
    int64_t set2_offset;      // byte offset of a second set of chunk buffers (two chunks in flight, api.hip), 0 = none
    // matrix-function fast path of the G-layer (spectral.hip, ADMMNET_SPECTRAL=1; null otherwise)
    float2 *spec_mat;         // [2][chunk][n][n]: A (then E in place), E^2
    float2 *spec_vec;         // [chunk][2][n] the two outlier eigenvectors
    double *spec_val;         // [chunk][8] lam0, lam1, c, residuals, trace
    int *spec_flag;           // [chunk] 1 = this matrix takes the eigen-pipeline after all
    const int *skip;          // per-matrix filter of the eigen-pipeline kernels: workgroups of matrices with skip[b] == 0 leave
                              // at once (null: every matrix runs)
};


// ---- kernel launchers (each enqueues on `st`, returns ADMMNET_* code) ----------
// (sw: the Switches of the call, resolved from its cfg by api.hip -- a launcher reads its own knobs from it, never the process's)
// prep.hip
// mode bits of prep_kernel; launch_prep adds PM_FIRST / PM_ZZERO from k, the caller states the rest from the route
constexpr int PM_FIRST = 1;      // layer 0: G = Z = 0, nothing is read
constexpr int PM_ZZERO = 2;      // layer 1: stored Z is still zero (never written)
constexpr int PM_PHI_ONLY = 4;   // last layer: only phi is needed (admm_net.py:757-764)
constexpr int PM_NO_MATRIX = 8;  // layer 0 on the arrowhead path (arrow.hip): phi and h only, A is never formed
constexpr int PM_HALF = 32;      // D = 256 (tridiag_panel.hip): G / Z streamed as lower triangles, the image written for the lower
                                 // 16-block triangle only (diagonal blocks in full) -- the tiles that kernel loads
constexpr int PM_NOIMG = 64;     // with PM_HALF: only the lazy Z update streams, no image -- the G-layer is evaluated as a matrix function
                                 // straight from Z (spectral_fused.hip); the matrices it rejects get their image from half_image_kernel
constexpr int PM_SMALL = 128;    // phi and h only: the lazy Z update is folded into the first sweep of the matrix-function kernel
constexpr int PM_LEAN = 16;      // G / Z kept as lower triangles, A built by the tridiagonalisation's own loader
                                 // (tridiag_reg.hip): only the lazy Z update streams here, 24 n^2 / 2 bytes per signal
constexpr int PM_DIAG = 256;     // with PM_SMALL, k >= 2: Re diag G and Re diag Z from the compact rows Ws::diag wherever Ws::diag_ok says so
// (eig_dim, here and below: Route::eig_dim -- the matrix lands in an eig_dim x eig_dim image, zero outside its own D x D block)
int launch_prep(const admmnet_cfg *cfg, const float *lw, int k, const float2 *y, const float2 *b,
                const float *sigma, int64_t b0, int64_t nb, const Ws &ws, int mode, int eig_dim, hipStream_t st);
// (the image of the matrices with ws.skip[s] != 0 from the updated Z, behind a PM_NOIMG prep)
int launch_half_image(int D, int64_t nb, const float *lw, const float2 *phi, const float *h, const float2 *Z, const Ws &ws,
                      int eig_dim, hipStream_t st);
int launch_build_generic(int n, int64_t nb, const float2 *A, const Ws &ws, int eig_dim, hipStream_t st);
int launch_build_block(int D, int64_t nb, float corner, float inv_rho, const float2 *phi, const float *h,
                       const float2 *Z, const Ws &ws, int eig_dim, hipStream_t st);
// tridiag.hip: r.tridiag at r.eig_dim.  Zlow != nullptr (ST_LEAN): tridiag_reg's own loader forms A = C - Z / rho
int launch_tridiag(const Route &r, const Switches &sw, int64_t nb, const Ws &ws, hipStream_t st, const float2 *Zlow, const float2 *phi,
                   const float *h, const float *lw);
int launch_tridiag_reg(const Switches &sw, int D, int64_t nb, const Ws &ws, hipStream_t st, const float2 *Zlow, const float2 *phi, const float *h,
                       const float *lw);   // tridiag_reg.hip, D <= 128
int launch_tridiag_big(const Switches &sw, int D, int64_t nb, const Ws &ws, hipStream_t st, bool panel, bool explicit_q);   // tridiag_big.hip, 128 < D <= 256
bool tridiag_panel_supported(int D);                                      // tridiag_panel.hip, D == 256
int launch_tridiag_panel(const Switches &sw, int D, int64_t nb, const Ws &ws, hipStream_t st, bool explicit_q);
int64_t tridiag_panel_tail_elems();                                       // float2 per matrix of Ws::Tail
int launch_wy_apply(int D, int64_t nb, const Ws &ws, hipStream_t st);     // wy_apply.hip: V = Q W without forming Q
// tql.hip
int launch_tql(int n, int64_t nb, const Ws &ws, int32_t *status, hipStream_t st);
// rotapply.hip
int launch_rotapply(int D, int64_t nb, const Ws &ws, hipStream_t st);
// rebuild.hip
int launch_dc(const Switches &sw, int n, int64_t nb, const Ws &ws, int32_t *status, hipStream_t st, bool rowmajor,
              bool colmap);   // dc.hip (colmap: leave the top level's deflated columns in place, write Ws::Wmap)
int64_t dc_final_offset(int n);                                                            // dc.hip
int launch_vgemm(int D, int64_t nb, const Ws &ws, hipStream_t st);                       // dc.hip
bool vgemm_big_supported(int D);                                                          // vgemm_big.hip
int launch_vgemm_big(int D, int64_t nb, const Ws &ws, hipStream_t st);                   // vgemm_big.hip (reads WT)
int launch_peaks(const float2 *phi, int64_t B, int xbase, int ybase, const double *Z, int nx, int ny,
                 const double *axis_x, const double *axis_y, const double *opt7, int iters, int max_peaks,
                 double *peaks, int32_t *counts, hipStream_t st);                          // peaks.hip
int launch_estimate(const float2 *phi, int64_t B, int xbase, int ybase, const double2 *tabD, int nx,
                    const double2 *tabS, int ny, const double *axis_x, const double *axis_y, const double *opt7,
                    int iters, int L, const int32_t *top_n, double *top, int32_t *counts, hipStream_t st);   // estimate.hip
bool arrow_rebuild_supported(int D);                                                       // arrow.hip
int launch_arrow_rebuild(const Route &r, const Switches &sw, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *G, float *rn,
                         float *w_out, int32_t *status, const Ws &ws, hipStream_t st, bool lower_only);   // arrow.hip: r.first
bool back_rebuild_supported(int D);                                                        // backrebuild.hip
int launch_back_rebuild(const Switches &sw, int D, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *G,
                        float *rn, float *w_out, const Ws &ws, hipStream_t st, bool lower_only);   // backrebuild.hip
// form: RB_BIG or RB_TILES; image_dim: the dimension the eigenvector image ws.VT is laid out for (Route::eig_dim behind the
// dense pipeline, D itself behind the arrowhead solver of the first layer)
int launch_rebuild(int D, int64_t nb, const float *lw, const float2 *phi, const float *h,
                   float2 *G, float *rn, float *w_out, const Ws &ws, hipStream_t st, bool lower_only, Rebuild form,
                   int image_dim);
int launch_vout(int n, int64_t nb, float2 *V, float *w, const Ws &ws, int eig_dim, hipStream_t st);
bool rebuild_big_supported(int D);                                                        // rebuild_big.hip, image dimension 256
int launch_rebuild_big(int D, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *G, float *rn,
                       const Ws &ws, hipStream_t st, bool lower_only);
// zstep.hip
int launch_rn_sum(int64_t B, const float *rn, double *sum, hipStream_t st);
int launch_mean_from_sum(const double *sum, int64_t B, float *mean, hipStream_t st);
int launch_mean_from_pair(const double *sum_count, float *mean, hipStream_t st);   // mean = sum_count[0] / sum_count[1]
int launch_zstep(const float *lw, int D, int64_t B, const float *rn, const float *mean, float *alpha, hipStream_t st);
// sub-batches of g signals (admmnet_cfg.sub_batch): pairs [ceil(B / g)][2] = (sum, count) per group, each with the bits
// launch_rn_sum gives that group alone; mean [ceil(B / g)]; zstep reads the mean of signal i's group i / g
int launch_rn_group_sum(int64_t B, int64_t g, const float *rn, double *pairs, hipStream_t st);
int launch_mean_from_pairs(const double *pairs, int64_t ngroups, float *mean, hipStream_t st);
int launch_zstep_groups(const float *lw, int D, int64_t B, int64_t g, const float *rn, const float *mean, float *alpha,
                        hipStream_t st);
// head.hip
int launch_head(const admmnet_cfg *cfg, const float *hw, int64_t B, const float2 *phi, float *kv,
                float *out, hipStream_t st);
// spectrum.hip
int launch_spectrum_tables(const double *taus, int nx, int xbase, const double *fs, int ny, int ybase,
                           double2 *tabD, double2 *tabS, hipStream_t st);
int launch_spectrum_main(const float2 *phi, int64_t B, int xbase, int ybase, const double2 *tabD, int nx,
                         const double2 *tabS, int ny, double *out, hipStream_t st);

// spectral.hip (form: MF_KERNELS, the five kernels there) / spectral_fused.hip (MF_FUSED: the whole evaluation in one kernel)
int launch_spectral_fused(const Switches &sw, int D, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *Z,
                          float2 *G, float *rn, int *flag, int32_t *status, const float *alpha, const float2 *phi_prev,
                          const float *h_prev, const float *lw_prev, int update_mode, int waves, float *diag, int *diag_ok, hipStream_t st);
// update_mode 0: Z is current; 1 / 2: the fused kernel applies Z <- Z + alpha (G - C_prev) in its first sweep (2: stored Z still zero)
// diag, diag_ok: Ws::diag / Ws::diag_ok of the chunk's first matrix, or both null: nothing is written
// waves: spectral_waves(D, B, sw) of the call the chunk belongs to; sw: the call's tolerance, pass cap and phase timer
int launch_spectral(const Switches &sw, int D, int64_t nb, const float *lw, const float2 *phi, const float *h, float2 *Z, float2 *G,
                    float *rn, const Ws &ws, int32_t *status, hipStream_t st, MatFun form, int waves, const float *alpha,
                    const float2 *phi_prev, const float *h_prev, const float *lw_prev, int update_mode, float *diag, int *diag_ok);
// vdvh.hip (training route)
int launch_vdvh(int n, int64_t nb, const float2 *V, const float *d, float2 *out, hipStream_t st);
int launch_vhsv(int n, int64_t nb, const float2 *V, const float2 *S, float *q, hipStream_t st);
// train_layer.hip (training route, the n^2-sized layer steps; r, s: device values)
int train_tile_pairs(int n);
int launch_train_matrix(int n, int64_t B, const float2 *phi, const float *h, const float2 *Z, const float *r, float corner,
                        float2 *A, hipStream_t st);
int launch_train_matrix_bwd(int n, int64_t B, const float2 *gA, const float2 *Z, const float *r, float2 *gZ, float2 *gphi,
                            float *gh, float *gr, float *part, hipStream_t st);
int launch_train_resnorm(int n, int64_t B, const float2 *G, const float2 *phi, const float *h, float corner, float *rn,
                         hipStream_t st);
int launch_train_resnorm_bwd(int n, int64_t B, const float *grn, const float *rn, const float2 *G, const float2 *phi,
                             const float *h, float corner, float2 *gG, float2 *gphi, float *gh, hipStream_t st);
int launch_train_zupdate(int n, int64_t B, const float2 *Z, const float2 *G, const float2 *phi, const float *h, const float *s,
                         float corner, float2 *Zn, hipStream_t st);
int launch_train_gather(int n, int64_t B, const float2 *X, float2 *col, float *dg, hipStream_t st);
int launch_train_scatter(int n, int64_t B, const float2 *gcol, const float *gdg, float2 *gX, hipStream_t st);
int launch_train_herm(int n, int64_t B, const float2 *g, const float2 *gcol, const float *gdg, float2 *S, hipStream_t st);
int launch_train_zupdate_bwd(int n, int64_t B, const float2 *g, const float2 *G, const float2 *phi, const float *h,
                             const float *s, float corner, float2 *gG, float2 *gphi, float *gh, float *gs, hipStream_t st);

// train_small.hip (training route "full", the O(B D)-sized layer steps; every parameter pointer is the RAW device value)
int64_t train_small_rows(int64_t B);                  // partial rows of the per-signal kernels: one per slab of signals
int64_t train_small_groups(int64_t B, int64_t g);     // groups of the step-size kernels (g = 0: one)
int launch_train_phi(int D, int64_t B, const float2 *y, const float2 *b, const float2 *gcol, const float2 *zcol,
                     const float *rho_raw, float2 *phi, hipStream_t st);
int launch_train_phi_bwd(int D, int64_t B, const float2 *gphi, const float2 *y, const float2 *b, const float2 *gcol,
                         const float2 *zcol, const float *rho_raw, float2 *ggcol, float2 *gzcol, float *grho, float *part,
                         hipStream_t st);
int launch_train_hinput(int D, int64_t B, const float *gdg, const float *zdg, const float *rho_raw, float *t, hipStream_t st);
int launch_train_hinput_bwd(int D, int64_t B, const float *gt, const float *zdg, const float *rho_raw, float *ggdg, float *gzdg,
                            float *grho, float *part, hipStream_t st);
int launch_train_hproject(int D, int64_t B, const float *t, const float *m, const float *sigma, const float *pw_raw, float *h,
                          hipStream_t st);
int launch_train_hproject_bwd(int D, int64_t B, const float *gh, const float *t, const float *m, const float *sigma,
                              const float *pw_raw, float *gt, float *gm, float *gpw, float *part, hipStream_t st);
int launch_train_eigmap(int n, int64_t B, const float *w, const float *thr, const float *W1, const float *b1, const float *W2,
                        const float *b2, float *wp, hipStream_t st);
int launch_train_eigmap_bwd(int n, int64_t B, const float *gwp, const float *w, const float *thr, const float *W1, const float *b1,
                            const float *W2, const float *b2, float *gw, float *gpar, float *part, hipStream_t st);
int launch_train_stepsize(int64_t B, int64_t g, float knorm, const float *rn, const float *rho_raw, const float *W1,
                          const float *b1, const float *W2, const float *b2, float *step, hipStream_t st);
int launch_train_stepsize_bwd(int64_t B, int64_t g, float knorm, const float *gstep, const float *rn, const float *rho_raw,
                              const float *W1, const float *b1, const float *W2, const float *b2, float *grn, float *gpar,
                              float *part, hipStream_t st);
// the step size from an outside (sum, count) pair: slabs of 256 signals, one thread each
int64_t train_pair_rows(int64_t B);                   // slabs of the pair kernels
int64_t train_pair_partials(int64_t B);               // floats of `part`: one double and 162 floats per slab
int launch_train_rnsum(int64_t B, const float *rn, double *pair, hipStream_t st);
int launch_train_stepsize_pair(int64_t B, float knorm, const float *rn, const double *pair, const float *rho_raw, const float *W1,
                               const float *b1, const float *W2, const float *b2, float *step, hipStream_t st);
int launch_train_stepsize_bwd_pair_front(int64_t B, float knorm, const float *gstep, const float *rn, const double *pair,
                                         const float *rho_raw, const float *W1, const float *b1, const float *W2, const float *b2,
                                         float *gu, float *gpar, double *total, float *part, hipStream_t st);
int launch_train_stepsize_bwd_pair_back(int64_t B, const float *gu, const double *pair, const double *total, float *grn,
                                        hipStream_t st);

// train_hlayer.hip (training route "native": the H layer with its correction_net inside; parameters RAW as in train_small.hip)
int64_t train_hlayer_workspace_floats(int D, int64_t B);   // float scratch of the backward: slab rows, then the batch-slab partials
int launch_train_hlayer(int D, int64_t B, const float *gdg, const float *zdg, const float *sigma, const float *rho_raw,
                        const float *pw_raw, const float *W1, const float *b1, const float *W2, const float *b2, float *h, float *t,
                        float *a1, float *m, hipStream_t st);
int launch_train_hlayer_bwd(int D, int64_t B, const float *gh, const float *zdg, const float *sigma, const float *rho_raw,
                            const float *pw_raw, const float *W1, const float *W2, const float *t, const float *a1, const float *m,
                            float *ggdg, float *gzdg, float *d1, float *d2, float *gpar, float *work, hipStream_t st);

// train_head.hip (training route "native": the PeakSearchLayer head; `params` is a HOST array of the 21 + 8 L device pointers to the
// RAW parameters in the order of training._head_params)
int64_t train_head_saved_floats(int D, int L, int64_t B);   // the forward's saved activations
int64_t train_head_work_floats(int D, int L, int64_t B);    // the backward's deltas and slab partials
int64_t train_head_grad_floats(int D, int L);               // the backward's gradient buffer
int launch_train_head(int D, int L, int64_t B, const float2 *phi, const float *const *params, const unsigned char *keep, float p,
                      float *tau, float *f, float *conf, float *saved, hipStream_t st);
int launch_train_head_bwd(int D, int L, int64_t B, const float *gtau, const float *gf, const float *gconf, const float2 *phi,
                          const float *const *params, const unsigned char *keep, float p, const float *tau, const float *f,
                          const float *conf, float *saved, float2 *gphi, float *g, float *work, hipStream_t st);

// loss.hip (the training losses; sums over the batch as in train_small.hip)
int64_t loss_partials(int loss, int64_t B);           // floats of partial-sum scratch of the forward of ADMMNET_LOSS_*
int launch_loss_anm(int Lmax, int D, int64_t B, const float *tau, const float *f, const float *conf, const float *tau_true,
                    const float *f_true, const int64_t *L_true, const float2 *phi, float lambda_reg, float *out, float *norms,
                    int32_t *status, float *part, hipStream_t st);
int launch_loss_anm_bwd(int Lmax, int D, int64_t B, const float *g_out, const float *tau, const float *f, const float *conf,
                        const float *tau_true, const float *f_true, const int64_t *L_true, const float2 *phi, const float *norms,
                        float lambda_reg, float *g_tau, float *g_f, float *g_conf, float2 *g_phi, hipStream_t st);
int launch_loss_phi(int D, int64_t B, const float2 *phi, const float2 *phi_true, float amplitude_weight, float phase_weight,
                    float *out, float *part, hipStream_t st);
int launch_loss_phi_bwd(int D, int64_t B, const float *g_out, const float2 *phi, const float2 *phi_true, float amplitude_weight,
                        float phase_weight, float2 *g_phi, hipStream_t st);

// loss_set.hip (the assignment loss of the head: slots matched to targets by the assignment that minimises the loss; one wave per
// signal, float64, one row of partials per signal).  opts: HOST double[6] = sx, sy, period_tau, period_f, w_conf, lambda_reg
int64_t loss_set_partials(int64_t B);                 // doubles of per-signal rows of the forward
int launch_loss_set(int Lmax, int Lt, int D, int64_t B, const float *tau, const float *f, const float *conf, const float *tau_true,
                    const float *f_true, const int64_t *L_true, const float2 *phi, const double *opts, float *out, int32_t *assign,
                    float *norms, int32_t *status, double *part, hipStream_t st);
int launch_loss_set_bwd(int Lmax, int Lt, int D, int64_t B, const float *g_out, const float *tau, const float *f, const float *conf,
                        const float *tau_true, const float *f_true, const int64_t *L_true, const float2 *phi, const int32_t *assign,
                        const float *norms, const double *opts, float *g_tau, float *g_f, float *g_conf, float2 *g_phi,
                        hipStream_t st);

// loss_spectrum.hip (the spectral, distribution and target terms of the phi loss on the delay-Doppler spectrum; one workgroup
// per signal, float64).  phi_true == nullptr: no grid terms; L_true == nullptr: no target term.
constexpr int LS_MAX_TARGETS = 16, LS_MAX_OVERSAMPLE = 4;
int64_t loss_spectrum_workspace_bytes(int xbase, int ybase, int oversample, int64_t B);   // -1: does not fit
int launch_loss_spectrum(int xbase, int ybase, int oversample, int Lmax, int64_t B, const float2 *phi, const float2 *phi_true,
                         const float *tau_true, const float *f_true, const int64_t *L_true, float spectral_weight,
                         float distribution_weight, float target_weight, float *out, int32_t *status, void *workspace,
                         hipStream_t st);
int launch_loss_spectrum_bwd(int xbase, int ybase, int oversample, int Lmax, int64_t B, const float *g_out, const float2 *phi,
                             const float *tau_true, const float *f_true, const int64_t *L_true, float spectral_weight,
                             float distribution_weight, float target_weight, int skip, const void *workspace, float2 *g_phi,
                             hipStream_t st);

// score.hip (estimates against ground truth: the truncated-cost assignment and the ordered RMSE; float64 sums over the batch)
int64_t score_partials(int64_t B);                    // doubles of partial-sum scratch of either call
int launch_score_match(int Le, int Lt, int64_t B, const double *est, const int32_t *n_est, const float *tau_true,
                       const float *f_true, const int64_t *L_true, const double *opts, int32_t *match, double *stats, double *totals,
                       int32_t *status, double *part, hipStream_t st);
int launch_score_ordered(int Lmax, int64_t B, const float *tau_est, const float *f_est, const float *tau_true, const float *f_true,
                         const int64_t *L_true, double *per_sample, double *out, int32_t *status, double *part, hipStream_t st);

// crb.hip (the Cramer-Rao bound of a scene's targets; 1 <= Lt <= 16)
int64_t crb_partials(int64_t B);                      // doubles of partial-sum scratch
int launch_crb(int Nb, int Nd, int Lt, int64_t B, const float *tau_true, const float *f_true, const float2 *C,
               const int64_t *L_true, const int32_t *match, const double *noise, int noise_is_snr, double *bound, double *totals,
               int32_t *status, double *part, hipStream_t st);

// refine.hip (target estimates refined against the received signal; 1 <= Le <= 16)
int64_t refine_lds_bytes(int Nb, int Nd, int Le);     // dynamic + static LDS of one workgroup
int64_t refine_lds_limit();
int launch_refine(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_est,
                  int mode, int psk_m, double psk_phase, int iters, double tol, double *rows_out, double2 *C_out, double *info,
                  int32_t *symbols_out, int32_t *status, hipStream_t st);

// order.hip (the number of targets of a scene selected among candidate rows; 1 <= Le <= 16)
int64_t order_lds_bytes(int Nb, int Nd, int Le);      // dynamic LDS of one workgroup
int64_t order_lds_limit();
int launch_order(int Nb, int Nd, int Le, int64_t B, const float2 *y, const float2 *b, const double *rows_in, const int32_t *n_cand,
                 const int32_t *n_held, const int32_t *symbols, int psk_m, double psk_phase, double penalty, int max_order,
                 int32_t *perm, int32_t *n_sel, double *rss, double *rows_out, double2 *C_out, float2 *residual, double *info,
                 int32_t *status, hipStream_t st);

// cfar.hip (a CFAR detector on the zero-padded periodogram of a scene; 1 <= r <= 8, 1 <= Le <= 16)
int64_t cfar_lds_bytes(int Nb, int Nd, int r);         // dynamic LDS of one workgroup
int64_t cfar_lds_limit();
int launch_cfar(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, double *rows,
                int32_t *counts, double *info, double *map_out, int32_t *status, hipStream_t st);

// cfar_relax.hip (successive cancellation with cyclic re-fitting on that periodogram; 0 <= iters <= 16, 0 <= sweeps <= 8)
int64_t cfar_relax_lds_bytes(int Nb, int Nd, int r);   // dynamic LDS of one workgroup
int64_t cfar_relax_lds_limit();
int launch_cfar_relax(int Nb, int Nd, int r, int Le, int64_t B, const float2 *y, const float2 *b, const int32_t *symbols, int psk_m,
                      double psk_phase, int method, int guard, int train, int rank, double alpha, const double *noise_var, int iters,
                      int sweeps, double *rows, double *amp, int32_t *counts, double *info, double *map_out, int32_t *status,
                      hipStream_t st);

// optim.hip (AdamW and gradient-norm clipping over a tensor list; host arrays of device pointers)
int64_t optim_blocks(int count, const int64_t *numel);   // blocks of the list = doubles of `partials`; -1: bad count or too many
int launch_optim_gradnorm(int count, const float *const *grads, const int64_t *numel, float max_norm, double *partials,
                          double *sumsq, float *total_norm, float *coef, hipStream_t st);
int launch_optim_scale(int count, float *const *grads, const int64_t *numel, const float *coef, hipStream_t st);
int launch_optim_adamw(int count, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                       const int64_t *numel, const int32_t *hyper_index, const admmnet_adamw_hyper *hyper, const float *coef,
                       hipStream_t st);
// tensors -> flat (to_flat) or flat -> tensors, in list order
int launch_optim_bucket(int count, float *const *tensors, const int64_t *numel, float *flat, bool to_flat, hipStream_t st);

// synth.hip
int64_t synth_max_cells();                            // the largest Nb * Nd a scene may have
int launch_synth(int64_t B, int Nb, int Nd, int L, unsigned long long seed, double snr_lo, double snr_hi, double snr_e,
                 double rho, int label_iters, float2 *y, float2 *b, float *sigma, float *tau, float *f, float2 *C,
                 float2 *phi_label, hipStream_t st);
int launch_synth_scenes(int64_t B, int Nb, int Nd, int L_min, int L_max, double min_sep, unsigned long long seed, double snr_lo,
                        double snr_hi, double snr_e, double rho, int label_iters, float2 *y, float2 *b, float *sigma,
                        float *tau, float *f, float2 *C, float2 *phi_label, int64_t *L_true, double *snr_db,
                        double *noise_var, float *ser, int32_t *state, hipStream_t st);

// ---- optional per-kernel-class HIP-event profiler (bench.py roofline leg) ------
enum KernelClass { KC_PREP = 0, KC_TRIDIAG, KC_TQL, KC_ROTAPPLY, KC_REBUILD, KC_ZSTEP, KC_HEAD, KC_SPECTRUM, KC_GFUNC, KC_COUNT };
struct ProfScope {   // records start/stop events on `st` around a launcher body when profiling is on
    int slot;
    hipStream_t st;
    ProfScope(int kclass, hipStream_t s);
    ~ProfScope();
};

// ---- developer phase timers (ADMMNET_*_TIMING) ----------------------------------
// n zeroed device counters for one launch (dev stays null when off); end() copies them back, synchronises and frees
struct PhaseTimer {
    unsigned long long *dev = nullptr;
    int n = 0;
    int begin(bool on, hipStream_t st, int n_counters) {
        if (!on) return ADMMNET_OK;
        n = n_counters;
        ADMM_HIP(hipMalloc(&dev, n * sizeof(unsigned long long)));
        ADMM_HIP(hipMemsetAsync(dev, 0, n * sizeof(unsigned long long), st));
        return ADMMNET_OK;
    }
    int end(hipStream_t st, unsigned long long *host) {
        ADMM_HIP(hipMemcpyAsync(host, dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        ADMM_HIP(hipStreamSynchronize(st));
        ADMM_HIP(hipFree(dev));
        return ADMMNET_OK;
    }
};

// ---- small device helpers ---------------------------------------------------
// the float register vectors, declared here only: a (re, im) pair for the packed complex arithmetic of lane_reduce.h, the
// four / sixteen accumulator registers of a 16 x 16 / 32 x 32 MFMA tile
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {  // a * conj(b)
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ float2 cmacc(float2 acc, float2 a, float2 b) {  // acc + conj(a) * b
    acc.x = fmaf(a.x, b.x, fmaf(a.y, b.y, acc.x));
    acc.y = fmaf(a.x, b.y, fmaf(-a.y, b.x, acc.y));
    return acc;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the same butterfly in float64 (lane_reduce.h's DPP forms are float-only)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

}  // namespace admmnet
