/*
 * admmnet.h -- C ABI of the MI355X (gfx950) ADMM-Net forward path.
 *
 * This is the drop-in boundary for ONE hot path of E-J408/admm-net: the
 * K-layer unrolled ADMM-Net forward.  Every entry point names the reference
 * interface it replaces (file:line under /root/reference).  The reference is
 * pure Python/torch with no FFI of its own, so the "binding a maintainer would
 * add" is the ctypes stub shown in INTEGRATION.md (admm_net_amd/_lib.py is that
 * stub, shipped).
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns 0 on
 *     success or a negative ADMMNET_E_* code, message via admmnet_last_error()
 *     (thread-local).
 *   - the CALLER owns every buffer (device and host); nothing here allocates
 *     device memory.  All device work is enqueued on the caller's stream and is
 *     asynchronous; no call synchronises the device.  (admmnet_layer_front may
 *     run part of a layer on an internal stream beside the caller's, ordered
 *     by events and joined before it returns: what the caller enqueues next on
 *     its stream runs behind all of it.  INTEGRATION.md section 6,
 *     ADMMNET_STREAMS.)
 *   - device = the caller's current HIP device.
 *   - complex64 = interleaved (re, im) float pairs, as torch.complex64.
 *   - D = M*N (signal length), n = D + 1 (state dimension), B = batch,
 *     K = number of unrolled layers.
 *   - which kernels serve a call, and with which tolerances, is decided per
 *     call from an OPTION SET (the switches of INTEGRATION.md section 6).  The
 *     environment gives the process defaults, read once; admmnet_options_intern
 *     turns overrides of them into a handle that admmnet_cfg carries, so two
 *     models of one process can run different routes.  Apart from that
 *     append-only table of immutable entries and the defaults, the library
 *     keeps no state between calls: every entry point is re-entrant.
 */
#ifndef ADMMNET_H
#define ADMMNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADMMNET_ABI_VERSION 1

enum {
    ADMMNET_OK = 0,
    ADMMNET_E_ARG = -1,        /* bad argument / unsupported shape            */
    ADMMNET_E_HIP = -2,        /* a HIP runtime call failed                   */
    ADMMNET_E_WORKSPACE = -3,  /* workspace too small                         */
    ADMMNET_E_NOCONV = -4      /* eigensolver did not converge / log overflow  */
};

/* Model geometry: admm_net.py:726-741 / :770-789 (ctor arguments). */
typedef struct admmnet_cfg {
    int32_t M;          /* reference "M" (= Nb)                                */
    int32_t N;          /* reference "N" (= Nd)                                */
    int32_t L;          /* max targets of the PeakSearchLayer head (3)         */
    int32_t K;          /* num_layers                                          */
    int32_t has_head;   /* 1: ADMMNet (PeakSearchLayer), 0: PhiEstADMMNet       */
    int32_t chunk;      /* signals per eigensolver work chunk (0 = auto); a
                           work split only: the bits of a signal depend on its
                           inputs, the weights, the batch mean and the batch
                           size B of the call (of its sub-batch, below), never
                           on chunk (a rank of a sharded forward is one call) */
    int32_t sub_batch;  /* 0: the call is one batch (admm_net.py:459 takes its
                           mean over all B signals).  g >= 1: the signals
                           [j g, min((j + 1) g, B)) form sub-batch j, of
                           ngroups = ceil(B / g), each with its own mean; every
                           sub-batch gets the bits a separate call on it alone
                           returns (g >= B: one sub-batch).  < 0: ADMMNET_E_ARG */
    int32_t reserved[1]; /* [0]: option handle of admmnet_options_intern; 0 =
                           the process defaults.  A handle never issued is
                           ADMMNET_E_ARG, before anything is enqueued.  One
                           forward uses ONE cfg, handle included, from
                           admmnet_workspace_bytes through admmnet_finish:
                           every call carves the workspace from the cfg it
                           is given                                         */
} admmnet_cfg;

int         admmnet_abi_version(void);
const char *admmnet_last_error(void);

/* ---- option sets ------------------------------------------------------------
 * admmnet_options_intern: the process defaults (environment over built-in values)
 *   overridden by count (name, value) pairs in the environment's own names and
 *   syntax, e.g. {"ADMMNET_SPECTRAL", "0"}; of two pairs with one name the later
 *   wins.  Returns a handle >= 1 for admmnet_cfg.reserved[0], or 0 when count == 0
 *   or nothing differs from the defaults; ADMMNET_E_ARG for a name that is no
 *   switch, a NULL name or value, or a full table (4096 distinct sets), with the
 *   name in admmnet_last_error().  Sets are compared by their RESOLVED settings:
 *   the same settings always give the same handle, whatever the order or the
 *   spelling ("0" and "00").  Handles are immutable and valid for the life of
 *   the process; the call is thread-safe.  A combination that no kernel serves
 *    still interns: the entry point that would run it
 *   returns ADMMNET_E_ARG before it enqueues anything, for that cfg only.
 * admmnet_options_describe: the resolved settings of a handle (0: the defaults)
 *   as "NAME value" lines, one per switch, NUL-terminated into buf[len].  Returns
 *   the length of the whole text (cut to len - 1 characters if buf is smaller),
 *   ADMMNET_E_ARG for a handle never issued. */
int32_t admmnet_options_intern(const char *const *names, const char *const *values, int32_t count);
int64_t admmnet_options_describe(int32_t handle, char *buf, int64_t len);

/* ---- weights -------------------------------------------------------------
 * Raw (host) order, all float32, concatenated:
 *   for k in 0..K-1:
 *     phiLayers.k.rho
 *     hLayers.k.rho, hLayers.k.projection_weight,
 *     hLayers.k.correction_net.0.weight[64][D], .0.bias[64],
 *     hLayers.k.correction_net.2.weight[D][64], .2.bias[D]
 *     gLayers.k.lambda_param, gLayers.k.rho, gLayers.k.threshold,
 *     gLayers.k.value_net.0.weight[16], .0.bias[16], .2.weight[16], .2.bias[1]
 *     zLayers.k.rho, zLayers.k.lambda_param,
 *     zLayers.k.residual_scale_net.0.weight[32][3], .0.bias[32], .2.weight[32], .2.bias[1]
 *   if has_head: peakSearchLayer.* in this order:
 *     position_encoder[D][2], feature_extractor.0.{weight[128][2D],bias[128]},
 *     feature_extractor.2.{weight[128][128],bias[128]},
 *     position_projection.{weight[128][2],bias[128]},
 *     attention.in_proj_weight[384][128], in_proj_bias[384],
 *     attention.out_proj.{weight[128][128],bias[128]},
 *     peak_extractor.0.{weight[64][128],bias[64]}, .2.{[32][64],[32]}, .4.{[16][32],[16]},
 *     for t in 0..L-1: tau_regressor.t.0.{[32][16],[32]}, .2.{[32],[1]},
 *                      f_regressor.t.0.{[32][16],[32]},   .2.{[32],[1]}
 *     confidence_net.0.{[16][16],[16]}, .2.{[16],[1]}
 * (zLayers.k.step_adjust_net is in the state_dict but never used by forward,
 *  admm_net.py:381-386, and is not part of the raw buffer.)
 *
 * admmnet_pack_weights resolves every softplus / sigmoid / reciprocal scalar
 * on the host (replaces the three .item() host syncs per layer at
 * admm_net.py:271,426,458) and lays the MLPs out for coalesced device reads.
 */
int64_t admmnet_raw_weight_count(const admmnet_cfg *cfg);     /* floats */
int64_t admmnet_packed_weight_count(const admmnet_cfg *cfg);  /* floats */
int     admmnet_pack_weights(const admmnet_cfg *cfg, const float *raw_host,
                             float *packed_host);

/* ---- workspace -------------------------------------------------------------*/
/* (with cfg->sub_batch > 0 it includes one (sum, count) pair and one mean per sub-batch) */
int64_t admmnet_workspace_bytes(const admmnet_cfg *cfg, int64_t B);

/* ---- whole forward ----------------------------------------------------------
 * Replaces PhiEstADMMNet.forward (admm_net.py:742-764) and ADMMNet.forward
 * (admm_net.py:791-816) with the batch mean of ZLayer (admm_net.py:459) taken
 * over the B signals of this call, or over each sub-batch of cfg->sub_batch signals.
 *   y, b      device complex64 [B][D]
 *   sigma     device float32   [B]
 *   phi_out   device complex64 [B][D]
 *   head_out  device float32   [3][B][L] (tau, f, confidence) or NULL
 *   status    device int32     [4] or NULL, zeroed by the call: [0] = #matrices whose eigensolver
 *             failed (must be 0).  The G-layer (admm_net.py:237-354: eigh, eigenvalue map f, V f(L) V^H) is
 *             evaluated as a matrix function wherever the per-matrix checks of csrc/spectral.hip allow it
 *             (ADMMNET_SPECTRAL=0 in the environment or the option set: never) and through the eigensolver otherwise; [1] = #matrix-layers that
 *             went through the eigensolver: those the matrix-function kernel rejected (it counts them), or, with that route
 *             off for the call, every matrix of every dense layer -- all G-layers but an arrowhead first one -- set by
 *             admmnet_layer_front, saturating at INT32_MAX (the building blocks below report word [0] only), [2] = #matrix-layers evaluated as a matrix
 *             function, [3] = of [1], those rejected because f is not a quadratic on the bulk of the spectrum.
 */
int admmnet_forward_f32(const admmnet_cfg *cfg, const float *weights_dev,
                        const void *y, const void *b, const float *sigma,
                        int64_t B, void *phi_out, float *head_out,
                        void *workspace, int64_t workspace_bytes,
                        int32_t *status, void *stream);

/* ---- layer-at-a-time API (multi-GPU "global" batch-mean scope) --------------
 * layer_front(k): lazy Z update with the step of layer k-1, phi/H/G of layer k
 *   (admm_net.py:806-810) and r_b = ||G_b - C_b||_F; writes the LOCAL sum of
 *   r_b to sum_out[0] and the local count B to sum_out[1] (device float64 [2]).
 *   With cfg->sub_batch > 0: sum_out is device float64 [ngroups][2], the
 *   (sum, count) pair of every sub-batch.  For k == K-1 only phi is produced.
 * layer_back(k): ZLayer step (admm_net.py:443-474) from a caller-supplied
 *   batch mean (device float, e.g. all-reduced sum / global B); with
 *   cfg->sub_batch > 0, mean_dev is device float [ngroups], one per sub-batch.
 * begin() zeroes the per-forward state; finish() writes phi_out (+ head).
 */
int admmnet_begin(const admmnet_cfg *cfg, int64_t B, void *workspace,
                  int64_t workspace_bytes, int32_t *status, void *stream);
int admmnet_layer_front(const admmnet_cfg *cfg, const float *weights_dev, int32_t k,
                        const void *y, const void *b, const float *sigma, int64_t B,
                        void *workspace, double *sum_out, int32_t *status, void *stream);
int admmnet_layer_back(const admmnet_cfg *cfg, const float *weights_dev, int32_t k,
                       int64_t B, void *workspace, const float *mean_dev, void *stream);
/* The same from the (all-reduced) pair the protocol carries: sum_count_dev = device float64 [2] = (sum of r_b, number of
 * signals) over all ranks -- the mean of admm_net.py:459 is formed on the device, no host arithmetic between the calls.
 * With cfg->sub_batch > 0: device float64 [ngroups][2], the pairs layer_front wrote (sub-batches need no all-reduce). */
int admmnet_layer_back_pair(const admmnet_cfg *cfg, const float *weights_dev, int32_t k,
                            int64_t B, void *workspace, const double *sum_count_dev, void *stream);
int admmnet_finish(const admmnet_cfg *cfg, const float *weights_dev, int64_t B,
                   void *workspace, void *phi_out, float *head_out, void *stream);

/* ---- building blocks (exported for unit tests and reuse) --------------------
 * Batched Hermitian eigen-function  G = V f(Lambda) V^H  of the block matrix
 *   A = [[diag(h), phi],[phi^H, corner]] - inv_rho * Z
 * i.e. GLayer.forward (admm_net.py:237-354).  Z may be NULL (treated as 0).
 *   G_out  device complex64 [B][n][n];  w_out device float [B][n] (eigenvalues,
 *   unsorted) or NULL;  rn_out device float [B] = ||G - [[diag h, phi],[phi^H,
 *   corner_z]]||_F or NULL.
 *   layer_weights: packed weights of ONE layer (admmnet_layer_weight_offset).
 */
int64_t admmnet_layer_weight_offset(const admmnet_cfg *cfg, int32_t k);   /* floats */
int64_t admmnet_glayer_workspace_bytes(const admmnet_cfg *cfg, int64_t B);
int admmnet_glayer_f32(const admmnet_cfg *cfg, const float *layer_weights,
                       const void *phi, const float *h, const void *Z, int64_t B,
                       void *G_out, float *w_out, float *rn_out,
                       void *workspace, int64_t workspace_bytes,
                       int32_t *status, void *stream);

/* Where the per-forward state lies in the workspace of (cfg, B): byte offsets from the workspace base, in layout order
 *   [0] G       complex64 [B][n][n]   (n = M N + 1)         [1] Z       complex64 [B][n][n]
 *   [2] phi[0]  complex64 [B][D]      [3] phi[1]            (layer k reads phi[(k - 1) & 1] and writes phi[k & 1])
 *   [4] h[0]    float32   [B][D]      [5] h[1]              (likewise)
 *   [6] alpha   float32   [B]         (the Z step of the layer before)
 *   [7] rn      float32   [B]         (the residual norms layer_front wrote)
 *   [8] the first byte behind rn's span: nothing of the above lies at or behind it
 * Every offset is a multiple of 256; a span ends at the next offset and holds its buffer from its start, the rest is padding.
 * *lower_only (may be NULL) is set to 1 where G and Z hold their lower triangles (row >= column) only -- the other triangle is
 * neither read nor written -- and to 0 where both triangles are stored; it follows the route of cfg's option set.
 * Host only: touches no device and enqueues nothing.  The answer is the carve the layer calls themselves use, so a caller
 * may read and write the state between admmnet_begin / layer_front / layer_back / finish through these offsets. */
#define ADMMNET_STATE_SPANS 8
int admmnet_state_layout(const admmnet_cfg *cfg, int64_t B, int64_t offsets[ADMMNET_STATE_SPANS + 1], int32_t *lower_only);

/* The matrix-function G-layer (csrc/spectral_fused.hip, the route of the forward's dense layers) on caller-supplied state,
 * one matrix per signal, with the forward's own tolerance and pass cap; for tests and utilities, the forward does not
 * call it.  Layout as in the workspace: n x n buffers per signal, only the lower triangle is read or written.
 *   layer_weights       packed weights of layer k
 *   phi [B][D] c64, h [B][D] f32    the inputs of layer k
 *   Z [B][n][n] c64     mode 0: input (the state G-layer k reads);
 *                       mode 1: in/out -- the Z-layer update of layer k-1 is applied first, Z <- Z + alpha_b (G - C_prev),
 *                               C_prev = [[diag h_prev, phi_prev], [phi_prev^H, corner_z of layer k-1]], G = G of layer k-1;
 *                       mode 2: as 1 with the stored Z taken as zero (never read, only written)
 *   prev_layer_weights, alpha [B] f32, phi_prev [B][D] c64, h_prev [B][D] f32: layer k-1 (modes 1, 2; else ignored)
 *   G [B][n][n] c64     G of layer k where the matrix is accepted (modes 1, 2: G of layer k-1 on entry); untouched otherwise
 *   rn_out [B] f32      ||G - [[diag h, phi], [phi^H, corner_z]]||_F where accepted; untouched otherwise
 *   flag [B] i32        0 = accepted, else the check that rejected it: 1 Ritz residual, 2 bulk not narrow against the
 *                       gaps, 4 f not a quadratic on the bulk, 8 non-finite, 16 second-order term too large
 *   status [4] i32      zeroed by the call; [1] = #rejected, [2] = #accepted, [3] = #(flag == 4)
 *   waves               0: the forward's choice for a call of B signals; 12, or 4 (D <= 128): that workgroup shape
 * D = M*N must be 8 .. 256. */
int admmnet_glayer_spectral_f32(const admmnet_cfg *cfg, const float *layer_weights,
                                const void *phi, const float *h, void *Z, int32_t mode,
                                const float *prev_layer_weights, const float *alpha,
                                const void *phi_prev, const float *h_prev, int64_t B,
                                void *G, float *rn_out, int32_t *flag, int32_t *status,
                                int32_t waves, void *stream);

/* Batched Hermitian eigendecomposition of arbitrary complex64 Hermitian
 * matrices (torch.linalg.eigh at admm_net.py:303).  A [B][n][n] (only the
 * lower triangle is read); w [B][n] unsorted; V [B][n][n] row-major,
 * columns = eigenvectors. */
int64_t admmnet_eigh_workspace_bytes(int32_t n, int64_t B);
int admmnet_eigh_c64(int32_t n, int64_t B, const void *A, float *w, void *V,
                     void *workspace, int64_t workspace_bytes,
                     int32_t *status, void *stream);
/* The same under an option set (admmnet_options_intern); the two above pass 0.  Size and call take the same handle. */
int64_t admmnet_eigh_workspace_bytes_o(int32_t n, int64_t B, int32_t options);
int admmnet_eigh_c64_o(int32_t n, int64_t B, const void *A, float *w, void *V,
                       void *workspace, int64_t workspace_bytes,
                       int32_t *status, void *stream, int32_t options);

/* Training route (trainPhi.py / train.py call forward in train mode).
 * admmnet_vdvh_c64: out = V diag(d) V^H, exactly Hermitian -- GLayer._rebuild_definite_matrix (admm_net.py:336-354: two
 *   bmm + the symmetrisation) and the backward of the eigenvalue-only eigh, dL/dA = V diag(dL/dw) V^H (admm_net.py:303-306,
 *   V detached).   V device complex64 [B][n][n] (columns = eigenvectors), d device float [B][n], out complex64 [B][n][n].
 * admmnet_vhsv_f32: its adjoint, q[c] = Re(v_c^H S v_c) for a Hermitian S (lower triangle read): the gradient of out with
 *   respect to d for an incoming S = (g + g^H) / 2.   S device complex64 [B][n][n], q device float [B][n]. */
int admmnet_vdvh_c64(int32_t n, int64_t B, const void *V, const float *d, void *out, void *stream);
int admmnet_vhsv_f32(int32_t n, int64_t B, const void *V, const void *S, float *q, void *stream);

/* Training route, the n^2-sized steps of one layer and their backwards as streaming kernels (csrc/train_layer.hip).
 * C(phi, h, c) = [[diag h, phi], [phi^H, c]] is never stored; herm(X) = (X + X^H) / 2; <X, Y> = Re sum conj(X_ij) Y_ij per
 * signal; D = n - 1 is the border index; n as for admmnet_eigh_c64 (2 ... 257), any B >= 1 with B * ceil(n/32)(ceil(n/32)+1)/2
 * below 2^31.  Matrices are device complex64 [B][n][n] with 16-byte aligned bases (otherwise the stream kernels move 8 bytes
 * per lane instead of 16), phi / g_phi complex64 [B][D], h / g_h float [B][D]; r (one float) and s [B] are DEVICE values;
 * corner is the host number the reference takes with .item().  Gradients follow torch's convention for complex tensors.
 * Every sum runs in a fixed order without atomics: two runs on the same inputs give the same bits.
 *   admmnet_train_matrix_f32      A = herm(C(phi, h, corner) - r Z), exactly Hermitian -- GLayer's block matrix, "- Z / rho"
 *                                 and symmetrisation, admm_net.py:262-300.
 *   admmnet_train_matrix_bwd_f32  from gA, with S = herm(gA): gZ = -r S, g_phi[i] = 2 S[i, D], g_h[i] = Re S[i, i],
 *                                 g_r[0] = -sum_b <S_b, Z_b> (float64 over the batch).  partials: float scratch of
 *                                 admmnet_train_partials(n, B) entries.
 *   admmnet_train_resnorm_f32     rn[b] = ||G_b - C(phi, h, corner)||_F -- ZLayer's block matrix, residual and norm,
 *                                 admm_net.py:428-459.
 *   admmnet_train_resnorm_bwd_f32 from g_rn [B], with q = g_rn / rn and R = G - C: gG = q R,
 *                                 g_phi[i] = -q (R[i, D] + conj R[D, i]), g_h[i] = -q Re R[i, i].
 *   admmnet_train_zupdate_c64     Z_new = Z + s_b (G - C(phi, h, corner)) -- the dual update, admm_net.py:460-474.
 *   admmnet_train_zupdate_bwd_c64 from g (which is also the gradient of Z, unchanged): gG = s g, g_s[b] = <R_b, g_b>,
 *                                 g_phi[i] = -s (g[i, D] + conj g[D, i]), g_h[i] = -s Re g[i, i].
 * The border column and the diagonal are all that PhiLayer (admm_net.py:98-99) and HLayer (:150-152) read of G and Z:
 *   admmnet_train_gather_c64      col[b][i] = X[b][i][D], diag[b][i] = Re X[b][i][i], i < D.
 *   admmnet_train_scatter_c64     its backward: gX = E(g_col, g_diag), the matrix with g_col in the border column, g_diag on
 *                                 the diagonal (rows < D) and zeros elsewhere, written in one pass.
 *   admmnet_train_herm_c64        S = herm(g + E(g_col, g_diag)), exactly Hermitian: the symmetrisation in the backward of the
 *                                 rebuild (admm_net.py:354) with the gather's gradient folded in; g_col and g_diag may both
 *                                 be null (S = herm(g)). */
int64_t admmnet_train_partials(int32_t n, int64_t B);
int admmnet_train_matrix_f32(int32_t n, int64_t B, const void *phi, const float *h, const void *Z, const float *r, float corner,
                             void *A, void *stream);
int admmnet_train_matrix_bwd_f32(int32_t n, int64_t B, const void *gA, const void *Z, const float *r, void *gZ, void *g_phi,
                                 float *g_h, float *g_r, float *partials, void *stream);
int admmnet_train_resnorm_f32(int32_t n, int64_t B, const void *G, const void *phi, const float *h, float corner, float *rn,
                              void *stream);
int admmnet_train_resnorm_bwd_f32(int32_t n, int64_t B, const float *g_rn, const float *rn, const void *G, const void *phi,
                                  const float *h, float corner, void *gG, void *g_phi, float *g_h, void *stream);
int admmnet_train_zupdate_c64(int32_t n, int64_t B, const void *Z, const void *G, const void *phi, const float *h,
                              const float *s, float corner, void *Z_new, void *stream);
int admmnet_train_zupdate_bwd_c64(int32_t n, int64_t B, const void *g, const void *G, const void *phi, const float *h,
                                  const float *s, float corner, void *gG, void *g_phi, float *g_h, float *g_s, void *stream);
int admmnet_train_gather_c64(int32_t n, int64_t B, const void *X, void *col, float *diag, void *stream);
int admmnet_train_scatter_c64(int32_t n, int64_t B, const void *g_col, const float *g_diag, void *gX, void *stream);
int admmnet_train_herm_c64(int32_t n, int64_t B, const void *g, const void *g_col, const float *g_diag, void *S, void *stream);

/* Training route "full", the O(B D)-sized steps of one layer and their backwards (csrc/train_small.hip): one kernel per
 * forward, one (plus a float64 sum over the batch) per backward.  D = M N <= 256, n = D + 1, B >= 1.  [B][D] tensors are dense
 * and need only their natural alignment (4 bytes float, 8 bytes complex64).  Every PARAMETER pointer (rho, projection_weight,
 * threshold, W1, b1, W2, b2) is the RAW device value: the kernels apply softplus (beta 1, linear above 20) / sigmoid
 * themselves, and the backwards return the gradients of the raw values.  eps = 1e-8.  relu'(0) = 0, d|x|/dx = 0 at 0,
 * the clamp passes the gradient where its argument is <= 1, the gradient of max|.| goes to the lowest index among ties.
 * Sums over the batch run in a fixed order without atomics (float64 across workgroups): two runs give the same bits.
 * `partials` is float scratch of admmnet_train_small_partials(step, B, sub_batch) entries (sub_batch read for STEPSIZE only).
 *   admmnet_train_phi_c64          phi = bs / (1 + rho bs) (y / (b + eps) + rho g_col + z_col), rho = softplus(*rho),
 *                                  bs = |b|^2 + eps; all tensors complex64 [B][D] -- PhiLayer, admm_net.py:79-105.
 *   admmnet_train_phi_bwd_c64      from g_phi: g_gcol, g_zcol [B][D] complex64 (torch's convention), g_rho[0].
 *   admmnet_train_hinput_f32       t = g_dg + z_dg / (softplus(*rho) + eps) -- HLayer's input, :150-152.
 *   admmnet_train_hinput_bwd_f32   from g_t: g_gdg, g_zdg [B][D], g_rho[0].
 *   admmnet_train_hproject_f32     tc = t + 0.1 m, c = A max|tc| + sum tc with A = 2 sqrt(D) sigma_b + sigma_b^2,
 *                                  s = min(sigmoid(*projection_weight) / (c + eps), 1), h = tc s -- :160-194; m is
 *                                  correction_net(t), evaluated by the caller.
 *   admmnet_train_hproject_bwd_f32 from g_h: g_t, g_m [B][D], g_pw[0].
 *   admmnet_train_eigmap_f32       wp = softplus(w - sigmoid(*threshold)) sigmoid(W2 relu(W1 |w| + b1) + b2) over [B][n], the
 *                                  1 -> 16 -> 1 value_net (W1, b1, W2 [16], b2 [1]) -- GLayer, :310-334.
 *   admmnet_train_eigmap_bwd_f32   from g_wp: g_w [B][n]; g_params[50] = g_threshold, gW1[16], gb1[16], gW2[16], gb2.
 *   admmnet_train_stepsize_f32     u_b = rn_b / (mean rn + eps), step_b = rho (0.5 + 1.5 sigmoid(W2 relu(W1 [knorm, rho, u_b]
 *                                  + b1) + b2)), rho = softplus(*rho), the 3 -> 32 -> 1 residual_scale_net (W1 [32][3], b1,
 *                                  W2 [32], b2 [1]) -- ZLayer, :440-474.  The mean (float64) is over the call (sub_batch = 0)
 *                                  or over each group of sub_batch consecutive signals, the last one possibly shorter.
 *   admmnet_train_stepsize_bwd_f32 from g_step: g_rn [B] including the coupling through the mean; g_params[162] = g_rho
 *                                  (through the leading factor only: the rho feature is a constant, the reference's .item()),
 *                                  gW1[32][3], gb1[32], gW2[32], gb2. */
enum {
    ADMMNET_TRAIN_PHI = 0,
    ADMMNET_TRAIN_HINPUT = 1,
    ADMMNET_TRAIN_HPROJECT = 2,
    ADMMNET_TRAIN_EIGMAP = 3,
    ADMMNET_TRAIN_STEPSIZE = 4,
    ADMMNET_TRAIN_EIGMAP_GRADS = 50,
    ADMMNET_TRAIN_STEPSIZE_GRADS = 162
};
int64_t admmnet_train_small_partials(int32_t step, int64_t B, int64_t sub_batch);
int admmnet_train_phi_c64(int32_t D, int64_t B, const void *y, const void *b, const void *g_col, const void *z_col,
                          const float *rho, void *phi, void *stream);
int admmnet_train_phi_bwd_c64(int32_t D, int64_t B, const void *g_phi, const void *y, const void *b, const void *g_col,
                              const void *z_col, const float *rho, void *g_gcol, void *g_zcol, float *g_rho, float *partials,
                              void *stream);
int admmnet_train_hinput_f32(int32_t D, int64_t B, const float *g_dg, const float *z_dg, const float *rho, float *t,
                             void *stream);
int admmnet_train_hinput_bwd_f32(int32_t D, int64_t B, const float *g_t, const float *z_dg, const float *rho, float *g_gdg,
                                 float *g_zdg, float *g_rho, float *partials, void *stream);
int admmnet_train_hproject_f32(int32_t D, int64_t B, const float *t, const float *m, const float *sigma,
                               const float *projection_weight, float *h, void *stream);
int admmnet_train_hproject_bwd_f32(int32_t D, int64_t B, const float *g_h, const float *t, const float *m, const float *sigma,
                                   const float *projection_weight, float *g_t, float *g_m, float *g_pw, float *partials,
                                   void *stream);
int admmnet_train_eigmap_f32(int32_t n, int64_t B, const float *w, const float *threshold, const float *W1, const float *b1,
                             const float *W2, const float *b2, float *wp, void *stream);
int admmnet_train_eigmap_bwd_f32(int32_t n, int64_t B, const float *g_wp, const float *w, const float *threshold, const float *W1,
                                 const float *b1, const float *W2, const float *b2, float *g_w, float *g_params, float *partials,
                                 void *stream);
int admmnet_train_stepsize_f32(int64_t B, int64_t sub_batch, float knorm, const float *rn, const float *rho, const float *W1,
                               const float *b1, const float *W2, const float *b2, float *step, void *stream);
int admmnet_train_stepsize_bwd_f32(int64_t B, int64_t sub_batch, float knorm, const float *g_step, const float *rn,
                                   const float *rho, const float *W1, const float *b1, const float *W2, const float *b2,
                                   float *g_rn, float *g_params, float *partials, void *stream);

/* The step size from a mean that comes from OUTSIDE the call (csrc/train_small.hip): the batch-sharded training of
 * admm_net_amd/sharded.py, where the mean of admm_net.py:459 is over the signals of all ranks.  `pair` is a DEVICE double[2] =
 * (sum of rn, number of signals) of the whole batch, 8-byte aligned; every kernel forms mean = (float)(pair[0] / pair[1]) itself
 * and den = mean + eps.  No reduction over the batch is left in the forward, so the grids are over slabs of 256 signals, one
 * thread each.  B >= 1; parameters RAW and conventions as above.  Sums run in a fixed order without atomics, float64 across
 * workgroups: two runs give the same bits.
 *   admmnet_train_rnsum_f64                  pair[0] = sum of rn[0 .. B) in float64 (thread t of one workgroup adds rn[t],
 *                                            rn[t + 256], ..., a tree halves the 256 slots), pair[1] = (double) B: this call's
 *                                            share, to be summed over the ranks.
 *   admmnet_train_stepsize_pair_f32          step_b as admmnet_train_stepsize_f32 computes it, from the mean of `pair`.
 *   admmnet_train_stepsize_bwd_pair_front_f32  from g_step: g_u [B] (the gradient of u_b = rn_b / den), g_params[162] as
 *                                            admmnet_train_stepsize_bwd_f32 lays them out (sums over THIS call's signals) and
 *                                            total[0] = sum_b g_u_b rn_b, products and sums in float64: this call's share of the
 *                                            coupling through the mean.  (dy_b of the kernel comment stays in LDS.)  `partials` holds
 *                                            admmnet_train_stepsize_pair_partials(B) floats (-1 for B < 1), 8-byte aligned.
 *   admmnet_train_stepsize_bwd_pair_back_f32 from g_u, the pair and total[0] summed over the ranks:
 *                                            g_rn_b = ((g_u_b mean - total / count) + g_u_b eps) / den^2, the cancellation-safe form
 *                                            of admmnet_train_stepsize_bwd_f32: with a pair of ONE signal the difference is an exact
 *                                            zero and g_u eps / den^2 remains.  g_rn may be g_u (in place). */
int64_t admmnet_train_stepsize_pair_partials(int64_t B);
int admmnet_train_rnsum_f64(int64_t B, const float *rn, double *pair, void *stream);
int admmnet_train_stepsize_pair_f32(int64_t B, float knorm, const float *rn, const double *pair, const float *rho, const float *W1,
                                    const float *b1, const float *W2, const float *b2, float *step, void *stream);
int admmnet_train_stepsize_bwd_pair_front_f32(int64_t B, float knorm, const float *g_step, const float *rn, const double *pair,
                                              const float *rho, const float *W1, const float *b1, const float *W2, const float *b2,
                                              float *g_u, float *g_params, double *total, float *partials, void *stream);
int admmnet_train_stepsize_bwd_pair_back_f32(int64_t B, const float *g_u, const double *pair, const double *total, float *g_rn,
                                             void *stream);

/* Training route "native", the H layer with its correction_net inside (csrc/train_hlayer.hip): one forward kernel; one backward
 * kernel plus a batch-reduced product on the matrix cores for the weight gradients.  1 <= D = M N <= 256, B >= 1 (at most
 * 65535 * 128).  Conventions, alignment and the RAW parameters as for the "full" route above; W1 [64][D], b1 [64], W2 [D][64],
 * b2 [D] are correction_net's Linear(D, 64) - ReLU - Linear(64, D) - Tanh.
 *   admmnet_train_hlayer_f32      t = g_dg + z_dg / (softplus(*rho) + eps), a1 = relu(W1 t + b1), m = tanh(W2 a1 + b2),
 *                                 tc = t + 0.1 m, h = the projection of admmnet_train_hproject_f32 -- HLayer, :134-194.
 *                                 t, m [B][D] and a1 [B][64] are written for the backward.
 *   admmnet_train_hlayer_bwd_f32  from g_h: g_gdg, g_zdg [B][D]; the pre-activation deltas delta1 [B][64] (relu'(0) = 0) and
 *                                 delta2 [B][D]; g_params[2 + 129 D + 64] = g_rho, g_projection_weight, gW1 [64][D], gb1 [64],
 *                                 gW2 [D][64], gb2 [D].  The weight gradients are sums over the batch: float32 on the matrix
 *                                 cores within fixed slabs of 128 signals, the slabs added in ascending order in float64; no
 *                                 atomics, two runs give the same bits.  `workspace` holds admmnet_train_hlayer_workspace(D, B)
 *                                 bytes (-1 for sizes outside the range), 4-byte aligned. */
int64_t admmnet_train_hlayer_workspace(int32_t D, int64_t B);
int admmnet_train_hlayer_f32(int32_t D, int64_t B, const float *g_dg, const float *z_dg, const float *sigma, const float *rho,
                             const float *projection_weight, const float *W1, const float *b1, const float *W2, const float *b2,
                             float *h, float *t, float *a1, float *m, void *stream);
int admmnet_train_hlayer_bwd_f32(int32_t D, int64_t B, const float *g_h, const float *z_dg, const float *sigma, const float *rho,
                                 const float *projection_weight, const float *W1, const float *W2, const float *t, const float *a1,
                                 const float *m, float *g_gdg, float *g_zdg, float *delta1, float *delta2, float *g_params,
                                 void *workspace, void *stream);

/* Training route "native", the PeakSearchLayer head (csrc/train_head.hip; PeakSearchLayer.forward, :570-630).  1 <= D = M N <= 256,
 * 1 <= L <= 16, B >= 1 with B L <= 65535 * 128.  `params` is a HOST array of the 21 + 8 L device pointers to the RAW float32
 * parameters: position_encoder, feature_extractor.{0,2}.{weight,bias}, position_projection.{weight,bias}, attention.in_proj_
 * {weight,bias}, attention.out_proj.{weight,bias}, peak_extractor.{0,2,4}.{weight,bias}, confidence_net.{0,2}.{weight,bias}, then
 * per target t tau_regressor.t.{0,2}.{weight,bias}, f_regressor.t.{0,2}.{weight,bias}; the array is read before the call returns.
 * `keep` is the attention dropout's keep mask [B][4][D], one byte per element (nonzero: kept), applied as a <- a keep / (1 - p)
 * between the softmax and the value product, 0 <= p < 1; NULL: no dropout (p is ignored).  phi, g_phi are complex64 [B][D].
 *   admmnet_train_head_f32      tau, f, conf [B][L]; `saved` receives the activations the backward reads,
 *                               admmnet_train_head_workspace(D, L, B, ADMMNET_TRAIN_HEAD_SAVED) bytes
 *                               (4 B (4 D + 752 + 80 L) + 12 * 128 D).
 *   admmnet_train_head_bwd_f32  from g_tau, g_f, g_conf [B][L] and the forward's tau, f, conf, saved: g_phi, and g_params
 *                               (..._GRADS bytes), the raw-parameter gradients, at float offsets:
 *                               confidence_net 0.weight 0, 0.bias 256, 2.weight 272, 2.bias 288; then from 289
 *                               feature_extractor 0.weight, 0.bias, 2.weight, 2.bias, out_proj weight, bias, peak_extractor
 *                               0.weight ... 4.bias, per target [tau 0.weight | f 0.weight] [tau 0.bias | f 0.bias] tau
 *                               2.weight, 2.bias, f 2.weight, 2.bias (1154 floats), 256 D floats of scratch, in_proj_weight
 *                               [384][128] at 289 + 512 D + 44016 + 1154 L, in_proj_bias [384] behind it, position_projection weight [128][2],
 *                               bias [128], position_encoder [D][2].  Every batch sum runs in float32 on the matrix cores within
 *                               fixed slabs of 128 signals, the slabs added in ascending order in float64; no atomics, two runs
 *                               give the same bits.  `workspace` holds ..._WORK bytes.
 * admmnet_train_head_workspace answers -1 for sizes outside the range or an unknown part. */
#define ADMMNET_TRAIN_HEAD_SAVED 0
#define ADMMNET_TRAIN_HEAD_WORK 1
#define ADMMNET_TRAIN_HEAD_GRADS 2
int64_t admmnet_train_head_workspace(int32_t D, int32_t L, int64_t B, int32_t part);
int admmnet_train_head_f32(int32_t D, int32_t L, int64_t B, const void *phi, const void *const *params, const uint8_t *keep, float p,
                           float *tau, float *f, float *conf, void *saved, void *stream);
int admmnet_train_head_bwd_f32(int32_t D, int32_t L, int64_t B, const float *g_tau, const float *g_f, const float *g_conf,
                               const void *phi, const void *const *params, const uint8_t *keep, float p, const float *tau,
                               const float *f, const float *conf, void *saved, void *g_phi, float *g_params, void *workspace,
                               void *stream);

/* The training losses of the reference's loss.py (csrc/loss.hip): one kernel per forward (plus a float64 sum over the batch
 * that also forms the outputs) and one elementwise kernel per backward.  B >= 1, D >= 1 (any signal length), 1 <= Lmax <= 64.
 * All tensors are dense and need only their natural alignment (4 bytes float, 8 bytes complex64 and int64).  Sums over the
 * batch run in a fixed order without atomics (float64 across workgroups): two runs give the same bits.  `partials` is float
 * scratch of admmnet_loss_partials(loss, B) entries.  `g_out` is a DEVICE float[3]: the gradients of out[0], out[1], out[2].
 * Complex gradients follow torch's convention (dL/dRe + i dL/dIm); the targets (tau_true, f_true, L_true, phi_true) get none.
 *   admmnet_loss_anm_f32      BasicANMLoss, loss.py:6-60.  tau, f, conf, tau_true, f_true float [B][Lmax], L_true int64 [B],
 *                             phi complex64 [B][D].  With L = L_true[b]:
 *                               L = 0:   loss_b = sum_j conf_j^2 over all Lmax slots;
 *                               L >= 1:  loss_b = mean_{j<L} (tau_j - tau_true_j)^2 + mean_{j<L} (f_j - f_true_j)^2
 *                                                 + 0.1 mean_{j<L} (conf_j - 1)^2.
 *                             out[3] = {param + reg, param, reg}, param = sum_b loss_b / B, reg = lambda_reg mean_b ||phi_b||_2;
 *                             norms [B] = ||phi_b||_2, kept for the backward; status[0] = the number of signals whose L_true
 *                             lies outside [0, Lmax] (the reference raises for those; the kernel evaluates them with L held
 *                             to that range and reads nothing out of bounds).
 *   admmnet_loss_anm_bwd_f32  with cp = g_out[0] + g_out[1], cr = g_out[0] + g_out[2]: g_tau, g_f, g_conf [B][Lmax] =
 *                             cp d loss_b / d(.) / B (zeros at j >= L when L >= 1; g_tau = g_f = 0 when L = 0),
 *                             g_phi[b] = cr lambda_reg / B phi_b / ||phi_b||, exactly 0 where the norm is 0.
 *   admmnet_loss_phi_c64      PhiAlignmentLoss, loss.py:62-98.  phi, phi_true complex64 [B][D].
 *                             amplitude = mean (|phi| - |phi_true|)^2, phase = mean wrap(arg phi - arg phi_true)^2 over the
 *                             B D entries, wrap(d) = ((d + pi) mod 2 pi) - pi with the floored mod (+pi maps to -pi);
 *                             out[3] = {amplitude_weight amplitude + phase_weight phase, amplitude, phase}.
 *   admmnet_loss_phi_bwd_c64  with ca = g_out[0] amplitude_weight + g_out[1], cp = g_out[0] phase_weight + g_out[2], phi = x + iy:
 *                             g_phi = ca 2 (|phi| - |phi_true|) / (B D) phi / |phi| + cp 2 wrap(.) / (B D) (-y + ix) / |phi|^2,
 *                             exactly 0 where phi = 0; the wrap has derivative 1. */
enum {
    ADMMNET_LOSS_ANM = 0,
    ADMMNET_LOSS_PHI = 1
};
int64_t admmnet_loss_partials(int32_t loss, int64_t B);
int admmnet_loss_anm_f32(int32_t Lmax, int32_t D, int64_t B, const float *tau, const float *f, const float *conf,
                         const float *tau_true, const float *f_true, const int64_t *L_true, const void *phi, float lambda_reg,
                         float *out, float *norms, int32_t *status, float *partials, void *stream);
int admmnet_loss_anm_bwd_f32(int32_t Lmax, int32_t D, int64_t B, const float *g_out, const float *tau, const float *f,
                             const float *conf, const float *tau_true, const float *f_true, const int64_t *L_true,
                             const void *phi, const float *norms, float lambda_reg, float *g_tau, float *g_f, float *g_conf,
                             void *g_phi, void *stream);
int admmnet_loss_phi_c64(int32_t D, int64_t B, const void *phi, const void *phi_true, float amplitude_weight,
                         float phase_weight, float *out, float *partials, void *stream);
int admmnet_loss_phi_bwd_c64(int32_t D, int64_t B, const float *g_out, const void *phi, const void *phi_true,
                             float amplitude_weight, float phase_weight, void *g_phi, void *stream);

/* The terms of the phi loss that are defined on the delay-Doppler spectrum (csrc/loss_spectrum.hip): one workgroup per signal,
 * float64 arithmetic, fixed-order sums without atomics (a signal's figures depend on neither B nor its place), no host read.
 * phi complex64 [B][ybase * xbase] laid out [ybase][xbase] (x = delay).  With the atom a(tau, f)[ks xbase + kd] =
 * exp(j 2 pi (ks f - kd tau)), z_b(tau, f) = sum_i conj(phi_b[i]) a(tau, f)[i], S = |z|^2 (admmnet_spectrum_f64's image), on the
 * uniform full-period grid taus_p = p / nx, fs_q = -0.5 + q / ny, nx = oversample xbase, ny = oversample ybase (an axis of
 * base 1 has one point), 1 <= oversample <= 4, G = nx ny points, m = mean_grid S, and S*, z*, m* the same of phi_true:
 *   spectral_b     = mean_grid (S / m - S* / m*)^2
 *   distribution_b = 1 - sum_grid |z| |z*| / sqrt(sum_grid S sum_grid S*)            (squared Hellinger distance)
 *   target_b       = mean_{l < L} (1 - rho_l), rho_l = |z_b(tau_true_l, f_true_l)|^2 / (D ||phi_b||^2), L = L_true[b] held to
 *                    [0, Lmax]; 0 for L = 0.  0 <= Lmax <= 16; tau_true, f_true float [B][Lmax], L_true int64 [B].
 * Each term is its mean over the batch; out[4] = {spectral_weight spectral + distribution_weight distribution + target_weight
 * target, spectral, distribution, target}.  phi_true == NULL: no grid terms (both are 0); L_true == NULL: no target term.
 * A signal whose phi row is all zero, or whose phi_true row is all zero when the grid terms run, gives 0 to every term and gets
 * a zero gradient row.  status[3] = {signals with L_true outside [0, Lmax], zero phi rows, zero phi_true rows}.
 * `workspace` (admmnet_loss_spectrum_workspace_bytes, -1 for sizes the kernels do not take: the working set must fit 150 KiB
 * of LDS) receives the steering tables, z, S* and the per-signal scalars; the backward reads it and leaves it unchanged.
 *   admmnet_loss_spectrum_bwd_f64  g_out: DEVICE float[4], the gradients of out[0 .. 3].  g_phi complex64 [B][D], torch's
 *                    convention: 2 sum_grid c conj(z) a[i] with c = d total / d S, plus the target rows 2 c_l conj(z_l) a_l[i]
 *                    and the derivative of ||phi||^2; d|z| / dz is taken as 0 at z = 0.  `skip`: bit 0 the spectral, bit 1 the
 *                    distribution, bit 2 the target term is left out of the gradient (its weight and its upstream gradient are
 *                    known to be zero on the host).  A term the forward did not evaluate (phi_true or L_true NULL there) is a
 *                    constant and adds nothing, whatever `skip` says: the forward records what it ran in the workspace. */
enum {
    ADMMNET_LOSS_SPECTRUM_SKIP_SPECTRAL = 1,
    ADMMNET_LOSS_SPECTRUM_SKIP_DISTRIBUTION = 2,
    ADMMNET_LOSS_SPECTRUM_SKIP_TARGET = 4
};
int64_t admmnet_loss_spectrum_workspace_bytes(int32_t xbase, int32_t ybase, int32_t oversample, int64_t B);
int admmnet_loss_spectrum_f64(int32_t xbase, int32_t ybase, int32_t oversample, int32_t Lmax, int64_t B, const void *phi,
                              const void *phi_true, const float *tau_true, const float *f_true, const int64_t *L_true,
                              float spectral_weight, float distribution_weight, float target_weight, float *out,
                              int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
int admmnet_loss_spectrum_bwd_f64(int32_t xbase, int32_t ybase, int32_t oversample, int32_t Lmax, int64_t B, const float *g_out,
                                  const void *phi, const float *tau_true, const float *f_true, const int64_t *L_true,
                                  float spectral_weight, float distribution_weight, float target_weight, int32_t skip,
                                  const void *workspace, int64_t workspace_bytes, void *g_phi, void *stream);

/* The assignment loss of the head (csrc/loss_set.hip, scalar core csrc/set_core.h): a permutation-invariant training loss for
 * slots (tau, f, conf) against targets that come in no particular order.  One wave per signal, all in float64 from the float
 * inputs, one row of per-signal values each, added over the batch in a fixed order by one workgroup: no atomics, two runs give
 * the same bits, and a signal's bits depend on neither B, nor its place, nor its neighbours.
 *   Inputs   tau, f, conf float [B][Lmax] (they get gradients); tau_true, f_true float [B][Lt]; L_true int64 [B]; phi complex64
 *            [B][D].  1 <= Lmax, Lt <= 64, B >= 1, D >= 1.
 *   opts     HOST double[6] = {sx, sy, period_tau, period_f, w_conf, lambda_reg}: scales > 0; a period 0 means the plain
 *            difference, P > 0 wraps it into [-P/2, P/2) (derivative 1); w_conf >= 0; lambda_reg >= 0; all finite.
 *   Per signal, n = L_true held to [0, Lt], all Lmax slots live:
 *       d2_ij = (sx wrap(tau_i - tau_true_j))^2 + (sy wrap(f_i - f_true_j))^2, every product rounded on its own;
 *       an assignment sigma matches k = min(Lmax, n) distinct slots to distinct targets j < n, t_i = 1 on a matched slot, else 0;
 *       match_b(sigma) = (1 / max(n, 1)) sum over matched (i, j) of d2_ij
 *       conf_b(sigma)  = (1 / Lmax) sum_i (conf_i - t_i)^2
 *       loss_b         = min over sigma of [match_b(sigma) + w_conf conf_b(sigma)]
 *     -- the minimum of ONE expression, so its gradient is the gradient at the minimiser.  Equivalently loss_b = (w_conf / Lmax)
 *     sum_i conf_i^2 + min_sigma sum_matched c_ij with c_ij = d2_ij / n + (w_conf / Lmax)(1 - 2 conf_i): a linear assignment with a
 *     per-slot term, solved by the shortest-augmenting-path search of admmnet_score_match_f64.  n = 0: nothing is matched,
 *     loss_b = (w_conf / Lmax) sum_i conf_i^2.  n > Lmax: the targets left unmatched cost nothing.  There is no truncation.
 *   Outputs  out[4] = {total, match, conf, reg}: match = mean_b match_b, conf = mean_b conf_b, reg = lambda_reg mean_b ||phi_b||_2,
 *            total = match + w_conf conf + reg.  assign int32 [B][Lmax]: the target of slot i, else -1.  norms float [B] =
 *            ||phi_b||_2.  status[2] = {signals with L_true outside [0, Lt], signals with a non-finite value among tau, f, conf or
 *            their first n truths}.  A signal of the second kind adds 0 to every sum, gets assign = -1 and zero gradients; one of
 *            the first kind is evaluated with n held to the range.  `partials`: double scratch of admmnet_loss_set_partials(B)
 *            entries; after the call it holds the rows [B][6] = loss_b, match_b, conf_b, ||phi_b||, and the two status flags.
 *   admmnet_loss_set_bwd_f32   g_out: DEVICE float[4], the gradients of out[0 .. 3]; assign and norms as the forward left them.
 *            With cm = g_out[0] + g_out[1], cc = g_out[0] w_conf + g_out[2], cr = g_out[0] + g_out[3]:
 *              g_tau_i = cm 2 sx^2 wrap(tau_i - tau_true_j) / (n B) on a matched slot, exactly 0 elsewhere; g_f_i the same with sy, f;
 *              g_conf_i = cc 2 (conf_i - t_i) / (Lmax B);  g_phi = admmnet_loss_anm_bwd_f32's with cr;  the targets get none.
 * Both are stream-ordered, allocate nothing and read nothing back.  Sizes out of range, a null pointer or bad options are refused
 * with ADMMNET_E_ARG before any launch, the outputs untouched. */
int64_t admmnet_loss_set_partials(int64_t B);
int admmnet_loss_set_f32(int32_t Lmax, int32_t Lt, int32_t D, int64_t B, const float *tau, const float *f, const float *conf,
                         const float *tau_true, const float *f_true, const int64_t *L_true, const void *phi, const double *opts,
                         float *out, int32_t *assign, float *norms, int32_t *status, double *partials, void *stream);
int admmnet_loss_set_bwd_f32(int32_t Lmax, int32_t Lt, int32_t D, int64_t B, const float *g_out, const float *tau, const float *f,
                             const float *conf, const float *tau_true, const float *f_true, const int64_t *L_true,
                             const void *phi, const int32_t *assign, const float *norms, const double *opts, float *g_tau,
                             float *g_f, float *g_conf, void *g_phi, void *stream);

/* Target estimates scored against ground truth (csrc/score.hip, scalar core csrc/score_core.h): one wave per signal, sums over
 * the batch in a fixed order without atomics (float64 across workgroups), so two runs give the same bits.  B >= 1; `partials` is
 * double scratch of admmnet_score_partials(B) entries.  All tensors are dense with their natural alignment.
 *   admmnet_score_match_f64   one optimal assignment per signal.  1 <= Le, Lt <= 64.
 *       est       double [B][Le][3], the rows of admmnet_peak_top_f64: (tau, f, height).  The height is ignored; a row whose tau
 *                 or f is not finite is absent.
 *       n_est     int32 [B] or NULL (= Le): only the first n_est rows count, held to 0 .. Le.
 *       tau_true, f_true   float [B][Lt];  L_true int64 [B] or NULL (= Lt): the first L_true slots are the targets.
 *       opts      HOST double[5] = {sx, sy, cutoff, period_tau, period_f}: scales > 0, cutoff c > 0, a period 0 means the plain
 *                 difference, P > 0 wraps it into [-P/2, P/2).
 *     Definition, all in float64: with the present estimates i (n_est of them) and the targets j (n_true),
 *       d2_ij = (sx dtau_ij)^2 + (sy df_ij)^2, the assignment matches k = min(n_est, n_true) pairs and minimises
 *       sum min(d2, c^2); a matched pair with d2 < c^2 is a HIT, no other pair is reported.  This is the GOSPA assignment
 *       (alpha = 2, p = 2): the truncation is inside the cost that is minimised -- solving without it and gating afterwards
 *       gives another, wrong answer.  The solver is a shortest-augmenting-path search with potentials (rows = the smaller side,
 *       costs recomputed from the coordinates, lowest lane first on ties).
 *       match     int32 [B][Lt]: the index in `est` of the estimate that hit target j, else -1.
 *       stats     double [B][8] = n_hit, n_miss = n_true - n_hit, n_false = n_est - n_hit, sum_hits dtau^2, sum_hits df^2,
 *                 sum_hits d2, gospa^2 = sum_hits d2 + c^2 / 2 (n_miss + n_false), the optimal truncated cost.
 *       totals    double [8]: the column sums of stats over the signals that were scored.
 *       status    int32 [2]: [0] signals whose L_true lies outside [0, Lt], [1] signals with a non-finite tau_true or f_true
 *                 among their first L_true.  Either kind gets NaN stats and a match row of -1 and is left out of totals;
 *                 nothing is read out of bounds.
 *   admmnet_score_ordered_f32   the validation RMSE of train.py:262-274, slot j against slot j.  tau_est, f_est, tau_true,
 *       f_true float [B][Lmax], 1 <= Lmax <= 64, L_true int64 [B].  For L = L_true[b] > 0:
 *       per_sample [B][2] = sqrt(mean_{j<L} (tau_est - tau_true)^2), the same for f, in float64 from the float inputs; NaN
 *       where L = 0.  out [3] = the mean of each column over the signals with L > 0 (0 when there are none), and their count.
 *       status [1] = signals whose L_true lies outside [0, Lmax]; they are evaluated with L held to that range. */
int64_t admmnet_score_partials(int64_t B);
int admmnet_score_match_f64(int32_t Le, int32_t Lt, int64_t B, const double *est, const int32_t *n_est, const float *tau_true,
                            const float *f_true, const int64_t *L_true, const double *opts, int32_t *match, double *stats,
                            double *totals, int32_t *status, double *partials, void *stream);
int admmnet_score_ordered_f32(int32_t Lmax, int64_t B, const float *tau_est, const float *f_est, const float *tau_true,
                              const float *f_true, const int64_t *L_true, double *per_sample, double *out, int32_t *status,
                              double *partials, void *stream);

/* The Cramer-Rao bound of a scene's targets (csrc/crb.hip, scalar core csrc/crb_core.h): one wave per scene, sums over the batch
 * as admmnet_score_match_f64 forms them (fixed order, no atomics: two runs give the same bits).  All in float64.
 *   Scene model (admmnet_synth_batch), Nb entries along f and Nd along tau, D = Nb Nd:
 *       mu[i_b Nd + i_d] = s[i] sum_l C_l exp(j 2 pi (i_b f_l - i_d tau_l)),  |s[i]| = 1,    y = mu + w,  w ~ CN(0, v) per entry.
 *   theta = (tau_1..L, f_1..L, Re C_1..L, Im C_1..L), F = (2 / v) Re(J^H J) with J = d mu / d theta; the bound of target l is
 *   [F^-1] at the diagonal entries of tau_l and f_l.  It is the bound of a receiver that KNOWS the symbols s (|s| = 1 drops out of
 *   J^H J), hence a lower bound for one that only has the demodulated b.  Every entry of J^H J for a pair (l, m) is a constant
 *   times S_p(f_m - f_l; Nb) S_q(-(tau_m - tau_l); Nd), S_p(x; N) = sum_{k<N} k^p exp(j 2 pi k x): O(L^2 (Nb + Nd)) per scene.
 *   F is scaled to unit diagonal, factored by Cholesky and unscaled.
 *       1 <= Lt <= 16, B >= 1, Nb, Nd >= 1 with Nb Nd within admmnet_synth_batch's ceiling.
 *       tau_true, f_true   float [B][Lt];  C: complex64 [B][Lt];  L_true int64 [B] or NULL (= Lt): the first L_true slots count.
 *       match     int32 [B][Lt] or NULL: admmnet_score_match_f64's match; target j is a hit where match >= 0.
 *       noise     double [B]: v itself (noise_is_snr = 0), or the SNR in dB of the generator's definition (noise_is_snr = 1),
 *                 v = sum |mu|^2 / (10^(snr / 10) D), the energy evaluated from the same power sums.
 *       bound     double [B][Lt][2]: the variance bound of tau_j and of f_j.  An axis of length 1 carries no information about its
 *                 parameter: it leaves theta and its bound is +inf.  Slots j >= L_true are NaN.
 *       totals    double [8]: sum of the tau bounds, sum of the f bounds and their two counts over the targets j < L_true, then
 *                 the same four over the hits (zeros without `match`); +inf bounds are left out of sums and counts.
 *       status    int32 [3] counts scenes: [0] L_true outside [0, Lt]; [1] a non-finite tau, f, C or noise entry, or a noise
 *                 variance that is not positive and finite; [2] an information matrix that is not positive definite: a diagonal
 *                 entry that is not positive, or a pivot of the unit-diagonal Cholesky below 2^-40 (coincident targets, C_l = 0).
 *                 Such a scene has NaN bounds and enters no total.
 *   `partials` is double scratch of admmnet_crb_partials(B) entries (-1: bad B). */
int64_t admmnet_crb_partials(int64_t B);
int admmnet_crb_f64(int32_t Nb, int32_t Nd, int32_t Lt, int64_t B, const float *tau_true, const float *f_true, const void *C,
                    const int64_t *L_true, const int32_t *match, const double *noise, int32_t noise_is_snr, double *bound,
                    double *totals, int32_t *status, double *partials, void *stream);

/* Target estimates refined against the received signal (csrc/refine.hip, scalar core csrc/refine_core.h): a local maximum-
 * likelihood fit of a scene's targets to y, started at the rows of a peak search.  One workgroup runs every iteration of a scene;
 * y and b are read once.  All arithmetic is float64; every sum has a fixed order and there are no atomics, so the bits of a scene
 * depend on neither B, nor its place in the batch, nor its neighbours.
 *   Model.   Grid (Nb, Nd), D = Nb Nd, i = i_b Nd + i_d.  As in admmnet_crb_f64,
 *                mu_i(theta) = sum_l C_l exp(j 2 pi (i_b f_l - i_d tau_l)),   theta = (Re C, Im C, tau, f) of the present estimates.
 *   Data.    x_i = y_i conj(s_i) with |s_i| = 1.          Cost.   Q(theta, s) = sum_i |x_i - mu_i(theta)|^2.
 *   Symbols. mode 0 ("given"): s_i = b_i / |b_i| throughout; an entry b_i = 0 or a non-finite b_i makes the scene non-finite.
 *            mode 1 ("psk"): before every linearisation s_i is the point of {p_k = exp(j (2 pi k / psk_m + psk_phase)), k < psk_m}
 *            nearest in angle to y_i conj(mu_i(theta)) -- the k of greatest Re(y_i conj(mu_i) conj(p_k)), ties to the smaller k.
 *            b only gives the starting symbols, the point nearest to b_i (b_i = 0 gives k = 0; a non-finite b_i makes the scene
 *            non-finite).  flips = the number of entries whose final s_i differs from the point nearest to b_i.  Both steps
 *            minimise Q over their own variables, so Q never increases.
 *   Start.   rows_in as admmnet_score_match_f64 reads them: (tau, f, .), a row with a non-finite tau or f is absent, only the
 *            first n_est rows count.  The starting C is the least-squares solution at the starting (tau, f): the Cholesky of the
 *            unit-diagonal C-block with admmnet_crb_f64's pivot floor 2^-40.
 *   One iteration.  G = Re(J^H J) and g = Re(J^H r), r = x - mu, at the current theta; A = D G D with D = diag(G)^-1/2; solve
 *            (A + lambda I) d' = D g, d = D d'; d is scaled so that no target moves more than half a cell (0.5 / Nd in tau,
 *            0.5 / Nb in f).  Accepted if Q(theta + d) <= Q(theta) with s held fixed, then lambda <- lambda / 10; otherwise
 *            lambda <- 10 lambda and the solve is repeated.  lambda starts at 1e-4.
 *   Stop.    state 0, converged: an accepted step moves every target by at most `tol` cells, or a rejected trial step is that
 *                     small (a scene without a present row is converged after 0 iterations, Q = sum |y|^2);
 *            state 1, limit: `iters` linearisations (1 .. 64) are used up;
 *            state 2, gave up: lambda > 1e8, a diagonal entry of G that is not positive and finite, or a starting C-block that
 *                     is not positive definite.  The last accepted theta is returned; on a failed start rows_out holds the input
 *                     (tau, f) with |C| = NaN and C_out is NaN;
 *            state 3, non-finite: an entry of y (or of b, above) is not finite.  rows_out, C_out, Q and Q / D of the scene are NaN,
 *                     its two counts 0;
 *            state 4, outside: n_est is not in 0 .. Le.  As state 3.
 *   An axis of length 1 carries no information about its parameter, which leaves theta and passes through unchanged.  Outputs
 *   are not wrapped into a period.
 *       1 <= Le <= 16, B >= 1, Nb, Nd >= 1 with Nb Nd within admmnet_synth_batch's ceiling (3406) and the scene's tables within
 *       the LDS of one workgroup (admmnet_refine_lds_bytes(Nb, Nd, Le) <= 160 KiB: 26 x 131 with Le = 16 fits, 2 x 1703 fits with Le <= 3);
 *       mode 0 or 1, 2 <= psk_m <= 64, a finite psk_phase, 1 <= iters <= 64, tol > 0 and finite.  Anything else: ADMMNET_E_ARG.
 *       y, b          complex64 [B][D];  rows_in double [B][Le][3];  n_est int32 [B] or NULL (= Le).
 *       rows_out      double [B][Le][3] = (tau, f, |C|); absent rows are NaN, the order is kept.
 *       C_out         complex128 [B][Le], NaN on absent rows.
 *       info          double [B][5] = Q, Q / D, linearisations used, flips, state (the codes above: exact in float64).
 *       symbols_out   int32 [B][D] or NULL: the k of the final s_i in mode 1, of the point nearest to b_i in mode 0
 *                     (-1 throughout a scene of state 3 or 4).
 *       status        int32 [4] counts scenes: [0] outside, [1] non-finite, [2] gave up, [3] limit reached -- added from `info`
 *                     by one workgroup in a fixed order.
 *   No host read, no allocation, stream-ordered. */
int64_t admmnet_refine_lds_bytes(int32_t Nb, int32_t Nd, int32_t Le);   /* -1: bad sizes */
int admmnet_refine_f64(int32_t Nb, int32_t Nd, int32_t Le, int64_t B, const void *y, const void *b, const double *rows_in,
                       const int32_t *n_est, int32_t mode, int32_t psk_m, double psk_phase, int32_t iters, double tol,
                       double *rows_out, void *C_out, double *info, int32_t *symbols_out, int32_t *status, void *stream);

/* The number of targets of a scene selected among candidate rows (csrc/order.hip, scalar core csrc/order_core.h): the rows ranked
 * by greedy orthogonal least squares against the received signal, the order chosen by a penalised log residual.  One workgroup per
 * scene, one launch; y and b are read once.  All arithmetic is float64; every sum has a fixed order and there are no atomics, so
 * the bits of a scene depend on neither B, nor its place in the batch, nor its neighbours.
 *   Data.    Grid (Nb, Nd), D = Nb Nd, i = i_b Nd + i_d, x_i = y_i conj(s_i) as in admmnet_refine_f64: s_i = b_i / |b_i| where
 *            `symbols` is NULL, else s_i = p_k with k = symbols_i and p_k = exp(j (2 pi k / psk_m + psk_phase)) -- what
 *            admmnet_refine_f64 writes to symbols_out.
 *   Atoms.   a_l(i) = exp(j 2 pi (i_b f_l - i_d tau_l)) for every present row: l < n_cand with a finite tau_l and f_l.
 *   Ranking. The present rows l < n_held are taken first, in their given order.  After them every step takes the remaining row
 *            of greatest gain |a~_j^H r|^2 / |a~_j|^2, a~_j = a_j made orthogonal to the rows already taken, r the present
 *            residual; ties go to the smaller index.  A row with |a~_j|^2 < 2^-40 D is never taken, held or not (it coincides with
 *            rows already taken).  The ranking ends when max_order rows are taken or none can be.  RSS_0 = sum |x_i|^2,
 *            RSS_k = RSS_(k-1) - gain_k.
 *   Order.   n_sel = the smallest k in h .. K that minimises D ln(max(RSS_k, 2^-80 RSS_0) / D) + penalty k, K the number of rows
 *            ranked, h <= n_held the number of held rows among them.
 *   States.  0, ranked;
 *            3, non-finite: an entry of y or b is not finite, or b_i = 0 where `symbols` is NULL;
 *            4, outside: n_cand not in 0 .. Le, n_held not in 0 .. n_cand, or a symbol not in 0 .. psk_m - 1 (admmnet_refine_f64
 *               marks a scene it did not fit with -1).  State 4 is looked for first.  The codes are admmnet_refine_f64's.
 *            A scene of state 3 or 4 is not ranked: perm is 0 .. Le - 1, n_sel = 0, everything else NaN.
 *       1 <= Le <= 16, B >= 1, Nb Nd <= 3406 and admmnet_order_lds_bytes(Nb, Nd, Le) != -1 (the scene's tables within the 160 KiB of
 *       LDS of one workgroup), 2 <= psk_m <= 64, a finite psk_phase, a finite penalty >= 0, 1 <= max_order <= Le, rows_out not
 *       rows_in.  Anything else: ADMMNET_E_ARG before a launch.
 *       y, b          complex64 [B][D];  rows_in double [B][Le][3] = (tau, f, .);  n_cand, n_held int32 [B] or NULL (= Le, = 0);
 *                     symbols int32 [B][D] or NULL.
 *       perm          int32 [B][Le]: the ranked rows in the order they were taken, then the other rows in index order.
 *       n_sel         int32 [B].
 *       rss           double [B][Le + 1]: RSS_0 .. RSS_K, NaN past K.
 *       rows_out      double [B][Le][3]: row perm[j] of rows_in, the third column |C_j| for j < n_sel and NaN beyond -- with
 *                     n_est = n_sel what admmnet_refine_f64 starts from.
 *       C_out         complex128 [B][Le]: the least-squares amplitudes of the selected rows, NaN beyond n_sel.
 *       residual      complex64 [B][D] = x - sum_(j < n_sel) C_j a_perm[j], evaluated entry by entry (not from RSS, whose closed
 *                     form cancels).
 *       info          double [B][4] = cost (the sum of |residual|^2, added in float64 before the rounding), cost / D, K, state.
 *       status        int32 [2] counts scenes: [0] non-finite, [1] outside -- added from `info` by one workgroup in a fixed order.
 *   No host read, no allocation, stream-ordered. */
int64_t admmnet_order_lds_bytes(int32_t Nb, int32_t Nd, int32_t Le);   /* -1: bad sizes, or more than a workgroup has */
int admmnet_order_f64(int32_t Nb, int32_t Nd, int32_t Le, int64_t B, const void *y, const void *b, const double *rows_in,
                      const int32_t *n_cand, const int32_t *n_held, const int32_t *symbols, int32_t psk_m, double psk_phase,
                      double penalty, int32_t max_order, int32_t *perm, int32_t *n_sel, double *rss, double *rows_out, void *C_out,
                      void *residual, double *info, int32_t *status, void *stream);

/* A CFAR detector on the zero-padded 2-D periodogram of a scene (csrc/cfar.hip, scalar core csrc/cfar_core.h): what an OFDM radar
 * runs -- strip the symbols, take the periodogram, threshold it at a constant false-alarm rate -- and a detector that is not
 * handed the number of targets.  One workgroup per scene, one launch; y and b are read once; x, the intermediate image and the map
 * stay in LDS.  All arithmetic is float64; every sum has a fixed order and there are no atomics, so the bits of a scene depend on
 * neither B, nor its place in the batch, nor its neighbours.
 *   Data.    Grid (Nb, Nd), D = Nb Nd, i = i_b Nd + i_d, x_i = y_i conj(s_i) exactly as in admmnet_order_f64: s_i = b_i / |b_i|
 *            where `symbols` is NULL, else s_i = p_k with k = symbols_i and p_k = exp(j (2 pi k / psk_m + psk_phase)).
 *   Map.     Oversampling r, an integer 1 .. 8; n_f = r Nb, n_tau = r Nd; f_j = -1/2 + j / n_f, tau_i = i / n_tau;
 *                P[j][i] = |sum_(i_b, i_d) x[i_b Nd + i_d] exp(-j 2 pi (i_b f_j - i_d tau_i))|^2 / D,
 *            the matched filter of the atoms a(i) = exp(j 2 pi (i_b f - i_d tau)) of the refinement and the selection, normalised
 *            so that white noise of variance w per complex sample gives E[P] = w.  It is evaluated separably, over i_b (in index
 *            order) and then over i_d (in index order).  Every twiddle is exp(-+j 2 pi k / n) with k = (i_b j) mod n_f or
 *            (i_d i) mod n_tau reduced in integer arithmetic (the -1/2 of f_j is the sign (-1)^i_b), from sincospi of k / n --
 *            never from a recurrence.
 *   Window.  In resolution cells, not map cells.  Per axis a with N_a > 1: G_a = guard, W_a = guard + train; on an axis with
 *            N_a = 1: G_a = W_a = 0.  Offsets Omega = {(p, q): |p| <= W_b, |q| <= W_d} \ {(p, q): |p| <= G_b, |q| <= G_d}, N = |Omega|.
 *            The training cells of (j, i) are P[(j + p r) mod n_f][(i + q r) mod n_tau]: cells r apart are samples of an orthogonal
 *            DFT, independent under white noise, which makes the factors below exact.  guard >= 0, train >= 1,
 *            guard + train <= 8 (so N <= 288: the offsets are a table of a fixed size in LDS; the rank selection counts the
 *            cells below a pivot, about 2 N ln N reads per cell, and needs no storage), 2 W_a + 1 <= N_a on every axis with N_a > 1 (no training cell is counted twice round the
 *            torus), N >= 1.  Method 0 has no window: guard, train and rank are not read.
 *   Level.   Z[j][i] and the factor alpha, by `method`:
 *            0, known: Z = noise_var of the scene,                              alpha = -ln(pfa);
 *            1, ca:    Z = the mean of the training cells, added with p ascending and, within p, q ascending, then divided by N,
 *                                                                                 alpha = N (pfa^(-1/N) - 1);
 *            2, os:    Z = the `rank`-th smallest training cell, 1 <= rank <= N,  alpha solves prod_(m < rank) (N-m)/(N-m+alpha) = pfa.
 *            alpha is the caller's (detect.cfar_alpha computes it on the host in float64): the entry takes alpha, not pfa.
 *   Over.    A cell is over iff P > alpha Z.  It is a detection iff it is over and beats each of its 8 torus neighbours (one map
 *            cell away, wrapping on both axes): c beats c' iff P_c > P_c', or P_c == P_c' and c < c', with c = j n_tau + i.  A
 *            neighbour that is the cell itself (an axis of one map cell) is skipped.  Detections are ordered by P descending,
 *            ties to the smaller c; the first Le (1 .. 16) are rows (tau_i, f_j, P), the rows beyond are NaN.
 *   States.  0, done;
 *            3, non-finite: an entry of y or b is not finite, b_i = 0 where `symbols` is NULL, or noise_var is not finite;
 *            4, outside: a symbol not in 0 .. psk_m - 1, or noise_var <= 0 in method 0.  State 4 is looked for first.
 *            A scene of state 3 or 4 has NaN rows, a NaN level (and map) and counts 0.
 *       B >= 1, Nb Nd <= 3406, r^2 Nb Nd <= 65535 and admmnet_cfar_lds_bytes(Nb, Nd, r) != -1 (within the 160 KiB of LDS of one
 *       workgroup: 16 D + 16 r D + 11 r^2 D + 16 r (Nb + Nd) + 3312 bytes and the 16-byte alignment of each array; 8 x 8 with
 *       r = 2 takes 9 712 bytes, 16 x 16 with r = 4 takes 70 896, 13 x 262 with r = 1 -- the largest grid -- 154 176; 25 x 24 fits
 *       with r = 4 and 25 x 25 does not), 2 <= psk_m <= 64, a finite psk_phase, a finite alpha > 0, noise_var non-NULL exactly
 *       in method 0.  Anything else: ADMMNET_E_ARG before a launch.
 *       y, b          complex64 [B][D];  symbols int32 [B][D] or NULL;  noise_var double [B] (method 0) or NULL.
 *       rows          double [B][Le][3] = (tau_i, f_j, P).
 *       counts        int32 [B][2] = n_det (all detections: it may exceed Le), n_over (the cells over the threshold).
 *       info          double [B][2] = level (the mean of Z over the map: a thread adds its cells c = t, t + 256, .. in that order,
 *                     the lanes of a wave are added by a butterfly, the waves in order; in method 0 the given value), state.
 *       map_out       double [B][n_f][n_tau] or NULL.
 *       status        int32 [2] counts scenes: [0] non-finite, [1] outside -- added from `info` by one workgroup in a fixed order.
 *   No host read, no allocation, stream-ordered. */
int64_t admmnet_cfar_lds_bytes(int32_t Nb, int32_t Nd, int32_t r);   /* -1: bad sizes, or more than a workgroup has */
int admmnet_cfar_f64(int32_t Nb, int32_t Nd, int32_t r, int32_t Le, int64_t B, const void *y, const void *b, const int32_t *symbols,
                     int32_t psk_m, double psk_phase, int32_t method, int32_t guard, int32_t train, int32_t rank, double alpha,
                     const double *noise_var, double *rows, int32_t *counts, double *info, double *map_out, int32_t *status,
                     void *stream);

/* Successive cancellation with cyclic re-fitting on that periodogram (csrc/cfar_relax.hip, scalar core csrc/relax_core.h): the
 * detector above run round after round on a residual.  A detected target is fitted off the grid, subtracted from the residual and
 * re-fitted with the others (RELAX), so that it neither sits in another target's training ring nor leaves sidelobes to detect.  One
 * workgroup per scene, one launch, float64, every sum in a fixed order, no atomics: the bits of a scene depend on neither B, nor its
 * place in the batch, nor its neighbours.
 *   Data.    x = y conj(s), the sizes, the window, the level Z, the factor alpha and the states exactly as admmnet_cfar_f64.  The
 *            residual starts as x.
 *   Filter.  S(tau, f) = sum_i x_i exp(-j 2 pi (i_b f - i_d tau)) over the residual, F = |S|^2 / D; the atom is
 *            a(tau, f)_i = exp(+j 2 pi (i_b f - i_d tau)).
 *   Round k = 0, 1, ..:  P_k is the map of admmnet_cfar_f64 of the residual (round 0's map is that entry's map bit for bit), Z and
 *            alpha are taken by `method` on P_k, the cells with P_k > alpha Z are over.  No cell over: stop.  k == Le: more = 1,
 *            stop.  Otherwise the highest over cell (ties to the smaller index c = j n_tau + i; under methods 1 and 2 it need not
 *            be the highest cell of the map) is fitted from (tau_i, f_j), which gives (tau, f) and c = S(tau, f) / D; c a(tau, f)
 *            is subtracted from the residual and the target appended.  With two or more targets `sweeps` sweeps follow: for every
 *            target in detection order, c a is added back, the target fitted from its (tau, f), c recomputed, c a subtracted.
 *   Fit.     At most `iters` Newton steps on F from (tau0, f0).  The gradient and the Hessian follow from the six sums
 *            S_w = sum_i x_i w_i exp(..), w = 1, i_b, i_d, i_b^2, i_d^2, i_b i_d, taken in ONE pass over D (a thread adds its entries
 *            i = t, t + 256, .. in that order, the lanes of a wave are added by a butterfly, the waves in order):
 *                dF/dtau = -(4 pi / D) Im(conj(S) S_d),                dF/df = (4 pi / D) Im(conj(S) S_b),
 *                h_tt = (8 pi^2 / D) (|S_d|^2 - Re(conj(S) S_dd)),      h_ff = (8 pi^2 / D) (|S_b|^2 - Re(conj(S) S_bb)),
 *                h_tf = (8 pi^2 / D) (Re(conj(S) S_bd) - Re(conj(S_d) S_b)).
 *            A step (tau, f) -= H^-1 grad is taken only where H is negative definite, h_tt < 0 and det H > 0; otherwise the fit
 *            ends where it is.  On an axis of length 1 that coordinate never moves and the test is h < 0 of the other.  After
 *            every step the point is clamped to tau0 -+ 1 / (2 n_tau), f0 -+ 1 / (2 n_f): half a MAP cell.  c is S / D of the sums
 *            at the last point.  iters = 0 leaves the grid point; a new detection then takes S from the map's own sums (the second
 *            sum of `Map` above over the row of the intermediate image), so its height is the cell of P_k bit for bit.
 *   States.  Those of admmnet_cfar_f64; a scene of state 3 or 4 has NaN rows, amp, level, resid (and map) and counts 0.
 *       The arguments of admmnet_cfar_f64 under its conditions, and 0 <= iters <= 16, 0 <= sweeps <= 8,
 *       admmnet_cfar_relax_lds_bytes(Nb, Nd, r) != -1 (16 D + 16 r D + 9 r^2 D + 16 (r + 1) (Nb + Nd) + 3216 bytes and the 16-byte
 *       alignment of each array: 8 x 8 with r = 2 takes 9 360 bytes, 16 x 16 with r = 4 takes 63 120, 13 x 262 with r = 1 -- the
 *       largest grid -- 151 664).  Anything else: ADMMNET_E_ARG before a launch.
 *       rows          double [B][Le][3] = (tau mod 1 in [0, 1), f wrapped into [-1/2, 1/2), |c|^2 D = F(tau, f)) in detection
 *                     order, the values after the last sweep; NaN beyond n_det.
 *       amp           complex128 [B][Le] = c, NaN beyond n_det.
 *       counts        int32 [B][3] = n_det (0 .. Le), more (1: a cell was over after Le targets), maps (the maps computed).
 *       info          double [B][3] = level (the mean of Z over the last map, added as `info` of admmnet_cfar_f64; method 0: the
 *                     given value), resid (the mean of |residual|^2 at the end: a noise estimate), state.
 *       map_out       double [B][n_f][n_tau] or NULL: the last map, the one the stop was decided on.
 *       status        int32 [2] as admmnet_cfar_f64.
 *   No host read, no allocation, stream-ordered. */
int64_t admmnet_cfar_relax_lds_bytes(int32_t Nb, int32_t Nd, int32_t r);   /* -1: bad sizes, or more than a workgroup has */
int admmnet_cfar_relax_f64(int32_t Nb, int32_t Nd, int32_t r, int32_t Le, int64_t B, const void *y, const void *b,
                           const int32_t *symbols, int32_t psk_m, double psk_phase, int32_t method, int32_t guard, int32_t train,
                           int32_t rank, double alpha, const double *noise_var, int32_t iters, int32_t sweeps, double *rows, void *amp,
                           int32_t *counts, double *info, double *map_out, int32_t *status, void *stream);

/* AdamW and gradient-norm clipping over a LIST of float32 tensors (csrc/optim.hip): what a training loop writes as
 * torch.nn.utils.clip_grad_norm_(params, max_norm) and torch.optim.AdamW(...).step().  `count` tensors, tensor i dense with
 * numel[i] >= 0 elements; grads, params, exp_avg, exp_avg_sq are HOST arrays of `count` DEVICE pointers (as `params` of
 * admmnet_train_head_f32), numel and hyper_index HOST arrays.  A pointer may be NULL only where numel[i] = 0.  Tensors need only
 * their natural 4-byte alignment; 16-byte accesses are used where every pointer of a tensor is 16-byte aligned and numel[i] is a
 * multiple of four.  The lists travel in the kernel arguments, a longer list in consecutive launches (256 tensors each for the
 * norm and the scaling, 64 for the update); the work is cut into blocks of 1024 elements of ONE tensor, numbered in list order,
 * so the order of every sum depends on the list alone.  No atomics: every run gives the same bits.  count = 0 succeeds and does
 * nothing.  The calls are stream-ordered and never synchronise with the host.
 *   admmnet_optim_partials      the float64 entries of `partials` for this list (its number of blocks); -1 for a negative
 *                               count or numel, or more than 2^31 - 1 blocks.
 *   admmnet_optim_gradnorm_f32  sumsq[0] = sum of g^2 over all tensors, squares and sums in float64;
 *                               total_norm[0] = (float) sqrt(sumsq);
 *                               coef[0] = clamp(max_norm / (total_norm + 1e-6), max = 1) in float32 as torch evaluates it:
 *                               (1 / (total_norm + 1e-6f)) * max_norm, a NaN kept (an infinite norm gives 0).
 *   admmnet_optim_scale_f32     g <- g coef[0] for every tensor (it multiplies by a coefficient of 1 too, as torch does).
 *   admmnet_optim_adamw_f32     per element, torch.optim.adam._single_tensor_adam with decoupled weight decay, in float32:
 *                                 p <- p decay;  m <- m + (g - m) one_minus_beta1;  v <- beta2 v + (one_minus_beta2 g) g;
 *                                 p <- p - step_size m / (sqrt(v) / bias_correction2_sqrt + eps)
 *                               with tensor i's constants hyper[hyper_index[i]] (each rounded to float32 once; nhyper >= 1 sets,
 *                               one per distinct (group, step count) pair; a launch holds eight).  sqrt and / are correctly
 *                               rounded.  With coef_or_null given, g coef[0] rounded to float32 takes the place of g (the
 *                               gradients themselves stay as they are): the same bits as admmnet_optim_scale_f32 followed by
 *                               the update without a coefficient.
 *   admmnet_optim_pack_f32      the list's tensors copied, in list order, into the contiguous buffer `flat` (the sum of numel
 *                               floats; anything behind stays untouched): the bucket of a gradient all-reduce or a parameter
 *                               broadcast, one launch per 256 tensors instead of one copy per tensor.
 *   admmnet_optim_unpack_f32    `flat` copied back into the list's tensors.  Both use the 16-byte path for a tensor whose
 *                               pointer AND place in `flat` are 16-byte aligned and whose numel is a multiple of four. */
typedef struct admmnet_adamw_hyper {
    double decay;                  /* 1 - lr weight_decay  */
    double one_minus_beta1;
    double beta2;
    double one_minus_beta2;
    double step_size;              /* lr / (1 - beta1^t)   */
    double bias_correction2_sqrt;  /* sqrt(1 - beta2^t)    */
    double eps;
} admmnet_adamw_hyper;
int64_t admmnet_optim_partials(int32_t count, const int64_t *numel);
int admmnet_optim_gradnorm_f32(int32_t count, const float *const *grads, const int64_t *numel, float max_norm, double *partials,
                               double *sumsq, float *total_norm, float *coef, void *stream);
int admmnet_optim_scale_f32(int32_t count, float *const *grads, const int64_t *numel, const float *coef, void *stream);
int admmnet_optim_adamw_f32(int32_t count, float *const *params, const float *const *grads, float *const *exp_avg,
                            float *const *exp_avg_sq, const int64_t *numel, const int32_t *hyper_index, int32_t nhyper,
                            const admmnet_adamw_hyper *hyper, const float *coef_or_null, void *stream);
int admmnet_optim_pack_f32(int32_t count, const float *const *tensors, const int64_t *numel, float *flat, void *stream);
int admmnet_optim_unpack_f32(int32_t count, float *const *tensors, const int64_t *numel, const float *flat, void *stream);

/* Spectrum |phi^H kron(s(f), conj d(tau))|^2 on a (tau, f) grid:
 * peak_search_func / peak_search, utils/peakSearchUtils.py:9-60, evaluated in
 * float64 like the reference.
 *   phi device complex64 [B][ybase*xbase] (index ks*xbase + kd);
 *   taus [nx], fs [ny] device float64;  out device float64 [B][ny][nx];
 *   workspace: device scratch of admmnet_spectrum_workspace_bytes() bytes. */
int64_t admmnet_spectrum_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny);
int admmnet_spectrum_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase,
                         const double *taus, int32_t nx, const double *fs, int32_t ny,
                         double *out, void *workspace, int64_t workspace_bytes, void *stream);

/* Batched grid peak search on that spectrum: alt_peak_search, utils/peakSearchUtils.py:63-173
 * (coarse grid -> regional maxima, skimage local_maxima(connectivity=2) semantics -> `iters`
 * refinement rounds), one signal per workgroup.
 *   axis_x [nx], axis_y [ny]: the coarse grid (np.arange(xmin, xmax - xstep, xstep) and the
 *     reference's np.arange(ymin, ymax - xstep, ystep), :105-106), device float64;
 *   opts7 (host): xmin, xmax, xstep, ymin, ymax, ystep, reducefactor;
 *   peaks device float64 [B][max_peaks][3] = (x = tau, y = f, height) in np.where row-major order
 *     of the coarse maxima (callers sort by height, main_for_net.py:119); rows >= count are not written;
 *   counts device int32 [B]: number of regional maxima found (may exceed max_peaks: truncated);
 *   workspace: device scratch of admmnet_peak_search_workspace_bytes() bytes (tables + coarse spectra). */
int64_t admmnet_peak_search_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny, int64_t B);
int admmnet_peak_search_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase,
                            const double *axis_x, int32_t nx, const double *axis_y, int32_t ny,
                            const double *opts7, int32_t iters, int32_t max_peaks, double *peaks,
                            int32_t *counts, void *workspace, int64_t workspace_bytes, void *stream);

/* Top-L target estimation: that peak search followed by the two lines both inference callers of the reference add,
 * res = sorted(res, key=lambda x: x[2], reverse=True); res = res[:L]  (main_for_net.py:117-126,
 * test/test_model_peaksearch.py:85-96), in one kernel, one signal per workgroup (csrc/estimate.hip).  The coarse
 * spectrum stays on the chip and no peak list is kept: every regional maximum takes part, whatever their number.
 *   phi, axis_x, axis_y, opts7, iters: as for admmnet_peak_search_f64, whose rows these are bit for bit;
 *   L: 1 .. 64;  top_n: device int32 [B], the number of rows wanted of signal b (clamped to 0 .. L; the sample's own
 *     L_true at test_model_peaksearch.py:91), or NULL for L rows of every signal;
 *   top device float64 [B][L][3] = (x = tau, y = f, height), row r = the peak of rank r, where peak k (np.where order)
 *     has rank #{j : h_j > h_k} + #{j < k : h_j == h_k} (Python's stable sort, reverse=True) and h is the height after
 *     the last refinement round that ran for the peak, 0.0 if none did (:136-171 leave res[k, 2] untouched);
 *     rows r >= min(counts[b], top_n[b]) are NaN;
 *   counts device int32 [B]: number of regional maxima, the value admmnet_peak_search_f64 reports;
 *   workspace: device scratch of admmnet_peak_top_workspace_bytes() bytes (the steering tables: independent of B).
 * B >= 0.  A grid whose image does not fit one workgroup's LDS is ADMMNET_E_ARG. */
int64_t admmnet_peak_top_workspace_bytes(int32_t xbase, int32_t ybase, int32_t nx, int32_t ny);
int admmnet_peak_top_f64(const void *phi, int64_t B, int32_t xbase, int32_t ybase,
                         const double *axis_x, int32_t nx, const double *axis_y, int32_t ny,
                         const double *opts7, int32_t iters,
                         int32_t L, const int32_t *top_n,
                         double *top, int32_t *counts,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* The regional-maxima stage of that kernel alone, on caller-supplied images: skimage.morphology.local_maxima(
 * connectivity=2) as used at utils/peakSearchUtils.py:118 (8-connected, plateau aware, borders allowed, a constant
 * image has none; the reference's own example input is the plateau matrix at :427-432).
 *   Z device float64 [B][ny][nx];  peaks device float64 [B][max_peaks][3] = (column, row, 0) of every maximum
 *   pixel in np.where row-major order;  counts device int32 [B]. */
int admmnet_regional_maxima_f64(const double *Z, int64_t B, int32_t nx, int32_t ny, int32_t max_peaks,
                                double *peaks, int32_t *counts, void *stream);

/* Batched scene synthesis + classical-solver labels on the device: generate_data.py:133-221 (_generate_single_sample,
 * _generate_communication_symbols) and the phi label of DatasetGeneratorCreatePhi (:410-463 = admm_for_us(y, b, ...),
 * which as written is the recursion phi_k = W (y / b + rho phi_{k-1}) stopped at min_iter).
 *   outputs (device): y, b complex64 [B][Nb*Nd]; sigma float [B]; tau, f float [B][L]; C complex64 [B][L];
 *   phi_label complex64 [B][Nb*Nd] or NULL.  snr_lo..snr_hi: range of the per-sample SNR in dB (equal = fixed);
 *   snr_e: demodulation SNR (7); rho, label_iters: the classical solver's rho (1) and its iteration count (5).
 *   Counter-based generator: (seed, sample index) fixes a sample regardless of B or launch geometry.
 *   1 <= L <= 8, label_iters >= 0, B < 2^31.  One workgroup holds y, b and the label recursion of a sample in float64 in
 *   LDS: 48 Nb Nd + 352 bytes, which must fit the 160 KiB of a CU, so Nb * Nd <= 3406.  Anything else returns
 *   ADMMNET_E_ARG with a message, before anything is launched. */
int admmnet_synth_batch(int64_t B, int32_t Nb, int32_t Nd, int32_t L, uint64_t seed, double snr_lo, double snr_hi,
                        double snr_e, double rho, int32_t label_iters, void *y, void *b, float *sigma, float *tau,
                        float *f, void *C, void *phi_label, void *stream);

/* admmnet_synth_batch with a varying number of targets per scene, an optional minimum separation between them, and what a
 * scene's consumer needs to know about it.  Same recipe, arithmetic, generator, geometry and LDS (Nb * Nd <= 3406).
 *   count      n = L_min + min(L_max - L_min, floor(u (L_max - L_min + 1))), u in (0, 1] the draw of stream 8, index 0.
 *   positions  target l < n, attempt t = 0 .. 31: tau = 0.1 + 0.8 u(stream tau, l + 8 t), f = -0.4 + 0.8 u(stream f, l + 8 t);
 *              attempt 0 is admmnet_synth_batch's draw.  Targets are placed in order l = 0, 1, ..; an attempt is accepted when
 *              every target j < l already placed has (Nd wrap(dtau))^2 + (Nb wrap(df))^2 >= min_sep^2, wrap(d) = d - round(d):
 *              a distance in resolution cells with period 1 on both axes, the measure of admmnet_score_match_f64 with
 *              scale (Nd, Nb) and period (1, 1).  min_sep = 0 accepts attempt 0 without evaluating anything.  If none of the
 *              32 attempts is accepted the last one stays and the scene's state is 1: no scene is dropped or redrawn whole.
 *   C          of target l as admmnet_synth_batch draws it, whatever the attempt.
 *   padding    slots l >= n of tau, f, C [B][L_max] are exact zeros (generate_data.py:91-103) and add nothing to Psi.
 *   outputs besides admmnet_synth_batch's (device, all required): L_true int64 [B] = n, as admmnet_score_match_f64 and
 *              admmnet_crb_f64 read it; snr_db double [B], the drawn SNR; noise_var double [B], the variance of a complex
 *              entry of w; ser float [B] = 100 #{decided symbol != sent symbol} / (Nb Nd) (generate_data.py:219);
 *              state int32 [B], 0 or 1.
 *   With L_min = L_max = L and min_sep = 0 the seven outputs shared with admmnet_synth_batch have its bits.
 *   1 <= L_min <= L_max <= 8, min_sep finite and >= 0, label_iters >= 0, 1 <= B < 2^31, Nb, Nd >= 1, Nb * Nd <= 3406, no
 *   null pointer but phi_label: anything else returns ADMMNET_E_ARG with a message, before anything is launched. */
int admmnet_synth_scenes(int64_t B, int32_t Nb, int32_t Nd, int32_t L_min, int32_t L_max, double min_sep, uint64_t seed,
                         double snr_lo, double snr_hi, double snr_e, double rho, int32_t label_iters, void *y, void *b,
                         float *sigma, float *tau, float *f, void *C, void *phi_label, int64_t *L_true, double *snr_db,
                         double *noise_var, float *ser, int32_t *state, void *stream);

/* ---- measurement hooks (bench.py roofline leg) ---------------------------------
 * When enabled, every kernel launcher brackets its launch with HIP events on the
 * caller's stream.  admmnet_profile_read synchronises those events, returns the
 * summed milliseconds and launch counts per kernel class and clears the buffer.
 * Classes: 0 prep, 1 tridiag, 2 tridiagonal eigensolver, 3 back-transform (V = Q W),
 * 4 rebuild, 5 zstep, 6 head, 7 spectrum, 8 G-layer as a matrix function (ADMMNET_KERNEL_CLASSES entries).
 * The event pool grows with the number of launches between two reads; a launch is only left out when an event
 * cannot be created, and admmnet_profile_dropped() returns how many were (0 in any healthy run; bench.py refuses
 * to print per-step sums otherwise).  Guarded by one mutex; off by default. */
#define ADMMNET_KERNEL_CLASSES 9
int admmnet_profile_enable(int32_t on);
int admmnet_profile_read(double *ms_total, int64_t *launches, int32_t nclasses);
int64_t admmnet_profile_dropped(void);

#ifdef __cplusplus
}
#endif
#endif /* ADMMNET_H */
