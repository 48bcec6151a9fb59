/*
 * spml_hip.h -- C-ABI of libspml_hip.so: the MI355X (gfx950) kernels behind the
 * SPML pixel-to-segment contrastive hot path.
 *
 * The reference (twke18/SPML) has no FFI: its hot path is a set of Python
 * callables made of ATen op chains.  Each entry point
 * below replaces one such chain; the reference file:line it replaces is cited
 * on the declaration.  The Python mirrors under spml_amd/ bind these with
 * ctypes (spml_amd/_ffi.py); INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions (every function):
 *   - plain device pointers + explicit sizes; row-major, densely packed;
 *   - float data is fp32, labels/indices are int64 at the boundary (the
 *     reference API is int64 everywhere), int32 inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are stream-ordered, nothing synchronises, nothing allocates;
 *   - scratch comes from the caller: `ws`/`ws_bytes`, sized by the matching
 *     `*_workspace_bytes()` query (host-only, no device access);
 *   - return value: SPML_OK (0) or a negative spml_status; never throws.
 */
#ifndef SPML_HIP_H_
#define SPML_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum spml_status {
  SPML_OK = 0,
  SPML_ERR_INVALID_ARG = -1,   /* null pointer, negative size, bad alignment */
  SPML_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels cover        */
  SPML_ERR_WORKSPACE = -3,     /* workspace missing or too small              */
  SPML_ERR_LAUNCH = -4         /* hipGetLastError() != hipSuccess after launch */
} spml_status;

/* Human-readable text for a status code (static storage). */
const char* spml_status_string(int status);

/* ABI version: bumped on any signature change. */
/* Bumped whenever an entry point changes its arguments or a flag its meaning; spml_amd/_ffi.py refuses a library
 * whose version differs from the header it was written against.  2: round 4 (count_dev in the batch-norm backward,
 * spml_bn_finalize_ranks_f32); 3: round 5 (SPML_KMEANS_NO_PASS64 / _TWO_KERNEL_FINALIZE / _NO_V4K, paths "mfma_f16x2_v4p", "mfma_f16x2_v4k");
 * 5: the softmax-inference entry points (spml_unit_hl8_from_nchw_f32 .. spml_iou_counts_i64);
 * 6: the pseudo-label entry points (spml_resample_unit_f32 .. spml_upsample_argmax_i64);
 * 7: the multi-scale inference entry point (spml_view_probs_accumulate_f32);
 * 8: spml_upsample_ce_bwd_path_name (entry points added since leave every earlier signature and flag as it was and
 *    keep the version: spml_view_votes_*, spml_segsort_nll_batched_*, spml_segment_majority_*, spml_tag_normalize_*,
 *    spml_dense_crf_*, spml_segment_tag_cam_*, spml_conv_hl8_path_name, spml_conv_wgrad_path_name / _splits,
 *    spml_augment_*, spml_image_views_*, spml_label_export_*, spml_score_*, spml_pca_*, spml_summary_panels_u8,
 *    spml_train_summary_workspace_bytes, spml_crf_guide_*, spml_export_scores_bytes, spml_label_export_scored_u8,
 *    spml_segsort_nll_path_name, spml_cam_ingest_*). */
#define SPML_ABI_VERSION 8
int spml_abi_version(void);

/* ------------------------------------------------------------------------
 * Deterministic mode (process-wide, off by default; 4: round 6).  The segment sums of A4 and the prototype
 * gradient of A9/A10 are sums of many fp32 terms that meet through atomics: run to run the bits differ (the reference's
 * own `scatter_add_` / `index_add` on a GPU does the same, segsort/common.py:34-39).  With the mode on, those sums are
 * formed in 64-bit fixed point (2^36 steps per unit, integer atomics: order-independent, hence bit-reproducible):
 *   - spml_segment_sum_normalize_f32 is refused (SPML_ERR_UNSUPPORTED); use spml_segment_sum_normalize_det_f32
 *     (same result to one fp32 rounding of the exact sum; domain |x| < 2^26 / P);
 *   - spml_segsort_nll_bwd_f32 accumulates d_protos / gscale in fixed point (its workspace grows by M * D * 8 bytes:
 *     query spml_segsort_nll_workspace_bytes AFTER switching the mode);
 *   - the generic k-means route does the same for its M-step (workspace: + n_img * K * D * 8 bytes);
 *   - spml_conv_hl8_pyramid_f32 does not split its taps over workgroups.
 * k-means fast paths, K1, the forward NLL, top-k, relabel and the convolutions are deterministic in either mode.
 * (Whole training steps: the Python side -- spml_amd/train.py -- additionally routes the framework convolutions that
 * remain through fixed-order GEMMs, spml_amd/nn/conv.py; tests/test_determinism_gpu.py.)
 * spml_set_deterministic returns the previous value.
 * ------------------------------------------------------------------------ */
int spml_set_deterministic(int on);
int spml_get_deterministic(void);

/* 0 for a product build.  Non-zero: the library was compiled with the profiling switches of csrc/conv.hip (low 16 bits,
 * SPML_CONV_EXP) or csrc/kmeans64.hip (high 16 bits, SPML_P64_EXP) -- variants that skip work and overwrite outputs;
 * spml_amd/_ffi.py refuses such a library unless the same environment variable is still set. */
int spml_build_experiment(void);

/* ------------------------------------------------------------------------
 * K1  normalise + NCHW->NHWC + location concat + normalise
 * replaces: segsort/common.py:306-310 (permute/contiguous/normalize),
 *           :313-317 (location features), :346-352 (cat + normalize),
 *           :355-365 (ignore-pixel removal, folded in through row_map),
 *           general/common.py:101-120 (normalize_embedding).
 *
 *   emb      [N,C,H,W]   input embedding map
 *   loc      [N,H,W,2]   location features, or NULL -> generated in-kernel as
 *                        (y/(H-1)-0.5, x/(W-1)-0.5)  (common.py:156-189 'float')
 *   row_map  [N*H*W]     destination row of every pixel, or -1 to drop it
 *                        (ignore_index pixels); NULL -> identity
 *   out_emb  [P',C]      x / max(|x|,1e-12)
 *   out_loc  [P',C+2]    normalize(cat(out_emb, loc))
 * backward: d_emb[N,C,H,W] from d_out_emb / d_out_loc (either may be NULL).
 * ------------------------------------------------------------------------ */
int spml_normalize_concat_loc_f32(const float* emb, int N, int C, int H, int W,
                                  const float* loc, const int64_t* row_map,
                                  float* out_emb, float* out_loc, void* stream);

int spml_normalize_concat_loc_bwd_f32(const float* emb, int N, int C, int H,
                                      int W, const float* loc,
                                      const int64_t* row_map,
                                      const float* d_out_emb,
                                      const float* d_out_loc, float* d_emb,
                                      void* stream);

/* K1 with L local-feature channels instead of the 2 location channels: local [N,H,W,L]
 * (1 <= L <= 8; the DensePose recipe appends (y, x) + 3 smoothed colours,
 * resnet_pspnet_densepose.py:37-38 -> L = 5); out_loc / d_out_loc are [P',C+L].
 * local == NULL is only allowed with L == 2 (location generated in-kernel). */
int spml_normalize_concat_local_f32(const float* emb, int N, int C, int H, int W,
                                    const float* local, int L,
                                    const int64_t* row_map, float* out_emb,
                                    float* out_loc, void* stream);

int spml_normalize_concat_local_bwd_f32(const float* emb, int N, int C, int H,
                                        int W, const float* local, int L,
                                        const int64_t* row_map,
                                        const float* d_out_emb,
                                        const float* d_out_loc, float* d_emb,
                                        void* stream);

/* The same two calls for a channels-last map (emb / d_emb stored [N, H, W, C], what the backbone hands
 * over when it runs NHWC): the pixel rows are already contiguous, K1 is a row-wise stream without a
 * transposition.  C in {16, 32, 64, 128, 256, 512} (spml_normalize_concat_local_nhwc_supported), else
 * SPML_ERR_UNSUPPORTED -- convert and use the NCHW entry points. */
int spml_normalize_concat_local_nhwc_supported(int C, int L);
int spml_normalize_concat_local_nhwc_f32(const float* emb, int N, int C, int H, int W,
                                         const float* local, int L,
                                         const int64_t* row_map, float* out_emb,
                                         float* out_loc, void* stream);
int spml_normalize_concat_local_nhwc_bwd_f32(const float* emb, int N, int C, int H,
                                             int W, const float* local, int L,
                                             const int64_t* row_map,
                                             const float* d_out_emb,
                                             const float* d_out_loc, float* d_emb,
                                             void* stream);

/* Plain row-wise L2 normalise of a [rows, D] matrix (general/common.py:101-120),
 * and its backward.  inv_norm_out (optional) receives 1/max(|x|,eps). */
int spml_normalize_rows_f32(const float* x, int64_t rows, int D, float* y,
                            void* stream);
int spml_normalize_rows_bwd_f32(const float* x, const float* dy, int64_t rows,
                                int D, float* dx, void* stream);

/* ------------------------------------------------------------------------
 * A7  dense re-indexing of integer keys (label algebra)
 * replaces: the `torch.unique(keys, return_inverse=True)` calls of
 *           segsort/common.py:192-218 (prepare_prototype_labels), :398-405 (segment_by_kmeans)
 *           and models/utils.py:94-111 (gather_clustering_and_update_prototypes)
 *   keys [P] int64 (any value except INT64_MIN) ->
 *   inv [P] int64: position of keys[i] among the sorted distinct keys;
 *   uniq [uniq_capacity] int64: the first uniq_capacity sorted distinct keys (pass P to get all);
 *   count [1] int64 (device): number of distinct keys.
 * Hash set + rank among the distinct keys: no sort of the P keys, deterministic, stream-ordered, no
 * host synchronisation (the caller reads `count` when it needs the number on the host).
 * ------------------------------------------------------------------------ */
size_t spml_relabel_unique_workspace_bytes(int64_t P);
int spml_relabel_unique_i64(const int64_t* keys, int64_t P, int64_t* inv, int64_t* uniq,
                            int64_t uniq_capacity, int64_t* count, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A3  grid initialisation of cluster labels
 * replaces: segsort/common.py:129-153 (initialize_cluster_labels)
 *   out [H,W] int64 = round(linspace(0,Ky-1,H))[:,None]
 *                     + (max_y+1) * round(linspace(0,Kx-1,W))[None,:]
 * ------------------------------------------------------------------------ */
int spml_kmeans_init_grid_i64(int H, int W, int Ky, int Kx, int64_t* out,
                              void* stream);

/* ------------------------------------------------------------------------
 * A4+A5+A6  spherical k-means over a ragged batch of images
 * replaces: segsort/common.py:67-97 (kmeans_with_initial_labels) and the
 *           per-image Python loop at :337-373, i.e. for every image
 *           `iterations` x { M-step :11-41 (scatter_add + normalize),
 *                            E-step :44-64 (mm + argmax) }.
 *
 *   x            [P,D]        unit-norm rows (embedding + location), P = sum of
 *                             all images' kept pixels, images back to back
 *   seg_offsets  [n_img+1]    DEVICE int64: image b owns rows
 *                             [seg_offsets[b], seg_offsets[b+1])
 *   max_seg_len               HOST upper bound on any image's row count (H*W)
 *   K                         clusters per image (labels are 0..K-1 per image)
 *   labels_init  [P]          int64 initial labels
 *   labels_out   [P]          int64 final labels (may alias labels_init)
 *   centroids_out [n_img,K,D] optional: the prototypes used by the last E-step
 *   flags                     SPML_KMEANS_* bits
 * One "pass" streams X once: E-step against the current prototypes fused with
 * the M-step accumulation for the next ones (iterations+1 passes in total, the
 * first one accumulate-only).  Results are run-to-run deterministic.
 * ------------------------------------------------------------------------ */
#define SPML_KMEANS_DEFAULT 0
#define SPML_KMEANS_FORCE_GENERIC 1 /* skip the MFMA fast paths (testing) */
#define SPML_KMEANS_FORCE_V2 4       /* use the 32x32-tile kernel even where v3 applies */
#define SPML_KMEANS_SEPARATE_PRECONVERT 16 /* convert X in its own kernel instead of inside
                                       the seed pass (testing / profiling) */
#define SPML_KMEANS_NO_PRECONVERT 8 /* keep X in fp32 and split it inside every pass (the
                                       default for < 3 passes) instead of converting it
                                       once to the MFMA operand layout up front */
#define SPML_KMEANS_NO_SCREEN 64     /* many-cluster path: skip the hi-half screening pass and score
                                       every pixel with the exact split-f16 kernel (testing / A-B) */
#define SPML_KMEANS_WS_PRECONVERTED 32 /* assign / fused pass: `ws` already holds X converted by
                                       spml_kmeans_preconvert_f32 (same x, sizes, ws) */
#define SPML_KMEANS_PASS_ONLY 256    /* spml_kmeans_fused_pass_f32 with SPML_KMEANS_WS_PRECONVERTED, measurement
                                       only: launch the pass kernel alone -- `ws` still holds the split centroids
                                       of a previous call with the same arguments, labels are written, the
                                       per-workgroup sums stay in `ws` and centroid_sums_out is not touched;
                                       bits 16..23 of flags: number of back-to-back launches (0 = 1) */

#define SPML_KMEANS_NO_PASS64 512    /* K <= 48 on pre-converted tiles: keep the E-step passes on the
                                       32-pixel-tile kernel (kmeans_pass16) instead of the pixel-split
                                       64-pixel-tile kernel (kmeans_pass64) (testing / A-B) */

#define SPML_KMEANS_TWO_KERNEL_FINALIZE 1024 /* slabs -> prototypes with kmeans_reduce_slabs + kmeans_normalize
                                       instead of the one-launch kmeans_finalize (testing / A-B).  NOTE on bits: a call
                                       is bit-reproducible run to run, but the two forms combine the per-workgroup
                                       partial sums in different (fixed) orders, and the default picks the one-launch
                                       form from 128 (padded cluster, image) rows on -- so the SAME image can get
                                       prototypes that differ in the last bit (and near-tie labels) depending on how
                                       many images share the call; pass this flag where the bits must not depend on
                                       the batch */

#define SPML_KMEANS_NO_V4K 2048      /* 64 < K <= 144 on wide rows (D = 128.. / 256.. + <= 8): skip the wave-split
                                       assign + accumulate passes on 64-pixel tiles ("mfma_f16x2_v4k"); the call
                                       takes the many-cluster kernels ("mfma_f16x2_bigk") (testing / A-B) */

/* Bytes of `ws` for any k-means entry point with these sizes, whatever its flags and iterations.  The size does not
 * depend on the deterministic mode (the fixed-point scratch of the generic route's sums, n_img * K * D * 8 bytes, is
 * always reserved): a workspace sized before spml_set_deterministic(1) serves the calls after it. */
size_t spml_kmeans_workspace_bytes(int64_t P, int D, int K, int n_img,
                                   int64_t max_seg_len);

/* Measurement aid (bench.py): one wave waits `spin_us` microseconds and writes out[0] = elapsed shader cycles
 * (s_memtime), out[1] = elapsed 100-MHz ticks (s_memrealtime): shader clock = 100 MHz * out[0] / out[1] while the
 * kernels of the other streams run. */
int spml_clock_probe(uint64_t* out, int spin_us, void* stream);

/* 3 x 3 / stride 2 / padding 1 max-pool of a channels-last map x [n][H][W][C] -> y [n][(H-1)/2+1][(W-1)/2+1][C]
 * (the stem's nn.MaxPool2d(kernel_size=3, stride=2, padding=1), spml/models/backbones/resnet.py:66-110).  Forward
 * only (conv1 / res2 are frozen: no gradient flows here).  C % 4 == 0, 16-byte aligned pointers. */
int spml_maxpool3x3s2_nhwc_f32(const float* x, int n, int H, int W, int C, float* y, void* stream);

int spml_kmeans_run_f32(const float* x, int64_t P, int D,
                        const int64_t* seg_offsets, int n_img,
                        int64_t max_seg_len, int K, const int64_t* labels_init,
                        int iterations, int64_t* labels_out,
                        float* centroids_out, int flags, void* ws,
                        size_t ws_bytes, void* stream);

/* E-step alone (find_nearest_prototypes, segsort/common.py:44-64) for a ragged
 * batch: labels_out[p] = argmax_k <x_p, centroids[img(p),k]>, ties -> lowest k.
 * centroids [n_img,K,D] need not be normalised.
 * Input domain of the MFMA paths: operands are split into two f16 halves (22 mantissa
 * bits, f16 exponent range), so every |x| and |centroid| element must be < 65504 and the
 * dot products are exact to ~2^-22 RELATIVE TO the operands' largest elements; unit-norm
 * rows (what the reference clusters) are the intended use.  The many-cluster path
 * ("mfma_f16x2_bigk") additionally needs |x| <= 1 in its M-step (fixed-point sums).  Pass
 * SPML_KMEANS_FORCE_GENERIC for arbitrary fp32 data (plain fp32 FMA kernels). */
int spml_kmeans_assign_f32(const float* x, int64_t P, int D,
                           const int64_t* seg_offsets, int n_img,
                           int64_t max_seg_len, int K, const float* centroids,
                           int64_t* labels_out, int flags, void* ws,
                           size_t ws_bytes, void* stream);

/* One fused pass (A5 + the scatter-sum half of A4; segsort/common.py:44-64 then :11-36):
 *   labels_out[p]        = argmax_k <x_p, centroids_in[img(p),k]>        int64 [P]
 *   centroid_sums_out    = sum of the rows of X by their NEW label       [n_img,K,D]
 * (un-normalised; the caller normalises, e.g. with spml_normalize_rows_f32, to get the
 * next prototypes).  X is streamed from HBM once.  This is the kernel the HBM roofline
 * of the k-means path is quoted on ("kmeans_pass16" for D = 32q + {0,2}, K <= 64).
 * With SPML_KMEANS_WS_PRECONVERTED the pass reads the split-f16 tiles that
 * spml_kmeans_preconvert_f32 left in `ws` (what spml_kmeans_run_f32 does from its second
 * pass on); without it X is split inside the pass. */
int spml_kmeans_fused_pass_f32(const float* x, int64_t P, int D,
                               const int64_t* seg_offsets, int n_img,
                               int64_t max_seg_len, int K,
                               const float* centroids_in, int64_t* labels_out,
                               float* centroid_sums_out, int flags, void* ws,
                               size_t ws_bytes, void* stream);

/* X fp32 [P,D] -> split-f16 fragment tiles inside `ws` (once per X; only for the shapes
 * whose pass kernels take pre-converted tiles, else SPML_ERR_UNSUPPORTED). */
int spml_kmeans_preconvert_f32(const float* x, int64_t P, int D,
                               const int64_t* seg_offsets, int n_img,
                               int64_t max_seg_len, int K, void* ws,
                               size_t ws_bytes, void* stream);

/* Name of the code path a k-means call with these (host-visible) arguments takes; a pure
 * function (no state), for tests and the bench report.  given_centroids != 0: the assign /
 * fused-pass entry points.
 *   "mfma_f16x2_v4p"  D = 32q + {0,2}, q in {1,2,4,8}, K <= 48, >= 3 passes (pre-converted X): E-step passes
 *                     on kmeans_pass64 (64-pixel tiles, pixel-split E-step), seed pass on kmeans_pass16
 *   "mfma_f16x2_v3p"  the same for 48 < K <= 64 (or SPML_KMEANS_NO_PASS64): every pass on kmeans_pass16
 *   "mfma_f16x2_v3"   same shapes, < 3 passes (tile split to f16 in LDS inside the pass)
 *   "mfma_f16x2_v3k"  64 < K <= 256, q in {1,2,4} within the register budget, >= 3 passes
 *   "mfma_f16x2_v4k"  64 < K <= 144, q in {4,8}, tail <= 8 outside v3k (e.g. K = 144, D = 258), >= 3 passes: an assign
 *                     kernel with the prototype tiles split over eight waves + an accumulate kernel on the same
 *                     64-pixel tiles (kmeans64k.hip); SPML_KMEANS_NO_V4K: "mfma_f16x2_bigk"
 *   "mfma_f16x2"      other even D <= 320 with K <= 64 (32x32x16 tiles, k-split)
 *   "mfma_f16x2_bigk" K > 64 outside the shapes above with D <= 528 (e.g. K = 1024, D = 514;
 *                     kmeans_big.hip): pixel-stationary MFMA E-step with a running arg-max,
 *                     counting-sort + fixed-point gather M-step
 *   "generic"         everything else (fp32 FMA assign + scatter-sum) */
const char* spml_kmeans_path_name(int64_t P, int D, int K, int n_img,
                                  int64_t max_seg_len, int iterations,
                                  int given_centroids, int flags);

/* Profiling variant of spml_kmeans_run_f32 (tile-kernel paths only): every workgroup of
 * every pass kernel stamps its start and end time (s_memrealtime, 100 MHz) into
 * pass_clocks[pass][workgroup][2] -- device memory, nothing is synchronised and no host
 * timers or events are involved; the caller derives each launch's duration as
 * max(end) - min(start).  Pass p of iterations+1: 0 = seed (M-step on labels_init),
 * 1..iterations-1 = fused E+M passes, iterations = final E-only pass.
 * spml_kmeans_profile_layout gives the two dimensions. */
int spml_kmeans_profile_layout(int64_t P, int D, int K, int n_img,
                               int64_t max_seg_len, int iterations,
                               int* n_passes, int* workgroups_per_pass);

int spml_kmeans_run_profiled_f32(const float* x, int64_t P, int D,
                                 const int64_t* seg_offsets, int n_img,
                                 int64_t max_seg_len, int K,
                                 const int64_t* labels_init, int iterations,
                                 int64_t* labels_out, int flags, void* ws,
                                 size_t ws_bytes, uint64_t* pass_clocks,
                                 size_t pass_clocks_len, void* stream);

/* ------------------------------------------------------------------------
 * A4  segment prototypes: scatter-sum rows by id, then L2 normalise
 * replaces: segsort/common.py:11-41 (calculate_prototypes_from_labels) as
 *           used at models/utils.py:113-116 and segsort.py:236-237.
 *   x [P,D], ids [P] int64 in [0,M)  ->  protos [M,D]; sums [M,D] is scratch
 *   that also feeds the backward (it holds the un-normalised sums).  D <= 1088.
 *   An id outside [0,M) -- negative, >= M, or beyond 32 bits: all 64 bits are
 *   compared -- marks a pixel that belongs to no segment: it adds nothing to
 *   any prototype and its dx row is 0 (with `accumulate`: left as it was).
 * backward: dx[p] = J(ids[p]) where J = d_sums = (dP - P<P,dP>)/|s|
 *           (or dP/eps where |s| < eps).  `accumulate` != 0 adds into dx.
 * ------------------------------------------------------------------------ */
int spml_segment_sum_normalize_f32(const float* x, const int64_t* ids,
                                   int64_t P, int D, int64_t M, float* sums,
                                   float* protos, void* stream);

/* deterministic form (see spml_set_deterministic): ws of spml_segment_sum_det_workspace_bytes(M, D) bytes */
size_t spml_segment_sum_det_workspace_bytes(int64_t M, int D);
int spml_segment_sum_normalize_det_f32(const float* x, const int64_t* ids,
                                       int64_t P, int D, int64_t M,
                                       float* sums, float* protos, void* ws,
                                       size_t ws_bytes, void* stream);

int spml_segment_sum_normalize_bwd_f32(const float* d_protos,
                                       const float* sums, const int64_t* ids,
                                       int64_t P, int D, int64_t M,
                                       float* d_sums_scratch, float* dx,
                                       int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * A9/A10  pixel-to-segment NCA negative log-likelihood ('segsort+' mode)
 * replaces: segsort/loss.py:15-82 (_calculate_log_likelihood) and :85-130
 *           (_one_hot_calculate_log_likelihood): mm -> *kappa -> exp ->
 *           gather own column -> label masks -> two masked row sums ->
 *           where / divide / log.
 *
 *   emb [P,D], protos [M,D] fp32; own [P] int64 = index of the pixel's own
 *   segment among the M prototypes.
 *   mode SPML_NLL_LABEL : positives have  px_code[p] == pr_code[m]
 *   mode SPML_NLL_TAGSET: positives have (px_code[p] &  pr_code[m]) != 0
 *        (multi-hot tag sets packed into 64-bit masks; loss.py:95-113 computes
 *        the same predicate as `tags_px @ tags_pr.T > 0`)
 *   outputs: nll [P]; stats [P,4] = (num, den, own_sim, fallback flag) kept
 *   for the backward.
 * backward: given d_nll [P] (upstream gradient per pixel) produces
 *   d_emb [P,D] and d_protos [M,D] (d_protos is ADDED into; zero it first).
 *   Prototypes [0, m_grad) receive their gradient (m_grad < 0 or > M: all M) -- rows of
 *   a detached memory bank appended after the live prototypes are skipped.  The
 *   kernels work on whole tiles of 32 prototypes: a row in [m_grad, ceil32(m_grad))
 *   receives either nothing or its full gradient (today: the full gradient), rows
 *   from ceil32(m_grad) on are never touched.
 * ------------------------------------------------------------------------ */
#define SPML_NLL_LABEL 0
#define SPML_NLL_TAGSET 1
/* OR-able: group_mode != 'segsort+' (loss.py:71-72): numerator = own-segment
 * similarity only, no positive set */
#define SPML_NLL_PLAIN 2
/* OR-able promise: every px_code / pr_code value fits in 32 bits (labels in [0, 2^31); tag sets
 * over <= 32 classes).  The predicate then runs on 32-bit words (the kernels are bound by
 * that per-pair epilogue); results are identical. */
#define SPML_NLL_CODE32 4

size_t spml_segsort_nll_workspace_bytes(int64_t P, int64_t M, int D);

int spml_segsort_nll_fwd_f32(const float* emb, const int64_t* own,
                             const int64_t* px_code, int64_t P,
                             const float* protos, const int64_t* pr_code,
                             int64_t M, int D, float kappa, int mode,
                             float* nll, float* stats, void* ws,
                             size_t ws_bytes, void* stream);

int spml_segsort_nll_bwd_f32(const float* emb, const int64_t* own,
                             const int64_t* px_code, int64_t P,
                             const float* protos, const int64_t* pr_code,
                             int64_t M, int D, float kappa, int mode,
                             const float* stats, const float* d_nll,
                             float* d_emb, float* d_protos, int64_t m_grad,
                             void* ws, size_t ws_bytes, void* stream);

/* What spml_segsort_nll_fwd_f32 (backward == 0) or spml_segsort_nll_bwd_f32 launches for these arguments, written
 * into buf (len bytes, NUL-terminated; SPML_ERR_INVALID_ARG when it does not fit -- 160 bytes always do).  A host
 * function: no GPU call; it reads the environment switches (SPML_NLL_DE3, SPML_NLL_DP3, SPML_NLL_TCACHE_MB) and the
 * deterministic mode as a call would, through the predicates the call launches by.  For tests and reports.
 *   forward   "fwd2<KS,MTB,label|tag> chunks=C"     D <= 80 with SPML_NLL_CODE32 (C chunks of 3072 prototypes);
 *             "fwd2_plain<...> chunks=C"             the same with SPML_NLL_PLAIN (sums the negatives directly)
 *             "fwd<KS,1,label|tag,c32|c64>"          everything else (KS: 2, 3, 4, 5, 9, 17, 33 k-steps of 16 channels)
 *   backward  "de3<..> rows=R + dp3<..> mt=T"       48 < D <= 64 with CODE32 (the pipelined kernels; R grid rows that
 *                                                    share the prototype chunks, T prototype tiles with a gradient)
 *             "de3<..> rows=R + dp<4,2,..> chunks=C mt=T"     the same with SPML_NLL_DP3=0
 *             "de2<KS,DT,..> rows=R + dp<KS,DT,..> chunks=C mt=T"   D <= 48 with CODE32, or SPML_NLL_DE3=0
 *             "de<KS,DT,..> + dp<KS,DT,..> chunks=C mt=T"     64-bit codes, and 64 < D <= 272
 *             "wide<..> strips=S launches=1+L mt=T"           272 < D <= 528: per strip of pixel tiles one launch pair
 *                                                    that keeps the weight tiles and L that read them back
 *             "... + no dp" where m_grad = 0; " fix64" appended in deterministic mode
 *   "nothing" for P = 0 (the calls return before their first launch); "unsupported" for what the calls refuse. */
int spml_segsort_nll_path_name(int64_t P, int64_t M, int D, int mode, int backward,
                               int64_t m_grad, char* buf, size_t len);

/* A9/A10 over N independent problems in one call
 * replaces: the per-image loop of the image-similarity term, spml/models/predictions/segsort.py:221-241 (one
 *           SegSortLoss per image over that image's pixels and prototypes), which reached the GPU as N times the
 *           launches of spml_segsort_nll_fwd_f32 / _bwd_f32 on grids far smaller than the chip.
 *
 *   Problem i owns the pixel rows [p_off[i], p_off[i+1]) of emb / own / px_code / nll / stats / d_nll / d_emb and
 *   the prototype rows [m_off[i], m_off[i+1]) of protos / pr_code / d_protos.  p_off, m_off: HOST arrays of
 *   n_problems + 1 non-decreasing offsets, p_off[0] = m_off[0] = 0.  own is ABSOLUTE: an index into the
 *   concatenated prototypes (the library subtracts m_off[i]).  D, kappa and mode are shared.
 *   One launch per kernel for every 32 problems (the problem is the grid's z coordinate); every problem runs the
 *   arithmetic of the single-problem call on its rows -- nll, stats and d_emb are bit-identical to N such calls,
 *   d_protos up to the order of its fp32 atomics (bit-identical in deterministic mode).  All prototypes receive a
 *   gradient; d_protos is ADDED into (zero it first).
 *   Covered: 64 < D <= 80 with SPML_NLL_CODE32 (LABEL or TAGSET, with or without PLAIN);
 *   spml_segsort_nll_batched_supported returns 0 for anything else and the calls SPML_ERR_UNSUPPORTED.
 *   A problem without pixels does nothing; n_problems = 0 or no pixel at all: SPML_OK.  Pixels without prototypes
 *   (P_i > 0, M_i <= 0): SPML_ERR_INVALID_ARG.  Workspace: query AFTER switching the deterministic mode. */
int spml_segsort_nll_batched_supported(int D, int mode);

size_t spml_segsort_nll_batched_workspace_bytes(int n_problems, const int64_t* p_off,
                                                const int64_t* m_off, int D);

int spml_segsort_nll_batched_fwd_f32(const float* emb, const int64_t* own,
                                     const int64_t* px_code, const int64_t* p_off,
                                     const float* protos, const int64_t* pr_code,
                                     const int64_t* m_off, int n_problems, int D,
                                     float kappa, int mode, float* nll, float* stats,
                                     void* ws, size_t ws_bytes, void* stream);

int spml_segsort_nll_batched_bwd_f32(const float* emb, const int64_t* own,
                                     const int64_t* px_code, const int64_t* p_off,
                                     const float* protos, const int64_t* pr_code,
                                     const int64_t* m_off, int n_problems, int D,
                                     float kappa, int mode, const float* stats,
                                     const float* d_nll, float* d_emb, float* d_protos,
                                     void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A11/B3  top-k retrieval by cosine affinity
 * replaces: segsort/eval.py:32-35 (mm + full argsort + [:, :k]) and
 *           models/utils.py:198-214 (mm + where(mask) + topk).
 *   q [Q,D], protos [M,D]  ->  idx [Q,k] int64 (descending affinity, ties ->
 *   lowest index), val [Q,k] fp32.  k <= 32, D <= 528.
 *   k > M: the first M entries of a row are all M candidates in that order,
 *   the remaining k - M entries are idx == 0 and val == -inf.
 *   Optional mask predicate (B3): candidate m is allowed for query i iff
 *   q_group[i] == pr_group[m] && pr_valid[m] != 0; disallowed candidates rank
 *   after every allowed one with value `masked_value` (a finite value below
 *   every affinity), among themselves by ascending index.  Pass NULLs for none.
 * ------------------------------------------------------------------------ */
size_t spml_topk_workspace_bytes(int64_t Q, int64_t M, int D, int k);

int spml_topk_affinity_f32(const float* q, int64_t Q, const float* protos,
                           int64_t M, int D, int k, const int64_t* q_group,
                           const int64_t* pr_group, const uint8_t* pr_valid,
                           float masked_value, int64_t* idx, float* val,
                           void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * N2  overlap accumulation of sliding-window crop embeddings (full-resolution
 *     inference, SURVEY.md 8f "next" row N2)
 * replaces: pyscripts/inference/prototype.py:163-178 (the same code is in
 *           inference.py:175-200): per crop, normalize_embedding over the
 *           channels, `embeddings[:, :, sh:eh, sw:ew] += crop`, `counts += 1`.
 *   patch  [C,h,w]   crop embedding of ONE image (NCHW, N = 1)
 *   acc    [C,H,W]   full-resolution sum, updated in place
 *   counts [H,W]     number of crops covering each pixel, updated in place
 *   (sh, sw)         top-left corner of the crop inside the full map
 * The caller divides acc by counts once all crops are in (prototype.py:180-181).
 * ------------------------------------------------------------------------ */
int spml_window_accumulate_f32(const float* patch, int C, int h, int w,
                               float* acc, float* counts, int H, int W, int sh,
                               int sw, void* stream);

/* ------------------------------------------------------------------------
 * N3  pixel x pixel affinity -> random-walk transition matrix (pseudo labels,
 *     SURVEY.md 8f "next" row N3)
 * replaces: pyscripts/inference/pseudo_camrw_crf.py:146-158 (the same code is in
 *           pseudo_softmaxrw_crf.py:137-163): per view
 *           `matmul(E^T, E).mul_(5).add_(-5).exp_()`, mean over the views,
 *           `** 20`, `/ sum(dim=0)`.
 *   emb    [B,C,n]  B augmented views of one image, columns already unit-norm
 *                   (n = (H/8)*(W/8) pixels, C channels)
 *   trans  [n,n]    (mean_b exp(scale*<e_i,e_j> - scale))^power / column sums
 * The walk (trans <- trans @ trans, x6) and `cam @ trans` stay library GEMMs.
 * ------------------------------------------------------------------------ */
size_t spml_affinity_workspace_bytes(int B, int C, int64_t n);

int spml_affinity_transition_f32(const float* emb, int B, int C, int64_t n,
                                 float scale, int power, float* trans, void* ws,
                                 size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * G1 (backbone)  training-mode batch normalisation fused with the ReLU and the residual add
 * replaces: the framework op chains of the reference's bottleneck unit,
 *           spml/models/backbones/resnet.py:42-63  (`relu(bn(conv(x)))` twice, then
 *           `relu(bn(conv(x)) + identity)`), and of its stem (:66-110), for channels-last
 *           fp32 activations.
 *   x, residual, y, dy, dx, d_residual   [R, C] rows = N*H*W pixels (NHWC), C % 4 == 0
 *   mean, m2, invstd, gamma, beta, sums  [C]
 * forward:  spml_bn_stats_f32 -> (the caller turns m2 into invstd = rsqrt(m2 / count + eps),
 *           combining ranks first for SyncBatchNorm, and updates the running statistics) ->
 *           spml_bn_act_apply_f32:  y = act((x - mean) * invstd * gamma + beta [+ residual]).
 * backward: spml_bn_act_bwd_reduce_f32 -> sum_dz = sum(dz), sum_dz_xhat = sum(dz * xhat) with
 *           dz = dy * (y > 0) (y == NULL: no ReLU), the gradients of beta / gamma ->
 *           (all-reduce for SyncBatchNorm) -> spml_bn_act_bwd_apply_f32:
 *           dx = gamma * invstd * (dz - sum_dz / count - xhat * sum_dz_xhat / count),
 *           d_residual = dz.  dx or d_residual may be NULL.  `count` is the number of rows the
 *           statistics were pooled over: a host value, or -- SyncBatchNorm, where the ranks' row
 *           counts may differ (lib/nn/sync_batchnorm/batchnorm.py:124-145 sums the gathered
 *           sizes) -- the device float `count_dev` that spml_bn_finalize_ranks_f32 wrote
 *           (non-NULL count_dev wins; no host read of the gathered counts).
 * ------------------------------------------------------------------------ */
size_t spml_bn_workspace_bytes(int64_t R, int C);

/* Single-rank batch norm, everything in one call: statistics -> invstd + running statistics
 * (momentum; unbiased variance, as torch.nn.BatchNorm2d) -> apply.  mean / invstd [C] are kept
 * for the backward call, which returns d_gamma = sum(dz * xhat), d_beta = sum(dz), dx and
 * (optionally) d_residual. */
int spml_bn_act_fwd_f32(const float* x, const float* residual, int64_t R, int C,
                        const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum,
                        float eps, int relu, float* y, float* mean, float* invstd,
                        void* ws, size_t ws_bytes, void* stream);

int spml_bn_act_bwd_f32(const float* dy, const float* y, const float* x, int64_t R,
                        int C, const float* mean, const float* invstd,
                        const float* gamma, float* d_gamma, float* d_beta,
                        float* dx, float* d_residual, void* ws, size_t ws_bytes,
                        void* stream);

int spml_bn_stats_f32(const float* x, int64_t R, int C, float* mean, float* m2,
                      void* ws, size_t ws_bytes, void* stream);

int spml_bn_act_apply_f32(const float* x, const float* residual, int64_t R, int C,
                          const float* mean, const float* invstd,
                          const float* gamma, const float* beta, int relu,
                          float* y, void* stream);

int spml_bn_act_bwd_reduce_f32(const float* dy, const float* y, const float* x,
                               int64_t R, int C, const float* mean,
                               const float* invstd, float* sum_dz,
                               float* sum_dz_xhat, void* ws, size_t ws_bytes,
                               void* stream);

int spml_bn_act_bwd_apply_f32(const float* dy, const float* y, const float* x,
                              int64_t R, int C, const float* mean,
                              const float* invstd, const float* gamma,
                              const float* sum_dz, const float* sum_dz_xhat,
                              double count, const float* count_dev, float* dx,
                              float* d_residual, void* stream);

/* ---- stride-1 convolutions of the bottleneck stack on the f16 matrix cores, fp32-class ----
 * Replaces the framework convolutions of spml/models/backbones/resnet.py:20-33,42-63 (conv1 /
 * conv2 / conv3 / downsample of a Bottleneck with stride 1: every unit of res4 and res5).
 * "hl8" = split-f16 copy of an fp32 tensor [rows][C] (C % 8 == 0), rows*C*4 bytes:
 *   v * S = h + l, 16-byte units ((row*C/8 + c/8)*2 + part) of 8 channels, part 0 = h, 1 = l;
 *   S = 2^(14-e) for the smallest e with *bound < 2^e (S = 1 when bound is NULL); *bound is a
 *   device float >= max|v|.                                                            */

/* x fp32 [rows][C] -> hl8.  compute_bound != 0: *bound = max|x| is computed first (one more
 * pass over x); otherwise *bound (may be NULL) is taken as given. */
int spml_hl8_from_f32(const float* x, int64_t rows, int C, float* bound,
                      int compute_bound, void* out, void* stream);

/* weights fp32 [Cout][taps][Cin] (the channels-last storage of a conv weight) -> hl8
 * [Cin][taps][Cout] with mirrored taps: the B operand of the data-gradient convolution. */
int spml_hl8_weight_transposed_f32(const float* w, int Cout, int taps, int Cin,
                                   const float* bound, void* out, void* stream);

/* 1 when spml_conv_hl8_f32 handles (K input channels, N output channels, taps in {1, 9}):
 * K % 16 == 0 and N % 64 == 0.  N % 256 == 0 runs the 256-column tiles the kernel is tuned for;
 * N % 128 == 0 and N % 64 == 0 run 128- / 64-column tiles (2 x 2 and 1 x 4 waves), which re-read
 * the activations more often per output (measured 1.5x the library on the res3 shapes, slower than
 * it on the 2048 -> 64 ASPP branches: profiles/r02_conv_kernels.md). */
int spml_conv_hl8_supported(int K, int N, int taps);

/* out[r][n] = sum_{tap,k} a[r + shift(tap)][k] * b[n][tap][k]  (+ addend[r][n]),
 * r = (img*H + oh)*W + ow, shift(tap) = ((tap/3-1)*W + (tap%3-1)) * dilation with zero padding
 * (taps == 9) or 0 (taps == 1).  a: hl8 [n_img*H*W][K], b: hl8 [N][taps*K], out fp32 NHWC.
 * Forward: a = activations, b = weights.  Data gradient: a = dy, b = transposed weights,
 * K = Cout, N = Cin, addend = gradient of the residual branch or NULL; with addend_mask (the ReLU
 * mask bytes of spml_bn_*: [R][N/4], bit n & 3) the addend is the unit's OUTPUT gradient and
 * addend * mask = the residual branch's gradient is formed here instead of being written by the
 * batch-norm backward. */
int spml_conv_hl8_f32(const void* a, const float* a_bound, const void* b,
                      const float* b_bound, const float* addend,
                      const unsigned char* addend_mask, float* out,
                      int n_img, int H, int W, int K, int N, int taps, int dilation,
                      void* stream);

/* The same convolution when a training-mode batch norm follows (resnet.py:42-63: every convolution of a
 * Bottleneck): the epilogue also leaves, per row tile of the launch and per output channel, the mean, the
 * sum of squared deviations, the max and the min of `out` in chunk_stats [4][chunks][N] -- what
 * spml_bn_fwd_hl8_chunks_f32 pools instead of reading `out` once more -- and resets *zero_me (that call's
 * y_bound; may be NULL).  spml_conv_hl8_stats_layout gives chunks / chunk_rows for a shape, or
 * SPML_ERR_UNSUPPORTED where the tiling has no per-tile column owner (N % 256 != 0). */
int spml_conv_hl8_stats_layout(int n_img, int H, int W, int K, int N, int taps,
                               int* chunks, int* chunk_rows);
int spml_conv_hl8_stats_f32(const void* a, const float* a_bound, const void* b,
                            const float* b_bound, float* out, float* chunk_stats,
                            float* zero_me, int n_img, int H, int W, int K, int N,
                            int taps, int dilation, void* stream);

/* The same convolution as the DATA GRADIENT in front of a training-mode batch norm + ReLU of the backward pass
 * (the gradients of conv3 and conv2 of a Bottleneck are the dy of bn2 and bn1): the epilogue also reads the tile of
 * that batch norm's saved input bn_x [R][N], its ReLU mask bytes [R][N/4] and bn_mean [N] and leaves, per row tile
 * of the launch and per channel, sum dz, sum dz * (bn_x - mean) and max |dz| (dz = out where the mask bit is set,
 * else 0) in chunk_stats [3][chunks][N] -- what spml_bn_bwd_hl8_chunks_f32 / spml_bn_act_bwd_reduce_ext_chunks_f32
 * pool instead of a pass over `out` and bn_x -- and resets *zero_me (that call's dx_bound; may be NULL).  `out` is
 * bit-identical to spml_conv_hl8_f32's.  The layout call follows spml_conv_hl8_stats_layout's rules. */
int spml_conv_hl8_bwd_stats_layout(int n_img, int H, int W, int K, int N, int taps,
                                   int* chunks, int* chunk_rows);
int spml_conv_hl8_bwd_stats_f32(const void* a, const float* a_bound, const void* b,
                                const float* b_bound, float* out, const float* bn_x,
                                const unsigned char* relu_mask, const float* bn_mean,
                                float* chunk_stats, float* zero_me, int n_img, int H, int W,
                                int K, int N, int taps, int dilation, void* stream);
/* ... whose output also takes an addend, as spml_conv_hl8_f32 applies it (out = conv + addend where addend_mask is
 * NULL or its bit is set; `out` bit-identical to that call's): the last data gradient of a bottleneck unit, whose
 * output is the dy of the bn3 + ReLU of the unit below (bn_x, relu_mask, bn_mean: that batch norm's).  Same layout
 * call, same route as spml_conv_hl8_bwd_stats_f32; launches with the chunked accumulation are not supported. */
int spml_conv_hl8_bwd_stats_addend_f32(const void* a, const float* a_bound, const void* b,
                                       const float* b_bound, float* out, const float* bn_x,
                                       const unsigned char* relu_mask, const float* bn_mean,
                                       float* chunk_stats, float* zero_me, int n_img, int H, int W,
                                       int K, int N, int taps, int dilation, const float* addend,
                                       const unsigned char* addend_mask, void* stream);

/* Weight gradient of the same convolutions:
 *   dw[n][tap][k] = sum_r dy[r][n] * x[r + shift(tap)][k]      (dw fp32 [N][taps][K] = the
 * channels-last storage of the weight gradient).  dy: hl8 [R][N], x: hl8 [R][K] (the forward
 * input).  K % 128 == 0 and N % 128 == 0 (256-wide output tiles where the channel count allows it,
 * 128-wide ones otherwise).  The pixel range is split over workgroups; the
 * partial tiles live in the caller's workspace and are summed in a fixed order. */
int spml_conv_wgrad_hl8_supported(int K, int N, int taps);
size_t spml_conv_wgrad_workspace_bytes(int n_img, int H, int W, int K, int N, int taps);
int spml_conv_wgrad_hl8_f32(const void* dy, const float* dy_bound, const void* x,
                            const float* x_bound, float* dw, int n_img, int H, int W,
                            int K, int N, int taps, int dilation, void* ws,
                            size_t ws_bytes, void* stream);

/* Weight gradients of the pyramid head's narrow branches (spml/models/heads/spp.py:8-43: up to four
 * dilated 3x3 convolutions of ONE input whose outputs are summed -- they share dy): N == 64,
 * K % 256 == 0, 1..4 branches with dilations[b] in 1..255 (host array).
 *   dw[b][n][tap][k] = sum_r dy[r][n] * x[r + shift_b(tap)][k]
 * dw fp32 [branches][64][9][K] = the channels-last storage of each branch's [64, K, 3, 3] weight
 * gradient, one branch after the other.  x is streamed once per FOUR taps (a 256-column tile is
 * four taps x 64 channels), not once per tap.  Workspace as above. */
int spml_conv_wgrad_pyramid_hl8_supported(int K, int N, int branches);
/* Forward of the same narrow branches as ONE 1x1 convolution + a gather: with
 *   z[r][tap * N + n] = x[r] . w_tap[n]        (spml_conv_hl8_f32 with 9 * branches * N columns,
 *                                                tap = 9 * branch + 3 * kh + kw)
 * the head's output is  out[p][n] = bias[n] + sum_tap z[p + shift(tap)][tap * N + n]  (taps whose
 * shifted pixel leaves the image contribute 0), which this call gathers (taps added in order:
 * deterministic).  z fp32 [R][9 * branches * N], out fp32 [R][N]; N a power of two in 16..1024,
 * bias [N] or NULL, dilations[b] in 1..255 (host array). */
int spml_conv_tap_gather_f32(const float* z, const float* bias, float* out, int n_img, int H,
                             int W, int N, int branches, const int* dilations, void* stream);
size_t spml_conv_wgrad_pyramid_workspace_bytes(int n_img, int H, int W, int K, int N,
                                               int branches);
int spml_conv_wgrad_pyramid_hl8_f32(const void* dy, const float* dy_bound, const void* x,
                                    const float* x_bound, float* dw, int n_img, int H, int W,
                                    int K, int N, int branches, const int* dilations,
                                    void* ws, size_t ws_bytes, void* stream);

/* Which conv_gemm instantiation a call launches (pure host functions: the launches' own expression -- the entry points,
 * the statistics layouts and these names read one route record, csrc/conv.hip: conv_route; every SPML_CONV_* switch
 * is read per call).  entry: 0 spml_conv_hl8_f32, 1 spml_conv_hl8_stats_f32, 2 spml_conv_hl8_bwd_stats_f32,
 * 3 spml_conv_hl8_affine_f32, 4 spml_conv_hl8_pyramid_f32 (taps_or_groups: its `groups`; otherwise taps).
 * Names (static strings), N % 256 == 0: "rb3" "rb4" "rb5" = 96- / 128- / 160-row tiles of 256 columns (by problem
 * size, or SPML_CONV_RB); "rb3_chunk" = 96 rows, chunked accumulation (K * taps >= SPML_CONV_CHUNK_MIN_K, default
 * 4096); "rb5_rg2" = 320 rows, two row groups (SPML_CONV_RG=2; never for entry 3).  N % 128 == 0: "n128" (256 rows)
 * "n128_chunk" (192 rows); N % 64 == 0: "n64" "n64_chunk" (256 rows), with SPML_CONV_NARROW_RB=3 "n64_rb3"
 * "n64_rb3_chunk" (384 rows).  Entries 1 / 2 append the statistics epilogue: "rb3+stats" "rb4+stats" "rb5+stats"
 * "rb3_chunk+stats" / "rb3+bstats" "rb4+bstats" "rb5+bstats" "rb3_chunk+bstats" (every other shape: "unsupported",
 * as the layout calls answer).  Entry 4 with groups > 1, no addend and the deterministic mode off splits the taps
 * over workgroups (fp32 atomics): "n128+tapgroups" "n128_chunk+tapgroups" "n64+tapgroups" "n64_chunk+tapgroups"
 * "n64_rb3+tapgroups" "n64_rb3_chunk+tapgroups".  Outside the domain: "unsupported". */
const char* spml_conv_hl8_path_name(int entry, int n_img, int H, int W, int K, int N,
                                    int taps_or_groups, int has_addend);
/* The same for the weight gradient (csrc/conv.hip: wgrad_route; pyramid != 0: spml_conv_wgrad_pyramid_hl8_f32 with
 * taps_or_branches = branches).  Names: "t256x256_pair4" (N x K tile of one tap, four ring slots, a barrier per two
 * stages: the default at N % 256 == 0 and K % 256 == 0); "t256x256_s2" "t256x256_s3" "t256x256_s4" "t256x256_s5"
 * (SPML_WGRAD_STAGES); "t256x128_s3" "t128x256_s3" "t128x128_s3"; "pyr_t256x256_pair4"; "unsupported".
 * spml_conv_wgrad_splits: workgroups per tile over the pixel range (0: unsupported); the workspace holds
 * splits * tiles * tile n * tile k floats. */
const char* spml_conv_wgrad_path_name(int n_img, int H, int W, int K, int N,
                                      int taps_or_branches, int pyramid);
int spml_conv_wgrad_splits(int n_img, int H, int W, int K, int N, int taps_or_branches,
                           int pyramid);

/* ---- batch norm producing the split-f16 ("hl8") copies the matrix-core convolutions read ----
 * Same math as the spml_bn_* calls above (spml/models/backbones/resnet.py:42-63); y / dx can be
 * written as fp32, as hl8, or both.  The tensor bounds that fix the hl8 scales come from
 * per-channel extremes gathered in the statistics / reduction pass (no extra pass over the
 * data).  C % 8 == 0.  Cross-rank statistics are combined by the caller between the halves. */
int spml_bn_stats_ext_f32(const float* x, int64_t R, int C, float* mean, float* m2,
                          float* cmax, float* cmin, void* ws, size_t ws_bytes,
                          void* stream);

/* spml_bn_stats_ext_f32 pooled from the chunk statistics of the producing convolution
 * (spml_conv_hl8_stats_f32: chunk_stats [4][chunks][C]) instead of a pass over x -- the local
 * half of SyncBatchNorm for the matrix-core units. */
int spml_bn_stats_ext_chunks_f32(const float* chunk_stats, int chunks, int chunk_rows,
                                 int64_t R, int C, float* mean, float* m2, float* cmax,
                                 float* cmin, void* stream);

/* invstd = rsqrt(m2/count + eps); running statistics updated in place (may be NULL). */
int spml_bn_finalize_f32(const float* mean, const float* m2, int C, double count,
                         float eps, float momentum, float* running_mean,
                         float* running_var, float* invstd, void* stream);

/* y (fp32, may be NULL) and/or y_hl8 = act((x-mean)*invstd*gamma + beta [+ residual]);
 * *y_bound (required with y_hl8, optional otherwise) receives max_c |bn(x)_c| (+ *residual_bound);
 * relu_mask (may be NULL): one byte per (row, channel quad), bit e = (y[row][4q+e] > 0) -- what
 * the backward calls read instead of y. */
int spml_bn_act_apply_hl8_f32(const float* x, const float* residual,
                              const float* residual_bound, int64_t R, int C,
                              const float* mean, const float* invstd,
                              const float* gamma, const float* beta,
                              const float* cmax, const float* cmin, int relu,
                              float* y, void* y_hl8, float* y_bound,
                              unsigned char* relu_mask, void* stream);

/* ReLU mask from y (fp32) or from relu_mask (or none); also max |dz| per channel. */
int spml_bn_act_bwd_reduce_ext_f32(const float* dy, const float* y,
                                   const unsigned char* relu_mask,
                                   const float* x, int64_t R, int C, const float* mean,
                                   const float* invstd, float* sum_dz,
                                   float* sum_dz_xhat, float* max_dz, void* ws,
                                   size_t ws_bytes, void* stream);

int spml_bn_act_bwd_apply_hl8_f32(const float* dy, const float* y,
                                  const unsigned char* relu_mask,
                                  const float* x, int64_t R, int C, const float* mean,
                                  const float* invstd, const float* gamma,
                                  const float* sum_dz, const float* sum_dz_xhat,
                                  const float* max_dz, const float* cmax,
                                  const float* cmin, double count,
                                  const float* count_dev, float* dx, void* dx_hl8,
                                  float* dx_bound, float* d_residual, void* stream);

/* Single-rank forms (no cross-rank statistics): the whole forward / backward of one batch norm
 * in one call each, three launches.  mean / invstd / cmax / cmin are outputs of the forward and
 * inputs of the backward; d_gamma / d_beta are the parameter gradients. */
int spml_bn_fwd_hl8_f32(const float* x, const float* residual, const float* residual_bound,
                        int64_t R, int C, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps,
                        int relu, float* y, void* y_hl8, float* y_bound,
                        unsigned char* relu_mask, float* mean, float* invstd, float* cmax,
                        float* cmin, void* ws, size_t ws_bytes, void* stream);

/* spml_bn_fwd_hl8_f32 from chunk statistics left by the producer of x (spml_conv_hl8_stats_f32):
 * chunk_stats [4][chunks][C] = mean, M2, max, min per chunk of chunk_rows rows (the last chunk
 * shorter); *y_bound must have been reset by the producer.  Two launches, x is read once. */
int spml_bn_fwd_hl8_chunks_f32(const float* x, const float* chunk_stats, int chunks,
                               int chunk_rows, const float* residual,
                               const float* residual_bound, int64_t R, int C,
                               const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, int relu,
                               float* y, void* y_hl8, float* y_bound,
                               unsigned char* relu_mask, float* mean, float* invstd,
                               float* cmax, float* cmin, void* stream);

int spml_bn_bwd_hl8_f32(const float* dy, const float* y, const unsigned char* relu_mask,
                        const float* x, int64_t R, int C, const float* mean,
                        const float* invstd, const float* gamma, const float* cmax,
                        const float* cmin, float* d_gamma, float* d_beta, float* dx,
                        void* dx_hl8, float* dx_bound, float* d_residual, void* ws,
                        size_t ws_bytes, void* stream);

/* spml_bn_bwd_hl8_f32 from the chunk sums left by the producer of dy (spml_conv_hl8_bwd_stats_f32):
 * chunk_stats [3][chunks][C] = sum dz, sum dz * (x - mean), max |dz| per chunk of chunk_rows rows (the last
 * chunk shorter); *dx_bound must have been reset by the producer; max_dz [C] receives the channel maxima.
 * Two launches, dy / x / relu_mask are read once.  Same results as spml_bn_bwd_hl8_f32 up to the fp32
 * summation order of the two sums (fixed: deterministic). */
int spml_bn_bwd_hl8_chunks_f32(const float* dy, const unsigned char* relu_mask, const float* x,
                               const float* chunk_stats, int chunks, int chunk_rows, int64_t R,
                               int C, const float* mean, const float* invstd, const float* gamma,
                               const float* cmax, const float* cmin, float* d_gamma,
                               float* d_beta, float* max_dz, float* dx, void* dx_hl8,
                               float* dx_bound, float* d_residual, void* stream);

/* spml_bn_act_bwd_reduce_ext_f32 from the same chunk sums (the local half of SyncBatchNorm's backward). */
int spml_bn_act_bwd_reduce_ext_chunks_f32(const float* chunk_stats, int chunks, int chunk_rows,
                                          int64_t R, int C, const float* invstd, float* sum_dz,
                                          float* sum_dz_xhat, float* max_dz, void* stream);

/* Sum of up to four 3x3 convolutions with different dilations over the same input in one launch
 * (the data gradient of the DeepLab-v2 ASPP head, spml/models/heads/spp.py:8-43: four dilated
 * branches whose outputs are summed, so all four see the same output gradient):
 *   out[r][n] = sum_g sum_{tap,k} a[r + shift_g(tap)][k] * b[n][(9 g + tap) * K + k]  (+ bias[n]) (+ addend)
 * -- with the forward weights concatenated along the taps it is also the head's forward pass.
 * b: hl8 [N][9 * groups * K]; spml_hl8_weight_transposed_into_f32 writes one branch's mirrored,
 * transposed weight into its tap range of that operand; spml_absmax_bound_f32 accumulates the
 * shared bound (max over calls unless zero_first). */
int spml_conv_hl8_pyramid_f32(const void* a, const float* a_bound, const void* b,
                              const float* b_bound, const float* bias, const float* addend,
                              float* out,
                              int n_img, int H, int W, int K, int N, int groups,
                              const int* dilations, void* stream);
int spml_hl8_weight_transposed_into_f32(const float* w, int Cout, int taps, int Cin,
                                        const float* bound, void* out, int taps_total,
                                        int tap_offset, void* stream);
int spml_absmax_bound_f32(const float* x, int64_t n, float* bound, int zero_first,
                          void* stream);

/* All conv weights of one bottleneck unit (n <= 4) in two launches: bounds[i] = max|w_i|, then
 * fwd[i] = hl8 [Cout][taps*Cin] and transposed[i] = hl8 [Cin][taps*Cout] (mirrored taps) of every
 * weight.  The pointer / size arrays are host arrays; bounds is a device array of 4 floats. */
int spml_hl8_weight_set_f32(const float* const* w, const int* cout, const int* cin,
                            const int* taps, int n, float* bounds, void* const* fwd,
                            void* const* transposed, void* stream);

/* SyncBatchNorm: stats [world][3][C] = the ranks' (count, mean, M2) as gathered by the caller ->
 * pooled mean, invstd = rsqrt(M2/count + eps), running statistics updated in place (may be NULL);
 * total_count [1] (may be NULL) receives the pooled row count = sum of the ranks' counts, the
 * `count_dev` of the backward apply calls. */
int spml_bn_finalize_ranks_f32(const float* stats, int world, int C, float eps,
                               float momentum, float* running_mean, float* running_var,
                               float* mean, float* invstd, float* total_count, void* stream);

/* Inference form of the same convolution (batch norm folded into weights and bias by the caller,
 * spml/models/backbones/resnet.py:42-63 in eval mode):
 *   out = act(conv(a, b) + bias[n] [+ addend]),   *out_bound = max |out|   (both optional)
 * so that the next convolution's hl8 input is one conversion pass away (spml_hl8_from_f32 with the
 * bound given). */
int spml_conv_hl8_affine_f32(const void* a, const float* a_bound, const void* b,
                             const float* b_bound, const float* bias, const float* addend,
                             int relu, float* out, float* out_bound, int n_img, int H,
                             int W, int K, int N, int taps, int dilation, void* stream);

/* ---- softmax head: cross-entropy of bilinearly up-sampled logits -------------------------
 * Replaces `F.interpolate(logits, size=labels.shape[-2:], mode='bilinear')` followed by
 * `CrossEntropyLoss(ignore_index)` in spml/models/predictions/segsort_softmax.py:112-131 (the
 * classifier head trained beside the contrastive terms) without materialising the [N, C, H, W]
 * logits.  logits: fp32 [N][h][w][C] (channels-last storage of the [N, C, h, w] map), C <= 64;
 * labels: int64 [N][H][W], every value in [0, C) or == ignore_index.
 *   fwd: lse [N][H][W] = logsumexp of each pixel's interpolated logits (kept for the backward pass),
 *        result[0] = sum of the pixel losses, result[1] = number of counted pixels,
 *        result[2] = their mean (NaN without counted pixels, like the framework loss);
 *   bwd: d_logits [N][h][w][C] = scale[0] * d(sum of the pixel losses) / d logits, scale a device
 *        scalar (d_loss / result[1] for the mean).  Gather formulation: deterministic, no atomics.
 *        Two kernels, chosen by shape (spml_upsample_ce_bwd_path_name, a pure host function with the launch's own
 *        expression): "tiled" -- a workgroup per 8 x 8 low-resolution pixels with the softmax rows of the output
 *        rectangle it feeds in LDS -- while that layout needs at most 72 KiB and N <= 65535; "gather" -- one thread
 *        per low-resolution pixel, no LDS -- otherwise (up-sampling ratios above ~4.4 at 21 classes, ~3.8 at 64);
 *        "unsupported" for arguments the backward refuses.
 * Interpolation arithmetic as ATen's upsample_bilinear2d (align_corners = False). */
int spml_upsample_ce_supported(int C);
size_t spml_upsample_ce_workspace_bytes(int N, int H, int W);
int spml_upsample_ce_fwd_f32(const float* logits, const int64_t* labels, int N, int C, int h,
                             int w, int H, int W, int64_t ignore_index, float* lse,
                             float* result, void* ws, size_t ws_bytes, void* stream);
int spml_upsample_ce_bwd_f32(const float* logits, const int64_t* labels, const float* lse,
                             int N, int C, int h, int w, int H, int W, int64_t ignore_index,
                             const float* scale, float* d_logits, void* stream);
const char* spml_upsample_ce_bwd_path_name(int N, int C, int h, int w, int H, int W);

/* ---- full-resolution softmax inference: classifier head on a sliding-window crop, label map, IoU counts ----
 * Replaces, per crop, pyscripts/inference/inference_softmax.py:126-137 with
 * spml/models/predictions/softmax_classifier.py:52-55 in eval mode (x / |x|, 3x3 convolution C -> 2C, batch norm,
 * ReLU, dropout = identity, 1x1 convolution 2C -> num_classes, `outputs[..., sh:eh, sw:ew] += crop_out`: the logits
 * of overlapping windows are SUMMED, there are no counts), then :140-148 (arg-max, crop to the un-padded size) and
 * pyscripts/benchmark/benchmark_by_mIoU.py:25-53 (iou_stats).  The 3x3 convolution + batch norm + ReLU between the
 * first two calls is spml_conv_hl8_affine_f32 with the batch norm folded into weight and bias by the caller. */

/* x fp32 [n][C][h][w] (NCHW) -> hl8 [n*h*w][C] of x / |x|_2 over the channels (softmax_classifier.py:52-54), one
 * pass.  The scale of the split is the one of a bound of 1.0f (S = 2^13): pass a device float 1.0f as `a_bound` of
 * the convolution.  C % 16 == 0, C <= 512.  The reference divides without an epsilon, so a zero-norm pixel is NaN
 * there; here it is outside the contract and written as a row of zeros (non-finite inputs give non-finite halves;
 * nothing faults). */
int spml_unit_hl8_from_nchw_f32(const float* x, int n, int C, int h, int w, void* out,
                                void* stream);

/* 1 when spml_class_head_accumulate_f32 takes (Ch hidden channels, ncls classes): Ch % 32 == 0, ncls <= 64 and the
 * weights plus one pixel tile fit the LDS. */
int spml_class_head_supported(int Ch, int ncls);

/* canvas[c][sh + y][sw + x] += sum_k hidden[y*w + x][k] * weight[c][k] + bias[c]   (softmax_classifier.py:26-30,55
 * and inference_softmax.py:137), in place.  hidden fp32 [h*w][Ch] (channels-last: `out` of the affine convolution of
 * ONE crop), weight [ncls][Ch], bias [ncls], canvas fp32 [ncls][Hp][Wp] (`semantic_logit`, N = 1).  fp32-input
 * matrix cores: exact fp32 products, fp32 accumulation.  Plain loads and stores on the canvas: the windows of one
 * image overlap, so their launches must be ordered (one stream). */
int spml_class_head_accumulate_f32(const float* hidden, int Ch, int h, int w,
                                   const float* weight, const float* bias, int ncls,
                                   float* canvas, int Hp, int Wp, int sh, int sw,
                                   void* stream);

/* out int64 [h][w] = arg-max over the classes of the top-left h x w region of canvas [ncls][Hp][Wp]
 * (inference_softmax.py:142-148).  Ties: the lowest class index; NaN (outside the contract) counts as the
 * largest value and the first one wins -- both as torch.argmax. */
int spml_argmax_channels_i64(const float* canvas, int ncls, int Hp, int Wp, int h, int w,
                             int64_t* out, void* stream);

/* counts int64 [3][ncls] += (TP+FN, TP+FP, TP) of pred / target (int64 [n]) over the pixels with
 * 0 <= target < ncls (benchmark_by_mIoU.py:25-53); accumulated INTO counts, so a caller loops over images and zeroes
 * it once.  TP+FP bins pred at those pixels: a prediction outside [0, ncls) falls into no bin (numpy's histogram
 * closes its last bin on the right, so the reference counts pred == ncls as class ncls - 1; an arg-max over ncls
 * planes never gives that value).  Integer atomics: bit-reproducible in either mode.  ncls <= 4096. */
int spml_iou_counts_i64(const int64_t* pred, const int64_t* target, int64_t n, int ncls,
                        int64_t* counts, void* stream);

/* ------------------------------------------------------------------------
 * N7  pseudo-label generation from the softmax head (csrc/pseudo_label.hip)
 * replaces: pyscripts/inference/pseudo_softmaxrw_crf.py:130-136, 141-157, 173-176 and pseudo_softmax.py:129-135,
 *           140-160, 176-179 -- everything of the two scripts around the affinity (spml_affinity_transition_f32 above)
 *           and the walk's GEMMs.  No entry point below uses floating-point atomics: results are bit-reproducible and
 *           the same with and without the deterministic mode.
 * Resampling is bilinear with half-pixel centres (`F.interpolate(mode='bilinear')`, align_corners = False, no
 * anti-aliasing) as ATen computes it: scale = in / out in fp32, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = floor(src),
 * i1 = min(i0 + 1, in - 1), lambda = src - i0.  A view's source is the top-left rh x rw region of a padded Hp x Wp
 * plane (in = rh, rw); with `flip` the source column of x is rw - 1 - x (the reference crops, flips back, then
 * interpolates).  Tensors of the network are read through element strides (stride_c, stride_y, stride_x > 0), so NCHW
 * and channels-last storage are both read as they are, with the same result bit for bit.
 * ------------------------------------------------------------------------ */
#define SPML_COMBINE_PROB_MEAN 0   /* softmax per view, mean of the probabilities (pseudo_softmaxrw_crf.py:143-147) */
#define SPML_COMBINE_LOGIT_MEAN 1  /* mean of the logits, then one softmax (pseudo_softmax.py:144-150) */

/* out[b][c][p] = r[c][p] / |r[:, p]|_2, r = view `emb` [C][Hp][Wp] cropped, un-flipped and resampled to oh x ow
 * (pseudo_softmaxrw_crf.py:130-136; plain division, no epsilon).  out: fp32 [B][C][oh*ow], the layout
 * spml_affinity_transition_f32 reads; this call writes slice b.  C <= 256. */
int spml_resample_unit_f32(const float* emb, int C, int Hp, int Wp, int64_t stride_c, int64_t stride_y,
                           int64_t stride_x, int rh, int rw, int flip, int oh, int ow, float* out, int B, int b,
                           void* stream);

/* acc[c][p] += softmax over c of r[c][p] (SPML_COMBINE_PROB_MEAN, pseudo_softmaxrw_crf.py:131-144) or r[c][p] itself
 * (SPML_COMBINE_LOGIT_MEAN, pseudo_softmax.py:130-144), r = view `logit` [ncls][Hp][Wp] cropped, un-flipped and
 * resampled.  acc: fp32 [ncls][oh*ow], zeroed by the caller before the first view; plain loads and stores, so the
 * views of one image are added in call order on one stream (a pixel's fp32 sum has the reference's order).
 * ncls <= 256. */
int spml_resample_classes_accumulate_f32(const float* logit, int ncls, int Hp, int Wp, int64_t stride_c,
                                         int64_t stride_y, int64_t stride_x, int rh, int rw, int flip, int oh,
                                         int ow, int combine, float* acc, void* stream);

/* cam [ncls][n] from the sum `acc` [ncls][n] of B views: acc / B; with SPML_COMBINE_LOGIT_MEAN the softmax over the
 * classes (pseudo_softmax.py:149-150); every class divided by its maximum over the n pixels; classes with tags[c] == 0
 * set to 0; class 0 set to `threshold` where has_threshold != 0 (pseudo_softmaxrw_crf.py:146-157; the reference's
 * TH = None is has_threshold = 0).  tags: one byte per class.  One launch (prob_mean) or two (logit_mean).  cam may not
 * alias acc.  ncls <= 256. */
int spml_cam_finalize_f32(const float* acc, int ncls, int64_t n, int B, int combine, const unsigned char* tags,
                          int has_threshold, float threshold, float* cam, void* stream);

/* out int64 [h][w] = arg-max over the classes of cam [ncls][oh][ow] resampled to h x w, in one kernel: the
 * ncls x h x w tensor of pseudo_softmaxrw_crf.py:173-176 (`cv2.resize(..., INTER_LINEAR)` + `np.argmax`, the same
 * half-pixel mapping) is never written.  Ties: the lowest class; NaN as torch.argmax (the rules of
 * spml_argmax_channels_i64). */
int spml_upsample_argmax_i64(const float* cam, int ncls, int oh, int ow, int h, int w, int64_t* out, void* stream);

/* ------------------------------------------------------------------------
 * N8  multi-scale + flip softmax inference: the per-view tail (csrc/msc_inference.hip)
 * replaces: pyscripts/inference/inference_softmax_msc.py:135-143 per view and the sum of :146-147 (divide the summed
 *           window logits by the overlap counts, crop, `F.interpolate(mode='bilinear')` to the image, softmax over the
 *           classes, flip back through host numpy, concatenate and sum: six passes over an ncls x H x W tensor).
 * ------------------------------------------------------------------------ */

/* acc[c][y][x] += softmax over c of r[c][y][xd], xd = flip ? w - 1 - x : x, where r is `canvas / counts` cropped to its
 * top-left rh x rw region and resampled bilinearly to h x w (the rule above spml_resample_unit_f32, in = rh, rw -- never
 * Hp, Wp: values outside the region are not read).  Unlike the N7 entries the view is interpolated as it is and the RESULT
 * is flipped (:141-142), which differs from flipping the source in the last bit.
 * canvas: fp32 [ncls][Hp][Wp], the window logits of ONE view, summed (spml_class_head_accumulate_f32).  cnt_y [Hp],
 * cnt_x [Wp]: the numbers of windows that cover a row / a column; the reference's counts[y][x] (:134) is
 * cnt_y[y] * cnt_x[x] exactly, the windows being a Cartesian product.  Each of the four taps is divided by its own count
 * product (a true fp32 division, before the interpolation, as :135), then combined as
 * h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11); softmax = subtract the maximum, exp, sum, divide.
 * acc: fp32 [ncls][h][w], zeroed by the caller before the first view; plain loads and stores, so the views of one image
 * are added in call order on one stream (a pixel's fp32 sum has the order of :147).  No atomics, no workspace: results
 * are bit-reproducible and the same with and without the deterministic mode.  acc may not alias canvas
 * (SPML_ERR_INVALID_ARG, as for rh > Hp, rw > Wp or a size below 1); ncls <= 64, else SPML_ERR_UNSUPPORTED. */
int spml_view_probs_accumulate_f32(const float* canvas, int ncls, int Hp, int Wp, const float* cnt_y,
                                   const float* cnt_x, int rh, int rw, int flip, int h, int w, float* acc,
                                   void* stream);

/* ------------------------------------------------------------------------
 * N9  multi-scale + flip kNN inference: the per-view tail (csrc/knn_msc.hip)
 * replaces: pyscripts/inference/inference_msc.py:223-234 per view and the sum of :237-239 (one-hot of the retrieved
 *           labels `topk[clu]` [rh * rw, k] over the classes, mean over k, host copy, `cv2.resize(..., INTER_LINEAR)` to
 *           the image, un-flip, stack + mean over the views -- here without the final division by the view count).
 *
 *   acc[c][y][x] += bilinear_{(rh, rw) -> (h, w)}( votes[clu[.]][c] )  evaluated at xd = flip ? w - 1 - x : x, stored at x
 *   votes[s][c]   = #{ j < k : topk[s][j] == c } / k
 *
 * clu: int64 [rh][rw] (contiguous), the dense segment id of every pixel of the view, 0 <= id < m (an id outside that
 * range is outside the contract and is clamped into it: nothing is read out of bounds).  topk: int64 [m][k], the labels
 * retrieved per SEGMENT (Segsort.segment_predictions); a label outside [0, ncls) adds to no class, so that row of votes
 * sums to less than 1 (the reference's one_hot would fail on it).  The count is an exact small integer, divided once by
 * (float)k: what `one_hot(...).float().mean(1)` gives.  Bilinear taps as ATen forms them (align_corners = False, the
 * half-pixel mapping of cv2's INTER_LINEAR) with in = rh / rw, combined as
 * h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
 * acc: fp32 [ncls][h][w], zeroed by the caller before the first view; plain loads and stores, so the views of one image
 * are added in call order on one stream (a pixel's fp32 sum has the order of :237-239).  ws: 16-byte aligned, at least
 * spml_view_votes_workspace_bytes(m, ncls) bytes (the votes table; that call returns 0 outside the limits), else
 * SPML_ERR_WORKSPACE.  No atomics: results are bit-reproducible and the same with and without the deterministic mode.
 * acc may alias neither clu, topk nor ws, and ws neither input (SPML_ERR_INVALID_ARG, as for a null pointer or a size
 * below 1); ncls <= 64 and m <= 4096, else SPML_ERR_UNSUPPORTED. */
size_t spml_view_votes_workspace_bytes(int m, int ncls);
int spml_view_votes_accumulate_f32(const int64_t* clu, int rh, int rw, const int64_t* topk, int m, int k, int ncls,
                                   int flip, int h, int w, float* acc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * N10  memory-bank generation: the majority label per segment (csrc/segment_majority.hip)
 * replaces: the labels of spml/utils/segsort/common.py:221-267 as pyscripts/inference/prototype.py:200-203 and
 *           prototype_msc.py:189-192 call it (a [P, ncls] int64 one-hot scatter-added by the segment id, arg-max per row).
 *
 *   count[s][c] = #{ p < P : clu[p] = s, sem[p] = c }          major[s] = argmax_c count[s][c]
 *
 * clu, sem: int64 [P], the dense segment id and the class of every pixel.  A pixel whose id is outside [0, m) or whose
 * class is outside [0, ncls) counts nowhere and forms no address.  Ties go to the lowest class (torch.argmax's rule on the
 * CPU); a row without a counted pixel gives 0.  major: int64 [m].  hist: int64 [m][ncls], the counts, or NULL.
 * ws: 4-byte aligned, at least spml_segment_majority_workspace_bytes(m, ncls) bytes (that call returns 0 outside the
 * limits), else SPML_ERR_WORKSPACE; the call zeroes it on `stream` itself, its previous content does not matter.
 * Counts meet through 32-bit integer atomics only (P < 2^31 bounds every bin): the result does not depend on the arrival
 * order and is bit-identical from run to run, with and without the deterministic mode.  No host read, three stream
 * operations (memset, count, arg-max).  ws, major and hist may alias neither an input nor each other
 * (SPML_ERR_INVALID_ARG, as for a null pointer, P < 0, m < 1 or ncls < 1); m <= 4096, ncls <= 256 and P < 2^31, else
 * SPML_ERR_UNSUPPORTED.  spml_segment_majority_path_name: which count kernel a shape takes -- "lds_table" (m * ncls <=
 * 8192: a per-workgroup LDS table flushed once) or "global_table" (global atomics), "unsupported" outside the limits,
 * "invalid" for a size below the domain.  In both kernels equal keys are merged inside a wave before the atomic; a
 * library built with SPML_MAJORITY_WAVE_COMBINE=0 (one atomic per counted pixel: the other side of the A/B of
 * tools/bench_prototype_msc.py) appends "_per_pixel_atomics". */
size_t spml_segment_majority_workspace_bytes(int m, int ncls);
int spml_segment_majority_i64(const int64_t* clu, const int64_t* sem, int64_t P, int m, int ncls, int64_t* major,
                              int64_t* hist, void* ws, size_t ws_bytes, void* stream);
const char* spml_segment_majority_path_name(int64_t P, int m, int ncls);

/* ------------------------------------------------------------------------
 * N11  tag-recipe kNN pseudo labels: tag-normalised arg-max (csrc/tag_normalize.hip)
 * replaces: pyscripts/inference/pseudo_inference_crf_msc.py:252-263,275 (mean of the stacked vote maps over the views,
 *           the maximum of every class over the image, a floor of 0.15, 1 for the classes the image does not carry, the
 *           division, and -- the denseCRF of :273 left out -- the arg-max over the classes).
 *
 *   mean[c][p] = acc[c][p] / (float)num_views          peak[c] = max_p mean[c][p]
 *   div[c]     = tags[c] ? max(peak[c], floor) : 1     prob[c][p] = mean[c][p] / div[c]
 *   labels[p]  = the lowest c that attains max_c prob[c][p]
 *
 * acc: fp32 [ncls][n], the SUM over the views as spml_view_votes_accumulate_f32 leaves it (n = h * w), finite values of
 * either sign; it is only read.  tags: one byte per class, non-zero = the image carries the class.  floor: a positive
 * finite number (the reference's 0.15 as fp32).  labels: int64 [n].  prob: fp32 [ncls][n] or NULL (not written).  divisor:
 * fp32 [ncls] (div) or NULL.  Both divisions are correctly rounded fp32 divisions and the maximum is exact: divisor and
 * prob carry the bits of the same chain in numpy or in ATen on the CPU (peak is formed as (max_p acc[c][p]) / num_views:
 * fp32 division is monotone).  ws: 4-byte aligned, at least spml_tag_normalize_workspace_bytes(ncls, n) bytes (that call
 * returns 0 outside the limits), else SPML_ERR_WORKSPACE; its previous content does not matter.  Two launches on
 * `stream` (the maxima of up to 16 parts per class plane; then normalise + arg-max, which finishes the parts in its
 * prologue), no host read, no atomics: results are bit-identical from call to call, with and without the deterministic
 * mode.  labels, prob, divisor and ws may alias neither acc, tags nor each other (SPML_ERR_INVALID_ARG, as for a null
 * acc / tags / labels, n < 1, ncls < 1, num_views < 1 or a floor that is not a positive finite number); ncls <= 64 and
 * n <= 2^30, else SPML_ERR_UNSUPPORTED. */
size_t spml_tag_normalize_workspace_bytes(int ncls, int64_t n);
int spml_tag_normalize_argmax_f32(const float* acc, int ncls, int64_t n, int num_views, const unsigned char* tags,
                                  float floor, int64_t* labels, float* prob, float* divisor, void* ws, size_t ws_bytes,
                                  void* stream);

/* ------------------------------------------------------------------------
 * N12  dense CRF refinement: exact mean-field inference over all pixel pairs (csrc/dense_crf.hip)
 * replaces: spml/models/crf.py:23-41 (unary_from_softmax, DenseCRF2D, addPairwiseGaussian, addPairwiseBilateral,
 *           inference(iter_max)) -- restated from the model, not ported: the reference approximates the two filters
 *           with a permutohedral lattice, this is the filter itself.
 *
 *   U = -log(clip(probmap, 1e-5, 1))                       Q_0 = softmax_c(-U)
 *   K1[i,j] = exp(-|p_i-p_j|^2 / (2 pos_xy_std^2))         K2[i,j] = exp(-|p_i-p_j|^2 / (2 bi_xy_std^2)
 *                                                                        - |I_i-I_j|^2 / (2 bi_rgb_std^2))
 *   n_m = 1 / sqrt(K_m 1 + 1e-20)                          M_m(Q)[c,i] = n_m[i] sum_j K_m[i,j] n_m[j] Q[c,j]
 *   Q <- softmax_c(-U + pos_w M_1(Q) + bi_w M_2(Q))        iter_max times (i = j included; Potts compatibility)
 *
 * One image per call; h, w <= 2048 and ncls <= 64, else SPML_ERR_UNSUPPORTED (spml_dense_crf_workspace_bytes returns 0
 * and spml_dense_crf_path_name "unsupported").  ws: 256-byte aligned, at least spml_dense_crf_workspace_bytes(h, w,
 * ncls) bytes, else SPML_ERR_WORKSPACE; its head is what prepare leaves for infer, the rest is scratch of infer.
 *
 * spml_dense_crf_prepare_u8 (spml/models/crf.py:23-41, the two addPairwise* calls): image uint8 [h][w][3]; the three
 *   standard deviations are positive finite numbers.  Writes the MFMA operands of the pair exponent and both norms n_1,
 *   n_2 into ws (its size does not depend on ncls: one prepared image serves any class count and any weights).
 * spml_dense_crf_infer_f32 (spml/models/crf.py:23-41, unary_from_softmax and inference): probmap fp32 [ncls][h][w], not
 *   necessarily normalised, zeros allowed; iter_max >= 0; q fp32 [ncls][h][w] (the result); labels int64 [h][w] or NULL:
 *   the lowest class that attains the maximum of q at a pixel, from the epilogue that writes q.  ws as prepare left it,
 *   for the same h and w.
 * spml_dense_crf_infer_upsampled_f32 (pyscripts/inference/pseudo_softmaxrw_crf.py:172-185 = pseudo_camrw_crf.py:166-179,
 *   and spml/models/crf.py:23-41): the same inference on probmap = the bilinear up-sampling of lowres fp32
 *   [ncls][oh][ow] to h x w (F.interpolate, align_corners = False: the taps and the scale expressions of
 *   spml_upsample_argmax_i64), formed inside the first launch and not stored.  oh, ow >= 1 (else
 *   SPML_ERR_INVALID_ARG), of any size relative to h x w (the programs pass h/8 x w/8; with oh = h, ow = w the up-sampled
 *   map is lowres itself); oh * ow <= 2^24, else SPML_ERR_UNSUPPORTED.  q, labels, ws and every other check as
 *   spml_dense_crf_infer_f32, whose result on the up-sampled map it equals bit for bit.  labels_before int64 [h][w] or
 *   NULL: the arg-max of the up-sampled values before the clip, equal to spml_upsample_argmax_i64(lowres) on every pixel
 *   (lowest class on ties, the first NaN wins).  prob_up fp32 [ncls][h][w] or NULL: the up-sampled values themselves.
 * spml_dense_crf_infer_votes_f32 (pyscripts/inference/inference_crf.py:237-254, and spml/models/crf.py:23-41; DESIGN.md
 *   8l): the same inference on probmap[c][i] = the share of topk[clu[i]] equal to c -- the vote map of the kNN label
 *   inference (one_hot, sum over k, / k, transpose), which is not formed: clu int64 [h][w], the dense segment id of every
 *   pixel (an id outside [0, m) is clamped into it); topk int64 [m][k], the labels retrieved per segment (a label outside
 *   [0, ncls) adds to no class).  One launch per call computes the votes, log p, Q_0 and both labels per SEGMENT into
 *   table_ws, the first launch of the inference gathers them per pixel.  m, k >= 1 (else SPML_ERR_INVALID_ARG, as for a
 *   null clu or topk or a misaligned pointer); m <= 4096, else SPML_ERR_UNSUPPORTED.  table_ws: 16-byte aligned, at least
 *   spml_dense_crf_votes_workspace_bytes(m, ncls) bytes (0 outside m <= 4096, ncls <= 64), else SPML_ERR_WORKSPACE; it
 *   may overlap no input, no output and not ws (SPML_ERR_INVALID_ARG); its previous content does not matter.  q, labels,
 *   ws and every other check as spml_dense_crf_infer_f32, whose result on the vote map it equals bit for bit.
 *   labels_before int64 [h][w] or NULL: the arg-max of the votes, the lowest class on ties (np.argmax).  prob fp32
 *   [ncls][h][w] or NULL: the vote map itself, with the bits of spml_view_votes_accumulate_f32's table.
 * spml_dense_crf_path_name (spml/models/crf.py:23-41; host only): "pairs_mfma_f16x2_c<32|64>+separable_r<R>" -- the
 *   class columns of the pair kernel and the taps R = ceil(6 pos_xy_std) kept on either side by the separable spatial
 *   filter (the tail it drops is below 4e-9 of the kernel's mass).
 *
 * Launches on `stream` only, no allocation, no host read, no atomics: results are bit-identical from call to call, with
 * and without the deterministic mode.  Numerics are fp32-class: squared feature distances are formed exactly on the
 * matrix cores, K and n Q enter the message product as split-f16 pairs (three MFMAs). */
size_t spml_dense_crf_workspace_bytes(int h, int w, int ncls);
int spml_dense_crf_prepare_u8(const unsigned char* image, int h, int w, float pos_xy_std, float bi_xy_std,
                              float bi_rgb_std, void* ws, size_t ws_bytes, void* stream);
int spml_dense_crf_infer_f32(const float* probmap, int ncls, int h, int w, int iter_max, float pos_w, float bi_w,
                             float* q, int64_t* labels, void* ws, size_t ws_bytes, void* stream);
int spml_dense_crf_infer_upsampled_f32(const float* lowres, int ncls, int oh, int ow, int h, int w, int iter_max,
                                       float pos_w, float bi_w, float* q, int64_t* labels, int64_t* labels_before,
                                       float* prob_up, void* ws, size_t ws_bytes, void* stream);
size_t spml_dense_crf_votes_workspace_bytes(int m, int ncls);
int spml_dense_crf_infer_votes_f32(const int64_t* clu, const int64_t* topk, int m, int k, int ncls, int h, int w,
                                   int iter_max, float pos_w, float bi_w, float* q, int64_t* labels,
                                   int64_t* labels_before, float* prob, void* table_ws, size_t table_ws_bytes, void* ws,
                                   size_t ws_bytes, void* stream);
const char* spml_dense_crf_path_name(int h, int w, int ncls, float pos_xy_std);

/* ------------------------------------------------------------------------
 * DensePose pseudo labels: class maps from propagated segment tags (csrc/segment_cam.hip)
 * replaces: pyscripts/inference/pseudo_denseposerw_crf.py:159-182 (one-hot of the nearest labelled prototype's label
 *           [N, ncls + 1], `segment_mean` by the segment id -- two scatter-adds --, the division of every row by its sum,
 *           `index_select` back to the pixels, transpose, `F.interpolate(mode='bilinear')` to 1/8 of the image).
 *
 *   class(p)     = proto_label[nn_index[p]], none where nn_value[p] < threshold or the label is outside [0, ncls)
 *   counts[s][c] = #{ p < N : cluster_index[p] = s, class(p) = c }            N = h2 * w2
 *   probs[s][c]  = counts[s][c] / sum_c counts[s][c]                          0 for a row without a counted pixel
 *   acc[c][y][x] = bilinear_{(h2, w2) -> (oh, ow)}( probs[cluster_index[.]][c] )
 *
 * nn_index int64 [N], nn_value fp32 [N]: the nearest labelled prototype of every pixel of the h2 x w2 map and its
 * similarity (spml_topk_affinity_f32 with k = 1); proto_label int64 [M]; threshold: a number (the program passes -1; NaN
 * is SPML_ERR_INVALID_ARG; a NaN nn_value is not below it and counts).  cluster_index int64 [h2][w2]: the dense segment
 * id of every pixel, 0 <= id < S.  A pixel whose nn_index is outside [0, M), whose segment id is outside [0, S) or that has
 * no class counts nowhere, and a bilinear tap on a segment id outside [0, S) contributes 0: no kernel forms an address
 * from such a value.  A row without a counted pixel (an empty segment id, a segment without a tagged pixel: the reference
 * has 0 / 0 there) is written as ncls zeros like any other row; nothing outside the table or the maps is read for it.
 * probs is one correctly rounded fp32 division of two exact integers (the reference divides segment_mean's row, itself
 * count / pixels of the segment, by its fp32 sum: the same quotient rounded three times).  Bilinear taps as ATen forms
 * them (align_corners = False; scale = (float)h2 / (float)oh), combined as h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 +
 * w1 * v11); the h2 x w2 map of rows is not formed.
 * acc: fp32 [ncls][oh][ow], overwritten.  counts: int32 [S][ncls] or NULL; probs: fp32 [S][ncls] or NULL (handed out
 * for tests; they do not change acc).  ws: 4-byte aligned, at least spml_segment_tag_cam_workspace_bytes(S, ncls) bytes
 * (that call returns 0 outside the limits), else SPML_ERR_WORKSPACE; the call zeroes what it needs zeroed on `stream`
 * itself.  Counts meet through 32-bit integer atomics only: every output is bit-identical from call to call, with and
 * without the deterministic mode.  No host read, four stream operations (memset, count, probs, gather).  ws, acc, counts
 * and probs may alias neither an input nor each other (SPML_ERR_INVALID_ARG, as for a null pointer or M, S, ncls or a
 * side below 1); S <= 4096, ncls <= 64, N < 2^31 and oh * ow <= 2^24, else SPML_ERR_UNSUPPORTED.
 * spml_segment_tag_cam_path_name (host only): which count kernel a shape takes -- "lds_table" (S * ncls <= 8192: a
 * per-workgroup LDS table flushed once) or "global_table" (global atomics), "unsupported" outside the limits, "invalid"
 * for a size below the domain. */
size_t spml_segment_tag_cam_workspace_bytes(int S, int ncls);
int spml_segment_tag_cam_f32(const int64_t* nn_index, const float* nn_value, const int64_t* proto_label, int64_t M,
                             float threshold, const int64_t* cluster_index, int S, int ncls, int h2, int w2, int oh,
                             int ow, float* acc, int* counts, float* probs, void* ws, size_t ws_bytes, void* stream);
const char* spml_segment_tag_cam_path_name(int64_t N, int S, int ncls);

/* ------------------------------------------------------------------------
 * Training batches from decoded files: one fused augmentation launch (csrc/augment.hip)
 * replaces: spml/data/datasets/base_dataset.py:135-155,183-186 (mirror, random_resize, random_crop_with_pad, mean / std,
 *           transpose), list_tag_dataset.py:75-78 (image tags), :179-218 (+ grayscale, 5x5 blur),
 *           densepose_dataset.py:78-103,157-198 (+ the left/right remap of the part labels), spml/data/transforms.py
 *           :26-37,76-78,134-151,179-191 and the collate of base_dataset.py:192-223 -- all of it host numpy / cv2 per
 *           image there, followed by the upload of the finished fp32 image and two int64 maps.
 *
 * packed: uint8, device: for every image its RGB bytes (h x w x 3, as PIL decodes them) and its two label planes
 * (semantic, instance; h x w), anywhere in the buffer.  One spml_augment_params record per image says where, and what was
 * drawn for it.  Output pixel (y, x) of image b, with (Y, X) = (y + start_h, x + start_w) in the padded plane of
 * max(new_h, S_h) x max(new_w, S_w) whose top-left corner holds the resized image:
 *   outside new_h x new_w: the pixel is mean[c], both labels are 255;
 *   image, cv2.resize(INTER_LINEAR) on uint8 / 255 in fp32: per axis scale = 1.0 / ((double)new / src),
 *     f = (X + 0.5) * scale - 0.5, s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0;
 *     the fraction rounded to fp32; value = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11);
 *   labels, INTER_NEAREST: s = min(floor(X * scale), src - 1), the same double scale;
 *   flip: source column w - 1 - s, and the semantic label (only it, only then) goes through remap[256];
 *   gray: (r * 0.3f + g * 0.59f) + b * 0.11f into all three channels, the padded area included;
 *   blur: 5 x 5 correlation of that S_h x S_w image with weights[25] (row-major, anchor at the centre), reflect-101 at the
 *     crop's own edges (cv2.filter2D's default border);
 *   then (v - mean[c]) / std[c].
 * The coordinates are formed in fp64 in the kernel with the operations above, unfused: the label maps equal the host
 * chain's bit for bit.  image fp32 [B][3][S_h][S_w]; semantic_label, instance_label int64 [B][S_h][S_w]; mean, std fp32
 * [3] and remap uint8 [256] are device pointers.  params_host and params_dev hold the same B records: the host copy is
 * checked before anything is launched, the device copy is what the kernel reads (and checks again: a record that fails
 * writes nothing and forms no address).  SPML_ERR_UNSUPPORTED, with nothing launched and no output touched: a side of a
 * source, a resized image or the crop outside [1, 16384] (new_h or new_w of 0 included), a crop start outside
 * [0, padded - S], an offset whose plane does not lie inside packed_bytes, blur with a crop side below 3, B > 65535.
 * SPML_ERR_INVALID_ARG: a null or misaligned pointer, B < 1, an output that overlaps an input or another output.
 * One launch, no workspace, no atomics, no host read of device memory: bit-identical from call to call.
 * spml_augment_tags_u8: semantic_tag int64 [B][256], 1 where the value occurs in the un-augmented semantic plane (np.unique
 * + a scatter of ones on the host there): a memset on `stream` and one launch; same record checks for h, w and sem_off.
 * spml_augment_path_name (host only; the expression the launch itself evaluates per record): "plain", "blur" (the tile
 * staged in LDS) or "unsupported".  spml_augment_params_bytes: sizeof(spml_augment_params), for bindings. */
typedef struct spml_augment_params {
  int64_t image_off, sem_off, inst_off;     /* byte offsets into `packed` */
  int32_t h, w;                             /* source size */
  int32_t new_h, new_w;                     /* int(ratio * h), int(ratio * w); = h, w without scaling */
  int32_t start_h, start_w;                 /* crop start in the padded plane */
  int32_t flip, gray, blur;                 /* 0 / non-zero */
  int32_t reserved0;
  float weights[25];                        /* of the blur; read only when blur is set */
  float reserved1;
} spml_augment_params;

size_t spml_augment_params_bytes(void);
const char* spml_augment_path_name(const spml_augment_params* record, int64_t packed_bytes, int S_h, int S_w);
int spml_augment_batch_u8(const unsigned char* packed, int64_t packed_bytes, const spml_augment_params* params_host,
                          const spml_augment_params* params_dev, int B, const float* mean, const float* std,
                          const unsigned char* remap, int S_h, int S_w, float* image, int64_t* semantic_label,
                          int64_t* instance_label, void* stream);
int spml_augment_tags_u8(const unsigned char* packed, int64_t packed_bytes, const spml_augment_params* params_host,
                         const spml_augment_params* params_dev, int B, int64_t* semantic_tag, void* stream);

/* ------------------------------------------------------------------------
 * Inference from decoded files: the view pyramid and the label export, one launch each (csrc/inference_io.hip;
 * DESIGN.md 8o)
 * replaces: spml/data/datasets/base_dataset.py:105-119,157-171 (uint8 / 255, mean / std), spml/utils/general/others.py
 *           :10-47 (create_image_pyramid) with spml/data/transforms.py:26-37 (resize), :110-119
 *           (resize_with_interpolation), :134-151 (resize_with_pad) and the upload of every finished fp32 view;
 *           pyscripts/inference/inference_softmax.py:142-160 (the padded prediction copied to the host, cropped, resized
 *           with cv2.INTER_NEAREST and coloured there).
 *
 * spml_image_views_u8: rgb uint8 [h][w][3] (as PIL decodes it) and, optionally, semantic uint8 [h][w] -> all V views of
 * the image.  One spml_view_params record per view.  View v is the contiguous plane set fp32 [3][pad_h][pad_w] at byte
 * image_off of `images` and, when `semantic` is given, its label int64 [new_h][new_w] (unpadded) at byte label_off of
 * `labels`.  Output pixel (y, x) of view v:
 *   outside new_h x new_w: exactly 0.0f in all three channels (the reference pads the normalised image with 0);
 *   inside: X = x, or new_w - 1 - x under flip (the reference resizes first and mirrors the resized image);
 *   image, cv2.resize(INTER_LINEAR) on the normalised fp32 image: per axis scale = 1.0 / ((double)new / src),
 *     f = (X + 0.5) * scale - 0.5, s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0;
 *     the fraction rounded to fp32; every tap is normalised first, v = (u8 / 255.0f - mean[c]) / std[c], then
 *     value = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11); new == src gives the normalised byte exactly;
 *   label, INTER_NEAREST: s = min(floor(X * scale), src - 1), the same double scale and the same mirror; no remap.
 * The coordinates are formed in fp64 in the kernel with the operations above, unfused: the labels equal the host
 * chain's bit for bit.  rgb, semantic, mean, std (fp32 [3]) and params_dev are device pointers; params_host and
 * params_dev hold the same V records: the host copy is checked before anything is launched, the device copy is what the
 * kernel reads (and checks again: a record that fails writes nothing and forms no address).  image_bytes / label_bytes:
 * the sizes of the two output buffers.  Every element of every plane is written: the buffers need no memset.
 * SPML_ERR_UNSUPPORTED, with nothing launched and no output touched: a side of the source, of a view or of its padded
 * plane outside [1, 16384], pad < new, V outside [1, 64], an offset that is negative, not a multiple of the element size
 * or whose plane leaves its buffer, two planes of one buffer that overlap.  SPML_ERR_INVALID_ARG: a null or misaligned
 * pointer (labels without semantic or the reverse included), an output that overlaps an input or the other output.
 * One launch, no workspace, no atomics, no host read of device memory: bit-identical from call to call.
 * spml_image_views_path_name (host only; the expression the entry itself evaluates): "views", "views+labels" or
 * "unsupported".  spml_view_params_bytes: sizeof(spml_view_params), for bindings.
 *
 * spml_label_export_u8: prediction int64 [pred_h][pred_w] (contiguous), its valid rectangle valid_h x valid_w at the top
 * left, color_map uint8 [256][3] -> gray uint8 [out_h][out_w] and rgb uint8 [out_h][out_w][3]: source pixel by
 * INTER_NEAREST from the valid rectangle to the output size (the index rule above; out == valid is the identity),
 * gray = (uint8)label, rgb = color_map[gray].  One launch; the table is read through the cache.  SPML_ERR_UNSUPPORTED:
 * a side outside [1, 16384], a valid rectangle larger than the prediction.  SPML_ERR_INVALID_ARG: a null or misaligned
 * pointer, an output that overlaps an input or the other output.  spml_label_export_path_name: "export" or
 * "unsupported". */
typedef struct spml_view_params {
  int64_t image_off, label_off;             /* byte offsets into `images` / `labels` */
  int32_t new_h, new_w;                     /* int(scale * h), int(scale * w) */
  int32_t pad_h, pad_w;                     /* max(new, crop) */
  int32_t flip;                             /* 0 / non-zero */
  int32_t reserved0;
} spml_view_params;

size_t spml_view_params_bytes(void);
const char* spml_image_views_path_name(const spml_view_params* records, int V, int h, int w, int64_t image_bytes,
                                       int64_t label_bytes, int with_labels);
int spml_image_views_u8(const unsigned char* rgb, const unsigned char* semantic, int h, int w, const float* mean,
                        const float* std, const spml_view_params* params_host, const spml_view_params* params_dev, int V,
                        float* images, int64_t image_bytes, int64_t* labels, int64_t label_bytes, void* stream);
const char* spml_label_export_path_name(int pred_h, int pred_w, int valid_h, int valid_w, int out_h, int out_w);
int spml_label_export_u8(const int64_t* prediction, int pred_h, int pred_w, int valid_h, int valid_w, int out_h, int out_w,
                         const unsigned char* color_map, unsigned char* gray, unsigned char* rgb, void* stream);

/* ------------------------------------------------------------------------
 * The dense CRF on decoded files: the guide image and the scored export, one launch each (csrc/inference_io.hip;
 * DESIGN.md 8r)
 * replaces: pyscripts/inference/inference_softmax_crf_msc.py:159-164 = inference_crf.py:247-252 (the uint8 image
 *           rebuilt on the host from the normalised fp32 input: image *= std, image += mean, * 255, astype(uint8));
 *           inference_crf.py:257-261 (the refined labels cropped and resized back with cv2.INTER_NEAREST) with
 *           pyscripts/benchmark/benchmark_by_mIoU.py:25-53 (iou_stats) for the labels after and before the CRF.
 *
 * spml_crf_guide_u8: rgb uint8 [h][w][3] -> guide uint8 [new_h][new_w][3].  Per output value: v = what
 * spml_image_views_u8 writes at that pixel of an un-flipped new_h x new_w view (the same device function and the same
 * unfused fp64 coordinates; new == src: (u8 / 255.0f - mean[c]) / std[c]), then numpy's steps on a float32 array and
 * float64 statistics: t = (float)((double)v * std64[c]); t = (float)((double)t + mean64[c]); t = t * 255.0f;
 * out = (uint8)((int32)t & 255).  No contraction anywhere.  The round trip is lossy (with the VOC statistics 129 of the
 * 768 (byte, channel) pairs come back one lower), which is why the file's bytes are not passed through.  mean / std:
 * device fp32 [3], as for spml_image_views_u8; mean64_host / std64_host: the same statistics as doubles on the host
 * (passed to the kernel by value).  Paths (spml_crf_guide_path_name, host only): "guide_table" when new == src in both
 * axes -- the guide is a function of (byte, channel), every workgroup evaluates the 768 pairs into LDS and streams the
 * image through the table in 12-byte spans (four pixels per lane, a fixed channel phase), no fp64 per pixel;
 * "guide_resized" otherwise, four taps per channel and the chain per pixel; "unsupported".  One launch, no workspace, no
 * atomics; every byte of guide is written.  SPML_ERR_UNSUPPORTED: a side outside [1, 16384].  SPML_ERR_INVALID_ARG: a
 * null pointer, rgb / guide / mean / std not 4-byte aligned, guide overlapping an input.  Both before any launch.
 *
 * spml_label_export_scored_u8: gray and rgb exactly as spml_label_export_u8 writes them for `refined`; `before` (int64
 * [pred_h][pred_w], or NULL) is resampled with the same source index and cast the same way; truth: uint8
 * [out_h][out_w] or NULL.  scores: int64 [2][3][ncls] followed by one counter (spml_export_scores_bytes(ncls) =
 * (2 * 3 * ncls + 1) * 8 bytes; 0 outside 1 <= ncls <= 256), accumulated INTO: scores[0] += the (TP+FN, TP+FP, TP)
 * counts of gray against truth by the rule of spml_iou_counts_i64 (only pixels with truth < ncls count, a prediction
 * >= ncls falls into no bin); scores[1] += the same for `before`; the counter += the output pixels whose two bytes
 * differ.  before == NULL leaves scores[1] and the counter alone, truth == NULL both tables.  Every workgroup counts
 * into an int32 LDS table and adds its non-zero bins with 64-bit integer atomics: bit-identical from run to run.
 * SPML_ERR_UNSUPPORTED: the cases of spml_label_export_u8, ncls outside [1, 256].  SPML_ERR_INVALID_ARG: a null or
 * misaligned pointer, an output that overlaps an input or another output. */
const char* spml_crf_guide_path_name(int h, int w, int new_h, int new_w);
int spml_crf_guide_u8(const unsigned char* rgb, int h, int w, const float* mean, const float* std,
                      const double* mean64_host, const double* std64_host, int new_h, int new_w, unsigned char* guide,
                      void* stream);
size_t spml_export_scores_bytes(int ncls);
int spml_label_export_scored_u8(const int64_t* refined, const int64_t* before, int pred_h, int pred_w, int valid_h,
                                int valid_w, int out_h, int out_w, const unsigned char* color_map,
                                const unsigned char* truth, int ncls, unsigned char* gray, unsigned char* rgb,
                                int64_t* scores, void* stream);

/* ------------------------------------------------------------------------
 * Scoring label files against ground truth, a batch of decoded files per call (csrc/score_batch.hip)
 * replaces: pyscripts/benchmark/benchmark_by_mIoU.py:25-53 (iou_stats, three np.histogram per file on the host) and
 *           pyscripts/benchmark/benchmark_by_instance.py:97-108 (np.unique, one mask and one np.histogram per instance).
 *
 * packed: uint8, device, 16-byte aligned: for every file its prediction and ground-truth planes and, optionally, its
 * instance plane, n = h * w bytes each, anywhere in the buffer.  One spml_score_params record per file says where.
 * Every plane offset is a multiple of 16 and every plane is padded inside `packed` to a multiple of 16 bytes (the kernel
 * loads 16-byte vectors); the padding bytes are never counted and their content does not matter.
 * stats: int64 [B][4][ncls], rows TP+FN, TP+FP, TP and the number of instances per class.  Every element is written: the
 * output needs no memset.  For file b and pixel i, with g = gt[i], p = pred[i], s = inst[i]:
 *   the pixel counts only if g < ncls; then TP+FN[g] += 1; TP+FP[p] += 1 if p < ncls, TP+FP[ncls-1] += 1 if p == ncls
 *     (np.histogram closes its last bin on the right; spml_iou_counts_i64 leaves this out because an arg-max never
 *     yields that value, a PNG of unknown origin can hold it), nothing for a larger p; TP[g] += 1 if p == g (a
 *     prediction of ncls over g = ncls - 1 is no true positive);
 *   instances (inst_off >= 0): an id occurs if any pixel carries it, pixels with g >= ncls included; its class is the
 *     lowest class with the largest count among its pixels with g < ncls, class 0 for an id with no such pixel; row 3
 *     counts the occurring ids per class; when all 256 ids occur, id 255 is dropped (`if i < 255` over the sorted unique
 *     ids); row 3 is all zero when inst_off = -1.
 * params_host and params_dev hold the same B records: the host copy is checked before anything is launched, the device
 * copy is what the kernels read (and check again: a record that fails counts nothing and forms no address).
 * ws: 4-byte aligned, at least spml_score_batch_workspace_bytes(B, ncls) bytes (the per-file tables; that call returns 0
 * outside the limits), else SPML_ERR_WORKSPACE; the call zeroes it on `stream` itself, its previous content does not
 * matter.  A memset and two launches on `stream`: the count (each workgroup owns one run of 8192 contiguous pixels of
 * one file; the grid is the SUM of the files' runs, found per workgroup by a prefix over the records) and the pass that
 * turns the tables into stats.  Only integer atomics on 32-bit counters: bit-identical from call to call, in either
 * deterministic mode.  No host read of device memory, no allocation.
 * SPML_ERR_UNSUPPORTED, with nothing launched and stats untouched: B outside [1, 256], ncls outside [1, 64], n outside
 * [1, 2^31), an offset that is negative (other than inst_off = -1), not a multiple of 16 or whose padded plane leaves
 * packed_bytes, two planes that overlap.  SPML_ERR_INVALID_ARG: a null or misaligned pointer, stats or ws overlapping an
 * input or each other.
 * spml_score_batch_path_name (host only; the expression the entry itself evaluates): "lds_table" (the tables of a file,
 * ncls * (ncls + 2) + 256 * (ncls + 1) counters, fit the 8192 entries a workgroup keeps in LDS: ncls <= 27),
 * "global_table" or
 * "unsupported".  spml_score_params_bytes: sizeof(spml_score_params), for bindings. */
typedef struct spml_score_params {
  int64_t pred_off, gt_off, inst_off;       /* byte offsets of the uint8 planes in `packed`; inst_off = -1: no instance plane */
  int64_t n;                                /* pixels of this file (h * w) */
} spml_score_params;

size_t spml_score_params_bytes(void);
size_t spml_score_batch_workspace_bytes(int B, int ncls);
const char* spml_score_batch_path_name(const spml_score_params* records, int B, int64_t packed_bytes, int ncls);
int spml_score_batch_u8(const unsigned char* packed, int64_t packed_bytes, const spml_score_params* params_host,
                        const spml_score_params* params_dev, int B, int ncls, int64_t* stats, void* ws, size_t ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------------
 * The picture of a training summary (csrc/train_summary.hip)
 * replaces: pyscripts/train/train.py:222-258 with spml/utils/general/vis.py:23-31 (write_image_to_tensorboard), :41-48
 *           (convert_label_to_color), :62-101 (embedding_to_rgb) and spml/utils/general/common.py:29-73 (pca through
 *           torch.svd of the gathered P x C matrix on the host), :101-120 (normalize_embedding).
 *
 * emb: fp32 [N, C, H, W], device, 16-byte aligned, in one of two storages named by its element strides: channels-last
 * (pixel_stride == C, channel_stride == 1) or NCHW-contiguous (pixel_stride == 1, channel_stride == H * W).  C is 32 or
 * 64 and P = N * H * W < 2^31, else SPML_ERR_UNSUPPORTED (as for any other pair of strides).  Every pixel is
 * L2-normalised first, x / max(||x||, 1e-12) in fp32; an all-zero pixel stays zero.
 *
 * spml_pca_moments_f32: mean fp64 [C] and cov fp64 [C][C] of the normalised pixels, cov = sum (x - mean)(x - mean)^T /
 * max(P - 1, 1): DIVIDED by P - 1.  Pass 1 takes the column sums, pass 2 the Gram matrix of the rows centred with the
 * mean rounded to fp32, on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation per workgroup); each pass
 * leaves one partial per workgroup in ws and a finishing kernel adds them in index order in fp64.  Four launches.  cov is
 * exactly symmetric.
 * spml_pca_project_minmax_f32: V fp32 [C][3] -> proj fp32 [N, H, W, 3] = normalised row . V (NOT centred, as
 * common.py:68) and minmax fp32 [N][3][2] = (minimum, maximum) of proj per image and channel, exactly the extrema of
 * the values written.  Two launches (per-workgroup partial extrema in ws, a finishing kernel).  N <= 65535.
 * ws: 16-byte aligned (else SPML_ERR_INVALID_ARG), at least spml_train_summary_workspace_bytes(N, C, H, W) bytes (0
 * outside the limits), else SPML_ERR_WORKSPACE; its previous content does not matter and nothing is kept in it between
 * the calls.  No float atomics, no ticket: bit-identical from call to call, in either deterministic mode.
 * spml_pca_path_name (host only; the expression the entries evaluate): "gram_mfma_f32_c32", "gram_mfma_f32_c64", the
 * same with "_nchw" where the transposing LDS tile is taken ("gram_mfma_f32_c32_nchw", "gram_mfma_f32_c64_nchw"), or
 * "unsupported".
 *
 * spml_summary_panels_u8: one launch writes the finished picture.  With the label maps semantic and instance, int64
 * [N, Hl, Wl] (both or neither), out is uint8 [3][out_h][out_w], the reference's rows stacked as
 * torchvision.utils.make_grid(nrow=1, padding=2, pad_value=0) stacks them: per image, side by side, semantic colour,
 * instance colour and embedding RGB, each h x w (the embedding's size), image i at row pad + i * (h + pad), column pad,
 * out_h = N * (h + pad) + pad, out_w = 3 * w + 2 * pad with pad = 2 (pad = 0 is allowed for N = 1: make_grid returns
 * a single image as it is); anything else is SPML_ERR_UNSUPPORTED.  Labels are resized as F.interpolate(mode='nearest'):
 * source = min((int)floorf(dst * ((float)in / out)), in - 1), and coloured with color_map uint8 [256][3] at label & 255
 * (the reference's index_select raises outside 0..255).  Embedding bytes: (uint8)(((v - min) / (max - min)) * 255) in
 * fp32, in that order, truncated (vis.py:92-95), from proj and minmax as the projection writes them; a channel with
 * max == min gives 0 where the reference divides 0 by 0.  Every byte of out is written.  Without label maps (both
 * NULL; Hl, Wl, pad, out_h, out_w and color_map are ignored) out is uint8 [N][3][h][w], the embedding panel alone.
 * Sides in [1, 16384], N * h * w < 2^31, 3 * out_h * out_w < 2^31, else SPML_ERR_UNSUPPORTED; a null or misaligned
 * pointer (proj 16 bytes, labels 8) is SPML_ERR_INVALID_ARG. */
size_t spml_train_summary_workspace_bytes(int N, int C, int H, int W);
const char* spml_pca_path_name(int C, int64_t pixel_stride, int64_t channel_stride);
int spml_pca_moments_f32(const float* emb, int N, int C, int H, int W, int64_t pixel_stride, int64_t channel_stride,
                         double* mean, double* cov, void* ws, size_t ws_bytes, void* stream);
int spml_pca_project_minmax_f32(const float* emb, int N, int C, int H, int W, int64_t pixel_stride,
                                int64_t channel_stride, const float* V, float* proj, float* minmax, void* ws,
                                size_t ws_bytes, void* stream);
int spml_summary_panels_u8(const int64_t* semantic, const int64_t* instance, int N, int Hl, int Wl, const float* proj,
                           const float* minmax, int h, int w, const unsigned char* color_map, int pad, int out_h,
                           int out_w, unsigned char* out, void* stream);

/* ------------------------------------------------------------------------
 * CAM ingest: the class activation maps of a file -> the class maps the random walk takes, one launch
 * (csrc/cam_ingest.hip)
 * replaces: pyscripts/inference/pseudo_camrw_crf.py:108-111 (np.zeros((21, h, w)), cam_full_arr[k + 1] = v for the
 *           entries of the pickled dict, cam_full_arr[0] = np.power(1 - np.max(cam_full_arr[1:], axis=0), ALPHA)) and
 *           :151-152 (F.interpolate(cam_full_arr, scale_factor=1/8., mode='bilinear')).
 *
 * planes: fp32 [K][h][w], device, the K planes the file carries, in any order (NULL allowed for K = 0).  classes: int
 * [K] ON THE HOST, classes[k] = the dict key of plane k = its class - 1; the entry checks the keys and hands the kernel
 * a class -> plane table by value, so nothing of `classes` is read after the call returns.  out: fp32
 * [ncls][h / 8][w / 8], device.  F.interpolate takes the given factor for the source coordinate (8 d + 3.5), so with
 * taps(a)(y, x) = the mean of a at rows 8 y + 3, 8 y + 4 and columns 8 x + 3, 8 x + 4:
 *   out[c]  = taps(plane of class c)               for a class c >= 1 the file carries,
 *   out[c]  = 0                                    for a class it does not carry (written by the kernel: out needs no
 *                                                  memset and may hold anything on entry),
 *   out[0]  = taps((1 - m) ^ alpha), m = the maximum over the carried planes at that source pixel, and over an
 *             implicit 0 exactly when some foreground class is absent (K < ncls - 1) -- with every class present and
 *             negative activations m is negative and is not clamped; a NaN wins the maximum, as in np.max; ncls == 1
 *             gives 1.
 * The [ncls][h][w] array is never formed.  Sums and the power (by multiplication, alpha an integer >= 0, x ^ 0 = 1) run
 * in fp64 and are rounded to fp32 once: every value is within one rounding of the exact expression on the fp32 inputs.
 * One launch of ceil(h / 8 * w / 8 / 64) single-wave workgroups, no workspace, no LDS, no atomics: bit-identical from
 * call to call.
 * SPML_ERR_UNSUPPORTED, with nothing launched and out untouched: h or w below 8 or above 16384, ncls outside [1, 256],
 * K outside [0, ncls - 1].  SPML_ERR_INVALID_ARG, the same: a null out (planes or classes with K > 0), planes or out
 * not 4-byte aligned, alpha < 0, a key outside [0, ncls - 2], a key given twice, out overlapping planes.
 * spml_cam_ingest_path_name (host only; the shape expression the entry evaluates): "cam_ingest" or "unsupported". */
const char* spml_cam_ingest_path_name(int K, int h, int w, int ncls);
int spml_cam_ingest_f32(const float* planes, const int* classes, int K, int h, int w, int ncls, int alpha, float* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPML_HIP_H_ */
