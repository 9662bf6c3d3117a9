/*
 * cslam_hip.h -- C ABI of libcslam_hip.so, the MI355X (gfx950) implementation of
 * cslam's global-descriptor loop-closure hot path.
 *
 * The reference (lajoiepy/cslam) has no FFI for this path: it is duck-typed Python
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference
 * Python function whose arithmetic it replaces; the Python classes in cslam_amd/
 * keep the reference signatures and call these through ctypes.
 *
 * Conventions
 *   - every function returns 0 (CSLAM_OK) or a negative CSLAM_E_* code;
 *     cslam_last_error() returns a thread-local message for the last failure;
 *   - plain pointers and sizes only; no torch / numpy types;
 *   - "_host" entry points take host pointers and synchronise before returning;
 *     "_dev" entry points take device pointers, enqueue on `stream`
 *     (a hipStream_t passed as void*, NULL = default stream) and do not synchronise;
 *   - bank rows are float32 (reference storage dtype, cslam/nns_matching.py:21,39);
 *     queries are float32 (CSLAM_F32) or float64 (CSLAM_F64);
 *   - row indices are int64 in the API (bank row number = order of insertion,
 *     the key of the reference's `items` dict, cslam/nns_matching.py:38);
 *   - threading: like the reference classes (one rclpy single-threaded executor per robot,
 *     loop_closure_detection_node.py:109) objects (banks, communicators) are not thread-safe.  The descriptor-head
 *     entry points keep the scratch they need between their own kernels per (device, stream): calls on
 *     different streams may be in flight together (cslam_amd's two extraction lanes are), calls on one stream
 *     run in order anyway;
 *   - scratch buffers and coefficient tables owned by the library only grow and are released at process exit,
 *     so device pointers captured in a hipGraph stay valid.  A stream that is being captured cannot allocate:
 *     run an entry point once, at the captured sizes, on the stream you capture on (otherwise CSLAM_E_INVALID).
 */
#ifndef CSLAM_HIP_H
#define CSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSLAM_OK 0
#define CSLAM_E_INVALID (-1)  /* bad argument */
#define CSLAM_E_HIP (-2)      /* HIP runtime error (message in cslam_last_error) */
#define CSLAM_E_NOMEM (-3)
#define CSLAM_E_DIM (-4)      /* descriptor dimension mismatch */
#define CSLAM_E_UNSUPPORTED (-5) /* an optional run-time dependency (RCCL) is not available on this host */
#define CSLAM_E_GRAPH (-6)    /* cslam_fiedler / cslam_mac_fw_subset: the graph admits no Fiedler pair (not connected, singular
                                 junction Laplacian, TraceMIN breakdown) -- where the reference's networkx call raises */
#define CSLAM_E_LIMIT (-7)    /* the input exceeds a size limit of this entry point (cslam_fiedler: junction count of the dense
                                 factor); the arguments are valid and another path serves them */

#define CSLAM_F32 0
#define CSLAM_F64 1

/* search strategy (cslam_bank_search_*: `mode`) */
#define CSLAM_MODE_AUTO 0  /* scan for small nq, MFMA for batches */
#define CSLAM_MODE_SCAN 1  /* HBM-bound exact fp64 scan kernel */
#define CSLAM_MODE_MFMA 2  /* fp32-MFMA candidates + fp64 re-score + certificate (+ scan fallback) */

typedef struct cslam_bank cslam_bank_t;
typedef struct cslam_comm cslam_comm_t;   /* one rank of the multi-GPU exchange (RCCL communicator), see the end of the file */

const char *cslam_last_error(void);
int cslam_version(void);
int cslam_device_count(int *count);
int cslam_device_info(int device, char *name, int name_len, int64_t *hbm_bytes, int *cu_count);

/* ---- descriptor bank: NearestNeighborsMatching.__init__/add_item ----------
 * replaces cslam/nns_matching.py:10-40 (growable float32 bank, amortised doubling).
 * The bank lives in HBM on `device`; rows are padded to a multiple of 32 floats.   */
int cslam_bank_create(int device, int dim, int64_t capacity_hint, cslam_bank_t **out);
int cslam_bank_destroy(cslam_bank_t *bank);
int cslam_bank_size(const cslam_bank_t *bank, int64_t *n, int *dim);
int cslam_bank_clear(cslam_bank_t *bank);
/* append n rows given on the host; dtype CSLAM_F32 or CSLAM_F64 (values are cast to
 * float32 on store exactly like `self.data[self.n] = vector`, nns_matching.py:39). */
int cslam_bank_add_host(cslam_bank_t *bank, const void *vecs, int dtype, int64_t n);
/* append n float32 rows already in device memory, row stride `ld` floats */
int cslam_bank_add_dev(cslam_bank_t *bank, const float *d_vecs, int64_t ld, int64_t n, void *stream);
/* copy rows [row0, row0+nrows) back to the host, dense [nrows, dim] float32
 * (backs the reference's public `.data` attribute, tests/test_sparse_matching.py:36) */
int cslam_bank_read_host(const cslam_bank_t *bank, int64_t row0, int64_t nrows, float *out);
/* raw device views (row stride in floats); valid until the next add that grows the bank */
int cslam_bank_device_ptr(const cslam_bank_t *bank, const float **d_rows, int64_t *ld);

/* ---- search: NearestNeighborsMatching.search / search_best -----------------
 * replaces cslam/nns_matching.py:42-76:
 *     sim[i] = 1 - clip(1 - q.b_i / sqrt((q.q)(b_i.b_i)), 0, 2)   for i < limit
 *     order  = descending sim (NaN first), ties -> larger row index
 * row_limit: NULL, or [nq] int64: query j only sees rows < row_limit[j] (the causal
 *     order of global_descriptor_loop_closure_detection.py:157-160).
 * out_idx [nq,k] int64 (-1 padded), out_sim [nq,k] float64 (NaN padded),
 * out_cnt [nq] int32 = min(k, rows visible).
 * Scores are computed in float64 from the float32 bank / given-dtype query; the
 * returned order is the exact order of those float64 scores in every mode.       */
int cslam_bank_search_host(cslam_bank_t *bank, const void *queries, int q_dtype, int64_t nq,
                           int k, const int64_t *row_limit, int mode,
                           int64_t *out_idx, double *out_sim, int32_t *out_cnt);
/* device-pointer variant: d_queries [nq, ldq] (ldq in elements), outputs device arrays */
int cslam_bank_search_dev(cslam_bank_t *bank, const void *d_queries, int q_dtype, int64_t ldq,
                          int64_t nq, int k, const int64_t *d_row_limit, int mode,
                          int64_t *d_out_idx, double *d_out_sim, int32_t *d_out_cnt,
                          void *stream);

/* One batch of queries against nb banks of one device -- a robot's own bank and its copies of the other robots' banks
 * (cslam/loop_closure_sparse_matching.py:21-31), which the reference searches one after the other for every keyframe
 * (lcsm.py:45-53 best-1 per other robot, lcsm.py:74-76 top-k in the local bank).  Same results as nb calls of
 * cslam_bank_search_dev with (k[i], d_row_limit[i], d_out_*[i]); all kernels are enqueued before the single host
 * synchronisation the uncertified-query counts need, each bank's on a stream of its own forked from and joined back into
 * `stream` (chunk-sized searches do not fill the chip one after the other).
 * d_row_limit may be NULL (no limits) or hold NULL entries.  A bank may appear only once in the list. */
int cslam_bank_search_multi_dev(cslam_bank_t *const *banks, int nb, const void *d_queries, int q_dtype, int64_t ldq,
                                int64_t nq, const int *k, const int64_t *const *d_row_limit, int mode,
                                int64_t *const *d_out_idx, double *const *d_out_sim, int32_t *const *d_out_cnt,
                                void *stream);
/* The two halves of cslam_bank_search_dev / cslam_bank_search_multi_dev, for a host that pipelines steps (the reference's
 * callbacks are serialised, cslam/loop_closure_detection_node.py:109; a batch host overlaps step i's read-back with step
 * i + 1's extraction):
 *   *_enqueue_dev  puts every kernel of the search on `stream` and returns without a host synchronisation;
 *   *_finish       waits for ONE event -- the 4-byte count of queries whose float32 candidate stage could not be
 *                  certified (see cslam_bank_last_stats), recorded right behind its copy, NOT for the stream: work enqueued
 *                  after the search keeps running -- and enqueues the exact float64 scan for those queries (normally none).
 * Results are valid in `stream` order after finish.  One search per bank may be in flight: queries, row limits and outputs
 * must stay alive and the bank unchanged until it is finished (add / clear / another search return CSLAM_E_INVALID).
 * n_uncertified (or NULL) receives that count.  finish without a pending search is a no-op. */
int cslam_bank_search_enqueue_dev(cslam_bank_t *bank, const void *d_queries, int q_dtype, int64_t ldq, int64_t nq, int k,
                                  const int64_t *d_row_limit, int mode, int64_t *d_out_idx, double *d_out_sim,
                                  int32_t *d_out_cnt, void *stream);
int cslam_bank_search_finish(cslam_bank_t *bank, int64_t *n_uncertified);
/* Between the halves: the uncertified-query count of the enqueued search as a 4-byte device-to-device copy on `stream` (the
 * enqueue's stream) into d_count; 0 when the search needs no certificate (exact-scan modes) or none is pending.  Lets a sharded
 * step (one robot bank, or one row shard, per GPU: loop_closure_sparse_matching.py:45-53 across ranks) ship the count WITH its
 * provisional lists, so that every rank knows in stream order -- no host round trip -- whether a shard still owes a re-scan. */
int cslam_bank_search_flag_copy_dev(cslam_bank_t *bank, int32_t *d_count, void *stream);
int cslam_bank_search_multi_enqueue_dev(cslam_bank_t *const *banks, int nb, const void *d_queries, int q_dtype, int64_t ldq,
                                        int64_t nq, const int *k, const int64_t *const *d_row_limit, int mode,
                                        int64_t *const *d_out_idx, double *const *d_out_sim, int32_t *const *d_out_cnt,
                                        void *stream);
int cslam_bank_search_multi_finish(cslam_bank_t *const *banks, int nb, int64_t *n_uncertified /* summed over the banks, or NULL */);
/* statistics of the last search on this bank (for tests / bench):
 * stats[0] = queries that failed the fp32 certificate and were re-done by the scan,
 * stats[1] = mode actually used (CSLAM_MODE_*), stats[2] = bank segments,
 * stats[3] = query tiles.  Synchronises the bank's last stream.                    */
int cslam_bank_last_stats(cslam_bank_t *bank, int64_t stats[4]);
/* which candidate stage the last MFMA-mode search of this bank ran, and the state of its back-off (a bank whose near-duplicates
 * overflow the fp16 stage's re-scoring window runs its next searches on the f32-input stage; results are exact either way, time is
 * not): info[0] = fp16 products per pair of the last search's stage (1: the default; 3: exact pairs; 0: the f32-input stage),
 * info[1] = searches left on the f32-input stage before the fp16 stage is retried, info[2] = length of the next back-off (8,
 * doubling up to 1024 while retries keep overflowing), info[3] = 1 when CSLAM_MFMA_STAGE1 fixed the stage (no back-off).
 * Valid after the search's finish; does not synchronise. */
int cslam_bank_last_stage(cslam_bank_t *bank, int32_t info[4]);
/* time (ms, HIP events on the launch stream) of the dominant kernel of the last
 * MFMA-mode search: sim_topk_mfma.  -1 if the last search did not use it.        */
int cslam_bank_last_kernel_ms(cslam_bank_t *bank, float *ms);
/* One bank row-sharded over several GPUs (the single-bank metric at > 1 GPU): merge of the
 * per-shard results of cslam_bank_search_dev into the top-k of the whole bank -- what
 * `argsort(sim)[::-1][:k]` (cslam/nns_matching.py:60-61) returns over all rows, because the global top-k
 * is contained in the union of the per-shard top-k lists.  Shard s holds the global rows
 * [row_offset[s], row_offset[s] + n_s); row_offset is a HOST array of `shards` (<= 64) entries.
 * d_idx / d_sim [shards, nq, k] and d_cnt [shards, nq] are the shards' outputs (each list in search order,
 * shard-local rows); outputs as cslam_bank_search_dev with GLOBAL rows; same order: descending similarity,
 * NaN first, ties -> larger global row.  Similarities are passed through bit for bit.            */
int cslam_topk_merge_dev(const int64_t *d_idx, const double *d_sim, const int32_t *d_cnt,
                         const int64_t *row_offset, int shards, int64_t nq, int k,
                         int64_t *d_out_idx, double *d_out_sim, int32_t *d_out_cnt, void *stream);

/* ---- descriptor heads (device pointers; all float32) -------------------------- */
/* rows of x [n, d] (stride ld) scaled to unit L2 norm, x / max(||x||, eps);
 * F.normalize(p=2) of cslam/vpr/cosplace_utils/layers.py:32-36, netvlad.py:105-106,126-128;
 * eps = 1e-12 (torch default).  zero_norm_to_one != 0 gives sklearn.preprocessing.normalize
 * semantics instead (zero rows stay zero; netvlad.py:235-236). */
int cslam_l2_normalize_dev(float *d_x, int64_t n, int d, int64_t ld, float eps,
                           int zero_norm_to_one, void *stream);
/* NetVLADLayer.forward, cslam/vpr/netvlad.py:94-130.
 * feat [B, C, P] (NCHW flattened), assign_w [K, C] (1x1 conv, no bias: vladv1),
 * assign_b [K] or NULL, centroids [K, C]; out [B, K*C] with row pitch ldo floats. */
int cslam_vlad_aggregate_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                             const float *d_centroids, int B, int C, int P, int K,
                             float *d_out, int64_t ldo, void *stream);
/* The same layer on a channels-last feature map d_feat [B][P][C] (what the Winograd trunk writes): batches only (B > 8,
 * P <= 256); spares the layout conversion in front of the head. */
int cslam_vlad_aggregate_nhwc_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                                  const float *d_centroids, int B, int C, int P, int K,
                                  float *d_out, int64_t ldo, void *stream);
/* The matrix form of the channels-last layer (C a multiple of 128 up to 512, 32 <= P <= 200, K = 64, any B) whose final store also
 * writes the row as the fp16 hi / lo pairs that cslam_pca_project_from_pairs_dev multiplies: d_A2 [S][B][K C / S / 32][hi 32 | lo 32]
 * of s v, s the power of two from x_bound (> 0: a bound of max |v|, 1 for the L2-normalised vector), S a power of two up to K.
 * d_out [B, K*C] (pitch ldo) or NULL when only the pairs are wanted.  Both outputs equal cslam_vlad_aggregate_nhwc_dev and the
 * rows cslam_pca_project_pairs_dev derives from it bit for bit. */
int cslam_vlad_aggregate_nhwc_pairs_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                                        const float *d_centroids, int B, int C, int P, int K, float x_bound, int S,
                                        void *d_A2, float *d_out, int64_t ldo, void *stream);
/* CosPlace aggregation head, cslam/vpr/cosplace_utils/network.py:23-29 + layers.py:8-36:
 * L2Norm(C) -> GeM(p, eps) -> Flatten -> Linear(W [Dout, C], b [Dout]) -> L2Norm.
 * feat [B, C, P]; out [B, Dout]. */
int cslam_gem_fc_head_dev(const float *d_feat, float p, float eps, const float *d_W,
                          const float *d_b, int B, int C, int P, int Dout,
                          float *d_out, void *stream);
/* the same head on a channels_last map: feat [B, P, C], C a multiple of 4 */
int cslam_gem_fc_head_nhwc_dev(const float *d_feat, float p, float eps, const float *d_W,
                               const float *d_b, int B, int C, int P, int Dout,
                               float *d_out, void *stream);
/* PCA projection + row L2, cslam/vpr/netvlad.py:234-236 (sklearn PCA.transform + normalize):
 *   y = x @ comp^T - mean_proj ;  y *= inv_scale (whitening) ;  y /= ||y|| (zero rows stay zero)
 * comp [Dout, Din]; mean_proj [Dout] = mean @ comp^T (precomputed once by the caller) or NULL;
 * inv_scale [Dout] = 1/sqrt(explained_variance) or NULL.  x [B, Din], out [B, Dout].
 * Din must be a multiple of 32; ldx / ldc are the row pitches of x / comp in floats (pad them off
 * multiples of 256 floats: power-of-two pitches alias in L2).  fp32 MFMA GEMM, deterministic split-K. */
int cslam_pca_project_dev(const float *d_x, int64_t ldx, const float *d_comp, int64_t ldc,
                          const float *d_mean_proj, const float *d_inv_scale, int B, int Din, int Dout,
                          float *d_out, void *stream);
/* The same projection for batches on the fp16 matrix pipe with fp32-grade results: x and the components as exact fp16 hi / lo
 * pairs, three partial products in fp32 accumulators (the arithmetic and the kernel of cslam_wino_gemm_h2_dev; Din is cut into
 * S splits whose partial products the epilogue sums).  d_W2: [S][Dout][Din / S / 32][hi 32 | lo 32] fp16 of sW * components
 * (`pca_pair_weights` in cslam_amd/vpr/heads.py), inv_sw = 1 / sW; Din a multiple of 32 S, Dout of 128.  x_bound > 0: a known
 * bound of max |x| (1 for the L2-normalised VLAD vectors of netvlad.py:130) spares the pass that measures it. */
int cslam_pca_project_pairs_dev(const float *d_x, int64_t ldx, float x_bound, const void *d_W2, float inv_sw, int S,
                                const float *d_mean_proj, const float *d_inv_scale, int B, int Din, int Dout,
                                float *d_out, void *stream);
/* The same projection of rows that already are pairs (d_A2 as cslam_vlad_aggregate_nhwc_pairs_dev writes it, scaled with the
 * same x_bound > 0): the products, the split sums and the epilogue of cslam_pca_project_pairs_dev without its pass over x. */
int cslam_pca_project_from_pairs_dev(const void *d_A2, float x_bound, const void *d_W2, float inv_sw, int S,
                                     const float *d_mean_proj, const float *d_inv_scale, int B, int Din, int Dout,
                                     float *d_out, void *stream);
/* image transform, cslam/vpr/netvlad.py:202-208 / cosplace.py:73-79:
 * CenterCrop(crop) -> Resize(out_hw, PIL bicubic, antialiased, 8-bit intermediate) ->
 * ToTensor (/255, HWC->CHW) -> Normalize(mean, std).
 * img [B, H, W, 3] uint8 RGB; out [B, 3, out_hw, out_hw] float32. */
int cslam_preprocess_dev(const uint8_t *d_img, int B, int H, int W, int crop, int out_hw,
                         const float mean[3], const float std_[3], float *d_out, void *stream);
/* the same transform, out [B, out_hw, out_hw, 3] float32: the channels_last storage the trunks' first convolution reads
 * (cosplace.py:73-79 feeds `self.model(...)` directly; the layout is this library's choice) */
int cslam_preprocess_nhwc_dev(const uint8_t *d_img, int B, int H, int W, int crop, int out_hw,
                              const float mean[3], const float std_[3], float *d_out, void *stream);

/* ---- candidate sparsifier pieces (cslam/mac/mac.py) --------------------------- */
/* grad_from_fiedler, mac.py:112-130: g[k] = w[k] * (v[i_k] - v[j_k])^2, float64 */
int cslam_mac_grad_dev(const double *d_fiedler, const int32_t *d_edge_i, const int32_t *d_edge_j,
                       const double *d_weights, int64_t m, double *d_grad, void *stream);
/* y = A x for a float64 CSR matrix (the Laplacian L(w) of mac.py:61-77), nvec dense columns,
 * x and y column-major [n, nvec]: the L @ X product inside networkx _tracemin_fiedler
 * (third-party).  One thread per (row, column): deterministic. */
int cslam_csr_spmm_dev(const int64_t *d_indptr, const int32_t *d_indices, const double *d_data,
                       int64_t n, const double *d_x, int nvec, double *d_y, void *stream);

/* same product with x, y stored [n][4] row-major (the layout of the chain-reduced solver below) */
int cslam_csr_spmm4_dev(const int64_t *d_indptr, const int32_t *d_indices, const double *d_data,
                        int64_t n, const double *d_x, double *d_y, void *stream);

/* 4-column block operations of the TraceMIN outer loop on [n][4] float64 row-major vectors
 * (the X'X, X'LX, X Y, projection and residual steps of networkx `_tracemin_fiedler`):
 *   gram:     out20[0..15] = A^T B (4x4 row-major), out20[16..19] = column sums of B
 *   affine:   out = A * M16 - shift4 (shift4 may be NULL)
 *   residual: out1 = sum_k | (W y4)[k] - sigma * X[k][0] |
 * d_partial: scratch of >= 20 * 1024 doubles.  Deterministic (fixed reduction order). */
int cslam_block4_gram_dev(const double *d_A, const double *d_B, int64_t n, double *d_partial,
                          double *d_out20, void *stream);
int cslam_block4_affine_dev(const double *d_A, int64_t n, const double *d_M16, const double *d_shift4,
                            double *d_out, void *stream);
int cslam_block4_residual_dev(const double *d_W, const double *d_X, int64_t n, const double *d_y4,
                              double sigma, double *d_partial, double *d_out1, void *stream);

/* Host-synchronous twins of the three calls above for the TraceMIN outer loop, whose 4 x 4 algebra runs on the host
 * (LAPACK, as in networkx): the 4 x 4 matrix / shift / Ritz vector are HOST pointers passed on as kernel arguments, and the
 * 20-double (1-double) result is copied to h_out and the stream synchronised inside the call. */
int cslam_block4_gram_sync(const double *d_A, const double *d_B, int64_t n, double *d_partial, double *d_out20,
                           double *h_out20, void *stream);
int cslam_block4_affine_host(const double *d_A, int64_t n, const double *h_M16, const double *h_shift4, double *d_out,
                             void *stream);
int cslam_block4_residual_sync(const double *d_W, const double *d_X, int64_t n, const double *h_y4, double sigma,
                               double *d_partial, double *d_out1, double *h_out1, void *stream);

/* Chain-reduced Laplacian solve (cslam_amd/mac/chain_solver.py): replaces the sparse-LU solves inside
 * networkx `_tracemin_fiedler` that cslam/mac/mac.py:52-58 calls (85 % of MAC's time).  Vectors are
 * [n][4] float64 row-major.  forward: segmented prefix sums of the right-hand side along the odometry
 * chains (Bn, Qn) and the reduced right-hand side bt [nJ][4] on the junction nodes; backward: closed-form
 * interior potentials from the junction solution xJ [nJ][4].  Structure arrays (is_junction [n] u8,
 * r [n-1] chain resistances, J [nJ], per-junction segment ids, per-segment end nodes sa/sb and total
 * resistance Rl, per-node Rn / jid / seg_of) are built once per Laplacian by the host.
 * d_tmp: [n][4]; d_scratch: >= 9 * ceil(n / 2048) doubles + slack (see mac_kernels.hip). */
int cslam_chain_forward_dev(const double *d_b, const uint8_t *d_is_junction, const double *d_r, int64_t n,
                            const int64_t *d_J, int nJ, const int *d_seg_start_of, const int *d_seg_end_of,
                            const int64_t *d_sa, const int64_t *d_sb, const double *d_Rl,
                            double *d_Bn, double *d_Qn, double *d_tmp, double *d_scratch, double *d_bt,
                            void *stream);
int cslam_chain_backward_dev(const double *d_xJ, const double *d_Bn, const double *d_Qn, const double *d_r,
                             const double *d_Rn, const int *d_jid, const int *d_seg_of, const int64_t *d_sa,
                             const int64_t *d_sb, const double *d_Rl, int64_t n, double *d_x, void *stream);
/* x <- (L L^T)^-1 x for the dense lower Cholesky factor L [m][ld] (float64, row-major; only the lower triangle is
 * read; col_major != 0: element (r, c) at c * ld + r instead of r * ld + c, the layout LAPACK-style library
 * factorisations return) of the grounded junction Laplacian, x [m][4]: the junction solve inside every TraceMIN iteration (SuperLU's
 * solve in networkx `_tracemin_fiedler`, called at cslam/mac/mac.py:52-58).  d_dinv: inverses of the bs x bs diagonal
 * blocks of L, [ceil(m / bs)][bs][bs] (a ragged last block in the top-left corner of its slot), d_dinvT: the same
 * blocks transposed (only the lower triangle of a d_dinv block and the upper triangle of a d_dinvT block are read);
 * d_tmp: [bs][4] scratch.  Blocked substitution, every factor element read exactly once per sweep, fixed summation order. */
int cslam_chol_solve4_dev(const double *d_L, int64_t m, int64_t ld, int col_major, const double *d_dinv,
                          const double *d_dinvT, int bs, double *d_x, double *d_tmp, void *stream);

/* (lambda_2, v_2) of a pose-graph Laplacian in ONE call, for a host without Python: replaces the whole of
 * cslam/mac/mac.py:35-59 (MAC.find_fiedler_pair -> networkx algebraic_connectivity / fiedler_vector with
 * method='tracemin_lu', seed RandomState(7)).  The Laplacian is a HOST CSR matrix (both triangles, column indices sorted
 * and unique within a row -- what mac.py:61-77 builds), n > 4 nodes, connected.  Same TraceMIN iteration as
 * cslam_amd/mac/fiedler.py; the inner solves run by the chain reduction above with the junction system factorised densely
 * on the GPU (rocBLAS / rocSOLVER, looked up at run time: CSLAM_E_UNSUPPORTED without them; at most 64000 junctions).
 *   h_x0        start block [n][4] row-major, or NULL = numpy RandomState(seed).normal(size=(4, n)).T (bit-identical;
 *               cslam_fiedler_start_block writes that block to a host buffer)
 *   tol         stopping rule ||L v - lambda v||_1 / ||L||_inf < tol (mac.py passes 1e-8)
 *   max_iters   <= 0: no practical limit (the reference has none); otherwise CSLAM_E_GRAPH when exceeded.  A graph that is
 *               not connected (networkx raises) or whose iteration breaks down returns CSLAM_E_GRAPH as well
 *   h_lambda2, h_v [n], h_iters (optional): results on the host.  The sign of v is arbitrary (as in the reference).
 * Work runs on the CURRENT device and `stream` (NULL: a non-blocking stream of the library's own; the blocked factorisation
 * also uses two side streams for its look-ahead, CSLAM_FIEDLER_LOOKAHEAD=0 keeps it on one); device memory is a workspace kept between calls (MAC calls this once per
 * Frank-Wolfe iteration), freed by cslam_fiedler_release.  Calls are serialised by a lock. */
int cslam_fiedler(int64_t n, const int64_t *h_indptr, const int32_t *h_indices, const double *h_data, const double *h_x0,
                  uint32_t seed, double tol, int max_iters, double *h_lambda2, double *h_v, int *h_iters, void *stream);
int cslam_fiedler_start_block(uint32_t seed, int64_t n, double *h_x0);
int cslam_fiedler_release(void);

/* The sparsifier's Frank-Wolfe loop around cslam_fiedler, for a host without Python: replaces cslam/mac/mac.py:191-233
 * (MAC.fw_subset) together with :61-77 (L(w) = L_fixed + sum_k w_k weight_k L_k over w_k > 1e-10), :112-130 (gradient
 * weight_k (v_i - v_j)^2), :132-147 (linear maximisation = indicator of the k largest gradients) and :168-189 (final
 * rounding: top k of w rounded to 10 decimals, ties towards the larger edge weight).  All arrays are HOST arrays:
 *   fixed_* [n_fixed], cand_* [n_cand]  edges (i, j, weight) over poses 0 .. num_poses-1 (the re-keyed edges of
 *                                       algebraic_connectivity_maximization.py:468-543; fixed includes the odometry chains)
 *   w_init [n_cand]      start point (the greedy indicator of acm.py:380-395), k edges to choose, max_iters as mac.py (5 in cslam)
 *   duality_gap_tol      1e-8 in the reference; fiedler_tol = the tol mac.py:33 passes on (1e-8)
 *   h_selected [n_cand]  1.0 for the chosen edges, 0.0 otherwise; h_w_unrounded [n_cand], h_upper, h_iters optional (NULL)
 * Exact ties in a top-k (left arbitrary by numpy's argpartition) go to the larger index.  A failing Fiedler solve (e.g. the
 * fixed edges do not connect the graph) returns that call's error; the reference's retry policy (acm.py:436-466) is the caller's. */
int cslam_mac_fw_subset(int64_t num_poses, int64_t n_fixed, const int64_t *fixed_i, const int64_t *fixed_j,
                        const double *fixed_w, int64_t n_cand, const int64_t *cand_i, const int64_t *cand_j,
                        const double *cand_w, const double *w_init, int64_t k, int max_iters, double duality_gap_tol,
                        double fiedler_tol, double *h_selected, double *h_w_unrounded, double *h_upper, int *h_iters,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pose-graph back end: GNC-TLS around Levenberg-Marquardt on SE(3).
 * Replaces src/back_end/decentralized_pgo.cpp:797-827 (DecentralizedPGO::optimize: GncOptimizer<GncParams<
 * LevenbergMarquardtParams>> over the aggregated graph), :64-70 (default sigmas 0.01 rad / 0.1 m), :843-845 (the prior on
 * the first pose) and the BetweenFactor<Pose3> edges of src/back_end/gtsam_utils.cpp:58-89.  GTSAM is third party and was
 * not available to compare against: the algorithm is the one csrc/pgo.hip states, tests/pgo_reference.py its float64 yardstick.
 *
 * Conventions: poses and measurements are 4 x 4 row-major float64 (16 doubles); the tangent is GTSAM's [omega, v]; factor k
 * in [0, nf) is the between factor (ei[k], ej[k]) with residual Log(Z_k^-1 T_i^-1 T_j), factor nf is the prior on pose `prior`
 * with residual Log(Z_nf^-1 T_prior); sigmas are [nf + 1][6]; E_k = 1/2 sum (e / sigma)^2; the cost is sum w_k E_k.
 * The entries share ONE workspace (grow-only, on the current device, freed by cslam_pgo_release) and are serialised by a lock.
 * No floating-point atomics anywhere: the same input gives the same bits. */
/* Structure pass (csrc/pgo_plan.h) of the edge list and upload of its index lists; every staged entry below works on the
 * graph of the last call.  CSLAM_E_INVALID on i == j or an index out of range, CSLAM_E_LIMIT on more junctions than the dense
 * junction system holds; both before anything touches HIP.  h_info (optional) [8]: junctions, segments, interior poses,
 * distinct pose pairs, poses promoted by the PGO_SEG_MAX cut, longest segment, PGO_SEG_MAX, the junction cap. */
int cslam_pgo_plan(int64_t n, int64_t nf, const int32_t *h_ei, const int32_t *h_ej, int64_t prior, int64_t *h_info);
/* decentralized_pgo.cpp:797-827 (what NonlinearFactorGraph::linearize does inside the LM iteration): E_k [nf + 1] to d_E and
 * the whitened (sqrt(w_k) / sigma) normal equations -- 6 x 6 diagonal block and gradient per pose, one block per pose pair --
 * to the workspace; cslam_pgo_system_host copies them out: h_Hdiag [n][36], h_g [n][6], h_Hoff [pairs][36] = block (row
 * h_pa, column h_pb), h_pa < h_pb sorted; any pointer may be NULL. */
int cslam_pgo_linearize_dev(const double *d_poses, const double *d_meas, const double *d_sigmas, const double *d_weights,
                            double *d_E, void *stream);
int cslam_pgo_system_host(double *h_Hdiag, double *h_g, double *h_Hoff, int32_t *h_pa, int32_t *h_pb, void *stream);
/* (H + lambda I) delta = -g on the system of the last linearise (LevenbergMarquardtOptimizer's damped solve, lambda I as
 * the reference's default, not the diagonal): segments by block recurrence, junctions by dense Cholesky, back substitution.
 * d_delta [n][6]; *h_status 0, or 1 on a non-positive pivot (nothing aborts; delta is then meaningless);
 * *h_predicted = -(g . delta + 1/2 delta . H delta), the decrease the quadratic model predicts. */
int cslam_pgo_solve_dev(double lambda, double *d_delta, int *h_status, double *h_predicted, void *stream);
/* The dense stage of cslam_pgo_solve_dev on its own (the same launch sequence, written once in csrc/pgo.hip): S x = b by the
 * panelled Cholesky factor and two triangular solves.  d_S [N][N] row-major: the lower triangle with the diagonal is read and
 * holds the factor on exit; the strict upper triangle never enters a result and is never written.  d_rhs [N]: b in, x out.
 * *h_status 0, or 1 on a non-positive pivot (the columns before it are still the factor's).  Any N in [1, 6 x the junction
 * cap], CSLAM_E_INVALID otherwise or on a NULL pointer, before any launch.  Needs no plan. */
int cslam_pgo_dense_solve_dev(double *d_S, int64_t N, double *d_rhs, int *h_status, void *stream);
/* Pose3::retract with the full exponential: out_v = T_v Exp(delta_v).  Needs no plan. */
int cslam_pgo_retract_dev(const double *d_poses, const double *d_delta, int64_t n, double *d_out, void *stream);
/* NonlinearFactorGraph::error of the weighted graph: E_k to d_E, *h_cost = sum w_k E_k (block partials in block order). */
int cslam_pgo_cost_dev(const double *d_poses, const double *d_meas, const double *d_sigmas, const double *d_weights, double *d_E,
                       double *h_cost, void *stream);
/* GncOptimizer::calculateWeights, TLS: 0 at E >= (mu + 1) / mu barc2, 1 at E <= mu / (mu + 1) barc2,
 * sqrt(barc2 mu (mu + 1) / E) - mu between; d_known (optional, bytes): known inliers keep 1.  Needs no plan. */
int cslam_pgo_weights_dev(const double *d_E, int64_t nfac, double mu, double barc2, const uint8_t *d_known, double *d_w,
                          void *stream);
/* The whole of DecentralizedPGO::optimize (decentralized_pgo.cpp:797-827) on HOST arrays, for a host without Python.
 *   h_poses [n][16]      initial estimate in, result out
 *   h_meas [nf + 1][16], h_sigmas [nf + 1][6] (positive, finite: CSLAM_E_INVALID otherwise), h_known [nf + 1] bytes or NULL
 *   h_params             NULL = the reference's defaults, or [12]: lambda_0 1e-5, lambda factor 10, lambda upper bound 1e5,
 *                        LM iterations 100, relative 1e-5 and absolute 1e-5 error tolerance, model fidelity 1e-3, GNC rounds
 *                        100, mu step 1.4, GNC relative cost tolerance 1e-5, weights tolerance 1e-4, barc^2 (1/2 chi2inv(0.99, 6))
 *   h_weights [nf + 1]   final GNC weights
 *   h_info [8]           GNC rounds, LM iterations, solves, final cost, final lambda, status (1: some trial step met a
 *                        non-positive pivot and was rejected), junctions, segments
 * cslam_pgo_trace: accept (1) / reject (0) of every trial step of the last call, in order. */
int cslam_pgo_optimize(int64_t n, int64_t nf, const int32_t *h_ei, const int32_t *h_ej, int64_t prior, double *h_poses,
                       const double *h_meas, const double *h_sigmas, const uint8_t *h_known, const double *h_params,
                       double *h_weights, double *h_info);
int cslam_pgo_trace(int32_t *h_out, int64_t cap, int64_t *h_count);
int cslam_pgo_release(void);

/* ------------------------------------------------------------------------------------------------
 * Lidar place recognition: ScanContext bank.
 * Replaces cslam/lidar_pr/scancontext_matching.py:5-104 (ScanContextMatching) with its helpers
 * scancontext_utils.py:78-79 (sc2rk) and :81-113 (distance_sc).  Scan contexts are float64
 * [rings, sectors] row-major (the reference's np.zeros default dtype), ring keys are the row means
 * in numpy's summation order, all arithmetic float64.
 *   add_*    : scancontext_matching.py:23-42 (copies; ring keys and column norms computed on device)
 *   read_host: the reference's public `scancontexts` / `ringkeys` arrays
 *   search_* : scancontext_matching.py:44-87 for a batch of queries.  Stage 1 = num_candidates
 *              nearest ring keys (brute force instead of the per-query KD-tree, same set, ascending
 *              distance, ties -> smaller row); stage 2 = distance_sc(candidate, query) for each;
 *              best = first strict minimum below 1.0.  best_idx[j] = -1 when no candidate is below 1.0
 *              (the reference then answers items[0] with similarity 0.0 -- the Python class does that),
 *              best_sim[j] = 1 - best distance, best_yaw[j] = yaw_diff in sectors (1..sectors).
 *              row_limit[j] (optional) hides bank rows >= row_limit[j] from query j.
 *              cand / cdist / cyaw [nq, num_candidates] are optional (NULL) diagnostics: candidate
 *              rows (-1 = bank smaller than num_candidates), their distances and yaw shifts.
 *   create   : rings in [1, 64], sectors in [1, 128], and stage 2 must fit one workgroup's LDS:
 *              8 * (2*rings*sectors + 3*sectors + sectors*(sectors+1)) <= 163840 bytes (64 x 91 and 14 x 128 are
 *              the largest such shapes; 20 x 128 is not one).  Any other shape is CSLAM_E_INVALID at create, so
 *              that no bank exists that no search can serve.
 */
typedef struct cslam_scbank cslam_scbank_t;
int cslam_scbank_create(int device, int rings, int sectors, int64_t capacity_hint, cslam_scbank_t **out);
int cslam_scbank_destroy(cslam_scbank_t *bank);
int cslam_scbank_size(const cslam_scbank_t *bank, int64_t *n, int *rings, int *sectors);
int cslam_scbank_clear(cslam_scbank_t *bank);
int cslam_scbank_add_host(cslam_scbank_t *bank, const double *sc, int64_t n);
int cslam_scbank_add_dev(cslam_scbank_t *bank, const double *d_sc, int64_t n, void *stream);
int cslam_scbank_read_host(const cslam_scbank_t *bank, int64_t first, int64_t count, double *sc_out,
                           double *ringkeys_out);
int cslam_scbank_search_host(cslam_scbank_t *bank, const double *queries, int64_t nq, int num_candidates,
                             const int64_t *row_limit, int64_t *best_idx, double *best_sim,
                             int32_t *best_yaw, int64_t *cand, double *cdist, int32_t *cyaw);
int cslam_scbank_search_dev(cslam_scbank_t *bank, const double *d_queries, int64_t nq, int num_candidates,
                            const int64_t *d_row_limit, int64_t *d_best_idx, double *d_best_sim,
                            int32_t *d_best_yaw, int64_t *d_cand, double *d_cdist, int32_t *d_cyaw,
                            void *stream);

/* Scan-context descriptor of float64 point clouds (cslam/lidar_pr/scancontext_utils.py:10-75 ptcloud2sc,
 * called by lidar_pr/scancontext.py:14-16 with rings x sectors = 20 x 60, max_length 80).
 * d_points: all frames concatenated, [total_points, 3]; frame f owns rows d_offsets[f] .. d_offsets[f+1]-1.
 * d_out [n_frames, rings*sectors] float64.  NaN points are skipped; a bin keeps the maximum of z + 2 over
 * its first 500 points in cloud order (the reference's storage cap), 0.0 when its storage has unused slots.
 * *d_status (device int32) is a bit set over all frames of the call; a point that sets a bit is skipped:
 *   bit 0: a point has theta == 360 exactly, where the reference raises IndexError;
 *   bit 1: a point's ring or sector index is NaN (x or y infinite, or so large that x*x + y*y overflows), where
 *          the reference raises ValueError ("cannot convert float NaN to integer").
 * The reference raises at the first such point of one cloud; a batch has no such order, so a caller that finds
 * both bits set raises ValueError.  An infinite z alone sets nothing: the bin holds +-inf, as in the reference. */
int cslam_scancontext_from_cloud_dev(const double *d_points, const int64_t *d_offsets, int n_frames,
                                     int rings, int sectors, double max_length, double *d_out,
                                     int32_t *d_status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Lidar loop-closure registration: batched point-to-point ICP.
 * Replaces the refinement of cslam/lidar_pr/icp_utils.py:126-134 (open3d registration_icp(src, dst, voxel_size, T,
 * TransformationEstimationPointToPoint, ICPConvergenceCriteria(max_iteration=100))) for n_pairs (source, target)
 * pairs at once.  Float64 throughout, brute-force nearest neighbours (ties -> lower target index).
 * d_src / d_dst: the clouds concatenated, [total, 3]; pair p owns source rows d_src_off[p] .. d_src_off[p+1]-1 and
 * target rows d_dst_off[p] .. d_dst_off[p+1]-1 (int64, n_pairs + 1 entries each, every cloud at least one point).
 * The offsets are read back once (the only host wait) and every size is checked before anything is launched:
 * CSLAM_E_INVALID on offsets that do not increase, a non-positive or non-finite radius, n_pairs outside [1, 65535].
 * Results do not depend on which other pairs are in the batch (no atomics; every sum has one fixed order).
 * Coordinate range: the clouds may lie anywhere float64 resolves them (map-frame, UTM or ENU coordinates included).  The sums of
 * an update are taken relative to the pair's first target point rounded to a 1024 m grid (zero, and so the sums as written,
 * for clouds around the frame origin), the shifted sets are fitted and the translation is moved back: for clouds of lidar
 * size the moved source points stay within a few ulp of the largest coordinate of an extended-precision centred fit (tested
 * up to 2^20 m: at most 3 ulp; bound of the tests 256).  One correspondence gives R = I and t = q - p exactly.
 *
 * correspondences: one evaluation at d_T ([n_pairs,16] row-major 4x4, NULL = identity).  d_idx[row] = the nearest
 *   target point of T . src[row] (index within the pair's target cloud), -1 where its squared distance exceeds
 *   max_dist^2; d_dist2[row] = that squared distance whether kept or not.  Both [total source rows]. */
int cslam_icp_correspondences_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                                  const int64_t *d_dst_off, int n_pairs, const double *d_T, double max_dist,
                                  int32_t *d_idx, double *d_dist2, void *stream);
/* register: open3d's loop (icp_utils.py:126-134), run as n_stages stages back to back; stage s uses the correspondence
 *   radius max_dist[s] and at most max_iter[s] updates (host arrays), starts from the previous stage's transform
 *   (stage 0 from d_init [n_pairs,16], NULL = identity) and stops a pair when |delta fitness| < rel_fitness and
 *   |delta inlier_rmse| < rel_rmse between two evaluations (absolute differences, open3d's defaults 1e-6).
 *   fitness = correspondences / source points, inlier_rmse = sqrt(sum d^2 / correspondences), both 0 without any.
 *   Everything is enqueued on `stream` without a host wait; finished pairs cost an empty launch per round.
 *   d_T_out [n_pairs,16]: source -> target.  d_stats_out [n_pairs,4]: fitness, inlier_rmse, correspondences and
 *   iterations of the LAST stage. */
int cslam_icp_register_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                           const int64_t *d_dst_off, int n_pairs, const double *d_init, const double *max_dist,
                           const int *max_iter, int n_stages, double rel_fitness, double rel_rmse, double *d_T_out,
                           double *d_stats_out, void *stream);
/* register_plane: the same loop with open3d's TransformationEstimationPointToPlane as the update.  Correspondences, fitness,
 *   inlier_rmse, the stopping rule, the stages and every argument and check are those of cslam_icp_register_dev (open3d
 *   evaluates a registration the same way whatever the estimator); d_dst_normals [total target rows, 3] holds the targets'
 *   normals in the layout of d_dst (NULL: CSLAM_E_INVALID, "d_dst_normals is NULL").  cslam_normals_dev computes them.
 *   The update, float64 throughout (csrc/plane.h), for the kept correspondences (p = T . src_i, q its target point, n the
 *   normal at q):
 *     r = (p - q) . n,   J = [(p - o) x n, n],   A = sum J J^T,   b = sum J r   (29 sums per block: n, sum d^2, the 21
 *     upper-triangle entries of A, the 6 of b; the same fixed shuffle tree and block order as the 17 of the rigid fit,
 *     no float atomics: a pair's result is the same bits alone or in any batch),
 *   o the pair's sum origin as above (zero for clouds around the frame origin: the sums are then open3d's as written).
 *   The shift is needed: p x n of frame coordinates far from the origin couples the rotation and translation columns of
 *   A (condition 2.8e3 at the origin, 7.8e18 for the same clouds at (2^17, -2^16, 1024) m); det A is the same in both frames.
 *   Solve: x = -A^-1 b by an unpivoted LDL^T of the symmetric 6 x 6, det A = the product of D.  The update is the
 *     IDENTITY when fewer than six correspondences are kept (rank A < 6: det A = 0 exactly), a pivot is exactly 0, det A is
 *     NaN, infinite or |det A| < 1e-6, or the solution is not finite.  This restates the determinant check of open3d's
 *     SolveLinearSystemPSD from memory; no open3d is available to pin it against, so parity with open3d is NOT pinned.
 *   Compose: U' = (Rz(x2) . Ry(x1) . Rx(x0), (x3, x4, x5)) (open3d's TransformVector6dToMatrix4d), the translation moved
 *     back to the frame, t = t' + o - R o, and T <- U . T as above.
 *   Known weakness: the 1e-6 threshold is absolute.  A scene with ONE sliding direction (two plane families that share a
 *     line) has a computed determinant far above it and takes whatever step the solve gives; that is open3d's behaviour and
 *     it is kept.  Point-to-plane also has the narrower basin of convergence: from a ScanContext yaw seed (up to 3 degrees
 *     off) run it through coarse stages (4x, 2x, 1x the voxel size), not in one stage at the voxel radius. */
int cslam_icp_register_plane_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                                 const int64_t *d_dst_off, const double *d_dst_normals, int n_pairs,
                                 const double *d_init, const double *max_dist, const int *max_iter, int n_stages,
                                 double rel_fitness, double rel_rmse, double *d_T_out, double *d_stats_out, void *stream);

/* Lidar keyframes: batched voxel down-sampling, the step every keyframe goes through before it is stored
 * (cslam/lidar_pr/icp_utils.py:93-100 `downsample`: drop the rows with a non-finite coordinate, then open3d's
 * voxel_down_sample; called by lidar_handler_node.py:180).  Per cloud, in float64: origin = min over the finite rows
 * - voxel / 2 per axis, voxel index = floor((p - origin) / voxel), one output row per occupied voxel = the sum of its
 * points in cloud order, accumulated one after another from the first, divided once by their number.  Rows come in
 * ascending lexicographic voxel index, x most significant (open3d's own order is that of a hash map).  The result does
 * not depend on which other clouds are in the batch (no float atomics; every sum has one fixed order).
 * d_points: the clouds concatenated, [total, 3]; cloud c owns rows d_offsets[c] .. d_offsets[c+1]-1 (int64,
 *   n_clouds + 1 entries from 0; empty clouds are allowed).  h_offsets: a host copy of the same offsets, or NULL.
 * d_out [total, 3] has the capacity of the input; cloud c's rows are d_out_offsets[c] .. d_out_offsets[c+1]-1
 *   (n_clouds + 1 entries, written on the device).  d_counts: NULL, or [total]: the points of every output row.
 * d_status [n_clouds]: 0, or 1 for a cloud with a voxel index of 2^21 or more on some axis (open3d: "voxel_size is too
 *   small"): it gets no rows.  A cloud without a finite row gets no rows and status 0.
 * CSLAM_E_INVALID, before anything touches HIP: voxel not finite or <= 0, n_clouds outside [1, 65535], host offsets
 *   that do not start at 0 or that decrease (device-only offsets are checked after the wait).
 * Scratch is the library's own, per (device, stream).  The call waits on the host once, after the per-cloud bounds:
 *   it reads the widest voxel key of the batch and whether any row is left out (8 bytes, which select the sort passes),
 *   and the offsets when h_offsets is NULL.  Everything after that is enqueued on `stream` without a wait. */
int cslam_voxel_downsample_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, double voxel,
                               double *d_out, int64_t *d_out_offsets, int32_t *d_counts, int32_t *d_status,
                               const int64_t *h_offsets, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Lidar loop closures: FPFH features and mutual nearest neighbours in feature space, the inputs of a robust fit
 * (cslam/lidar_pr/icp_utils.py:26-65: `extract_fpfh`, `find_knn_cpu`, `find_correspondences`).  The robust fit that consumes
 * them (TEASER++, icp_utils.py:68-83,116-121) is csrc/robust.hip, declared after these.  Float64 throughout, nothing contracted, no
 * float atomics, every sum in one fixed order: a cloud's (a pair's) result does not depend on the rest of the batch.
 * The rules follow open3d's EstimateNormals.cpp and Feature.cpp in structure and fix what those leave to a KD-tree, a
 * hash map or an eigen-solver; parity with open3d itself is not pinned (as for the ICP above).
 * Clouds are batched as for cslam_voxel_downsample_dev: d_points [total, 3], cloud c owns rows d_offsets[c] ..
 * d_offsets[c+1]-1 (int64, n_clouds + 1 entries from 0, empty clouds allowed); h_offsets is a host copy of the offsets
 * or NULL (then they are read back once: the call's only host wait).  Neighbour indices are cloud-local int32.
 * CSLAM_E_INVALID, before anything touches HIP: a radius that is not finite or <= 0, max_nn < 1 (or > 256 for the
 * search), a list width outside [1, 256], dim outside [1, 64], n_clouds / n_pairs outside [1, 65535], NULL arguments,
 * host offsets that do not start at 0, that decrease, or (matching) that leave a feature array without a row.
 *
 * cslam_knn_radius_dev -- the hybrid search of open3d's KDTreeSearchParamHybrid(radius, max_nn) (icp_utils.py:29-30,
 *   35-36), brute force.  The list of point i is i itself first (d^2 = 0), then the other points j of its cloud with
 *   d^2 = fma(dz, dz, fma(dy, dy, dx * dx)) <= radius^2 in ascending (d^2, j), cut to max_nn entries in all; points
 *   that coincide with i are ordinary neighbours at d^2 = 0.  d_idx [total, max_nn] (-1 beyond the count), d_d2
 *   [total, max_nn] (+infinity beyond the count), d_count [total].  Any density is handled: the on-chip candidate buffer
 *   is cut to its best max_nn - 1 whenever it fills. */
int cslam_knn_radius_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, double radius, int max_nn,
                         int32_t *d_idx, double *d_d2, int32_t *d_count, const int64_t *h_offsets, void *stream);
/* cslam_normals_dev -- open3d's estimate_normals (icp_utils.py:28-30) from neighbour lists of width list_width.  It uses
 *   the first min(max_nn, entries with d^2 <= radius^2) entries of a list, i.e. exactly the list of a search at
 *   (radius, max_nn) when the given lists come from a search at least as wide.  With fewer than 3 entries the normal is
 *   (0, 0, 1).  Otherwise: coordinates relative to the query point, their mean in list order, the 3 x 3 covariance of the
 *   centred values in list order divided by the count, and the unit eigenvector of its smallest eigenvalue (cyclic Jacobi).
 *   Sign -- the one deliberate deviation from open3d, which leaves it to its eigen-solver: n . (viewpoint - p) >= 0, and
 *   where that product is exactly 0 the component of largest magnitude is positive.  viewpoint: host [3], NULL = the
 *   origin (keyframe clouds are in the sensor frame).  d_normals [total, 3]. */
int cslam_normals_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, const int32_t *d_idx,
                      const double *d_d2, const int32_t *d_count, int list_width, double radius, int max_nn,
                      const double *viewpoint, double *d_normals, const int64_t *h_offsets, void *stream);
/* cslam_fpfh_dev -- open3d's compute_fpfh_feature (icp_utils.py:32-37) from points, normals and neighbour lists.
 *   Pair features are open3d's ComputePairFeatures, with its swap when acos|n1.d| > acos|n2.d| and the zero vector for
 *   coinciding points or a vanishing cross product; bins floor(11 (f0 + pi) / (2 pi)), floor(11 (f1 + 1) / 2),
 *   floor(11 (f2 + 1) / 2), each clamped to [0, 10].  An SPFH bin is an integer count times 100 / (k - 1), k the list's
 *   count (0 when k <= 1).  FPFH of point i: for the list entries 1 .. k-1 in order with d^2 != 0, acc[j] +=
 *   spfh[j, idx] / d^2 (the weight is the squared distance, as in open3d); s_g = the sum of acc over group g's 11 bins in
 *   ascending j; result acc[j] * (100 / s_g) + spfh[j, i], without the scaling where s_g == 0.
 *   d_fpfh [total, 33]; d_spfh: NULL (the library's scratch is used) or [total, 33], the SPFH. */
int cslam_fpfh_dev(const double *d_points, const double *d_normals, const int64_t *d_offsets, int n_clouds,
                   const int32_t *d_idx, const double *d_d2, const int32_t *d_count, int list_width, double *d_fpfh,
                   double *d_spfh, const int64_t *h_offsets, void *stream);
/* cslam_feature_match_dev -- find_knn_cpu in both directions and the mutual filter of find_correspondences
 *   (icp_utils.py:40-65) for n_pairs pairs of feature arrays: d_a [total_a, dim], d_b [total_b, dim], offsets as above
 *   with at least one row per array.  d_nn01[i] = argmin over the rows j of the pair's b of sum_d (a_d - b_d)^2,
 *   accumulated in ascending d, ties -> the lower j (pair-local index); d_nn10 likewise from b to a.  Brute force.
 *   d_pairs / d_pair_count: both NULL, or [total_a, 2] and [n_pairs]: pair p's rows (i, nn01[i]) with nn10[nn01[i]] == i
 *   in ascending i, written from row d_a_off[p] on, and their number. */
int cslam_feature_match_dev(const double *d_a, const int64_t *d_a_off, const double *d_b, const int64_t *d_b_off,
                            int n_pairs, int dim, int32_t *d_nn01, int32_t *d_nn10, int32_t *d_pairs,
                            int32_t *d_pair_count, const int64_t *h_a_off, const int64_t *h_b_off, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Lidar loop closures: the robust coarse fit from the mutual matches (csrc/robust.hip), the TEASER++ step of
 * `solve_teaser` (cslam/lidar_pr/icp_utils.py:116-121) with the parameters of `get_teaser_solver` (icp_utils.py:68-83):
 * cbar2 = 1, no scale estimation, exact maximum clique, CHAIN graph for the rotation, GNC-TLS with factor 1.4, at most
 * 10000 iterations and cost threshold 1e-16.  Neither TEASER++ nor its source is available where this is built, so parity
 * with TEASER++ itself is not pinned (as for open3d above); the kernels implement the rules written here.  Float64
 * throughout, nothing contracted (but the 4 x 4 eigen-solve shared with the ICP, csrc/horn.h, which is compiled as it is
 * there), no float atomics, every floating sum in one order that depends on the pair's own sizes only: a pair's bytes are
 * the same alone, in any batch and on any run.  c = noise_bound below.
 * The staged entries take the MATCHED points: d_ms / d_md [total, 3], row k of pair p's arrays is the k-th matched source /
 * target point; pair p owns rows d_off[p] .. d_off[p+1]-1 (int64, n_pairs + 1 entries from 0: its capacity) and uses the
 * first d_count[p] of them (int32; d_count NULL = all).  That is the layout cslam_feature_match_dev writes (rows from
 * d_a_off[p] on, d_pair_count[p]).  N = the count; a pair with N > CSLAM_ROBUST_MAX_N is not attempted (it is treated as
 * N = 0 by the stages and gets status 2 from the chained call) and the other pairs are not affected.  Per-pair int32 /
 * float64 arrays "in the capacity layout" have `total` entries and pair p's begin at d_off[p].
 * h_off / h_count: host copies, or NULL; when one that is needed to plan the launch is missing, offsets and counts are
 * read back once (the only host wait of a call).  CSLAM_E_INVALID, before anything touches HIP: n_pairs outside
 * [1, 65535], a noise bound that is not finite or <= 0, a node budget < 1, NULL arguments, host offsets that do not start
 * at 0 or that decrease, host counts that are negative or beyond the capacity.  Scratch is the library's own, per
 * (device, stream). */
#define CSLAM_ROBUST_MAX_N 8192
#define CSLAM_ROBUST_DEFAULT_NODE_BUDGET 2097152
/* cslam_robust_graph_dev -- the consistency graph of TEASER's translation-invariant measurements (the pairwise test of
 *   its inlier selection, icp_utils.py:116-118 `solver.solve`): for i < j, a = sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) of
 *   the two matched source points, b the same of the target points; an edge iff |b - a| <= 2 c (equality is an edge).
 *   d_adj: the N x N bit matrices, pair p's at word d_adj_off[p] (written here, n_pairs + 1 entries: sum of N * W words,
 *   W = ceil(N / 64)), row i = W 64-bit words, bit j of a row = word j / 64, bit j % 64; symmetric, zero diagonal, the
 *   padding bits zero.  d_deg: the degrees, capacity layout.  Nothing is stored per pair of matches. */
int cslam_robust_graph_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_count, int n_pairs,
                           double noise_bound, uint64_t *d_adj, int64_t *d_adj_off, int32_t *d_deg, const int64_t *h_off,
                           const int32_t *h_count, void *stream);
/* cslam_robust_clique_dev -- the exact maximum clique (TEASER's inlier selection, icp_utils.py:116-118; its size is what
 *   solve_teaser compares with min_inliers, icp_utils.py:136).  Core numbers by peeling; vertices ordered by ascending
 *   (core number, index); the GREEDY clique: the vertex of largest core number (the lowest index of equals), then again
 *   and again the common neighbour of those taken with the largest core number (the lowest index of equals).  Then branch
 *   and bound on bitsets, one root vertex per wave: root r looks for the largest clique of r and vertices after it in the
 *   order that beats the greedy one; at a node with clique R and candidates P (taken in ascending order position) the
 *   candidates are coloured greedily and only those of a colour above (best so far of this root, at least the greedy size)
 *   - |R| are branched on.  WHICH CLIQUE WINS: the greedy clique unless a larger one exists; otherwise the largest, and of
 *   equal ones the first that the search of the lowest root in the order meets.  A root's search uses nothing that other
 *   roots find (their sizes only skip whole roots that cannot hold a clique of the largest size), so the result does not
 *   depend on timing whenever the search completes.  node_budget: nodes (colourings) of one pair's search in all; when it
 *   runs out, or a branch would get 512 deep below its root, the pair returns the best clique found (never smaller than
 *   the greedy one) and certified = 0; a search that completes sets certified = 1.  A branch 511 below its root, a clique
 *   of 512, is the deepest that is searched; the best clique found counts what every root recorded until the search
 *   ended, the one that ended it too.  A bit on the diagonal of d_adj is not an edge: no vertex is its own candidate.
 *   d_clique: ascending correspondence indices, capacity layout; d_clique_size, d_certified [n_pairs]; d_nodes: NULL or
 *   [n_pairs], the nodes used. */
int cslam_robust_clique_dev(const uint64_t *d_adj, const int64_t *d_adj_off, const int32_t *d_deg, const int64_t *d_off,
                            const int32_t *d_count, int n_pairs, int64_t node_budget, int32_t *d_clique, int32_t *d_clique_size,
                            int32_t *d_certified, int64_t *d_nodes, const int64_t *h_off, const int32_t *h_count, void *stream);
/* cslam_robust_rotation_dev -- GNC-TLS on the chain of an index list q[0 .. K-1] (d_clique / d_clique_size, as above)
 *   (TEASER's rotation solver, icp_utils.py:75-80,116-118): a_k = ms[q[k+1]] - ms[q[k]], b_k likewise on the targets,
 *   nb2 = 4 c^2 (1e-2 if that is below 1e-16).  w = 1, mu = 1, prev = +inf; for it = 0 .. 9999:
 *   R = argmax sum w_k b_k . (R a_k) over proper rotations (Horn's quaternion form, no centring); r2_k = |b_k - R a_k|^2;
 *   at it == 0: mu = 1 / (2 max r2 / nb2 - 1), stop if mu <= 0; th1 = (mu + 1) / mu nb2, th2 = mu / (mu + 1) nb2,
 *   cost = sum w_k r2_k (old weights); w_k = 0 if r2_k >= th1, 1 if r2_k <= th2, else sqrt(nb2 mu (mu + 1) / r2_k) - mu;
 *   d = |cost - prev|, mu *= 1.4, prev = cost, stop if d < 1e-16.  One launch, one workgroup per pair, no host wait.
 *   d_R [n_pairs, 9] row-major; d_weights: the K - 1 final weights, capacity layout; d_iters [n_pairs]: the weight updates
 *   made (0 when the loop stops at mu <= 0).  K < 2: the identity and 0. */
int cslam_robust_rotation_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_clique,
                              const int32_t *d_clique_size, int n_pairs, double noise_bound, double *d_R, double *d_weights,
                              int32_t *d_iters, const int64_t *h_off, void *stream);
/* cslam_robust_translation_dev -- per-axis TLS (TEASER's translation solver, icp_utils.py:116-121): per axis
 *   x_k = md[q[k]][axis] - ((R0 sx + R1 sy) + R2 sz) with the axis' row of d_R and s = ms[q[k]]; the 2K endpoints x_k -+ c
 *   in ascending (value, index), the 2K - 1 centres midway between consecutive ones; per centre the consensus set
 *   |x_k - centre| <= c, the estimate = its mean (summed in index order), the cost sum_set (x_k - estimate)^2 + c (K - |set|);
 *   a centre with an empty set is left out; the estimate of the lowest cost, ties -> the lower centre.
 *   d_t [n_pairs, 3]; d_set: NULL or [3, total] int32, 1 for the members of the winning set (axis-major, capacity layout). */
int cslam_robust_translation_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_clique,
                                 const int32_t *d_clique_size, const double *d_R, int n_pairs, double noise_bound, double *d_t,
                                 int32_t *d_set, const int64_t *h_off, void *stream);
/* cslam_robust_fit_dev -- the chain (icp_utils.py:116-121) from clouds and correspondence rows: d_src / d_dst and their
 *   offsets as for cslam_icp_register_dev, d_rows [total, 2] int32 (source row, target row; pair-local) with d_row_off /
 *   d_count exactly as cslam_feature_match_dev writes d_pairs / d_pair_count with d_a_off.  A row that points outside its
 *   clouds is consistent with nothing.  Everything runs on the device; the counts are read back once to plan the scratch
 *   unless h_row_off and h_count are given.
 *   d_T [n_pairs, 16]: source -> target.  d_info [n_pairs, 6] int64: status, clique size, rotation iterations, certified,
 *   nodes of the clique search, N.  status 0: solved; 1: fewer than 3 clique members -- the transform is the identity and
 *   there is never a fit (TEASER's own answer there is arbitrary); 2: N above CSLAM_ROBUST_MAX_N, not attempted.
 *   d_clique: NULL, or the clique in the capacity layout. */
int cslam_robust_fit_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst, const int64_t *d_dst_off,
                         const int32_t *d_rows, const int64_t *d_row_off, const int32_t *d_count, int n_pairs, double noise_bound,
                         int64_t node_budget, double *d_T, int64_t *d_info, int32_t *d_clique, const int64_t *h_row_off,
                         const int32_t *h_count, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Visual loop closures: geometric verification of a candidate keyframe pair (csrc/vis.hip, csrc/pnp.h).
 * Replaces the `registration_.computeTransformation(from, to, ...)` calls of src/front_end/rgbd_handler.cpp:433-469
 * (receive_local_keyframe_match, intra-robot) and :493-554 (receive_local_image_descriptors, inter-robot) on keyframes
 * that carry 2D keypoints, their 3D points and their descriptors (:471-491), with frontend.pnp_min_inliers = 20
 * (map_manager_node.cpp:18, rgbd_handler.cpp:72,115-117); stereo_handler.cpp shares the path.  Behind that call is rtabmap's
 * visual registration, taken here at its defaults as nearest-neighbour matching of binary descriptors with a ratio test and
 * 3D -> 2D PnP inside RANSAC (300 iterations, 2 px, refinement on the inliers).  rtabmap and OpenCV are third party and
 * were not available: parity with them is unpinned; tests/vis_reference.py is the float64 yardstick of what is stated here.
 *
 * Convention: T maps points of the "from" camera frame into the "to" camera frame; the 3D points come from "from", the
 * pixels and the intrinsics (fx, fy, cx, cy: pinhole, rectified, no distortion) from "to".  Arrays of a batch are
 * concatenated with int64 offsets [n_pairs + 1]; all floating arrays are float64.  No float atomics: the same input gives
 * the same bytes, alone or in any batch. */
/* cslam_vis_match_dev -- the matching half of computeTransformation (rgbd_handler.cpp:443-445, :519-520).  Descriptors uint8 [n, 32] (desc_bytes must be 32).  Per "from" row the nearest and second-nearest
 *   "to" row by Hamming distance (the lowest index on ties); the row is a match iff n_to >= 2 and d1 <= nndr d2 (in float64);
 *   when several "from" rows claim one "to" row the smallest distance keeps it, then the lowest "from" row.
 *   d_rows [total from, 2] int32 (from row, to row; pair-local) at the pair's "from" offset, ascending in the from row;
 *   d_count [n_pairs] their number.  h_from_off / h_to_off: the offsets on the host (required; they size the launch). */
int cslam_vis_match_dev(const uint8_t *d_desc_from, const int64_t *d_from_off, const uint8_t *d_desc_to, const int64_t *d_to_off,
                        int n_pairs, int desc_bytes, double nndr, int32_t *d_rows, int32_t *d_count, const int64_t *h_from_off,
                        const int64_t *h_to_off, void *stream);
/* cslam_vis_pnp_dev -- the PnP RANSAC half of computeTransformation (rgbd_handler.cpp:443-445, :519-520) with
 *   frontend.pnp_min_inliers (rgbd_handler.cpp:72,115-117), one workgroup per pair.  Correspondence k of pair p is (d_rows[k][0]: a row
 *   of its d_points [., 3], d_rows[k][1]: a row of its d_pixels [., 2]), k < d_count[p] (NULL: all rows of d_row_off).  One
 *   whose row lies outside its arrays or whose point or pixel is not finite (a keypoint without depth) is dropped and
 *   counted; M usable ones remain, in order.
 *   Hypothesis h in [0, iterations): four distinct indices from the stateless sampler of pnp.h on (seed, h, M); Lambda Twist
 *   P3P on the first three; of its roots the one with the smallest reprojection error of the fourth (lowest root on ties);
 *   its inliers: depth > 0 and squared pixel error <= reproj_error^2.  The best hypothesis has the most inliers, then the
 *   lowest h; one without a root counts 0.  Then refine_rounds rounds of { Gauss-Newton on the inlier set (left perturbation,
 *   at most refine_iterations steps, stopping after a step of norm < 1e-10 or on a singular system), recount the inliers }.
 *   d_T [n_pairs, 16] row-major; d_info [n_pairs, 8] int32: status, correspondences given, usable, dropped, final inliers,
 *   best h (-1: not attempted), its inliers, Gauss-Newton steps taken; d_flags [total rows] int32: 1 for the final inliers.
 *   status 3: M above 2048, not attempted, T = identity; else 2: M below max(4, min_inliers), not attempted, T = identity;
 *   else 0: accepted, final inliers >= min_inliers; 1: rejected, T = the best fit found. */
int cslam_vis_pnp_dev(const double *d_points, const int64_t *d_points_off, const double *d_pixels, const int64_t *d_pixels_off,
                      const int32_t *d_rows, const int64_t *d_row_off, const int32_t *d_count, const double *d_cameras, int n_pairs,
                      int iterations, double reproj_error, int min_inliers, int refine_iterations, int refine_rounds, uint64_t seed,
                      double *d_T, int32_t *d_info, int32_t *d_flags, void *stream);
/* cslam_vis_register_dev -- the whole call of rgbd_handler.cpp:443-445 / :519-520: both chained on the stream with no host wait between them: the matches of
 *   (d_desc_from, d_desc_to) select rows of d_points_from [., 3] and d_pixels_to [., 2]; d_rows / d_count as
 *   cslam_vis_match_dev writes them, d_T / d_info / d_flags as cslam_vis_pnp_dev (d_flags in the layout of d_rows). */
int cslam_vis_register_dev(const uint8_t *d_desc_from, const double *d_points_from, const int64_t *d_from_off,
                           const uint8_t *d_desc_to, const double *d_pixels_to, const int64_t *d_to_off, const double *d_cameras,
                           int n_pairs, int desc_bytes, double nndr, int iterations, double reproj_error, int min_inliers,
                           int refine_iterations, int refine_rounds, uint64_t seed, int32_t *d_rows, int32_t *d_count, double *d_T,
                           int32_t *d_info, int32_t *d_flags, const int64_t *h_from_off, const int64_t *h_to_off, void *stream);
/* Level-aware PnP, for keyframes of the scale pyramid below (csrc/pnp.h; tests/vis_levels_reference.py restates it).  A
 *   keypoint of level l is located on an image 1.2^l times coarser, so its pixel error is worth that much less:
 *   sigma2[l] = (double)36^l / (double)25^l for l = 0 .. 7, exact integers and one division.  A correspondence whose "to"
 *   keypoint has level l is an inlier iff its depth is positive and its squared pixel error <= reproj_error^2 sigma2[l]: in
 *   hypothesis scoring, in the inlier set of the best hypothesis and in every recount; each of its 27 Gauss-Newton terms is
 *   multiplied by 1 / sigma2[l].  The sampler, P3P, the selection by the fourth point, the best-hypothesis key, the stopping
 *   rule, the status rules and the limit of 2048 are those of cslam_vis_pnp_dev; with every level 0 the rule is its rule.
 *   Parity with rtabmap's and OpenCV's use of cv::KeyPoint::octave is unpinned like the rest. */
/* cslam_vis_pnp_levels_dev -- the PnP RANSAC half of computeTransformation (rgbd_handler.cpp:443-445, :519-520) in the
 *   level-aware form: cslam_vis_pnp_dev plus d_levels_to int32, the level of every "to" row in the layout of d_pixels
 *   (d_pixels_off).  h_pixels_off and h_levels_to: the same on the host, required: a level outside 0 .. 7 is refused before
 *   any launch. */
int cslam_vis_pnp_levels_dev(const double *d_points, const int64_t *d_points_off, const double *d_pixels, const int64_t *d_pixels_off,
                             const int32_t *d_levels_to, const int32_t *d_rows, const int64_t *d_row_off, const int32_t *d_count,
                             const double *d_cameras, int n_pairs, int iterations, double reproj_error, int min_inliers,
                             int refine_iterations, int refine_rounds, uint64_t seed, double *d_T, int32_t *d_info, int32_t *d_flags,
                             const int64_t *h_pixels_off, const int32_t *h_levels_to, void *stream);
/* cslam_vis_register_levels_dev -- the whole call of rgbd_handler.cpp:443-445 / :519-520 in the level-aware form: the match
 *   of cslam_vis_register_dev, unchanged, then the level-aware PnP on its rows, chained on the stream with no host wait.
 *   d_levels_to / h_levels_to int32 [total to]: the levels of the "to" keypoints. */
int cslam_vis_register_levels_dev(const uint8_t *d_desc_from, const double *d_points_from, const int64_t *d_from_off,
                                  const uint8_t *d_desc_to, const double *d_pixels_to, const int64_t *d_to_off, const int32_t *d_levels_to,
                                  const double *d_cameras, int n_pairs, int desc_bytes, double nndr, int iterations, double reproj_error,
                                  int min_inliers, int refine_iterations, int refine_rounds, uint64_t seed, int32_t *d_rows,
                                  int32_t *d_count, double *d_T, int32_t *d_info, int32_t *d_flags, const int64_t *h_from_off,
                                  const int64_t *h_to_off, const int32_t *h_levels_to, void *stream);
/* Two-view bundle adjustment after PnP (csrc/vis_ba.hip, csrc/ba.h; tests/vis_ba_reference.py restates it).  rtabmap's
 *   computeTransformation, which rgbd_handler.cpp:443-445 and :519-520 call, follows its PnP at its defaults with a local bundle
 *   adjustment over the two views; rtabmap and g2o are third party and were not available: parity with them is unpinned, and
 *   what follows is this library's own rule.
 *   Input per pair: keypoints [., 2], points [., 3] (camera frame), camera (fx, fy, cx, cy), baseline and optional levels of
 *   both keyframes, the match rows, and what PnP wrote for them (T0, its info and flags).  The depth weight of a view is
 *   w = fx * baseline: the real baseline of a stereo camera, a virtual one for RGB-D (the Python default 0.1 m is this
 *   library's choice; parity with rtabmap's value is unpinned).
 *   The adjusted set: the correspondences PnP flagged, in row order, whose rows lie inside their keyframes, whose two keypoints
 *   and "from" X, Y are finite and whose "from" Z is finite and positive with a finite 1 / Z; a flagged row that is not
 *   adjustable gets flag 0.  At most 2048; more (which no PnP status 0 of these entry points precedes): status 3, T0 and PnP's flags.
 *   Unknowns: T = (R, t) from T0, and a point Y_k per member in the "from" camera frame, started at the "from" point.
 *   Residuals of member k with levels la, lb and sigma2[l] = (double)36^l / (double)25^l:
 *     view "from": (fx_a Yx / Yz + cx_a - u_a, fy_a Yy / Yz + cy_a - v_a, w_a (1 / Yz - 1 / Z_a)), squares weighted 1 / sigma2[la];
 *     view "to":   the same of Q = R Y + t, the "to" keypoint, w_b and 1 / sigma2[lb]; the third component only where the
 *                  "to" point's Z is finite and positive (and 1 / Z finite).
 *   Yz <= 0 or Qz <= 0 at the linearisation point: the member adds nothing to that step and its point does not move; it adds
 *   nothing to a cost either.
 *   One step (Gauss-Newton, Schur complement, no damping): per point H_pp (3 x 3), g_p, H_cp (6 x 3) for the left perturbation
 *   T <- Exp(delta) T, delta = [omega, v]; H_pp^-1 = adjugate / determinant.  Pivot rule: a point is free iff det H_pp is finite
 *   and det > 1e-11 * H_pp[0][0] H_pp[1][1] H_pp[2][2]; otherwise it is held fixed for the step and its "to" pixel enters with
 *   the 27 plain PnP terms of the level-aware form.  A free point adds H_cc - H_cp H_pp^-1 H_cp^T and g_c - H_cp H_pp^-1 g_p:
 *   27 sums in the order of cslam_vis_pnp_dev's refinement (member k on lane k mod 256, a fixed shuffle tree per wave, the waves
 *   added in wave order).  delta by the unpivoted LDL^T of pnp.h, T by the left perturbation, then per free point
 *   Y_k <- Y_k - H_pp^-1 (g_p + H_cp^T delta) with the blocks of the same linearisation point.  A round stops after
 *   ba_iterations steps, after a step with |delta| < 1e-10 (taken), or on a singular or non-finite system (not taken).
 *   ba_rounds rounds of { steps; guard; recount }.  Guard: the weighted cost (sum of the weighted squared residuals, no
 *   robust kernel) over the round's starting set, summed in the same fixed order, before and after the steps; if the cost
 *   after is not finite or exceeds (1 + 1e-9) times the cost before, the round is discarded: T and the points go back to the
 *   round's start (the slack is above the rounding of the two sums, so that at a converged start rounding does not decide).
 *   Recount: a member stays iff Yz > 0, Qz > 0 and its squared pixel error is <= reproj_error^2 sigma2[la] in "from" and
 *   <= reproj_error^2 sigma2[lb] in "to", with the refined Y and T.  The set only shrinks.
 *   Status 0: at least min_inliers remain; 1: fewer, T is still the fit found.  A PnP status other than 0, ba_rounds == 0 or
 *   ba_iterations == 0: nothing is adjusted, d_T, d_flags and the status are PnP's byte for byte, no refined points, costs NaN,
 *   both set sizes = PnP's final inliers.
 *   float64, no float atomics: the same input gives the same bytes alone, in any batch, in any order. */
/* cslam_vis_ba_dev -- the adjustment alone (the step of computeTransformation after PnP, rgbd_handler.cpp:443-445, :519-520),
 *   one workgroup per pair.  d_rows / d_row_off / d_count as for cslam_vis_pnp_dev: (row of "from", row of "to").  d_T0 [n, 16],
 *   d_info0 [n, 8], d_flags0 [total rows]: what PnP wrote for these rows.  d_levels_from / d_levels_to int32 in the layout of
 *   the keypoints, NULL = every level 0; the host copy of a given array is required and a level outside 0 .. 7 is refused
 *   before any launch.  d_cameras_from / d_cameras_to [n, 4]; d_baselines / h_baselines [n, 2] (from, to), positive and finite.
 *   Outputs, none of which may be a PnP array: d_T [n, 16]; d_info [n, 8] int32: status, set size in, set size out,
 *   Gauss-Newton steps, rounds discarded, points held fixed (summed over the steps), PnP status, 0; d_flags [total rows] int32;
 *   d_points [total rows, 3]: the refined point, in the "from" frame, of every row whose flag is 1, NaN elsewhere;
 *   d_cost [n, 2]: the cost of the set at (T0, the "from" points), and the cost the last round ended with over its starting set. */
int cslam_vis_ba_dev(const double *d_kp_from, const double *d_points_from, const int64_t *d_from_off, const double *d_kp_to,
                     const double *d_points_to, const int64_t *d_to_off, const int32_t *d_levels_from, const int32_t *d_levels_to,
                     const double *d_cameras_from, const double *d_cameras_to, const double *d_baselines, const int32_t *d_rows,
                     const int64_t *d_row_off, const int32_t *d_count, const double *d_T0, const int32_t *d_info0,
                     const int32_t *d_flags0, int n_pairs, double reproj_error, int min_inliers, int ba_iterations, int ba_rounds,
                     double *d_T, int32_t *d_info, int32_t *d_flags, double *d_points, double *d_cost, const int64_t *h_from_off,
                     const int64_t *h_to_off, const int64_t *h_row_off, const int32_t *h_levels_from, const int32_t *h_levels_to,
                     const double *h_baselines, void *stream);
/* cslam_vis_register_ba_dev -- the whole call of rgbd_handler.cpp:443-445 / :519-520 with the adjustment: match, PnP (the
 *   uniform form where d_levels_to is NULL, the level-aware form otherwise; the PnP camera is d_cameras_to) and the adjustment,
 *   chained on the stream with no host wait.  d_rows / d_count / d_T0 / d_info0 / d_flags0: what cslam_vis_register_dev (or
 *   _levels_dev) writes; the rest as cslam_vis_ba_dev with d_row_off = d_from_off. */
int cslam_vis_register_ba_dev(const uint8_t *d_desc_from, const double *d_kp_from, const double *d_points_from,
                              const int64_t *d_from_off, const uint8_t *d_desc_to, const double *d_kp_to, const double *d_points_to,
                              const int64_t *d_to_off, const int32_t *d_levels_from, const int32_t *d_levels_to,
                              const double *d_cameras_from, const double *d_cameras_to, const double *d_baselines, int n_pairs,
                              int desc_bytes, double nndr, int iterations, double reproj_error, int min_inliers, int refine_iterations,
                              int refine_rounds, uint64_t seed, int ba_iterations, int ba_rounds, int32_t *d_rows, int32_t *d_count,
                              double *d_T0, int32_t *d_info0, int32_t *d_flags0, double *d_T, int32_t *d_info, int32_t *d_flags,
                              double *d_points, double *d_cost, const int64_t *h_from_off, const int64_t *h_to_off,
                              const int32_t *h_levels_from, const int32_t *h_levels_to, const double *h_baselines, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Visual keyframes: corners, steered BRIEF-32 descriptors and 3D points from the image (csrc/feat.hip, csrc/feat.h).
 * Replaces RGBDHandler::compute_local_descriptors of src/front_end/rgbd_handler.cpp:266-312 (grey conversion, depth mask,
 * rtabmap's Feature2D::generateKeypoints, generateDescriptors, generateKeypoints3D), whose result feeds the keyframe
 * decision of generate_new_keyframe (:314-351) and every later computeTransformation.  rtabmap and OpenCV are third party
 * and were not available, and OpenCV's learned ORB / BRIEF sampling tables are not ours to restate: parity with rtabmap's
 * features is unpinned and stays so.  What is pinned is the algorithm stated here, which is integer arithmetic from the
 * image to the descriptors: the GPU, csrc/feat.h on the host and tests/feat_reference.py agree bit for bit.  Matching only
 * needs every robot to use the same rule.
 *
 * A batch is ragged: n images of their own sizes, d_off int64 [n + 1] PIXEL offsets, d_hw int32 [n, 2] = (H, W) with
 * H W = the image's pixels, H, W >= 2.  h_off / h_hw: the same on the host (required; they size the launches).  The result
 * for an image is the same bytes alone or in any batch.  x runs to the right, y downwards; a keypoint is (x, y) int32.
 *
 * Grey: one channel is taken as it is; three are B, G, R: gray = (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * Response (Shi-Tomasi, exact): Ix, Iy = 3 x 3 Sobel on the uint8 image, the border reflected without repeating the edge
 *   pixel (index -1 -> 1, n -> n - 2), |.| <= 1020; a = sum Ix^2, b = sum Ix Iy, c = sum Iy^2 over the 3 x 3 box with the
 *   same border rule applied to the derivative maps; T = a + c, D = (a - c)^2 + 4 b^2 in int64 (<= 4.4e14),
 *   R = T - isqrt(D) with the exact integer floor square root: twice the smaller eigenvalue of the structure matrix,
 *   floored to a unit, in [0, 1.9e7], int32.  Rmax = the maximum over the image.
 * Candidates: a pixel with (double)R > quality_level * (double)Rmax (one multiplication), R >= each of its 8 neighbours
 *   (outside the image: -1), at least `border` pixels from every edge (border <= x <= W - 1 - border; border >= 18 = patch
 *   radius 15 + blur radius 3) and, with a mask or a depth image, valid there.  Their order: R descending, then the pixel
 *   index y W + x ascending (the key (Rmax - R) << 32 | y W + x ascending).
 * Selection = the sequential greedy rule: walk the candidates in that order, accept one iff no candidate accepted earlier
 *   lies nearer than min_distance (dx^2 + dy^2 < min_distance^2 on integers), stop after max_features.
 * Orientation: m10 = sum x I, m01 = sum y I over the disc x^2 + y^2 <= 15^2 around the keypoint on the grey image;
 *   bin = argmax_k (m10 C_k + m01 S_k) in int64, the lowest k on ties; (C_k, S_k), k = 0 .. 7 = (16384, 0), (16069, 3196),
 *   (15137, 6270), (13623, 9102), (11585, 11585), (9102, 13623), (6270, 15137), (3196, 16069); bins 8 .. 31 by exact
 *   quarter turns (c, s) -> (-s, c).
 * Descriptor (steered BRIEF-32): the grey patch blurred by the separable binomial kernel [1, 6, 15, 20, 15, 6, 1] in both
 *   directions, kept as unnormalised integer sums.  The base pattern = 256 point pairs (p, q) from the stateless generator
 *   of feat.h: draw n = splitmix64(0x0BADC0FFEE0DDF00 + n), x = (low 32 bits) mod 27 - 13, y = (high 32 bits) mod 27 - 13,
 *   kept when x^2 + y^2 <= 13^2; a pair = the next two kept points, drawn again when q = p.  The pattern of bin k: each
 *   point rotated by (C, S) of k mod 8, ((x C - y S), (x S + y C)) / 16384 rounded half away from zero in integers, then
 *   k / 8 quarter turns (x, y) -> (-y, x).  Bit i = blur(p_i) < blur(q_i), bit i mod 8 of byte i / 8.
 * Points (generateKeypoints3D): depth float32 metres of the image's size, valid iff finite and > 0; in float64
 *   X = ((u - cx) d) / fx, Y = ((v - cy) d) / fy, Z = d; a keypoint without valid depth gives a NaN row.
 * Out of scope: depth images smaller than the colour image.  Scale pyramids and sub-pixel keypoints: the section after
 *   the stereo keyframes. */
/* cslam_feat_gray_dev -- the grey conversion of rgbd_handler.cpp:266-312.  d_src uint8, image c = the bytes
 *   [d_src_off[c], d_src_off[c + 1]): H W of them (one channel) or 3 H W (B, G, R interleaved).  d_gray uint8 [total pixels]. */
int cslam_feat_gray_dev(const uint8_t *d_src, const int64_t *d_src_off, const int64_t *d_off, const int32_t *d_hw, int n,
                        uint8_t *d_gray, const int64_t *h_src_off, const int64_t *h_off, const int32_t *h_hw, void *stream);
/* cslam_feat_response_dev -- the corner measure inside generateKeypoints (rgbd_handler.cpp:266-312): grey images ->
 *   d_R int32 [total pixels], d_rmax int32 [n]. */
int cslam_feat_response_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, int32_t *d_R, int32_t *d_rmax,
                            const int64_t *h_off, const int32_t *h_hw, void *stream);
/* cslam_feat_select_dev -- the keypoints of generateKeypoints (rgbd_handler.cpp:266-312) from a response map, which is an
 *   input so that a map can be constructed: d_R, d_rmax as above, d_valid NULL or uint8 [total pixels] (0: masked out, the
 *   depth mask of the reference).  quality_level in [0, 1], min_distance in [1, 1024], border >= 18, max_features in
 *   [1, 65535].  d_count int32 [n]; d_kp int32 [n, max_features, 2] = (x, y) and d_resp int32 [n, max_features], the first
 *   d_count[c] rows of image c written. */
int cslam_feat_select_dev(const int32_t *d_R, const int32_t *d_rmax, const uint8_t *d_valid, const int64_t *d_off, const int32_t *d_hw,
                          int n, double quality_level, int min_distance, int border, int max_features, int32_t *d_count, int32_t *d_kp,
                          int32_t *d_resp, const int64_t *h_off, const int32_t *h_hw, void *stream);
/* cslam_feat_describe_dev -- generateDescriptors (rgbd_handler.cpp:266-312): grey images and ragged keypoints d_kp int32
 *   [total, 2] with d_kp_off int64 [n + 1] (h_kp_off: the same on the host, required) -> d_bins int32 [total], d_desc uint8
 *   [total, 32].  A keypoint nearer than 18 pixels to an edge reads nothing: bin -1, descriptor 0. */
int cslam_feat_describe_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                            const int64_t *d_kp_off, int32_t *d_bins, uint8_t *d_desc, const int64_t *h_off, const int32_t *h_hw,
                            const int64_t *h_kp_off, void *stream);
/* cslam_feat_points_dev -- generateKeypoints3D (rgbd_handler.cpp:266-312): d_depth float32 [total pixels], keypoints as
 *   above, d_cameras float64 [n, 4] = (fx, fy, cx, cy) -> d_points float64 [total, 3].  A keypoint outside its image gives
 *   a NaN row. */
int cslam_feat_points_dev(const float *d_depth, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                          const int64_t *d_kp_off, const double *d_cameras, double *d_points, const int64_t *h_off, const int32_t *h_hw,
                          const int64_t *h_kp_off, void *stream);
/* cslam_feat_extract_dev -- the whole of compute_local_descriptors (rgbd_handler.cpp:266-312) on one stream with no host
 *   wait in between: grey, response, selection (depth_as_mask != 0: only pixels of valid depth are candidates), bins and
 *   descriptors, points.  Outputs in the layout of cslam_feat_select_dev: d_count [n], d_kp [n, max_features, 2], d_resp and
 *   d_bins [n, max_features], d_desc [n, max_features, 32], d_points [n, max_features, 3]. */
int cslam_feat_extract_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                           const int32_t *d_hw, const double *d_cameras, int n, double quality_level, int min_distance, int border,
                           int max_features, int depth_as_mask, int32_t *d_count, int32_t *d_kp, int32_t *d_resp, int32_t *d_bins,
                           uint8_t *d_desc, double *d_points, const int64_t *h_src_off, const int64_t *h_off, const int32_t *h_hw,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stereo keyframes: sparse disparity at the keypoints (feat_stereo_kernel in csrc/feat.hip, the rules in csrc/stereo.h).
 * StereoHandler inherits compute_local_descriptors (rgbd_handler.cpp:266-312) unchanged; a stereo frame differs only in
 * where generateKeypoints3D (rgbd_handler.cpp:309) gets depth: the SensorData is built from a left and a right rectified
 * image and a stereo camera model (stereo_handler.cpp:148-227), rtabmap looks each keypoint up in the right image along
 * its row and triangulates from the disparity.  There is no depth image and so no depth mask; a keypoint without a
 * correspondence keeps a NaN point.  Parity with rtabmap's Stereo::computeCorrespondences is unpinned, as for the features
 * above.  What is pinned is the rule stated here: integer arithmetic up to one float64 division, so the GPU, csrc/stereo.h
 * on the host and tests/stereo_reference.py agree bit for bit.
 *
 * Inputs per frame: left and right grey images L, R, uint8, the same H x W, rectified (a point of left column u and
 *   disparity d lies at right column u - d of the same row); keypoints (u, v) int32 in the left image; a camera row of five
 *   float64 (fx, fy, cx, cy, baseline): baseline in metres and > 0, the same principal point in both images.
 * Parameters: 1 <= min_disparity <= max_disparity <= 255 (defaults 1, 128); uniqueness in [0, 100] percent (15);
 *   lr_tolerance in [-1, 255] (1), -1 = no left-right check.  Constants: window half-width 7, half-height 1 (15 x 3).
 * Cost: C(d) = sum over dy = -1 .. 1, dx = -7 .. 7 of (L[v + dy, u + dx] - R[v + dy, u - d + dx])^2, an int32
 *   <= 45 * 255^2 = 2926125 < 2^22; (C << 9) | d is a 31-bit key whose minimum is the best cost, the lowest d among equals.
 * Status, the first rule that applies:
 *   1 outside     not (7 <= u <= W - 8 and 1 <= v <= H - 2).
 *   2 no range    D_lo = min_disparity - 1, D_hi = min(max_disparity + 1, u - 7), and D_hi - D_lo < 2.
 *   3 edge        d* = argmin C over [D_lo, D_hi], the lowest d on ties, is D_lo or D_hi: the disparity lies outside
 *                 [min, max] or the parabola lacks a neighbour.  Constant images land here.
 *   4 not unique  S = min C(d) over the range with |d - d*| >= 2 exists and S * 100 <= C(d*) * (100 + uniqueness) in int64.
 *   5 left-right  only when lr_tolerance >= 0: ur = u - d*, C'(e) = sum (R[v + dy, ur + dx] - L[v + dy, ur + e + dx])^2 over
 *                 e in [D_lo, min(max_disparity + 1, W - 8 - ur)], e* = argmin C', the lowest e on ties, and
 *                 |e* - d*| > lr_tolerance.
 *   0 accepted    otherwise.
 * Disparity (status 0, otherwise NaN): a = C(d* - 1), b = C(d*), c = C(d* + 1), den = a - 2 b + c > 0 (a > b by the tie
 *   rule, c >= b); disparity = (double)d* + (double)(a - c) / (double)(2 den): one division, one addition.
 * Point (status 0, otherwise a NaN row): Z = (baseline fx) / disparity, X = ((u - cx) Z) / fx, Y = ((v - cy) Z) / fy.
 * Diagnostic: best int32 [rows, 4] = (d*, a, b, c); d* = -1 for status 1 and 2; each of a, b, c is -1 where that disparity
 *   lies outside [D_lo, D_hi].
 * Raw pairs are rectified by the raw-camera section below.  Out of scope: different principal points in the two images, a
 *   pyramid inside the correspondence search (the keypoints' scale pyramid: the next section), rtabmap's optical-flow
 *   variant of the correspondence search, Vis/MinDepth and Vis/MaxDepth. */
/* cslam_feat_stereo_dev -- the depth of generateKeypoints3D (rgbd_handler.cpp:309) for a stereo frame
 *   (stereo_handler.cpp:148-227): d_left, d_right uint8 [total pixels] grey in the ragged layout of the feature section
 *   (d_off, d_hw, h_off, h_hw), keypoints d_kp int32 [total, 2] with d_kp_off int64 [n + 1] (h_kp_off: the same on the
 *   host), d_cameras float64 [n, 5] (h_cameras: the same on the host, required: it is checked before the launch) ->
 *   d_disparity float64 [total], d_status int32 [total], d_best int32 [total, 4], d_points float64 [total, 3]. */
int cslam_feat_stereo_dev(const uint8_t *d_left, const uint8_t *d_right, const int64_t *d_off, const int32_t *d_hw, int n,
                          const int32_t *d_kp, const int64_t *d_kp_off, const double *d_cameras, int min_disparity, int max_disparity,
                          int uniqueness, int lr_tolerance, double *d_disparity, int32_t *d_status, int32_t *d_best, double *d_points,
                          const int64_t *h_off, const int32_t *h_hw, const int64_t *h_kp_off, const double *h_cameras, void *stream);
/* cslam_feat_extract_stereo_dev -- compute_local_descriptors for a stereo frame (rgbd_handler.cpp:266-312 with the depth
 *   of :309 from stereo_handler.cpp:148-227) on one stream with no host wait in between: grey of left and right, response
 *   and selection on the left without a mask, bins and descriptors on the left, the stereo rule.  d_left / d_right with
 *   d_left_off / d_right_off as d_src / d_src_off of cslam_feat_gray_dev: the two sides of a frame have the same H x W but
 *   may differ in channels.  Outputs as cslam_feat_extract_dev, plus d_disparity float64 and d_status int32
 *   [n, max_features]. */
int cslam_feat_extract_stereo_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right, const int64_t *d_right_off,
                                  const int64_t *d_off, const int32_t *d_hw, const double *d_cameras, int n, double quality_level,
                                  int min_distance, int border, int max_features, int min_disparity, int max_disparity, int uniqueness,
                                  int lr_tolerance, int32_t *d_count, int32_t *d_kp, int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc,
                                  double *d_points, double *d_disparity, int32_t *d_status, const int64_t *h_left_off,
                                  const int64_t *h_right_off, const int64_t *h_off, const int32_t *h_hw, const double *h_cameras,
                                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * Scale pyramid of the visual keyframes (feat_pyr_level_kernel, feat_pyr_merge_kernel in csrc/feat.hip, the rules in
 * csrc/feat_pyr.h).  compute_local_descriptors (rgbd_handler.cpp:266-312) detects and describes over rtabmap's ORB scale
 * pyramid; the sections above do so at one scale, which cannot verify a loop closure seen from another distance.  Here a
 * frame becomes L images, each an image of its own to the kernels above, and their rows are merged.  Parity with OpenCV's
 * ORB pyramid is unpinned like the rest of the features.  What is pinned is the rule stated here: integer arithmetic up to
 * the final coordinates (one float64 division and one subtraction), so the GPU, csrc/feat_pyr.h on the host and
 * tests/feat_pyramid_reference.py agree bit for bit.  Existing entry points keep their behaviour; levels = 1 gives the rows
 * of cslam_feat_extract_dev.
 *
 * Levels: L = levels in [1, 8], the scale per level 6 / 5.  Level l of an n-pixel axis has n_l = (n 5^l + 6^l / 2) / 6^l
 *   pixels by integer division.  Every level is at least 2 x 2, and for the extraction at least 2 border + 1 on each side;
 *   H, W <= 2^20; n L <= 65535.
 * Resampling: level l from level l - 1 (level 0 is the grey image).  Per axis, for output index x:
 *   u = ((2 x + 1) n_prev 1024) / (2 n_l) - 512 by floor division in int64, clamped to [0, (n_prev - 1) 1024]; i0 = u >> 10,
 *   a = u & 1023, i1 = min(i0 + 1, n_prev - 1); likewise (j0, j1, b) for the row.  Pixel = ((g[j0, i0] (1024 - a) + g[j0, i1] a)
 *   (1024 - b) + (g[j1, i0] (1024 - a) + g[j1, i1] a) b + 2^19) >> 20, which never leaves 0 .. 255.
 * Level 0 under a level pixel: (x, y) of level l lies over the level-0 pixel px = ((2 x + 1) W) / (2 W_l), py likewise,
 *   always inside the image.  With a depth image the validity map of level l is 1 where depth[py, px] is valid (finite
 *   and > 0); it is what the candidate rule above takes as its mask on that level.
 * Detection and description: per level, in level pixels: its own Rmax, the same quality_level, min_distance and border;
 *   orientation and descriptor on the level image.
 * Budget: w_l = 5^l 6^(L - 1 - l); level l gives at most max_features w_l / sum w rows by integer division, level 0 the
 *   remainder as well (1000 over 4 levels: 323, 268, 223, 186).  Budget a level does not use is not passed on.
 * Rows of a frame: level 0 first, then level 1, ...; within a level in selection order.  Keypoint in level-0 coordinates,
 *   float64: kx = (double)((2 x + 1) W) / (double)(2 W_l) - 0.5, ky likewise; at level 0 exactly x.  Point: Z =
 *   (double)depth[py, px], X = ((kx - cx) Z) / fx, Y = ((ky - cy) Z) / fy; an invalid Z gives a NaN row.
 * Layout of the level images: image l n + c = level l of frame c (level-major: the images of a level lie one
 *   after another); d_lvl_hw int32 [n L, 2]; d_lvl_off int64 [n L + 1] PIXEL
 *   offsets in which every image takes its H_l W_l pixels rounded up to a multiple of 4 (a thread of the level kernel
 *   stores 4 pixels as one word).  h_lvl_off / h_lvl_hw: the same on the host, required, and checked against h_hw.
 * Sub-pixel keypoints (the *_subpix_dev chains and cslam_feat_subpixel_dev; tests/feat_subpixel_reference.py restates
 *   them): per axis, from the int32 responses of the level's map R at the keypoint and its two neighbours along the axis,
 *   m (before), c (at), p (after): den = m - 2 c + p and num = m - p in int64.  den >= 0 (a plateau, or no maximum along
 *   the axis) or a neighbour outside the image: off = 0.  Otherwise off = (double)num / (double)(2 den), one division,
 *   clamped to [-0.5, 0.5].  Level-0 coordinate, float64 in exactly this order:
 *   kx = ((double)(2 x + 1) + 2 off) (double)W / (double)(2 W_l) - 0.5, ky likewise; with off = 0 the kx above bit for bit.
 *   No product feeds an addition, so contraction changes no bit.  The integer level-0 pixel (px, py) under the keypoint is
 *   unchanged: depth is read and the stereo rule evaluated there, and the point is the point rule above on the refined
 *   (kx, ky) at that Z.  levels = 1 is the single-scale chain with sub-pixel keypoints.  Parity with OpenCV's cornerSubPix
 *   is unpinned.
 * Out of scope: a scale gate in the match rule (measured on the two-distance scene of the tests: at a factor wide enough
 *   for level quantisation and depth noise, 1.3, it changes nothing), guided re-matching after the fit, dense stereo.
 *   Per-level thresholds in PnP: cslam_vis_pnp_levels_dev above. */
/* cslam_feat_pyramid_dev -- the level images of the pyramid under compute_local_descriptors (rgbd_handler.cpp:266-312):
 *   d_gray uint8 in the ragged layout of the feature section -> d_lvl_gray uint8 [d_lvl_off[n L]] in the level layout.
 *   d_depth NULL, or float32 [total pixels] together with d_lvl_valid uint8 in the level layout: the validity maps, written
 *   in the same passes.  d_lvl_gray and d_lvl_valid start on 4-byte boundaries.  One launch per level, no host wait. */
int cslam_feat_pyramid_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, int levels, const float *d_depth,
                           const int64_t *d_lvl_off, const int32_t *d_lvl_hw, uint8_t *d_lvl_gray, uint8_t *d_lvl_valid,
                           const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw, void *stream);
/* cslam_feat_pyramid_merge_dev -- the per-level keypoints of compute_local_descriptors (rgbd_handler.cpp:266-312) gathered
 *   into the rows of a frame.  Per level image i = l n + c: d_lvl_count int32 [n L], d_lvl_kp int32 [n L, stride, 2] in level
 *   pixels, d_lvl_resp and d_lvl_bins int32 [n L, stride], d_lvl_desc uint8 [n L, stride, 32], d_lvl_z float64 [n L, stride]
 *   = the Z of each keypoint (not finite or <= 0: a NaN point); the first min(d_lvl_count[i], budget of l, stride) rows of an
 *   image are taken.  d_cameras float64 [n, 4].  Outputs: d_count int32 [n], d_kp float64 [n, max_features, 2] level-0
 *   coordinates, d_level_kp int32 [n, max_features, 2], d_levels, d_resp, d_bins int32 [n, max_features], d_desc uint8
 *   [n, max_features, 32], d_points float64 [n, max_features, 3].  Descriptor arrays start on 16-byte boundaries.  No
 *   atomics: a row's position is the exclusive sum of the L counts of its frame. */
int cslam_feat_pyramid_merge_dev(const int32_t *d_lvl_count, const int32_t *d_lvl_kp, const int32_t *d_lvl_resp, const int32_t *d_lvl_bins,
                                 const uint8_t *d_lvl_desc, const double *d_lvl_z, int stride, const int32_t *d_hw,
                                 const int32_t *d_lvl_hw, const double *d_cameras, int n, int levels, int max_features, int32_t *d_count,
                                 double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc,
                                 double *d_points, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw, void *stream);
/* cslam_feat_extract_pyramid_dev -- the whole of compute_local_descriptors (rgbd_handler.cpp:266-312) over the pyramid on
 *   one stream with no host wait in between: grey, the level images (with depth_as_mask != 0 also the validity maps),
 *   response, selection, bins and descriptors on the n L level images, the merge with Z from d_depth.  Arguments as
 *   cslam_feat_extract_dev plus the level layout; outputs as cslam_feat_pyramid_merge_dev. */
int cslam_feat_extract_pyramid_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                                   const int32_t *d_hw, const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                   const int32_t *d_lvl_hw, double quality_level, int min_distance, int border, int max_features,
                                   int depth_as_mask, int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels,
                                   int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points, const int64_t *h_src_off,
                                   const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                                   void *stream);
/* cslam_feat_extract_stereo_pyramid_dev -- compute_local_descriptors for a stereo frame (rgbd_handler.cpp:266-312 with the
 *   depth of :309 from stereo_handler.cpp:148-227) over the pyramid: the chain above on the left image without a mask; the
 *   stereo rule runs at the integer level-0 pixel (px, py) under each keypoint on the level-0 greys, and the Z it gives
 *   goes into the point rule above at (kx, ky); a rejected keypoint keeps its NaN row.  Arguments as
 *   cslam_feat_extract_stereo_dev plus the level layout; outputs as cslam_feat_pyramid_merge_dev plus d_disparity float64
 *   and d_status int32 [n, max_features]. */
int cslam_feat_extract_stereo_pyramid_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right,
                                          const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw, const double *d_cameras,
                                          int n, int levels, const int64_t *d_lvl_off, const int32_t *d_lvl_hw, double quality_level,
                                          int min_distance, int border, int max_features, int min_disparity, int max_disparity,
                                          int uniqueness, int lr_tolerance, int32_t *d_count, double *d_kp, int32_t *d_level_kp,
                                          int32_t *d_levels, int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points,
                                          double *d_disparity, int32_t *d_status, const int64_t *h_left_off, const int64_t *h_right_off,
                                          const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                                          const double *h_cameras, void *stream);

/* cslam_feat_subpixel_dev -- the sub-pixel step behind generateKeypoints (rgbd_handler.cpp:266-312; rtabmap refines corners
 *   with cornerSubPix), staged: response maps d_R int32 [total pixels] as a ragged batch (d_off, d_hw as in the feature
 *   section: level images are images of their own), integer keypoints d_kp int32 [total, 2] with d_kp_off int64 [n + 1]
 *   (h_kp_off: the same on the host) -> d_offsets float64 [total, 2] = (off x, off y).  A keypoint outside its image gives
 *   (0, 0).  A thread per keypoint, five loads, no atomics. */
int cslam_feat_subpixel_dev(const int32_t *d_R, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                            const int64_t *d_kp_off, double *d_offsets, const int64_t *h_off, const int32_t *h_hw,
                            const int64_t *h_kp_off, void *stream);
/* cslam_feat_extract_pyramid_subpix_dev -- compute_local_descriptors (rgbd_handler.cpp:266-312) over the pyramid with
 *   sub-pixel keypoints: cslam_feat_extract_pyramid_dev, whose host function it shares, plus d_offsets float64
 *   [n, max_features, 2], the offsets of every row in level pixels.  d_kp and d_points hold the refined coordinates; every
 *   other output equals the chain without it byte for byte. */
int cslam_feat_extract_pyramid_subpix_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                                          const int32_t *d_hw, const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                          const int32_t *d_lvl_hw, double quality_level, int min_distance, int border, int max_features,
                                          int depth_as_mask, int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels,
                                          int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_offsets,
                                          const int64_t *h_src_off, const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off,
                                          const int32_t *h_lvl_hw, void *stream);
/* cslam_feat_extract_stereo_pyramid_subpix_dev -- compute_local_descriptors for a stereo frame (rgbd_handler.cpp:266-312,
 *   stereo_handler.cpp:148-227) over the pyramid with sub-pixel keypoints: cslam_feat_extract_stereo_pyramid_dev plus
 *   d_offsets as above.  The stereo rule still runs at the integer level-0 pixel under each keypoint. */
int cslam_feat_extract_stereo_pyramid_subpix_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right,
                                                 const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw,
                                                 const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                                 const int32_t *d_lvl_hw, double quality_level, int min_distance, int border,
                                                 int max_features, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance,
                                                 int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp,
                                                 int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_disparity, int32_t *d_status,
                                                 double *d_offsets, const int64_t *h_left_off, const int64_t *h_right_off,
                                                 const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off,
                                                 const int32_t *h_lvl_hw, const double *h_cameras, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Dense stereo: the rule above at every pixel of a rectified pair, and the keyframe cloud made from it
 * (csrc/stereo_dense.hip, its tile plan and bookkeeping in csrc/stereo_dense.h, the rule itself csrc/stereo.h's).  The
 * reference sends no cloud for a stereo frame (stereo_handler.cpp has no depth image to hand to
 * send_visualization_pointcloud, rgbd_handler.cpp:665-682); this is what gives stereo robots the map of csrc/cloud.hip.
 * Pinned: a pixel's status, best and float64 disparity are the bits cslam_feat_stereo_dev gives for a keypoint at that
 * pixel, for every admitted parameter value; tests/stereo_dense_reference.py restates the dense form in numpy (cost slab by
 * prefix sums, one back search per right pixel, the rival among the four smallest keys) and agrees bit for bit.  Unpinned:
 * parity with rtabmap's or OpenCV's dense matchers (StereoBM / StereoSGBM).
 * Raw pairs are rectified by the section below.  Out of scope: different principal points, pyramids, speckle and median
 * post-filters.
 *
 * cslam_stereo_dense_dev -- d_left, d_right uint8 grey [total pixels] in the ragged layout of the feature section, d_cameras
 *   float64 [n, 5] (h_cameras required), parameters as cslam_feat_stereo_dev, whose argument checks these are, all before any
 *   launch ->  d_status uint8 [total]; d_disparity float32 [total] = the float64 disparity rounded once, NaN unless accepted;
 *   d_depth float32 [total] = (baseline fx) / disparity in float64 rounded once, metres, NaN unless accepted (the float32
 *   depth of cslam_cloud_keyframes_dev, where a non-finite depth is an invalid pixel); d_best int32 [total, 4] = (d*, a, b, c)
 *   as cslam_feat_stereo_dev reports it, may be NULL.  No atomics; a frame's bytes are the same alone or in any batch.
 *   Everything is enqueued on `stream`; scratch is 6 bytes per pixel of the library's own.
 * cslam_cloud_keyframes_stereo_dev -- what send_visualization_pointcloud would publish for a stereo frame, on one stream with
 *   the one host wait of cslam_cloud_keyframes_dev: cslam_feat_gray_dev of both sides (d_left / d_right with d_left_off /
 *   d_right_off as d_src / d_src_off there; every left image has `channels` channels, 1 or 3, the right ones 1 or 3 each),
 *   cslam_stereo_dense_dev, then cslam_cloud_keyframes_dev on the left image's colours, the float32 depth and the cameras'
 *   (fx, fy, cx, cy): the same bytes as the staged calls, the same result buffers. */
int cslam_stereo_dense_dev(const uint8_t *d_left, const uint8_t *d_right, const int64_t *d_off, const int32_t *d_hw, int n,
                           const double *d_cameras, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance,
                           float *d_disparity, uint8_t *d_status, float *d_depth, int32_t *d_best, const int64_t *h_off,
                           const int32_t *h_hw, const double *h_cameras, void *stream);
int cslam_cloud_keyframes_stereo_dev(const uint8_t *d_left, const int64_t *d_left_off, int channels, const uint8_t *d_right,
                                     const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw, const double *d_cameras,
                                     int n, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance, double leaf,
                                     double max_range, float *d_out, uint32_t *d_out_rgb, int32_t *d_counts, int64_t *d_out_offsets,
                                     int32_t *d_status, const int64_t *h_left_off, const int64_t *h_right_off, const int64_t *h_off,
                                     const int32_t *h_hw, const double *h_cameras, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Raw cameras: undistort and rectify images and depth (csrc/rectify.hip, the rule csrc/rectify.h's).  Replaces image_proc's
 * and stereo_image_proc's rectify in front of the reference, that is OpenCV initUndistortRectifyMap + remap
 * (stereo_handler.cpp:120 hard-codes alreadyRectified = true): the step between a camera driver's frame with its
 * CameraInfo and every visual stage above.
 * A raw camera is 26 float64: K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3, k4, k5, k6), R row-major 3 x 3,
 * P = (fx', fy', cx', cy') and P[0][3] = Tx fx', which the map ignores.  The rule, in float64 with every operation rounded
 * on its own: x = (u - cx') / fx', y = (v - cy') / fy', (X, Y, Wd) = R^T (x, y, 1), outside unless Wd > 0, xn = X / Wd,
 * yn = Y / Wd, r2 = xn xn + yn yn, rad = (1 + k1 r2 + k2 r4 + k3 r6) / (1 + k4 r2 + k5 r4 + k6 r6),
 * xd = xn rad + 2 p1 xn yn + p2 (r2 + 2 xn xn), yd = yn rad + p1 (r2 + 2 yn yn) + 2 p2 xn yn, m = (fx xd + cx, fy yd + cy),
 * q = floor(32 m + 0.5) as int32, both INT32_MIN when outside, not finite or |q| >= 2^26.
 * Pinned: tests/rectify_reference.py restates map, bilinear and nearest sampling in numpy and agrees bit for bit.
 * Unpinned: parity with OpenCV / image_proc (fixed-point tables, border handling), which were not available to compare.
 * Out of scope: different principal points of the two sides, computing R and P from an extrinsic calibration (Bouguet;
 * CameraInfo carries them), fisheye / equidistant models.
 *
 * cslam_rectify_map_dev -- d_cameras float64 [n, 26] (h_cameras required: finite, positive focal lengths, R orthonormal to
 *   1e-9 with positive determinant), destination sizes d_hw / d_off in the ragged layout of the feature section ->
 *   d_map int32 [total, 2] = (qx, qy).  A thread per pixel, no atomics.
 * cslam_rectify_remap_dev -- n frames; frame c reads d_src + d_src_off[c] (uint8, d_src_hw[c] = (Hs, Ws), 1 channel or 3
 *   interleaved by its length), goes through map d_map_index[c] of the n_maps maps at d_map_off (pixels; the map's size is
 *   the frame's d_hw[c]) and writes its channels at d_dst + d_dst_off[c] (bytes) and d_valid uint8 [total] at d_off[c].
 *   Bilinear on the 1/32 grid: x0 = qx >> 5, ax = qx & 31, weights (32 - ax)(32 - ay), ..., a tap outside contributes 0,
 *   value = (sum + 512) >> 10, valid = 1 iff every tap of non-zero weight lies inside.  A frame's bytes are the same alone, in
 *   any batch and in any order.
 * cslam_rectify_nearest_dev -- the same for depth, never interpolated: src_type CSLAM_RECTIFY_U16 or CSLAM_RECTIFY_F32,
 *   offsets in elements, the element at ((qx + 16) >> 5, (qy + 16) >> 5) with its bits preserved, 0 outside; d_dst in the
 *   layout of d_off.  d_mask uint8 [total] may be NULL; where it is 0 the output is 0 (the validity of the colour image,
 *   so that the depth mask of cslam_feat_extract_dev drops what the image does not cover).
 * All host copies are required, every check precedes the launch, everything is enqueued on `stream`. */
#define CSLAM_RECTIFY_U16 0
#define CSLAM_RECTIFY_F32 1
int cslam_rectify_map_dev(const double *d_cameras, const int64_t *d_off, const int32_t *d_hw, int n, int32_t *d_map,
                          const int64_t *h_off, const int32_t *h_hw, const double *h_cameras, void *stream);
int cslam_rectify_remap_dev(const uint8_t *d_src, const int64_t *d_src_off, const int32_t *d_src_hw, const int32_t *d_map,
                            const int64_t *d_map_off, const int32_t *d_map_index, int n_maps, const int64_t *d_off,
                            const int32_t *d_hw, int n, uint8_t *d_dst, const int64_t *d_dst_off, uint8_t *d_valid,
                            const int64_t *h_src_off, const int32_t *h_src_hw, const int64_t *h_map_off, const int32_t *h_map_hw,
                            const int32_t *h_map_index, const int64_t *h_off, const int32_t *h_hw, const int64_t *h_dst_off,
                            void *stream);
int cslam_rectify_nearest_dev(const void *d_src, int src_type, const int64_t *d_src_off, const int32_t *d_src_hw,
                              const int32_t *d_map, const int64_t *d_map_off, const int32_t *d_map_index, int n_maps,
                              const int64_t *d_off, const int32_t *d_hw, int n, const uint8_t *d_mask, void *d_dst,
                              const int64_t *h_src_off, const int32_t *h_src_hw, const int64_t *h_map_off, const int32_t *h_map_hw,
                              const int32_t *h_map_index, const int64_t *h_off, const int32_t *h_hw, void *stream);

/* Winograd F(2x2, 3x3) transforms for the 3x3 / stride 1 / pad 1 convolutions of the extractor backbone
 * (the VGG-16 trunk built at cslam/vpr/netvlad.py:163-171; the reference runs it through torch's direct
 * convolution).  Activations are NHWC float32.  conv(x, g) + bias = output(bmm(input(x), U)) with
 * U[xi][ci][co] = (G g G^T)[xi]; the 16 GEMMs V[xi] (T x C) . U[xi] (C x Cout) are plain library GEMMs.
 *   input : x [B,H,W,C] -> V [16, T, C], T = B*ceil(H/2)*ceil(W/2) (tiles may hang over an odd map), C % 4 == 0
 *   output: M [16, T, C] -> y [B,H,W,C], or [B,floor(H/2),floor(W/2),C] when pool != 0 (the MaxPool2d(2,2) that follows
 *           the layer fused in); bias [C] or NULL; residual (NULL, or an NHWC tensor shaped like y, pool == 0:
 *           the shortcut of a ResNet block, cosplace_utils/network.py:39-56) is added before the activation;
 *           relu != 0 applies max(., 0) before the pooling. */
/* bias + ReLU (+ MaxPool2d(2,2)) in one pass over an NHWC activation, for the layers left on the direct
 * convolution: y = pool(relu(x + bias)).  Without pooling y may be x (in place); with pooling y is
 * [B,H/2,W/2,C]. */
int cslam_bias_act_pool_dev(const float *d_x, const float *d_bias, int B, int H, int W, int C, int relu,
                            int pool, float *d_y, void *stream);
/* First backbone layer (3 input channels): y = relu(conv3x3(x, w) + bias), stride 1, zero padding 1.
 * x [B,3,H,W] planar (the output of cslam_preprocess_dev), wt [27, Cout] = weight[co][ci][kh][kw] transposed
 * to [(ci*3+kh)*3+kw][co], y [B,H,W,Cout] NHWC. */
int cslam_conv3x3_c3_dev(const float *d_x, const float *d_wt, const float *d_bias, int B, int H, int W,
                         int Cout, int relu, float *d_y, void *stream);
int cslam_wino_input_dev(const float *d_x, int B, int H, int W, int C, float *d_V, void *stream);
int cslam_wino_output_dev(const float *d_M, const float *d_bias, const float *d_residual, int B, int H, int W,
                          int C, int relu, int pool, float *d_y, void *stream);
/* F(4x4, 3x3) variant: 6x6 input tiles, V / M [36, T, C] with T = B*ceil(H/4)*ceil(W/4) (ragged maps allowed), C even.
 * 4x fewer multiplications than the direct form, about one decimal digit less accurate than F(2x2, 3x3). */
int cslam_wino4_input_dev(const float *d_x, int B, int H, int W, int C, float *d_V, void *stream);
int cslam_wino4_output_dev(const float *d_M, const float *d_bias, const float *d_residual, int B, int H, int W,
                           int C, int relu, int pool, float *d_y, void *stream);
/* Split-fp16 form of the 36 per-frequency GEMMs of the same layer (opt-in; same fp32-grade result, fp16 MFMA rate):
 * a float times a power of two is split exactly into an fp16 pair hi + lo, and V U = vh uh + vl uh + vh ul is ONE fp16
 * GEMM with fp32 accumulation over K' = 3 C:  V3 [36, T, 3 C] fp16 rows = [vh | vl | vh],  U3 [36, 3 C, Cout] = [uh ; uh ; ul].
 * cslam_absmax_dev: *d_slot = bits of max |x| (n a multiple of 4); the V scale sV = 2^floor(log2(2^15 / (100 max|x|))) is
 * derived from it on the device by both transforms.  cslam_wino4_output_scaled_dev: as cslam_wino4_output_dev on
 * M' = sV sU M, multiplied by inv_su / sV (inv_su = 1 / sU, a power of two: exact) before bias / residual / ReLU
 * (d_amax NULL: M unscaled, inv_su ignored); d_amax_out (or NULL): atomic max of the bits of max |y| before pooling --
 * the next layer's d_amax without another pass over y; the caller zeroes it beforehand. */
int cslam_absmax_dev(const float *d_x, int64_t n, unsigned *d_slot, void *stream);
int cslam_wino4_output_scaled_dev(const float *d_M, const float *d_bias, const float *d_residual, int B, int H, int W,
                                  int C, int relu, int pool, const unsigned *d_amax, float inv_su, unsigned *d_amax_out,
                                  float *d_y, void *stream);
/* ---- split-fp16 Winograd GEMM of this library (csrc/wino_gemm.hip) ------------------------------------------------
 * The 36 per-frequency products M[xi] = V[xi] U[xi] of the F(4x4,3x3) form of the trunk's wide 3x3 convolutions
 * (the Conv2d layers of cslam/vpr/netvlad.py:163-171 / cosplace_utils/network.py:38-68) on the fp16 matrix pipe with
 * fp32-grade results: both operands are exact fp16 pairs hi + lo of the (power-of-two scaled) float32 values and
 * vh uh + vl uh + vh ul is accumulated in fp32.  Operand layout, both sides: row r = Cin/32 blocks of 128 bytes,
 * block kb = [hi of channels 32 kb .. 32 kb + 31 | lo of the same] as fp16; V2 [36][T][Cin/32][64] (rows = tiles),
 * U2 [36][Cout][Cin/32][64] (rows = OUTPUT channels, i.e. U transposed).
 * cslam_wino4_input_h2_dev: x [B,H,W,C] NHWC float32 -> V2 (scaled by the power of two derived from *d_amax, the bits
 *   of a bound of max |x|, see cslam_absmax_dev above); C a multiple of 32.
 * cslam_wino_gemm_h2_dev: M [36][T][Cout] float32 = (sV V)(sU U); Cin a multiple of 32, Cout of 128.  The result carries
 *   the two scales; cslam_wino4_output_scaled_dev removes them. */
int cslam_wino4_input_h2_dev(const float *d_x, int B, int H, int W, int C, const unsigned *d_amax, void *d_V2,
                             void *stream);
int cslam_wino_gemm_h2_dev(const void *d_V2, const void *d_U2, int64_t T, int Cin, int Cout, float *d_M, void *stream);
/* Output transform of layer L chained into the input transform of layer L + 1 on the same map (csrc/wino_chain.hip): what
 * cslam_wino4_output_scaled_dev (ReLU, no pool, no residual) followed by cslam_wino4_input_h2_dev compute, with y_L kept in LDS.
 * d_M [36][T][C] of layer L (C a multiple of 32, W <= 64); *d_vscale = the slot V_L was scaled by, inv_su as above;
 * V2 of layer L + 1 is scaled by the power of two derived from the bound  *d_amax_x * wl1 + bmax  (*d_amax_x = bits of max |x_L|,
 * wl1 = largest L1 norm of an output channel of layer L's 3x3 weights, bmax = max |bias|), which is stored in *d_bound_out: the
 * d_amax of layer L + 1's output stage.  d_amax_out (zeroed by the caller) receives the bits of the measured max |y_L|. */
int cslam_wino4_chain_h2_dev(const float *d_M, const float *d_bias, int B, int H, int W, int C, const unsigned *d_vscale,
                             float inv_su, const unsigned *d_amax_x, float wl1, float bmax, unsigned *d_amax_out,
                             unsigned *d_bound_out, void *d_V2, void *stream);
/* The same products with the column half of the output transform Y = A^T M A folded in (the "Z form", for the layers whose
 * product is HBM-bound, Cin <= 256): d_Z [24][T][Cout] float32, plane 4 i + q = sum_j M[6 i + j] A^T[q][j] -- 2/3 of M's bytes
 * written and read.  cslam_wino4_output_z_dev finishes: Y[p][q] = sum_i A^T[p][i] Z_i[q], then the epilogue of
 * cslam_wino4_output_scaled_dev (no residual input). */
int cslam_wino_zgemm_h2_dev(const void *d_V2, const void *d_U2, int64_t T, int Cin, int Cout, float *d_Z, void *stream);
int cslam_wino4_output_z_dev(const float *d_Z, const float *d_bias, int B, int H, int W, int C, int relu, int pool,
                             const unsigned *d_amax, float inv_su, unsigned *d_amax_out, float *d_y, void *stream);

/* The one-kernel F(4x4,3x3) convolution of the 64-input-channel layers (64 -> 64 / 128: VGG-16 conv1_2 and conv2_1,
 * netvlad.py:163-171 + the call at :227; the BasicBlock convolutions of ResNet-18/34 layer1, cosplace_utils/network.py:38-68,
 * with d_residual = the block's shortcut) -- input transform, the 36 products and output transform + bias + ReLU
 * (+ MaxPool2d(2,2)) with V and M kept on the compute unit; x [B,H,W,64] NHWC, y [B,H,W,Cout] or pooled -- on the fp16
 * matrix pipe with fp32-grade results (csrc/wino_fused_h.hip): V and U as exact fp16 pairs packed [hi | lo << 16] per
 * value, two v_mfma_f32_16x16x32_f16 per frequency and 16-channel quarter.  d_Uh = U [36,64,Cout] of the F(4x4) form,
 * scaled by the power of two sU, split and permuted to [kq 4][xi 36][w Cout/16][g 4][c 16][s 4] uint32 with
 * Uh[kq][xi][w][g][c][s] = pack(U[xi][16 kq + 4 g + s][16 w + c]) (vpr/winograd.py `fused64_pair_weights`), inv_su = 1/sU;
 * *d_amax = float bits of (a bound of) max |x| (fixes the power-of-two scale of V, as cslam_wino4_input_h2_dev);
 * d_amax_out (optional, zeroed by the caller) receives the bits of max |y| before pooling.  B H W 64 < 2^31. */
int cslam_wino4_fused_c64_h_dev(const float *d_x, const void *d_Uh, const float *d_bias, const float *d_residual, int B,
                                int H, int W, int Cout, int relu, int pool, const unsigned *d_amax, float inv_su,
                                unsigned *d_amax_out, float *d_y, void *stream);
/* The direct (non-Winograd) one-kernel form of the same convolution for 128 output channels (csrc/conv_direct_h.hip; VGG-16
 * conv2_1, conv2_2 of cslam/vpr/netvlad.py:163-171,227): an implicit GEMM over the 9 taps on exact fp16 pairs (three products,
 * fp32 accumulate: fp32-grade), the 18 x 18 input patch of a 16 x 16-pixel block read once into LDS, the output written once --
 * HBM sees activation in + out only.  x [B][H][W][Cin] float32 (Cin a multiple of 32), y [B][H | H/2][W | W/2][128];
 * d_w2 = [9 taps][128][Cin/32][hi 32 | lo 32] halfs of s_w w (cslam_amd/vpr/winograd.py `direct_pair_weights`), inv_sw = 1 / s_w;
 * d_amax: 4-byte slot with (a bound of) max |x|; d_amax_out (or NULL): zeroed slot receiving max |y|. */
int cslam_conv3x3_direct_h_dev(const float *d_x, const void *d_w2, const float *d_bias, int B, int H, int W, int Cin, int Cout,
                               int relu, int pool, const unsigned *d_amax, float inv_sw, unsigned *d_amax_out, float *d_y,
                               void *stream);
/* cslam_conv3x3_c3_dev that also delivers max |y| (float bits, into the zeroed 4-byte slot d_amax_out; NULL = off):
 * the first trunk layer feeds the scale of the fused fp16 layer behind it without a separate pass over its output. */
int cslam_conv3x3_c3_amax_dev(const float *d_x, const float *d_wt, const float *d_bias, int B, int H, int W, int Cout,
                              int relu, float *d_y, unsigned *d_amax_out, void *stream);

/* The same kernel with the trunk's FIRST convolution folded in (VGG-16 conv1_1 -> conv1_2, cslam/vpr/netvlad.py:163-171,227):
 * y = [MaxPool2d](ReLU(conv3x3_{64->64}(ReLU(conv3x3_{3->64}(x0) + b1)) + bias)).  d_x0: planar image batch [B][3][H][W] f32;
 * d_w1 / inv_sw / d_sumw: the first layer's weights as packed fp16 pairs, the inverse of their power-of-two scale, and
 * sum |w| per output channel [64] (`stem_pair_weights` in cslam_amd/vpr/winograd.py); d_amax_x0: 4-byte slot holding the bits of
 * max |x0|; the 64-channel intermediate never exists in HBM.  d_Uh / inv_su / d_amax_out / d_y as in cslam_wino4_fused_c64_h_dev. */
int cslam_wino4_stem_c64_h_dev(const float *d_x0, const void *d_w1, const float *d_b1, const float *d_sumw, float inv_sw,
                               const void *d_Uh, const float *d_bias, int B, int H, int W, int pool,
                               const unsigned *d_amax_x0, float inv_su, unsigned *d_amax_out, float *d_y, void *stream);

/* Strided / 1x1 / 7x7 convolution of the ResNet trunks (cslam/vpr/cosplace_utils/network.py:38-68: torchvision ResNet-18 without
 * avgpool / fc, CosPlace's default backbone, cslam/vpr/cosplace.py:81-101) as an implicit GEMM on exact fp16 pairs
 * (csrc/conv_igemm.hip): y = act(conv(x, w) + bias (+ res)), x [B,H,W,Cin] NHWC float32 -> y [B,Ho,Wo,Cout] NHWC float32,
 * Ho = (H + 2 pad - KH) / stride + 1; BatchNorm folded into w / bias by the caller.  Cin a multiple of 32, or 3 with 3 KW <= 32 (the
 * 7x7 stem); Cout a multiple of 64.  d_w2 = `igemm_pair_weights(weight)` (cslam_amd/vpr/winograd.py): rows = output channels, K blocks
 * of 32 channels as [hi 32 | lo 32] fp16 in (kh, kw, Cin / 32) order (stem: one block per kernel row, slot kw * 3 + c); inv_sw = the
 * inverse of the weights' power-of-two scale.  d_res: optional shortcut, y's shape.  d_amax_in: 4-byte slot with the float bits of
 * (a bound of) max |x|; d_amax_out: optional zeroed slot that receives max |y|.  Replaces torch.nn.functional.conv2d there. */
int cslam_conv_igemm_h2_dev(const float *d_x, const void *d_w2, const float *d_bias, const float *d_res, int B, int H, int W,
                            int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, const unsigned *d_amax_in,
                            float inv_sw, unsigned *d_amax_out, float *d_y, void *stream);
/* the ResNet stem with its pooling, MaxPool2d(3, 2, 1)(ReLU(conv(x, w) + bias)): x [B,H,W,3] -> y [B,Ho/2,Wo/2,Cout], Ho a multiple
 * of 8 and Wo of 16; the un-pooled map never exists in HBM (conv1, bn1 folded, relu, maxpool of the torchvision trunk that
 * cslam/vpr/cosplace_utils/network.py:38-68 builds); d_amax_out receives max of the un-pooled map (a bound) */
int cslam_conv_stem_pool_igemm_h2_dev(const float *d_x, const void *d_w2, const float *d_bias, int B, int H, int W, int Cout,
                                      int KH, int KW, int stride, int pad, const unsigned *d_amax_in, float inv_sw,
                                      unsigned *d_amax_out, float *d_y, void *stream);
/* the same convolution between PAIR-FORMAT activations (csrc/conv_igemm.hip): a tensor [B,H,W,C], C a multiple of 32, whose every
 * (pixel, 32-channel block) is 128 bytes [hi 32 | lo 32] fp16 of s x, s = the power of two that brings the tensor's 4-byte bound slot
 * into [2^13, 2^14) -- written once by the producing layer's epilogue, read by LDS-DMA (same bytes as float32; the format never
 * leaves the trunk: the BasicBlock chain of cslam/vpr/cosplace_utils/network.py:38-68).  x_pairs / res_pairs / out_pairs select the
 * format per operand (0 = float32); d_amax_in = MEASURED max |x| (or a bound); wl1 = max_co sum |w[co]|, bmax = max |bias| give the
 * output's bound max|x| wl1 + bmax (+ *d_res_bound), stored to d_bound_out; d_amax_out receives the measured max |y| */
int cslam_conv_igemm_h2p_dev(const void *d_x, int x_pairs, const unsigned *d_xbound, const void *d_w2, const float *d_bias,
                             const void *d_res, int res_pairs, const unsigned *d_res_bound, int B, int H, int W, int Cin,
                             int Cout, int KH, int KW, int stride, int pad, int relu, const unsigned *d_amax_in, float inv_sw,
                             float wl1, float bmax, unsigned *d_amax_out, int out_pairs, unsigned *d_bound_out, void *d_y,
                             void *stream);

/* 3x3 / stride 1 / pad 1 convolution 64 -> 128 channels (cslam/vpr/netvlad.py:163-171,227: VGG-16 conv2_1) as ONE direct kernel whose
 * weights (295 KB of exact fp16 pairs) stay in the registers of the four waves of a workgroup, 32 output channels each
 * (csrc/conv_direct_r.hip).  Arguments as cslam_conv3x3_direct_h_dev with Cin = 64, Cout = 128; d_w2r = `direct_r_pair_weights`:
 * [4 output-channel quarters][9 taps][2 K steps][2 channel tiles][hi | lo][64 lanes][8 halfs]. */
int cslam_conv3x3_direct_r_dev(const float *d_x, const void *d_w2r, const float *d_bias, int B, int H, int W, int Cin, int Cout,
                               int relu, int pool, const unsigned *d_amax, float inv_sw, unsigned *d_amax_out, float *d_y,
                               void *stream);

/* 3x3 / stride 1 / pad 1 convolution 128 -> 128 channels (cslam/vpr/netvlad.py:163-171,227: VGG-16 conv2_2, + MaxPool2d) on the same
 * register-resident form: half the output channels' weights (295 KB of exact fp16 pairs) fit a compute unit's registers, the two
 * workgroups 2 j, 2 j + 1 of an XCD walk the same blocks, one per output-channel half (csrc/conv_direct_r.hip).  Arguments as
 * cslam_conv3x3_direct_r_dev with Cin = Cout = 128; d_w2r2 = `direct_r2_pair_weights`: [2 output-channel halves][4 quarters of a
 * half][9 taps][2 K steps][2 input-channel slabs][hi | lo][64 lanes][8 halfs]. */
int cslam_conv3x3_direct_r2_dev(const float *d_x, const void *d_w2r2, const float *d_bias, int B, int H, int W, int Cin, int Cout,
                                int relu, int pool, const unsigned *d_amax, float inv_sw, unsigned *d_amax_out, float *d_y,
                                void *stream);

/* conv2_1 -> conv2_2 of VGG-16 (cslam/vpr/netvlad.py:163-171,227) with the 112 x 112 x 128 map between them in the PAIR FORMAT of
 * cslam_conv_igemm_h2p_dev: cslam_conv3x3_direct_r_pairs_dev = cslam_conv3x3_direct_r_dev (+ bias + ReLU, no pooling) writing
 * [B,H,W,4 blocks][hi 32 | lo 32] fp16 of s y, s the power of two of the bound *d_amax wl1 + bmax (-> d_bound_out; wl1 = max_co
 * sum |w[co]|, bmax = max |bias|); cslam_conv3x3_direct_hp_dev = cslam_conv3x3_direct_h_dev reading such a map (d_xbound = its bound slot)
 * and staging its patch without the split into pairs (csrc/conv_direct_r.hip, csrc/conv_direct_h.hip). */
int cslam_conv3x3_direct_r_pairs_dev(const float *d_x, const void *d_w2r, const float *d_bias, int B, int H, int W, int Cin, int Cout,
                                     const unsigned *d_amax, float inv_sw, float wl1, float bmax, unsigned *d_amax_out,
                                     unsigned *d_bound_out, void *d_y, void *stream);
int cslam_conv3x3_direct_hp_dev(const void *d_x, const unsigned *d_xbound, const void *d_w2, const float *d_bias, int B, int H, int W,
                                int Cin, int Cout, int relu, int pool, float inv_sw, unsigned *d_amax_out, float *d_y, void *stream);

/* 3x3 / stride 1 / pad 1 convolution 64 -> 64 channels between PAIR-FORMAT maps (the four stride-1 convolutions of ResNet-18/34's layer1:
 * cslam/vpr/cosplace_utils/network.py:38-68, the reference's default extractor) as ONE direct kernel whose weights stay in the registers
 * of the four waves of a workgroup, 16 output channels each, the input patch arriving by LDS-DMA (csrc/conv_direct_p.hip).  The
 * contract of cslam_conv_igemm_h2p_dev with KH = KW = 3, stride = pad = 1: d_x / d_xbound the pair-format input and its bound slot
 * (x_pairs = 0: a float32 NHWC map, split while its patch is staged; no shortcut then), d_amax_in the measured max |x|; d_res optional
 * shortcut in pair format (res_pairs, d_res_bound = its bound slot) or float32
 * NHWC (d_res_bound = a bound of max |res|); out_pairs: y in pair format scaled for max|x| wl1 + bmax (+ *d_res_bound) -> d_bound_out,
 * else float32 NHWC; d_amax_out (optional, zeroed) receives max |y|.  d_w2r / inv_sw = `stem_direct_pair_weights(weight)`:
 * [4 output-channel quarters][9 taps][2 K steps][hi | lo][64 lanes][8 halfs]. */
int cslam_conv3x3_direct_p_dev(const void *d_x, int x_pairs, const unsigned *d_xbound, const void *d_w2r, const float *d_bias, const void *d_res,
                               int res_pairs, const unsigned *d_res_bound, int B, int H, int W, int Cin, int Cout, int relu,
                               const unsigned *d_amax_in, float inv_sw, float wl1, float bmax, unsigned *d_amax_out, int out_pairs,
                               unsigned *d_bound_out, void *d_y, void *stream);

/* The same pair of layers (cslam/vpr/netvlad.py:163-171,227: VGG-16 conv1_1 + ReLU + conv1_2 + ReLU (+ MaxPool2d)) as ONE DIRECT
 * convolution kernel (csrc/conv_stem_direct_h.hip): the 147 KB of second-layer weights (exact fp16 pairs) stay in the registers of the
 * four waves of a workgroup, each wave owning 16 of the 64 intermediate channels; no Winograd transforms, no weight stream.
 * d_w1 / inv_sw1 / d_sumw as above; d_w2r / inv_sw2: the second layer's weights in MFMA-fragment order
 * [4 channel quarters][9 taps][2 x 32 output channels][hi | lo][64 lanes][8 halfs] (`stem_direct_pair_weights`). */
int cslam_conv_stem_direct_h_dev(const float *d_x0, const void *d_w1, const float *d_b1, const float *d_sumw, float inv_sw1,
                                 const void *d_w2r, const float *d_bias, float inv_sw2, int B, int H, int W, int pool,
                                 const unsigned *d_amax_x0, unsigned *d_amax_out, float *d_y, void *stream);

/* ---- multi-GPU exchange (csrc/comm.hip): RCCL over xGMI, one process per GPU ---------------------------------------
 * Replaces, inside one node, the ROS 2 transport of descriptors between robots
 * (cslam/global_descriptor_loop_closure_detection.py:198-227 publish GlobalDescriptors, :407-422 receive): rank g owns
 * robot g's bank (BASELINE config 4) or a row shard of ONE bank (the metric's bank at N > 1 GPUs).  Per step: ONE
 * all-gather of the new descriptors; every rank searches all of them in its bank (cslam_bank_search_dev); for a
 * row-sharded bank ONE all-to-all returns the (rows | score bits | count) lists to the keyframes' owners, who merge them
 * with cslam_topk_merge_dev.  cslam_amd/sharded.py is the Python twin over torch.distributed.
 * RCCL is looked up at run time (dlopen); without it these return CSLAM_E_UNSUPPORTED and nothing else is affected.
 *   cslam_comm_unique_id   rank 0: 128 bytes to hand to every rank (file, socket, launcher environment ...)
 *   cslam_comm_init        collective over all `world` processes; `device` = this rank's HIP device
 *   cslam_allgather_queries_dev  d_local [rows][row_bytes] -> d_all [world * rows][row_bytes], rank-major, on `stream`
 *   cslam_exchange_lists_dev     slice r of d_send [world][bytes_per_rank] goes to rank r; slice s of d_recv came from s */
int cslam_comm_unique_id(void *id128);
int cslam_comm_init(int world, int rank, const void *id128, int device, cslam_comm_t **out);
int cslam_comm_destroy(cslam_comm_t *comm);
int cslam_comm_info(const cslam_comm_t *comm, int *world, int *rank);
int cslam_allgather_queries_dev(cslam_comm_t *comm, const void *d_local, int64_t rows, int64_t row_bytes, void *d_all,
                                void *stream);
int cslam_exchange_lists_dev(cslam_comm_t *comm, const void *d_send, void *d_recv, int64_t bytes_per_rank, void *stream);

/* ---- coloured keyframe clouds and the merged map (csrc/cloud.hip, rules in csrc/cloud.h) -----------------------------
 * PCL, image_geometry and depth_image_proc were not available to compare against, and PCL's VoxelGrid sorts with an
 * unstable std::sort, so its float sums have no defined order: parity with PCL is unpinned.  The rule is what is stated
 * here and restated in tests/cloud_reference.py; the kernels agree with that restatement bit for bit.  No float atomics:
 * a cloud's bytes are the same alone or in any batch.  Every call below takes host copies of its offsets (and frame
 * sizes), which are mandatory, and uses the library's own scratch per (device, stream).
 *
 * Frames are batched as for cslam_feat_gray_dev: frame c owns the pixels d_offsets[c] .. d_offsets[c+1]-1 (int64,
 * n_frames + 1 entries from 0), d_hw[c] = (H, W) int32, H * W = its pixel count.  d_image: uint8, `channels` = 3 (B, G, R)
 * or 1 per pixel for the whole call; d_depth: uint16 millimetres (depth_type 0) or float32 metres (depth_type 1) for the
 * whole call; d_cam [n_frames, 4] float64 (fx, fy, cx, cy).  Colours are one uint32 per point, r | g << 8 | b << 16.
 *
 * cslam_cloud_from_depth_dev -- `create_colored_pointcloud` (src/front_end/visualization_utils.cpp:8-137, unit rules
 * of include/cslam/front_end/utils/depth_traits.h:50-64), all in float32: cx_f = float(cx), unit = double(float(1) *
 * float(0.001)) for uint16 and 1 for float32, kx = float(unit / fx); x = ((float(u) - cx_f) * float(d)) * kx, y likewise,
 * z = float(d) * float(0.001) for uint16 and d for float32.  Valid: d != 0 (uint16), isfinite(d) (float32: 0 and negative
 * depths are valid here, as in the reference); an invalid pixel gives three NaNs.  d_points [total, 3] float32 and d_rgb
 * [total] are the organised clouds, row-major pixel order.
 *
 * cslam_cloud_voxel_dev -- `visualization_pointcloud_voxel_subsampling` (src/front_end/rgbd_handler.cpp:640-663):
 * pcl::VoxelGrid's index rule in float32 with the sum order fixed, then pcl::PassThrough on z.  inv = float(1) /
 * float(leaf); over the rows with three finite coordinates min_b[a] = floor(min[a] * inv), index i[a] = floor(p[a] * inv) -
 * float(min_b[a]); one output row per occupied voxel in ascending (iz, iy, ix); xyz = the float32 sum of the voxel's points
 * in input order, one at a time from zero, divided once by float(count); colour = exact integer sums per channel,
 * truncating division by the count (PCL's float sums give the same below 65 793 points per voxel).  Then the rows with
 * 0.0f <= z <= float(max_range) are kept, in order.  d_rgb / d_out_rgb / d_counts may be NULL.  d_out [total, 3], d_out_rgb
 * and d_counts [total] have the capacity of the input; cloud c's rows are d_out_offsets[c] .. d_out_offsets[c+1]-1.
 * d_status [n_clouds]: 1 for a cloud with a non-finite cell, a cell of magnitude 2^31 or more, or an index of 2^21 or more
 * on some axis; it gets no rows (PCL prints a warning and returns the input unfiltered).
 *
 * cslam_cloud_keyframes_dev -- both chained on the device (`send_visualization_pointcloud`, rgbd_handler.cpp:665-682,
 * for visualization.voxel_size > 0): the same bytes as the two calls above.
 *
 * cslam_map_assemble_dev -- what the reference's visualiser does with the keyframe clouds at the poses of
 * `optimized_estimates_callback`, merged into one grid.  d_points [total, 3] float32 or float64 (dtype CSLAM_F32 /
 * CSLAM_F64), keyframe k owns rows d_offsets[k] .. d_offsets[k+1]-1; d_poses [n_keyframes, 16] float64 row-major.
 * All in float64: pw[r] = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3]; cell = floor(pw / voxel) with a true division (a
 * grid anchored at the world origin, not cslam_voxel_downsample_dev's origin rule), index = cell - the map's smallest
 * cell per axis; rows in ascending (iz, iy, ix); xyz = sequential float64 sums in input order (keyframe order, then row
 * order) divided once by the count; colours as above; d_counts = input rows per voxel.  Input rows with a non-finite
 * coordinate do not exist.  d_out_offsets [2] = {0, rows}; d_status [1] as above (the whole map gets no rows).
 *
 * CSLAM_E_INVALID, before anything touches HIP: leaf / voxel not finite or <= 0, max_range negative or NaN, a count
 * outside [1, 65535], a NULL pointer, host offsets that do not start at 0, that decrease, that do not match the frame
 * sizes, or that hold 2^31 - 2048 points or more.  Each filter call waits on the host once, after the bounds. */
int cslam_cloud_from_depth_dev(const uint8_t *d_image, int channels, const void *d_depth, int depth_type,
                               const int64_t *d_offsets, const int32_t *d_hw, const double *d_cam, int n_frames,
                               float *d_points, uint32_t *d_rgb, const int64_t *h_offsets, const int32_t *h_hw, void *stream);
int cslam_cloud_voxel_dev(const float *d_points, const uint32_t *d_rgb, const int64_t *d_offsets, int n_clouds, double leaf,
                          double max_range, float *d_out, uint32_t *d_out_rgb, int32_t *d_counts, int64_t *d_out_offsets,
                          int32_t *d_status, const int64_t *h_offsets, void *stream);
int cslam_cloud_keyframes_dev(const uint8_t *d_image, int channels, const void *d_depth, int depth_type,
                              const int64_t *d_offsets, const int32_t *d_hw, const double *d_cam, int n_frames, double leaf,
                              double max_range, float *d_out, uint32_t *d_out_rgb, int32_t *d_counts, int64_t *d_out_offsets,
                              int32_t *d_status, const int64_t *h_offsets, const int32_t *h_hw, void *stream);
int cslam_map_assemble_dev(const void *d_points, int dtype, const uint32_t *d_rgb, const int64_t *d_offsets, const double *d_poses,
                           int n_keyframes, double voxel, double *d_out, uint32_t *d_out_rgb, int32_t *d_counts,
                           int64_t *d_out_offsets, int32_t *d_status, const int64_t *h_offsets, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CSLAM_HIP_H */
