/* include/weasal_hip.h -- C ABI of libweasal_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary of the KPConv hot path: plain pointers and sizes, no
 * torch / numpy / C++ types.  Every pointer is a DEVICE pointer unless the parameter
 * name starts with `h_` (host).  `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  All functions are asynchronous on `stream` unless documented
 * otherwise, never allocate device memory unless documented, and return a ws_status.
 *
 * Each entry names the reference interface it replaces (paths relative to the reference
 * repository JohannesErnst/WeaSAL).  INTEGRATION.md shows the Python-side bindings.
 */
#ifndef WEASAL_HIP_H
#define WEASAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WS_OK = 0,
    WS_ERR_INVALID = 1,      /* bad shape / NULL pointer / inconsistent sizes          */
    WS_ERR_UNSUPPORTED = 2,  /* valid request this build has no kernel for             */
    WS_ERR_HIP = 3,          /* a HIP runtime call failed (see ws_last_error)          */
    WS_ERR_EMPTY = 4,        /* empty result: the reference raises RuntimeError("Error")
                                (cpp_wrappers/cpp_neighbors/wrapper.cpp:201-205,
                                 cpp_wrappers/cpp_subsampling/wrapper.cpp:266-270)     */
    WS_ERR_CAPACITY = 5      /* a caller-provided buffer is too small                  */
} ws_status;

/* KP_influence / aggregation_mode of models/blocks.py:147 */
enum { WS_INFLUENCE_LINEAR = 0, WS_INFLUENCE_CONSTANT = 1, WS_INFLUENCE_GAUSSIAN = 2 };
enum { WS_AGGREGATION_SUM = 0, WS_AGGREGATION_CLOSEST = 1 };

const char* ws_last_error(void);
/* kernels launched by this library since it was loaded (all threads, all streams): launches-per-step accounting */
int64_t ws_launch_count(void);   /* thread-local message of the last failing call */
const char* ws_version(void);
int ws_device_count(void);         /* number of HIP devices visible (no context is created) */

/* ------------------------------------------------------------------------------------------
 * KPConv (models/blocks.py:238-374).
 *
 * Shapes:  q_pts [nq,3] f32, s_pts [ns,3] f32, inds [nq,h] int64 with values in [0,ns]
 * (ns = shadow neighbour: point (1e6,1e6,1e6), zero feature, blocks.py:278,357),
 * x [ns,ci] f32, kernel_points [k,3] f32.
 *
 * ws_kpconv_gather_fwd: the fused neighbour-gather -> kernel-point influence -> feature
 *   aggregate (blocks.py:278-363):   wf[q,kk,c] = sum_h w(q,h,kk) * x[inds[q,h], c]
 *   with w = clamp(1 - sqrt(d2)/extent, 0) (linear, :337), 1 (constant, :332) or
 *   exp(-d2 / (2 (0.3 extent)^2 + 1e-9)) (gaussian, :343 and :70-77); aggregation CLOSEST
 *   keeps only the arg-min kernel point of each neighbour (:349-351).
 *   wf is [nq, k, ci] row-major, so that  out = wf.reshape(nq, k*ci) @ weights.reshape(k*ci, co)
 *   is the dense contraction of blocks.py:370-374 (done by the caller on MFMA).
 *   Deformable variant (blocks.py:244-325): deformed_kp [nq,k,3] (= kernel_points + offsets,
 *   :288) replaces kernel_points when non-NULL; neighbours with no kernel point within
 *   `extent` contribute nothing (:301-325); min_d2 [nq,k] (:304) is written when non-NULL;
 *   modulations [nq,k] (:256,:367) scale wf[q,kk,:] when non-NULL.
 * ws_kpconv_gather_bwd_x: dx[s,c] = sum over (q,h) with inds[q,h]==s of
 *   sum_kk w(q,h,kk) * (mod[q,kk]) * dwf[q,kk,c]   -- the autograd of the gather
 *   (a scatter_add in the reference), computed as a deterministic gather over the transposed
 *   neighbour table built by ws_transpose_build.
 * ws_kpconv_gather_bwd_geom (deformable only): gradients w.r.t. deformed_kp [nq,k,3] and
 *   modulations [nq,k], from dwf and from d(min_d2).
 * ------------------------------------------------------------------------------------------ */
int ws_kpconv_gather_fwd(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                         const int64_t* inds, int32_t h,
                         const float* x, int32_t ci,
                         const float* kernel_points, int32_t k,
                         const float* deformed_kp,    /* NULL = rigid */
                         const float* modulations,    /* NULL = none  */
                         float extent, int32_t influence, int32_t aggregation,
                         const int32_t* order,        /* NULL or a permutation of [0,nq): the order in which
                                                         queries are scheduled (results do not depend on it;
                                                         a spatial order keeps gathered rows in L2) */
                         float* wf,                   /* out [nq,k,ci] */
                         float* min_d2,               /* out [nq,k] or NULL */
                         void* stream);

int ws_kpconv_gather_bwd_x(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                           const int64_t* inds, int32_t h,
                           const int32_t* t_offsets,  /* [ns+2] from ws_transpose_build */
                           const int32_t* t_pairs,    /* [nq*h]  from ws_transpose_build */
                           const float* dwf, int32_t ci,      /* [nq,k,ci] */
                           const float* kernel_points, int32_t k,
                           const float* deformed_kp, const float* modulations,
                           float extent, int32_t influence, int32_t aggregation,
                           const int32_t* order,      /* NULL or a permutation of [0,ns): scheduling order */
                           float* dx,                 /* out [ns,ci] (fully overwritten) */
                           void* stream);

int ws_kpconv_gather_bwd_geom(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                              const int64_t* inds, int32_t h,
                              const float* x, int32_t ci,
                              const float* dwf,          /* [nq,k,ci] */
                              const float* kernel_points, int32_t k,
                              const float* deformed_kp,  /* [nq,k,3], required */
                              const float* modulations,  /* [nq,k] or NULL */
                              const float* d_min_d2,     /* [nq,k] or NULL */
                              float extent, int32_t influence, int32_t aggregation,
                              float* d_deformed_kp,      /* out [nq,k,3] */
                              float* d_modulations,      /* out [nq,k] or NULL */
                              void* stream);

/* Transposed neighbour table (support -> list of flat pair ids q*h+col), the deterministic
 * replacement of the scatter_add in the autograd of blocks.gather (blocks.py:36-67).
 * t_offsets [ns+2] int32: entries of support s are t_pairs[t_offsets[s] .. t_offsets[s+1]);
 * shadow pairs (index == ns) are not tabulated (slot ns stays empty).  Lists are sorted by pair id.
 * Requires nq*h < 2^31.
 * scratch: at least ws_transpose_scratch_bytes(nq,h,ns) bytes. */
int64_t ws_transpose_scratch_bytes(int64_t nq, int32_t h, int64_t ns);
int ws_transpose_build(const int64_t* inds, int64_t nq, int32_t h, int64_t ns,
                       int32_t* t_offsets, int32_t* t_pairs, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pooling helpers (models/blocks.py:80-111).
 * ws_max_pool_fwd: out[q,c] = max_h xpad[inds[q,h], c] with xpad = [x; 0] (blocks.py:95-111);
 *   arg[q,c] = the column h of the (first) maximum, kept for the backward.
 * ws_max_pool_bwd: dx[s,c] = sum of dy[q,c] over (q,h) with inds[q,h]==s and arg[q,c]==h.
 * ws_closest_pool_fwd: out[q,:] = xpad[inds[q,0], :] (blocks.py:80-92).
 * ws_closest_pool_bwd: dx[s,:] = sum of dy[q,:] over q with inds[q,0]==s.
 * The backward forms take the transposed table of `inds` (ws_transpose_build).
 * ------------------------------------------------------------------------------------------ */
int ws_max_pool_fwd(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                    float* out, int32_t* arg, void* stream);
int ws_max_pool_bwd(const float* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c,
                    const int32_t* t_offsets, const int32_t* t_pairs, int64_t ns,
                    float* dx, void* stream);
/* the same with a spatially coherent walking order (int32 permutation: the cell order of the queries' / supports' level,
 * ws_radius_neighbors_order; NULL = index order): results do not depend on it, only the memory traffic does -- consecutive
 * work items gather overlapping rows, and the workgroups of an XCD walk its part of the order together (pools.hip). */
int ws_max_pool_fwd_ordered(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, float* out,
                            int32_t* arg, const int32_t* order_q, void* stream);
int ws_max_pool_bwd_ordered(const float* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                            const int32_t* t_pairs, int64_t ns, float* dx, const int32_t* order_s, void* stream);
int ws_max_pool_fwd_ordered_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, uint16_t* out,
                                 int32_t* arg, const int32_t* order_q, void* stream);
int ws_max_pool_bwd_ordered_bf16(const uint16_t* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                                 const int32_t* t_pairs, int64_t ns, uint16_t* dx, const int32_t* order_s, void* stream);
int ws_closest_pool_fwd(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                        float* out, void* stream);
int ws_closest_pool_bwd(const float* dy, int64_t nq, int32_t h, int32_t c,
                        const int32_t* t_offsets, const int32_t* t_pairs, int64_t ns,
                        float* dx, void* stream);
/* the launch a pooling entry makes for these arguments (the launchers' own plan functions; pointers are only tested for
 * alignment, nothing is read or launched), as a name into out[cap]: "max_fwd vec G=32 U=4 AT=i32 f32 split=1 interleaved"
 * (G lanes per row, U neighbour rows in flight, the arg-max record's element, the row type, channel chunks per row, the
 * work assignment), "max_bwd generic bf16", "closest_fwd scalar f32", "closest_bwd vec G=16".  op names the entry family
 * (its _bf16 / _ordered forms included: rows_bf16 = 1 for bf16 rows, ordered = 1 when an order is passed); rows = nq for
 * the forwards, ns for the backwards; rows_a, rows_b: x and out, or dy and dx; arg: the arg-max record (the closest pools
 * ignore it), arg_bytes 4, or 1 for the byte record the fused blocks keep (f32 rows, c % 4 == 0, 16-byte aligned rows:
 * refused otherwise).  grid, when not NULL, receives the workgroups of the launch.  The closest backward follows
 * ws_closest_bwd_vec. */
enum { WS_POOL_MAX_FWD = 0, WS_POOL_MAX_BWD = 1, WS_POOL_CLOSEST_FWD = 2, WS_POOL_CLOSEST_BWD = 3 };
int ws_pool_variant(int32_t op, int64_t rows, int32_t c, const void* rows_a, const void* rows_b, const void* arg, int32_t rows_bf16,
                    int32_t arg_bytes, int32_t ordered, char* out, int32_t cap, int32_t* grid);

/* ------------------------------------------------------------------------------------------
 * Tall-skinny fp32 GEMMs on the f32-input MFMA -- the dense parts of the path:
 *   the unary 1x1 MLPs  y = x W^T (models/blocks.py:490-501, nn.Linear without bias) and the kernel
 *   contraction  out = wf[N,15Ci] @ weights[15Ci,Co]  (blocks.py:370-374), plus their autograd.
 * ws_gemm_xb :  y[m,n] = x[m,k] @ b[k,n]        (b row-major, ld = n; x/y row-major with ldx/ldy)
 * ws_gemm_xty:  out[k,n] = x[m,k]^T @ y[m,n]    (reduction over the tall dimension m; partial sums per
 *               row chunk in `scratch` (>= ws_gemm_xty_scratch_bytes), added in a fixed order)
 * Exact fp32 products and sums (v_mfma_f32_32x32x2_f32), i.e. rocBLAS-equivalent up to summation order.
 * ------------------------------------------------------------------------------------------ */
int ws_gemm_xb(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
               float* y, int64_t ldy, void* stream);
/* y = act(x @ b + bias[n] + residual[m,n]) -- the BatchNormBlock bias (models/blocks.py:465), the
 * residual sum and LeakyReLU(0.1) of the blocks (blocks.py:497-500, :563-564, :709) applied in the GEMM
 * epilogue.  bias / residual may be NULL; act: 0 = none, 1 = LeakyReLU(slope). */
int ws_gemm_xb_epilogue(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                        const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                        float* y, int64_t ldy, void* stream);
/* the same with split-K for short, deep products (m below ~32 k rows, k >= 512: the bottom of the pyramid):
 * up to 16 workgroup layers contract disjoint k ranges into `scratch` (>= ws_gemm_xb_scratch_bytes, may be
 * 0 = never split) and a second kernel adds them in a fixed order and applies the epilogue. */
int64_t ws_gemm_xb_scratch_bytes(int64_t m, int32_t k, int32_t n);
int ws_gemm_xb_epilogue_splitk(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                               const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                               float* y, int64_t ldy, void* scratch, int64_t scratch_bytes, void* stream);
/* backward of that epilogue in one pass over [m,n]: dz = dy * (y > 0 ? 1 : slope)  (LeakyReLU backward from
 * the OUTPUT y, models/blocks.py:500,564,709; y == NULL: no activation, dz untouched) and
 * colsum[n] = sum over rows of dz (the gradient of the BatchNormBlock bias, blocks.py:465; NULL: skipped).
 * Partial sums per row chunk in `scratch` (>= ws_act_bwd_colsum_scratch_bytes), added in a fixed order. */
int64_t ws_act_bwd_colsum_scratch_bytes(int64_t m, int32_t n);
int ws_act_bwd_colsum(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                      float* dz, int64_t lddz, float* colsum, void* scratch, void* stream);
int64_t ws_gemm_xty_scratch_bytes(int64_t m, int32_t k, int32_t n);
int ws_gemm_xty(const float* x, int64_t m, int32_t k, int64_t ldx, const float* y, int32_t n, int64_t ldy,
                float* out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Radius neighbours -- replaces cpp_wrappers/cpp_neighbors (radius_neighbors.batch_query,
 * wrapper.cpp:58-238 -> batch_nanoflann_neighbors, neighbors/neighbors.cpp:211-332).
 * For every query of batch element b: supports j of the same element with
 *   fl(fl(fl(dx*dx)+fl(dy*dy))+fl(dz*dz)) < fl(radius*radius)     (no FMA contraction)
 * sorted ascending by that d2 (ties: by index), as global support indices; rows padded with ns.
 *
 * Two-call protocol (the width is data dependent, neighbors.cpp:296-304):
 *   ws_radius_neighbors_plan   builds the per-element cell grid in `ws` and counts; synchronises
 *                              `stream` and returns *h_max_count (host).  WS_ERR_EMPTY if it is 0
 *                              or nq == 0.
 *   ws_radius_neighbors_fill   writes out[nq, width] with width <= max_count columns (cropping
 *                              columns is what datasets/common.py:336-346 does afterwards);
 *                              exactly one of out_i32 / out_i64 is non-NULL (int64 is what
 *                              common.py:551-553 converts to).
 * q_lens / s_lens are DEVICE int32 [nb]; h_q_lens / h_s_lens the same values on the host.
 * ------------------------------------------------------------------------------------------ */
typedef struct ws_neighbors_ws ws_neighbors_ws;     /* opaque workspace, owns device scratch */
int ws_neighbors_ws_create(ws_neighbors_ws** ws);
void ws_neighbors_ws_destroy(ws_neighbors_ws* ws);
int ws_radius_neighbors_plan(ws_neighbors_ws* ws,
                             const float* queries, int64_t nq, const float* supports, int64_t ns,
                             const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                             float radius, int32_t* h_max_count, void* stream);
int ws_radius_neighbors_fill(ws_neighbors_ws* ws, int32_t width,
                             int32_t* out_i32, int64_t* out_i64, void* stream);
/* One-call form for callers that crop anyway (datasets/common.py:336-346): builds the grid and makes
 * ONE query pass that writes out[nq,width] (rows padded with ns) and counts at the same time;
 * synchronises and returns the true *h_max_count -- if it is smaller than `width` the caller keeps the
 * first max_count columns (the rest is padding).  WS_ERR_EMPTY as above. */
int ws_radius_neighbors_search(ws_neighbors_ws* ws,
                               const float* queries, int64_t nq, const float* supports, int64_t ns,
                               const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                               float radius, int32_t width, int32_t* out_i32, int64_t* out_i64,
                               int32_t* h_max_count, void* stream);
/* Same single pass without any host synchronisation: the true max count is written to the DEVICE
 * int32 *d_max_count.  The rows are exact when that value is <= 128 (the sort slab of the fast
 * kernel); the caller checks the value later (e.g. once per batch for all its searches) and repeats
 * a search with ws_radius_neighbors_search if it was larger, or trims columns if it was smaller than
 * `width`.  An empty result shows as *d_max_count == 0. */
/* capacity (neighbours inside the radius per query) of the row slab ws_radius_neighbors_search_async uses for rows of `width`
 * entries: 128 up to width 128, else 576 / 704 / 1024; a maximum count beyond it (d_max_count) means truncated candidates:
 * the caller repeats that search with the two-call protocol. */
int32_t ws_radius_neighbors_async_cap(int32_t width);
int ws_radius_neighbors_search_async(ws_neighbors_ws* ws,
                                     const float* queries, int64_t nq, const float* supports, int64_t ns,
                                     const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                     float radius, int32_t width, int32_t* out_i32, int64_t* out_i64,
                                     int32_t* d_max_count, void* stream);
/* Count-only search for the neighbourhood-limit calibration (datasets/DALES_PseudoLabel.py:1238-1240): the arguments of
 * ws_radius_neighbors_plan without the host count; builds the cell grid as the plan does, then ADDS to hist[c] (DEVICE int64
 * [hist_n], zeroed by the caller once per calibration) the number of queries with exactly c supports inside the radius.  A
 * count of hist_n or more is dropped, as np.bincount(c, minlength=hist_n)[:hist_n] does (:1239).  No row, no per-query count
 * (ws_radius_neighbors_counts is not refreshed) and no device-to-host read: nothing synchronises beyond the staging copy of
 * the per-element table for nb > 48.  Integer atomics only -- per workgroup a histogram in LDS, flushed once with 64-bit adds
 * -- so the bins are bit-identical from run to run.  1 <= hist_n <= WS_NB_HIST_MAX (32 KB of LDS per workgroup; the
 * reference's histogram size ceil(4/3 pi (deform_radius + 1)^3) is 5576 at deform_radius 10): hist_n < 1 is WS_ERR_INVALID,
 * above the maximum WS_ERR_UNSUPPORTED, both found before the device is touched.  WS_ERR_EMPTY for nq == 0 or ns == 0, as
 * the plan.  A fill after it needs a plan of its own. */
#define WS_NB_HIST_MAX 8192
int ws_radius_neighbors_histogram(ws_neighbors_ws* ws,
                                  const float* queries, int64_t nq, const float* supports, int64_t ns,
                                  const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                  float radius, int64_t* hist, int32_t hist_n, void* stream);
/* Nearest neighbour only (opt-in): out [nq] = column 0 of the row ws_radius_neighbors_search_async would write -- the support
 * with the smallest (distance, index) inside `radius`, or ns -- without building and sorting the row.  For the UPSAMPLING
 * searches of the pyramid, of which KP-FCNN reads the first column only (models/blocks.py:80-92); *d_any (device) becomes
 * 1 if any query found a support, else 0.  Same grid reuse (ws_radius_neighbors_reuse_grid) as the full search. */
int ws_radius_neighbors_nearest_async(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                                      int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                      float radius, int32_t* out_i32, int64_t* out_i64, int32_t* d_any, void* stream);
/* supports of the last plan/search in cell order (device int32 [ns], a permutation): a spatially
 * coherent scheduling order for the kernels that take `order`. */
int ws_radius_neighbors_order(const ws_neighbors_ws* ws, int32_t* out_order, void* stream);
/* per-query neighbour counts of the last plan (device int32 [nq]); valid until the next plan.
 * Feeds the neighbourhood-limit calibration (datasets/DALES_PseudoLabel.py:1238-1240). */
const int32_t* ws_radius_neighbors_counts(const ws_neighbors_ws* ws);
/* Which fill kernel ran.  ws_radius_neighbors_fill_variant: name of the launch that fills rows of up to `cap` neighbours,
 * "kernel<row type[,slab]> grid<=blocks" (slabs 128 / 576 / 704 / 1024 / 2048; `beside`: through the asynchronous entries;
 * cap 0: the nearest-only kernel; WS_ERR_UNSUPPORTED above 2048) -- the launcher's own rule, no device work.
 * ws_radius_neighbors_last_fills: the caps of the fill launches the last public entry on `ws` made, in order (every entry
 * resets the record; the nearest-only search records 0): *n of them, the first min(*n, max) in caps. */
int ws_radius_neighbors_fill_variant(int32_t cap, int32_t out_i32, int32_t beside, char* out, int32_t out_cap);
int ws_radius_neighbors_last_fills(const ws_neighbors_ws* ws, int32_t* caps, int32_t max, int32_t* n);

/* Exact nearest neighbour, no radius -- replaces sklearn's KDTree.query(points, k=1) where the reference asks for the nearest
 * sub-cloud point of every original point (datasets/DALES_PseudoLabel.py:888-893 and its sibling dataset files; the round
 * trip of pseudoLabel_refinement.py:112-125).  For query q of batch element b: the support j of the same element that
 * minimises the key (d2, j),
 *   d2 = fl(fl(fl(dx*dx)+fl(dy*dy))+fl(dz*dz)) in FLOAT64,  dx = (double)q.x - (double)s.x     (no FMA contraction)
 * -- the arithmetic of the tree, so the index equals KDTree.query wherever the two nearest float64 distances differ; exact
 * float64 ties go to the smallest global index.  out [nq] = the global support index, or ns when the element has no
 * supports; out_d2 (optional, DEVICE float64 [nq]) = the winning d2, +inf beside ns.  Any query is answered, however far
 * from the supports; a query with a non-finite coordinate gets ns / +inf and sets WS_NN_STATUS_NONFINITE_QUERY in *d_status
 * (optional DEVICE int32, OR-ed into: the caller zeroes it); a non-finite support is never chosen.  The result is a pure
 * function of the inputs: no atomics on the result path, bit-identical from run to run, independent of `cell`.
 * cell: the cell size of the workspace's counting-sort grid the search walks (the grid's own caps may enlarge it);
 * 0 = chosen by the library per element from its bounding box and support count.  Only the speed depends on it.
 * Exactly one of out_i32 / out_i64 is non-NULL.  nq == 0: WS_OK, nothing queued.  ns == 0 with nq > 0: ns everywhere (NOT
 * WS_ERR_EMPTY: a batch with one empty element still gets its other elements).  NULL required pointers, both outputs or
 * none, negative lengths, lengths that do not sum to nq / ns: WS_ERR_INVALID, found before the device is touched.
 * Queued on `stream` without any device-to-host read; nothing synchronises beyond the staging copy of the per-element table
 * for nb > 48.  The plan state of `ws` (counts, a pending fill, the reusable grid) is gone afterwards. */
#define WS_NN_STATUS_NONFINITE_QUERY 1
int ws_nearest_neighbors(ws_neighbors_ws* ws,
                         const float* queries, int64_t nq, const float* supports, int64_t ns,
                         const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                         float cell, int32_t* out_i32, int64_t* out_i64, double* out_d2, int32_t* d_status, void* stream);

/* Table-free backward of self-query KPConv layers (queries == supports): the cell grid of the last search and the
 * key of the last neighbour kept per query replace the transposed table (ws_transpose_build).
 *   ws_radius_neighbors_set_key_last  one-shot request: the NEXT search/fill also writes key_last[nq]
 *                                     = (d2 bits << 32 | index) of the last kept neighbour, ~0 for untruncated rows
 *   ws_radius_neighbors_grid_info / _grid_export   copy the grid of the last plan (per-element table, cell offsets,
 *                                     cell-sorted supports) into a caller-owned device blob of `blob_bytes`
 *   ws_kpconv_gather_bwd_x_grid       = ws_kpconv_gather_bwd_x for q_pts == s_pts, pairs re-derived per support from
 *                                     that blob: q -> s iff d2 < radius^2 and (d2, s) <= key_last[q]; same pair order,
 *                                     same sums.  `overflow` (device int32, zero-initialised by the caller) receives the
 *                                     in-degree of a support with more than 192 incoming pairs (result then invalid);
 *                                     impossible when the search reported max_count <= 128 for that matrix. */
int ws_radius_neighbors_set_key_last(ws_neighbors_ws* ws, uint64_t* d_key_last);
/* one-shot hint: the NEXT plan / search uses the same supports (pointer, lengths, radius AND unchanged contents -- the
 * caller vouches) as the previous one and keeps its cell grid; ignored when anything checkable differs.  In the pyramid
 * of datasets/common.py:487-545 the conv, pool and (previous level's) upsample searches share one support set and one
 * radius per level: 5 grids instead of 13. */
int ws_radius_neighbors_reuse_grid(ws_neighbors_ws* ws, int32_t on);
int ws_radius_neighbors_grid_info(const ws_neighbors_ws* ws, int32_t* nb, int64_t* cells, int64_t* ns, int64_t* blob_bytes);
int ws_radius_neighbors_grid_export(const ws_neighbors_ws* ws, void* blob, void* stream);
int ws_kpconv_gather_bwd_x_grid(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                const uint64_t* key_last, float radius, const float* dwf, int32_t ci,
                                const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                float extent, int32_t influence, int32_t aggregation, const int32_t* order, float* dx,
                                int32_t* overflow, void* stream);

/* K4 / K4G with the activation backward of the preceding unary block folded into the store: dx * LeakyReLU'(gate_y),
 * gate_y [ns, ci] = that block's activated output (this layer's input x); gate_y NULL = the plain entries.
 * K4G also takes `rows` [ns, rows_h] (NULL = none): the index matrix of the same self-query search.  A support whose own
 * row was not truncated (key_last[s] = all ones) finds the queries that kept it among its row's entries (the distance is
 * symmetric bit for bit) instead of walking the 27 cells around it; truncated rows still walk the grid.
 * Replaces the autograd of nn.LeakyReLU between unary1 and KPConv (models/blocks.py:676-683). */
int ws_kpconv_gather_bwd_x_gated(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                 const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                                 const float* dwf, int32_t ci, const float* kernel_points, int32_t k,
                                 const float* deformed_kp, const float* modulations, float extent,
                                 int32_t influence, int32_t aggregation, const int32_t* order, const float* gate_y,
                                 float gate_slope, float* dx, void* stream);
/* ws_kpconv_gather_bwd_x_gated with four supports per wave (kpconv_gather_bwd_x_packed_kernel) where that form applies: f32
 * rows with ci % 4 == 0 and 16-byte aligned dwf / dx, rigid kernel, linear influence, sum, nq < ns and at most PACK_MEAN_MAX
 * (kpconv.hip) incoming pairs per support on average -- the strided layers of the pyramid.  Elsewhere it launches what
 * ws_kpconv_gather_bwd_x_gated launches; dx is the same bit for bit either way.  The reporter names the packed kernel and
 * its template arguments, or "none". */
int ws_kpconv_gather_bwd_x_packed(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                  const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                                  const float* dwf, int32_t ci, const float* kernel_points, int32_t k,
                                  const float* deformed_kp, const float* modulations, float extent,
                                  int32_t influence, int32_t aggregation, const int32_t* order, const float* gate_y,
                                  float gate_slope, float* dx, void* stream);
int ws_kpconv_gather_bwd_x_packed_variant(int64_t nq, int64_t ns, int32_t h, int32_t ci, const void* dwf, const void* dx, int32_t deformed,
                                          int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t ordered,
                                          char* out, int32_t cap);
int ws_kpconv_gather_bwd_x_grid_gated(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                      const uint64_t* key_last, float radius, const float* dwf, int32_t ci,
                                      const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                      float extent, int32_t influence, int32_t aggregation, const int32_t* order,
                                      const float* gate_y, float gate_slope, const int64_t* rows, int32_t rows_h, float* dx,
                                      int32_t* overflow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grid subsampling -- replaces cpp_wrappers/cpp_subsampling (grid_subsampling.subsample_batch /
 * subsample, wrapper.cpp:62-333,338-566 -> grid_subsampling.cpp:5-106,109-211).
 * Per batch element: origin = floor(min*(1/dl))*dl, cell key = iX + nX*iY + nX*nY*iZ (all f32,
 * IEEE divide), per cell the SEQUENTIAL f32 sum of its points in input order times
 * (float)(1.0/count); features: sequential sum / (float)count; labels: arg-max of the per-cell
 * histogram, the first maximum in the iteration order of the reference's libstdc++
 * unordered_map<int,int> (replayed for any number of distinct labels in a cell).
 * order_mode WS_ORDER_REFERENCE reproduces the reference's row order (the iteration order of a
 * libstdc++ unordered_map filled in first-occurrence order); WS_ORDER_FIRST_SEEN orders cells by
 * first occurrence (cheaper; same set of rows).
 *
 * Two-call protocol:
 *   ws_grid_subsample_plan  bins the points, synchronises and returns the per-element row counts
 *                           h_out_lens[nb] (after max_p truncation) and *h_m = their sum.
 *   ws_grid_subsample_fill  writes out_points [m,3] (+ out_features [m,fd], out_labels [m,ld]).
 * ------------------------------------------------------------------------------------------ */
enum { WS_ORDER_REFERENCE = 0, WS_ORDER_FIRST_SEEN = 1 };
typedef struct ws_subsample_ws ws_subsample_ws;
int ws_subsample_ws_create(ws_subsample_ws** ws);
void ws_subsample_ws_destroy(ws_subsample_ws* ws);
int ws_grid_subsample_plan(ws_subsample_ws* ws, const float* points, int64_t n,
                           const int32_t* h_lens, int32_t nb, float dl, int32_t max_p,
                           int32_t order_mode, int32_t* h_out_lens, int64_t* h_m, void* stream);
int ws_grid_subsample_fill(ws_subsample_ws* ws,
                           const float* features, int32_t fd,   /* [n,fd] or NULL */
                           const int32_t* labels, int32_t ld,   /* [n,ld] or NULL */
                           float* out_points, float* out_features, int32_t* out_labels,
                           uint64_t* out_keys,                  /* [m] cell keys or NULL (test aid) */
                           int32_t* out_counts,                 /* [m] points per cell or NULL */
                           void* stream);

/* Rotation of stacked clouds by one 3x3 matrix per batch element, f32, no FMA:
 * out[i,j] = (p0*R[b,0,j] + p1*R[b,1,j]) + p2*R[b,2,j]   (transpose=1 uses R[b,j,:]),
 * the arithmetic of datasets/common.py:116-119 and :131-135 (random grid orientation). */
int ws_rotate_clouds(const float* points, int64_t n, const int32_t* lens /*device [nb]*/, int32_t nb,
                     const float* rot /*device [nb,3,3]*/, int32_t transpose, float* out, void* stream);

/* same with HOST lengths / matrices (h_lens [nb], h_rot [nb,3,3]), passed as a kernel argument: no
 * host-to-device copy and no synchronisation; nb <= 64 (WS_ERR_UNSUPPORTED beyond). */
int ws_rotate_clouds_host(const float* points, int64_t n, const int32_t* h_lens, int32_t nb,
                          const float* h_rot, int32_t transpose, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole input pyramid of one batch in ONE call: the per-layer loop of PointCloudDataset.segmentation_inputs
 * (datasets/common.py:461-577) -- conv / pool / upsample searches and the grid subsampling with its random grid
 * orientation (:77-135) for every level, matrices cropped to the neighbourhood limits (:336-346).  Same kernels and
 * schedule as the per-call entries above (which it calls); the caller's interpreter stays released for the whole build.
 * All outputs live in the caller's `arena` at the returned byte offsets (-1: not produced): points of level l >= 1
 * (float [n[l],3]), neighbors (int64 [n[l], limit[l]]), pools (int64 [n[l+1], limit[l]]), upsamples (int64 [n[l],
 * limit[l+1]]), the cell order of every searched level (int32 [n[l]]), with want_grids the exported search grid and
 * key_last of the self-query searches (ws_radius_neighbors_grid_export / _set_key_last), the lengths (int32
 * [n_levels][nb]) and 4 n_levels int32 slots (maximum row lengths; then n_levels zeroed flags for the grid backward).
 * max_count [3 l + {0 conv, 1 pool, 2 upsample}] = true maximum row length of that search (host; -1: no such search):
 * 0 = the reference's empty-result error, < width = the caller may trim, > 128 (1024 for limits > 128) = the row slab
 * of the asynchronous search overflowed and the caller repeats that search with the two-call protocol.
 * Matrices whose widest row is shorter than the limit are cropped in place to that width (final_width; 0 = left to the
 * caller: empty / overflowed).  want_tables: the transposed tables (ws_transpose_build) of the pooling matrices, of the
 * first column of the upsampling matrices and -- without want_grids -- of the convolution matrices, at off_toffsets /
 * off_tpairs [3 l + kind] (-1: none).  scratch must also hold the largest matrix and the largest table's scratch.
 * WS_ERR_CAPACITY: the arena is too small; needed_bytes is set, nothing else is valid.  Synchronises the stream.
 * ------------------------------------------------------------------------------------------ */
#define WS_PYRAMID_MAX_LEVELS 8
#define WS_PYRAMID_MAX_BATCH 64
typedef struct ws_pyramid_desc {
    /* in */
    int32_t n_levels, nb, want_grids, want_tables;
    const float* points;                 /* level 0: [n0,3] device */
    int64_t n0;
    const float* h_rot;                  /* host [n_levels-1][nb][3][3] grid orientations (common.py:99-121) or NULL */
    void* arena; int64_t arena_bytes;    /* device, 256-byte aligned */
    void* scratch; int64_t scratch_bytes;/* device, >= 2 * align256(12 n0) */
    int32_t conv_on[WS_PYRAMID_MAX_LEVELS], pool_on[WS_PYRAMID_MAX_LEVELS];
    float r_conv[WS_PYRAMID_MAX_LEVELS], r_pool[WS_PYRAMID_MAX_LEVELS], r_up[WS_PYRAMID_MAX_LEVELS], dl[WS_PYRAMID_MAX_LEVELS];
    int32_t limit[WS_PYRAMID_MAX_LEVELS + 1];
    int32_t nearest_up;                  /* 1: upsampling matrices hold the nearest support only, [n, 1] (ws_radius_neighbors_nearest_async) */
    /* in (level 0) / out (levels >= 1) */
    int32_t lens[WS_PYRAMID_MAX_LEVELS][WS_PYRAMID_MAX_BATCH];
    /* out */
    int64_t needed_bytes;
    int64_t n[WS_PYRAMID_MAX_LEVELS];
    int64_t off_points[WS_PYRAMID_MAX_LEVELS], off_neighbors[WS_PYRAMID_MAX_LEVELS], off_pools[WS_PYRAMID_MAX_LEVELS],
            off_upsamples[WS_PYRAMID_MAX_LEVELS], off_order[WS_PYRAMID_MAX_LEVELS], off_key_last[WS_PYRAMID_MAX_LEVELS],
            off_blob[WS_PYRAMID_MAX_LEVELS], blob_bytes[WS_PYRAMID_MAX_LEVELS], grid_cells[WS_PYRAMID_MAX_LEVELS];
    int64_t off_lens, off_slots;
    int32_t max_count[3 * WS_PYRAMID_MAX_LEVELS], width[3 * WS_PYRAMID_MAX_LEVELS], final_width[3 * WS_PYRAMID_MAX_LEVELS];
    int32_t cap[3 * WS_PYRAMID_MAX_LEVELS];   /* sort slab each search was launched with (ws_radius_neighbors_async_cap then) */
    int64_t off_toffsets[3 * WS_PYRAMID_MAX_LEVELS], off_tpairs[3 * WS_PYRAMID_MAX_LEVELS];
} ws_pyramid_desc;
int ws_pyramid_build(ws_neighbors_ws* nws, ws_subsample_ws* sws, ws_pyramid_desc* desc, void* stream);
int64_t ws_pyramid_desc_bytes(void);   /* sizeof(ws_pyramid_desc): lets a binding check its mirror of the struct */

/* The pyramid of one calibration batch, count-only (DALES_PseudoLabel.py:1238-1240 reads one number per point and layer of
 * an un-limited batch: how many supports lie inside the convolution radius).  Per level with conv_on one
 * ws_radius_neighbors_histogram of the level's points against themselves at r_conv[l], ADDED to row l of `hists` (device
 * int64 [n_levels][hist_n], zeroed by the caller once per calibration); per level with pool_on the rotation, grid
 * subsampling and back rotation of ws_pyramid_build (the same code), which give the next level.  No index matrix, no pool or
 * upsample search, no table, no arena.
 * Reads of `desc`: n_levels, nb, points, n0, h_rot, conv_on, pool_on, r_conv, dl, lens[0], scratch, scratch_bytes (at least
 * ws_pyramid_histograms_scratch_bytes(n0) = 2 * align256(12 n0), 256-byte aligned); the limits, the arena and the
 * want-flags are ignored.  Writes lens[l] and n[l] of every level, nothing else.
 * Host waits: the ones ws_grid_subsample_plan makes, one per pooling level = n_levels - 1 per batch (the next level's size
 * is data); the count passes and their flushes are queued behind them without a read.
 * hist_n as ws_radius_neighbors_histogram; a NULL argument or inconsistent sizes: WS_ERR_INVALID; all found before the device
 * is touched.  WS_ERR_EMPTY where ws_pyramid_build returns it (a level subsampled to nothing). */
int64_t ws_pyramid_histograms_scratch_bytes(int64_t n0);
int ws_pyramid_histograms(ws_neighbors_ws* nws, ws_subsample_ws* sws, ws_pyramid_desc* desc, int64_t* hists, int32_t hist_n,
                          void* stream);



/* ------------------------------------------------------------------------------------------
 * Supervised contrastive loss of the pseudo-label trainer, the [N, slc_con] part of
 * KPFCNN.contrast_loss (models/architectures.py:455-497), fused: per point i
 *   loss[i] = -T * mean over the positive slice columns of log-softmax(<on_i, xs_j>/T over the usable columns)
 * with usable = (slc_idx[j] != i) and certain[slc_idx[j]] == certain[i], positive = usable and
 * lbl[slc_idx[j]] == lbl[i].  on [n,c] = L2-normalised logits (:475), xs [s,c] = on[slc_idx] (:476),
 * certain [n] uint8 (:433-435), lbl [n] int64 pseudo labels (:438-439).  rowmax / den / npos [n] are saved
 * for the backward, which returns d loss / d on (d_on [n,c], the slice rows' own contribution excluded) and
 * d loss / d xs (d_xs [s,c]; per-chunk partials in `scratch`, added in a fixed order).  c <= 16, s <= 1024
 * (WS_ERR_UNSUPPORTED beyond).  Preconditions, the caller's to keep:
 *   - the rows of on / xs have norm <= 1 (unit rows, or all-zero ones): the sums are taken against the bound |logit| <= 1/T;
 *   - 0.023 <= temperature <= 1e26 (WS_ERR_INVALID outside): exp(-2/T) must be a normal float, -T / 1e-12 finite;
 *   - lbl >= 0 wherever certain == 0 (a negative label of an uncertain point would collide with the kernels' markers for
 *     padding columns and rows beyond n; ws_contrast_head_fwd cannot produce one: a given label, -1 included, is certain).
 * ------------------------------------------------------------------------------------------ */
int ws_contrast_rows_fwd(const float* on, int64_t n, int32_t c, const float* xs, int32_t s, const int64_t* slc_idx,
                         const uint8_t* certain, const int64_t* lbl, float temperature, float eps, float* loss,
                         float* rowmax, float* den, float* npos, void* stream);
int64_t ws_contrast_rows_bwd_scratch_bytes(int64_t n, int32_t c, int32_t s);
int ws_contrast_rows_bwd(const float* on, int64_t n, int32_t c, const float* xs, int32_t s, const int64_t* slc_idx,
                         const uint8_t* certain, const int64_t* lbl, float temperature, const float* rowmax,
                         const float* den, const float* npos, const float* g, float* d_on, float* d_xs, void* scratch,
                         void* stream);

/* The rest of KPFCNN.contrast_loss around the [N, slc_con] part (models/architectures.py:425-454 before it, :475-476 the
 * normalisation, :498-504 after it), so that the whole loss is a few launches and never synchronises with the host.
 * head_fwd: x [n, c] logits (row stride ldx), labels [n] int64 (values >= 10 = unlabelled, :430-433), threshold
 *   (config.contrast_thd / 100).  Writes on [n,c] = F.normalize(x) (:475), inv_norm [n] = 1 / max(|x|, 1e-12), certain [n]
 *   uint8 = (max softmax > threshold) | labelled, lbl [n] int64 = the label where given else the arg-max class, then draws the
 *   slice: slot j of s takes the r_j-th valid point (0-based, in index order), r_j = r_given[j], or from the uniforms u [s] as
 *   floor(u_j * num_valid) -- with fewer than s valid points slot j < num_valid takes point j (:450-454) -- clamped to
 *   num_valid - 1; slc_idx [s] int64 and xs [s,c] = on[slc_idx] (:476).  state [2] int32: number of valid points, and the
 *   tail's arrival counter (zeroed here).  No valid point: slc_idx = n - 1 everywhere and the tail returns 0 (:441-443).
 * tail_fwd: pts_loss [n] from ws_contrast_rows_fwd -> per_class [n_cls] (mean of the points with loss > 0 per label),
 *   loss [1] = mean of the per_class entries > 0 (:498-504), w_cls [n_cls] = d loss / d pts_loss of a kept point of the class.
 * tail_bwd: g [1] -> g_row [n] (the `g` operand of ws_contrast_rows_bwd).
 * head_bwd: d_on [n,c] (modified in place: the slice rows' gradients d_xs [s,c] are added onto their points, duplicates in
 *   slot order) -> d_x [n, c] (row stride ldd) through the backward of the normalisation.
 * c <= 16, n_cls <= 16 (WS_ERR_INVALID beyond); s <= 1024, the limit of the rows entries (WS_ERR_UNSUPPORTED beyond, before
 * any launch). */
int64_t ws_contrast_head_scratch_bytes(int64_t n);
int ws_contrast_head_fwd(const float* x, int64_t n, int32_t c, int64_t ldx, const int64_t* labels, float threshold,
                         const float* u, const int64_t* r_given, int32_t s, float* on, float* inv_norm, uint8_t* certain,
                         int64_t* lbl, int64_t* slc_idx, float* xs, int32_t* state, void* scratch, void* stream);
int64_t ws_contrast_tail_scratch_bytes(int64_t n);
int ws_contrast_tail_fwd(const float* pts_loss, const int64_t* lbl, int64_t n, int32_t n_cls, int32_t* state, float* per_class,
                         float* w_cls, float* loss, void* scratch, void* stream);
int ws_contrast_tail_bwd(const float* pts_loss, const int64_t* lbl, int64_t n, int32_t n_cls, const float* w_cls, const float* g,
                         float* g_row, void* stream);
int ws_contrast_head_bwd(float* d_on, const float* d_xs, const int64_t* slc_idx, int32_t s, const float* on,
                         const float* inv_norm, int64_t n, int32_t c, float* d_x, int64_t ldd, void* stream);


/* ------------------------------------------------------------------------------------------
 * bf16-feature path (BASELINE.json configs[4]: "deformable-KPConv ... bf16"; SURVEY.md section 8d C5:
 * feature rows / weights bf16 in HBM, fp32 accumulate, geometry fp32).  The reference has no reduced-precision
 * path; these entries are the bf16-row forms of the operators above and replace the same reference lines
 * (models/blocks.py:36-134 pools, :238-374 KPConv, :370-374 / :490-501 the dense products).  Feature rows are
 * bf16 (uint16_t bit patterns, round-to-nearest-even on store), everything geometric (points, kernel points,
 * deformed_kp, modulations, min_d2 and their gradients) stays f32; sums run in f32 and are rounded once.
 * Rows need c % 4 == 0 and 8-byte alignment (WS_ERR_INVALID otherwise -- the 3-channel input layer stays f32).
 * ------------------------------------------------------------------------------------------ */
int ws_kpconv_gather_fwd_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                              const uint16_t* x, int32_t ci, const float* kernel_points, int32_t k, const float* deformed_kp,
                              const float* modulations, float extent, int32_t influence, int32_t aggregation,
                              const int32_t* order, uint16_t* wf, float* min_d2, void* stream);
int ws_kpconv_gather_bwd_x_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                                const int32_t* t_offsets, const int32_t* t_pairs, const uint16_t* dwf, int32_t ci,
                                const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                float extent, int32_t influence, int32_t aggregation, const int32_t* order, uint16_t* dx,
                                void* stream);
int ws_kpconv_gather_bwd_x_grid_bf16(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                     const uint64_t* key_last, float radius, const uint16_t* dwf, int32_t ci,
                                     const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                     float extent, int32_t influence, int32_t aggregation, const int32_t* order, uint16_t* dx,
                                     int32_t* overflow, void* stream);
int ws_kpconv_gather_bwd_geom_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                                   const uint16_t* x, int32_t ci, const uint16_t* dwf, const float* kernel_points, int32_t k,
                                   const float* deformed_kp, const float* modulations, const float* d_min_d2, float extent,
                                   int32_t influence, int32_t aggregation, float* d_deformed_kp, float* d_modulations,
                                   void* stream);
int ws_max_pool_fwd_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                         uint16_t* out, int32_t* arg, void* stream);
int ws_max_pool_bwd_bf16(const uint16_t* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                         const int32_t* t_pairs, int64_t ns, uint16_t* dx, void* stream);
int ws_closest_pool_fwd_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                             uint16_t* out, void* stream);
int ws_closest_pool_bwd_bf16(const uint16_t* dy, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                             const int32_t* t_pairs, int64_t ns, uint16_t* dx, void* stream);

/* Y[m,n] = act( X[m,k] * Bt[n,k]^T + bias + residual ) on v_mfma_f32_32x32x16_bf16: X, Bt, residual bf16 rows
 * (K-contiguous: Bt is nn.Linear's own [out,in] layout, blocks.py:490), bias f32 [n], fp32 accumulate, one rounding
 * to bf16 on store -- or f32 output (out_f32 = 1: the logits, the offsets of deformable KPConv blocks.py:244-267).
 * k % 32 == 0, ldx % 8 == 0, ldbt % 8 == 0, 16-byte aligned x / bt (WS_ERR_INVALID otherwise; callers keep such
 * products on the f32 kernels).  act: 0 = identity, 1 = LeakyReLU(slope). */
int ws_gemm_xbt_bf16(const uint16_t* x, int64_t m, int32_t k, int64_t ldx, const uint16_t* bt, int32_t n, int64_t ldbt,
                     const float* bias, const uint16_t* residual, int64_t ldr, int32_t act, float slope,
                     void* y, int64_t ldy, int32_t out_f32, void* stream);
/* out[k,n] f32 = X[m,k]^T * Y[m,n] with bf16 rows (the fp32 master gradient dW; exact products, fp32 sums on the
 * f32 MFMA); scratch as ws_gemm_xty_scratch_bytes(m, k, n). */
int ws_gemm_xty_bf16(const uint16_t* x, int64_t m, int32_t k, int64_t ldx, const uint16_t* y, int32_t n, int64_t ldy,
                     float* out, void* scratch, void* stream);
/* dz = dy * LeakyReLU'(y) as bf16 rows (y = the layer's bf16 output, NULL = identity: then dz may be NULL) and the f32
 * column sums of dz (colsum NULL = not wanted); dy is bf16, or f32 when dy_f32 = 1.  n % 4 == 0. */
int64_t ws_act_bwd_colsum_bf16_scratch_bytes(int64_t m, int32_t n);
int ws_act_bwd_colsum_bf16(const void* dy, int32_t dy_f32, int64_t m, int32_t n, int64_t lddy, const uint16_t* y, int64_t ldy,
                           float slope, uint16_t* dz, int64_t lddz, float* colsum, void* scratch, void* stream);


/* ------------------------------------------------------------------------------------------
 * Whole network blocks behind ONE call each (rigid KPConv, linear influence, sum aggregation, f32 rows).
 *
 * The reference runs a block as ~10 separate torch ops plus their autograd nodes (models/blocks.py:510-564
 * SimpleBlock, :624-709 ResnetBottleneckBlock; the decoder step models/architectures.py:339-343: nearest_upsample ->
 * concat(skip) -> unary); driven from Python each launch costs ~15 us of host time, more than most of these kernels
 * take.  ws_kpblock_fwd / _bwd launch the whole sequence from C on one stream:
 *
 *   x1   = lrelu(feat @ w1^T + b1)                          unary1   (absent when w1 == NULL: x1 = feat)
 *   wf   = gather(x1)                                       K3, ws_kpconv_gather_fwd
 *   x2   = lrelu(wf @ wk + bk)                              the kernel contraction + BatchNormBlock bias + LeakyReLU
 *   out  = lrelu(x2 @ w2^T + b2 + shortcut)                 unary2 + residual sum (absent when w2 == NULL: out = x2)
 *   shortcut = max_pool(feat, inds) if strided else feat,   then @ ws^T + bs when ws != NULL
 *
 * and in the backward every gradient accumulation is the residual operand of a GEMM epilogue (no separate adds),
 * LeakyReLU' and the bias gradients share one pass (ws_act_bwd_colsum), dX of the KPConv goes through the search grid
 * of the level (ws_kpconv_gather_bwd_x_grid) when grid_blob != NULL, else through the transposed table.
 * Linear weights are nn.Linear's [out,in] row-major; wk is KPConv.weights [k, conv_in, conv_out] (blocks.py:171).
 * Biases may be NULL (BatchNormBlock with use_bn is an identity, blocks.py:453-463).
 * Requirements (WS_ERR_UNSUPPORTED otherwise; the caller then runs the operators one by one): in_dim, conv_out,
 * out_dim multiples of 4 and conv_in a multiple of 4 (or the 3..4-channel input layer without unary1), k = 15.
 * Empty sides: nq = 0 (with or without supports) is an empty call whose backward clears every gradient; queries without
 * a single support (ns = 0, nq > 0) are WS_ERR_UNSUPPORTED in both entries and both size queries.
 * All buffers are caller-owned; `scratch` must hold ws_kpblock_*_scratch_bytes(desc) bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct ws_kpblock {
    /* geometry of the convolution */
    const float* q_pts; int64_t nq;
    const float* s_pts; int64_t ns;
    const int64_t* inds; int32_t h;
    const float* kernel_points; int32_t k; float extent;
    const int32_t* order_q;              /* scheduling hints (NULL allowed) */
    const int32_t* order_s;
    /* dX route: search grid of a self-query level ... */
    const void* grid_blob; int32_t grid_nb; int64_t grid_cells; const uint64_t* key_last; float grid_radius;
    int32_t* grid_overflow;
    /* ... or the transposed table of inds (also used by the max-pool shortcut of strided blocks) */
    const int32_t* t_offsets; const int32_t* t_pairs;
    /* widths */
    int32_t in_dim, conv_in, conv_out, out_dim, strided;
    float slope;
    /* parameters */
    const float *w1, *b1, *wk, *bk, *w2, *b2, *ws, *bs;
    /* activations: feat [ns,in_dim] in; x1 [ns,conv_in] (w1 != NULL), wf [nq,k*conv_in], x2 [nq,conv_out] (w2 != NULL),
     * pooled [nq,in_dim] + arg (strided with w2), out [nq,out_dim]: written by fwd, read by bwd */
    const float* feat; float* x1; float* wf; float* x2; float* pooled; int32_t* arg; float* out;
    /* backward: dout [nq,out_dim] in; gradients out (dfeat NULL = not wanted; parameter gradients NULL where the
     * parameter is NULL; the shortcut bias gradient equals db2) */
    const float* dout; float* dfeat; float *dw1, *db1, *dwk, *dbk, *dw2, *db2, *dws;
    int32_t timed;                       /* 1: bracket the K3 launch with HIP events (ws_timer_*) */
    int32_t rows_sorted;                 /* 1: the rows of inds are sorted by distance from their query (radius search output):
                                            the gather stops at the reach of the kernel points (ws_kpconv_gather_fwd_ex) */
    int32_t infer;                       /* 1: forward only -- no backward will follow: `wf` may be NULL and layers the fused
                                            forward kernel covers (ws_kpconv_layer_fwd_fused) run as one launch */
    int32_t dout_pregated;               /* backward: 1 = `dout` already carries this block's output LeakyReLU' (the consumer of
                                            `out` multiplied it into the gradient it wrote: its gate_dfeat): the block's first
                                            activation-backward pass is skipped (bias gradients: column sums of dout) */
    int32_t gate_dfeat;                  /* backward: 1 = write dfeat * LeakyReLU'(feat) -- feat is the activated output of the
                                            block that produced it, which then runs with dout_pregated; the multiplication
                                            rides on the kernel that writes dfeat */
    const float* dfeat_add;              /* backward, optional [ns,in_dim]: a second gradient of `feat` (the decoder's skip
                                            connection reads the same tensor, architectures.py:339-341), summed into dfeat by
                                            the kernel that writes the shortcut's share instead of by a pass of its own */
} ws_kpblock;

/* Scratch: the size queries return a multiple of 256 bytes (-1: the descriptor is refused, ws_last_error says why); the
 * runs return WS_ERR_CAPACITY for any scratch_bytes below what the query returns for the same descriptor (size the
 * buffer by the query, not by hand; the size depends on ws_block_group_rows).  The same holds for ws_upunary_*. */
int64_t ws_kpblock_fwd_scratch_bytes(const ws_kpblock* d);
int64_t ws_kpblock_bwd_scratch_bytes(const ws_kpblock* d);
int ws_kpblock_fwd(const ws_kpblock* d, void* scratch, int64_t scratch_bytes, void* stream);
int ws_kpblock_bwd(const ws_kpblock* d, void* scratch, int64_t scratch_bytes, void* stream);

/* Decoder step (models/architectures.py:339-343 + blocks.py:473-507): with the unary's weight w = [wx | wsk]
 * ([out, c_up + c_skip], leading dimension ldw), evaluated as
 *   yc  = xc @ wx^T                        at the coarse resolution [nc,out]
 *   out = lrelu(skip @ wsk^T + b + yc[ups[:,0]])          (closest_pool = nearest upsampling, blocks.py:80-92)
 * identical in exact arithmetic to upsample -> concat -> unary (a row gather commutes with a per-row linear map).
 * Backward: dw [out, c_up + c_skip] (same layout as w), db, dxc [nc,c_up], dskip [nf,c_skip]; t_offsets / t_pairs =
 * transposed table of column 0 of `ups`.  nf = 0 is an empty call (the backward clears every gradient); fine rows without
 * a single coarse row (nc = 0, nf > 0) are WS_ERR_UNSUPPORTED in both entries and both size queries. */
typedef struct ws_upunary {
    const float* xc; int64_t nc; int32_t c_up;
    const float* skip; int64_t nf; int32_t c_skip;
    const int64_t* ups; int32_t h_up;
    const int32_t* t_offsets; const int32_t* t_pairs;
    const float* w; int64_t ldw; const float* b; int32_t out_dim; int32_t relu; float slope;
    float* yc; float* out;               /* fwd outputs (yc is scratch-like but caller-owned: not needed by bwd) */
    const float* dout; float* dxc; float* dskip; float* dw; float* db;
    /* nn.Dropout on `out` (models/architectures.py:345-346: the droplayer in front of the head), fused: drop_p > 0 makes the
     * forward's last epilogue write dropout(out) (keep decision = function of (drop_seed, element index), the bits of
     * ws_dropout_apply) and the backward treat `dout` as the gradient of that dropped tensor.  Needs relu != 0. */
    float drop_p; uint64_t drop_seed;
    int32_t dout_pregated;               /* as in ws_kpblock: dout already multiplied by LeakyReLU'(out) by the consumer (and run
                                            through the dropout backward when drop_p > 0: ws_gemm_xb_gate_dropout) */
    int32_t gate_dxc;                    /* backward: write dxc * LeakyReLU'(xc) (xc = the activated output of its producer) */
} ws_upunary;

int64_t ws_kpblock_bytes(void);   /* sizeof(ws_kpblock), sizeof(ws_upunary): hold a binding's layout of the descriptors */
int64_t ws_upunary_bytes(void);   /* to the compiler's, as ws_pyramid_desc_bytes does */
int64_t ws_upunary_fwd_scratch_bytes(const ws_upunary* d);
int64_t ws_upunary_bwd_scratch_bytes(const ws_upunary* d);
int ws_upunary_fwd(const ws_upunary* d, void* scratch, int64_t scratch_bytes, void* stream);
int ws_upunary_bwd(const ws_upunary* d, void* scratch, int64_t scratch_bytes, void* stream);

/* y = act(x @ B + bias + residual) with a strided small matrix: B[kk][col] = b[kk*b_row_stride + col*b_col_stride]
 * (b_row_stride = 1, b_col_stride = K reads nn.Linear's [N,K] weight as its transpose in place).  Strided forms need
 * k % 32 == 0, n % 4 == 0 and 16-byte aligned rows. */
int ws_gemm_xb_epilogue_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                                int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                                int32_t act, float slope, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                                void* stream);

/* The same product with nn.Dropout applied to the activated output in the epilogue: y = keep ? act(..) / (1 - p) : 0, the keep
 * decision of element (row, col) being that of ws_dropout_apply for index row * n + col and the same seed (bit-identical to
 * the product followed by ws_dropout_apply on a contiguous [m, n] tensor; no mask is stored). */
int ws_gemm_xb_dropout_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                               int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                               int32_t act, float slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                               int64_t scratch_bytes, void* stream);

/* dX = dZ @ B (B row-major [K, N]) as the gradient of a layer INPUT that came out of a LeakyReLU and, optionally, an nn.Dropout
 * after it: y = dropout_bwd(x @ b) * LeakyReLU'(gate_y), in that order (the order of the separate backward passes: same bits);
 * gate_y [m, n] = the activated (and dropped: same signs where kept) tensor, NULL = no gate; drop_p = 0 = no dropout.  The
 * producer of gate_y then needs no activation-backward pass of its own (ws_kpblock / ws_upunary: dout_pregated). */
int ws_gemm_xb_gate_dropout(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, const float* gate_y,
                            int64_t ldg, float gate_slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                            int64_t scratch_bytes, void* stream);

/* ws_act_bwd_colsum for a tensor that went through that dropout: dy is the gradient of dropout(y') where y' is the activated
 * output and y = dropout(y') is what was kept (same sign wherever the mask keeps): dz = dropout_bwd(dy) * act'(y), column sums. */
int ws_act_bwd_colsum_dropout(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                              float drop_p, uint64_t drop_seed, float* dz, int64_t lddz, float* colsum, void* scratch, void* stream);

/* The same product with multiplicative gates on the epilogue (after bias / residual / activation):
 *   gate_y [m, n] (pitch ldg, NULL = none): y *= LeakyReLU'(gate_y) = (gate_y > 0 ? 1 : gate_slope) -- when this product is the
 *     gradient dX = dY W^T of a layer whose input came out of a LeakyReLU, gate_y is that activated tensor and the
 *     activation backward (models/blocks.py:473-507, autograd of nn.LeakyReLU) costs no pass of its own;
 *   mask [m, n] bytes (pitch ldm, NULL = none): y = mask ? y * mask_scale : 0 -- nn.Dropout (models/architectures.py:354-356),
 *     forward on the activated output and backward on the gradient. */
int ws_gemm_xb_gated_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                             int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                             int32_t act, float slope, const float* gate_y, int64_t ldg, float gate_slope, const uint8_t* mask,
                             int64_t ldm, float mask_scale, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                             void* stream);

/* HIP-event timing of selected kernel launches inside the block calls (bench.py's roofline figure): events are
 * recorded on the launch stream around the K3 launch of blocks with timed = 1.  ws_timer_read synchronises on the
 * events of record i and returns its key (nq, h, ci) and the elapsed milliseconds. */
int ws_timer_reset(void);
int ws_timer_count(void);
int ws_timer_read(int32_t i, int64_t* nq, int32_t* h, int32_t* ci, float* ms);
/* the same record, from the start of the K3 launch to the end of the contraction that follows it: the whole KPConv layer
 * (models/blocks.py:278-374), the unit SURVEY section 8d's B_fwd describes */
int ws_timer_read_layer(int32_t i, float* ms);


/* ------------------------------------------------------------------------------------------
 * Forward-only callers of the hot path: the voting test loop and the sampler potentials.
 * ws_vote_update: utils/tester_PseudoLabel.py:168-194 -- for every point i of a sphere (n rows of `logits` [n,c]):
 *   probs[inds[i], :] = smooth * probs[inds[i], :] + (1 - smooth) * softmax(logits[i, :]); with radius_mask > 0 only the
 *   points with |points[i]|^2 < radius_mask^2 take part (test_radius_ratio * in_radius).  inds are unique inside a sphere.
 * ws_project_confusion: tester_PseudoLabel.py:283-307 + utils/metrics.py:35-110 -- preds[i] = argmax_k probs[proj[i], k]
 *   (first maximum; proj NULL = identity), confusion[t, p] += 1 for t = labels[i] in [0, nc) (int64 [nc, nc], must be
 *   zeroed by the caller; accumulated over calls).
 * ws_potentials_update: datasets/DALES_PseudoLabel.py:335-350 -- potentials[i] += (1 - d2/r^2)^2 for the coarse points
 *   within `radius` of h_center (host double[3]), float64 arithmetic of the KDTree-based reference; then the new minimum
 *   (value, first index) into out_min / out_argmin (device).  scratch: ws_potentials_scratch_bytes(n).
 * The nearest-neighbour projection indices themselves (DALES_PseudoLabel.py:888-892) are column 0 of the K1 radius search.
 * ------------------------------------------------------------------------------------------ */
int ws_vote_update(const float* logits, int64_t n, int32_t c, const float* points, float radius_mask, const int64_t* inds,
                   float* probs, int64_t n_cloud, float smooth, void* stream);
int ws_project_confusion(const float* probs, int32_t c, const int32_t* proj, int64_t m, const int32_t* labels, int32_t* preds,
                         int32_t nc, int64_t* confusion, void* stream);
int64_t ws_potentials_scratch_bytes(int64_t n);
int ws_potentials_update(const float* pot_points, int64_t n, const double* h_center, double radius, double* potentials,
                         double* out_min, int64_t* out_argmin, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * The validation pass that closes every training epoch (csrc/validation.hip): utils/trainer_PseudoLabel.py:368-407
 * (votes) and :423-436 with utils/metrics.py:35-110 (confusion); utils/trainer_WeakLabel.py:312- is the same routine.
 * ws_validation_update: ONE launch for all nb spheres of a batch.  logits [n, c] float32 with leading dimension ld,
 *   input_inds [n] int64, ASCENDING inside every sphere.  Per sphere b, HOST arrays [nb] that travel as kernel arguments
 *   (no copy, no synchronisation): h_offsets (first row), h_lens, h_clouds (cloud id in [0, n_clouds)) and h_overlap, a
 *   bit mask of the other spheres that may share points with b (bit b2 of word b must equal bit b of word b2; pairs on
 *   different clouds and the sphere itself are dropped here).  Spheres lie in ascending, disjoint row ranges inside
 *   [0, n); a row outside every range takes no part.  votes [n_clouds]: device table of the per-cloud vote buffers
 *   [cloud_rows[k], c] float32, cloud_rows int64 [n_clouds] on the device.
 *   Votes (:401-402): votes[cloud_b][inds_b] = smooth * votes[cloud_b][inds_b] + (1 - smooth) * softmax(logits_b) for
 *   b = 0, 1, ... in order, in the float32 expressions of ws_vote_update.  A point listed by several spheres takes the
 *   chain of updates in sphere order: the row in the last such sphere reads the vote row once, applies all of them and
 *   writes it once; no other row touches it (no atomics on floats, the same bits on every run).  radius_mask > 0 (the
 *   test loop, utils/tester_PseudoLabel.py:168-194): only rows with sum(points^2) < radius_mask^2 take part, as updates
 *   and as owners; points [n,3] may be NULL otherwise.
 *   Confusion (labels != NULL): for EVERY row in a sphere, whatever the mask, k = the first maximum of its float32
 *   softmax; confusion[true_row[labels[i]] * nc + pred_row[k]] += 1.  true_row int32 [n_true] and pred_row int32 [c] on
 *   the device carry fast_confusion's label_map for the truth position and the predicted value (validation.py:
 *   confusion_tables); confusion int64 [nc, nc], ACCUMULATED.  labels == NULL: votes only, nc / tables / confusion unused.
 *   status: WS_VAL_STATUS_WORDS int64 on the device, accumulated, never a fault: [WS_VAL_UNSORTED] += 1 per row whose
 *   index is not above its predecessor's in the same sphere (the votes of that batch are then unspecified, every access
 *   stays in bounds); [WS_VAL_BAD_INDEX] += 1 per row whose index is outside [0, cloud_rows[cloud]) (skipped, in the
 *   votes and in every chain); [WS_VAL_BAD_LABEL] += 1 per row whose label is outside [0, n_true) or whose table entry is
 *   outside [0, nc) (left out of the confusion).
 *   c, nc <= 64 and nb <= WS_PYRAMID_MAX_BATCH, else WS_ERR_UNSUPPORTED; other bad sizes, a NULL required pointer or an
 *   inconsistent host array: WS_ERR_INVALID; n == 0: WS_OK and nothing is queued; all found before the device is touched.
 *   The launch is queued on `stream`; nothing synchronises and nothing is read back.
 * ------------------------------------------------------------------------------------------ */
enum { WS_VAL_UNSORTED = 0, WS_VAL_BAD_INDEX = 1, WS_VAL_BAD_LABEL = 2, WS_VAL_STATUS_WORDS = 3 };
int ws_validation_update(const float* logits, int64_t n, int32_t c, int64_t ld, const int64_t* input_inds, const int64_t* labels,
                         const float* points, float radius_mask, const int64_t* h_offsets, const int32_t* h_lens,
                         const int32_t* h_clouds, const uint64_t* h_overlap, int32_t nb, float* const* votes,
                         const int64_t* cloud_rows, int32_t n_clouds, float smooth, const int32_t* true_row, int32_t n_true,
                         const int32_t* pred_row, int32_t nc, int64_t* confusion, int64_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * The end of a test run (csrc/testrun.hip; weasal_amd/testrun.py): utils/tester_PseudoLabel.py:270-348, the same lines
 * of utils/tester_WeakLabel.py, and the sub-cloud form of :225-244.
 * ws_test_outputs: ONE launch per cloud, no [m, c] intermediate.  votes [n_sub, c] float32 (a VoteAccumulator buffer),
 *   proj int32 [m]: the sub-cloud row of every full-resolution point (:277); NULL = identity (the sub-cloud itself, m
 *   rows of votes).  col_of int32 [c], ascending, and label_values int32 [c_all], both on the device: the expanded row
 *   [c_all] of point i holds votes[proj[i], k] at position col_of[k] and zeros at the ignored positions (np.insert,
 *   :297-300); it is stored to proj_probs [m, c_all] float32 when that pointer is given.  k* = the first maximum of the
 *   expanded row (np.argmax: strict >), preds[i] = label_values[k*] (:303) -- a row nobody voted on is all zeros and gets
 *   label_values[0], ignored or not, as the reference does.  targets int32 [m] (label VALUES) and error int8 [m]:
 *   error[i] = preds[i] != targets[i] (:345-348).  confusion int64 [c_all, c_all], ACCUMULATED:
 *   confusion[true_row[targets[i]] * c_all + k*] += 1, true_row int32 [n_true] on the device = fast_confusion's label_map
 *   indexed by the label value (utils/metrics.py:35-110; testrun.value_rows); it needs targets and true_row.
 *   proj_probs, preds, targets, error and confusion are optional (NULL), each on its own.
 *   status: WS_TEST_STATUS_WORDS int64 on the device, accumulated, never a fault: [WS_TEST_BAD_PROJ] += 1 per proj[i]
 *   outside [0, n_sub) (the row takes no part: zeros, preds[i] = label_values[0], left out of the confusion);
 *   [WS_TEST_BAD_TARGET] += 1, when a confusion is asked for, per target outside [0, n_true) or whose table entry is
 *   outside [0, c_all) (left out of the confusion).  A col_of entry outside [0, c_all) drops its column.
 *   c_all <= 64 and c <= c_all, else WS_ERR_UNSUPPORTED; other bad sizes or a NULL required pointer (votes, col_of,
 *   label_values, status; targets for error; targets and true_row for confusion): WS_ERR_INVALID; m == 0: WS_OK and
 *   nothing is queued; all found before the device is touched.  The launch is queued on `stream`; nothing synchronises,
 *   no float is added, every run gives the same bits.
 * ------------------------------------------------------------------------------------------ */
enum { WS_TEST_BAD_PROJ = 0, WS_TEST_BAD_TARGET = 1, WS_TEST_STATUS_WORDS = 2 };
int ws_test_outputs(const float* votes, int64_t n_sub, int32_t c, const int32_t* proj, int64_t m, const int32_t* col_of,
                    const int32_t* label_values, int32_t c_all, const int32_t* targets, const int32_t* true_row, int32_t n_true,
                    float* proj_probs, int32_t* preds, int8_t* error, int64_t* confusion, int64_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Active-learning selection on the votes of a pass over the training clouds (csrc/active.hip).
 * ws_al_point_scores: utils/tester_PseudoLabel.py:400-414 -- per row of probs [n,c] (float32 votes, c <= 32, else
 *   WS_ERR_UNSUPPORTED): entropy = -sum_k p_k * log2f(p_k + 1e-12f), float32, summed in column order; preds = the first
 *   maximum (np.argmax); score = (double)entropy * class_score[pred], class_score [c] float64 on the device =
 *   exp(class_w), computed by the caller.  A row without votes gives (0, 0, 0).
 * ws_al_anchor_scores: utils/tester_WeakLabel.py:436-454 -- anchors as CSR (anchor_ptr [n_anchors + 1], anchor_idx [nnz],
 *   int64, point ids in [0, n)): out[a] = float32(mean_f32(entropy[idx]) * sum of class_score over the classes that
 *   occur among preds[idx]); class_score = exp(-label_sum / len(used)) (:428-434) from the caller.  An empty anchor: 0.
 * ws_topk_select: tester_PseudoLabel.py:416-429, tester_WeakLabel.py:456-465 -- ids [k] = the first k entries of
 *   argsort(-score) once the excluded ids are removed.  The order is exact: descending score, ascending index among
 *   equal scores, -0.0 == +0.0, NaN below every number.  h_exclude [m] is a HOST array (the id lists live on the host in
 *   the reference too), any order, duplicates allowed; an id outside [0, n) or k > n - |unique exclude| is
 *   WS_ERR_INVALID, found before the device is touched.  score [n] float64, ids and scratch (ws_topk_scratch_bytes)
 *   on the device; every kernel is queued on `stream` and nothing is read back.  The ids travel as an n-bit map built
 *   on the host and uploaded from pageable memory: that copy returns only when the work queued on `stream` before it
 *   has finished, so the call waits for its predecessors on the stream (never for its own kernels).  n <= 2^30.
 * ------------------------------------------------------------------------------------------ */
int ws_al_point_scores(const float* probs, int64_t n, int32_t c, const double* class_score, float* entropy, int32_t* preds,
                       double* score, void* stream);
int ws_al_anchor_scores(const float* entropy, const int32_t* preds, int64_t n, const int64_t* anchor_ptr, const int64_t* anchor_idx,
                        int64_t nnz, int64_t n_anchors, const double* class_score, int32_t c, float* out, void* stream);
int64_t ws_topk_scratch_bytes(int64_t n, int64_t k);
int ws_topk_select(const double* score, int64_t n, const int64_t* h_exclude, int64_t m, int64_t k, int64_t* ids, void* scratch,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Selection with a minimum spacing between new labels ("spaced greedy"; opt-in, no counterpart in the reference).
 * Contract: walk the candidates in the priority order of ws_topk_select (used ids removed, descending score, ascending
 *   index among equal scores, -0.0 == +0.0, NaN below every number); accept a candidate iff no point accepted before it
 *   and no used point blocks it; stop after k acceptances; ids = the accepted ids in acceptance order.  q blocks p iff
 *   d2 < s * s, strict, with the coordinates widened to float64, d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded
 *   on its own, and s * s formed in float64 from the float64 spacing s.  No float atomics; every run gives the same ids.
 * ws_al_spaced_select: coords [n, 3] on the device, float32 (coords_f64 == 0) or float64 (!= 0).  cand [m]: device ids
 *   ALREADY in priority order with the used ids removed (a prefix, or a further run, of ws_topk_select's output).
 *   h_used [n_used]: the used ids, a HOST array like ws_topk_select's h_exclude, any order, duplicates allowed; it is
 *   uploaded from pageable memory, so the call waits for its predecessors on the stream.  state: two int64 words on the
 *   device, { acceptances so far, candidates consumed }; ids [k] on the device.  resume == 0 starts a walk (state is
 *   zeroed); resume != 0 continues the walk recorded in state and ids [0, state[0]) with the further run `cand` and keeps
 *   what was accepted.  The caller reads state[0]: below k means the run is used up (state[1] has grown by m).
 *   Two launches (the blocking pass over the used points, skipped when n_used == 0, and the walk of one workgroup whose
 *   accepted coordinates live in LDS) and nothing is read back.  scratch: ws_al_spaced_scratch_bytes(m, n_used, k).
 *   Found before the device is touched: spacing not finite or <= 0, a negative size, a NULL required pointer, a used id
 *   outside [0, n): WS_ERR_INVALID; k > WS_AL_SPACED_MAX_K: WS_ERR_UNSUPPORTED.  k == 0 or m == 0: WS_OK and nothing is
 *   launched (resume == 0 with a non-NULL state zeroes it).  An id of cand outside [0, n) is never dereferenced or accepted.
 * ws_al_spaced_variant: the launches a call takes, from the launcher's own plan; nothing is read or launched.  Text:
 *   "spaced_used_kernel<float|double> blocks=.. tiles=..|no used pass + spaced_walk_kernel<float|double> chunks=..
 *   tail=<m mod 1024> resume=0|1", or "none (k == 0|m == 0)".
 * ------------------------------------------------------------------------------------------ */
#define WS_AL_SPACED_MAX_K 6144
int64_t ws_al_spaced_scratch_bytes(int64_t m, int64_t n_used, int64_t k);
int ws_al_spaced_select(const void* coords, int32_t coords_f64, int64_t n, const int64_t* cand, int64_t m, const int64_t* h_used,
                        int64_t n_used, double spacing, int64_t k, int64_t* ids, int64_t* state, int32_t resume, void* scratch,
                        void* stream);
int ws_al_spaced_variant(int32_t coords_f64, int64_t n, int64_t m, int64_t n_used, double spacing, int64_t k, int32_t resume,
                         char* text, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * Pseudo-label refinement on the votes of a pass over the training clouds (csrc/refine.hip): pseudoLabel_refinement.py.
 * ws_weak_mask: :63-68 -- mask [n] uint32, bit k set while class k survives: every word starts as the low c bits
 *   (weak = ones) and takes the AND of anchor_bits[a] (the 0/1 label row of anchor a, bit k = column k, packed by the
 *   caller) for every selected anchor a that lists the point (weak[idx_a] *= lb_a).  Anchors as CSR like
 *   ws_al_anchor_scores (anchor_ptr [n_anchors + 1], anchor_idx [nnz], int64).  anchor_sel [n_sel] int64: the rows that
 *   take part, any order, duplicates allowed (the dictionary after active.select_anchors); NULL = all n_anchors rows
 *   (n_sel is then ignored and must be 0); non-NULL with n_sel = 0 = none.  A duplicate index applies once (AND).
 * ws_refine_labels: :123-151 -- for point i < n, r = proj[i] (int32; NULL: r = i, and m >= n is required) selects the
 *   row of probs [m, c] float32 and preds [m] int32 (:123-125, :136, :144); mask [n] is NOT projected.
 *   labels[i] = (double) max_k(mask bit k ? probs[r, k] : 0) < thr ? no_label : preds[r]  (:137, :143-145; thr is the
 *   host's double 0.01 * threshold; for votes, which are >= 0, the maximum over the surviving classes, 0 without any);
 *   counts[v] += 1 for every written label v in [0, n_counts) (:148-151: by value, after emptying), int64, ACCUMULATED:
 *   one buffer serves all tiles, the caller zeroes it once.  n_counts <= 4096, else WS_ERR_UNSUPPORTED.
 * Both: c <= 32, else WS_ERR_UNSUPPORTED; c < 1, a negative size or a NULL required pointer: WS_ERR_INVALID; n == 0:
 *   WS_OK and nothing is queued; all found before the device is touched.  Every kernel is queued on `stream`; nothing
 *   synchronises and nothing is read back.  An index outside its range -- anchor_idx outside [0, n), anchor_sel outside
 *   [0, n_anchors), proj outside [0, m) -- is never dereferenced: the entry is skipped (a bad proj[i] writes no_label
 *   and is counted in no class) and status[WS_REFINE_BAD_*] += 1.  status: 3 int64 words on the device, accumulated
 *   like counts; the caller zeroes them and reads them with the counts.
 * ------------------------------------------------------------------------------------------ */
enum { WS_REFINE_BAD_ANCHOR_IDX = 0, WS_REFINE_BAD_ANCHOR_SEL = 1, WS_REFINE_BAD_PROJ = 2, WS_REFINE_STATUS_WORDS = 3 };
int ws_weak_mask(uint32_t* mask, int64_t n, int32_t c, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz,
                 const uint32_t* anchor_bits, int64_t n_anchors, const int64_t* anchor_sel, int64_t n_sel, int64_t* status,
                 void* stream);
int ws_refine_labels(const float* probs, const int32_t* preds, int64_t m, int32_t c, const uint32_t* mask, const int32_t* proj,
                     int64_t n, double thr, int32_t no_label, int32_t* labels, int64_t* counts, int32_t n_counts, int64_t* status,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * The weak-label anchors of one tile (csrc/anchors.hip): utils/anchors.py, driven by datasets/DALES_WeakLabel.py:201-269.
 * Distances: a float32 coordinate widened to float64, d = p - a per axis, d2 = (dx*dx + dy*dy) + dz*dz, every product
 *   and sum rounded (no FMA); inside iff d2 <= radius*radius (sklearn's query_radius keeps the boundary).
 * h_grid: HOST double [7] = { origin x, y, z, cell, nx, ny, nz } of a uniform grid over the searched centres, cell >=
 *   radius, z the fastest axis; cell_start int32 [nx*ny*nz + 1] and cell_item int32 [items] list the items of every cell.
 *   The grid proposes candidates (27 cells), the comparison above decides.
 * ws_anchor_bounds: utils/anchors.py:33-38 -- bounds [6] float32 on the device = { x min, x max, y min, y max, z min,
 *   z max } of points [n,3]; n >= 1.
 * ws_anchor_members_plan: :83-99 -- per input anchor a < a0 (anchors [a0,3] float64): counts[a] = the points inside
 *   (query_radius, :87), bits[a] = OR of 1 << labels[i] over them (np.unique + cloud_labels, :94-98); slot [a0 + 1] = the
 *   exclusive scan of (counts > 0), i.e. the index among the survivors (:91), ptr32 [a0 + 1] that of counts.
 *   totals[WS_ANCHOR_TOTAL_ROWS] = survivors, [WS_ANCHOR_TOTAL_NNZ] = members in all, summed in 64 bits.  A label
 *   outside [0, n_class) sets no bit and status[WS_ANCHOR_BAD_LABEL] += 1 per such point (the reference: IndexError).
 *   n_class <= 32 and n, a0 < 2^31, else WS_ERR_UNSUPPORTED.  scratch: ws_anchor_scratch_bytes(a0).
 * ws_anchor_members_fill: :91-103 -- after ONE host read of totals: kept [A] = the input index of every survivor, in
 *   order; anchor_ptr [A + 1], anchor_idx [nnz] ascending inside every anchor (filled through atomic cursors, then sorted
 *   per anchor: the same bytes on every run); centres [A,3]; anchor_bits [A].  cursor: int32 [a0] scratch.  nnz >= 2^31:
 *   WS_ERR_CAPACITY (the offsets are planned in 32 bits).
 * ws_anchor_pairs_plan / _fill: :114-121 -- the candidates of the overlap pass: positions s < t of the selection
 *   (sel [n_sel] int64 anchor ids, duplicates allowed, DALES_WeakLabel.py:241-263; NULL: all n_anchors, n_sel =
 *   n_anchors) whose centres are within `radius` (1.5 * sub_radius), same recipe.  The grid lists POSITIONS.
 *   pair_cnt / pair_ptr [n_sel + 1]; totals[WS_ANCHOR_TOTAL_ROWS] = pairs; then pair_i / pair_j [n_pairs] int32 in
 *   (s, t) lexicographic order.  A sel entry outside [0, n_anchors) has no pairs and status[WS_ANCHOR_BAD_SEL] += 1.
 * ws_anchor_overlap_plan: :122-134 -- inter_cnt[p] = |list(i) & list(j)| when the label bits differ (:134), else 0;
 *   new_slot / new_ptr [n_pairs + 1] their scans, sel_ptr [n_sel + 1] the scan of the selected lists' lengths;
 *   totals = { new anchors, their members, members of the selection }.  scratch: ws_anchor_scratch_bytes(max(n_pairs,
 *   n_sel)).  One wave per pair, the shorter list binary-searched in the longer.
 * ws_anchor_overlap_fill: :130-138 -- after ONE host read of totals: rows [0, n_sel) of the output copy the selected
 *   anchors (select_anchors, :145-160), rows n_sel + new_slot[p] are the new ones in pair order: members = the
 *   intersection, ascending (:130, ballot + prefix popcount, no atomics); bits = AND (:137); centre = float64 mean of
 *   the members' widened coordinates (:135; summed in a fixed order).  New anchors are never paired themselves.
 * All: every kernel is queued on `stream`, nothing synchronises, nothing is read back; sizes are checked before the
 *   device is touched.  status: WS_ANCHOR_STATUS_WORDS int64 on the device, accumulated; totals: WS_ANCHOR_TOTAL_WORDS
 *   int64 on the device, rewritten by every plan.
 * ------------------------------------------------------------------------------------------ */
enum { WS_ANCHOR_BAD_LABEL = 0, WS_ANCHOR_BAD_SEL = 1, WS_ANCHOR_STATUS_WORDS = 2 };
enum { WS_ANCHOR_TOTAL_ROWS = 0, WS_ANCHOR_TOTAL_NNZ = 1, WS_ANCHOR_TOTAL_BASE = 2, WS_ANCHOR_TOTAL_WORDS = 3 };
int ws_anchor_bounds(const float* points, int64_t n, float* bounds, void* stream);
int64_t ws_anchor_scratch_bytes(int64_t items);
int ws_anchor_members_plan(const float* points, const int32_t* labels, int64_t n, int32_t n_class, const double* anchors, int64_t a0,
                           double radius, const double* h_grid, const int32_t* cell_start, const int32_t* cell_item,
                           int32_t* counts, int32_t* slot, int32_t* ptr32, uint32_t* bits, int64_t* totals, int64_t* status,
                           void* scratch, void* stream);
int ws_anchor_members_fill(const float* points, int64_t n, const double* anchors, int64_t a0, double radius, const double* h_grid,
                           const int32_t* cell_start, const int32_t* cell_item, int32_t* counts, const int32_t* slot,
                           const int32_t* ptr32, const uint32_t* bits, int64_t n_kept, int64_t nnz, int64_t* kept, int64_t* anchor_ptr,
                           int64_t* anchor_idx, double* centres, uint32_t* anchor_bits, int32_t* cursor, void* stream);
int ws_anchor_pairs_plan(const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel, double radius,
                         const double* h_grid, const int32_t* cell_start, const int32_t* cell_item, int32_t* pair_cnt,
                         int32_t* pair_ptr, int64_t* totals, int64_t* status, void* scratch, void* stream);
int ws_anchor_pairs_fill(const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel, double radius,
                         const double* h_grid, const int32_t* cell_start, const int32_t* cell_item, const int32_t* pair_ptr,
                         int64_t n_pairs, int32_t* pair_i, int32_t* pair_j, void* stream);
int ws_anchor_overlap_plan(const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz, const uint32_t* anchor_bits,
                           int64_t n_anchors, const int64_t* sel, int64_t n_sel, const int32_t* pair_i, const int32_t* pair_j,
                           int64_t n_pairs, int32_t* inter_cnt, int32_t* new_slot, int32_t* new_ptr, int32_t* sel_ptr, int64_t* totals,
                           void* scratch, void* stream);
int ws_anchor_overlap_fill(const float* points, int64_t n, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz,
                           const uint32_t* anchor_bits, const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel,
                           const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs, const int32_t* inter_cnt,
                           const int32_t* new_slot, const int32_t* new_ptr, const int32_t* sel_ptr, int64_t n_new, int64_t nnz_new,
                           int64_t nnz_sel, int64_t* out_ptr, int64_t* out_idx, uint32_t* out_bits, double* out_centres, void* stream);

/* ------------------------------------------------------------------------------------------
 * The per-sphere regions of the weak-label sampler and their means (csrc/regions.hip): datasets/DALES_WeakLabel.py:424-451
 * (identical in Vaihingen3D_WeakLabel.py:418-445) and the averaging of models/architectures.py:752-768.
 * A batch holds n_spheres <= 64 spheres; sphere s owns the rows row_off[s] .. row_off[s + 1] of the stacked batch, its slice
 * of input_inds [n_rows] (ASCENDING tile point ids, the sampler's order) and its float64 centre.  The (sphere, anchor) pairs
 * are numbered pair_off[s] + a, a < anchors of the sphere's tile: `pairs` in all, sphere by sphere, so that the pair order
 * is (sphere, ascending anchor id).  row_off / pair_off: int64 [n_spheres + 1] on the device.  The tile-dependent entries
 * take one tile and `group` [n_group] int32, the spheres of the batch that were cut from it: one call per tile.
 * ws_region_cut_count: :433-449 -- for every pair of the group: candidate iff d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius,
 *   d = anchor centre - sphere centre, float64, every product and sum rounded (radius is the host's in_radius - sub_radius
 *   - 0.01, :434); cnt[pair] = the members of the anchor (anchor_ptr / anchor_idx, the AnchorSet's CSR) found in the
 *   sphere's slice by binary search (np.in1d, :445), or 0 when the pair is no candidate, when nothing is found, or when the
 *   only one found is the slice's row 0 (`if idx.any()`, :449).  Every pair of the group is written.
 * ws_region_cut_scan: slot / ptr32 [pairs + 1] = exclusive scans of (cnt > 0) and cnt; words[WS_REGION_TOTAL_ROWS] = kept
 *   regions, [WS_REGION_TOTAL_NNZ] = their rows in all; cloud_lb [n_spheres, n_class] float32, column k = 1 iff a row of
 *   the sphere has label k (:474-476; labels int64 [n_rows], already mapped); a label outside [0, n_class) sets nothing
 *   and words[WS_REGION_BAD_LABEL] += 1.  words: WS_REGION_WORDS int64, rewritten here: the ONE thing the host reads.
 *   pairs = 0 computes cloud_lb only.  scratch: ws_region_scratch_bytes(pairs).  n_class <= 32, pairs < 2^31.
 * ws_region_cut_fill: :445-451 -- after the read, for the kept pairs of the group, region r = slot[pair]: out_ptr[r] =
 *   ptr32[pair] (the caller sets out_ptr[n_regions] = nnz), out_idx = row_off[s] + position in the slice, ascending
 *   (np.searchsorted, :447; ballot + prefix popcount, no atomics), out_reg [nnz] int32 = r at every row of the region,
 *   out_sphere [R] int32, out_anchor [R] int64, out_lb [R, n_class] float32 unpacked from anchor_bits (:451), out_inv_len
 *   [R] float32 = 1.0f / (float) length.
 * ws_region_mean_fwd: architectures.py:752-768 -- out[r, :] = (sum over i in region_ptr[r] .. region_ptr[r + 1] of
 *   x[region_idx[i], :]) * inv_len[r], x [n, w] float32 row-major, w <= 256 (else WS_ERR_UNSUPPORTED), float32 sums in an
 *   order fixed by w and the region's length alone.  Every element of out [n_regions, w] is stored.
 * ws_region_mean_bwd: grad_x[p, :] = sum over i in t_ptr[p] .. t_ptr[p + 1] of grad_out[t_reg[i], :] * inv_len[t_reg[i]],
 *   in that order (t_ptr int64 [n + 1], t_reg int32 [nnz]: the transpose point -> regions).  No atomics; every row of
 *   grad_x [n, w] is stored, a row in no region as zeros.
 * All: queued on `stream`, nothing synchronises, nothing is read back; sizes are checked before the device is touched; an
 *   offset or index outside its range is never dereferenced (the entry is skipped).  The same bytes on every run.
 * ------------------------------------------------------------------------------------------ */
enum { WS_REGION_TOTAL_ROWS = 0, WS_REGION_TOTAL_NNZ = 1, WS_REGION_BAD_LABEL = 2, WS_REGION_WORDS = 3 };
enum { WS_REGION_MAX_SPHERES = 64, WS_REGION_MAX_WIDTH = 256 };
int64_t ws_region_scratch_bytes(int64_t pairs);
int ws_region_cut_count(const double* centres, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t anchor_nnz,
                        int64_t n_anchors, const int32_t* group, int32_t n_group, int32_t n_spheres, const double* sphere_centres,
                        const int64_t* row_off, const int64_t* pair_off, const int64_t* input_inds, int64_t n_rows, int64_t pairs,
                        double radius, int32_t* cnt, void* stream);
int ws_region_cut_scan(int32_t* cnt, int64_t pairs, int32_t* slot, int32_t* ptr32, const int64_t* labels, const int64_t* row_off,
                       int64_t n_rows, int32_t n_spheres, int32_t n_class, float* cloud_lb, int64_t* words, void* scratch, void* stream);
int ws_region_cut_fill(const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t anchor_nnz, const uint32_t* anchor_bits,
                       int64_t n_anchors, const int32_t* group, int32_t n_group, int32_t n_spheres, const int64_t* row_off,
                       const int64_t* pair_off, const int64_t* input_inds, int64_t n_rows, int64_t pairs, const int32_t* cnt,
                       const int32_t* slot, const int32_t* ptr32, int64_t n_regions, int64_t nnz, int32_t n_class, int64_t* out_ptr,
                       int64_t* out_idx, int32_t* out_reg, int32_t* out_sphere, int64_t* out_anchor, float* out_lb, float* out_inv_len,
                       void* stream);
int ws_region_mean_fwd(const float* x, int64_t n, int32_t w, const int64_t* region_ptr, const int64_t* region_idx, int64_t nnz,
                       const float* inv_len, int64_t n_regions, float* out, void* stream);
int ws_region_mean_bwd(const float* grad_out, int64_t n_regions, int32_t w, const int64_t* t_ptr, const int32_t* t_reg, int64_t nnz,
                       const float* inv_len, int64_t n, float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * The sphere sampler on tiles resident in device memory: datasets/DALES_PseudoLabel.py:265-518 (`potential_item`) with
 * datasets/common.py:252-334 (`augmentation_transform`), a whole batch per call and no host round trip per sphere.
 *
 * ws_sampler_create / _destroy: the table of clouds (at most 4096) and the chain's scratch.
 * ws_sampler_add_cloud: one tile -- sub_points [n,3] f32, sub_labels [n] i32 (NULL when every batch is cut with
 *   labels_zero), pot_points [p,3] f32 (DALES_PseudoLabel.py:826-845), potentials [p] f64 (initialised by the caller,
 *   :211; updated in place by ws_sampler_batch).  Computes the cloud's (min, first arg-min) pair (:212-214); synchronises.
 *   The pointers must stay valid for the life of the sampler.
 * ws_sampler_batch: queues the chain for max_spheres (<= 64) sphere slots on `stream` and returns; nothing synchronises.
 *   Per slot k (:321-408), skipped once `done` is set:
 *     cloud = first arg-min of the per-cloud minima, point = its arg-min (:322-323);
 *     centre = f64(pot_points[point]) + h_draws[k].noise (:329-333; pot_points itself is NOT modified);
 *     members = { i : (dx*dx + dy*dy) + dz*dz <= in_radius^2 }, d = f64(sub_points[i]) - centre, float64, no FMA, in
 *       ASCENDING index order (the KD-tree's :358 set, index-ordered);
 *     n < 2: dropped, n_fail += 1 (:367-373); row_off + n > capacity_rows: `overflow` and `done` are set and the slot is
 *       left undone (nothing written, potentials untouched) -- call again with resume = 1, larger buffers holding the rows
 *       written so far, the same draws: the chain goes on with this slot;
 *     otherwise the potentials take their Tukey update (:340-350, float64: dist = sqrt(rd), d2 = dist^2,
 *       (1 - d2 / r^2)^2; update_potentials = 0 skips it: set 'ERF', :344) and the rows row_off .. row_off + n receive
 *       points = (((p0 R[0,j] + p1 R[1,j]) + p2 R[2,j]) * scale[j]) + augment_noise * N(0,1), p = f32(f64(sub_points[i])
 *       - centre) (:376, common.py:316; float32, no FMA; the normal deviate is a pure function of (seed, seq0 + k, row
 *       in the sphere, j): counter hash of ws_dropout_apply + Box-Muller; augment_noise = 0 adds nothing),
 *       features = [1] (fd = 1) or [1, f32(f64(z') + centre_z), z'] (fd = 3) (:389, :430-434; any other fd:
 *       WS_ERR_UNSUPPORTED with the reference's message), labels = label_lut[sub_labels[i]] (:381; -1 outside
 *       [0, lut_n); NULL lut: the raw label; labels_zero: 0, :377-378), input_inds = i; the slot's lengths / scales /
 *       rots / cloud_inds / point_inds entries are written at the sphere's ordinal (:419-427, :456);
 *       `done` once row_off > batch_limit (:404-408) or the last slot is used.
 *   h_draws: max_spheres records of ws_sampler_draw_bytes() = 72 bytes { double noise[3]; float rot[9]; float scale[3]; }
 *   (host; pinned memory makes the upload asynchronous).  d_state: ws_sampler_state_bytes() bytes of device memory, int64
 *   words { done, overflow, n_spheres, n_fail, row_off, attempts, cur_slot, cur_flags } followed by 64 slot records of 8
 *   words { n, cloud, point, row, ord (-1: not kept), centre x, y, z as float64 }: the one thing the host reads back.
 *   Launches: 1 + 3 * max_spheres, whatever the data.
 * ------------------------------------------------------------------------------------------ */
typedef struct ws_sampler ws_sampler;
int ws_sampler_create(ws_sampler** ws);
void ws_sampler_destroy(ws_sampler* ws);
int ws_sampler_add_cloud(ws_sampler* ws, const float* sub_points, const int32_t* sub_labels, int64_t n, const float* pot_points,
                         double* potentials, int64_t p, void* stream);
int64_t ws_sampler_state_bytes(void);
int64_t ws_sampler_draw_bytes(void);
int ws_sampler_batch(ws_sampler* ws, const void* h_draws, int32_t max_spheres, int32_t resume, int64_t batch_limit, double in_radius,
                     float augment_noise, uint64_t seed, uint64_t seq0, int32_t fd, const int32_t* label_lut, int32_t lut_n,
                     int32_t labels_zero, int32_t update_potentials, float* out_points, float* out_features, int64_t* out_labels,
                     int64_t* out_input_inds, int32_t* out_lengths, float* out_scales, float* out_rots, int32_t* out_cloud_inds,
                     int32_t* out_point_inds, int64_t capacity_rows, void* d_state, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same chain with colour columns and with centres from a list, and the class-balanced draw of that list.
 *
 * ws_sampler_add_cloud also takes pot_points = potentials = NULL with p = 0: a tile that only the random mode serves.
 * ws_sampler_set_colors: sub_colors [n, ncol] f32 of an added cloud, 1 <= ncol <= 3 (any other ncol: WS_ERR_UNSUPPORTED);
 *   replaces `self.input_colors[cloud_ind][input_inds]` (datasets/Vaihingen3D_PseudoLabel.py:366, :562; Vaihingen3D_WeakLabel.py
 *   :463-535).  Every cloud of a sampler carries the same ncol.  Synchronises; the pointer must stay valid.
 * ws_sampler_batch_items: ws_sampler_batch behind one descriptor; the fields named as its arguments mean what they mean
 *   there, and with no colours, h_colour_keep = NULL and random_centres = 0 it queues the same launches and writes the same
 *   bits (ws_sampler_batch fills this descriptor and calls it; on a sampler with colours it keeps every slot's).  In addition:
 *     features = [1] followed by the first fd - 1 columns of [colours..., f32(f64(z') + centre_z), z']
 *       (Vaihingen3D_PseudoLabel.py:383, :424-432); accepted fd: {1, 3} without colours, {1, 1 + ncol, 3 + ncol} with them,
 *       any other: WS_ERR_UNSUPPORTED with the reference's message ('... 1 and 3' / '... 1, 2 and 4' for ncol = 1);
 *     h_colour_keep: host int32 [max_spheres] or NULL (all 1) -- slot k with 0 writes +0.0f in its colour columns
 *       (`if np.random.rand() > config.augment_color: input_colors *= 0`, :379-380), else the colour is copied bit for bit;
 *     random_centres = 1: `random_item` (datasets/DALES_PseudoLabel.py:520-640, Vaihingen3D_PseudoLabel.py:516-643).  Slot k
 *       takes cloud = epoch_inds[0, e], point = epoch_inds[1, e], e = *epoch_i (device int64 [2, n_centres] and device
 *       int64; indices outside the tables are clamped into them), centre = f64(sub_points[point]) + noise (:547-551; the
 *       tile itself is NOT modified), point_inds = point.  *epoch_i advances by one, wrapping at n_centres (:538-540), with
 *       every sphere the chain commits, kept or dropped (n < 2; the reference has no such guard), and stays where it is
 *       for a sphere left undone by `overflow`.  No potential is read or written, update_potentials is ignored.
 *   Launches: 1 + 3 * max_spheres in both modes, whatever the data.
 * ws_sampler_class_counts / ws_sampler_class_select: the lookups of the class-balanced centre draw (`*Sampler.__iter__`,
 *   datasets/DALES_PseudoLabel.py:961-975) on the resident labels.  values: device int32 [n_class <= 64], the raw label
 *   values of the non-ignored classes.  _counts: out_counts[cloud, c] (device int64 [n_clouds, n_class]) =
 *   len(np.where(sub_labels == values[c])[0]) (:965); two launches; keeps per-chunk scanned counts inside `ws`.  _select:
 *   triples device int64 [n_triples, 3] rows (cloud, c, position) -> out_points[t] = np.where(sub_labels == values[c])[0]
 *   [position], or -1 when the class has no such member; one launch; needs the _counts of the same labels first.
 *   Neither synchronises.
 * ------------------------------------------------------------------------------------------ */
typedef struct ws_sampler_items {
    const void* h_draws;
    const int32_t* h_colour_keep;
    int32_t max_spheres, resume;
    int64_t batch_limit;
    double in_radius;
    float augment_noise;
    int32_t fd;
    uint64_t seed, seq0;
    const int32_t* label_lut;
    int32_t lut_n, labels_zero, update_potentials, random_centres;
    const int64_t* epoch_inds;
    int64_t n_centres;
    int64_t* epoch_i;
    float* out_points;
    float* out_features;
    int64_t* out_labels;
    int64_t* out_input_inds;
    int32_t* out_lengths;
    float* out_scales;
    float* out_rots;
    int32_t* out_cloud_inds;
    int32_t* out_point_inds;
    int64_t capacity_rows;
    void* d_state;
    void* stream;
} ws_sampler_items;
int64_t ws_sampler_items_bytes(void);   /* sizeof(ws_sampler_items) */
int ws_sampler_set_colors(ws_sampler* ws, int32_t cloud, const float* colors, int32_t ncol, void* stream);
int ws_sampler_batch_items(ws_sampler* ws, const ws_sampler_items* items);
int ws_sampler_class_counts(ws_sampler* ws, const int32_t* values, int32_t n_class, int64_t* out_counts, void* stream);
int ws_sampler_class_select(ws_sampler* ws, const int32_t* values, int32_t n_class, const int64_t* triples, int64_t n_triples,
                            int64_t* out_points, void* stream);

/* nn.Dropout on the decoder output in front of the head, training mode (models/architectures.py:345-346): out[i] = keep(i) ? in[i] / (1 - p) : 0,
 * keep(i) a pure function of (seed, i) (counter-based; Bernoulli(1 - p)): the backward is the same call on the incoming
 * gradient with the same seed, no mask is stored.  in / out float32 [n], 16-byte aligned; in == out allowed. */
int ws_dropout_apply(const float* in, int64_t n, float p, uint64_t seed, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The two ends of the training step around the network (forward + backward + SGD).
 * ws_softmax_ce_fwd / _bwd: models/architectures.py:362-373 (KPFCNN.loss) -- the label mapping (:362-365; lut [lut_n]
 *   maps raw label values to class positions, its last entry is the spare -1 every out-of-table label takes; lut NULL =
 *   labels are positions, < 0 ignored) and torch.nn.CrossEntropyLoss(weight = class_w or NULL, ignore_index = -1) over the
 *   n rows of logits [n, c] (row pitch ldl), c <= 64: loss[0] = weighted mean over the valid rows, wsum[0] = sum of their
 *   weights (both device floats; no valid row -> nan like the stock loss).  The backward takes d loss as a device
 *   float (grad_loss[0]) so that nothing synchronises; rows with ignored labels get zeros.
 * ws_sgd_step: utils/trainer_PseudoLabel.py:216-218 with the optimizer of :72-82 -- clip_grad_value_(clip_value; <= 0 =
 *   off), weight decay, momentum buffer (first != 0: buf = g, the first step of torch.optim.SGD) and p -= lr * buf for
 *   `count` tensors in one pass; h_params / h_grads / h_bufs / h_sizes are HOST arrays of device pointers / element counts
 *   (one parameter group per call: lr, momentum and weight_decay are per group).  No dampening, no Nesterov.
 * ------------------------------------------------------------------------------------------ */
int64_t ws_softmax_ce_scratch_bytes(int64_t n);
int ws_softmax_ce_fwd(const float* logits, int64_t n, int32_t c, int64_t ldl, const int64_t* labels, const int64_t* lut,
                      int32_t lut_n, const float* class_w, float* loss, float* wsum, void* scratch, void* stream);
int ws_softmax_ce_bwd(const float* logits, int64_t n, int32_t c, int64_t ldl, const int64_t* labels, const int64_t* lut,
                      int32_t lut_n, const float* class_w, const float* grad_loss, const float* wsum, float* dlogits, int64_t ldd,
                      void* stream);
int ws_sgd_step(float* const* h_params, const float* const* h_grads, float* const* h_bufs, const int64_t* h_sizes, int32_t count,
                float lr, float momentum, float weight_decay, float clip_value, int32_t first, void* stream);

/* ------------------------------------------------------------------------------------------
 * Clip by norm inside the update: utils/trainer_WeakLabel.py:216 (torch.nn.utils.clip_grad_norm_) followed by
 * optimizer.step() (the optimizer of :72-82), weasal_amd/csrc/optim.hip.
 * ws_grad_norm: out[0] = total 2-norm of the `count` gradient tensors (HOST arrays of device pointers / element counts, all
 *   parameter groups in one call), out[1] = coef = min(1, max_norm / (out[0] + 1e-6)); out is device memory, nothing is read
 *   back.  Every workgroup writes the sum of squares of its WS_SGD_CHUNK elements into a slot of its own, a finishing launch
 *   adds the slots in index order: no float atomic, run-to-run bit-identical.  slots: device scratch of nslots >=
 *   ws_grad_norm_slots(h_sizes, count) floats.  The tensor table travels in the kernel arguments, WS_SGD_MAX tensors per launch.
 * ws_sgd_step_scaled: ws_sgd_step with g = g * coef[0] (the device word ws_grad_norm wrote) in front of weight decay and
 *   momentum instead of the clamp; the scaled gradient is written back to h_grads (what clip_grad_norm_ leaves in p.grad).
 * ------------------------------------------------------------------------------------------ */
#define WS_SGD_MAX 96
#define WS_SGD_CHUNK 4096
int64_t ws_grad_norm_slots(const int64_t* h_sizes, int32_t count);
int ws_grad_norm(const float* const* h_grads, const int64_t* h_sizes, int32_t count, float max_norm, float* slots, int64_t nslots,
                 float* out, void* stream);
int ws_sgd_step_scaled(float* const* h_params, float* const* h_grads, float* const* h_bufs, const int64_t* h_sizes, int32_t count,
                       float lr, float momentum, float weight_decay, const float* coef, int32_t first, void* stream);

/* ------------------------------------------------------------------------------------------
 * The log line of a training step, kept on the device: utils/trainer_PseudoLabel.py:209,244-253 and
 * utils/trainer_WeakLabel.py:208,243-252 (net.output_loss, net.reg_loss or the gradient norm, KPFCNN.accuracy of
 * models/architectures.py:386-399, :786-799), weasal_amd/csrc/stats.hip.
 * ws_step_stats: writes record `row` of `ring` [cap] (device memory): the three floats are bit copies of the device scalars
 *   out_loss[0], reg_loss[0], extra[0] (each may be NULL: 0), correct = #{i < n : argmax_c logits[i, :] == target_i} with
 *   torch.argmax's rules (the first maximum on ties, a row with NaN predicts its first NaN) and the label mapping of
 *   ws_softmax_ce_fwd (lut [lut_n], last entry the spare -1; lut NULL = labels are positions, < 0 ignored).  Ignored rows
 *   never count: the caller divides by all n rows as KPFCNN.accuracy does.  logits float32 [n, c], row pitch ldl >= c,
 *   c <= WS_STEP_STATS_MAX_C (what ws_softmax_ce_fwd accepts), n < 2^31.  The record is zeroed by the call; the count is one
 *   ballot + popcount per wave and one int32 atomic per workgroup of a grid-stride launch of at most WS_STEP_STATS_BLOCKS
 *   workgroups of 256 rows: no float atomic, run-to-run identical.  n = 0 writes correct = 0 and launches nothing else.
 *   Nothing is read back; the other records of the ring are not touched.
 * ------------------------------------------------------------------------------------------ */
#define WS_STEP_STATS_MAX_C 64
#define WS_STEP_STATS_BLOCKS 256
typedef struct ws_step_record {
    float out_loss, reg_loss, extra;
    int32_t correct;
} ws_step_record;
int ws_step_stats(const float* logits, int64_t n, int32_t c, int64_t ldl, const int64_t* labels, const int64_t* lut,
                  int32_t lut_n, const float* out_loss, const float* reg_loss, const float* extra, ws_step_record* ring,
                  int64_t cap, int64_t row, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deformable KPConv, the fast path of BASELINE config 5 (models/blocks.py:244-325, 366-367 with KP_influence = 'linear',
 * aggregation_mode = 'sum'; neighbour rows of several hundred columns: datasets/common.py:500-502).
 *
 * ws_kpconv_deform_prepare: blocks.py:250-267, 287-288 in one pass.  offset_features [n, od] f32 (od = 3k, or 4k when
 *   modulated) -> deformed_kp [n,k,3] = offset * extent + kernel_points (two roundings, like the reference's mul and
 *   add), modulations [n,k] = 2 sigmoid(last k columns) (NULL / ignored when not modulated), and kp4 [n,k] float4 =
 *   (x, y, z, modulation or 1): the packed operand of the entries below (16-byte aligned).  deformed_kp may be NULL.
 *   kp_rmax (device float, may be NULL) receives max |deformed kernel point| of the call: ws_kpconv_gather_bwd_x_grid_wide
 *   drops the pairs farther apart than kp_rmax + extent (no kernel point reaches them); given kp4 without kp_rmax it takes
 *   the same maximum over kp4 itself first, so its result does not depend on whether the caller kept the scalar.
 * rows_sorted != 0 (ws_kpconv_gather_fwd_def, _bwd_geom_def, ws_kpconv_gather_fwd_ex): the caller vouches that every index
 *   row is sorted by distance from its query (what the radius search delivers).  A neighbour beyond the reach of every
 *   kernel point (max |kp| + extent) has 15 zero influences and one beyond max_k (sqrt(min_d2[k]) + |kp_k|) cannot lower
 *   a minimum: the walk over the row stops there.  Exact (the skipped terms are zeros); with the deformable search radius
 *   (2 r against a reach of ~1.1 r) it skips most of every row.
 * ws_kpconv_deform_prepare_bwd: d offset_features [n, od] from d_kp4 [n,k,4] (NULL = zero) and / or a second gradient
 *   d_deformed_kp [n,k,3] of the positions (NULL = none; the regulariser's).
 * ws_kpconv_gather_fwd_def / _bwd_x_def / _bwd_geom_def: ws_kpconv_gather_fwd / _bwd_x / _bwd_geom for that mode with
 *   kp4 in place of (kernel_points, deformed_kp, modulations).  The in-range filter of blocks.py:301-325 is implied: with
 *   the linear influence a neighbour without a kernel point inside the extent has 15 zero influences.  _bwd_geom_def
 *   (the dense product dwf[q] . x[neighbours]^T on the matrix core; ci % 16 == 0) writes d_kp4 [nq,k,4] =
 *   (d x, d y, d z, d modulation), including the min_d2 path when d_min_d2 != NULL.  rows_bf16 != 0: the feature rows
 *   x / wf / dwf / dx are bf16.
 * ws_kpconv_gather_bwd_x_grid_wide: ws_kpconv_gather_bwd_x_grid for ANY in-degree (rows wider than 128 neighbours): the
 *   candidate slab is a queue that is consumed 64 pairs at a time.  Rigid (kp4 NULL, kernel_points given) or deformable
 *   (kp4); linear influence, sum aggregation.  rows / rows_h as in ws_kpconv_gather_bwd_x_grid_gated (NULL = walk the grid).
 * ws_p2p_regularizer_fwd / _bwd: models/architectures.py:24-57 for ONE layer.  out2[0] = mean |min_d2 / extent^2|,
 *   out2[1] = sum_i mean_n |sum_{j != i} min(|kp_i - kp_j| / extent - repulse_extent, 0)^2| / k (the other points
 *   detached); positions from deformed_kp [n,k,3] or, when that is NULL, from kp4.  The backward takes g2 = (d loss /
 *   d out2[0], d loss / d out2[1]) as DEVICE floats and writes d_min_d2 [n,k], d_deformed_kp [n,k,3].
 *   scratch: ws_p2p_regularizer_scratch_bytes(n).
 * ------------------------------------------------------------------------------------------ */
int ws_kpconv_deform_prepare(const float* offset_features, int64_t n, int32_t od, const float* kernel_points, int32_t k,
                             float extent, int32_t modulated, float* deformed_kp, float* modulations, float* kp4, float* kp_rmax,
                             void* stream);
int ws_kpconv_deform_prepare_bwd(const float* d_kp4, const float* d_deformed_kp, const float* kp4, int64_t n, int32_t od, int32_t k,
                                 float extent, int32_t modulated, float* d_offset_features, void* stream);
int ws_kpconv_gather_fwd_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                             const void* x, int32_t ci, const float* kp4, int32_t k, float extent, const int32_t* order,
                             void* wf, float* min_d2, int32_t rows_bf16, int32_t rows_sorted, void* stream);
int ws_kpconv_gather_fwd_ex(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                            const void* x, int32_t ci, const float* kernel_points, int32_t k, const float* deformed_kp,
                            const float* modulations, float extent, int32_t influence, int32_t aggregation, const int32_t* order,
                            void* wf, float* min_d2, int32_t rows_bf16, int32_t rows_sorted, void* stream);
int ws_kpconv_gather_bwd_x_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                               const int32_t* t_offsets, const int32_t* t_pairs, const void* dwf, int32_t ci, const float* kp4,
                               int32_t k, float extent, const int32_t* order, void* dx, int32_t rows_bf16, void* stream);
int ws_kpconv_gather_bwd_x_grid_wide(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                     const uint64_t* key_last, float radius, const void* dwf, int32_t ci,
                                     const float* kernel_points, int32_t k, const float* kp4, const float* kp_rmax, float extent,
                                     const int32_t* order, const int64_t* rows, int32_t rows_h, void* dx, int32_t rows_bf16,
                                     void* stream);
int ws_kpconv_gather_bwd_geom_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                                  const void* x, int32_t ci, const void* dwf, const float* kp4, int32_t k, const float* d_min_d2,
                                  float extent, const int32_t* order, float* d_kp4, int32_t rows_bf16, int32_t rows_sorted,
                                  void* stream);
/* A whole forward KPConv layer in one launch, out [nq, co] = act(KPConv(x) + bias) with the contraction inside the gather
 * kernel (models/blocks.py:278-374 + the BatchNormBlock bias / LeakyReLU of :556-563); rigid, linear influence, sum, f32,
 * ci = co = 32 (else WS_ERR_UNSUPPORTED).  Forward only: nothing is kept for a backward pass (the weighted features
 * never reach memory) -- the testers' forward passes, utils/tester_PseudoLabel.py:164. */
int ws_kpconv_layer_fwd_fused(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                              const float* x, int32_t ci, const float* kernel_points, int32_t k, float extent,
                              const int32_t* order, const float* weights, int32_t co, const float* bias, int32_t act, float slope,
                              float* out, void* stream);
/* name of the forward gather kernel the library launches for a layer of ci channels (mode 0 rigid, 1 deformable through the
 * generic entries, 2 deformable fast path): for reports, no device work.  It assumes 16-byte aligned rows and a level of
 * 4096 queries or more (no narrowed channel blocks, no csplit items); ws_kpconv_gather_variant answers for any arguments */
int ws_kpconv_gather_fwd_variant(int32_t ci, int32_t mode, int32_t influence, int32_t aggregation, int32_t rows_bf16,
                                 int32_t rows_sorted, char* out, int32_t cap);
/* the launch a KPConv gather entry makes for these arguments (the launchers' own plan functions; pointers are only tested for
 * alignment, nothing is read or launched): "kernel<template arguments> grid=... [csplit=... | ilv=... | vec4=...]" into
 * out[cap], or the entry's own refusal.  op names the entry family (its _bf16 / _ex / _gated forms included, rows_bf16 = 1
 * for bf16 rows); rows_a, rows_b: its two feature-row operands (x and wf for the forward entries, dwf and dx for bwd_x*,
 * x and dwf for bwd_geom*).  deformed / modulated: deformed_kp / modulations given (WS_GATHER_BWD_X_GRID_WIDE: kp4 given);
 * rows_sorted as in the _ex / _def entries; ordered: a point order is passed.  The grid entries also follow
 * ws_kpconv_grid_sorted.  Arguments an entry does not take are ignored. */
enum {
    WS_GATHER_FWD = 0, WS_GATHER_BWD_X = 1, WS_GATHER_BWD_GEOM = 2, WS_GATHER_BWD_X_GRID = 3,
    WS_GATHER_FWD_DEF = 4, WS_GATHER_BWD_X_DEF = 5, WS_GATHER_BWD_X_GRID_WIDE = 6, WS_GATHER_BWD_GEOM_DEF = 7
};
int ws_kpconv_gather_variant(int32_t op, int64_t nq, int64_t ns, int32_t ci, const void* rows_a, const void* rows_b, int32_t deformed,
                             int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t rows_sorted,
                             int32_t ordered, char* out, int32_t cap);
/* Kernel sizes.  The gather entries are built for num_kernel_points k in {9, 13, 15}: 15 in every form; 9 and 13 with f32 rows
 * through the generic forms (MODE 0 rigid / linear / sum and MODE 1, deformable layers included).  bf16 rows, the deformable
 * fast path with packed kernel points (MODE 2: the _def entries, ws_kpconv_gather_bwd_x_grid_wide with kp4) and
 * ws_kpconv_layer_fwd_fused are 15 only; everything else is WS_ERR_UNSUPPORTED with the built sizes in the message.
 * ws_kpconv_supported_k: 1 where the entries run k with these rows in this mode (0, 1, 2 as above), else 0.
 * ws_kpconv_gather_variant_k: ws_kpconv_gather_variant (which answers for k = 15) for k kernel points; the text names the size
 * ("K=13" in the kernels that have a K argument, a leading "K=13, " in the matrix-core forward's list) unless it is 15. */
int ws_kpconv_supported_k(int32_t k, int32_t rows_bf16, int32_t mode);
int ws_kpconv_gather_variant_k(int32_t op, int64_t nq, int64_t ns, int32_t ci, const void* rows_a, const void* rows_b, int32_t deformed,
                               int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t rows_sorted,
                               int32_t ordered, int32_t k, char* out, int32_t cap);
/* the launches the dense products make for these arguments (the dispatchers' own plan functions; pointers are only tested
 * for alignment, nothing is read or launched): "kernel<template arguments> key=value ..." into out[cap].
 * ws_gemm_xb_variant: any ws_gemm_xb* entry (b_row_stride < 0 = row-major [K, N]; gate_y / mask NULL when absent);
 * ws_gemm_xty_variant: ws_gemm_xty (ldo = 0), the pitched dW (ldo >= n), ws_gemm_xty_bf16 (rows_bf16 = 1);
 * ws_act_bwd_colsum_variant: ws_act_bwd_colsum[_dropout]; the bf16 forms: ws_gemm_xbt_bf16, ws_act_bwd_colsum_bf16 */
int ws_gemm_xb_variant(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride, int64_t b_col_stride,
                       int32_t n, const float* bias, const float* residual, int64_t ldr, const float* gate_y, int64_t ldg,
                       const uint8_t* mask, int64_t ldm, const float* y, int64_t ldy, const void* scratch, int64_t scratch_bytes,
                       char* out, int32_t cap);
int ws_gemm_xty_variant(const void* x, int64_t m, int32_t k, int64_t ldx, const void* y, int32_t n, int64_t ldy, float* out_m,
                        int64_t ldo, void* scratch, int32_t rows_bf16, char* out, int32_t cap);
int ws_act_bwd_colsum_variant(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, const float* dz,
                              int64_t lddz, float* colsum, void* scratch, char* out, int32_t cap);
int ws_gemm_xbt_bf16_variant(int64_t m, int32_t k, int32_t n, const float* bias, const uint16_t* residual, int64_t ldr, const void* y,
                             int64_t ldy, int32_t out_f32, char* out, int32_t cap);
int ws_act_bwd_colsum_bf16_variant(int32_t dy_f32, int64_t m, int32_t n, float* colsum, void* scratch, char* out, int32_t cap);
int64_t ws_p2p_regularizer_scratch_bytes(int64_t n);
int ws_p2p_regularizer_fwd(const float* deformed_kp, const float* kp4, const float* min_d2, int64_t n, int32_t k, float extent,
                           float repulse_extent, float* out2, void* scratch, void* stream);
int ws_p2p_regularizer_bwd(const float* deformed_kp, const float* kp4, const float* min_d2, int64_t n, int32_t k, float extent,
                           float repulse_extent, const float* g2, float* d_min_d2, float* d_deformed_kp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-sphere dense attention of KPFCNN_mprm (models/blocks.py:758-1011), weasal_amd/csrc/attention.hip.
 * `lengths` is a HOST vector of `nspheres` sphere sizes (rows are stacked sphere after sphere); every entry validates on the
 * host before anything is queued: widths, lengths >= 0, sum(lengths) == n, NULL pointers.  The offsets travel in the kernel
 * arguments: more than WS_ATT_MAX_SPHERES spheres is WS_ERR_UNSUPPORTED.  Zero-length spheres are legal and write nothing.
 * No float atomics: every entry is run-to-run bit-identical.
 *
 * ws_sphere_attention_fwd (spatial_att, blocks.py:788-821: the loop over spheres with torch.matmul / nn.Softmax):
 *   att [n, dv] = softmax(Q_s K_s^T) V_s per sphere s (no 1/sqrt(d) scale), xn = att / n_s; q, k [n, dq], v [n, dv] contiguous.
 *   Streaming: no [n_s, n_s] tensor reaches memory.  lse: NULL, or [n] for the row log-sum-exp the backward entry needs;
 *   att does not depend on whether it is given.  dq % 8 == 0, dq <= 64, dv % 64 == 0, dv <= 512, else WS_ERR_UNSUPPORTED.
 * ws_sphere_attention_bwd: d_q, d_k [n, dq], d_v [n, dv] for the incoming d_att, d_xn [n, dv] (either may be NULL = zeros,
 *   not both); att, lse as the forward wrote them; scratch >= ws_sphere_attention_bwd_scratch_bytes(n, dv).
 *
 * ws_channel_attention_fwd (channel_att, blocks.py:853-882, max_minus = 1; ele_att, blocks.py:984-1011, max_minus = 0):
 *   per sphere E = X1_s^T X2_s [c, c], A_s = softmax_rows(max_minus ? rowmax(E) - E : E), out_s = Val_s A_s;
 *   x1, x2, value, out [n, c] contiguous; a [nspheres, c, c] receives the A_s (kept for the backward entry).
 *   c % 4 == 0, c <= 512, else WS_ERR_UNSUPPORTED.  scratch >= ws_channel_attention_scratch_bytes(lengths, nspheres, c, 0).
 * ws_channel_attention_bwd: d_x1, d_x2, d_value [n, c] for d_out [n, c]; scratch >= ..._scratch_bytes(lengths, nspheres, c, 1).
 *   In the max-minus form the gradient torch sends through the row maximum is sum_j dT_ij of a softmax backward, zero up
 *   to rounding: it is not replayed. */
#define WS_ATT_MAX_SPHERES 64
int ws_sphere_attention_fwd(const float* q, const float* k, const float* v, int64_t n, int32_t dq, int32_t dv, const int64_t* lengths,
                            int32_t nspheres, float* att, float* xn, float* lse, void* stream);
int64_t ws_sphere_attention_bwd_scratch_bytes(int64_t n, int32_t dv);
int ws_sphere_attention_bwd(const float* q, const float* k, const float* v, const float* att, const float* lse, const float* d_att,
                            const float* d_xn, int64_t n, int32_t dq, int32_t dv, const int64_t* lengths, int32_t nspheres,
                            float* d_q, float* d_k, float* d_v, void* scratch, int64_t scratch_bytes, void* stream);
int64_t ws_channel_attention_scratch_bytes(const int64_t* lengths, int32_t nspheres, int32_t c, int32_t backward);
int ws_channel_attention_fwd(const float* x1, const float* x2, const float* value, int64_t n, int32_t c, const int64_t* lengths,
                             int32_t nspheres, int32_t max_minus, float* a, float* out, void* scratch, int64_t scratch_bytes,
                             void* stream);
int ws_channel_attention_bwd(const float* x1, const float* x2, const float* value, const float* a, const float* d_out, int64_t n,
                             int32_t c, const int64_t* lengths, int32_t nspheres, int32_t max_minus, float* d_x1, float* d_x2,
                             float* d_value, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * What follows the attention blocks in the weak-label step of KPFCNN_mprm, weasal_amd/csrc/mprm_head.hip.  The four paths lie
 * side by side in one [rows, heads * c] tensor (row pitch ldx >= heads * c).  float32 throughout, no float atomics, every sum
 * in an order fixed by the shapes: run-to-run bit-identical.  Nothing is read back.
 *
 * ws_segment_mean_fwd (global_average, models/blocks.py:114-134: split / mean / stack): out [nspheres, w] = per sphere the sum
 *   of its rows of x [n, w] (row pitch ldx >= w: a column view works) in a fixed order, divided by the length; a sphere of
 *   length 0 gives nan as torch.mean does.  `lengths`: HOST vector as in the attention entries (offsets in the kernel
 *   arguments, more than WS_ATT_MAX_SPHERES spheres is WS_ERR_UNSUPPORTED); 1 <= w <= WS_SEGMENT_MAX_WIDTH.
 * ws_segment_mean_bwd: dx [n, w] contiguous, dx[row, :] = d_out[sphere(row), :] / length (d_out row pitch ldd).
 * ws_max_heads_fwd (models/architectures.py:700-702: torch.max(torch.max(torch.max(h0, h1), h2), h3)): out [n, c] contiguous =
 *   the maximum over the `heads` column blocks of x, nested from the left, nan propagating; heads <= WS_HEADS_MAX.
 * ws_max_heads_bwd: dx [n, heads * c] contiguous = the backward of that nested expression as autograd runs it: per
 *   maximum(a, b) both sides get (a == b ? g / 2 : g), a's zeroed where a < b and b's where a > b, outermost first.
 * ws_bce_heads_fwd (models/architectures.py:709-733 and :778-783: BCEWithLogitsLoss(weight = class_w) per path, summed):
 *   out[k] = mean over r rows and c columns of weight[col] * (max(x, 0) - x y + log1p(exp(-|x|))) for column block k of x
 *   against target [r, c] (contiguous), out[heads] = out[0] + out[1] + ... in that order; weight NULL = ones; r >= 1.
 * ws_bce_heads_bwd: dx [r, heads * c] contiguous = (g_heads[k] + g_sum[0]) * weight[col] * (sigmoid(x) - y) / (r c); g_heads
 *   [heads] and g_sum [1] are device floats (either may be NULL = zero, not both): nothing synchronises.
 * ------------------------------------------------------------------------------------------ */
#define WS_SEGMENT_MAX_WIDTH 1024
#define WS_HEADS_MAX 8
int ws_segment_mean_fwd(const float* x, int64_t n, int32_t w, int64_t ldx, const int64_t* lengths, int32_t nspheres, float* out,
                        void* stream);
int ws_segment_mean_bwd(const float* d_out, int64_t ldd, int64_t n, int32_t w, const int64_t* lengths, int32_t nspheres, float* dx,
                        void* stream);
int ws_max_heads_fwd(const float* x, int64_t n, int32_t c, int32_t heads, int64_t ldx, float* out, void* stream);
int ws_max_heads_bwd(const float* x, int64_t n, int32_t c, int32_t heads, int64_t ldx, const float* d_out, int64_t ldd, float* dx,
                     void* stream);
int ws_bce_heads_fwd(const float* x, int64_t r, int32_t c, int32_t heads, int64_t ldx, const float* target, const float* weight,
                     float* out, void* stream);
int ws_bce_heads_bwd(const float* x, int64_t r, int32_t c, int32_t heads, int64_t ldx, const float* target, const float* weight,
                     const float* g_heads, const float* g_sum, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batch normalisation over the point axis of the stacked batch, with the residual sum and the LeakyReLU that follow it in
 * the blocks: weasal_amd/csrc/batchnorm.hip.  Stands for the BatchNormBlock of models/blocks.py:430-470 run the way KPConv
 * applies nn.BatchNorm1d to [N, C] features (the reference constructs the module and returns 2-D inputs untouched; that
 * identity stays this project's default, these entries are what `batch_norm_mode = points` runs).
 * y, out, residual, dout, dy, dresidual: [n, c] float32 rows of unit column stride at the given pitch (>= c); gamma, beta,
 * running_mean, running_var, save_mean, save_rstd, dgamma, dbeta: [c] float32; num_batches_tracked: one int64 (NULL = none).
 * act: 0 none, 1 LeakyReLU(slope).  Any c >= 1 up to 2^20.  16-byte accesses when c % 4 == 0 and every pitch is a multiple
 * of 4 and every [n, c] pointer is 16-byte aligned; scalar accesses otherwise.  float32 arithmetic, centred variance
 * (two passes over registers, Chan's merge of (count, mean, M2) beyond), no float atomics, every merge in an order fixed by
 * the shapes: run-to-run bit-identical.  The plan depends on shapes, pitches and pointer alignment only.  Argument checks
 * need no device.  n == 0: WS_OK, no kernel, statistics untouched (ws_bn_bwd zeroes dgamma / dbeta).
 *
 * ws_bn_scratch_bytes: bytes of `scratch` for either entry at these sizes, whatever the alignment; -1 for bad sizes.
 * ws_bn_fwd (nn.BatchNorm1d.forward, then `+ residual`, then nn.LeakyReLU -- models/blocks.py:430-470, :497-506):
 *   training != 0: mean_c, biased var_c over the n rows; out = act((y - mean) * rstd * gamma + beta [+ residual]) with
 *     rstd = 1 / sqrt(var + eps); save_mean, save_rstd are written for ws_bn_bwd; on the device, nothing read back:
 *     running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with var n / (n - 1),
 *     *num_batches_tracked += 1.  n == 1 is WS_ERR_INVALID, as torch refuses it.  Three launches.
 *   training == 0: the same with mean = running_mean, var = running_var; nothing else is written (save_mean, save_rstd and
 *     scratch may be NULL).  One launch.
 * ws_bn_bwd: dz = dout * (out > 0 ? 1 : slope) -- the gate is taken from the OUTPUT -- or dout when act == 0 (out may then
 *   be NULL); dbeta = column sums of dz, dgamma = column sums of dz * xhat; dresidual = dz unless NULL;
 *   training != 0: dy = gamma rstd (dz - dbeta / n - xhat dgamma / n) with save_mean / save_rstd of the forward call;
 *   training == 0 (BN frozen, gradients wanted): dy = gamma rstd dz with running_mean / running_var and eps.
 *   One reduction pass for both column sums, a finish kernel, one apply pass.
 * ws_bn_variant: the branch a call takes, from the launchers' own plan function; nothing is read or launched.  backward
 *   == 0: ws_bn_fwd (dout, dy unused); != 0: ws_bn_bwd (residual / ldr stand for dresidual / lddr).  Pointers are tested
 *   for NULL and alignment only.  Text: "kernels<V=..> vector|scalar rows=<rows per chunk> chunks=.. depth=<merge levels>
 *   tile=<columns per workgroup> lanes=<row lanes> ctiles=.. mode=training|evaluation residual=0|1 act=0|1".
 * ------------------------------------------------------------------------------------------ */
int64_t ws_bn_scratch_bytes(int64_t n, int32_t c);
int ws_bn_fwd(const float* y, int64_t n, int32_t c, int64_t ldy, const float* gamma, const float* beta, float eps, int32_t training,
              float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* residual,
              int64_t ldr, int32_t act, float slope, float* out, int64_t ldo, float* save_mean, float* save_rstd, void* scratch,
              void* stream);
int ws_bn_bwd(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
              const float* gamma, const float* save_mean, const float* save_rstd, const float* running_mean,
              const float* running_var, float eps, int32_t training, int32_t act, float slope, float* dy, int64_t lddy,
              float* dresidual, int64_t lddr, float* dgamma, float* dbeta, void* scratch, void* stream);
int ws_bn_variant(int32_t backward, int64_t n, int32_t c, const void* y, int64_t ldy, const void* out, int64_t ldo,
                  const void* residual, int64_t ldr, const void* dout, int64_t lddo, const void* dy, int64_t lddy, int32_t training,
                  int32_t act, char* text, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * The same normalisation with batch statistics over the rows of SEVERAL ranks (data parallelism; what torch users know as
 * SyncBatchNorm): the training launch sequence of ws_bn_fwd / ws_bn_bwd cut at the two points where a collective goes.
 * The library moves nothing between ranks: the caller gathers the records (ops.batch_norm_act(group=...): one
 * all_gather_into_tensor per direction).  Every rank runs the two finishing entries on the same gathered bytes, merging
 * in rank order, so every rank gets the same bits in save_mean, save_rstd, the running statistics and num_batches_tracked.
 * A rank may hold no row (n == 0).  Conventions, pitches, alignment rule and plan as above.
 *
 * ws_bn_moments: this rank's record [5, c] float32 = n, sum, hi, lo, M2 per column (mean = hi + lo for merging, the
 *   centred M2; see batchnorm.hip), the chunks merged in the order ws_bn_fwd merges them.  n == 0: the record is zeroed, no
 *   kernel.  The count is a float: n up to 2^24 per rank (WS_ERR_UNSUPPORTED beyond).  scratch: ws_bn_scratch_bytes(n, c).
 *   Two launches.
 * ws_bn_moments_finish: records [world, 5, c] (rank order) -> N = the integer sum of the counts, written to *n_global (one
 *   int64 on the device, read by ws_bn_bwd_apply); the ranks merged with Chan's formula in rank order; save_mean = sum / N,
 *   save_rstd = 1 / sqrt(M2 / N + eps); running_mean / running_var as ws_bn_fwd with the factor N / (N - 1);
 *   *num_batches_tracked += 1.  The count lives on the device, so the refusal of a single row cannot be a status: with
 *   N < 2 ONLY *n_global is written, and a caller that cannot rule N == 1 out by its own n >= 2 reads it and refuses
 *   (ops does, on every rank, after the gather).  One launch.
 * ws_bn_apply: out = act((y - mean) * rstd * gamma + beta [+ residual]) with the given mean and rstd: the kernel ws_bn_fwd
 *   launches last in training.  n == 0: nothing.  One launch.
 * ws_bn_bwd_sums: this rank's record [2, c] = column sums of dz, of dz * xhat (dz as in ws_bn_bwd, xhat from save_mean /
 *   save_rstd): the LOCAL dbeta and dgamma, which are what autograd gets (gradient averaging then treats them like every
 *   other gradient).  n == 0: zeroed, no kernel.  Two launches.
 * ws_bn_bwd_apply: records [world, 2, c] added in rank order -> S1, S2; dy = gamma rstd (dz - S1 / N - xhat S2 / N) with N
 *   read from *n_global; dresidual = dz unless NULL.  n == 0: nothing.  scratch: ws_bn_scratch_bytes(n, c).  Two launches.
 * With world == 1 the sequence gives the bits of ws_bn_fwd / ws_bn_bwd.
 * ws_bn_sync_variant: the branch of one of them, from the same plan function; nothing is read or launched.  stage: 0
 *   moments, 1 moments_finish, 2 apply, 3 bwd_sums, 4 bwd_apply (residual / ldr stand for dresidual / lddr).  Text:
 *   "kernels<V=..> vector|scalar rows=.. chunks=.. depth=.. tile=.. lanes=.. ctiles=.. world=.. residual=0|1 act=0|1";
 *   stage 1: "bn_sync_finish_kernel world=.. blocks=..".
 * ------------------------------------------------------------------------------------------ */
int ws_bn_moments(const float* y, int64_t n, int32_t c, int64_t ldy, float* record, void* scratch, void* stream);
int ws_bn_moments_finish(const float* records, int32_t world, int32_t c, float eps, float momentum, float* running_mean,
                         float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_rstd, int64_t* n_global,
                         void* stream);
int ws_bn_apply(const float* y, int64_t n, int32_t c, int64_t ldy, const float* mean, const float* rstd, const float* gamma,
                const float* beta, const float* residual, int64_t ldr, int32_t act, float slope, float* out, int64_t ldo, void* stream);
int ws_bn_bwd_sums(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
                   const float* save_mean, const float* save_rstd, int32_t act, float slope, float* record, void* scratch, void* stream);
int ws_bn_bwd_apply(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
                    const float* gamma, const float* save_mean, const float* save_rstd, const float* records, int32_t world,
                    const int64_t* n_global, int32_t act, float slope, float* dy, int64_t lddy, float* dresidual, int64_t lddr,
                    void* scratch, void* stream);
int ws_bn_sync_variant(int32_t stage, int64_t n, int32_t c, int32_t world, const void* y, int64_t ldy, const void* out, int64_t ldo,
                       const void* residual, int64_t ldr, const void* dout, int64_t lddo, const void* dy, int64_t lddy, int32_t act,
                       char* text, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * Evaluation-mode batch normalisation folded into the product in front of it: weasal_amd/csrc/bn_fold.hip.  With running
 * statistics BN is an affine map per output channel, rstd = 1 / sqrt(running_var + eps), a = gamma rstd,
 * t = beta - running_mean a, and act(BN(x W^T) + residual) = act(x (a (.)rows W)^T + t + residual): the bias / residual /
 * LeakyReLU epilogue every product and block call above already takes.
 * A SITE is a weight seen as [outer, c, inner] float32, contiguous, the BN channel on the middle axis (nn.Linear.weight
 * [c, k]: outer 1, inner k; KPConv weights [K, Ci, Co]: outer K Ci, inner 1) with gamma, beta, running_mean, running_var [c]
 * and eps.  Both entries take a TABLE of `count` sites as HOST arrays (h_*) of device pointers, sizes and eps values, the
 * idiom of ws_sgd_step; the table travels in the kernel arguments, WS_BN_FOLD_MAX sites per launch, and workgroups are dealt
 * to the sites by a prefix over their element counts (4096 per workgroup).  A site with c == 0 is passed over; count == 0 or
 * nothing but such sites: WS_OK, no launch.  outer c inner < 2^31 - 4096.  float32 arithmetic, every operation rounded on
 * its own (the unit is compiled with -ffp-contract=off): rstd = 1 / sqrtf(var + eps), a = gamma * rstd.  16-byte accesses
 * to the [outer, c, inner] tensors when they are 16-byte aligned and inner % 4 == 0 or (inner == 1 and c % 4 == 0); scalar
 * accesses otherwise; [c] vectors may have any alignment.  Argument checks need no device.
 *
 * ws_bn_fold_fwd: w_out = a * w (a buffer of its own, the shape of w), t_out = beta - mean * a.  One launch per
 *   WS_BN_FOLD_MAX sites.
 * ws_bn_fold_bwd: dw = a * dw_out, dbeta = dt_out, dgamma_c = rstd_c * (sum over outer, inner of dw_out * w - mean_c *
 *   dt_out_c); the running buffers get no gradient.  h_dw_out[t] / h_dt_out[t] NULL: zeros (a folded weight used without its
 *   bias, a site whose output nobody differentiated).  h_dw[t] / h_dgamma[t] / h_dbeta[t] NULL: that output is not written
 *   (all three NULL: the site is passed over).  The per-channel sum runs in an order fixed by the shapes -- inner > 1: a
 *   wave per channel, lane l adds elements l, l + 64, ... of every outer slice in index order, lanes folded by xor-shuffles
 *   (row sums); inner == 1: a workgroup per 64 columns (16 from 1024 rows on), row lane r adds rows r, r + lanes, ..., the
 *   lanes of a column added in lane order (column sums) -- no float atomics, run-to-run bit-identical.  One launch per
 *   WS_BN_FOLD_MAX sites holds the element-wise part and the sums.
 * ws_bn_fold_variant: the branch ONE site takes and the launches of a table of `count` sites, from the launchers' own plan
 *   function; nothing is read or launched.  src / dst: the pointers of the element-wise part (forward w, w_out; backward
 *   dw_out, dw), tested for alignment only (NULL passes).  Text, forward: "bn_fold_fwd_kernel vector|scalar blocks=..
 *   launches=.."; backward: "bn_fold_bwd_kernel vector|scalar row-sum|column-sum tile=<channels per workgroup>
 *   ew_blocks=.. sum_blocks=.. launches=.."; c == 0 or count == 0: "none (..) launches=..".
 * ------------------------------------------------------------------------------------------ */
#define WS_BN_FOLD_MAX 32
int ws_bn_fold_fwd(const float* const* h_w, const int64_t* h_outer, const int32_t* h_c, const int64_t* h_inner,
                   const float* const* h_gamma, const float* const* h_beta, const float* const* h_mean, const float* const* h_var,
                   const float* h_eps, float* const* h_w_out, float* const* h_t_out, int32_t count, void* stream);
int ws_bn_fold_bwd(const float* const* h_w, const int64_t* h_outer, const int32_t* h_c, const int64_t* h_inner,
                   const float* const* h_gamma, const float* const* h_mean, const float* const* h_var, const float* h_eps,
                   const float* const* h_dw_out, const float* const* h_dt_out, float* const* h_dw, float* const* h_dgamma,
                   float* const* h_dbeta, int32_t count, void* stream);
int ws_bn_fold_variant(int32_t backward, int64_t outer, int32_t c, int64_t inner, const void* src, const void* dst, int32_t count,
                       char* text, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* WEASAL_HIP_H */
