/* sfmx.h — C ABI of the MI355X-native SfM hot path (libsfmx.so, gfx950).
 *
 * The reference (RoozbehSanaei/Structure-from-Motion-3D-Reconstruction, cpp/) has no plugin / FFI
 * layer: its hot functions are file-static in cpp/src/templering_sfm.cpp ("T:" below).  Each entry
 * point here replaces one of those function seams and is what a maintainer would
 * bind from the reference's own code (see INTEGRATION.md for the call-site patch).
 *
 * Conventions
 *  - plain C, no exceptions across the boundary; every call returns an sfmx_status (0 = ok).
 *  - caller owns host buffers; the library owns device memory inside the context.
 *  - one HIP stream per context; a context is thread-compatible, not thread-safe (one per thread).
 *  - all floating point is IEEE binary64, evaluated WITHOUT fused multiply-add in the reference's
 *    operation order, so results are bit-identical to the x86-64 reference build.
 *  - arrays of 2-D points are [n][2] doubles (x,y), row-major 3x3 matrices are 9 doubles.
 */
#ifndef SFMX_H
#define SFMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sfmx_status {
  SFMX_OK = 0,
  SFMX_ERR_INVALID = 1,   /* bad argument (null pointer, size <= 0, level out of range, ...)      */
  SFMX_ERR_HIP = 2,       /* a HIP runtime call failed; see sfmx_last_error()                      */
  SFMX_ERR_NO_DEVICE = 3, /* no gfx950 device / extension unusable: callers must fail, not fall back */
  SFMX_ERR_SINGULAR = 4,  /* sfmx_solve_dense: pivot < 1e-15 — where dense.hpp:67 throws           */
  SFMX_ERR_UNSUPPORTED = 5
} sfmx_status;

typedef struct sfmx_ctx sfmx_ctx;
typedef struct sfmx_pyramid sfmx_pyramid;

/* ---- context ------------------------------------------------------------------------------ */
int sfmx_ctx_create(int device_id, sfmx_ctx** out);
/* same, with a stream priority hint: <0 high (short latency-critical launches), 0 normal, >0 low (background) */
int sfmx_ctx_create_prio(int device_id, int priority, sfmx_ctx** out);
/* (include/sfmx_ctx_split.h: the same in steps -- a context without streams, then each stream -- for the host pipeline, which
 * interleaves the stream creations of its helper contexts to place them on the hardware queues) */
void sfmx_ctx_destroy(sfmx_ctx* ctx);
const char* sfmx_last_error(const sfmx_ctx* ctx);
int sfmx_sync(sfmx_ctx* ctx);
int sfmx_ctx_device(const sfmx_ctx* ctx);  /* device index the context was created on */
/* HIP's current device is per host thread: a thread that did not create the context calls this once before
 * using it (one context per thread; contexts of several threads may share a device). */
int sfmx_ctx_make_current(sfmx_ctx* ctx);
/* raw hipStream_t of the context (for event timing by the caller) */
void* sfmx_stream(sfmx_ctx* ctx);
/* microseconds of GPU time of the most recent hot kernel launched by the last API call, measured
 * with HIP events on the context stream (0 when timing is disabled, see sfmx_set_timing). */
int sfmx_set_timing(sfmx_ctx* ctx, int enabled);
int sfmx_get_timing(const sfmx_ctx* ctx); /* 1 if enabled (so that helper contexts can inherit the setting) */
double sfmx_last_kernel_us(const sfmx_ctx* ctx);
/* Per-kernel profile of this context while timing is enabled: accumulated GPU microseconds and launch counts of each
 * hot kernel (HIP events recorded on the context's stream around every launch).  Enabling timing starts a fresh
 * profile.  Returns the number of kernel ids; at most cap entries are written; reset != 0 clears after reading. */
int sfmx_kernel_profile(sfmx_ctx* ctx, int reset, int cap, double* us_out, uint64_t* calls_out);
const char* sfmx_kernel_profile_name(int id);

/* ---- image pyramid: replaces sfm::GrayImage + build_pyr/downsample2 (T:200-232) ------------ */
/* level 0 is the image itself; level l is (w>>l) x (h>>l), 2x2 box with integer /4 truncation and
 * +1 neighbours clamped to the edge.  All levels live in one HBM allocation. */
int sfmx_pyramid_create(sfmx_ctx* ctx, int w, int h, int levels, sfmx_pyramid** out);
void sfmx_pyramid_destroy(sfmx_ctx* ctx, sfmx_pyramid* pyr);
/* host pixels -> HBM, then build levels 1.. on the device */
int sfmx_pyramid_upload(sfmx_ctx* ctx, sfmx_pyramid* pyr, const uint8_t* host_pixels);
/* pixels already resident in HBM (device pointer): device copy + build */
int sfmx_pyramid_set_device(sfmx_ctx* ctx, sfmx_pyramid* pyr, const void* device_pixels);
/* The same build on the context's SECOND stream (it overlaps with kernels already queued on the first, e.g. the KLT launch of
 * the previous frame); fetch_level >= 0 also copies that level's pixels to pinned host memory.  Nothing that still reads the
 * pyramid may be in flight.  sfmx_pyramid_wait orders the context's main stream behind the build (no host wait; calls of THIS
 * context that take the pyramid do it themselves, another context that reads it must be started after a host-side wait such as
 * sfmx_pyramid_fetched_level or sfmx_sync); sfmx_pyramid_fetched_level waits for the copy and returns the pixels (*out == NULL
 * if that level was not fetched). */
int sfmx_pyramid_set_device_async(sfmx_ctx* ctx, sfmx_pyramid* pyr, const void* device_pixels, int fetch_level);
int sfmx_pyramid_wait(sfmx_ctx* ctx, sfmx_pyramid* pyr);
int sfmx_pyramid_fetched_level(sfmx_ctx* ctx, sfmx_pyramid* pyr, int level, const uint8_t** out);
int sfmx_pyramid_download_level(sfmx_ctx* ctx, const sfmx_pyramid* pyr, int level, uint8_t* host_out);
int sfmx_pyramid_level_size(const sfmx_pyramid* pyr, int level, int* w, int* h);

/* ---- Shi-Tomasi score map: replaces the per-pixel loop of shi_tomasi (T:242-272) ----------- */
/* score_out [h][w] doubles (0 outside the r=2 interior band); max_out = max over the map (T:274).
 * Thresholding, std::sort and the greedy min-distance pick (T:275-301) stay on the host because
 * their result depends on libstdc++'s sort permutation. */
int sfmx_shi_tomasi_score(sfmx_ctx* ctx, const sfmx_pyramid* pyr, double* score_out, double* max_out);
/* candidates only: pixels with score >= max*quality in row-major order (T:280-285), as
 * (x | y<<16) in cand_xy and the score in cand_score.  *n_out is the total number of candidates;
 * at most cap are written. */
int sfmx_shi_tomasi_candidates(sfmx_ctx* ctx, const sfmx_pyramid* pyr, double quality, int cap,
                               uint32_t* cand_xy, double* cand_score, int* n_out, double* max_out);

/* Same, after resolving on the device every candidate whose fate under the greedy min-distance pick
 * (T:288-300) is certain whatever the sort's tie order (parallel fixpoint: "accepted" once every pixel
 * within min_dist with score >= its own is rejected; "rejected" once an accepted pixel of strictly
 * greater score lies within min_dist).  Rejected candidates are dropped; bit 31 of cand_xy marks the
 * certainly accepted ones, the rest are still undecided; x = bits 0..14, y = bits 16..30.
 * *n_out = survivors (row-major order), *n_total_out = all candidates before resolution. */
int sfmx_shi_tomasi_candidates_pruned(sfmx_ctx* ctx, const sfmx_pyramid* pyr, double quality, int min_dist,
                                      int cap, uint32_t* cand_xy, double* cand_score, int32_t* cand_full_index,
                                      int* n_out, int* n_total_out, double* max_out);
/* cand_full_index[k] (optional) = position of survivor k in the row-major list of ALL candidates.  That list
 * is kept as 16-byte records {double score; uint32 id (= position); uint32 mark (= 0)} and is downloaded
 * speculatively into pinned host memory owned by the context; *keys_out stays valid (and may be modified
 * in place) until the next Shi-Tomasi call on this context. */
int sfmx_shi_tomasi_fetch_all_keys(sfmx_ctx* ctx, int n_total, void** keys_out);

/* ---- KLT: replaces KLTTracker::track_one fwd+bwd and the FB test (T:356-362, 402-460) ------- */
typedef struct sfmx_klt_cfg {
  int levels;       /* LKConfig::pyr_levels (T:312) */
  int win_radius;   /* LKConfig::win_radius (T:313); supported 1..7 */
  int iters;        /* LKConfig::iters (T:314) */
  double fb_thresh; /* LKConfig::fb_thresh (T:315) */
} sfmx_klt_cfg;
/* For every point: fwd = track_one(A,B,p), back = track_one(B,A,fwd), keep = !(hypot(back-p) >= fb).
 * xy_back may be NULL.  n_steps_out (optional) receives the number of lk_step evaluations executed. */
int sfmx_klt_track(sfmx_ctx* ctx, const sfmx_pyramid* pyr_a, const sfmx_pyramid* pyr_b,
                   const double* xy_in, int n, const sfmx_klt_cfg* cfg, double* xy_fwd,
                   double* xy_back, uint8_t* keep, uint64_t* n_steps_out);

/* ---- RANSAC scoring: replaces the hypothesis loop of find_E_ransac (T:664-677) --------------- */
/* xi,xj: K^-1-normalised correspondences [n][2]; idx8: pre-drawn sample octets [H][8] (the
 * caller draws them with the libstdc++-compatible generator so the stream matches T:657-665).
 * Every 8-point hypothesis (T:609-627) is built and all n points are scored against it with the
 * Sampson error (T:629-638, bit-exact arithmetic for a given E), counting err < thr.
 *
 * Which E a hypothesis is scored with.  The reference's eight_point_E calls the platform libm
 * (atan2/cos/sin, linalg.hpp:156-157); the device runs the same Jacobi with algebraic rotations and
 * reports a conditioning estimate cond per hypothesis (relative gap of the two smallest
 * eigenvalues, relative singular-value gap of the rank-2 projection; 0 if a Jacobi pivot was
 * nearly tied with another entry).  Its E differs from the reference's by at most 1e-16 / cond per
 * entry (measured <= 3e-18 / cond).  Octets with a repeated sample index (sampling is with
 * replacement, T:665: null space of dimension >= 2, cond ~ 0) and hypotheses with cond < 1e-13
 * are derived on the host with libm instead (the reference's E bit for bit, flags bit 0) and
 * scored with that.
 *
 * counts_out [H]: #{err < thr}.  lo_out/hi_out [H] (optional): bounds of the REFERENCE's count of
 * that iteration under the EMPIRICAL contract above (|E_dev - E_ref| <= 1e-16 / cond: measured, not
 * derived; a caller that needs the reference's winner verifies candidates exactly, as
 * ransac_local in csrc/host/pipeline.cpp does, and falls back to exact counts if a bound fails): a point counts for lo only if it stays an inlier, for hi
 * if it can become one, when every entry of E moves by 1e-16 / cond (per-point bound, see
 * k_score); lo == hi == count for the exact hypotheses.  flags_out [H] (optional): bit 0 = exact
 * host hypothesis.  cond_out [H] (optional): the conditioning estimate (+inf for exact ones).
 * best_iter/best_count = argmax of counts with the LOWEST iteration on ties (the reference's
 * strict '>').  E_out [H][9] (optional): the hypotheses that were scored. */
int sfmx_ransac_score_ex(sfmx_ctx* ctx, const double* xi, const double* xj, int n, const int32_t* idx8,
                         int H, double thr, int32_t* counts_out, int32_t* lo_out, int32_t* hi_out,
                         uint8_t* flags_out, double* cond_out, int32_t* best_iter,
                         int32_t* best_count, double* E_out);
/* same without the certification outputs */
int sfmx_ransac_score(sfmx_ctx* ctx, const double* xi, const double* xj, int n, const int32_t* idx8,
                      int H, double thr, int32_t* counts_out, int32_t* best_iter, int32_t* best_count,
                      double* E_out);
/* inlier mask of ONE essential matrix (used for the winner after the host has re-derived its E
 * with the platform libm, so the mask and E are bit-identical to the reference's).  Passing
 * xi == xj == NULL reuses the n correspondences left in HBM by the preceding sfmx_ransac_score. */
int sfmx_sampson_mask(sfmx_ctx* ctx, const double* xi, const double* xj, int n, const double* E9,
                      double thr, uint8_t* mask_out, int32_t* count_out);

/* ---- local BA: replaces the S,b build of bundle_adjust_window (T:893-1071) ------------------ */
/* poses_wc [W][12] = world->camera (R row-major, t); X [P][3]; CSR observations: obs_ptr [P+1],
 * obs_li [R] window-local pose index, obs_uv [R][2] pixels.  Points are consumed in array order
 * (the caller passes them in the reference's unordered_map iteration order).
 * Output: S [6W][6W] row-major and b [6W] AFTER damping (+lambda on the diagonal) and gauge
 * (+1e9 on DoF 0..5, b[0..5] = 0) when damp != 0.  Accumulation order is the reference's, so S,b
 * are bit-identical on one GPU. */
typedef struct sfmx_ba_problem sfmx_ba_problem;
int sfmx_ba_create(sfmx_ctx* ctx, int W, int P, const double* X, const int32_t* obs_ptr,
                   const int32_t* obs_li, const double* obs_uv, sfmx_ba_problem** out);
/* re-target an existing problem object at new data (device buffers are kept and only grow) */
int sfmx_ba_reset(sfmx_ctx* ctx, sfmx_ba_problem* prob, int W, int P, const double* X, const int32_t* obs_ptr,
                  const int32_t* obs_li, const double* obs_uv);
void sfmx_ba_destroy(sfmx_ctx* ctx, sfmx_ba_problem* prob);
int sfmx_ba_build(sfmx_ctx* ctx, sfmx_ba_problem* prob, const double* poses_wc, double fx, double fy,
                  double cx, double cy, double huber, double lambda, int damp, double* S_out,
                  double* b_out);
/* build + solve on the device in one submission: dx [6W]; returns SFMX_ERR_SINGULAR where the
 * reference's solve_gauss would throw (the caller then skips BA as T:1076-1078 does). */
int sfmx_ba_step(sfmx_ctx* ctx, sfmx_ba_problem* prob, const double* poses_wc, double fx, double fy,
                 double cx, double cy, double huber, double lambda, double* dx_out);
/* Optional bracket around the sfmx_ba_step calls of ONE bundle_adjust_window call (T:893-1096: `iters` iterations on the same
 * window and intrinsics).  For window-sized problems sfmx_ba_begin launches a kernel that stays resident for the whole job, so
 * that an iteration is a hand-over of poses and a poll for S | b instead of two launches that queue behind the kernels of other
 * contexts; sfmx_ba_end releases it when the job stops early (SFMX_ERR_SINGULAR).  Results are identical with and without. */
int sfmx_ba_begin(sfmx_ctx* ctx, sfmx_ba_problem* prob, int iters, double fx, double fy, double cx, double cy, double huber,
                  double lambda);
int sfmx_ba_end(sfmx_ctx* ctx, sfmx_ba_problem* prob);
/* partial sums for point-sharded multi-GPU BA: raw S,b of this problem's points only (no damping);
 * device pointers (valid until the next call on prob) so the caller can all-reduce them in HBM. */
int sfmx_ba_build_partial(sfmx_ctx* ctx, sfmx_ba_problem* prob, const double* poses_wc, double fx,
                          double fy, double cx, double cy, double huber, void** S_dev, void** b_dev);

/* ---- multi-GPU exchange steps (one process per GPU, RCCL over xGMI) ---------------------------- */
/* The reference is single-process; these are the collectives the sharded modes of this library add.
 * A communicator belongs to ONE host thread / context at a time (a pipeline uses one per lane).  world == 1 (or a NULL
 * communicator) makes every call below a local no-op, so the sharded entry points can be used unconditionally. */
typedef struct sfmx_comm sfmx_comm;
#define SFMX_COMM_ID_BYTES 128
int sfmx_comm_get_unique_id(void* id_out);  /* rank 0; the application carries the 128 bytes to the other ranks */
int sfmx_comm_create(int device_id, const void* id_bytes, int rank, int world, sfmx_comm** out);
void sfmx_comm_destroy(sfmx_comm* comm);
int sfmx_comm_rank(const sfmx_comm* comm);
int sfmx_comm_world(const sfmx_comm* comm);
/* contiguous, order-preserving split of range(n): the first n % world ranks get one item more */
void sfmx_shard_range(int n, int rank, int world, int* lo, int* hi);
/* all-reduce of a small host array through the context's stream; op 0 = sum, 1 = max */
int sfmx_comm_allreduce_f64(sfmx_ctx* ctx, sfmx_comm* comm, double* host_inout, int n, int op);
int sfmx_comm_allreduce_u64_max(sfmx_ctx* ctx, sfmx_comm* comm, uint64_t* host_inout, int n);
/* Point-sharded BA iteration (T:893-1095): prob holds THIS rank's contiguous range of the window's points (reference
 * order); raw S | b of the shard -> one all-reduce(sum) of D*D + D doubles in HBM -> damping + gauge (T:1064-1071) ->
 * solve on the device -> dx (identical on every rank).  TOLERANCE mode: the rank-ordered sum rounds differently from the
 * sequential reference (1e-9 relative per step; with world == 1 it equals sfmx_ba_step bit for bit), and whole runs of the
 * reference's BA do NOT stay within the task's 1e-6 of the one-GPU run (tools/virtual_world_probe.py).  The pipeline uses
 * sfmx_ba_step_sharded_elements below; this entry remains for callers that accept the tolerance (SFMX_BA_SHARD=points). */
int sfmx_ba_step_sharded(sfmx_ctx* ctx, sfmx_comm* comm, sfmx_ba_problem* prob, const double* poses_wc, double fx,
                         double fy, double cx, double cy, double huber, double lambda, double* dx_out);

/* Element-sharded BA iteration (T:893-1095) -- the sharded mode that keeps the reference's arithmetic.  prob holds the WHOLE
 * window on every rank.  The per-point records are computed by every rank (replicated); rank r forms and reduces only its
 * contiguous slice of the elements of S | b (every element's sum runs over all points in the reference's order) and contributes
 * +0.0 elsewhere, so the all-reduce(sum) of D*D + D doubles only ever adds zeros: S, b and dx are bit-identical to sfmx_ba_step
 * at any world size.  (sfmx_ba_step_sharded regroups the addends instead; the reference's BA amplifies that rounding
 * difference -- it ADDS the Schur term, T:1055 -- to a different trajectory within tens of keyframes) */
int sfmx_ba_step_sharded_elements(sfmx_ctx* ctx, sfmx_comm* comm, sfmx_ba_problem* prob, const double* poses_wc, double fx,
                                  double fy, double cx, double cy, double huber, double lambda, double* dx_out);

/* ---- dense solve: replaces sfm::solve_gauss (cpp/include/dense.hpp:54-93) -------------------- */
/* Gaussian elimination with partial pivoting in the reference's operation order; A [n][n]
 * row-major and b [n] are not modified; x [n].  SFMX_ERR_SINGULAR when a pivot is < 1e-15. */
int sfmx_solve_dense(sfmx_ctx* ctx, const double* A, const double* b, int n, double* x);

/* lk_step evaluations of the last sfmx_klt_track call that could not use the shared sample grid (more distinct
 * sample coordinates than its descriptor table holds) and took the per-pixel path: a performance counter, the
 * results are identical either way. */
uint64_t sfmx_debug_klt_slow_steps(const sfmx_ctx* ctx);

/* ---- pose-graph normal equations, structured (TOLERANCE mode): replaces the dense 3N x 3N solve of
 * posegraph_optimize_centers (T:1131-1197 -> dense.hpp:54-93) for large keyframe counts ------------ */
/* The system is H = L (x) I_3 with L the N x N weighted graph Laplacian plus the gauge term, so the three coordinates
 * are solved together on L: blocked Cholesky with the trailing update on the FP64 matrix cores
 * (v_mfma_f64_16x16x4_f64), then blocked triangular solves.  entry_ij [m][2] / entry_v [m]: the distinct entries of
 * the LOWER triangle of L (row >= column), already summed; g3, x3 [n][3].  A different factorisation than the
 * reference's elimination: agrees with solve_gauss on the dense system to ~1e-12 relative (tests: 1e-9), not bit for
 * bit.  SFMX_ERR_SINGULAR where a pivot is not > 1e-15: that catches exact singularity (a zero row, a component without
 * node 0 whose entries are all small integers), a matrix that is not positive definite and non-finite entries.  It does
 * NOT decide connectivity: the last pivot of a cut-off component that holds loop edges is zero only up to rounding and
 * lands either side of the threshold, so the caller checks on the graph that every node reaches node 0 before it calls
 * (posegraph_optimize_centers does).  NaN in g3 alone is not an error: it fills its column of x3. */
int sfmx_posegraph_solve(sfmx_ctx* ctx, int n, const int32_t* entry_ij, const double* entry_v, int m,
                         const double* g3, double* x3);

/* ---- keyframe-pair stereo: rectification + census SGM (not in the reference's C++) ------------------------ */
/* Every stage is integer arithmetic or IEEE double with a fixed expression order, so the disparity map is bit-identical to
 * the NumPy restatement in tests/stereo_ref.py.  Stages: bilinear remap through H (rectified pixel -> source pixel), census
 * transform, Hamming cost, 4-path SGM (left->right, right->left, top->bottom, bottom->top) summed into S (u16), winner with
 * uniqueness test, integer sub-pixel refinement, left-right check, speckle filter (4-connected components). */
typedef struct sfmx_stereo sfmx_stereo;  /* device buffers for one (w, h, params) */
typedef struct sfmx_stereo_params {
  int num_disparities; /* D: multiple of 16, 16..256 */
  int census;          /* census window side: 3, 5 or 7 */
  int p1, p2;          /* SGM penalties, 0 < p1 < p2 <= 2048 (defaults 8, 96) */
  int uniqueness;      /* percent, 0..100 (default 10; 0 = off) */
  int lr_max_diff;     /* left-right check in whole pixels (default 1; < 0 = off) */
  int speckle_window;  /* components with fewer pixels become invalid (default 100; 0 = off) */
  int speckle_range;   /* max disparity step inside a component, whole pixels (default 2) */
} sfmx_stereo_params;
void sfmx_stereo_default_params(sfmx_stereo_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_stereo_check_params(int w, int h, const sfmx_stereo_params* p);
int sfmx_stereo_create(sfmx_ctx* ctx, int w, int h, const sfmx_stereo_params* p, sfmx_stereo** out);
void sfmx_stereo_destroy(sfmx_ctx* ctx, sfmx_stereo* st);
/* img_l / img_r: u8 [h][w], host pointers or (on_device = 1) device pointers.
 * H_l, H_r: row-major 3x3 maps from a rectified pixel to a source pixel.
 * disp16_out: int16 [h][w] on the host, disparity x 16 in the left rectified view, -16 = invalid.
 * rect_out (optional): u8 [2][h][w] rectified images.  sum_out (optional): u16 [h][w][D] aggregated cost S. */
int sfmx_stereo_disparity(sfmx_ctx* ctx, sfmx_stereo* st, const uint8_t* img_l, const uint8_t* img_r, int on_device,
                          const double* H_l, const double* H_r, int16_t* disp16_out, uint8_t* rect_out, uint16_t* sum_out);
/* the rectification alone: both rectified images are left on the device inside st (for the _add_stereo_view entries that take
 * the left rectified image); the disparity map inside st no longer belongs to these images, and until the next
 * sfmx_stereo_disparity every entry that takes st's map (sfmx_fusion / _shade / _consist _add_stereo_view, sfmx_align_stereo_view)
 * returns SFMX_ERR_INVALID */
int sfmx_stereo_rectify(sfmx_ctx* ctx, sfmx_stereo* st, const uint8_t* img_l, const uint8_t* img_r, int on_device, const double* H_l,
                        const double* H_r);
/* device time (us) of the kernels of the last sfmx_stereo_disparity call when timing is on (sfmx_set_timing), else 0 */
double sfmx_stereo_last_us(const sfmx_stereo* st);

/* ---- multi-pair depth fusion: TSDF volume + marching tetrahedra ------------------------------------------ */
/* Integration is IEEE double in one fixed expression order per view and grid point, views in the order they were added, so
 * sum / count do not depend on how the views are batched into launches; extraction is integer scans plus one fixed double
 * expression per vertex.  Both are bit-identical to the NumPy restatement in tests/fusion_ref.py.
 * Grid point (i, j, k) sits at origin + (i, j, k) * voxel; arrays are [nz][ny][nx] (i fastest). */
typedef struct sfmx_fusion sfmx_fusion;  /* device volume + pending views */
typedef struct sfmx_fusion_params {
  double origin[3];  /* world position of grid point (0, 0, 0); no default */
  double voxel;      /* grid spacing, > 0; no default */
  int nx, ny, nz;    /* grid points per axis, each >= 2, nx * ny * nz <= 2^27; no default */
  double trunc;      /* truncation distance, >= 0 (default 0 = 4 * voxel, resolved at create) */
  double disp_min;   /* disparities below this (pixels) are not integrated (default 1.0, the grid mesh's rule) */
  int min_weight;    /* a grid point is defined for extraction when count >= min_weight (default 1) */
  int max_views;     /* pending views held on the device (default 64); adding to a full stack integrates it first */
} sfmx_fusion_params;
/* one view: the left rectified camera of a pair (sfmx_stereo_rect: rows of R_rw are the camera axes in world coordinates,
 * c_left its centre, f / cx / cy its pinhole, B the baseline) and the size of its disparity map */
typedef struct sfmx_fusion_view {
  double R_rw[9], c_left[3];
  double f, cx, cy, B;
  int w, h;
} sfmx_fusion_view;
void sfmx_fusion_default_params(sfmx_fusion_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_fusion_check_params(const sfmx_fusion_params* p);
int sfmx_fusion_create(sfmx_ctx* ctx, const sfmx_fusion_params* p, sfmx_fusion** out);
void sfmx_fusion_destroy(sfmx_ctx* ctx, sfmx_fusion* fu);
/* zero sum and count, drop the pending views */
int sfmx_fusion_reset(sfmx_ctx* ctx, sfmx_fusion* fu);
/* queue a view: disp16 int16 [h][w] (x 16, -16 = invalid), a host pointer or (on_device = 1) a device pointer */
int sfmx_fusion_add_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device);
/* queue a view whose disparity is the last map sfmx_stereo_disparity computed on st (copied device to device) */
int sfmx_fusion_add_stereo_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_stereo* st);
/* integrate every pending view in one launch */
int sfmx_fusion_integrate(sfmx_ctx* ctx, sfmx_fusion* fu);
/* integrates the pending views, then sum (double) / count (int32) [nz][ny][nx] to the host; either may be NULL */
int sfmx_fusion_read(sfmx_ctx* ctx, sfmx_fusion* fu, double* sum, int32_t* count);
/* integrates the pending views, then extracts the surface: verts double [n][3], faces int32 [m][3].  n_verts / n_faces are
 * always set; with verts and faces NULL only the counts are computed; caps below the counts give SFMX_ERR_INVALID. */
int sfmx_fusion_extract(sfmx_ctx* ctx, sfmx_fusion* fu, double* verts, int verts_cap, int32_t* faces, int faces_cap, int* n_verts,
                        int* n_faces);
/* device time (us) of the last sfmx_fusion_integrate / _extract when timing is on (sfmx_set_timing), else 0 */
double sfmx_fusion_last_us(const sfmx_fusion* fu);

/* ---- appearance of the fused surface: vertex normals and multi-view vertex intensity ---------------------- */
/* Normals are the normalised gradient of the volume's signed distance (central differences, one-sided next to undefined grid
 * points), interpolated along each vertex's edge with the extraction's own t; they point out of the surface.  Intensity is
 * the rounded mean of the rectified left images over the views that see the vertex: it faces the camera (cull) and the view's
 * own depth at its pixel agrees with the vertex's within depth_tol.  The projection is the integration's, everything after
 * the depth test is integer, so both are bit-identical to the NumPy restatement in tests/appearance_ref.py. */
/* sfmx_fusion_extract with normals: the same verts and faces bit for bit, plus normals double [n][3] in vertex order (zero
 * where the gradient vanishes).  With verts, faces and normals NULL only the counts are computed; otherwise all three are
 * required.  The vertices and normals stay on the device inside fu for sfmx_shade_fusion until the volume changes
 * (integrate, reset) or sfmx_fusion_extract overwrites them. */
int sfmx_fusion_extract_normals(sfmx_ctx* ctx, sfmx_fusion* fu, double* verts, int verts_cap, int32_t* faces, int faces_cap,
                                double* normals, int* n_verts, int* n_faces);
/* device time (us) of the normals kernel of the last sfmx_fusion_extract_normals when timing is on, else 0 (it is also part
 * of sfmx_fusion_last_us) */
double sfmx_fusion_normals_us(const sfmx_fusion* fu);

typedef struct sfmx_shade sfmx_shade;  /* retained views: camera, disparity map and left rectified image, on the device */
typedef struct sfmx_shade_params {
  double depth_tol;  /* a view sees a vertex when |Z(view pixel) - depth of the vertex| <= depth_tol; > 0; no default */
  double disp_min;   /* disparities below this (pixels) are not used (default 1.0) */
  int cull;          /* 1 (default): only views the vertex's normal faces, n . (X - c_left) < 0; 0: off */
  int fill;          /* grey of a vertex no view sees, 0..255 (default 0) */
} sfmx_shade_params;
void sfmx_shade_default_params(sfmx_shade_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_shade_check_params(const sfmx_shade_params* p);
int sfmx_shade_create(sfmx_ctx* ctx, sfmx_shade** out);
void sfmx_shade_destroy(sfmx_ctx* ctx, sfmx_shade* sh);
/* drop every view (the device memory is kept for the next ones) */
int sfmx_shade_reset(sfmx_ctx* ctx, sfmx_shade* sh);
/* append a view: disp16 int16 [h][w] (x 16, -16 = invalid) and its left rectified image u8 [h][w], both host pointers or
 * (on_device = 1) both device pointers; copied (3 bytes per pixel, kept until reset / destroy).  Views of different sizes
 * may be mixed; w <= 4096.  There is no view limit: the storage grows. */
int sfmx_shade_add_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const int16_t* disp16, const uint8_t* image,
                        int on_device);
/* append the last disparity map and left rectified image sfmx_stereo_disparity computed on st (copied device to device) */
int sfmx_shade_add_stereo_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const sfmx_stereo* st);
int sfmx_shade_view_count(const sfmx_shade* sh);
/* verts / normals double [n][3], host pointers or (on_device = 1) device pointers; normals may be NULL only with cull = 0.
 * grey_out u8 [n] and views_out int32 [n] (the number of views that saw the vertex) on the host; either may be NULL.
 * n = 0 or no views is not an error (every vertex gets fill and 0). */
int sfmx_shade_vertices(sfmx_ctx* ctx, sfmx_shade* sh, const double* verts, const double* normals, int n, int on_device,
                        const sfmx_shade_params* p, uint8_t* grey_out, int32_t* views_out);
/* the same for the vertices and normals the last sfmx_fusion_extract_normals left on the device inside fu (no host round
 * trip); SFMX_ERR_INVALID when fu holds none.  grey_out / views_out are sized by that call's n_verts. */
int sfmx_shade_fusion(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion* fu, const sfmx_shade_params* p, uint8_t* grey_out,
                      int32_t* views_out);
/* device time (us) of the kernel of the last sfmx_shade_vertices / _fusion when timing is on (sfmx_set_timing), else 0 */
double sfmx_shade_last_us(const sfmx_shade* sh);

/* ---- multi-view consistency filtering of disparity maps before fusion ----------------------------------- */
/* A consist object keeps an ordered list of views (a sfmx_fusion_view and its disp16 map, as sfmx_fusion / sfmx_shade take
 * them).  sfmx_consist_filter keeps a pixel's disparity only if at least min_support OTHER views (other by index), looked up
 * at the pixel its 3-D point projects to, hold a depth that agrees within rel_tol and whose own 3-D point projects back to
 * within reproj_px of the pixel; every other pixel becomes -16.  Every test reads the unfiltered maps, the results go to a
 * second slab, and the support is an integer count of independent tests: IEEE double in one fixed expression order up to
 * each comparison, so the filtered maps, the support counts and the counters are bit-identical to the NumPy restatement in
 * tests/consist_ref.py whatever the launch shape. */
typedef struct sfmx_consist sfmx_consist;  /* retained views: camera and disparity map, and the filtered maps, on the device */
typedef struct sfmx_consist_params {
  double rel_tol;    /* the other view's depth Z' agrees when |Z' - q2| <= rel_tol * q2; > 0, finite (default 0.01) */
  double reproj_px;  /* its point projects back to within this many pixels; >= 0 (default 1.0) */
  double disp_min;   /* disparities below this (pixels) are invalid, here and in the other views (default 1.0) */
  int min_support;   /* agreeing other views a pixel needs to be kept; >= 0 (default 2; 0 keeps every valid pixel) */
} sfmx_consist_params;
void sfmx_consist_default_params(sfmx_consist_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_consist_check_params(const sfmx_consist_params* p);
int sfmx_consist_create(sfmx_ctx* ctx, sfmx_consist** out);
void sfmx_consist_destroy(sfmx_ctx* ctx, sfmx_consist* cs);
/* drop every view and the result (the device memory is kept for the next ones) */
int sfmx_consist_reset(sfmx_ctx* ctx, sfmx_consist* cs);
/* append a view: disp16 int16 [h][w] (x 16, -16 = invalid), a host pointer or (on_device = 1) a device pointer; copied.
 * Views of different sizes may be mixed; w <= 4096, w * h < 2^30.  There is no view limit: the storage grows. */
int sfmx_consist_add_view(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_fusion_view* view, const int16_t* disp16, int on_device);
/* append the last disparity map sfmx_stereo_disparity computed on st (copied device to device) */
int sfmx_consist_add_stereo_view(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_fusion_view* view, const sfmx_stereo* st);
int sfmx_consist_view_count(const sfmx_consist* cs);
/* filter every view against every other in one launch; 0 views is not an error.  The result stays valid until a view is
 * added or the object is reset. */
int sfmx_consist_filter(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_consist_params* p);
/* view i of the last filter to the host: disp16_out int16 [h][w] (the kept disparities, -16 elsewhere) and support_out u8
 * [h][w] (agreeing views, saturated at 255; 0 where the input is invalid); either may be NULL.  SFMX_ERR_INVALID without a
 * current result or with i out of range. */
int sfmx_consist_read(sfmx_ctx* ctx, sfmx_consist* cs, int i, int16_t* disp16_out, uint8_t* support_out);
/* per view of the last filter: valid_out / kept_out int32 [view count], the pixels that were valid and the pixels kept
 * (counted on the device); either may be NULL.  SFMX_ERR_INVALID without a current result. */
int sfmx_consist_counts(sfmx_ctx* ctx, sfmx_consist* cs, int32_t* valid_out, int32_t* kept_out);
/* queue view i of cs (its camera and its FILTERED map, copied device to device) into fu, as sfmx_fusion_add_view would.
 * SFMX_ERR_INVALID without a current result or with i out of range. */
int sfmx_fusion_add_consist_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_consist* cs, int i);
/* device time (us) of the kernel of the last sfmx_consist_filter when timing is on (sfmx_set_timing), else 0 */
double sfmx_consist_last_us(const sfmx_consist* cs);

/* ---- small connected components of a triangle mesh, removed on the device -------------------------------- */
/* Two vertices are connected when a face holds both; label(v) is the smallest vertex index of v's component and
 * comp_faces(v) the number of faces f with label(f[0]) == label(v) (a vertex no face uses is a component of 0 faces).  A
 * component of cf faces is kept when cf >= 1, cf >= min_faces and cf * 1000 >= largest * min_permille (64-bit; largest = the
 * greatest cf, so components of equal size are kept or dropped together).  Kept faces stay in input order, kept vertices (those
 * a kept face uses) in ascending input index with their bytes copied, face indices are renumbered.  Everything is an integer
 * or a byte copy, so every output is bit-identical to the NumPy restatement in tests/clean_ref.py whatever the schedule. */
typedef struct sfmx_clean sfmx_clean;  /* device work buffers and the last result; they grow on demand and are kept */
typedef struct sfmx_clean_params {
  int min_faces;     /* a kept component has at least this many faces; >= 0 (default 0) */
  int min_permille;  /* ... and at least this many thousandths of the largest component's faces; 0..1000 (default 10) */
} sfmx_clean_params;
void sfmx_clean_default_params(sfmx_clean_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_clean_check_params(const sfmx_clean_params* p);
int sfmx_clean_create(sfmx_ctx* ctx, sfmx_clean** out);
void sfmx_clean_destroy(sfmx_ctx* ctx, sfmx_clean* cl);
/* verts double [n][3] (copied as bytes, never computed with: NaN is allowed), normals double [n][3] or NULL, faces int32
 * [m][3]; host pointers or (on_device = 1) device pointers, 0 <= n, m < 2^30.  A face index outside [0, n) is found on the
 * device without any access through it and gives SFMX_ERR_INVALID; the object stays usable.  The four counts (cleaned
 * vertices and faces, components with at least one face, faces of the largest) may each be NULL. */
int sfmx_clean_run(sfmx_ctx* ctx, sfmx_clean* cl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_clean_params* p, int* n_verts_out, int* n_faces_out, int* n_components, int* largest);
/* the same for the surface the last sfmx_fusion_extract / _extract_normals with arrays left on the device inside fu (no host
 * round trip), with its normals when that call made them; SFMX_ERR_INVALID when fu holds none (never extracted, or the volume
 * has changed since: integrate, reset) */
int sfmx_clean_fusion(sfmx_ctx* ctx, sfmx_clean* cl, const sfmx_fusion* fu, const sfmx_clean_params* p, int* n_verts_out,
                      int* n_faces_out, int* n_components, int* largest);
/* the last successful run to the host: verts_out / normals_out double [n'][3], faces_out int32 [m'][3], vert_src int32 [n'] and
 * face_src int32 [m'] (the input index of each output element), vert_label / vert_comp_faces int32 [n] (per INPUT vertex); any
 * may be NULL (normals_out is left alone when the run had no normals).  SFMX_ERR_INVALID before a successful run; a run or
 * _fusion call that fails for any reason (parameters included) leaves no result. */
int sfmx_clean_read(sfmx_ctx* ctx, sfmx_clean* cl, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src,
                    int32_t* face_src, int32_t* vert_label, int32_t* vert_comp_faces);
/* the sizes sfmx_clean_read copies by: input vertices and faces (n, m) and cleaned vertices and faces (n', m') of the last
 * successful run; any pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_clean_sizes(const sfmx_clean* cl, int* n, int* m, int* n_verts_out, int* n_faces_out);
/* the cleaned vertices and normals of the last successful run on the device (for sfmx_shade_vertices with on_device = 1);
 * *normals is NULL when the run had none.  Returns n', or -1 before a successful run.  Valid until the next run on cl. */
int sfmx_clean_device_surface(const sfmx_clean* cl, const double** verts, const double** normals);
/* device time (us) of the launches of the last sfmx_clean_run / _fusion when timing is on (sfmx_set_timing), else 0 */
double sfmx_clean_last_us(const sfmx_clean* cl);

/* ---- distance from points to the nearest point of a triangle mesh ------------------------------------------ */
/* For each query p: d2 = the smallest squared point-triangle distance over the faces whose bounding box, grown by
 * d_max (1 + 2^-10) on every side, holds p, and face = the smallest index of a face attaining it; when there is no such face
 * or !(d2 < d_max^2), d2 = d_max^2 and face = -1.  The point-triangle distance is one fixed sequence of IEEE double operations
 * (csrc/hip/sfmx_sdist_math.h), and a minimum does not depend on the order of its candidates: d2 and face are bit-identical to
 * the brute-force NumPy restatement in tests/sdist_ref.py for every cell size.  The distance itself is sqrt(d2), taken by
 * the caller.  The uniform grid behind it only changes the speed. */
#define SFMX_SDIST_CHUNK 64 /* triangles of a cell staged through LDS at a time */
typedef struct sfmx_sdist sfmx_sdist;  /* a copy of the target mesh, its grid and the work buffers; they grow on demand and are kept */
typedef struct sfmx_sdist_params {
  double d_max;  /* distances are clipped here; 2^-500 <= d_max <= 2^60 (its square neither underflows nor, with the coordinate
                  * limit below, does a distance overflow); no default (a length in the caller's units) */
  double cell;   /* edge of a grid cell; 0 (default): 2 d_max, doubled until the grid has <= 2^24 cells and <= 2^30 entries */
} sfmx_sdist_params;
void sfmx_sdist_default_params(sfmx_sdist_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_sdist_check_params(const sfmx_sdist_params* p);
int sfmx_sdist_create(sfmx_ctx* ctx, sfmx_sdist** out);
void sfmx_sdist_destroy(sfmx_ctx* ctx, sfmx_sdist* sd);
/* verts double [nv][3], faces int32 [m][3]; host pointers or (on_device = 1) device pointers, copied; 0 <= nv, m < 2^30.
 * SFMX_ERR_INVALID (found on the device, nothing is read through a bad index) for a face index outside [0, nv), a non-finite
 * coordinate in a vertex that a face uses, a coordinate beyond 2^40 d_max in magnitude, or an explicit cell that does not fit
 * the two limits above.  A failed call leaves no target; the object stays usable.  m = 0 is a valid target (every query is
 * clipped).  Faces with repeated indices and collinear faces are allowed: their distance is that of their segments. */
int sfmx_sdist_set_target(sfmx_ctx* ctx, sfmx_sdist* sd, const double* verts, int nv, const int32_t* faces, int m, int on_device,
                          const sfmx_sdist_params* p);
/* the same for the surface the last sfmx_fusion_extract / _extract_normals with arrays left on the device inside fu, and for
 * the cleaned surface of the last successful run on cl (no host round trip); SFMX_ERR_INVALID when there is none */
int sfmx_sdist_set_target_fusion(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_fusion* fu, const sfmx_sdist_params* p);
int sfmx_sdist_set_target_clean(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_clean* cl, const sfmx_sdist_params* p);
/* points double [n][3], a host pointer or (on_device = 1) a device pointer; d2_out double [n] and face_out int32 [n] on the
 * host, either may be NULL.  n = 0 is not an error.  SFMX_ERR_INVALID before a successful set_target, and for a non-finite
 * coordinate in a query (the target stays). */
int sfmx_sdist_query(sfmx_ctx* ctx, sfmx_sdist* sd, const double* points, int n, int on_device, double* d2_out, int32_t* face_out);
/* the same with the vertices of that device surface as queries.  The outputs hold cap entries each; a surface with more
 * vertices is refused (SFMX_ERR_INVALID, nothing written) unless both outputs are NULL.  *n_out (may be NULL) = its vertex
 * count, 0 on failure. */
int sfmx_sdist_query_fusion(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_fusion* fu, int cap, double* d2_out, int32_t* face_out,
                            int* n_out);
int sfmx_sdist_query_clean(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_clean* cl, int cap, double* d2_out, int32_t* face_out,
                           int* n_out);
/* of the current target: dims3 int [3] (cells per axis, zeros for a target without faces), entries (triangle-cell pairs), the
 * cell size used; tests = point-triangle pairs the last query visited (an integer counter on the device); kernel_us = the device
 * time (us) of the query kernel alone inside the last query when timing is on, else 0 (the rest of sfmx_sdist_last_us is the
 * binning).  Any may be NULL.  SFMX_ERR_INVALID (and zeros) without a target; needs no context. */
int sfmx_sdist_stats(const sfmx_sdist* sd, int* dims3, int* entries, double* cell, uint64_t* tests, double* kernel_us);
/* device time (us) from the first to the last launch of the last sfmx_sdist_set_target* / _query* when timing is on, else 0 */
double sfmx_sdist_last_us(const sfmx_sdist* sd);

/* ---- rendering the volume from any camera: TSDF ray casting ------------------------------------------------ */
/* Per pixel (x, y) of a pinhole camera the ray c + z dw, dw = R_rw^T ((x - cx) / f, (y - cy) / f, 1), is sampled at the depths
 * z_k = z_min + k step, k = 0 .. K - 1 with K = floor((z_max - z_min) / step) + 1.  The value at a sample is the trilinear
 * interpolation of s = sum / count over the 8 corners of its cell and exists only inside the grid with all 8 corners defined
 * (count >= min_weight).  The hit is the first k >= 1 whose two samples both have a value with s_{k-1} > 0 >= s_k, placed by
 * linear interpolation between them; its normal is the volume's gradient interpolated the same way at the hit
 * point and normalised (0 where a corner of that cell is undefined or the gradient vanishes); shaded is a head light,
 * round(255 max(0, -n . dw / |dw|)).  A pixel without a hit has depth 0, a zero point and normal, and shaded = background.
 * Everything is IEEE double in one fixed expression order, the sample lattice never moves (samples outside the grid are
 * skipped, which is exact), so every output is bit-identical to the NumPy restatement in tests/raycast_ref.py.
 * The camera is a sfmx_fusion_view: R_rw, c_left, f (> 0), cx, cy, w, h are used, B is ignored.  w <= 4096, w * h <= 2^24. */
#define SFMX_RAYCAST_MAX_SAMPLES (1 << 20) /* K */
#define SFMX_RAYCAST_MAX_PIXELS (1 << 24)  /* w * h */
typedef struct sfmx_raycast sfmx_raycast;  /* the device outputs of the last render; they grow on demand and are kept */
typedef struct sfmx_raycast_params {
  double z_min, z_max; /* depths along the optical axis: 0 < z_min < z_max, finite; no default */
  double step;         /* sample spacing in depth, >= 0; 0 (default) = voxel / 2, resolved per call */
  int min_weight;      /* a grid point is defined when count >= min_weight; 0 (default) = the volume's own */
  uint8_t background;  /* shaded value of a pixel without a hit (default 0) */
} sfmx_raycast_params;
void sfmx_raycast_default_params(sfmx_raycast_params* p);
/* SFMX_OK or SFMX_ERR_INVALID (K is checked when step > 0; a step of 0 is checked again per render); needs no device */
int sfmx_raycast_check_params(const sfmx_raycast_params* p);
int sfmx_raycast_create(sfmx_ctx* ctx, sfmx_raycast** out);
void sfmx_raycast_destroy(sfmx_ctx* ctx, sfmx_raycast* rc);
/* integrates fu's pending views (as sfmx_fusion_extract does), then renders its volume.  A render that hits nothing is not an
 * error.  A failed render leaves no result. */
int sfmx_raycast_render(sfmx_ctx* ctx, sfmx_raycast* rc, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_raycast_params* p);
/* the same for any volume: sum double / count int32 [nz][ny][nx], host pointers (copied) or (on_device = 1) device pointers
 * (read in place); vol gives origin, voxel, nx, ny, nz and min_weight and is checked by sfmx_fusion_check_params */
int sfmx_raycast_render_arrays(sfmx_ctx* ctx, sfmx_raycast* rc, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                               int on_device, const sfmx_fusion_view* view, const sfmx_raycast_params* p);
/* the last render to the host: depth double [h][w], normals / points double [h][w][3], shaded u8 [h][w], *hits = hit pixels;
 * any may be NULL.  SFMX_ERR_INVALID before a render. */
int sfmx_raycast_read(sfmx_ctx* ctx, sfmx_raycast* rc, double* depth, double* normals, double* points, uint8_t* shaded, int32_t* hits);
/* the points and normals of all w * h pixels of the last render on the device (for sfmx_shade_vertices with on_device = 1);
 * *n = w * h.  SFMX_ERR_INVALID (and NULLs, 0) before a render; needs no context.  Valid until the next render on rc. */
int sfmx_raycast_device_surface(const sfmx_raycast* rc, const double** points, const double** normals, int* n);
/* a novel-view grey image: sfmx_shade_vertices over the last render's device points and normals (no host round trip), then
 * every pixel without a hit gets the render's background and 0 views.  grey_out u8 [h][w], views_out int32 [h][w]; either may
 * be NULL.  SFMX_ERR_INVALID before a render. */
int sfmx_raycast_shade(sfmx_ctx* ctx, sfmx_raycast* rc, sfmx_shade* sh, const sfmx_shade_params* p, uint8_t* grey_out,
                       int32_t* views_out);
/* device time (us) of the kernel of the last render when timing is on (sfmx_set_timing), else 0 */
double sfmx_raycast_last_us(const sfmx_raycast* rc);
/* samples the last render evaluated (inside the grid, up to each ray's hit), counted on the device; 0 before a render */
uint64_t sfmx_raycast_last_samples(const sfmx_raycast* rc);

/* ---- registering a view to the volume: direct TSDF pose alignment ----------------------------------------- */
/* The pixels (stride i, stride j) of a view's disparity map are lifted to world points X with the view's pose (the integration's
 * own lift); a sample is used when its disparity counts (not -16, >= disp_min), X lies inside the grid with all 8 corners of its
 * cell defined (count >= min_weight) and the interpolated signed distance s has |s| < 1.  With the volume's gradient G
 * interpolated the same way, gw = G / voxel, the pivot p = the box centre and q = X - p, the row of the sample is
 * J = (q x gw, gw).  One evaluation gives 28 sums over the samples in one fixed order: A_mn = sum J_m J_n for m <= n (21, row by
 * row), b_m = sum J_m s (6), e = sum s^2 (1), and n, the samples used.  A Gauss-Newton step solves (A + damping I) delta = -b by
 * Cholesky on the host and applies delta = (omega, v) as a rotation about p (Cayley: rational, no trigonometry) and a
 * translation.  Everything is IEEE double in one fixed expression order and the sums are one fixed tree, so sums, n and every
 * iterate are bit-identical to the NumPy restatement in tests/align_ref.py. */
#define SFMX_ALIGN_ITERS_CAP 64 /* max_iters, and the length of the trace */
enum { SFMX_ALIGN_CONVERGED = 0, SFMX_ALIGN_MAX_ITERS = 1, SFMX_ALIGN_TOO_FEW = 2, SFMX_ALIGN_DEGENERATE = 3 };
typedef struct sfmx_align sfmx_align;  /* device work buffers; they grow on demand and are kept */
typedef struct sfmx_align_params {
  int max_iters;    /* evaluations at most, 1 .. 64 (default 10) */
  int stride;       /* every stride-th pixel of every stride-th row is a sample, >= 1 (default 1) */
  double disp_min;  /* disparities below this (pixels) are not used (default 1.0); finite */
  int min_weight;   /* a grid point is defined when count >= min_weight; 0 (default) = the volume's own */
  int min_pixels;   /* fewer used samples than this end the loop with TOO_FEW, >= 1 (default 64) */
  double damping;   /* added to the diagonal of A, >= 0 (default 0) */
  double eps_rot;   /* converged when |omega| <= eps_rot (radians to first order; default 1e-6) ... */
  double eps_trans; /* ... and |v| <= eps_trans * voxel (default 1e-4) */
} sfmx_align_params;
typedef struct sfmx_align_result {
  sfmx_fusion_view view; /* the refined view: R_rw and c_left move, f, cx, cy, B, w, h are the input's */
  int status;            /* SFMX_ALIGN_CONVERGED, _MAX_ITERS, _TOO_FEW (n < min_pixels) or _DEGENERATE (a Cholesky pivot <= 0) */
  int iterations;        /* evaluations made */
  int32_t n[SFMX_ALIGN_ITERS_CAP];   /* per evaluation: samples used ... */
  double e[SFMX_ALIGN_ITERS_CAP];     /* ... sum s^2 ... */
  double rot[SFMX_ALIGN_ITERS_CAP];   /* ... |omega| of the step taken (0 when none was) ... */
  double trans[SFMX_ALIGN_ITERS_CAP]; /* ... and |v| */
} sfmx_align_result;
void sfmx_align_default_params(sfmx_align_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_align_check_params(const sfmx_align_params* p);
int sfmx_align_create(sfmx_ctx* ctx, sfmx_align** out);
void sfmx_align_destroy(sfmx_ctx* ctx, sfmx_align* al);
/* one evaluation at the given view, no step: integrates fu's pending views (as sfmx_fusion_extract does), then sums double [28]
 * (A row by row upper, b, e) and *n.  disp16 int16 [h][w] (x 16, -16 = invalid), a host pointer or (on_device = 1) a device one */
int sfmx_align_system(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                      const sfmx_align_params* p, double* sums, int32_t* n);
/* the same for any volume: sum double / count int32 [nz][ny][nx], host pointers (copied) or (volume_on_device = 1) device
 * pointers (read in place); vol gives origin, voxel, nx, ny, nz and min_weight and is checked by sfmx_fusion_check_params */
int sfmx_align_system_arrays(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                             int volume_on_device, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                             const sfmx_align_params* p, double* sums, int32_t* n);
/* the Gauss-Newton loop from the given view: at most max_iters evaluations, each followed by a step unless it ends the loop.
 * TOO_FEW and DEGENERATE return the last view whose evaluation gave a step (the input view if none did).  The statuses are
 * results: the call returns SFMX_OK with them. */
int sfmx_align_view(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                    const sfmx_align_params* p, sfmx_align_result* out);
/* the loop for any volume, as sfmx_align_system_arrays */
int sfmx_align_view_arrays(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                           int volume_on_device, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                           const sfmx_align_params* p, sfmx_align_result* out);
/* the loop on the last map sfmx_stereo_disparity computed on st, read in place on the device */
int sfmx_align_stereo_view(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_stereo* st,
                           const sfmx_align_params* p, sfmx_align_result* out);
/* device time (us) of the evaluations of the last call when timing is on (sfmx_set_timing), else 0 */
double sfmx_align_last_us(const sfmx_align* al);

/* ---- registering a surface to a reference mesh: Sim(3) point-to-plane Gauss-Newton ------------------------- */
/* Everything is IEEE double in the written order, nothing is contracted, and sqrt is taken on the host only.
 *   transform T = (s, R[3][3], t[3]); identity = (1.0, I, 0)
 *   apply:      y_a = s*((R_a0*x0 + R_a1*x1) + R_a2*x2) + t_a
 *   target:     V double [nv][3], F int32 [m][3], d_max (and cell) exactly as sfmx_sdist_set_target takes them (same refusals)
 *   pivot:      p_a = 0.5*(min_a + max_a) over the target vertices that a face uses; min and max are taken in the order of the
 *               finite doubles with -0.0 below +0.0, so any reduction order gives the same bits; a target with m = 0 has
 *               pivot 0 and every evaluation has n_used = 0
 *   samples:    source points X double [n][3]; sample k = 0 .. ns-1, ns = ceil(n/stride), is point i = stride*k
 *   per sample: y = apply(T, x_i); (d2, f) = the sdist query of y against the target (unchanged)
 *               used iff f >= 0 and nn > 0, with a, b, c = V[F[f]]; u = b-a; v = c-a; n = cross(u, v) and nn = dot(n, n) in
 *               sfmx_sdist_math.h's own expressions
 *               h = dot(y-a, n); q = y - p; w = 1.0/nn
 *               J = (q1*n2 - q2*n1, q2*n0 - q0*n2, q0*n1 - q1*n0, n0, n1, n2, dot(q, n))
 *   terms (37, this order): A_mn = (J_m*J_n)*w for m <= n row by row (28); b_m = (J_m*h)*w (7); e = (h*h)*w (1); c = d2 (1);
 *               an unused sample contributes +0.0 to all 37; n_used = used samples (int32)
 *   ordered sum: the tree of the view alignment above with rows of 37: sample k is in block k/256, lane = k%64,
 *               wave = (k%256)/64, tree index 4*lane + wave; block partials in groups of 256 rows, recursively, padding +0.0;
 *               ns = 0 gives 37 times +0.0
 *   solve (host): that stage's Cholesky, forward and backward substitution at dimension 7 (with_scale) or 6 (rows / columns
 *               0..5 only), M_mm = A_mm + damping; a pivot d <= 0 or not finite: DEGENERATE
 *               omega = delta[0:3], v = delta[3:6], sigma = delta[6] (0.0 without scale)
 *   update:     D = that stage's Cayley matrix of omega, element by element; g = 1.0 + sigma; !(g > 0): DEGENERATE
 *               s' = g*s; R'_ab = (D_a0*R_0b + D_a1*R_1b) + D_a2*R_2b; u = t - p
 *               t'_a = (p_a + g*((D_a0*u0 + D_a1*u1) + D_a2*u2)) + v_a
 *               a T' with a non-finite entry or !(s' > 0) (overflow, underflow): DEGENERATE
 *   loop:       at most max_iters evaluations, starting from init (identity when NULL).  n_used < min_points: TOO_FEW.
 *               Otherwise step; CONVERGED when, after the update, |omega| <= eps_rot and fabs(sigma) <= eps_scale and
 *               |v| <= eps_trans*d_max (|x| = sqrt((x0*x0 + x1*x1) + x2*x2)).  Out of evaluations: MAX_ITERS.
 *               TOO_FEW / DEGENERATE return the last transform whose evaluation gave a step (init if none did).
 *               trace per evaluation: n_used, e, c, |omega|, |v|, sigma (zeros when no step was taken)
 * (h*h)/nn is the squared distance to the plane of the face sdist names (the smallest index among those attaining the minimum),
 * even where the nearest point lies on its edge or corner; a correspondence is dropped exactly when sdist clips it, so d_max is
 * the trimming distance.  c only gives the point-to-point RMS sqrt(c/n_used) of the trace.  Sums, n_used, the pivot and every
 * iterate are bit-identical to the NumPy restatement in tests/register_ref.py. */
#define SFMX_REGISTER_ITERS_CAP 64 /* max_iters, and the length of the trace */
#define SFMX_REGISTER_TERMS 37
enum { SFMX_REGISTER_CONVERGED = 0, SFMX_REGISTER_MAX_ITERS = 1, SFMX_REGISTER_TOO_FEW = 2, SFMX_REGISTER_DEGENERATE = 3 };
typedef struct sfmx_register sfmx_register;  /* an sdist object with the target, and device work buffers; they grow on demand */
typedef struct sfmx_register_params {
  double d_max;     /* the trimming distance, as sfmx_sdist_params.d_max; no default */
  double cell;      /* as sfmx_sdist_params.cell (default 0) */
  int max_iters;    /* evaluations at most, 1 .. 64 (default 20) */
  int stride;       /* every stride-th source point is a sample, >= 1 (default 1) */
  int min_points;   /* fewer used samples than this end the loop with TOO_FEW, >= 7 (default 16) */
  int with_scale;   /* 1 (default): seven parameters; 0: six, the scale stays */
  double damping;   /* added to the diagonal of A, >= 0 (default 0) */
  double eps_rot;   /* converged when |omega| <= eps_rot (default 1e-4) ... */
  double eps_scale; /* ... and fabs(sigma) <= eps_scale (default 1e-4) ... */
  double eps_trans; /* ... and |v| <= eps_trans * d_max (default 1e-3); all three >= 0 and finite */
} sfmx_register_params;
typedef struct sfmx_register_transform {
  double s;    /* > 0 */
  double R[9]; /* row-major */
  double t[3];
} sfmx_register_transform;
typedef struct sfmx_register_result {
  sfmx_register_transform T; /* source -> target */
  int status;                /* SFMX_REGISTER_CONVERGED, _MAX_ITERS, _TOO_FEW or _DEGENERATE */
  int iterations;            /* evaluations made */
  int32_t n[SFMX_REGISTER_ITERS_CAP];    /* per evaluation: samples used ... */
  double e[SFMX_REGISTER_ITERS_CAP];     /* ... sum (h h) / nn ... */
  double c[SFMX_REGISTER_ITERS_CAP];     /* ... sum d2 ... */
  double rot[SFMX_REGISTER_ITERS_CAP];   /* ... |omega| of the step taken (0 when none was) ... */
  double trans[SFMX_REGISTER_ITERS_CAP]; /* ... |v| ... */
  double sigma[SFMX_REGISTER_ITERS_CAP]; /* ... and sigma */
} sfmx_register_result;
void sfmx_register_default_params(sfmx_register_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_register_check_params(const sfmx_register_params* p);
int sfmx_register_create(sfmx_ctx* ctx, sfmx_register** out);
void sfmx_register_destroy(sfmx_ctx* ctx, sfmx_register* rg);
/* as sfmx_sdist_set_target with p's d_max and cell (host pointers, or device pointers with on_device = 1; copied), every
 * refusal of it included; p is checked as a whole.  A failed call leaves no target; the object stays usable. */
int sfmx_register_set_target(sfmx_ctx* ctx, sfmx_register* rg, const double* verts, int nv, const int32_t* faces, int m, int on_device,
                             const sfmx_register_params* p);
/* the pivot of the current target; SFMX_ERR_INVALID (and zeros) without one; needs no context */
int sfmx_register_pivot(const sfmx_register* rg, double* pivot3);
/* one evaluation at T (identity when NULL), no step: sums double [37] and *n_used.  points double [n][3], a host pointer or
 * (on_device = 1) a device pointer, 0 <= n < 2^30.  SFMX_ERR_INVALID, with the target kept, before a successful set_target, for
 * a sampled source coordinate (or its transform) that is not finite, a T with non-finite entries or s <= 0, bad parameters, and
 * a d_max or cell other than the target's. */
int sfmx_register_system(sfmx_ctx* ctx, sfmx_register* rg, const double* points, int n, int on_device, const sfmx_register_transform* T,
                         const sfmx_register_params* p, double* sums, int32_t* n_used);
/* the loop from init (identity when NULL); the statuses are results: the call returns SFMX_OK with them */
int sfmx_register_run(sfmx_ctx* ctx, sfmx_register* rg, const double* points, int n, int on_device, const sfmx_register_transform* init,
                      const sfmx_register_params* p, sfmx_register_result* out);
/* out double [n][3] on the host = apply(T, every point) */
int sfmx_register_apply(sfmx_ctx* ctx, sfmx_register* rg, const sfmx_register_transform* T, const double* points, int n, int on_device,
                        double* out);
/* device time (us) of the last call's own launches (k_rg_apply, k_rg_system, the tree; the pivot's reduction in set_target),
 * and of its sdist queries (set_target: the target's grid), when timing is on (sfmx_set_timing), else 0 */
double sfmx_register_last_us(const sfmx_register* rg);
double sfmx_register_last_query_us(const sfmx_register* rg);

/* ---- simplifying a triangle mesh: exact vertex clustering on a uniform grid --------------------------------- */
/* Per vertex and component q = (x - origin) / cell, c = floor(q), t = q - c and Q = (int64)floor(t 2^30 + 0.5), in this order in
 * IEEE double without contraction.  A cluster is an occupied cell; clusters are numbered in ascending linear index
 * (cx - cmin0) + dims0 ((cy - cmin1) + dims1 (cz - cmin2)) over the box of the occupied cells.  Every input vertex contributes to
 * its cluster: S = sum Q (int64) and cnt per cluster, position = origin + ((double)c + ((double)S / (double)cnt) / 2^30) cell.
 * With normals, Qn = (int64)floor(n 2^30 + 0.5), s = (double)sum Qn, len = sqrt((s0 s0 + s1 s1) + s2 s2), normal = s / len or 0
 * when len == 0.  A face becomes the triple of its corners' clusters: dropped as degenerate when two are equal, else rotated
 * (never reflected) so that its smallest cluster comes first; of the faces with the same triple only the one with the smallest
 * input index is kept (the others are duplicates; the reversed triple is another triple).  Kept faces stay in input order,
 * output vertices are the clusters a kept face uses in ascending cluster number, face indices are renumbered.  The sums are
 * integers, so every output is bit-identical to the NumPy restatement in tests/simplify_ref.py whatever the schedule. */
typedef struct sfmx_simplify sfmx_simplify;  /* device work buffers and the last result; they grow on demand and are kept */
typedef struct sfmx_simplify_params {
  double cell;       /* edge of a grid cell; finite, > 0; no default (a length in the caller's units) */
  double origin[3];  /* a corner of the grid; finite (default 0) */
} sfmx_simplify_params;
void sfmx_simplify_default_params(sfmx_simplify_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_simplify_check_params(const sfmx_simplify_params* p);
int sfmx_simplify_create(sfmx_ctx* ctx, sfmx_simplify** out);
void sfmx_simplify_destroy(sfmx_ctx* ctx, sfmx_simplify* sp);
/* verts double [n][3], normals double [n][3] or NULL, faces int32 [m][3]; host pointers or (on_device = 1) device pointers,
 * 0 <= n, m < 2^30.  SFMX_ERR_INVALID (found on the device, nothing is accessed through a bad index; the object stays usable
 * and no result is left) for a coordinate that is not finite or whose cell index exceeds 2^30 in magnitude, a normal component
 * that is not finite or exceeds 4 in magnitude, a face index outside [0, n), and a box of occupied cells of more than 2^27
 * cells.  The two counts (output vertices and faces) may each be NULL. */
int sfmx_simplify_run(sfmx_ctx* ctx, sfmx_simplify* sp, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                      int on_device, const sfmx_simplify_params* p, int* n_verts_out, int* n_faces_out);
/* the same for the surface the last sfmx_fusion_extract / _extract_normals with arrays left on the device inside fu, with its
 * normals when that call made them, and for the cleaned surface (and normals) of the last successful run on cl; no host round
 * trip.  SFMX_ERR_INVALID when there is none. */
int sfmx_simplify_fusion(sfmx_ctx* ctx, sfmx_simplify* sp, const sfmx_fusion* fu, const sfmx_simplify_params* p, int* n_verts_out,
                         int* n_faces_out);
int sfmx_simplify_clean(sfmx_ctx* ctx, sfmx_simplify* sp, const sfmx_clean* cl, const sfmx_simplify_params* p, int* n_verts_out,
                        int* n_faces_out);
/* the last successful run to the host: verts_out / normals_out double [n'][3], faces_out int32 [m'][3] (canonical form),
 * vert_dst int32 [n] (the output vertex of each INPUT vertex, or -1), face_src int32 [m'] (the input index of each output
 * face), members int32 [n'] (input vertices per output vertex); any may be NULL (normals_out is left alone when the run had no
 * normals).  SFMX_ERR_INVALID before a successful run; a call that fails for any reason (parameters included) leaves no result. */
int sfmx_simplify_read(sfmx_ctx* ctx, sfmx_simplify* sp, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_dst,
                       int32_t* face_src, int32_t* members);
/* the sizes sfmx_simplify_read copies by: input vertices and faces (n, m) and output vertices and faces (n', m') of the last
 * successful run; any pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_simplify_sizes(const sfmx_simplify* sp, int* n, int* m, int* n_verts_out, int* n_faces_out);
/* of the last successful run: clusters (occupied cells), degenerate and duplicate faces (m = degenerate + duplicates + m'), n'
 * and m'; any pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_simplify_counts(const sfmx_simplify* sp, int* clusters, int* degenerate, int* duplicates, int* n_verts_out, int* n_faces_out);
/* the output vertices and normals of the last successful run on the device (for sfmx_shade_vertices with on_device = 1);
 * *normals is NULL when the run had none.  Returns n', or -1 before a successful run.  Valid until the next run on sp. */
int sfmx_simplify_device_surface(const sfmx_simplify* sp, const double** verts, const double** normals);
/* the output vertices and faces on the device and *n_faces = m' (for sfmx_sdist_set_target / _query with on_device = 1); any
 * pointer may be NULL.  Returns n', or -1 before a successful run.  Valid until the next run on sp. */
int sfmx_simplify_device_mesh(const sfmx_simplify* sp, const double** verts, const int32_t** faces, int* n_faces);
/* device time (us) from the first to the last launch of the last run when timing is on (sfmx_set_timing), else 0 */
double sfmx_simplify_last_us(const sfmx_simplify* sp);

/* ---- smoothing a triangle mesh: exact Taubin lambda|mu filtering ------------------------------------------- */
/* Fixed point: per vertex and component q = (x - origin) / unit and Q = (int64)floor(q 2^20 + 0.5), in this order in IEEE double
 * without contraction.
 * Edges: face (a, b, c) has the directed edges a->b, b->c, c->a; one with equal ends is ignored (the face's other edges still
 * count).  An edge is an unordered pair {lo < hi} that some directed edge uses; fwd counts its uses as lo->hi and bwd as hi->lo.
 * It is regular when fwd == 1 && bwd == 1, boundary when fwd + bwd == 1, irregular otherwise.
 * Vertices: cnt is the number of edges at a vertex (its distinct neighbours N).  A vertex is isolated when cnt == 0; with pin = 1
 * it is pinned when at least one of its edges is not regular (with pin = 0 none is); it moves when it is neither.
 * Steps: 2 iters Jacobi steps, numbered from 0, each reading the positions the previous one left; the factor f is lambda on even
 * and mu on odd steps.  For a moving vertex and each component S = sum over N of Q_j (int64), m = (double)S / (double)cnt,
 * d = m - (double)Q, Q' = Q + (int64)floor(f d + 0.5), with no fma anywhere; other vertices keep their Q.  |Q'| > 2^38 at any
 * step fails the call (diverged).
 * Output: a moving vertex gets origin + ((double)Q 2^-20) unit, a pinned or isolated one keeps its input bytes; flags uint8 [n]
 * has bit 0 pinned and bit 1 isolated.  Faces are not touched and normals are not an input.  The sums are integers, so every
 * output is bit-identical to the NumPy restatement in tests/smooth_ref.py whatever the schedule. */
typedef struct sfmx_smooth sfmx_smooth;  /* device work buffers and the last result; they grow on demand and are kept */
typedef struct sfmx_smooth_params {
  double unit;       /* the length of one fixed-point unit 2^20; finite, > 0; no default (the voxel in the pipeline) */
  double origin[3];  /* finite (default 0) */
  double lambda;     /* 0 < lambda <= 1 (default 0.5) */
  double mu;         /* -1 <= mu <= 0 (default -0.53); 0 is plain Laplacian smoothing */
  int iters;         /* lambda|mu pairs, 1 .. 64 (default 10) */
  int pin;           /* 0 or 1 (default 1) */
} sfmx_smooth_params;
void sfmx_smooth_default_params(sfmx_smooth_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_smooth_check_params(const sfmx_smooth_params* p);
int sfmx_smooth_create(sfmx_ctx* ctx, sfmx_smooth** out);
void sfmx_smooth_destroy(sfmx_ctx* ctx, sfmx_smooth* sm);
/* verts double [n][3], faces int32 [m][3]; host pointers or (on_device = 1) device pointers, 0 <= n < 2^24, 0 <= m < 2^30.
 * SFMX_ERR_INVALID (found on the device, nothing is accessed through a bad index; the object stays usable and no result is
 * left) for a coordinate that is not finite or with |q| > 2^18, a face index outside [0, n), and divergence.  A mesh with more
 * than 2^30 - 1024 edges is refused the same way: the neighbour lists are indexed by int32. */
int sfmx_smooth_run(sfmx_ctx* ctx, sfmx_smooth* sm, const double* verts, int n, const int32_t* faces, int m, int on_device,
                    const sfmx_smooth_params* p);
/* the same for the surface the last sfmx_fusion_extract / _extract_normals with arrays left on the device inside fu, and for the
 * cleaned surface of the last successful run on cl; no host round trip.  SFMX_ERR_INVALID when there is none. */
int sfmx_smooth_fusion(sfmx_ctx* ctx, sfmx_smooth* sm, const sfmx_fusion* fu, const sfmx_smooth_params* p);
int sfmx_smooth_clean(sfmx_ctx* ctx, sfmx_smooth* sm, const sfmx_clean* cl, const sfmx_smooth_params* p);
/* the last successful run to the host: verts_out double [n][3], flags_out uint8 [n]; either may be NULL.  SFMX_ERR_INVALID
 * before a successful run; a call that fails for any reason (parameters included) leaves no result. */
int sfmx_smooth_read(sfmx_ctx* ctx, sfmx_smooth* sm, double* verts_out, uint8_t* flags_out);
/* vertices and faces (n, m) of the last successful run; either pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before a
 * successful run; needs no context. */
int sfmx_smooth_sizes(const sfmx_smooth* sm, int* n, int* m);
/* of the last successful run: edges, boundary and irregular edges, pinned and isolated vertices; any pointer may be NULL.
 * SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_smooth_counts(const sfmx_smooth* sm, int* edges, int* boundary_edges, int* irregular_edges, int* pinned, int* isolated);
/* the smoothed vertices and the input's faces on the device and *n_faces = m (for sfmx_simplify_run, sfmx_shade_vertices and
 * sfmx_sdist_set_target / _query with on_device = 1; the normals to go with them are the caller's own, unchanged); any pointer
 * may be NULL.  The faces are the object's own copy when the run had host pointers, else the pointer the run was given: they
 * live as long as their owner keeps them.  Returns n, or -1 before a successful run.  Valid until the next run on sm. */
int sfmx_smooth_device_mesh(const sfmx_smooth* sm, const double** verts, const int32_t** faces, int* n_faces);
/* the smoothed vertices, and the normals the run's source carried on the device: those of the extraction (sfmx_smooth_fusion) or
 * of the cleaned surface (sfmx_smooth_clean), unchanged and still owned by that object; *normals is NULL when it had none and
 * after sfmx_smooth_run.  Returns n, or -1 before a successful run.  Valid until the next run on sm. */
int sfmx_smooth_device_surface(const sfmx_smooth* sm, const double** verts, const double** normals);
/* device time (us) from the first to the last launch of the last run when timing is on (sfmx_set_timing), else 0 */
double sfmx_smooth_last_us(const sfmx_smooth* sm);

/* ---- filling the small holes of a triangle mesh: exact centroid fans ---------------------------------------- */
/* Fixed point, directed edges, the edge table {lo < hi} with fwd / bwd, and regular / boundary / irregular: as for sfmx_smooth
 * above.
 * Gaps: a boundary edge used as a->b has the gap half-edge b->a (tail b, head a).  out(v) and in(v) count the gap half-edges
 * that leave and enter v.  A vertex is simple when out == 1 && in == 1 and none of its edges is irregular, and complex when it
 * has a gap half-edge and is not simple.  next(v) of a simple v is the head of its one outgoing gap half-edge.
 * Loops: a cycle v0 -> next(v0) -> ... -> v0 of L >= 3 distinct vertices that are all simple; its leader is its smallest vertex
 * index and it is traversed from the leader along next.  It is filled when L <= max_edges.  Chains through a complex vertex and
 * longer cycles are left alone (the gaps at a complex vertex are not paired up).
 * Filling, in ascending leader order: L == 3 gives the face (v0, v1, v2) and no vertex.  L > 3 gives one new vertex c (numbered
 * n, n + 1, ... in loop order) and the faces (v_i, v_(i+1) mod L, c), i = 0 .. L-1: per component S = sum of Q over the loop
 * (int64), Qc = floor((2 S + L) / (2 L)) (a true floor), position origin + ((double)Qc 2^-20) unit.  With normals the new
 * vertex gets s / ln, or 0.0 unless ln > 0, where s starts at +0.0 and adds the loop's normals one by one in traversal order and
 * ln = sqrt((s0 s0 + s1 s1) + s2 s2), in IEEE double with no fma (a sum that becomes infinite is outside the contract).
 * Output: verts_out [n + K][3], normals_out [n + K][3], faces_out [m + F][3]; the first n (m) rows are the input bytes, the new
 * faces follow loop by loop.  Every filled rim edge becomes regular, a second run with the same parameters fills nothing, and
 * every output is bit-identical to the NumPy restatement in tests/fill_ref.py whatever the schedule. */
typedef struct sfmx_fill sfmx_fill;  /* device work buffers and the last result; they grow on demand and are kept */
typedef struct sfmx_fill_params {
  double unit;       /* the length of one fixed-point unit 2^20; finite, > 0; no default (the voxel in the pipeline) */
  double origin[3];  /* finite (default 0) */
  int max_edges;     /* the longest loop that is filled, 3 .. 1024 (default 32) */
} sfmx_fill_params;
void sfmx_fill_default_params(sfmx_fill_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_fill_check_params(const sfmx_fill_params* p);
int sfmx_fill_create(sfmx_ctx* ctx, sfmx_fill** out);
void sfmx_fill_destroy(sfmx_ctx* ctx, sfmx_fill* fl);
/* verts and normals double [n][3] (normals may be NULL), faces int32 [m][3]; host pointers or (on_device = 1) device pointers
 * that are not fl's own result arrays, 0 <= n < 2^24, 0 <= m < 2^30.  SFMX_ERR_INVALID (found on the device, nothing is accessed
 * through a bad index; the object stays usable and no result is left) for a coordinate that is not finite or with |q| > 2^18, a
 * face index outside [0, n), and n + K >= 2^24 or m + F >= 2^30.  A mesh with more than 2^30 - 1024 edges is refused the same
 * way: the offsets of the new faces are int32. */
int sfmx_fill_run(sfmx_ctx* ctx, sfmx_fill* fl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                  int on_device, const sfmx_fill_params* p);
/* the same for the surface the last sfmx_fusion_extract / _extract_normals with arrays left on the device inside fu (with its
 * normals if it made them), and for the cleaned surface of the last successful run on cl; no host round trip.
 * SFMX_ERR_INVALID when there is none. */
int sfmx_fill_fusion(sfmx_ctx* ctx, sfmx_fill* fl, const sfmx_fusion* fu, const sfmx_fill_params* p);
int sfmx_fill_clean(sfmx_ctx* ctx, sfmx_fill* fl, const sfmx_clean* cl, const sfmx_fill_params* p);
/* the last successful run to the host: verts_out and normals_out double [n + K][3], faces_out int32 [m + F][3]; any may be
 * NULL.  SFMX_ERR_INVALID before a successful run, and for normals_out after a run without normals; a call that fails for any
 * reason (parameters included) leaves no result. */
int sfmx_fill_read(sfmx_ctx* ctx, sfmx_fill* fl, double* verts_out, double* normals_out, int32_t* faces_out);
/* input and output vertices and faces (n, m, n + K, m + F) of the last successful run; any pointer may be NULL.
 * SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_fill_sizes(const sfmx_fill* fl, int* n, int* m, int* n_out, int* m_out);
/* of the last successful run: edges, boundary and irregular edges and complex vertices of the input, the loops filled, their
 * edges, K and F; any pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before a successful run; needs no context. */
int sfmx_fill_counts(const sfmx_fill* fl, int* edges, int* boundary_edges, int* irregular_edges, int* complex_vertices, int* filled_loops,
                     int* filled_edges, int* new_verts, int* new_faces);
/* the filled mesh on the device, the object's own arrays: *n_verts = n + K and *n_faces = m + F (for sfmx_smooth_run,
 * sfmx_simplify_run, sfmx_shade_vertices and sfmx_sdist_set_target / _query with on_device = 1); any pointer may be NULL.
 * Returns n + K, or -1 before a successful run.  Valid until the next run on fl. */
int sfmx_fill_device_mesh(const sfmx_fill* fl, const double** verts, const int32_t** faces, int* n_verts, int* n_faces);
/* the filled vertices and their normals, the object's own arrays of n + K rows: after a fill the vertex count differs from the
 * source's, so every later stage takes its normals from here.  *normals is NULL after a run without normals.  Returns n + K, or
 * -1 before a successful run.  Valid until the next run on fl. */
int sfmx_fill_device_surface(const sfmx_fill* fl, const double** verts, const double** normals);
/* device time (us) from the first to the last launch of the last run when timing is on (sfmx_set_timing), else 0 */
double sfmx_fill_last_us(const sfmx_fill* fl);

/* ---- rendering a triangle mesh from any camera: an exact z-buffer ------------------------------------------- */
/* Per vertex X: p = X - c, q_r = (R_rw[r][0] p0 + R_rw[r][1] p1) + R_rw[r][2] p2; near iff q2 >= z_min; u = (f q0) / q2 + cx,
 * v = (f q1) / q2 + cy; inband iff near and |u|, |v| <= 16384; U = (int64)floor(u 256 + 0.5), V likewise; r = 1 / q2.  Pixel
 * (x, y) is the point (256 x, 256 y).
 * Per face, in this order: an index outside [0, n) fails the call; a vertex that is not near: faces_behind (there is NO
 * near-plane clipping: such a face is dropped whole); a vertex that is not inband: faces_outside; A = (U1 - U0)(V2 - V0) -
 * (V1 - V0)(U2 - U0) == 0: faces_degenerate; the face is back-facing iff A > 0 (the image's y points down), counted in faces_back
 * before culling; cull = 1 drops back faces and cull = 2 front faces (faces_culled).
 * Coverage: with sg = sign(A) and, for vertex i, j = i + 1 mod 3, k = i + 2 mod 3: dx = sg (U_k - U_j), dy = sg (V_k - V_j),
 * e_i(x, y) = dx (256 y - V_j) - dy (256 x - U_j) in int64.  Pixel (x, y) of the image is covered iff for every i e_i > 0, or
 * e_i == 0 and (dy < 0 or (dy == 0 and dx > 0)) (the top-left rule: of two faces that share an edge exactly one owns a centre on
 * it).  A covered (face, pixel) pair is a fragment; faces_drawn counts the faces with at least one.
 * Depth of a fragment: s = ((double)e0 r0 + (double)e1 r1) + (double)e2 r2, depth = (double)|A| / s.  The pixel's winner is the
 * fragment with the smallest key (bits((float)depth) << 32) | face: depths are compared after rounding to float and equal ones go
 * to the smaller face index.
 * Per pixel with a winner, recomputed in double from the winning face: depth; point = c + depth dw with dw as in the ray
 * casting above; t_i = (double)e_i r_i; N = cross(X1 - X0, X2 - X0), or with normals N_a = (t0 n0a + t1 n1a) + t2 n2a;
 * normal = N / len or 0 unless len > 0; shaded = the ray casting's head light; with grey, g = ((t0 g0 + t1 g1) + t2 g2) / s and
 * grey = min(255, floor(g + 0.5)).  A pixel without one has face -1, depth 0, a zero point and normal and shaded = grey =
 * background.  hits counts the pixels with a winner, back_pixels those whose winner is back-facing.
 * Coverage and the counts are integers, a key depends on (face, pixel) alone and a minimum on no order, so every output is
 * bit-identical to the NumPy restatement in tests/raster_ref.py whatever the schedule.
 * The camera is a sfmx_fusion_view: R_rw, c_left, f (> 0), cx, cy, w, h are used, B is ignored.  w <= 4096, w * h <= 2^24. */
#define SFMX_RASTER_MAX_PIXELS (1 << 24) /* w * h */
#define SFMX_RASTER_MAX_VERTS (1 << 24)  /* n < this */
#define SFMX_RASTER_MAX_FACES (1 << 30)  /* m < this */
typedef struct sfmx_raster sfmx_raster;  /* the device outputs of the last run and the work buffers; they grow on demand and are kept */
typedef struct sfmx_raster_params {
  double z_min;       /* a vertex nearer than this drops its faces; finite, > 0; no default */
  int cull;           /* 0 = none (default), 1 = drop back faces, 2 = drop front faces */
  uint8_t background; /* shaded and grey of a pixel without a winner (default 0) */
} sfmx_raster_params;
void sfmx_raster_default_params(sfmx_raster_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_raster_check_params(const sfmx_raster_params* p);
int sfmx_raster_create(sfmx_ctx* ctx, sfmx_raster** out);
void sfmx_raster_destroy(sfmx_ctx* ctx, sfmx_raster* rs);
/* verts double [n][3], normals double [n][3] or NULL, grey u8 [n] or NULL, faces int32 [m][3]; host pointers (copied into the
 * object) or (on_device = 1) device pointers (read in place; they must stay until the call returns); 0 <= n < 2^24,
 * 0 <= m < 2^30.  A face index outside [0, n) is found on the device without any access through it and gives SFMX_ERR_INVALID;
 * the object stays usable.  A failed call leaves no result.  A render that hits nothing (m = 0 included) is not an error.
 * The device meshes of the fusion, clean, fill, smooth and simplify objects are fed from their _device_mesh / _device_surface
 * getters with on_device = 1. */
int sfmx_raster_run(sfmx_ctx* ctx, sfmx_raster* rs, const double* verts, const double* normals, const uint8_t* grey, int n,
                    const int32_t* faces, int m, int on_device, const sfmx_fusion_view* view, const sfmx_raster_params* p);
/* the last run to the host: depth double [h][w], face int32 [h][w], points / normals double [h][w][3], shaded / grey u8 [h][w];
 * any may be NULL.  SFMX_ERR_INVALID before a run, and for grey after a run without grey. */
int sfmx_raster_read(sfmx_ctx* ctx, sfmx_raster* rs, double* depth, int32_t* face, double* points, double* normals, uint8_t* shaded,
                     uint8_t* grey);
/* of the last run: counts8 int32 [8] = faces_behind, faces_outside, faces_degenerate, faces_back, faces_culled, faces_drawn, hits,
 * back_pixels, and *fragments; either may be NULL.  SFMX_ERR_INVALID (and zeros) before a run; needs no context. */
int sfmx_raster_counts(const sfmx_raster* rs, int32_t* counts8, uint64_t* fragments);
/* the points and normals of all w * h pixels of the last run on the device (for sfmx_shade_vertices with on_device = 1);
 * *n = w * h.  SFMX_ERR_INVALID (and NULLs, 0) before a run; needs no context.  Valid until the next run on rs. */
int sfmx_raster_device_surface(const sfmx_raster* rs, const double** points, const double** normals, int* n);
/* device time (us) from the first to the last launch of the last run when timing is on (sfmx_set_timing), else 0 */
double sfmx_raster_last_us(const sfmx_raster* rs);
/* faces of the last run whose box of pixel centres went to the tiled path (a property of the schedule, not of the result) */
int sfmx_raster_last_big_faces(const sfmx_raster* rs);

/* ---- which faces and vertices a set of cameras sees: exact multi-view visibility ----------------------------- */
/* The object holds an ordered list of V >= 0 views, each a sfmx_fusion_view under the z-buffer's camera rules above (B ignored,
 * sizes may differ), and optionally one image u8 [h][w] per view; a run needs an image on every view or on none.
 * Per view k: the key image of the whole mesh at cull = 0 (back faces occlude too), exactly as sfmx_raster_run builds it.
 * Vertex i is visible in view k iff it is inband, its pixel x = (U + 128) >> 8, y = (V + 128) >> 8 lies in the image, and that
 * pixel's key is empty or q2 <= D + depth_tol, with q2 the vertex's depth and D = (double)(float) of the key's high word: one
 * double addition and one comparison, false for a NaN.  vert_views[i] counts such views.
 * Face f in view k, with A the z-buffer's integer area from the snapped corners: seen iff its three vertices are visible and
 * A < 0; seen from behind iff they are and A > 0; neither with A == 0 or a corner that is not visible.  face_views[f] and
 * face_back_views[f] count these views.
 * Face f is kept iff face_views[f] >= min_views (0 keeps everything and only measures).  The output is as sfmx_clean gives it:
 * kept faces in input order, the vertices a kept face uses in ascending input index with their bytes (and their normals')
 * copied, indices renumbered, vert_src and face_src.
 * Grey (only with images), per input vertex: over the views where the vertex is visible and, with cull = 1,
 * ((n0 p0 + n1 p1) + n2 p2) < 0 (p = X - c), acc += image[y][x], cnt += 1; grey = cnt ? (2 acc + cnt) / (2 cnt) : fill,
 * grey_views = cnt.  cull = 1 with images needs normals; without images cull and fill are not used.
 * Counts, int32: faces_seen (face_views >= 1), faces_back_only (face_views == 0 and face_back_views >= 1), faces_unseen (both 0),
 * faces_kept, verts_kept.  uint64, over all (vertex, view) pairs: pairs_visible, pairs_occluded (the depth test failed),
 * pairs_off (not inband, or the pixel outside the image); the three sum to n V.
 * A key is a function of (face, pixel), a minimum has no order, everything after the one depth comparison is an integer and
 * every offset comes from a scan, so every output is bit-identical to the NumPy restatement in tests/visib_ref.py whatever the
 * schedule, the order of the views and their batching. */
typedef struct sfmx_visib sfmx_visib;  /* the views, their images, the work buffers and the last result; they grow and are kept */
typedef struct sfmx_visib_params {
  double z_min;     /* the z-buffer's: a vertex nearer than this is not inband and drops its faces; finite, > 0; no default */
  double depth_tol; /* a vertex this far behind the z-buffer is still visible; finite, >= 0; no default */
  int min_views;    /* a face seen from the front by fewer views is removed; >= 0 (default 1) */
  int cull;         /* grey only: 1 = skip the views a vertex's normal points away from (default), 0 = do not */
  int fill;         /* grey of a vertex no view contributes to, 0 .. 255 (default 0) */
} sfmx_visib_params;
void sfmx_visib_default_params(sfmx_visib_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_visib_check_params(const sfmx_visib_params* p);
int sfmx_visib_create(sfmx_ctx* ctx, sfmx_visib** out);
void sfmx_visib_destroy(sfmx_ctx* ctx, sfmx_visib* vb);
/* drops the views and their images and keeps the memory (and the last result) */
int sfmx_visib_reset(sfmx_ctx* ctx, sfmx_visib* vb);
/* appends a view; image u8 [h][w] or NULL, a host pointer or (on_device = 1) a device pointer, copied into the object */
int sfmx_visib_add_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const uint8_t* image, int on_device);
/* the same with the left rectified image of st's last sfmx_stereo_disparity call, from where it lies on the device; the view's
 * size must be the stereo object's */
int sfmx_visib_add_stereo_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const sfmx_stereo* st);
int sfmx_visib_view_count(const sfmx_visib* vb);
/* the views are processed in batches (at most 64 per launch), sized by a memory budget for the key images and the per-view
 * records; k >= 1 (<= 64) forces k views per batch, 0 restores the automatic size.  The result does not depend on it. */
int sfmx_visib_set_batch(sfmx_visib* vb, int k);
/* verts double [n][3], normals double [n][3] or NULL, faces int32 [m][3]; host pointers (copied into the object) or
 * (on_device = 1) device pointers that are not vb's own result arrays (read in place; they must stay until the call returns);
 * 0 <= n < 2^24, 0 <= m < 2^30.  A face index outside [0, n) is found on the device without any access through it and gives
 * SFMX_ERR_INVALID, as do images on some views only and cull = 1 with images and no normals; the object stays usable and a
 * failed call leaves no result.  V = 0, m = 0, n = 0 and a result with nothing left are not errors. */
int sfmx_visib_run(sfmx_ctx* ctx, sfmx_visib* vb, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_visib_params* p);
/* the last successful run to the host: verts_out / normals_out double [n'][3], faces_out int32 [m'][3], vert_src int32 [n'],
 * face_src int32 [m'], face_views / face_back_views int32 [m], vert_views int32 [n], grey u8 [n], grey_views int32 [n]; any may
 * be NULL.  SFMX_ERR_INVALID before a successful run, for normals_out after a run without normals and for grey / grey_views
 * after a run without images. */
int sfmx_visib_read(sfmx_ctx* ctx, sfmx_visib* vb, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src,
                    int32_t* face_src, int32_t* face_views, int32_t* face_back_views, int32_t* vert_views, uint8_t* grey,
                    int32_t* grey_views);
/* input and output vertices and faces (n, m, n', m') of the last successful run; any pointer may be NULL.  SFMX_ERR_INVALID
 * (and zeros) before a successful run; needs no context. */
int sfmx_visib_sizes(const sfmx_visib* vb, int* n, int* m, int* n_verts_out, int* n_faces_out);
/* of the last successful run: counts5 int32 [5] = faces_seen, faces_back_only, faces_unseen, faces_kept, verts_kept and pairs3
 * uint64 [3] = pairs_visible, pairs_occluded, pairs_off; either may be NULL.  SFMX_ERR_INVALID (and zeros) before one. */
int sfmx_visib_counts(const sfmx_visib* vb, int32_t* counts5, uint64_t* pairs3);
/* the culled mesh on the device, the object's own arrays (for sfmx_raster_run, sfmx_simplify_run, sfmx_shade_vertices and
 * sfmx_sdist_set_target / _query with on_device = 1); any pointer may be NULL.  Returns n', or -1 before a successful run.
 * Valid until the next run on vb. */
int sfmx_visib_device_mesh(const sfmx_visib* vb, const double** verts, const int32_t** faces, int* n_verts, int* n_faces);
/* the culled vertices and their normals (NULL after a run without normals).  Returns n', or -1 before a successful run. */
int sfmx_visib_device_surface(const sfmx_visib* vb, const double** verts, const double** normals);
/* device time (us) from the first to the last launch of the last run when timing is on (sfmx_set_timing), else 0 */
double sfmx_visib_last_us(const sfmx_visib* vb);
/* the largest number of views the last successful run put into one batch (a property of the schedule, not of the result) */
int sfmx_visib_last_batch(const sfmx_visib* vb);

/* ---- a texture atlas from the cameras that see the mesh: best view per face, one patch per face ------------- */
/* The object holds an ordered list of V >= 1 views, each a sfmx_fusion_view under the z-buffer's camera rules above (B ignored,
 * sizes may differ) with an image u8 [h][w]; a run needs an image on every view.
 * Seen: face f is seen by view k exactly as sfmx_visib defines it (its three vertices visible in k, A < 0).
 * Best view: face_view[f] is the seen view with the largest -A (int64), a tie goes to the smallest view index, face_area[f] is
 * that -A; a face no view sees has face_view = -1 and face_area = 0.  view_faces[k] counts the faces of view k.
 * Layout, S = patch, L = S - 2: the textured faces in ascending index get ranks r = 0, 1, ...; rank r uses cell r >> 1, half
 * r & 1.  cells = ceil(n_tex / 2) + (n_un > 0 ? 1 : 0); the extra last cell is the fill cell.  A cell is S + 1 texels wide and S
 * high.  C = cells_per_row, or with 0 the smallest C with C C >= cells, at least 1, at most floor(16384 / (S + 1)).  The atlas is
 * W = C (S + 1) wide and H = ceil(cells / C) S high (W = H = 0 with cells = 0); cell c has its top-left texel at
 * ((c % C) (S + 1), (c / C) S).  W > 16384 or W H > 2^28 is SFMX_ERR_INVALID, decided before the atlas is allocated.
 * Ownership: half 0 owns the local texels (i, j), i, j >= 0, i + j <= S - 1; half 1 owns (S - i, S - 1 - j) for the same (i, j).
 * A texel of the fill cell, of a half without a face and of a cell past the last one is `fill`.
 * Corners, in half-texels relative to the cell: half 0 has a at (1, 1), b at (2 S - 3, 1), c at (1, 2 S - 3); half 1 the half
 * turn (2 (S + 1) - x, 2 S - y).  uv_half int32 [m][3][2] holds them plus twice the cell's origin; an untextured face has all
 * three on the centre of the fill cell, (2 x0 + S + 1, 2 y0 + S).  u = hx / (2 W), v = 1 - hy / (2 H).
 * Texel (i, j) of face (a, b, c) with view k: i' = min(i, L), j' = min(j, L - i') (the texels with i + j = S - 1 repeat the
 * hypotenuse); X_r = (((double)(L - i' - j') Xa_r + (double)i' Xb_r) + (double)j' Xc_r) / (double)L; p = X - c,
 * q_r = (R[r][0] p0 + R[r][1] p1) + R[r][2] p2, u = (f q0) / q2 + cx, v = (f q1) / q2 + cy; `fill` unless q2 > 0 and u, v finite;
 * uc = min(max(u, -1), w), x0 = floor(uc), ax = uc - x0, xi0 = clamp((int)x0, 0, w - 1), xi1 = clamp((int)x0 + 1, 0, w - 1),
 * likewise v and h; top = (1 - ax) I[yi0][xi0] + ax I[yi0][xi1], bot likewise on yi1, g = (1 - ay) top + ay bot;
 * texel = (u8)min(255, floor(g + 0.5)).  A pixel is its centre.  Nothing is contracted.
 * Counts, int32: faces_textured, faces_untextured, cells, W, H, cells_per_row.
 * Every output is bit-identical to the NumPy restatement in tests/texture_ref.py whatever the schedule and the batching. */
typedef struct sfmx_texture sfmx_texture;  /* the views, their images, the work buffers and the last result; they grow and are kept */
typedef struct sfmx_texture_params {
  double z_min;      /* the z-buffer's; finite, > 0; no default */
  double depth_tol;  /* a vertex this far behind the z-buffer is still visible; finite, >= 0; no default */
  int patch;         /* S: a face's patch is S texels along each leg, its cell S + 1 by S; 3 .. 64 (default 8) */
  int cells_per_row; /* C >= 1, or 0 for the automatic value (default) */
  int fill;          /* the texel no face owns, 0 .. 255 (default 0) */
} sfmx_texture_params;
void sfmx_texture_default_params(sfmx_texture_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_texture_check_params(const sfmx_texture_params* p);
int sfmx_texture_create(sfmx_ctx* ctx, sfmx_texture** out);
void sfmx_texture_destroy(sfmx_ctx* ctx, sfmx_texture* tx);
/* drops the views and their images and keeps the memory (and the last result) */
int sfmx_texture_reset(sfmx_ctx* ctx, sfmx_texture* tx);
/* appends a view; image u8 [h][w], a host pointer or (on_device = 1) a device pointer, copied into the object.  NULL is
 * accepted here and refused by the run. */
int sfmx_texture_add_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const uint8_t* image, int on_device);
/* the same with the left rectified image of st's last sfmx_stereo_disparity call, from where it lies on the device */
int sfmx_texture_add_stereo_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const sfmx_stereo* st);
int sfmx_texture_view_count(const sfmx_texture* tx);
/* as sfmx_visib_set_batch: k >= 1 (<= 64) forces k views per batch, 0 restores the automatic size; the result does not depend
 * on it */
int sfmx_texture_set_batch(sfmx_texture* tx, int k);
/* verts double [n][3], faces int32 [m][3]; host pointers (copied into the object) or (on_device = 1) device pointers (read in
 * place; they must stay until the call returns); 0 <= n < 2^24, 0 <= m < 2^30.  SFMX_ERR_INVALID for a face index outside
 * [0, n) (found on the device without any access through it), no views, a view without an image, parameters outside their
 * range and an atlas that is too wide or too large; the object stays usable and a failed call leaves no result.  m = 0 (an
 * atlas of 0 x 0) and a mesh no view sees (the fill cell alone) are not errors. */
int sfmx_texture_run(sfmx_ctx* ctx, sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m, int on_device,
                     const sfmx_texture_params* p);
/* the last successful run to the host: atlas u8 [H][W], face_view int32 [m], face_area int64 [m], uv_half int32 [m][3][2],
 * view_faces int32 [V]; any may be NULL.  SFMX_ERR_INVALID before a successful run. */
int sfmx_texture_read(sfmx_ctx* ctx, sfmx_texture* tx, uint8_t* atlas, int32_t* face_view, int64_t* face_area, int32_t* uv_half,
                      int32_t* view_faces);
/* n, m, V, W and H of the last successful run; any pointer may be NULL.  SFMX_ERR_INVALID (and zeros) before one. */
int sfmx_texture_sizes(const sfmx_texture* tx, int* n, int* m, int* n_views, int* W, int* H);
/* counts6 int32 [6] = faces_textured, faces_untextured, cells, W, H, cells_per_row.  SFMX_ERR_INVALID (and zeros) before a
 * successful run. */
int sfmx_texture_counts(const sfmx_texture* tx, int32_t* counts6);
/* the atlas on the device, the object's own array; any pointer may be NULL.  Returns W H, or -1 before a successful run.  Valid
 * until the next run on tx. */
int sfmx_texture_device_atlas(const sfmx_texture* tx, const uint8_t** atlas, int* W, int* H);
/* device time (us) from the first to the last launch of the last run, and of the bake kernel alone, when timing is on
 * (sfmx_set_timing), else 0 */
double sfmx_texture_last_us(const sfmx_texture* tx);
double sfmx_texture_last_bake_us(const sfmx_texture* tx);
/* the largest number of views the last successful run put into one batch (a property of the schedule, not of the result) */
int sfmx_texture_last_batch(const sfmx_texture* tx);

/* ---- levelling the seams of a texture atlas: exact per-view vertex offsets ---------------------------------- */
/* Inputs: a mesh and a sfmx_texture tx whose last successful sfmx_texture_run was on this mesh; that run supplies face_view, the
 * layout (S = patch, L = S - 2, C, W, H, cells), fill, the views and their images (do not change tx's views in between).
 * All integer divisions are floor divisions.
 * Nodes: every corner (f, c) of a textured face (k = face_view[f] >= 0) with vertex v belongs to node (v, k); nodes are the
 * distinct pairs.  Node sample: graw is the texture's bilinear g (not rounded) in view k at X_r = ((double)L verts[v][r]) /
 * (double)L, the point of v's corner texel; fx = (int64)floor(graw 256.0 + 0.5), or 256 fill where the texel would be `fill`.
 * Seam vertices: vertex_views[v] counts the distinct views among v's nodes; v is a seam vertex when it is >= 2, and then
 * target[v] = (2 sum_k fx(v, k) + c) / (2 c), c = vertex_views[v].  The nodes of a seam vertex are pinned with g = target - fx;
 * every other node is free and starts at 0.  Neighbours: N(v, k) are the distinct nodes (w, k), w != v, for which a face of
 * view k has v and w as corners; deg = |N|.  Sweeps (Jacobi), t = 0 .. iterations - 1: every free node gets
 * g' = (2 sum_N g + deg) / (2 deg), all reads from the values before the sweep; pinned nodes keep theirs.
 * corner_adj[f][c] = g(node), corner_sample[f][c] = fx(node), both 0 on an untextured face.
 * Atlas: tx's layout, ownership and fill texels; texel (i, j) of a textured face: i', j', validity and g as the texture's,
 * N = (L - i' - j') ga + i' gb + j' gc (int64; ga, gb, gc the face's corner_adj),
 * texel = (u8)min(255, max(0, floor((g + (double)N / (double)(256 L)) + 0.5))).  Nothing is contracted.
 * Counts, int32: nodes, seam_vertices, pinned_nodes, free_nodes, node_edges (undirected, distinct), iterations.
 * Every output is bit-identical to the NumPy restatement in tests/level_ref.py whatever the schedule. */
typedef struct sfmx_level sfmx_level;  /* the work buffers and the last result; they grow and are kept */
typedef struct sfmx_level_params {
  int iterations; /* T: Jacobi sweeps, 0 .. 65536 (default 64) */
} sfmx_level_params;
void sfmx_level_default_params(sfmx_level_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_level_check_params(const sfmx_level_params* p);
int sfmx_level_create(sfmx_ctx* ctx, sfmx_level** out);
void sfmx_level_destroy(sfmx_ctx* ctx, sfmx_level* lv);
/* verts double [n][3], faces int32 [m][3]: host pointers (copied into the object) or (on_device = 1) device pointers (read in
 * place; they must stay until the call returns).  SFMX_ERR_INVALID for a tx without a successful run, n or m other than that
 * run's, a face index outside [0, n) (found on the device without any access through it), 3 m > 2^31 - 1 (decided before any
 * allocation) and parameters outside their range; the object stays usable and a failed call leaves no result.  m = 0 and a mesh
 * without a textured face are not errors.  tx and its atlas are not modified. */
int sfmx_level_run(sfmx_ctx* ctx, sfmx_level* lv, const sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_level_params* p);
/* the last successful run to the host: atlas u8 [H][W], corner_adj int32 [m][3], corner_sample int32 [m][3], vertex_views
 * int32 [n]; any may be NULL.  SFMX_ERR_INVALID before a successful run. */
int sfmx_level_read(sfmx_ctx* ctx, sfmx_level* lv, uint8_t* atlas, int32_t* corner_adj, int32_t* corner_sample, int32_t* vertex_views);
/* counts6 int32 [6] = nodes, seam_vertices, pinned_nodes, free_nodes, node_edges, iterations.  SFMX_ERR_INVALID (and zeros)
 * before a successful run. */
int sfmx_level_counts(const sfmx_level* lv, int32_t* counts6);
/* the levelled atlas on the device, the object's own array; any pointer may be NULL.  Returns W H, or -1 before a successful
 * run.  Valid until the next run on lv. */
int sfmx_level_device_atlas(const sfmx_level* lv, const uint8_t** atlas, int* W, int* H);
/* device time (us) from the first to the last launch of the last run, of the sweeps alone and of the bake kernel alone, when
 * timing is on (sfmx_set_timing), else 0 */
double sfmx_level_last_us(const sfmx_level* lv);
double sfmx_level_last_sweeps_us(const sfmx_level* lv);
double sfmx_level_last_bake_us(const sfmx_level* lv);

/* ---- the textured mesh rendered back into the cameras: exact photometric error ------------------------------- */
/* The object holds an ordered list of Q >= 0 views, each a sfmx_fusion_view under the z-buffer's camera rules above (B ignored,
 * sizes may differ), optionally an image u8 [h][w], and an int tex_view: the index of this camera in the texture object's view
 * list, or -1 when it is not one of them (a held-out or novel camera).  View q's pixels start at off_q = sum_{p < q} w_p h_p in
 * every per-pixel output.
 * Inputs of a run: a mesh; a sfmx_texture tx whose last successful sfmx_texture_run was on this mesh (it supplies face_view,
 * uv_half, W, H and fill); optionally a sfmx_level lv whose last successful run was on tx: then the atlas A is the levelled one,
 * otherwise tx's; z_min and background.
 * Per view q: the key image of the whole mesh at cull = 0, exactly as sfmx_raster_run builds it.
 * Per pixel (x, y) of view q.  No winner: cls = 0, face = -1, rendered = background.  Otherwise f is the winner, with e0, e1, e2,
 * r_i, t_i = (double)e_i r_i and s = ((double)e0 r0 + (double)e1 r1) + (double)e2 r2 exactly as in the renderer (s > 0 for a
 * fragment, so everything below is finite).  A_f > 0 (back-facing): cls = 1, rendered = background.  Else k = face_view[f] < 0:
 * cls = 2, rendered = fill.  Else cls = 3 if k == tex_view[q], otherwise cls = 4, and with h_i = uv_half[f][i] (int32, as doubles)
 *   hx = ((t0 h0x + t1 h1x) + t2 h2x) / s;  hy likewise
 *   a = hx * 0.5 - 0.5;  ac = min(max(a, 0.0), (double)(W - 1));  x0 = floor(ac);  fx = ac - x0
 *   xi0 = (int)x0;  xi1 = min(xi0 + 1, W - 1);  the same with hy and H: yi0, yi1, fy
 *   top = (1.0 - fx) A[yi0][xi0] + fx A[yi0][xi1];  bot = (1.0 - fx) A[yi1][xi0] + fx A[yi1][xi1]
 *   g = (1.0 - fy) top + fy bot;  rendered = (u8)min(255.0, floor(g + 0.5)).
 * Nothing is contracted.
 * Error (views with an image only): per pixel of class 3 or 4, d = |rendered - I_q[y][x]|, an integer 0 .. 255.
 * Results.  Per pixel: rendered u8, cls u8, face int32.  Per view: classes int64 [Q][5], the pixels of each class; stats int64
 * [Q][2][3], for own (class 3) and cross (class 4) the count, the sum of d and the sum of d d; hist int64 [Q][2][256], the
 * histogram of d.  A view without an image has zero stats and hist.
 * The keys are the renderer's, a pixel's values are a fixed double sequence on (face, pixel) alone, written by exactly one thread,
 * and all sums are integer adds, so every byte equals the NumPy restatement in tests/photo_ref.py whatever the schedule, the batch
 * size and the order of the views. */
typedef struct sfmx_photo sfmx_photo;  /* the views, their images, the work buffers and the last result; they grow and are kept */
typedef struct sfmx_photo_params {
  double z_min;       /* the z-buffer's; finite, > 0; no default */
  uint8_t background; /* rendered of a pixel without a winner or with a back-facing one (default 0) */
} sfmx_photo_params;
void sfmx_photo_default_params(sfmx_photo_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_photo_check_params(const sfmx_photo_params* p);
int sfmx_photo_create(sfmx_ctx* ctx, sfmx_photo** out);
void sfmx_photo_destroy(sfmx_ctx* ctx, sfmx_photo* ph);
/* drops the views and their images and keeps the memory (and the last result) */
int sfmx_photo_reset(sfmx_ctx* ctx, sfmx_photo* ph);
/* appends a view; image u8 [h][w] or NULL, a host pointer or (on_device = 1) a device pointer, copied into the object;
 * tex_view >= -1 (its upper end is checked by the run, which knows the texture object) */
int sfmx_photo_add_view(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_fusion_view* view, const uint8_t* image, int on_device, int tex_view);
/* appends all of tx's views with their images, device to device, view k with tex_view = k */
int sfmx_photo_add_texture_views(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_texture* tx);
int sfmx_photo_view_count(const sfmx_photo* ph);
/* as sfmx_visib_set_batch: k >= 1 (<= 64) forces k views per batch, 0 restores the automatic size; the result does not depend
 * on it */
int sfmx_photo_set_batch(sfmx_photo* ph, int k);
/* verts double [n][3], faces int32 [m][3]: host pointers (copied into the object) or (on_device = 1) device pointers (read in
 * place; they must stay until the call returns); lv may be NULL.  SFMX_ERR_INVALID for a tx without a successful run, n or m
 * other than that run's, an lv without a successful run or with another W or H, a tex_view outside [-1, V), a face index outside
 * [0, n) (found on the device without any access through it), views of more than 2^28 pixels in all (decided before any
 * allocation) and parameters outside their range; the object stays usable and a failed call leaves no result.  Q = 0, m = 0 and
 * a view that hits nothing are not errors.  tx and lv are not modified. */
int sfmx_photo_run(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_texture* tx, const sfmx_level* lv, const double* verts, int n,
                   const int32_t* faces, int m, int on_device, const sfmx_photo_params* p);
/* the last successful run to the host: rendered u8, cls u8, face int32 [sum w h], classes int64 [Q][5], stats int64 [Q][2][3],
 * hist int64 [Q][2][256]; any may be NULL.  SFMX_ERR_INVALID before a successful run. */
int sfmx_photo_read(sfmx_ctx* ctx, sfmx_photo* ph, uint8_t* rendered, uint8_t* cls, int32_t* face, int64_t* classes, int64_t* stats,
                    int64_t* hist);
/* Q and the sum of w h of the last successful run; either may be NULL.  SFMX_ERR_INVALID (and zeros) before one. */
int sfmx_photo_sizes(const sfmx_photo* ph, int* n_views, int* pixels);
/* the rendered pixels on the device, the object's own array (view q at off_q); returns the sum of w h, or -1 before a
 * successful run.  Valid until the next run on ph. */
int sfmx_photo_device_rendered(const sfmx_photo* ph, const uint8_t** rendered);
/* device time (us) from the first to the last launch of the last run, and of the k_ph_resolve launches alone, when timing is on
 * (sfmx_set_timing), else 0 */
double sfmx_photo_last_us(const sfmx_photo* ph);
double sfmx_photo_last_resolve_us(const sfmx_photo* ph);
/* the largest number of views the last successful run put into one batch (a property of the schedule, not of the result) */
int sfmx_photo_last_batch(const sfmx_photo* ph);

/* ---- registering a camera to the textured mesh: direct photometric alignment -------------------------------- */
/* Inputs: a mesh, a sfmx_texture tx whose last successful run was on it, optionally a sfmx_level lv run on tx (then its atlas is
 * read, as in the photometric error above), one picture I u8 [h][w], a camera (a sfmx_fusion_view under the z-buffer's camera
 * rules, w and h the picture's) and the parameters.  Everything is IEEE double in the written order, nothing is contracted, and
 * sqrt is taken on the host only.
 *   render:     the key image of the whole mesh at cull = 0 for the current view, as sfmx_photo_run builds it
 *   ok(x, y):   there is a winner f, f is front-facing and face_view[f] >= 0 (classes 3 and 4 above); outside the image: not ok
 *   samples:    x = stride*i, y = stride*j with x < w, y < h;  nsx = ceil(w/stride), nsy = ceil(h/stride)
 *   candidate:  ok(x', y') for every integer |x' - x| <= margin, |y' - y| <= margin
 *   per candidate, with f, e_i, r_i, t_i, s of the photometric error at (x, y):
 *     g   = that definition's g (the bilinear atlas read before its rounding)
 *     z   = (double)|A_f| / s
 *     r   = (double)I[y][x] - g;  used iff fabs(r) <= r_max (a NaN is not)
 *     Gx  = 0.5*((double)I[y][x+1] - (double)I[y][x-1]);  Gy = 0.5*((double)I[y+1][x] - (double)I[y-1][x])
 *     dx  = ((double)x - cx)/f;  dy = ((double)y - cy)/f;  q = (dx*z, dy*z, z);  iz = 1.0/z
 *     a0  = (Gx*f)*iz;  a1 = (Gy*f)*iz;  a2 = -((a0*dx) + (a1*dy))
 *     gw_b = (a0*R[0][b] + a1*R[1][b]) + a2*R[2][b]                  R = R_rw, its rows are the camera's axes
 *     X_b  = c_b + ((R[0][b]*q0 + R[1][b]*q1) + R[2][b]*q2);  Q = X - pivot
 *     J = (Q2*gw1 - Q1*gw2,  Q0*gw2 - Q2*gw0,  Q1*gw0 - Q0*gw1,  -gw0,  -gw1,  -gw2)
 *   terms (28, the view alignment's order): A_mn = J_m*J_n for m <= n row by row (21), b_m = J_m*r (6), e = r*r (1); a sample
 *     that is not used adds +0.0 to all 28; n = the used samples
 *   ordered sum, solve, update, loop: the view alignment's, with p = pivot.  n < min_pixels: TOO_FEW.  A refused
 *     Cholesky pivot, or a view with a non-finite entry after the update: DEGENERATE.  CONVERGED when, after the update,
 *     |omega| <= eps_rot and |v| <= eps_trans.  TOO_FEW / DEGENERATE return the last view whose evaluation gave a step.
 * The mesh is rendered again at every evaluation; the picture is read at integer positions only.  The gradient is the central
 * difference (a forward difference shares the rounding error of I[y][x] with r and biases b), and margin >= 1 keeps its taps
 * inside the image.  Sums, n and every iterate are bit-identical to the NumPy restatement in tests/palign_ref.py. */
#define SFMX_PALIGN_ITERS_CAP 64 /* max_iters, and the length of the trace */
#define SFMX_PALIGN_MARGIN_CAP 64
enum { SFMX_PALIGN_CONVERGED = 0, SFMX_PALIGN_MAX_ITERS = 1, SFMX_PALIGN_TOO_FEW = 2, SFMX_PALIGN_DEGENERATE = 3 };
typedef struct sfmx_palign sfmx_palign;  /* the model, the picture and the work buffers; they grow on demand and are kept */
typedef struct sfmx_palign_params {
  double z_min;     /* the z-buffer's; finite, > 0; no default */
  double pivot[3];  /* the rotation's fixed point; finite; no default */
  int max_iters;    /* evaluations at most, 1 .. 64 (default 10) */
  int stride;       /* every stride-th pixel of every stride-th row is a sample, >= 1 (default 1) */
  int margin;       /* a sample needs ok pixels this far around it, 1 .. 64 (default 4) */
  int min_pixels;   /* fewer used samples than this end the loop with TOO_FEW, >= 1 (default 64) */
  double r_max;     /* a candidate with |r| above this is not used; finite, >= 0 (default 255) */
  double damping;   /* added to the diagonal of A, >= 0 (default 0) */
  double eps_rot;   /* converged when |omega| <= eps_rot (default 5e-5) ... */
  double eps_trans; /* ... and |v| <= eps_trans, a length in the mesh's units (default 1e-6) */
} sfmx_palign_params;
typedef struct sfmx_palign_result {
  sfmx_fusion_view view; /* the refined view: R_rw and c_left move, the rest is the input's */
  int status;            /* SFMX_PALIGN_CONVERGED, _MAX_ITERS, _TOO_FEW or _DEGENERATE */
  int iterations;        /* evaluations made */
  int32_t n[SFMX_PALIGN_ITERS_CAP];    /* per evaluation: samples used ... */
  double e[SFMX_PALIGN_ITERS_CAP];     /* ... sum r^2 ... */
  double rot[SFMX_PALIGN_ITERS_CAP];   /* ... |omega| of the step taken (0 when none was) ... */
  double trans[SFMX_PALIGN_ITERS_CAP]; /* ... and |v| */
} sfmx_palign_result;
void sfmx_palign_default_params(sfmx_palign_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_palign_check_params(const sfmx_palign_params* p);
int sfmx_palign_create(sfmx_ctx* ctx, sfmx_palign** out);
void sfmx_palign_destroy(sfmx_ctx* ctx, sfmx_palign* pa);
/* the model: tx (and lv, or NULL) are kept by reference and must outlive their use here, unchanged; verts double [n][3] and
 * faces int32 [m][3] are copied into the object, from host pointers or (on_device = 1) device pointers.  SFMX_ERR_INVALID for a
 * tx without a successful run, n or m other than that run's, an lv without a run or with another W or H, and a face index
 * outside [0, n) (found on the device without any access through it); the model set before stays. */
int sfmx_palign_set_model(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_texture* tx, const sfmx_level* lv, const double* verts, int n,
                          const int32_t* faces, int m, int on_device);
/* the same from a texture result on the host (sfmx_texture_read's arrays, the atlas tx's or a levelled one): face_view int32 [m],
 * uv_half int32 [m][3][2], atlas u8 [H][W], all host pointers, copied; the object then refers to no texture object.  A textured
 * face needs W, H >= 1; the atlas is read with the clamps of the definition whatever uv_half holds. */
int sfmx_palign_set_model_arrays(sfmx_ctx* ctx, sfmx_palign* pa, const int32_t* face_view, const int32_t* uv_half, const uint8_t* atlas, int W,
                                 int H, const double* verts, int n, const int32_t* faces, int m);
/* the picture u8 [h][w], copied into the object from a host pointer or (on_device = 1) a device pointer; w <= 4096 and
 * w h <= the z-buffer's limit */
int sfmx_palign_set_image(sfmx_ctx* ctx, sfmx_palign* pa, const uint8_t* image, int w, int h, int on_device);
/* one evaluation at the given view, no step: sums double [28] (A row by row upper, b, e) and *n.  SFMX_ERR_INVALID before a
 * successful set_model and set_image, for a view whose w, h are not the picture's, that the z-buffer or sfmx_view_ok refuses,
 * and for parameters outside their range; the object stays usable, and the model and picture stay set. */
int sfmx_palign_system(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_fusion_view* view, const sfmx_palign_params* p, double* sums,
                       int32_t* n);
/* the Gauss-Newton loop from the given view.  The statuses are results: the call returns SFMX_OK with them.  A view that sees
 * nothing is TOO_FEW. */
int sfmx_palign_view(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_fusion_view* view, const sfmx_palign_params* p,
                     sfmx_palign_result* out);
/* the last evaluation, nsy x nsx values each: state u8 (0 not a candidate, 1 trimmed by r_max, 2 used) and r double (0.0 where
 * the state is 0); either may be NULL.  SFMX_ERR_INVALID before a successful evaluation. */
int sfmx_palign_read(sfmx_ctx* ctx, sfmx_palign* pa, uint8_t* state, double* r);
/* nsx and nsy of the last evaluation; SFMX_ERR_INVALID (and zeros) before one */
int sfmx_palign_sizes(const sfmx_palign* pa, int* nsx, int* nsy);
/* device time (us) of the evaluations of the last call, of their z-buffers alone, and of k_pa_system with the tree's levels
 * alone (the rest is the mask and its erosion), when timing is on (sfmx_set_timing), else 0 */
double sfmx_palign_last_us(const sfmx_palign* pa);
double sfmx_palign_last_zbuffer_us(const sfmx_palign* pa);
double sfmx_palign_last_system_us(const sfmx_palign* pa);

/* ---- shape from silhouette: the visual hull on the fusion grid, and carving a volume with it --------------- */
/* A carve object keeps an ordered list of views: a sfmx_fusion_view (B is unused, f > 0) and the signed squared distance map of
 * its silhouette.  For a picture I u8 [h][w] and a threshold, m = I >= threshold is the inside class, D2 the squared distance to
 * the nearest pixel OF THE IMAGE of the other class, capped at cap * cap, and sd2 = m ? -D2 : +D2 (int16, never 0): the exact
 * truncated Euclidean distance transform.  sfmx_carve_run gives every grid point of a volume the largest, over the views that
 * see it, of clamp((d * q2) / (f * trunc), -1, 1) with d = +-(sqrt(|sd2|) - 0.5) pixels at the point's nearest pixel and q2 its
 * depth: negative inside every silhouette, positive where some camera sees the point outside its own (the sign convention of
 * DESIGN.md 13).  The maps are integers and the views are combined by max, so maps, hull, view counts, the carved volume and the
 * counters are bit-identical to the NumPy restatement in tests/carve_ref.py whatever the batching or the order of the views. */
typedef struct sfmx_carve sfmx_carve;  /* retained views (camera and sd2 map) and the hull of the last run, on the device */
enum { SFMX_CARVE_INTERSECT = 0, SFMX_CARVE_CLEAR = 1 };
typedef struct sfmx_carve_params {
  int cap;        /* the distance maps' cap in pixels, 1 .. 64 (default 16); the run's must be the one its views were built with */
  int min_views;  /* a grid point's hull value is defined when at least this many views see it; >= 1 (default 1) */
  double margin;  /* sfmx_carve_apply carves where hull > margin; finite, >= 0, < 1 (default 0.5) */
  int mode;       /* sfmx_carve_apply: SFMX_CARVE_INTERSECT (default) or SFMX_CARVE_CLEAR */
  double trunc;   /* the length a hull value of 1 stands for, >= 0 (default 0 = 4 * voxel, as the fusion resolves it) */
} sfmx_carve_params;
/* the grid of a run: point (i, j, k) at origin + (i, j, k) * voxel, with sfmx_fusion_params' limits */
typedef struct sfmx_carve_volume {
  double origin[3];
  double voxel;
  int nx, ny, nz;
} sfmx_carve_volume;
void sfmx_carve_default_params(sfmx_carve_params* p);
/* SFMX_OK or SFMX_ERR_INVALID; needs no device */
int sfmx_carve_check_params(const sfmx_carve_params* p);
int sfmx_carve_create(sfmx_ctx* ctx, sfmx_carve** out);
void sfmx_carve_destroy(sfmx_ctx* ctx, sfmx_carve* cv);
/* drop every view and the result (the device memory is kept for the next ones) */
int sfmx_carve_reset(sfmx_ctx* ctx, sfmx_carve* cv);
/* append a view: image u8 [h][w], a host pointer or (on_device = 1) a device pointer; its sd2 map at threshold (1 .. 255) and
 * cap (1 .. 64) is built and kept (2 bytes per pixel), the picture is not.  Views of different sizes may be mixed (w <= 4096,
 * w * h < 2^30, as every stage's views).  SFMX_ERR_INVALID for f <= 0 and for anything the other stages' views refuse. */
int sfmx_carve_add_view(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_fusion_view* view, const uint8_t* image, int on_device, int threshold,
                        int cap);
/* the same with the left rectified image of st's last sfmx_stereo_disparity / sfmx_stereo_rectify call, from where it lies on
 * the device (a rectified picture is 0 where its source has no pixel) */
int sfmx_carve_add_stereo_view(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_fusion_view* view, const sfmx_stereo* st, int threshold, int cap);
int sfmx_carve_view_count(const sfmx_carve* cv);
/* out int32 [view count]: the pixels of each view's inside class (counted on the device when the view was added) */
int sfmx_carve_inside_pixels(const sfmx_carve* cv, int32_t* out);
/* view i's map to the host: sd2_out int16 [h][w] */
int sfmx_carve_read_view(sfmx_ctx* ctx, sfmx_carve* cv, int i, int16_t* sd2_out);
/* views per launch of the hull kernel, 1 .. 4096; 0 (default) = automatic.  Changes the speed only. */
int sfmx_carve_set_batch(sfmx_carve* cv, int k);
/* the hull of every view on vol.  SFMX_ERR_INVALID without a view, with a view built at another cap, a volume outside the
 * fusion's limits or parameters outside their range; a failed run leaves no result. */
int sfmx_carve_run(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_carve_volume* vol, const sfmx_carve_params* p);
/* the last run to the host: hull double / views int32 [nz][ny][nx] (the views that saw the point; hull is -1 where none did);
 * either may be NULL.  SFMX_ERR_INVALID before a successful run. */
int sfmx_carve_read(sfmx_ctx* ctx, sfmx_carve* cv, double* hull, int32_t* views);
/* carve fu's volume (its pending views are integrated first) with the last run, whose grid must be fu's.  With
 * W = max(1, fu's min_weight), at every defined point with hull > margin, hm = hull - margin: CLEAR makes the point undefined
 * (count 0, sum +0); INTERSECT gives an undefined point, or a point whose value sum / count is below hm, the value hm (count
 * W, sum hm * W).  Every other point keeps its bits.  counts int32 [3] (or NULL): the defined points, those outside (hull >
 * margin) and those whose sum or count changed.  Of p only margin and mode are read.  A refused call (no run, another grid, bad parameters)
 * leaves fu as it was: its pending views stay pending and its cached surface stays. */
int sfmx_carve_apply(sfmx_ctx* ctx, sfmx_carve* cv, sfmx_fusion* fu, const sfmx_carve_params* p, int32_t* counts);
/* counts int32 [3]: the defined points and those outside (hull > p->margin) of the last run, from the hull alone, and 0: what
 * sfmx_carve_apply would return as its first two counters, without a fusion object */
int sfmx_carve_count(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_carve_params* p, int32_t* counts);
/* write the last run into fu (same grid; pending views are integrated first, then every point is overwritten): count W and sum
 * hull * W where defined, count 0 and sum +0 elsewhere.  The extraction and every stage behind it then work on the hull. */
int sfmx_carve_store(sfmx_ctx* ctx, sfmx_carve* cv, sfmx_fusion* fu);
/* device time (us) of the kernels of the last sfmx_carve_run / _apply / _store, and of the two distance transform kernels of
 * the last sfmx_carve_add_view, when timing is on (sfmx_set_timing), else 0 */
double sfmx_carve_last_us(const sfmx_carve* cv);
double sfmx_carve_last_edt_us(const sfmx_carve* cv);

/* ---- self-check hooks used by the parity tests (device arithmetic vs the host libm) ---------- */
int sfmx_debug_hypot(sfmx_ctx* ctx, const double* x, const double* y, int n, double* out);
int sfmx_debug_divsqrt(sfmx_ctx* ctx, const double* x, const double* y, int n, double* div_out,
                       double* sqrt_out);

#ifdef __cplusplus
}
#endif
#endif /* SFMX_H */
