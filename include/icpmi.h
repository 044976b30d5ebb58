/*
 * icpmi.h — C ABI of libicpmi.so: the MI355X (gfx950) implementation of the
 * per-scan hot path of DUBSON0/iterative-closest-point-avmi.
 *
 * The reference has no FFI layer: its boundary is the Python module surface of
 * utilities/icp.py and utilities/mapping.py.  Each entry point below names the
 * reference function (file:line under /root/reference) it replaces; the Python
 * modules in iterative-closest-point-avmi_amd/utilities/ bind these with ctypes
 * and keep the reference signatures.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (e.g. torch.Tensor.data_ptr()) unless the
 *    parameter name ends in _host.  No device memory is allocated, freed or
 *    retained by the library; scratch memory is passed in as a workspace.
 *  - Process-wide state, all of it listed under "library state" below: the
 *    ICPMI_* option switches (read from the environment once, at first use) and
 *    up to three side streams per device that launchers use to overlap the
 *    independent launches of one call (made on first use, destroyed by
 *    icpmi_shutdown).  Calls may come from several host threads.  Every caller
 *    stream of a device shares these side streams and their events: a launcher
 *    holds one lock over its fork / launch / join sequence, so calls from
 *    different streams never interleave their event records; their side work
 *    runs one after the other on the side stream, and a caller's stream waits
 *    for the side stream up to its own launch, never for a later caller's.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*).
 *  - Return value: ICPMI_OK (0) or a negative ICPMI_ERR_* code; no exceptions
 *    cross the boundary.  Launch-time HIP errors are reported as ICPMI_ERR_HIP.
 *  - Point clouds are row-major float64 (n, dim), dim = 2 or 3, like the
 *    reference's NumPy arrays.  A *cloud set* is several clouds packed in one
 *    buffer: `off[c]` is the first row of cloud c (C+1 entries, capacity based),
 *    `cnt[c]` the number of valid rows (device side, so that voxel filtering,
 *    normals and ICP chain without a host round trip).  cnt == NULL means full
 *    capacity (off[c+1]-off[c]).
 *
 * The shape of the declarations
 *  The Python binding is not written beside this file, it is read from it (icpmi/_header.py, at import): the constants,
 *  the struct classes and the restype / argtypes of every entry.  So the declarations keep a shape a small reader can
 *  follow, and the reader refuses the file when a line falls outside it:
 *  - one `#define ICPMI_<NAME> <integer>` per line, the integer decimal or hex, bare or in parentheses — no expressions;
 *  - a prototype starts in column 0, `<type> icpmi_<name>(<type> <name>, ...);` over any number of lines, `(void)` for
 *    no parameters; types are the <stdint.h> names, int, size_t, float, double, and pointers to those, to void, to char
 *    and to a struct declared above;
 *  - a struct is `typedef struct icpmi_x { ... } icpmi_x;`, its fields of the same types, declared before its first use.
 *  Comments may hold anything.  Nothing else stands outside them but the include guard, the two includes and the
 *  extern "C" guard.
 */
#ifndef ICPMI_H
#define ICPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPMI_OK 0
#define ICPMI_ERR_ARG (-1)        /* bad argument (dim, sizes, null pointer)      */
#define ICPMI_ERR_WORKSPACE (-2)  /* workspace too small                          */
#define ICPMI_ERR_HIP (-3)        /* HIP runtime error at launch                  */
#define ICPMI_ERR_UNSUPPORTED (-4)

/* ICP method, reference utilities/icp.py:133 `method=` */
#define ICPMI_POINT_TO_POINT 0
#define ICPMI_POINT_TO_LINE 1

/* per-pair termination status (slot ICPMI_RES_STATUS of a result record) */
#define ICPMI_ST_CONVERGED 1      /* icp.py:216-219                               */
#define ICPMI_ST_MAXITER 2        /* icp.py:222-223                               */
#define ICPMI_ST_FEW_INLIERS 3    /* icp.py:186-187 `break`                       */
#define ICPMI_ST_EMPTY 4          /* a cloud of the pair is empty after filtering */
#define ICPMI_ST_SKIPPED 5        /* icpmi_icp_batch_gated: a candidate after the first accepted one was left unfinished */

/* One ICP result = 16 float64: R row-major in [0, dim*dim), t in [9, 9+dim),
 * then error, last |prev_error - error|, iterations executed, status.
 * All-double so that one RCCL all_gather moves a batch of results. */
#define ICPMI_RES_DOUBLES 16
#define ICPMI_RES_R 0
#define ICPMI_RES_T 9
#define ICPMI_RES_ERR 12
#define ICPMI_RES_DELTA 13
#define ICPMI_RES_ITERS 14
#define ICPMI_RES_STATUS 15

typedef struct icpmi_icp_params {
    double error_threshold;   /* icp.py:132 */
    double max_corr_dist;     /* icp.py:134; < 0 means None */
    int32_t max_iterations;   /* icp.py:132 */
    int32_t method;           /* ICPMI_POINT_TO_POINT / ICPMI_POINT_TO_LINE */
    int32_t has_init;         /* 1: R_init AND t_init given (icp.py:153) */
    int32_t dim;              /* 2 or 3 */
} icpmi_icp_params;

const char* icpmi_version(void);
const char* icpmi_strerror(int code);

/* ---- library state --------------------------------------------------------
 * Options are experiment / test switches (none is needed in production); each is
 * read from the environment variable ICPMI_<NAME> ONCE, when the library first
 * looks at an option, and icpmi_set_option overrides it afterwards (value NULL
 * unsets).  Names (with or without the ICPMI_ prefix): ICP2_SIDE (0: no side
 * streams), ICP2_STAGES (1: one launch, 2: two stages also for
 * point_to_point), ICP2_FAR (mean squared error in m^2 of a pair's first step
 * above which it finishes on the kernel for far queries; default 1, 0: never),
 * POLAR (0 never / 2 always the bearing order), PREP_KNN
 * (grid | sweep), RAYCAST (atomic | tiles | owner: the pass of the occupancy
 * update), RS_BATCH (full: the batched rotation search scores every angle;
 * projection: no bearing order).
 * Unknown names: ICPMI_ERR_ARG.  Must not race with running calls.
 * icpmi_shutdown synchronises and destroys the side streams and events the
 * library made (they are made again on demand); call it before unloading. */
int icpmi_set_option(const char* name, const char* value);
int icpmi_shutdown(void);
/* One HIP runtime per process: the streams and device pointers a caller hands over must belong to the runtime the
 * library's launches go through.  A process that maps TWO copies of libamdhip64 (this library's /opt/rocm one, loaded
 * first, and the copy PyTorch bundles, loaded later — or the other way round without the loader finding the first)
 * fails every launch with ICPMI_ERR_HIP and nothing to tell why.  icpmi_runtime_check walks the loaded objects
 * (dl_iterate_phdr): ICPMI_OK when at most one libamdhip64 is mapped, else ICPMI_ERR_HIP with the paths written to
 * msg (NUL-terminated, at most msg_bytes; msg may be NULL).  The reference has no counterpart (pure Python); the
 * Python host layer (icpmi/_lib.py) calls it right after loading the library and whenever a call returns ICPMI_ERR_HIP. */
int icpmi_runtime_check(char* msg, size_t msg_bytes);

/* ---- voxel_downsample, utilities/icp.py:117-129 --------------------------
 * For every cloud c: keys floor((p - min_c) / voxel) per axis, lexicographic
 * unique, per-voxel mean with the sum taken in input order.  out_pts uses the
 * same offsets as the input; out_cnt[c] = number of voxels (or -1 if the key
 * range overflows 64 bits).  off_host mirrors off_dev (the launcher routes
 * clouds larger than 8192 points to the multi-kernel path). */
size_t icpmi_voxel_workspace_bytes(int32_t max_n);
int icpmi_voxel_downsample_batch(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                                 int32_t n_clouds, int32_t dim, double voxel_size,
                                 double* out_pts, int32_t* out_cnt,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- nearest neighbour, icp.py:35-46,173,179 (scipy KDTree.query, k=1) ----
 * Pair b matches every valid row of cloud pair_src[b] against cloud
 * pair_tgt[b] (exhaustive, LDS-tiled, float64 direct differences, lowest index
 * on ties).  out_idx/out_dist are [n_pairs][out_stride]; dist is the Euclidean
 * distance (sqrt), index is relative to the target cloud.
 * max_src_n bounds the rows written per pair: rows [0, min(N, max_src_n)) of pair b's out rows are written and nothing
 * else is, so a source cloud with more valid rows than max_src_n is truncated to it (out_stride >= max_src_n keeps
 * every write inside pair b's rows).  A pair with an empty target gets index -1 and distance +inf. */
int icpmi_nn_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                   const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs,
                   int32_t max_src_n, int32_t dim,
                   int32_t* out_idx, double* out_dist, int32_t out_stride, void* stream);

/* What icpmi_nn_batch starts for these three arguments — no HIP call, no launch, no device pointer; the entry takes
 * its launch shape from this function.  The refusals are that entry's for them (ICPMI_ERR_ARG: a null out, n_pairs or
 * max_src_n < 0, dim outside {2, 3}).  A call that launches nothing (n_pairs == 0 or max_src_n == 0): ICPMI_OK and a
 * plan of zeros.
 *   rows_per_lane  S: source rows a lane holds in registers (1, 2 or 4, by the number of workgroups the call makes)
 *   threads        lanes of a workgroup;  rows_per_wg = threads * S consecutive source rows of one pair
 *   tile_points    target rows staged in LDS at a time;  chunk: target rows per running minimum (tile_points is a
 *                  multiple of it)
 *   grid_x         workgroups per pair, ceil(max_src_n / rows_per_wg);  launches: slices of at most 65 535 pairs
 * A workgroup whose rows reach past its cloud's count runs the body for min(S, ceil(rows left / threads)) rows. */
typedef struct icpmi_nn_plan {
    int32_t rows_per_lane, threads, rows_per_wg, tile_points, chunk, grid_x, launches;
} icpmi_nn_plan;
int icpmi_nn_batch_plan(int32_t n_pairs, int32_t max_src_n, int32_t dim, icpmi_nn_plan* out);

/* ---- estimate_normals_2d, icp.py:51-76 ------------------------------------
 * k+1 nearest neighbours (self included, k clamped to n-1), 2x2 covariance,
 * eigenvector of the smaller eigenvalue, unit length.  Sign is arbitrary, as
 * in the reference (it cancels in the point-to-line solve).  k <= 31 here (the
 * exhaustive companion of icpmi_nn_batch); icpmi_prepare_targets takes any k.
 * One workgroup per selected cloud: cloud_ids[n_sel] lists the clouds to
 * process (NULL = clouds 0..n_sel-1).  max_n bounds the rows of any selected
 * cloud; total_rows = off[C].  The workspace is only needed when max_n > 8192
 * (the x-sorted index then lives in global memory instead of LDS). */
size_t icpmi_normals_workspace_bytes(int32_t total_rows, int32_t max_n);
int icpmi_normals_2d_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                           const int32_t* cloud_ids, int32_t n_sel, int32_t total_rows,
                           int32_t max_n, int32_t k, double* out_normals,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- _point_to_line_solve_2d, icp.py:79-115 --------------------------------
 * One linearised point-to-line step over n_src correspondences. out_Rt = 6
 * doubles: R row-major (4) then t (2). Exactly singular system -> identity. */
int icpmi_p2l_solve_2d(const double* src, int32_t n_src, const double* tgt, const double* normals,
                       const int32_t* nn_idx, double* out_Rt, void* stream);

/* ---- ICP, icp.py:132-223 (after its two voxel_downsample calls) ------------
 * Runs n_pairs independent registrations to completion on the device: NN
 * search, correspondence rejection, point-to-line / point-to-point solve,
 * apply, error, convergence test; one workgroup per pair, no host round trip.
 * normals: same row layout as pts (only rows of target clouds are read; may be
 * NULL for point_to_point).  init: [n_pairs][dim*dim + dim] (R then t) or NULL.
 * results: [n_pairs][ICPMI_RES_DOUBLES].  max_src_n bounds the valid rows of
 * any source cloud, max_tgt_n those of any target cloud, total_rows = off[C].
 *
 * prepared (optional): buffer filled by icpmi_prepare_targets for the target
 * clouds of this batch.  With it, 2-D pairs whose source has at most 4096 rows
 * run on the fast kernel (exact sweep search on the axis-sorted target copy —
 * staged in LDS up to 4096 target rows, read in place through L2 above; pair
 * state in registers; `normals` is then not read, and `workspace` is optional:
 * given, a point_to_line batch of >= 1024 pairs runs in two stages — every pair
 * up to 12 iterations, then the pairs still running, parked there with their
 * moving rows and matches, together in a second launch — and a pair of any
 * batch whose first step leaves a mean squared error above option ICP2_FAR (it
 * starts metres from its target) is parked likewise and finished by the kernel
 * for far queries; both give the same results bit for bit, sooner).  Without
 * `prepared`, or for 3-D / larger
 * sources, the exhaustive LDS-tiled kernel runs and needs `workspace` (and
 * `normals` for point_to_line).  Results agree. */
size_t icpmi_icp_workspace_bytes(int32_t n_pairs, int32_t max_src_n, int32_t dim);
int icpmi_icp_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                    const double* normals, const void* prepared,
                    const int32_t* pair_src, const int32_t* pair_tgt,
                    int32_t n_pairs, int32_t max_src_n, int32_t max_tgt_n, int32_t total_rows,
                    const icpmi_icp_params* params_host, const double* init, double* results,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The loop-closure gate of slam.py:582-597: the candidates are tried in order and the first whose error is below
 * the gate is taken (`break  # one closure per scan is enough`), so the ones after it are never computed.  Same call
 * as icpmi_icp_batch (same results), plus: pair b is candidate index_base + b * index_stride (index_base >= 0,
 * index_stride >= 1: a rank of a sharded run passes its rank and the world size); it is ELIGIBLE when
 * search_records == NULL or the status of its rotation-search record (slot ICPMI_RSBREC_STATUS, stride
 * ICPMI_RSBREC_DOUBLES, icpmi_rotation_search_batch) is below ICPMI_RSB_ST_CAPACITY (ok, or too few points: the ICP
 * starts from the identity as the reference's does; ICPMI_RSB_ST_CAPACITY: the caller redoes the candidate,
 * ICPMI_RSB_ST_NO_FINE: no fine grid), and ACCEPTED when it is eligible, not skipped and its error is < error_accept
 * (NaN: never).  A candidate whose index is above that of an accepted one may stop early with status
 * ICPMI_ST_SKIPPED: its record then holds the totals of the steps it applied, `iterations` is their count, and
 * error / delta are those of the last step whose error was taken (the step before, for a candidate stopped between
 * the launches of a two-stage run).  Every other record — every candidate up to the first accepted one included —
 * is bit for bit the record icpmi_icp_batch writes; skipping is allowed, never required (the exhaustive kernel
 * never skips).  first_accepted_dev (device, one int32): on completion the lowest accepted candidate index, -1 when
 * none; it also serves as the gate word during the call.  error_accept <= 0 accepts nothing and skips nothing. */
int icpmi_icp_batch_gated(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                          const double* normals, const void* prepared,
                          const int32_t* pair_src, const int32_t* pair_tgt,
                          int32_t n_pairs, int32_t max_src_n, int32_t max_tgt_n, int32_t total_rows,
                          const icpmi_icp_params* params_host, const double* init, double* results,
                          void* workspace, size_t workspace_bytes, double error_accept, const double* search_records,
                          int32_t index_base, int32_t index_stride, int32_t* first_accepted_dev, void* stream);

/* ---- information matrix of an ICP result: the normal equations of _point_to_line_solve_2d, icp.py:92-104 (ATA, ATb),
 * evaluated once at a given transform; matching and rejection as icp.py:179, 184-186 --------------------------------
 * The reference weights its pose-graph edges isotropically (slam.py:548, 592); the Gauss-Newton Hessian of the last
 * ICP step says how well each direction of [theta, tx, ty] is constrained.  A pass of its own, after the ICP: the fused
 * kernels are not touched.  2-D rows only (the entry takes no `dim`); a method other than the two below:
 * ICPMI_ERR_UNSUPPORTED.
 * For pair b, S the valid rows of cloud pair_src[b], Q and N the valid rows of cloud pair_tgt[b] and their normals
 * (`normals`: row layout of pts; required for ICPMI_POINT_TO_LINE, NULL: ICPMI_ERR_ARG; not read for
 * ICPMI_POINT_TO_POINT), transforms[b] = {R row-major (4), t (2)}:
 *   moved row   p' = ((R00 * sx + R01 * sy) + tx, (R10 * sx + R11 * sy) + ty) — float64, evaluated exactly as written:
 *               two products, their sum, then the translation, every operation rounded on its own (no fused
 *               multiply-add);
 *   match       j = the exact nearest row of Q to p', d2 = dx * dx + dy * dy, lowest index on ties (icpmi_nn_batch);
 *   inlier      max_corr_dist < 0 (None), or dist * dist < max_corr_dist * max_corr_dist with dist = sqrt(d2);
 *   point_to_line, per inlier, n = N[j], q = Q[j]:  c = ny * p'x - nx * p'y, A row = [c, nx, ny],
 *               b = -(nx * (p'x - qx) + ny * (p'y - qy));
 *   point_to_point, per inlier, two rows:  [-p'y, 1, 0 | -(p'x - qx)] and [p'x, 0, 1 | -(p'y - qy)];
 *   H = sum A^T A, g = sum A^T b, sse = sum b * b over those rows.
 * out [n_pairs][ICPMI_INFO_DOUBLES], slots ICPMI_INFO_*: H's upper triangle (theta-theta, theta-x, theta-y, xx, xy, yy),
 * g (theta, x, y), sse, inliers, source rows, status; the rest zero.  Status 0: ok; ICPMI_ST_FEW_INLIERS: a gate is
 * given and inliers < max(3, rows / 10) (icp.py:186; the sums over the inliers are still written); ICPMI_ST_EMPTY: a
 * cloud of the pair has no rows (every other slot zero).
 * One workgroup of ICPMI_INFO_THREADS threads per pair: thread l takes the source rows l, l + ICPMI_INFO_THREADS, ...
 * (any number of them: max_src_n, their upper bound, sizes nothing and is only checked to be >= 0), the target passes
 * through LDS ICPMI_INFO_TILE_ROWS rows at a time (any number of them), and the partial sums meet in one fixed tree —
 * no atomics — so a record is the same bits run after run and in whatever batch its pair is computed.  The search is
 * exhaustive: rows(S) * rows(Q) distance evaluations by one workgroup.  No workspace. */
#define ICPMI_INFO_DOUBLES 16
#define ICPMI_INFO_H 0            /* 6: theta-theta, theta-x, theta-y, xx, xy, yy */
#define ICPMI_INFO_G 6            /* 3: theta, x, y                               */
#define ICPMI_INFO_SSE 9
#define ICPMI_INFO_INLIERS 10
#define ICPMI_INFO_ROWS 11
#define ICPMI_INFO_STATUS 12
#define ICPMI_INFO_THREADS 512
#define ICPMI_INFO_TILE_ROWS 2048
int icpmi_icp_information_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                const double* normals, const int32_t* pair_src, const int32_t* pair_tgt,
                                int32_t n_pairs, int32_t max_src_n, const double* transforms,
                                int32_t method, double max_corr_dist, double* out, void* stream);

/* ---- prepared targets: axis choice + sort (+ normals) for the sweep search ----
 * For every selected cloud (<= 4096 rows): pick the projection axis (x, y, x+y
 * or x-y) with the smallest expected search window, sort the cloud along it and
 * store the sorted points, the sorted->row map and the axis in `prepared`
 * (icpmi_prepared_bytes(total_rows, n_clouds) bytes).  normal_k >= 0 also
 * computes estimate_normals_2d (icp.py:51-76) with k = normal_k (any k, as the reference:
 * up to 31 from register lists, beyond that a wave per query): stored in sorted order inside
 * `prepared`, and in row order in out_normals if given.
 * normal_k < 0 skips normals (point_to_point).
 *
 * Clouds above 4096 rows (a rolling submap) are prepared through global memory
 * (rocPRIM sort) and later searched in place through L2; for them the launcher
 * needs the sizes on the host: off_host mirrors off_dev and cloud_ids_host
 * mirrors cloud_ids (both may be NULL when max_n <= 4096).  max_n = rows of the
 * largest selected cloud; it also sizes the sort scratch inside `prepared`. */
size_t icpmi_prepared_bytes(int32_t total_rows, int32_t n_clouds, int32_t max_n);
int icpmi_prepare_targets(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                          const int32_t* cnt_dev, const int32_t* cloud_ids, const int32_t* cloud_ids_host,
                          int32_t n_sel, int32_t n_clouds, int32_t total_rows, int32_t max_n,
                          int32_t normal_k, double* out_normals, void* prepared, size_t prepared_bytes,
                          void* stream);

/* The same, with the sort order left to the library: allow_polar != 0 lets clouds of at most 2048 rows be sorted
 * by BEARING about the frame origin instead of along a projection, when the library estimates smaller search
 * windows for it (a lidar scan in its sensor frame has one return per bearing, so the points within a distance B
 * of a query lie in a wedge of a few points, while a projection slab holds every wall that crosses it).  The
 * order only changes how fast icpmi_icp_batch searches — results are the exact nearest neighbours either way.
 * Buffers prepared with allow_polar may only be passed to icpmi_icp_batch (icpmi_nn_prepared_batch walks
 * projections).  Replaces no reference function: the KDTree construction of icp.py:173 is the closest analogue. */
int icpmi_prepare_targets_ex(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                             const int32_t* cnt_dev, const int32_t* cloud_ids, const int32_t* cloud_ids_host,
                             int32_t n_sel, int32_t n_clouds, int32_t total_rows, int32_t max_n,
                             int32_t normal_k, double* out_normals, void* prepared, size_t prepared_bytes,
                             int32_t allow_polar, void* stream);

/* Nearest neighbour on prepared targets (same contract as icpmi_nn_batch, same
 * answers bit for bit, icp.py:179): binary search + outward sweep on the sorted
 * copy instead of the exhaustive scan.  Target clouds of the pairs must have
 * been prepared (<= 4096 rows).  out_second_sq (optional) receives the squared
 * distance of the second nearest target point.  As there, max_src_n bounds the
 * rows written per pair: a longer source cloud is truncated to it. */
int icpmi_nn_prepared_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                            const void* prepared, const int32_t* pair_src, const int32_t* pair_tgt,
                            int32_t n_pairs, int32_t max_src_n, int32_t max_tgt_n, int32_t total_rows,
                            int32_t* out_idx, double* out_dist, double* out_second_sq,
                            int32_t out_stride, void* stream);

/* ---- rotation search scoring, utilities/features.py:213-232 (and slam.py:138-159) ----
 * For every angle a (given as cos, sin pairs — computed by the caller with the
 * reference's own NumPy calls): mean over the rows of src_c of the squared
 * nearest-neighbour distance of (src_c @ R(a).T + shift) in tgt, R = [[c,-s],[s,c]].
 * One launch for a whole sweep.  src_c: (n_src, 2), tgt: (n_tgt, 2), row-major.  An angle whose cos / sin is NaN (or a
 * source row that is) scores NaN, as the mean of NumPy's distances would — not the +inf a scan that skips NaN leaves. */
int icpmi_rotation_scores(const double* src_c, int32_t n_src, const double* tgt, int32_t n_tgt,
                          const double* cos_sin, int32_t n_angles, double shift_x, double shift_y,
                          double* out_scores, void* stream);

/* The whole correlative search on the device — utilities/features.py:198-232 (voxel filter of both clouds, their
 * means, the coarse sweep, its arg-min, the fine sweep around the winner, its arg-min) and the sweeps of
 * slam.py:146-159 — one chain of launches, nothing returns to the host in between.
 * pts: n_src source rows followed by n_tgt target rows (raw clouds, (n, 2) float64).  coarse_cs: cos, sin of the
 * n_coarse coarse angles.  fine_cs / fine_cnt: for EVERY coarse angle k the fine grid that follows when k wins
 * (fine_cnt[k] <= max_fine angles, cos, sin at fine_cs[(k * max_fine + j) * 2]) — the grids and their cos / sin are
 * the caller's (the reference's own NumPy expressions), so the chosen angle is the reference's bit for bit.
 * centred != 0: the source is centred on its mean and shifted to the target's mean (features.py:205-216);
 * else the rows are rotated as they are and shifted by (shift_x, shift_y) (slam.py:138-143).
 * out_record (device, ICPMI_RSREC_DOUBLES doubles, slots ICPMI_RSREC_*): voxel counts of source and target, mean of
 * the source (2), shift (2), winning coarse index, its score, length of its fine grid, winning fine index, its score,
 * reserved.  np.argmin semantics (first minimum; first NaN if any).  The voxel-filtered clouds stay in the workspace
 * (ICPMI_RS_WS_CLOUDS bytes in: source rows, then target rows — n_src rows further on; counts as int32 at byte
 * ICPMI_RS_WS_COUNTS) for a following icpmi_nn_batch-style refinement. */
#define ICPMI_RSREC_DOUBLES 12
#define ICPMI_RSREC_NS 0          /* rows of the filtered source                  */
#define ICPMI_RSREC_NT 1          /* rows of the filtered target                  */
#define ICPMI_RSREC_MUS 2         /* mean of the source (2; zeros when not centred) */
#define ICPMI_RSREC_MUT 4         /* shift (2): mean of the target, or the caller's */
#define ICPMI_RSREC_K 6           /* winning coarse index                         */
#define ICPMI_RSREC_CSCORE 7      /* its score                                    */
#define ICPMI_RSREC_NF 8          /* length of its fine grid                      */
#define ICPMI_RSREC_J 9           /* winning fine index                           */
#define ICPMI_RSREC_FSCORE 10     /* its score                                    */
#define ICPMI_RS_WS_COUNTS 16     /* byte offsets into the search workspace       */
#define ICPMI_RS_WS_CLOUDS 256
size_t icpmi_rotation_search_workspace_bytes(int32_t n_src, int32_t n_tgt, int32_t n_coarse, int32_t max_fine);
int icpmi_rotation_search(const double* pts, int32_t n_src, int32_t n_tgt, double voxel_size,
                          const double* coarse_cs, int32_t n_coarse,
                          const double* fine_cs, const int32_t* fine_cnt, int32_t max_fine,
                          int32_t centred, double shift_x, double shift_y,
                          double* out_record, void* workspace, size_t workspace_bytes, void* stream);

/* Translation refinement of the submap variant, slam.py:161-181, on the state icpmi_rotation_search left behind
 * (search_workspace: the same buffer, untouched since; record: its out_record; the same angle tables): the filtered
 * source rotated by the winning angle (NumPy's own (n, 2) @ (2, 2) arithmetic) and placed at (pred_x, pred_y), its
 * nearest target rows, np.percentile(d^2, 80) with linear interpolation, and the mean of (matched - rotated) over the
 * rows at or below it — out4 (device): refined t (2; the predicted position when fewer than 5 rows qualify, slam.py:
 * 175-181), the inlier count, the percentile.  n_src / n_tgt: the RAW row counts passed to the search; n_src <=
 * ICPMI_RSR_MAX_ROWS (ICPMI_ERR_UNSUPPORTED above: refine on the host from the filtered clouds). */
#define ICPMI_RSR_MAX_ROWS 2048
size_t icpmi_rotation_refine_workspace_bytes(int32_t n_src);
int icpmi_rotation_refine(const void* search_workspace, int32_t n_src, int32_t n_tgt, const double* record,
                          const double* coarse_cs, const double* fine_cs, int32_t max_fine,
                          double pred_x, double pred_y, double* out4, void* scratch, size_t scratch_bytes, void* stream);

/* ---- batched pre-alignment: rotation_search (utilities/features.py:165-242) for every pair of a batch — the first
 * half of _run_icp_pair (slam.py:53-98), which slam.py:575-579 calls once per loop-closure candidate ----------------
 * pts / off_dev / off_host: a cloud set of RAW 2-D clouds (at most 4096 rows each); pair b searches the rotation of
 * cloud pair_src[b] onto cloud pair_tgt[b].  tgt_ids (device, optional): the distinct target clouds (only they are
 * put in search order; NULL = every cloud).  One chain of launches: voxel filter of every cloud at voxel_size, the
 * means of the filtered clouds, the search order of the targets, then ONE workgroup per pair for both sweeps.  Angle
 * grids as in icpmi_rotation_search (coarse_cs; fine_cs / fine_cnt / max_fine: one fine grid per coarse winner; the
 * caller's NumPy cos / sin; at most ICPMI_RSB_MAX_ANGLES coarse angles and as many per fine grid).
 * Only the arg-min of the coarse scores matters to the reference (features.py:223), so a workgroup bounds every
 * coarse score from below with a distance field of its target (one look-up per row), scores angles exactly — same
 * float64 nearest-neighbour distances as icpmi_rotation_search — in order of that bound, and stops at the first angle
 * whose bound exceeds the best exact score: np.argmin over the scored angles (first minimum) is np.argmin over all.
 * out_records [n_pairs][ICPMI_RSBREC_DOUBLES]: the ICPMI_RSREC_* slots as icpmi_rotation_search's record (filtered
 * counts, mean of the source (2), mean of the target (2), winning coarse index, its score, length of its fine grid,
 * winning fine index, its score); ICPMI_RSBREC_STATUS — ICPMI_RSB_ST_OK searched; _FEW a filtered cloud has fewer
 * than 5 points (features.py:203-204: identity, zeros, inf); _CAPACITY a filtered cloud exceeds the on-chip capacity
 * (not searched: use icpmi_rotation_search); _NO_FINE the winner's fine grid is empty (np.argmin raises in the
 * reference); ICPMI_RSBREC_EVALS the coarse angles scored exactly, counted as a schedule-free number: those
 * whose bound does not exceed the winning score (every run scores these), and at least one per wave of the workgroup (8,
 * or all the coarse angles if fewer: a wave's first angle is scored before any result exists); a run may score a few
 * more, depending on when its waves see each other's results, and those are not counted, so that a record is the same
 * bits run after run — ICPMI_RSBREC_FEVALS the fine angles scored (diagnostic).
 * out_init (optional) [n_pairs][6]: R row-major then t = mu_t - R mu_s (features.py:235-237) — the `init` argument of
 * icpmi_icp_batch, so pre-alignment and ICP chain on one stream with no host round trip; identity for a status other
 * than ICPMI_RSB_ST_OK.
 * max_rows_hint: an upper bound the caller expects for the FILTERED clouds (0: none).  The on-chip copies are sized
 * by min(largest raw cloud, ICPMI_RSB_MAX_ROWS, hint); up to 1024 rows two workgroups share a CU.  A pair beyond it
 * gets ICPMI_RSB_ST_CAPACITY. */
#define ICPMI_RSBREC_DOUBLES 16
#define ICPMI_RSBREC_STATUS 11
#define ICPMI_RSBREC_EVALS 12
#define ICPMI_RSBREC_FEVALS 13
#define ICPMI_RSB_ST_OK 0
#define ICPMI_RSB_ST_FEW 1
#define ICPMI_RSB_ST_CAPACITY 2
#define ICPMI_RSB_ST_NO_FINE 3
#define ICPMI_RSB_MAX_ANGLES 1024 /* coarse angles, and angles per fine grid      */
#define ICPMI_RSB_MAX_ROWS 2048   /* rows of a filtered cloud a workgroup holds   */
size_t icpmi_rotation_search_batch_workspace_bytes(int32_t total_rows, int32_t n_clouds, int32_t max_n);
int icpmi_rotation_search_batch(const double* pts, const int32_t* off_dev, const int32_t* off_host, int32_t n_clouds,
                                const int32_t* tgt_ids, int32_t n_tgt_ids,
                                const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs,
                                double voxel_size, const double* coarse_cs, int32_t n_coarse,
                                const double* fine_cs, const int32_t* fine_cnt, int32_t max_fine,
                                int32_t max_rows_hint, double* out_records, double* out_init,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- resident scan history: the loop-closure candidates of slam.py:566-597 are PAST scans (slam.py:554 appends one per
 * scan to scan_history; pose-graph optimisation moves their poses, slam.py:606-607, never their points), so everything
 * _run_icp_pair (slam.py:53-98) derives from a target alone is computed once, when the scan enters the history --------
 * The state is the caller's memory, named by this struct (host).  pts / off_dev: a cloud set of scan_capacity RAW 2-D
 * clouds packed back to back (the filter takes a cloud's rows from its offsets), a cloud not added yet having zero rows:
 * off[c] = rows in use for every c at or above the number of scans.  ids[c] = c (device).  Per row of row_capacity:
 * the raw rows, the two filtered copies (16 B each) and the two prepared buffers (icpmi_prepared_bytes(row_capacity,
 * scan_capacity, 0) bytes each, about 40 B a row); per cloud: the two counts and the mean (rs_means [scan_capacity][2]).
 * Both prepared buffers are laid out for (row_capacity, scan_capacity) — never for the rows in use, which change with
 * every scan — and start out from icpmi_prepared_relayout.  voxel_ws: icpmi_voxel_workspace_bytes(4096) bytes. */
typedef struct icpmi_history {
    const double* pts;        /* raw clouds                                                   */
    const int32_t* off_dev;   /* [scan_capacity + 1]                                          */
    const int32_t* ids;       /* [scan_capacity], ids[c] = c                                  */
    double* icp_vox;          /* filtered at icp_voxel (icp.py:149-150), cloud set layout     */
    int32_t* icp_cnt;
    void* icp_prepared;       /* icpmi_prepare_targets_ex of them, allow_polar, normal_k      */
    double* rs_vox;           /* filtered at rs_voxel (features.py:198-199)                   */
    int32_t* rs_cnt;
    double* rs_means;         /* np.mean(axis=0) of each (features.py:205-206)                */
    void* rs_prepared;        /* search order of them, no normals                             */
    void* voxel_ws;
    size_t prepared_bytes;    /* of each prepared buffer                                      */
    size_t voxel_ws_bytes;
    double icp_voxel;
    double rs_voxel;
    int32_t scan_capacity;
    int32_t row_capacity;
    int32_t normal_k;         /* < 0: no normals (a point_to_point history)                   */
    int32_t allow_polar;      /* of the ICP's prepared buffer; 0 once a scan has more than 2048 rows */
} icpmi_history;

/* Processes the clouds [first, first + n_new) and leaves every other cloud's state as it is: voxel filter at icp_voxel,
 * icpmi_prepare_targets_ex of them into icp_prepared (prepare != 0), voxel filter at rs_voxel, their means, their search
 * order into rs_prepared (prepare != 0) — the steps ICP (icp.py:149-173) and rotation_search (features.py:198-211) take
 * per call, by the same kernels.  prepare == 0: a cloud that is only ever a SOURCE (the current scan staged behind the
 * last one).  off_host mirrors off_dev.  A cloud above 4096 rows: ICPMI_ERR_UNSUPPORTED. */
int icpmi_history_add(const icpmi_history* h, const int32_t* off_host, int32_t first, int32_t n_new, int32_t prepare,
                      void* stream);

/* The second half of icpmi_rotation_search_batch on the resident state: same arguments from pair_src on, same records,
 * out_init and statuses (features.py:213-242).  max_n: rows of the largest RAW cloud any pair names (sizes the on-chip
 * copies).  A pair whose target was never added reports ICPMI_RSB_ST_CAPACITY. */
int icpmi_history_search(const icpmi_history* h, const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs,
                         int32_t max_n, const double* coarse_cs, int32_t n_coarse, const double* fine_cs,
                         const int32_t* fine_cnt, int32_t max_fine, int32_t max_rows_hint, double* out_records,
                         double* out_init, void* stream);

/* transform_points_2d (slam.py:46-50) of resident raw rows, for the rebuilds that follow an accepted closure: the map
 * replay of _rebuild_map (slam.py:271-277) and the submap buffer of slam.py:612-615 take scan ids and poses, and the world
 * rows never visit the host.  Rows [out_off[k], out_off[k + 1]) of out_rows are the raw rows of scan ids[k] (h->pts at
 * off_dev[ids[k]] .. off_dev[ids[k] + 1]) under poses[k] = {R row-major, t}, six doubles, the layout of `init` above.  ids,
 * poses, out_off [n_ids + 1] and out_rows are device memory; scans may repeat and come in any order; only pts, off_dev and
 * scan_capacity of h are used.  Bit for bit what NumPy's `points @ T[:2, :2].T + T[:2, 2]` gives: a scan of two or more rows
 * is a gemm there, fma(y, R[c][1], x * R[c][0]) + t[c]; a scan of exactly ONE row is a gemv, fma(x, R[c][0], y * R[c][1]) +
 * t[c].  n_ids == 0: no launch, ICPMI_OK.  One launch, no workspace. */
int icpmi_history_world_rows(const icpmi_history* h, const int32_t* ids, int32_t n_ids, const double* poses,
                             const int32_t* out_off, double* out_rows, void* stream);

/* Copies the first rows_used rows and clouds_used clouds of a prepared buffer laid out for (src_rows, src_clouds) into
 * one laid out for (dst_rows, dst_clouds) >= them, and marks every further cloud of dst "no order" (what
 * icpmi_history_search reports as ICPMI_RSB_ST_CAPACITY).  src == NULL with nothing in use: a fresh buffer.  No
 * reference counterpart: scan_history is a Python list (slam.py:554). */
int icpmi_prepared_relayout(const void* src, int32_t src_rows, int32_t src_clouds, int32_t rows_used, int32_t clouds_used,
                            void* dst, size_t dst_bytes, int32_t dst_rows, int32_t dst_clouds, void* stream);

/* ---- feature-based pre-alignment, utilities/features.py:35-160, 247-315 ------------------------------------------
 * The five stages of feature_based_alignment, each on a cloud set of 2-D clouds (pts / off_dev / cnt_dev as above;
 * cloud_ids[n_sel]: the clouds to process, NULL = clouds 0..n_sel-1), one workgroup per cloud or per pair with the cloud
 * in LDS: at most ICPMI_FT_MAX_ROWS valid rows per cloud (a larger cloud is left alone: no output, 0 keypoints), k <= 31,
 * at most ICPMI_FT_MAX_KP keypoints per cloud.  Per-cloud tables are indexed by the cloud's number in the set.
 * A pair's record is ICPMI_FTREC_DOUBLES doubles with the slots ICPMI_FTREC_* and a status ICPMI_FT_ST_*. */
#define ICPMI_FT_MAX_ROWS 2048
#define ICPMI_FT_MAX_KP 256
#define ICPMI_FT_DESC_STRIDE 32   /* doubles per descriptor row (k <= 31)         */
#define ICPMI_FTREC_DOUBLES 16
#define ICPMI_FTREC_NS 0          /* rows of the filtered source                  */
#define ICPMI_FTREC_NT 1          /* rows of the filtered target                  */
#define ICPMI_FTREC_KPS 2         /* keypoints of the source                      */
#define ICPMI_FTREC_KPT 3         /* keypoints of the target                      */
#define ICPMI_FTREC_MATCHES 4
#define ICPMI_FTREC_INLIERS 5
#define ICPMI_FTREC_R 6           /* R row-major (4)                              */
#define ICPMI_FTREC_T 10          /* t (2)                                        */
#define ICPMI_FTREC_STATUS 12
#define ICPMI_FTREC_BEST 13       /* index of the winning hypothesis (-1: none)   */
#define ICPMI_FT_ST_OK 0          /* aligned                                      */
#define ICPMI_FT_ST_FEW_ROWS 1    /* a filtered cloud has fewer than 10 rows, features.py:281-282 */
#define ICPMI_FT_ST_CAPACITY 2    /* a filtered cloud exceeds ICPMI_FT_MAX_ROWS (not aligned: the caller falls back) */
#define ICPMI_FT_ST_FEW_KP 3      /* fewer than 2 keypoints, features.py:290-291  */
#define ICPMI_FT_ST_FEW_MATCHES 4 /* fewer than 2 matches, features.py:299-300    */
#define ICPMI_FT_ST_DESC_LEN 5    /* the two clouds' descriptors differ in length (NumPy raises in the reference) */

/*
 * compute_curvature, features.py:35-54.  out_curvature: one double per row (row layout of pts).  The k+1 nearest rows
 * (k clamped to n-1, the lower row on equal distances), np.cov of them, eigenvalues in closed form,
 * ev[0] / (ev[-1] + 1e-10); fewer than 3 neighbours: 0.  The neighbours are summed in ascending row order (the reference
 * sums them in distance order: equal to its own rounding), so rows with one neighbour set get one value bit for bit. */
int icpmi_feature_curvature_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                  const int32_t* cloud_ids, int32_t n_sel, int32_t k, double* out_curvature,
                                  void* stream);

/* extract_keypoints, features.py:57-71.  The candidates of a cloud are walked in `order` (int32 per row, row layout:
 * order[off[c] + i] = i-th candidate row of cloud c — the drop-in passes np.argsort(-curvatures)) or, with order == NULL,
 * by descending `curvature` (row layout) with ties by ascending row; a candidate is kept when no kept point is closer
 * than min_dist (sqrt(dx*dx + dy*dy) < min_dist, the reference's comparison bit for bit), until top_n are kept.
 * out_kp[c * kp_stride + s]: row of the s-th keypoint of cloud c; out_kp_cnt[c]: their number.  top_n <= kp_stride. */
int icpmi_feature_keypoints_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                  const int32_t* cloud_ids, int32_t n_sel, const double* curvature,
                                  const int32_t* order, int32_t top_n, double min_dist, int32_t* out_kp,
                                  int32_t* out_kp_cnt, int32_t kp_stride, void* stream);

/* compute_descriptors, features.py:76-87.  out_desc[(c * kp_stride + s) * ICPMI_FT_DESC_STRIDE + q]: distance from
 * keypoint s of cloud c to its (q+1)-th nearest other row, ascending, q < out_desc_len[c] = min(k, n-1) (the rest of
 * the row is zero): exact
 * neighbour distances with IEEE sqrt, as KDTree.query returns them. */
int icpmi_feature_descriptors_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                    const int32_t* cloud_ids, int32_t n_sel, const int32_t* kp, const int32_t* kp_cnt,
                                    int32_t kp_stride, int32_t k, double* out_desc, int32_t* out_desc_len, void* stream);

/* match_descriptors, features.py:92-106, for every pair (pair_src[b], pair_tgt[b]) of clouds: squared descriptor
 * distances by direct differences, the two smallest per source keypoint (the lower index on ties), D0 < ratio_sq * D1
 * (ratio_sq = ratio ** 2 from the caller, as the reference forms it).  out_matches[(b * kp_stride + m) * 2]: source and
 * target keypoint of match m, in source-keypoint order; out_match_cnt[b].  No source descriptors, fewer than 2 target
 * descriptors or descriptors of different lengths: no matches. */
int icpmi_feature_match_batch(const double* desc, const int32_t* desc_len, const int32_t* kp_cnt, int32_t kp_stride,
                              const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs, double ratio_sq,
                              int32_t* out_matches, int32_t* out_match_cnt, void* stream);

/* ransac_align, features.py:125-160 (with _rigid_from_points, features.py:111-122), for every pair.  The hypotheses are
 * an INPUT: hyp_idx (int32 [n_iter][2], the index pairs np.random.choice(n, 2, replace=False) drew) or hyp_u (double
 * [n_iter][2] uniform in [0, 1), mapped on the device to i = floor(u0 * n), j = floor(u1 * (n - 1)), j += (j >= i), n
 * the pair's match count) — exactly one of the two; pair b reads from element b * hyp_pair_stride on (0: one table for
 * all).  Per hypothesis: two-point rigid fit in closed form (both matches on one target keypoint, W = 0: R = I as the
 * reference's SVD gives), error of every match, inliers err < inlier_thresh; the first hypothesis with the largest
 * count wins, a count of 0 never replaces the identity; then the refit on the inliers of the best when there are at
 * least 2.  A hypothesis with an index outside [0, n) or two equal indices counts 0.
 * out_records [n_pairs][ICPMI_FTREC_DOUBLES]: ICPMI_FTREC_MATCHES, _INLIERS, _R (row-major), _T, _STATUS (ICPMI_FT_ST_OK,
 * or ICPMI_FT_ST_FEW_MATCHES: fewer than 2 matches — identity, zeros, 0), _BEST (-1: none); the other slots 0.
 * out_counts (optional) [n_pairs][n_iter]: inliers of every hypothesis. */
int icpmi_feature_ransac_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev, const int32_t* kp,
                               const int32_t* kp_cnt, int32_t kp_stride, const int32_t* pair_src, const int32_t* pair_tgt,
                               int32_t n_pairs, const int32_t* matches, const int32_t* match_cnt, const int32_t* hyp_idx,
                               const double* hyp_u, int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh,
                               double* out_records, int32_t* out_counts, void* stream);

/* feature_based_alignment, features.py:247-315, as _run_icp_pair calls it (slam.py:68-88), for every pair of a batch:
 * voxel filter of every cloud at voxel_size, then the five stages above (candidate order: descending curvature, ties by
 * ascending row) — one chain of launches on `stream`, nothing returns to the host.  pts / off_dev / off_host: RAW 2-D
 * clouds.  init_in (optional) [n_pairs][6], R row-major then t: the source of pair b is transformed by it before the
 * filter (slam.py:69-71; pair_src_host, the host mirror of pair_src, is then required).  init_out (optional)
 * [n_pairs][6]: R_feat @ R_init, t_init @ R_feat.T + t_feat when the pair has at least min_inliers inliers, else init_in
 * (the identity without one) (slam.py:83-88) — the `init` of icpmi_icp_batch.
 * out_records [n_pairs][ICPMI_FTREC_DOUBLES]: every ICPMI_FTREC_* slot (filtered rows of source and target, their
 * keypoints, matches, inliers, R, t, status, winning hypothesis).  Status ICPMI_FT_ST_*, listed above (_DESC_LEN:
 * k_descriptor > rows - 1 of one of the clouds).  Every status but ICPMI_FT_ST_OK leaves identity, zeros, 0 inliers. */
size_t icpmi_feature_align_batch_workspace_bytes(int32_t total_rows, int32_t n_clouds, int32_t max_n, int32_t n_pairs,
                                                 int32_t top_n, int32_t with_init);
int icpmi_feature_align_batch(const double* pts, const int32_t* off_dev, const int32_t* off_host, int32_t n_clouds,
                              const int32_t* pair_src, const int32_t* pair_src_host, const int32_t* pair_tgt,
                              int32_t n_pairs, double voxel_size, int32_t k_curvature, int32_t top_n, double min_kp_dist,
                              int32_t k_descriptor, double ratio_sq, const int32_t* hyp_idx, const double* hyp_u,
                              int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh, int32_t min_inliers,
                              const double* init_in, double* init_out, double* out_records,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- resident features: the feature start of _run_icp_pair (slam.py:68-88) against past scans ------------------------
 * Filtering a cloud at the feature voxel size, compute_curvature, extract_keypoints and compute_descriptors are functions
 * of ONE cloud, and a past scan never changes: a history keeps their results in a feature store and a query runs
 * matching, RANSAC and the record only.  The store is the caller's memory, named by this struct (host), laid out over the
 * history's own cloud set — the same off_dev and ids, the history's scan_capacity and row_capacity, addressed by those
 * capacities and never by the rows or scans in use:
 *   per row of row_capacity    vox (16 B) and the curvature scratch curv (8 B): 24 B a raw row;
 *   per scan of scan_capacity  cnt, kp_cnt, desc_len (4 B each), kp [kp_stride] (4 B each) and
 *                              desc [kp_stride][ICPMI_FT_DESC_STRIDE] (256 B a keypoint slot): 12 + 260 * kp_stride bytes,
 *                              27 052 B a scan at the reference's top_n of 100 (kp_stride 104).
 * The cloud-side configuration the tables were computed with is part of the store; kp_stride is top_n rounded up to 8 (at
 * least 8), the stride of icpmi_feature_align_batch's own tables. */
typedef struct icpmi_feature_store {
    double* vox;              /* filtered at voxel_size (features.py:262-263), cloud set layout */
    double* curv;             /* [row_capacity] curvature of every filtered row (scratch)       */
    int32_t* cnt;             /* [scan_capacity] filtered rows                                  */
    int32_t* kp;              /* [scan_capacity][kp_stride]                                     */
    int32_t* kp_cnt;          /* [scan_capacity]                                                */
    double* desc;             /* [scan_capacity][kp_stride][ICPMI_FT_DESC_STRIDE]               */
    int32_t* desc_len;        /* [scan_capacity]                                                */
    double voxel_size;
    double min_kp_dist;
    int32_t k_curvature;
    int32_t top_n;
    int32_t k_descriptor;
    int32_t kp_stride;
} icpmi_feature_store;

/* Processes the clouds [first, first + n_new) of the history into the store and leaves every other cloud's state as it is:
 * voxel filter at the store's voxel size (on the tail of the offsets, as icpmi_history_add), curvature, keypoints by the
 * device order rule, descriptors — the launches of icpmi_feature_align_batch's first half, for this range.  Uses pts,
 * off_dev, ids, the voxel workspace and the capacities of h; off_host mirrors off_dev.  Refused on the host, before any
 * launch: a null pointer or a range beyond a capacity (ICPMI_ERR_ARG); k > 31, top_n > ICPMI_FT_MAX_KP or top_n > kp_stride
 * (ICPMI_ERR_UNSUPPORTED).  A scan whose filtered cloud exceeds ICPMI_FT_MAX_ROWS is left without features (0 keypoints):
 * its pairs report ICPMI_FT_ST_CAPACITY. */
int icpmi_history_features_add(const icpmi_history* h, const icpmi_feature_store* store, const int32_t* off_host, int32_t first,
                               int32_t n_new, void* stream);

/* The pair half of icpmi_feature_align_batch on the resident state: same arguments from pair_src on, same records,
 * init_out and statuses.  Sources and targets are clouds of the history (a staged source included).  max_n: rows of the
 * largest RAW source any pair names.
 * init_in == NULL ("features"): matching, RANSAC and the record straight on the store's tables; the workspace holds the
 * matches and their counts only, and off_host / pair_src_host are not read.
 * init_in != NULL ("both"): a work set of one transformed copy of its source per pair (h->pts rows @ R_init.T + t_init,
 * the gemm form fma(y, R[c][1], x * R[c][0]) + t[c] for every row count) is filtered and given curvature, keypoints and
 * descriptors in the workspace; the pair stages then take sources from it and targets from the store.  off_host (the
 * history's offsets) and pair_src_host are then required; a source beyond the capacities or above max_n rows:
 * ICPMI_ERR_ARG.  n_pairs == 0: no launch, ICPMI_OK. */
size_t icpmi_history_feature_align_workspace_bytes(int32_t n_pairs, int32_t max_n, int32_t top_n, int32_t with_init);
int icpmi_history_feature_align(const icpmi_history* h, const icpmi_feature_store* store, const int32_t* off_host,
                                const int32_t* pair_src, const int32_t* pair_src_host, const int32_t* pair_tgt,
                                int32_t n_pairs, int32_t max_n, double ratio_sq, const int32_t* hyp_idx, const double* hyp_u,
                                int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh, int32_t min_inliers,
                                const double* init_in, double* init_out, double* out_records, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- appearance signatures: loop-closure candidates by what a scan looks like, not by where the pose graph puts it ------
 * _find_loop_candidates (slam.py:230-268) keeps the past scans whose position ESTIMATE lies near the current one, so a
 * revisit drift has carried beyond its threshold is never matched.  A history can keep, per scan, a binary polar occupancy
 * image about the sensor (a 2-D Scan Context): ICPMI_SIG_RINGS rings of ring_width from min_range outwards by
 * ICPMI_SIG_SECTORS sectors of 2 pi / 64 from the x axis counter-clockwise, 260 bytes a scan, and rank its scans against
 * one by the overlap of the images under the best of the 64 rotations.  Integers end to end and no transcendental
 * function on the device: every result is bit-equal to a NumPy restatement (tests/signatures_ref.py).
 * The store is the caller's device memory, addressed by the history's scan_capacity:
 *   sig      [scan_capacity][ICPMI_SIG_RINGS] uint64: bit s of word r — ring r, sector s holds at least one raw row;
 *   sig_bits [scan_capacity] int32: the set bits of the scan's 32 words;
 *   tables   [ICPMI_SIG_TABLE_DOUBLES] double, made on the host: edge2[33], edge2[j] = (min_range + j * ring_width)^2,
 *            ascending; then bc[k] = cos(k pi / 32) and bs[k] = sin(k pi / 32) for k = 1 .. 15 (15 and 15).
 * (The store is three pointers in the argument lists, not a struct: ring_width and min_range reach the device through
 * edge2 alone.)
 * The rule of a RAW row (x, y) of the sensor frame (h->pts; no voxel size plays a part), each product and sum rounded:
 *   d2 = x * x + y * y;  ring = #{ j in 0 .. 32 : d2 >= edge2[j] } - 1;  the row is skipped unless 0 <= ring < 32 (NaN: every
 *   comparison false; inf: ring 32; a return below min_range; a row beyond the reach);
 *   q = (y >= 0) ? (x > 0 ? 0 : 1) : (x < 0 ? 2 : 3);  (u, v) = (x, y), (y, -x), (-x, -y), (-y, x) for q = 0 .. 3 (exact);
 *   sector = 16 q + #{ k in 1 .. 15 : v * bc[k] >= u * bs[k] }. */
#define ICPMI_SIG_RINGS 32
#define ICPMI_SIG_SECTORS 64
#define ICPMI_SIG_TABLE_DOUBLES 63
#define ICPMI_SIG_MAX_TOP 64
#define ICPMI_SIG_REC_INTS 4
#define ICPMI_SIG_REC_ID 0
#define ICPMI_SIG_REC_SCORE 1
#define ICPMI_SIG_REC_SHIFT 2
#define ICPMI_SIG_REC_BEST 3
#define ICPMI_SIG_TILE 64         /* candidates a workgroup of the pair kernel takes */

/* Writes sig and sig_bits of the clouds [first, first + n_new) of the history and leaves every other cloud's alone.  Uses
 * pts, off_dev and the capacities of h; off_host mirrors off_dev.  A cloud of zero rows gets 32 zero words and 0 bits;
 * nothing caps a cloud's rows (they are streamed).  One launch; n_new == 0: none, ICPMI_OK.  Refused on the host, before
 * the launch: a null pointer, a range beyond the scan capacity, a negative row count or rows beyond the row capacity
 * (ICPMI_ERR_ARG). */
int icpmi_history_signatures_add(const icpmi_history* h, uint64_t* sig, int32_t* sig_bits, const double* tables,
                                 const int32_t* off_host, int32_t first, int32_t n_new, void* stream);

/* Ranks scans against scans by their signatures.  query_ids [n_queries], lo, hi [n_queries] (device): the candidates of
 * query i are the scans c with lo[i] <= c < hi[i], clipped to [0, n_scans); an empty range is fine.  A query id is a
 * cloud of the store, n_scans (a source staged behind the last scan) included; one outside [0, scan_capacity) has no
 * candidates.  For a candidate with words B against the query's A:
 *   inter(s) = sum over r of popcount(A[r] & rotl64(B[r], s)), s = 0 .. 63;  best = the largest, shift = the LOWEST s with it;
 *   union = bits(A) + bits(B) - best;  score = union ? (best * 65535) / union : 0 (unsigned integer division: 0 .. 65535).
 * rotl by s turns the candidate's image counter-clockwise by s sectors, so the query's heading is the candidate's minus
 * s * 2 pi / 64.
 * out_records [n_queries][top_k][ICPMI_SIG_REC_INTS] int32 {id, score, shift, best}: the top_k candidates by descending
 * score, equal scores by ascending id; slots without a candidate {-1, 0, 0, 0}.  1 <= top_k <= ICPMI_SIG_MAX_TOP.
 * out_all (optional) [n_queries][n_scans] int32: (score << 8) | shift of every candidate, -1 outside the query's range.
 * workspace: icpmi_history_similar_workspace_bytes(n_queries, n_scans, top_k) bytes, 16-byte aligned (the rows of
 * out_all for a call without one; 0 for arguments the entry refuses; at least 256).  Only scan_capacity of h is used.
 * At most two launches (every pair; the selection), nothing returns to the host; n_queries == 0: none, ICPMI_OK.
 * Refused on the host, before any launch: n_queries or n_scans negative, n_scans above the scan capacity, top_k outside
 * [1, ICPMI_SIG_MAX_TOP], a null pointer other than out_all, a misaligned workspace (ICPMI_ERR_ARG); more than 65 535
 * queries or n_queries * n_scans reaching 2^31 (ICPMI_ERR_UNSUPPORTED); a workspace below its size (ICPMI_ERR_WORKSPACE).
 * A row exactly on the negative x axis (y = +0 or -0, x < 0) belongs to the second quadrant by the rule above and lands
 * in sector 31, not 32: the one place where a quarter turn of a cloud is not a rotation of its image by 16 sectors. */
size_t icpmi_history_similar_workspace_bytes(int32_t n_queries, int32_t n_scans, int32_t top_k);
int icpmi_history_similar(const icpmi_history* h, const uint64_t* sig, const int32_t* sig_bits, const int32_t* query_ids,
                          int32_t n_queries, const int32_t* lo, const int32_t* hi, int32_t n_scans, int32_t top_k,
                          int32_t* out_records, int32_t* out_all, void* workspace, size_t workspace_bytes, void* stream);

/* ---- OccupancyGrid2D, utilities/mapping.py ---------------------------------
 * world -> cell index, mapping.py:57-60,94-98: floor((w - min) / res), float64
 * IEEE division, result as int64. */
int icpmi_world_to_grid(const double* w, int64_t n, double min_w, double resolution,
                        int64_t* out, void* stream);

/* Cells of _bresenham(x0,y0,x1,y1), mapping.py:68-89 (start included, end
 * excluded), for n_seg segments {x0,y0,x1,y1} (int32).  Segment s writes its
 * max(|dx|,|dy|) cells (x,y int32 pairs) at out_cells[2*cell_off[s] ...]. This
 * is the device function the ray-cast kernel walks; exposed for parity tests
 * and for the `_bresenham` method of the drop-in class. */
int icpmi_bresenham_cells(const int32_t* segs, const int64_t* cell_off, int32_t n_seg,
                          int32_t* out_cells, void* stream);

/* update_scan, mapping.py:103-141, for n_scans consecutive scans (n_scans = 1
 * is the reference call; more is the _rebuild_map replay of slam.py:271-277).
 * One scan with a cell box from the caller (icpmi_grid_update_scans_box) and no
 * full_clip is ONE launch: workgroups own rectangles of the box, count in LDS and
 * apply the replay and the clip to their own cells; the counter workspace is not
 * touched.
 * log_odds: float32 (ny, nx), updated in place.  Scan s has origin
 * origins[2s..2s+1] and hits rows [hit_off_host[s], hit_off_host[s+1]) of
 * hits (world frame, float64).  Per cell the result equals the reference's
 * sequence: H adds of l_hit, then M adds of l_miss, each rounded to float32
 * from a float64 sum, then one clip to [lo, hi] per scan.
 * counts: workspace of icpmi_grid_workspace_bytes(ny, nx) bytes — room for four grids of uint32 counters plus
 * bounding-box slots and the cell boxes of the scans of two groups — zeroed once by the caller before first use
 * and owned by this grid afterwards.  With
 * n_scans > 1, consecutive scans are counted in ONE launch, each into its own counter region, and finalised
 * together in scan order per cell (so the result is the sequential one bit for bit); the count pass of a group
 * shares its launch with the finalise pass of the previous group (the other set of regions).  A region covers the
 * box the rays stay in (icpmi_grid_update_scans_box; the whole grid otherwise), so a group holds up to 32 scans
 * when the box is at most 1/16 of the grid and at least 2 always: a replay of S scans is about S/32 + 1 launches.
 * Every call leaves the four counter grids — the first 16 * ny * nx bytes — all zero again; the bounding-box slots and the
 * scans' cell boxes behind them keep what the call's last group left there.  No call depends on them: a call clears the
 * slots unless it is the one-scan call with a box, which does not read them, and writes the boxes before it reads them.
 * A call that is refused (icpmi_grid_update_plan lists the reasons) is refused before anything is started.
 * scan_seq: ignored (kept for binary compatibility; calls are independent).
 * full_clip != 0 clips every cell of the grid on the first scan (needed only
 * when cells may lie outside [lo, hi] beforehand).
 * Coordinates far from the grid (the same rule for this entry, _band and _box, and for every pass): the cell index of
 * a coordinate is q = floor((w - min) / resolution), the IEEE quotient.  A scan whose origin has a q that is NaN or
 * not below 1e300 in magnitude adds nothing; a beam whose hit has one is dropped, as a non-finite coordinate is (the
 * reference raises on both).  Any other q beyond +-2^29 is replaced by +-2^29: the beam is the Bresenham line between
 * the CLAMPED cells, which is not the direction of the world line, and its length is at most 2^30 cells.  The
 * reference walks the unclamped line; the two agree for every coordinate within 2^29 cells of the grid's minimum. */
size_t icpmi_grid_workspace_bytes(int32_t ny, int32_t nx);
int icpmi_grid_update_scans(float* log_odds, void* counts, int32_t ny, int32_t nx,
                            double min_x, double min_y, double resolution,
                            const double* origins, const double* hits, const int32_t* hit_off_host,
                            int32_t n_scans, double l_hit, double l_miss, double lo, double hi,
                            int64_t scan_seq, int32_t full_clip, void* stream);

/* The same update restricted to the rows [row_begin, row_end) of the grid: one
 * rank's band of a sharded map replay (the replay of slam.py:271-277 over a
 * long history).  Cells are independent and each keeps its scan
 * order, so replaying every scan on every rank with disjoint bands and then
 * gathering the bands gives the same grid bit for bit.  log_odds and counts
 * are FULL-size (ny x nx) buffers; only rows of the band are read or written,
 * rays are clipped to the band analytically (no steps are walked outside it),
 * and full_clip clips the band only.  Coordinates beyond +-2^29 cells or with a
 * quotient >= 1e300: as stated for icpmi_grid_update_scans. */
int icpmi_grid_update_scans_band(float* log_odds, void* counts, int32_t ny, int32_t nx,
                                 double min_x, double min_y, double resolution,
                                 const double* origins, const double* hits, const int32_t* hit_off_host,
                                 int32_t n_scans, double l_hit, double l_miss, double lo, double hi,
                                 int64_t scan_seq, int32_t full_clip, int32_t row_begin, int32_t row_end,
                                 void* stream);

/* The same with a promise about where the rays lie: box_host = {x0, y0, x1, y1}, inclusive CELL bounds (host
 * memory) that contain the origin cell and every hit cell of every scan of the call (Bresenham stays inside the
 * rectangle spanned by its end points; cells outside the grid need not be covered), or NULL for "anywhere".
 * Counters are then kept for that box only, which is what lets 32 scans be counted per launch inside a workspace
 * of four grids (the Python class computes the box from the scans it is given), and a replay of several scans is
 * counted tile by tile in LDS instead of with one device atomic per beam and cell (same counts, ~1.4x the rate).
 * A ray cell outside the box is not counted: the box is a contract, not a clip the reference has.
 * Coordinates beyond +-2^29 cells or with a quotient >= 1e300: as stated for icpmi_grid_update_scans — the box holds the
 * CLAMPED cells (so its bounds lie in [-2^29 - 1, 2^29 + 1]). */
int icpmi_grid_update_scans_box(float* log_odds, void* counts, int32_t ny, int32_t nx,
                                double min_x, double min_y, double resolution,
                                const double* origins, const double* hits, const int32_t* hit_off_host,
                                int32_t n_scans, double l_hit, double l_miss, double lo, double hi,
                                int64_t scan_seq, int32_t full_clip, int32_t row_begin, int32_t row_end,
                                const int32_t* box_host, void* stream);

/* What icpmi_grid_update_scans_box starts for its HOST arguments (have_hits: whether `hits` is non-null), under the
 * RAYCAST option as it stands — no HIP call, no launch, no device pointer.  The refusals are that entry's: both ask
 * one check, which that entry makes before its first launch, so a refused call has touched neither the grid nor the
 * workspace (ICPMI_ERR_ARG: a null out or hit_off_host, ny, nx <= 0 or > 2^29, n_scans < 0, a band outside [0, ny], a
 * resolution that is not > 0, a negative beam count in any scan, beams without hits).  An empty band starts nothing:
 * ICPMI_OK and a plan of zeros (ICPMI_RC_PASS_NONE).
 *   pass        the counting pass of the scans that fit a 16-bit counter: one launch in which a workgroup owns a
 *               rectangle of cells (OWNER), counters of a 64 x 64 tile in LDS (TILES), an atomic per (wave, cell) on
 *               the scan's counter region (ATOMIC)
 *   group_max   scans counted per launch at most;  tiles_x, tiles_y: 64 x 64 tiles of the window (grid or band cut to
 *               the box);  live_scans: scans with beams
 *   wide        1: a scan has more than 65 535 beams and goes through the two-round route (hits, then misses, on the
 *               atomic counters) whatever `pass` says about the others
 *   rounds      what the call issues one after the other: groups of up to group_max scans, and wide scans one each
 *               (the owner pass: 1; no scan with beams: 0)
 *   launches    kernel launches of those rounds (the memset of the box slots is none): a group is one launch that also
 *               finalises the group before it, plus one for its scan boxes (TILES, live_scans > 1) when no group went
 *               before and one to finalise it when no group follows; a wide scan is four */
#define ICPMI_RC_PASS_NONE 0
#define ICPMI_RC_PASS_OWNER 1
#define ICPMI_RC_PASS_TILES 2
#define ICPMI_RC_PASS_ATOMIC 3
typedef struct icpmi_grid_plan {
    int32_t pass, group_max, tiles_x, tiles_y, live_scans, wide, rounds, launches;
} icpmi_grid_plan;
int icpmi_grid_update_plan(int32_t ny, int32_t nx, double resolution, const int32_t* hit_off_host, int32_t n_scans,
                           int32_t have_hits, int32_t full_clip, int32_t row_begin, int32_t row_end,
                           const int32_t* box_host, icpmi_grid_plan* out);

/* ---- correlative scan-to-map matching: the grid of utilities/mapping.py read back as a target -----------------------
 * The reference registers a scan against a cloud only (slam.py:53-98, 111-183).  These entries score a scan against the
 * occupancy grid itself over a window of rotations and whole-cell shifts.  After the cells are formed everything is
 * integer, so the result does not depend on how the work is split or on the order of the integer atomics.
 *
 * icpmi_grid_score_field: field[iy][ix] = clip(rint(log_odds[iy][ix] * 2^shift_bits), -32767, 32767) as int16 — the
 * product in float32 (a power of two: exact), rint half to even, NaN -> 0, +-inf and anything beyond the clamp saturate.
 * shift_bits in [0, ICPMI_GM_MAX_SHIFT_BITS] is the caller's choice (the Python layer takes the largest one with
 * max(|log_odds_min|, |log_odds_max|) * 2^shift_bits <= 32767: 12 for the default +-5).  Both pointers 16-byte aligned
 * (vector loads and stores); ny * nx == 0: no launch, ICPMI_OK.
 *
 * icpmi_grid_match_batch: pair b names cloud pair_cloud[b] of the set (pts, off_dev, cnt_dev: 2-D rows; cnt_dev NULL =
 * every cloud full), a translation pair_t[2b .. 2b+1] and n_angles rotations cos_sin[(b * n_angles + a) * 2 .. + 1] =
 * (cos, sin) — the caller's own doubles.  With W = window and S = 2W + 1, for angle a and source row (x, y), float64,
 * evaluated exactly as written, every operation rounded on its own (no fused multiply-add):
 *   wx = (c * x - s * y) + tx,  wy = (s * x + c * y) + ty,
 *   cx = floor((wx - min_x) / resolution),  cy = floor((wy - min_y) / resolution)   (IEEE divide, mapping.py:94-98);
 * a row whose wx or wy is not finite, or whose cx or cy lies outside [-2^29, 2^29], has no cell and adds nothing.
 *   score[b][a][j][i] = sum over the rows with a cell of field[cy + j - W][cx + i - W],
 * a cell outside [0, ny) x [0, nx) counting 0, as unknown space does.  int32: at most ICPMI_GM_MAX_ROWS rows of at most
 * 32767 each cannot overflow.  The winner is the first maximum of score[b] over (a, j, i) in C order (np.argmax); the
 * host forms the pose from it: translation (tx + (i - W) * resolution, ty + (j - W) * resolution), rotation the
 * caller's (cos, sin) at a.
 * out_records [n_pairs][ICPMI_GMREC_INTS] int32, slots ICPMI_GMREC_*: status, rows with a cell at the winning angle,
 * the winner's flat index (a * S + j) * S + i, a, j, i, its score, and the score of the centre candidate
 * (centre_angle, W, W) — 0 when centre_angle < 0.  Status ICPMI_GM_ST_OK; ICPMI_GM_ST_EMPTY: no row has a cell at any
 * angle (every score 0, index 0); ICPMI_GM_ST_CAPACITY: the cloud's device count is negative (the voxel filter's
 * overflow mark) or exceeds the cloud's own rows or ICPMI_GM_MAX_ROWS (not read: every score 0).
 * out_scores (optional): receives the whole volume [n_pairs][n_angles][S][S] int32 (it is then accumulated there
 * instead of in the workspace).  workspace: icpmi_grid_match_workspace_bytes(n_pairs, n_angles, window) bytes (0 for a
 * negative argument); the call zeroes what it accumulates into, so a workspace is reusable as it is.
 * Every refusal is decided on the host before any launch.  off_host mirrors off_dev and pair_cloud_host mirrors
 * pair_cloud (both required: they size the launch); a pair's cloud outside [0, n_clouds), a null pointer, a grid with
 * ny * nx >= 2^31, a non-positive or non-finite resolution, centre_angle >= n_angles, n_angles < 1: ICPMI_ERR_ARG;
 * window > ICPMI_GM_MAX_WINDOW, n_angles > ICPMI_GM_MAX_ANGLES or a pair's cloud above ICPMI_GM_MAX_ROWS rows by
 * off_host: ICPMI_ERR_UNSUPPORTED; a short workspace: ICPMI_ERR_WORKSPACE.  n_pairs == 0: no launch, ICPMI_OK.
 * Launches: two memsets, one scoring launch — a workgroup of ICPMI_GM_THREADS threads per (pair, angle, chunk of
 * ICPMI_GM_CHUNK_ROWS rows), ending in one int32 atomicAdd per shift — and one arg-max workgroup per pair. */
#define ICPMI_GM_MAX_WINDOW 31
#define ICPMI_GM_MAX_ANGLES 1024
#define ICPMI_GM_MAX_ROWS 65535
#define ICPMI_GM_MAX_SHIFT_BITS 14
#define ICPMI_GM_THREADS 256
#define ICPMI_GM_CHUNK_ROWS 256
#define ICPMI_GM_ST_OK 0
#define ICPMI_GM_ST_EMPTY 1
#define ICPMI_GM_ST_CAPACITY 2
#define ICPMI_GMREC_INTS 8
#define ICPMI_GMREC_STATUS 0
#define ICPMI_GMREC_ROWS 1
#define ICPMI_GMREC_INDEX 2
#define ICPMI_GMREC_A 3
#define ICPMI_GMREC_J 4
#define ICPMI_GMREC_I 5
#define ICPMI_GMREC_SCORE 6
#define ICPMI_GMREC_CENTRE 7
int icpmi_grid_score_field(const float* log_odds, int32_t ny, int32_t nx, int32_t shift_bits, int16_t* field,
                           void* stream);
size_t icpmi_grid_match_workspace_bytes(int32_t n_pairs, int32_t n_angles, int32_t window);
int icpmi_grid_match_batch(const int16_t* field, int32_t ny, int32_t nx, double min_x, double min_y, double resolution,
                           const double* pts, const int32_t* off_dev, const int32_t* off_host, const int32_t* cnt_dev,
                           int32_t n_clouds, const int32_t* pair_cloud, const int32_t* pair_cloud_host,
                           int32_t n_pairs, const double* pair_t, const double* cos_sin, int32_t n_angles,
                           int32_t window, int32_t centre_angle, int32_t* out_records, int32_t* out_scores,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same search over a wide window: bounded blocks, the exhaustive winner ---------------------------------------
 * icpmi_grid_search_batch returns what icpmi_grid_match_batch would over a window of up to ICPMI_GMW_MAX_WINDOW cells,
 * without forming the volume.  Fields, cells, scores, clouds, cnt_dev, the statuses and the record's first eight int32 are
 * icpmi_grid_match_batch's, unchanged; n_angles may go up to ICPMI_GMW_MAX_ANGLES, and n_angles * S^2 >= 2^31 (S = 2W + 1)
 * is refused.  The winner is the first maximum over (a, j, i) in C order of the full exhaustive volume.
 *
 * icpmi_grid_bound_field: with D = block in {4, 8, 16} and q~ the int16 field extended by 0 outside the grid,
 *   M(y, x) = max over 0 <= dy, dx < D of q~(y + dy, x + dx)   for y in [-(D - 1), ny), x in [-(D - 1), nx),
 * stored as out[y + D - 1][x + D - 1], int16 of shape (ny + D - 1, nx + D - 1); M is 0 outside that domain.  Both pointers
 * 16-byte aligned; ny * nx == 0: no launch, ICPMI_OK; (ny + D - 1) * (nx + D - 1) >= 2^31 or another block: ICPMI_ERR_ARG.
 *
 * Blocks: NB = ceil(S / D) per axis; block (a, J, I) holds the shifts j in [J * D, min((J + 1) * D, S)) and i likewise.
 *   U[b][a][J][I] = sum over the rows with a cell at angle a of M(cy + J * D - W, cx + I * D - W),
 * int32, no smaller than any score of the block.  The search, all on the caller's stream without a host synchronisation:
 * (1) U for every block; (2) for each angle the first block in C order of maximal U is scored exactly, and best0[b] is the
 * largest exact score over these n_angles seed blocks; (3) every block with U >= best0 survives (>=: a block whose bound
 * equals best0 may hold an equal score at a lower index) and is scored exactly, shifts with j >= S or i >= S ignored;
 * (4) the winner is the largest exact score, on equal scores the lower flat index a * S^2 + j * S + i.  Every flat index that
 * attains the true maximum m lies in a block with U >= m >= best0, which survives: the record equals the exhaustive one.
 * out_records [n_pairs][ICPMI_GMW_REC_INTS] int32: slots 0-7 are ICPMI_GMREC_* (slot 7, the exact score of (centre_angle,
 * W, W), is always evaluated, pruned or not; 0 when centre_angle < 0); ICPMI_GMW_REC_BLOCKS: n_angles * NB^2;
 * ICPMI_GMW_REC_SURVIVORS: blocks with U >= best0; ICPMI_GMW_REC_SEED: best0; ICPMI_GMW_REC_MAX_BOUND: the largest U.  All
 * twelve are functions of the inputs alone.  An EMPTY or CAPACITY pair has every U and score 0: every block survives, index 0.
 * bound: icpmi_grid_bound_field's output for `field` and `block`.  out_bounds (optional): receives U, [n_pairs][n_angles]
 * [NB][NB] int32 (accumulated there instead of in the workspace).  workspace: icpmi_grid_search_workspace_bytes(n_pairs,
 * n_angles, window, block) bytes (0 for a negative argument or another block) — two int32 per block, and per (pair, angle)
 * and per pair a few words; the call zeroes what it accumulates into, so a workspace is reusable as it is.
 * Refusals, on the host before any launch, are icpmi_grid_match_batch's, with: a block outside {4, 8, 16}: ICPMI_ERR_ARG;
 * window > ICPMI_GMW_MAX_WINDOW, n_angles > ICPMI_GMW_MAX_ANGLES, n_angles * S^2 >= 2^31 or n_pairs * n_angles * NB^2 >=
 * 2^31: ICPMI_ERR_UNSUPPORTED.  Launches: two memsets; the bound pass (gm_score_kernel's walk over M, lanes owning blocks);
 * one arg-max workgroup per (pair, angle); the seeds' exact scores, one workgroup per seed block over all rows of its cloud,
 * merged by one 64-bit atomicMax on (score + 2^31) << 32 | (0xFFFFFFFF - flat); a compaction of the survivors; their exact
 * scores by a fixed grid of at most ICPMI_GMW_SCORE_GROUPS workgroups striding over the device-side count; the records. */
#define ICPMI_GMW_MAX_WINDOW 255
#define ICPMI_GMW_MAX_ANGLES 16384
#define ICPMI_GMW_SCORE_GROUPS 2048
#define ICPMI_GMW_REC_INTS 12
#define ICPMI_GMW_REC_BLOCKS 8
#define ICPMI_GMW_REC_SURVIVORS 9
#define ICPMI_GMW_REC_SEED 10
#define ICPMI_GMW_REC_MAX_BOUND 11
int icpmi_grid_bound_field(const int16_t* field, int32_t ny, int32_t nx, int32_t block, int16_t* out, void* stream);
size_t icpmi_grid_search_workspace_bytes(int32_t n_pairs, int32_t n_angles, int32_t window, int32_t block);
int icpmi_grid_search_batch(const int16_t* field, const int16_t* bound, int32_t ny, int32_t nx, double min_x, double min_y,
                            double resolution, const double* pts, const int32_t* off_dev, const int32_t* off_host,
                            const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                            const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                            int32_t n_angles, int32_t window, int32_t block, int32_t centre_angle, int32_t* out_records,
                            int32_t* out_bounds, void* workspace, size_t workspace_bytes, void* stream);

/* ---- moments of a match: the sub-cell pose and the covariance the score volume holds ---------------------------------
 * icpmi_grid_match_batch returns the first maximum of an integer volume: one whole cell, one whole angle step, and no
 * word on how well the map constrained it.  icpmi_grid_match_moments reads that volume once more and leaves the weighted
 * moments of the candidates about the winner (Olson's covariance of a correlative match), in integers: twelve int64 per
 * pair that do not depend on how the candidates are split or in which order they are added.
 *
 * volume: device, [n_pairs][n_angles][S][S] int32 contiguous, S = 2 * window + 1 — what icpmi_grid_match_batch leaves in
 * out_scores.  records: device, [n_pairs][ICPMI_GMREC_INTS] int32 as icpmi_grid_match_batch wrote them earlier on the same
 * stream (nothing synchronises); slots A, J, I lie inside the volume.  moments: device, [n_pairs][ICPMI_GMOM_INTS] int64,
 * 8-byte aligned; the call zeroes it itself (a memset), so a buffer is reusable as it is.
 *
 * Per pair, in int64: (a*, j*, i*, best, rows) = slots A, J, I, SCORE, ROWS of its record, h = max(1, rows * half_step),
 * and for every candidate (a, j, i) with score s
 *   d = max(0, best - s),  u = floor(8 * d / h),  e = u >> 3,  f = u & 7,  w = e > 20 ? 0 : T[f] >> e,
 *   T = {1048576, 961548, 881744, 808563, 741455, 679917, 623487, 571740} = rint(2^20 * 2^(-f / 8))
 * (fractional parts .43 .80 .63 .20 .42 .02 .12: none near a tie).  A candidate h below the best counts half, in eight
 * sub-steps per halving; half_step is the score drop per scored row, in field units (2^shift_bits per unit of log-odds),
 * that halves the weight — scaled by the rows at the winning angle, so the setting does not depend on the cloud's size.
 * With da = a - a*, dj = j - j*, di = i - i* the slots ICPMI_GMOM_* are: W = sum w; A, J, I = sum w * da, w * dj, w * di;
 * AA, AJ, AI, JJ, JI, II = sum w * da^2, w * da * dj, w * da * di, w * dj^2, w * dj * di, w * di^2; SUPPORT = the number of
 * candidates with w > 0; EDGE = sum w over the candidates on a face of the volume (a in {0, n_angles - 1} when
 * n_angles > 1, or j or i in {0, S - 1} when S > 1): a large share of W there says the window cut the distribution.
 * Headroom: at the capacities (1 024 angles, window 31, every score equal, the winner at index 0) the largest slot is
 * AA = 1 487 384 306 207 686 656 < 2^61, and 8 * d <= 2^35: no sum overflows.
 * A pair whose record says ICPMI_GM_ST_CAPACITY gets twelve zeros.  ICPMI_GM_ST_EMPTY goes through the rule: every score
 * is 0, the winner index 0, every weight 2^20 — the uniform distribution of "no information".
 * Refusals, on the host before anything is enqueued: n_pairs == 0: ICPMI_OK, nothing done; a null volume, records or
 * moments, n_pairs < 0, n_angles < 1, window < 0, half_step outside [1, ICPMI_GMOM_MAX_HALF_STEP] or moments not 8-byte
 * aligned: ICPMI_ERR_ARG; window > ICPMI_GM_MAX_WINDOW or n_angles > ICPMI_GM_MAX_ANGLES: ICPMI_ERR_UNSUPPORTED.
 * Launches: one memset and gm_moments_kernel — workgroups of ICPMI_GM_THREADS threads over (chunk of candidates, pair),
 * each ending in one 64-bit integer atomicAdd per non-zero slot. */
#define ICPMI_GMOM_INTS 12
#define ICPMI_GMOM_W 0
#define ICPMI_GMOM_A 1
#define ICPMI_GMOM_J 2
#define ICPMI_GMOM_I 3
#define ICPMI_GMOM_AA 4
#define ICPMI_GMOM_AJ 5
#define ICPMI_GMOM_AI 6
#define ICPMI_GMOM_JJ 7
#define ICPMI_GMOM_JI 8
#define ICPMI_GMOM_II 9
#define ICPMI_GMOM_SUPPORT 10
#define ICPMI_GMOM_EDGE 11
#define ICPMI_GMOM_WEIGHT_BITS 20
#define ICPMI_GMOM_MAX_HALF_STEP 32767
int icpmi_grid_match_moments(const int32_t* volume, const int32_t* records, int32_t n_pairs, int32_t n_angles,
                             int32_t window, int32_t half_step, int64_t* moments, void* stream);

/* ---- likelihood field: the exact truncated distance transform of the occupied cells, mapped to a score ---------------
 * The matchers above read the raw field: a hit scores only where earlier hits raised that very cell.  This entry makes the
 * field they read instead while a wall is one cell wide: every cell scored by its distance to the nearest occupied cell.
 * The result is an int16 (ny, nx) field like icpmi_grid_score_field's, so every matching entry, icpmi_grid_bound_field and
 * the moments take it unchanged.  All of it is integer: the outputs are functions of the inputs alone, to the bit.
 *
 * field: device, int16 [ny][nx], what icpmi_grid_score_field wrote.  A cell is occupied iff field[y][x] >= threshold (any
 * int32); cells outside the grid are never occupied.  radius R in [0, ICPMI_LF_MAX_RADIUS], in cells.
 * d2_out (device, int16 [ny][nx], optional): the smallest (y - y')^2 + (x - x')^2 over the occupied cells (y', x') where
 * that is at most R^2, and the sentinel R^2 + 1 everywhere else — exact.  (Evaluated in two passes: g(y, x) = the
 * distance along the column to the nearest occupied cell within R; then the minimum over |dx| <= R of dx^2 + g(y, x + dx)^2;
 * whatever exceeds R^2 becomes the sentinel.  A cell within R^2 has |dx|, |dy| <= R, so the two windows lose nothing.)
 * lf_out (device, int16 [ny][nx], optional): table[d2] where d2 <= R^2; beyond the radius min(field, 0) when keep_free != 0
 * — the raw field's penalty for a hit in observed free space stays — and 0 otherwise.
 * table: R^2 + 1 int16 on the HOST, indexed by the squared distance (the Python layer: a Gaussian of the distance with the
 * map's clamp as its peak).  It is read and checked before anything is enqueued and copied into the workspace on the
 * stream, so the caller may free it when the call returns.  A table that holds -32768 is refused: every matcher's int32
 * score bound rests on |field| <= 32767.  NULL is allowed only when lf_out is NULL.
 * workspace: device, icpmi_grid_likelihood_workspace_bytes(ny, nx, radius) bytes (the device copy of the table, 256-byte
 * granules; 0 for a refused argument); may be NULL when lf_out is NULL.
 * Refusals, on the host before anything is enqueued: ny <= 0 or nx <= 0, ny * nx >= 2^31, field NULL, both outputs NULL,
 * lf_out without a table, a pointer that is not 16-byte aligned (vector loads and stores), a table that holds -32768:
 * ICPMI_ERR_ARG; a radius outside [0, ICPMI_LF_MAX_RADIUS] or more than 65 535 tile rows: ICPMI_ERR_UNSUPPORTED; lf_out
 * with a workspace that is NULL or short: ICPMI_ERR_WORKSPACE.
 * Launches: one copy of the table (only with lf_out) and lf_field_kernel — a workgroup of ICPMI_GM_THREADS threads per tile
 * of ICPMI_LF_TILE_Y x ICPMI_LF_TILE_X outputs.  It stages the occupancy of the tile and a halo of R as bits in LDS, runs
 * both passes there and writes each output once: 2 bytes read and 2 or 4 written per cell, and the halo from L2. */
#define ICPMI_LF_MAX_RADIUS 64
#define ICPMI_LF_TILE_X 128
#define ICPMI_LF_TILE_Y 64
size_t icpmi_grid_likelihood_workspace_bytes(int32_t ny, int32_t nx, int32_t radius);
int icpmi_grid_likelihood_field(const int16_t* field, int32_t ny, int32_t nx, int32_t threshold, int32_t radius,
                                const int16_t* table, int32_t keep_free, int16_t* d2_out, int16_t* lf_out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- the cast: the grid read back as ranges (no counterpart in the reference) ------------------------------------------
 * icpmi_grid_update_scans writes along rays; these entries read along them: from a cell, towards a cell, where is the first
 * wall, and is there unexplored space before it?  The cells of a ray are exactly the cells the update would lower, plus the
 * end cell, so the map's writer and its reader agree cell for cell.  Behind the end cells everything is integer: a record
 * is a function of the inputs alone, to the bit.
 *
 * Field and cells.  field: device, int16 [ny][nx] — icpmi_grid_score_field's, or any other such as a likelihood field.  A
 * cell inside the grid is OCCUPIED iff field[y][x] >= occ_threshold (any int32; icpmi_grid_likelihood_field's rule) and
 * UNKNOWN iff field[y][x] == 0.  A cell outside [0, ny) x [0, nx) is neither.
 *
 * Segments and steps.  A segment is (x0, y0, x1, y1) in cells, int32, each within +-2^29 (a value beyond is replaced by
 * +-2^29, as icpmi_grid_update_scans clamps).  With dx = |x1 - x0|, dy = |y1 - y0| its steps are k = 0 .. K, K = max(dx, dy).
 * Step k < K is the k-th cell of _bresenham, mapping.py:68-89 (icpmi_bresenham_cells); step K is the end cell (x1, y1), which
 * that list leaves out.  In closed form, x the major axis when dx >= dy (y otherwise), sm and sn the signs of the deltas
 * (-1 for a delta of 0), dmaj = K and dmin the other delta: step k lies at major = m0 + sm * k and minor = n0 + sn *
 * floor((2 * k * dmin + dmaj - 1) / (2 * dmaj)); K = 0 has the one step (x0, y0).
 *
 * Record: four int32 per ray, slots ICPMI_GC_*, written as one 16-byte store: [k_hit, x_hit, y_hit, k_unknown].
 * k_hit: the first step whose cell is occupied, (x_hit, y_hit) that cell; without one k_hit = ICPMI_GC_NONE and (x_hit,
 * y_hit) = (x1, y1).  k_unknown: the first step BEFORE k_hit whose cell is unknown — without a hit, among all K + 1 steps —
 * or ICPMI_GC_NONE.  A ray without cells (below): [ICPMI_GC_NO_CELLS, 0, 0, ICPMI_GC_NONE].
 *
 * icpmi_grid_occupancy_planes packs a field into the two bit planes the casts read: `planes` (device, 16-byte aligned,
 * icpmi_grid_occupancy_planes_bytes(ny, nx) bytes; 0 for a refused grid) holds uint32 [ny][wpr] for "occupied", then, from
 * the next multiple of 256 bytes on, the same for "unknown"; wpr = ceil(nx / 32), bit x & 31 of word x >> 5 of row y is cell
 * (y, x), and the pad bits of a row's last word are clear in both.  A caller may keep planes across calls, as a field is
 * kept: a cast against kept planes reads the map as it was when they were made, whatever has been applied since, and
 * ignores `field` and `occ_threshold`.
 *
 * icpmi_grid_cast_segments: segs device, int32 [n][4], 16-byte aligned; out_records device, int32 [n][ICPMI_GC_INTS], 16-byte
 * aligned.  planes: what icpmi_grid_occupancy_planes wrote for this ny, nx — or NULL, and the call packs `field` with
 * occ_threshold into `workspace` (device, 16-byte aligned, icpmi_grid_occupancy_planes_bytes(ny, nx) bytes) first.
 *
 * icpmi_grid_cast_rays: ray (p, b) of n_poses x n_beams leaves pose p — poses[2p .. 2p+1] = (px, py), pose_cs[2p .. 2p+1] =
 * (ct, st) = (cos, sin) of its heading — along beam b, beam_cs[2b .. 2b+1] = (ca, sa) = (cos, sin) of the bearing in the
 * sensor frame: the caller's own doubles, as icpmi_grid_match_batch takes its cos_sin (all device).  Float64, evaluated
 * exactly as written, every operation rounded on its own (no fused multiply-add):
 *   c = ct * ca - st * sa,  s = st * ca + ct * sa,  ex = px + reach * c,  ey = py + reach * s      (reach in metres)
 *   x0 = cell(px, min_x), y0 = cell(py, min_y), x1 = cell(ex, min_x), y1 = cell(ey, min_y),
 *   cell(w, min) = floor((w - min) / resolution), the IEEE quotient (world_to_cell, mapping.py:57-59), clamped to +-2^29.
 * A ray one of whose four quotients is NaN or not below 1e300 in magnitude — a pose or an end point that is not finite —
 * has no cells.  out_records: device, int32 [n_poses][n_beams][ICPMI_GC_INTS].  field, planes, workspace: as above.
 *
 * Refusals, on the host before any launch: ny or nx negative or above 2^29, ny * nx >= 2^31, n, n_poses or n_beams
 * negative, a resolution or reach that is not positive and finite, a null or misaligned pointer that the call would use:
 * ICPMI_ERR_ARG; n >= 2^29 or n_poses * n_beams >= 2^29: ICPMI_ERR_UNSUPPORTED; planes NULL and a workspace that is NULL,
 * misaligned or short (for icpmi_grid_occupancy_planes: planes_bytes short): ICPMI_ERR_WORKSPACE.  No ray: no launch,
 * ICPMI_OK.  ny * nx == 0: nothing is packed (no planes launch; planes and workspace may be NULL) and every ray that has
 * cells gets the record of "no hit".  There is no limit on a ray's length: only the steps inside the grid can matter, and
 * their range is found in closed form.
 * Launches: gc_planes_kernel (only when the call packs: a lane per word of a plane, 2 bytes read and 2 bits written per
 * cell) and gc_cast_kernel — workgroups of ICPMI_GC_THREADS threads, one lane per ray, a wave 64 consecutive beams of one
 * pose.  A lane cuts its steps to the grid, walks them bit by bit with the words of a few steps loaded together, and leaves
 * at its hit. */
#define ICPMI_GC_INTS 4
#define ICPMI_GC_K_HIT 0
#define ICPMI_GC_X_HIT 1
#define ICPMI_GC_Y_HIT 2
#define ICPMI_GC_K_UNKNOWN 3
#define ICPMI_GC_NONE (-1)        /* k_hit: nothing occupied on the ray; k_unknown: nothing unknown before the hit */
#define ICPMI_GC_NO_CELLS (-2)    /* k_hit of a ray whose pose or end point has no cell */
#define ICPMI_GC_THREADS 256
size_t icpmi_grid_occupancy_planes_bytes(int32_t ny, int32_t nx);
int icpmi_grid_occupancy_planes(const int16_t* field, int32_t ny, int32_t nx, int32_t occ_threshold, void* planes,
                                size_t planes_bytes, void* stream);
int icpmi_grid_cast_segments(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                             const int32_t* segs, int32_t n, int32_t* out_records, void* workspace, size_t workspace_bytes,
                             void* stream);
int icpmi_grid_cast_rays(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                         double min_x, double min_y, double resolution, const double* poses, const double* pose_cs,
                         int32_t n_poses, const double* beam_cs, int32_t n_beams, double reach, int32_t* out_records,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- the check: measured scans held against the map along their beams (no counterpart in the reference) ----------------
 * The matchers score the map under a scan's end points; the cast reads the map back as ranges.  icpmi_grid_check_batch asks
 * what a loop-closure gate or a particle filter needs: does this scan, at this pose, contradict the free space and the
 * walls the map already holds?  Every measured beam is walked from the pose's cell to the cell of its own hit — exactly the
 * cells icpmi_grid_update_scans would touch for that beam — and classified; the classes are counted per pair on the device
 * and eight integers per pair come back.  After the cells are formed everything is integer, and the counts are sums of int32
 * atomics of at most ICPMI_GM_MAX_ROWS rows: a record is a function of the inputs alone, to the bit.
 *
 * The map: field + occ_threshold + workspace, or kept planes, exactly as icpmi_grid_cast_segments takes them (planes given:
 * field, occ_threshold and workspace are ignored; planes NULL: the call packs `field` into `workspace` first).
 * The scans: a cloud set and pairs exactly as icpmi_grid_match_batch takes them — pts (here 16-byte aligned: a row is one
 * load), off_dev, off_host, cnt_dev (NULL = every cloud full), n_clouds, pair_cloud, pair_cloud_host, n_pairs, pair_t — and
 * cos_sin [n_pairs][2], one rotation (cos, sin) per pair.  int32 tolerance >= 0, in steps.
 *
 * Cells of a row.  Row (x, y) of pair b has its end cell (cx, cy) by icpmi_grid_match_batch's expressions, float64, every
 * operation rounded on its own:  wx = (c * x - s * y) + tx,  wy = (s * x + c * y) + ty,  cx = floor((wx - min_x) /
 * resolution),  cy = floor((wy - min_y) / resolution).  The row has no cell if wx or wy is not finite or if cx or cy lies
 * outside [-2^29, 2^29].  The origin cell (ox, oy) comes from (tx, ty) by the same rule; if the origin has no cell, no row of
 * that pair has cells.
 *
 * Classes of a row.  Let [k_hit, ., ., k_unknown] be the cast's record of the segment (ox, oy) -> (cx, cy): steps 0 .. K, the
 * end cell included, K = max(|cx - ox|, |cy - oy|).  A row with cells falls in exactly one class:
 *   ICPMI_GK_CLASS_CONFIRMED   k_hit >= 0 and k_hit >= K - tolerance: the beam ends where the map has a wall;
 *   ICPMI_GK_CLASS_VIOLATED    k_hit >= 0 and k_hit <  K - tolerance: it returned from behind something the map holds occupied;
 *   ICPMI_GK_CLASS_IN_FREE     no hit, the end cell inside the grid with its unknown bit clear: a return from observed free space;
 *   ICPMI_GK_CLASS_UNEXPLORED  no hit, the end cell outside the grid or unknown.
 * (K <= 2^30 and tolerance <= 2^30: K - tolerance does not overflow.)  The tolerance exists because a noisy return lands a
 * cell behind the first occupied layer of a mapped wall.
 *
 * out_records: device, int32 [n_pairs][ICPMI_GK_INTS], slots ICPMI_GK_REC_*: STATUS, ROWS (the rows with cells), the four
 * class counts (slot ICPMI_GK_REC_CONFIRMED + class; they sum to ROWS), THROUGH_UNKNOWN (the rows with cells whose k_unknown
 * >= 0) and a 0.  Status ICPMI_GK_ST_OK; ICPMI_GK_ST_EMPTY: no row has a cell; ICPMI_GK_ST_CAPACITY: icpmi_grid_match_batch's
 * rule for cnt_dev (negative, beyond the cloud's own rows or beyond ICPMI_GM_MAX_ROWS) — nothing is read, every count 0.
 * out_rows (optional, NULL: off): device, 16-byte aligned, int32 [n_pairs][row_stride][ICPMI_GK_ROW_INTS], one 16-byte
 * store per row: [class, k_hit, K, k_unknown]; a row without cells is [ICPMI_GK_NO_CELLS, 0, 0, -1].  row_stride is the
 * caller's, at least every named cloud's row count by off_host.  Rows at or behind a cloud's count are not written.
 *
 * Refusals, on the host before anything is enqueued.  n_pairs == 0: ICPMI_OK, nothing done.  ICPMI_ERR_ARG: n_pairs or
 * n_clouds negative; off_host or pair_cloud_host NULL; a pair's cloud outside [0, n_clouds) or with a negative row count; a
 * grid the casts refuse (ny or nx negative or above 2^29, ny * nx >= 2^31); a resolution that is not positive and finite,
 * a min_x or min_y that is not finite; tolerance < 0 or > 2^30; pts, off_dev, pair_cloud, pair_t, cos_sin or out_records
 * NULL; pts, out_rows or planes not 16-byte aligned; with out_rows, a row_stride below the largest named cloud; planes NULL
 * on a grid with cells and field NULL or not 16-byte aligned.  ICPMI_ERR_UNSUPPORTED: a named cloud above
 * ICPMI_GM_MAX_ROWS rows by off_host; the sum of the named clouds' rows reaching 2^29; n_pairs * ceil(largest named cloud
 * / ICPMI_GK_CHUNK_ROWS) reaching 2^31.  ICPMI_ERR_WORKSPACE: planes NULL on a grid with cells and a workspace that is NULL,
 * misaligned or below icpmi_grid_occupancy_planes_bytes(ny, nx).  ny * nx == 0: nothing is packed and no step is inside the
 * grid — every row with cells is UNEXPLORED.
 * Launches: one memset of the records; gc_planes_kernel (only when the call packs); gk_check_kernel — a workgroup of
 * ICPMI_GK_THREADS threads per (pair, chunk of ICPMI_GK_CHUNK_ROWS rows), a lane per row, a wave 64 consecutive rows of one
 * pair; ballots count the classes per wave, LDS per workgroup, one int32 atomicAdd per non-zero counter per workgroup —
 * (only when a named cloud has rows); and pair_status_kernel, a lane per pair, which settles the status. */
#define ICPMI_GK_THREADS 256
#define ICPMI_GK_CHUNK_ROWS 256
#define ICPMI_GK_MAX_TOLERANCE 1073741824
#define ICPMI_GK_INTS 8
#define ICPMI_GK_REC_STATUS 0
#define ICPMI_GK_REC_ROWS 1
#define ICPMI_GK_REC_CONFIRMED 2
#define ICPMI_GK_REC_VIOLATED 3
#define ICPMI_GK_REC_IN_FREE 4
#define ICPMI_GK_REC_UNEXPLORED 5
#define ICPMI_GK_REC_THROUGH_UNKNOWN 6
#define ICPMI_GK_ST_OK 0
#define ICPMI_GK_ST_EMPTY 1
#define ICPMI_GK_ST_CAPACITY 2
#define ICPMI_GK_CLASS_CONFIRMED 0
#define ICPMI_GK_CLASS_VIOLATED 1
#define ICPMI_GK_CLASS_IN_FREE 2
#define ICPMI_GK_CLASS_UNEXPLORED 3
#define ICPMI_GK_NO_CELLS (-2)    /* class of a row whose pose or end point has no cell */
#define ICPMI_GK_ROW_INTS 4
#define ICPMI_GK_ROW_CLASS 0
#define ICPMI_GK_ROW_K_HIT 1
#define ICPMI_GK_ROW_K 2
#define ICPMI_GK_ROW_K_UNKNOWN 3
int icpmi_grid_check_batch(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                           double min_x, double min_y, double resolution, const double* pts, const int32_t* off_dev,
                           const int32_t* off_host, const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                           const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                           int32_t tolerance, int32_t* out_records, int32_t* out_rows, int32_t row_stride,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- the beam model: measured scans scored against the ranges the map expects (no counterpart in the reference) --------
 * The check sorts a beam into four classes with a hard tolerance; the cast hands the expected ranges to the host.
 * icpmi_grid_beam_batch gives what a particle filter's measurement update, a ranking of loop-closure candidates and a sigma
 * estimate from residuals read: one number per (scan, pose) that falls smoothly with the signed distance, along each beam,
 * between where the map has its first wall and where the beam returned.  Every measured beam is walked from the pose's cell
 * through the cell of its own hit to a far end `beyond` metres behind it; the difference in steps picks an entry of the
 * caller's table, and the entries are summed per pair on the device.  After the cells are formed everything is integer and
 * added with integer atomics: a record is a function of the inputs alone, to the bit.
 *
 * The map, the cloud set, the pairs, pair_t and cos_sin: exactly as icpmi_grid_check_batch takes them.  In place of its
 * tolerance: beyond, float64 metres, finite and >= 0 — how far past its return a beam is walked; half_width H, 0 <= H <=
 * ICPMI_GB_MAX_HALF_WIDTH; table, device, 16-byte aligned, int32 [2 H + 3].
 *
 * Cells of a row.  For row (x, y) of pair b, in float64 with every operation rounded on its own (sqrt the IEEE one):
 *   r = sqrt(x * x + y * y),  s = (r + beyond) / r,  fx = x * s,  fy = y * s.
 * Three cells by icpmi_grid_check_batch's expressions and rule: the origin o from (tx, ty), the hit h from (x, y) and the
 * far end f from (fx, fy).  If any of the three has no cell — a coordinate that is not finite or a cell outside [-2^29,
 * 2^29]; r = 0 among them, where s is not finite — the row has no cells.
 *
 * Index of a row.  Let [k_hit, ., ., k_unknown] be the cast's record of the segment o -> f, the end cell included, and k_z =
 * |h_major - o_major| on the major axis OF THAT WALK (x where |fx_cell - ox| >= |fy_cell - oy|, else y): the step at which
 * the beam returned.  The row's table index i is
 *   clamp(k_hit - k_z, -H, H) + H   where k_hit >= 0: positive differences mean the beam came back short of the map's wall,
 *                                   negative ones that it came back from behind it;
 *   2 H + 1                         else, where h lies inside the grid with its unknown bit clear: a return out of observed
 *                                   free space with no wall within `beyond`;
 *   2 H + 2                         else: a return from unexplored space or from off the grid.
 * Differences are in steps along the walk's major axis, as the check's tolerance is: a step is `resolution` metres along an
 * axis and up to sqrt(2) * resolution along a diagonal, so the same table is up to sqrt(2) wider in metres on a diagonal.
 * (k_hit and k_z lie in [-1, 2^30]: the difference does not overflow.)
 *
 * out_records: device, int32 [n_pairs][ICPMI_GB_INTS], slots ICPMI_GB_REC_*: STATUS, ROWS (the rows with cells), SCORE,
 * EXPECTED (rows with k_hit >= 0), NOVEL (rows at index 2 H + 1), UNEXPLORED (rows at index 2 H + 2; the three sum to ROWS)
 * and two 0.  SCORE is the sum over the rows with cells of clip(table[i], -ICPMI_GB_TABLE_CLIP, ICPMI_GB_TABLE_CLIP): the
 * kernel clips while it stages the table, so ICPMI_GM_MAX_ROWS rows cannot overflow an int32.  Status ICPMI_GB_ST_OK /
 * _EMPTY / _CAPACITY by icpmi_grid_check_batch's rules, the one for cnt_dev included.
 * out_hist (optional, NULL: off): device, 16-byte aligned, int32 [n_pairs][2 H + 3]: the rows with cells per index (they sum
 * to ROWS, and SCORE is their product with the clipped table); all 0 for a pair with CAPACITY.
 * out_rows (optional, NULL: off): device, 16-byte aligned, int32 [n_pairs][row_stride][ICPMI_GB_ROW_INTS], one 16-byte
 * store per row: [i, k_hit, k_z, k_unknown]; a row without cells is [ICPMI_GB_NO_CELLS, 0, 0, -1].  row_stride and what is
 * written as for icpmi_grid_check_batch.
 *
 * Refusals, on the host before anything is enqueued: icpmi_grid_check_batch's for everything shared, in its order (n_pairs
 * == 0: ICPMI_OK, nothing done, whatever else is passed).  In addition ICPMI_ERR_ARG for: half_width outside [0,
 * ICPMI_GB_MAX_HALF_WIDTH]; beyond negative, NaN or infinite; table NULL or not 16-byte aligned; out_hist not 16-byte
 * aligned.
 * Launches: one memset of the records and one of the histograms when asked for; gc_planes_kernel (only when the call
 * packs); gb_beam_kernel — a workgroup of ICPMI_GB_THREADS threads per (pair, chunk of ICPMI_GB_CHUNK_ROWS rows), a lane per
 * row; the clipped table and the chunk's histogram in LDS, the score summed per wave, one int32 atomicAdd per non-zero slot
 * and bin per workgroup — (only when a named cloud has rows); and pair_status_kernel, a lane per pair. */
#define ICPMI_GB_THREADS 256
#define ICPMI_GB_CHUNK_ROWS 256
#define ICPMI_GB_MAX_HALF_WIDTH 127
#define ICPMI_GB_TABLE_CLIP 32767
#define ICPMI_GB_INTS 8
#define ICPMI_GB_REC_STATUS 0
#define ICPMI_GB_REC_ROWS 1
#define ICPMI_GB_REC_SCORE 2
#define ICPMI_GB_REC_EXPECTED 3
#define ICPMI_GB_REC_NOVEL 4
#define ICPMI_GB_REC_UNEXPLORED 5
#define ICPMI_GB_ST_OK 0
#define ICPMI_GB_ST_EMPTY 1
#define ICPMI_GB_ST_CAPACITY 2
#define ICPMI_GB_NO_CELLS (-2)    /* index of a row whose pose, hit or far end has no cell */
#define ICPMI_GB_ROW_INTS 4
#define ICPMI_GB_ROW_INDEX 0
#define ICPMI_GB_ROW_K_HIT 1
#define ICPMI_GB_ROW_K_Z 2
#define ICPMI_GB_ROW_K_UNKNOWN 3
int icpmi_grid_beam_batch(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                          double min_x, double min_y, double resolution, const double* pts, const int32_t* off_dev,
                          const int32_t* off_host, const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                          const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                          double beyond, int32_t half_width, const int32_t* table, int32_t* out_records, int32_t* out_hist,
                          int32_t* out_rows, int32_t row_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the particle filter on the occupancy grid: predict, weigh, resample (no counterpart in the reference) ---------------
 * Localisation in a finished map, with the particles resident on the device.  N particles, 1 <= N <=
 * ICPMI_PF_MAX_PARTICLES, are three float64 device arrays: pair_t [N][2] (x, y), theta [N] and cos_sin [N][2] (cos theta,
 * sin theta) — pair_t and cos_sin in exactly the layout icpmi_grid_beam_batch takes under those names, so the beam model
 * reads the particles where they are.  A step is icpmi_pf_predict, icpmi_grid_beam_batch (every pair naming the one scan),
 * icpmi_pf_weights, icpmi_pf_resample when the caller decides so, and icpmi_pf_estimate.  After the beam model's integer
 * score everything but the estimate is integer, and the estimate is summed in a fixed order: a step is a function of
 * (inputs, seed, step) to the bit.  No entry synchronises.
 *
 * Random numbers: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
 * constants M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85), counter-based, no state.  The key is
 * (seed & 0xffffffff, seed >> 32); the counter is [particle, block, step, purpose], purpose ICPMI_PF_PURPOSE_PREDICT or
 * ICPMI_PF_PURPOSE_RESAMPLE (or ICPMI_PFG_PURPOSE_UNIFORM, below).  A round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to (hi(M1 c2) ^ c1 ^ k0,
 * lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); ten rounds, the key raised by (W0, W1) between them.
 * Normal deviates without a transcendental function: particle i takes blocks 0 .. ICPMI_PF_PREDICT_BLOCKS - 1, 20 words in
 * order, each word as two 16-bit halves, the low one first: 40 halves.  Deviate m (m = 0, 1, 2) is z_m = (S_m - 393210) *
 * 2^-16 with S_m the sum of halves 12 m .. 12 m + 11, an integer in [0, 786420]: the sum of twelve uniforms, exact in float64,
 * of standard deviation 1 to within 2^-33 and tails to +-6.
 *
 * icpmi_pf_predict — the motion model, in place, a lane per particle.  The control (dx, dy, dtheta) is in the robot's
 * frame.  In float64, every operation rounded on its own:
 *   ux = dx + sigma_x * z0,  uy = dy + sigma_y * z1,  ut = dtheta + sigma_theta * z2,
 *   x' = x + (c * ux - s * uy),  y' = y + (s * ux + c * uy),  theta' = theta + ut   (c, s: the particle's cos_sin),
 *   (c', s') = (cos theta', sin theta') by the device library's sincos (OCML: within 4 ulp).  theta is not wrapped.
 * Refusals, on the host before anything is enqueued, in this order: n < 0: ICPMI_ERR_ARG; n > ICPMI_PF_MAX_PARTICLES:
 * ICPMI_ERR_UNSUPPORTED; n == 0: ICPMI_OK, nothing done, whatever else is passed; a null pointer, pair_t or cos_sin not
 * 16-byte aligned, theta not 8-byte aligned; a control or a deviation that is not finite; a deviation below zero: ICPMI_ERR_ARG.
 * Launches: pf_predict_kernel, workgroups of ICPMI_PF_THREADS lanes.
 *
 * icpmi_pf_weights — beam records to integer weights.  records: device, 16-byte aligned, int32 [n][ICPMI_GB_INTS] as
 * icpmi_grid_beam_batch left them.  s_max is the largest SCORE among the records with status ICPMI_GB_ST_OK.  An OK record
 * has d = s_max - score (int64: int32 extremes do not overflow) and the weight min(wtable[d >> shift], ICPMI_PF_MAX_WEIGHT)
 * where d >> shift < entries, else 0; a record that is not OK has 0.  wtable: device, uint32 [entries], 1 <= entries <=
 * ICPMI_PF_MAX_ENTRIES, staged (and clipped) into LDS; 0 <= shift <= ICPMI_PF_MAX_SHIFT.  w: device, uint32 [n].  sums:
 * device, int64 [ICPMI_PF_SUMS] = [W = sum w, sum w^2, OK records, s_max], by integer atomics — the order does not matter;
 * w <= 2^20 and n <= 2^20 keep W <= 2^40 and sum w^2 <= 2^60.  No OK record: W = 0, and s_max is the least int64.
 * Refusals, in this order: n as for icpmi_pf_predict; a null pointer, records not 16-byte aligned, sums not 8-byte aligned,
 * entries or shift outside their ranges: ICPMI_ERR_ARG.
 * Launches: pf_sums_init_kernel (one wave), pf_max_kernel and pf_weights_kernel (a lane per record; one atomic per
 * workgroup and slot).
 *
 * icpmi_pf_resample — systematic resampling in integers.  C_i: the inclusive prefix sum of w (uint64), W = C_{n-1}.
 * rho = (r1 * 2^32 + r0) mod W, r0 and r1 the first two words of Philox at counter [0, 0, step, ICPMI_PF_PURPOSE_RESAMPLE].
 * E_i = floor((n * C_i + rho) / W) in uint64 (n * C_i + rho < 2^61), E_{-1} = 0: particle i has E_i - E_{i-1} offspring,
 * which sum to n exactly, and new particle j has the ancestor i with E_{i-1} <= j < E_i.  ancestors: device, int32 [n]; the
 * state is gathered by ancestor from (pair_t, theta, cos_sin) into (out_pair_t, out_theta, out_cos_sin), bit copies; info:
 * device, int32 [ICPMI_PF_INFO_INTS] = [status, 0, 0, 0], status ICPMI_PF_ST_OK or, where W = 0, ICPMI_PF_ST_DEGENERATE:
 * the ancestors are then the identity and the state is copied unchanged.
 * Refusals, in this order: n as for icpmi_pf_predict; a null pointer, a pair_t or cos_sin (in or out) not 16-byte aligned, a
 * theta not 8-byte aligned, an output that is its own input: ICPMI_ERR_ARG; a workspace that is NULL, not 16-byte aligned or
 * below icpmi_pf_workspace_bytes(n): ICPMI_ERR_WORKSPACE.
 * Launches, none of which waits on another workgroup: pf_block_sums_kernel (a workgroup per ICPMI_PF_SCAN_BLOCK weights:
 * their sum), pf_scan_sums_kernel (ONE workgroup: the exclusive scan of up to ICPMI_PF_MAX_PARTICLES / ICPMI_PF_SCAN_BLOCK
 * block sums, ICPMI_PF_SUMS_PER_LANE consecutive sums per lane; W, rho, info), pf_offspring_kernel (a workgroup per block
 * scans it again from its offset and stores E_i as uint32) and pf_gather_kernel (a lane per new particle: a bisection of E,
 * the ancestor, the copy).
 *
 * icpmi_pf_estimate — weighted moments: out, device, float64 [ICPMI_PF_EST_DOUBLES] = [sum w, sum w x, sum w y, sum w c,
 * sum w s, sum (w x) x, sum (w x) y, sum (w y) y], every product rounded on its own.  Added in a fixed order: a workgroup
 * per ICPMI_PF_EST_CHUNK particles, lane t adding particles base + t + ICPMI_PF_THREADS k in the order of k, the lanes by
 * the library's fixed tree; the workgroups' partials in index order by one lane per sum.  No floating-point atomics: the
 * same inputs give the same bits on every run.
 * Refusals: n as above (n == 0: ICPMI_OK, nothing written); a null pointer or misaligned pair_t / cos_sin / out (16, 16, 8
 * bytes): ICPMI_ERR_ARG; the workspace as for icpmi_pf_resample.
 * Launches: pf_moments_kernel, pf_moments_sum_kernel (one wave).
 *
 * icpmi_pf_workspace_bytes(n): what icpmi_pf_resample and icpmi_pf_estimate need for n particles (one buffer serves both,
 * one call at a time); 0 for n outside [1, ICPMI_PF_MAX_PARTICLES]. */
#define ICPMI_PF_MAX_PARTICLES 1048576
#define ICPMI_PF_THREADS 256
#define ICPMI_PF_PREDICT_BLOCKS 5
#define ICPMI_PF_PURPOSE_PREDICT 0
#define ICPMI_PF_PURPOSE_RESAMPLE 1
#define ICPMI_PF_MAX_ENTRIES 4096
#define ICPMI_PF_MAX_SHIFT 32
#define ICPMI_PF_MAX_WEIGHT 1048576
#define ICPMI_PF_SUMS 4
#define ICPMI_PF_SUM_W 0
#define ICPMI_PF_SUM_WW 1
#define ICPMI_PF_SUM_OK 2
#define ICPMI_PF_SUM_SMAX 3
#define ICPMI_PF_SCAN_BLOCK 1024
#define ICPMI_PF_SUMS_PER_LANE 4
#define ICPMI_PF_INFO_INTS 4
#define ICPMI_PF_ST_OK 0
#define ICPMI_PF_ST_DEGENERATE 1
#define ICPMI_PF_EST_CHUNK 1024
#define ICPMI_PF_EST_DOUBLES 8
int icpmi_pf_predict(int32_t n, double* pair_t, double* theta, double* cos_sin, double dx, double dy, double dtheta,
                     double sigma_x, double sigma_y, double sigma_theta, uint64_t seed, uint32_t step, void* stream);
int icpmi_pf_weights(int32_t n, const int32_t* records, const uint32_t* wtable, int32_t entries, int32_t shift, uint32_t* w,
                     int64_t* sums, void* stream);
int icpmi_pf_resample(int32_t n, const uint32_t* w, const double* pair_t, const double* theta, const double* cos_sin,
                      double* out_pair_t, double* out_theta, double* out_cos_sin, int32_t* ancestors, int32_t* info,
                      uint64_t seed, uint32_t step, void* workspace, size_t workspace_bytes, void* stream);
int icpmi_pf_estimate(int32_t n, const uint32_t* w, const double* pair_t, const double* cos_sin, double* out, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t icpmi_pf_workspace_bytes(int32_t n);

/* ---- the particle filter: a start over the map's free cells, recovery by injection (ICPMI_PFG_*: "global") ---------------
 * Poses drawn uniformly from the map's free space, on the device: once for the whole population (a start without a prior)
 * and after a resampling for a share of it (random injection, the recovery of augmented MCL).  A draw is a function of
 * (planes, box, seed, step) to the bit.  No entry synchronises.
 *
 * Free cell: a cell inside the grid whose bit is clear in BOTH planes of icpmi_grid_occupancy_planes — neither occupied nor
 * unknown — and that lies inside the cell box [x0, x1) x [y0, y1).  The box is clipped to the grid; a box that is empty
 * after clipping is legal and has no free cell.  The pad bits of a row's last word are never free.
 *
 * Free index: with words = ny * wpr in the planes' row-major word order, the index buffer (device, 16-byte aligned,
 * icpmi_pf_free_index_bytes(ny, nx) bytes) holds uint32 header [ICPMI_PFG_FREE_HEADER] = [F, words, wpr, 0 ...]; then, each
 * from the next multiple of 256 bytes on, free [words]: the masked free word of every plane word; rank [words]: the
 * exclusive prefix sum of popcount(free[.]); and the ceil(words / ICPMI_PFG_FREE_BLOCK) block sums the build scans (its
 * scratch).  F is the total, below 2^31.  The index is a function of (planes, box) to the bit.
 *
 * icpmi_pf_free_index — builds the index of `planes` (what icpmi_grid_occupancy_planes wrote for this ny, nx).
 * Refusals, on the host before anything is enqueued, in this order: the grid as icpmi_grid_occupancy_planes refuses it (ny
 * or nx negative or above 2^29, ny * nx >= 2^31): ICPMI_ERR_ARG; words > ICPMI_PFG_FREE_MAX_WORDS: ICPMI_ERR_UNSUPPORTED;
 * planes NULL or not 16-byte aligned where words > 0: ICPMI_ERR_ARG; an index that is NULL, not 16-byte aligned or below
 * icpmi_pf_free_index_bytes(ny, nx): ICPMI_ERR_WORKSPACE.  x0, y0, x1, y1 are any int32: each is clipped into
 * [0, nx] or [0, ny] on the host, and the kernels see no other value.
 * Launches, none of which waits on another workgroup: pf_free_sums_kernel (a workgroup per ICPMI_PFG_FREE_BLOCK words: the
 * free cells among them), pf_free_scan_kernel (ONE workgroup: the exclusive scan of up to ICPMI_PFG_FREE_MAX_WORDS /
 * ICPMI_PFG_FREE_BLOCK block sums, ICPMI_PF_SUMS_PER_LANE consecutive sums per lane; the header) and pf_free_write_kernel (a
 * workgroup per block scans it again from its offset and stores free and rank).  words == 0: the header alone.
 *
 * icpmi_pf_draw_uniform — of n slots, m are drawn, 0 <= m <= n: slot j iff ((j + 1) * m) div n > (j * m) div n in 64-bit
 * integers, which is exactly m slots, spread evenly (m == n: every slot).  The other slots are not touched.  Slot j at
 * (seed, step): r = Philox4x32-10 at the counter [j, 0, step, ICPMI_PFG_PURPOSE_UNIFORM] under the filter's key;
 *   k = (uint64(r0) * F) >> 32;  J = the largest word index with rank[J] <= k;  bit = the (k - rank[J])-th set bit of
 *   free[J], counted from bit 0;  cx = 32 * (J mod wpr) + bit,  cy = J div wpr;
 *   ux = (double(r1 >> 8) + 0.5) * 2^-24,  uy the same from r2;
 *   x = min_x + (double(cx) + ux) * resolution,  y = min_y + (double(cy) + uy) * resolution;
 *   theta = theta0 + ((double(r3) + 0.5) * 2^-32 - 0.5) * theta_span, not wrapped;
 * float64, every operation rounded on its own (no fused multiply-add); cos_sin by the device library's sincos of theta.
 * pair_t, theta, cos_sin: the filter's state arrays.  ancestors: device, int32 [n], or NULL; a drawn slot gets
 * ICPMI_PFG_INJECTED.  info: device, int32 [ICPMI_PF_INFO_INTS] = [status, F, 0, 0]; with F == 0 the status is
 * ICPMI_PFG_ST_NO_FREE and nothing else is written.
 * Refusals, in this order: n as for icpmi_pf_predict (n == 0: ICPMI_OK, nothing done); m outside [0, n]; index, pair_t,
 * theta, cos_sin or info NULL, index, pair_t or cos_sin not 16-byte aligned, theta not 8-byte aligned; a resolution that is
 * not positive and finite, a theta_span outside [0, 2 pi], a theta0, min_x or min_y that is not finite: ICPMI_ERR_ARG.
 * Launches: pf_draw_uniform_kernel, a lane per slot.  The search over rank is a bisection of at most 23 steps over
 * [0, words), words read from the header and clamped to [1, ICPMI_PFG_FREE_MAX_WORDS]; the bit select takes at most 32
 * steps: an index of stale or zero bytes yields wrong particles or ICPMI_PFG_ST_NO_FREE, never an address outside the
 * buffers of an index that was once built there.
 *
 * icpmi_pf_free_index_bytes(ny, nx): the index buffer's size; 0 for a grid icpmi_pf_free_index refuses. */
#define ICPMI_PFG_PURPOSE_UNIFORM 2
#define ICPMI_PFG_FREE_HEADER 64
#define ICPMI_PFG_FREE_BLOCK 4096
#define ICPMI_PFG_FREE_MAX_WORDS 4194304
#define ICPMI_PFG_INJECTED (-1)
#define ICPMI_PFG_ST_NO_FREE 2
size_t icpmi_pf_free_index_bytes(int32_t ny, int32_t nx);
int icpmi_pf_free_index(const void* planes, int32_t ny, int32_t nx, int32_t x0, int32_t y0, int32_t x1, int32_t y1, void* index,
                        size_t index_bytes, void* stream);
int icpmi_pf_draw_uniform(int32_t n, int32_t m, const void* index, double min_x, double min_y, double resolution, double theta0,
                          double theta_span, double* pair_t, double* theta, double* cos_sin, int32_t* ancestors, int32_t* info,
                          uint64_t seed, uint32_t step, void* stream);

/* ── pose graph: PoseGraph2D.optimize, utilities/pose_graph.py:83-134 ──────────
 * Gauss-Newton on SE(2) over n_nodes poses [x, y, theta] (nodes: device, updated
 * in place) and n_edges constraints (i, j, z_ij [3], Omega [3][3] row-major).
 * edges_ij_host: int32 pairs on the HOST (the library classifies the edges and
 * builds its gather lists from them); edges_z / edges_omega: device.
 * All iterations run in one launch.  Graphs whose consecutive nodes are all
 * joined by an edge (the odometry chain slam.py:543-549 builds) are solved as
 * block-tridiagonal + low-rank (the split); any other graph through the dense
 * 3n x 3n matrix, as the reference does.  fix_node is held by the 1e10 diagonal
 * of pose_graph.py:107-112.
 * The split inverts the chain part T on its own, so a chain edge with (almost)
 * no information would cost it digits that a solve of the whole system keeps.
 * The call reads the information matrices back and treats a chain edge as weak
 * when the smallest eigenvalue of its symmetric part (closed form) is below
 * S / (3 n), S the largest row sum of |Omega| in the graph: such an edge enters
 * T as S I and its remainder Omega - S I joins the closures (same sum, T as
 * stiff there as anywhere).  That needs room: size the workspace with
 * icpmi_pose_graph_weighted_workspace_bytes (edges_omega_host: the same
 * matrices on the host); with the plain size query a graph that has weak chain
 * edges ends at once with ICPMI_PG_ST_REFUSED.  That status also ends a launch
 * where a block of T is exactly singular or the closure system has an exactly
 * zero pivot.
 * info (device, ICPMI_PGINFO_DOUBLES doubles), slots ICPMI_PGINFO_*:
 * ITERATIONS run; STATUS, one of ICPMI_PG_ST_* (NOTHING to do: fewer than two
 * nodes or no edges; CONVERGED: step norm < convergence_eps; MAXITER: iteration
 * limit; SINGULAR system, reported by the dense elimination only (an exactly
 * zero pivot, LAPACK's error): the nodes keep the values of the previous
 * iteration, pose_graph.py:117-119; REFUSED split step: the nodes keep the
 * values of the previous iteration and ITERATIONS counts the applied ones —
 * continue with icpmi_pose_graph_optimize_dense for the remaining iterations,
 * as PoseGraph2D.optimize does); STEP, the norm of the last step; then from
 * PHASE_US on the ICPMI_PGINFO_PHASES device clocks in microseconds, summed over
 * the iterations: assembly; the closure columns W; the chain solve (cyclic
 * reduction of T, which is its factorisation, and the back substitution, on all
 * columns); the closure system; its solve; dx; apply.  On the dense path the
 * four clocks between assembly and dx stay 0 and the whole elimination is in dx.
 * icpmi_pose_graph_optimize_dense: the same call with the dense path forced;
 * it never returns ICPMI_PG_ST_REFUSED.
 * Refused on the host before anything is enqueued: null nodes or info,
 * negative sizes, null edge arrays with n_edges > 0, fix_node or an edge index
 * outside the graph (ICPMI_ERR_ARG); a null workspace, or one below the plain
 * size query's value (ICPMI_ERR_WORKSPACE: also where the graph has weak chain
 * edges; ICPMI_PG_ST_REFUSED is for a workspace that holds the graph without
 * its twins).
 * workspace: icpmi_pose_graph_workspace_bytes(edges_ij_host, n_nodes, n_edges),
 * icpmi_pose_graph_dense_workspace_bytes(...) for the dense call. */
#define ICPMI_PG_ST_NOTHING 0
#define ICPMI_PG_ST_CONVERGED 1
#define ICPMI_PG_ST_MAXITER 2
#define ICPMI_PG_ST_SINGULAR 3
#define ICPMI_PG_ST_REFUSED 4
#define ICPMI_PGINFO_DOUBLES 10
#define ICPMI_PGINFO_ITERATIONS 0
#define ICPMI_PGINFO_STATUS 1
#define ICPMI_PGINFO_STEP 2
#define ICPMI_PGINFO_PHASE_US 3
#define ICPMI_PGINFO_PHASES 7
size_t icpmi_pose_graph_workspace_bytes(const int32_t* edges_ij_host, int32_t n_nodes, int32_t n_edges);
size_t icpmi_pose_graph_weighted_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                                 int32_t n_nodes, int32_t n_edges);
int icpmi_pose_graph_optimize(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                              const double* edges_omega, int32_t n_nodes, int32_t n_edges,
                              int32_t n_iterations, int32_t fix_node, double convergence_eps,
                              double* info, void* workspace, size_t workspace_bytes, void* stream);
size_t icpmi_pose_graph_dense_workspace_bytes(const int32_t* edges_ij_host, int32_t n_nodes, int32_t n_edges);
int icpmi_pose_graph_optimize_dense(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                    const double* edges_omega, int32_t n_nodes, int32_t n_edges,
                                    int32_t n_iterations, int32_t fix_node, double convergence_eps,
                                    double* info, void* workspace, size_t workspace_bytes, void* stream);

/* total_error, pose_graph.py:189-194: sum over edges of e^T Omega e, in edge
 * order.  Everything on the device; scratch: n_edges doubles; out: 1 double. */
int icpmi_pose_graph_error(const double* nodes, const int32_t* edges_i, const int32_t* edges_j,
                           const double* edges_z, const double* edges_omega, int32_t n_edges,
                           double* scratch, double* out, void* stream);

/* ── pose graph: marginal covariances ──────────────────────────────────────────
 * 3 x 3 blocks of H^-1, H exactly the matrix pose_graph.py:93-114 assembles at
 * the current nodes: every edge's four blocks, the rows and columns of fix_node
 * zeroed, 1e10 I on its diagonal block.  Block (v, w) is rows 3v..3v+2, columns
 * 3w..3w+2; nothing is symmetrised, and information matrices that are not
 * symmetric or not positive definite are accepted as optimize accepts them.  For
 * symmetric positive definite information this is the covariance of the poses
 * given the anchor.  No iteration is run; nodes are only read.
 * Arguments as icpmi_pose_graph_optimize (edges_ij_host on the HOST, nodes /
 * edges_z / edges_omega on the device), and:
 * selected_host: n_selected node indices on the HOST (duplicates allowed).
 * out_diagonal (device, or null): block (v, v) of every node, [n_nodes][9]
 *   row-major.
 * out_columns (device, or null): block (v, selected[a]) of every node v,
 *   [n_selected][n_nodes][9]: every joint marginal of selected nodes.
 * force_dense != 0: the dense path whatever the graph.
 * Paths: the split of optimize on the same plan (chain, closures, twins of weak
 * chain edges) through H^-1 = T^-1 - T^-1 W (I + C W^T T^-1 W)^-1 C W^T T^-1;
 * its sweeps along the chain are serial in n_nodes, everything else is spread
 * over the device.  A graph that optimize does not split, or force_dense, takes
 * the dense matrix eliminated with partial pivoting: O(n_nodes^3) time like
 * optimize's dense path, and for the diagonal all 3 n_nodes unit columns are
 * solved, a second 3n x 3n array in the workspace.
 * info (device, ICPMI_MARG_DOUBLES doubles), slots ICPMI_MARG_*: STATUS, one of
 * ICPMI_PG_ST_* (CONVERGED: done; SINGULAR: an exactly zero pivot of the dense
 * elimination, which alone reports it — the outputs are filled with NaN;
 * REFUSED: a block of the split is exactly singular, or the plan does not split
 * this graph (a chain edge without information along some direction, or twins
 * without room because the workspace was sized without the information
 * matrices) — nothing was written, repeat with force_dense; NOTHING: fewer than
 * two nodes or no edges, nothing was written); PATH, ICPMI_MARG_PATH_*;
 * CLOSURES and TWINS of the plan.
 * Refused on the host before anything is enqueued: null nodes or info, both
 * outputs null, n_selected < 0, a selected index, fix_node or an edge index
 * outside the graph (ICPMI_ERR_ARG); a workspace below the size query's value
 * (ICPMI_ERR_WORKSPACE).
 * workspace: icpmi_pose_graph_marginals_workspace_bytes (edges_omega_host: the
 * information matrices on the host, for the twins, or null; 0 for sizes below
 * zero or an edge outside the graph). */
#define ICPMI_MARG_DOUBLES 4
#define ICPMI_MARG_STATUS 0
#define ICPMI_MARG_PATH 1
#define ICPMI_MARG_CLOSURES 2
#define ICPMI_MARG_TWINS 3
#define ICPMI_MARG_PATH_SPLIT 0
#define ICPMI_MARG_PATH_DENSE 1
size_t icpmi_pose_graph_marginals_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                                  int32_t n_nodes, int32_t n_edges, int32_t n_selected,
                                                  int32_t want_diagonal, int32_t force_dense);
int icpmi_pose_graph_marginals(const double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                               const double* edges_omega, int32_t n_nodes, int32_t n_edges, int32_t fix_node,
                               const int32_t* selected_host, int32_t n_selected, double* out_diagonal,
                               double* out_columns, int32_t force_dense, double* info, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ── pose graph: robust edges (no counterpart in the reference) ────────────────
 * icpmi_pose_graph_optimize (the Gauss-Newton of pose_graph.py:93-134) with a
 * robust loss on the edges the caller masks.  chi2_q = e_q^T Omega_q e_q,
 * evaluated as icpmi_pose_graph_error evaluates it, with the caller's Omega;
 * c = delta^2;
 *     F(x) = sum over unmasked edges of chi2_q + sum over masked edges of rho(chi2_q)
 * kernel (ICPMI_ROB_KERNEL_*)   rho(s)                                  w(s) = rho'(s)
 *   HUBER 0           s if s <= c, else 2 delta sqrt(s) - c   1 if s <= c, else delta / sqrt(s)
 *   CAUCHY 1          c log1p(s / c)                          c / (c + s)
 *   GEMAN_MCCLURE 2   c s / (c + s)                           (c / (c + s))^2
 * Geman-McClure is the closed form of switchable constraints / dynamic
 * covariance scaling (DCS) with Phi = c.  Every w is continuous in s, lies in
 * (0, 1] for s >= 0 and is exactly 1.0 where the loss is quadratic (an unmasked
 * edge, Huber up to c), so such a call computes bit for bit what
 * icpmi_pose_graph_optimize computes.  log1p and sqrt are taken on the device
 * in float64; Geman-McClure's rho is evaluated as (c / (c + s)) s.
 * Evaluation order: iteratively re-weighted least squares inside Gauss-Newton.
 * Every iteration starts with the phase `weights`: every edge of the caller's
 * list is linearised at the current poses, chi2_q and w_q = rho'(chi2_q) are
 * stored (an unmasked edge has w_q = 1); then H = sum w_q J^T Omega J and
 * b = sum w_q J^T Omega e are assembled and solved as in
 * icpmi_pose_graph_optimize, w_q Omega_q in the place of Omega_q.  After the
 * last iteration one more weights pass runs, so that edge_chi2, edge_weight and
 * COST_AFTER describe the poses that are returned.  COST_BEFORE is the cost at
 * the input poses.  Both costs are summed in a fixed order.
 * Path rule: the plan of icpmi_pose_graph_optimize on the caller's unweighted
 * Omega (weights <= 1 on closures only make the weak-edge rule conservative).
 * A masked edge between consecutive nodes cannot stay in the chain part T,
 * whose stiffness its weight would move under the plan: a graph with one takes
 * the dense path, as with dense != 0.  ICPMI_PG_ST_REFUSED and the dense
 * continuation are those of icpmi_pose_graph_optimize: repeat the call with
 * dense != 0 for the remaining iterations.
 * edges_mask_host: uint8 [n_edges] on the HOST, non-zero = robust.
 * edge_chi2, edge_weight: device, n_edges doubles each, the caller's edge order.
 * info (device, ICPMI_ROB_DOUBLES doubles): the ICPMI_PGINFO_* record in its
 * slots, then COST_BEFORE, COST_AFTER and WEIGHTS_US (the device clock of the
 * weights phase in microseconds, all passes).
 * n_iterations == 0 is evaluation only: chi2, weights and both costs (equal)
 * at the given poses, status MAXITER, nothing moved.
 * Refused on the host before anything is enqueued (ICPMI_ERR_ARG): an unknown
 * kernel; delta not > 0, or NaN; a null mask with n_edges > 0; a null output;
 * null nodes or info, negative sizes, null edge arrays with n_edges > 0,
 * fix_node or an edge index outside the graph; and (ICPMI_ERR_WORKSPACE) a
 * workspace below the size query's value.
 * workspace: icpmi_pose_graph_robust_workspace_bytes (edges_omega_host: the
 * information matrices on the host, for the twins, or null; 0 for sizes below
 * zero, a missing list or an edge outside the graph). */
#define ICPMI_ROB_KERNEL_HUBER 0
#define ICPMI_ROB_KERNEL_CAUCHY 1
#define ICPMI_ROB_KERNEL_GEMAN_MCCLURE 2
#define ICPMI_ROB_DOUBLES 13
#define ICPMI_ROB_COST_BEFORE 10
#define ICPMI_ROB_COST_AFTER 11
#define ICPMI_ROB_WEIGHTS_US 12
size_t icpmi_pose_graph_robust_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                               const uint8_t* edges_mask_host, int32_t n_nodes, int32_t n_edges,
                                               int32_t dense);
int icpmi_pose_graph_optimize_robust(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                     const double* edges_omega, const uint8_t* edges_mask_host, int32_t n_nodes,
                                     int32_t n_edges, int32_t n_iterations, int32_t fix_node, double convergence_eps,
                                     int32_t kernel, double delta, int32_t dense, double* edge_chi2,
                                     double* edge_weight, double* info, void* workspace, size_t workspace_bytes,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICPMI_H */
