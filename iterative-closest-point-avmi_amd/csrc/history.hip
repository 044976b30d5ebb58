// history.hip — a resident, append-only set of prepared scans for loop-closure matching.
//
// Reference slam.py:566-597: the candidates of a loop closure are past scans (scan_history, appended at slam.py:554), and
// each is matched by _run_icp_pair (slam.py:53-98), which filters the target twice (features.py:198-199, icp.py:149-150),
// takes its mean (features.py:206) and builds two k-d trees of it (features.py:211, icp.py:173) — every time, although a
// past scan never changes (pose-graph optimisation moves its pose, slam.py:606-607).  Here those steps run once, when the
// scan is added, and a query is the search kernel and the ICP kernels on the state they left.
//
// Adding and matching have no kernel of their own: the filter (voxel.hip), the prepare kernels (prep.hip), both halves
// of the rotation search (rotsearch.hip, through rotsearch.hpp) and the per-cloud half of the feature alignment (features.hip,
// through features.hpp: icpmi_history_features_add is ft_cloud_stages into a feature store, icpmi_history_feature_align of
// features.hip runs the pair stages on it) are the batch path's, run on a range of clouds; growing is device-to-device copies.
//
// One kernel lives here: history_world_rows_kernel, transform_points_2d (slam.py:46-50) of resident raw rows.  After an
// accepted closure the reference moves every pose (slam.py:606-607), transforms every past scan again on the host and
// replays it into the map (_rebuild_map, slam.py:271-277) and into the submap buffer (slam.py:612-615).  The rows are
// already here; what changed is six doubles per scan, so the rebuild takes scan ids and poses and the world rows never
// visit the host.
//
// Two things a history must get right, both because its clouds are a prefix of a larger allocation:
//  - a prepared buffer's arrays are carved from a row count (PreparedView).  That count is the history's row CAPACITY,
//    fixed until a relayout — with the rows in use, every array would move at every add;
//  - the filter takes a cloud's rows from off[c + 1] - off[c], so the raw clouds lie back to back and the clouds not
//    added yet have zero rows (off[c] = rows in use).
#include "features.hpp"
#include "prep_common.hpp"
#include "rotsearch.hpp"

namespace icpmi {

constexpr int HISTORY_MAX_ROWS = 4096;      // the on-chip path of every kernel involved (prep.hip: PREP_MAX_POINTS)

// ── world rows ──────────────────────────────────────────────────────────────────────────────────────────────────────
// points @ T[:2, :2].T + T[:2, 2] as NumPy rounds it.  The product is BLAS: a scan of two or more rows goes to gemm, whose
// element is fma(y, R[c][1], x * R[c][0]) (ft_transform_kernel of features.hip has the same form); a scan of exactly one
// row goes to gemv, which accumulates the other way round, fma(x, R[c][0], y * R[c][1]).  Both are written out; the file is
// compiled with -ffp-contract=off, so nothing else fuses.
//
// One thread per row, double2 in and double2 out (both streams coalesced), a workgroup per (scan of the list, chunk of
// WR_THREADS of its rows).  The host knows no row count here (the offsets are the device's), so every scan gets the chunks
// of the largest scan a history holds and a workgroup past its scan's rows leaves at once.  Scan id, offsets and the pose
// depend on the workgroup alone: scalar loads, once.
constexpr int WR_THREADS = 256;
constexpr int WR_CHUNKS = HISTORY_MAX_ROWS / WR_THREADS;
static_assert(WR_CHUNKS * WR_THREADS == HISTORY_MAX_ROWS, "the chunks of a scan cover the largest scan exactly");

__global__ __launch_bounds__(WR_THREADS) void history_world_rows_kernel(const double2* __restrict__ pts, const int32_t* __restrict__ off,
                                                                        int scan_capacity, const int32_t* __restrict__ ids,
                                                                        const double* __restrict__ poses,
                                                                        const int32_t* __restrict__ out_off, double2* __restrict__ out) {
    const int k = blockIdx.x / WR_CHUNKS;
    const int first = (blockIdx.x % WR_CHUNKS) * WR_THREADS;
    const int id = ids[k];
    if (id < 0 || id >= scan_capacity) return;                  // (the callers refuse such an id; never read past the offsets)
    const int begin = off[id];
    const int n = off[id + 1] - begin;
    const int out_begin = out_off[k];
    const int room = out_off[k + 1] - out_begin;
    const int rows = n < room ? n : room;                       // equal for a well-formed call
    if (begin < 0 || out_begin < 0 || first >= rows) return;
    const double* r = poses + (size_t)k * 6;
    const double r00 = r[0], r01 = r[1], r10 = r[2], r11 = r[3], tx = r[4], ty = r[5];
    const int i = first + (int)threadIdx.x;
    if (i >= rows) return;
    const double2 p = pts[(size_t)begin + i];
    double2 w;
    if (n == 1) w = make_double2(__builtin_fma(p.x, r00, p.y * r01) + tx, __builtin_fma(p.x, r10, p.y * r11) + ty);     // gemv
    else w = make_double2(__builtin_fma(p.y, r01, p.x * r00) + tx, __builtin_fma(p.y, r11, p.x * r10) + ty);            // gemm
    out[(size_t)out_begin + i] = w;
}

struct WorldRowsPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    unsigned grid, block;     // grid == 0: nothing to do
};
static WorldRowsPlan plan_world_rows(int n_ids) {
    WorldRowsPlan p{ICPMI_OK, 0, WR_THREADS};
    if (n_ids < 0 || n_ids > INT32_MAX / WR_CHUNKS) { p.rc = ICPMI_ERR_ARG; return p; }
    p.grid = (unsigned)n_ids * WR_CHUNKS;
    return p;
}

static bool history_complete(const icpmi_history* h) {
    return h && h->pts && h->off_dev && h->ids && h->icp_vox && h->icp_cnt && h->icp_prepared && h->rs_vox && h->rs_cnt &&
           h->rs_means && h->rs_prepared && h->scan_capacity > 0 && h->row_capacity > 0 &&
           h->prepared_bytes >= icpmi_prepared_bytes(h->row_capacity, h->scan_capacity, 0);
}

}  // namespace icpmi

extern "C" int icpmi_history_add(const icpmi_history* h, const int32_t* off_host, int32_t first, int32_t n_new, int32_t prepare,
                                 void* stream) {
    using namespace icpmi;
    if (!history_complete(h) || !off_host || first < 0 || n_new < 0 || first > h->scan_capacity - n_new) return ICPMI_ERR_ARG;
    if (!(h->icp_voxel > 0.0) || !(h->rs_voxel > 0.0)) return ICPMI_ERR_ARG;
    if (n_new == 0) return ICPMI_OK;
    int max_n, end_row;
    if (off_host[first] < 0 || !cloud_rows(off_host + first, n_new, max_n, end_row)) return ICPMI_ERR_ARG;
    if (end_row > h->row_capacity) return ICPMI_ERR_ARG;
    if (max_n > HISTORY_MAX_ROWS) return ICPMI_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int32_t* ids = h->ids + first;
    // ICP: filter, then search order and normals (IcpBatch.run's two launches, for this range)
    int rc = icpmi_voxel_downsample_batch(h->pts, h->off_dev + first, off_host + first, n_new, 2, h->icp_voxel, h->icp_vox,
                                          h->icp_cnt + first, h->voxel_ws, h->voxel_ws_bytes, stream);
    if (rc != ICPMI_OK) return rc;
    if (prepare) {
        rc = icpmi_prepare_targets_ex(h->icp_vox, h->off_dev, off_host, h->icp_cnt, ids, nullptr, n_new, h->scan_capacity,
                                      h->row_capacity, max_n, h->normal_k < 0 ? -1 : h->normal_k, nullptr, h->icp_prepared,
                                      h->prepared_bytes, h->allow_polar, stream);
        if (rc != ICPMI_OK) return rc;
    }
    // rotation search: filter, means, search order (the first half of icpmi_rotation_search_batch, for this range)
    rc = rsb_filter_means(h->pts, h->off_dev, off_host, first, n_new, h->rs_voxel, h->rs_vox, h->rs_cnt, h->rs_means, h->voxel_ws,
                          h->voxel_ws_bytes, st);
    if (rc != ICPMI_OK || !prepare) return rc;
    return icpmi_prepare_targets_ex(h->rs_vox, h->off_dev, off_host, h->rs_cnt, ids, nullptr, n_new, h->scan_capacity, h->row_capacity,
                                    max_n, -1, nullptr, h->rs_prepared, h->prepared_bytes, rsb_allow_polar(), stream);
}

extern "C" int icpmi_history_features_add(const icpmi_history* h, const icpmi_feature_store* s, const int32_t* off_host, int32_t first,
                                          int32_t n_new, void* stream) {
    using namespace icpmi;
    if (!h || !h->pts || !h->off_dev || !h->ids || !h->voxel_ws || h->scan_capacity <= 0 || h->row_capacity <= 0) return ICPMI_ERR_ARG;
    if (!off_host || first < 0 || n_new < 0 || first > h->scan_capacity - n_new) return ICPMI_ERR_ARG;
    const int rc = ft_store_check(s);
    if (rc != ICPMI_OK || n_new == 0) return rc;
    int max_n, end_row;
    if (off_host[first] < 0 || !cloud_rows(off_host + first, n_new, max_n, end_row)) return ICPMI_ERR_ARG;
    if (end_row > h->row_capacity) return ICPMI_ERR_ARG;
    if (max_n > HISTORY_MAX_ROWS) return ICPMI_ERR_UNSUPPORTED;
    // the first half of icpmi_feature_align_batch for this range, into the store
    return ft_cloud_stages(ft_store_tables(h, s), h->pts, off_host, first, n_new, h->ids + first, ft_store_cfg(s), h->voxel_ws,
                           h->voxel_ws_bytes, (hipStream_t)stream);
}

extern "C" int icpmi_history_search(const icpmi_history* h, const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs,
                                    int32_t max_n, const double* coarse_cs, int32_t n_coarse, const double* fine_cs,
                                    const int32_t* fine_cnt, int32_t max_fine, int32_t max_rows_hint, double* out_records,
                                    double* out_init, void* stream) {
    using namespace icpmi;
    if (!history_complete(h)) return ICPMI_ERR_ARG;
    const RsbState s{h->rs_vox, h->off_dev, h->rs_cnt, h->rs_means, h->rs_prepared, h->row_capacity};
    return rsb_search(s, max_n, max_rows_hint, pair_src, pair_tgt, n_pairs, coarse_cs, n_coarse, fine_cs, fine_cnt, max_fine,
                      out_records, out_init, (hipStream_t)stream);
}

extern "C" int icpmi_history_world_rows(const icpmi_history* h, const int32_t* ids, int32_t n_ids, const double* poses,
                                        const int32_t* out_off, double* out_rows, void* stream) {
    using namespace icpmi;
    if (!h || !h->pts || !h->off_dev || h->scan_capacity <= 0) return ICPMI_ERR_ARG;
    const WorldRowsPlan plan = plan_world_rows(n_ids);
    if (plan.rc != ICPMI_OK || plan.grid == 0) return plan.rc;
    if (!ids || !poses || !out_off || !out_rows) return ICPMI_ERR_ARG;
    history_world_rows_kernel<<<plan.grid, plan.block, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const double2*>(h->pts), h->off_dev, h->scan_capacity, ids, poses, out_off, reinterpret_cast<double2*>(out_rows));
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" int icpmi_prepared_relayout(const void* src, int32_t src_rows, int32_t src_clouds, int32_t rows_used, int32_t clouds_used,
                                       void* dst, size_t dst_bytes, int32_t dst_rows, int32_t dst_clouds, void* stream) {
    using namespace icpmi;
    if (!dst || rows_used < 0 || clouds_used < 0 || dst_rows < rows_used || dst_clouds < clouds_used) return ICPMI_ERR_ARG;
    if (src ? (src_rows < rows_used || src_clouds < clouds_used) : (rows_used > 0 || clouds_used > 0)) return ICPMI_ERR_ARG;
    if (dst_bytes < icpmi_prepared_bytes(dst_rows, dst_clouds, 0)) return ICPMI_ERR_WORKSPACE;
    const PreparedView from(src, src ? src_rows : 0), to(dst, dst_rows);
    if (prepared_relayout(from, to, (size_t)rows_used, (size_t)clouds_used, (size_t)dst_clouds, (hipStream_t)stream) != hipSuccess)
        return ICPMI_ERR_HIP;
    return ICPMI_OK;
}
