// gridcheck.hip — measured scans held against the occupancy grid along their beams (include/icpmi.h: icpmi_grid_check_batch).
// The matchers score the map under a scan's end points and cannot see a beam that ends on a wall after passing through
// another wall; the cast reads ranges back and leaves the comparison to the host.  This walks every measured beam of a
// (cloud, pose) pair from the pose's cell to the cell of its own hit — the cells update_scan would touch for it — over the
// cast's bit planes (gridcast.hpp: GcPlanes, gc_walk), classifies the beam against what the map holds and counts the classes
// per pair on the device: eight int32 per pair come back.
//   gk_check_kernel     one workgroup per (pair, chunk of PAIR_THREADS rows), a lane per row, so a wave holds 64 consecutive
//                       rows of one scan: neighbouring bearings, neighbouring words of the planes.  The cells are the
//                       matcher's (gridmatch.hpp: gm_cell), the walk is the cast's.  Ballots count the classes per wave, LDS
//                       adds them per workgroup, one int32 atomicAdd per non-zero counter goes to the pair's record;
//   pair_status_kernel  (gridpairs.hpp) a lane per pair, after the counts: the record's status.
// The pair list, the frame of a workgroup, the counters, the plan and the launch are gridpairs.hpp's, shared with the beam
// model; this file holds which cells a row forms, how it is classified and what is counted.
// After the cells are formed everything is integer, and integer atomics commute: a record is a function of the inputs alone.
#include "gridmatch.hpp"

namespace icpmi {

static_assert(GM_CELL_MAX == RC_COORD_MAX, "a row's cell is a cell the walk takes unclamped");
static_assert(2 * (long long)GM_CELL_MAX <= (1ll << 30) && ICPMI_GK_MAX_TOLERANCE == 1 << 30, "K - tolerance lies in [-2^30, 2^30]");
static_assert(ICPMI_GK_REC_CONFIRMED + ICPMI_GK_CLASS_UNEXPLORED == ICPMI_GK_REC_UNEXPLORED, "a class's counter is slot CONFIRMED + class");
static_assert(ICPMI_GK_REC_THROUGH_UNKNOWN < ICPMI_GK_INTS, "the counters fit the record");

struct GkArgs {
    const unsigned char* planes;                               // (null only for an empty grid: no step is inside it)
    int ny, nx;
    GmPairs pairs;                                             // cos_sin: [n_pairs][2]; pts 16-byte aligned
    int tolerance, n_chunks, n_pairs, row_stride;
    int32_t* records;                                          // [n_pairs][ICPMI_GK_INTS], zeroed on the stream before the launch
    int4* rows;                                                // [n_pairs][row_stride], or null
};

__global__ __launch_bounds__(PAIR_THREADS) void gk_check_kernel(GkArgs a) {
    __shared__ int counts[ICPMI_GK_INTS];
    const GmPairs& pl = a.pairs;
    const int tid = threadIdx.x;
    const GmFrame f = gm_frame(pl, blockIdx.x, a.n_chunks);
    if (f.base >= f.N) return;                                 // uniform per workgroup, before any barrier (CAPACITY: N = -1)
    const size_t b = f.b;
    if (tid < ICPMI_GK_INTS) counts[tid] = 0;
    __syncthreads();
    const int row = f.base + tid;
    bool cells = false, through = false;
    int cls = ICPMI_GK_NO_CELLS;
    if (row < f.N) {
        const double2 p = reinterpret_cast<const double2*>(pl.pts)[(size_t)pl.off[f.c] + row];
        const double tx = pl.pair_t[2 * b], ty = pl.pair_t[2 * b + 1];
        double wx, wy;
        gm_world(p.x, p.y, pl.cos_sin[2 * b], pl.cos_sin[2 * b + 1], tx, ty, wx, wy);
        int ox = 0, oy = 0, cx = 0, cy = 0;
        cells = gm_cell(tx, pl.min_x, pl.res, ox) && gm_cell(ty, pl.min_y, pl.res, oy) && gm_cell(wx, pl.min_x, pl.res, cx) &&
                gm_cell(wy, pl.min_y, pl.res, cy);
        int4 out = make_int4(ICPMI_GK_NO_CELLS, 0, 0, ICPMI_GC_NONE);
        if (cells) {
            const GcPlanes L(a.ny, a.nx);
            const int4 rec = gc_walk(a.planes, L, a.ny, a.nx, ox, oy, cx, cy);
            const int K = max(abs(cx - ox), abs(cy - oy));         // <= 2^30
            if (rec.x >= 0) cls = rec.x >= K - a.tolerance ? ICPMI_GK_CLASS_CONFIRMED : ICPMI_GK_CLASS_VIOLATED;
            else cls = gc_observed(a.planes, L, a.ny, a.nx, cx, cy) ? ICPMI_GK_CLASS_IN_FREE : ICPMI_GK_CLASS_UNEXPLORED;   // the end cell
            through = rec.w >= 0;
            out = make_int4(cls, rec.x, K, rec.w);
        }
        if (a.rows) a.rows[b * a.row_stride + row] = out;              // one 16-byte store
    }
    pair_count(&counts[ICPMI_GK_REC_ROWS], cells);
    pair_count(&counts[ICPMI_GK_REC_THROUGH_UNKNOWN], through);
#pragma unroll
    for (int k = 0; k < 4; ++k) pair_count(&counts[ICPMI_GK_REC_CONFIRMED + k], cells && cls == k);
    __syncthreads();
    pair_flush(counts, ICPMI_GK_REC_ROWS, ICPMI_GK_REC_THROUGH_UNKNOWN, a.records + b * ICPMI_GK_INTS);
}

}  // namespace icpmi

extern "C" int icpmi_grid_check_batch(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                                      double min_x, double min_y, double resolution, const double* pts, const int32_t* off_dev,
                                      const int32_t* off_host, const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                                      const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                                      int32_t tolerance, int32_t* out_records, int32_t* out_rows, int32_t row_stride,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (n_pairs == 0) return ICPMI_OK;
    const PairPlan plan = plan_pairs(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (!world_ok(resolution, min_x, min_y)) return ICPMI_ERR_ARG;
    if (tolerance < 0 || tolerance > ICPMI_GK_MAX_TOLERANCE) return ICPMI_ERR_ARG;
    const GkArgs a{nullptr, ny, nx, {min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin},
                   tolerance, 0, n_pairs, row_stride, out_records, reinterpret_cast<int4*>(out_rows)};
    if (!pair_rows_ok(plan, a.pairs, out_records, out_rows, row_stride)) return ICPMI_ERR_ARG;
    const GcSource src = resolve_planes(plan.grid, field, planes, workspace, workspace_bytes);
    if (src.rc != ICPMI_OK) return src.rc;
    return launch_pair_rows(plan, src, field, occ_threshold, gk_check_kernel, a, nullptr, 0, (hipStream_t)stream);
}
