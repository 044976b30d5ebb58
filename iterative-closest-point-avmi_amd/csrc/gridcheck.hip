// gridcheck.hip — measured scans held against the occupancy grid along their beams (include/icpmi.h: icpmi_grid_check_batch).
// The matchers score the map under a scan's end points and cannot see a beam that ends on a wall after passing through
// another wall; the cast reads ranges back and leaves the comparison to the host.  This walks every measured beam of a
// (cloud, pose) pair from the pose's cell to the cell of its own hit — the cells update_scan would touch for it — over the
// cast's bit planes (gridcast.hpp: GcPlanes, gc_walk), classifies the beam against what the map holds and counts the classes
// per pair on the device: eight int32 per pair come back.
//   gk_check_kernel   one workgroup per (pair, chunk of GK_CHUNK rows), a lane per row, so a wave holds 64 consecutive rows
//                     of one scan: neighbouring bearings, neighbouring words of the planes.  The cells are the matcher's
//                     (gridmatch.hpp: gm_cell, gm_rows), the walk is the cast's.  Ballots count the classes per wave, LDS
//                     adds them per workgroup, one int32 atomicAdd per non-zero counter goes to the pair's record;
//   gk_status_kernel  a lane per pair, after the counts: the record's status.
// After the cells are formed everything is integer, and integer atomics commute: a record is a function of the inputs alone.
#include "gridpairs.hpp"
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GK_THREADS = ICPMI_GK_THREADS;
constexpr int GK_CHUNK = ICPMI_GK_CHUNK_ROWS;                  // rows of one workgroup
static_assert(GK_CHUNK == GK_THREADS, "a lane handles one row of the chunk");
static_assert(GK_THREADS % ICPMI_WAVE == 0, "whole waves");
static_assert(GM_CELL_MAX == RC_COORD_MAX, "a row's cell is a cell the walk takes unclamped");
static_assert(2 * (long long)GM_CELL_MAX <= (1ll << 30) && ICPMI_GK_MAX_TOLERANCE == 1 << 30, "K - tolerance lies in [-2^30, 2^30]");
static_assert(ICPMI_GK_REC_CONFIRMED + ICPMI_GK_CLASS_UNEXPLORED == ICPMI_GK_REC_UNEXPLORED, "a class's counter is slot CONFIRMED + class");
static_assert(ICPMI_GK_REC_THROUGH_UNKNOWN < ICPMI_GK_INTS, "the counters fit the record");

struct GkArgs {
    const unsigned char* planes;                               // (null only for an empty grid: no step is inside it)
    int ny, nx;
    double min_x, min_y, res;
    const double* pts;
    const int32_t* off;
    const int32_t* cnt;
    const int32_t* pair_cloud;
    const double* pair_t;
    const double* cos_sin;
    int tolerance, n_chunks, n_pairs, row_stride;
    int32_t* records;                                          // [n_pairs][ICPMI_GK_INTS], zeroed on the stream before the launch
    int4* rows;                                                // [n_pairs][row_stride], or null
};

__global__ __launch_bounds__(GK_THREADS) void gk_check_kernel(GkArgs a) {
    __shared__ int counts[ICPMI_GK_INTS];
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x / (unsigned)a.n_chunks;
    const int base = (int)(blockIdx.x - b * (unsigned)a.n_chunks) * GK_CHUNK;
    const int c = a.pair_cloud[b];
    const int N = gm_rows(a.off, a.cnt, c);
    if (base >= N) return;                                     // uniform per workgroup, before any barrier (CAPACITY: N = -1)
    if (tid < ICPMI_GK_INTS) counts[tid] = 0;
    __syncthreads();
    const int row = base + tid;
    bool cells = false, through = false;
    int cls = ICPMI_GK_NO_CELLS;
    if (row < N) {
        // as include/icpmi.h states it: every operation rounded on its own (no contraction)
        const double2 p = reinterpret_cast<const double2*>(a.pts)[(size_t)a.off[c] + row];
        const double co = a.cos_sin[2 * (size_t)b], si = a.cos_sin[2 * (size_t)b + 1];
        const double tx = a.pair_t[2 * (size_t)b], ty = a.pair_t[2 * (size_t)b + 1];
        const double wx = (co * p.x - si * p.y) + tx;
        const double wy = (si * p.x + co * p.y) + ty;
        int ox = 0, oy = 0, cx = 0, cy = 0;
        cells = gm_cell(tx, a.min_x, a.res, ox) && gm_cell(ty, a.min_y, a.res, oy) && gm_cell(wx, a.min_x, a.res, cx) &&
                gm_cell(wy, a.min_y, a.res, cy);
        int4 out = make_int4(ICPMI_GK_NO_CELLS, 0, 0, ICPMI_GC_NONE);
        if (cells) {
            const GcPlanes L(a.ny, a.nx);
            const int4 rec = gc_walk(a.planes, L, a.ny, a.nx, ox, oy, cx, cy);
            const int K = max(abs(cx - ox), abs(cy - oy));         // <= 2^30
            if (rec.x >= 0) {
                cls = rec.x >= K - a.tolerance ? ICPMI_GK_CLASS_CONFIRMED : ICPMI_GK_CLASS_VIOLATED;
            } else {
                // one more masked read: the end cell's unknown bit (a cell outside the grid is not observed space either)
                bool observed = false;
                if ((unsigned)cx < (unsigned)a.nx && (unsigned)cy < (unsigned)a.ny) {
                    const uint32_t* unk = reinterpret_cast<const uint32_t*>(a.planes + L.unk);
                    observed = !(unk[(uint32_t)cy * (uint32_t)L.wpr + (uint32_t)(cx >> 5)] & (1u << (cx & 31)));
                }
                cls = observed ? ICPMI_GK_CLASS_IN_FREE : ICPMI_GK_CLASS_UNEXPLORED;
            }
            through = rec.w >= 0;
            out = make_int4(cls, rec.x, K, rec.w);
        }
        if (a.rows) a.rows[(size_t)b * a.row_stride + row] = out;      // one 16-byte store
    }
    // per wave: a 64-bit ballot and a population count per counter, one LDS add each
    const unsigned long long with_cells = __ballot(cells), through_unknown = __ballot(through);
    unsigned long long of_class[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) of_class[k] = __ballot(cells && cls == k);
    if (lane_id() == 0) {
        if (with_cells) atomicAdd(&counts[ICPMI_GK_REC_ROWS], __popcll(with_cells));
        if (through_unknown) atomicAdd(&counts[ICPMI_GK_REC_THROUGH_UNKNOWN], __popcll(through_unknown));
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (of_class[k]) atomicAdd(&counts[ICPMI_GK_REC_CONFIRMED + k], __popcll(of_class[k]));
    }
    __syncthreads();
    if (tid >= ICPMI_GK_REC_ROWS && tid <= ICPMI_GK_REC_THROUGH_UNKNOWN && counts[tid])
        atomicAdd(a.records + (size_t)b * ICPMI_GK_INTS + tid, counts[tid]);
}

// Behind the counts on the stream: CAPACITY by the matcher's rule (nothing was read, the memset's zeros stay), else EMPTY
// where no row had a cell.
__global__ __launch_bounds__(GK_THREADS) void gk_status_kernel(GkArgs a) {
    const unsigned b = blockIdx.x * GK_THREADS + threadIdx.x;
    if (b >= (unsigned)a.n_pairs) return;
    int32_t* rec = a.records + (size_t)b * ICPMI_GK_INTS;
    const int N = gm_rows(a.off, a.cnt, a.pair_cloud[b]);
    rec[ICPMI_GK_REC_STATUS] = N < 0 ? ICPMI_GK_ST_CAPACITY : (rec[ICPMI_GK_REC_ROWS] > 0 ? ICPMI_GK_ST_OK : ICPMI_GK_ST_EMPTY);
}

// ── host: the plan, the entry ────────────────────────────────────────────────
// What a call starts, decided as a whole and without a HIP call: the plan of the pairs (gridpairs.hpp: the grid's GcPlan,
// the (pair, chunk) grid, the status grid) and the bytes zeroed.  The chunk never depends on the batch and the sums are
// integers: a pair's record does not depend on the batch it is computed in.
struct GkPlan : PairPlan {
    size_t record_bytes;      // what is zeroed before the launch
};
static GkPlan plan_check(int ny, int nx, int n_pairs, int n_clouds, const int32_t* off_host, const int32_t* pair_cloud_host) {
    GkPlan p{plan_pairs(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host, GK_CHUNK, GK_THREADS), 0};
    if (p.rc == ICPMI_OK) p.record_bytes = (size_t)n_pairs * ICPMI_GK_INTS * sizeof(int32_t);
    return p;
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
    const GkPlan plan = plan_check(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host);
    if (plan.rc != ICPMI_OK) return plan.rc;
    const double inf = __builtin_inf();
    if (!(resolution > 0.0 && resolution < inf) || !(fabs(min_x) < inf) || !(fabs(min_y) < inf)) return ICPMI_ERR_ARG;
    if (tolerance < 0 || tolerance > ICPMI_GK_MAX_TOLERANCE) return ICPMI_ERR_ARG;
    if (!pts || !off_dev || !pair_cloud || !pair_t || !cos_sin || !out_records || misaligned16(pts)) return ICPMI_ERR_ARG;
    if (out_rows && (misaligned16(out_rows) || row_stride < plan.max_n)) return ICPMI_ERR_ARG;
    const bool pack = !planes && plan.grid.plane_blocks;
    if (planes && misaligned16(planes)) return ICPMI_ERR_ARG;
    if (pack) {
        if (!field || misaligned16(field)) return ICPMI_ERR_ARG;
        if (!workspace || misaligned16(workspace) || workspace_bytes < plan.grid.plane_bytes) return ICPMI_ERR_WORKSPACE;
    }

    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_records, 0, plan.record_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    GkArgs a{(const unsigned char*)planes, ny, nx, min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin,
             tolerance, plan.n_chunks, n_pairs, row_stride, out_records, reinterpret_cast<int4*>(out_rows)};
    if (plan.row_grid) {
        if (pack) {
            const int rc = launch_planes(plan.grid, field, ny, nx, occ_threshold, workspace, st);
            if (rc != ICPMI_OK) return rc;
            a.planes = (const unsigned char*)workspace;
        }
        gk_check_kernel<<<plan.row_grid, GK_THREADS, 0, st>>>(a);
        ICPMI_LAUNCH_CHECK();
    }
    gk_status_kernel<<<plan.status_grid, GK_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
