// gridbeam.hip — the beam model: measured scans scored against the ranges the occupancy grid expects (include/icpmi.h:
// icpmi_grid_beam_batch).  The check (gridcheck.hip) walks a measured beam to its own return and sorts it into four classes
// with a hard tolerance; this walks the same beam `beyond` metres past its return over the cast's bit planes (gridcast.hpp:
// GcPlanes, gc_walk), takes the signed number of steps between the map's first wall and the step at which the beam
// returned, and adds the entry of a caller's table at that difference: one int32 score per (cloud, pose) pair, with the
// histogram of the differences and the rows' own records on request.
//   gb_beam_kernel      one workgroup per (pair, chunk of PAIR_THREADS rows), a lane per row, so a wave holds 64 consecutive
//                       rows of one scan.  The cells are the matcher's (gridmatch.hpp: gm_cell), the walk is the cast's.
//                       The clipped table is staged into LDS; the score is summed per wave and added to LDS once per wave,
//                       ballots count the rows, and one int32 atomicAdd per non-zero slot and per non-zero bin goes out;
//   pair_status_kernel  (gridpairs.hpp) a lane per pair, after the sums: the record's status.
// The pair list, the frame of a workgroup, the counters, the plan and the launch are gridpairs.hpp's, shared with the check;
// this file holds which cells a row forms, how its difference indexes the table and what is summed.
// After the cells are formed everything is integer, and integer atomics commute: a record is a function of the inputs alone.
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GB_MAX_BINS = 2 * ICPMI_GB_MAX_HALF_WIDTH + 3;   // the table's entries at the widest half width
static_assert(GM_CELL_MAX == RC_COORD_MAX, "a row's cell is a cell the walk takes unclamped");
static_assert(2 * (long long)GM_CELL_MAX <= (1ll << 30), "k_hit and k_z lie in [-1, 2^30]: their difference is an int32");
static_assert((long long)ICPMI_GB_TABLE_CLIP * ICPMI_GM_MAX_ROWS < (1ll << 31), "a score, and every partial sum of one, is an int32");
static_assert(ICPMI_GB_REC_UNEXPLORED < ICPMI_GB_INTS && GB_MAX_BINS == 257, "the counters fit the record; the table fits its LDS");

struct GbArgs {
    const unsigned char* planes;                               // (null only for an empty grid: no step is inside it)
    int ny, nx;
    GmPairs pairs;                                             // cos_sin: [n_pairs][2]; pts 16-byte aligned
    double beyond;
    const int32_t* table;                                      // [2 * half_width + 3]
    int half_width, n_chunks, n_pairs, row_stride;
    int32_t* records;                                          // [n_pairs][ICPMI_GB_INTS], zeroed on the stream before the launch
    int32_t* hist;                                             // [n_pairs][2 * half_width + 3], zeroed likewise, or null
    int4* rows;                                                // [n_pairs][row_stride], or null
};

__global__ __launch_bounds__(PAIR_THREADS) void gb_beam_kernel(GbArgs a) {
    __shared__ int table[GB_MAX_BINS];
    __shared__ int bins[GB_MAX_BINS];
    __shared__ int counts[ICPMI_GB_INTS];
    const GmPairs& pl = a.pairs;
    const int tid = threadIdx.x;
    const GmFrame f = gm_frame(pl, blockIdx.x, a.n_chunks);
    if (f.base >= f.N) return;                                 // uniform per workgroup, before any barrier (CAPACITY: N = -1)
    const size_t b = f.b;
    const int H = a.half_width, n_bins = 2 * H + 3;            // <= GB_MAX_BINS: the host refuses a wider table
    for (int i = tid; i < n_bins; i += PAIR_THREADS) {
        table[i] = min(max(a.table[i], -ICPMI_GB_TABLE_CLIP), ICPMI_GB_TABLE_CLIP);
        bins[i] = 0;
    }
    if (tid < ICPMI_GB_INTS) counts[tid] = 0;
    __syncthreads();
    const int row = f.base + tid;
    bool cells = false;
    int idx = ICPMI_GB_NO_CELLS, k_hit = ICPMI_GC_NONE, value = 0;
    if (row < f.N) {
        const double2 p = reinterpret_cast<const double2*>(pl.pts)[(size_t)pl.off[f.c] + row];
        const double co = pl.cos_sin[2 * b], si = pl.cos_sin[2 * b + 1];
        const double tx = pl.pair_t[2 * b], ty = pl.pair_t[2 * b + 1];
        const double r = sqrt(p.x * p.x + p.y * p.y);
        const double s = (r + a.beyond) / r;                   // (r = 0: inf or NaN, and the far end has no cell)
        double hwx, hwy, fwx, fwy;
        gm_world(p.x, p.y, co, si, tx, ty, hwx, hwy);
        gm_world(p.x * s, p.y * s, co, si, tx, ty, fwx, fwy);
        int ox = 0, oy = 0, hx = 0, hy = 0, ex = 0, ey = 0;
        cells = gm_cell(tx, pl.min_x, pl.res, ox) && gm_cell(ty, pl.min_y, pl.res, oy) && gm_cell(hwx, pl.min_x, pl.res, hx) &&
                gm_cell(hwy, pl.min_y, pl.res, hy) && gm_cell(fwx, pl.min_x, pl.res, ex) && gm_cell(fwy, pl.min_y, pl.res, ey);
        int4 out = make_int4(ICPMI_GB_NO_CELLS, 0, 0, ICPMI_GC_NONE);
        if (cells) {
            const GcPlanes L(a.ny, a.nx);
            const int4 rec = gc_walk(a.planes, L, a.ny, a.nx, ox, oy, ex, ey);
            k_hit = rec.x;
            // the step at which the beam returned, on the major axis of the walk (the walk's rule: x where |dx| >= |dy|)
            const int k_z = abs(ex - ox) >= abs(ey - oy) ? abs(hx - ox) : abs(hy - oy);      // <= 2^30
            if (k_hit >= 0) idx = min(max(k_hit - k_z, -H), H) + H;
            else idx = gc_observed(a.planes, L, a.ny, a.nx, hx, hy) ? 2 * H + 1 : 2 * H + 2;    // the hit cell
            value = table[idx];
            if (a.hist) atomicAdd(&bins[idx], 1);
            out = make_int4(idx, k_hit, k_z, rec.w);
        }
        if (a.rows) a.rows[b * a.row_stride + row] = out;              // one 16-byte store
    }
    // per wave: the score's sum, one LDS add; the counters
    const int score = wave_sum(value);
    if (lane_id() == 0 && score) atomicAdd(&counts[ICPMI_GB_REC_SCORE], score);
    pair_count(&counts[ICPMI_GB_REC_ROWS], cells);
    pair_count(&counts[ICPMI_GB_REC_EXPECTED], cells && k_hit >= 0);
    pair_count(&counts[ICPMI_GB_REC_NOVEL], cells && idx == 2 * H + 1);
    pair_count(&counts[ICPMI_GB_REC_UNEXPLORED], cells && idx == 2 * H + 2);
    __syncthreads();
    pair_flush(counts, ICPMI_GB_REC_ROWS, ICPMI_GB_REC_UNEXPLORED, a.records + b * ICPMI_GB_INTS);
    if (a.hist)
        for (int i = tid; i < n_bins; i += PAIR_THREADS)
            if (bins[i]) atomicAdd(a.hist + b * n_bins + i, bins[i]);
}

}  // namespace icpmi

extern "C" int icpmi_grid_beam_batch(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                                     double min_x, double min_y, double resolution, const double* pts, const int32_t* off_dev,
                                     const int32_t* off_host, const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                                     const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                                     double beyond, int32_t half_width, const int32_t* table, int32_t* out_records, int32_t* out_hist,
                                     int32_t* out_rows, int32_t row_stride, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (n_pairs == 0) return ICPMI_OK;
    const PairPlan plan = plan_pairs(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (half_width < 0 || half_width > ICPMI_GB_MAX_HALF_WIDTH) return ICPMI_ERR_ARG;
    if (!world_ok(resolution, min_x, min_y) || !(beyond >= 0.0 && beyond < __builtin_inf())) return ICPMI_ERR_ARG;
    const GbArgs a{nullptr, ny, nx, {min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin}, beyond, table,
                   half_width, 0, n_pairs, row_stride, out_records, out_hist, reinterpret_cast<int4*>(out_rows)};
    if (!pair_rows_ok(plan, a.pairs, out_records, out_rows, row_stride)) return ICPMI_ERR_ARG;
    if (!table || misaligned16(table) || (out_hist && misaligned16(out_hist))) return ICPMI_ERR_ARG;
    const GcSource src = resolve_planes(plan.grid, field, planes, workspace, workspace_bytes);
    if (src.rc != ICPMI_OK) return src.rc;
    const size_t hist_bytes = (size_t)n_pairs * (2 * half_width + 3) * sizeof(int32_t);
    return launch_pair_rows(plan, src, field, occ_threshold, gb_beam_kernel, a, out_hist, hist_bytes, (hipStream_t)stream);
}
