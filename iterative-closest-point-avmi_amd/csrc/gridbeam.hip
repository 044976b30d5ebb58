// gridbeam.hip — the beam model: measured scans scored against the ranges the occupancy grid expects (include/icpmi.h:
// icpmi_grid_beam_batch).  The check (gridcheck.hip) walks a measured beam to its own return and sorts it into four classes
// with a hard tolerance; this walks the same beam `beyond` metres past its return over the cast's bit planes (gridcast.hpp:
// GcPlanes, gc_walk), takes the signed number of steps between the map's first wall and the step at which the beam
// returned, and adds the entry of a caller's table at that difference: one int32 score per (cloud, pose) pair, with the
// histogram of the differences and the rows' own records on request.
//   gb_beam_kernel    one workgroup per (pair, chunk of GB_CHUNK rows), a lane per row, so a wave holds 64 consecutive rows
//                     of one scan.  The cells are the matcher's (gridmatch.hpp: gm_cell, gm_rows), the walk is the cast's.
//                     The clipped table is staged into LDS; the score is summed per wave and added to LDS once per wave,
//                     ballots count the rows, and one int32 atomicAdd per non-zero slot and per non-zero bin goes out;
//   gb_status_kernel  a lane per pair, after the sums: the record's status.
// After the cells are formed everything is integer, and integer atomics commute: a record is a function of the inputs alone.
#include "gridpairs.hpp"
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GB_THREADS = ICPMI_GB_THREADS;
constexpr int GB_CHUNK = ICPMI_GB_CHUNK_ROWS;                  // rows of one workgroup
constexpr int GB_MAX_BINS = 2 * ICPMI_GB_MAX_HALF_WIDTH + 3;   // the table's entries at the widest half width
static_assert(GB_CHUNK == GB_THREADS, "a lane handles one row of the chunk");
static_assert(GB_THREADS % ICPMI_WAVE == 0, "whole waves");
static_assert(GM_CELL_MAX == RC_COORD_MAX, "a row's cell is a cell the walk takes unclamped");
static_assert(2 * (long long)GM_CELL_MAX <= (1ll << 30), "k_hit and k_z lie in [-1, 2^30]: their difference is an int32");
static_assert((long long)ICPMI_GB_TABLE_CLIP * ICPMI_GM_MAX_ROWS < (1ll << 31), "a score, and every partial sum of one, is an int32");
static_assert(ICPMI_GB_REC_UNEXPLORED < ICPMI_GB_INTS && GB_MAX_BINS == 257, "the counters fit the record; the table fits its LDS");

struct GbArgs {
    const unsigned char* planes;                               // (null only for an empty grid: no step is inside it)
    int ny, nx;
    double min_x, min_y, res;
    const double* pts;
    const int32_t* off;
    const int32_t* cnt;
    const int32_t* pair_cloud;
    const double* pair_t;
    const double* cos_sin;
    double beyond;
    const int32_t* table;                                      // [2 * half_width + 3]
    int half_width, n_chunks, n_pairs, row_stride;
    int32_t* records;                                          // [n_pairs][ICPMI_GB_INTS], zeroed on the stream before the launch
    int32_t* hist;                                             // [n_pairs][2 * half_width + 3], zeroed likewise, or null
    int4* rows;                                                // [n_pairs][row_stride], or null
};

__global__ __launch_bounds__(GB_THREADS) void gb_beam_kernel(GbArgs a) {
    __shared__ int table[GB_MAX_BINS];
    __shared__ int bins[GB_MAX_BINS];
    __shared__ int counts[ICPMI_GB_INTS];
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x / (unsigned)a.n_chunks;
    const int base = (int)(blockIdx.x - b * (unsigned)a.n_chunks) * GB_CHUNK;
    const int c = a.pair_cloud[b];
    const int N = gm_rows(a.off, a.cnt, c);
    if (base >= N) return;                                     // uniform per workgroup, before any barrier (CAPACITY: N = -1)
    const int H = a.half_width, n_bins = 2 * H + 3;            // <= GB_MAX_BINS: the host refuses a wider table
    for (int i = tid; i < n_bins; i += GB_THREADS) {
        table[i] = min(max(a.table[i], -ICPMI_GB_TABLE_CLIP), ICPMI_GB_TABLE_CLIP);
        bins[i] = 0;
    }
    if (tid < ICPMI_GB_INTS) counts[tid] = 0;
    __syncthreads();
    const int row = base + tid;
    bool cells = false;
    int idx = ICPMI_GB_NO_CELLS, k_hit = ICPMI_GC_NONE, value = 0;
    if (row < N) {
        // as include/icpmi.h states it: every operation rounded on its own (no contraction)
        const double2 p = reinterpret_cast<const double2*>(a.pts)[(size_t)a.off[c] + row];
        const double co = a.cos_sin[2 * (size_t)b], si = a.cos_sin[2 * (size_t)b + 1];
        const double tx = a.pair_t[2 * (size_t)b], ty = a.pair_t[2 * (size_t)b + 1];
        const double r = sqrt(p.x * p.x + p.y * p.y);
        const double s = (r + a.beyond) / r;                   // (r = 0: inf or NaN, and the far end has no cell)
        const double fx = p.x * s, fy = p.y * s;
        const double hwx = (co * p.x - si * p.y) + tx, hwy = (si * p.x + co * p.y) + ty;
        const double fwx = (co * fx - si * fy) + tx, fwy = (si * fx + co * fy) + ty;
        int ox = 0, oy = 0, hx = 0, hy = 0, ex = 0, ey = 0;
        cells = gm_cell(tx, a.min_x, a.res, ox) && gm_cell(ty, a.min_y, a.res, oy) && gm_cell(hwx, a.min_x, a.res, hx) &&
                gm_cell(hwy, a.min_y, a.res, hy) && gm_cell(fwx, a.min_x, a.res, ex) && gm_cell(fwy, a.min_y, a.res, ey);
        int4 out = make_int4(ICPMI_GB_NO_CELLS, 0, 0, ICPMI_GC_NONE);
        if (cells) {
            const GcPlanes L(a.ny, a.nx);
            const int4 rec = gc_walk(a.planes, L, a.ny, a.nx, ox, oy, ex, ey);
            k_hit = rec.x;
            // the step at which the beam returned, on the major axis of the walk (the walk's rule: x where |dx| >= |dy|)
            const int k_z = abs(ex - ox) >= abs(ey - oy) ? abs(hx - ox) : abs(hy - oy);      // <= 2^30
            if (k_hit >= 0) {
                idx = min(max(k_hit - k_z, -H), H) + H;
            } else {
                // one more masked read: the hit cell's unknown bit (a cell outside the grid is not observed space either)
                bool observed = false;
                if ((unsigned)hx < (unsigned)a.nx && (unsigned)hy < (unsigned)a.ny) {
                    const uint32_t* unk = reinterpret_cast<const uint32_t*>(a.planes + L.unk);
                    observed = !(unk[(uint32_t)hy * (uint32_t)L.wpr + (uint32_t)(hx >> 5)] & (1u << (hx & 31)));
                }
                idx = observed ? 2 * H + 1 : 2 * H + 2;
            }
            value = table[idx];
            if (a.hist) atomicAdd(&bins[idx], 1);
            out = make_int4(idx, k_hit, k_z, rec.w);
        }
        if (a.rows) a.rows[(size_t)b * a.row_stride + row] = out;      // one 16-byte store
    }
    // per wave: the score's sum, a 64-bit ballot and a population count per counter, one LDS add each
    const int score = wave_sum(value);
    const unsigned long long with_cells = __ballot(cells), expected = __ballot(cells && k_hit >= 0);
    const unsigned long long novel = __ballot(cells && idx == 2 * H + 1), unexplored = __ballot(cells && idx == 2 * H + 2);
    if (lane_id() == 0) {
        if (with_cells) atomicAdd(&counts[ICPMI_GB_REC_ROWS], __popcll(with_cells));
        if (score) atomicAdd(&counts[ICPMI_GB_REC_SCORE], score);
        if (expected) atomicAdd(&counts[ICPMI_GB_REC_EXPECTED], __popcll(expected));
        if (novel) atomicAdd(&counts[ICPMI_GB_REC_NOVEL], __popcll(novel));
        if (unexplored) atomicAdd(&counts[ICPMI_GB_REC_UNEXPLORED], __popcll(unexplored));
    }
    __syncthreads();
    if (tid >= ICPMI_GB_REC_ROWS && tid <= ICPMI_GB_REC_UNEXPLORED && counts[tid])
        atomicAdd(a.records + (size_t)b * ICPMI_GB_INTS + tid, counts[tid]);
    if (a.hist)
        for (int i = tid; i < n_bins; i += GB_THREADS)
            if (bins[i]) atomicAdd(a.hist + (size_t)b * n_bins + i, bins[i]);
}

// Behind the sums on the stream: CAPACITY by the matcher's rule (nothing was read, the memset's zeros stay), else EMPTY
// where no row had a cell.
__global__ __launch_bounds__(GB_THREADS) void gb_status_kernel(GbArgs a) {
    const unsigned b = blockIdx.x * GB_THREADS + threadIdx.x;
    if (b >= (unsigned)a.n_pairs) return;
    int32_t* rec = a.records + (size_t)b * ICPMI_GB_INTS;
    const int N = gm_rows(a.off, a.cnt, a.pair_cloud[b]);
    rec[ICPMI_GB_REC_STATUS] = N < 0 ? ICPMI_GB_ST_CAPACITY : (rec[ICPMI_GB_REC_ROWS] > 0 ? ICPMI_GB_ST_OK : ICPMI_GB_ST_EMPTY);
}

// ── host: the plan, the entry ────────────────────────────────────────────────
// What a call starts, decided as a whole and without a HIP call: the plan of the pairs (gridpairs.hpp, the check's) and
// the bytes zeroed.
struct GbPlan : PairPlan {
    size_t record_bytes;      // the records: always zeroed before the launch
    size_t hist_bytes;        // the histograms: zeroed when one was asked for
};
static GbPlan plan_beam(int ny, int nx, int n_pairs, int n_clouds, const int32_t* off_host, const int32_t* pair_cloud_host, int half_width) {
    GbPlan p{plan_pairs(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host, GB_CHUNK, GB_THREADS), 0, 0};
    if (p.rc != ICPMI_OK) return p;
    if (half_width < 0 || half_width > ICPMI_GB_MAX_HALF_WIDTH) { p.rc = ICPMI_ERR_ARG; return p; }
    p.record_bytes = (size_t)n_pairs * ICPMI_GB_INTS * sizeof(int32_t);
    p.hist_bytes = (size_t)n_pairs * (2 * half_width + 3) * sizeof(int32_t);
    return p;
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
    const GbPlan plan = plan_beam(ny, nx, n_pairs, n_clouds, off_host, pair_cloud_host, half_width);
    if (plan.rc != ICPMI_OK) return plan.rc;
    const double inf = __builtin_inf();
    if (!(resolution > 0.0 && resolution < inf) || !(fabs(min_x) < inf) || !(fabs(min_y) < inf)) return ICPMI_ERR_ARG;
    if (!(beyond >= 0.0 && beyond < inf)) return ICPMI_ERR_ARG;
    if (!pts || !off_dev || !pair_cloud || !pair_t || !cos_sin || !table || !out_records || misaligned16(pts) || misaligned16(table))
        return ICPMI_ERR_ARG;
    if (out_hist && misaligned16(out_hist)) return ICPMI_ERR_ARG;
    if (out_rows && (misaligned16(out_rows) || row_stride < plan.max_n)) return ICPMI_ERR_ARG;
    const bool pack = !planes && plan.grid.plane_blocks;
    if (planes && misaligned16(planes)) return ICPMI_ERR_ARG;
    if (pack) {
        if (!field || misaligned16(field)) return ICPMI_ERR_ARG;
        if (!workspace || misaligned16(workspace) || workspace_bytes < plan.grid.plane_bytes) return ICPMI_ERR_WORKSPACE;
    }

    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_records, 0, plan.record_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (out_hist && hipMemsetAsync(out_hist, 0, plan.hist_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    GbArgs a{(const unsigned char*)planes, ny, nx, min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin,
             beyond, table, half_width, plan.n_chunks, n_pairs, row_stride, out_records, out_hist, reinterpret_cast<int4*>(out_rows)};
    if (plan.row_grid) {
        if (pack) {
            const int rc = launch_planes(plan.grid, field, ny, nx, occ_threshold, workspace, st);
            if (rc != ICPMI_OK) return rc;
            a.planes = (const unsigned char*)workspace;
        }
        gb_beam_kernel<<<plan.row_grid, GB_THREADS, 0, st>>>(a);
        ICPMI_LAUNCH_CHECK();
    }
    gb_status_kernel<<<plan.status_grid, GB_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
