// gridpairs.hpp — what every entry shares that holds a list of (cloud, pose) pairs against the occupancy grid (gridmatch.hip,
// gridmatch_wide.hip: the matchers; gridcheck.hip: the check; gridbeam.hip: the beam model).  Device: the pair list in the
// kernel arguments, the rule for a cloud's rows and for a record's status, the (pair, chunk) frame of a workgroup, the rigid
// transform of a row, a record's counters and the status kernel.  Host: the one walk over the host pair list, the world
// refusal, the plan of the row kernels and their launch.  Each exists once, so the entries judge one pair list alike.
#pragma once
#include "gridcast.hpp"

namespace icpmi {

constexpr int PAIR_THREADS = ICPMI_GK_THREADS;                 // a row kernel's workgroup: a lane per row of its chunk
static_assert(ICPMI_GB_THREADS == PAIR_THREADS && ICPMI_GK_CHUNK_ROWS == PAIR_THREADS && ICPMI_GB_CHUNK_ROWS == PAIR_THREADS &&
              PAIR_THREADS % ICPMI_WAVE == 0, "the check and the beam model: whole waves, a lane handles one row of the chunk");
// one status kernel and one rule serve the check, the beam model and the matchers' records
static_assert(ICPMI_GK_INTS == ICPMI_GB_INTS && ICPMI_GK_INTS == ICPMI_GMREC_INTS, "one record width");
static_assert(ICPMI_GK_REC_STATUS == ICPMI_GB_REC_STATUS && ICPMI_GK_REC_STATUS == ICPMI_GMREC_STATUS, "one status slot");
static_assert(ICPMI_GK_REC_ROWS == ICPMI_GB_REC_ROWS && ICPMI_GK_REC_ROWS == ICPMI_GMREC_ROWS, "one rows slot");
static_assert(ICPMI_GK_ST_OK == ICPMI_GB_ST_OK && ICPMI_GK_ST_OK == ICPMI_GM_ST_OK && ICPMI_GK_ST_EMPTY == ICPMI_GB_ST_EMPTY &&
              ICPMI_GK_ST_EMPTY == ICPMI_GM_ST_EMPTY && ICPMI_GK_ST_CAPACITY == ICPMI_GB_ST_CAPACITY &&
              ICPMI_GK_ST_CAPACITY == ICPMI_GM_ST_CAPACITY, "one set of status values");

// The pair list as a kernel reads it: the world, the cloud set, and per pair its cloud, translation and rotation(s)
struct GmPairs {
    double min_x, min_y, res;
    const double* pts;
    const int32_t* off;
    const int32_t* cnt;
    const int32_t* pair_cloud;
    const double* pair_t;
    const double* cos_sin;
};

// rows of a pair's cloud: the device count where the set has one; -1 for a count that is negative (the voxel filter's
// overflow mark) or beyond the cloud's own rows or ICPMI_GM_MAX_ROWS — such a cloud is not read (ICPMI_GM_ST_CAPACITY)
__device__ __forceinline__ int gm_rows(const GmPairs& p, int c) {
    const int cap = p.off[c + 1] - p.off[c];
    const int n = p.cnt ? p.cnt[c] : cap;
    return n < 0 || n > cap || n > ICPMI_GM_MAX_ROWS ? -1 : n;
}

// a record's status, N = gm_rows of the pair's cloud: CAPACITY (nothing was read), else OK if any row had a cell, else EMPTY
__device__ __forceinline__ int gm_status(int N, bool any) { return N < 0 ? ICPMI_GM_ST_CAPACITY : (any ? ICPMI_GM_ST_OK : ICPMI_GM_ST_EMPTY); }

// The frame of workgroup `group` of a (pair, angle, chunk of PAIR_THREADS rows) grid, chunks fastest: the pair b, the angle,
// the first row of the chunk, the pair's cloud c and its N rows.  A workgroup with base >= N has nothing to do (CAPACITY:
// N = -1) and returns — uniformly, before any barrier.
struct GmFrame {
    int b, ang, base, c, N;
};
__device__ __forceinline__ GmFrame gm_frame(const GmPairs& p, unsigned group, int n_chunks, int n_angles = 1) {
    const unsigned unit = group / (unsigned)n_chunks, b = unit / (unsigned)n_angles;
    GmFrame f;
    f.b = (int)b;
    f.ang = (int)(unit - b * (unsigned)n_angles);
    f.base = (int)(group - unit * (unsigned)n_chunks) * PAIR_THREADS;
    f.c = p.pair_cloud[b];
    f.N = gm_rows(p, f.c);
    return f;
}

// world = R (x, y) + t as include/icpmi.h states it: every operation rounded on its own (no contraction)
__device__ __forceinline__ void gm_world(double x, double y, double co, double si, double tx, double ty, double& wx, double& wy) {
    wx = (co * x - si * y) + tx;
    wy = (si * x + co * y) + ty;
}

// A record's counters in LDS.  Per wave: a 64-bit ballot and a population count, one LDS add (none for a count of 0);
// every lane of the workgroup calls it.
__device__ __forceinline__ void pair_count(int* slot, bool flag) {
    const unsigned long long lanes = __ballot(flag);
    if (lane_id() == 0 && lanes) atomicAdd(slot, __popcll(lanes));
}
// Behind the barrier after them: one int32 atomicAdd per non-zero LDS slot in [first, last] into the pair's record
__device__ __forceinline__ void pair_flush(const int* counts, int first, int last, int32_t* rec) {
    const int tid = threadIdx.x;
    if (tid >= first && tid <= last && counts[tid]) atomicAdd(rec + tid, counts[tid]);
}

// A lane per pair, behind the row kernel on the stream: the record's status (CAPACITY: the memset's zeros stay).  A template
// over the record's width, so that it is emitted where it is launched (launch_pair_rows) and the library links one copy.
template <int INTS>
__global__ __launch_bounds__(PAIR_THREADS) void pair_status_kernel(GmPairs p, int n_pairs, int32_t* records) {
    const unsigned b = blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (b >= (unsigned)n_pairs) return;
    int32_t* rec = records + (size_t)b * INTS;
    rec[ICPMI_GK_REC_STATUS] = gm_status(gm_rows(p, p.pair_cloud[b]), rec[ICPMI_GK_REC_ROWS] > 0);
}

// ── host ─────────────────────────────────────────────────────────────────────
// The only walk over the host pair list: every index inside the set, no cloud of negative length.  Which limits apply to
// max_n, total and above is each plan's decision.
struct PairScan {
    int rc;                   // ICPMI_OK or ICPMI_ERR_ARG
    int max_n;                // rows of the largest named cloud
    long long total;          // rows of all pairs
    bool above;               // some named cloud is above ICPMI_GM_MAX_ROWS
};
inline PairScan scan_pairs(int n_pairs, int n_clouds, const int32_t* off_host, const int32_t* pair_cloud_host) {
    PairScan s{ICPMI_OK, 0, 0, false};
    if (n_pairs < 0 || n_clouds < 0 || !off_host || !pair_cloud_host) { s.rc = ICPMI_ERR_ARG; return s; }
    for (int b = 0; b < n_pairs; ++b) {
        const int c = pair_cloud_host[b];
        if (c < 0 || c >= n_clouds) { s.rc = ICPMI_ERR_ARG; return s; }
        const int rows = off_host[c + 1] - off_host[c];
        if (rows < 0) { s.rc = ICPMI_ERR_ARG; return s; }
        s.above |= rows > ICPMI_GM_MAX_ROWS;
        s.max_n = rows > s.max_n ? rows : s.max_n;
        s.total += rows;
    }
    return s;
}

// the world of a map: a positive, finite resolution and a finite corner
inline bool world_ok(double resolution, double min_x, double min_y) {
    const double inf = __builtin_inf();
    return resolution > 0.0 && resolution < inf && fabs(min_x) < inf && fabs(min_y) < inf;
}

// What a row-kernel entry starts, decided as a whole and without a HIP call.  The chunk never depends on the batch: a pair's
// record does not depend on the batch it is computed in.
struct PairPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    GcPlan grid;              // the planes of the grid: what is packed when the call packs, and their size
    unsigned row_grid;        // (pair, chunk) workgroups; 0: no named cloud has a row (the records are still written)
    unsigned status_grid;     // the status kernel: a lane per pair
    int n_chunks, max_n;      // row chunks of, and rows of, the largest named cloud
    size_t record_bytes;      // the records: zeroed before the launch
};
inline PairPlan plan_pairs(int ny, int nx, int n_pairs, int n_clouds, const int32_t* off_host, const int32_t* pair_cloud_host) {
    const PairScan s = scan_pairs(n_pairs, n_clouds, off_host, pair_cloud_host);
    PairPlan p{s.rc, plan_cast(ny, nx, 0, 0), 0, 0, 0, s.max_n, 0};
    if (p.rc != ICPMI_OK) return p;
    if (p.grid.rc != ICPMI_OK) { p.rc = p.grid.rc; return p; }
    p.n_chunks = (p.max_n + PAIR_THREADS - 1) / PAIR_THREADS;
    const unsigned long long groups = (unsigned long long)n_pairs * p.n_chunks;
    if (s.above || s.total >= (1ll << 29) || groups >= (1ull << 31)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.row_grid = (unsigned)groups;
    p.status_grid = (unsigned)(((long long)n_pairs + PAIR_THREADS - 1) / PAIR_THREADS);
    p.record_bytes = (size_t)n_pairs * ICPMI_GK_INTS * sizeof(int32_t);
    return p;
}

// The refusals every row-kernel entry makes of the pair list's device side and of the rows' records
inline bool pair_rows_ok(const PairPlan& plan, const GmPairs& p, const int32_t* records, const int32_t* rows, int row_stride) {
    if (!p.pts || !p.off || !p.pair_cloud || !p.pair_t || !p.cos_sin || !records || misaligned16(p.pts)) return false;
    return !rows || (!misaligned16(rows) && row_stride >= plan.max_n);
}

// What a row-kernel entry enqueues once every refusal has been decided, in this order: the memsets of the records (and of
// the histogram, where there is one), the planes packed from the field where `src` says so, the row kernel where a named
// cloud has a row, the status kernel.  Args: the kernel's argument struct, with planes, ny, nx, pairs, n_chunks, n_pairs and
// records among its members.
template <class Args>
int launch_pair_rows(const PairPlan& plan, const GcSource& src, const int16_t* field, int threshold, void (*row_kernel)(Args), Args a,
                     int32_t* hist, size_t hist_bytes, hipStream_t st) {
    if (hipMemsetAsync(a.records, 0, plan.record_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (hist && hipMemsetAsync(hist, 0, hist_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    a.planes = (const unsigned char*)src.planes;               // (null only for an empty grid: no step is inside it)
    a.n_chunks = plan.n_chunks;
    if (plan.row_grid) {
        if (src.pack) {
            const int rc = launch_planes(plan.grid, field, a.ny, a.nx, threshold, src.workspace, st);
            if (rc != ICPMI_OK) return rc;
        }
        row_kernel<<<plan.row_grid, PAIR_THREADS, 0, st>>>(a);
        ICPMI_LAUNCH_CHECK();
    }
    pair_status_kernel<ICPMI_GK_INTS><<<plan.status_grid, PAIR_THREADS, 0, st>>>(a.pairs, a.n_pairs, a.records);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

}  // namespace icpmi
