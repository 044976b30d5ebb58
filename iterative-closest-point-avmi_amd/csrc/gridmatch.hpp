// gridmatch.hpp — what the scan-to-map kernels share (gridmatch.hip: the exhaustive window; gridmatch_wide.hip: the pruned
// wide window): the arguments, the cell of a row, the workgroup's LDS, phase 1 (the cells of a chunk of rows) and the
// branch-free walk of a lane's shifts over those cells.  Each exists once.  The pair list, the rule for a cloud's rows and
// the frame of a workgroup are gridpairs.hpp's; the check and the beam model form their cells with gm_cell too.
#pragma once
#include "gridpairs.hpp"

namespace icpmi {

constexpr int GM_THREADS = ICPMI_GM_THREADS;
constexpr int GM_WAVES = GM_THREADS / ICPMI_WAVE;
constexpr int GM_CHUNK = ICPMI_GM_CHUNK_ROWS;              // source rows of one workgroup
constexpr int GM_CELL_MAX = 1 << 29;                       // a row whose cell lies beyond +-2^29 is not scored
constexpr int GM_FAR = 1 << 30;                            // an offset no cell reaches the grid with (nx, ny <= 2^29)
static_assert(GM_CHUNK == GM_THREADS && GM_CHUNK == PAIR_THREADS, "a thread forms one cell of the chunk; gm_frame's chunk");
static_assert((long long)ICPMI_GM_MAX_ROWS * 32767 < (1ll << 31), "a score is an int32");

struct GmArgs {
    const short* field;
    int ny, nx;
    GmPairs pairs;           // cos_sin: [n_pairs][n_angles][2]
    int n_angles, window, centre_angle, n_chunks;
    int32_t* valid;          // [n_pairs][n_angles]: rows with a cell, per angle
    int32_t* volume;         // [n_pairs][n_angles][S][S]
    int32_t* records;
};

// floor((w - mn) / res), the IEEE divide of world_to_grid_kernel; false for a non-finite w or a cell beyond +-2^29
__device__ __forceinline__ bool gm_cell(double w, double mn, double res, int& out) {
    if (!(fabs(w) < __builtin_inf())) return false;
    const double f = floor((w - mn) / res);
    if (!(fabs(f) <= (double)GM_CELL_MAX)) return false;
    out = (int)f;
    return true;
}

// The workgroup's static LDS: the chunk's cells (only rows whose shifts reach the array; the slots behind them, one past the
// chunk included, hold a cell that fails every bounds test), how many there are, how many rows had a cell at all, and —
// where several lanes share a shift — the shifts' sums.
struct GmLds {
    int2 cells[GM_CHUNK + 1];
    int acc[GM_THREADS];
    int kept, valid;
};

// The offsets a workgroup's shifts span on each axis, and the extent of the array they index (the field, or the bound field)
struct GmReach {
    int lo_x, hi_x, lo_y, hi_y;
    int nx, ny;
};

// Phase 1: thread r forms the cell of row base + r of cloud c (N rows) under angle `ang` of pair b in float64 and appends it
// to lds.cells; a row none of whose shifts reaches the array adds 0 to every candidate and is dropped here, a row with a cell
// is counted in lds.valid either way.  -> the kept cells (uniform); behind them lds.cells holds far cells, unless none is kept.
// Ends in a barrier; the caller's earlier reads of lds.cells, lds.kept and lds.valid must lie behind one too.
__device__ __forceinline__ int gm_form_cells(GmLds& lds, const GmArgs& a, int b, int ang, int c, int N, int base, const GmReach& reach) {
    const GmPairs& pl = a.pairs;
    const int tid = threadIdx.x;
    if (tid == 0) { lds.kept = 0; lds.valid = 0; }
    __syncthreads();
    const int row = base + tid;
    if (row < N) {
        const double* p = pl.pts + ((size_t)pl.off[c] + row) * 2;
        const double* cs = pl.cos_sin + ((size_t)b * a.n_angles + ang) * 2;
        double wx, wy;
        gm_world(p[0], p[1], cs[0], cs[1], pl.pair_t[2 * b], pl.pair_t[2 * b + 1], wx, wy);
        int cx, cy;
        if (gm_cell(wx, pl.min_x, pl.res, cx) && gm_cell(wy, pl.min_y, pl.res, cy)) {
            atomicAdd(&lds.valid, 1);
            if (cx + reach.hi_x >= 0 && cx + reach.lo_x < reach.nx && cy + reach.hi_y >= 0 && cy + reach.lo_y < reach.ny)
                lds.cells[atomicAdd(&lds.kept, 1)] = make_int2(cx, cy);
        }
    }
    __syncthreads();
    const int kept = lds.kept;
    if (kept == 0) return 0;                                   // uniform
    const int2 far = make_int2(GM_FAR, GM_FAR);
    if (tid >= kept) lds.cells[tid] = far;                     // what the unrolled walk reads behind the kept cells
    if (tid == 0) lds.cells[GM_CHUNK] = far;
    __syncthreads();
    return kept;
}

// Phase 2's walk: the lane adds array[cell + (dx[k], dy[k])] to acc[k] for its NS offsets over the kept cells first,
// first + stride, ..., each cell read as an LDS broadcast.  Branch-free — a load that fails the bounds test reads element 0
// and adds 0 — so the loads of U cells (4, 2 or 1) times NS offsets are in flight together.  An offset of GM_FAR fails
// every test (unsigned sums: far + far wraps to 2^31, still out of bounds).
template <int NS>
__device__ __forceinline__ void gm_walk(const GmLds& lds, const short* __restrict__ arr, unsigned nx, unsigned ny, int kept, int first,
                                        int stride, const int (&dx)[NS], const int (&dy)[NS], int (&acc)[NS]) {
    constexpr int U = NS == 1 ? 4 : (NS <= 4 ? 2 : 1);         // cells per step: U * NS loads in flight
    for (int r = first; r < kept; r += stride * U) {
        int2 cell[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cell[u] = lds.cells[min(r + u * stride, GM_CHUNK)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const unsigned x = (unsigned)cell[u].x + (unsigned)dx[k], y = (unsigned)cell[u].y + (unsigned)dy[k];
                const bool in = x < nx && y < ny;
                const int v = arr[in ? y * nx + x : 0u];
                acc[k] += in ? v : 0;
            }
        }
    }
}

// Phase 2 for n offsets laid out as rows of `cols`: offset s is ((s % cols) * step + origin, (s / cols) * step + origin).
// NS > 1: lane t owns the offsets from + t, from + t + GM_THREADS, ... (those below n) with their sums in registers and walks
// every kept cell; lanes with consecutive s read consecutive elements of a row (step 1) or every step-th.  NS == 1 (from
// == 0, n <= GM_THREADS, lds.acc zeroed behind a barrier): G = GM_THREADS / n groups of lanes share the cells (group g takes
// cells g, g + G, ...), lane t owning offset t mod n, and the groups meet in LDS integer adds.  Either way ONE int32
// atomicAdd per offset into out[s] (zeroed on the stream before the launch), zeros skipped.
template <int NS>
__device__ __forceinline__ void gm_accumulate(GmLds& lds, const short* __restrict__ arr, int nx, int ny, int kept, int n, int cols, int step,
                                              int origin, int from, int32_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const int G = NS == 1 ? GM_THREADS / n : 1;                // lane groups that share the cells
    const int g = NS == 1 ? tid / n : 0;
    int dx[NS], dy[NS], acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = NS == 1 ? tid - g * n : from + tid + k * GM_THREADS;
        const bool owns = NS == 1 ? g < G : s < n;
        dx[k] = owns ? (s % cols) * step + origin : GM_FAR;    // a lane without an offset fails every bounds test
        dy[k] = owns ? (s / cols) * step + origin : GM_FAR;
        acc[k] = 0;
    }
    gm_walk<NS>(lds, arr, (unsigned)nx, (unsigned)ny, kept, NS == 1 && g >= G ? kept : g, G, dx, dy, acc);   // (no offset: no walk)
    if (NS == 1) {
        if (g < G && acc[0]) atomicAdd(&lds.acc[tid - g * n], acc[0]);
        __syncthreads();
        if (tid < n && lds.acc[tid]) atomicAdd(out + tid, lds.acc[tid]);
    } else {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = from + tid + k * GM_THREADS;
            if (s < n && acc[k]) atomicAdd(out + s, acc[k]);
        }
    }
}

}  // namespace icpmi
