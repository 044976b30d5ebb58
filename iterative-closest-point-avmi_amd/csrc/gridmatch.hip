// gridmatch.hip — correlative scan-to-map matching on the occupancy grid (include/icpmi.h: icpmi_grid_score_field,
// icpmi_grid_match_batch).  The reference registers cloud against cloud only (slam.py:53-98, 111-183); this reads the map
// it builds (utilities/mapping.py) instead: the log-odds quantised to int16, and for every pair, angle and whole-cell shift
// of a (2W + 1)^2 window the sum of the field under the scan's cells.  Cells are formed once in float64 exactly as
// world_to_grid does (mapping.py:94-98); everything after that is integer, so any split of the rows over workgroups and any
// order of the integer atomics gives the same bits.
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GM_MAX_NS = 16;                              // shifts a lane owns, at most
constexpr int GM_FIELD_VEC = 8;                            // cells a thread of the field kernel converts
static_assert((2 * ICPMI_GM_MAX_WINDOW + 1) * (2 * ICPMI_GM_MAX_WINDOW + 1) <= GM_MAX_NS * GM_THREADS, "every shift has an owner");
static_assert(ICPMI_GMREC_CENTRE + 1 == ICPMI_GMREC_INTS, "the record is eight int32");

// ── the score field ──────────────────────────────────────────────────────────
// q = clip(rint(L * 2^k), -32767, 32767): the product in float32 (a power of two: exact), half to even, NaN -> 0
__device__ __forceinline__ short gm_quantise(float v, float scale) {
    const float r = rintf(v * scale);
    if (r != r) return 0;
    return (short)(int)fminf(fmaxf(r, -32767.0f), 32767.0f);
}

// thread t converts cells [8t, 8t + 8): two 16-byte loads, one 16-byte store; the last thread's ragged tail cell by cell
__global__ __launch_bounds__(GM_THREADS) void gm_field_kernel(const float* __restrict__ lo, short* __restrict__ q, long long n, float scale) {
    const long long at = ((long long)blockIdx.x * GM_THREADS + threadIdx.x) * GM_FIELD_VEC;
    if (at >= n) return;
    if (at + GM_FIELD_VEC <= n) {
        const float4 a = *reinterpret_cast<const float4*>(lo + at), b = *reinterpret_cast<const float4*>(lo + at + 4);
        union { short s[GM_FIELD_VEC]; uint4 v; } o;
        o.s[0] = gm_quantise(a.x, scale); o.s[1] = gm_quantise(a.y, scale); o.s[2] = gm_quantise(a.z, scale); o.s[3] = gm_quantise(a.w, scale);
        o.s[4] = gm_quantise(b.x, scale); o.s[5] = gm_quantise(b.y, scale); o.s[6] = gm_quantise(b.z, scale); o.s[7] = gm_quantise(b.w, scale);
        *reinterpret_cast<uint4*>(q + at) = o.v;
    } else {
        for (long long i = at; i < n; ++i) q[i] = gm_quantise(lo[i], scale);
    }
}

// ── scoring ──────────────────────────────────────────────────────────────────
// One workgroup per (pair, angle, chunk of GM_CHUNK rows).  Phase 1 (gm_form_cells): thread r forms the cell of row r of the
// chunk in float64.  Phase 2 (gm_accumulate over the S^2 shifts, rows of S, step 1 from -W), NS > 1 (S^2 > GM_THREADS): lane t
// owns the shifts t, t + GM_THREADS, ... with their sums in registers and walks every kept cell, the cell read as an LDS
// broadcast; lanes with consecutive i read consecutive int16 of a grid row.  NS == 1 (S^2 <= GM_THREADS): G = GM_THREADS /
// S^2 groups of lanes share the rows (group g takes rows g, g + G, ...), lane t owning shift t mod S^2, and the groups meet
// in LDS integer adds.  The walk is branch-free (gm_walk).  Either way the workgroup ends with ONE int32 atomicAdd per shift
// into the volume (zeroed on the stream before the launch).  No workgroup waits for another.
template <int NS>
__global__ __launch_bounds__(GM_THREADS) void gm_score_kernel(GmArgs a) {
    __shared__ GmLds lds;
    const int tid = threadIdx.x;
    const GmFrame f = gm_frame(a.pairs, blockIdx.x, a.n_chunks, a.n_angles);
    if (f.base >= f.N) return;                                 // uniform per workgroup, before any barrier
    const int b = f.b, ang = f.ang;
    const int W = a.window, S = 2 * W + 1, S2 = S * S;
    if (NS == 1) lds.acc[tid] = 0;
    // a row whose whole window misses the grid adds 0 to every candidate: dropped in phase 1
    const int kept = gm_form_cells(lds, a, b, ang, f.c, f.N, f.base, GmReach{-W, W, -W, W, a.nx, a.ny});
    if (tid == 0 && lds.valid) atomicAdd(a.valid + (size_t)b * a.n_angles + ang, lds.valid);
    if (kept == 0) return;                                     // uniform
    gm_accumulate<NS>(lds, a.field, a.nx, a.ny, kept, S2, S, 1, -W, 0, a.volume + ((size_t)b * a.n_angles + ang) * S2);
}

// ── arg-max and record ───────────────────────────────────────────────────────
// One workgroup per pair over its n_angles * S^2 scores: thread t scans t, t + GM_THREADS, ... in rising order (a later
// equal score never replaces an earlier one), then the fixed butterfly of wave_first_best and the four waves in order:
// the first maximum in C order, as np.argmax.
__global__ __launch_bounds__(GM_THREADS) void gm_argmax_kernel(GmArgs a) {
    __shared__ int wave_v[GM_WAVES], wave_i[GM_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int W = a.window, S = 2 * W + 1, S2 = S * S, n = a.n_angles * S2;
    const int32_t* vol = a.volume + (size_t)b * n;
    const int32_t* valid = a.valid + (size_t)b * a.n_angles;
    int best = INT32_MIN, at = INT32_MAX, any = 0;
    for (int i = tid; i < n; i += GM_THREADS) {
        const int v = vol[i];
        if (v > best) { best = v; at = i; }
    }
    for (int i = tid; i < a.n_angles; i += GM_THREADS) any |= valid[i];
    const auto greater = [](int x, int y) { return x > y; };
    wave_first_best(best, at, greater);
    if (lane_id() == 0) { wave_v[wave_id()] = best; wave_i[wave_id()] = at; }
    any = __syncthreads_or(any);
    if (tid != 0) return;
    for (int w = 1; w < GM_WAVES; ++w) take_first_best(best, at, wave_v[w], wave_i[w], greater);
    const int ang = at / S2, rem = at - ang * S2;
    int32_t* rec = a.records + (size_t)b * ICPMI_GMREC_INTS;
    rec[ICPMI_GMREC_STATUS] = gm_status(gm_rows(a.pairs, a.pairs.pair_cloud[b]), any);
    rec[ICPMI_GMREC_ROWS] = valid[ang];
    rec[ICPMI_GMREC_INDEX] = at;
    rec[ICPMI_GMREC_A] = ang;
    rec[ICPMI_GMREC_J] = rem / S;
    rec[ICPMI_GMREC_I] = rem % S;
    rec[ICPMI_GMREC_SCORE] = best;
    rec[ICPMI_GMREC_CENTRE] = a.centre_angle >= 0 ? vol[(a.centre_angle * S + W) * S + W] : 0;
}

// ── host: the workspace, the plan, the entries ──────────────────────────────
// The workspace, described once: the valid-row counts per (pair, angle), then the score volume.
struct GmWs {
    Carve c;
    int32_t* valid;
    int32_t* volume;
    GmWs(void* base, size_t n_pairs, size_t n_angles, size_t shifts)
        : c(base), valid(c.take<int32_t>(n_pairs * n_angles * sizeof(int32_t))),
          volume(c.take<int32_t>(n_pairs * n_angles * shifts * sizeof(int32_t))) {}
    size_t bytes() const { return c.off; }
};

// What a call starts, decided as a whole and without a HIP call.  The chunk and the block never depend on the batch, and
// the sums are integers: a pair's record does not depend on the batch it is computed in.
struct GmPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    unsigned score_grid;      // (pair, angle, chunk) workgroups; 0: nothing to score (the records are still written)
    unsigned argmax_grid;     // pairs; 0: nothing to do
    int n_chunks, ns;         // row chunks of the largest cloud; shifts a lane owns
    size_t valid_bytes, volume_bytes;   // what is zeroed before the launch
};
static GmPlan plan_grid_match(int n_pairs, int max_n, int n_angles, int window) {
    GmPlan p{ICPMI_OK, 0, 0, 0, 1, 0, 0};
    if (n_pairs < 0 || max_n < 0 || n_angles < 1 || window < 0) { p.rc = ICPMI_ERR_ARG; return p; }
    if (window > ICPMI_GM_MAX_WINDOW || n_angles > ICPMI_GM_MAX_ANGLES || max_n > ICPMI_GM_MAX_ROWS) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    const int S = 2 * window + 1, S2 = S * S;
    p.ns = (S2 + GM_THREADS - 1) / GM_THREADS;
    p.n_chunks = (max_n + GM_CHUNK - 1) / GM_CHUNK;
    const unsigned long long groups = (unsigned long long)n_pairs * n_angles * p.n_chunks;
    if (groups >= (1ull << 31)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.score_grid = (unsigned)groups;
    p.argmax_grid = (unsigned)n_pairs;
    p.valid_bytes = (size_t)n_pairs * n_angles * sizeof(int32_t);
    p.volume_bytes = p.valid_bytes * S2;
    return p;
}

template <int NS>
static void gm_launch_score(int ns, unsigned grid, const GmArgs& a, hipStream_t st) {
    if (ns == NS) gm_score_kernel<NS><<<grid, GM_THREADS, 0, st>>>(a);
    else if constexpr (NS < GM_MAX_NS) gm_launch_score<NS + 1>(ns, grid, a, st);
}

}  // namespace icpmi

extern "C" int icpmi_grid_score_field(const float* log_odds, int32_t ny, int32_t nx, int32_t shift_bits, int16_t* field, void* stream) {
    using namespace icpmi;
    if (ny < 0 || nx < 0 || shift_bits < 0 || shift_bits > ICPMI_GM_MAX_SHIFT_BITS) return ICPMI_ERR_ARG;
    const long long n = (long long)ny * nx;
    if (n == 0) return ICPMI_OK;
    if (!log_odds || !field || ((uintptr_t)log_odds & 15) || ((uintptr_t)field & 15)) return ICPMI_ERR_ARG;
    const long long per_block = (long long)GM_THREADS * GM_FIELD_VEC;
    const long long blocks = (n + per_block - 1) / per_block;
    if (blocks >= (1ll << 31)) return ICPMI_ERR_UNSUPPORTED;
    gm_field_kernel<<<(unsigned)blocks, GM_THREADS, 0, (hipStream_t)stream>>>(log_odds, field, n, (float)(1 << shift_bits));
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" size_t icpmi_grid_match_workspace_bytes(int32_t n_pairs, int32_t n_angles, int32_t window) {
    using namespace icpmi;
    if (n_pairs < 0 || n_angles < 0 || window < 0) return 0;
    const size_t S = 2 * (size_t)window + 1;
    return GmWs(nullptr, (size_t)n_pairs, (size_t)n_angles, S * S).bytes();
}

extern "C" int icpmi_grid_match_batch(const int16_t* field, int32_t ny, int32_t nx, double min_x, double min_y, double resolution,
                                      const double* pts, const int32_t* off_dev, const int32_t* off_host, const int32_t* cnt_dev,
                                      int32_t n_clouds, const int32_t* pair_cloud, const int32_t* pair_cloud_host,
                                      int32_t n_pairs, const double* pair_t, const double* cos_sin, int32_t n_angles,
                                      int32_t window, int32_t centre_angle, int32_t* out_records, int32_t* out_scores,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (n_pairs == 0) return ICPMI_OK;
    const PairScan pairs = scan_pairs(n_pairs, n_clouds, off_host, pair_cloud_host);
    if (pairs.rc != ICPMI_OK) return pairs.rc;
    const GmPlan plan = plan_grid_match(n_pairs, pairs.max_n, n_angles, window);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (!field || !pts || !off_dev || !pair_cloud || !pair_t || !cos_sin || !out_records || !workspace) return ICPMI_ERR_ARG;
    if (ny < 1 || nx < 1 || ny > GM_CELL_MAX || nx > GM_CELL_MAX || (long long)ny * nx >= (1ll << 31)) return ICPMI_ERR_ARG;
    if (!world_ok(resolution, min_x, min_y) || centre_angle >= n_angles) return ICPMI_ERR_ARG;
    const int S = 2 * window + 1;
    const GmWs ws(workspace, (size_t)n_pairs, (size_t)n_angles, (size_t)S * S);
    if (workspace_bytes < ws.bytes()) return ICPMI_ERR_WORKSPACE;

    int32_t* volume = out_scores ? out_scores : ws.volume;
    const GmArgs a{(const short*)field, ny, nx, {min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin},
                   n_angles, window, centre_angle, plan.n_chunks, ws.valid, volume, out_records};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws.valid, 0, plan.valid_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (hipMemsetAsync(volume, 0, plan.volume_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (plan.score_grid) {
        gm_launch_score<1>(plan.ns, plan.score_grid, a, st);
        ICPMI_LAUNCH_CHECK();
    }
    gm_argmax_kernel<<<plan.argmax_grid, GM_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
