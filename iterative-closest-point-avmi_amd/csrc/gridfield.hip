// gridfield.hip — the likelihood field of the occupancy grid (include/icpmi.h: icpmi_grid_likelihood_field): the exact squared
// Euclidean distance of every cell to the nearest occupied cell, truncated at a radius R, and that distance mapped to an int16
// score through the caller's table.  Truncation makes an output depend on its (2R + 1)^2 neighbourhood alone, so a workgroup
// owns a tile of outputs, stages the tile and a halo of R in LDS and finishes both passes of the separable transform there:
// the field is read once from HBM (the halo from L2) and every output written once.  All of it is integer arithmetic.
#include "gridmatch.hpp"

namespace icpmi {

constexpr int LF_TX = ICPMI_LF_TILE_X, LF_TY = ICPMI_LF_TILE_Y;   // the output tile of one workgroup
constexpr int LF_MAX_R = ICPMI_LF_MAX_RADIUS;
constexpr int LF_PAIRS = LF_TX / 2;                                // the row pass: a lane owns two neighbouring columns
constexpr int LF_ROWS_PER_STEP = GM_THREADS / LF_PAIRS;            // rows the workgroup's lanes span in the row pass
constexpr int LF_NG_OUT = (LF_TX + 14) / 8;                        // groups of 8 flat cells a span of LF_TX cells can touch
constexpr int LF_STAGE = 6;                                        // groups of 8 cells a lane stages with their loads in flight together
constexpr int LF_OUT_ITEMS = (LF_TY * LF_NG_OUT + GM_THREADS - 1) / GM_THREADS;   // output groups of a lane
constexpr int LF_BATCH = 8;                                        // rows of the column pass whose words are loaded together
constexpr int LF_UNROLL = 4;                                       // rows a lane carries through one walk over the window
constexpr int LF_FAR = 0x7fff;                                     // g^2 of a column without an occupied cell within R
static_assert(LF_TX + 2 * LF_MAX_R <= GM_THREADS, "the column pass: one lane per staged column");
static_assert(LF_TX % 2 == 0 && GM_THREADS % LF_PAIRS == 0 && LF_TY % (LF_ROWS_PER_STEP * LF_UNROLL) == 0, "the row pass covers the tile in whole steps");
static_assert(LF_MAX_R * LF_MAX_R + LF_FAR < (1 << 16) && LF_MAX_R * LF_MAX_R + 1 <= 32767, "g^2 + dx^2 fits 16 bits, the sentinel an int16");

// The workgroup's dynamic LDS for a radius, described once (the host sizes the launch with it, the kernel finds its arrays):
//   bits  uint32 [TY + 2R][wpr]   the occupancy of tile + halo, one BIT per cell, 32 columns to a word
//   g2    uint16 [TY][TX + 2R]    the squared column distance of the tile's rows, LF_FAR beyond R
//   d2    uint16 [TY][TX]         the tile's result, read back by the lanes that form the 16-byte stores
//   table int16  [R^2 + 1]        the caller's table (only when the likelihood is asked for)
// Bits, not bytes: at R = 64 the staged area is 192 x 256 cells — 48 KB as bytes, 6 KB as bits — and with bits the whole
// layout is 62 KB, two workgroups to a CU's 160 KB with room to spare (bytes: 104 KB, one); at R <= 6 it is under 37 KB, four.
// The column pass reads a word per row and lane, 32 lanes the same word (a broadcast), so bits cost it nothing.
struct LfLds {
    int cols, rows, wpr;
    size_t bits, g2, d2, table, bytes;
    __host__ __device__ LfLds(int R, bool with_table) {
        cols = LF_TX + 2 * R;
        rows = LF_TY + 2 * R;
        wpr = (cols + 31) / 32;
        const auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        bits = 0;
        g2 = a16(bits + (size_t)rows * wpr * sizeof(uint32_t));
        d2 = a16(g2 + (size_t)LF_TY * cols * sizeof(uint16_t));
        table = a16(d2 + (size_t)LF_TY * LF_TX * sizeof(uint16_t));
        bytes = a16(table + (with_table ? (size_t)(R * R + 1) * sizeof(int16_t) : 0));
    }
};

struct LfArgs {
    const short* q;
    short* d2;               // either output may be null, not both
    short* lf;
    const short* table;      // device, R^2 + 1 (null without lf)
    int ny, nx, threshold, R, keep_free;
};

// Rows of the field start at any int16, so a row's span is cut at multiples of 8 of the FLAT index (gridmatch_wide.hip's
// rule).  A group that lies inside the array is LOADED as one aligned 16-byte access even where only a part of it belongs
// to the span — the rest is the neighbouring row's, read and masked away — so no lane of a wave waits on a cell-by-cell path.
// The cells behind the array's last whole group (ny * nx not a multiple of 8: at most 7) are left out of the groups and taken
// by one lane each.  Stores are whole only where the whole group belongs to the span.
union LfGroup {
    short s[8];
    uint4 v;
};
// The k-th group of 8 flat cells that the span [xb, xe) of row y touches: cells lo + s .. lo + e - 1 belong to the span
// (none when e <= s, and none of a group that reaches past the array's end); f0 is the flat index of (y, xb)
struct LfSpan {
    long long lo, f0;
    int s, e;
    __device__ bool empty() const { return e <= s; }
    __device__ bool whole() const { return s == 0 && e == 8; }
};
__device__ __forceinline__ LfSpan lf_no_span() { return LfSpan{0, 0, 0, 0}; }
__device__ __forceinline__ LfSpan lf_span(int y, int ny, int nx, int xb, int xe, int k) {
    const long long f0 = (long long)y * nx + xb, f1 = f0 + (xe - xb), lo = ((f0 >> 3) + k) << 3;
    return lo + 8 <= (long long)ny * nx ? LfSpan{lo, f0, (int)max(f0 - lo, 0ll), (int)min(f1 - lo, 8ll)} : lf_no_span();
}
// Cell j of a loaded group.  The group stays four dwords until it is used, so that the loads of several groups stay in flight
// together (taken apart where it is loaded, every load would be waited for on the spot).
__device__ __forceinline__ int lf_cell(const uint4& v, int j) {
    const uint32_t w = j < 2 ? v.x : (j < 4 ? v.y : (j < 6 ? v.z : v.w));
    return (int)(short)((j & 1) ? w >> 16 : w & 0xffffu);
}

__global__ __launch_bounds__(GM_THREADS) void lf_field_kernel(LfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const LfLds L(a.R, a.lf != nullptr);
    uint32_t* bits = reinterpret_cast<uint32_t*>(dyn + L.bits);
    uint16_t* g2 = reinterpret_cast<uint16_t*>(dyn + L.g2);
    uint16_t* d2s = reinterpret_cast<uint16_t*>(dyn + L.d2);
    short* tab = reinterpret_cast<short*>(dyn + L.table);
    const int tid = threadIdx.x, R = a.R, R2 = R * R, C = L.cols, wpr = L.wpr;
    const int x_lo = (int)blockIdx.x * LF_TX - R, y_lo = (int)blockIdx.y * LF_TY - R;     // the cell of bit (0, 0)

    // 0. no cell is occupied until one is found to be (outside the grid none ever is); the table
    for (int i = tid; i < L.rows * wpr; i += GM_THREADS) bits[i] = 0;
    if (a.lf)
        for (int i = tid; i <= R2; i += GM_THREADS) tab[i] = a.table[i];
    __syncthreads();

    // 1. the occupancy of tile + halo: 8 cells per lane and group, their bits merged into at most two words; the loads of
    // LF_STAGE groups are in flight together.  Then the field under this lane's output groups (step 4), where free space keeps
    // its penalty: asked for here, used after the two passes.
    const int xb = max(x_lo, 0), xe = min(x_lo + C, a.nx);
    const int ng_in = (C + 14) / 8, staged = xb < xe ? L.rows * ng_in : 0;
    const auto stage = [&](int base) {
        uint4 u[LF_STAGE];                                         // (set, and read, only where the span is not empty)
        LfSpan g[LF_STAGE];
#pragma unroll
        for (int i = 0; i < LF_STAGE; ++i) {
            const int item = base + i * GM_THREADS, r = item / ng_in, y = y_lo + r;
            g[i] = lf_no_span();
            if (item < staged && y >= 0 && y < a.ny) g[i] = lf_span(y, a.ny, a.nx, xb, xe, item - r * ng_in);
            if (!g[i].empty()) u[i] = *reinterpret_cast<const uint4*>(a.q + g[i].lo);
        }
#pragma unroll
        for (int i = 0; i < LF_STAGE; ++i) {
            if (g[i].empty()) continue;
            unsigned m = 0;                                        // bit j: cell lo + j is occupied
#pragma unroll
            for (int j = 0; j < 8; ++j) m |= (unsigned)(lf_cell(u[i], j) >= a.threshold) << j;
            m &= (1u << g[i].e) - (1u << g[i].s);                  // the span's cells alone
            if (!m) continue;
            const int r = (base + i * GM_THREADS) / ng_in;
            const int c = (int)(g[i].lo + g[i].s - g[i].f0) + (xb - x_lo);     // the column of cell lo + s: c + 7 < C where a bit is set
            const unsigned long long wide = (unsigned long long)(m >> g[i].s) << (c & 31);
            uint32_t* w = bits + r * wpr + (c >> 5);
            atomicOr(w, (uint32_t)wide);
            if (wide >> 32) atomicOr(w + 1, (uint32_t)(wide >> 32));
        }
    };
    // (the first batch outside the loop: inside one, every load waits for the one before it)
    stage(tid);
    for (int base = tid + GM_THREADS * LF_STAGE; base < staged; base += GM_THREADS * LF_STAGE) stage(base);
    const long long cells = (long long)a.ny * a.nx, tail = cells & ~7ll;
    if (tid < (int)(cells - tail)) {                               // a cell behind the last whole group
        const long long f = tail + tid;
        const int y = (int)(f / a.nx), r = y - y_lo, c = (int)(f - (long long)y * a.nx) - x_lo;
        if (r >= 0 && r < L.rows && c >= 0 && c < C && (int)a.q[f] >= a.threshold) atomicOr(bits + r * wpr + (c >> 5), 1u << (c & 31));
    }
    const int ob = (int)blockIdx.x * LF_TX, oe = min(ob + LF_TX, a.nx);
    const bool free_kept = a.lf && a.keep_free;
    LfSpan out[LF_OUT_ITEMS];
    uint4 raw[LF_OUT_ITEMS];                                       // (set, and read, only where free space is kept and the span is not empty)
#pragma unroll
    for (int i = 0; i < LF_OUT_ITEMS; ++i) {
        const int item = tid + i * GM_THREADS, ty = item / LF_NG_OUT, Y = (int)blockIdx.y * LF_TY + ty;
        out[i] = lf_no_span();
        if (item < LF_TY * LF_NG_OUT && Y < a.ny) out[i] = lf_span(Y, a.ny, a.nx, ob, oe, item - ty * LF_NG_OUT);
        if (free_kept && !out[i].empty()) raw[i] = *reinterpret_cast<const uint4*>(a.q + out[i].lo);
    }
    __syncthreads();

    // 2. the column pass, one lane per staged column: the distance to the nearest occupied cell above (on the way down), then
    // below (on the way up), capped at R + 1; the tile's rows keep the square of the smaller one.  R + TY steps each way for
    // every lane, whatever the map holds, in batches of LF_BATCH rows whose words are loaded together (the chain through
    // `dist` is arithmetic alone).  A lane reads only what it wrote itself: no barrier between the two sweeps.
    if (tid < C) {
        const uint32_t* col = bits + (tid >> 5);
        const int sh = tid & 31, far = R + 1, n = R + LF_TY;
        uint16_t* g = g2 + tid;
        int dist = far;
        for (int r0 = 0; r0 < n; r0 += LF_BATCH) {                 // rows 0 .. R + TY - 1
            uint32_t w[LF_BATCH];
#pragma unroll
            for (int j = 0; j < LF_BATCH; ++j) w[j] = col[min(r0 + j, n - 1) * wpr];
#pragma unroll
            for (int j = 0; j < LF_BATCH; ++j) {
                const int r = r0 + j;
                if (r >= n) continue;
                dist = (w[j] >> sh & 1) ? 0 : min(dist + 1, far);
                if (r >= R) g[(r - R) * C] = (uint16_t)dist;
            }
        }
        dist = far;
        for (int i0 = 0; i0 < n; i0 += LF_BATCH) {                 // rows TY + 2R - 1 .. R, counted from the bottom
            uint32_t w[LF_BATCH];
            int down[LF_BATCH];
#pragma unroll
            for (int j = 0; j < LF_BATCH; ++j) {
                const int r = L.rows - 1 - min(i0 + j, n - 1);
                w[j] = col[r * wpr];
                down[j] = g[min(r - R, LF_TY - 1) * C];            // (of a halo row: read and dropped)
            }
#pragma unroll
            for (int j = 0; j < LF_BATCH; ++j) {
                const int r = L.rows - 1 - (i0 + j);
                if (i0 + j >= n) continue;
                dist = (w[j] >> sh & 1) ? 0 : min(dist + 1, far);
                if (r >= R + LF_TY) continue;
                const int d = min(dist, down[j]);
                g[(r - R) * C] = (uint16_t)(d > R ? LF_FAR : d * d);
            }
        }
    }
    __syncthreads();

    // 3. the row pass: a lane owns two neighbouring columns of LF_UNROLL rows at a time, a wave one row of the tile.  It reads
    // the R + 1 aligned dwords that hold the 2R + 2 squared column distances around its pair — consecutive lanes consecutive
    // dwords, one bank each — and every dword serves four (output, offset) sums; dx^2 is the same for the whole wave (a
    // scalar).  The same R + 1 steps for every lane.  The one offset of R + 1 each column meets on the way adds more than
    // R^2, so it cannot win below the clamp.
    {
        const int j = tid % LF_PAIRS, yb = tid / LF_PAIRS, Cw = C / 2;
        const uint32_t* g2w = reinterpret_cast<const uint32_t*>(g2);
        uint32_t* d2w = reinterpret_cast<uint32_t*>(d2s);
        for (int y = yb; y < LF_TY; y += LF_ROWS_PER_STEP * LF_UNROLL) {
            const uint32_t* p[LF_UNROLL];
            int left[LF_UNROLL], right[LF_UNROLL];
#pragma unroll
            for (int u = 0; u < LF_UNROLL; ++u) {
                p[u] = g2w + (y + u * LF_ROWS_PER_STEP) * Cw + j;
                left[u] = right[u] = LF_FAR;
            }
            for (int m = 0; m <= R; ++m) {
                const int e = 2 * m - R, ee = e * e, above = (e + 1) * (e + 1), below = (e - 1) * (e - 1);
#pragma unroll
                for (int u = 0; u < LF_UNROLL; ++u) {
                    const uint32_t w = p[u][m];
                    const int lo = (int)(w & 0xffffu), hi = (int)(w >> 16);
                    left[u] = min(left[u], min(lo + ee, hi + above));          // column 2j: offsets e and e + 1
                    right[u] = min(right[u], min(lo + below, hi + ee));        // column 2j + 1: offsets e - 1 and e
                }
            }
#pragma unroll
            for (int u = 0; u < LF_UNROLL; ++u) {
                const uint32_t l = left[u] > R2 ? R2 + 1 : left[u], r = right[u] > R2 ? R2 + 1 : right[u];
                d2w[(y + u * LF_ROWS_PER_STEP) * LF_PAIRS + j] = l | r << 16;
            }
        }
    }
    __syncthreads();

    // 4. out: groups of 8 flat cells, whole ones as 16-byte stores
#pragma unroll
    for (int i = 0; i < LF_OUT_ITEMS; ++i) {
        const LfSpan& g = out[i];
        if (g.empty()) continue;
        const int ty = (tid + i * GM_THREADS) / LF_NG_OUT;
        LfGroup dist, like;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int tx = min(max((int)(g.lo + j - g.f0), 0), LF_TX - 1);     // (a cell outside the span is computed and dropped)
            const int d = d2s[ty * LF_TX + tx];
            dist.s[j] = (short)d;
            like.s[j] = 0;
            if (a.lf) like.s[j] = d <= R2 ? tab[d] : (short)(free_kept ? min(lf_cell(raw[i], j), 0) : 0);
        }
        if (g.whole()) {
            if (a.d2) *reinterpret_cast<uint4*>(a.d2 + g.lo) = dist.v;
            if (a.lf) *reinterpret_cast<uint4*>(a.lf + g.lo) = like.v;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j < g.s || j >= g.e) continue;
                if (a.d2) a.d2[g.lo + j] = dist.s[j];
                if (a.lf) a.lf[g.lo + j] = like.s[j];
            }
        }
    }
    if (tid < (int)(cells - tail)) {                               // a cell behind the last whole group
        const long long f = tail + tid;
        const int y = (int)(f / a.nx), ty = y - (int)blockIdx.y * LF_TY, tx = (int)(f - (long long)y * a.nx) - ob;
        if (ty >= 0 && ty < LF_TY && tx >= 0 && tx < LF_TX) {
            const int d = d2s[ty * LF_TX + tx];
            if (a.d2) a.d2[f] = (short)d;
            if (a.lf) a.lf[f] = d <= R2 ? tab[d] : (short)(free_kept ? min((int)a.q[f], 0) : 0);
        }
    }
}

// ── host: the workspace, the plan, the entry ─────────────────────────────────
// The workspace, described once: the device copy of the caller's table.
struct LfWs {
    Carve c;
    int16_t* table;
    LfWs(void* base, size_t entries) : c(base), table(c.take<int16_t>(entries * sizeof(int16_t))) {}
    size_t bytes() const { return c.off; }
};

// What a call starts, decided as a whole and without a HIP call
struct LfPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    dim3 grid;                // tiles of LF_TY x LF_TX outputs
    size_t lds;               // LfLds of the radius
    size_t table_bytes;       // copied into the workspace before the launch; 0 without the likelihood
};
static LfPlan plan_likelihood_field(int ny, int nx, int radius, bool with_table) {
    LfPlan p{ICPMI_OK, dim3(0, 0, 1), 0, 0};
    if (ny <= 0 || nx <= 0 || (long long)ny * nx >= (1ll << 31)) { p.rc = ICPMI_ERR_ARG; return p; }
    if (radius < 0 || radius > LF_MAX_R) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.grid = dim3((unsigned)((nx + LF_TX - 1) / LF_TX), (unsigned)((ny + LF_TY - 1) / LF_TY));
    if (p.grid.y > 65535u) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.lds = LfLds(radius, with_table).bytes;
    p.table_bytes = with_table ? (size_t)(radius * radius + 1) * sizeof(int16_t) : 0;
    return p;
}

}  // namespace icpmi

extern "C" size_t icpmi_grid_likelihood_workspace_bytes(int32_t ny, int32_t nx, int32_t radius) {
    using namespace icpmi;
    if (plan_likelihood_field(ny, nx, radius, true).rc != ICPMI_OK) return 0;
    return LfWs(nullptr, (size_t)radius * radius + 1).bytes();
}

extern "C" int icpmi_grid_likelihood_field(const int16_t* field, int32_t ny, int32_t nx, int32_t threshold, int32_t radius,
                                           const int16_t* table, int32_t keep_free, int16_t* d2_out, int16_t* lf_out,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const LfPlan plan = plan_likelihood_field(ny, nx, radius, lf_out != nullptr);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (!field || (!d2_out && !lf_out) || (lf_out && !table)) return ICPMI_ERR_ARG;
    if (((uintptr_t)field & 15) || ((uintptr_t)d2_out & 15) || ((uintptr_t)lf_out & 15)) return ICPMI_ERR_ARG;
    const LfWs ws(workspace, (size_t)radius * radius + 1);
    if (lf_out) {
        for (int i = 0; i <= radius * radius; ++i)
            if (table[i] == INT16_MIN) return ICPMI_ERR_ARG;
        if (!workspace || workspace_bytes < ws.bytes()) return ICPMI_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (lf_out && hipMemcpyAsync(ws.table, table, plan.table_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (dyn_lds((const void*)lf_field_kernel, plan.lds) != hipSuccess) return ICPMI_ERR_HIP;
    const LfArgs a{(const short*)field, (short*)d2_out, (short*)lf_out, lf_out ? (const short*)ws.table : nullptr, ny, nx, threshold, radius, keep_free};
    lf_field_kernel<<<plan.grid, GM_THREADS, plan.lds, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
