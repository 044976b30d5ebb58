// gridmatch_wide.hip — the wide-window scan-to-map search (include/icpmi.h: icpmi_grid_bound_field,
// icpmi_grid_search_batch): the winner of icpmi_grid_match_batch's exhaustive volume for windows up to
// ICPMI_GMW_MAX_WINDOW cells, found without forming that volume.  The shifts are cut into blocks of D x D; a max-pooled copy
// of the field bounds every score of a block from above; one block per angle is scored exactly for a seed score, and then
// every block whose bound reaches the seed.  All of it is integer arithmetic behind gridmatch.hpp's phase 1, so every slot of
// a record — the survivor count included — is a function of the inputs alone, whatever the schedule.
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GMW_TX = 128, GMW_TY = 32;                   // the bound field's output tile of one workgroup
constexpr int GMW_BOUND_NS = 4;                            // blocks a lane of the bound pass owns per sweep (above GM_THREADS blocks)
constexpr int GMW_SELECT_VEC = 8;                          // blocks a thread of the selection tests
constexpr int GMW_RECORD_THREADS = ICPMI_WAVE;
static_assert(ICPMI_GMW_REC_MAX_BOUND + 1 == ICPMI_GMW_REC_INTS && ICPMI_GMW_REC_BLOCKS == ICPMI_GMREC_INTS, "eight slots of the old record, then four");
static_assert(GM_THREADS == 16 * 16, "one lane per shift of the largest block");

// ── the bound field ──────────────────────────────────────────────────────────
// out[Y][X], (ny + D - 1, nx + D - 1), = max of q~ over rows [Y - D + 1, Y] and columns [X - D + 1, X], q~ the field extended
// by 0: M(y, x) of the contract at (Y, X) = (y + D - 1, x + D - 1).  A workgroup makes a tile of GMW_TY x GMW_TX of it: the
// (GMW_TY + D - 1) x (GMW_TX + D - 1) cells under it into LDS (zeros where the grid ends), the sliding maximum along the rows,
// then down the columns on the way out.  Rows of the field and of the output start at any int16, so a row's span is cut at
// multiples of 8 of the FLAT index: a whole group moves as one 16-byte access, a ragged one cell by cell.
template <int D>
__global__ __launch_bounds__(GM_THREADS) void gmw_bound_field_kernel(const short* __restrict__ q, short* __restrict__ out, int ny, int nx) {
    constexpr int R = GMW_TY + D - 1, C = GMW_TX + D - 1, CP = (C + 1) & ~1;
    constexpr int NG_IN = (C + 14) / 8, NG_OUT = (GMW_TX + 14) / 8;            // groups of 8 a span of C (GMW_TX) cells can touch
    __shared__ short in[R * CP];
    __shared__ short rows[R * GMW_TX];
    const int tid = threadIdx.x;
    const int x_lo = (int)blockIdx.x * GMW_TX - (D - 1), y_lo = (int)blockIdx.y * GMW_TY - (D - 1);    // the cell of in[0][0]
    for (int i = tid; i < R * CP; i += GM_THREADS) in[i] = 0;
    __syncthreads();
    const int xb = max(x_lo, 0), xe = min(x_lo + C, nx);
    for (int item = tid; item < R * NG_IN && xb < xe; item += GM_THREADS) {
        const int r = item / NG_IN, k = item - r * NG_IN, y = y_lo + r;
        if (y < 0 || y >= ny) continue;
        const long long f0 = (long long)y * nx + xb, f1 = f0 + (xe - xb), lo = ((f0 >> 3) + k) << 3;
        if (lo >= f1) continue;
        short* dst = in + r * CP + (xb - x_lo);                                // the cell of flat index f goes to dst[f - f0]
        if (lo >= f0 && lo + 8 <= f1) {
            union { short s[8]; uint4 v; } u;
            u.v = *reinterpret_cast<const uint4*>(q + lo);
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[lo - f0 + j] = u.s[j];
        } else {
            for (long long f = lo > f0 ? lo : f0; f < lo + 8 && f < f1; ++f) dst[f - f0] = q[f];
        }
    }
    __syncthreads();
    for (int i = tid; i < R * GMW_TX; i += GM_THREADS) {
        const int r = i / GMW_TX, c = i - r * GMW_TX;
        short m = in[r * CP + c];
#pragma unroll
        for (int k = 1; k < D; ++k) m = max(m, in[r * CP + c + k]);
        rows[i] = m;
    }
    __syncthreads();
    const int nyo = ny + D - 1, nxo = nx + D - 1;
    const int ob = (int)blockIdx.x * GMW_TX, oe = min(ob + GMW_TX, nxo);
    for (int item = tid; item < GMW_TY * NG_OUT; item += GM_THREADS) {
        const int ty = item / NG_OUT, k = item - ty * NG_OUT, Y = (int)blockIdx.y * GMW_TY + ty;
        if (Y >= nyo) continue;
        const long long f0 = (long long)Y * nxo + ob, f1 = f0 + (oe - ob), lo = ((f0 >> 3) + k) << 3;
        if (lo >= f1) continue;
        const long long s = lo > f0 ? lo : f0, e = lo + 8 < f1 ? lo + 8 : f1;
        union { short s[8]; uint4 v; } u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int tx = min(max((int)(lo + j - f0), 0), GMW_TX - 1);        // (a cell outside [s, e) is computed and dropped)
            short m = rows[ty * GMW_TX + tx];
#pragma unroll
            for (int kk = 1; kk < D; ++kk) m = max(m, rows[(ty + kk) * GMW_TX + tx]);
            u.s[j] = m;
        }
        if (e - s == 8) {
            *reinterpret_cast<uint4*>(out + lo) = u.v;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (lo + j >= s && lo + j < e) out[lo + j] = u.s[j];
        }
    }
}

// ── the search ───────────────────────────────────────────────────────────────
// What a pair accumulates, zeroed on the stream before the launches.  seed and best hold (score + 2^31) << 32 |
// (0xFFFFFFFF - flat index): one 64-bit unsigned atomicMax keeps the larger score and, on equal scores, the lower index; the
// zero it starts from is below every real entry.  max_u holds bound + 2^31 the same way.
struct GmwPair {
    unsigned long long seed, best;
    int32_t centre, survivors;
    uint32_t max_u, pad;
};
__device__ __forceinline__ unsigned long long gmw_key(int score, int flat) {
    return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (0xFFFFFFFFu - (uint32_t)flat);
}
__device__ __forceinline__ int gmw_key_score(unsigned long long key) { return (int)((uint32_t)(key >> 32) ^ 0x80000000u); }
__device__ __forceinline__ int gmw_key_flat(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

struct GmwArgs {
    GmArgs g;                // the field, the clouds, the pairs, the angles, W, the centre angle; valid; records (12 int32 each)
    const short* bound;      // the bound field for this D, (ny + D - 1, nx + D - 1)
    int n_pairs, D, nb;      // block edge; blocks per axis
    int32_t* U;              // [n_pairs][n_angles][nb][nb]
    int32_t* seeds;          // [n_pairs][n_angles]: the angle's seed block, as a block of the pair (a * nb^2 + J * nb + I)
    int32_t* list;           // the survivors, as blocks of the batch (b * n_angles * nb^2 + block of the pair), in any order
    int32_t* n_listed;
    GmwPair* pair;
};

// 1. the bounds.  The scoring walk of gm_score_kernel over the bound field: one workgroup per (pair, angle, chunk of rows),
// lanes own blocks — offset (I * D + D - 1 - W, J * D + D - 1 - W) into the stored bound field — and end in one int32
// atomicAdd per block.  NS == 1: at most GM_THREADS blocks, lane groups share the rows; else sweeps of NS * GM_THREADS blocks.
template <int NS>
__global__ __launch_bounds__(GM_THREADS) void gmw_bound_kernel(GmwArgs w) {
    __shared__ GmLds lds;
    const GmArgs& a = w.g;
    const int tid = threadIdx.x;
    const GmFrame f = gm_frame(a.pairs, blockIdx.x, a.n_chunks, a.n_angles);
    if (f.base >= f.N) return;                                 // uniform per workgroup, before any barrier
    const int b = f.b, ang = f.ang;
    const int nb2 = w.nb * w.nb, origin = w.D - 1 - a.window, nxo = a.nx + w.D - 1, nyo = a.ny + w.D - 1;
    if (NS == 1) lds.acc[tid] = 0;
    const int last = origin + (w.nb - 1) * w.D;
    const int kept = gm_form_cells(lds, a, b, ang, f.c, f.N, f.base, GmReach{origin, last, origin, last, nxo, nyo});
    if (tid == 0 && lds.valid) atomicAdd(a.valid + (size_t)b * a.n_angles + ang, lds.valid);
    if (kept == 0) return;                                     // uniform
    int32_t* out = w.U + ((size_t)b * a.n_angles + ang) * nb2;
    if (NS == 1) gm_accumulate<1>(lds, w.bound, nxo, nyo, kept, nb2, w.nb, w.D, origin, 0, out);
    else for (int from = 0; from < nb2; from += NS * GM_THREADS) gm_accumulate<NS>(lds, w.bound, nxo, nyo, kept, nb2, w.nb, w.D, origin, from, out);
}

// The workgroup's first maximum of (v, i) pairs (lower i on equal v), valid in thread 0; ends in a barrier
__device__ __forceinline__ void gmw_block_first_max(int& v, int& i, int* wave_v, int* wave_i) {
    const auto greater = [](int x, int y) { return x > y; };
    wave_first_best(v, i, greater);
    if (lane_id() == 0) { wave_v[wave_id()] = v; wave_i[wave_id()] = i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < GM_WAVES; ++k) take_first_best(v, i, wave_v[k], wave_i[k], greater);
}

// 2a. the seeds: one workgroup per (pair, angle), the first block in C order of maximal bound; the pair's largest bound
__global__ __launch_bounds__(GM_THREADS) void gmw_seed_kernel(GmwArgs w) {
    __shared__ int wave_v[GM_WAVES], wave_i[GM_WAVES];
    const int nb2 = w.nb * w.nb, ang = blockIdx.x % w.g.n_angles, b = blockIdx.x / w.g.n_angles;
    const int32_t* u = w.U + (size_t)blockIdx.x * nb2;
    int best = INT32_MIN, at = INT32_MAX;
    for (int i = threadIdx.x; i < nb2; i += GM_THREADS) {
        const int v = u[i];
        if (v > best) { best = v; at = i; }
    }
    gmw_block_first_max(best, at, wave_v, wave_i);
    if (threadIdx.x != 0) return;
    w.seeds[blockIdx.x] = ang * nb2 + at;
    atomicMax(&w.pair[b].max_u, (uint32_t)best ^ 0x80000000u);
}

// The exact scores of block `blk` of pair b over all rows of its cloud, in chunks of GM_CHUNK through phase 1: lane t owns
// shift t mod D^2 of the block, and G = GM_THREADS / D^2 groups of lanes share the rows as gm_score_kernel's NS == 1 path does
// (one lane per shift at D = 16).  Afterwards lds.acc holds the D^2 sums and thread 0 the block's maximum over the shifts
// with j, i < S and its lowest flat index a * S^2 + j * S + i.  Ends in a barrier.
template <int D>
__device__ __forceinline__ void gmw_score_block(GmLds& lds, int* wave_v, int* wave_i, const GmwArgs& w, int b, int blk, int& best, int& at) {
    constexpr int D2 = D * D, G = GM_THREADS / D2;
    const GmArgs& a = w.g;
    const int tid = threadIdx.x, g = tid / D2, s = tid - g * D2;
    const int W = a.window, S = 2 * W + 1, nb2 = w.nb * w.nb;
    const int ang = blk / nb2, rem = blk - ang * nb2, J = rem / w.nb, I = rem - J * w.nb;
    const int c = a.pairs.pair_cloud[b];
    const int N = gm_rows(a.pairs, c);
    const int dx[1] = {I * D - W + s % D}, dy[1] = {J * D - W + s / D};
    int acc[1] = {0};
    lds.acc[tid] = 0;
    const GmReach reach{I * D - W, I * D - W + D - 1, J * D - W, J * D - W + D - 1, a.nx, a.ny};
    for (int base = 0; base < N; base += GM_CHUNK) {
        __syncthreads();                                       // the chunk before has been walked
        const int kept = gm_form_cells(lds, a, b, ang, c, N, base, reach);
        if (kept) gm_walk<1>(lds, a.field, (unsigned)a.nx, (unsigned)a.ny, kept, g, G, dx, dy, acc);
    }
    __syncthreads();
    if (acc[0]) atomicAdd(&lds.acc[s], acc[0]);
    __syncthreads();
    const int j = J * D + tid / D, i = I * D + tid % D;        // (tid < D2: tid is the shift)
    const bool owns = tid < D2 && j < S && i < S;
    best = owns ? lds.acc[tid] : INT32_MIN;
    at = owns ? (ang * S + j) * S + i : INT32_MAX;
    gmw_block_first_max(best, at, wave_v, wave_i);
}

// 2b and 4. exact scores.  Seeds (survivors == 0): workgroup x < n_pairs * n_angles scores the seed block of (pair, angle) into
// the pair's seed word; workgroup n_pairs * n_angles + b scores the block that holds (centre_angle, W, W) and stores that one
// score.  Survivors: a fixed grid strides over the device-side list and merges into the pair's best word.  Every loop is
// bounded by the list's count, a cloud's rows or an argument; no workgroup waits for another.
template <int D>
__global__ __launch_bounds__(GM_THREADS) void gmw_exact_kernel(GmwArgs w, int survivors) {
    __shared__ GmLds lds;
    __shared__ int wave_v[GM_WAVES], wave_i[GM_WAVES];
    const int A = w.g.n_angles, W = w.g.window, nb2 = w.nb * w.nb, per = A * nb2;
    const int n_seeds = w.n_pairs * A;
    // the jobs of this workgroup: entries first, first + step, ... below n of the survivor list, or the one seed or centre block
    const int n = survivors ? min(*w.n_listed, w.n_pairs * per) : (int)blockIdx.x + 1;
    for (long long e = blockIdx.x; e < n; e += gridDim.x) {   // (64-bit: n + the grid may pass 2^31)
        int b, blk;
        if (survivors) {
            const int gb = w.list[e];
            b = gb / per;
            blk = gb - b * per;
        } else if (e < n_seeds) {
            b = (int)e / A;
            blk = w.seeds[e];
        } else {
            b = (int)e - n_seeds;
            blk = w.g.centre_angle * nb2 + (W / D) * w.nb + W / D;
        }
        int best, at;
        gmw_score_block<D>(lds, wave_v, wave_i, w, b, blk, best, at);
        if (threadIdx.x != 0) continue;
        if (survivors) atomicMax(&w.pair[b].best, gmw_key(best, at));
        else if (e < n_seeds) atomicMax(&w.pair[b].seed, gmw_key(best, at));
        else w.pair[b].centre = lds.acc[(W % D) * D + W % D];
    }
}

// 3. the survivors: every block whose bound is >= the pair's seed score (>=, not >: a block whose bound equals it may hold an
// equal score at a lower index).  A workgroup tests GMW_SELECT_VEC * GM_THREADS blocks of one pair, counts in LDS, reserves its
// span of the list with one atomicAdd and adds its count to the pair's.
__global__ __launch_bounds__(GM_THREADS) void gmw_select_kernel(GmwArgs w, int tiles) {
    __shared__ int n_local, span;
    const int tid = threadIdx.x, per = w.g.n_angles * w.nb * w.nb;
    const int b = blockIdx.x / tiles, first = (blockIdx.x - b * tiles) * (GMW_SELECT_VEC * GM_THREADS);
    const int best0 = gmw_key_score(w.pair[b].seed);
    const int32_t* u = w.U + (size_t)b * per;
    if (tid == 0) n_local = 0;
    __syncthreads();
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < GMW_SELECT_VEC; ++k) {
        const unsigned s = (unsigned)first + k * GM_THREADS + tid;             // (unsigned: the last tile may pass 2^31)
        if (s < (unsigned)per && u[s] >= best0) mask |= 1u << k;
    }
    int mine = mask ? atomicAdd(&n_local, __popc(mask)) : 0;
    __syncthreads();
    if (tid == 0 && n_local) {
        span = atomicAdd(w.n_listed, n_local);
        atomicAdd(&w.pair[b].survivors, n_local);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GMW_SELECT_VEC; ++k)
        if (mask >> k & 1) w.list[span + mine++] = b * per + first + k * GM_THREADS + tid;
}

// 5. the record: one wave per pair
__global__ __launch_bounds__(GMW_RECORD_THREADS) void gmw_record_kernel(GmwArgs w) {
    const GmArgs& a = w.g;
    const int b = blockIdx.x, S = 2 * a.window + 1, S2 = S * S;
    const int32_t* valid = a.valid + (size_t)b * a.n_angles;
    int any = 0;
    for (int i = threadIdx.x; i < a.n_angles; i += GMW_RECORD_THREADS) any |= valid[i];
    any = __syncthreads_or(any);
    if (threadIdx.x != 0) return;
    const GmwPair p = w.pair[b];
    const int at = gmw_key_flat(p.best), ang = at / S2, rem = at - ang * S2;
    int32_t* rec = a.records + (size_t)b * ICPMI_GMW_REC_INTS;
    rec[ICPMI_GMREC_STATUS] = gm_status(gm_rows(a.pairs, a.pairs.pair_cloud[b]), any);
    rec[ICPMI_GMREC_ROWS] = valid[ang];
    rec[ICPMI_GMREC_INDEX] = at;
    rec[ICPMI_GMREC_A] = ang;
    rec[ICPMI_GMREC_J] = rem / S;
    rec[ICPMI_GMREC_I] = rem % S;
    rec[ICPMI_GMREC_SCORE] = gmw_key_score(p.best);
    rec[ICPMI_GMREC_CENTRE] = p.centre;
    rec[ICPMI_GMW_REC_BLOCKS] = a.n_angles * w.nb * w.nb;
    rec[ICPMI_GMW_REC_SURVIVORS] = p.survivors;
    rec[ICPMI_GMW_REC_SEED] = gmw_key_score(p.seed);
    rec[ICPMI_GMW_REC_MAX_BOUND] = (int)(p.max_u ^ 0x80000000u);
}

// ── host: the workspace, the plan, the entries ──────────────────────────────
// The workspace, described once: what is zeroed before the launches (the valid-row counts per (pair, angle), the pairs'
// words, the list's count), then the seeds, the bounds and the survivor list — two int32 per block.
struct GmwWs {
    Carve c;
    int32_t* valid;
    GmwPair* pair;
    int32_t* n_listed;
    size_t zeroed;
    int32_t* seeds;
    int32_t* U;
    int32_t* list;
    GmwWs(void* base, size_t n_pairs, size_t n_angles, size_t blocks)
        : c(base), valid(c.take<int32_t>(n_pairs * n_angles * sizeof(int32_t))), pair(c.take<GmwPair>(n_pairs * sizeof(GmwPair))),
          n_listed(c.take<int32_t>(sizeof(int32_t))), zeroed(c.off), seeds(c.take<int32_t>(n_pairs * n_angles * sizeof(int32_t))),
          U(c.take<int32_t>(n_pairs * n_angles * blocks * sizeof(int32_t))), list(c.take<int32_t>(n_pairs * n_angles * blocks * sizeof(int32_t))) {}
    size_t bytes() const { return c.off; }
};

static bool gmw_block_ok(int block) { return block == 4 || block == 8 || block == 16; }

// What a call starts, decided as a whole and without a HIP call.  Nothing depends on the batch but the grids' sizes, and the
// sums are integers: a pair's record does not depend on the batch it is computed in.
struct GmwPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    int nb, n_chunks;         // blocks per axis; row chunks of the largest cloud
    int bound_ns;             // 1: lane groups share the rows (at most GM_THREADS blocks per angle); else GMW_BOUND_NS
    int select_tiles;         // selection workgroups per pair
    unsigned bound_grid;      // (pair, angle, chunk) workgroups; 0: no cloud has a row (every bound is 0)
    unsigned seed_grid;       // (pair, angle)
    unsigned exact_seed_grid; // (pair, angle) and, with a centre angle, one more per pair
    unsigned select_grid;     // pairs * select_tiles
    unsigned score_grid;      // fixed: min(blocks of the batch, ICPMI_GMW_SCORE_GROUPS), striding over the survivors
    unsigned record_grid;     // pairs
    size_t bound_bytes;       // the bounds, zeroed before the launch
};
static GmwPlan plan_grid_search(int n_pairs, int max_n, int n_angles, int window, int block, int centre_angle) {
    GmwPlan p{ICPMI_OK, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n_pairs < 0 || max_n < 0 || n_angles < 1 || window < 0 || !gmw_block_ok(block) || centre_angle >= n_angles) { p.rc = ICPMI_ERR_ARG; return p; }
    if (window > ICPMI_GMW_MAX_WINDOW || n_angles > ICPMI_GMW_MAX_ANGLES || max_n > ICPMI_GM_MAX_ROWS) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    const unsigned long long S = 2ull * window + 1, nb = (S + block - 1) / block, per = n_angles * nb * nb;
    p.nb = (int)nb;
    p.n_chunks = (max_n + GM_CHUNK - 1) / GM_CHUNK;
    const unsigned long long groups = (unsigned long long)n_pairs * n_angles * p.n_chunks;
    if (n_angles * S * S >= (1ull << 31) || n_pairs * per >= (1ull << 31) || groups >= (1ull << 31)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.bound_ns = nb * nb <= GM_THREADS ? 1 : GMW_BOUND_NS;
    p.select_tiles = (int)((per + GMW_SELECT_VEC * GM_THREADS - 1) / (GMW_SELECT_VEC * GM_THREADS));
    p.bound_grid = (unsigned)groups;
    p.seed_grid = (unsigned)n_pairs * n_angles;
    p.exact_seed_grid = p.seed_grid + (centre_angle >= 0 ? n_pairs : 0);
    p.select_grid = (unsigned)n_pairs * p.select_tiles;
    p.score_grid = (unsigned)(n_pairs * per < ICPMI_GMW_SCORE_GROUPS ? n_pairs * per : ICPMI_GMW_SCORE_GROUPS);
    p.record_grid = (unsigned)n_pairs;
    p.bound_bytes = (size_t)(n_pairs * per) * sizeof(int32_t);
    return p;
}

template <int D>
static void gmw_launch_exact(int block, unsigned grid, const GmwArgs& w, int survivors, hipStream_t st) {
    if (block == D) gmw_exact_kernel<D><<<grid, GM_THREADS, 0, st>>>(w, survivors);
    else if constexpr (D < 16) gmw_launch_exact<2 * D>(block, grid, w, survivors, st);
}

}  // namespace icpmi

extern "C" int icpmi_grid_bound_field(const int16_t* field, int32_t ny, int32_t nx, int32_t block, int16_t* out, void* stream) {
    using namespace icpmi;
    if (ny < 0 || nx < 0 || !gmw_block_ok(block)) return ICPMI_ERR_ARG;
    if ((long long)ny * nx == 0) return ICPMI_OK;
    if (!field || !out || ((uintptr_t)field & 15) || ((uintptr_t)out & 15)) return ICPMI_ERR_ARG;
    if ((long long)(ny + block - 1) * (nx + block - 1) >= (1ll << 31)) return ICPMI_ERR_ARG;
    const dim3 grid((unsigned)((nx + block - 1 + GMW_TX - 1) / GMW_TX), (unsigned)((ny + block - 1 + GMW_TY - 1) / GMW_TY));
    if (grid.y > 65535u) return ICPMI_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (block == 4) gmw_bound_field_kernel<4><<<grid, GM_THREADS, 0, st>>>((const short*)field, (short*)out, ny, nx);
    else if (block == 8) gmw_bound_field_kernel<8><<<grid, GM_THREADS, 0, st>>>((const short*)field, (short*)out, ny, nx);
    else gmw_bound_field_kernel<16><<<grid, GM_THREADS, 0, st>>>((const short*)field, (short*)out, ny, nx);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" size_t icpmi_grid_search_workspace_bytes(int32_t n_pairs, int32_t n_angles, int32_t window, int32_t block) {
    using namespace icpmi;
    if (n_pairs < 0 || n_angles < 0 || window < 0 || !gmw_block_ok(block)) return 0;
    const size_t nb = (2 * (size_t)window + 1 + block - 1) / block;
    return GmwWs(nullptr, (size_t)n_pairs, (size_t)n_angles, nb * nb).bytes();
}

extern "C" int icpmi_grid_search_batch(const int16_t* field, const int16_t* bound, int32_t ny, int32_t nx, double min_x, double min_y,
                                       double resolution, const double* pts, const int32_t* off_dev, const int32_t* off_host,
                                       const int32_t* cnt_dev, int32_t n_clouds, const int32_t* pair_cloud,
                                       const int32_t* pair_cloud_host, int32_t n_pairs, const double* pair_t, const double* cos_sin,
                                       int32_t n_angles, int32_t window, int32_t block, int32_t centre_angle, int32_t* out_records,
                                       int32_t* out_bounds, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (n_pairs == 0) return ICPMI_OK;
    const PairScan pairs = scan_pairs(n_pairs, n_clouds, off_host, pair_cloud_host);
    if (pairs.rc != ICPMI_OK) return pairs.rc;
    const GmwPlan plan = plan_grid_search(n_pairs, pairs.max_n, n_angles, window, block, centre_angle);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (!field || !bound || !pts || !off_dev || !pair_cloud || !pair_t || !cos_sin || !out_records || !workspace) return ICPMI_ERR_ARG;
    if (ny < 1 || nx < 1 || ny > GM_CELL_MAX || nx > GM_CELL_MAX || (long long)(ny + block - 1) * (nx + block - 1) >= (1ll << 31)) return ICPMI_ERR_ARG;
    if (!world_ok(resolution, min_x, min_y)) return ICPMI_ERR_ARG;
    const GmwWs ws(workspace, (size_t)n_pairs, (size_t)n_angles, (size_t)plan.nb * plan.nb);
    if (workspace_bytes < ws.bytes()) return ICPMI_ERR_WORKSPACE;

    int32_t* U = out_bounds ? out_bounds : ws.U;
    const GmwArgs w{GmArgs{(const short*)field, ny, nx, {min_x, min_y, resolution, pts, off_dev, cnt_dev, pair_cloud, pair_t, cos_sin},
                           n_angles, window, centre_angle, plan.n_chunks, ws.valid, nullptr, out_records},
                    (const short*)bound, n_pairs, block, plan.nb, U, ws.seeds, ws.list, ws.n_listed, ws.pair};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws.valid, 0, ws.zeroed, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (hipMemsetAsync(U, 0, plan.bound_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    if (plan.bound_grid) {
        if (plan.bound_ns == 1) gmw_bound_kernel<1><<<plan.bound_grid, GM_THREADS, 0, st>>>(w);
        else gmw_bound_kernel<GMW_BOUND_NS><<<plan.bound_grid, GM_THREADS, 0, st>>>(w);
        ICPMI_LAUNCH_CHECK();
    }
    gmw_seed_kernel<<<plan.seed_grid, GM_THREADS, 0, st>>>(w);
    ICPMI_LAUNCH_CHECK();
    gmw_launch_exact<4>(block, plan.exact_seed_grid, w, 0, st);
    ICPMI_LAUNCH_CHECK();
    gmw_select_kernel<<<plan.select_grid, GM_THREADS, 0, st>>>(w, plan.select_tiles);
    ICPMI_LAUNCH_CHECK();
    gmw_launch_exact<4>(block, plan.score_grid, w, 1, st);
    ICPMI_LAUNCH_CHECK();
    gmw_record_kernel<<<plan.record_grid, GMW_RECORD_THREADS, 0, st>>>(w);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
