// signature.hip — appearance signatures of a resident scan history: loop-closure candidates by what a scan looks like.
//
// Reference slam.py:230-268 (_find_loop_candidates) picks candidates by the distance between pose ESTIMATES; once drift
// exceeds its threshold the true revisit is never tried.  A signature is a binary polar occupancy image of a scan about
// its sensor (32 rings x 64 sectors, one uint64 per ring), and two scans of one place taken under different headings
// have images that differ by a rotation of the sector axis — a 64-bit rotate of every word.  include/icpmi.h states the
// row rule, the score and the records; tests/signatures_ref.py restates them in NumPy, and everything here is bit-equal
// to that: integers throughout, the only floating-point work is products, one sum and comparisons of the row rule
// (the file is compiled with -ffp-contract=off like the rest), and the sector directions come in a table from the host.
//
// Three kernels:
//   sig_add_kernel      one workgroup per cloud: rows strided over the threads, OR into 32 words of LDS (OR is commutative
//                       and idempotent: no order to fix), then 32 lanes write the words and their popcount.
//   sig_pairs_kernel    the hot path, every (query, candidate) pair: a wave holds its query for its whole life with lane s
//                       keeping rotr64(A[r], s) for the 32 rings (64 registers), because
//                       popcount(A & rotl(B, s)) == popcount(rotr(A, s) & B): the rotation is paid once per wave, and a
//                       candidate costs each lane 32 x (two ANDs with wave-uniform words, two popcount-accumulates) — 128
//                       vector operations.  The candidate's words depend on the wave alone (scalar loads, no LDS).  The
//                       arg-max over the 64 shifts with the lowest shift on ties is one wave max of (best << 6) | (63 - s).
//   sig_select_kernel   one workgroup per query: top_k rounds of a workgroup-wide minimum of ((65535 - score) << 32) | id
//                       over the query's row of packed scores, then `best` of the winners again from their words.
#include "common.hpp"

namespace icpmi {

constexpr int SIG_ADD_THREADS = 256;
constexpr int SIG_PAIR_WAVES = 4;                                     // waves of a workgroup of the pair kernel
constexpr int SIG_PAIRS_PER_WAVE = ICPMI_SIG_TILE / SIG_PAIR_WAVES;   // candidates a wave takes behind one query setup
constexpr int SIG_SELECT_THREADS = 256;
static_assert(ICPMI_SIG_SECTORS == ICPMI_WAVE, "one lane per shift");
static_assert(SIG_PAIRS_PER_WAVE * SIG_PAIR_WAVES == ICPMI_SIG_TILE && SIG_PAIRS_PER_WAVE <= ICPMI_WAVE, "lane j keeps candidate j");
static_assert(ICPMI_SIG_TABLE_DOUBLES == ICPMI_SIG_RINGS + 1 + 2 * 15, "edge2[33], bc[1..15], bs[1..15]");

// ── the row rule ────────────────────────────────────────────────────────────────────────────────────────────────────
__global__ __launch_bounds__(SIG_ADD_THREADS) void sig_add_kernel(const double2* __restrict__ pts, const int32_t* __restrict__ off,
                                                                  int row_capacity, int first, const double* __restrict__ tables,
                                                                  unsigned long long* __restrict__ sig, int32_t* __restrict__ sig_bits) {
    __shared__ unsigned int words[ICPMI_SIG_RINGS * 2];               // {low, high} halves of the 32 words
    __shared__ double tab[ICPMI_SIG_TABLE_DOUBLES];
    const int c = first + (int)blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (tid < ICPMI_SIG_RINGS * 2) words[tid] = 0u;
    if (tid < ICPMI_SIG_TABLE_DOUBLES) tab[tid] = tables[tid];
    __syncthreads();
    const double* edge2 = tab;
    const double* bc = tab + (ICPMI_SIG_RINGS + 1) - 1;               // bc[k], k = 1 .. 15
    const double* bs = bc + 15;
    const int begin = off[c];
    int n = off[c + 1] - begin;
    if (begin < 0 || n < 0 || begin > row_capacity - n) n = 0;        // (the host refuses such offsets; never read past the rows)
    for (int i = tid; i < n; i += SIG_ADD_THREADS) {
        const double2 p = pts[(size_t)begin + i];
        const double d2 = p.x * p.x + p.y * p.y;
        int ring = -1;
#pragma unroll
        for (int j = 0; j <= ICPMI_SIG_RINGS; ++j) ring += d2 >= edge2[j] ? 1 : 0;
        if (ring < 0 || ring >= ICPMI_SIG_RINGS) continue;
        const int q = p.y >= 0.0 ? (p.x > 0.0 ? 0 : 1) : (p.x < 0.0 ? 2 : 3);
        const double u = q == 0 ? p.x : q == 1 ? p.y : q == 2 ? -p.x : -p.y;
        const double v = q == 0 ? p.y : q == 1 ? -p.x : q == 2 ? -p.y : p.x;
        int sector = 16 * q;
#pragma unroll
        for (int k = 1; k <= 15; ++k) sector += v * bc[k] >= u * bs[k] ? 1 : 0;
        atomicOr(&words[2 * ring + (sector >> 5)], 1u << (sector & 31));
    }
    __syncthreads();
    if (tid < ICPMI_WAVE) {                                            // one whole wave: lanes 0 .. 31 carry a word each
        const bool has = tid < ICPMI_SIG_RINGS;
        const unsigned lo = has ? words[2 * tid] : 0u, hi = has ? words[2 * tid + 1] : 0u;
        if (has) sig[(size_t)c * ICPMI_SIG_RINGS + tid] = ((unsigned long long)hi << 32) | lo;
        const int bits = wave_sum((int)(__popc(lo) + __popc(hi)));
        if (tid == 0) sig_bits[c] = bits;
    }
}

// ── every pair ──────────────────────────────────────────────────────────────────────────────────────────────────────
__device__ __forceinline__ unsigned wave_max(unsigned v) {            // as common.hpp's wave_max(float): four steps inside the rows, two across
    v = max(v, (unsigned)dpp_b32<0xB1>((int)v));
    v = max(v, (unsigned)dpp_b32<0x4E>((int)v));
    v = max(v, (unsigned)dpp_b32<0x141>((int)v));
    v = max(v, (unsigned)dpp_b32<0x140>((int)v));
    unsigned x, y;
    swap_self<true>(v, x, y);
    swap_self<false>(max(x, y), x, y);
    return max(x, y);
}

__device__ __forceinline__ int sig_score(int bits_a, int bits_b, int best) {
    const unsigned uni = (unsigned)(bits_a + bits_b - best);
    return uni ? (int)(((unsigned)best * 65535u) / uni) : 0;
}

// The range of query i clipped to [0, n_scans); empty for a query id that names no cloud of the store.
__device__ __forceinline__ void sig_range(const int32_t* query_ids, const int32_t* lo, const int32_t* hi, int i, int n_scans,
                                          int scan_capacity, int& qid, int& from, int& to) {
    qid = query_ids[i];
    from = max(lo[i], 0);
    to = min(hi[i], n_scans);
    if (qid < 0 || qid >= scan_capacity || from > to) from = to;     // (from <= to <= n_scans from here on)
}

// grid (tiles of ICPMI_SIG_TILE candidates, queries); rows [n_queries][n_scans]: (score << 8) | shift, -1 outside the range
__global__ __launch_bounds__(SIG_PAIR_WAVES* ICPMI_WAVE) void sig_pairs_kernel(const unsigned long long* __restrict__ sig,
                                                                               const int32_t* __restrict__ sig_bits,
                                                                               const int32_t* __restrict__ query_ids,
                                                                               const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                               int n_scans, int scan_capacity, int32_t* __restrict__ rows) {
    const int i = (int)blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(wave_id());          // wave-uniform, and known to be: the loads below are scalar
    const int lane = lane_id();
    const int c0 = (int)blockIdx.x * ICPMI_SIG_TILE + w * SIG_PAIRS_PER_WAVE;
    if (c0 >= n_scans) return;
    const int c1 = min(c0 + SIG_PAIRS_PER_WAVE, n_scans);
    int qid, from, to;
    sig_range(query_ids, lo, hi, i, n_scans, scan_capacity, qid, from, to);
    int32_t* out = rows + (size_t)i * n_scans;
    if (to <= c0 || from >= c1 || from >= to) {                       // no candidate of this wave is in the range
        if (c0 + lane < c1) out[c0 + lane] = -1;
        return;
    }
    // the query, turned back by this lane's shift, once
    const unsigned long long* A = sig + (size_t)qid * ICPMI_SIG_RINGS;
    unsigned a_lo[ICPMI_SIG_RINGS], a_hi[ICPMI_SIG_RINGS];
#pragma unroll
    for (int r = 0; r < ICPMI_SIG_RINGS; ++r) {
        const unsigned long long x = A[r], t = (x >> lane) | (x << ((64 - lane) & 63));
        a_lo[r] = (unsigned)t;
        a_hi[r] = (unsigned)(t >> 32);
    }
    const int bits_a = sig_bits[qid];
    unsigned mine = 0;                                                 // lane j: the key of candidate c0 + j
    for (int c = c0; c < c1; ++c) {
        if (c < from || c >= to) continue;                             // (wave-uniform)
        const unsigned* B = reinterpret_cast<const unsigned*>(sig + (size_t)c * ICPMI_SIG_RINGS);      // {low, high} of every word
        unsigned inter = 0;                                            // one chain: each popcount adds into it (v_bcnt_u32_b32 dst, src, acc)
#pragma unroll
        for (int r = 0; r < ICPMI_SIG_RINGS; ++r) {
            inter = (unsigned)__popc(a_lo[r] & B[2 * r]) + inter;
            inter = (unsigned)__popc(a_hi[r] & B[2 * r + 1]) + inter;
        }
        const unsigned key = wave_max((inter << 6) | (unsigned)(63 - lane));
        if (lane == c - c0) mine = key;
    }
    const int c = c0 + lane;
    if (c < c1) {
        int packed = -1;
        if (c >= from && c < to) {
            const int best = (int)(mine >> 6), shift = 63 - (int)(mine & 63u);
            packed = (sig_score(bits_a, sig_bits[c], best) << 8) | shift;
        }
        out[c] = packed;
    }
}

// ── the selection ───────────────────────────────────────────────────────────────────────────────────────────────────
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)v, o, ICPMI_WAVE);
        v = other < v ? other : v;
    }
    return v;
}

__global__ __launch_bounds__(SIG_SELECT_THREADS) void sig_select_kernel(const unsigned long long* __restrict__ sig,
                                                                        const int32_t* __restrict__ query_ids,
                                                                        const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                        int n_scans, int scan_capacity, int top_k,
                                                                        const int32_t* __restrict__ rows, int32_t* __restrict__ out_records) {
    constexpr int WAVES = SIG_SELECT_THREADS / ICPMI_WAVE;
    constexpr unsigned long long NONE = ~0ull;
    __shared__ unsigned long long part[2][WAVES];
    __shared__ unsigned long long chosen[ICPMI_SIG_MAX_TOP];
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, w = wave_id(), lane = lane_id();
    int qid, from, to;
    sig_range(query_ids, lo, hi, i, n_scans, scan_capacity, qid, from, to);
    const int32_t* row = rows + (size_t)i * n_scans;
    unsigned long long floor_key = 0;                                  // keys are distinct (the id is part of them): the next one is above the last
    for (int k = 0; k < top_k; ++k) {
        unsigned long long best = NONE;
        for (int c = from + tid; c < to; c += SIG_SELECT_THREADS) {
            const int packed = row[c];
            if (packed < 0) continue;
            const unsigned long long key = ((unsigned long long)(65535 - (packed >> 8)) << 32) | (unsigned)c;
            if (key >= floor_key && key < best) best = key;
        }
        best = wave_min(best);
        if (lane == 0) part[k & 1][w] = best;
        __syncthreads();                                               // one barrier a round: the slots alternate
        best = part[k & 1][0];
#pragma unroll
        for (int j = 1; j < WAVES; ++j) best = part[k & 1][j] < best ? part[k & 1][j] : best;
        if (tid == 0) chosen[k] = best;
        floor_key = best == NONE ? NONE : best + 1;
    }
    __syncthreads();
    // records: wave w writes slots w, w + WAVES, ...; `best` of a winner is its 32 popcounts at the winning shift again
    for (int k = w; k < top_k; k += WAVES) {
        const unsigned long long key = chosen[k];
        int32_t* rec = out_records + ((size_t)i * top_k + k) * ICPMI_SIG_REC_INTS;
        if (key == NONE) {
            if (lane < ICPMI_SIG_REC_INTS) rec[lane] = lane == ICPMI_SIG_REC_ID ? -1 : 0;
            continue;
        }
        const int id = (int)(key & 0xffffffffull), score = 65535 - (int)(key >> 32);
        const int shift = row[id] & 63;
        int part_bits = 0;
        if (lane < ICPMI_SIG_RINGS) {
            const unsigned long long a = sig[(size_t)qid * ICPMI_SIG_RINGS + lane], b = sig[(size_t)id * ICPMI_SIG_RINGS + lane];
            part_bits = __popcll(a & ((b << shift) | (b >> ((64 - shift) & 63))));
        }
        const int best = wave_sum(part_bits);
        if (lane == 0) {
            rec[ICPMI_SIG_REC_ID] = id;
            rec[ICPMI_SIG_REC_SCORE] = score;
            rec[ICPMI_SIG_REC_SHIFT] = shift;
            rec[ICPMI_SIG_REC_BEST] = best;
        }
    }
}

struct SimilarPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    dim3 pairs_grid;          // x == 0: no candidate at all, the selection alone writes its padding
    unsigned select_grid;     // 0: nothing to do
    size_t rows_bytes;        // of the [n_queries][n_scans] rows
};
static SimilarPlan plan_similar(int n_queries, int n_scans, int top_k) {
    SimilarPlan p{ICPMI_OK, dim3(0, 1, 1), 0, 0};
    if (n_queries < 0 || n_scans < 0 || top_k < 1 || top_k > ICPMI_SIG_MAX_TOP) { p.rc = ICPMI_ERR_ARG; return p; }
    if ((long long)n_queries * n_scans >= (1ll << 31) || n_queries > 65535) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.pairs_grid = dim3((unsigned)((n_scans + ICPMI_SIG_TILE - 1) / ICPMI_SIG_TILE), (unsigned)n_queries, 1);
    p.select_grid = (unsigned)n_queries;
    p.rows_bytes = (size_t)n_queries * n_scans * sizeof(int32_t);
    return p;
}

}  // namespace icpmi

extern "C" int icpmi_history_signatures_add(const icpmi_history* h, uint64_t* sig, int32_t* sig_bits, const double* tables,
                                            const int32_t* off_host, int32_t first, int32_t n_new, void* stream) {
    using namespace icpmi;
    if (!h || !h->pts || !h->off_dev || h->scan_capacity <= 0 || h->row_capacity <= 0) return ICPMI_ERR_ARG;
    if (!sig || !sig_bits || !tables || !off_host || first < 0 || n_new < 0 || first > h->scan_capacity - n_new) return ICPMI_ERR_ARG;
    if (n_new == 0) return ICPMI_OK;
    int max_n, end_row;
    if (off_host[first] < 0 || !cloud_rows(off_host + first, n_new, max_n, end_row)) return ICPMI_ERR_ARG;
    if (end_row > h->row_capacity) return ICPMI_ERR_ARG;
    sig_add_kernel<<<(unsigned)n_new, SIG_ADD_THREADS, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const double2*>(h->pts), h->off_dev, h->row_capacity, first, tables,
        reinterpret_cast<unsigned long long*>(sig), sig_bits);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" size_t icpmi_history_similar_workspace_bytes(int32_t n_queries, int32_t n_scans, int32_t top_k) {
    using namespace icpmi;
    const SimilarPlan p = plan_similar(n_queries, n_scans, top_k);
    return p.rc == ICPMI_OK ? align256(p.rows_bytes) + (p.rows_bytes ? 0 : 256) : 0;
}

extern "C" int icpmi_history_similar(const icpmi_history* h, const uint64_t* sig, const int32_t* sig_bits, const int32_t* query_ids,
                                     int32_t n_queries, const int32_t* lo, const int32_t* hi, int32_t n_scans, int32_t top_k,
                                     int32_t* out_records, int32_t* out_all, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const SimilarPlan p = plan_similar(n_queries, n_scans, top_k);
    if (p.rc != ICPMI_OK) return p.rc;
    if (!h || h->scan_capacity <= 0 || n_scans > h->scan_capacity) return ICPMI_ERR_ARG;
    if (p.select_grid == 0) return ICPMI_OK;
    if (!sig || !sig_bits || !query_ids || !lo || !hi || !out_records || !workspace || ((uintptr_t)workspace & 15)) return ICPMI_ERR_ARG;
    if (workspace_bytes < icpmi_history_similar_workspace_bytes(n_queries, n_scans, top_k)) return ICPMI_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* rows = out_all ? out_all : (int32_t*)workspace;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(sig);
    if (p.pairs_grid.x) {
        sig_pairs_kernel<<<p.pairs_grid, SIG_PAIR_WAVES * ICPMI_WAVE, 0, st>>>(words, sig_bits, query_ids, lo, hi, n_scans, h->scan_capacity, rows);
        ICPMI_LAUNCH_CHECK();
    }
    sig_select_kernel<<<p.select_grid, SIG_SELECT_THREADS, 0, st>>>(words, query_ids, lo, hi, n_scans, h->scan_capacity, top_k, rows, out_records);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
