// particles.hpp — what the particle filter's kernels and its host entries share (particles.hip; include/icpmi.h: icpmi_pf_*):
// the counter-based generator and the deviates made of its halves, for the host and the device alike; the workspace and the
// free index, each once; and the host plans: what each entry starts, decided as a whole and without a HIP call (the idiom
// of gridpairs.hpp).
#pragma once
#include "gridcast.hpp"

namespace icpmi {

constexpr int PF_THREADS = ICPMI_PF_THREADS;
constexpr int PF_WAVES = PF_THREADS / ICPMI_WAVE;
constexpr int PF_LANE_WEIGHTS = ICPMI_PF_SCAN_BLOCK / PF_THREADS;             // consecutive weights of a lane in a scan block
constexpr int PF_MAX_BLOCKS = ICPMI_PF_MAX_PARTICLES / ICPMI_PF_SCAN_BLOCK;   // block sums the one second-level workgroup scans
static_assert(PF_THREADS % ICPMI_WAVE == 0 && ICPMI_PF_SCAN_BLOCK % PF_THREADS == 0 && ICPMI_PF_EST_CHUNK % PF_THREADS == 0, "whole waves, whole lanes");
static_assert(PF_MAX_BLOCKS == PF_THREADS * ICPMI_PF_SUMS_PER_LANE, "one workgroup scans every block sum of the largest filter");
static_assert((unsigned long long)ICPMI_PF_MAX_WEIGHT * ICPMI_PF_MAX_PARTICLES <= (1ull << 40), "W <= 2^40: n * C + rho < 2^61");
static_assert(ICPMI_PF_MAX_PARTICLES <= (1 << 30), "E_i <= n is a uint32, an ancestor an int32");
static_assert(ICPMI_PF_PREDICT_BLOCKS * 8 >= 36, "three deviates of twelve halves each");

// ── Philox4x32-10 (Random123): ten rounds over a 4-word counter under a 2-word key, the key raised between rounds ─────────
struct Philox {
    uint32_t v[4];
};
__host__ __device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}
__host__ __device__ __forceinline__ Philox pf_draw(uint64_t seed, uint32_t particle, uint32_t block, uint32_t step, uint32_t purpose) {
    return philox4x32_10(particle, block, step, purpose, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// The three deviates of a particle: halves 12 m .. 12 m + 11 of its 40, the low half of a word first.  S_m is an integer
// below 2^20, so (S_m - 393210) * 2^-16 is exact.
__host__ __device__ __forceinline__ void pf_deviates(uint64_t seed, uint32_t particle, uint32_t step, double (&z)[3]) {
    uint32_t S[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < ICPMI_PF_PREDICT_BLOCKS; ++b) {
        const Philox r = pf_draw(seed, particle, (uint32_t)b, step, ICPMI_PF_PURPOSE_PREDICT);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int h = 8 * b + 2 * k;                       // the word's low half; h + 1 its high half (h even: one deviate holds both)
            if (h < 36) S[h / 12] += (r.v[k] & 0xffffu) + (r.v[k] >> 16);
        }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) z[m] = (double)((int)S[m] - 393210) * (1.0 / 65536.0);
}

// ── the workspace of icpmi_pf_resample and icpmi_pf_estimate, described once (common.hpp: Carve) ─────────────────────────
struct PfWs {
    Carve c;
    uint64_t* head;           // [2]: W, rho
    uint64_t* block_sums;     // [blocks]: the sum of each scan block, then (in place) the sum of the blocks before it
    uint32_t* E;              // [n]: E_i
    double* partials;         // [chunks][ICPMI_PF_EST_DOUBLES]
    PfWs(void* base, int blocks, int chunks, int n)
        : c(base), head(c.take<uint64_t>(2 * sizeof(uint64_t))), block_sums(c.take<uint64_t>((size_t)blocks * sizeof(uint64_t))),
          E(c.take<uint32_t>((size_t)n * sizeof(uint32_t))), partials(c.take<double>((size_t)chunks * ICPMI_PF_EST_DOUBLES * sizeof(double))) {}
    size_t bytes() const { return c.off; }
};

// ── the host plan ────────────────────────────────────────────────────────────
struct PfPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    bool nothing;             // n == 0: ICPMI_OK and nothing to do
    unsigned lanes_grid;      // a lane per particle: predict, max, weights, gather
    unsigned blocks;          // scan blocks: block sums, offspring
    unsigned chunks;          // the estimate's workgroups
    size_t ws_bytes;
};
inline PfPlan plan_particles(int n) {
    PfPlan p{ICPMI_OK, n == 0, 0, 0, 0, 0};
    if (n < 0) p.rc = ICPMI_ERR_ARG;
    else if (n > ICPMI_PF_MAX_PARTICLES) p.rc = ICPMI_ERR_UNSUPPORTED;
    if (p.rc != ICPMI_OK || p.nothing) return p;
    p.lanes_grid = (unsigned)((n + PF_THREADS - 1) / PF_THREADS);
    p.blocks = (unsigned)((n + ICPMI_PF_SCAN_BLOCK - 1) / ICPMI_PF_SCAN_BLOCK);
    p.chunks = (unsigned)((n + ICPMI_PF_EST_CHUNK - 1) / ICPMI_PF_EST_CHUNK);
    p.ws_bytes = PfWs(nullptr, (int)p.blocks, (int)p.chunks, n).bytes();
    return p;
}
// ── the free index of icpmi_pf_free_index, described once: the host sizes and carves it, the draw finds its parts from the
// header's `words` alone ─────────────────────────────────────────────────────
constexpr int PF_FREE_LANE_WORDS = ICPMI_PFG_FREE_BLOCK / PF_THREADS;         // consecutive words of a lane in a scan block
constexpr int PF_FREE_MAX_BLOCKS = ICPMI_PFG_FREE_MAX_WORDS / ICPMI_PFG_FREE_BLOCK;
static_assert(ICPMI_PFG_FREE_BLOCK % (4 * PF_THREADS) == 0, "a lane's words are whole groups of four");
static_assert(PF_FREE_MAX_BLOCKS == PF_THREADS * ICPMI_PF_SUMS_PER_LANE, "one workgroup scans every block sum of the largest index");
static_assert(ICPMI_PFG_FREE_MAX_WORDS == (1 << 22), "the draw's bisection: 22 halvings, at most 23 steps");
static_assert(ICPMI_PFG_FREE_HEADER >= 3 && ICPMI_PFG_FREE_HEADER <= ICPMI_WAVE, "one wave writes the header");

struct PfFreeIndex {
    Carve c;
    uint32_t* header;         // [ICPMI_PFG_FREE_HEADER]: F, words, wpr, 0 ...
    uint32_t* free;           // [words]: the masked free word of every plane word
    uint32_t* rank;           // [words]: the free cells in the words before it
    uint32_t* block_sums;     // [blocks]: the build's scratch — the free cells of each scan block, then of the blocks before it
    __host__ __device__ static unsigned blocks_of(size_t words) { return (unsigned)((words + ICPMI_PFG_FREE_BLOCK - 1) / ICPMI_PFG_FREE_BLOCK); }
    __host__ __device__ PfFreeIndex(void* base, size_t words)
        : c(base), header(c.take<uint32_t>(ICPMI_PFG_FREE_HEADER * sizeof(uint32_t))), free(c.take<uint32_t>(words * sizeof(uint32_t))),
          rank(c.take<uint32_t>(words * sizeof(uint32_t))), block_sums(c.take<uint32_t>(blocks_of(words) * sizeof(uint32_t))) {}
    __host__ __device__ size_t bytes() const { return c.off; }
};

// What icpmi_pf_free_index starts, decided as a whole and without a HIP call
struct PfFreePlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    int wpr;
    unsigned words, blocks;   // blocks == 0 (an empty grid): the header alone
    int x0, y0, x1, y1;       // the box clipped to the grid; x1 <= x0 or y1 <= y0: empty
    size_t plane_bytes, index_bytes;
};
inline PfFreePlan plan_free_index(int ny, int nx, int x0, int y0, int x1, int y1) {
    PfFreePlan p{ICPMI_OK, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const GcPlan grid = plan_cast(ny, nx, 0, 0);
    if (grid.rc != ICPMI_OK) { p.rc = grid.rc; return p; }
    const GcPlanes L(ny, nx);
    if (L.words > (size_t)ICPMI_PFG_FREE_MAX_WORDS) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.wpr = L.wpr;
    p.words = (unsigned)L.words;
    p.blocks = PfFreeIndex::blocks_of(L.words);
    // both ends of both axes into the grid: the kernels only ever see 0 <= x0, x1 <= nx and 0 <= y0, y1 <= ny, so their
    // mask arithmetic stays far from the ends of int whatever int32 the caller passed
    const auto into = [](int v, int n) { return v < 0 ? 0 : (v > n ? n : v); };
    p.x0 = into(x0, nx);
    p.y0 = into(y0, ny);
    p.x1 = into(x1, nx);
    p.y1 = into(y1, ny);
    p.plane_bytes = L.bytes;
    p.index_bytes = PfFreeIndex(nullptr, L.words).bytes();
    return p;
}

inline bool misaligned8(const void* p) { return ((uintptr_t)p & 7) != 0; }
inline int pf_workspace_rc(const PfPlan& plan, const void* workspace, size_t workspace_bytes) {
    return !workspace || misaligned16(workspace) || workspace_bytes < plan.ws_bytes ? ICPMI_ERR_WORKSPACE : ICPMI_OK;
}

}  // namespace icpmi
