// gridmoments.hip — the moments of a correlative match (include/icpmi.h: icpmi_grid_match_moments).  gridmatch.hip leaves a
// score volume and the record of its first maximum; this reads the volume once more and sums, per pair, the weighted moments
// of the candidates about that winner — what the host turns into a sub-cell pose and a covariance (icpmi/gridmatch.py:
// gaussian_of_moments).  The weight of a candidate is an integer function of its score, the sums are int64, so any split of
// the candidates over workgroups and any order of the integer atomics gives the same twelve numbers.
#include "gridmatch.hpp"

namespace icpmi {

constexpr int GMOM_LOADS = 4;                              // candidates of a thread in flight together
constexpr int GMOM_STEP = GM_THREADS * GMOM_LOADS;         // candidates a workgroup takes per step
constexpr int GMOM_MAX_CHUNKS = 64;                        // workgroups of one pair, at most
constexpr int GMOM_ZERO_AT = 8 * (ICPMI_GMOM_WEIGHT_BITS + 1);   // u from which the weight is 0: e = u >> 3 > 20
constexpr int GMOM_A_BITS = 34, GMOM_J_BITS = 18;          // the shifts of the two multiply-shift divisions (plan_grid_moments)
static_assert(ICPMI_GMOM_II + 1 == ICPMI_GMOM_SUPPORT && ICPMI_GMOM_EDGE + 1 == ICPMI_GMOM_INTS, "twelve slots");
static_assert((1 << ICPMI_GMOM_WEIGHT_BITS) >> (GMOM_ZERO_AT >> 3) == 0, "T[0] >> 21 is 0: the clamp of d needs no second test");
static_assert((long long)ICPMI_GM_MAX_ANGLES * (2 * ICPMI_GM_MAX_WINDOW + 1) * (2 * ICPMI_GM_MAX_WINDOW + 1) < (1ll << 22), "a flat index has 22 bits");
static_assert((2 * ICPMI_GM_MAX_WINDOW + 1) < (1 << 6), "S has 6 bits, S^2 has 12");

struct GmomArgs {
    const int32_t* volume;    // [n_pairs][n]
    const int32_t* records;   // [n_pairs][ICPMI_GMREC_INTS]
    long long* moments;       // [n_pairs][ICPMI_GMOM_INTS], zeroed on the stream before the launch
    int n_angles, S, S2, n;   // n = n_angles * S2 candidates of a pair
    int n_chunks, span;       // workgroups of a pair; candidates of one (a multiple of GMOM_STEP)
    int half_step;
    unsigned long long magic_a;   // floor(2^34 / S2) + 1
    unsigned magic_j;             // floor(2^18 / S) + 1
};

// w(d) of include/icpmi.h for a drop d >= 0 below the best score; h >= 1, cut = 21 h, inv_h ~ 1 / h in float32.
// d is clamped to 21 h first: u is then at most 168 = GMOM_ZERO_AT, where e = 21 shifts every table value to 0.  u = floor(8 d
// / h) exactly: the float32 estimate is within 168 * 2^-21 of the quotient, so its floor is off by at most one either way, and
// the 64-bit test u h <= 8 d < (u + 1) h settles it.  No division, no branch.
__device__ __forceinline__ int gmom_weight(long long d, long long h, long long cut, float inv_h) {
    const long long d8 = 8 * (d < cut ? d : cut);
    int u = (int)((float)d8 * inv_h);
    const long long uh = (long long)u * h;
    u += (uh + h <= d8) - (uh > d8);
    const int f = u & 7, e = u >> 3;
    // T[f] = rint(2^20 * 2^(-f / 8)), picked by the three bits of f
    const int t0 = f & 1 ? 961548 : 1048576, t2 = f & 1 ? 808563 : 881744, t4 = f & 1 ? 679917 : 741455, t6 = f & 1 ? 571740 : 623487;
    const int t03 = f & 2 ? t2 : t0, t47 = f & 2 ? t6 : t4;
    return (f & 4 ? t47 : t03) >> e;
}

// One workgroup per (chunk of `span` candidates, pair).  Thread t takes the candidates from + t, from + t + GM_THREADS, ... —
// consecutive lanes read consecutive int32 — GMOM_LOADS of them in flight per step, derives (a, j, i) from the flat index by
// two multiply-shifts and keeps the twelve sums in registers.  Then a wave reduction of each sum, the four waves meet in LDS,
// and ONE 64-bit integer atomicAdd per non-zero slot.  No workgroup waits for another; every loop is bounded by an argument.
__global__ __launch_bounds__(GM_THREADS) void gm_moments_kernel(GmomArgs a) {
    __shared__ long long part[GM_WAVES][ICPMI_GMOM_INTS];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % a.n_chunks, b = blockIdx.x / a.n_chunks;
    const int32_t* rec = a.records + (size_t)b * ICPMI_GMREC_INTS;
    if (rec[ICPMI_GMREC_STATUS] == ICPMI_GM_ST_CAPACITY) return;   // uniform, before the barrier: the memset's twelve zeros stay
    const int wa = rec[ICPMI_GMREC_A], wj = rec[ICPMI_GMREC_J], wi = rec[ICPMI_GMREC_I];
    const long long best = rec[ICPMI_GMREC_SCORE];
    const long long hh = (long long)rec[ICPMI_GMREC_ROWS] * a.half_step, h = hh < 1 ? 1 : hh, cut = (GMOM_ZERO_AT / 8) * h;
    const float inv_h = 1.0f / (float)h;
    const int32_t* __restrict__ vol = a.volume + (size_t)b * a.n;
    const int from = chunk * a.span, to = min(from + a.span, a.n);
    const int A1 = a.n_angles > 1 ? a.n_angles - 1 : -1, S1 = a.S > 1 ? a.S - 1 : -1;     // the far faces; -1: the axis has none
    const int lowA = a.n_angles > 1 ? 0 : -1, lowS = a.S > 1 ? 0 : -1;

    long long m[ICPMI_GMOM_INTS];
#pragma unroll
    for (int s = 0; s < ICPMI_GMOM_INTS; ++s) m[s] = 0;
    for (int at = from + tid; at < to; at += GMOM_STEP) {         // (the lanes of a wave may leave at different steps: no barrier inside)
        int score[GMOM_LOADS];
#pragma unroll
        for (int k = 0; k < GMOM_LOADS; ++k) score[k] = vol[min(at + k * GM_THREADS, to - 1)];
#pragma unroll
        for (int k = 0; k < GMOM_LOADS; ++k) {
            const unsigned f = at + k * GM_THREADS;
            const int ia = (int)(((unsigned long long)f * a.magic_a) >> GMOM_A_BITS);
            const unsigned rem = f - (unsigned)ia * (unsigned)a.S2;
            const int ij = (int)((rem * a.magic_j) >> GMOM_J_BITS), ii = (int)rem - ij * a.S;
            const long long drop = best - (long long)score[k];
            const int wt = gmom_weight(drop < 0 ? 0 : drop, h, cut, inv_h);
            const int w = (int)f < to ? wt : 0;                    // a load past the chunk re-read its last candidate: no weight
            const int da = ia - wa, dj = ij - wj, di = ii - wi;
            const int wda = w * da, wdj = w * dj, wdi = w * di;    // |da| < 2^10, w <= 2^20: int32
            const bool face = ia == lowA || ia == A1 || ij == lowS || ij == S1 || ii == lowS || ii == S1;
            m[ICPMI_GMOM_W] += w;
            m[ICPMI_GMOM_A] += wda;
            m[ICPMI_GMOM_J] += wdj;
            m[ICPMI_GMOM_I] += wdi;
            m[ICPMI_GMOM_AA] += (long long)wda * da;
            m[ICPMI_GMOM_AJ] += (long long)wda * dj;
            m[ICPMI_GMOM_AI] += (long long)wda * di;
            m[ICPMI_GMOM_JJ] += (long long)wdj * dj;
            m[ICPMI_GMOM_JI] += (long long)wdj * di;
            m[ICPMI_GMOM_II] += (long long)wdi * di;
            m[ICPMI_GMOM_SUPPORT] += w > 0;
            m[ICPMI_GMOM_EDGE] += face ? w : 0;
        }
    }
#pragma unroll
    for (int s = 0; s < ICPMI_GMOM_INTS; ++s) {
        const long long v = wave_sum(m[s]);
        if (lane_id() == 0) part[wave_id()][s] = v;
    }
    __syncthreads();
    if (tid >= ICPMI_GMOM_INTS) return;
    long long v = part[0][tid];
#pragma unroll
    for (int w = 1; w < GM_WAVES; ++w) v += part[w][tid];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.moments + (size_t)b * ICPMI_GMOM_INTS + tid), (unsigned long long)v);
}

// ── host: the plan, the entry ────────────────────────────────────────────────
// What a call starts, decided as a whole and without a HIP call.  A pair's n candidates are cut into at most GMOM_MAX_CHUNKS
// chunks of whole steps; the sums are integers, so neither the cut nor the batch shows in a pair's moments.
// The two divisions of a flat index f < 2^22 by S2 < 2^12 and of its remainder r < 2^12 by S < 2^6 are multiply-shifts with
// M = floor(2^k / D) + 1: M D - 2^k = e in (0, D], and floor(x M / 2^k) = floor(x / D) as long as x e < 2^k — 2^22 * 2^12 <=
// 2^34 and 2^12 * 2^6 <= 2^18 (x below the first factor, e at most D below the second); r * M < 2^31 stays in 32 bits.
struct GmomPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    unsigned grid;            // (chunk, pair) workgroups
    int S, n, n_chunks, span;
    unsigned long long magic_a;
    unsigned magic_j;
    size_t moments_bytes;     // what is zeroed before the launch
};
static GmomPlan plan_grid_moments(int n_pairs, int n_angles, int window) {
    GmomPlan p{ICPMI_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n_pairs < 0 || n_angles < 1 || window < 0) { p.rc = ICPMI_ERR_ARG; return p; }
    if (window > ICPMI_GM_MAX_WINDOW || n_angles > ICPMI_GM_MAX_ANGLES) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.S = 2 * window + 1;
    const int S2 = p.S * p.S;
    p.n = n_angles * S2;
    const int steps = (p.n + GMOM_STEP - 1) / GMOM_STEP;
    p.n_chunks = steps < GMOM_MAX_CHUNKS ? steps : GMOM_MAX_CHUNKS;
    p.span = (steps + p.n_chunks - 1) / p.n_chunks * GMOM_STEP;
    p.n_chunks = (p.n + p.span - 1) / p.span;                     // no workgroup without a candidate
    const unsigned long long groups = (unsigned long long)n_pairs * p.n_chunks;
    if (groups >= (1ull << 31)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.grid = (unsigned)groups;
    p.magic_a = (1ull << GMOM_A_BITS) / (unsigned)S2 + 1;
    p.magic_j = (1u << GMOM_J_BITS) / (unsigned)p.S + 1;
    p.moments_bytes = (size_t)n_pairs * ICPMI_GMOM_INTS * sizeof(int64_t);
    return p;
}

}  // namespace icpmi

extern "C" int icpmi_grid_match_moments(const int32_t* volume, const int32_t* records, int32_t n_pairs, int32_t n_angles,
                                        int32_t window, int32_t half_step, int64_t* moments, void* stream) {
    using namespace icpmi;
    if (n_pairs == 0) return ICPMI_OK;
    if (!volume || !records || !moments || ((uintptr_t)moments & 7)) return ICPMI_ERR_ARG;
    if (half_step < 1 || half_step > ICPMI_GMOM_MAX_HALF_STEP) return ICPMI_ERR_ARG;
    const GmomPlan plan = plan_grid_moments(n_pairs, n_angles, window);
    if (plan.rc != ICPMI_OK) return plan.rc;
    const GmomArgs a{volume, records, (long long*)moments, n_angles, plan.S, plan.S * plan.S, plan.n, plan.n_chunks, plan.span,
                     half_step, plan.magic_a, plan.magic_j};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(moments, 0, plan.moments_bytes, st) != hipSuccess) return ICPMI_ERR_HIP;
    gm_moments_kernel<<<plan.grid, GM_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
