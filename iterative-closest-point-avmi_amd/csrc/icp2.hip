// icp2.hip — fused 2-D ICP on prepared (axis-sorted) targets: the fast path.
//
// Same loop as icp.hip (reference utilities/icp.py:153-223), same arithmetic and
// the same correspondences, but the nearest-neighbour step is the exact sweep
// of sweep.hpp over the target copy that prep.hip sorted along its best axis,
// and everything a pair needs lives on chip: the sorted target points, their
// normals and the sorted->row map in LDS (36 B per point), the moving source
// points and their matches in registers (up to 4 rows per thread).  One
// workgroup per pair, no traffic between workgroups, no host round trip.
//
// What bounds a pair is the instruction stream of its own workgroup (the tail of
// a batch is a few pairs that run to max_iterations, each alone on a CU), so
// work that is uniform across the workgroup is done by ONE wave: wave 0 combines
// the wave partials, tests convergence, solves the 3x3 system and publishes the
// step through LDS while the other waves wait at the barrier.  The squared
// error of a step is reduced together with the normal equations of the next
// one (one reduction per iteration for point_to_line); its convergence test
// therefore arrives one search late, and the totals it returns are the ones
// held back from before that search — the reference's results exactly.
//
// Pairs that do not fit (more than 4 rows per thread, target larger than the
// LDS copy, 3-D) run on the exhaustive kernel of icp.hip.
#include <cstdlib>

#include "linalg.hpp"
#include "prep_common.hpp"
#include "sweep.hpp"

namespace icpmi {


struct Icp2Args {
    const double* pts;
    const int32_t* off;
    const int32_t* cnt;
    const int32_t* pair_src;
    const int32_t* pair_tgt;
    const double* init;
    double* results;
    const double2* g_sxy;
    const double2* g_snrm;
    const int32_t* g_sorig;
    const float* g_skey;      // float32 images of the sort key (bearing order only)
    const int32_t* g_dir;
    int lds_points;           // capacity of the LDS copy (points)
    double error_threshold;
    double max_corr_dist;
    int max_iterations;
    int method;
    int has_init;
    int n_lo, m_lo;           // second launch: only the pairs whose source has more than n_lo rows or whose target more than m_lo
    int skip_over;            // first launch: leave pairs beyond THREADS x SMAX source rows or lds_points target rows to the second
    // Two-stage run of a large batch (launch_icp2): the first launch takes every pair up to it_limit iterations and
    // parks the ones still running (moving rows, matches, totals); the second continues exactly those, all started
    // together, instead of the last of them finishing alone at the end of one long launch.
    int it_begin, it_limit;   // iterations [it_begin, min(it_limit, max_iterations)) run here
    int resume;               // 1: the pairs are list[0 .. *list_count), their state comes from st_*
    double2* st_xy = nullptr; // [pair][st_stride]: moving source rows of a parked pair
    int32_t* st_pos = nullptr; //                   and the position of each row's match in the sorted target
    int32_t* list = nullptr;
    int32_t* list_count = nullptr;
    int st_stride = 0;
    int32_t* wide_list = nullptr;    // pairs the first launch leaves to the wider shape (when the caller gave a workspace): the second
    int32_t* wide_count = nullptr;   // launch walks this list instead of starting a workgroup per pair of the batch just to look
    // Pairs that start FAR from their target (a candidate whose pre-alignment is wrong: every row metres from the nearest
    // wall) walk most of the sorted target in every search.  A first launch that finds the mean squared error of step 0
    // (the convergence test of iteration 1 has it anyway) above far_d2 parks the pair after iteration 1 (same state as
    // above) on far_list, and icp2_far_kernel continues it with searches that give up long walks for a box hierarchy
    // (sweep.hpp).  Same matches, same arithmetic: the pair's result does not depend on which kernel finished it.
    int32_t* far_list = nullptr;     // nullptr: never
    int32_t* far_count = nullptr;
    double far_d2 = __builtin_inf(); // +inf: never
    // Stop after the first accepted candidate (icpmi_icp_batch_gated; gate.hint == nullptr: ungated).  The lead lane
    // reads the hint at the top of an iteration and the lead wave tests it where it decides CTRL_STOP; parked pairs test
    // it once before they stage anything; a pair's final record lowers it (common.hpp, IcpGate).
    IcpGate gate = {nullptr, nullptr, 0.0, 0, 1};
    // The far continuation (far_list above).  "Same arithmetic" includes the order of the sums over the rows: a thread adds
    // up its own rows, then the waves are added in order.  The continuation therefore gives a pair's rows to its threads as
    // the launch that parked the pair did: row n to thread n % far_row_threads (the threads beyond stay without rows) when
    // the pair was the first launch's (at most far_row_n source rows and far_row_m target rows), as its own shape does when
    // it was the wide launch's.  (Behind everything else: the other kernels' arguments stay where they were.)
    int far_row_threads = 0, far_row_n = 0, far_row_m = 0;
};
constexpr int ICP2_FAR_THREADS = 1024, ICP2_FAR_SMAX = 2, ICP2_FAR_POINTS = 2048;   // the continuation's shape: most source rows, target points
constexpr int ICP2_ST_PARKED = 100;     // internal status between the two stages

// ── workgroup sums of NV values per thread ───────────────────────────────────────────────────────────
// Per wave, a TRANSPOSING reduction: v_permlane32_swap exchanges the upper half of one register with the lower
// half of another, so one add halves the partials of TWO values at once ((a_lo, b_lo) + (a_hi, b_hi)); the
// 16-lane form (v_permlane16_swap: odd rows of one register against even rows of the other) does the same for
// the two resulting registers, which leaves four different values in the four 16-lane rows of one register, and
// the four DPP steps inside the rows then finish all four together: 5 instructions per value instead of the 12
// of a DPP tree per value, and ONE total per value and wave (not one per row).  The lead wave adds the totals of
// the waves in wave order.  Every tree is fixed: bitwise reproducible run to run.
__device__ __forceinline__ double swap_add(double a, double b, bool rows16) {
    const long long ab = __double_as_longlong(a), bb = __double_as_longlong(b);
    const unsigned alo = (unsigned)ab, ahi = (unsigned)(ab >> 32), blo = (unsigned)bb, bhi = (unsigned)(bb >> 32);
    unsigned xl, xh, yl, yh;
    if (rows16) {
        const auto r0 = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        xl = r0[0]; yl = r0[1]; xh = r1[0]; yh = r1[1];
    } else {
        const auto r0 = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        xl = r0[0]; yl = r0[1]; xh = r1[0]; yh = r1[1];
    }
    return __longlong_as_double(((long long)xh << 32) | xl) + __longlong_as_double(((long long)yh << 32) | yl);
}

constexpr int RED_MAXW = 16;                                   // waves per workgroup at most
template <int NV>
constexpr int red_doubles() { return (NV + 3) / 4 * 4 * RED_MAXW; }

// totals of this wave's NV values -> scratch[value * RED_MAXW + wave]
template <int NV>
__device__ __forceinline__ void wave_totals(double* scratch, const double (&v)[NV]) {
    constexpr int NP = (NV + 3) / 4 * 4;
    const int w = wave_id(), l = lane_id();
    double h[NP / 2];
#pragma unroll
    for (int j = 0; j < NP / 2; ++j)                           // lanes 0-31: value 2j, lanes 32-63: value 2j + 1
        h[j] = swap_add(2 * j < NV ? v[2 * j] : 0.0, 2 * j + 1 < NV ? v[2 * j + 1] : 0.0, false);
#pragma unroll
    for (int k = 0; k < NP / 4; ++k) {
        // rows 0..3 of q: values 4k, 4k + 2, 4k + 1, 4k + 3 (16 partials each)
        const double q = row_sum(swap_add(h[2 * k], h[2 * k + 1], true));
        const int row = l >> 4;
        const int idx = 4 * k + ((row & 1) << 1) + (row >> 1);
        // every lane of a row holds the row's total; the LAST lane stores it: with the store in lane 0 the second stage
        // (icp2_resume_kernel<768, 2, true, true>, at its 80-register cap) spills four registers in the lead wave's solve
        if ((l & 15) == 15 && idx < NV) scratch[idx * RED_MAXW + w] = q;
    }
}

// lead wave: v[i] = sum over the waves (in wave order) of scratch[i * RED_MAXW + wave], uniform in every lane
template <int NV>
__device__ __forceinline__ void combine_totals(const double* scratch, int n_waves, double (&v)[NV]) {
    const int l = lane_id();
    double s = 0.0;
    if (l < NV)
        for (int w = 0; w < n_waves; ++w) s += scratch[l * RED_MAXW + w];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = readlane_f64(s, i);
}

// control block published by wave 0: r (4), t (2), stop flag, mean_p (2), mean_q (2)
constexpr int CTRL_R = 0, CTRL_T = 4, CTRL_STOP = 6, CTRL_MP = 8, CTRL_MQ = 10;
// state carried from iteration to iteration by thread 0 alone (accumulated transform, errors, outcome): kept in LDS,
// not in registers — live across the search it would cost every thread of the workgroup 20 registers
constexpr int CTRL_RT = 12, CTRL_TT = 16, CTRL_ERR = 18, CTRL_PREV = 19, CTRL_DELTA = 20, CTRL_ITERS = 21, CTRL_STATUS = 22,
              CTRL_DOUBLES = 24;

#ifndef ICP2_STAGE1_ITERS
#define ICP2_STAGE1_ITERS 12    // iterations of the first stage of a large batch (launch_icp2)
#endif
#ifndef ICP2_PK_MIN
#define ICP2_PK_MIN 16          // searching lanes of a wave from which the packed walk is taken
#endif
#ifndef ICP2_PLAIN_ITERS
#define ICP2_PLAIN_ITERS 2      // iterations that search the plain nearest neighbour before budgets are kept
#endif
#ifndef ICP2_CENTRED_ITERS
#define ICP2_CENTRED_ITERS 2    // iterations whose top-two search starts at the row's own projection; later ones walk from the kept match
                                // (= ICP2_PLAIN_ITERS: none does; measured 5.22 / 5.13 ms at 3 / 2 for 16 384 pairs, 5.42 with 1 plain iteration)
#endif
#ifndef ICP2_PLAIN_CENTRED
#define ICP2_PLAIN_CENTRED ICP2_PLAIN_ITERS     // plain iterations that start at the row's own projection
#endif
// A value every lane of the wave holds alike, moved to scalar registers (it stays live across the whole search).
__device__ __forceinline__ double wave_uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ float wave_uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// far continuation: a searching row's query on its way to the lane that runs the search, and the answer on its way back
union FarSlot {
    struct { double x, y; int seed, pad; } in;
    struct { double s1, s3; int p1, p2; } out;
};
static_assert(sizeof(FarSlot) == 24, "24 B per row");

// ── the dynamic LDS of a launch, stated once: kernel, icp2_shape and plan_icp2 read it here ─────────────────────────
// sorted points | normals | row map (4 B per point) or, filter, float32 images (16 B per point, one padding entry at either end)
// | far: box hierarchy over blocks of 16 images (sweep.hpp; 2 B per point at most) | far: a FarSlot per row of the shape, each
// wave its own stretch.  Byte offsets, not pointers (a layout that holds pointers cost the prepare kernel 6 %).
struct Icp2Lds {
    size_t xy, nrm, orig, sq, tree, slots, bytes;
    __host__ __device__ constexpr Icp2Lds(int lds_points, bool filter, bool far = false, int far_rows = 0)
        : xy(0), nrm((size_t)lds_points * 16), orig((size_t)lds_points * 32), sq(orig + 16),
          tree(sq + (size_t)lds_points * 16 + 16), slots(tree + (size_t)lds_points * 2),
          bytes(far ? slots + sizeof(FarSlot) * (size_t)far_rows : (filter ? tree : orig + (size_t)lds_points * 4)) {}
};
constexpr bool icp2_lds_pinned(size_t c) {               // the layout this file has always had, at capacity c
    const Icp2Lds p((int)c, false), f((int)c, true), r((int)c, true, true, ICP2_FAR_THREADS * ICP2_FAR_SMAX);
    return p.bytes == c * 36 && f.bytes == c * 48 + 32 && r.bytes == c * 50 + 32 + 24 * 1024 * 2 && f.xy == 0 && f.nrm == c * 16 &&
           p.orig == c * 32 && f.sq == c * 32 + 16 && r.tree == c * 48 + 32 && r.slots == c * 50 + 32;
}
static_assert(icp2_lds_pinned(64) && icp2_lds_pinned(1536) && icp2_lds_pinned(2048) && icp2_lds_pinned(4096), "sizes and offsets of the areas");
// The error of a step (icp.py:215-220: mean squared error, its change, convergence), taken by the lead wave: every lane
// evaluates the same values, the writer lane stores.  `it`: the iterations the error belongs to.
__device__ __forceinline__ bool step_error(double* ctrl, double err_sum, int N, double error_threshold, int it, bool writer, double& err) {
    err = err_sum / (double)N;
    const double delta = fabs(ctrl[CTRL_PREV] - err);
    const bool stop = delta < error_threshold;
    if (writer) {
        ctrl[CTRL_ERR] = err; ctrl[CTRL_DELTA] = delta; ctrl[CTRL_PREV] = err; ctrl[CTRL_ITERS] = (double)it;
        if (stop) ctrl[CTRL_STATUS] = (double)ICPMI_ST_CONVERGED;
    }
    return stop;
}
// Finish step it-1 (step_error) and test the inlier count of step it (icp.py:186), in every lane of the lead wave: FIN_STOP
// when the pair is done, FIN_FAR when step 0 left a mean squared error above far_err (the pair goes to the far continuation
// after this iteration, launch_icp2), else FIN_GO.
constexpr int FIN_GO = 0, FIN_STOP = 1, FIN_FAR = 2;
__device__ __forceinline__ int finish_step(double* ctrl, int it, double err_sum, double inliers, int N, bool has_corr,
                                           int need, double error_threshold, bool writer, double far_err) {
    bool stop = false, far = false;
    if (it > 0) {
        double err;
        stop = step_error(ctrl, err_sum, N, error_threshold, it, writer, err);
        far = it == 1 && err > far_err;
    }
    if (!stop && has_corr && inliers < (double)need) {
        stop = true;
        if (writer) { ctrl[CTRL_STATUS] = (double)ICPMI_ST_FEW_INLIERS; ctrl[CTRL_ITERS] = (double)it; }
    }
    return stop ? FIN_STOP : (far ? FIN_FAR : FIN_GO);
}
// The gate (Icp2Args::gate), where the lead wave decides CTRL_STOP: a pair that goes on although a candidate before it
// has been accepted stops as SKIPPED instead — its record then holds the totals of the `it` iterations whose error
// finish_step has just taken.  gate_seen: what lane 0 loaded at the top of the iteration.
__device__ __forceinline__ int gate_stop(double* ctrl, const int32_t* hint, int gate_seen, int gate_index, bool writer, int fin) {
    if (fin == FIN_STOP || !hint || __builtin_amdgcn_readfirstlane(gate_seen) >= gate_index) return fin;
    if (writer) ctrl[CTRL_STATUS] = (double)ICPMI_ST_SKIPPED;
    return FIN_STOP;
}
// The writer lane publishes a step: into the totals (R_total = R R_total, t_total = t_total R^T + t: icp.py:210-211), out to the rows.
__device__ __forceinline__ void publish_step(double* ctrl, const double (&r)[4], const double (&t)[2]) {
    const double rt0 = ctrl[CTRL_RT], rt1 = ctrl[CTRL_RT + 1], rt2 = ctrl[CTRL_RT + 2], rt3 = ctrl[CTRL_RT + 3];
    const double tt0 = ctrl[CTRL_TT], tt1 = ctrl[CTRL_TT + 1];
    ctrl[CTRL_RT] = r[0] * rt0 + r[1] * rt2; ctrl[CTRL_RT + 1] = r[0] * rt1 + r[1] * rt3;
    ctrl[CTRL_RT + 2] = r[2] * rt0 + r[3] * rt2; ctrl[CTRL_RT + 3] = r[2] * rt1 + r[3] * rt3;
    ctrl[CTRL_TT] = (tt0 * r[0] + tt1 * r[1]) + t[0]; ctrl[CTRL_TT + 1] = (tt0 * r[2] + tt1 * r[3]) + t[1];
    ctrl[CTRL_R] = r[0]; ctrl[CTRL_R + 1] = r[1]; ctrl[CTRL_R + 2] = r[2]; ctrl[CTRL_R + 3] = r[3];
    ctrl[CTRL_T] = t[0]; ctrl[CTRL_T + 1] = t[1];
}
// Totals <-> result record (thread 0).  A parked pair's totals travel through its record.
__device__ __forceinline__ void load_totals(double* ctrl, const double* res) {
    ctrl[CTRL_RT] = res[0]; ctrl[CTRL_RT + 1] = res[1]; ctrl[CTRL_RT + 2] = res[2]; ctrl[CTRL_RT + 3] = res[3];
    ctrl[CTRL_TT] = res[ICPMI_RES_T]; ctrl[CTRL_TT + 1] = res[ICPMI_RES_T + 1];
    ctrl[CTRL_ERR] = res[ICPMI_RES_ERR]; ctrl[CTRL_PREV] = res[ICPMI_RES_ERR]; ctrl[CTRL_DELTA] = res[ICPMI_RES_DELTA]; ctrl[CTRL_ITERS] = res[ICPMI_RES_ITERS];
}
// ... and the final record of a pair; a finished, eligible, accepted pair lowers the gate (NaN: never)
__device__ __forceinline__ void store_record(double* res, const double* ctrl, const IcpGate& gate, int gate_index, int b) {
#pragma unroll
    for (int i = 0; i < ICPMI_RES_DOUBLES; ++i) res[i] = 0.0;
    res[0] = ctrl[CTRL_RT]; res[1] = ctrl[CTRL_RT + 1]; res[2] = ctrl[CTRL_RT + 2]; res[3] = ctrl[CTRL_RT + 3];
    res[ICPMI_RES_T] = ctrl[CTRL_TT]; res[ICPMI_RES_T + 1] = ctrl[CTRL_TT + 1];
    res[ICPMI_RES_ERR] = ctrl[CTRL_ERR]; res[ICPMI_RES_DELTA] = ctrl[CTRL_DELTA];
    res[ICPMI_RES_ITERS] = ctrl[CTRL_ITERS]; res[ICPMI_RES_STATUS] = ctrl[CTRL_STATUS];
    const double st = ctrl[CTRL_STATUS];
    if (gate.hint && st != (double)ICP2_ST_PARKED && st != (double)ICPMI_ST_SKIPPED && ctrl[CTRL_ERR] < gate.accept && gate_eligible(gate.search, b))
        atomicMin(gate.hint, gate_index);
}
// ── the rules of a row, each written once ────────────────────────────────────────────────────────────
// squared residual of a row at (x, y) against its match q: one term of the error of a step, icp.py:215
__device__ __forceinline__ double row_residual(const double2 q, double x, double y) {
    const double ex = q.x - x, ey = q.y - y;
    double se = 0.0;
    se += ex * ex; se += ey * ey;
    return se;
}
// squared distances of a row to its two kept candidates (positions pa, pb)
__device__ __forceinline__ void kept_pair_d2(const double2* sxy, double px, double py, int pa, int pb, double& q2, double& w2) {
    const double2 c = sxy[pa], e = sxy[pb];
    const double dx = px - c.x, dy = py - c.y;
    const double ex = px - e.x, ey = py - e.y;
    q2 = 0.0; w2 = 0.0;
    q2 += dx * dx; q2 += dy * dy;
    w2 += ex * ex; w2 += ey * ey;
}
// the correspondence gate, icp.py:184-185: nn_dists**2 < max_corr_dist**2 — the search's squared distance, bit for bit, squared again after its root
__device__ __forceinline__ bool within_gate(double dx, double dy, double max_corr_sq) {
    double s2 = 0.0;
    s2 += dx * dx; s2 += dy * dy;
    const double dist = sqrt(s2);
    return dist * dist < max_corr_sq;
}
// The movement budget a top-two search leaves its row (icp2_pair).
template <bool FAR>
__device__ __forceinline__ float budget_of(const Top2& t2, double px, double py) {
    float bf;
    if constexpr (FAR) {
        const double d1 = sqrt(t2.s1), d3 = sqrt(t2.s3);   // the far continuation keeps d3 itself (see the keep test) ...
        bf = (float)(d3 - 1e-13 * (d3 + d1) - 1.3e-7 * (fabs(px) + fabs(py)));   // ... minus the rounding of the single-precision anchor; rounded down
    } else {
        // (d3 - d1) / 2 minus the rounding of the single-precision anchor, from float32 roots rounded the safe way —
        // d3 down, d1 up (conversion 2^-24, v_sqrt_f32 one ulp: 1.2e-7 in all, 3e-7 taken) —: two float64 roots were a
        // tenth of a top-two search; the budget only has to be a lower bound (round 4)
        const float r3 = __builtin_amdgcn_sqrtf((float)t2.s3) * 0.9999997f;
        const float r1 = __builtin_amdgcn_sqrtf((float)t2.s1) * 1.0000003f + 1e-30f;
        bf = (r3 - r1) * 0.4999999f - 1.3e-7f * (fabsf((float)px) + fabsf((float)py));
    }
    bf = bf - fabsf(bf) * 1e-6f;
    return t2.s3 < __builtin_inf() ? bf : __builtin_inff();
}

// THREADS x ICP2_SMAX = most source rows a pair may have on this instantiation
// TGT_LDS: the prepared target is staged in LDS (<= 4096 points); otherwise it is read in place, through L2
// FILT (with TGT_LDS): the LDS copy carries a float32 image per point instead of the row map (48 B instead of
// 36 B per point) and the searches judge every candidate on it first (sweep.hpp, "single-precision filter")
template <int THREADS, int ICP2_SMAX, bool TGT_LDS, bool FILT, bool RESUME, bool FAR = false>
__device__ __forceinline__ void icp2_pair(const Icp2Args& a, const int b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ double redA[red_doubles<11>()];         // normal equations (10) / centroid sums (5) + carried squared error
    __shared__ double redB[red_doubles<4>()];          // cross-covariance
    __shared__ double ctrl[CTRL_DOUBLES];
    constexpr int NWAVES = THREADS / ICPMI_WAVE;

    const int tid = threadIdx.x;
    const bool lead = tid < ICPMI_WAVE;                      // wave 0 carries the uniform state
    const int sc = a.pair_src[b], tc = a.pair_tgt[b];
    const int N = a.cnt ? a.cnt[sc] : a.off[sc + 1] - a.off[sc];
    const int M = a.cnt ? a.cnt[tc] : a.off[tc + 1] - a.off[tc];
    const double* src = a.pts + (size_t)a.off[sc] * 2;
    double* res = a.results + (size_t)b * ICPMI_RES_DOUBLES;
    const int dir = a.g_dir[tc];
    // RT: threads that hold rows, row n = s * RT + tid (the far continuation: as in the launch that parked the pair, Icp2Args)
    const int RT = FAR && N <= a.far_row_n && M <= a.far_row_m ? a.far_row_threads : THREADS;
    const bool row_lane = !FAR || tid < RT;
    // The voxel filter leaves the row counts on the device, so the launcher sizes the rows per thread for the usual
    // case and sends the (rare) larger clouds to a second launch of a wider shape: each pair is registered by
    // exactly one of the two (uniform per workgroup, before any barrier).
    if (a.skip_over ? (N > THREADS * ICP2_SMAX || (TGT_LDS && M > a.lds_points)) : (a.n_lo >= 0 && N <= a.n_lo && M <= a.m_lo)) {
        if (a.skip_over && a.wide_list && threadIdx.x == 0) a.wide_list[atomicAdd(a.wide_count, 1)] = b;
        return;
    }
    const int gate_index = a.gate.base + b * a.gate.stride;
    if (RESUME && a.gate.hint) {
        // a parked pair tests the gate once, before it stages anything: skipped, its record keeps the totals the first
        // stage left there (one step more than the iterations whose error it holds)
        __shared__ int gate_skip;
        if (tid == 0) {
            gate_skip = __hip_atomic_load(a.gate.hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gate_index;
            if (gate_skip) {
                res[ICPMI_RES_ITERS] += 1.0;
                res[ICPMI_RES_STATUS] = (double)ICPMI_ST_SKIPPED;
            }
        }
        __syncthreads();
        if (gate_skip) return;
    }
    // two instantiations, each sees ONE address space behind these pointers
    const Icp2Lds lds(a.lds_points, FILT, FAR, THREADS * ICP2_SMAX);
    double2* lds_xy = reinterpret_cast<double2*>(dyn + lds.xy);
    double2* lds_nrm = reinterpret_cast<double2*>(dyn + lds.nrm);
    int32_t* lds_orig = reinterpret_cast<int32_t*>(dyn + lds.orig);    // !FILT: row map
    float4* lds_sq = reinterpret_cast<float4*>(dyn + lds.sq);          //  FILT: float32 images
    // (no block boxes here: the far scan of sweep.hpp costs this kernel 11 registers — spills at six waves per SIMD — and
    // 35 % of its time on pairs that start close, to halve the time of pairs that start metres away; measured, round 3)
    const double2* sxy = TGT_LDS ? lds_xy : a.g_sxy + a.off[tc];
    const double2* snrm = TGT_LDS ? lds_nrm : a.g_snrm + a.off[tc];
    const int32_t* sorig = TGT_LDS ? lds_orig : a.g_sorig + a.off[tc];
    static_assert(TGT_LDS || !FILT, "the filter images live in LDS");
    static_assert(!FAR || (FILT && RESUME), "the far continuation: filter images, parked state");
    float4* lds_tree = reinterpret_cast<float4*>(dyn + lds.tree);      // FAR: box hierarchy over blocks of 16 images (sweep.hpp) ...
    const int tree_leaves = sweepf_tree_leaves(M);                     // ... and ICP2_SMAX slots per lane, each wave its own stretch
    FarSlot* far_q = reinterpret_cast<FarSlot*>(dyn + lds.slots) + (size_t)(threadIdx.x / ICPMI_WAVE) * (ICPMI_WAVE * ICP2_SMAX);
    __shared__ int rt_bits;                                      // max(|x - ox|, |y - oy|) over the target, float32 bits
    if (FILT && tid == 0) rt_bits = 0;
    if (tid == 0) {
        if (RESUME) load_totals(ctrl, res);                 // the totals the first stage left in the result record
        else {                                              // a fresh pair: identity or the caller's initial guess (icp.py:153-156)
            const double* in = a.init + (size_t)b * 6;
            ctrl[CTRL_RT] = a.has_init ? in[0] : 1.0; ctrl[CTRL_RT + 1] = a.has_init ? in[1] : 0.0;
            ctrl[CTRL_RT + 2] = a.has_init ? in[2] : 0.0; ctrl[CTRL_RT + 3] = a.has_init ? in[3] : 1.0;
            ctrl[CTRL_TT] = a.has_init ? in[4] : 0.0; ctrl[CTRL_TT + 1] = a.has_init ? in[5] : 0.0;
            ctrl[CTRL_ERR] = __builtin_inf(); ctrl[CTRL_PREV] = __builtin_inf(); ctrl[CTRL_DELTA] = __builtin_inf(); ctrl[CTRL_ITERS] = 0.0;
        }
        ctrl[CTRL_STATUS] = (double)ICPMI_ST_MAXITER;
    }

    if (N <= 0 || M <= 0 || dir < 0 || (TGT_LDS && M > a.lds_points) || N > RT * ICP2_SMAX || (!FILT && dir >= SWEEP_POLAR)) {
        if (tid == 0) ctrl[CTRL_STATUS] = (double)ICPMI_ST_EMPTY;   // the launcher only sends pairs that fit
    } else {
        const bool use_p2l = a.method == ICPMI_POINT_TO_LINE;
        // stage the prepared target: coalesced 16-B reads
        const double2* gx = a.g_sxy + a.off[tc];
        const double2* gn = a.g_snrm + a.off[tc];
        const int32_t* go = a.g_sorig + a.off[tc];
        const float* gk = a.g_skey + a.off[tc];
        SweepF filt{0.0, 0.0, 0.0, 0.0f, 0.0f};
        if constexpr (TGT_LDS && !FILT)
            for (int i = tid; i < M; i += THREADS) {
                lds_xy[i] = gx[i];
                lds_orig[i] = go[i];
                if (use_p2l) lds_nrm[i] = gn[i];
            }
        if constexpr (FILT) {
            // float32 images: relative to the point in the middle of the sort order (small magnitudes), or — bearing
            // order — to the frame origin the bearings are taken about
            if (dir != SWEEP_POLAR) {
                const double2 o = gx[M >> 1];
                filt.ox = wave_uniform(o.x); filt.oy = wave_uniform(o.y); filt.uo = wave_uniform(proj(dir, o.x, o.y));
            }
            float rmax = 0.0f;
            for (int i = tid; i < M; i += THREADS) {
                const double2 p = gx[i];
                lds_xy[i] = p;
                if (use_p2l) lds_nrm[i] = gn[i];
                const float4 q = make_float4((float)(p.x - filt.ox), (float)(p.y - filt.oy),
                                             dir == SWEEP_POLAR ? gk[i] : (float)(proj(dir, p.x, p.y) - filt.uo),
                                             __int_as_float(go[i]));
                lds_sq[i] = q;
                rmax = fmaxf(rmax, fmaxf(fabsf(q.x), fabsf(q.y)));
            }
            if (tid == 0) { lds_sq[-1] = make_float4(0.f, 0.f, 0.f, 0.f); lds_sq[M] = make_float4(0.f, 0.f, 0.f, 0.f); }
            __syncthreads();                                     // rt_bits = 0 is visible, the images are complete
            rmax = wave_max(rmax);                               // one atomic per wave, not one per thread, on the one word
            if (lane_id() == 0) atomicMax(&rt_bits, __float_as_int(rmax));      // non-negative floats order like their bits
        }
        // moving source rows in registers: row n = s*RT + tid
        double px[ICP2_SMAX], py[ICP2_SMAX];
        int pos[ICP2_SMAX];
        // Movement budget of each row's match.  A search returns the two nearest
        // target points and the distance d3 of the third.  While the row is
        // displaced from where it was searched (the anchor) by less than
        // (d3 - d1)/2, every other target point is still farther than the nearer
        // of those two (triangle inequality), so the match is the better of the
        // two — two distance evaluations instead of a search.  Exact: margins cover
        // rounding, equal distances fall back on the row rule or on a new search.
        // Net displacement, so a pair that oscillates in a limit cycle (the usual
        // reason for running to max_iterations) stops searching too.
        // Anchor and budget are kept in SINGLE precision (registers: four rows per
        // thread must not spill): the budget is lowered by the rounding of the
        // anchor (2^-24 of each coordinate) and rounded down, so the test stays
        // conservative — it can only send a row to a search it did not need.
        float ax[ICP2_SMAX], ay[ICP2_SMAX], budget[ICP2_SMAX];
        int pos2[ICP2_SMAX];
#pragma unroll
        for (int s = 0; s < ICP2_SMAX; ++s) { ax[s] = 0.0f; ay[s] = 0.0f; budget[s] = -1.0f; pos2[s] = -1; }
        const int S = row_lane ? (N + RT - 1) / RT : 0;
#pragma unroll
        for (int s = 0; s < ICP2_SMAX; ++s) {
            const int n = row_lane ? s * RT + tid : N;
            px[s] = 0.0; py[s] = 0.0; pos[s] = -1;                       // -1: no previous match yet
            if (n < N && RESUME) {
                const double2 v = a.st_xy[(size_t)b * a.st_stride + n];
                px[s] = v.x; py[s] = v.y; pos[s] = a.st_pos[(size_t)b * a.st_stride + n];
            } else if (n < N) {
                const double x = src[2 * n], y = src[2 * n + 1];
                if (a.has_init) {                           // source @ R_init.T + t_init
                    const double* in = a.init + (size_t)b * 6;
                    double sx = 0.0, sy = 0.0;
                    sx += x * in[0]; sx += y * in[1]; sx += in[4];
                    sy += x * in[2]; sy += y * in[3]; sy += in[5];
                    px[s] = sx; py[s] = sy;
                } else { px[s] = x; py[s] = y; }
            }
        }
        const bool has_corr = a.max_corr_dist >= 0.0;
        const double max_corr_sq = wave_uniform(a.max_corr_dist * a.max_corr_dist);   // icp.py:169
        const int need = max(3, N / 10);                                 // icp.py:186
        __syncthreads();
        if constexpr (FAR) {
            sweepf_build_tree(lds_sq, M, lds_tree, tree_leaves, tid, THREADS);
            __syncthreads();
        }
        // largest |projection| of the target (the copy is sorted along it): rounding slack of the diagonal axes
        const double2 c_lo = sxy[0], c_hi = sxy[M - 1];
        const double uabs = wave_uniform(fmax(fabs(proj(dir, c_lo.x, c_lo.y)), fabs(proj(dir, c_hi.x, c_hi.y))));
        if constexpr (FILT) {
            filt.rt = wave_uniform(__int_as_float(rt_bits) * 1.000001f);
            filt.ut = wave_uniform(fmaxf(fabsf(lds_sq[0].z), fabsf(lds_sq[M - 1].z)) * 1.000001f);     // the images are sorted like the keys
        }

        double e_part = 0.0;          // this thread's share of the squared error of the step just applied
        if (RESUME) {
            // the squared residual of the last step of the first stage against the matches it used: the sums of the
            // apply loop below, term by term
#pragma unroll
            for (int s = 0; s < ICP2_SMAX; ++s) {
                if (!(s < S && s * RT + tid < N)) continue;
                e_part += row_residual(sxy[pos[s]], px[s], py[s]);
            }
        }
        bool stopped = false;
        // a first launch hands a pair whose FIRST step leaves a mean squared error above far_d2 to the far continuation, which
        // runs iterations 2 .. max_iterations - 1 (the test rides on the convergence test of iteration 1: no arithmetic of its own)
        const double far_err = !RESUME && a.max_iterations > 2 && N <= ICP2_FAR_THREADS * ICP2_FAR_SMAX && M <= ICP2_FAR_POINTS
                                   ? a.far_d2 : __builtin_inf();
        const int it_end = RESUME ? a.max_iterations : min(a.max_iterations, a.it_limit);
        for (int it = RESUME ? a.it_begin : 0; it < it_end; ++it) {
            // the gate, loaded by one lane now and tested after the search (gate_stop): a cross-XCD load is a large part
            // of a tail iteration; agent scope, so that no stale copy in this CU's L1 hides a lower value
            int gate_seen = 0x7fffffff;
            if (a.gate.hint && tid == 0) gate_seen = __hip_atomic_load(a.gate.hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ── correspondences: exact sweep search in LDS, icp.py:179 ───────
            // (This phase, the searches and the apply loop as named local lambdas, with a row_valid lambda for the row test below, leave
            // every kernel's registers, scratch and occupancy as they are and cost time all the same: 16 384 pairs 4.624 -> 4.651 ms, 512
            // pairs 0.637 -> 0.651, step 7.298 -> 7.336, each outside the parent's spread.  row_valid as a function: 4 B of scratch in one kernel.)
            // A row whose net displacement since its last search is inside its budget keeps one of its two candidates; the others search.
            bool srch[ICP2_SMAX];
#pragma unroll
            for (int s = 0; s < ICP2_SMAX; ++s) {
                const bool valid = s < S && s * RT + tid < N;
                // |dx| + |dy| >= the distance between the row and its anchor
                // (Tried in round 3: testing delta + dq < d3 with the CURRENT distance dq to the better kept candidate — about
                // twice as generous, 0.7 % instead of 2 % of the rows of a limit cycle search — costs 8 registers (a spill at
                // six waves per SIMD) and the distances of the rows that then search after all: no faster, 5.11 against 5.07 ms.)
                bool within;
                if constexpr (FAR) {
                    // The far continuation (a search costs ten times the usual) keeps d3 itself — lowered by the same
                    // margins — instead of the budget, and tests with the row's CURRENT distance dq to the better of its
                    // two candidates: every other target point was at least d3 from the anchor, so it is at least
                    // d3 - delta from the row now; dq < d3 - delta keeps the match.  About twice as generous as
                    // delta < (d3 - d1) / 2; both distances are evaluated for every row (they are cheap here).
                    within = false;
                    if (valid && budget[s] > 0.0f) {
                        const int pa = pos[s], pb = pos2[s] >= 0 ? pos2[s] : pos[s];
                        double q2, w2;
                        kept_pair_d2(sxy, px[s], py[s], pa, pb, q2, w2);
                        const double g = (double)budget[s] - (fabs(px[s] - (double)ax[s]) + fabs(py[s] - (double)ay[s])) * 1.000000001;
                        within = g > 0.0 && fmin(q2, w2) * 1.000000000001 < g * g * 0.999999999999;
                    }
                } else {
                    within = valid && (fabs(px[s] - (double)ax[s]) + fabs(py[s] - (double)ay[s])) * 1.000000001 < (double)budget[s];
                }
                srch[s] = valid && !within;
                if (within) {
                    // straight-line: a missing second candidate stands in as the first (never better), and only an
                    // exact tie of the two distances takes a branch (to compare the rows)
                    const int pa = pos[s], pb = pos2[s] >= 0 ? pos2[s] : pos[s];
                    double q2, w2;
                    kept_pair_d2(sxy, px[s], py[s], pa, pb, q2, w2);
                    bool second_wins = w2 < q2;
                    if (w2 == q2 && pb != pa) {
                        if constexpr (FILT) second_wins = sweepf_row(lds_sq[pb]) < sweepf_row(lds_sq[pa]);
                        else second_wins = sorig[pb] < sorig[pa];
                    }
                    pos[s] = second_wins ? pb : pa;
                    pos2[s] = pos2[s] >= 0 ? (second_wins ? pa : pb) : -1;
                }
            }
            // (a continuation starts at iteration STAGE1_ITERATIONS > ICP2_PLAIN_ITERS: its instantiation holds the top-two search only)
            if (!RESUME && it < ICP2_PLAIN_ITERS) {
                // the first steps move every row by more than any budget: plain 1-NN (smallest window), started at
                // the row's own projection — the previous match only seeds the bound (it lies a whole step away)
#pragma unroll
                for (int s = 0; s < ICP2_SMAX; ++s)
                    if (srch[s]) {
                        double d2s;
                        if constexpr (FILT) {
                            if (__popcll(__ballot(true)) >= ICP2_PK_MIN)
                                pos[s] = sweepf_nn_pk(lds_sq, sxy, filt, M, dir, uabs, px[s], py[s], pos[s], it < ICP2_PLAIN_CENTRED);
                            else pos[s] = sweepf_nn(lds_sq, sxy, filt, M, dir, uabs, px[s], py[s], pos[s], it < ICP2_PLAIN_CENTRED, d2s);
                        }
                        else pos[s] = sweep_nn(sxy, sorig, M, dir, uabs, px[s], py[s], pos[s], it < ICP2_PLAIN_CENTRED, d2s);
                    }
            } else {
                const bool centred = !RESUME && it < ICP2_CENTRED_ITERS;
                // The far continuation packs the searching rows of a wave: a far search costs thousands of instructions and
                // a wave pays for one per row slot in which ANY lane searches — with a quarter of the rows searching, both
                // slots, at a quarter of the lanes.  The queries of all slots go through the wave's stretch of LDS to the
                // low lanes (a slot's rows stay neighbours there) and the answers come back the same way: one round of
                // searches per 64 searching rows.  Wave-private: no barrier, LDS operations of a wave complete in order.
                int slot[ICP2_SMAX];
                if constexpr (FAR) {
                    int nq = 0;
#pragma unroll
                    for (int s = 0; s < ICP2_SMAX; ++s) {
                        const unsigned long long bal = __ballot(srch[s]);
                        slot[s] = nq + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                        nq += __popcll(bal);
                        if (srch[s]) {
                            FarSlot e;
                            e.in.x = px[s]; e.in.y = py[s]; e.in.seed = pos[s]; e.in.pad = 0;
                            far_q[slot[s]] = e;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    for (int j = tid & (ICPMI_WAVE - 1); j < nq; j += ICPMI_WAVE) {
                        const FarSlot e = far_q[j];
                        const Top2 r = sweepf_top2_far(lds_sq, sxy, lds_tree, tree_leaves, filt, M, dir, uabs, e.in.x, e.in.y, e.in.seed);
                        FarSlot o;
                        o.out.s1 = r.s1; o.out.s3 = r.s3; o.out.p1 = r.p1; o.out.p2 = r.p2;
                        far_q[j] = o;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
#pragma unroll
                for (int s = 0; s < ICP2_SMAX; ++s)
                    if (srch[s]) {
                        Top2 t2;
                        // (Tried first: ONE queue for the whole workgroup, worked off by its lanes in order — 7.8 against 6.4 ms
                        // on the 3 m / 20 degree candidates: the lanes of a wave then hold rows from all over the scan and
                        // their descents diverge; two barriers more per iteration.)
                        if constexpr (FAR) {
                            const FarSlot o = far_q[slot[s]];
                            t2.p1 = o.out.p1; t2.p2 = o.out.p2; t2.s1 = o.out.s1; t2.s2 = o.out.s1; t2.s3 = o.out.s3;
                        }
                        else if constexpr (FILT) {
                            // the packed walk costs a wave the same whether one lane searches or all do; the branching walk
                            // is cheap while few do (its exact path is then rarely entered): chosen per wave by the count
                            if (__popcll(__ballot(true)) >= ICP2_PK_MIN)
                                t2 = sweepf_top2_pk(lds_sq, sxy, filt, M, dir, uabs, px[s], py[s], pos[s], centred);
                            else t2 = sweepf_top2(lds_sq, sxy, filt, M, dir, uabs, px[s], py[s], pos[s], centred);
                        }
                        else t2 = sweep_top2(sxy, sorig, M, dir, uabs, px[s], py[s], pos[s], centred);
                        pos[s] = t2.p1; pos2[s] = t2.p2;
                        budget[s] = budget_of<FAR>(t2, px[s], py[s]);
                        ax[s] = (float)px[s]; ay[s] = (float)py[s];
                    }
            }
            // rows that take part in the solve: all valid rows, or those within max_corr_dist of their match (within_gate)
            bool in[ICP2_SMAX];
#pragma unroll
            for (int s = 0; s < ICP2_SMAX; ++s) in[s] = s < S && s * RT + tid < N;
            if (use_p2l) {
                // ── point-to-line normal equations, icp.py:88-104, + carried error ─
                double acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < ICP2_SMAX; ++s) {
                    if (!in[s]) continue;
                    const double2 q = sxy[pos[s]], nm = snrm[pos[s]];
                    const double dx = px[s] - q.x, dy = py[s] - q.y;
                    if (has_corr && !within_gate(dx, dy, max_corr_sq)) continue;
                    const double c = nm.y * px[s] - nm.x * py[s];
                    const double bi = -(nm.x * dx + nm.y * dy);
                    acc[0] += c * c;       acc[1] += c * nm.x;    acc[2] += c * nm.y;
                    acc[3] += nm.x * nm.x; acc[4] += nm.x * nm.y; acc[5] += nm.y * nm.y;
                    acc[6] += c * bi;      acc[7] += nm.x * bi;   acc[8] += nm.y * bi;
                    acc[9] += 1.0;
                }
                acc[10] = e_part;
                wave_totals<11>(redA, acc);
                __syncthreads();
                if (lead) {
                    combine_totals<11>(redA, NWAVES, acc);
                    const int fin = gate_stop(ctrl, a.gate.hint, gate_seen, gate_index, tid == 0,
                                              finish_step(ctrl, it, acc[10], acc[9], N, has_corr, need, a.error_threshold, tid == 0, far_err));
                    const bool stop = fin == FIN_STOP;
                    if (!stop) {
                        double A[3][3] = {{acc[0], acc[1], acc[2]}, {acc[1], acc[3], acc[4]}, {acc[2], acc[4], acc[5]}};
                        // (Written out: through linalg.hpp's p2l_step_from_solution, or with this solve as a phase of its own, the code
                        // of all 49 kernels moves — 4-6 VGPRs fewer, 16 384 pairs 4.61 -> 4.67 ms, 512 pairs 0.636 -> 0.660.)
                        double rhs[3] = {acc[6], acc[7], acc[8]}, x[3], r[4], t[2];
                        if (solve3(A, rhs, x)) {
                            double st, ct;
                            sincos_step(x[0], st, ct);                             // icp.py:110-114
                            r[0] = ct; r[1] = -st; r[2] = st; r[3] = ct; t[0] = x[1]; t[1] = x[2];
                        } else {
                            r[0] = 1.0; r[1] = 0.0; r[2] = 0.0; r[3] = 1.0; t[0] = 0.0; t[1] = 0.0;
                        }
                        if (tid == 0) publish_step(ctrl, r, t);                    // accumulate totals, icp.py:210-211
                    }
                    if (tid == 0) ctrl[CTRL_STOP] = (double)fin;
                }
                __syncthreads();
            } else {
                // ── point-to-point: centroids (+ carried error), icp.py:197-198 ──
                double m[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < ICP2_SMAX; ++s) {
                    if (!in[s]) continue;
                    const double2 q = sxy[pos[s]];
                    if (has_corr) {
                        in[s] = within_gate(px[s] - q.x, py[s] - q.y, max_corr_sq);
                        if (!in[s]) continue;
                    }
                    m[0] += px[s]; m[1] += py[s]; m[2] += q.x; m[3] += q.y; m[4] += 1.0;
                }
                m[5] = e_part;
                wave_totals<6>(redA, m);
                __syncthreads();
                if (lead) {
                    combine_totals<6>(redA, NWAVES, m);
                    const int fin = gate_stop(ctrl, a.gate.hint, gate_seen, gate_index, tid == 0,
                                              finish_step(ctrl, it, m[5], m[4], N, has_corr, need, a.error_threshold, tid == 0, far_err));
                    if (tid == 0) {
                        ctrl[CTRL_STOP] = (double)fin;
                        ctrl[CTRL_MP] = m[0] / m[4]; ctrl[CTRL_MP + 1] = m[1] / m[4];
                        ctrl[CTRL_MQ] = m[2] / m[4]; ctrl[CTRL_MQ + 1] = m[3] / m[4];
                    }
                }
                __syncthreads();
                if (ctrl[CTRL_STOP] == (double)FIN_STOP) { stopped = true; break; }
                const double mpx = ctrl[CTRL_MP], mpy = ctrl[CTRL_MP + 1], mqx = ctrl[CTRL_MQ], mqy = ctrl[CTRL_MQ + 1];
                // centred cross-covariance, icp.py:199-201
                double W[4] = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < ICP2_SMAX; ++s) {
                    if (!in[s]) continue;
                    const double2 q = sxy[pos[s]];
                    const double pcx = px[s] - mpx, pcy = py[s] - mpy, qcx = q.x - mqx, qcy = q.y - mqy;
                    W[0] += pcx * qcx; W[1] += pcx * qcy; W[2] += pcy * qcx; W[3] += pcy * qcy;
                }
                wave_totals<4>(redB, W);
                __syncthreads();
                if (lead) {
                    combine_totals<4>(redB, NWAVES, W);
                    double r[4], t[2];
                    kabsch2(W, r);                                                 // icp.py:202-206
                    double s0 = 0.0, s1 = 0.0;
                    s0 += r[0] * mpx; s0 += r[1] * mpy;
                    s1 += r[2] * mpx; s1 += r[3] * mpy;
                    t[0] = mqx - s0; t[1] = mqy - s1;                              // icp.py:207
                    if (tid == 0) publish_step(ctrl, r, t);
                }
                __syncthreads();
            }
            if (ctrl[CTRL_STOP] == (double)FIN_STOP) { stopped = true; break; }
            // ── apply to ALL rows; squared residual against this search's matches, icp.py:212-215 ─
            const double r0 = ctrl[CTRL_R], r1 = ctrl[CTRL_R + 1], r2 = ctrl[CTRL_R + 2], r3 = ctrl[CTRL_R + 3];
            const double t0 = ctrl[CTRL_T], t1 = ctrl[CTRL_T + 1];
            e_part = 0.0;
#pragma unroll
            for (int s = 0; s < ICP2_SMAX; ++s) {
                if (!(s < S && s * RT + tid < N)) continue;
                const double2 q = sxy[pos[s]];
                double nx = 0.0, ny = 0.0;
                nx += px[s] * r0; nx += py[s] * r1; nx += t0;
                ny += px[s] * r2; ny += py[s] * r3; ny += t1;
                px[s] = nx; py[s] = ny;
                e_part += row_residual(q, nx, ny);
            }
            if (!RESUME && it == 1 && ctrl[CTRL_STOP] == (double)FIN_FAR) break;
        }
        const bool far_parked = !RESUME && !stopped && ctrl[CTRL_STOP] == (double)FIN_FAR;      // left after iteration 1
        if (!RESUME && !stopped && (far_parked || it_end < a.max_iterations)) {
            // parked for the second stage: rows and matches as they are, totals through the result record
#pragma unroll
            for (int s = 0; s < ICP2_SMAX; ++s) {
                const int n = s * RT + tid;
                if (s < S && n < N) {
                    a.st_xy[(size_t)b * a.st_stride + n] = make_double2(px[s], py[s]);
                    a.st_pos[(size_t)b * a.st_stride + n] = pos[s];
                }
            }
            if (tid == 0) {
                ctrl[CTRL_STATUS] = (double)ICP2_ST_PARKED;
                if (far_parked) a.far_list[atomicAdd(a.far_count, 1)] = b;
                else a.list[atomicAdd(a.list_count, 1)] = b;
            }
        } else if (!stopped && a.max_iterations > 0) {
            // the last step's error has not been reduced yet: icp.py:215-223 for it = max_iterations - 1
            double e[1] = {e_part};
            __syncthreads();                      // redA may still be read by the lead wave of the last iteration
            wave_totals<1>(redA, e);
            __syncthreads();
            if (lead) {
                combine_totals<1>(redA, NWAVES, e);
                double err;
                if (tid == 0) step_error(ctrl, e[0], N, a.error_threshold, a.max_iterations, true, err);
            }
        }
    }
    if (tid == 0) store_record(res, ctrl, a.gate, gate_index, b);
}

template <int THREADS, int ICP2_SMAX, bool TGT_LDS, bool FILT>
__global__ __launch_bounds__(THREADS, THREADS == 768 ? 6 : 4) void icp2_fused_kernel(Icp2Args a) {   // 4 waves/SIMD: 2 x 512 or 1 x 1024 per CU; 6: 2 x 768
    icp2_pair<THREADS, ICP2_SMAX, TGT_LDS, FILT, false>(a, blockIdx.x);                              // one pair per workgroup
}

// the launch for wide clouds when the first one listed them: the workgroups walk that list
template <int THREADS, int ICP2_SMAX, bool TGT_LDS, bool FILT>
__global__ __launch_bounds__(THREADS, THREADS == 768 ? 6 : 4) void icp2_wide_kernel(Icp2Args a) {
    const int count = *a.wide_count;
    for (int j = blockIdx.x; j < count; j += gridDim.x) {
        icp2_pair<THREADS, ICP2_SMAX, TGT_LDS, FILT, false>(a, __builtin_amdgcn_readfirstlane(a.wide_list[j]));
        __syncthreads();                                    // LDS is staged again for the next pair
    }
}

// second stage of a two-stage run: workgroup j continues the j-th parked pair.  No loop over the list here: with one the
// 768 x 2 shape needs 93 registers instead of 79 and spills 56 B per lane at its budget of 80 (six waves per SIMD); the
// launcher starts an eighth of the batch's pairs as workgroups (about one pair in twelve is parked; a workgroup beyond the
// list leaves at once) and ...
template <int THREADS, int ICP2_SMAX, bool TGT_LDS, bool FILT>
__global__ __launch_bounds__(THREADS, THREADS == 768 ? 6 : 4) void icp2_resume_kernel(Icp2Args a) {
    if ((int)blockIdx.x >= *a.list_count) return;
    icp2_pair<THREADS, ICP2_SMAX, TGT_LDS, FILT, true>(a, __builtin_amdgcn_readfirstlane(a.list[blockIdx.x]));
}

// ... the parked pairs beyond that (none, usually) are walked by the few workgroups of this one
template <int THREADS, int ICP2_SMAX, bool TGT_LDS, bool FILT>
__global__ __launch_bounds__(THREADS, THREADS == 768 ? 6 : 4) void icp2_resume_rest_kernel(Icp2Args a, int first) {
    const int count = *a.list_count;
    for (int j = first + blockIdx.x; j < count; j += gridDim.x) {
        // the pair index in a scalar register: everything addressed through it stays scalar
        icp2_pair<THREADS, ICP2_SMAX, TGT_LDS, FILT, true>(a, __builtin_amdgcn_readfirstlane(a.list[j]));
        __syncthreads();                                    // LDS is staged again for the next pair
    }
}

// continuation of the pairs found far from their target (Icp2Args::far_list): one shape for all of them
__global__ __launch_bounds__(ICP2_FAR_THREADS, 4) void icp2_far_kernel(Icp2Args a) {
    const int count = *a.far_count;
    for (int j = blockIdx.x; j < count; j += gridDim.x) {
        icp2_pair<ICP2_FAR_THREADS, ICP2_FAR_SMAX, true, true, true, true>(a, __builtin_amdgcn_readfirstlane(a.far_list[j]));
        __syncthreads();                                    // LDS is staged again for the next pair
    }
}

// The parked state of the stages (see Icp2Args), in the caller's workspace: transformed rows | sweep positions (max_src_n of
// each per pair) | the three lists of pairs (second stage, wide, far) | their three counters, no gap between them.
struct Icp2Ws {                 // (tests/test_icp2_layout_gpu.py and tests/stream_cases.py read the counters at their offset here: keep them together)
    Carve c;
    int n_pairs, max_src_n;
    size_t st_rows = (size_t)n_pairs * (size_t)max_src_n;
    double2* st_xy = c.packed<double2>(st_rows * 16);
    int32_t* st_pos = c.packed<int32_t>(st_rows * 4);
    int32_t *list = c.packed<int32_t>((size_t)n_pairs * 4), *wide_list = c.packed<int32_t>((size_t)n_pairs * 4);
    int32_t* far_list = c.packed<int32_t>((size_t)n_pairs * 4);
    int32_t* list_count = c.packed<int32_t>(64);                   // [0 .. 2]: second stage, wide, far
    size_t bytes = c.off;
};

// ── host side ────────────────────────────────────────────────────────────────────────────────────────
// What a call starts is decided first and as a whole (plan_icp2: a function of its arguments, no HIP call), then issued
// (launch_icp2).

// One launch: the instantiation, its LDS, and the part of the batch it takes.
struct Icp2Shape {
    int threads, smax;        // THREADS x ICP2_SMAX
    bool in_lds, filter;      // TGT_LDS, FILT
    int lds_points;           // capacity of the LDS copy (points)
    size_t lds;               // dynamic LDS of the launch (bytes)
    int n_lo, m_lo;           // Icp2Args: only the pairs whose source has more than n_lo rows or whose target more than m_lo
    int skip_over;            // Icp2Args: leave the pairs this shape cannot hold to the launch for wide clouds
};
struct Icp2Plan {
    Icp2Shape first;          // every pair of the batch (but the ones it leaves to `wide`)
    bool has_wide;            // a launch for the pairs the first shape cannot hold
    Icp2Shape wide;
    bool two_stage;           // `first` stops after stage1_iterations and a second stage continues the parked pairs
    int stage1_iterations, stage2_grid, wide_grid;
    bool far_wanted;          // the far continuation may run (if the device grants its LDS)
    Icp2Shape far;
    double far_d2;
    bool needs_lists;         // the parked state and the lists of the workspace are used (whether or not `far` runs)
};
constexpr int ICP2_NO_LIMIT = 0x7fffffff;               // it_limit of a launch that runs a pair to its end

// `points` target points at most in LDS (when the targets are staged there at all), for `threads` x `smax` source rows
static Icp2Shape icp2_shape(int threads, int smax, int points, bool in_lds) {
    int cap = 64;
    while (cap < points) cap <<= 1;
    if (points > 1024 && points <= 1536) cap = 1536;
    // The filter needs <= 2 048 points (96 KB, one workgroup per CU).
    const bool filter = in_lds && cap <= 2048;
    return {threads, smax, in_lds, filter, cap, in_lds ? Icp2Lds(cap, filter).bytes : 0, -1, 0, 0};
}

// stages_opt, far_opt: the options ICP2_STAGES and ICP2_FAR (nullptr: not set); have_ws: the caller gave a workspace that
// holds the parked state (Icp2Ws)
static Icp2Plan plan_icp2(int n_pairs, int max_src_n, int max_tgt_n, const icpmi_icp_params& p, bool have_ws,
                          const char* stages_opt, const char* far_opt) {
    Icp2Plan plan{};
    const bool in_lds = max_tgt_n <= 4096;
    const bool many = n_pairs >= 1024;
    // Workgroup shape by source size (rows per thread bounded by the instantiation).
    // A voxel-filtered 2 048-beam scan keeps ~1 400 rows: 768 threads x 2 rows, two workgroups per CU (6 waves per
    // SIMD at 80 registers; 512 x 3 at 4 waves per SIMD is 5 % slower) — one pair's serial solve and barrier waits
    // overlap the other's search.  Clouds that keep more than 1 536 rows go to a second launch (1 024 threads).
    // With few pairs (less than two per CU) 1 024 threads x 2 rows finish a pair soonest.
    int T, SM;
    if (max_src_n <= 1024) { T = 512; SM = 2; }
    else if (many) { T = 768; SM = 2; }
    else if (max_src_n <= 2048) { T = 1024; SM = 2; }
    else { T = 1024; SM = 4; }
    // Two workgroups of the 512-thread shapes share a CU only up to 1 536 filter points (2 x 73.7 KB): larger targets,
    // like larger sources, are left to the second launch.
    const int cap1 = ((T == 512 || T == 768) && many && in_lds && max_tgt_n > 1536) ? 1536 : max_tgt_n;
    plan.first = icp2_shape(T, SM, cap1, in_lds);
    // second launch for the pairs the first shape cannot hold
    plan.has_wide = T * SM < max_src_n || cap1 < max_tgt_n;
    if (plan.has_wide) {
        plan.first.skip_over = 1;
        plan.wide = icp2_shape(1024, max_src_n <= 2048 ? 2 : 4, max_tgt_n, in_lds);
        plan.wide.n_lo = T * SM; plan.wide.m_lo = cap1;
    }
    // Two stages for a large batch (see Icp2Args): needs the caller's workspace for the parked state.  Below ~1 000 pairs
    // every long pair starts within the first two rounds anyway and the stages only add their own cost (512 pairs: 0.70
    // against 0.65 ms).  About one pair
    // in thirteen of a loop-closure batch runs to the iteration limit; 12 iterations settle the others.
    // option ICP2_STAGES = 1 keeps one launch (experiments, and the test that both give the same bits).
    plan.stage1_iterations = ICP2_STAGE1_ITERS;                            // measured 6.12 / 5.42 / 5.36 / 5.38 / 5.39 ms at 8 / 10 / 12 / 14 / 16
    // point-to-line only: its pairs either settle within ~10 iterations or circle to the limit; point-to-point pairs all
    // take 25-40 and would all be parked (ICP2_STAGES = 2 forces the stages for them too: tests)
    plan.two_stage = many && have_ws && p.max_iterations >= 2 * plan.stage1_iterations &&
                     !(stages_opt && stages_opt[0] == '1') &&
                     (p.method == ICPMI_POINT_TO_LINE || (stages_opt && stages_opt[0] == '2'));
    // second-stage workgroups: an eighth of the pairs, one parked pair each (about one pair in twelve is parked; the others
    // leave at once), then 256 workgroups that walk whatever the list holds beyond that
    plan.stage2_grid = n_pairs / 8 > 256 ? n_pairs / 8 : 256;
    // the launch for wide clouds: a thirty-second (a launch of 4 096 workgroups that find an empty list still takes 100 us)
    plan.wide_grid = n_pairs < 256 ? n_pairs : (n_pairs / 32 > 256 ? n_pairs / 32 : 256);
    // option ICP2_FAR = the mean squared error (m^2) of the first step above which a pair goes to the far continuation
    // (default 1: one metre rms — the candidates ICP converges from by itself stay below it: with 0.5 some of them are
    // sent over and the 16 384-pair batch takes 5.7 instead of 5.05 ms; 0 = never)
    plan.far_d2 = far_opt ? atof(far_opt) : 1.0;
    plan.far_wanted = have_ws && in_lds && plan.far_d2 > 0.0 && p.max_iterations > 2;
    // the far continuation's LDS (Icp2Lds): every wave owns the slots behind its own lanes, whatever the batch's source sizes
    int far_cap = 64;
    while (far_cap < max_tgt_n && far_cap < ICP2_FAR_POINTS) far_cap <<= 1;
    plan.far = {ICP2_FAR_THREADS, ICP2_FAR_SMAX, true, true, far_cap,
                Icp2Lds(far_cap, true, true, ICP2_FAR_THREADS * ICP2_FAR_SMAX).bytes, -1, 0, 0};
    plan.needs_lists = have_ws && (plan.two_stage || plan.has_wide);
    return plan;
}

// The four kernels of a shape.
struct Icp2Kernels {
    void (*fused)(Icp2Args);
    void (*wide)(Icp2Args);
    void (*resume)(Icp2Args);
    void (*resume_rest)(Icp2Args, int);
};
template <int T, int S, bool L, bool F>
constexpr Icp2Kernels icp2_kernels() {
    return {icp2_fused_kernel<T, S, L, F>, icp2_wide_kernel<T, S, L, F>, icp2_resume_kernel<T, S, L, F>,
            icp2_resume_rest_kernel<T, S, L, F>};
}
template <int T, int S>
static Icp2Kernels icp2_kernels_of(const Icp2Shape& s) {
    if (!s.in_lds) return icp2_kernels<T, S, false, false>();
    if (s.filter) return icp2_kernels<T, S, true, true>();
    return icp2_kernels<T, S, true, false>();
}
// every instantiation there is; fused == nullptr: none for this shape
static Icp2Kernels icp2_kernels_of(const Icp2Shape& s) {
    if (s.threads == 512 && s.smax == 2) return icp2_kernels_of<512, 2>(s);
    if (s.threads == 768 && s.smax == 2) return icp2_kernels_of<768, 2>(s);
    if (s.threads == 1024 && s.smax == 2) return icp2_kernels_of<1024, 2>(s);
    if (s.threads == 1024 && s.smax == 4) return icp2_kernels_of<1024, 4>(s);
    return {nullptr, nullptr, nullptr, nullptr};
}

// the arguments of one launch: the shape's part of the batch and LDS capacity, iterations [it_begin, it_limit)
static Icp2Args icp2_args(const Icp2Args& base, const Icp2Shape& s, int it_begin, int it_limit, int resume) {
    Icp2Args a = base;
    a.lds_points = s.lds_points; a.n_lo = s.n_lo; a.m_lo = s.m_lo; a.skip_over = s.skip_over;
    a.it_begin = it_begin; a.it_limit = it_limit; a.resume = resume;
    return a;
}

// called by icpmi_icp_batch (icp.hip) when a prepared buffer is given and everything fits
int launch_icp2(const double* pts, const int32_t* off, const int32_t* cnt, const int32_t* ps, const int32_t* pt,
                int n_pairs, int max_src_n, int max_tgt_n, int total_rows, const icpmi_icp_params* p, const double* init,
                double* results, const void* prepared, void* workspace, size_t workspace_bytes, const IcpGate* gate,
                hipStream_t st) {
    const Icp2Ws w{workspace, n_pairs, max_src_n};
    const bool have_ws = workspace && workspace_bytes >= w.bytes;
    const Icp2Plan plan = plan_icp2(n_pairs, max_src_n, max_tgt_n, *p, have_ws, option("ICP2_STAGES"), option("ICP2_FAR"));
    const Icp2Kernels k1 = icp2_kernels_of(plan.first), k2 = icp2_kernels_of(plan.wide);
    if (!k1.fused || (plan.has_wide && !k2.fused)) return ICPMI_ERR_ARG;
    Icp2Args base;                                          // the parked state, the lists and the gate: none unless set below
    if (gate) base.gate = *gate;
    const PreparedView v(prepared, total_rows);
    base.pts = pts; base.off = off; base.cnt = cnt; base.pair_src = ps; base.pair_tgt = pt; base.init = init; base.results = results;
    base.g_sxy = v.sxy; base.g_snrm = v.snrm; base.g_sorig = v.sorig; base.g_skey = v.skey; base.g_dir = v.dir;
    base.error_threshold = p->error_threshold; base.max_corr_dist = p->max_corr_dist;
    base.max_iterations = p->max_iterations; base.method = p->method; base.has_init = p->has_init;
    // The far continuation's LDS is asked for BEFORE the first launch: without it (another ARCH than gfx950's 160 KB) no
    // pair is parked for a kernel that could not start.
    const bool far_go = plan.far_wanted && dyn_lds((const void*)icp2_far_kernel, plan.far.lds) == hipSuccess;
    if (plan.needs_lists || far_go) {
        base.st_xy = w.st_xy; base.st_pos = w.st_pos; base.st_stride = max_src_n;
        base.list = w.list; base.list_count = w.list_count;
        if (plan.has_wide) { base.wide_list = w.wide_list; base.wide_count = w.list_count + 1; }
        if (far_go) { base.far_list = w.far_list; base.far_count = w.list_count + 2; base.far_d2 = plan.far_d2; }
        if (hipMemsetAsync(w.list_count, 0, 3 * sizeof(int32_t), st) != hipSuccess) return ICPMI_ERR_HIP;
    }
    // (state.hip: the library's side streams, one set per device; the lock is held for the fork / launch / join sequence)
    SideLock side_lock;
    Side* const side = side_lock.side;

    // first launch: every pair, to its end or (two stages) to the end of the first stage
    const Icp2Shape& s1 = plan.first;
    if (dyn_lds((const void*)k1.fused, s1.lds) != hipSuccess) return ICPMI_ERR_HIP;
    k1.fused<<<n_pairs, s1.threads, s1.lds, st>>>(
        icp2_args(base, s1, 0, plan.two_stage ? plan.stage1_iterations : ICP2_NO_LIMIT, 0));
    bool forked = false;
    if (plan.two_stage) {
        // The launch for wide clouds (a handful of pairs, ~0.1 ms at a few per cent of the chip) only needs the first stage's
        // list: it runs on a side stream beside the second stage and joins the caller's stream afterwards.
        if (base.wide_list && side) forked = hipEventRecord(side->fork, st) == hipSuccess;
        // second stage: the parked pairs, all started together
        const Icp2Args second = icp2_args(base, s1, plan.stage1_iterations, ICP2_NO_LIMIT, 1);
        if (dyn_lds((const void*)k1.resume, s1.lds) != hipSuccess) return ICPMI_ERR_HIP;
        k1.resume<<<plan.stage2_grid, s1.threads, s1.lds, st>>>(second);
        if (plan.stage2_grid < n_pairs) {                   // more parked pairs than workgroups: the rest of the list
            if (dyn_lds((const void*)k1.resume_rest, s1.lds) != hipSuccess) return ICPMI_ERR_HIP;
            k1.resume_rest<<<256, s1.threads, s1.lds, st>>>(second, plan.stage2_grid);
        }
    }
    if (plan.has_wide) {
        const Icp2Shape& s2 = plan.wide;
        const Icp2Args wide = icp2_args(base, s2, 0, ICP2_NO_LIMIT, 0);
        if (base.wide_list) {                               // the listed pairs: few workgroups walking the list
            if (dyn_lds((const void*)k2.wide, s2.lds) != hipSuccess) return ICPMI_ERR_HIP;
            hipStream_t ws = st;                            // beside the second stage when the side stream is there
            if (forked && hipStreamWaitEvent(side->stream[0], side->fork, 0) == hipSuccess) ws = side->stream[0];
            k2.wide<<<plan.wide_grid, s2.threads, s2.lds, ws>>>(wide);
            if (ws != st && (hipEventRecord(side->join[0], ws) != hipSuccess ||
                             hipStreamWaitEvent(st, side->join[0], 0) != hipSuccess)) {
                (void)hipStreamSynchronize(ws);             // never return with a launch the caller cannot order against
                return ICPMI_ERR_HIP;
            }
        } else {                                            // no workspace, no list: a workgroup per pair of the batch looks
            if (dyn_lds((const void*)k2.fused, s2.lds) != hipSuccess) return ICPMI_ERR_HIP;
            k2.fused<<<n_pairs, s2.threads, s2.lds, st>>>(wide);
        }
    }
    if (base.far_list) {                                    // after every first launch (the wide one has joined the stream)
        Icp2Args far = icp2_args(base, plan.far, 2, ICP2_NO_LIMIT, 1);
        far.far_row_threads = s1.threads; far.far_row_n = s1.threads * s1.smax; far.far_row_m = s1.lds_points;
        icp2_far_kernel<<<n_pairs < 256 ? n_pairs : 256, plan.far.threads, plan.far.lds, st>>>(far);
    }
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

}  // namespace icpmi
