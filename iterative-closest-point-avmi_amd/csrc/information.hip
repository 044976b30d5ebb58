// information.hip — the Gauss-Newton information matrix of an ICP result, as a pass of its own.
// Evaluates the normal equations of reference utilities/icp.py:92-104 (_point_to_line_solve_2d: ATA, ATb) — and the
// point-to-point counterpart the reference never forms — ONCE, at a transform the caller hands in: the fused ICP kernels
// (icp.hip, icp2.hip) keep their register budget, and a pose-graph caller gets H = A^T A in [theta, tx, ty] for the
// pairs it accepted.  Matching and the inlier test are the ICP's own (nn.hpp; icp.py:179, 184-186).
#include "nn.hpp"

namespace icpmi {

constexpr int INFO_THREADS = ICPMI_INFO_THREADS;          // 8 waves: one workgroup per pair
constexpr int INFO_WAVES = INFO_THREADS / ICPMI_WAVE;
constexpr int INFO_TILE_ROWS = ICPMI_INFO_TILE_ROWS;      // target rows per LDS tile (32 KiB)
constexpr int INFO_NV = 11;                               // H (6), g (3), sse, inliers: the sums of a record
static_assert(INFO_TILE_ROWS % NN_CHUNK == 0, "a full tile needs no padding");
static_assert(INFO_WAVES <= 16, "block_sum combines at most 16 waves");
static_assert(ICPMI_INFO_H + 6 == ICPMI_INFO_G && ICPMI_INFO_G + 3 == ICPMI_INFO_SSE && ICPMI_INFO_SSE + 1 == ICPMI_INFO_INLIERS,
              "the sums are consecutive slots, in the order the kernel accumulates them");

// The workgroup's dynamic LDS, described once: the target tile, then the scratch of the one block_sum.
struct InfoLds {
    static constexpr int tile_doubles = INFO_TILE_ROWS * 2;
    static constexpr int sum_doubles = block_sum_doubles<INFO_NV>();
    static constexpr size_t bytes = (size_t)(tile_doubles + sum_doubles) * sizeof(double);
};

struct InfoArgs {
    const double* pts;
    const int32_t* off;
    const int32_t* cnt;
    const double* normals;
    const int32_t* pair_src;
    const int32_t* pair_tgt;
    const double* transforms;
    double max_corr_dist;
    double* out;
};

// one residual row [a0, a1, a2 | b] into the sums: H upper triangle, g, sse
__device__ __forceinline__ void info_add_row(double (&acc)[INFO_NV], double a0, double a1, double a2, double b) {
    acc[0] += a0 * a0; acc[1] += a0 * a1; acc[2] += a0 * a2;
    acc[3] += a1 * a1; acc[4] += a1 * a2; acc[5] += a2 * a2;
    acc[6] += a0 * b;  acc[7] += a1 * b;  acc[8] += a2 * b;
    acc[9] += b * b;
}

// grid = pairs.  Lane l of the workgroup owns the source rows l, l + INFO_THREADS, ... of its pair (a fixed assignment),
// each pass of INFO_THREADS rows streams the whole target through LDS (nn.hpp), and the lane partials meet in ONE
// block_sum: the DPP tree inside a wave, LDS in wave order across waves.  No atomics: a record is the same bits every run
// and for every batch its pair is part of.
template <bool P2L>
__global__ __launch_bounds__(INFO_THREADS) void information_kernel(InfoArgs a) {
    extern __shared__ __attribute__((aligned(16))) double info_lds[];
    double* tile = info_lds;
    double* sums = info_lds + InfoLds::tile_doubles;
    const int b = blockIdx.x;
    const int sc = a.pair_src[b], tc = a.pair_tgt[b];
    const int N = a.cnt ? a.cnt[sc] : a.off[sc + 1] - a.off[sc];
    const int M = a.cnt ? a.cnt[tc] : a.off[tc + 1] - a.off[tc];
    double* out = a.out + (size_t)b * ICPMI_INFO_DOUBLES;
    if (N <= 0 || M <= 0) {                                    // uniform per workgroup, before any barrier
        if (threadIdx.x < ICPMI_INFO_DOUBLES) out[threadIdx.x] = threadIdx.x == ICPMI_INFO_STATUS ? (double)ICPMI_ST_EMPTY : 0.0;
        return;
    }
    const double* src = a.pts + (size_t)a.off[sc] * 2;
    const double* tgt = a.pts + (size_t)a.off[tc] * 2;
    const double* nrm = P2L ? a.normals + (size_t)a.off[tc] * 2 : nullptr;
    const double* T = a.transforms + (size_t)b * 6;
    const double r00 = T[0], r01 = T[1], r10 = T[2], r11 = T[3], tx = T[4], ty = T[5];
    const bool has_corr = a.max_corr_dist >= 0.0;
    const double max_corr_sq = a.max_corr_dist * a.max_corr_dist;   // icp.py:169

    double acc[INFO_NV];
#pragma unroll
    for (int i = 0; i < INFO_NV; ++i) acc[i] = 0.0;
    block_sum_init(sums, InfoLds::sum_doubles);                // (the first tile's barrier orders it before the reduction)

    for (int base = 0; base < N; base += INFO_THREADS) {       // uniform trip count: the barriers inside are reached by all
        const int n = base + (int)threadIdx.x;
        const int nn = n < N ? n : N - 1;                      // clamp: tail lanes repeat the last row and add nothing
        const double sx = src[(size_t)nn * 2], sy = src[(size_t)nn * 2 + 1];
        double p[1][2], best[1] = {__builtin_inf()};
        int bestj[1] = {0};
        p[0][0] = (r00 * sx + r01 * sy) + tx;                  // the moved row, as include/icpmi.h states it (no contraction)
        p[0][1] = (r10 * sx + r11 * sy) + ty;
        for (int t0 = 0; t0 < M; t0 += INFO_TILE_ROWS) {
            const int c = min(INFO_TILE_ROWS, M - t0);
            __syncthreads();
            const int padded = stage_targets<2>(tgt + (size_t)t0 * 2, c, tile);
            __syncthreads();
            nn_scan_tile<2, 1>(tile, padded, t0, p, best, bestj);
        }
        if (n >= N) continue;
        const double dist = sqrt(best[0]);                     // IEEE sqrt, as KDTree returns (icp.py:179)
        if (has_corr && !(dist * dist < max_corr_sq)) continue;    // icp.py:184-185
        const double px = p[0][0], py = p[0][1];
        const double qx = tgt[(size_t)bestj[0] * 2], qy = tgt[(size_t)bestj[0] * 2 + 1];
        const double dx = px - qx, dy = py - qy;
        if (P2L) {                                             // icp.py:92-101
            const double nx = nrm[(size_t)bestj[0] * 2], ny = nrm[(size_t)bestj[0] * 2 + 1];
            info_add_row(acc, ny * px - nx * py, nx, ny, -(nx * dx + ny * dy));
        } else {                                               // d(R(theta) p + t)/d(theta, tx, ty) at theta = 0, both axes
            info_add_row(acc, -py, 1.0, 0.0, -dx);
            info_add_row(acc, px, 0.0, 1.0, -dy);
        }
        acc[10] += 1.0;
    }
    block_sum<INFO_NV, INFO_WAVES>(acc, sums);
    if (threadIdx.x == 0) {
        const double inliers = acc[10];
        const int need = max(3, N / 10);                       // icp.py:186
        const double status = has_corr && inliers < (double)need ? (double)ICPMI_ST_FEW_INLIERS : 0.0;
        double2* o = reinterpret_cast<double2*>(out);
        o[0] = make_double2(acc[0], acc[1]);
        o[1] = make_double2(acc[2], acc[3]);
        o[2] = make_double2(acc[4], acc[5]);
        o[3] = make_double2(acc[6], acc[7]);
        o[4] = make_double2(acc[8], acc[9]);
        o[5] = make_double2(inliers, (double)N);
        o[6] = make_double2(status, 0.0);
        o[7] = make_double2(0.0, 0.0);
    }
}

// What a call starts, decided as a whole and without a HIP call: one workgroup per pair, whatever the sizes — the block
// and the tile never depend on the batch, so a pair's record does not depend on the batch it is computed in.
struct InfoPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    unsigned grid, block;     // grid == 0: nothing to do
    size_t lds_bytes;
};
static InfoPlan plan_information(int n_pairs, int max_src_n) {
    InfoPlan p{ICPMI_OK, 0, INFO_THREADS, InfoLds::bytes};
    if (n_pairs < 0 || max_src_n < 0) { p.rc = ICPMI_ERR_ARG; return p; }
    p.grid = (unsigned)n_pairs;
    return p;
}

}  // namespace icpmi

extern "C" int icpmi_icp_information_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                           const double* normals, const int32_t* pair_src, const int32_t* pair_tgt,
                                           int32_t n_pairs, int32_t max_src_n, const double* transforms, int32_t method,
                                           double max_corr_dist, double* out, void* stream) {
    using namespace icpmi;
    if (method != ICPMI_POINT_TO_POINT && method != ICPMI_POINT_TO_LINE) return ICPMI_ERR_UNSUPPORTED;
    const InfoPlan plan = plan_information(n_pairs, max_src_n);
    if (plan.rc != ICPMI_OK || plan.grid == 0) return plan.rc;
    if (!pts || !off_dev || !pair_src || !pair_tgt || !transforms || !out) return ICPMI_ERR_ARG;
    if (method == ICPMI_POINT_TO_LINE && !normals) return ICPMI_ERR_ARG;
    if (max_corr_dist != max_corr_dist) return ICPMI_ERR_ARG;  // NaN: neither a gate nor None
    const InfoArgs a{pts, off_dev, cnt_dev, normals, pair_src, pair_tgt, transforms, max_corr_dist, out};
    hipStream_t st = (hipStream_t)stream;
    if (method == ICPMI_POINT_TO_LINE) information_kernel<true><<<plan.grid, plan.block, plan.lds_bytes, st>>>(a);
    else information_kernel<false><<<plan.grid, plan.block, plan.lds_bytes, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
