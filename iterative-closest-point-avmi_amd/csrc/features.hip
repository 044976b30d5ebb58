// features.hip — feature_based_alignment (reference utilities/features.py:247-315) and its five stages.
//
// The reference pre-aligns a scan pair by curvature keypoints, sorted-distance descriptors, Lowe matching and a two-point
// RANSAC.  Its clouds are a few hundred rows (voxel filter at 0.2 m), so every stage is one workgroup per cloud or per
// pair with the cloud staged in LDS and an exhaustive float64 neighbour scan (the lists of prep_common.hpp, ordered by
// (distance, row) as icpmi_normals_2d_batch orders them).  The stages are separate kernels: the single-stage entry
// points and the chain (icpmi_feature_align_batch) launch the SAME kernels, so the chain is the composition of the
// stages by construction.  The three pair stages (matching, RANSAC, the record) read a source side and a target side
// (FtSide): the batch passes one set of tables twice, the resident chain of a scan history (icpmi_history_feature_align,
// at the end of this file) takes its targets — and without a start per pair its sources — from the history's feature store.
//
// The host side, after the kernels, has each thing once: the cloud-side limits (ft_cfg_check), the workspace of both chains
// (FtWs), the per-cloud half of both chains and of a history's feature store (ft_cloud_stages, in features.hpp for
// history.hip), the work set of a call with a start per pair (ft_build_work_set), the pair half (ft_pair_stages).
//
// What is pinned to the reference's numbers, stage by stage ("feature alignment"):
//   curvature     to the reference's own sensitivity to summation order: np.cov sums the neighbours in per-point distance
//                 order; here they are summed in ASCENDING ROW order, so rows with the same neighbour set get the same bits
//   keypoints     bit for bit, given the candidate order (sqrt(dx*dx + dy*dy) without contraction, the `<` of features.py:67)
//   descriptors   bit for bit (exact neighbour distances, IEEE sqrt, as KDTree.query)
//   matches       identical lists when the ratio test is not within rounding of equality (the fixtures check their margins)
//   RANSAC        the hypotheses are an input; inlier counts equal when no error is within rounding of the threshold
#include "features.hpp"
#include "linalg.hpp"
#include "prep_common.hpp"
#include "sort.hpp"

#include <vector>

namespace icpmi {

constexpr int FT_MAX_ROWS = ICPMI_FT_MAX_ROWS;          // rows of a cloud the stage kernels hold in LDS
constexpr int FT_MAX_KP = ICPMI_FT_MAX_KP;              // keypoints per cloud (top_n), matches per pair
constexpr int FT_DESC_STRIDE = ICPMI_FT_DESC_STRIDE;    // doubles per descriptor row (k <= 31)
constexpr int FT_MAX_K = 31;
constexpr int FT_THREADS = 256;
// (record slots and statuses: ICPMI_FTREC_*, ICPMI_FT_ST_*, include/icpmi.h)

// the cloud of a workgroup: its rows in LDS, and the identity map the (distance, row) lists break ties with
struct FtCloud {
    int c, n, first;          // cloud, valid rows (0: nothing to do), first row in the set
};
// valid rows of cloud c of a set: its count (nullptr: every cloud is full), at most the rows its offsets give it
__device__ __forceinline__ int ft_rows(const int32_t* __restrict__ off, const int32_t* __restrict__ cnt, int c) {
    const int cap = off[c + 1] - off[c];
    return min(cnt ? cnt[c] : cap, cap);
}
// keypoints of a cloud, matches of a pair: a stored count never reaches past its slots
__device__ __forceinline__ int ft_clamp_kp(int n, int kp_stride) { return min(min(n, kp_stride), FT_MAX_KP); }

__device__ __forceinline__ FtCloud ft_stage_cloud(const double* __restrict__ pts, const int32_t* __restrict__ off,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ cloud_ids,
                                                  double2* P, int32_t* ident) {
    FtCloud f;
    f.c = cloud_ids ? cloud_ids[blockIdx.x] : (int)blockIdx.x;
    f.first = off[f.c];
    const int n = ft_rows(off, cnt, f.c);
    f.n = (n < 0 || n > FT_MAX_ROWS) ? 0 : n;               // beyond the capacity: left alone (the chain reports status 2)
    const double2* g = reinterpret_cast<const double2*>(pts) + f.first;
    for (int i = threadIdx.x; i < f.n; i += blockDim.x) {
        P[i] = g[i];
        if (ident) ident[i] = i;
    }
    __syncthreads();
    return f;
}

__device__ __forceinline__ double ft_d2(const double2 q, const double2 c) {
    const double dx = q.x - c.x, dy = q.y - c.y;
    double s = 0.0;
    s += dx * dx;
    s += dy * dy;
    return s;
}

// the KK best (distance^2, row) of q over the n rows of P, ascending, ties by the lower row
template <int KK>
__device__ __forceinline__ void ft_knn(const double2* P, const int32_t* ident, int n, const double2 q, TopKP<KK>& top) {
    top.init();
    for (int j = 0; j < n; ++j) top.push(ft_d2(q, P[j]), j, ident);
}

// ── 1. compute_curvature, features.py:35-54 ─────────────────────────────────────────────────────────
// Row i: its kk = min(k, n - 1) + 1 nearest rows (itself included), np.cov of them (mean, deviations, sums scaled by
// 1 / (kk - 1)), the eigenvalues of the 2 x 2 matrix in closed form, ev[0] / (ev[-1] + 1e-10).  The neighbours are summed
// in ascending row order: row j belongs to the set when (d2_j, j) <= (d2, row) of the last list entry.
template <int KK>
__device__ __forceinline__ void ft_curvature_rows(const double2* P, const int32_t* ident, int n, int kk, double* __restrict__ out) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (kk < 3) { out[i] = 0.0; continue; }                    // features.py:49-50
        const double2 q = P[i];
        TopKP<KK> top;
        ft_knn<KK>(P, ident, n, q, top);
        const double dk = kk == KK ? top.d[KK - 1] : top.kth(kk - 1);
        int pk = 0;
        top.template for_first<0>(kk, [&](int pos) { pk = pos; });   // row of the last entry
        double mx = 0.0, my = 0.0;
        for (int j = 0; j < n; ++j) {
            const double2 c = P[j];
            const double d = ft_d2(q, c);
            if (d < dk || (d == dk && j <= pk)) { mx += c.x; my += c.y; }
        }
        mx /= (double)kk; my /= (double)kk;
        double sxx = 0.0, sxy = 0.0, syy = 0.0;
        for (int j = 0; j < n; ++j) {
            const double2 c = P[j];
            const double d = ft_d2(q, c);
            if (d < dk || (d == dk && j <= pk)) {
                const double dx = c.x - mx, dy = c.y - my;
                sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
            }
        }
        const double f = 1.0 / (double)(kk - 1);                   // np.cov: c *= 1 / (N - ddof)
        const double a = sxx * f, b = sxy * f, c2 = syy * f;
        const double h = 0.5 * (a - c2), rad = sqrt(h * h + b * b), mid = 0.5 * (a + c2);
        out[i] = (mid - rad) / ((mid + rad) + 1e-10);              // features.py:53
    }
}

__global__ __launch_bounds__(FT_THREADS) void ft_curvature_kernel(const double* __restrict__ pts, const int32_t* __restrict__ off,
                                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ cloud_ids,
                                                                  int k, double* __restrict__ out_curv) {
    __shared__ double2 P[FT_MAX_ROWS];
    __shared__ int32_t ident[FT_MAX_ROWS];
    const FtCloud f = ft_stage_cloud(pts, off, cnt, cloud_ids, P, ident);
    if (f.n <= 0) return;
    const int kk = min(k, f.n - 1) + 1;                            // features.py:43, 45
    double* out = out_curv + f.first;
    if (kk <= 8) ft_curvature_rows<8>(P, ident, f.n, kk, out);
    else if (kk <= 16) ft_curvature_rows<16>(P, ident, f.n, kk, out);
    else ft_curvature_rows<32>(P, ident, f.n, kk, out);
}

// ── 2. extract_keypoints, features.py:57-71 ─────────────────────────────────────────────────────────
// One wave per cloud.  The candidates are walked in `order` (rows of the cloud; the drop-in passes np.argsort(-curvatures))
// or, without one, by descending curvature with ties by ascending row (sort.hpp).  A candidate is kept when no kept point
// is closer than min_dist: the kept points are spread over the lanes, the walk itself is sequential as the reference's.
__global__ __launch_bounds__(ICPMI_WAVE) void ft_keypoints_kernel(const double* __restrict__ pts, const int32_t* __restrict__ off,
                                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ cloud_ids,
                                                                  const double* __restrict__ curv, const int32_t* __restrict__ order,
                                                                  int top_n, double min_dist, int32_t* __restrict__ out_kp,
                                                                  int32_t* __restrict__ out_kp_cnt, int kp_stride) {
    __shared__ double2 P[FT_MAX_ROWS];
    __shared__ uint64_t keys[FT_MAX_ROWS];
    __shared__ uint32_t rows[FT_MAX_ROWS];
    __shared__ double2 kept[FT_MAX_KP];
    const FtCloud f = ft_stage_cloud(pts, off, cnt, cloud_ids, P, nullptr);
    const int n = f.n;
    int32_t* kp = out_kp + (size_t)f.c * kp_stride;
    if (n <= 0) { if (threadIdx.x == 0) out_kp_cnt[f.c] = 0; return; }
    if (order) {
        for (int i = threadIdx.x; i < n; i += ICPMI_WAVE) rows[i] = (uint32_t)order[f.first + i];
        __syncthreads();
    } else {
        const int npad = sort_npad(n);
        for (int i = threadIdx.x; i < npad; i += ICPMI_WAVE) {
            keys[i] = i < n ? f64_sortable(-curv[f.first + i]) : ~0ull;       // ascending -curvature = descending curvature
            rows[i] = i < n ? (uint32_t)i : 0xffffffffu;
        }
        __syncthreads();
        bitonic_sort_pairs(keys, rows, npad);
    }
    const int limit = ft_clamp_kp(top_n, kp_stride);
    int nk = 0;                                                     // the same in every lane
    for (int c = 0; c < n && nk < limit; ++c) {
        const uint32_t idx = rows[c];
        if (idx >= (uint32_t)n) continue;                           // not a row of this cloud: ignored
        const double2 p = P[idx];
        bool close = false;
        for (int t = threadIdx.x; t < nk; t += ICPMI_WAVE) {
            const double dx = kept[t].x - p.x, dy = kept[t].y - p.y;
            close = close || sqrt(dx * dx + dy * dy) < min_dist;    // np.linalg.norm(kp_pts - p, axis=1) < min_dist, features.py:67
        }
        if (__syncthreads_or(close ? 1 : 0)) continue;
        if (threadIdx.x == 0) { kept[nk] = p; kp[nk] = (int32_t)idx; }
        ++nk;
        __syncthreads();
    }
    if (threadIdx.x == 0) out_kp_cnt[f.c] = nk;
}

// ── 3. compute_descriptors, features.py:76-87 ───────────────────────────────────────────────────────
// A thread per keypoint: the distances to its min(k, n - 1) nearest other rows, ascending — columns 1 .. of the sorted
// distances to its kk = min(k, n - 1) + 1 nearest rows, whichever of them the point itself is (KDTree.query, dists[:, 1:]).
template <int KK>
__device__ __forceinline__ void ft_descriptor_rows(const double2* P, const int32_t* ident, int n, int kk, const int32_t* __restrict__ kp,
                                                   int n_kp, double* __restrict__ desc) {
    for (int s = threadIdx.x; s < n_kp; s += blockDim.x) {
        double* out = desc + (size_t)s * FT_DESC_STRIDE;
        const int row = kp[s];
        if (row < 0 || row >= n) {                                  // not a row of this cloud: a row of NaN matches nothing
#pragma unroll
            for (int i = 0; i < FT_DESC_STRIDE; ++i) out[i] = __builtin_nan("");
            continue;
        }
        TopKP<KK> top;
        ft_knn<KK>(P, ident, n, P[row], top);
#pragma unroll
        for (int i = 1; i < KK; ++i) out[i - 1] = i < kk ? sqrt(top.d[i]) : 0.0;
#pragma unroll
        for (int i = KK - 1; i < FT_DESC_STRIDE; ++i) out[i] = 0.0;
    }
}

__global__ __launch_bounds__(FT_THREADS) void ft_descriptors_kernel(const double* __restrict__ pts, const int32_t* __restrict__ off,
                                                                    const int32_t* __restrict__ cnt, const int32_t* __restrict__ cloud_ids,
                                                                    const int32_t* __restrict__ kp, const int32_t* __restrict__ kp_cnt,
                                                                    int kp_stride, int k, double* __restrict__ out_desc,
                                                                    int32_t* __restrict__ out_desc_len) {
    __shared__ double2 P[FT_MAX_ROWS];
    __shared__ int32_t ident[FT_MAX_ROWS];
    const FtCloud f = ft_stage_cloud(pts, off, cnt, cloud_ids, P, ident);
    if (f.n <= 0) { if (threadIdx.x == 0) out_desc_len[f.c] = 0; return; }
    const int kk = min(k, f.n - 1) + 1;                            // features.py:82, 85
    const int n_kp = ft_clamp_kp(kp_cnt[f.c], kp_stride);
    const int32_t* my_kp = kp + (size_t)f.c * kp_stride;
    double* desc = out_desc + (size_t)f.c * kp_stride * FT_DESC_STRIDE;
    if (kk <= 8) ft_descriptor_rows<8>(P, ident, f.n, kk, my_kp, n_kp, desc);
    else if (kk <= 16) ft_descriptor_rows<16>(P, ident, f.n, kk, my_kp, n_kp, desc);
    else ft_descriptor_rows<32>(P, ident, f.n, kk, my_kp, n_kp, desc);
    if (threadIdx.x == 0) out_desc_len[f.c] = kk - 1;
}

// ── one side of a pair ───────────────────────────────────────────────────────────────────────────────
// The pair stages read a source cloud and a target cloud.  Each comes from a set of per-cloud tables — filtered points,
// offsets, counts, keypoints, descriptors — described once here.  A batch whose clouds are all of one set passes that set
// as both sides; a resident history with a start per pair takes its sources from a work set and its targets from the
// store.  Both sides share kp_stride.
struct FtSide {
    const double* __restrict__ pts;
    const int32_t* __restrict__ off;
    const int32_t* __restrict__ cnt;          // nullptr: every cloud is full (off[c + 1] - off[c] rows)
    const int32_t* __restrict__ kp;
    const int32_t* __restrict__ kp_cnt;
    const double* __restrict__ desc;
    const int32_t* __restrict__ desc_len;
};

// ── 4. match_descriptors, features.py:92-106 ────────────────────────────────────────────────────────
// A thread per source keypoint: squared descriptor distance to every target keypoint by direct differences, the two
// smallest (the lower index on ties), Lowe's test D0 < ratio^2 * D1.  The matches leave in source-keypoint order.
__global__ __launch_bounds__(FT_MAX_KP) void ft_match_kernel(const FtSide src, const FtSide tgt, int kp_stride,
                                                            const int32_t* __restrict__ pair_src, const int32_t* __restrict__ pair_tgt,
                                                            double ratio_sq, int32_t* __restrict__ out_matches,
                                                            int32_t* __restrict__ out_match_cnt) {
    __shared__ int wave_tot[FT_MAX_KP / ICPMI_WAVE];
    const int b = blockIdx.x, i = threadIdx.x;
    const int sc = pair_src[b], tc = pair_tgt[b];
    const int ns = ft_clamp_kp(src.kp_cnt[sc], kp_stride), nt = ft_clamp_kp(tgt.kp_cnt[tc], kp_stride);
    const int len = src.desc_len[sc];
    // features.py:97; descriptors of different lengths cannot be compared (NumPy raises; the chain reports status 5)
    const bool any = ns > 0 && nt >= 2 && len == tgt.desc_len[tc] && len > 0 && len <= FT_MAX_K;
    bool ok = false;
    int j0 = 0;
    if (any && i < ns) {
        const double* a_row = src.desc + ((size_t)sc * kp_stride + i) * FT_DESC_STRIDE;
        double a[FT_MAX_K];
#pragma unroll
        for (int q = 0; q < FT_MAX_K; ++q) a[q] = q < len ? a_row[q] : 0.0;
        double best0 = __builtin_inf(), best1 = __builtin_inf();
        const double* t_rows = tgt.desc + (size_t)tc * kp_stride * FT_DESC_STRIDE;
        for (int j = 0; j < nt; ++j) {
            const double* b_row = t_rows + (size_t)j * FT_DESC_STRIDE;
            double D = 0.0;
#pragma unroll
            for (int q = 0; q < FT_MAX_K; ++q)
                if (q < len) { const double t = a[q] - b_row[q]; D += t * t; }
            if (D < best0) { best1 = best0; best0 = D; j0 = j; }
            else if (D < best1) best1 = D;
        }
        ok = best0 < ratio_sq * best1;                             // features.py:104
    }
    // positions in source-keypoint order: wave ballots, then the totals of the waves before
    const unsigned long long mask = __ballot(ok);
    const int before = __popcll(mask & ((1ull << lane_id()) - 1ull));
    if (lane_id() == 0) wave_tot[wave_id()] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < FT_MAX_KP / ICPMI_WAVE; ++w) { if (w < wave_id()) base += wave_tot[w]; total += wave_tot[w]; }
    if (ok) {
        int32_t* m = out_matches + ((size_t)b * kp_stride + base + before) * 2;
        m[0] = i; m[1] = j0;
    }
    if (i == 0) out_match_cnt[b] = total;
}

// ── 5. ransac_align, features.py:125-160 ────────────────────────────────────────────────────────────
// _rigid_from_points (features.py:111-122) of two matches in closed form.  W = sum (s - mu_s)(d - mu_d)^T has rank <= 1;
// V U^T with the det fix is the rotation that carries the source difference onto the target difference (kabsch2), and
// for W = 0 — both matches share their target keypoint — the SVD of the reference gives R = I, as kabsch2 does.
struct FtRigid {
    double r[4], tx, ty;
};
__device__ __forceinline__ FtRigid ft_rigid2(const double2 s0, const double2 s1, const double2 d0, const double2 d1) {
    const double msx = (s0.x + s1.x) / 2.0, msy = (s0.y + s1.y) / 2.0, mdx = (d0.x + d1.x) / 2.0, mdy = (d0.y + d1.y) / 2.0;
    const double p0x = s0.x - msx, p0y = s0.y - msy, p1x = s1.x - msx, p1y = s1.y - msy;
    const double q0x = d0.x - mdx, q0y = d0.y - mdy, q1x = d1.x - mdx, q1y = d1.y - mdy;
    const double W[4] = {p0x * q0x + p1x * q1x, p0x * q0y + p1x * q1y, p0y * q0x + p1y * q1x, p0y * q0y + p1y * q1y};
    FtRigid g;
    kabsch2(W, g.r);
    g.tx = mdx - (g.r[0] * msx + g.r[1] * msy);                     // t = mu_d - R @ mu_s
    g.ty = mdy - (g.r[2] * msx + g.r[3] * msy);
    return g;
}
__device__ __forceinline__ double ft_err(const FtRigid& g, const double2 s, const double2 d) {
    const double ex = ((s.x * g.r[0] + s.y * g.r[1]) + g.tx) - d.x, ey = ((s.x * g.r[2] + s.y * g.r[3]) + g.ty) - d.y;
    return sqrt(ex * ex + ey * ey);                                 // np.linalg.norm(src @ R.T + t - dst, axis=1)
}

// "no alignment" in a pair's record: identity, zeros, 0 inliers, no winning hypothesis
__device__ __forceinline__ void ft_write_no_alignment(double* __restrict__ rec) {
    rec[ICPMI_FTREC_INLIERS] = 0.0;
    rec[ICPMI_FTREC_R] = 1.0; rec[ICPMI_FTREC_R + 1] = 0.0; rec[ICPMI_FTREC_R + 2] = 0.0; rec[ICPMI_FTREC_R + 3] = 1.0;
    rec[ICPMI_FTREC_T] = 0.0; rec[ICPMI_FTREC_T + 1] = 0.0;
    rec[ICPMI_FTREC_BEST] = -1.0;
}

// hypothesis h of a pair with n matches: the index pair, from the int32 table or from two uniform doubles in [0, 1):
// i = floor(u0 * n), j = floor(u1 * (n - 1)), j += (j >= i) — two distinct indices, each pair equally likely
__device__ __forceinline__ bool ft_hypothesis(const int32_t* __restrict__ hyp_idx, const double* __restrict__ hyp_u, size_t h, int n,
                                              int& i, int& j) {
    if (hyp_idx) { i = hyp_idx[2 * h]; j = hyp_idx[2 * h + 1]; }
    else {
        i = min((int)(hyp_u[2 * h] * (double)n), n - 1);
        j = min((int)(hyp_u[2 * h + 1] * (double)(n - 1)), n - 2);
        j += j >= i ? 1 : 0;
    }
    return i >= 0 && j >= 0 && i < n && j < n && i != j;            // anything else counts no inliers
}

__global__ __launch_bounds__(FT_THREADS) void ft_ransac_kernel(const FtSide src, const FtSide tgt, int kp_stride,
                                                               const int32_t* __restrict__ pair_src, const int32_t* __restrict__ pair_tgt,
                                                               const int32_t* __restrict__ matches, const int32_t* __restrict__ match_cnt,
                                                               const int32_t* __restrict__ hyp_idx, const double* __restrict__ hyp_u,
                                                               int n_iter, int hyp_pair_stride, double thresh,
                                                               double* __restrict__ records, int32_t* __restrict__ out_counts) {
    __shared__ double2 S[FT_MAX_KP], D[FT_MAX_KP];
    __shared__ int red_cnt[FT_THREADS / ICPMI_WAVE], red_idx[FT_THREADS / ICPMI_WAVE], bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int sc = pair_src[b], tc = pair_tgt[b];
    double* rec = records + (size_t)b * ICPMI_FTREC_DOUBLES;
    int32_t* counts = out_counts ? out_counts + (size_t)b * n_iter : nullptr;
    int n = ft_clamp_kp(match_cnt[b], kp_stride);
    if (tid == 0) bad = 0;
    __syncthreads();
    {   // the matched keypoints' coordinates, features.py:133-134
        // (bounded by the slots alone, without ft_clamp_kp's FT_MAX_KP: the single-stage entry admits any kp_stride and any count)
        const int ns_kp = min(src.kp_cnt[sc], kp_stride), nt_kp = min(tgt.kp_cnt[tc], kp_stride);
        const int rows_s = ft_rows(src.off, src.cnt, sc), rows_t = ft_rows(tgt.off, tgt.cnt, tc);
        const double2* Ps = reinterpret_cast<const double2*>(src.pts) + src.off[sc];
        const double2* Pt = reinterpret_cast<const double2*>(tgt.pts) + tgt.off[tc];
        for (int m = tid; m < n; m += FT_THREADS) {
            const int ms = matches[((size_t)b * kp_stride + m) * 2], mt = matches[((size_t)b * kp_stride + m) * 2 + 1];
            int rs = -1, rt = -1;
            if (ms >= 0 && ms < ns_kp) rs = src.kp[(size_t)sc * kp_stride + ms];
            if (mt >= 0 && mt < nt_kp) rt = tgt.kp[(size_t)tc * kp_stride + mt];
            if (rs < 0 || rs >= rows_s || rt < 0 || rt >= rows_t) { atomicOr(&bad, 1); continue; }
            S[m] = Ps[rs]; D[m] = Pt[rt];
        }
    }
    __syncthreads();
    if (bad) n = 0;                                                 // a match outside the keypoint lists: no alignment
    if (n < 2) {                                                    // features.py:130-131 (uniform per workgroup)
        for (int h = tid; counts && h < n_iter; h += FT_THREADS) counts[h] = 0;
        if (tid == 0) {
            for (int q = 0; q < ICPMI_FTREC_DOUBLES; ++q) rec[q] = 0.0;
            ft_write_no_alignment(rec);
            rec[ICPMI_FTREC_MATCHES] = (double)n; rec[ICPMI_FTREC_STATUS] = (double)ICPMI_FT_ST_FEW_MATCHES;
        }
        return;
    }
    const size_t hyp_base = (size_t)b * (size_t)hyp_pair_stride;
    int bc = 0, bh = 0x7fffffff;                                    // best_inliers = 0: a count of 0 never replaces the identity
    for (int h = tid; h < n_iter; h += FT_THREADS) {
        int i, j, c = 0;
        if (ft_hypothesis(hyp_idx, hyp_u, hyp_base + h, n, i, j)) {
            const FtRigid g = ft_rigid2(S[i], S[j], D[i], D[j]);
            for (int m = 0; m < n; ++m) c += ft_err(g, S[m], D[m]) < thresh ? 1 : 0;   // features.py:146-147
        }
        if (counts) counts[h] = c;
        if (c > bc) { bc = c; bh = h; }                             // ascending h per thread: the first of equal counts stays
    }
    // the first hypothesis with the largest count, features.py:148 (strict >)
    const auto more = [](int a, int b) { return a > b; };
    wave_first_best(bc, bh, more);
    if (lane_id() == 0) { red_cnt[wave_id()] = bc; red_idx[wave_id()] = bh; }
    __syncthreads();
    if (wave_id() != 0) return;                                     // the refit is one wave's work
    bc = red_cnt[0]; bh = red_idx[0];
    for (int w = 1; w < FT_THREADS / ICPMI_WAVE; ++w) take_first_best(bc, bh, red_cnt[w], red_idx[w], more);
    FtRigid g;
    g.r[0] = 1.0; g.r[1] = 0.0; g.r[2] = 0.0; g.r[3] = 1.0; g.tx = 0.0; g.ty = 0.0;
    int inl = 0;
    if (bc > 0) {
        int i, j;
        (void)ft_hypothesis(hyp_idx, hyp_u, hyp_base + bh, n, i, j);
        g = ft_rigid2(S[i], S[j], D[i], D[j]);
        inl = bc;
    }
    if (bc >= 2) {                                                  // features.py:153-158: refit on the inliers of the best
        const int lane = lane_id();
        double k = 0.0, sx = 0.0, sy = 0.0, dx = 0.0, dy = 0.0;
        for (int m = lane; m < n; m += ICPMI_WAVE)
            if (ft_err(g, S[m], D[m]) < thresh) { k += 1.0; sx += S[m].x; sy += S[m].y; dx += D[m].x; dy += D[m].y; }
        k = wave_sum(k); sx = wave_sum(sx) / k; sy = wave_sum(sy) / k; dx = wave_sum(dx) / k; dy = wave_sum(dy) / k;
        double W[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = lane; m < n; m += ICPMI_WAVE)
            if (ft_err(g, S[m], D[m]) < thresh) {
                const double px = S[m].x - sx, py = S[m].y - sy, qx = D[m].x - dx, qy = D[m].y - dy;
                W[0] += px * qx; W[1] += px * qy; W[2] += py * qx; W[3] += py * qy;
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) W[q] = wave_sum(W[q]);
        if (k >= 2.0) {
            kabsch2(W, g.r);
            g.tx = dx - (g.r[0] * sx + g.r[1] * sy);
            g.ty = dy - (g.r[2] * sx + g.r[3] * sy);
            inl = (int)k;
        }
    }
    if (lane_id() == 0) {
        for (int q = 0; q < ICPMI_FTREC_DOUBLES; ++q) rec[q] = 0.0;
        rec[ICPMI_FTREC_MATCHES] = (double)n; rec[ICPMI_FTREC_INLIERS] = (double)inl;
        rec[ICPMI_FTREC_R] = g.r[0]; rec[ICPMI_FTREC_R + 1] = g.r[1]; rec[ICPMI_FTREC_R + 2] = g.r[2]; rec[ICPMI_FTREC_R + 3] = g.r[3];
        rec[ICPMI_FTREC_T] = g.tx; rec[ICPMI_FTREC_T + 1] = g.ty;
        rec[ICPMI_FTREC_STATUS] = (double)ICPMI_FT_ST_OK; rec[ICPMI_FTREC_BEST] = bc > 0 ? (double)bh : -1.0;
    }
}

// ── the chain: feature_based_alignment for every pair (features.py:247-315 inside slam.py:68-88) ─────────────────
// With a start per pair (slam.py:69-71) every pair has its own source, `source @ R_init.T + t_init`: the work set is
// the caller's clouds followed by one transformed copy of its source per pair.
__global__ void ft_work_offsets_kernel(const int32_t* __restrict__ off, int n_clouds, const int32_t* __restrict__ pair_src, int n_pairs,
                                       int32_t* __restrict__ work_off, int32_t* __restrict__ work_src) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    for (int c = tid; c <= n_clouds; c += blockDim.x) work_off[c] = off[c];
    int run = off[n_clouds];                                        // the same in every thread
    for (int b0 = 0; b0 < n_pairs; b0 += blockDim.x) {              // uniform trip count
        const int b = b0 + tid;
        const int rows = b < n_pairs ? off[pair_src[b] + 1] - off[pair_src[b]] : 0;
        part[tid] = rows;
        __syncthreads();
        for (int o = 1; o < (int)blockDim.x; o <<= 1) {             // inclusive scan
            const int v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (b < n_pairs) { work_off[n_clouds + b + 1] = run + part[tid]; work_src[b] = n_clouds + b; }
        run += part[blockDim.x - 1];
        __syncthreads();
    }
}

// copy b of the work set (its cloud first_copy + b) = rows of cloud pair_src[b] of the raw set @ R_init.T + t_init.  NumPy's
// (n, 2) @ (2, 2) is a BLAS gemm whose element is fma(y, R[c][1], x * R[c][0]) (rotsearch.hip, the refinement, has the
// same product) — for every row count: the source is transformed as the (n, 2) array it is
__global__ __launch_bounds__(FT_THREADS) void ft_transform_kernel(const double* __restrict__ raw_pts, const int32_t* __restrict__ raw_off,
                                                                  double* __restrict__ work_pts, const int32_t* __restrict__ work_off,
                                                                  int first_copy, const int32_t* __restrict__ pair_src,
                                                                  const double* __restrict__ init) {
    const int b = blockIdx.x;
    const int sc = pair_src[b];
    const int room = work_off[first_copy + b + 1] - work_off[first_copy + b];
    const int rows = min(raw_off[sc + 1] - raw_off[sc], room);      // equal for a well-formed call
    const double2* src = reinterpret_cast<const double2*>(raw_pts) + raw_off[sc];
    double2* dst = reinterpret_cast<double2*>(work_pts) + work_off[first_copy + b];
    const double* r = init + (size_t)b * 6;
    for (int i = threadIdx.x; i < rows; i += FT_THREADS) {
        const double2 p = src[i];
        dst[i] = make_double2(__builtin_fma(p.y, r[1], p.x * r[0]) + r[4], __builtin_fma(p.y, r[3], p.x * r[2]) + r[5]);
    }
}

// the record of a pair, with the early returns of features.py:281-300 in the reference's order, and the start of the ICP
// that follows (slam.py:83-88)
__global__ void ft_finish_kernel(const FtSide src, const FtSide tgt, const int32_t* __restrict__ work_src,
                                 const int32_t* __restrict__ pair_tgt, int n_pairs, int min_inliers, const double* __restrict__ init_in,
                                 double* __restrict__ init_out, double* __restrict__ records) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_pairs) return;
    const int sc = work_src[b], tc = pair_tgt[b];
    double* rec = records + (size_t)b * ICPMI_FTREC_DOUBLES;
    const int ns = src.cnt[sc], nt = tgt.cnt[tc];
    int status = (int)rec[ICPMI_FTREC_STATUS];                            // the RANSAC kernel's: ok, or fewer than 2 matches
    if (ns > FT_MAX_ROWS || nt > FT_MAX_ROWS || ns < 0 || nt < 0) status = ICPMI_FT_ST_CAPACITY;
    else if (ns < 10 || nt < 10) status = ICPMI_FT_ST_FEW_ROWS;           // features.py:281-282
    else if (src.kp_cnt[sc] < 2 || tgt.kp_cnt[tc] < 2) status = ICPMI_FT_ST_FEW_KP;   // features.py:290-291
    else if (src.desc_len[sc] != tgt.desc_len[tc]) status = ICPMI_FT_ST_DESC_LEN;
    rec[ICPMI_FTREC_NS] = (double)ns; rec[ICPMI_FTREC_NT] = (double)nt;
    const bool looked = status != ICPMI_FT_ST_CAPACITY && status != ICPMI_FT_ST_FEW_ROWS;      // else the reference never extracts keypoints
    rec[ICPMI_FTREC_KPS] = looked ? (double)src.kp_cnt[sc] : 0.0; rec[ICPMI_FTREC_KPT] = looked ? (double)tgt.kp_cnt[tc] : 0.0;
    if (status != ICPMI_FT_ST_OK) {
        if (status != ICPMI_FT_ST_FEW_MATCHES) rec[ICPMI_FTREC_MATCHES] = 0.0;
        ft_write_no_alignment(rec);
    }
    rec[ICPMI_FTREC_STATUS] = (double)status;
    if (!init_out) return;
    double o[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
    if (init_in)
        for (int q = 0; q < 6; ++q) o[q] = init_in[(size_t)b * 6 + q];
    if (status == ICPMI_FT_ST_OK && (int)rec[ICPMI_FTREC_INLIERS] >= min_inliers) {
        const double f0 = rec[ICPMI_FTREC_R], f1 = rec[ICPMI_FTREC_R + 1], f2 = rec[ICPMI_FTREC_R + 2], f3 = rec[ICPMI_FTREC_R + 3];
        const double tx = rec[ICPMI_FTREC_T], ty = rec[ICPMI_FTREC_T + 1];
        if (init_in) {                                              // R_feat @ R_init, t_init @ R_feat.T + t_feat (slam.py:85-86)
            const double i0 = o[0], i1 = o[1], i2 = o[2], i3 = o[3], ix = o[4], iy = o[5];
            o[0] = __builtin_fma(f1, i2, f0 * i0); o[1] = __builtin_fma(f1, i3, f0 * i1);
            o[2] = __builtin_fma(f3, i2, f2 * i0); o[3] = __builtin_fma(f3, i3, f2 * i1);
            o[4] = __builtin_fma(iy, f1, ix * f0) + tx; o[5] = __builtin_fma(iy, f3, ix * f2) + ty;
        } else { o[0] = f0; o[1] = f1; o[2] = f2; o[3] = f3; o[4] = tx; o[5] = ty; }
    }
    for (int q = 0; q < 6; ++q) init_out[(size_t)b * 6 + q] = o[q];
}

// ── what the two chains share on the host ────────────────────────────────────────────────────────────────────────
// keypoint slots per cloud: top_n rounded up to 8
static int ft_kp_stride(int top_n) { return top_n <= 0 ? 8 : (top_n + 7) / 8 * 8; }

static FtSide ft_side(const FtTables& t) { return FtSide{t.pts, t.off, t.cnt, t.kp, t.kp_cnt, t.desc, t.desc_len}; }

// The cloud-side limits, stated once: the batch chain checks its arguments with it, a store its own configuration, a
// single-stage entry its subset (the fields it does not have take values that pass).
static int ft_cfg_check(const FtCloudCfg& c, int kp_stride) {
    if (!(c.voxel_size > 0.0) || c.k_curvature < 0 || c.k_descriptor < 0 || kp_stride <= 0) return ICPMI_ERR_ARG;
    if (c.k_curvature > FT_MAX_K || c.k_descriptor > FT_MAX_K || c.top_n > FT_MAX_KP || c.top_n > kp_stride) return ICPMI_ERR_UNSUPPORTED;
    return ICPMI_OK;
}
int ft_store_check(const icpmi_feature_store* s) {
    if (!s || !s->vox || !s->curv || !s->cnt || !s->kp || !s->kp_cnt || !s->desc || !s->desc_len) return ICPMI_ERR_ARG;
    return ft_cfg_check(ft_store_cfg(s), s->kp_stride);
}

// The workspace of a chain call, described once.  The work set — the clouds the per-cloud stages run on — is `front` clouds
// of the caller's (the batch chain: all of them, the resident chain: none, its targets are in the store) followed, with a
// start per pair, by one transformed copy of its source per pair (room for max_n rows each).
// matches | their counts | the work set's raw rows, its offsets, the source of every pair in it (with a start only: without
// one the caller's arrays are the work set) | its tables: filtered rows, counts, curvature, keypoints, their counts,
// descriptors, their lengths | voxel scratch.  A work set of no clouds has none of the last two.
struct FtWs {
    Carve c;
    int32_t front_rows, front_clouds, max_n, n_pairs, kp_stride, with_init;
    size_t work_clouds = (size_t)front_clouds + (with_init ? (size_t)n_pairs : 0);
    size_t work_rows = (size_t)front_rows + (with_init ? (size_t)n_pairs * (size_t)max_n : 0);
    int32_t* matches = c.take<int32_t>((size_t)n_pairs * kp_stride * 8);
    int32_t* match_cnt = c.take<int32_t>((size_t)n_pairs * 4);
    double* raw = c.take<double>(with_init ? work_rows * 16 : 0);
    int32_t* off = c.take<int32_t>(with_init ? (work_clouds + 1) * 4 : 0);
    int32_t* pair_work = c.take<int32_t>(with_init ? (size_t)n_pairs * 4 : 0);
    FtTables work{c.take<double>(work_rows * 16), off, c.take<int32_t>(work_clouds * 4), c.take<double>(work_rows * 8),
                  c.take<int32_t>(work_clouds * kp_stride * 4), c.take<int32_t>(work_clouds * 4),
                  c.take<double>(work_clouds * kp_stride * FT_DESC_STRIDE * 8), c.take<int32_t>(work_clouds * 4), kp_stride};
    size_t vws_bytes = work_clouds ? icpmi_voxel_workspace_bytes(max_n) : 0;
    void* vws = c.take<void>(vws_bytes);
    size_t bytes = c.off + 256;
};

// What a chain call starts, read off its workspace description (no HIP call): the grid of every stage.
struct FtPlan {
    int work_clouds;          // clouds of the work set: one workgroup each in the per-cloud stages (0: those do not run)
    int kp_stride;
    int pair_grid;            // one workgroup per pair: transform, matching, RANSAC
    int finish_grid;          // a thread per pair
};
static FtPlan plan_features(const FtWs& w) {
    return FtPlan{(int)w.work_clouds, w.kp_stride, w.n_pairs, (w.n_pairs + FT_THREADS - 1) / FT_THREADS};
}

static bool ft_stage_args_ok(const void* pts, const void* off, int n_sel) { return pts && off && n_sel >= 0; }

// the per-cloud stages on the clouds cloud_ids[0 .. n_sel) of a set (the callers have checked their arguments; n_sel > 0)
static int ft_launch_curvature(const double* pts, const int32_t* off, const int32_t* cnt, const int32_t* cloud_ids, int n_sel, int k,
                               double* out_curv, hipStream_t st) {
    ft_curvature_kernel<<<n_sel, FT_THREADS, 0, st>>>(pts, off, cnt, cloud_ids, k, out_curv);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
static int ft_launch_keypoints(const double* pts, const int32_t* off, const int32_t* cnt, const int32_t* cloud_ids, int n_sel,
                               const double* curv, const int32_t* order, int top_n, double min_dist, int32_t* out_kp, int32_t* out_kp_cnt,
                               int kp_stride, hipStream_t st) {
    ft_keypoints_kernel<<<n_sel, ICPMI_WAVE, 0, st>>>(pts, off, cnt, cloud_ids, curv, order, top_n, min_dist, out_kp, out_kp_cnt, kp_stride);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
static int ft_launch_descriptors(const double* pts, const int32_t* off, const int32_t* cnt, const int32_t* cloud_ids, int n_sel,
                                 const int32_t* kp, const int32_t* kp_cnt, int kp_stride, int k, double* out_desc, int32_t* out_desc_len,
                                 hipStream_t st) {
    ft_descriptors_kernel<<<n_sel, FT_THREADS, 0, st>>>(pts, off, cnt, cloud_ids, kp, kp_cnt, kp_stride, k, out_desc, out_desc_len);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// the per-cloud half of both chains and of a history's feature store (features.hpp)
int ft_cloud_stages(const FtTables& t, const double* raw, const int32_t* off_host, int first, int n, const int32_t* cloud_ids,
                    const FtCloudCfg& cfg, void* vws, size_t vws_bytes, hipStream_t st) {
    int rc = icpmi_voxel_downsample_batch(raw, t.off + first, off_host + first, n, 2, cfg.voxel_size, t.pts, t.cnt + first, vws, vws_bytes, st);
    if (rc != ICPMI_OK) return rc;
    rc = ft_launch_curvature(t.pts, t.off, t.cnt, cloud_ids, n, cfg.k_curvature, t.curv, st);
    if (rc != ICPMI_OK) return rc;
    rc = ft_launch_keypoints(t.pts, t.off, t.cnt, cloud_ids, n, t.curv, nullptr, cfg.top_n, cfg.min_kp_dist, t.kp, t.kp_cnt, t.kp_stride, st);
    if (rc != ICPMI_OK) return rc;
    return ft_launch_descriptors(t.pts, t.off, t.cnt, cloud_ids, n, t.kp, t.kp_cnt, t.kp_stride, cfg.k_descriptor, t.desc, t.desc_len, st);
}

// ── the work set ─────────────────────────────────────────────────────────────────────────────────────────────────
// The clouds the per-cloud stages of a chain call run on: raw rows, the host mirror of t.off, the source of every pair in
// the set, and the set's tables.  Without a start it is the caller's own set on the workspace's tables.
struct FtWorkSet {
    const double* raw;
    const int32_t* off_host;
    const int32_t* pair_src;
    FtTables t;
};
// With a start per pair, `set` — the raw set on entry — becomes `front` of its clouds as they are (copied) followed by
// `source @ R_init.T + t_init` of every pair's source, laid out by ft_work_offsets_kernel's rule; off_host receives the host
// mirror of its offsets.  A source must be a cloud below n_sources with at most max_rows rows that end at or before row
// max_end; with nothing in front the set starts at the raw set's first offset, which must be 0.  Every refusal comes before
// the first HIP call.
static int ft_build_work_set(const FtPlan& plan, const FtWs& w, int front, int n_sources, int max_rows, int max_end,
                             const int32_t* pair_src_host, const double* init, std::vector<int32_t>& off_host, FtWorkSet& set,
                             hipStream_t st) {
    if (front == 0 && set.off_host[0] != 0) return ICPMI_ERR_ARG;
    off_host.assign(set.off_host, set.off_host + front + 1);
    for (int b = 0; b < plan.pair_grid; ++b) {
        const int sc = pair_src_host[b];
        if (sc < 0 || sc >= n_sources) return ICPMI_ERR_ARG;
        const int rows = set.off_host[sc + 1] - set.off_host[sc];
        if (rows < 0 || rows > max_rows || set.off_host[sc + 1] > max_end) return ICPMI_ERR_ARG;
        off_host.push_back(off_host.back() + rows);
    }
    if (front && hipMemcpyAsync(w.raw, set.raw, (size_t)set.off_host[front] * 16, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ICPMI_ERR_HIP;
    ft_work_offsets_kernel<<<1, 1024, 0, st>>>(set.t.off, front, set.pair_src, plan.pair_grid, w.off, w.pair_work);
    ft_transform_kernel<<<plan.pair_grid, FT_THREADS, 0, st>>>(set.raw, set.t.off, w.raw, w.off, front, set.pair_src, init);
    ICPMI_LAUNCH_CHECK();
    set = FtWorkSet{w.raw, off_host.data(), w.pair_work, w.work};
    return ICPMI_OK;
}

// ── the pair stages ──────────────────────────────────────────────────────────────────────────────────────────────
// over two sides (the callers have checked their arguments; n_pairs > 0)
static int ft_launch_match(const FtSide& src, const FtSide& tgt, int kp_stride, const int32_t* pair_src, const int32_t* pair_tgt, int n_pairs,
                           double ratio_sq, int32_t* out_matches, int32_t* out_match_cnt, hipStream_t st) {
    ft_match_kernel<<<n_pairs, FT_MAX_KP, 0, st>>>(src, tgt, kp_stride, pair_src, pair_tgt, ratio_sq, out_matches, out_match_cnt);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
static int ft_launch_ransac(const FtSide& src, const FtSide& tgt, int kp_stride, const int32_t* pair_src, const int32_t* pair_tgt, int n_pairs,
                            const int32_t* matches, const int32_t* match_cnt, const int32_t* hyp_idx, const double* hyp_u, int n_iter,
                            int hyp_pair_stride, double inlier_thresh, double* out_records, int32_t* out_counts, hipStream_t st) {
    ft_ransac_kernel<<<n_pairs, FT_THREADS, 0, st>>>(src, tgt, kp_stride, pair_src, pair_tgt, matches, match_cnt, hyp_idx, hyp_u, n_iter,
                                                     hyp_pair_stride, inlier_thresh, out_records, out_counts);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// matching, RANSAC and the record of every pair: the second half of both chains
struct FtPairArgs {
    const int32_t* pair_src;      // the source of pair b in the source side's tables
    const int32_t* pair_tgt;
    int n_pairs;
    double ratio_sq;
    const int32_t* hyp_idx;
    const double* hyp_u;
    int n_iter, hyp_pair_stride;
    double inlier_thresh;
    int min_inliers;
    const double* init_in;
    double* init_out;
    double* out_records;
};
static int ft_pair_stages(const FtPlan& plan, const FtSide& src, const FtSide& tgt, const FtPairArgs& a, int32_t* matches, int32_t* match_cnt,
                          hipStream_t st) {
    int rc = ft_launch_match(src, tgt, plan.kp_stride, a.pair_src, a.pair_tgt, a.n_pairs, a.ratio_sq, matches, match_cnt, st);
    if (rc != ICPMI_OK) return rc;
    rc = ft_launch_ransac(src, tgt, plan.kp_stride, a.pair_src, a.pair_tgt, a.n_pairs, matches, match_cnt, a.hyp_idx, a.hyp_u, a.n_iter,
                          a.hyp_pair_stride, a.inlier_thresh, a.out_records, nullptr, st);
    if (rc != ICPMI_OK) return rc;
    ft_finish_kernel<<<plan.finish_grid, FT_THREADS, 0, st>>>(src, tgt, a.pair_src, a.pair_tgt, a.n_pairs, a.min_inliers, a.init_in, a.init_out,
                                                             a.out_records);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

}  // namespace icpmi

// ── the single-stage entry points: argument check, then the chain's launcher ─────────────────────────────────────────
extern "C" int icpmi_feature_curvature_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                             const int32_t* cloud_ids, int32_t n_sel, int32_t k, double* out_curvature,
                                             void* stream) {
    using namespace icpmi;
    if (!ft_stage_args_ok(pts, off_dev, n_sel) || !out_curvature) return ICPMI_ERR_ARG;
    const int rc = ft_cfg_check(FtCloudCfg{1.0, k, 0, 0.0, 0}, 1);
    if (rc != ICPMI_OK || n_sel == 0) return rc;
    return ft_launch_curvature(pts, off_dev, cnt_dev, cloud_ids, n_sel, k, out_curvature, (hipStream_t)stream);
}

extern "C" int icpmi_feature_keypoints_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                             const int32_t* cloud_ids, int32_t n_sel, const double* curvature,
                                             const int32_t* order, int32_t top_n, double min_dist, int32_t* out_kp,
                                             int32_t* out_kp_cnt, int32_t kp_stride, void* stream) {
    using namespace icpmi;
    if (!ft_stage_args_ok(pts, off_dev, n_sel) || (!curvature && !order) || !out_kp || !out_kp_cnt) return ICPMI_ERR_ARG;
    const int rc = ft_cfg_check(FtCloudCfg{1.0, 0, top_n, min_dist, 0}, kp_stride);
    if (rc != ICPMI_OK || n_sel == 0) return rc;
    return ft_launch_keypoints(pts, off_dev, cnt_dev, cloud_ids, n_sel, curvature, order, top_n, min_dist, out_kp, out_kp_cnt, kp_stride,
                               (hipStream_t)stream);
}

extern "C" int icpmi_feature_descriptors_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev,
                                               const int32_t* cloud_ids, int32_t n_sel, const int32_t* kp, const int32_t* kp_cnt,
                                               int32_t kp_stride, int32_t k, double* out_desc, int32_t* out_desc_len, void* stream) {
    using namespace icpmi;
    if (!ft_stage_args_ok(pts, off_dev, n_sel) || !kp || !kp_cnt || !out_desc || !out_desc_len) return ICPMI_ERR_ARG;
    const int rc = ft_cfg_check(FtCloudCfg{1.0, 0, 0, 0.0, k}, kp_stride);
    if (rc != ICPMI_OK || n_sel == 0) return rc;
    return ft_launch_descriptors(pts, off_dev, cnt_dev, cloud_ids, n_sel, kp, kp_cnt, kp_stride, k, out_desc, out_desc_len,
                                 (hipStream_t)stream);
}

extern "C" int icpmi_feature_match_batch(const double* desc, const int32_t* desc_len, const int32_t* kp_cnt, int32_t kp_stride,
                                         const int32_t* pair_src, const int32_t* pair_tgt, int32_t n_pairs, double ratio_sq,
                                         int32_t* out_matches, int32_t* out_match_cnt, void* stream) {
    using namespace icpmi;
    if (!desc || !desc_len || !kp_cnt || !pair_src || !pair_tgt || !out_matches || !out_match_cnt || kp_stride <= 0 || n_pairs < 0)
        return ICPMI_ERR_ARG;
    if (n_pairs == 0) return ICPMI_OK;
    const FtSide side{nullptr, nullptr, nullptr, nullptr, kp_cnt, desc, desc_len};
    return ft_launch_match(side, side, kp_stride, pair_src, pair_tgt, n_pairs, ratio_sq, out_matches, out_match_cnt, (hipStream_t)stream);
}

extern "C" int icpmi_feature_ransac_batch(const double* pts, const int32_t* off_dev, const int32_t* cnt_dev, const int32_t* kp,
                                          const int32_t* kp_cnt, int32_t kp_stride, const int32_t* pair_src, const int32_t* pair_tgt,
                                          int32_t n_pairs, const int32_t* matches, const int32_t* match_cnt, const int32_t* hyp_idx,
                                          const double* hyp_u, int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh,
                                          double* out_records, int32_t* out_counts, void* stream) {
    using namespace icpmi;
    if (!pts || !off_dev || !kp || !kp_cnt || !pair_src || !pair_tgt || !matches || !match_cnt || !out_records) return ICPMI_ERR_ARG;
    if (kp_stride <= 0 || n_pairs < 0 || n_iter < 0 || hyp_pair_stride < 0 || (n_iter > 0 && !hyp_idx == !hyp_u)) return ICPMI_ERR_ARG;
    if (n_pairs == 0) return ICPMI_OK;
    const FtSide side{pts, off_dev, cnt_dev, kp, kp_cnt, nullptr, nullptr};
    return ft_launch_ransac(side, side, kp_stride, pair_src, pair_tgt, n_pairs, matches, match_cnt, hyp_idx, hyp_u, n_iter, hyp_pair_stride,
                            inlier_thresh, out_records, out_counts, (hipStream_t)stream);
}

// ── the chain: feature_based_alignment for every pair (features.py:247-315 inside slam.py:68-88) ─────────────────
extern "C" size_t icpmi_feature_align_batch_workspace_bytes(int32_t total_rows, int32_t n_clouds, int32_t max_n, int32_t n_pairs,
                                                            int32_t top_n, int32_t with_init) {
    if (total_rows < 0 || n_clouds < 0 || max_n < 0 || n_pairs < 0) return 0;
    return icpmi::FtWs{nullptr, total_rows, n_clouds, max_n, n_pairs, icpmi::ft_kp_stride(top_n), with_init ? 1 : 0}.bytes;
}

extern "C" int icpmi_feature_align_batch(const double* pts, const int32_t* off_dev, const int32_t* off_host, int32_t n_clouds,
                                         const int32_t* pair_src, const int32_t* pair_src_host, const int32_t* pair_tgt,
                                         int32_t n_pairs, double voxel_size, int32_t k_curvature, int32_t top_n, double min_kp_dist,
                                         int32_t k_descriptor, double ratio_sq, const int32_t* hyp_idx, const double* hyp_u,
                                         int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh, int32_t min_inliers,
                                         const double* init_in, double* init_out, double* out_records,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (!pts || !off_dev || !off_host || !pair_src || !pair_tgt || !out_records || !workspace) return ICPMI_ERR_ARG;
    if (n_clouds <= 0 || n_pairs < 0 || n_iter < 0 || hyp_pair_stride < 0) return ICPMI_ERR_ARG;
    if (n_iter > 0 && !hyp_idx == !hyp_u) return ICPMI_ERR_ARG;
    if (init_in && !pair_src_host) return ICPMI_ERR_ARG;
    const FtCloudCfg cfg{voxel_size, k_curvature, top_n, min_kp_dist, k_descriptor};
    int rc = ft_cfg_check(cfg, ft_kp_stride(top_n));
    if (rc != ICPMI_OK || n_pairs == 0) return rc;
    int max_n, total_rows;
    if (!cloud_rows(off_host, n_clouds, max_n, total_rows)) return ICPMI_ERR_ARG;
    const FtWs w{workspace, total_rows, n_clouds, max_n, n_pairs, ft_kp_stride(top_n), init_in ? 1 : 0};
    if (workspace_bytes < w.bytes) return ICPMI_ERR_WORKSPACE;
    const FtPlan plan = plan_features(w);
    hipStream_t st = (hipStream_t)stream;
    // the work set: the caller's clouds as they are, or followed by a transformed source per pair
    FtWorkSet set{pts, off_host, pair_src, w.work};
    set.t.off = off_dev;
    std::vector<int32_t> work_off_host;
    if (init_in) rc = ft_build_work_set(plan, w, n_clouds, n_clouds, max_n, total_rows, pair_src_host, init_in, work_off_host, set, st);
    if (rc != ICPMI_OK) return rc;
    rc = ft_cloud_stages(set.t, set.raw, set.off_host, 0, plan.work_clouds, nullptr, cfg, w.vws, w.vws_bytes, st);
    if (rc != ICPMI_OK) return rc;
    const FtSide side = ft_side(set.t);                             // sources and targets: clouds of the one work set
    const FtPairArgs a{set.pair_src, pair_tgt, n_pairs, ratio_sq, hyp_idx, hyp_u, n_iter, hyp_pair_stride, inlier_thresh, min_inliers,
                       init_in, init_out, out_records};
    return ft_pair_stages(plan, side, side, a, w.matches, w.match_cnt, st);
}

// ── the resident chain: the pair half of icpmi_feature_align_batch on a history's feature store ──────────────────────
// Without a start the sources are clouds of the store as the targets are; with one they are a work set with no clouds in
// front, which goes through the per-cloud half here, with the store's configuration.
extern "C" size_t icpmi_history_feature_align_workspace_bytes(int32_t n_pairs, int32_t max_n, int32_t top_n, int32_t with_init) {
    if (n_pairs < 0 || max_n < 0) return 0;
    return icpmi::FtWs{nullptr, 0, 0, max_n, n_pairs, icpmi::ft_kp_stride(top_n), with_init ? 1 : 0}.bytes;
}

extern "C" int icpmi_history_feature_align(const icpmi_history* h, const icpmi_feature_store* s, const int32_t* off_host,
                                           const int32_t* pair_src, const int32_t* pair_src_host, const int32_t* pair_tgt,
                                           int32_t n_pairs, int32_t max_n, double ratio_sq, const int32_t* hyp_idx, const double* hyp_u,
                                           int32_t n_iter, int32_t hyp_pair_stride, double inlier_thresh, int32_t min_inliers,
                                           const double* init_in, double* init_out, double* out_records, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (!h || !h->pts || !h->off_dev || !h->ids || h->scan_capacity <= 0 || h->row_capacity <= 0) return ICPMI_ERR_ARG;
    if (n_pairs < 0 || max_n < 0 || n_iter < 0 || hyp_pair_stride < 0) return ICPMI_ERR_ARG;
    int rc = ft_store_check(s);
    if (rc != ICPMI_OK || n_pairs == 0) return rc;
    if (!pair_src || !pair_tgt || !out_records || !workspace) return ICPMI_ERR_ARG;
    if (n_iter > 0 && !hyp_idx == !hyp_u) return ICPMI_ERR_ARG;
    if (init_in && (!pair_src_host || !off_host)) return ICPMI_ERR_ARG;
    if (s->kp_stride != ft_kp_stride(s->top_n)) return ICPMI_ERR_ARG;              // the work set's tables share the store's stride
    const FtWs w{workspace, 0, 0, max_n, n_pairs, s->kp_stride, init_in ? 1 : 0};
    if (workspace_bytes < w.bytes) return ICPMI_ERR_WORKSPACE;
    const FtPlan plan = plan_features(w);
    hipStream_t st = (hipStream_t)stream;
    const FtTables store_tables = ft_store_tables(h, s);
    const FtSide store = ft_side(store_tables);
    FtPairArgs a{pair_src, pair_tgt, n_pairs, ratio_sq, hyp_idx, hyp_u, n_iter, hyp_pair_stride, inlier_thresh, min_inliers,
                 init_in, init_out, out_records};
    if (!init_in) return ft_pair_stages(plan, store, store, a, w.matches, w.match_cnt, st);
    FtWorkSet set{h->pts, off_host, pair_src, store_tables};                        // the history's raw set, before it is built
    std::vector<int32_t> work_off_host;
    rc = ft_build_work_set(plan, w, 0, h->scan_capacity, max_n, h->row_capacity, pair_src_host, init_in, work_off_host, set, st);
    if (rc != ICPMI_OK) return rc;
    rc = ft_cloud_stages(set.t, set.raw, set.off_host, 0, plan.work_clouds, nullptr, ft_store_cfg(s), w.vws, w.vws_bytes, st);
    if (rc != ICPMI_OK) return rc;
    a.pair_src = set.pair_src;
    return ft_pair_stages(plan, ft_side(set.t), store, a, w.matches, w.match_cnt, st);
}
