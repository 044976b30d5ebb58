// prep.hip — prepare target clouds for the sweep search, and K4 normals on top.
//
// Per target cloud (one workgroup): pick the sort axis, sort the points along
// it in LDS, publish the sorted copy (points, original rows, axis) for the
// fused ICP kernel, and — for point_to_line — estimate_normals_2d (reference
// utilities/icp.py:51-76) by an outward sweep from every point's own sorted
// position, which is an exact k-NN search (see sweep.hpp).
#include <vector>

#include "prep_common.hpp"

namespace icpmi {

#ifndef PREP_AXIS_STEP
#define PREP_AXIS_STEP 4        // large batches estimate the search axis on every PREP_AXIS_STEP-th point
#endif
#ifndef ICPMI_PREP_WPS
#define ICPMI_PREP_WPS 6      // waves per SIMD the k-NN kernel is compiled for up to KK = 13: three workgroups per CU
#endif
constexpr int PREP_THREADS = 512;
constexpr int PREP_MAXW = PREP_THREADS / ICPMI_WAVE;
constexpr int PREP_MAX_POINTS = 4096;   // sorted copy + sort scratch stay in LDS (PrepLds)

// Dynamic LDS of prep_targets_kernel, stated once: the kernel takes its pointers from here (lds_points from the launch, npad
// from its own cloud), the launcher its size (npad of the largest cloud).  The sorted copy of lds_points rows: xy |
// original row | float32 bearing (bearing order only).  The sort scratch of the cloud's npad slots: behind the copy when the
// grid is built there afterwards (GRID), otherwise ON the copy (the sorted rows pass through registers) — 40 KB instead of
// 64 KB for ~1 500 points, so that the k-NN loops of three workgroups instead of two share a CU.  Up to 4 * PREP_THREADS
// slots the network runs on registers (at least a slot per thread) and the scratch is keys by row | sorted keys | their
// rows; beyond, the pair sort's keys | rows alone.  The grid's cell ends and positions by cell then take the scratch's place.
struct PrepLds {
    size_t sorig_at, sth_at;              // the sorted copy: sxy at 0
    size_t by_row_at, keys_at;            // the sort scratch: keys by row (register sort), then `pairs` = sorted keys | their rows
    size_t cell_end_at, cell_pts_at;      // the grid, in the scratch's place afterwards
    size_t bytes;
    bool reg_sort;
    int nsort, cells_cap;                 // slots of the sort; cells of the grid
    PairSortLds pairs;
    __host__ __device__ PrepLds(int lds_points, int npad, bool grid)
        : reg_sort(npad <= 4 * PREP_THREADS), nsort(reg_sort && npad < PREP_THREADS ? PREP_THREADS : npad),
          cells_cap(2 * npad < 4096 ? 2 * npad : 4096), pairs(nsort) {
        const size_t copy_bytes = (size_t)lds_points * 24;
        sorig_at = (size_t)lds_points * 16;
        sth_at = (size_t)lds_points * 20;
        by_row_at = cell_end_at = grid ? copy_bytes : 0;
        keys_at = by_row_at + (reg_sort ? (size_t)nsort * sizeof(uint64_t) : 0);
        cell_pts_at = cell_end_at + (size_t)cells_cap * sizeof(uint32_t);
        bytes = keys_at + pairs.bytes > copy_bytes ? keys_at + pairs.bytes : copy_bytes;
    }
    template <class T> static __device__ T* at(unsigned char* dyn, size_t o) { return reinterpret_cast<T*>(dyn + o); }
};

// KK = capacity of the per-query neighbour list (0: no normals); GRID: k-NN through a grid instead of the sweep
// Sort of up to E * PREP_THREADS rows by (key, row) on registers; leaves keys[i] / rows[i] = full sortable key and row of
// the i-th smallest, like bitonic_sort_pairs.  by_row, keys: E * PREP_THREADS slots of LDS each; rows: as many.
// Bearing order (round 4): the key is the float32 bearing in 21 bits of fixed point (steps of 2 pi / 2^21 = 3.0e-6 rad)
// with the row below it — ONE 32-bit word per point, the network of the voxel filter instead of the 64-bit one, atan2f
// instead of the float64 atan2 (2.02 -> see DESIGN section 6).  Any order of the points is a correct order for the exact
// searches; what they need is (a) images that do not decrease along the sorted array — the image IS the quantised key —
// and (b) every image within the searches' key slack of the true bearing: the floor 3.0e-6 + the float32 product in
// front of it (up to an eighth of a step at 2^21) + atan2f and its float32 inputs ~1e-6 + the image's own two roundings
// 7e-7 < 5.3e-6 (SweepFQuery::mu = 1e-5 with the query's own atan2f and the subtraction; the normals' walk compares two
// images: 1.6e-5).  Equal keys keep row order; no fix-up.
constexpr float PREP_POLAR_Q = 6.283185307179586f / 2097152.0f;        // 2 pi / 2^21
__device__ __forceinline__ uint32_t prep_polar_key21(double x, double y) {
    const float t = (atan2f((float)y, (float)x) + 3.14159265f) * (2097152.0f / 6.283185307179586f);
    const int k = (int)t;
    return (uint32_t)(k < 0 ? 0 : (k > 2097151 ? 2097151 : k));        // NaN -> 0: any key is a correct key
}
__device__ __forceinline__ float prep_polar_image(uint32_t k21) { return (float)k21 * PREP_POLAR_Q - 3.14159265f; }

// MED3: the network's exchange is one median (sort.hpp).  It costs six registers through the sort, which the leanest
// instantiations do not have below their occupancy step: prep_targets_kernel<0, *> (62 -> 68 VGPRs, 8 -> 7 waves a SIMD)
// and <6, true> (70 -> 76, 7 -> 6) keep min / max / select; every other one is unchanged in registers, scratch and
// occupancy and takes the median.
constexpr bool prep_sort_med3(int kk, bool grid) { return !(kk == 0 || (kk == 6 && grid)); }

template <int E, bool MED3>
__device__ __forceinline__ void prep_sort_polar32(const double* __restrict__ P, int M, uint64_t* keys, uint32_t* rows) {
    uint32_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * PREP_THREADS + (int)threadIdx.x;            // coalesced; any start order sorts the same
        v[e] = i < M ? (prep_polar_key21(P[2 * i], P[2 * i + 1]) << 11) | (uint32_t)i : 0xffffffffu;
    }
    bitonic_sort_regs_fixed<uint32_t, E, PREP_THREADS, MED3>(v, reinterpret_cast<uint32_t*>(keys));
    __syncthreads();                                                   // the network's scratch is the key array written next
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = (int)threadIdx.x * E + e;
        rows[i] = v[e] == 0xffffffffu ? 0xffffffffu : (v[e] & 0x7ffu);
        keys[i] = v[e] == 0xffffffffu ? ~0ull : f64_sortable((double)prep_polar_image(v[e] >> 11));   // the image is the key from here on
    }
    __syncthreads();
}

template <int E, bool MED3>
__device__ __forceinline__ void prep_sort_regs(const double* __restrict__ P, int M, int dir, uint64_t* by_row, uint64_t* keys,
                                               uint32_t* rows) {
    if (dir == SWEEP_POLAR) { prep_sort_polar32<E, MED3>(P, M, keys, rows); return; }
    constexpr uint64_t ROW_MASK = 0x7ff;                               // rows below 2 048
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = (int)threadIdx.x * E + e;
        const uint64_t k = i < M ? f64_sortable(proj(dir, P[2 * i], P[2 * i + 1])) : ~0ull;
        by_row[i] = k;
        v[e] = i < M ? ((k & ~ROW_MASK) | (uint64_t)i) : ~0ull;
    }
    bitonic_sort_regs_fixed<uint64_t, E, PREP_THREADS>(v, keys);       // its LDS stages hold barriers: by_row is complete too
    int bad = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = (int)threadIdx.x * E + e;
        const uint32_t r = v[e] == ~0ull ? 0xffffffffu : (uint32_t)(v[e] & ROW_MASK);
        rows[i] = r;
        keys[i] = r == 0xffffffffu ? ~0ull : by_row[r];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = (int)threadIdx.x * E + e;
        if (i + 1 < M && (keys[i] > keys[i + 1] || (keys[i] == keys[i + 1] && rows[i] > rows[i + 1]))) bad = 1;
    }
    if (__syncthreads_or(bad)) {
        // keys that agree in their upper 53 bits came out in row order: one thread puts such runs in (key, row) order
        if (threadIdx.x == 0)
            for (int i = 1; i < M; ++i) {
                const uint64_t k = keys[i];
                const uint32_t r = rows[i];
                int j = i - 1;
                while (j >= 0 && (keys[j] > k || (keys[j] == k && rows[j] > r))) { keys[j + 1] = keys[j]; rows[j + 1] = rows[j]; --j; }
                keys[j + 1] = k; rows[j + 1] = r;
            }
        __syncthreads();
    }
}

template <int KK, bool GRID>
__global__ __launch_bounds__(PREP_THREADS, (KK <= 13 ? ICPMI_PREP_WPS : (KK <= 16 ? 4 : 2))) void prep_targets_kernel(   // three workgroups per CU up to KK = 13, two up to 16
    const double* __restrict__ pts, const int32_t* __restrict__ off, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ cloud_ids, int k, double2* __restrict__ g_sxy, double2* __restrict__ g_snrm,
    int32_t* __restrict__ g_sorig, float* __restrict__ g_skey, int32_t* __restrict__ g_dir, double* __restrict__ out_normals,
    int lds_points, int split, int polar) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ double dsc[8 * PREP_MAXW];
    __shared__ int hist[6 * PREP_BINS];
    // `split` workgroups share one cloud: each repeats the (cheap) axis choice and sort, then takes its
    // slice of the normal queries — small batches would otherwise leave a cloud's k-NN sweeps to one CU
    const int ci = blockIdx.x / split, part = blockIdx.x % split;
    const int c = cloud_ids ? cloud_ids[ci] : ci;
    const int M = cnt ? cnt[c] : off[c + 1] - off[c];
    if (off[c + 1] - off[c] > PREP_MAX_POINTS) return;          // prepared through global memory (prep_big.hip)
    if (M <= 0 || M > lds_points) { if (threadIdx.x == 0) g_dir[c] = -1; return; }
    const double* P = pts + (size_t)off[c] * 2;
    const int npad = sort_npad(M);
    const PrepLds lds(lds_points, npad, GRID);
    double2* sxy = lds.at<double2>(dyn, 0);
    int32_t* sorig = lds.at<int32_t>(dyn, lds.sorig_at);
    float* sth = lds.at<float>(dyn, lds.sth_at);
    uint64_t *by_row = lds.at<uint64_t>(dyn, lds.by_row_at), *keys = lds.pairs.keys(dyn + lds.keys_at);
    uint32_t* rows = lds.pairs.rows(dyn + lds.keys_at);

    double bounds[4];
    const int dir = choose_axis<PREP_THREADS>(P, M, dsc, hist, bounds, polar, (!GRID && M >= 512) ? PREP_AXIS_STEP : 1);   // bounds: the grid's
    // ── sort along the chosen axis (or by bearing) ───────────────────────────
    if (lds.reg_sort) {
        // (key, row) as ONE 64-bit element: the key's low 11 bits give way to the row, the network runs on registers
        // (sort.hpp: thread t owns slots t E .. t E + E - 1), and the rare neighbours whose keys agree in the 53 bits
        // that are left are put right afterwards from the full keys — the order is exactly the pair sort's.
        if (lds.nsort == PREP_THREADS) prep_sort_regs<1, prep_sort_med3(KK, GRID)>(P, M, dir, by_row, keys, rows);
        else if (lds.nsort == 2 * PREP_THREADS) prep_sort_regs<2, prep_sort_med3(KK, GRID)>(P, M, dir, by_row, keys, rows);
        else prep_sort_regs<4, prep_sort_med3(KK, GRID)>(P, M, dir, by_row, keys, rows);
    } else {
        for (int i = threadIdx.x; i < npad; i += PREP_THREADS) {
            keys[i] = i < M ? f64_sortable(dir == SWEEP_POLAR ? polar_key(P[2 * i], P[2 * i + 1]) : proj(dir, P[2 * i], P[2 * i + 1])) : ~0ull;
            rows[i] = i < M ? (uint32_t)i : 0xffffffffu;
        }
        __syncthreads();
        bitonic_sort_pairs(keys, rows, npad);
    }
    double2* o_sxy = g_sxy + off[c];
    int32_t* o_sorig = g_sorig + off[c];
    float* o_skey = g_skey + off[c];
    int my_row[PREP_MAX_POINTS / PREP_THREADS];
    float my_key[PREP_MAX_POINTS / PREP_THREADS];          // float32 image of the sort key (the bearing: one atan2 per point in all)
#pragma unroll
    for (int u = 0; u < PREP_MAX_POINTS / PREP_THREADS; ++u) {
        const int i = u * PREP_THREADS + (int)threadIdx.x;
        my_row[u] = i < M ? (int)rows[i] : 0;
        my_key[u] = i < M ? (float)f64_unsortable(keys[i]) : 0.0f;
    }
    __syncthreads();                                             // the scratch may be the memory written next
#pragma unroll
    for (int u = 0; u < PREP_MAX_POINTS / PREP_THREADS; ++u) {
        const int i = u * PREP_THREADS + (int)threadIdx.x;
        if (i < M) {
            const int row = my_row[u];
            const double2 p = make_double2(P[2 * row], P[2 * row + 1]);
            sxy[i] = p; sorig[i] = row;
            if (KK > 0 && !GRID && dir == SWEEP_POLAR) sth[i] = my_key[u];
            if (part == 0) { o_sxy[i] = p; o_sorig[i] = row; o_skey[i] = my_key[u]; }
        }
    }
    if (threadIdx.x == 0 && part == 0) g_dir[c] = dir;
    __syncthreads();
    if constexpr (KK > 0) {
        const int kc = min(k, M - 1);              // icp.py:61
        const int kk = kc + 1;                     // self included, icp.py:66
        double2* o_snrm = g_snrm + off[c];
        double* o_rows = out_normals ? out_normals + (size_t)off[c] * 2 : nullptr;
        const int per = (M + split - 1) / split;
        if constexpr (GRID) {
            // Few clouds (a single scan pair): the time of the launch is the longest search of any lane, and a
            // grid bounds that far better than a 1-D window (a wall across the sweep axis puts hundreds of
            // points in it).  Built in the LDS the sort has released: cell ends (4 B per cell), then positions
            // by cell.  Same neighbours, same order.
            const PrepGrid grid = prep_grid_build(sxy, M, bounds, kk, lds.at<uint32_t>(dyn, lds.cell_end_at), lds.at<uint16_t>(dyn, lds.cell_pts_at),
                                                   lds.cells_cap, hist);
            prep_normals_grid<KK>(sxy, sorig, M, min(M, part * per), min(M, (part + 1) * per), kk, grid, o_snrm, o_rows);
        } else {
            // Many clouds: every CU is busy, the sum of the work counts, and the sweep has less of it per candidate.
            if (dir == SWEEP_POLAR) prep_normals_polar<KK>(sxy, sorig, sth, M, min(M, part * per), min(M, (part + 1) * per), kk, o_snrm, o_rows);
            else prep_normals<KK>(sxy, sorig, M, min(M, part * per), min(M, (part + 1) * per), dir, kk, o_snrm, o_rows);
        }
    }
}


// estimate_normals_2d for ANY k (the reference accepts every k, icp.py:61; the register lists above stop at 31):
// one wave per query on the sorted copy in global memory.  The k + 1 nearest are drawn one after the other — each
// round every lane scans its share of the cloud for the smallest (distance, row) beyond the last one drawn, and a
// wave reduction picks the overall next — so the neighbours come out in the (distance, row) order every other path
// sums them in: same lists, same arithmetic, same normals.  O(k M / 64) per query: a fallback, not a fast path.
constexpr int ANYK_THREADS = 256;
// first sorted position whose key is >= v (wave-uniform)
__device__ __forceinline__ int anyk_lower_bound(const double2* sxy, int M, int dir, double v) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double2 c = sxy[mid];
        if (proj(dir, c.x, c.y) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(ANYK_THREADS) void normals_anyk_kernel(
    const int32_t* __restrict__ off, const int32_t* __restrict__ cnt, const int32_t* __restrict__ cloud_ids, int k,
    const double2* __restrict__ g_sxy, double2* __restrict__ g_snrm, const int32_t* __restrict__ g_sorig,
    const int32_t* __restrict__ g_dir, double* __restrict__ out_normals, int sel_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    int32_t* sel = reinterpret_cast<int32_t*>(dyn) + (size_t)wave_id() * sel_cap;
    const int c = cloud_ids ? cloud_ids[blockIdx.y] : blockIdx.y;
    const int M = cnt ? min(cnt[c], off[c + 1] - off[c]) : off[c + 1] - off[c];
    const int dir = g_dir[c];
    if (M <= 0 || dir < 0) return;
    const double2* sxy = g_sxy + off[c];
    const int32_t* sorig = g_sorig + off[c];
    double2* o_snrm = g_snrm + off[c];
    double* o_rows = out_normals ? out_normals + (size_t)off[c] * 2 : nullptr;
    const int kk = min(min(k, M - 1) + 1, sel_cap);             // icp.py:61,66: k clamped, self included
    const int lane = lane_id();
    const int waves = gridDim.x * (ANYK_THREADS / ICPMI_WAVE);
    for (int s = blockIdx.x * (ANYK_THREADS / ICPMI_WAVE) + wave_id(); s < M; s += waves) {     // wave-uniform
        const double2 q = sxy[s];
        // Only a window of the sort order can hold the k nearest: the 2 kk + 1 points around the query's own place
        // contain at least kk points, so the kk-th nearest is no farther than the farthest of THEM (R), and every
        // candidate has its key within kappa R of the query's (|du| <= d along x or y, <= sqrt(2) d on the diagonals).
        // A rolling submap of 10 000 points then scans a few hundred per query, not all of them.  (Bearing order: no
        // such bound — the whole cloud, at most 2 048 points.)
        int lo = 0, hi = M;
        if (dir < SWEEP_POLAR) {
            const int a0 = max(0, s - kk), a1 = min(M - 1, s + kk);
            double r2 = 0.0;
            for (int i = a0 + lane; i <= a1; i += ICPMI_WAVE) r2 = fmax(r2, sweep_d2(q.x, q.y, sxy[i]));
            r2 = wave_max(r2);
            if (a1 - a0 + 1 >= kk) {
                const double uq = proj(dir, q.x, q.y);
                const double w = sqrt(r2) * 1.4142135623730951 * 1.000001 + 1e-9 * (1.0 + fabs(uq));
                lo = anyk_lower_bound(sxy, M, dir, uq - w);
                hi = anyk_lower_bound(sxy, M, dir, uq + w + 1e-9 * (1.0 + fabs(uq)));
                hi = min(M, hi + 1);
            }
        }
        double last_d = -1.0;
        int last_row = -1;
        for (int j = 0; j < kk; ++j) {
            double bd = __builtin_inf();
            int brow = 0x7fffffff, bpos = -1;
            for (int i = lo + lane; i < hi; i += ICPMI_WAVE) {
                const double d2 = sweep_d2(q.x, q.y, sxy[i]);
                const int row = sorig[i];
                const bool after = d2 > last_d || (d2 == last_d && row > last_row);
                if (after && (d2 < bd || (d2 == bd && row < brow))) { bd = d2; brow = row; bpos = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(bd, o, ICPMI_WAVE);
                const int orow = __shfl_xor(brow, o, ICPMI_WAVE), opos = __shfl_xor(bpos, o, ICPMI_WAVE);
                if (od < bd || (od == bd && orow < brow)) { bd = od; brow = orow; bpos = opos; }
            }
            last_d = bd; last_row = brow;
            if (lane == 0) sel[j] = bpos;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane == 0) {
            // np.cov over the neighbours in (distance, row) order, eigenvector of the smaller eigenvalue: emit_normal's arithmetic
            double mx = 0.0, my = 0.0;
            for (int j = 0; j < kk; ++j) { const double2 p = sxy[sel[j]]; mx += p.x; my += p.y; }
            mx /= (double)kk; my /= (double)kk;
            double sxx = 0.0, sxy_ = 0.0, syy = 0.0;
            for (int j = 0; j < kk; ++j) {
                const double2 p = sxy[sel[j]];
                const double dx = p.x - mx, dy = p.y - my;
                sxx += dx * dx; sxy_ += dx * dy; syy += dy * dy;
            }
            double vx = 1.0, vy = 0.0;
            if (kk > 1) {
                const double den = (double)(kk - 1);
                smallest_evec_2x2(sxx / den, sxy_ / den, syy / den, vx, vy);
            }
            double nn = sqrt(vx * vx + vy * vy);
            nn = nn < 1e-10 ? 1e-10 : nn;
            const double2 n2 = make_double2(vx / nn, vy / nn);
            o_snrm[s] = n2;
            if (o_rows) { const int row = sorig[s]; o_rows[2 * row] = n2.x; o_rows[2 * row + 1] = n2.y; }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The instantiation of prep_targets_kernel for normals from `normal_k` neighbours, and its list capacity kk.
using PrepKernel = void (*)(const double*, const int32_t*, const int32_t*, const int32_t*, int, double2*, double2*, int32_t*,
                            float*, int32_t*, double*, int, int, int);
struct PrepChoice {
    PrepKernel kernel;
    int kk;                   // 0: sort only
    bool grid;
};
template <int KK>
static PrepChoice prep_choice_of(bool use_grid) {
    if (use_grid && KK > 0) return {prep_targets_kernel<KK, true>, KK, true};       // the grid serves the k-NN search alone
    return {prep_targets_kernel<KK, false>, KK, false};
}
static PrepChoice prep_choice(int normal_k, bool use_grid) {
    // beyond 31 neighbours: sort only, then the any-k kernel on the sorted copy
    if (normal_k > 31) return {prep_targets_kernel<0, false>, 0, false};
    // list capacity = k + 1 exactly for the usual k (5, 10 = reference default, 12 = config.yaml), else the next size up
    if (normal_k < 0) return prep_choice_of<0>(use_grid);
    if (normal_k + 1 <= 6) return prep_choice_of<6>(use_grid);
    if (normal_k + 1 <= 8) return prep_choice_of<8>(use_grid);
    if (normal_k + 1 <= 11) return prep_choice_of<11>(use_grid);
    if (normal_k + 1 <= 13) return prep_choice_of<13>(use_grid);
    if (normal_k + 1 <= 16) return prep_choice_of<16>(use_grid);
    return prep_choice_of<32>(use_grid);
}

// What a call starts, decided as a whole from its arguments and the host mirrors (no HIP call).  need_bytes: what
// icpmi_prepared_bytes asks for these arguments; polar_opt, knn_opt: the options POLAR and PREP_KNN, read once by the caller.
struct PrepPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    std::vector<int32_t> big; // selected clouds above PREP_MAX_POINTS rows, prepared one by one (prep_big.hip) in front of the launches
    int sel_rc;               // ICPMI_ERR_ARG: the selection names a cloud outside the set — returned after the large clouds in front of it
    int small_max, lds_points;    // rows of the largest cloud of the main launch, and of its sorted copy in LDS (rounded to 64)
    PrepChoice pc;
    int polar, split, parts;
    unsigned grid;            // main launch (0: none): workgroups,
    size_t lds;               // ... their dynamic LDS (PrepLds)
    int sel_cap, per_cloud;   // any-k launch behind it (per_cloud 0: none): list capacity of a query, workgroups per cloud,
    size_t lds_k;             // ... their dynamic LDS
};
static PrepPlan plan_prepare(const int32_t* off_host, const int32_t* cloud_ids, const int32_t* cloud_ids_host, int n_sel,
                             int n_clouds, int max_n, int normal_k, size_t prepared_bytes, size_t need_bytes, int allow_polar,
                             const char* polar_opt, const char* knn_opt) {
    PrepPlan p{};
    const auto fail = [&p](int rc) { p.rc = rc; return p; };
    if (normal_k > 31 && (size_t)(normal_k + 1) * 4 * (ANYK_THREADS / ICPMI_WAVE) > 96 * 1024) return fail(ICPMI_ERR_UNSUPPORTED);   // k beyond 6 143
    if (prepared_bytes < need_bytes) return fail(ICPMI_ERR_WORKSPACE);
    if (max_n > PREP_MAX_POINTS && !off_host) return fail(ICPMI_ERR_ARG);       // sizes are needed on the host to route big clouds
    if (cloud_ids && max_n > PREP_MAX_POINTS && !cloud_ids_host) return fail(ICPMI_ERR_ARG);
    if (n_sel == 0 || max_n == 0) return p;
    // clouds above the LDS capacity go one by one through global memory (prep_big.hip)
    p.small_max = max_n;
    if (max_n > PREP_MAX_POINTS) {
        p.small_max = 0;
        for (int i = 0; i < n_sel; ++i) {
            const int c = cloud_ids ? cloud_ids_host[i] : i;
            if (c < 0 || c >= n_clouds) { p.sel_rc = ICPMI_ERR_ARG; return p; }
            const int n = off_host[c + 1] - off_host[c];
            if (n > PREP_MAX_POINTS) p.big.push_back(c);
            else p.small_max = n > p.small_max ? n : p.small_max;
        }
        if (p.small_max == 0 && normal_k <= 31) return p;
    }
    // sorted copy sized to the largest cloud (rounded to 64) — with ~1 500-point clouds 53 KB instead of 64 KB: three
    // workgroups per CU instead of two
    p.lds_points = (p.small_max + 63) / 64 * 64;
    // bearing order (sweep.hpp, SWEEP_POLAR) only where every consumer understands it: on request, and only when EVERY
    // selected cloud has at most 2 048 rows — the fused ICP launch picks ONE instantiation for the whole batch from the
    // same max_n, and the ones for larger targets (no float32 images) cannot walk a bearing order: a batch that mixes
    // scans with one rolling submap therefore sorts everything along projections.  Option "POLAR": 0 never, 2 always
    // (tests).
    p.polar = allow_polar && max_n <= 2048 ? 1 : 0;
    if (polar_opt) p.polar = p.polar ? (polar_opt[0] == '0' ? 0 : (polar_opt[0] == '2' ? 2 : 1)) : 0;
    p.split = 256 / n_sel;                 // a workgroup for every CU when the batch is small
    p.split = p.split < 1 ? 1 : (p.split > 16 ? 16 : p.split);
    // k-NN search of the normals: grid for few clouds that will be sorted along a projection (a wall across the sweep axis
    // puts hundreds of points into a window, and a small launch lasts as long as its longest search), sweep otherwise —
    // in bearing order a scan's windows are short everywhere (round 4, one 2 048-beam scan, k = 12: sweep 0.037 ms, grid
    // 0.076; 64 scans: 0.050 / 0.115).  Where the bearing order is allowed the device may still pick a projection for a
    // cloud that is no scan: the sweep is then slower, never wrong.  Option PREP_KNN = grid | sweep forces one of the two
    // (tests run both on the same inputs)
    int use_grid = p.split > 1 && !p.polar;
    if (knn_opt) use_grid = knn_opt[0] == 'g' ? 1 : (knn_opt[0] == 's' ? 0 : use_grid);
    p.pc = prep_choice(normal_k, use_grid);
    p.parts = p.pc.kk > 0 ? p.split : 1;
    if (p.small_max > 0) {
        p.grid = (unsigned)(n_sel * p.parts);
        p.lds = PrepLds(p.lds_points, sort_npad(p.small_max), p.pc.grid).bytes;
    }
    if (normal_k > 31) {
        // the list of a query: k + 1 positions, at most the largest cloud
        const int kcap = normal_k + 1 < max_n ? normal_k + 1 : max_n;
        p.sel_cap = (kcap + 63) / 64 * 64;
        p.lds_k = (size_t)p.sel_cap * 4 * (ANYK_THREADS / ICPMI_WAVE);
        p.per_cloud = 2048 / n_sel;
        p.per_cloud = p.per_cloud < 1 ? 1 : (p.per_cloud > 256 ? 256 : p.per_cloud);
    }
    return p;
}

}  // namespace icpmi

// the buffer (PreparedView, prep_common.hpp) + the scratch for the sort of clouds above 4096 rows (max_n = rows of the
// largest cloud that will be prepared)
extern "C" size_t icpmi_prepared_bytes(int32_t total_rows, int32_t n_clouds, int32_t max_n) {
    if (total_rows < 0 || n_clouds < 0 || max_n < 0) return 0;
    return icpmi::PreparedView(nullptr, total_rows, n_clouds).core_bytes +
           (max_n > icpmi::PREP_MAX_POINTS ? icpmi::prep_big_scratch_bytes(max_n) : 0);
}

extern "C" int icpmi_prepare_targets(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                                     const int32_t* cnt_dev, const int32_t* cloud_ids, const int32_t* cloud_ids_host,
                                     int32_t n_sel, int32_t n_clouds, int32_t total_rows, int32_t max_n,
                                     int32_t normal_k, double* out_normals, void* prepared, size_t prepared_bytes,
                                     void* stream) {
    return icpmi_prepare_targets_ex(pts, off_dev, off_host, cnt_dev, cloud_ids, cloud_ids_host, n_sel, n_clouds, total_rows, max_n,
                                    normal_k, out_normals, prepared, prepared_bytes, 0, stream);
}

extern "C" int icpmi_prepare_targets_ex(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                                        const int32_t* cnt_dev, const int32_t* cloud_ids, const int32_t* cloud_ids_host,
                                        int32_t n_sel, int32_t n_clouds, int32_t total_rows, int32_t max_n,
                                        int32_t normal_k, double* out_normals, void* prepared, size_t prepared_bytes,
                                        int32_t allow_polar, void* stream) {
    using namespace icpmi;
    if (!pts || !off_dev || !prepared || n_sel < 0 || n_clouds < 0 || total_rows < 0 || max_n < 0) return ICPMI_ERR_ARG;
    const PrepPlan plan = plan_prepare(off_host, cloud_ids, cloud_ids_host, n_sel, n_clouds, max_n, normal_k, prepared_bytes,
                                       icpmi_prepared_bytes(total_rows, n_clouds, max_n), allow_polar, option("POLAR"), option("PREP_KNN"));
    if (plan.rc != ICPMI_OK) return plan.rc;
    hipStream_t st = (hipStream_t)stream;
    const PreparedView v(prepared, total_rows, n_clouds);
    void* scratch = (unsigned char*)prepared + v.core_bytes;
    for (const int32_t c : plan.big) {
        const size_t o = (size_t)off_host[c];
        const int rc = prep_big_cloud(pts + o * 2, cnt_dev ? cnt_dev + c : nullptr, off_host[c + 1] - off_host[c], normal_k > 31 ? -1 : normal_k,
                                      v.sxy + o, v.snrm + o, v.sorig + o, v.dir + c, out_normals ? out_normals + o * 2 : nullptr, scratch,
                                      prepared_bytes - v.core_bytes, st);
        if (rc != ICPMI_OK) return rc;
    }
    if (plan.sel_rc != ICPMI_OK) return plan.sel_rc;
    if (!plan.grid && !plan.per_cloud) return ICPMI_OK;
    if (plan.grid) {
        if (dyn_lds((const void*)plan.pc.kernel, plan.lds) != hipSuccess) return ICPMI_ERR_HIP;
        plan.pc.kernel<<<plan.grid, PREP_THREADS, plan.lds, st>>>(pts, off_dev, cnt_dev, cloud_ids, normal_k, v.sxy, v.snrm, v.sorig, v.skey,
                                                                  v.dir, out_normals, plan.lds_points, plan.parts, plan.polar);
    }
    if (plan.per_cloud) {
        ICPMI_LAUNCH_CHECK();
        if (dyn_lds((const void*)normals_anyk_kernel, plan.lds_k) != hipSuccess) return ICPMI_ERR_HIP;
        normals_anyk_kernel<<<dim3(plan.per_cloud, n_sel), ANYK_THREADS, plan.lds_k, st>>>(off_dev, cnt_dev, cloud_ids, normal_k, v.sxy, v.snrm,
                                                                                           v.sorig, v.dir, out_normals, plan.sel_cap);
    }
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
