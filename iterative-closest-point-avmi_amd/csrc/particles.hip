// particles.hip — the particle filter on the occupancy grid (include/icpmi.h: icpmi_pf_predict, icpmi_pf_weights,
// icpmi_pf_resample, icpmi_pf_estimate, icpmi_pf_workspace_bytes, icpmi_pf_free_index, icpmi_pf_draw_uniform).  The particles stay on the device in the layout the
// beam model takes its poses in (gridbeam.hip reads them where they are); this file moves them, turns the beam model's
// records into integer weights, resamples by an integer prefix sum and adds the weighted moments in a fixed order.
//   pf_predict_kernel       a lane per particle: three deviates from Philox (particles.hpp), the motion model, sincos;
//   pf_sums_init_kernel, pf_max_kernel, pf_weights_kernel
//                           a lane per record: the largest OK score, then the table entry of each record's distance to it;
//                           one integer atomic per workgroup and slot;
//   pf_block_sums_kernel, pf_scan_sums_kernel, pf_offspring_kernel, pf_gather_kernel
//                           the prefix sum as a chain of launches — block sums, ONE workgroup over the sums, the blocks
//                           again from their offsets — so no workgroup waits on another inside a launch; E_i per particle,
//                           then a lane per new particle bisects E for its ancestor and copies the state;
//   pf_moments_kernel, pf_moments_sum_kernel
//                           per-workgroup partial sums by the fixed tree of common.hpp, combined in index order;
//   pf_free_sums_kernel, pf_free_scan_kernel, pf_free_write_kernel
//                           icpmi_pf_free_index: the map's free cells as masked words and their ranks — the same chain of
//                           launches as the resampling's prefix sum, over the words of the bit planes;
//   pf_draw_uniform_kernel  icpmi_pf_draw_uniform: a lane per slot draws a free cell by its rank (a bounded bisection, a
//                           bounded bit select), a point inside it and a heading.
#include "particles.hpp"

namespace icpmi {

__global__ __launch_bounds__(PF_THREADS) void pf_predict_kernel(int n, double2* pair_t, double* theta, double2* cos_sin, double dx, double dy,
                                                                double dth, double sx, double sy, double sth, uint64_t seed, uint32_t step) {
    const unsigned i = blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= (unsigned)n) return;
    double z[3];
    pf_deviates(seed, i, step, z);
    const double ux = dx + sx * z[0], uy = dy + sy * z[1], ut = dth + sth * z[2];
    const double2 t = pair_t[i], r = cos_sin[i];
    const double th = theta[i] + ut;
    double s, c;
    sincos(th, &s, &c);
    pair_t[i] = make_double2(t.x + (r.x * ux - r.y * uy), t.y + (r.y * ux + r.x * uy));
    theta[i] = th;
    cos_sin[i] = make_double2(c, s);
}

// ── weights ──────────────────────────────────────────────────────────────────
constexpr long long PF_NO_SCORE = (long long)0x8000000000000000ull;            // below every score: no OK record

__global__ void pf_sums_init_kernel(long long* sums) {
    if (threadIdx.x < ICPMI_PF_SUMS) sums[threadIdx.x] = threadIdx.x == ICPMI_PF_SUM_SMAX ? PF_NO_SCORE : 0;
}

// (status, rows, score, expected): the first 16 bytes of a record
__device__ __forceinline__ long long pf_ok_score(const int32_t* records, unsigned i, int n) {
    if (i >= (unsigned)n) return PF_NO_SCORE;
    const int4 r = *reinterpret_cast<const int4*>(records + (size_t)i * ICPMI_GB_INTS);
    static_assert(ICPMI_GB_REC_STATUS == 0 && ICPMI_GB_REC_SCORE == 2 && ICPMI_GB_INTS % 4 == 0, "the record's first int4");
    return r.x == ICPMI_GB_ST_OK ? (long long)r.z : PF_NO_SCORE;
}

__device__ __forceinline__ long long wave_max_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, ICPMI_WAVE);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(PF_THREADS) void pf_max_kernel(int n, const int32_t* records, long long* sums) {
    __shared__ long long best[PF_WAVES];
    __shared__ int oks[PF_WAVES];
    const long long s = pf_ok_score(records, blockIdx.x * PF_THREADS + threadIdx.x, n);
    const long long m = wave_max_ll(s);
    const unsigned long long lanes = __ballot(s != PF_NO_SCORE);
    if (lane_id() == 0) {
        best[wave_id()] = m;
        oks[wave_id()] = __popcll(lanes);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long b = best[0];
        int k = oks[0];
#pragma unroll
        for (int q = 1; q < PF_WAVES; ++q) {
            b = best[q] > b ? best[q] : b;
            k += oks[q];
        }
        if (k) {
            atomicMax(&sums[ICPMI_PF_SUM_SMAX], b);
            atomicAdd(reinterpret_cast<unsigned long long*>(&sums[ICPMI_PF_SUM_OK]), (unsigned long long)k);
        }
    }
}

__global__ __launch_bounds__(PF_THREADS) void pf_weights_kernel(int n, const int32_t* records, const uint32_t* wtable, int entries, int shift,
                                                                uint32_t* w, long long* sums) {
    __shared__ uint32_t table[ICPMI_PF_MAX_ENTRIES];
    __shared__ unsigned long long part[2][PF_WAVES];
    for (int q = threadIdx.x; q < entries; q += PF_THREADS) table[q] = min(wtable[q], (uint32_t)ICPMI_PF_MAX_WEIGHT);
    __syncthreads();
    const long long s_max = sums[ICPMI_PF_SUM_SMAX];           // (pf_max_kernel has finished: the launch before this one)
    const unsigned i = blockIdx.x * PF_THREADS + threadIdx.x;
    const long long s = pf_ok_score(records, i, n);
    uint32_t wi = 0;
    if (s != PF_NO_SCORE) {
        const long long q = (s_max - s) >> shift;              // >= 0 and below 2^32
        if (q < (long long)entries) wi = table[q];
    }
    if (i < (unsigned)n) w[i] = wi;
    const long long sw = wave_sum((long long)wi), sww = wave_sum((long long)wi * (long long)wi);
    if (lane_id() == 0) {
        part[0][wave_id()] = (unsigned long long)sw;
        part[1][wave_id()] = (unsigned long long)sww;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
#pragma unroll
        for (int q = 0; q < PF_WAVES; ++q) t += part[threadIdx.x][q];
        static_assert(ICPMI_PF_SUM_W == 0 && ICPMI_PF_SUM_WW == 1, "lane 0 adds W, lane 1 the squares");
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(&sums[threadIdx.x]), t);
    }
}

// ── resampling ───────────────────────────────────────────────────────────────
// The scan of a workgroup: every lane gives the total of its own consecutive items and gets the total of all lanes before
// it; `all` is the workgroup's total.  One barrier; wave_tot: PF_WAVES slots of LDS.
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long mine, unsigned long long* wave_tot, unsigned long long& all) {
    long long inc = (long long)mine;
#pragma unroll
    for (int o = 1; o < ICPMI_WAVE; o <<= 1) {
        const long long up = __shfl_up(inc, o, ICPMI_WAVE);
        if (lane_id() >= o) inc += up;
    }
    if (lane_id() == ICPMI_WAVE - 1) wave_tot[wave_id()] = (unsigned long long)inc;
    __syncthreads();
    unsigned long long before = 0;
    all = 0;
#pragma unroll
    for (int q = 0; q < PF_WAVES; ++q) {
        if (q < wave_id()) before += wave_tot[q];
        all += wave_tot[q];
    }
    return before + (unsigned long long)inc - mine;
}

// the lane's PF_LANE_WEIGHTS consecutive weights of scan block `block` (0 behind the last particle)
__device__ __forceinline__ void pf_lane_weights(const uint32_t* w, int n, unsigned block, uint32_t (&v)[PF_LANE_WEIGHTS], unsigned& first) {
    first = block * ICPMI_PF_SCAN_BLOCK + threadIdx.x * PF_LANE_WEIGHTS;
#pragma unroll
    for (int k = 0; k < PF_LANE_WEIGHTS; ++k) v[k] = first + k < (unsigned)n ? w[first + k] : 0u;
}

__global__ __launch_bounds__(PF_THREADS) void pf_block_sums_kernel(int n, const uint32_t* w, uint64_t* block_sums) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    uint32_t v[PF_LANE_WEIGHTS];
    unsigned first;
    pf_lane_weights(w, n, blockIdx.x, v, first);
    unsigned long long mine = 0, all;
#pragma unroll
    for (int k = 0; k < PF_LANE_WEIGHTS; ++k) mine += v[k];
    block_exclusive(mine, wave_tot, all);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = all;
}

// ONE workgroup: lane t owns sums ICPMI_PF_SUMS_PER_LANE t ... + ICPMI_PF_SUMS_PER_LANE - 1 (at most PF_MAX_BLOCKS in all)
__global__ __launch_bounds__(PF_THREADS) void pf_scan_sums_kernel(int blocks, uint64_t* block_sums, uint64_t* head, uint64_t seed, uint32_t step,
                                                                  int32_t* info) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    unsigned long long v[ICPMI_PF_SUMS_PER_LANE], mine = 0, all;
    const int first = threadIdx.x * ICPMI_PF_SUMS_PER_LANE;
#pragma unroll
    for (int k = 0; k < ICPMI_PF_SUMS_PER_LANE; ++k) {
        v[k] = first + k < blocks ? block_sums[first + k] : 0ull;
        mine += v[k];
    }
    unsigned long long run = block_exclusive(mine, wave_tot, all);
#pragma unroll
    for (int k = 0; k < ICPMI_PF_SUMS_PER_LANE; ++k) {
        if (first + k < blocks) block_sums[first + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) {
        const Philox r = pf_draw(seed, 0u, 0u, step, ICPMI_PF_PURPOSE_RESAMPLE);
        const unsigned long long u = ((unsigned long long)r.v[1] << 32) | r.v[0];
        head[0] = all;
        head[1] = all ? u % all : 0ull;
    }
    if (threadIdx.x < ICPMI_PF_INFO_INTS) info[threadIdx.x] = threadIdx.x == 0 ? (all ? ICPMI_PF_ST_OK : ICPMI_PF_ST_DEGENERATE) : 0;
}

__global__ __launch_bounds__(PF_THREADS) void pf_offspring_kernel(int n, const uint32_t* w, const uint64_t* block_sums, const uint64_t* head,
                                                                  uint32_t* E) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    uint32_t v[PF_LANE_WEIGHTS];
    unsigned first;
    pf_lane_weights(w, n, blockIdx.x, v, first);
    unsigned long long mine = 0, all;
#pragma unroll
    for (int k = 0; k < PF_LANE_WEIGHTS; ++k) mine += v[k];
    unsigned long long C = block_sums[blockIdx.x] + block_exclusive(mine, wave_tot, all);
    const unsigned long long W = head[0], rho = head[1];
#pragma unroll
    for (int k = 0; k < PF_LANE_WEIGHTS; ++k) {
        C += v[k];
        if (first + k < (unsigned)n) E[first + k] = W ? (uint32_t)(((unsigned long long)n * C + rho) / W) : first + k + 1u;
    }
}

// New particle j: the least i with E_i > j (E does not fall, and E_{n-1} = n > j).  Bit copies of the ancestor's state.
__global__ __launch_bounds__(PF_THREADS) void pf_gather_kernel(int n, const uint32_t* E, const double2* pair_t, const double* theta,
                                                               const double2* cos_sin, double2* out_pair_t, double* out_theta, double2* out_cos_sin,
                                                               int32_t* ancestors) {
    const unsigned j = blockIdx.x * PF_THREADS + threadIdx.x;
    if (j >= (unsigned)n) return;
    int lo = 0, hi = n - 1;                                    // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (E[mid] > j) hi = mid;
        else lo = mid + 1;
    }
    ancestors[j] = lo;
    out_pair_t[j] = pair_t[lo];
    out_theta[j] = theta[lo];
    out_cos_sin[j] = cos_sin[lo];
}

// ── the estimate ─────────────────────────────────────────────────────────────
__global__ __launch_bounds__(PF_THREADS) void pf_moments_kernel(int n, const uint32_t* w, const double2* pair_t, const double2* cos_sin, double* partials) {
    __shared__ double scratch[block_sum_doubles<ICPMI_PF_EST_DOUBLES>()];
    block_sum_init(scratch, block_sum_doubles<ICPMI_PF_EST_DOUBLES>());
    __syncthreads();
    double v[ICPMI_PF_EST_DOUBLES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < ICPMI_PF_EST_CHUNK / PF_THREADS; ++k) {
        const unsigned i = blockIdx.x * ICPMI_PF_EST_CHUNK + threadIdx.x + k * PF_THREADS;
        if (i < (unsigned)n) {
            const double wi = (double)w[i];
            const double2 t = pair_t[i], r = cos_sin[i];
            const double wx = wi * t.x, wy = wi * t.y;
            v[0] += wi;
            v[1] += wx;
            v[2] += wy;
            v[3] += wi * r.x;
            v[4] += wi * r.y;
            v[5] += wx * t.x;
            v[6] += wx * t.y;
            v[7] += wy * t.y;
        }
    }
    block_sum<ICPMI_PF_EST_DOUBLES, PF_WAVES>(v, scratch);
    if (threadIdx.x < ICPMI_PF_EST_DOUBLES) {
        double mine = v[0];
#pragma unroll
        for (int q = 1; q < ICPMI_PF_EST_DOUBLES; ++q) mine = (int)threadIdx.x == q ? v[q] : mine;
        partials[(size_t)blockIdx.x * ICPMI_PF_EST_DOUBLES + threadIdx.x] = mine;
    }
}

__global__ __launch_bounds__(ICPMI_WAVE) void pf_moments_sum_kernel(int chunks, const double* partials, double* out) {
    if (threadIdx.x >= ICPMI_PF_EST_DOUBLES) return;
    double s = 0.0;
    for (int g = 0; g < chunks; ++g) s += partials[(size_t)g * ICPMI_PF_EST_DOUBLES + threadIdx.x];
    out[threadIdx.x] = s;
}

// ── the free index ───────────────────────────────────────────────────────────
struct PfFreeArgs {
    const uint32_t* occ;      // the two planes (gridcast.hpp: GcPlanes)
    const uint32_t* unk;
    unsigned words;
    int wpr;
    int x0, y0, x1, y1;       // the box, every end clipped into the grid by plan_free_index: 0 <= x0, x1 <= nx (which keeps a
                              // row's pad bits out, and x - 32 wx inside int), 0 <= y0, y1 <= ny
};

// the bits of word wx of row y that lie inside the box
__device__ __forceinline__ uint32_t pf_box_mask(const PfFreeArgs& a, int y, int wx) {
    if (y < a.y0 || y >= a.y1) return 0u;
    const int lo = min(max(a.x0 - 32 * wx, 0), 32), hi = min(max(a.x1 - 32 * wx, 0), 32);
    if (hi <= lo) return 0u;                                   // (so lo < 32)
    return (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// The lane's PF_FREE_LANE_WORDS consecutive free words of scan block `block` (0 behind the last word).  Four words are one
// 16-byte load of each plane; the last group of a plane may reach past `words`, into the plane's padding to 256 bytes,
// and what it finds there is dropped.
__device__ __forceinline__ void pf_lane_free(const PfFreeArgs& a, unsigned block, uint32_t (&v)[PF_FREE_LANE_WORDS], unsigned& first) {
    first = block * ICPMI_PFG_FREE_BLOCK + threadIdx.x * PF_FREE_LANE_WORDS;
    int y = (int)(first / (unsigned)a.wpr), wx = (int)(first - (unsigned)y * (unsigned)a.wpr);
#pragma unroll
    for (int g = 0; g < PF_FREE_LANE_WORDS / 4; ++g) {
        const unsigned t = first + 4 * g;
        uint4 o = make_uint4(~0u, ~0u, ~0u, ~0u), u = o;
        if (t < a.words) {
            o = *reinterpret_cast<const uint4*>(a.occ + t);
            u = *reinterpret_cast<const uint4*>(a.unk + t);
        }
        const uint32_t f[4] = {~(o.x | u.x), ~(o.y | u.y), ~(o.z | u.z), ~(o.w | u.w)};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[4 * g + q] = t + q < a.words ? f[q] & pf_box_mask(a, y, wx) : 0u;
            if (++wx == a.wpr) {
                wx = 0;
                ++y;
            }
        }
    }
}

__global__ __launch_bounds__(PF_THREADS) void pf_free_sums_kernel(PfFreeArgs a, uint32_t* block_sums) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    uint32_t v[PF_FREE_LANE_WORDS];
    unsigned first;
    pf_lane_free(a, blockIdx.x, v, first);
    unsigned long long mine = 0, all;
#pragma unroll
    for (int k = 0; k < PF_FREE_LANE_WORDS; ++k) mine += (unsigned)__popc(v[k]);
    block_exclusive(mine, wave_tot, all);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)all;             // at most 32 * ICPMI_PFG_FREE_BLOCK
}

// ONE workgroup, as pf_scan_sums_kernel: lane t owns sums ICPMI_PF_SUMS_PER_LANE t ... (at most PF_FREE_MAX_BLOCKS in all)
__global__ __launch_bounds__(PF_THREADS) void pf_free_scan_kernel(int blocks, uint32_t* block_sums, uint32_t* header, unsigned words, int wpr) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    unsigned long long v[ICPMI_PF_SUMS_PER_LANE], mine = 0, all;
    const int first = threadIdx.x * ICPMI_PF_SUMS_PER_LANE;
#pragma unroll
    for (int k = 0; k < ICPMI_PF_SUMS_PER_LANE; ++k) {
        v[k] = first + k < blocks ? block_sums[first + k] : 0ull;
        mine += v[k];
    }
    unsigned long long run = block_exclusive(mine, wave_tot, all);
#pragma unroll
    for (int k = 0; k < ICPMI_PF_SUMS_PER_LANE; ++k) {
        if (first + k < blocks) block_sums[first + k] = (uint32_t)run;
        run += v[k];
    }
    if (threadIdx.x < ICPMI_PFG_FREE_HEADER)                     // F = all < 2^31: a grid has fewer cells
        header[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)all : threadIdx.x == 1 ? words : threadIdx.x == 2 ? (uint32_t)wpr : 0u;
}

__global__ __launch_bounds__(PF_THREADS) void pf_free_write_kernel(PfFreeArgs a, const uint32_t* block_sums, uint32_t* free, uint32_t* rank) {
    __shared__ unsigned long long wave_tot[PF_WAVES];
    uint32_t v[PF_FREE_LANE_WORDS];
    unsigned first;
    pf_lane_free(a, blockIdx.x, v, first);
    unsigned long long mine = 0, all;
#pragma unroll
    for (int k = 0; k < PF_FREE_LANE_WORDS; ++k) mine += (unsigned)__popc(v[k]);
    uint32_t C = block_sums[blockIdx.x] + (uint32_t)block_exclusive(mine, wave_tot, all);
    // groups of four again: the last one may reach past `words`, into the padding of free and rank to 256 bytes
#pragma unroll
    for (int g = 0; g < PF_FREE_LANE_WORDS / 4; ++g) {
        uint32_t r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r[q] = C;
            C += (uint32_t)__popc(v[4 * g + q]);
        }
        const unsigned t = first + 4 * g;
        if (t < a.words) {
            *reinterpret_cast<uint4*>(free + t) = make_uint4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
            *reinterpret_cast<uint4*>(rank + t) = make_uint4(r[0], r[1], r[2], r[3]);
        }
    }
}

// ── the draw ─────────────────────────────────────────────────────────────────
// A lane per slot.  Everything read from the index is bounded: words to [1, ICPMI_PFG_FREE_MAX_WORDS], the bisection to 23
// steps inside [0, words), the bit select to 32 steps and a bit below 32 — an index of stale or zero bytes gives wrong
// particles or NO_FREE, and no address outside the index.
__global__ __launch_bounds__(PF_THREADS) void pf_draw_uniform_kernel(int n, int m, const void* index, double min_x, double min_y, double res,
                                                                     double theta0, double span, double2* pair_t, double* theta, double2* cos_sin,
                                                                     int32_t* ancestors, int32_t* info, uint64_t seed, uint32_t step) {
    const unsigned j = blockIdx.x * PF_THREADS + threadIdx.x;
    const uint32_t* header = reinterpret_cast<const uint32_t*>(index);
    const uint32_t F = header[0];
    const unsigned words = min(max(header[1], 1u), (unsigned)ICPMI_PFG_FREE_MAX_WORDS), wpr = max(header[2], 1u);
    if (j < ICPMI_PF_INFO_INTS) info[j] = j == 0 ? (F ? ICPMI_PF_ST_OK : ICPMI_PFG_ST_NO_FREE) : j == 1 ? (int32_t)F : 0;
    if (j >= (unsigned)n || F == 0u) return;
    const unsigned long long jm = (unsigned long long)j * (unsigned)m;
    if ((jm + (unsigned)m) / (unsigned)n == jm / (unsigned)n) return;          // not one of the m slots
    const PfFreeIndex ix(const_cast<void*>(index), words);
    const Philox r = pf_draw(seed, j, 0u, step, ICPMI_PFG_PURPOSE_UNIFORM);
    const uint32_t k = (uint32_t)(((unsigned long long)r.v[0] * F) >> 32);     // < F
    unsigned lo = 0, hi = words - 1;                           // the largest J with rank[J] <= k lies in [lo, hi] (rank[0] = 0)
    for (int it = 0; it < 23 && lo < hi; ++it) {
        const unsigned mid = lo + ((hi - lo + 1) >> 1);
        if (ix.rank[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    uint32_t fw = ix.free[lo];
    const uint32_t skip = k - ix.rank[lo];
    for (uint32_t s = 0; s < 32u && s < skip; ++s) fw &= fw - 1u;              // drop the set bits below the one drawn
    const int bit = fw ? __ffs((int)fw) - 1 : 31;
    const unsigned cy = lo / wpr, cx = 32u * (lo - cy * wpr) + (unsigned)bit;
    const double ux = ((double)(r.v[1] >> 8) + 0.5) * (1.0 / 16777216.0), uy = ((double)(r.v[2] >> 8) + 0.5) * (1.0 / 16777216.0);
    const double th = theta0 + (((double)r.v[3] + 0.5) * (1.0 / 4294967296.0) - 0.5) * span;
    double s, c;
    sincos(th, &s, &c);
    pair_t[j] = make_double2(min_x + ((double)cx + ux) * res, min_y + ((double)cy + uy) * res);
    theta[j] = th;
    cos_sin[j] = make_double2(c, s);
    if (ancestors) ancestors[j] = ICPMI_PFG_INJECTED;
}

}  // namespace icpmi

extern "C" size_t icpmi_pf_free_index_bytes(int32_t ny, int32_t nx) {
    const icpmi::PfFreePlan plan = icpmi::plan_free_index(ny, nx, 0, 0, nx, ny);
    return plan.rc == ICPMI_OK ? plan.index_bytes : 0;
}

extern "C" int icpmi_pf_free_index(const void* planes, int32_t ny, int32_t nx, int32_t x0, int32_t y0, int32_t x1, int32_t y1, void* index,
                                   size_t index_bytes, void* stream) {
    using namespace icpmi;
    const PfFreePlan plan = plan_free_index(ny, nx, x0, y0, x1, y1);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (plan.words && (!planes || misaligned16(planes))) return ICPMI_ERR_ARG;
    if (!index || misaligned16(index) || index_bytes < plan.index_bytes) return ICPMI_ERR_WORKSPACE;
    const PfFreeIndex ix(index, plan.words);
    const GcPlanes L(ny, nx);
    const unsigned char* base = reinterpret_cast<const unsigned char*>(planes);
    const PfFreeArgs a{reinterpret_cast<const uint32_t*>(base + L.occ), reinterpret_cast<const uint32_t*>(base + L.unk), plan.words, plan.wpr,
                       plan.x0, plan.y0, plan.x1, plan.y1};
    const hipStream_t st = (hipStream_t)stream;
    if (plan.blocks) {
        pf_free_sums_kernel<<<plan.blocks, PF_THREADS, 0, st>>>(a, ix.block_sums);
        ICPMI_LAUNCH_CHECK();
    }
    pf_free_scan_kernel<<<1, PF_THREADS, 0, st>>>((int)plan.blocks, ix.block_sums, ix.header, plan.words, plan.wpr);
    ICPMI_LAUNCH_CHECK();
    if (plan.blocks) {
        pf_free_write_kernel<<<plan.blocks, PF_THREADS, 0, st>>>(a, ix.block_sums, ix.free, ix.rank);
        ICPMI_LAUNCH_CHECK();
    }
    return ICPMI_OK;
}

extern "C" int icpmi_pf_draw_uniform(int32_t n, int32_t m, const void* index, double min_x, double min_y, double resolution, double theta0,
                                     double theta_span, double* pair_t, double* theta, double* cos_sin, int32_t* ancestors, int32_t* info,
                                     uint64_t seed, uint32_t step, void* stream) {
    using namespace icpmi;
    const PfPlan plan = plan_particles(n);
    if (plan.rc != ICPMI_OK || plan.nothing) return plan.rc;
    if (m < 0 || m > n) return ICPMI_ERR_ARG;
    if (!index || !pair_t || !theta || !cos_sin || !info || misaligned16(index) || misaligned16(pair_t) || misaligned16(cos_sin) ||
        misaligned8(theta))
        return ICPMI_ERR_ARG;
    const double inf = __builtin_inf();
    for (double v : {min_x, min_y, resolution, theta0, theta_span})
        if (!(fabs(v) < inf)) return ICPMI_ERR_ARG;
    if (!(resolution > 0.0) || theta_span < 0.0 || theta_span > 6.283185307179586) return ICPMI_ERR_ARG;
    pf_draw_uniform_kernel<<<plan.lanes_grid, PF_THREADS, 0, (hipStream_t)stream>>>(
        n, m, index, min_x, min_y, resolution, theta0, theta_span, reinterpret_cast<double2*>(pair_t), theta, reinterpret_cast<double2*>(cos_sin),
        ancestors, info, seed, step);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" size_t icpmi_pf_workspace_bytes(int32_t n) {
    const icpmi::PfPlan plan = icpmi::plan_particles(n);
    return plan.rc == ICPMI_OK ? plan.ws_bytes : 0;
}

extern "C" int icpmi_pf_predict(int32_t n, double* pair_t, double* theta, double* cos_sin, double dx, double dy, double dtheta, double sigma_x,
                                double sigma_y, double sigma_theta, uint64_t seed, uint32_t step, void* stream) {
    using namespace icpmi;
    const PfPlan plan = plan_particles(n);
    if (plan.rc != ICPMI_OK || plan.nothing) return plan.rc;
    if (!pair_t || !theta || !cos_sin || misaligned16(pair_t) || misaligned16(cos_sin) || misaligned8(theta)) return ICPMI_ERR_ARG;
    const double inf = __builtin_inf();
    for (double v : {dx, dy, dtheta, sigma_x, sigma_y, sigma_theta})
        if (!(fabs(v) < inf)) return ICPMI_ERR_ARG;
    if (sigma_x < 0.0 || sigma_y < 0.0 || sigma_theta < 0.0) return ICPMI_ERR_ARG;
    pf_predict_kernel<<<plan.lanes_grid, PF_THREADS, 0, (hipStream_t)stream>>>(n, reinterpret_cast<double2*>(pair_t), theta,
                                                                               reinterpret_cast<double2*>(cos_sin), dx, dy, dtheta, sigma_x, sigma_y,
                                                                               sigma_theta, seed, step);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" int icpmi_pf_weights(int32_t n, const int32_t* records, const uint32_t* wtable, int32_t entries, int32_t shift, uint32_t* w,
                                int64_t* sums, void* stream) {
    using namespace icpmi;
    const PfPlan plan = plan_particles(n);
    if (plan.rc != ICPMI_OK || plan.nothing) return plan.rc;
    if (!records || !wtable || !w || !sums || misaligned16(records) || misaligned8(sums)) return ICPMI_ERR_ARG;
    if (entries < 1 || entries > ICPMI_PF_MAX_ENTRIES || shift < 0 || shift > ICPMI_PF_MAX_SHIFT) return ICPMI_ERR_ARG;
    const hipStream_t st = (hipStream_t)stream;
    long long* s = reinterpret_cast<long long*>(sums);
    pf_sums_init_kernel<<<1, ICPMI_WAVE, 0, st>>>(s);
    ICPMI_LAUNCH_CHECK();
    pf_max_kernel<<<plan.lanes_grid, PF_THREADS, 0, st>>>(n, records, s);
    ICPMI_LAUNCH_CHECK();
    pf_weights_kernel<<<plan.lanes_grid, PF_THREADS, 0, st>>>(n, records, wtable, entries, shift, w, s);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" int icpmi_pf_resample(int32_t n, const uint32_t* w, const double* pair_t, const double* theta, const double* cos_sin, double* out_pair_t,
                                 double* out_theta, double* out_cos_sin, int32_t* ancestors, int32_t* info, uint64_t seed, uint32_t step,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const PfPlan plan = plan_particles(n);
    if (plan.rc != ICPMI_OK || plan.nothing) return plan.rc;
    if (!w || !pair_t || !theta || !cos_sin || !out_pair_t || !out_theta || !out_cos_sin || !ancestors || !info) return ICPMI_ERR_ARG;
    if (misaligned16(pair_t) || misaligned16(cos_sin) || misaligned16(out_pair_t) || misaligned16(out_cos_sin) || misaligned8(theta) ||
        misaligned8(out_theta))
        return ICPMI_ERR_ARG;
    if (out_pair_t == pair_t || out_theta == theta || out_cos_sin == cos_sin) return ICPMI_ERR_ARG;
    const int rc = pf_workspace_rc(plan, workspace, workspace_bytes);
    if (rc != ICPMI_OK) return rc;
    const PfWs ws(workspace, (int)plan.blocks, (int)plan.chunks, n);
    const hipStream_t st = (hipStream_t)stream;
    pf_block_sums_kernel<<<plan.blocks, PF_THREADS, 0, st>>>(n, w, ws.block_sums);
    ICPMI_LAUNCH_CHECK();
    pf_scan_sums_kernel<<<1, PF_THREADS, 0, st>>>((int)plan.blocks, ws.block_sums, ws.head, seed, step, info);
    ICPMI_LAUNCH_CHECK();
    pf_offspring_kernel<<<plan.blocks, PF_THREADS, 0, st>>>(n, w, ws.block_sums, ws.head, ws.E);
    ICPMI_LAUNCH_CHECK();
    pf_gather_kernel<<<plan.lanes_grid, PF_THREADS, 0, st>>>(n, ws.E, reinterpret_cast<const double2*>(pair_t), theta,
                                                             reinterpret_cast<const double2*>(cos_sin), reinterpret_cast<double2*>(out_pair_t),
                                                             out_theta, reinterpret_cast<double2*>(out_cos_sin), ancestors);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

extern "C" int icpmi_pf_estimate(int32_t n, const uint32_t* w, const double* pair_t, const double* cos_sin, double* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const PfPlan plan = plan_particles(n);
    if (plan.rc != ICPMI_OK || plan.nothing) return plan.rc;
    if (!w || !pair_t || !cos_sin || !out || misaligned16(pair_t) || misaligned16(cos_sin) || misaligned8(out)) return ICPMI_ERR_ARG;
    const int rc = pf_workspace_rc(plan, workspace, workspace_bytes);
    if (rc != ICPMI_OK) return rc;
    const PfWs ws(workspace, (int)plan.blocks, (int)plan.chunks, n);
    const hipStream_t st = (hipStream_t)stream;
    pf_moments_kernel<<<plan.chunks, PF_THREADS, 0, st>>>(n, w, reinterpret_cast<const double2*>(pair_t), reinterpret_cast<const double2*>(cos_sin),
                                                          ws.partials);
    ICPMI_LAUNCH_CHECK();
    pf_moments_sum_kernel<<<1, ICPMI_WAVE, 0, st>>>((int)plan.chunks, ws.partials, out);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
