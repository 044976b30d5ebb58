// particles.hip — the particle filter on the occupancy grid (include/icpmi.h: icpmi_pf_predict, icpmi_pf_weights,
// icpmi_pf_resample, icpmi_pf_estimate, icpmi_pf_workspace_bytes).  The particles stay on the device in the layout the
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
//                           per-workgroup partial sums by the fixed tree of common.hpp, combined in index order.
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

}  // namespace icpmi

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
