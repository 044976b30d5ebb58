// voxel.hip — K5: voxel_downsample (reference utilities/icp.py:117-129).
//
// Reference semantics reproduced exactly:
//   min_bound = points.min(0)                      per cloud, per call
//   key       = floor((p - min_bound) / voxel)     float64 IEEE divide, per axis
//   rows      = np.unique(keys, axis=0)            lexicographic order of the keys
//   mean      = bincount(weights=p) / bincount     sum taken in INPUT order
// A stable sort by the linearised key ((k0*E1 + k1)*E2 + k2, E = key extent per
// axis) followed by an in-order per-voxel sum gives bit-identical output.
//
// Clouds of <= 8192 points (every scan) take a single-workgroup path: keys and
// row ids live in LDS, bitonic sort on (key, row) pairs, one launch for a whole
// batch of clouds.  Larger clouds (the ~82k-point rolling submap of
// slam.py:103-108) use rocPRIM's radix sort on the same keys.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "sort.hpp"

namespace icpmi {

constexpr int VOX_THREADS = 1024;   // upper bound; the launcher picks 512 for large batches (loops use blockDim.x)
constexpr int VOX_MAXW = VOX_THREADS / ICPMI_WAVE;
constexpr int VOX_SMALL_MAX = 8192;

template <int DIM>
__device__ __forceinline__ uint64_t vox_key(const double* p, const double* mn, const double* ext, double voxel) {
    // floor((p - min) / voxel).astype(int), linearised so that integer order ==
    // lexicographic order of the per-axis keys
    uint64_t k = 0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        const int64_t kd = (int64_t)floor((p[d] - mn[d]) / voxel);
        k = k * (uint64_t)ext[d] + (uint64_t)kd;
    }
    return k;
}

// Per-thread min / max per axis -> the workgroup's, in every thread: wave reduction, one slot per wave and bound in
// `scratch` (6 * VOX_MAXW doubles of LDS), ONE barrier, the wave slots combined (NW of them; 0: as many as the workgroup
// has).  The caller orders earlier uses of `scratch` before the call.
template <int DIM, int NW>
__device__ __forceinline__ void bounds_combine(double (&mn)[3], double (&mx)[3], double* scratch) {
    const int nw = NW ? NW : blockDim.x / ICPMI_WAVE;
#pragma unroll
    for (int d = 0; d < DIM; ++d) { mn[d] = wave_min(mn[d]); mx[d] = wave_max(mx[d]); }
    if (lane_id() == 0)
#pragma unroll
        for (int d = 0; d < DIM; ++d) { scratch[d * VOX_MAXW + wave_id()] = mn[d]; scratch[(3 + d) * VOX_MAXW + wave_id()] = mx[d]; }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        double a = __builtin_inf(), b = -__builtin_inf();
        for (int k = 0; k < nw; ++k) { a = fmin(a, scratch[d * VOX_MAXW + k]); b = fmax(b, scratch[(3 + d) * VOX_MAXW + k]); }
        mn[d] = a; mx[d] = b;
    }
}

// min / max over the rows of one cloud, result in every thread
template <int DIM>
__device__ __forceinline__ void cloud_bounds(const double* pts, int n, double (&mn)[3], double (&mx)[3], double* scratch) {
    for (int d = 0; d < 3; ++d) { mn[d] = __builtin_inf(); mx[d] = -__builtin_inf(); }
    for (int i = threadIdx.x; i < n; i += blockDim.x)
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const double v = pts[(size_t)i * DIM + d];
            mn[d] = fmin(mn[d], v);
            mx[d] = fmax(mx[d], v);
        }
    __syncthreads();                                          // whoever used `scratch` before is done with it
    bounds_combine<DIM, 0>(mn, mx, scratch);
}

// key extents; returns false when the linear key would not fit in 63 bits
template <int DIM>
__device__ __forceinline__ bool key_extents(const double (&mn)[3], const double (&mx)[3], double voxel, double (&ext)[3]) {
    double prod = 1.0;
    bool ok = true;
    for (int d = 0; d < 3; ++d) ext[d] = 1.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        const double e = floor((mx[d] - mn[d]) / voxel) + 1.0;
        if (!(e >= 1.0) || !(e < 9.0e18)) ok = false;
        ext[d] = e;
        prod *= e;
    }
    return ok && prod < 9.0e18;
}

// (key, row) as ONE integer key << row_bits | row: row_bits = bits of a row below npad; returns the bound of the packed values
// (keys are below the product of the extents).  Below 4e9 they sort as 32-bit words, below 9e18 as 64-bit ones, else as pairs.
template <int DIM>
__device__ __forceinline__ double vox_packed_range(const double (&ext)[3], int npad, int& row_bits) {
    row_bits = 6;
    while ((1 << row_bits) < npad) ++row_bits;
    double cells = 1.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) cells *= ext[d];
    return cells * (double)npad;
}

// Exclusive prefix sum of one int per thread over the workgroup; `total` gets
// the grand total.  scratch: VOX_MAXW ints of LDS.
__device__ __forceinline__ int block_exscan(int v, int* scratch, int& total) {
    const int l = lane_id(), w = wave_id(), nw = blockDim.x / ICPMI_WAVE;
    const int inc = wave_incscan(v);
    __syncthreads();
    if (l == ICPMI_WAVE - 1) scratch[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < nw; ++k) { const int s = scratch[k]; if (k < w) base += s; tot += s; }
    total = tot;
    return base + inc - v;
}

// Mean of the voxel whose run of equal keys starts at sorted position r: the sum over its rows in order (rows ascending ==
// input order, as np.bincount adds them), divided by their count.
template <int DIM>
__device__ __forceinline__ void run_mean(const uint64_t* keys, const uint32_t* rows, int r, int n,
                                         const double* __restrict__ pts, double* __restrict__ mean) {
    const uint64_t k = keys[r];
    double s[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) s[d] = 0.0;
    int q = r;
    for (; q < n && keys[q] == k; ++q) {
        const double* p = pts + (size_t)rows[q] * DIM;
#pragma unroll
        for (int d = 0; d < DIM; ++d) s[d] += p[d];
    }
    const double c = (double)(q - r);
#pragma unroll
    for (int d = 0; d < DIM; ++d) mean[d] = s[d] / c;
}

// After the sort: voxel boundaries, voxel ids, in-order sums, means.
// keys/rows are sorted by (key, row); thread t owns sorted positions
// [t*ipt, (t+1)*ipt).  Works on LDS or global arrays (generic pointers).
template <int DIM>
__device__ __forceinline__ void voxel_finish(const uint64_t* keys, const uint32_t* rows, int n,
                                             const double* __restrict__ pts, double* __restrict__ out,
                                             int32_t* out_cnt, int* iscratch) {
    const int ipt = (n + blockDim.x - 1) / blockDim.x;
    const int lo = min(n, (int)threadIdx.x * ipt), hi = min(n, lo + ipt);
    int heads = 0;
    for (int r = lo; r < hi; ++r) heads += (r == 0 || keys[r] != keys[r - 1]);
    int total;
    int vid = block_exscan(heads, iscratch, total);
    for (int r = lo; r < hi; ++r) {
        if (!(r == 0 || keys[r] != keys[r - 1])) continue;
        run_mean<DIM>(keys, rows, r, n, pts, out + (size_t)vid * DIM);
        ++vid;
    }
    if (threadIdx.x == 0) *out_cnt = total;
}

// The usual shape — a 2 048-beam scan on 512 or 1 024 threads, keys and rows in one 32-bit word — from the sort to the
// means on REGISTERS (round 4; before: the sorted words were unpacked to 12 B per element of LDS, every voxel head re-read
// its neighbours' keys from there and fetched its members' points one dependent load after the other: a third of the
// kernel).  After the sort thread t holds the sorted elements t E .. t E + E - 1: it fetches THEIR points at once (E
// independent loads), finds the voxel heads among them from its own registers (the element before its first through
// LDS), and a head adds up its run out of the thread's own registers; only a run that continues past the thread's last
// element goes on through LDS and global memory.  Same sums in the same order: rows ascending inside a voxel.
template <int DIM>
__device__ __forceinline__ uint32_t vox_key32(const double* p, const double (&mn)[3], const uint32_t (&ext)[3], double voxel) {
    uint32_t k = 0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) k = k * ext[d] + (uint32_t)(int)floor((p[d] - mn[d]) / voxel);   // every factor below 2^31 here
    return k;
}

// Returns false (nothing written) when key and row do not fit one 32-bit word: the caller's general path takes over.
template <int DIM, int E, int THREADS>
__device__ __forceinline__ bool voxel_small_regs(const double* __restrict__ P, double* __restrict__ O, int n, double voxel,
                                                 uint32_t* sorted, double* dscratch, int* iscratch, int32_t* out_cnt) {
    constexpr uint32_t PAD = 0xffffffffu;
    const int tid = (int)threadIdx.x;
    // the thread's rows e THREADS + t (coalesced; any start order sorts the same) stay in registers from the bounds to the keys
    double raw[E][DIM];
    double mn[3], mx[3], extd[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { mn[d] = __builtin_inf(); mx[d] = -__builtin_inf(); }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * THREADS + tid;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            raw[e][d] = i < n ? P[(size_t)i * DIM + d] : 0.0;
            if (i < n) { mn[d] = fmin(mn[d], raw[e][d]); mx[d] = fmax(mx[d], raw[e][d]); }
        }
    }
    bounds_combine<DIM, THREADS / ICPMI_WAVE>(mn, mx, dscratch);    // (dscratch is untouched so far: no barrier in front)
    if (!key_extents<DIM>(mn, mx, voxel, extd)) { if (tid == 0) *out_cnt = -1; return true; }
    int row_bits;
    if (!(vox_packed_range<DIM>(extd, E * THREADS, row_bits) < 4.0e9)) return false;     // (uniform: every thread holds the same bounds)
    const uint32_t ext[3] = {(uint32_t)extd[0], (uint32_t)extd[1], (uint32_t)extd[2]};
    const uint32_t row_mask = (1u << row_bits) - 1u;
    uint32_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * THREADS + tid;
        v[e] = i < n ? (vox_key32<DIM>(raw[e], mn, ext, voxel) << row_bits) | (uint32_t)i : PAD;
    }
    bitonic_sort_regs_fixed<uint32_t, E, THREADS>(v, sorted);
    __syncthreads();                                                 // the last LDS stage's reads are done
    double pt[E][DIM];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        sorted[tid * E + e] = v[e];
        const double* p = P + (size_t)(v[e] == PAD ? 0u : (v[e] & row_mask)) * DIM;
#pragma unroll
        for (int d = 0; d < DIM; ++d) pt[e][d] = p[d];
    }
    if (tid == 0) sorted[E * THREADS] = PAD;                         // one slot behind the last element
    __syncthreads();
    const uint32_t before = tid > 0 ? sorted[tid * E - 1] : PAD;
    bool head[E];
    int nh = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t prev = e > 0 ? v[e - 1] : before;
        head[e] = v[e] != PAD && ((tid == 0 && e == 0) || (prev >> row_bits) != (v[e] >> row_bits));
        nh += head[e] ? 1 : 0;
    }
    int total;
    int vid = block_exscan(nh, iscratch, total);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (!head[e]) continue;
        const uint32_t key = v[e] >> row_bits;
        double s[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) s[d] = 0.0 + pt[e][d];         // np.bincount starts from zero
        int c = 1;
        bool open = true;                                            // the run has not met another key yet
#pragma unroll
        for (int f = e + 1; f < E; ++f) {
            open = open && v[f] != PAD && (v[f] >> row_bits) == key;
            if (open) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) s[d] += pt[f][d];
                ++c;
            }
        }
        if (open) {                                                  // past the thread's own elements (the slot behind the array ends it)
            for (int q = tid * E + E; ; ++q) {
                const uint32_t w = sorted[q];
                if (w == PAD || (w >> row_bits) != key) break;
                const double* p = P + (size_t)(w & row_mask) * DIM;
#pragma unroll
                for (int d = 0; d < DIM; ++d) s[d] += p[d];
                ++c;
            }
        }
        const double cd = (double)c;
#pragma unroll
        for (int d = 0; d < DIM; ++d) O[(size_t)vid * DIM + d] = s[d] / cd;
        ++vid;
    }
    if (tid == 0) *out_cnt = total;
    return true;
}

// The packed fallbacks: key << row_bits | row of every slot into `pk` (all ones = padding), sorted there as words of type
// T, unpacked into keys / rows (pk may be either of them: a slot is read before it is written, by the same thread).
template <typename T, int DIM>
__device__ __forceinline__ void sort_packed_keys(T* pk, uint64_t* keys, uint32_t* rows, int n, int npad, int row_bits,
                                                 const double* __restrict__ P, const double (&mn)[3], const double (&ext)[3], double voxel) {
    constexpr T PAD = ~(T)0;
    for (int i = threadIdx.x; i < npad; i += blockDim.x)
        pk[i] = i < n ? (T)(vox_key<DIM>(P + (size_t)i * DIM, mn, ext, voxel) << row_bits) | (T)i : PAD;
    __syncthreads();
    bitonic_sort_packed<T>(pk, npad);
    for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        const T v = pk[i];
        keys[i] = v == PAD ? ~0ull : (uint64_t)(v >> row_bits);
        rows[i] = v == PAD ? 0xffffffffu : (uint32_t)(v & (((T)1 << row_bits) - (T)1));
    }
    __syncthreads();
}

// ── small path: one workgroup per cloud, everything in LDS ─────────────────
template <int DIM>
__global__ __launch_bounds__(VOX_THREADS) void voxel_small_kernel(
    const double* __restrict__ pts, const int32_t* __restrict__ off, double voxel,
    double* __restrict__ out_pts, int32_t* __restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ double dscratch[6 * VOX_MAXW];
    __shared__ int iscratch[VOX_MAXW];
    const int c = blockIdx.x;
    const int n = off[c + 1] - off[c];
    if (n > VOX_SMALL_MAX) return;                            // routed to the big path by the host
    if (n <= 0) { if (threadIdx.x == 0) out_cnt[c] = 0; return; }
    const double* P = pts + (size_t)off[c] * DIM;
    double* O = out_pts + (size_t)off[c] * DIM;
    const int npad = sort_npad(n);
    const PairSortLds lds(npad);
    uint64_t* keys = lds.keys(dyn);
    uint32_t* rows = lds.rows(dyn);

    if ((npad == 4 * (int)blockDim.x || npad == 2 * (int)blockDim.x) && (blockDim.x == 512 || blockDim.x == 1024)) {
        // the usual shape (a 2 048-beam scan on 512 or 1 024 threads): the network runs on registers (sort.hpp)
        uint32_t* sorted = reinterpret_cast<uint32_t*>(keys);            // npad + 1 words, in the key array
        bool done;
        if (blockDim.x == 512) {
            if (npad == 2048) done = voxel_small_regs<DIM, 4, 512>(P, O, n, voxel, sorted, dscratch, iscratch, out_cnt + c);
            else done = voxel_small_regs<DIM, 2, 512>(P, O, n, voxel, sorted, dscratch, iscratch, out_cnt + c);
        } else {
            if (npad == 4096) done = voxel_small_regs<DIM, 4, 1024>(P, O, n, voxel, sorted, dscratch, iscratch, out_cnt + c);
            else done = voxel_small_regs<DIM, 2, 1024>(P, O, n, voxel, sorted, dscratch, iscratch, out_cnt + c);
        }
        if (done) return;                                                // else: key and row need more than 32 bits
        __syncthreads();                                                 // dscratch is written again below
    }
    double mn[3], mx[3], ext[3];
    cloud_bounds<DIM>(P, n, mn, mx, dscratch);
    if (!key_extents<DIM>(mn, mx, voxel, ext)) { if (threadIdx.x == 0) out_cnt[c] = -1; return; }
    // (key, row) sorts as ONE integer key << row_bits | row when that fits: the sort is bound by LDS traffic,
    // and a 2 048-beam scan in a room needs ~18 + 11 bits
    int row_bits;
    const double packed_range = vox_packed_range<DIM>(ext, npad, row_bits);
    if (packed_range < 4.0e9) {
        sort_packed_keys<uint32_t, DIM>(rows, keys, rows, n, npad, row_bits, P, mn, ext, voxel);   // in the row array, unpacked in place
    } else if (packed_range < 9.0e18) {
        sort_packed_keys<uint64_t, DIM>(keys, keys, rows, n, npad, row_bits, P, mn, ext, voxel);   // in the key array
    } else {
        for (int i = threadIdx.x; i < npad; i += blockDim.x) {
            keys[i] = i < n ? vox_key<DIM>(P + (size_t)i * DIM, mn, ext, voxel) : ~0ull;
            rows[i] = i < n ? (uint32_t)i : 0xffffffffu;
        }
        __syncthreads();
        bitonic_sort_pairs(keys, rows, npad);     // == stable sort by key (rows are unique)
    }
    voxel_finish<DIM>(keys, rows, n, P, O, out_cnt + c, iscratch);
}

// ── big path: every step spread over the chip ───────────────────────────────
struct VoxBounds {          // order-preserving uint64 images of the per-axis min / max (atomicMin / atomicMax)
    unsigned long long mn[3];
    unsigned long long mx[3];
};

__global__ void vox_bounds_init_kernel(VoxBounds* b) {
    if (threadIdx.x < 3) { b->mn[threadIdx.x] = ~0ull; b->mx[threadIdx.x] = 0ull; }
}

template <int DIM>
__global__ __launch_bounds__(256) void vox_bounds_kernel(const double* __restrict__ P, int n, VoxBounds* b) {
    double mn[DIM], mx[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) { mn[d] = __builtin_inf(); mx[d] = -__builtin_inf(); }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const double v = P[(size_t)i * DIM + d];
            mn[d] = fmin(mn[d], v);
            mx[d] = fmax(mx[d], v);
        }
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        const double a = wave_min(mn[d]), c = wave_max(mx[d]);
        if (lane_id() == 0) {
            atomicMin(&b->mn[d], (unsigned long long)f64_sortable(a));
            atomicMax(&b->mx[d], (unsigned long long)f64_sortable(c));
        }
    }
}

template <int DIM>
__device__ __forceinline__ bool vox_header(const VoxBounds* __restrict__ b, double voxel, double (&mn)[3], double (&ext)[3]) {
    double mx[3];
    for (int d = 0; d < 3; ++d) { mn[d] = 0.0; mx[d] = 0.0; }
#pragma unroll
    for (int d = 0; d < DIM; ++d) { mn[d] = f64_unsortable(b->mn[d]); mx[d] = f64_unsortable(b->mx[d]); }
    return key_extents<DIM>(mn, mx, voxel, ext);
}

template <int DIM>
__global__ void vox_keys_kernel(const double* __restrict__ P, int n, double voxel, const VoxBounds* __restrict__ b,
                                uint64_t* __restrict__ keys, uint32_t* __restrict__ rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double mn[3], ext[3];
    const bool ok = vox_header<DIM>(b, voxel, mn, ext);
    keys[i] = ok ? vox_key<DIM>(P + (size_t)i * DIM, mn, ext, voxel) : 0ull;
    rows[i] = (uint32_t)i;
}

// 1 where a new voxel starts in the sorted order
__global__ void vox_heads_kernel(const uint64_t* __restrict__ keys, int n, uint32_t* __restrict__ heads) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) heads[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// one thread per voxel head: in-order sum over its run of equal keys, mean, voxel id from the scan
template <int DIM>
__global__ void vox_means_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rows,
                                 const uint32_t* __restrict__ heads, const uint32_t* __restrict__ vid, int n, double voxel,
                                 const VoxBounds* __restrict__ b, const double* __restrict__ P, double* __restrict__ O,
                                 int32_t* __restrict__ out_cnt) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double mn[3], ext[3];
    const bool ok = vox_header<DIM>(b, voxel, mn, ext);
    if (r == n - 1) *out_cnt = ok ? (int32_t)(vid[r] + heads[r]) : -1;
    if (!ok || !heads[r]) return;
    run_mean<DIM>(keys, rows, r, n, P, O + (size_t)vid[r] * DIM);
}

size_t radix_temp_bytes(int n) {                             // (sort.hpp; also prep_big.hip)
    size_t bytes = 0;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)n, 0, 64, (hipStream_t)0, false);
    return bytes;
}

static size_t scan_temp_bytes(int n) {
    size_t bytes = 0;
    uint32_t* v = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, v, v, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0, false);
    return bytes;
}

// workspace of one large cloud: bounds | keys, twice | rows, twice | voxel heads | voxel ids | temporary storage of the
// sort and of the scan (one after the other in the same bytes)
struct VoxBigWs {
    Carve c;
    int n;
    size_t radix_bytes = radix_temp_bytes(n), scan_bytes = scan_temp_bytes(n);
    VoxBounds* h = c.take<VoxBounds>(256);
    uint64_t *k0 = c.take<uint64_t>((size_t)n * 8), *k1 = c.take<uint64_t>((size_t)n * 8);
    uint32_t *r0 = c.take<uint32_t>((size_t)n * 4), *r1 = c.take<uint32_t>((size_t)n * 4);
    uint32_t *heads = c.take<uint32_t>((size_t)n * 4), *vid = c.take<uint32_t>((size_t)n * 4);
    void* temp = c.take<void>(radix_bytes > scan_bytes ? radix_bytes : scan_bytes);
    size_t bytes = c.off + 256;
};

template <int DIM>
static int voxel_big(const double* P, int n, double voxel, double* O, int32_t* out_cnt, void* ws, size_t ws_bytes, hipStream_t st) {
    VoxBigWs w{ws, n};                   // (rocprim takes the sizes by reference)
    if (ws_bytes < w.bytes) return ICPMI_ERR_WORKSPACE;
    const int blocks = (n + 255) / 256;
    vox_bounds_init_kernel<<<1, 64, 0, st>>>(w.h);
    // few workgroups: every wave ends with 2*DIM atomics on the same words, and those serialise
    vox_bounds_kernel<DIM><<<blocks < 64 ? blocks : 64, 256, 0, st>>>(P, n, w.h);
    vox_keys_kernel<DIM><<<blocks, 256, 0, st>>>(P, n, voxel, w.h, w.k0, w.r0);
    if (rocprim::radix_sort_pairs(w.temp, w.radix_bytes, w.k0, w.k1, w.r0, w.r1, (size_t)n, 0, 64, st, false) != hipSuccess) return ICPMI_ERR_HIP;
    vox_heads_kernel<<<blocks, 256, 0, st>>>(w.k1, n, w.heads);
    if (rocprim::exclusive_scan(w.temp, w.scan_bytes, w.heads, w.vid, 0u, (size_t)n, rocprim::plus<uint32_t>(), st, false) != hipSuccess) return ICPMI_ERR_HIP;
    vox_means_kernel<DIM><<<blocks, 256, 0, st>>>(w.k1, w.r1, w.heads, w.vid, n, voxel, w.h, P, O, out_cnt);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// What a batch call starts, decided from its arguments and the host mirror of the offsets (no HIP call).
struct VoxPlan {
    int rc;            // ICPMI_OK, or why nothing is launched
    int threads;       // of the one launch of voxel_small_kernel over the whole set; 0: no cloud has at most VOX_SMALL_MAX rows
    size_t lds;        // ... with the pair-sort area of the largest such cloud
    int n_big;         // clouds above VOX_SMALL_MAX rows: one by one through voxel_big
};
static VoxPlan plan_voxel(const int32_t* off_host, int n_clouds, int dim, double voxel_size) {
    VoxPlan p{ICPMI_ERR_ARG, 0, 0, 0};
    if (n_clouds < 0 || (dim != 2 && dim != 3) || !(voxel_size > 0.0)) return p;
    int max_small = 0, total_rows;
    if (n_clouds > 0 && !cloud_rows(off_host, n_clouds, max_small, total_rows, VOX_SMALL_MAX, &p.n_big)) return p;
    p.rc = ICPMI_OK;
    // The kernel is a chain of latency-bound phases (two passes over the points, 66 sort stages, a gather): with
    // many clouds, four 512-thread workgroups per CU overlap them better than two of 1 024 (2.17 -> 1.55 ms for
    // 32 768 clouds); a lone cloud finishes sooner with 1 024 threads.
    p.threads = p.n_big == n_clouds ? 0 : (n_clouds > 256 ? 512 : VOX_THREADS);
    p.lds = PairSortLds(sort_npad(max_small)).bytes;
    return p;
}

template <int DIM>
static int voxel_launch(const VoxPlan& plan, const double* pts, const int32_t* off_dev, const int32_t* off_host, int n_clouds,
                        double voxel, double* out_pts, int32_t* out_cnt, void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (plan.threads) {
        if (dyn_lds((const void*)voxel_small_kernel<DIM>, plan.lds) != hipSuccess) return ICPMI_ERR_HIP;
        voxel_small_kernel<DIM><<<n_clouds, plan.threads, plan.lds, st>>>(pts, off_dev, voxel, out_pts, out_cnt);
        ICPMI_LAUNCH_CHECK();
    }
    for (int c = 0; c < n_clouds && plan.n_big > 0; ++c) {
        const int n = off_host[c + 1] - off_host[c];
        if (n <= VOX_SMALL_MAX) continue;
        if (!workspace) return ICPMI_ERR_WORKSPACE;
        const size_t o = (size_t)off_host[c] * DIM;
        const int rc = voxel_big<DIM>(pts + o, n, voxel, out_pts + o, out_cnt + c, workspace, workspace_bytes, st);
        if (rc != ICPMI_OK) return rc;
    }
    return ICPMI_OK;
}

}  // namespace icpmi

extern "C" size_t icpmi_voxel_workspace_bytes(int32_t max_n) {
    using namespace icpmi;
    if (max_n <= VOX_SMALL_MAX) return 256;
    return VoxBigWs{nullptr, max_n}.bytes;
}

extern "C" int icpmi_voxel_downsample_batch(const double* pts, const int32_t* off_dev, const int32_t* off_host,
                                            int32_t n_clouds, int32_t dim, double voxel_size,
                                            double* out_pts, int32_t* out_cnt, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    if (!pts || !off_dev || !off_host || !out_pts || !out_cnt) return ICPMI_ERR_ARG;
    const VoxPlan plan = plan_voxel(off_host, n_clouds, dim, voxel_size);
    if (plan.rc != ICPMI_OK) return plan.rc;
    return dim == 2 ? voxel_launch<2>(plan, pts, off_dev, off_host, n_clouds, voxel_size, out_pts, out_cnt, workspace, workspace_bytes, (hipStream_t)stream)
                    : voxel_launch<3>(plan, pts, off_dev, off_host, n_clouds, voxel_size, out_pts, out_cnt, workspace, workspace_bytes, (hipStream_t)stream);
}
