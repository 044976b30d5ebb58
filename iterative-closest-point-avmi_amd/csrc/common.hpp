// common.hpp — shared device helpers for libicpmi.so (gfx950 / wave64 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/icpmi.h"

#define ICPMI_WAVE 64

#define ICPMI_LAUNCH_CHECK()                                   \
    do {                                                       \
        hipError_t e__ = hipGetLastError();                    \
        if (e__ != hipSuccess) return ICPMI_ERR_HIP;           \
    } while (0)

namespace icpmi {

// ── process-wide state (state.hip): options read once, side streams of the library ───────────────────
// option("NAME"): value of the ICPMI_NAME switch (environment at first use, icpmi_set_option later) or nullptr.
const char* option(const char* name);
// dyn_lds(kernel, bytes): the kernel's dynamic-LDS limit on the current device raised to at least `bytes` (state.hip: the
// attribute is set when a launch needs more than any before it, not on every launch)
hipError_t dyn_lds(const void* fn, size_t bytes);
constexpr int ICPMI_SIDE_STREAMS = 3;
struct Side {
    hipStream_t stream[ICPMI_SIDE_STREAMS] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr;
    hipEvent_t join[ICPMI_SIDE_STREAMS] = {nullptr, nullptr, nullptr};
    bool failed = false;
};
// Holds the library's side-stream lock for a whole fork / launch / join sequence; `side` is the current device's
// set (made on first use) or nullptr when side streams are off or could not be made.
struct SideLock {
    Side* side;
    SideLock();
    ~SideLock();
    SideLock(const SideLock&) = delete;
    SideLock& operator=(const SideLock&) = delete;
};

// Gate of icpmi_icp_batch_gated (icp.hip): pair b has the gate index base + b * stride; a pair whose index is above the
// value of *hint it reads may stop (ICPMI_ST_SKIPPED); a finished, eligible pair with err < accept lowers *hint to its
// index.  Eligible: search == nullptr, or the status of its rotation-search record (ICPMI_RSBREC_STATUS) below
// ICPMI_RSB_ST_CAPACITY (ok, or too few points: the ICP then starts from the identity, as the reference's does).
struct IcpGate {
    int32_t* hint;
    const double* search;
    double accept;
    int base, stride;
};
__device__ __forceinline__ bool gate_eligible(const double* search, int b) {
    return !search || search[(size_t)b * ICPMI_RSBREC_DOUBLES + ICPMI_RSBREC_STATUS] < (double)ICPMI_RSB_ST_CAPACITY;
}

// The fused 2-D ICP on prepared targets (icp2.hip), called by icpmi_icp_batch (icp.hip) when a prepared buffer is given and
// everything fits.
int launch_icp2(const double* pts, const int32_t* off, const int32_t* cnt, const int32_t* ps, const int32_t* pt,
                int n_pairs, int max_src_n, int max_tgt_n, int total_rows, const icpmi_icp_params* p, const double* init,
                double* results, const void* prepared, void* workspace, size_t workspace_bytes, const IcpGate* gate,
                hipStream_t st);

// ── carving a caller's buffer (host) ─────────────────────────────────────────
__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Rows of the clouds of a set, from the host mirror of its offsets: false when a cloud has a negative row count.  With a
// `limit` (and a counter), max_n is the largest cloud at or below it and *n_above counts the clouds above it.
inline bool cloud_rows(const int32_t* off_host, int n_clouds, int& max_n, int& total_rows, int limit = 0x7fffffff,
                       int* n_above = nullptr) {
    max_n = 0;
    if (n_above) *n_above = 0;
    for (int c = 0; c < n_clouds; ++c) {
        const int rows = off_host[c + 1] - off_host[c];
        if (rows < 0) return false;
        if (rows > limit) ++*n_above;
        else max_n = rows > max_n ? rows : max_n;
    }
    total_rows = off_host[n_clouds];
    return true;
}

// Bump pointer over a caller's buffer.  take<T>(bytes) is the current position, and moves on by `bytes` rounded up to
// 256; packed<T>(bytes) moves on by exactly `bytes` (the layouts that keep no gaps).  Every layout is described ONCE, by a
// struct whose first member is a Carve and whose pointers are initialised from it, in the order they are declared (which
// is the order of the layout).  Over a null base it only counts (every pointer is nullptr): that is the layout's *_bytes
// query; over the caller's buffer it yields the pointers the launcher uses.  (Host and device: a kernel that is handed a
// buffer alone — the free index of particles.hpp — finds its parts by the same description.)
struct Carve {
    unsigned char* base;
    size_t off = 0;
    __host__ __device__ Carve(void* b) : base((unsigned char*)b) {}
    template <class T> __host__ __device__ T* packed(size_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return p;
    }
    template <class T> __host__ __device__ T* take(size_t bytes) { return packed<T>(align256(bytes)); }
};

__device__ __forceinline__ int lane_id() { return threadIdx.x & (ICPMI_WAVE - 1); }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// ── cross-lane moves on the VALU (DPP), no LDS crossbar ─────────────────────
// dpp_ctrl: quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E,
// row_half_mirror = 0x141, row_mirror = 0x140 (rows are 16 lanes).
// These four only permute lanes inside a row, so with full row and bank masks every lane reads a lane that exists: the
// destination needs no old value.  mov_dpp with bound_ctrl on says so (an undefined old value); update_dpp(0, ...) made
// the compiler write a zero into the destination in front of every move.  (An INACTIVE source lane reads as 0, as it
// did: the reductions below are for whole waves.)
template <int CTRL>
__device__ __forceinline__ int dpp_b32(int v) {
    static_assert(CTRL == 0xB1 || CTRL == 0x4E || CTRL == 0x141 || CTRL == 0x140, "a permutation inside the row");
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return __int_as_float(dpp_b32<CTRL>(__float_as_int(v))); }
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_b32<CTRL>((int)(b & 0xffffffffll));
    const int hi = dpp_b32<CTRL>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Sum over each 16-lane row; afterwards every lane of a row holds its row's sum.
__device__ __forceinline__ double row_sum(double v) {
    v += dpp_f64<0xB1>(v);     // lane ^ 1
    v += dpp_f64<0x4E>(v);     // lane ^ 2
    v += dpp_f64<0x141>(v);    // mirror inside each half row: the other quad
    v += dpp_f64<0x140>(v);    // mirror inside the row: the other half row
    return v;
}

// Wave-wide sum, identical (wave-uniform) in every lane.  Fixed tree: quads,
// half rows, rows, then rows 0..3 left to right — reproducible run to run.
__device__ __forceinline__ double wave_sum(double v) {
    v = row_sum(v);
    return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ICPMI_WAVE);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {     // the two halves shuffled apart, one 64-bit add per step
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ICPMI_WAVE);
    return v;
}
// Wave-wide min / max, identical in every lane: the same four DPP steps inside the rows, then two steps across the rows
// on the VALU (no LDS crossbar, no scalar registers).  v_permlane16_swap of a register with a copy of itself leaves rows
// (0, 0, 2, 2) in one and (1, 1, 3, 3) in the other, v_permlane32_swap the lower half twice and the upper half twice.
// min and max are exact, so the tree does not matter to the result.
template <bool ROWS16>
__device__ __forceinline__ void swap_self(unsigned v, unsigned& x, unsigned& y) {
    if constexpr (ROWS16) { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); x = r[0]; y = r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); x = r[0]; y = r[1]; }
}
template <bool ROWS16>
__device__ __forceinline__ void swap_self(double v, double& x, double& y) {
    const long long b = __double_as_longlong(v);
    unsigned xl, yl, xh, yh;
    swap_self<ROWS16>((unsigned)b, xl, yl);
    swap_self<ROWS16>((unsigned)(b >> 32), xh, yh);
    x = __longlong_as_double(((long long)xh << 32) | xl);
    y = __longlong_as_double(((long long)yh << 32) | yl);
}
__device__ __forceinline__ double wave_min(double v) {
    v = fmin(v, dpp_f64<0xB1>(v));
    v = fmin(v, dpp_f64<0x4E>(v));
    v = fmin(v, dpp_f64<0x141>(v));
    v = fmin(v, dpp_f64<0x140>(v));
    double x, y;
    swap_self<true>(v, x, y);
    swap_self<false>(fmin(x, y), x, y);
    return fmin(x, y);
}
__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    double x, y;
    swap_self<true>(v, x, y);
    swap_self<false>(fmax(x, y), x, y);
    return fmax(x, y);
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_f32<0xB1>(v));
    v = fmaxf(v, dpp_f32<0x4E>(v));
    v = fmaxf(v, dpp_f32<0x141>(v));
    v = fmaxf(v, dpp_f32<0x140>(v));
    unsigned x, y;
    swap_self<true>((unsigned)__float_as_int(v), x, y);
    swap_self<false>((unsigned)__float_as_int(fmaxf(__int_as_float((int)x), __int_as_float((int)y))), x, y);
    return fmaxf(__int_as_float((int)x), __int_as_float((int)y));
}

// Inclusive prefix sum over the wave (integer adds: any tree is exact).  Four shifts inside the rows (row_shr:1, 2, 4, 8;
// a lane the shift leaves without a source adds 0), then the running totals across the rows: lane 15 of rows 0 and 2 into
// rows 1 and 3 (row_bcast:15, row mask 0xa), lane 31 into rows 2 and 3 (row_bcast:31, row mask 0xc).  Whole waves only.
__device__ __forceinline__ int wave_incscan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}

// (value, index) pairs: the other pair replaces this one when its value is better — `better` is a strict order, `<` for
// an arg-min, `>` for an arg-max — or equal with the lower index: the FIRST of equal values wins, as np.argmin's scan.
template <class T, class Better>
__device__ __forceinline__ void take_first_best(T& v, int& i, T ov, int oi, Better better) {
    if (better(ov, v) || (ov == v && oi < i)) { v = ov; i = oi; }
}
// ... over the wave (butterfly): every lane gets the wave's pair
template <class T, class Better>
__device__ __forceinline__ void wave_first_best(T& v, int& i, Better better) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take_first_best(v, i, __shfl_xor(v, o, ICPMI_WAVE), __shfl_xor(i, o, ICPMI_WAVE), better);
}

// Workgroup-wide sum of NV doubles per thread; the result is in every thread.
// scratch: NV4 * 16 doubles of LDS (NV4 = NV rounded up to a multiple of 4) owned
// by this call site, zero-initialised once by the caller (block_sum_init).
// ONE barrier per reduction: two consecutive uses of the same scratch must be
// separated by some other workgroup barrier (in the ICP loop the reductions
// alternate, each one's barrier protects the other's scratch).  MAXW <= 16.
// Wave partials (fixed DPP tree) are combined by a second fixed tree over the
// wave index, four values at a time (one value per 16-lane row): reproducible.
template <int NV, int MAXW>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* scratch) {
    static_assert(MAXW <= 16, "at most 16 waves per workgroup");
    constexpr int NV4 = (NV + 3) / 4 * 4;
    const int w = wave_id(), l = lane_id();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum(v[i]);
        if (l == 0) scratch[i * 16 + w] = s;      // slots w >= #waves stay zero
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NV4 / 4; ++g) {
        const double x = row_sum(scratch[(g * 4 + (l >> 4)) * 16 + (l & 15)]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (g * 4 + q < NV) v[g * 4 + q] = readlane_f64(x, 16 * q);
    }
}

template <int NV>
constexpr int block_sum_doubles() { return (NV + 3) / 4 * 4 * 16; }

// zero a scratch area (all threads; caller adds the barrier)
__device__ __forceinline__ void block_sum_init(double* scratch, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) scratch[i] = 0.0;
}

}  // namespace icpmi
