// gridcast.hpp — what the kernels that read the occupancy planes share (gridcast.hip: the cast; gridcheck.hip, gridbeam.hip:
// the check and the beam model of measured beams): the layout of the planes, the walk of one segment over them, the read of
// one cell's unknown bit, the plan of the grid, where a call's planes come from and the launch that packs a field into
// planes.  Each exists once, so the three read the map through one copy.
#pragma once
#include "raywalk.hpp"

namespace icpmi {

constexpr int GC_THREADS = ICPMI_GC_THREADS;
#ifndef ICPMI_GC_CHUNK
#define ICPMI_GC_CHUNK 4                   // (make variant: 1, 8 and 16 were measured against it)
#endif
constexpr int GC_CHUNK = ICPMI_GC_CHUNK;   // steps of a walk whose words are loaded together

// The planes of an (ny, nx) grid, described once (the host sizes the buffer with it, the kernels find their words):
//   occ  uint32 [ny][wpr]   bit x & 31 of word x >> 5 of row y: cell (y, x) is occupied
//   unk  uint32 [ny][wpr]   the same for "unknown"
// Rows are padded to whole words and the pad bits are clear, so a masked word never shows a cell outside the grid.
struct GcPlanes {
    int wpr;
    size_t words, occ, unk, bytes;
    __host__ __device__ GcPlanes(int ny, int nx) {
        wpr = (nx + 31) / 32;
        words = (size_t)ny * wpr;
        const auto a256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
        occ = 0;
        unk = a256(words * sizeof(uint32_t));
        bytes = unk + a256(words * sizeof(uint32_t));
    }
};

// The record of the segment (x0, y0) -> (x1, y1) over the planes
__device__ __forceinline__ int4 gc_walk(const unsigned char* __restrict__ planes, const GcPlanes& L, int ny, int nx,
                                        int x0, int y0, int x1, int y1) {
    Ray r;
    r.init(x0, y0, x1, y1);
    r.n = r.dmaj + 1;                                              // steps 0 .. K: the end cell is a step of the cast
    // only the steps inside the grid can matter: a range [klo, khi), in closed form
    int klo = 0, khi = 0;
    if (r.xmajor) { r.clip_major(0, nx, klo, khi); r.clip_minor(0, ny, klo, khi); }
    else { r.clip_major(0, ny, klo, khi); r.clip_minor(0, nx, klo, khi); }
    int k_hit = ICPMI_GC_NONE, k_unk = ICPMI_GC_NONE, xh = x1, yh = y1;
    if (klo >= khi) return make_int4(k_hit, xh, yh, k_unk);
    if (r.dmaj > 0) r.seek(klo);                                   // (K = 0: the origin cell alone, offset 0)
    const uint32_t* occ = reinterpret_cast<const uint32_t*>(planes + L.occ);
    const uint32_t* unk = reinterpret_cast<const uint32_t*>(planes + L.unk);
    // Bit by bit, GC_CHUNK steps at a time: their words are asked for together and looked at in order, so the chain of
    // dependent loads of a ray is a GC_CHUNK-th of its steps (a step past the range repeats the chunk's first word, unused).
    // A lane leaves at its hit; a wave when all of its lanes have.
    for (int k0 = klo; k0 < khi && k_hit < 0; k0 += GC_CHUNK) {
        int xs[GC_CHUNK], ys[GC_CHUNK];
        uint32_t wi[GC_CHUNK], o[GC_CHUNK], u[GC_CHUNK];           // (ny * wpr < 2^31 words)
        const bool want_unk = k_unk < 0;
#pragma unroll
        for (int j = 0; j < GC_CHUNK; ++j) {
            r.cell(k0 + j, xs[j], ys[j]);
            wi[j] = k0 + j < khi ? (uint32_t)ys[j] * (uint32_t)L.wpr + (uint32_t)(xs[j] >> 5) : wi[0];
            r.step();
        }
#pragma unroll
        for (int j = 0; j < GC_CHUNK; ++j) o[j] = occ[wi[j]];
#pragma unroll
        for (int j = 0; j < GC_CHUNK; ++j) u[j] = want_unk ? unk[wi[j]] : 0u;
#pragma unroll
        for (int j = 0; j < GC_CHUNK; ++j) {
            const uint32_t bit = 1u << (xs[j] & 31);
            const bool live = k0 + j < khi && k_hit < 0;
            if (live && (o[j] & bit)) { k_hit = k0 + j; xh = xs[j]; yh = ys[j]; }
            else if (live && k_unk < 0 && (u[j] & bit)) k_unk = k0 + j;          // (only BEFORE the hit: a hit ends `live`)
        }
    }
    return make_int4(k_hit, xh, yh, k_unk);
}

// One more masked read: is cell (x, y) observed space — its unknown bit clear?  A cell outside the grid is not.
__device__ __forceinline__ bool gc_observed(const unsigned char* __restrict__ planes, const GcPlanes& L, int ny, int nx, int x, int y) {
    if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny) return false;
    const uint32_t* unk = reinterpret_cast<const uint32_t*>(planes + L.unk);
    return !(unk[(uint32_t)y * (uint32_t)L.wpr + (uint32_t)(x >> 5)] & (1u << (x & 31)));
}

// ── host: the plan, the source of the planes, the packing launch ─────────────
// What a call starts, decided as a whole and without a HIP call
struct GcPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    unsigned plane_blocks;    // gc_planes_kernel: a lane per word of a plane; 0: nothing to pack
    unsigned cast_blocks;     // gc_cast_kernel: whole waves per pose; 0: no ray
    int wpp;
    size_t plane_bytes;       // GcPlanes of the grid
};
inline GcPlan plan_cast(int ny, int nx, long long n_poses, long long n_beams) {
    GcPlan p{ICPMI_OK, 0, 0, 0, 0};
    if (ny < 0 || nx < 0 || ny > RC_COORD_MAX || nx > RC_COORD_MAX || (long long)ny * nx >= (1ll << 31) || n_poses < 0 || n_beams < 0) {
        p.rc = ICPMI_ERR_ARG;
        return p;
    }
    if (n_poses * n_beams >= (1ll << 29)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    const GcPlanes L(ny, nx);
    p.plane_bytes = L.bytes;
    p.plane_blocks = (unsigned)((L.words + GC_THREADS - 1) / GC_THREADS);
    p.wpp = (int)((n_beams + ICPMI_WAVE - 1) / ICPMI_WAVE);
    p.cast_blocks = (unsigned)((n_poses * p.wpp * ICPMI_WAVE + GC_THREADS - 1) / GC_THREADS);
    return p;
}

inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// Where a call's planes come from: the caller's, or packed from the field into the workspace first.  Decided without a HIP
// call, so that a caller enqueues nothing before every refusal has been made; launch_planes into `workspace` where `pack`.
struct GcSource {
    int rc;                   // ICPMI_OK, or the refusal
    const void* planes;       // what the kernel reads (null only for an empty grid: no step is inside it)
    bool pack;
    void* workspace;
};
inline GcSource resolve_planes(const GcPlan& plan, const int16_t* field, const void* planes, void* workspace, size_t workspace_bytes) {
    GcSource s{ICPMI_OK, planes, !planes && plan.plane_blocks, workspace};
    if (planes && misaligned16(planes)) s.rc = ICPMI_ERR_ARG;
    else if (s.pack && (!field || misaligned16(field))) s.rc = ICPMI_ERR_ARG;
    else if (s.pack && (!workspace || misaligned16(workspace) || workspace_bytes < plan.plane_bytes)) s.rc = ICPMI_ERR_WORKSPACE;
    if (s.pack) s.planes = workspace;
    return s;
}

// gc_planes_kernel of `field` into `planes` (gridcast.hip): ICPMI_OK, at once where the plan has nothing to pack
int launch_planes(const GcPlan& plan, const int16_t* field, int ny, int nx, int threshold, void* planes, hipStream_t st);

}  // namespace icpmi
