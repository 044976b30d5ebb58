// gridcast.hip — the occupancy grid read back as ranges (include/icpmi.h: icpmi_grid_occupancy_planes, icpmi_grid_cast_segments,
// icpmi_grid_cast_rays): along a ray, the first occupied cell and the first unknown cell before it.  The ray's cells are those
// raycast.hip lowers (raywalk.hpp: one walker for the writer and the reader), with the end cell as one more step.
//   gc_planes_kernel  packs the int16 field into two bit planes, occupied and unknown, one bit per cell: 2 bytes read and 2
//                     bits written per cell, so the casts read 1/16 of the field's bytes — planes that stay in L2 where the
//                     field does not;
//   gc_cast_kernel    one lane per ray, a wave = 64 consecutive beams of one pose.  A lane cuts its steps to the grid in closed
//                     form and walks what is left bit by bit, GC_CHUNK steps at a time with their words loaded together.
// Measured and not kept (DESIGN.md has the times): walking an x-major ray run by run — the steps between two changes of y
// as masked words of one row, __ffs / __clz for the hit — and a second, transposed pair of planes so that y-major rays walk
// runs too.  Both lost to the plain walk at 4 096 poses x 360 beams: at a cell of 0.05 m most runs are a cell or two long,
// and the lanes of a wave spend them in different branches.
// After the end cells are formed everything is integer: a record is a function of the inputs alone.
// The layout of the planes, the walk of a segment over them (gc_walk) and the plan are gridcast.hpp's: gridcheck.hip walks
// measured beams over the same planes.
#include "gridcast.hpp"

namespace icpmi {

struct GcPlaneArgs {
    const short* q;
    unsigned char* planes;
    int ny, nx, threshold;
};

// The 8 flat cells from lo (a multiple of 8) on: bit j of occ says q[lo + j] >= threshold, of unk q[lo + j] == 0.  A group
// inside the array is one aligned 16-byte load (gridfield.hip's rule); the array's last, partial group goes cell by cell,
// and a cell at or behind `total` has no bits.
__device__ __forceinline__ void gc_group_bits(const short* __restrict__ q, long long lo, long long total, int threshold,
                                              unsigned& occ, unsigned& unk) {
    occ = unk = 0;
    if (lo + 8 <= total) {
        const uint4 v = *reinterpret_cast<const uint4*>(q + lo);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(short)((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu);
            occ |= (unsigned)(c >= threshold) << j;
            unk |= (unsigned)(c == 0) << j;
        }
    } else {
        for (int j = 0; j < 8 && lo + j < total; ++j) {
            const int c = q[lo + j];
            occ |= (unsigned)(c >= threshold) << j;
            unk |= (unsigned)(c == 0) << j;
        }
    }
}

// One lane per word of the planes: the 32 cells of row y from column 32 w on are 64 bytes of the field that start at any
// int16, so the lane loads the (at most five) aligned groups of 8 that hold them, forms their bits as one 40-bit mask and
// shifts the row's own cells down; what lies behind the row's end — the next row's cells, or nothing — is masked away.
__global__ __launch_bounds__(GC_THREADS) void gc_planes_kernel(GcPlaneArgs a) {
    const GcPlanes L(a.ny, a.nx);
    const size_t t = (size_t)blockIdx.x * GC_THREADS + threadIdx.x;
    if (t >= L.words) return;
    const unsigned y = (unsigned)t / (unsigned)L.wpr, w = (unsigned)t - y * (unsigned)L.wpr;     // words < 2^31
    const int x0 = (int)w * 32, n = min(32, a.nx - x0);
    const long long total = (long long)a.ny * a.nx, f0 = (long long)y * a.nx + x0, lo = f0 & ~7ll;
    const int s = (int)(f0 - lo);
    unsigned long long occ = 0, unk = 0;
#pragma unroll
    for (int g = 0; g < 5; ++g) {
        unsigned o = 0, u = 0;
        if (g * 8 < s + n) gc_group_bits(a.q, lo + 8 * g, total, a.threshold, o, u);
        occ |= (unsigned long long)o << (8 * g);
        unk |= (unsigned long long)u << (8 * g);
    }
    const uint32_t mask = n == 32 ? ~0u : (1u << n) - 1u;
    reinterpret_cast<uint32_t*>(a.planes + L.occ)[t] = (uint32_t)(occ >> s) & mask;
    reinterpret_cast<uint32_t*>(a.planes + L.unk)[t] = (uint32_t)(unk >> s) & mask;
}


struct GcArgs {
    const unsigned char* planes;
    int ny, nx;
    const int32_t* segs;      // [n_beams][4] cells: the segment entry (n_poses = 1); null: the ray entry
    const double* poses;      // [n_poses][2]
    const double* pose_cs;    // [n_poses][2]
    const double* beam_cs;    // [n_beams][2]
    double reach, min_x, min_y, res;
    int n_poses, n_beams, wpp;   // wpp: waves per pose — a wave never spans two poses
    int4* out;
};

__global__ __launch_bounds__(GC_THREADS) void gc_cast_kernel(GcArgs a) {
    const unsigned gw = (unsigned)(((unsigned long long)blockIdx.x * GC_THREADS + threadIdx.x) >> 6);   // < 2^29 waves
    const unsigned pose = gw / (unsigned)a.wpp;
    const int beam = (int)(gw - pose * (unsigned)a.wpp) * ICPMI_WAVE + lane_id();
    if (pose >= (unsigned)a.n_poses || beam >= a.n_beams) return;
    const size_t ray = (size_t)pose * a.n_beams + beam;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool cells = true;
    if (a.segs) {
        const int4 s = reinterpret_cast<const int4*>(a.segs)[ray];
        const auto clamped = [](int v) { return min(max(v, -RC_COORD_MAX), RC_COORD_MAX); };
        x0 = clamped(s.x); y0 = clamped(s.y); x1 = clamped(s.z); y1 = clamped(s.w);
    } else {
        // as include/icpmi.h states it: every operation rounded on its own (no contraction)
        const double px = a.poses[2 * (size_t)pose], py = a.poses[2 * (size_t)pose + 1];
        const double ct = a.pose_cs[2 * (size_t)pose], st = a.pose_cs[2 * (size_t)pose + 1];
        const double ca = a.beam_cs[2 * (size_t)beam], sa = a.beam_cs[2 * (size_t)beam + 1];
        const double c = ct * ca - st * sa, s = st * ca + ct * sa;
        const double ex = px + a.reach * c, ey = py + a.reach * s;
        const bool ox = world_to_cell(px, a.min_x, a.res, x0), oy = world_to_cell(py, a.min_y, a.res, y0);
        const bool hx = world_to_cell(ex, a.min_x, a.res, x1), hy = world_to_cell(ey, a.min_y, a.res, y1);
        cells = ox && oy && hx && hy;
    }
    int4 rec = make_int4(ICPMI_GC_NO_CELLS, 0, 0, ICPMI_GC_NONE);
    if (cells) {
        const GcPlanes L(a.ny, a.nx);
        rec = gc_walk(a.planes, L, a.ny, a.nx, x0, y0, x1, y1);
    }
    a.out[ray] = rec;                                              // one 16-byte store
}

// ── host: the entries (the plan and the rule for a pointer are gridcast.hpp's) ──
int launch_planes(const GcPlan& plan, const int16_t* field, int ny, int nx, int threshold, void* planes, hipStream_t st) {
    if (!plan.plane_blocks) return ICPMI_OK;
    const GcPlaneArgs a{(const short*)field, (unsigned char*)planes, ny, nx, threshold};
    gc_planes_kernel<<<plan.plane_blocks, GC_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// The part the two cast entries share (where the planes come from is gridcast.hpp's resolve_planes)
static int cast(const GcPlan& plan, GcArgs a, const int16_t* field, const void* planes, int threshold, int32_t* out,
                void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (!plan.cast_blocks) return ICPMI_OK;
    if (!out || misaligned16(out)) return ICPMI_ERR_ARG;
    const GcSource src = resolve_planes(plan, field, planes, workspace, workspace_bytes);
    if (src.rc != ICPMI_OK) return src.rc;
    if (src.pack) {
        const int rc = launch_planes(plan, field, a.ny, a.nx, threshold, src.workspace, st);
        if (rc != ICPMI_OK) return rc;
    }
    a.planes = (const unsigned char*)src.planes;
    a.wpp = plan.wpp;
    a.out = reinterpret_cast<int4*>(out);
    gc_cast_kernel<<<plan.cast_blocks, GC_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

}  // namespace icpmi

extern "C" size_t icpmi_grid_occupancy_planes_bytes(int32_t ny, int32_t nx) {
    using namespace icpmi;
    const GcPlan plan = plan_cast(ny, nx, 0, 0);
    return plan.rc == ICPMI_OK ? plan.plane_bytes : 0;
}

extern "C" int icpmi_grid_occupancy_planes(const int16_t* field, int32_t ny, int32_t nx, int32_t occ_threshold, void* planes,
                                           size_t planes_bytes, void* stream) {
    using namespace icpmi;
    const GcPlan plan = plan_cast(ny, nx, 0, 0);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (!plan.plane_blocks) return ICPMI_OK;
    if (!field || !planes || misaligned16(field) || misaligned16(planes)) return ICPMI_ERR_ARG;
    if (planes_bytes < plan.plane_bytes) return ICPMI_ERR_WORKSPACE;
    return launch_planes(plan, field, ny, nx, occ_threshold, planes, (hipStream_t)stream);
}

extern "C" int icpmi_grid_cast_segments(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                                        const int32_t* segs, int32_t n, int32_t* out_records, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const GcPlan plan = plan_cast(ny, nx, 1, n);
    if (plan.rc != ICPMI_OK) return plan.rc;
    if (n > 0 && (!segs || misaligned16(segs))) return ICPMI_ERR_ARG;
    GcArgs a{};
    a.ny = ny; a.nx = nx; a.segs = segs; a.n_poses = 1; a.n_beams = n;
    return cast(plan, a, field, planes, occ_threshold, out_records, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int icpmi_grid_cast_rays(const int16_t* field, const void* planes, int32_t ny, int32_t nx, int32_t occ_threshold,
                                    double min_x, double min_y, double resolution, const double* poses, const double* pose_cs,
                                    int32_t n_poses, const double* beam_cs, int32_t n_beams, double reach,
                                    int32_t* out_records, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace icpmi;
    const GcPlan plan = plan_cast(ny, nx, n_poses, n_beams);
    if (plan.rc != ICPMI_OK) return plan.rc;
    const double inf = __builtin_inf();
    if (!(resolution > 0.0 && resolution < inf) || !(reach > 0.0 && reach < inf)) return ICPMI_ERR_ARG;
    if (plan.cast_blocks && (!poses || !pose_cs || !beam_cs)) return ICPMI_ERR_ARG;
    GcArgs a{};
    a.ny = ny; a.nx = nx; a.poses = poses; a.pose_cs = pose_cs; a.beam_cs = beam_cs;
    a.reach = reach; a.min_x = min_x; a.min_y = min_y; a.res = resolution;
    a.n_poses = n_poses; a.n_beams = n_beams;
    return cast(plan, a, field, planes, occ_threshold, out_records, workspace, workspace_bytes, (hipStream_t)stream);
}
