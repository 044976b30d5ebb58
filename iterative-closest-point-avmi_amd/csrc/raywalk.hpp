// raywalk.hpp — the cells of a ray, shared by the kernels that WRITE along rays (raycast.hip: update_scan) and the kernel that
// READS along them (gridcast.hip: the cast): the cell of a world coordinate, the closed-form walker over the Bresenham cells
// of mapping.py:68-89, and the cut of a beam to a rectangle of cells.  Each exists once, so the map's writer and its reader
// agree cell for cell.
#pragma once
#include "common.hpp"

namespace icpmi {

constexpr int RC_COORD_MAX = 1 << 29; // cell coordinates are clamped to +-2^29

__device__ __forceinline__ bool world_to_cell(double w, double mn, double res, int& out) {
    const double f = floor((w - mn) / res);          // mapping.py:58-59,96-97
    if (!(fabs(f) < 1e300)) return false;            // NaN / inf: the reference raises on int()
    out = f > (double)RC_COORD_MAX ? RC_COORD_MAX : (f < -(double)RC_COORD_MAX ? -RC_COORD_MAX : (int)f);
    return true;
}

// Walker over the cells of one ray.
struct Ray {
    int m0, n0, sm, sn;       // start on major / minor axis, step signs
    int dmaj, dmin, n;        // |delta| on major / minor axis, number of cells
    bool xmajor;
    int q;                    // minor offset at the current step
    long long rem;            // (2*k*dmin + dmaj - 1) mod (2*dmaj)

    __device__ __forceinline__ void init(int x0, int y0, int x1, int y1) {
        const int dx = abs(x1 - x0), dy = abs(y1 - y0);
        const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
        xmajor = dx >= dy;
        m0 = xmajor ? x0 : y0; n0 = xmajor ? y0 : x0;
        sm = xmajor ? sx : sy; sn = xmajor ? sy : sx;
        dmaj = xmajor ? dx : dy; dmin = xmajor ? dy : dx;
        n = dmaj;
        q = 0; rem = 0;
    }
    // position the walker on step k (k < n, so dmaj >= 1)
    __device__ __forceinline__ void seek(int k) {
        const long long num = 2ll * k * dmin + dmaj - 1, den = 2ll * dmaj;
        long long qq = (long long)floor((double)num / (double)den);   // quotient < 2^30: off by at most one
        long long r = num - qq * den;
        while (r < 0) { --qq; r += den; }
        while (r >= den) { ++qq; r -= den; }
        q = (int)qq; rem = r;
    }
    __device__ __forceinline__ void step() {
        rem += 2ll * dmin;
        if (rem >= 2ll * dmaj) { rem -= 2ll * dmaj; ++q; }
    }
    __device__ __forceinline__ void cell(int k, int& x, int& y) const {
        const int mj = m0 + sm * k, mn = n0 + sn * q;
        x = xmajor ? mj : mn; y = xmajor ? mn : mj;
    }
    // steps whose MAJOR coordinate lies inside [lo, hi): [klo, khi)
    __device__ __forceinline__ void clip_major(int lo, int hi, int& klo, int& khi) const {
        if (sm > 0) { klo = max(0, lo - m0); khi = min(n, hi - m0); }
        else { klo = max(0, m0 - hi + 1); khi = min(n, m0 - lo + 1); }
        if (khi < klo) khi = klo;
    }
    // first step whose minor offset is >= qq (n if none): q(k) >= qq  <=>  2*k*dmin + dmaj - 1 >= 2*dmaj*qq
    __device__ __forceinline__ int first_step_with_offset(long long qq) const {
        if (qq <= 0) return 0;
        if (qq > dmin) return n;
        const long long num = 2ll * dmaj * qq - dmaj + 1, den = 2ll * dmin;       // num > 0, den > 0 (qq <= dmin)
        // ceil(num / den) without a 64-bit integer division (a few hundred instructions on this machine, and every beam
        // that crosses a tile pays two): the float64 quotient is within a few units of it (num < 2^61), exact products settle it
        long long k = (long long)((double)num / (double)den);
        while (k * den < num) ++k;
        while (k > 0 && (k - 1) * den >= num) --k;
        return k > n ? n : (int)k;
    }
    // narrow [klo, khi) to the steps whose MINOR coordinate lies inside [lo, hi) (the offset grows with k)
    __device__ __forceinline__ void clip_minor(int lo, int hi, int& klo, int& khi) const {
        const long long qa = sn > 0 ? (long long)lo - n0 : (long long)n0 - hi + 1;   // offsets qa .. qb are inside
        const long long qb = sn > 0 ? (long long)hi - 1 - n0 : (long long)n0 - lo;
        if (qb < qa) { khi = klo; return; }
        klo = max(klo, first_step_with_offset(qa));
        khi = min(khi, first_step_with_offset(qb + 1));
        if (khi < klo) khi = klo;
    }
};

// The steps [klo, khi) of the beam (ox, oy) -> (hx, hy) that lie in the cells [x0, x1) x [y0, y1); left as they are (the
// caller's empty range) when there are none.
__device__ __forceinline__ void cut_beam(int ox, int oy, int hx, int hy, int x0, int y0, int x1, int y1, int& klo, int& khi) {
    // Bresenham stays inside the rectangle of its end points ...
    bool cross = !(max(ox, hx) < x0 || min(ox, hx) >= x1 || max(oy, hy) < y0 || min(oy, hy) >= y1);
    if (cross) {
        // ... and within one cell of the straight line: a rectangle (grown by a cell) whose corners all lie
        // strictly on one side of the line cannot be touched
        const long long dx = hx - ox, dy = hy - oy;
        const long long cxa = x0 - 1 - ox, cxb = x1 - ox, cya = y0 - 1 - oy, cyb = y1 - oy;
        const long long c0 = dx * cya - dy * cxa, c1 = dx * cya - dy * cxb, c2 = dx * cyb - dy * cxa, c3 = dx * cyb - dy * cxb;
        cross = !((c0 > 0 && c1 > 0 && c2 > 0 && c3 > 0) || (c0 < 0 && c1 < 0 && c2 < 0 && c3 < 0));
    }
    if (cross) {
        Ray ray;
        ray.init(ox, oy, hx, hy);
        if (ray.xmajor) { ray.clip_major(x0, x1, klo, khi); ray.clip_minor(y0, y1, klo, khi); }
        else { ray.clip_major(y0, y1, klo, khi); ray.clip_minor(x0, x1, klo, khi); }
    }
}

}  // namespace icpmi
