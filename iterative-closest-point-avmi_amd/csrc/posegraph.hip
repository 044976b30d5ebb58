// posegraph.hip — PoseGraph2D.optimize (reference utilities/pose_graph.py:83-134) in one launch.
//
// The reference builds the dense 3n x 3n normal matrix H edge by edge in Python
// and solves it with LAPACK on every Gauss-Newton iteration.  The graphs it
// builds (slam.py:543-549, 593) are an odometry chain 0-1-2-...-(n-1) plus a few
// loop-closure edges, so here
//     H = T + W C W^T
// with T block tridiagonal (3x3 blocks: the chain edges and the anchor), W the
// 3n x 3k Jacobian columns of the k other edges and C = blockdiag(Omega_e):
//     T^-1 by block cyclic reduction along the chain (log2 n levels, each parallel
//     over nodes and over all 1 + 3k right-hand sides), then the 3k x 3k system
//     (I + C W^T T^-1 W) y = C W^T T^-1 r,  dx = T^-1 r - T^-1 W y.
// O(n k^2) work instead of O(n^3), and the whole optimisation — every
// iteration's linearisation, solve, update and convergence test — runs inside
// ONE persistent workgroup: no launches or host round trips between iterations.
// A graph with a gap in the chain (or whose nodes are not numbered along it)
// takes the general path: the same dense matrix as the reference, eliminated
// with partial pivoting by the workgroup in global memory.
//
// An iteration of pose_graph_kernel (pg_gauss_newton, inlined into it) is its phases in this order (PgPhase names their clocks):
//     assemble; then either the dense solve, or closure columns -> chain solve (reduce, back-substitute) ->
//     closure system -> closure solve -> dx; then apply.
// Each is a function called once, but for two that stay as they were because the measured time depends on it: the
// chain solve is written out in the iteration loop (as a function, of the same text, it runs 4 % slower at 2 000 and 4 000
// nodes), and the assembly is one node loop that branches on the path where it stores (split into a chain and a
// dense loop over a shared gather, dx ran 4 to 9 % slower).  With 256 VGPRs in use and over a hundred SGPRs spilled,
// the allocation of the whole kernel moves with the shape of any of its parts.
//
// The split is only as good as T.  The host plan (pg_plan) reads the information
// matrices and gives every weak chain edge a twin among the closures, so that T
// stays as stiff as the whole system; a graph with a chain edge that carries no
// information at all along some direction is not split.  Where a block of T or
// the closure system still turns out exactly singular, the launch ends with
// status ICPMI_PG_ST_REFUSED and the poses of the previous iteration, and the
// caller continues from there on the dense path.  Only the dense elimination,
// like the reference's LAPACK call, ever reports a singular system.
//
// Every sum has a fixed order (per-node gathers in edge order, fixed reduction
// trees): results are reproducible run to run.
//
// pose_graph_robust_kernel (PoseGraph2D.optimize_robust: Huber, Cauchy or Geman-McClure on the edges the caller masks)
// is the same iteration, pg_gauss_newton, under the other edge policy: a `weights` phase in front of every iteration
// sets w_q = rho'(chi2_q) at the current poses, and the assembly and the closure system load w_q Omega_q where the
// plain kernel loads Omega_q.  The two kernels share every phase's one copy; the plain one keeps the registers, scratch
// and LDS it had (DESIGN.md has both resource reports).
//
// Where things are, in this order.  PgPlanWs, the plan's device arrays, listed once as the base of every layout; the
// optimiser's layouts (PgWs, and PgRobWs = PgWs + two arrays) and kernel arguments (layout + PgCaller, the caller's fields,
// once for both); the 3 x 3 helpers and pg_linearise; the phases, the two kernels and total_error's kernel; the host plan;
// pg_stage, the ONE host front of every entry that runs on a plan — it checks the arguments, refuses what the host can
// refuse before the first HIP call, reads Omega back, finds the weak chain edges, makes the twins' rows, uploads and
// synchronises — and per entry a host function that hands it a PgCall, fills the kernel's argument and launches; then
// PoseGraph2D.marginals (blocks of H^-1 on the same plan and front, its own layout MgWs and kernels marg_*).  One file: as
// a translation unit of their own the marginals left both Gauss-Newton kernels their instructions and 0.3 % more time
// (DESIGN.md).
#include "common.hpp"
#include <optional>
#include <type_traits>
#include <vector>

namespace icpmi {

constexpr int PG_THREADS = 512;                    // one workgroup, 2 waves per SIMD
constexpr double PG_PI = 3.141592653589793;        // np.pi
constexpr double PG_2PI = 6.283185307179586;       // 2 * np.pi

// The plan's device arrays, listed ONCE for every layout that runs on a plan (PgWs, PgRobWs, MgWs): a layout derives from
// this, so the index arrays are carved first, lists its own arrays, and ends with the twins' rows and its size.  Over a
// null base a layout only counts (the *_workspace_bytes queries); over the caller's workspace it is the pointer block
// its kernels get by value.  n nodes, m edges with the twins, k closures, w twins.  The + 1 keep zero-sized arrays distinct.
struct PgPlanWs {
    Carve c;
    int n, m, k, dense, w;
    // rows of the system, closure unknowns, columns of the optimiser's X, bytes of [n][9]: int like the kernels' indices
    // (the workspace of a graph near 2^31 / 3 rows would not fit any device); every product of two of them is taken in
    // size_t.  The last two are the optimiser's alone and stand here, in front of the pointers, because that is where
    // pose_graph_kernel's argument had them: behind the index arrays its SGPR spills rose from 120 to 137.
    int N3 = 3 * n, K = 3 * k, ncols = 1 + K;
    size_t blocks = 9 * (size_t)n * 8;
    int32_t* ei = c.take<int32_t>((size_t)m * 2 * 4);            // [m] ei, then [m] ej
    int32_t* ej = ei ? ei + m : nullptr;
    int32_t* csr_ptr = c.take<int32_t>(((size_t)n + 1) * 4);     // [n+1] incident edges of every node ...
    int32_t* csr_edge = c.take<int32_t>(((size_t)2 * m + 1) * 4);        // ... in edge order
    int32_t* loop_slot = c.take<int32_t>((size_t)(m + 1) * 4);   // [m] index among the non-chain edges, -1 for a chain edge
    int32_t* loop_edge = c.take<int32_t>((size_t)(k + 1) * 4);   // [k] edge ids of the non-chain edges
};

// The optimiser's layout: what pose_graph_kernel works in, inside PgArgs.
struct PgWs : PgPlanWs {
    using Base = PgPlanWs;
    // block tridiagonal T per node: D[v] = H[v][v], U[v] = H[v][v+s], L[v] = H[v][v-s] (s = level stride)
    double *D = c.take<double>(blocks), *U = c.take<double>(blocks), *L = c.take<double>(blocks);
    // per even node of a level: L[e] * inv(D[e-s]) and U[e] * inv(D[e+s])
    double *Dinv = c.take<double>(blocks), *G = c.take<double>(blocks);
    double* X = c.take<double>((size_t)N3 * ncols * 8);                // [3n][1 + 3k] right-hand sides -> solutions (column 0 = r = -b, then W)
    double* AB = c.take<double>(18 * (size_t)(k + 1) * 8);       // [k][18] Jacobians of the non-chain edges
    double *M = c.take<double>(((size_t)K * K + 1) * 8), *g = c.take<double>(((size_t)K + 1) * 8);       // [3k][3k], [3k] -> y
    double* dx = c.take<double>((size_t)N3 * 8);                         // [3n]
    double* Hd = dense ? c.take<double>((size_t)N3 * N3 * 8) : nullptr;  // [3n][3n], dense path only
    double* tw_omega = w ? c.take<double>((size_t)m * 9 * 8) : nullptr;  // the caller's Omega and z with the twins' rows:
    double* tw_z = w ? c.take<double>((size_t)m * 3 * 8) : nullptr;      // only where there are twins
    size_t bytes = c.off + 256;
};

// what the caller of either optimiser passes: its arrays and settings
struct PgCaller {
    double* nodes;                 // [n][3] x, y, theta — updated in place
    const double* z;               // [m][3]    the caller's arrays, or tw_z / tw_omega
    const double* omega;           // [m][9]
    int n_iter, fix;
    double eps;
    double* info;                  // [ICPMI_PGINFO_DOUBLES], the robust kernel's [ICPMI_ROB_DOUBLES]
};
struct PgArgs : PgWs, PgCaller {};

// The robust optimiser's device arrays: PgWs, then per edge of the plan (m: with the twins) its weight and its mask.
struct PgRobWs : PgWs {
    using Base = PgWs;
    double* wgt = c.take<double>(((size_t)m + 1) * 8);           // [m] w_q of this iteration: 1.0 for an unmasked edge and for a twin
    uint8_t* rob = c.take<uint8_t>((size_t)m + 1);               // [m] the caller's mask, 0 for the twins
    size_t bytes = c.off + 256;                                  // of the whole layout (PgWs::bytes ends before wgt)
};

struct PgRobArgs : PgRobWs, PgCaller {
    const double* omega0;          // [m0][9] the caller's Omega: chi2 is taken of the edge as given, also where it has a twin
    int m0, kernel;                // the caller's edges; ICPMI_ROB_KERNEL_*
    double delta;
    double* edge_chi2;             // [m0] out
    double* edge_weight;           // [m0] out
};

// How an edge's Omega enters H and b: weigh(g, q, x) is what a loaded entry x of Omega_q contributes with.
struct PgPlainEdges {              // Omega_q as given
    static constexpr bool weighted = false;
    using Args = PgArgs;
    static __device__ __forceinline__ double weigh(const PgArgs&, int, double x) { return x; }
};
struct PgWeightedEdges {           // w_q Omega_q, w_q from the weights phase: the loaded entries multiplied, nothing else
    static constexpr bool weighted = true;
    using Args = PgRobArgs;
    static __device__ __forceinline__ double weigh(const PgRobArgs& g, int q, double x) { return x * g.wgt[q]; }
};

// the phases of an iteration, in the order of their clocks in info[ICPMI_PGINFO_PHASE_US + .]
enum PgPhase { PG_ASSEMBLE, PG_CLOSURE_COLUMNS, PG_CHAIN_SOLVE, PG_CLOSURE_SYSTEM, PG_CLOSURE_SOLVE, PG_DX, PG_APPLY, PG_PHASES };
static_assert(PG_PHASES == ICPMI_PGINFO_PHASES && ICPMI_PGINFO_PHASE_US + PG_PHASES == ICPMI_PGINFO_DOUBLES, "info record");
// the robust kernel's record: the same ten slots, then its own three
static_assert(ICPMI_ROB_COST_BEFORE == ICPMI_PGINFO_DOUBLES && ICPMI_ROB_COST_AFTER == ICPMI_PGINFO_DOUBLES + 1 &&
              ICPMI_ROB_WEIGHTS_US == ICPMI_PGINFO_DOUBLES + 2 && ICPMI_ROB_DOUBLES == ICPMI_PGINFO_DOUBLES + 3, "robust info record");

// phase clocks: thread 0, the 100 MHz wall clock; mark(p) books the time since the last mark to phase p
struct PgClock {
    long long acc[PG_PHASES] = {0, 0, 0, 0, 0, 0, 0}, last = wall_clock64();
    __device__ __forceinline__ void mark(PgPhase p) {
        if (threadIdx.x == 0) { const long long now = wall_clock64(); acc[p] += now - last; last = now; }
    }
    __device__ __forceinline__ long long lap() {                  // the time since the last mark, for a clock kept elsewhere
        long long d = 0;
        if (threadIdx.x == 0) { const long long now = wall_clock64(); d = now - last; last = now; }
        return d;
    }
};

// ── 3x3 helpers (row-major, fully unrolled) ─────────────────────────────────
struct M3 { double a[9]; };
__device__ __forceinline__ M3 m3_zero() { M3 r; for (int i = 0; i < 9; ++i) r.a[i] = 0.0; return r; }
__device__ __forceinline__ M3 m3_load(const double* p) { M3 r; for (int i = 0; i < 9; ++i) r.a[i] = p[i]; return r; }
__device__ __forceinline__ void m3_store(double* p, const M3& m) { for (int i = 0; i < 9; ++i) p[i] = m.a[i]; }
__device__ __forceinline__ M3 m3_mul(const M3& x, const M3& y) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[3 * i + j] = (x.a[3 * i] * y.a[j] + x.a[3 * i + 1] * y.a[3 + j]) + x.a[3 * i + 2] * y.a[6 + j];
    return r;
}
__device__ __forceinline__ M3 m3_tmul(const M3& x, const M3& y) {      // x^T y
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[3 * i + j] = (x.a[i] * y.a[j] + x.a[3 + i] * y.a[3 + j]) + x.a[6 + i] * y.a[6 + j];
    return r;
}
__device__ __forceinline__ void m3_add(M3& x, const M3& y) { for (int i = 0; i < 9; ++i) x.a[i] += y.a[i]; }
__device__ __forceinline__ void m3_sub(M3& x, const M3& y) { for (int i = 0; i < 9; ++i) x.a[i] -= y.a[i]; }
__device__ __forceinline__ void m3_vec(const M3& m, const double* v, double* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (m.a[3 * i] * v[0] + m.a[3 * i + 1] * v[1]) + m.a[3 * i + 2] * v[2];
}
__device__ __forceinline__ void m3_tvec(const M3& m, const double* v, double* out) {   // m^T v
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (m.a[i] * v[0] + m.a[3 + i] * v[1]) + m.a[6 + i] * v[2];
}
// inverse by cofactors; false when the determinant is exactly zero
__device__ __forceinline__ bool m3_inv(const M3& m, M3& r) {
    const double* a = m.a;
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
    if (det == 0.0 || !(fabs(det) < 1e308)) return false;
    const double id = 1.0 / det;
    r.a[0] = c0 * id; r.a[1] = (a[2] * a[7] - a[1] * a[8]) * id; r.a[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    r.a[3] = c1 * id; r.a[4] = (a[0] * a[8] - a[2] * a[6]) * id; r.a[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    r.a[6] = c2 * id; r.a[7] = (a[1] * a[6] - a[0] * a[7]) * id; r.a[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}

// normalize_angle, pose_graph.py:15-17, with Python's float modulo (result takes the sign of the divisor)
__device__ __forceinline__ double pg_wrap(double a) {
    double r = fmod(a + PG_PI, PG_2PI);
    if (r < 0.0) r += PG_2PI;
    return r - PG_PI;
}

// _error_and_jacobians, pose_graph.py:138-182
__device__ __forceinline__ void pg_linearise(const double* xi, const double* xj, const double* z, double* e, M3& A, M3& B) {
    const double ci = cos(xi[2]), si = sin(xi[2]);
    const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
    e[0] = (ci * dx + si * dy) - z[0];
    e[1] = (-si * dx + ci * dy) - z[1];
    e[2] = pg_wrap(pg_wrap(xj[2] - xi[2]) - z[2]);
    A = m3_zero(); B = m3_zero();
    A.a[0] = -ci; A.a[1] = -si; A.a[3] = si; A.a[4] = -ci;
    A.a[2] = -si * dx + ci * dy;
    A.a[5] = -ci * dx + -si * dy;
    A.a[8] = -1.0;
    B.a[0] = ci; B.a[1] = si; B.a[3] = -si; B.a[4] = ci; B.a[8] = 1.0;
}

// ── workgroup-wide helpers ───────────────────────────────────────────────────
__device__ __forceinline__ double block_total(double v, double* s_val) {
    s_val[threadIdx.x] = v;
    __syncthreads();
    for (int o = PG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_val[threadIdx.x] += s_val[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s_val[0];
    __syncthreads();
    return r;
}

// Solve a x = rhs (a: N x N row-major in global memory, destroyed; x may alias rhs) by Gaussian elimination
// with partial pivoting, the whole workgroup on one system.  false = a pivot is exactly zero (LAPACK's
// "singular matrix", the LinAlgError of pose_graph.py:117-119).
__device__ bool block_lu_solve(double* a, int N, double* rhs, double* s_val, int* s_idx) {
    const int tid = threadIdx.x;
    const int tx = tid & 31, ty = tid >> 5;                       // update tile: 32 columns x (PG_THREADS / 32) rows
    for (int p = 0; p < N; ++p) {
        if (wave_id() == 0) {                                     // pivot search: one wave, no workgroup barriers
            double best = -1.0; int bi = 0x7fffffff;
            for (int r = p + lane_id(); r < N; r += ICPMI_WAVE) {
                const double v = fabs(a[(size_t)r * N + p]);
                if (v > best) { best = v; bi = r; }
            }
            wave_first_best(best, bi, [](double x, double y) { return x > y; });      // the lowest row among equal |a|
            if (lane_id() == 0) { s_val[0] = best; s_idx[0] = bi; }
        }
        __syncthreads();
        const double pv = s_val[0];
        const int pr = s_idx[0];
        if (!(pv > 0.0)) return false;
        if (pr != p) {
            for (int c = p + tid; c < N; c += PG_THREADS) {       // columns left of p are never read again
                const double t = a[(size_t)p * N + c];
                a[(size_t)p * N + c] = a[(size_t)pr * N + c];
                a[(size_t)pr * N + c] = t;
            }
            if (tid == 0) { const double t = rhs[p]; rhs[p] = rhs[pr]; rhs[pr] = t; }
        }
        __syncthreads();
        // eliminate column p from the rows below; column p itself is only read here, so every thread takes its
        // row's multiplier from it directly (column index N stands for the right-hand side)
        const double piv = a[(size_t)p * N + p];
        for (int r = p + 1 + ty; r < N; r += PG_THREADS / 32) {
            const double l = a[(size_t)r * N + p] / piv;
            for (int c = p + 1 + tx; c <= N; c += 32) {
                if (c == N) rhs[r] -= l * rhs[p];
                else a[(size_t)r * N + c] -= l * a[(size_t)p * N + c];
            }
        }
        __syncthreads();
    }
    for (int r = N - 1; r >= 0; --r) {                                                     // back substitution
        if (tid == 0) rhs[r] = rhs[r] / a[(size_t)r * N + r];
        __syncthreads();
        const double xr = rhs[r];
        for (int q = tid; q < r; q += PG_THREADS) rhs[q] -= a[(size_t)q * N + r] * xr;
        __syncthreads();
    }
    return true;
}

// ── assemble: linearise every edge and gather per node (pose_graph.py:96-105) ──
// One loop for both paths (see the head of the file): what a node gathers is the same, where it is stored differs.
template <class E> __device__ __forceinline__ M3 pg_edge_omega(const typename E::Args& g, int q) {
    M3 r = m3_load(g.omega + 9 * (size_t)q);
    for (int i = 0; i < 9; ++i) r.a[i] = E::weigh(g, q, r.a[i]);
    return r;
}
template <class E> __device__ __forceinline__ void pg_assemble(const typename E::Args& g) {
    const int tid = threadIdx.x, n = g.n, ncols = g.ncols, N3 = g.N3, f = g.fix;
    for (int v = tid; v < n; v += PG_THREADS) {
        M3 D = m3_zero(), U = m3_zero(), L = m3_zero();
        double b[3] = {0.0, 0.0, 0.0};
        for (int t = g.csr_ptr[v]; t < g.csr_ptr[v + 1]; ++t) {
            const int q = g.csr_edge[t];
            const int i = g.ei[q], j = g.ej[q];
            double e[3], tmp[3], Oe[3];
            M3 A, B;
            pg_linearise(g.nodes + 3 * i, g.nodes + 3 * j, g.z + 3 * q, e, A, B);
            const M3 Om = pg_edge_omega<E>(g, q);
            const M3 OA = m3_mul(Om, A), OB = m3_mul(Om, B);
            m3_vec(Om, e, Oe);
            const bool in_T = g.dense || g.loop_slot[q] < 0;
            if (i == v) {
                m3_tvec(A, Oe, tmp); b[0] += tmp[0]; b[1] += tmp[1]; b[2] += tmp[2];
                if (in_T) m3_add(D, m3_tmul(A, OA));
            }
            if (j == v) {
                m3_tvec(B, Oe, tmp); b[0] += tmp[0]; b[1] += tmp[1]; b[2] += tmp[2];
                if (in_T) m3_add(D, m3_tmul(B, OB));
            }
            if (g.dense) {
                if (i == v && j != f && v != f) {                    // H[i][j] += A^T O B (row block owned by this thread)
                    const M3 c = m3_tmul(A, OB);
                    for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.Hd[(size_t)(3 * v + r) * N3 + 3 * j + cc] += c.a[3 * r + cc];
                }
                if (j == v && i != f && v != f) {                    // H[j][i] += B^T O A
                    const M3 c = m3_tmul(B, OA);
                    for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.Hd[(size_t)(3 * v + r) * N3 + 3 * i + cc] += c.a[3 * r + cc];
                }
            } else if (in_T && v == min(i, j) && i != j) {
                if (i == v) { m3_add(U, m3_tmul(A, OB)); m3_add(L, m3_tmul(B, OA)); }
                else { m3_add(U, m3_tmul(B, OA)); m3_add(L, m3_tmul(A, OB)); }
            }
        }
        if (v == f) {                                                // anchor, pose_graph.py:107-112
            D = m3_zero(); D.a[0] = D.a[4] = D.a[8] = 1e10;
            U = m3_zero(); L = m3_zero();
            b[0] = b[1] = b[2] = 0.0;
        }
        if (v + 1 == f) { U = m3_zero(); L = m3_zero(); }
        if (g.dense) {
            if (v == f) { for (int r = 0; r < 3; ++r) g.Hd[(size_t)(3 * v + r) * N3 + 3 * v + r] = 1e10; }
            else for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.Hd[(size_t)(3 * v + r) * N3 + 3 * v + cc] += D.a[3 * r + cc];
            for (int c = 0; c < 3; ++c) g.dx[3 * v + c] = -b[c];
        } else {
            // per node: D[v] = H[v][v], U[v] = H[v][v+1] (zero for the last node), L[v] = H[v][v-1] (zero for node 0)
            m3_store(g.D + 9 * (size_t)v, D); m3_store(g.U + 9 * (size_t)v, U);
            if (v + 1 < n) m3_store(g.L + 9 * (size_t)(v + 1), L);
            if (v == 0) m3_store(g.L, m3_zero());
            for (int c = 0; c < 3; ++c) g.X[(size_t)(3 * v + c) * ncols] = -b[c];           // column 0: r = -b
        }
    }
    __syncthreads();
}

// ── closure columns: right-hand sides 1..3k of X, the Jacobian columns W of the non-chain edges ──
template <class G> __device__ __forceinline__ void pg_closure_columns(const G& g) {
    const int K = g.K, ncols = g.ncols, f = g.fix;
    for (size_t t = threadIdx.x; t < (size_t)g.N3 * (size_t)K; t += PG_THREADS) g.X[(t / K) * ncols + 1 + (t % K)] = 0.0;
    __syncthreads();
    for (int q = threadIdx.x; q < g.k; q += PG_THREADS) {
        const int eq = g.loop_edge[q], i = g.ei[eq], j = g.ej[eq];
        double e[3];
        M3 A, B;
        pg_linearise(g.nodes + 3 * i, g.nodes + 3 * j, g.z + 3 * eq, e, A, B);     // the Jacobians alone: no Omega here
        m3_store(g.AB + 18 * (size_t)q, A); m3_store(g.AB + 18 * (size_t)q + 9, B);
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {                        // W_e = [A^T ; B^T]: rows of node i / j, column 3q + a
                if (i != f) g.X[(size_t)(3 * i + c) * ncols + 1 + 3 * q + a] += A.a[3 * a + c];
                if (j != f) g.X[(size_t)(3 * j + c) * ncols + 1 + 3 * q + a] += B.a[3 * a + c];
            }
    }
    __syncthreads();
}

// ── closure system: M = I + C W^T Y, g = C W^T T^-1 r ─────────────────────────
template <class E> __device__ __forceinline__ void pg_closure_system(const typename E::Args& g) {
    const int K = g.K, ncols = g.ncols, f = g.fix;
    for (int t = threadIdx.x; t < K * (K + 1); t += PG_THREADS) {
        const int r = t / (K + 1), c = t % (K + 1);                  // c == K: the right-hand side (column 0 of X)
        const int q = r / 3, a = r % 3;
        const int eq = g.loop_edge[q];
        const int i = g.ei[eq], j = g.ej[eq];
        const int col = c == K ? 0 : 1 + c;
        const double* AB = g.AB + 18 * (size_t)q;
        const double* Om = g.omega + 9 * (size_t)eq;
        double acc = 0.0;
        for (int bb = 0; bb < 3; ++bb) {
            double s = 0.0;
            for (int cc = 0; cc < 3; ++cc) {
                if (i != f) s += AB[3 * bb + cc] * g.X[(size_t)(3 * i + cc) * ncols + col];
                if (j != f) s += AB[9 + 3 * bb + cc] * g.X[(size_t)(3 * j + cc) * ncols + col];
            }
            acc += E::weigh(g, eq, Om[3 * a + bb]) * s;
        }
        if (c == K) g.g[r] = acc;
        else g.M[(size_t)r * K + c] = acc + (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
}

// ── dx = Y[:, 0] - Y[:, 1:] y (y in g.g): 16 lanes per row, lanes along the row (coalesced), fixed-tree sum ──
template <class G> __device__ __forceinline__ void pg_dx(const G& g) {
    const int tid = threadIdx.x, l16 = tid & 15, K = g.K, ncols = g.ncols, N3 = g.N3;
    for (int t0 = 0; t0 < N3; t0 += PG_THREADS / 16) {                           // uniform trip count
        const int t = min(t0 + (tid >> 4), N3 - 1);
        double part = 0.0;
        for (int c = l16; c < K; c += 16) part += g.X[(size_t)t * ncols + 1 + c] * g.g[c];
        const double tot = row_sum(part);
        if (l16 == 0 && t0 + (tid >> 4) < N3) g.dx[t] = g.X[(size_t)t * ncols] - tot;
    }
}

// ── apply the update, pose_graph.py:121-129; returns the norm of the step ─────
template <class G> __device__ __forceinline__ double pg_apply(const G& g, double* s_val) {
    double ss = 0.0;
    for (int v = threadIdx.x; v < g.n; v += PG_THREADS) {
        const double d0 = g.dx[3 * v], d1 = g.dx[3 * v + 1], d2 = g.dx[3 * v + 2];
        g.nodes[3 * v] += d0;
        g.nodes[3 * v + 1] += d1;
        g.nodes[3 * v + 2] = pg_wrap(g.nodes[3 * v + 2] + d2);
        ss += (d0 * d0 + d1 * d1) + d2 * d2;
    }
    return sqrt(block_total(ss, s_val));
}

// ── weights (robust kernel only): chi2_q = e^T Omega e of every edge of the caller's list, evaluated as
// pose_graph_error_kernel evaluates it with the caller's Omega, and on a masked edge w_q = rho'(chi2_q), c = delta^2:
//     Huber           rho = s (s <= c), 2 delta sqrt(s) - c     w = 1 (s <= c), delta / sqrt(s)
//     Cauchy          rho = c log1p(s / c)                      w = c / (c + s)
//     Geman-McClure   rho = (c / (c + s)) s                     w = (c / (c + s))^2
// Every other edge, and every twin, has rho = s and w = 1.0.  Returns the cost, sum of rho: per thread in edge order
// (edges tid, tid + PG_THREADS, ...), then block_total's tree.
__device__ __forceinline__ double pg_weights(const PgRobArgs& g, double* s_val) {
    const double c = g.delta * g.delta;
    double part = 0.0;
    for (int q = threadIdx.x; q < g.m; q += PG_THREADS) {
        double w = 1.0;
        if (q < g.m0) {
            double e[3], Oe[3];
            M3 A, B;
            pg_linearise(g.nodes + 3 * g.ei[q], g.nodes + 3 * g.ej[q], g.z + 3 * q, e, A, B);
            m3_vec(m3_load(g.omega0 + 9 * (size_t)q), e, Oe);
            const double s = (e[0] * Oe[0] + e[1] * Oe[1]) + e[2] * Oe[2];
            double rho = s;
            if (g.rob[q]) {
                if (g.kernel == ICPMI_ROB_KERNEL_HUBER) {
                    if (!(s <= c)) { const double r = sqrt(s); w = g.delta / r; rho = (2.0 * g.delta) * r - c; }
                } else {
                    const double t = c / (c + s);
                    if (g.kernel == ICPMI_ROB_KERNEL_CAUCHY) { w = t; rho = c * log1p(s / c); }
                    else { w = t * t; rho = t * s; }
                }
            }
            g.edge_chi2[q] = s;
            g.edge_weight[q] = w;
            part += rho;
        }
        g.wgt[q] = w;
    }
    return block_total(part, s_val);
}

// ── the optimisation: every iteration of both kernels.  E: how an edge's Omega enters (PgPlainEdges, PgWeightedEdges) ──
// s_val, s_idx, s_flag: the kernel's LDS (s_flag: a block of T turned out exactly singular)
template <class E> __device__ __forceinline__ void pg_gauss_newton(const typename E::Args& g, double* s_val, int* s_idx, int& s_flag) {
    int status = ICPMI_PG_ST_MAXITER, iters = g.n_iter;
    double step = 0.0;
    PgClock clock;
    [[maybe_unused]] double cost = 0.0, cost_before = 0.0;
    [[maybe_unused]] long long weights_clock = 0;
    const int tid = threadIdx.x, n = g.n, ncols = g.ncols;
    for (int it = 0; it < g.n_iter; ++it) {
        if (threadIdx.x == 0) s_flag = 0;
        if (g.dense) for (size_t t = threadIdx.x; t < (size_t)g.N3 * g.N3; t += PG_THREADS) g.Hd[t] = 0.0;
        __syncthreads();
        bool singular = false, refused = false;
        if constexpr (E::weighted) {
            cost = pg_weights(g, s_val);
            if (it == 0) cost_before = cost;
            weights_clock += clock.lap();
        }
        pg_assemble<E>(g);
        clock.mark(PG_ASSEMBLE);
        if (g.dense) singular = !block_lu_solve(g.Hd, g.N3, g.dx, s_val, s_idx);
        else {
            pg_closure_columns(g);
            clock.mark(PG_CLOSURE_COLUMNS);
            // ── chain solve: T^-1 on every column of X by block cyclic reduction along the chain ──
            // Level with stride s: the nodes that are odd multiples of s are eliminated into their neighbours at
            // distance s (which then couple at distance 2s); log2(n) levels, every level parallel over nodes and
            // columns.  An eliminated node keeps its inverted diagonal block and its two couplings for the way back.
            int s = 1;
            for (; s < n; s <<= 1) {
                for (int idx = tid; s * (2 * idx + 1) < n; idx += PG_THREADS) {          // odd nodes: invert the diagonal block
                    const int i = s * (2 * idx + 1);
                    M3 inv;
                    if (!m3_inv(m3_load(g.D + 9 * (size_t)i), inv)) s_flag = 1;
                    m3_store(g.D + 9 * (size_t)i, inv);
                }
                __syncthreads();
                for (int idx = tid; 2 * s * idx < n; idx += PG_THREADS) {                // even nodes: absorb both odd neighbours
                    const int e = 2 * s * idx, i1 = e - s, i2 = e + s;
                    M3 P = m3_zero(), Q = m3_zero(), Dn = m3_load(g.D + 9 * (size_t)e), Ln = m3_zero(), Un = m3_zero();
                    if (i1 >= 0) {
                        P = m3_mul(m3_load(g.L + 9 * (size_t)e), m3_load(g.D + 9 * (size_t)i1));
                        m3_sub(Dn, m3_mul(P, m3_load(g.U + 9 * (size_t)i1)));
                        Ln = m3_mul(P, m3_load(g.L + 9 * (size_t)i1));
                        for (int c = 0; c < 9; ++c) Ln.a[c] = -Ln.a[c];
                    }
                    if (i2 < n) {
                        Q = m3_mul(m3_load(g.U + 9 * (size_t)e), m3_load(g.D + 9 * (size_t)i2));
                        m3_sub(Dn, m3_mul(Q, m3_load(g.L + 9 * (size_t)i2)));
                        Un = m3_mul(Q, m3_load(g.U + 9 * (size_t)i2));
                        for (int c = 0; c < 9; ++c) Un.a[c] = -Un.a[c];
                    }
                    m3_store(g.Dinv + 9 * (size_t)e, P); m3_store(g.G + 9 * (size_t)e, Q);
                    m3_store(g.D + 9 * (size_t)e, Dn); m3_store(g.L + 9 * (size_t)e, Ln); m3_store(g.U + 9 * (size_t)e, Un);
                }
                __syncthreads();
                const int n_even = (n + 2 * s - 1) / (2 * s);
                for (int t = tid; t < n_even * ncols; t += PG_THREADS) {                 // right-hand sides of the even nodes
                    const int e = 2 * s * (t / ncols), col = t % ncols, i1 = e - s, i2 = e + s;
                    double r[3], x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0}, t1[3], t2[3];
                    for (int c = 0; c < 3; ++c) r[c] = g.X[(size_t)(3 * e + c) * ncols + col];
                    if (i1 >= 0) for (int c = 0; c < 3; ++c) x1[c] = g.X[(size_t)(3 * i1 + c) * ncols + col];
                    if (i2 < n) for (int c = 0; c < 3; ++c) x2[c] = g.X[(size_t)(3 * i2 + c) * ncols + col];
                    m3_vec(m3_load(g.Dinv + 9 * (size_t)e), x1, t1);
                    m3_vec(m3_load(g.G + 9 * (size_t)e), x2, t2);
                    for (int c = 0; c < 3; ++c) g.X[(size_t)(3 * e + c) * ncols + col] = (r[c] - t1[c]) - t2[c];
                }
                __syncthreads();
            }
            if (tid == 0) {                                                              // the last node standing: node 0
                M3 inv;
                if (!m3_inv(m3_load(g.D), inv)) s_flag = 1;
                m3_store(g.D, inv);
            }
            __syncthreads();
            refused = s_flag != 0;                                                       // a block of T is exactly singular
            if (!refused) {
                for (int col = tid; col < ncols; col += PG_THREADS) {
                    double r[3], x[3];
                    for (int c = 0; c < 3; ++c) r[c] = g.X[(size_t)c * ncols + col];
                    m3_vec(m3_load(g.D), r, x);
                    for (int c = 0; c < 3; ++c) g.X[(size_t)c * ncols + col] = x[c];
                }
                __syncthreads();
                // back-substitute: node 0 above, then the odd nodes of every level from the top stride down; X becomes T^-1 [r W]
                for (s >>= 1; s >= 1; s >>= 1) {
                    const int n_odd = (n - s + 2 * s - 1) / (2 * s);                     // nodes s, 3s, 5s, ... below n
                    for (int t = tid; t < n_odd * ncols; t += PG_THREADS) {
                        const int i = s * (2 * (t / ncols) + 1), col = t % ncols, a = i - s, b = i + s;
                        double r[3], xa[3], xb[3] = {0.0, 0.0, 0.0}, t1[3], t2[3], w[3], x[3];
                        for (int c = 0; c < 3; ++c) { r[c] = g.X[(size_t)(3 * i + c) * ncols + col]; xa[c] = g.X[(size_t)(3 * a + c) * ncols + col]; }
                        if (b < n) for (int c = 0; c < 3; ++c) xb[c] = g.X[(size_t)(3 * b + c) * ncols + col];
                        m3_vec(m3_load(g.L + 9 * (size_t)i), xa, t1);
                        m3_vec(m3_load(g.U + 9 * (size_t)i), xb, t2);
                        for (int c = 0; c < 3; ++c) w[c] = (r[c] - t1[c]) - t2[c];
                        m3_vec(m3_load(g.D + 9 * (size_t)i), w, x);
                        for (int c = 0; c < 3; ++c) g.X[(size_t)(3 * i + c) * ncols + col] = x[c];
                    }
                    __syncthreads();
                }
                clock.mark(PG_CHAIN_SOLVE);
                if (g.k > 0) {
                    pg_closure_system<E>(g);
                    clock.mark(PG_CLOSURE_SYSTEM);
                    refused = !block_lu_solve(g.M, g.K, g.g, s_val, s_idx);           // y, in place of g
                    clock.mark(PG_CLOSURE_SOLVE);
                }
                if (!refused) pg_dx(g);
            }
        }
        __syncthreads();
        clock.mark(PG_DX);                                       // on the dense path: the whole elimination
        if (singular) { status = ICPMI_PG_ST_SINGULAR; iters = it; break; }      // pose_graph.py:117-119: nodes keep their values
        if (refused) { status = ICPMI_PG_ST_REFUSED; iters = it; break; }        // nodes keep their values; the caller goes on densely
        step = pg_apply(g, s_val);
        clock.mark(PG_APPLY);
        if (step < g.eps) { status = ICPMI_PG_ST_CONVERGED; iters = it + 1; break; }
    }
    if constexpr (E::weighted) {                                 // chi2, weights and the cost of the poses that are returned
        cost = pg_weights(g, s_val);
        if (g.n_iter == 0) cost_before = cost;
        weights_clock += clock.lap();
    }
    if (threadIdx.x == 0) {
        g.info[ICPMI_PGINFO_ITERATIONS] = (double)iters; g.info[ICPMI_PGINFO_STATUS] = (double)status; g.info[ICPMI_PGINFO_STEP] = step;
        for (int i = 0; i < PG_PHASES; ++i) g.info[ICPMI_PGINFO_PHASE_US + i] = (double)clock.acc[i] * 0.01;      // microseconds, all iterations
        if constexpr (E::weighted) {
            g.info[ICPMI_ROB_COST_BEFORE] = cost_before; g.info[ICPMI_ROB_COST_AFTER] = cost;
            g.info[ICPMI_ROB_WEIGHTS_US] = (double)weights_clock * 0.01;
        }
    }
}

__global__ __launch_bounds__(PG_THREADS) void pose_graph_kernel(PgArgs g) {
    __shared__ double s_val[PG_THREADS];
    __shared__ int s_idx[PG_THREADS];
    __shared__ int s_flag;
    pg_gauss_newton<PgPlainEdges>(g, s_val, s_idx, s_flag);
}
__global__ __launch_bounds__(PG_THREADS) void pose_graph_robust_kernel(PgRobArgs g) {
    __shared__ double s_val[PG_THREADS];
    __shared__ int s_idx[PG_THREADS];
    __shared__ int s_flag;
    pg_gauss_newton<PgWeightedEdges>(g, s_val, s_idx, s_flag);
}

// total_error, pose_graph.py:189-194: e^T Omega e summed in edge order
__global__ __launch_bounds__(PG_THREADS) void pose_graph_error_kernel(const double* nodes, const int32_t* ei, const int32_t* ej,
                                                                      const double* z, const double* omega, int m,
                                                                      double* per_edge, double* out) {
    for (int q = threadIdx.x; q < m; q += PG_THREADS) {
        double e[3], Oe[3];
        M3 A, B;
        pg_linearise(nodes + 3 * ei[q], nodes + 3 * ej[q], z + 3 * q, e, A, B);
        m3_vec(m3_load(omega + 9 * (size_t)q), e, Oe);
        per_edge[q] = (e[0] * Oe[0] + e[1] * Oe[1]) + e[2] * Oe[2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < m; ++q) t += per_edge[q];
        out[0] = t;
    }
}

// ── the host plan: everything a launch needs, decided without a HIP call ─────
struct PgPlan {
    int rc = ICPMI_OK;                             // ICPMI_ERR_ARG: an edge names a node outside the graph
    bool refused = false;                          // a chain edge without information along some direction: no split, no launch
    int k = 0, dense = 0, m2 = 0, twins = 0;       // m2: edges after the weak chain edges got their twins
    std::vector<int32_t> weak;                     // [twins] ids of the weak chain edges
    double stiff = 0.0;                            // the information a weak chain edge keeps inside T (times I)
    std::vector<int32_t> ei_ej, csr_ptr, csr_edge, loop_slot, loop_edge;     // ei_ej: [m2] ei, then [m2] ej, the twins appended
    std::vector<double> z, omega;                  // [m2][3], [m2][9] with the twins' rows: add_twin_rows, only where there are twins
    // the caller's Omega and z ([m][9], [m][3] on the host) with the twins' rows: the chain edge keeps S I, its twin gets the rest
    void add_twin_rows(const double* omega_host, const double* z_host, int m) {
        z.assign(z_host, z_host + 3 * (size_t)m); z.resize(3 * (size_t)m2);
        omega.assign(omega_host, omega_host + 9 * (size_t)m); omega.resize(9 * (size_t)m2);
        for (int t = 0; t < twins; ++t) {
            const size_t q = (size_t)weak[t], q2 = (size_t)m + t;
            for (int c = 0; c < 3; ++c) z[3 * q2 + c] = z[3 * q + c];
            for (int c = 0; c < 9; ++c) {
                const double s = c % 4 == 0 ? stiff : 0.0;
                omega[9 * q2 + c] = omega[9 * q + c] - s;
                omega[9 * q + c] = s;
            }
        }
    }
};

// Classify the edges (host side: the edge list is a few KB of integers the caller holds on the host anyway).
//
// With the information matrices at hand (omega: [m][9] on the host, or null) the chain edges too weak for T are found
// here.  The split inverts T without the closures, and what it loses against a solve of the whole system grows with
// S / lambda, S the largest information in the graph and lambda the smallest of a chain edge: T^-1 r grows with
// 1 / lambda, the step does not, and the difference of the two cancels that many digits (measured: the step error is
// proportional to 1 / eps for Omega = diag(eps, 1e4, 1e4)).  A step may be off by 3n times what a stable solve of the
// whole system leaves, so a chain edge counts as weak when lambda < S / (3n), lambda the smallest eigenvalue of the
// symmetric part.  A weak edge (i, j, z, Omega) is split in two that sum to it: (i, j, z, S I) stays in the chain, so T
// is as stiff there as anywhere, and its twin (i, j, z, Omega - S I) goes with the closures, whose system is eliminated
// with pivoting.  An edge with an eigenvalue that is zero to rounding (|lambda| <= 64 u max |lambda|: the closed form
// below is good to a few u of the largest) may leave the whole system exactly singular, which only the dense elimination
// can tell as the reference's LAPACK call does: such a graph is not split at all.
// The twins' rows of z and Omega need the caller's z on the host too: add_twin_rows completes a plan that has twins;
// without them the plan already has every size and index list, which is all the size queries need.
static void pg_sym_eigenvalues(const double* o, double* e) {                 // symmetric part of a 3 x 3, closed form
    const double a00 = o[0], a11 = o[4], a22 = o[8], a01 = 0.5 * (o[1] + o[3]), a02 = 0.5 * (o[2] + o[6]), a12 = 0.5 * (o[5] + o[7]);
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    if (p1 == 0.0) { e[0] = a00; e[1] = a11; e[2] = a22; return; }
    const double q = (a00 + a11 + a22) / 3.0;
    const double p2 = (a00 - q) * (a00 - q) + (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    const double b00 = (a00 - q) / p, b11 = (a11 - q) / p, b22 = (a22 - q) / p, b01 = a01 / p, b02 = a02 / p, b12 = a12 / p;
    double r = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double phi = acos(r) / 3.0;
    e[0] = q + 2.0 * p * cos(phi);
    e[2] = q + 2.0 * p * cos(phi + 2.0943951023931953);
    e[1] = 3.0 * q - e[0] - e[2];
}

static bool pg_chained(const int32_t* ij, int q) { return ij[2 * q] - ij[2 * q + 1] == 1 || ij[2 * q + 1] - ij[2 * q] == 1; }
// the weak chain edges of a graph that is split (above): p.stiff, p.weak, or p.refused
static void pg_find_weak(PgPlan& p, const int32_t* ij, const double* omega, int n, int m) {
    for (size_t t = 0; t < 9 * (size_t)m; t += 3) p.stiff = fmax(p.stiff, (fabs(omega[t]) + fabs(omega[t + 1])) + fabs(omega[t + 2]));
    for (int q = 0; q < m; ++q) {
        if (!pg_chained(ij, q)) continue;
        double e[3];
        pg_sym_eigenvalues(omega + 9 * (size_t)q, e);
        const double lo = fmin(fmin(e[0], e[1]), e[2]);
        const double amin = fmin(fmin(fabs(e[0]), fabs(e[1])), fabs(e[2])), amax = fmax(fmax(fabs(e[0]), fabs(e[1])), fabs(e[2]));
        if (!(amin > 64 * 0x1p-53 * amax)) p.refused = true;             // all zero and NaN included
        else if (!(lo >= p.stiff / (3.0 * n))) p.weak.push_back(q);
    }
    if (p.refused) p.weak.clear();
}

static PgPlan pg_plan(const int32_t* ij, const double* omega, int n, int m, bool force_dense) {
    PgPlan p;
    p.dense = force_dense;
    const auto chained = [&](int q) { return pg_chained(ij, q); };
    std::vector<char> linked(n > 1 ? n - 1 : 0, 0);
    for (int q = 0; q < m; ++q) {
        const int i = ij[2 * q], j = ij[2 * q + 1];
        if (i < 0 || i >= n || j < 0 || j >= n) { p.rc = ICPMI_ERR_ARG; return p; }
        if (chained(q)) linked[i < j ? i : j] = 1;
    }
    for (char c : linked) if (!c) p.dense = 1;               // a gap in the chain: T would be singular
    if (!p.dense && omega) pg_find_weak(p, ij, omega, n, m);
    p.twins = (int)p.weak.size();
    const int m2 = p.m2 = m + p.twins;
    p.ei_ej.resize(2 * (size_t)m2);
    int32_t *ei = p.ei_ej.data(), *ej = ei + m2;
    for (int q = 0; q < m2; ++q) { const int src = q < m ? q : p.weak[q - m]; ei[q] = ij[2 * src]; ej[q] = ij[2 * src + 1]; }
    p.csr_ptr.assign(n + 1, 0); p.loop_slot.assign(m2, -1);
    for (int q = 0; q < m2; ++q) {
        ++p.csr_ptr[ei[q] + 1];
        if (ej[q] != ei[q]) ++p.csr_ptr[ej[q] + 1];
        if (!p.dense && (q >= m || !chained(q))) { p.loop_slot[q] = p.k++; p.loop_edge.push_back(q); }
    }
    for (int v = 0; v < n; ++v) p.csr_ptr[v + 1] += p.csr_ptr[v];
    p.csr_edge.resize(p.csr_ptr[n]);
    std::vector<int32_t> fill(p.csr_ptr.begin(), p.csr_ptr.end() - 1);
    for (int q = 0; q < m2; ++q) {
        p.csr_edge[fill[ei[q]]++] = q;
        if (ej[q] != ei[q]) p.csr_edge[fill[ej[q]]++] = q;
    }
    return p;
}

// the layout W of a plan over `base`, built base by base (W::Base) down to PgPlanWs; tail: what W lists after its base (MgWs: s, diag)
template <class W, class... Tail> static W pg_layout(void* base, int n, const PgPlan& p, Tail... tail) {
    if constexpr (std::is_same_v<W, PgPlanWs>) return PgPlanWs{base, n, p.m2, p.k, p.dense, p.twins};
    else return W{pg_layout<typename W::Base>(base, n, p), tail...};
}
// a size query: the layout W of the graph's plan, counted over a null base (0: sizes below zero, no edge list, a bad index)
template <class W, class... Tail> static size_t pg_layout_bytes(const int32_t* edges_ij_host, const double* omega_host, int32_t n_nodes,
                                                                int32_t n_edges, bool force_dense, Tail... tail) {
    if (n_nodes < 0 || n_edges < 0 || (n_edges > 0 && !edges_ij_host)) return 0;
    const PgPlan p = pg_plan(edges_ij_host, omega_host, n_nodes, n_edges, force_dense);
    return p.rc == ICPMI_OK ? pg_layout<W>(nullptr, n_nodes, p, tail...).bytes : 0;
}

// host <-> device copies of whole vectors (nothing for an empty one); the caller synchronises
template <class T> static bool pg_upload(T* dst, const std::vector<T>& v, hipStream_t st) {
    return v.empty() || hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess;
}
static bool pg_read_back(std::vector<double>& v, const double* src, size_t count, hipStream_t st) {
    v.resize(count);
    return hipMemcpyAsync(v.data(), src, count * 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
// pageable host memory: the runtime stages these copies before returning; the plan lives until the synchronise anyway
static bool pg_upload_plan(const PgPlanWs& w, const PgPlan& p, hipStream_t st) {
    return pg_upload(w.ei, p.ei_ej, st) && pg_upload(w.csr_ptr, p.csr_ptr, st) && pg_upload(w.csr_edge, p.csr_edge, st) &&
           pg_upload(w.loop_slot, p.loop_slot, st) && pg_upload(w.loop_edge, p.loop_edge, st);
}
// the info record of a call that launches nothing, written from the host
static int pg_write_info(double* info, const double* record, int doubles, hipStream_t st) {
    if (hipMemcpyAsync(info, record, (size_t)doubles * 8, hipMemcpyHostToDevice, st) != hipSuccess) return ICPMI_ERR_HIP;
    return hipStreamSynchronize(st) == hipSuccess ? ICPMI_OK : ICPMI_ERR_HIP;          // `record` is on the caller's stack frame
}

// ── the host front of every entry that runs on a plan: optimize / optimize_dense, optimize_robust, marginals ──
// What an entry hands it: the caller's arguments that all of them have, and what differs between their info records.
struct PgCall {
    const void* nodes;             // only tested for null here
    const int32_t* ij;             // [m][2] on the host
    const double *z, *omega;       // [m][3], [m][9] on the device
    int n, m, n_iter, fix;
    bool dense;                    // the entry's path rule: forced by the caller, or pg_robust_dense
    bool evaluates;                // n_iter == 0 still launches (the robust entry's evaluation-only call); else: a MAXITER record
    double* info;                  // device
    int info_doubles, status_slot, path_slot;      // of a record written here: its length, where its status goes and (or -1) its path
    void* workspace;
    size_t workspace_bytes;
    hipStream_t st;
};
// What it hands back.  Nothing to launch (an error, or a record written here): rc alone.  Else the layout over the
// caller's workspace, the plan uploaded into it, and z / Omega as the kernels are to read them: the caller's, or the rows
// with the twins in the workspace.
template <class W> struct PgStaged {
    int rc;
    std::optional<W> w;
    const double *z, *omega;
};
// extras(w, st): the entry's own uploads and memsets, enqueued in front of the one synchronise (what they read on the
// host lives in the entry's frame); tail: what the layout W lists after its base.  Everything down to the workspace
// check is decided without a HIP call: a refusal of the host costs no round trip and touches no pointer.
template <class W, class Extras, class... Tail> static PgStaged<W> pg_stage(const PgCall& c, Extras extras, Tail... tail) {
    const auto done = [](int rc) { return PgStaged<W>{rc, std::nullopt, nullptr, nullptr}; };
    const auto record = [&](int status) {
        double rec[ICPMI_ROB_DOUBLES] = {};                      // the longest of the three
        static_assert(ICPMI_ROB_DOUBLES >= ICPMI_PGINFO_DOUBLES && ICPMI_ROB_DOUBLES >= ICPMI_MARG_DOUBLES, "info records");
        rec[c.status_slot] = (double)status;
        if (c.path_slot >= 0) rec[c.path_slot] = (double)(c.dense ? ICPMI_MARG_PATH_DENSE : ICPMI_MARG_PATH_SPLIT);
        return done(pg_write_info(c.info, rec, c.info_doubles, c.st));
    };
    if (!c.nodes || !c.info || c.n < 0 || c.m < 0 || c.n_iter < 0) return done(ICPMI_ERR_ARG);
    if (c.m > 0 && (!c.ij || !c.z || !c.omega)) return done(ICPMI_ERR_ARG);
    if (c.n < 2 || c.m == 0) return record(ICPMI_PG_ST_NOTHING);                       // pose_graph.py:89-91
    if (c.n_iter == 0 && !c.evaluates) return record(ICPMI_PG_ST_MAXITER);
    if (c.fix < 0 || c.fix >= c.n) return done(ICPMI_ERR_ARG);
    const int n = c.n, m = c.m;
    PgPlan p = pg_plan(c.ij, nullptr, n, m, c.dense);            // without the matrices: every index and the path, no twins
    if (p.rc != ICPMI_OK) return done(p.rc);
    if (!c.workspace || c.workspace_bytes < pg_layout<W>(nullptr, n, p, tail...).bytes) return done(ICPMI_ERR_WORKSPACE);
    std::vector<double> om, zz;
    if (!p.dense) {                                              // the information matrices, to find the weak chain edges
        if (!pg_read_back(om, c.omega, 9 * (size_t)m, c.st)) return done(ICPMI_ERR_HIP);
        pg_find_weak(p, c.ij, om.data(), n, m);
        if (!p.weak.empty()) p = pg_plan(c.ij, om.data(), n, m, false);      // the lists again, with the twins
    }
    PgStaged<W> s{ICPMI_OK, pg_layout<W>(c.workspace, n, p, tail...), c.z, c.omega};
    const W& w = *s.w;
    // a chain edge with a null direction, or a workspace sized without the information matrices and so without room for
    // the twins: the split is refused before anything is launched and the caller continues on the dense path
    if (p.refused || c.workspace_bytes < w.bytes) return record(ICPMI_PG_ST_REFUSED);
    if (p.twins) {                                               // the twins' rows are made of the caller's z
        if (!pg_read_back(zz, c.z, 3 * (size_t)m, c.st)) return done(ICPMI_ERR_HIP);
        p.add_twin_rows(om.data(), zz.data(), m);
        if (!pg_upload(w.tw_omega, p.omega, c.st) || !pg_upload(w.tw_z, p.z, c.st)) return done(ICPMI_ERR_HIP);
        s.z = w.tw_z; s.omega = w.tw_omega;
    }
    if (!pg_upload_plan(w, p, c.st) || !extras(w, c.st)) return done(ICPMI_ERR_HIP);
    if (hipStreamSynchronize(c.st) != hipSuccess) return done(ICPMI_ERR_HIP);          // the plan's vectors are on this stack frame
    return s;
}

static int pg_optimize(double* nodes, const int32_t* edges_ij_host, const double* edges_z, const double* edges_omega,
                       int32_t n_nodes, int32_t n_edges, int32_t n_iterations, int32_t fix_node, double convergence_eps,
                       double* info, void* workspace, size_t workspace_bytes, void* stream, bool force_dense) {
    hipStream_t st = (hipStream_t)stream;
    const PgCall c{nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, n_iterations, fix_node, force_dense, false,
                   info, ICPMI_PGINFO_DOUBLES, ICPMI_PGINFO_STATUS, -1, workspace, workspace_bytes, st};
    const PgStaged<PgWs> s = pg_stage<PgWs>(c, [](const PgWs&, hipStream_t) { return true; });
    if (!s.w) return s.rc;
    const PgArgs a{*s.w, {nodes, s.z, s.omega, n_iterations, fix_node, convergence_eps, info}};
    pose_graph_kernel<<<1, PG_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// ── the robust optimiser's host side ─────────────────────────────────────────
// A masked chain edge cannot stay in T (its weight would move T's stiffness under the plan): such a graph is planned
// dense, like force_dense.  The weak-edge rule stays on the caller's unweighted Omega.
static bool pg_robust_dense(const int32_t* ij, const uint8_t* mask, int m, bool force_dense) {
    for (int q = 0; q < m && !force_dense; ++q) {
        const int d = ij[2 * q] - ij[2 * q + 1];
        if (mask[q] && (d == 1 || d == -1)) force_dense = true;
    }
    return force_dense;
}
static size_t pg_robust_workspace_bytes(const int32_t* edges_ij_host, const double* omega_host, const uint8_t* mask_host,
                                        int32_t n_nodes, int32_t n_edges, bool force_dense) {
    if (n_edges > 0 && (!edges_ij_host || !mask_host)) return 0;
    return pg_layout_bytes<PgRobWs>(edges_ij_host, omega_host, n_nodes, n_edges,
                                    pg_robust_dense(edges_ij_host, mask_host, n_edges, force_dense));
}

static int pg_optimize_robust(double* nodes, const int32_t* edges_ij_host, const double* edges_z, const double* edges_omega,
                              const uint8_t* mask_host, int32_t n_nodes, int32_t n_edges, int32_t n_iterations, int32_t fix_node,
                              double convergence_eps, int32_t kernel, double delta, bool force_dense, double* edge_chi2,
                              double* edge_weight, double* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!edge_chi2 || !edge_weight || (n_edges > 0 && (!edges_ij_host || !mask_host))) return ICPMI_ERR_ARG;
    if (kernel != ICPMI_ROB_KERNEL_HUBER && kernel != ICPMI_ROB_KERNEL_CAUCHY && kernel != ICPMI_ROB_KERNEL_GEMAN_MCCLURE) return ICPMI_ERR_ARG;
    if (!(delta > 0.0)) return ICPMI_ERR_ARG;                // NaN included
    hipStream_t st = (hipStream_t)stream;
    const PgCall c{nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, n_iterations, fix_node,
                   pg_robust_dense(edges_ij_host, mask_host, n_edges, force_dense), true,
                   info, ICPMI_ROB_DOUBLES, ICPMI_PGINFO_STATUS, -1, workspace, workspace_bytes, st};
    std::vector<uint8_t> rob;                                // [m2] the caller's mask, then the twins: unmasked by construction
    const PgStaged<PgRobWs> s = pg_stage<PgRobWs>(c, [&](const PgRobWs& w, hipStream_t st) {
        rob.assign(mask_host, mask_host + n_edges);
        rob.resize(w.m, 0);
        return pg_upload(w.rob, rob, st);
    });
    if (!s.w) return s.rc;
    const PgRobArgs a{*s.w, {nodes, s.z, s.omega, n_iterations, fix_node, convergence_eps, info}, edges_omega, n_edges, kernel, delta,
                      edge_chi2, edge_weight};
    pose_graph_robust_kernel<<<1, PG_THREADS, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

// ═════════════════════════════════════════════════════════════════════════════
// Marginals: 3 x 3 blocks of H^-1, H the matrix pose_graph.py:93-114 assembles at the current nodes (nothing is
// iterated, the nodes are only read).  Two outputs, either may be left out:
//     diagonal  block (v, v) of every node                      [n][9]
//     columns   block (v, S[a]) of every node, S the selection  [s][n][9]
// Split path, on the same plan as the optimiser (chain / closures, twins of weak chain edges), H = T + W C W^T:
//     H^-1 = T^-1 - Y (I + C W^T Y)^-1 C W^T T^-1,      Y = T^-1 W.
//   T = block LU along the chain: left Schur complements Sl[v] = D[v] - L[v] Sl[v-1]^-1 U[v-1], kept inverted.  The
//   sweep is SERIAL in n (one thread); so are the two substitutions of a chain solve, which run one column per lane
//   over the whole grid.  The transposed solve Z = T^-T W reuses the factors (the left Schur complements of T^T are
//   the transposes of those of T).
//   columns:  V = T^-1 E_S,  y = M^-1 (C W^T V),  block (v, S[a]) = V - Y y            (M = I + C W^T Y, pivoted LU)
//   diagonal: G[v] = (T^-1)[v][v] by a second serial sweep, from the last node down, that only adds:
//             G[n-1] = Sl[n-1]^-1,  G[v] = Sl[v]^-1 + (Sl[v]^-1 U[v]) G[v+1] (L[v+1] Sl[v]^-1);
//             the correction of node v is the columns' own, with the node's three right-hand sides read off Z:
//             C W^T T^-1 E_v = C Z_v^T,  y_v = M^-1 (C Z_v^T),  block (v, v) = G[v] - Y_v y_v.
//             (Two forms that cost the same lose digits the bound does not allow, in NumPy float64 on the test graphs:
//             inverting D - L Sl^-1 U - U Sr^-1 L cancels where the chain alone is loose, up to 14 times the bound;
//             Y_v (M^-1 C) Z_v^T pays the full condition of M, up to 26 times.  This one stays below 0.4 of it there and
//             below 0.71 on the device.)
// Dense path (gap in the chain, other numbering, forced): the reference's dense matrix, eliminated with partial
// pivoting in global memory, O(n^3) like the optimiser's dense path; the right-hand sides are the selected unit
// columns, and ALL 3n of them for the diagonal.  Only this path reports a singular system (outputs: NaN).
// Plain launches one after another on the caller's stream; a kernel that finds the refusal / singular flag set by an
// earlier one returns at once.  The pivoted systems (M, or the dense H) are factorised by one workgroup and solved
// one right-hand side per lane.  Every sum has a fixed order.
// ═════════════════════════════════════════════════════════════════════════════
constexpr int MG_THREADS = 256;                    // the grid-wide kernels
enum MgFlag { MG_REFUSED, MG_SINGULAR, MG_FLAGS };

// The device arrays of a marginals call: the plan's (PgPlanWs), then its own.  s selected nodes, diag: the diagonal is
// wanted.  Its X has other columns than the optimiser's, and no T on the dense path: xcols and tblocks, not the base's.
struct MgWs : PgPlanWs {
    using Base = PgPlanWs;
    int s, diag;
    int xcols = dense ? 0 : K + 3 * s + (diag ? K : 0);          // columns of X: Y = T^-1 W | V = T^-1 E_S | Z = T^-T W
    int NL = dense ? N3 : K;                                     // order of the pivoted system: H, or M
    int nrhs = 3 * s + (diag ? N3 : 0);                          // its right-hand sides: 3 per selected node, then (diagonal) 3 per node
    size_t tblocks = dense ? 0 : blocks;
    int32_t* sel = c.take<int32_t>((size_t)(s + 1) * 4);         // [s] the selected nodes
    int32_t* piv = c.take<int32_t>((size_t)(NL + 1) * 4);        // [NL] pivot rows of the elimination
    int32_t* flag = c.take<int32_t>(MG_FLAGS * 4);               // MgFlag
    double *D = c.take<double>(tblocks), *U = c.take<double>(tblocks), *L = c.take<double>(tblocks);   // T, as in PgWs
    double* Sl = c.take<double>(tblocks);                        // [n][9] the left Schur complements, inverted
    double* Td = c.take<double>(diag ? tblocks : 0);             // [n][9] the diagonal blocks of T^-1
    double* X = c.take<double>((size_t)N3 * xcols * 8);          // [3n][xcols] right-hand sides -> solutions
    double* AB = c.take<double>(18 * (size_t)(k + 1) * 8);       // [k][18] Jacobians of the closures
    double* A = c.take<double>(((size_t)NL * NL + 1) * 8);       // [NL][NL] M or H -> its LU factors
    double* R = c.take<double>(((size_t)NL * nrhs + 1) * 8);     // [NL][nrhs] right-hand sides -> solutions
    double* tw_omega = w ? c.take<double>((size_t)m * 9 * 8) : nullptr;      // as in PgWs
    double* tw_z = w ? c.take<double>((size_t)m * 3 * 8) : nullptr;
    size_t bytes = c.off + 256;
};

struct MgArgs : MgWs {
    const double* nodes;           // [n][3], read only
    const double* z;               // [m][3]    the caller's arrays, or tw_z / tw_omega
    const double* omega;           // [m][9]
    int fix;
    double* out_diagonal;          // [n][9] or null
    double* out_columns;           // [s][n][9] or null
    double* info;                  // [ICPMI_MARG_DOUBLES]
};

// assemble: what pg_assemble gathers per node, without the gradient; one thread per node over the grid.  The dense
// matrix g.A was zeroed before; a node writes its own three rows only.
__global__ __launch_bounds__(MG_THREADS) void marg_assemble_kernel(MgArgs g) {
    const int v = blockIdx.x * MG_THREADS + threadIdx.x, n = g.n, N3 = g.N3, f = g.fix;
    if (v >= n) return;
    M3 D = m3_zero(), U = m3_zero(), L = m3_zero();
    for (int t = g.csr_ptr[v]; t < g.csr_ptr[v + 1]; ++t) {
        const int q = g.csr_edge[t];
        const int i = g.ei[q], j = g.ej[q];
        double e[3];
        M3 A, B;
        pg_linearise(g.nodes + 3 * i, g.nodes + 3 * j, g.z + 3 * q, e, A, B);
        const M3 Om = m3_load(g.omega + 9 * (size_t)q);
        const M3 OA = m3_mul(Om, A), OB = m3_mul(Om, B);
        const bool in_T = g.dense || g.loop_slot[q] < 0;
        if (i == v && in_T) m3_add(D, m3_tmul(A, OA));
        if (j == v && in_T) m3_add(D, m3_tmul(B, OB));
        if (g.dense) {
            if (i == v && j != f && v != f) {
                const M3 c = m3_tmul(A, OB);
                for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.A[(size_t)(3 * v + r) * N3 + 3 * j + cc] += c.a[3 * r + cc];
            }
            if (j == v && i != f && v != f) {
                const M3 c = m3_tmul(B, OA);
                for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.A[(size_t)(3 * v + r) * N3 + 3 * i + cc] += c.a[3 * r + cc];
            }
        } else if (in_T && v == min(i, j) && i != j) {
            if (i == v) { m3_add(U, m3_tmul(A, OB)); m3_add(L, m3_tmul(B, OA)); }
            else { m3_add(U, m3_tmul(B, OA)); m3_add(L, m3_tmul(A, OB)); }
        }
    }
    if (v == f) { D = m3_zero(); D.a[0] = D.a[4] = D.a[8] = 1e10; U = m3_zero(); L = m3_zero(); }     // pose_graph.py:107-112
    if (v + 1 == f) { U = m3_zero(); L = m3_zero(); }
    if (g.dense) {
        if (v == f) { for (int r = 0; r < 3; ++r) g.A[(size_t)(3 * v + r) * N3 + 3 * v + r] = 1e10; }
        else for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) g.A[(size_t)(3 * v + r) * N3 + 3 * v + cc] += D.a[3 * r + cc];
    } else {
        m3_store(g.D + 9 * (size_t)v, D); m3_store(g.U + 9 * (size_t)v, U);       // U[v] = H[v][v+1], L[v] = H[v][v-1]
        if (v + 1 < n) m3_store(g.L + 9 * (size_t)(v + 1), L);
        if (v == 0) m3_store(g.L, m3_zero());
    }
}

// the Jacobians of the closures (no Omega here), one thread per closure
__global__ __launch_bounds__(MG_THREADS) void marg_closure_jacobians_kernel(MgArgs g) {
    const int q = blockIdx.x * MG_THREADS + threadIdx.x;
    if (q >= g.k) return;
    const int eq = g.loop_edge[q], i = g.ei[eq], j = g.ej[eq];
    double e[3];
    M3 A, B;
    pg_linearise(g.nodes + 3 * i, g.nodes + 3 * j, g.z + 3 * eq, e, A, B);
    m3_store(g.AB + 18 * (size_t)q, A); m3_store(g.AB + 18 * (size_t)q + 9, B);
}

// Right-hand sides of the chain solves, every element on its own (a gather: nothing is accumulated across threads):
// columns [0, K) and, for the diagonal, [K + 3s, K + 3s + K): W, whose column 3q + a holds row a of A_q at node i and
// of B_q at node j (both for a self-edge), nothing at the anchor; columns [K, K + 3s): the unit columns of the selection.
__global__ __launch_bounds__(MG_THREADS) void marg_chain_rhs_kernel(MgArgs g) {
    const size_t t = (size_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (t >= (size_t)g.N3 * g.xcols) return;
    const int row = (int)(t / g.xcols), col = (int)(t % g.xcols), v = row / 3, c = row % 3, K = g.K;
    double x = 0.0;
    if (col >= K && col < K + 3 * g.s) x = (g.sel[(col - K) / 3] == v && (col - K) % 3 == c) ? 1.0 : 0.0;
    else if (v != g.fix) {
        const int w = col < K ? col : col - K - 3 * g.s, q = w / 3, a = w % 3;
        const int eq = g.loop_edge[q];
        if (g.ei[eq] == v) x += g.AB[18 * (size_t)q + 3 * a + c];
        if (g.ej[eq] == v) x += g.AB[18 * (size_t)q + 9 + 3 * a + c];
    }
    g.X[t] = x;
}

// The factorisation of T, serial along the chain (one thread): the left Schur complements from node 0 up, kept
// inverted; an exactly singular one refuses the split.  Then, for the diagonal, the blocks (T^-1)[v][v] from the last
// node down.
__global__ void marg_chain_factor_kernel(MgArgs g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n = g.n;
    M3 S = m3_load(g.D), inv;
    for (int v = 0; v < n; ++v) {
        if (!m3_inv(S, inv)) { g.flag[MG_REFUSED] = 1; return; }
        m3_store(g.Sl + 9 * (size_t)v, inv);
        if (v + 1 < n) {
            S = m3_load(g.D + 9 * (size_t)(v + 1));
            m3_sub(S, m3_mul(m3_mul(m3_load(g.L + 9 * (size_t)(v + 1)), inv), m3_load(g.U + 9 * (size_t)v)));
        }
    }
    if (!g.diag) return;
    M3 G = inv;                                                  // Sl[n-1]^-1
    m3_store(g.Td + 9 * (size_t)(n - 1), G);
    for (int v = n - 2; v >= 0; --v) {
        const M3 Si = m3_load(g.Sl + 9 * (size_t)v);
        const M3 left = m3_mul(Si, m3_load(g.U + 9 * (size_t)v)), right = m3_mul(m3_load(g.L + 9 * (size_t)(v + 1)), Si);
        G = m3_mul(m3_mul(left, G), right);
        m3_add(G, Si);
        m3_store(g.Td + 9 * (size_t)v, G);
    }
}

// T^-1 (columns below K + 3s) or T^-T (the others) on the columns of X: one column per lane, serial along the chain.
__global__ __launch_bounds__(ICPMI_WAVE) void marg_chain_solve_kernel(MgArgs g) {
    const int col = blockIdx.x * ICPMI_WAVE + threadIdx.x, n = g.n, ncols = g.xcols;
    if (col >= ncols || g.flag[MG_REFUSED]) return;
    const bool tr = col >= g.K + 3 * g.s;
    double y[3] = {0.0, 0.0, 0.0}, t1[3], t2[3];
    for (int v = 0; v < n; ++v) {                                // forward: y[v] = r[v] - L[v] Sl[v-1]^-1 y[v-1]
        double r[3];
        for (int c = 0; c < 3; ++c) r[c] = g.X[(size_t)(3 * v + c) * ncols + col];
        if (v > 0) {
            if (tr) { m3_tvec(m3_load(g.Sl + 9 * (size_t)(v - 1)), y, t1); m3_tvec(m3_load(g.U + 9 * (size_t)(v - 1)), t1, t2); }
            else { m3_vec(m3_load(g.Sl + 9 * (size_t)(v - 1)), y, t1); m3_vec(m3_load(g.L + 9 * (size_t)v), t1, t2); }
            for (int c = 0; c < 3; ++c) r[c] -= t2[c];
        }
        for (int c = 0; c < 3; ++c) { y[c] = r[c]; g.X[(size_t)(3 * v + c) * ncols + col] = r[c]; }
    }
    double x[3] = {0.0, 0.0, 0.0};
    for (int v = n - 1; v >= 0; --v) {                           // back: x[v] = Sl[v]^-1 (y[v] - U[v] x[v+1])
        double r[3];
        for (int c = 0; c < 3; ++c) r[c] = g.X[(size_t)(3 * v + c) * ncols + col];
        if (v + 1 < n) {
            if (tr) m3_tvec(m3_load(g.L + 9 * (size_t)(v + 1)), x, t1);
            else m3_vec(m3_load(g.U + 9 * (size_t)v), x, t1);
            for (int c = 0; c < 3; ++c) r[c] -= t1[c];
        }
        if (tr) m3_tvec(m3_load(g.Sl + 9 * (size_t)v), r, x);
        else m3_vec(m3_load(g.Sl + 9 * (size_t)v), r, x);
        for (int c = 0; c < 3; ++c) g.X[(size_t)(3 * v + c) * ncols + col] = x[c];
    }
}

// The closure system, one element per thread: M = I + C W^T Y into A, then the right-hand sides into R: C W^T V (the
// selection, three per selected node) and C Z_v^T (the diagonal, three per node).  The gathers are pg_closure_system's.
__global__ __launch_bounds__(MG_THREADS) void marg_closure_system_kernel(MgArgs g) {
    const int K = g.K, s3 = 3 * g.s, width = K + g.nrhs, f = g.fix;
    const size_t t = (size_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (t >= (size_t)K * width || g.flag[MG_REFUSED]) return;
    const int r = (int)(t / width), c = (int)(t % width), q = r / 3, a = r % 3;
    const int eq = g.loop_edge[q];
    const double* Om = g.omega + 9 * (size_t)eq;
    if (c >= K + s3) {                                           // row r of C Z_v^T, column c - K - s3 = 3v + component
        const double* Zr = g.X + (size_t)(c - K - s3) * g.xcols + K + s3 + 3 * q;
        g.R[(size_t)r * g.nrhs + (c - K)] = (Om[3 * a] * Zr[0] + Om[3 * a + 1] * Zr[1]) + Om[3 * a + 2] * Zr[2];
        return;
    }
    const int i = g.ei[eq], j = g.ej[eq];                       // column c of X: Y below K, V from there
    const double* AB = g.AB + 18 * (size_t)q;
    double acc = 0.0;
    for (int bb = 0; bb < 3; ++bb) {
        double sum = 0.0;
        for (int cc = 0; cc < 3; ++cc) {
            if (i != f) sum += AB[3 * bb + cc] * g.X[(size_t)(3 * i + cc) * g.xcols + c];
            if (j != f) sum += AB[9 + 3 * bb + cc] * g.X[(size_t)(3 * j + cc) * g.xcols + c];
        }
        acc += Om[3 * a + bb] * sum;
    }
    if (c < K) g.A[(size_t)r * K + c] = acc + (r == c ? 1.0 : 0.0);
    else g.R[(size_t)r * g.nrhs + (c - K)] = acc;
}

// unit right-hand sides of the dense system: 3 per selected node, then (diagonal) the whole identity
__global__ __launch_bounds__(MG_THREADS) void marg_dense_rhs_kernel(MgArgs g) {
    const size_t t = (size_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (t >= (size_t)g.N3 * g.nrhs) return;
    const int row = (int)(t / g.nrhs), c = (int)(t % g.nrhs), s3 = 3 * g.s;
    const int target = c < s3 ? 3 * g.sel[c / 3] + c % 3 : c - s3;
    g.R[t] = row == target ? 1.0 : 0.0;
}

// P A = L U in place (a: N x N row-major in global memory) with partial pivoting, one workgroup: the multipliers stay
// below the diagonal, whole rows are exchanged, piv[p] is the row exchanged with row p.  An exactly zero pivot column
// raises flag[on_zero] (refused for the closure system, LAPACK's singular matrix for the dense one) and ends it.
__global__ __launch_bounds__(PG_THREADS) void marg_lu_factor_kernel(double* a, int N, int32_t* piv, int32_t* flag, int on_zero) {
    __shared__ double s_val;
    __shared__ int s_idx;
    if (flag[MG_REFUSED]) return;
    const int tid = threadIdx.x;
    const int tx = tid & 31, ty = tid >> 5;                       // update tile: 32 columns x (PG_THREADS / 32) rows
    for (int p = 0; p < N; ++p) {
        if (wave_id() == 0) {                                     // pivot search as in block_lu_solve: the lowest row among equal |a|
            double best = -1.0; int bi = 0x7fffffff;
            for (int r = p + lane_id(); r < N; r += ICPMI_WAVE) {
                const double v = fabs(a[(size_t)r * N + p]);
                if (v > best) { best = v; bi = r; }
            }
            wave_first_best(best, bi, [](double x, double y) { return x > y; });
            if (lane_id() == 0) { s_val = best; s_idx = bi; }
        }
        __syncthreads();
        const double pv = s_val;
        const int pr = s_idx;
        if (!(pv > 0.0)) { if (tid == 0) flag[on_zero] = 1; return; }        // uniform
        if (tid == 0) piv[p] = pr;
        if (pr != p)
            for (int c = tid; c < N; c += PG_THREADS) {
                const double t = a[(size_t)p * N + c];
                a[(size_t)p * N + c] = a[(size_t)pr * N + c];
                a[(size_t)pr * N + c] = t;
            }
        __syncthreads();
        const double pivot = a[(size_t)p * N + p];
        for (int r = p + 1 + tid; r < N; r += PG_THREADS) a[(size_t)r * N + p] = a[(size_t)r * N + p] / pivot;
        __syncthreads();
        for (int r = p + 1 + ty; r < N; r += PG_THREADS / 32) {
            const double l = a[(size_t)r * N + p];
            for (int c = p + 1 + tx; c < N; c += 32) a[(size_t)r * N + c] -= l * a[(size_t)p * N + c];
        }
        __syncthreads();
    }
}

// the factors on the columns of R ([N][nrhs] row-major), one column per lane over the grid: row exchanges, L, U
__global__ __launch_bounds__(ICPMI_WAVE) void marg_lu_solve_kernel(const double* a, int N, const int32_t* piv, double* R, int nrhs,
                                                                   const int32_t* flag) {
    const int col = blockIdx.x * ICPMI_WAVE + threadIdx.x;
    if (col >= nrhs || flag[MG_REFUSED] || flag[MG_SINGULAR]) return;
    for (int p = 0; p < N; ++p) {
        const int pr = piv[p];
        if (pr != p) { const double t = R[(size_t)p * nrhs + col]; R[(size_t)p * nrhs + col] = R[(size_t)pr * nrhs + col]; R[(size_t)pr * nrhs + col] = t; }
    }
    for (int r = 1; r < N; ++r) {
        double acc = R[(size_t)r * nrhs + col];
        for (int q = 0; q < r; ++q) acc -= a[(size_t)r * N + q] * R[(size_t)q * nrhs + col];
        R[(size_t)r * nrhs + col] = acc;
    }
    for (int r = N - 1; r >= 0; --r) {
        double acc = R[(size_t)r * nrhs + col];
        for (int q = r + 1; q < N; ++q) acc -= a[(size_t)r * N + q] * R[(size_t)q * nrhs + col];
        R[(size_t)r * nrhs + col] = acc / a[(size_t)r * N + r];
    }
}

// both outputs of the split path, one entry per thread, the K products summed in column order:
// block (v, S[a]) = V - Y_v y_a, then block (v, v) = G[v] - Y_v y_v
__global__ __launch_bounds__(MG_THREADS) void marg_split_out_kernel(MgArgs g) {
    const size_t t = (size_t)blockIdx.x * MG_THREADS + threadIdx.x, nc = g.out_columns ? (size_t)g.s * g.n * 9 : 0;
    if (t >= nc + (g.out_diagonal ? (size_t)g.n * 9 : 0) || g.flag[MG_REFUSED]) return;
    const size_t d = t < nc ? t : t - nc;
    const int e = (int)(d % 9), v = (int)(d / 9 % g.n), K = g.K;
    const int rhs = t < nc ? 3 * (int)(d / 9 / g.n) + e % 3 : 3 * g.s + 3 * v + e % 3;     // column of R
    const double* Xr = g.X + (size_t)(3 * v + e / 3) * g.xcols;
    double acc = 0.0;
    for (int q = 0; q < K; ++q) acc += Xr[q] * g.R[(size_t)q * g.nrhs + rhs];
    if (t < nc) g.out_columns[t] = Xr[K + rhs] - acc;
    else g.out_diagonal[d] = g.Td[d] - acc;
}

// both outputs of the dense path, out of the solved unit columns; NaN after a singular elimination
__global__ __launch_bounds__(MG_THREADS) void marg_dense_out_kernel(MgArgs g) {
    const size_t t = (size_t)blockIdx.x * MG_THREADS + threadIdx.x, nc = g.out_columns ? (size_t)g.s * g.n * 9 : 0;
    if (t >= nc + (g.out_diagonal ? (size_t)g.n * 9 : 0)) return;
    const bool singular = g.flag[MG_SINGULAR] != 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int s3 = 3 * g.s;
    if (t < nc) {
        const int e = (int)(t % 9), v = (int)(t / 9 % g.n), a = (int)(t / 9 / g.n);
        g.out_columns[t] = singular ? nan : g.R[(size_t)(3 * v + e / 3) * g.nrhs + 3 * a + e % 3];
    } else {
        const size_t d = t - nc;
        const int e = (int)(d % 9), v = (int)(d / 9);
        g.out_diagonal[d] = singular ? nan : g.R[(size_t)(3 * v + e / 3) * g.nrhs + s3 + 3 * v + e % 3];
    }
}

__global__ void marg_info_kernel(MgArgs g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    g.info[ICPMI_MARG_STATUS] = (double)(g.flag[MG_SINGULAR] ? ICPMI_PG_ST_SINGULAR : g.flag[MG_REFUSED] ? ICPMI_PG_ST_REFUSED : ICPMI_PG_ST_CONVERGED);
    g.info[ICPMI_MARG_PATH] = (double)(g.dense ? ICPMI_MARG_PATH_DENSE : ICPMI_MARG_PATH_SPLIT);
    g.info[ICPMI_MARG_CLOSURES] = (double)g.k;
    g.info[ICPMI_MARG_TWINS] = (double)g.w;
}

// the kernels index [n][9] and [s][9] in int
static bool mg_indexable(int32_t n_nodes, int32_t n_selected) { return (size_t)n_nodes <= 0x7fffffffu / 9 && (size_t)n_selected <= 0x7fffffffu / 9; }
static size_t mg_workspace_bytes(const int32_t* edges_ij_host, const double* omega_host, int32_t n_nodes, int32_t n_edges,
                                 int32_t n_selected, bool diag, bool force_dense) {
    if (n_selected < 0 || !mg_indexable(n_nodes, n_selected)) return 0;
    return pg_layout_bytes<MgWs>(edges_ij_host, omega_host, n_nodes, n_edges, force_dense, (int)n_selected, (int)diag);
}

static inline unsigned mg_grid(size_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

static int mg_marginals(const double* nodes, const int32_t* edges_ij_host, const double* edges_z, const double* edges_omega,
                        int32_t n_nodes, int32_t n_edges, int32_t fix_node, const int32_t* selected_host, int32_t n_selected,
                        double* out_diagonal, double* out_columns, bool force_dense, double* info, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if ((!out_diagonal && !out_columns) || n_selected < 0 || (n_selected > 0 && !selected_host)) return ICPMI_ERR_ARG;
    const int n = n_nodes, s = out_columns ? n_selected : 0, diag = out_diagonal != nullptr;
    if (n >= 2 && n_edges > 0) {                                 // not where there is nothing to do: that is no error
        for (int a = 0; a < n_selected; ++a) if (selected_host[a] < 0 || selected_host[a] >= n) return ICPMI_ERR_ARG;
        if (!mg_indexable(n, s)) return ICPMI_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const PgCall c{nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, 0, fix_node, force_dense, true,
                   info, ICPMI_MARG_DOUBLES, ICPMI_MARG_STATUS, ICPMI_MARG_PATH, workspace, workspace_bytes, st};
    const std::vector<int32_t> sel(selected_host, selected_host + s);
    const PgStaged<MgWs> staged = pg_stage<MgWs>(c, [&](const MgWs& w, hipStream_t st) {
        return pg_upload(w.sel, sel, st) && hipMemsetAsync(w.flag, 0, MG_FLAGS * 4, st) == hipSuccess &&
               (!w.dense || hipMemsetAsync(w.A, 0, (size_t)w.NL * w.NL * 8, st) == hipSuccess);
    }, s, diag);
    if (!staged.w) return staged.rc;
    const MgWs& w = *staged.w;
    const MgArgs a{w, nodes, staged.z, staged.omega, fix_node, out_diagonal, out_columns, info};
    const size_t outs = (size_t)s * n * 9;
    marg_assemble_kernel<<<mg_grid(n, MG_THREADS), MG_THREADS, 0, st>>>(a);
    if (w.dense) {
        if (w.nrhs > 0) {
            marg_dense_rhs_kernel<<<mg_grid((size_t)w.N3 * w.nrhs, MG_THREADS), MG_THREADS, 0, st>>>(a);
            marg_lu_factor_kernel<<<1, PG_THREADS, 0, st>>>(w.A, w.NL, w.piv, w.flag, MG_SINGULAR);
            marg_lu_solve_kernel<<<mg_grid(w.nrhs, ICPMI_WAVE), ICPMI_WAVE, 0, st>>>(w.A, w.NL, w.piv, w.R, w.nrhs, w.flag);
            marg_dense_out_kernel<<<mg_grid(outs + (diag ? (size_t)n * 9 : 0), MG_THREADS), MG_THREADS, 0, st>>>(a);
        }
    } else {
        if (w.k > 0) marg_closure_jacobians_kernel<<<mg_grid(w.k, MG_THREADS), MG_THREADS, 0, st>>>(a);
        if (w.xcols > 0) marg_chain_rhs_kernel<<<mg_grid((size_t)w.N3 * w.xcols, MG_THREADS), MG_THREADS, 0, st>>>(a);
        marg_chain_factor_kernel<<<1, ICPMI_WAVE, 0, st>>>(a);
        if (w.xcols > 0) marg_chain_solve_kernel<<<mg_grid(w.xcols, ICPMI_WAVE), ICPMI_WAVE, 0, st>>>(a);
        if (w.k > 0) {
            marg_closure_system_kernel<<<mg_grid((size_t)w.K * (w.K + w.nrhs), MG_THREADS), MG_THREADS, 0, st>>>(a);
            marg_lu_factor_kernel<<<1, PG_THREADS, 0, st>>>(w.A, w.NL, w.piv, w.flag, MG_REFUSED);
            if (w.nrhs > 0) marg_lu_solve_kernel<<<mg_grid(w.nrhs, ICPMI_WAVE), ICPMI_WAVE, 0, st>>>(w.A, w.NL, w.piv, w.R, w.nrhs, w.flag);
        }
        marg_split_out_kernel<<<mg_grid(outs + (diag ? (size_t)n * 9 : 0), MG_THREADS), MG_THREADS, 0, st>>>(a);
    }
    marg_info_kernel<<<1, ICPMI_WAVE, 0, st>>>(a);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}

}  // namespace icpmi

extern "C" size_t icpmi_pose_graph_marginals_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                                             int32_t n_nodes, int32_t n_edges, int32_t n_selected,
                                                             int32_t want_diagonal, int32_t force_dense) {
    return icpmi::mg_workspace_bytes(edges_ij_host, edges_omega_host, n_nodes, n_edges, n_selected, want_diagonal != 0, force_dense != 0);
}
extern "C" int icpmi_pose_graph_marginals(const double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                          const double* edges_omega, int32_t n_nodes, int32_t n_edges, int32_t fix_node,
                                          const int32_t* selected_host, int32_t n_selected, double* out_diagonal,
                                          double* out_columns, int32_t force_dense, double* info, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return icpmi::mg_marginals(nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, fix_node, selected_host, n_selected,
                               out_diagonal, out_columns, force_dense != 0, info, workspace, workspace_bytes, stream);
}

extern "C" size_t icpmi_pose_graph_workspace_bytes(const int32_t* edges_ij_host, int32_t n_nodes, int32_t n_edges) {
    return icpmi::pg_layout_bytes<icpmi::PgWs>(edges_ij_host, nullptr, n_nodes, n_edges, false);
}
extern "C" size_t icpmi_pose_graph_weighted_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                                            int32_t n_nodes, int32_t n_edges) {
    return icpmi::pg_layout_bytes<icpmi::PgWs>(edges_ij_host, edges_omega_host, n_nodes, n_edges, false);
}
extern "C" size_t icpmi_pose_graph_dense_workspace_bytes(const int32_t* edges_ij_host, int32_t n_nodes, int32_t n_edges) {
    return icpmi::pg_layout_bytes<icpmi::PgWs>(edges_ij_host, nullptr, n_nodes, n_edges, true);
}

extern "C" int icpmi_pose_graph_optimize(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                         const double* edges_omega, int32_t n_nodes, int32_t n_edges,
                                         int32_t n_iterations, int32_t fix_node, double convergence_eps,
                                         double* info, void* workspace, size_t workspace_bytes, void* stream) {
    return icpmi::pg_optimize(nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, n_iterations, fix_node,
                              convergence_eps, info, workspace, workspace_bytes, stream, false);
}
extern "C" int icpmi_pose_graph_optimize_dense(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                               const double* edges_omega, int32_t n_nodes, int32_t n_edges,
                                               int32_t n_iterations, int32_t fix_node, double convergence_eps,
                                               double* info, void* workspace, size_t workspace_bytes, void* stream) {
    return icpmi::pg_optimize(nodes, edges_ij_host, edges_z, edges_omega, n_nodes, n_edges, n_iterations, fix_node,
                              convergence_eps, info, workspace, workspace_bytes, stream, true);
}

extern "C" size_t icpmi_pose_graph_robust_workspace_bytes(const int32_t* edges_ij_host, const double* edges_omega_host,
                                                          const uint8_t* edges_mask_host, int32_t n_nodes, int32_t n_edges,
                                                          int32_t dense) {
    return icpmi::pg_robust_workspace_bytes(edges_ij_host, edges_omega_host, edges_mask_host, n_nodes, n_edges, dense != 0);
}
extern "C" int icpmi_pose_graph_optimize_robust(double* nodes, const int32_t* edges_ij_host, const double* edges_z,
                                                const double* edges_omega, const uint8_t* edges_mask_host, int32_t n_nodes,
                                                int32_t n_edges, int32_t n_iterations, int32_t fix_node, double convergence_eps,
                                                int32_t kernel, double delta, int32_t dense, double* edge_chi2,
                                                double* edge_weight, double* info, void* workspace, size_t workspace_bytes,
                                                void* stream) {
    return icpmi::pg_optimize_robust(nodes, edges_ij_host, edges_z, edges_omega, edges_mask_host, n_nodes, n_edges, n_iterations,
                                     fix_node, convergence_eps, kernel, delta, dense != 0, edge_chi2, edge_weight, info, workspace,
                                     workspace_bytes, stream);
}

extern "C" int icpmi_pose_graph_error(const double* nodes, const int32_t* edges_i, const int32_t* edges_j, const double* edges_z,
                                      const double* edges_omega, int32_t n_edges, double* scratch, double* out, void* stream) {
    if (!out || n_edges < 0) return ICPMI_ERR_ARG;
    if (n_edges > 0 && (!nodes || !edges_i || !edges_j || !edges_z || !edges_omega || !scratch)) return ICPMI_ERR_ARG;
    icpmi::pose_graph_error_kernel<<<1, icpmi::PG_THREADS, 0, (hipStream_t)stream>>>(nodes, edges_i, edges_j, edges_z, edges_omega,
                                                                                  n_edges, scratch, out);
    ICPMI_LAUNCH_CHECK();
    return ICPMI_OK;
}
