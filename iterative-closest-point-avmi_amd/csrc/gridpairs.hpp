// gridpairs.hpp — the host plan the kernels share that hold a list of (cloud, pose) pairs against the occupancy planes, one
// workgroup per (pair, chunk of rows) with a status kernel behind it (gridcheck.hip: the check; gridbeam.hip: the beam
// model): what the pair list and the grid allow, decided as a whole and without a HIP call.  It exists once, so the two
// entries refuse the same calls.
#pragma once
#include "gridcast.hpp"

namespace icpmi {

struct PairPlan {
    int rc;                   // ICPMI_OK, or why nothing is launched
    GcPlan grid;              // the planes of the grid: what is packed when the call packs, and their size
    unsigned row_grid;        // (pair, chunk) workgroups; 0: no named cloud has a row (the records are still written)
    unsigned status_grid;     // the status kernel: a lane per pair
    int n_chunks, max_n;      // row chunks of, and rows of, the largest named cloud
};
// The chunk never depends on the batch: a pair's record does not depend on the batch it is computed in.
inline PairPlan plan_pairs(int ny, int nx, int n_pairs, int n_clouds, const int32_t* off_host, const int32_t* pair_cloud_host, int chunk,
                           int threads) {
    PairPlan p{ICPMI_OK, plan_cast(ny, nx, 0, 0), 0, 0, 0, 0};
    if (n_pairs < 0 || n_clouds < 0 || !off_host || !pair_cloud_host) { p.rc = ICPMI_ERR_ARG; return p; }
    long long total = 0;
    bool above = false;
    for (int b = 0; b < n_pairs; ++b) {
        const int c = pair_cloud_host[b];
        if (c < 0 || c >= n_clouds) { p.rc = ICPMI_ERR_ARG; return p; }
        const int rows = off_host[c + 1] - off_host[c];
        if (rows < 0) { p.rc = ICPMI_ERR_ARG; return p; }
        above |= rows > ICPMI_GM_MAX_ROWS;
        p.max_n = rows > p.max_n ? rows : p.max_n;
        total += rows;
    }
    if (p.grid.rc != ICPMI_OK) { p.rc = p.grid.rc; return p; }
    p.n_chunks = (p.max_n + chunk - 1) / chunk;
    const unsigned long long groups = (unsigned long long)n_pairs * p.n_chunks;
    if (above || total >= (1ll << 29) || groups >= (1ull << 31)) { p.rc = ICPMI_ERR_UNSUPPORTED; return p; }
    p.row_grid = (unsigned)groups;
    p.status_grid = (unsigned)(((long long)n_pairs + threads - 1) / threads);
    return p;
}

}  // namespace icpmi
