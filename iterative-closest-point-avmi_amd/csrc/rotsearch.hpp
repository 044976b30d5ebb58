// rotsearch.hpp — the two halves of the batched rotation search (rotsearch.hip), for the callers that keep its state:
// icpmi_rotation_search_batch runs both on its own workspace, the resident scan history (history.hip) the first when a
// scan is added and the second at every query.
#pragma once
#include "common.hpp"

namespace icpmi {

// What the search kernel reads of a cloud set: the voxel-filtered clouds (cloud set layout), their counts and means, the
// prepared targets.  layout_rows: the row count the prepared buffer is laid out for (PreparedView, prep_common.hpp).
struct RsbState {
    const double* vox;
    const int32_t* off;
    const int32_t* cnt;
    const double* means;
    const void* prepared;
    int32_t layout_rows;
};

// First half, for the clouds [first, first + n) of a set: voxel filter at `voxel` into vox / cnt, then np.mean(axis=0) of each
// filtered cloud into means.  Every other cloud's rows, count and mean stay as they are.
int rsb_filter_means(const double* pts, const int32_t* off_dev, const int32_t* off_host, int first, int n, double voxel,
                     double* vox, int32_t* cnt, double* means, void* vws, size_t vws_bytes, hipStream_t st);

// May the targets of the search be put in bearing order (option RS_BATCH)?
int rsb_allow_polar();

// Second half: one workgroup per pair on the state.  max_n: rows of the largest RAW cloud of any pair (it sizes the on-chip
// copies as the largest cloud of icpmi_rotation_search_batch's set does).
int rsb_search(const RsbState& s, int max_n, int max_rows_hint, const int32_t* pair_src, const int32_t* pair_tgt, int n_pairs,
               const double* coarse_cs, int n_coarse, const double* fine_cs, const int32_t* fine_cnt, int max_fine,
               double* out_records, double* out_init, hipStream_t st);

}  // namespace icpmi
