// features.hpp — the per-cloud half of the feature alignment (features.hip), for the callers that keep its results:
// icpmi_feature_align_batch runs it on its own workspace at every call, the resident scan history (history.hip) once per
// scan, into a feature store.
#pragma once
#include "common.hpp"

namespace icpmi {

// The tables of a set of clouds: the voxel-filtered rows (cloud set layout, on the raw set's offsets) and what the per-cloud
// stages leave per row (curv) and per cloud (everything else).  Per-cloud tables are indexed by the cloud's number.
struct FtTables {
    double* pts;
    const int32_t* off;
    int32_t* cnt;
    double* curv;
    int32_t* kp;              // [clouds][kp_stride]
    int32_t* kp_cnt;
    double* desc;             // [clouds][kp_stride][ICPMI_FT_DESC_STRIDE]
    int32_t* desc_len;
    int32_t kp_stride;
};

// What the per-cloud stages are computed with.
struct FtCloudCfg {
    double voxel_size;
    int32_t k_curvature, top_n;
    double min_kp_dist;
    int32_t k_descriptor;
};

// The tables and the configuration of a history's feature store (ft_store_check has passed).
inline FtTables ft_store_tables(const icpmi_history* h, const icpmi_feature_store* s) {
    return FtTables{s->vox, h->off_dev, s->cnt, s->curv, s->kp, s->kp_cnt, s->desc, s->desc_len, s->kp_stride};
}
inline FtCloudCfg ft_store_cfg(const icpmi_feature_store* s) {
    return FtCloudCfg{s->voxel_size, s->k_curvature, s->top_n, s->min_kp_dist, s->k_descriptor};
}

// ICPMI_OK, ICPMI_ERR_ARG (a table missing, a voxel size that is not > 0, a negative k, kp_stride <= 0) or
// ICPMI_ERR_UNSUPPORTED (k or top_n above what the kernels hold, top_n > kp_stride) — in this order.
int ft_store_check(const icpmi_feature_store* s);

// The per-cloud half: voxel filter of the raw clouds [first, first + n) at cfg.voxel_size into t.pts / t.cnt (the filter
// runs on the tail of the offsets and writes a cloud where it was), then curvature, keypoints by the device order rule and
// descriptors of the clouds cloud_ids[0 .. n) — the same clouds by number; nullptr, with first == 0: clouds 0 .. n.  Every
// other cloud's tables stay as they are.  raw: the rows t.off and off_host (its host mirror) address.  n > 0, cfg checked.
int ft_cloud_stages(const FtTables& t, const double* raw, const int32_t* off_host, int first, int n, const int32_t* cloud_ids,
                    const FtCloudCfg& cfg, void* vws, size_t vws_bytes, hipStream_t st);

}  // namespace icpmi
