"""utilities.features — the two pre-alignment methods of the reference
(utilities/features.py) with the same signatures, computed on the MI355X.

``rotation_search`` (features.py:165-242, the default, config.yaml:34): about half
of every non-IMU scan pair of the reference goes into its ~270 nearest-neighbour
sweeps.  Here the whole search is one chain of launches (voxel filters, means,
coarse sweep, arg-min, fine sweep, arg-min) behind ``icpmi_rotation_search``; the
angle grids and their cos/sin are computed with the reference's own NumPy
expressions (cached on the device), so the chosen angle, R and t are the
reference's numbers bit for bit.

``feature_based_alignment`` (features.py:247-315) and its five public stages
(``compute_curvature``, ``extract_keypoints``, ``compute_descriptors``,
``match_descriptors``, ``ransac_align``): each stage is a kernel of
csrc/features.hip.  What stays on the host is what decides the reference's result
through NumPy's own state: ``np.argsort(-curvatures)`` (unstable, and the order
of tied curvatures decides the keypoints) and the ``np.random.choice`` draws of
RANSAC, made in the reference's order so that a seeded run tests the reference's
hypotheses and leaves the global stream where the reference leaves it.
``icpmi.prealign.FeatureAlignBatch`` is the whole pipeline for a batch of pairs
with no host round trip.
"""
import numpy as np
import torch

from icpmi import _lib
from icpmi import batch as _b
from icpmi.prealign import (AngleTables, FeatureAlignBatch, arange_rows, device_angle_tables,  # noqa: F401
                            rotation_search_batch, run_icp_pair_batch, winning_angle)

VERBOSE = True      # the reference prints one line per search


def rotation_scores(src_rows, target, angles, shift):
    """Mean squared NN distance of ``src_rows @ R(a).T + shift`` in ``target`` for every angle (radians).

    The scoring function of features.py:213-218 and slam.py:138-143, all angles in one launch."""
    _b.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())

    def on_device(x):        # NumPy rows are uploaded; float64 device tensors (a resident submap) are used in place
        if isinstance(x, torch.Tensor):
            return x.to(dev, torch.float64).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)

    d_s, d_t = on_device(src_rows), on_device(target)
    a = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    if d_s.dim() != 2 or d_s.shape[1] != 2 or d_t.dim() != 2 or d_t.shape[1] != 2 or len(d_s) == 0 or len(d_t) == 0:
        raise ValueError("rotation_scores needs non-empty (n, 2) arrays")
    if len(a) == 0:
        return np.empty(0)
    cs = np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))       # features.py:214
    d_cs = torch.from_numpy(cs).to(dev)
    out = torch.empty(len(a), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().icpmi_rotation_scores(_b._ptr(d_s), len(d_s), _b._ptr(d_t), len(d_t), _b._ptr(d_cs), len(a),
                                                float(shift[0]), float(shift[1]), _b._ptr(out), _b._stream()),
               "rotation_search")
    return out.cpu().numpy()


class _SearchContext:
    """Device buffers and angle tables of the rotation searches, kept between calls (one per device): the scans of a
    SLAM loop have the same size every time, and allocating, uploading offsets and reading sizes back per call cost
    several times the kernels themselves."""
    _per_device = {}

    @classmethod
    def get(cls):
        _b.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in cls._per_device:
            cls._per_device[dev] = cls(dev)
        return cls._per_device[dev]

    def __init__(self, dev):
        self.dev = dev
        self.cap = 0
        self.tables = {}
        self.rec = torch.zeros(_lib.RSREC_DOUBLES, dtype=torch.float64, device=dev)
        self.rec_host = torch.zeros(_lib.RSREC_DOUBLES, dtype=torch.float64).pin_memory()
        self.ws = None

    def upload(self, src, tgt):
        """source rows then target rows in one pinned staging buffer -> one asynchronous copy."""
        n = len(src) + len(tgt)
        if n > self.cap:
            self.cap = max(2 * n, 8192)
            self.stage = torch.empty((self.cap, 2), dtype=torch.float64).pin_memory()
            self.pts = torch.empty((self.cap, 2), dtype=torch.float64, device=self.dev)
        h = self.stage.numpy()
        h[:len(src)] = src
        h[len(src):n] = tgt
        self.pts[:n].copy_(self.stage[:n], non_blocking=True)
        return self.pts

    def workspace(self, n_src, n_tgt, n_coarse, max_fine):
        need = _lib.lib().icpmi_rotation_search_workspace_bytes(n_src, n_tgt, n_coarse, max_fine)
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(2 * need, dtype=torch.uint8, device=self.dev)
        return self.ws

    def device_table(self, coarse, fine, fine_n):
        return device_angle_tables(self.dev, coarse, fine, fine_n)

    def run(self, src, tgt, voxel_size, coarse, fine, fine_n, dtab, centred, shift):
        """-> the record on the host (one synchronisation; slots _lib.RSREC_*, include/icpmi.h icpmi_rotation_search)."""
        d_cs, d_fcs, d_fn = dtab
        pts = self.upload(src, tgt)
        max_fine = int(fine.shape[1]) if fine.ndim == 2 else 0
        ws = self.workspace(len(src), len(tgt), len(coarse), max_fine)
        _lib.check(_lib.lib().icpmi_rotation_search(_b._ptr(pts), len(src), len(tgt), float(voxel_size), _b._ptr(d_cs), len(coarse),
                                                    _b._ptr(d_fcs) if max_fine else None, _b._ptr(d_fn) if max_fine else None,
                                                    max_fine, 1 if centred else 0, float(shift[0]), float(shift[1]),
                                                    _b._ptr(self.rec), _b._ptr(ws), ws.numel(), _b._stream()), "rotation_search")
        self.rec_host.copy_(self.rec, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.rec_host.numpy().copy()

    def filtered_clouds(self, n_src, n_tgt, rec):
        """Views of the voxel-filtered source and target the last run left in the workspace (device, no copy)."""
        v = self.ws[_lib.RS_WS_CLOUDS:_lib.RS_WS_CLOUDS + (n_src + n_tgt) * 16].view(torch.float64).reshape(-1, 2)
        return v[:int(rec[_lib.RSREC_NS])], v[n_src:n_src + int(rec[_lib.RSREC_NT])]


def _as_rows(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{name} must have shape (n, 2), got {a.shape}")
    if a.shape[0] == 0:
        # the reference fails inside np.min of voxel_downsample on an empty array (icp.py:119)
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    return a


def rotation_search(source, target, voxel_size=0.3, angle_step_coarse=2.0, angle_step_fine=0.2):
    """Brute-force rotation search — features.py:165-242.  Returns (R (2,2), t (2,), score).

    One chain of launches on the device (voxel filters, means, coarse sweep, arg-min, fine sweep, arg-min) and one
    read-back of the record; the angle grids, their cos / sin and the final R, t are the reference's NumPy expressions."""
    src, tgt = _as_rows(source, "source"), _as_rows(target, "target")
    ctx = _SearchContext.get()
    tab = AngleTables.get(ctx.dev, angle_step_coarse, angle_step_fine)            # features.py:221, 227-229 for every possible winner
    angles_coarse, fine, fine_n, dtab = tab.coarse, tab.fine, tab.fine_n, tab.device_table
    rec = ctx.run(src, tgt, voxel_size, angles_coarse, fine, fine_n, dtab, True, (0.0, 0.0))
    if rec[_lib.RSREC_NS] < 5 or rec[_lib.RSREC_NT] < 5:                       # features.py:203-204
        return np.eye(2), np.zeros(2), float("inf")
    best_angle = winning_angle(angles_coarse, fine, rec)                       # (raises as np.argmin on an empty fine grid)
    best_score = np.float64(rec[_lib.RSREC_FSCORE])
    mu_s, mu_t = rec[_lib.RSREC_MUS:_lib.RSREC_MUS + 2].copy(), rec[_lib.RSREC_MUT:_lib.RSREC_MUT + 2].copy()
    ca, sa = np.cos(best_angle), np.sin(best_angle)
    R = np.array([[ca, -sa], [sa, ca]])
    t = mu_t - R @ mu_s
    if VERBOSE:
        print(f"  Rotation search: best angle {np.degrees(best_angle):.1f}°, "
              f"score {best_score:.4f}")
    return R, t, best_score


# ── feature-based pre-alignment, features.py:22-160, 247-315 ─────────────────────────────────────────
FEAT_MAX_ROWS, FEAT_MAX_KP, FEAT_DESC_STRIDE = _lib.FT_MAX_ROWS, _lib.FT_MAX_KP, _lib.FT_DESC_STRIDE


def _pairwise_sq(a, b):
    """Squared L2 distances between every row of a (N, D) and b (M, D) -> (N, M), features.py:22-30 (NumPy: the module
    exports it; ``match_descriptors`` takes direct differences on the device instead)."""
    a_sq = np.sum(a ** 2, axis=1, keepdims=True)
    b_sq = np.sum(b ** 2, axis=1, keepdims=True)
    return np.maximum(a_sq + b_sq.T - 2.0 * a @ b.T, 0.0)


def _rigid_from_points(src, dst):
    """Closed-form rigid (R, t) aligning src -> dst, both (N, 2), N >= 2 — features.py:111-122, in NumPy as the reference."""
    mu_s = src.mean(0)
    mu_d = dst.mean(0)
    W = (src - mu_s).T @ (dst - mu_d)
    U, _, Vt = np.linalg.svd(W)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[-1] *= -1
        R = Vt.T @ U.T
    t = mu_d - R @ mu_s
    return R, t


def _feature_rows(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0:
        raise ValueError(f"{name} must have shape (n, 2) with n >= 1, got {a.shape}")
    if a.shape[0] > FEAT_MAX_ROWS:
        raise _lib.IcpmiError(f"{name}: {a.shape[0]} rows; the feature kernels hold at most {FEAT_MAX_ROWS} rows of a cloud on "
                              "chip (the pipeline runs on voxel-filtered clouds) and there is no CPU fallback")
    return a


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def compute_curvature(points, k=10):
    """Curvature of every point from the PCA of its k nearest neighbours — features.py:35-54.  The neighbours of a point
    are summed in ascending row order (the reference: in distance order), which agrees with the reference to its own
    rounding and gives points with the same neighbour set the same bits."""
    pts = _feature_rows(points, "points")
    cs = _b.CloudSet.from_numpy([pts])
    out = torch.zeros(len(pts), dtype=torch.float64, device=cs.pts.device)
    _lib.check(_lib.lib().icpmi_feature_curvature_batch(_b._ptr(cs.pts), _b._ptr(cs.off), None, None, 1, int(k), _b._ptr(out),
                                                        _b._stream()), "compute_curvature")
    return out.cpu().numpy()


def extract_keypoints(points, curvatures, top_n=100, min_dist=0.3):
    """The top_n highest-curvature points with spatial non-max suppression — features.py:57-71.  The candidate order is
    ``np.argsort(-curvatures)`` taken HERE, with the reference's expression: equal curvatures are common (points with the
    same neighbours) and NumPy's unstable sort decides their order, so the same code in the same process is the only way
    to walk the reference's order; the walk itself runs on the device."""
    pts = _feature_rows(points, "points")
    order = np.argsort(-curvatures)                       # descending, features.py:59
    if len(order) != len(pts):
        raise ValueError("points and curvatures differ in length")
    top_n = int(top_n)
    if top_n <= 0:
        return np.array([], dtype=int)
    if top_n > FEAT_MAX_KP:
        raise _lib.IcpmiError(f"top_n = {top_n}: the keypoint kernel keeps at most {FEAT_MAX_KP}")
    cs = _b.CloudSet.from_numpy([pts])
    dev = cs.pts.device
    kp = torch.zeros(top_n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_order = _i32(order, dev)
    _lib.check(_lib.lib().icpmi_feature_keypoints_batch(_b._ptr(cs.pts), _b._ptr(cs.off), None, None, 1, None, _b._ptr(d_order),
                                                        top_n, float(min_dist), _b._ptr(kp), _b._ptr(cnt), top_n, _b._stream()),
               "extract_keypoints")
    return kp.cpu().numpy()[:int(cnt.item())].astype(int)


def compute_descriptors(points, kp_idx, k=30):
    """Sorted distances from every keypoint to its k nearest other points — features.py:76-87, (n_kp, min(k, n - 1))."""
    pts = _feature_rows(points, "points")
    kp_idx = np.asarray(kp_idx, dtype=np.int64).reshape(-1)
    n_kp = len(kp_idx)
    kd = min(int(k), len(pts) - 1)
    if n_kp == 0:
        return np.empty((0, max(kd, 0)))
    if n_kp > FEAT_MAX_KP:
        raise _lib.IcpmiError(f"{n_kp} keypoints: the descriptor kernel takes at most {FEAT_MAX_KP} per cloud")
    if kp_idx.min() < -len(pts) or kp_idx.max() >= len(pts):
        raise IndexError("keypoint index out of bounds")
    cs = _b.CloudSet.from_numpy([pts])
    dev = cs.pts.device
    desc = torch.zeros((n_kp, FEAT_DESC_STRIDE), dtype=torch.float64, device=dev)
    dlen = torch.zeros(1, dtype=torch.int32, device=dev)
    d_kp, d_cnt = _i32(kp_idx % len(pts), dev), _i32([n_kp], dev)
    _lib.check(_lib.lib().icpmi_feature_descriptors_batch(_b._ptr(cs.pts), _b._ptr(cs.off), None, None, 1, _b._ptr(d_kp),
                                                          _b._ptr(d_cnt), n_kp, int(k), _b._ptr(desc), _b._ptr(dlen),
                                                          _b._stream()), "compute_descriptors")
    return desc.cpu().numpy()[:, :int(dlen.item())].copy()


def match_descriptors(da, db, ratio=0.8):
    """Nearest-neighbour matching with Lowe's ratio test — features.py:92-106 -> list of (idx_a, idx_b)."""
    if len(da) == 0 or len(db) < 2:
        return []
    da, db = np.asarray(da, dtype=np.float64), np.asarray(db, dtype=np.float64)
    if da.ndim != 2 or db.ndim != 2 or da.shape[1] != db.shape[1]:
        raise ValueError(f"descriptors of different lengths: {da.shape} and {db.shape}")
    if max(len(da), len(db)) > FEAT_MAX_KP or da.shape[1] >= FEAT_DESC_STRIDE or da.shape[1] == 0:
        raise _lib.IcpmiError(f"match_descriptors takes at most {FEAT_MAX_KP} descriptors of 1 to {FEAT_DESC_STRIDE - 1} distances")
    _b.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    stride = max(len(da), len(db))
    host = np.zeros((2, stride, FEAT_DESC_STRIDE))
    host[0, :len(da), :da.shape[1]] = da
    host[1, :len(db), :db.shape[1]] = db
    desc = torch.from_numpy(host).to(dev)
    ratio_sq = ratio ** 2                                  # features.py:100
    out = torch.zeros((stride, 2), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_len, d_cnt, d_ps, d_pt = _i32([da.shape[1]] * 2, dev), _i32([len(da), len(db)], dev), _i32([0], dev), _i32([1], dev)
    _lib.check(_lib.lib().icpmi_feature_match_batch(_b._ptr(desc), _b._ptr(d_len), _b._ptr(d_cnt),
                                                    stride, _b._ptr(d_ps), _b._ptr(d_pt), 1, float(ratio_sq),
                                                    _b._ptr(out), _b._ptr(cnt), _b._stream()), "match_descriptors")
    m = out.cpu().numpy()[:int(cnt.item())]
    return [(int(i), int(j)) for i, j in m]


def ransac_align(kp_s, kp_t, matches, n_iter=1000, inlier_thresh=0.5):
    """RANSAC rigid 2-D transform from matched keypoints — features.py:125-160 -> (R, t, n_inliers), (None, None, 0) under
    two matches.

    The n_iter hypotheses are drawn HERE, before the launch, with the reference's own call in the reference's order
    (``np.random.choice(n, 2, replace=False)`` once per iteration): after ``np.random.seed(s)`` they are the reference's
    hypotheses and the global stream is left where the reference leaves it.  That costs about 6 ms of host time per 1 000
    draws; ``icpmi.prealign.FeatureAlignBatch`` draws a whole batch's hypotheses in one vectorised call instead.  All of
    them are then scored in one launch."""
    if len(matches) < 2:
        return None, None, 0
    kp_s, kp_t = _feature_rows(kp_s, "kp_s"), _feature_rows(kp_t, "kp_t")
    m = np.ascontiguousarray(np.asarray(matches, dtype=np.int64).reshape(-1, 2))
    n = len(m)
    if n > FEAT_MAX_KP:
        raise _lib.IcpmiError(f"{n} matches: the RANSAC kernel takes at most {FEAT_MAX_KP}")
    if m[:, 0].min() < 0 or m[:, 0].max() >= len(kp_s) or m[:, 1].min() < 0 or m[:, 1].max() >= len(kp_t):
        raise IndexError("match index out of bounds")
    n_iter = int(n_iter)
    hyp = np.zeros((max(n_iter, 1), 2), dtype=np.int32)
    for h in range(n_iter):
        hyp[h] = np.random.choice(n, 2, replace=False)    # features.py:141
    cs = _b.CloudSet.from_numpy([kp_s, kp_t])
    dev = cs.pts.device
    stride = max(len(kp_s), len(kp_t), n)
    kp = np.zeros((2, stride), dtype=np.int32)
    kp[0, :len(kp_s)] = np.arange(len(kp_s))
    kp[1, :len(kp_t)] = np.arange(len(kp_t))
    mm = np.zeros((stride, 2), dtype=np.int32)
    mm[:n] = m
    rec = torch.zeros((1, _lib.FTREC_DOUBLES), dtype=torch.float64, device=dev)
    d_kp, d_kc, d_ps, d_pt = _i32(kp, dev), _i32([len(kp_s), len(kp_t)], dev), _i32([0], dev), _i32([1], dev)
    d_m, d_mc, d_hyp = _i32(mm, dev), _i32([n], dev), _i32(hyp, dev)
    _lib.check(_lib.lib().icpmi_feature_ransac_batch(
        _b._ptr(cs.pts), _b._ptr(cs.off), None, _b._ptr(d_kp), _b._ptr(d_kc), stride, _b._ptr(d_ps), _b._ptr(d_pt), 1,
        _b._ptr(d_m), _b._ptr(d_mc), _b._ptr(d_hyp) if n_iter else None, None, n_iter, 0, float(inlier_thresh), _b._ptr(rec),
        None, _b._stream()),
        "ransac_align")
    r = rec.cpu().numpy()[0]
    return r[_lib.FTREC_R:_lib.FTREC_R + 4].reshape(2, 2).copy(), r[_lib.FTREC_T:_lib.FTREC_T + 2].copy(), int(r[_lib.FTREC_INLIERS])


def feature_based_alignment(source, target, voxel_size=0.2, k_curvature=10, top_n=100, min_kp_dist=0.3, k_descriptor=30,
                            ratio_threshold=0.8, ransac_iterations=1000, inlier_threshold=0.5):
    """Full feature-based alignment pipeline — features.py:247-315 -> (R (2,2), t (2,), n_inliers); identity, zeros, 0 when
    a filtered cloud has fewer than 10 points, fewer than 2 keypoints are found or fewer than 2 matches survive.

    The reference's own composition of the stages above, each on the device; the candidate order of the keypoints and the
    RANSAC draws are NumPy's, taken on the host (see ``extract_keypoints`` and ``ransac_align``)."""
    from .icp import voxel_downsample                     # avoid circular import

    src = voxel_downsample(source, voxel_size)
    tgt = voxel_downsample(target, voxel_size)

    if len(src) < 10 or len(tgt) < 10:
        return np.eye(2), np.zeros(2), 0

    curv_s = compute_curvature(src, k=k_curvature)
    curv_t = compute_curvature(tgt, k=k_curvature)
    kpi_s = extract_keypoints(src, curv_s, top_n=top_n, min_dist=min_kp_dist)
    kpi_t = extract_keypoints(tgt, curv_t, top_n=top_n, min_dist=min_kp_dist)

    if len(kpi_s) < 2 or len(kpi_t) < 2:
        return np.eye(2), np.zeros(2), 0

    desc_s = compute_descriptors(src, kpi_s, k=k_descriptor)
    desc_t = compute_descriptors(tgt, kpi_t, k=k_descriptor)

    matches = match_descriptors(desc_s, desc_t, ratio=ratio_threshold)
    if len(matches) < 2:
        return np.eye(2), np.zeros(2), 0

    R, t, n_inliers = ransac_align(src[kpi_s], tgt[kpi_t], matches, n_iter=ransac_iterations, inlier_thresh=inlier_threshold)

    if R is None:
        return np.eye(2), np.zeros(2), 0

    if VERBOSE:
        print(f"  Feature alignment: {len(matches)} matches, {n_inliers} inliers")
    return R, t, n_inliers
