"""A scan history that stays prepared on the device, for loop-closure matching.

The reference picks its loop-closure candidates from ``scan_history`` (slam.py:566-574, ``_find_loop_candidates``,
slam.py:230-268) and runs ``_run_icp_pair(points, scan_history[idx][0], ...)`` on each (slam.py:575-579).  A past scan
never changes — pose-graph optimisation moves its pose, not its points (slam.py:606-607) — yet every ``_run_icp_pair``
filters it twice, takes its mean and builds two k-d trees of it.  ``ScanHistory`` does that work once, when the scan is
appended (slam.py:554), and a query is the rotation-search kernel and the ICP kernels on what it left:

    hist = ScanHistory(voxel_size=0.06, normal_k=10, rotation_voxel_size=0.3)
    sid = hist.add(points)                                     # slam.py:554
    cands = find_loop_candidates(pose, poses, sid, 3.0, 50, 5) # slam.py:566-574
    m = hist.match(sid, [k for k, _ in cands], error_accept=0.05, stop_after_first_accepted=True)
    m.run(); first = m.first_accepted()                        # slam.py:575-597

After an accepted closure every pose has moved and the reference transforms every past scan again on the host to rebuild
the map and the submap buffer (slam.py:271-277, 612-615).  The raw rows are here, so ``world_rows(poses, ids)`` is one
launch of ``icpmi_history_world_rows`` — NumPy's ``points @ T[:2, :2].T + T[:2, 2]`` bit for bit — and
``OccupancyGrid2D.rebuild_from_history`` / ``RollingSubmap.reset_from_history`` take the history and the poses.

``find_loop_candidates`` trusts the pose estimates: a revisit that drift has carried beyond its threshold is never tried.
A history built with ``signature={}`` also keeps a polar occupancy image of every scan (260 bytes) and finds candidates by
appearance, on the device, whatever the headings and the estimates:

    hist = ScanHistory(..., signature={"ring_width": 0.5})
    cands = similar_loop_candidates(hist, sid, min_interval=50, max_candidates=5, min_score=0.3)   # [(idx, score), ...]
    m = hist.match(sid, [k for k, _ in cands], ...)

``hist.similar(sources, top_k=...)`` is the query behind it (``SimilarScans``: ids, scores, a heading estimate per
candidate, optionally the whole similarity row).

``match`` returns a ``RunIcpPairBatch`` whose clouds are the resident ones: ``run()`` / ``unpack()`` / ``first_accepted()``
are that class's own code, and its records are the batch path's bit for bit (same kernels on the same filtered rows).

torch is used for device memory and streams only; the device work is include/icpmi.h's ``icpmi_history_*``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .batch import PREP_MAX_POINTS, CloudSet, IcpBatch, PairList, _ptr, _stream, require_gpu
from .prealign import (ALIGNMENT_METHODS, FEAT_CLOUD_KEYS, FEAT_DEFAULTS, FeatureAlignBatch, RotationSearchBatch, RunIcpPairBatch,
                       _gate_given)


def find_loop_candidates(current_pose, poses, current_idx, distance_threshold, min_interval, max_candidates,
                         min_cumulative_travel=10.0):
    """``_find_loop_candidates`` (slam.py:230-268) -> [(idx, dist), ...]: the scans at least ``min_interval`` scans old,
    closer than ``distance_threshold`` to the current position and at least ``min_cumulative_travel`` of driven path away
    (a robot standing still has not come back), nearest first (equal distances in scan order), at most ``max_candidates``.

    poses: a sequence of 3 x 3 pose matrices or an (n, 2) array of positions; current_pose: a 3 x 3 matrix or a position.
    Host only and vectorised: the poses live in the pose graph on the host, and there are thousands of them at most."""
    cur = np.asarray(current_pose, dtype=np.float64)
    cur = cur[:2, 2] if cur.ndim == 2 else cur[:2]
    P = np.asarray(poses, dtype=np.float64)
    if P.ndim == 3:
        P = P[:, :2, 2]
    P = P.reshape(-1, 2)
    n = len(P)
    if n == 0:
        return []
    step = np.diff(P, axis=0)
    cum = np.zeros(n)
    np.cumsum(np.sqrt(step[:, 0] ** 2 + step[:, 1] ** 2), out=cum[1:])        # slam.py:247-251, summed in scan order
    d = cur[None, :] - P
    dist = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)                                # slam.py:258
    travel = cum[current_idx] - cum if current_idx < n else np.zeros(n)        # slam.py:263
    # the reference's three `continue`s, negated as it writes them (a NaN fails none of them)
    keep = ~(current_idx - np.arange(n) < min_interval) & ~(dist >= distance_threshold) & ~(travel < min_cumulative_travel)
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(dist[idx], kind="stable")][:max_candidates]
    return [(int(k), float(dist[k])) for k in idx]


SIG_DEFAULTS = {"ring_width": 0.5, "min_range": 0.1}


def signature_config(signature):
    """The ``signature`` argument of ``ScanHistory`` over ``SIG_DEFAULTS``, checked -> {ring_width, min_range} as floats."""
    unknown = set(signature) - set(SIG_DEFAULTS)
    if unknown:
        raise ValueError(f"signature takes {sorted(SIG_DEFAULTS)}: got {sorted(unknown)}")
    cfg = {k: float(signature.get(k, v)) for k, v in SIG_DEFAULTS.items()}
    for k, v in cfg.items():
        if not (v > 0 and np.isfinite(v)):
            raise ValueError(f"signature[{k!r}] must be positive and finite: got {v!r}")
    return cfg


def signature_tables(ring_width, min_range):
    """The 63 doubles of a signature store (include/icpmi.h): edge2[33] = (min_range + j * ring_width) ** 2, then cos and
    sin of k pi / 32 for k = 1 .. 15.  The device only compares against them: no libm of its own has to agree with NumPy's."""
    edge = min_range + np.arange(_lib.SIG_RINGS + 1, dtype=np.float64) * ring_width
    a = np.arange(1, 16, dtype=np.float64) * np.pi / 32
    return np.ascontiguousarray(np.concatenate([edge * edge, np.cos(a), np.sin(a)]))


def shift_yaw(shift):
    """The heading of a source relative to a candidate that a record's ``shift`` implies, in (-pi, pi]: rotating the
    candidate's image by ``shift`` sectors counter-clockwise gives the source's, and a scene seen turned counter-clockwise
    is a sensor turned clockwise — source yaw - candidate yaw = -shift * 2 pi / 64 (to within a sector, and to within the
    symmetries of the place)."""
    yaw = -(np.asarray(shift, dtype=np.float64) % _lib.SIG_SECTORS) * (2.0 * np.pi / _lib.SIG_SECTORS)
    return np.where(yaw <= -np.pi, yaw + 2.0 * np.pi, yaw)


def similar_args(ids, n_scans, top_k=10, min_interval=0, lo=None, hi=None):
    """The host side of ``ScanHistory.similar``, checked: (ids, lo, hi) as int32 arrays, one entry per source.  ids: scan ids
    in [0, n_scans] — n_scans is a staged source.  Without ``lo`` / ``hi`` the candidates of source id are the scans
    [0, id - min_interval + 1): the reference's ``current_idx - i < min_interval -> continue`` (slam.py:255).  ``lo`` /
    ``hi``: one integer for all sources or one per source; the device clips them to [0, n_scans)."""
    if not 1 <= int(top_k) <= _lib.SIG_MAX_TOP:
        raise ValueError(f"top_k must lie in [1, {_lib.SIG_MAX_TOP}]: got {top_k}")
    if int(min_interval) < 0:
        raise ValueError(f"min_interval must not be negative: got {min_interval}")
    ids = _scan_ids(ids, ("sources", "source ids"), n_scans + 1)

    def bound(v, default, name):
        if v is None:
            return default
        a = np.asarray(v)
        if a.ndim > 1 or not np.issubdtype(a.dtype, np.integer) or (a.ndim == 1 and len(a) != len(ids)):
            raise ValueError(f"{name} must be one integer or one per source ({len(ids)})")
        return np.ascontiguousarray(np.broadcast_to(np.clip(a, -2 ** 31, 2 ** 31 - 1), ids.shape), dtype=np.int32)
    return ids, bound(lo, np.zeros(len(ids), dtype=np.int32), "lo"), bound(hi, ids - np.int32(min_interval) + 1, "hi")


def similar_loop_candidates(hist, source, *, min_interval, max_candidates, min_score):
    """Loop-closure candidates by appearance -> [(idx, score), ...], the shape of ``find_loop_candidates``' return (its
    second entry a similarity in [0, 1], best first, where that one's is a distance, nearest first): the at most
    ``max_candidates`` scans at least ``min_interval`` scans older than ``source`` (a scan id, or an (n, 2) array taken as the
    scan after the last) that look most like it, those scoring below ``min_score`` dropped.  ``[k for k, _ in cands]``
    goes into ``hist.match``.  One query of ``hist.similar``; synchronises."""
    if not (isinstance(source, (int, np.integer)) or np.ndim(source) == 2):
        raise ValueError("source must be one scan id or one (n, 2) array")
    found = hist.similar(source, top_k=max_candidates, min_interval=min_interval)
    found.run()
    return [(k, score) for k, score, _ in found.unpack()[0] if score >= min_score]


def scan_reach(points):
    """The largest row norm of an (n, 2) array, 0.0 for no rows; NaN or inf as soon as one coordinate is (``hypot``: no
    overflow or underflow on the way, so a finite reach is the norm to within an ulp)."""
    a = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(a) == 0:
        return 0.0
    return float(np.hypot(a[:, 0], a[:, 1]).max())               # (max propagates a NaN)


def pose_rows(poses, n):
    """n pose matrices (3 x 3 each: ``PoseGraph2D.get_poses_as_matrices()``) -> (n, 6) float64 rows {R row-major, t}."""
    P = np.asarray(poses, dtype=np.float64)
    if n == 0 and P.size == 0:
        return np.zeros((0, 6))
    if P.shape != (n, 3, 3):
        raise ValueError(f"poses must be {n} matrices of 3 x 3 (one per scan id): got shape {P.shape}")
    return np.ascontiguousarray(np.concatenate([P[:, :2, :2].reshape(n, 4), P[:, :2, 2]], axis=1))


def _scan_ids(ids, what, n_scans, one=False):
    """``ids`` as a contiguous int32 array, checked: a 1-D sequence of integers, every one in [0, n_scans) (repeats and
    an empty list are fine).  what: (the argument's name, its entries' name) for the messages.  ``one``: a single id,
    not a sequence -> that id as an int."""
    name, entries = what
    a = np.asarray([int(ids)] if one else ids)
    if a.ndim != 1 or (len(a) and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{name} must be a 1-D sequence of scan ids")
    if len(a) and (a.min() < 0 or a.max() >= n_scans):
        raise ValueError(f"{entries} must lie in [0, {n_scans}): got " + (f"{ids}" if one else f"{int(a.min())}..{int(a.max())}"))
    return int(a[0]) if one else np.ascontiguousarray(a, dtype=np.int32)


class _ResidentIcp(IcpBatch):
    """``IcpBatch`` over a history's filtered clouds and prepared targets: ``run()`` is the ICP launch alone."""
    strict_method = True        # nothing here is the reference's call: an unknown method string is refused

    def __init__(self, hist, pair_src, pair_tgt, error_threshold, max_iterations, method, max_corr_dist, R_init, t_init):
        if method == "point_to_line" and hist.normal_k is None:
            raise ValueError("this history holds no normals (normal_k=None): point_to_point only")
        self.history = hist
        self._init_common(hist.raw, pair_src, pair_tgt, error_threshold, max_iterations, hist.voxel_size, R_init, t_init, method,
                          -1 if hist.normal_k is None else hist.normal_k, max_corr_dist)
        self.vox, self.normals, self.prepared, self.fast = hist.vox, None, hist.icp_prepared, True

    @property
    def layout_rows(self):
        return self.history.row_capacity

    def prepare(self):
        raise _lib.IcpmiError("a resident batch is prepared when its scans are added")

    def run(self, events=None):
        return self.launch_icp(events)


class _ResidentSearch(RotationSearchBatch):
    """``RotationSearchBatch`` over a history's search state: ``run()`` is ``icpmi_history_search``."""

    def __init__(self, hist, pair_src, pair_tgt, angle_step_coarse, angle_step_fine, init, max_rows_hint):
        self.history = hist
        self._init_common(hist.raw, pair_src, pair_tgt, hist.rotation_voxel_size, angle_step_coarse, angle_step_fine, init,
                          max_rows_hint)
        sizes = hist.sizes()
        self.max_n = int(max(sizes[self.pair_src_host].max(), sizes[self.pair_tgt_host].max())) if self.B else 0

    def run(self):
        if self.too_many_angles:
            return self.mark_over_capacity()
        t = self.tables
        mf = t.max_fine
        check(_lib.lib().icpmi_history_search(
            C.byref(self.history.state), _ptr(self.pair_src), _ptr(self.pair_tgt), self.B, self.max_n, _ptr(t.d_cs), len(t.coarse),
            _ptr(t.d_fcs) if mf else None, _ptr(t.d_fn) if mf else None, mf, self.max_rows_hint, _ptr(self.records),
            _ptr(self.init), _stream()), "rotation_search (history)")
        return self.records


class _ResidentFeatures(FeatureAlignBatch):
    """``FeatureAlignBatch`` over a history's feature store: ``run()`` is ``icpmi_history_feature_align`` — matching, RANSAC
    and the record on the tables the scans got when they were added (with a start per pair, after the per-cloud stages of
    the transformed sources, which are per pair by nature)."""

    def __init__(self, hist, pair_src, pair_tgt, cfg, hypotheses, rng, init_in, init_out):
        self.history = hist
        self._init_common(hist.raw, pair_src, pair_tgt, cfg, hypotheses, rng, init_in, init_out)
        self.max_n = int(hist.sizes()[self.pair_src_host].max()) if self.B else 0
        need = _lib.lib().icpmi_history_feature_align_workspace_bytes(self.B, self.max_n, int(self.cfg["top_n"]),
                                                                      1 if init_in is not None else 0)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=hist.device)

    def run(self):
        c, h = self.cfg, self.history
        check(_lib.lib().icpmi_history_feature_align(
            C.byref(h.state), C.byref(h.store), h.raw.off_host.ctypes.data_as(C.c_void_p), _ptr(self.pair_src),
            self.pair_src_host.ctypes.data_as(C.c_void_p), _ptr(self.pair_tgt), self.B, self.max_n, float(c["ratio_threshold"] ** 2),
            _ptr(self.hyp_idx), _ptr(self.hyp_u), self.n_iter, 0, float(c["inlier_threshold"]), int(c["min_inliers"]),
            _ptr(self.init_in), _ptr(self.init_out), _ptr(self.records), _ptr(self.ws), self.ws.numel(), _stream()),
            "feature_based_alignment (history)")
        return self.records


class HistoryMatch(RunIcpPairBatch):
    """What ``ScanHistory.match`` returns: ``RunIcpPairBatch`` (its ``run`` / ``unpack`` / ``first_accepted``) with the
    history's resident clouds behind it.  Valid while the history keeps its buffers: ``run()`` raises once the history has
    grown, or — for a source that was an array — once another scan or source has been staged over it."""

    def __init__(self, hist, source_id, candidates, staged, error_threshold, max_iterations, method, max_corr_dist,
                 angle_step_coarse, angle_step_fine, max_rows_hint, error_accept, stop_after_first_accepted, index_base,
                 index_stride, alignment_method="rotation_search", feat_cfg=None, hypotheses=None, rng=None):
        _gate_given(stop_after_first_accepted, error_accept)
        B = len(candidates)
        pairs = PairList(np.full(B, source_id, dtype=np.int32), candidates)
        self.history = hist
        self.layout_generation = hist.layout_generation
        self.stage_generation = hist.stage_generation if staged else None
        icp = _ResidentIcp(hist, pairs, None, error_threshold, max_iterations, method, max_corr_dist,
                           np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2)))
        search = features = None
        if alignment_method in ("rotation_search", "both"):                         # slam.py:60
            search = _ResidentSearch(hist, pairs, None, angle_step_coarse, angle_step_fine, icp.init, max_rows_hint)
        if alignment_method in ("features", "both"):                                # slam.py:68-88, as RunIcpPairBatch wires it
            features = _ResidentFeatures(hist, pairs, None, feat_cfg, hypotheses, rng,
                                         init_in=icp.init if search is not None else None, init_out=icp.init)
        sizes = hist.sizes()
        max_raw_n = int(max(sizes[pairs.src_host].max(), sizes[pairs.tgt_host].max())) if B else 0
        self._init_parts(alignment_method, icp, search, features, error_accept, stop_after_first_accepted, index_base,
                         index_stride, max_rows_hint, max_raw_n)

    def run(self, events=None):
        h = self.history
        if h.layout_generation != self.layout_generation:
            raise _lib.IcpmiError("the history has grown since this match was made: call match() again")
        if self.stage_generation is not None and h.stage_generation != self.stage_generation:
            raise _lib.IcpmiError("the staged source of this match has been overwritten: call match() again")
        return super().run(events)


class SimilarScans:
    """What ``ScanHistory.similar`` returns: one ``icpmi_history_similar`` query, its buffers allocated and its arguments
    uploaded.  ``run()`` enqueues it on the current stream (two launches, nothing returns to the host) and may be repeated;
    ``unpack()`` synchronises.  Valid while the history keeps its buffers and its staged source, as a ``HistoryMatch`` is."""

    def __init__(self, hist, ids, lo, hi, top_k, all_scores, staged):
        self.history, self.top_k, self.n_queries, self.n_scans = hist, int(top_k), len(ids), hist.n_scans
        self.layout_generation = hist.layout_generation
        self.stage_generation = hist.stage_generation if staged else None
        dev = hist.device
        self.ids_host = ids
        self.query_ids, self.lo, self.hi = (torch.from_numpy(a).to(dev) for a in (ids, lo, hi))
        self.records_dev = torch.zeros((self.n_queries, self.top_k, _lib.SIG_REC_INTS), dtype=torch.int32, device=dev)
        self.all_dev = torch.zeros((self.n_queries, self.n_scans), dtype=torch.int32, device=dev) if all_scores else None
        need = _lib.lib().icpmi_history_similar_workspace_bytes(self.n_queries, self.n_scans, self.top_k)
        if need == 0:
            raise ValueError(f"{self.n_queries} sources against {self.n_scans} scans: too many pairs for one query (2^31 - 1 at most, "
                             "65 535 sources at most)")
        self.ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        self.records = self.all = None                             # NumPy arrays, from unpack()

    def run(self):
        h = self.history
        if h.layout_generation != self.layout_generation:
            raise _lib.IcpmiError("the history has grown since this query was made: call similar() again")
        if self.stage_generation is not None and h.stage_generation != self.stage_generation:
            raise _lib.IcpmiError("the staged source of this query has been overwritten: call similar() again")
        check(_lib.lib().icpmi_history_similar(C.byref(h.state), _ptr(h.sig), _ptr(h.sig_bits), _ptr(self.query_ids), self.n_queries,
                                               _ptr(self.lo), _ptr(self.hi), self.n_scans, self.top_k, _ptr(self.records_dev),
                                               _ptr(self.all_dev), _ptr(self.ws), self.ws.numel(), _stream()), "history_similar")
        return self.records_dev

    def unpack(self):
        """-> per source, the list of its (id, score in [0, 1], yaw) best first — yaw: ``shift_yaw`` of the record's shift,
        the heading of the source relative to that candidate.  Leaves ``records`` (n_sources, top_k, 4) int32 {id, score,
        shift, best} and ``all`` (n_sources, n_scans) int32 (score << 8) | shift, -1 outside a source's range (None without
        ``all_scores``) as NumPy arrays.  Synchronises."""
        self.records = self.records_dev.cpu().numpy()
        self.all = None if self.all_dev is None else self.all_dev.cpu().numpy()
        yaw = shift_yaw(self.records[:, :, _lib.SIG_REC_SHIFT])
        return [[(int(r[_lib.SIG_REC_ID]), r[_lib.SIG_REC_SCORE] / 65535.0, float(y)) for r, y in zip(recs, yaws) if r[_lib.SIG_REC_ID] >= 0]
                for recs, yaws in zip(self.records, yaw)]


class ScanHistory:
    """An append-only set of 2-D scans (at most 4096 rows each: the on-chip kernels) resident on one device, each filtered
    at the ICP voxel size and at the rotation search's, with its mean and both search orders (and normals from ``normal_k``
    neighbours; ``None``: a point_to_point-only history) — everything ``_run_icp_pair`` (slam.py:53-98) derives from a
    target alone, computed once by ``add``.

    The buffers hold ``scan_capacity`` scans and ``row_capacity`` raw rows (128 bytes of device memory per row); either
    doubles when it is exceeded (new buffers, device-to-device copies), and results do not depend on that.

    ``feat_cfg`` (a dict, possibly empty): the history also keeps what ``feature_based_alignment`` (features.py:247-315)
    derives from a cloud alone — the filter at the feature voxel size, curvature, keypoints, descriptors — so that
    ``match(alignment_method="features" / "both")`` is resident too.  Its cloud-side keys (``FEAT_CLOUD_KEYS``) over
    ``FEAT_DEFAULTS`` fix that store: 24 more bytes per row and 12 + 260 * kp_stride bytes per scan (27 052 at the
    reference's ``top_n`` of 100).  ``None``: no store, and ``match`` refuses those two methods.

    ``signature`` (a dict, possibly empty: ``ring_width`` 0.5 and ``min_range`` 0.1 unless given, in the scans' unit): the
    history also keeps an appearance signature of every scan — a binary polar occupancy image of its raw rows about the
    sensor, 32 rings by 64 sectors, 260 bytes a scan (include/icpmi.h) — and ``similar`` ranks scans against a scan by
    it, whatever their headings and wherever the pose graph believes them to be.  ``None``: no signatures, nothing
    allocated, and ``similar`` refuses."""

    def __init__(self, voxel_size=0.06, normal_k=10, rotation_voxel_size=0.3, scan_capacity=256, row_capacity=None, device=None,
                 feat_cfg=None, signature=None):
        require_gpu()
        if not voxel_size > 0 or not rotation_voxel_size > 0:
            raise ValueError("voxel sizes must be positive")
        self.sig_cfg = None if signature is None else signature_config(signature)
        self.feat_cfg = self.store = None
        if feat_cfg is not None:
            self.feat_cfg = {k: feat_cfg.get(k, FEAT_DEFAULTS[k]) for k in FEAT_CLOUD_KEYS}
            c = self.feat_cfg
            if not c["voxel_size"] > 0:
                raise ValueError("voxel sizes must be positive")
            if max(int(c["k_curvature"]), int(c["k_descriptor"])) > 31 or int(c["top_n"]) > _lib.FT_MAX_KP:
                raise ValueError(f"resident features hold k <= 31 neighbours and top_n <= {_lib.FT_MAX_KP} keypoints")
            self.kp_stride = 8 if int(c["top_n"]) <= 0 else (int(c["top_n"]) + 7) // 8 * 8
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.voxel_size, self.rotation_voxel_size = float(voxel_size), float(rotation_voxel_size)
        self.normal_k = None if normal_k is None else int(normal_k)
        self.n_scans = self.rows_used = 0
        self.reach = np.zeros(0)           # host: the largest row norm of every scan (non-finite if a coordinate is)
        self.allow_polar = True            # until a scan above 2048 rows arrives (the ICP kernels for such targets walk projections)
        self.layout_generation = self.stage_generation = 0
        self.scan_capacity = self.row_capacity = 0
        if self.sig_cfg is not None:
            self.sig_tables = torch.from_numpy(signature_tables(**self.sig_cfg)).to(self.device)
        scan_capacity = max(int(scan_capacity), 1)
        self._allocate(scan_capacity, max(int(row_capacity), 1) if row_capacity is not None else 1024 * scan_capacity)

    # ── buffers ──────────────────────────────────────────────────────────────
    def _allocate(self, S, R):
        """Buffers for S scans and R rows, holding what the current ones hold."""
        L = _lib.lib()
        dev, n, rows = self.device, self.n_scans, self.rows_used
        old = self.__dict__.copy() if self.scan_capacity else None
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        off_host = np.full(S + 1, rows, dtype=np.int32)
        if old:
            off_host[:n + 1] = old["raw"].off_host[:n + 1]
        self.raw = CloudSet(torch.empty((R, 2), **f64), off_host)
        self.vox = CloudSet(torch.empty((R, 2), **f64), off_host, cnt=torch.zeros(S, **i32), off=self.raw.off)
        self.rs_vox = CloudSet(torch.empty((R, 2), **f64), off_host, cnt=torch.zeros(S, **i32), off=self.raw.off)
        self.rs_means = torch.zeros((S, 2), **f64)
        self.ids = torch.arange(S, **i32)
        nbytes = L.icpmi_prepared_bytes(R, S, 0)
        self.icp_prepared = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.rs_prepared = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.voxel_ws = torch.empty(L.icpmi_voxel_workspace_bytes(PREP_MAX_POINTS), dtype=torch.uint8, device=dev)
        for name in ("icp_prepared", "rs_prepared"):
            check(L.icpmi_prepared_relayout(_ptr(old[name]) if old else None, self.row_capacity, self.scan_capacity, rows, n,
                                            _ptr(getattr(self, name)), nbytes, R, S, _stream()), "prepared_relayout")
        per_row = [("raw", None), ("vox", None), ("rs_vox", None)]
        per_scan = [("vox", "cnt"), ("rs_vox", "cnt"), ("rs_means", None)]
        if self.feat_cfg is not None:
            # the feature store: tables per row or per scan, so growing is plain prefix copies (curvature is scratch of an add)
            K = self.kp_stride
            self.ft_vox = CloudSet(torch.empty((R, 2), **f64), off_host, cnt=torch.zeros(S, **i32), off=self.raw.off)
            self.ft_curv = torch.empty(R, **f64)
            self.ft_kp, self.ft_kp_cnt = torch.zeros((S, K), **i32), torch.zeros(S, **i32)
            self.ft_desc, self.ft_desc_len = torch.zeros((S, K, _lib.FT_DESC_STRIDE), **f64), torch.zeros(S, **i32)
            per_row += [("ft_vox", None)]
            per_scan += [("ft_vox", "cnt"), ("ft_kp", None), ("ft_kp_cnt", None), ("ft_desc", None), ("ft_desc_len", None)]
        if self.sig_cfg is not None:
            # the signature store: 32 words and their bit count per scan (int64 holds the uint64 words: the bits are what matters)
            self.sig, self.sig_bits = torch.zeros((S, _lib.SIG_RINGS), dtype=torch.int64, device=dev), torch.zeros(S, **i32)
            per_scan += [("sig", None), ("sig_bits", None)]
        if old:
            pick = lambda d, name, part: getattr(d[name], part or "pts") if isinstance(d[name], CloudSet) else d[name]   # noqa: E731
            for name, part in per_row:
                pick(self.__dict__, name, part)[:rows].copy_(pick(old, name, part)[:rows])
            for name, part in per_scan:
                pick(self.__dict__, name, part)[:n].copy_(pick(old, name, part)[:n])
        self.scan_capacity, self.row_capacity = S, R
        self.state = _lib.History(self.raw.pts.data_ptr(), self.raw.off.data_ptr(), self.ids.data_ptr(), self.vox.pts.data_ptr(),
                                  self.vox.cnt.data_ptr(), self.icp_prepared.data_ptr(), self.rs_vox.pts.data_ptr(),
                                  self.rs_vox.cnt.data_ptr(), self.rs_means.data_ptr(), self.rs_prepared.data_ptr(),
                                  self.voxel_ws.data_ptr(), nbytes, self.voxel_ws.numel(), self.voxel_size, self.rotation_voxel_size,
                                  S, R, -1 if self.normal_k is None else self.normal_k, 1 if self.allow_polar else 0)
        if self.feat_cfg is not None:
            c = self.feat_cfg
            self.store = _lib.FeatureStore(self.ft_vox.pts.data_ptr(), self.ft_curv.data_ptr(), self.ft_vox.cnt.data_ptr(),
                                           self.ft_kp.data_ptr(), self.ft_kp_cnt.data_ptr(), self.ft_desc.data_ptr(),
                                           self.ft_desc_len.data_ptr(), float(c["voxel_size"]), float(c["min_kp_dist"]),
                                           int(c["k_curvature"]), int(c["top_n"]), int(c["k_descriptor"]), self.kp_stride)
        self.layout_generation += 1

    def _reserve(self, scans, rows):
        S, R = self.scan_capacity, self.row_capacity
        while S < scans:
            S *= 2
        while R < rows:
            R *= 2
        if R >= 2 ** 31:
            raise ValueError("history too large for 32-bit row offsets")
        if (S, R) != (self.scan_capacity, self.row_capacity):
            self._allocate(S, R)

    def _place(self, arrs, first, prepare, features=True):
        """Upload the clouds behind the rows in use as clouds first, first + 1, ... and process that range (``features``: into
        the feature store too, when the history has one)."""
        rows = self.rows_used
        ends = rows + np.cumsum([len(a) for a in arrs])
        self._reserve(first + len(arrs), int(ends[-1]))
        host = np.concatenate(arrs, axis=0)
        if len(host):
            self.raw.pts[rows:int(ends[-1])].copy_(torch.from_numpy(host))
        k = len(arrs)
        off = self.raw.off_host                                  # shared by the three cloud sets; clouds behind: zero rows
        off[first + 1:first + 1 + k] = ends
        off[first + 1 + k:] = ends[-1]
        self.raw.off[first + 1:first + 1 + k].copy_(torch.from_numpy(off[first + 1:first + 1 + k]))
        self.raw.off[first + 1 + k:].fill_(int(ends[-1]))
        self._process(first, k, prepare, features)
        self.stage_generation += 1
        return int(ends[-1])

    def _process(self, first, n, prepare, features=True, signatures=True):
        off_host = self.raw.off_host.ctypes.data_as(C.c_void_p)
        check(_lib.lib().icpmi_history_add(C.byref(self.state), off_host, first, n, 1 if prepare else 0, _stream()), "history_add")
        if features and self.store is not None:
            check(_lib.lib().icpmi_history_features_add(C.byref(self.state), C.byref(self.store), off_host, first, n, _stream()),
                  "history_features_add")
        if signatures and self.sig_cfg is not None:
            check(_lib.lib().icpmi_history_signatures_add(C.byref(self.state), _ptr(self.sig), _ptr(self.sig_bits), _ptr(self.sig_tables),
                                                          off_host, first, n, _stream()), "history_signatures_add")

    @staticmethod
    def _clouds(clouds):
        arrs = [np.ascontiguousarray(c, dtype=np.float64) for c in clouds]
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError("a scan must be an (n, 2) array")
            if len(a) > PREP_MAX_POINTS:
                raise ValueError(f"a scan of {len(a)} rows: the resident history holds scans of at most {PREP_MAX_POINTS} rows "
                                 "(the on-chip kernels); match larger clouds with RunIcpPairBatch")
        return arrs

    # ── the public interface ─────────────────────────────────────────────────
    def __len__(self):
        return self.n_scans

    def sizes(self):
        """Raw row count of every cloud slot (host; the scans, then a staged source, then zeros)."""
        return np.diff(self.raw.off_host)

    def counts(self):
        """Rows of every scan after the ICP's voxel filter (synchronises)."""
        return self.vox.cnt[:self.n_scans].cpu().numpy()

    def search_counts(self):
        """Rows of every scan after the rotation search's voxel filter (synchronises)."""
        return self.rs_vox.cnt[:self.n_scans].cpu().numpy()

    def feature_counts(self):
        """(rows after the feature voxel filter, keypoints) of every scan (synchronises); needs a feature store."""
        if self.store is None:
            raise ValueError("this history keeps no features (feat_cfg=None)")
        return self.ft_vox.cnt[:self.n_scans].cpu().numpy(), self.ft_kp_cnt[:self.n_scans].cpu().numpy()

    def signatures(self, ids=None):
        """(words (n, 32) uint64, bits (n,) int32) of the scans ``ids`` (every scan in order without) on the host: bit s of
        word r — ring r, sector s of the scan's polar image holds a raw row (synchronises); needs ``signature``."""
        if self.sig_cfg is None:
            raise ValueError("this history keeps no signatures (signature=None)")
        if ids is None:
            words, bits = self.sig[:self.n_scans], self.sig_bits[:self.n_scans]
        else:
            at = torch.from_numpy(_scan_ids(ids, ("ids", "scan ids"), self.n_scans).astype(np.int64)).to(self.device)
            words, bits = self.sig[at], self.sig_bits[at]
        return words.cpu().numpy().view(np.uint64), bits.cpu().numpy()

    def similar(self, sources, *, top_k=10, min_interval=0, lo=None, hi=None, all_scores=False):
        """The scans that look most like each source, whatever the headings -> a ``SimilarScans`` (``run()``, then
        ``unpack()``).  ``sources``: a scan id, a sequence of ids, or ONE (n, 2) array, which is staged behind the last scan as
        ``match`` stages its source, given a signature for this query and not added — it counts as scan id ``len(self)``.
        The candidates of source id are the scans [0, id - min_interval + 1) (slam.py:255: at least ``min_interval`` scans
        older; 0: the source itself included, with score 1), or [lo, hi) where given (one integer or one per source).  Per
        source the ``top_k`` (1 .. 64) best by score — the overlap of the two polar images over their union under the best
        of the 64 rotations, 0 .. 65535 — equal scores by lower id.  ``all_scores``: every candidate's score and shift as
        well, an (n_sources, n_scans) array (all scans as sources: the similarity matrix of the run)."""
        if self.sig_cfg is None:
            raise ValueError("this history keeps no signatures (signature=None)")
        staged = not isinstance(sources, (int, np.integer)) and np.ndim(sources) == 2
        if staged:
            ids = [self.n_scans]
        else:
            ids = [int(sources)] if isinstance(sources, (int, np.integer)) else sources
            ids = _scan_ids(ids, ("sources", "source ids"), self.n_scans)          # (a staged source is named by passing it)
        args = similar_args(ids, self.n_scans, top_k, min_interval, lo, hi)
        if staged:
            # cloud n_scans, for this query: rows_used stays; filtered too, so that a match of the same array finds its state
            self._place(self._clouds([sources]), self.n_scans, prepare=False, features=False)
        return SimilarScans(self, *args, top_k, all_scores, staged)

    def add(self, points):
        """Append one scan (slam.py:554) -> its id."""
        return self.add_many([points])[0]

    def add_many(self, clouds):
        """Append scans: one upload and one ``icpmi_history_add`` for the whole range -> their ids."""
        arrs = self._clouds(clouds)
        if not arrs:
            return []
        first = self.n_scans
        redo = self.allow_polar and max(len(a) for a in arrs) > 2048 and first > 0
        if max(len(a) for a in arrs) > 2048:
            self.allow_polar = False
            self.state.allow_polar = 0
        self.rows_used = self._place(arrs, first, prepare=True)
        self.n_scans = first + len(arrs)
        self.reach = np.concatenate([self.reach, [scan_reach(a) for a in arrs]])
        if redo:
            # a target above 2048 rows makes the ICP launch walk projections for every target of its batch: the earlier
            # scans, in bearing order until now, are put in order again (once in a history's life; their raw rows are here)
            # (their features and signatures do not depend on the search order: those stores are left alone)
            self._process(0, first, True, features=False, signatures=False)
        return list(range(first, self.n_scans))

    def match(self, source, candidates, *, error_threshold=1e-7, max_iterations=100, method="point_to_line", max_corr_dist=None,
              angle_step_coarse=2.0, angle_step_fine=0.2, max_rows_hint=0, error_accept=None, stop_after_first_accepted=False,
              alignment_method="rotation_search", index_base=0, index_stride=1, feat_cfg=None, hypotheses=None, rng=None):
        """``_run_icp_pair(source, scan k, ...)`` for every k of ``candidates`` (slam.py:575-579), in that order (repeats
        allowed) -> a ``HistoryMatch``.  ``source``: a scan id — the current scan is appended before its candidates are
        matched, slam.py:554 — or an (n, 2) array, which is staged behind the last scan, filtered and given its means for
        this match only and is not added.  Voxel sizes and ``normal_k`` are the history's; the other arguments are
        ``RunIcpPairBatch``'s.  ``index_base`` / ``index_stride``: the candidate number of pair b is index_base + b *
        index_stride, as there — what a form sharded over ranks (icpmi.dist) would pass; sharding itself is not built.

        ``alignment_method`` "features" / "both" need a history built with ``feat_cfg``: the cloud-side keys are the
        history's (one given here that differs is refused), the pair-side keys (``ratio_threshold``, ``ransac_iterations``,
        ``inlier_threshold``, ``min_inliers``) come from ``feat_cfg`` here over ``FEAT_DEFAULTS``; ``hypotheses`` / ``rng``
        as ``FeatureAlignBatch`` takes them.  Without a feature store only "rotation_search" is resident."""
        if alignment_method != "rotation_search" and self.store is None:
            raise ValueError(f"alignment_method {alignment_method!r} is not resident in a ScanHistory (only 'rotation_search' is): "
                             "use RunIcpPairBatch for 'features' and 'both'")
        if alignment_method not in ALIGNMENT_METHODS:
            raise ValueError(f"alignment_method must be one of {ALIGNMENT_METHODS}, got {alignment_method!r}")
        cfg = None
        if alignment_method != "rotation_search":
            cfg = dict(feat_cfg or {})
            for k in FEAT_CLOUD_KEYS:
                if k in cfg and cfg[k] != self.feat_cfg[k]:
                    raise ValueError(f"feat_cfg[{k!r}] = {cfg[k]!r} differs from the history's {self.feat_cfg[k]!r}: the resident "
                                     "features were computed with the history's")
            cfg.update(self.feat_cfg)
        cands = _scan_ids(candidates, ("candidates", "candidate ids"), self.n_scans)
        staged = not isinstance(source, (int, np.integer))
        if staged:
            arr = self._clouds([source])
            # cloud n_scans, for this match: rows_used stays.  Its own features serve "features" alone ("both" computes
            # them of the transformed copies)
            self._place(arr, self.n_scans, prepare=False, features=alignment_method == "features")
            source = self.n_scans
        else:
            source = _scan_ids(source, ("source", "source id"), self.n_scans, one=True)
        return HistoryMatch(self, int(source), cands, staged, error_threshold, max_iterations, method, max_corr_dist,
                            angle_step_coarse, angle_step_fine, max_rows_hint, error_accept, stop_after_first_accepted,
                            index_base, index_stride, alignment_method, cfg, hypotheses, rng)

    # ── world rows: transform_points_2d (slam.py:46-50) of resident scans ─────
    def world_row_args(self, poses, ids=None):
        """The host side of ``world_rows``, checked: (ids int32 [n], poses (n, 6), out offsets int32 [n + 1]).  ``ids=None``:
        every scan in order.  Only [0, len(self)) is addressable — a staged source is not a scan of the history."""
        if ids is None:
            ids = np.arange(self.n_scans, dtype=np.int32)
        else:
            ids = _scan_ids(ids, ("ids", "scan ids"), self.n_scans)
        pose6 = pose_rows(poses, len(ids))
        ends = np.cumsum(self.sizes()[ids], dtype=np.int64)
        if len(ends) and ends[-1] >= 2 ** 31:
            raise ValueError("too many rows for 32-bit row offsets: transform the list in parts")
        off = np.zeros(len(ids) + 1, dtype=np.int32)
        off[1:] = ends
        return ids, pose6, off

    def world_rows_into(self, out, ids_dev, poses_dev, off_dev, n):
        """One ``icpmi_history_world_rows`` launch on the current stream: scan ids_dev[k] under poses_dev[k] into rows
        [off_dev[k], off_dev[k + 1]) of ``out`` — device tensors as ``world_row_args`` lays them out; ``out`` holds at
        least off_dev[n] rows."""
        check(_lib.lib().icpmi_history_world_rows(C.byref(self.state), _ptr(ids_dev), n, _ptr(poses_dev), _ptr(off_dev), _ptr(out),
                                                  _stream()), "history_world_rows")

    def world_rows(self, poses, ids=None):
        """``points @ T[:2, :2].T + T[:2, 2]`` (slam.py:46-50), NumPy's result bit for bit, of scan ids[k] under poses[k] (3 x 3
        matrices, one per id; ids may repeat, in any order) -> (rows: a new (sum n, 2) float64 device tensor, offsets: host
        int32 [len(ids) + 1]).  Three small uploads and one launch; the history is not written."""
        ids, pose6, off = self.world_row_args(poses, ids)
        rows = torch.empty((int(off[-1]), 2), dtype=torch.float64, device=self.device)
        if len(ids):
            dev = [torch.from_numpy(a).to(self.device) for a in (ids, pose6, off)]
            self.world_rows_into(rows, dev[0], dev[1], dev[2], len(ids))
        return rows, off

    def icp(self, source_id, target_id, R_init=None, t_init=None, error_threshold=1e-7, max_iterations=100,
            method="point_to_line", max_corr_dist=None):
        """``ICP(scan source_id, scan target_id, ...)`` (icp.py:132-223) against the resident prepared target — the
        scan-to-scan step of slam.py:471 with the previous scan already prepared -> (R, t, err, info) like ``icp_pair``
        (synchronises)."""
        source_id, target_id = (_scan_ids(k, ("ids", "scan ids"), self.n_scans, one=True) for k in (source_id, target_id))
        b = _ResidentIcp(self, [source_id], [target_id], error_threshold, max_iterations, method, max_corr_dist, R_init, t_init)
        b.run()
        return b.unpack()
