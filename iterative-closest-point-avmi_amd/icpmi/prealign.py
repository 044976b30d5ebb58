"""Batched ``_run_icp_pair``: correlative rotation search + ICP for many scan pairs, nothing returning to the host
in between.

The reference matches its loop-closure candidates one after another (slam.py:575-579), and each match is
``_run_icp_pair`` (slam.py:53-98): ``rotation_search`` (utilities/features.py:165-242, the default pre-alignment,
config.yaml:34) and then ``ICP`` started from its result.  Here the searches of a whole batch are one chain of launches
behind ``icpmi_rotation_search_batch`` — voxel filter of every cloud at the search's own voxel size, their means, the
search order of the targets, one workgroup per pair for both sweeps — which leaves R_init / t_init of every pair in
device memory, where the batched ICP (``icpmi.batch.IcpBatch``) reads them.

The angle grids and their cos / sin are computed on the host with the reference's own NumPy expressions (cached on the
device), so the chosen angle, R and t are the reference's numbers bit for bit.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .batch import (CloudSet, IcpBatch, PairList, _Paired, _ptr, _stream, icp_pair, pack_results, pair_lists, require_gpu,
                    unpack_results)

# the records' layout, statuses and capacities are include/icpmi.h's, mirrored once in _lib; the names users import stay
REC_DOUBLES = _lib.RSBREC_DOUBLES                                # (the feature record has the same stride)
ST_OK, ST_FEW, ST_CAPACITY, ST_NO_FINE = _lib.RSB_ST_OK, _lib.RSB_ST_FEW, _lib.RSB_ST_CAPACITY, _lib.RSB_ST_NO_FINE
RSB_MAX_ANGLES = _lib.RSB_MAX_ANGLES                             # angles per sweep the batched kernel tabulates
ALIGNMENT_METHODS = ("rotation_search", "features", "both")      # slam.py:60, 68


def arange_rows(lo, hi, step):
    """``np.arange(lo[k], hi[k], step)`` for every k at once -> (values [K, L], lengths [K]); rows are padded with
    their last value.  Bit for bit NumPy's own numbers: arange takes ceil((stop - start) / step) elements and fills
    them as start + i * delta with delta = (start + step) - start."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    step = np.float64(step)
    n = np.ceil((hi - lo) / step)
    n = np.where(np.isfinite(n) & (n > 0), n, 0).astype(np.int64)
    L = int(n.max()) if len(n) else 0
    i = np.arange(L, dtype=np.float64)[None, :]
    delta = ((lo + step) - lo)[:, None]
    vals = lo[:, None] + i * delta
    if L > 1:
        vals[:, 1] = lo + step
    if L > 0:
        vals[:, 0] = lo
    last = np.clip(n - 1, 0, None)
    vals = np.where(np.arange(L)[None, :] < n[:, None], vals, vals[np.arange(len(n)), last][:, None]) if L else vals
    return vals, n


def device_angle_tables(dev, coarse, fine, fine_n):
    """cos / sin of the coarse angles [K, 2] and of every fine grid [K, L, 2] (features.py:214 uses np.cos / np.sin) and the
    grids' lengths (int32), on the device."""
    cs = np.ascontiguousarray(np.stack([np.cos(coarse), np.sin(coarse)], axis=1))
    fcs = np.ascontiguousarray(np.stack([np.cos(fine), np.sin(fine)], axis=2)) if fine.size else np.zeros((len(coarse), 0, 2))
    return (torch.from_numpy(cs).to(dev), torch.from_numpy(fcs).to(dev),
            torch.from_numpy(np.ascontiguousarray(fine_n, dtype=np.int32)).to(dev))


def winning_angle(coarse, fine, rec, coarse_without_fine=False):
    """The angle a search record names (one record, or [B, .] records -> [B] angles): entry RSREC_J of the fine grid of the
    winning coarse angle RSREC_K (features.py:231-232).  A winner whose fine grid is empty: np.argmin raises in
    rotation_search (features.py:231); with ``coarse_without_fine`` the coarse angle stands (slam.py:157-159)."""
    rec = np.asarray(rec)
    k, j = rec[..., _lib.RSREC_K].astype(np.int64), rec[..., _lib.RSREC_J].astype(np.int64)
    has_fine = rec[..., _lib.RSREC_NF] > 0
    if has_fine.all():
        return fine[k, j]
    if not coarse_without_fine:
        raise ValueError("attempt to get argmin of an empty sequence")          # np.argmin(scores_fine) on an empty grid
    return np.where(has_fine, fine[k, j], coarse[k]) if has_fine.any() else coarse[k]


class AngleTables:
    """Coarse angles of features.py:221 and, for every coarse angle that can win, the fine grid of features.py:227-229,
    with cos / sin of all of them on the device (features.py:214 uses np.cos / np.sin).  One per (device, steps)."""
    _cache = {}

    @classmethod
    def get(cls, dev, angle_step_coarse, angle_step_fine):
        key = (dev, float(angle_step_coarse), float(angle_step_fine))
        if key not in cls._cache:
            cls._cache[key] = cls(dev, angle_step_coarse, angle_step_fine)
        return cls._cache[key]

    def __init__(self, dev, angle_step_coarse, angle_step_fine):
        self.coarse = np.deg2rad(np.arange(-180, 180, angle_step_coarse))            # features.py:221
        lo = self.coarse - np.deg2rad(angle_step_coarse)                             # features.py:227-229, for every possible winner
        hi = self.coarse + np.deg2rad(angle_step_coarse)
        self.fine, self.fine_n = arange_rows(lo, hi, np.deg2rad(angle_step_fine))
        self.max_fine = int(self.fine.shape[1]) if self.fine.ndim == 2 else 0
        self.d_cs, self.d_fcs, self.d_fn = device_angle_tables(dev, self.coarse, self.fine, self.fine_n)

    @property
    def device_table(self):
        return self.d_cs, self.d_fcs, self.d_fn


class RotationSearchBatch(_Paired):
    """rotation_search (features.py:165-242) of every pair of a cloud set, resident on the device.

    ``run()`` enqueues the chain on the current stream and returns the (B, 16) record tensor; ``init`` ([B, 6]: R row
    major, t) then holds R_init / t_init of every pair for ``icpmi_icp_batch``.  ``results()`` reads the records back
    and forms (R, t, score) with the reference's NumPy expressions (features.py:235-237)."""

    def __init__(self, clouds, pair_src, pair_tgt, voxel_size=0.3, angle_step_coarse=2.0, angle_step_fine=0.2,
                 init=None, max_rows_hint=0):
        require_gpu()
        raw = clouds if isinstance(clouds, CloudSet) else CloudSet.from_numpy(clouds)
        self._init_common(raw, pair_src, pair_tgt, voxel_size, angle_step_coarse, angle_step_fine, init, max_rows_hint)
        dev = raw.pts.device
        self.tgt_ids = torch.from_numpy(np.unique(self.pair_tgt_host).astype(np.int32)).to(dev)
        need = _lib.lib().icpmi_rotation_search_batch_workspace_bytes(raw.total_rows, raw.n_clouds, raw.max_n)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)

    def _init_common(self, raw, pair_src, pair_tgt, voxel_size, angle_step_coarse, angle_step_fine, init, max_rows_hint):
        """What every variant needs: the pairs, the angle tables, the records and where the starts go.  The filtered
        clouds and their search order are the workspace's (a resident variant: a history's)."""
        if raw.dim != 2:
            raise ValueError("rotation_search is 2-D")
        if not voxel_size > 0:
            raise ValueError("voxel_size must be positive")
        dev = raw.pts.device
        self.raw, self.voxel_size = raw, float(voxel_size)
        self.pairs = PairList.of(pair_src, pair_tgt).to(dev)
        self.steps = (angle_step_coarse, angle_step_fine)
        self.tables = AngleTables.get(dev, angle_step_coarse, angle_step_fine)
        self.max_rows_hint = int(max_rows_hint)
        self.too_many_angles = len(self.tables.coarse) > RSB_MAX_ANGLES or self.tables.max_fine > RSB_MAX_ANGLES
        self.records = torch.zeros((max(self.B, 1), REC_DOUBLES), dtype=torch.float64, device=dev)
        self.init = init if init is not None else torch.zeros((max(self.B, 1), 6), dtype=torch.float64, device=dev)

    def mark_over_capacity(self):
        """More angles than the batched kernel tabulates (a step below ~0.36 degrees; icpmi_rotation_search_batch would
        answer ICPMI_ERR_UNSUPPORTED): every record becomes ST_CAPACITY, and such pairs are searched one by one through
        the single-pair entry when the results are read — same numbers."""
        self.records.zero_()
        self.records[:, _lib.RSBREC_STATUS] = ST_CAPACITY
        return self.records

    def run(self):
        if self.too_many_angles:
            return self.mark_over_capacity()
        t = self.tables
        mf = t.max_fine
        check(_lib.lib().icpmi_rotation_search_batch(
            _ptr(self.raw.pts), _ptr(self.raw.off), self.raw.off_host.ctypes.data_as(C.c_void_p), self.raw.n_clouds,
            _ptr(self.tgt_ids), len(self.tgt_ids), _ptr(self.pair_src), _ptr(self.pair_tgt), self.B, self.voxel_size,
            _ptr(t.d_cs), len(t.coarse), _ptr(t.d_fcs) if mf else None, _ptr(t.d_fn) if mf else None, mf,
            self.max_rows_hint, _ptr(self.records), _ptr(self.init), _ptr(self.ws), self.ws.numel(), _stream()),
            "rotation_search (batch)")
        return self.records

    def host_records(self, records=None):
        """The records of the last run on the host (synchronises); raises as np.argmin(scores_fine) does in the reference
        (features.py:231) when a winning coarse angle has an empty fine grid."""
        rec = (self.records if records is None else records).cpu().numpy()[:self.B]
        if (rec[:, _lib.RSBREC_STATUS].astype(np.int64) == ST_NO_FINE).any():
            raise ValueError("attempt to get argmin of an empty sequence")
        return rec

    def results(self, records=None):
        """-> (R [B,2,2], t [B,2], score [B], records [B,16]) on the host (synchronises).  Pairs the on-chip search could
        not hold (ST_CAPACITY: a filtered cloud above the capacity hint) are searched one by one through the single-pair
        entry — same numbers."""
        rec = self.host_records(records)
        t = self.tables
        R = np.tile(np.eye(2), (self.B, 1, 1))
        tt = np.zeros((self.B, 2))
        score = np.full(self.B, np.inf)
        status = rec[:, _lib.RSBREC_STATUS].astype(np.int64)
        ok = np.flatnonzero(status == ST_OK)
        if len(ok):
            ang = winning_angle(t.coarse, t.fine, rec[ok])
            ca, sa = np.cos(ang), np.sin(ang)
            mu_s, mu_t = rec[:, _lib.RSREC_MUS:_lib.RSREC_MUS + 2], rec[:, _lib.RSREC_MUT:_lib.RSREC_MUT + 2]
            for q, i in enumerate(ok):                                              # features.py:235-237, NumPy's own matmul
                Ri = np.array([[ca[q], -sa[q]], [sa[q], ca[q]]])
                R[i] = Ri
                tt[i] = mu_t[i] - Ri @ mu_s[i]
            score[ok] = rec[ok, _lib.RSREC_FSCORE]
        over = np.flatnonzero(status == ST_CAPACITY)
        if len(over):
            from utilities import features
            clouds = self.raw.to_numpy()
            keep = features.VERBOSE
            features.VERBOSE = False
            try:
                for i in over:
                    R[i], tt[i], score[i] = features.rotation_search(
                        clouds[self.pair_src_host[i]], clouds[self.pair_tgt_host[i]], self.voxel_size, *self.steps)
            finally:
                features.VERBOSE = keep
        return R, tt, score, rec

FEAT_ST_OK, FEAT_ST_FEW_ROWS, FEAT_ST_CAPACITY, FEAT_ST_FEW_KP, FEAT_ST_FEW_MATCHES, FEAT_ST_DESC_LEN = (
    _lib.FT_ST_OK, _lib.FT_ST_FEW_ROWS, _lib.FT_ST_CAPACITY, _lib.FT_ST_FEW_KP, _lib.FT_ST_FEW_MATCHES, _lib.FT_ST_DESC_LEN)
FEAT_DEFAULTS = dict(voxel_size=0.2, k_curvature=10, top_n=100, min_kp_dist=0.3, k_descriptor=30, ratio_threshold=0.8,
                     ransac_iterations=1000, inlier_threshold=0.5, min_inliers=3)            # slam.py:72-83
# the keys a cloud's own tables depend on (what a resident history computes once per scan); the others are per pair
FEAT_CLOUD_KEYS = ("voxel_size", "k_curvature", "top_n", "min_kp_dist", "k_descriptor")


class FeatureAlignBatch(_Paired):
    """feature_based_alignment (features.py:247-315) of every pair of a cloud set, resident on the device.

    ``run()`` enqueues the chain of ``icpmi_feature_align_batch`` on the current stream — voxel filter at the feature voxel
    size, curvature, keypoints, descriptors, matching, RANSAC — and returns the (B, 16) record tensor (include/icpmi.h).
    ``init_in`` ([B, 6] device tensor: R row major, t): the start every source is transformed by first (slam.py:69-71);
    ``init_out`` then receives the start of the ICP that follows (slam.py:83-88) and may be the same tensor.

    The candidate order of the keypoints is the device's rule (descending curvature, ties by ascending row): the
    reference's order among equal curvatures is an accident of NumPy's unstable sort, which a batch cannot reproduce.
    The RANSAC hypotheses are an input, one table for every pair: ``hypotheses`` ((n_iter, 2) integers, used as they are;
    a row that names a match the pair does not have counts no inliers) or ``rng`` (a ``numpy.random.Generator``): the match
    count of a pair is only known on the device, so ``rng.random((n_iter, 2))`` is drawn once and the kernel maps a row
    (u0, u1) to the matches i = floor(u0 * n), j = floor(u1 * (n - 1)), j += (j >= i) — two distinct matches, every
    pair of them equally likely, as ``np.random.choice(n, 2, replace=False)`` gives.  Neither: ``rng`` seeded with 0.

    A pair the kernels could not align — FEAT_ST_CAPACITY, a filtered cloud above the 2 048 rows they hold on chip, or
    FEAT_ST_DESC_LEN, descriptors of different lengths (NumPy raises there in the reference) — has no feature start:
    identity, zeros, 0 inliers in its record and ``init_out`` left as ``init_in``, as for the reference's own early returns;
    the status in slot ``_lib.FTREC_STATUS`` says which."""

    def __init__(self, clouds, pair_src, pair_tgt, feat_cfg=None, hypotheses=None, rng=None, init_in=None, init_out=None, like=None):
        require_gpu()
        raw = clouds if isinstance(clouds, CloudSet) else CloudSet.from_numpy(clouds)
        self._init_common(raw, pair_src, pair_tgt, feat_cfg, hypotheses, rng, init_in, init_out, like)
        need = _lib.lib().icpmi_feature_align_batch_workspace_bytes(raw.total_rows, raw.n_clouds, raw.max_n, self.B,
                                                                    int(self.cfg["top_n"]), 1 if init_in is not None else 0)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=raw.pts.device)

    def _init_common(self, raw, pair_src, pair_tgt, feat_cfg, hypotheses, rng, init_in, init_out, like=None):
        """What every variant needs: the configuration, the pairs, the hypothesis table, the records and where the starts
        come from and go.  The per-cloud tables are the workspace's (a resident variant: a history's feature store)."""
        if raw.dim != 2:
            raise ValueError("feature_based_alignment is 2-D")
        self.raw = raw
        dev = raw.pts.device
        cfg = dict(FEAT_DEFAULTS)
        cfg.update({k: v for k, v in (feat_cfg or {}).items() if k in FEAT_DEFAULTS})
        self.cfg = cfg
        if not cfg["voxel_size"] > 0:
            raise ValueError("voxel_size must be positive")
        self.pairs = PairList.of(pair_src, pair_tgt).to(dev)
        self.n_iter = int(cfg["ransac_iterations"])
        self.hyp_idx = self.hyp_u = None
        if like is not None:                               # another batch's hypothesis table (a pair redone on its own)
            self.n_iter, self.hyp_idx, self.hyp_u = like.n_iter, like.hyp_idx, like.hyp_u
        elif hypotheses is not None:
            h = np.ascontiguousarray(hypotheses, dtype=np.int32)
            if h.shape != (self.n_iter, 2):
                raise ValueError(f"hypotheses must have shape ({self.n_iter}, 2), got {h.shape}")
            self.hyp_idx = torch.from_numpy(h).to(dev) if self.n_iter else None
        elif self.n_iter:
            rng = rng if rng is not None else np.random.default_rng(0)
            self.hyp_u = torch.from_numpy(rng.random((self.n_iter, 2))).to(dev)
        self.init_in, self.init_out = init_in, init_out
        self.records = torch.zeros((max(self.B, 1), _lib.FTREC_DOUBLES), dtype=torch.float64, device=dev)

    def run(self):
        c = self.cfg
        check(_lib.lib().icpmi_feature_align_batch(
            _ptr(self.raw.pts), _ptr(self.raw.off), self.raw.off_host.ctypes.data_as(C.c_void_p), self.raw.n_clouds,
            _ptr(self.pair_src), self.pair_src_host.ctypes.data_as(C.c_void_p), _ptr(self.pair_tgt), self.B,
            float(c["voxel_size"]), int(c["k_curvature"]), int(c["top_n"]), float(c["min_kp_dist"]), int(c["k_descriptor"]),
            float(c["ratio_threshold"] ** 2), _ptr(self.hyp_idx), _ptr(self.hyp_u), self.n_iter, 0, float(c["inlier_threshold"]),
            int(c["min_inliers"]), _ptr(self.init_in), _ptr(self.init_out), _ptr(self.records), _ptr(self.ws), self.ws.numel(),
            _stream()), "feature_based_alignment (batch)")
        return self.records

    def results(self, records=None):
        """-> (R [B,2,2], t [B,2], n_inliers [B], records [B,16]) on the host (synchronises); slot ``_lib.FTREC_STATUS`` of a
        record is the status."""
        rec = (self.records if records is None else records).cpu().numpy()[:self.B]
        R, t = rec[:, _lib.FTREC_R:_lib.FTREC_R + 4], rec[:, _lib.FTREC_T:_lib.FTREC_T + 2]
        return R.reshape(-1, 2, 2).copy(), t.copy(), rec[:, _lib.FTREC_INLIERS].astype(np.int64), rec


def rotation_search_batch(sources, targets, voxel_size=0.3, angle_step_coarse=2.0, angle_step_fine=0.2):
    """rotation_search(sources[i], targets[i]) for every i in one chain of launches -> (R [B,2,2], t [B,2], score [B]).
    ``sources`` may be one array shared by every pair (the loop-closure shape, slam.py:576-579)."""
    clouds, ps, pt = pair_lists(sources, targets)
    b = RotationSearchBatch(clouds, ps, pt, voxel_size, angle_step_coarse, angle_step_fine)
    b.run()
    R, t, score, _ = b.results()
    return R, t, score


def _gate_given(stop_after_first_accepted, error_accept):
    if stop_after_first_accepted and error_accept is None:
        raise ValueError("stop_after_first_accepted needs a gate: error_accept")


class RunIcpPairBatch(_Paired):
    """``_run_icp_pair`` (slam.py:53-98) for a batch of pairs resident in HBM: ``run()`` = the pre-alignment of every pair
    — rotation search (``alignment_method`` "rotation_search", the default), feature alignment ("features") or the search
    followed by the feature alignment from its result ("both") — then ICP of every pair from its own R_init / t_init:
    one stream, no host round trip; returns the (B, 16) ICP result tensor (icpmi.batch.unpack_results).  With a feature
    alignment, ``unpack()`` adds ``info["feature_records"]`` (FeatureAlignBatch; slot FTREC_STATUS: status — a pair the feature
    kernels could not align simply has no feature start).

    The pairs are loop-closure candidates in the caller's order.  ``error_accept``: the gate of slam.py:582-597 (the first
    candidate with err < error_accept is taken); ``unpack()`` then reports it as ``info["first_accepted"]``.  With
    ``stop_after_first_accepted`` the candidates after it may stop early, as the reference never computes them
    (icpmi_icp_batch_gated): their status is ST_SKIPPED (5); every candidate up to the accepted one is the full run's
    bit for bit.  ``index_base`` / ``index_stride``: the candidate number of pair b is index_base + b * index_stride
    (a rank of a sharded run, icpmi.dist)."""

    def __init__(self, clouds, pair_src, pair_tgt, error_threshold=1e-7, max_iterations=100, voxel_size=0.06,
                 method="point_to_line", normal_k=10, rotation_voxel_size=0.3, angle_step_coarse=2.0, angle_step_fine=0.2,
                 max_corr_dist=None, max_rows_hint=0, stop_after_first_accepted=False, error_accept=None,
                 index_base=0, index_stride=1, alignment_method="rotation_search", feat_cfg=None, hypotheses=None, rng=None):
        if alignment_method not in ALIGNMENT_METHODS:
            raise ValueError(f"alignment_method must be one of {ALIGNMENT_METHODS}, got {alignment_method!r}")
        _gate_given(stop_after_first_accepted, error_accept)
        raw = clouds if isinstance(clouds, CloudSet) else CloudSet.from_numpy(clouds)
        pairs = PairList.of(pair_src, pair_tgt)                 # one pair list, uploaded once, for every part
        B = pairs.B
        icp = IcpBatch(raw, pairs, None, error_threshold, max_iterations, voxel_size,
                       np.tile(np.eye(2), (B, 1, 1)), np.zeros((B, 2)), method, normal_k, max_corr_dist)
        search = features = None
        if alignment_method in ("rotation_search", "both"):                         # slam.py:60
            search = RotationSearchBatch(raw, pairs, None, rotation_voxel_size, angle_step_coarse, angle_step_fine,
                                         init=icp.init, max_rows_hint=max_rows_hint)
        # slam.py:68-88: the feature alignment starts from the search's result ("both") or from the raw source, and leaves
        # the start of the ICP where the search would have: in the ICP's own init tensor
        if alignment_method in ("features", "both"):
            features = FeatureAlignBatch(raw, pairs, None, feat_cfg, hypotheses, rng,
                                         init_in=icp.init if search is not None else None, init_out=icp.init)
        self._init_parts(alignment_method, icp, search, features, error_accept, stop_after_first_accepted, index_base,
                         index_stride, max_rows_hint, raw.max_n)

    def _init_parts(self, alignment_method, icp, search, features, error_accept, stop_after_first_accepted, index_base,
                    index_stride, max_rows_hint, max_raw_n):
        """The job over parts already built — ``icp``, ``search`` (None: no search) and ``features`` (None: none) over one
        pair list, the search writing its starts into ``icp.init`` — and the gate of slam.py:582-597 over them
        (max_raw_n: rows of the largest raw cloud of a pair)."""
        self.icp, self.search, self.features = icp, search, features
        self.pairs = icp.pairs
        self.alignment_method, self.use_search = alignment_method, search is not None
        self.error_accept = None if error_accept is None else float(error_accept)
        self.stop = bool(stop_after_first_accepted)
        self.index_base, self.index_stride = int(index_base), int(index_stride)
        if self.stop:
            self.icp.set_gate(self.error_accept, self.search.records if self.use_search else None, self.index_base, self.index_stride)
        # a pair can fall outside the on-chip search (ST_CAPACITY) only with a capacity hint, a raw cloud above the rows the
        # search holds or more angles than it tabulates: only then may first_accepted() need the host
        self.capacity_possible = self.use_search and (self.search.too_many_angles or max_rows_hint > 0 or
                                                      max_raw_n > _lib.RSB_MAX_ROWS)

    def run(self, events=None):
        if not self.use_search:                            # "features": no search
            self.features.run()
            return self.icp.run(events=events)
        if self.search.too_many_angles:
            self.search.mark_over_capacity()
            if self.stop:
                self.icp.first_accepted_dev.fill_(-1)  # no candidate ran on the device: unpack() redoes them in order
            if events is not None:
                events[0].record(); events[1].record()
            return self.icp.results
        self.search.run()
        if self.features is not None:
            self.features.run()
        return self.icp.run(events=events)

    def information(self, pairs=None):
        """``IcpBatch.information`` of the ICP part: the information records of the pairs ``pairs`` (indices b into the pair
        list — the pair of candidate number c is b = (c - index_base) / index_stride; None: all) at the transforms of the last ``run()`` -> a
        device (len(pairs), 16) tensor.  Typically asked for the ``first_accepted()`` pair alone.  A record with status
        ST_SKIPPED is answered at the transform it holds (the steps the candidate had applied when it stopped), and a pair
        ``unpack()`` redoes on the host (search status 2) at the device's, not the redone, transform."""
        return self.icp.information(pairs)

    def first_accepted(self):
        """Index (in candidate numbers) of the candidate slam.py:582-597 accepts after the last gated ``run()``, -1 when
        none: a 4-byte read of the device's answer — unless a candidate fell outside the on-chip search (status 2), which
        only ``unpack()`` can settle (it redoes such candidates on the host)."""
        if not self.stop:
            raise ValueError("first_accepted() needs stop_after_first_accepted=True")
        first = int(self.icp.first_accepted_dev.item())
        if self.capacity_possible:
            st = self.search.records[:self.B, _lib.RSBREC_STATUS]
            lim = self.B if first < 0 else (first - self.index_base) // self.index_stride
            if bool((st[:lim] == ST_CAPACITY).any()) or bool((st == ST_NO_FINE).any()):
                return self.unpack()[3]["first_accepted"]
        return first

    def _redo(self, i, R0, t0, clouds):
        """The ICP of pair i through the single-pair entry, from the single-pair search's start — with "both", carried on
        by the pair's own feature alignment (same configuration, same hypothesis table) -> its 16-double record."""
        p = self.icp.params
        Rs, ts = R0[i], t0[i]
        if self.features is not None:
            start = torch.from_numpy(np.concatenate([Rs.reshape(4), ts])[None, :].copy()).to(self.icp.results.device)
            one = FeatureAlignBatch([clouds[self.icp.pair_src_host[i]], clouds[self.icp.pair_tgt_host[i]]], [0], [1],
                                    self.features.cfg, init_in=start, init_out=start, like=self.features)
            self.redone_feature_records[int(i)] = one.run().cpu().numpy()[0]
            v = start.cpu().numpy()[0]
            Rs, ts = v[:4].reshape(2, 2), v[4:]
        return pack_results(*icp_pair(clouds[self.icp.pair_src_host[i]], clouds[self.icp.pair_tgt_host[i]],
                                      p.error_threshold, p.max_iterations, self.icp.voxel_size, Rs, ts,
                                      "point_to_line" if self.icp.use_p2l else "point_to_point", self.icp.normal_k,
                                      None if p.max_corr_dist < 0 else p.max_corr_dist))[0]

    def unpack(self):
        """(R, t, err, info) of the ICPs; pairs whose search fell outside the on-chip capacity (status 2) are redone
        with the single-pair search's result as their start (and, with "both", their own feature alignment from it).  With a gate, info["first_accepted"] is the candidate
        slam.py:582-597 accepts (-1: none); with stop_after_first_accepted, a status-2 candidate after it is not redone
        but reported SKIPPED (identity, err inf, 0 iterations), and info["status"] is 5 for every skipped candidate."""
        rec = self.search.host_records() if self.use_search else np.zeros((self.B, REC_DOUBLES))
        res = self.icp.results.cpu().numpy()[:self.B].copy()
        self.redone_feature_records = {}
        over = np.flatnonzero(rec[:, _lib.RSBREC_STATUS].astype(np.int64) == ST_CAPACITY)
        first = -1
        if self.stop:
            # the device's answer never counts a status-2 candidate (its device ICP started from the wrong pose): the
            # ones before it are redone in order, and the first of them that is accepted comes first
            first = int(self.icp.first_accepted_dev.item())
        if len(over):
            R0, t0, _, _ = self.search.results()
            clouds = self.search.raw.to_numpy()
            for i in over:
                idx = self.index_base + int(i) * self.index_stride
                if self.stop and 0 <= first < idx:
                    res[i, :] = 0.0
                    res[i, _lib.RES_R] = res[i, _lib.RES_R + 3] = 1.0
                    res[i, _lib.RES_ERR] = res[i, _lib.RES_DELTA] = np.inf
                    res[i, _lib.RES_STATUS] = _lib.ST_SKIPPED
                    continue
                res[i, :] = self._redo(i, R0, t0, clouds)
                if self.stop and res[i, _lib.RES_ERR] < self.error_accept:
                    first = idx
        R, t, err, info = unpack_results(res, 2)
        if self.features is not None:
            info["feature_records"] = self.features.records.cpu().numpy()[:self.B].copy()
            for i, r in self.redone_feature_records.items():
                info["feature_records"][i] = r
        if self.error_accept is not None:
            if not self.stop:                                                  # the full run: first in order below the gate
                ok = np.flatnonzero(err < self.error_accept)
                first = self.index_base + int(ok[0]) * self.index_stride if len(ok) else -1
            info["first_accepted"] = first
        return R, t, err, info


def run_icp_pair_batch(sources, targets, icp_cfg=None, feat_cfg=None, error_accept=None, stop_after_first_accepted=False,
                       alignment_method="rotation_search", hypotheses=None, rng=None):
    """``_run_icp_pair(sources[i], targets[i], icp_cfg, feat_cfg, alignment_method)`` for every i (slam.py:53-98, same
    configuration keys and defaults) -> (R [B,2,2], t [B,2], err [B], info).  With ``error_accept``,
    ``info["first_accepted"]`` is the candidate slam.py:582-597 accepts (-1: none); ``stop_after_first_accepted`` lets
    the candidates after it stop early (status 5, RunIcpPairBatch).  ``alignment_method``: "rotation_search" (the
    default: exactly the launches of before), "features" or "both" (FeatureAlignBatch, with its ``hypotheses`` / ``rng``;
    ``info["feature_records"]`` then holds its records)."""
    icp_cfg, feat_cfg = icp_cfg or {}, feat_cfg or {}
    clouds, ps, pt = pair_lists(sources, targets)
    b = RunIcpPairBatch(clouds, ps, pt,
                        error_threshold=icp_cfg.get("error_threshold", 1e-7), max_iterations=icp_cfg.get("max_iterations", 100),
                        voxel_size=icp_cfg.get("voxel_size", 0.06), method=icp_cfg.get("method", "point_to_line"),
                        normal_k=icp_cfg.get("normal_k", 10), rotation_voxel_size=feat_cfg.get("rotation_voxel_size", 0.3),
                        angle_step_coarse=feat_cfg.get("angle_step_coarse", 2.0), angle_step_fine=feat_cfg.get("angle_step_fine", 0.2),
                        stop_after_first_accepted=stop_after_first_accepted, error_accept=error_accept,
                        alignment_method=alignment_method, feat_cfg=feat_cfg, hypotheses=hypotheses, rng=rng)
    b.run()
    return b.unpack()
