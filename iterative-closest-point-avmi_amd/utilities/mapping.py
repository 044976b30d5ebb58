"""utilities.mapping — ``OccupancyGrid2D`` with the reference's interface
(/root/reference/utilities/mapping.py), the grid living in MI355X HBM.

``update_scan`` runs the Bresenham ray-cast and the log-odds update as two HIP
kernels (integer hit/miss counts per cell, then an exact replay of the
reference's float32(float64 + l) adds and the per-scan clip), so cell indices
and cell values are bit-identical to the NumPy implementation.
"""
import ctypes as C

import math

import numpy as np
import torch

from icpmi import _lib
from icpmi import batch as _b

UNEXPLORED = 0.0   # log-odds 0 = probability 0.5 (mapping.py:10)


class OccupancyGrid2D:
    """2-D log-odds occupancy grid; layout ``log_odds[iy, ix]``, shape (ny, nx), float32."""

    def __init__(self, min_x, max_x, min_y, max_y, resolution=0.1, p_hit=0.7, p_miss=0.4,
                 log_odds_min=-5.0, log_odds_max=5.0):
        _b.require_gpu()
        self.min_x, self.max_x = float(min_x), float(max_x)
        self.min_y, self.max_y = float(min_y), float(max_y)
        self.resolution = float(resolution)
        self.nx = int(np.ceil((self.max_x - self.min_x) / self.resolution))     # mapping.py:44-45
        self.ny = int(np.ceil((self.max_y - self.min_y) / self.resolution))
        if self.nx <= 0 or self.ny <= 0:
            raise ValueError("empty grid")
        self.l_hit = np.log(p_hit / (1.0 - p_hit))                                # np.float64, mapping.py:49-50
        self.l_miss = np.log(p_miss / (1.0 - p_miss))
        self.log_odds_min = float(log_odds_min)
        self.log_odds_max = float(log_odds_max)
        self._dev = torch.device("cuda", torch.cuda.current_device())
        self._grid = torch.zeros((self.ny, self.nx), dtype=torch.float32, device=self._dev)
        self._ws = None                    # counter workspace (four grids of uint32): allocated by the first update
        self._seq = 0                      # non-empty scans applied so far (selects counter grid / box slot)
        self._host = None                  # cached host copy of the grid
        self._full_clip = not (self.log_odds_min <= 0.0 <= self.log_odds_max)
        self._stages = None                # pinned staging rows of update_scan (NumPy in)
        self._call = None                  # converted constant arguments of the update call (see _apply)
        self._replay_scratch = None        # world rows of one piece of replay_history
        self.cell_updates = 0              # not tracked on the device; see update_scans()

    # ── the grid as the reference exposes it ─────────────────────────────────
    @property
    def log_odds(self):
        """READ-ONLY host copy (ny, nx) float32 of the device grid.

        The reference's attribute is the live array; here the live grid is in HBM, so an in-place edit of
        this copy (``grid.log_odds[...] = x``, ``np.clip(..., out=grid.log_odds)``) could not reach it and
        raises instead of being silently lost.  ASSIGN an array (``grid.log_odds = a``) to upload one."""
        if self._host is None:
            self._host = self._grid.cpu().numpy()
            self._host.setflags(write=False)
        return self._host

    @log_odds.setter
    def log_odds(self, value):
        v = np.ascontiguousarray(value, dtype=np.float32)
        if v.shape != (self.ny, self.nx):
            raise ValueError(f"log_odds must have shape {(self.ny, self.nx)}")
        self._grid.copy_(torch.from_numpy(v))
        self._host = None
        self._full_clip = True             # arbitrary values: the next scan clips every cell like np.clip does

    @property
    def device_log_odds(self):
        """The float32 (ny, nx) torch tensor in HBM (no copy)."""
        return self._grid

    # ── coordinate helpers, mapping.py:57-63,94-98 ───────────────────────────
    def _world_to_grid(self, wx, wy):
        ix = int(np.floor((wx - self.min_x) / self.resolution))
        iy = int(np.floor((wy - self.min_y) / self.resolution))
        return ix, iy

    def _in_bounds(self, ix, iy):
        return 0 <= ix < self.nx and 0 <= iy < self.ny

    def _world_to_grid_batch(self, wx, wy):
        L = _lib.lib()
        out = []
        for w, mn in ((wx, self.min_x), (wy, self.min_y)):
            w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(self._dev)
            o = torch.empty(max(w.numel(), 1), dtype=torch.int64, device=self._dev)
            _lib.check(L.icpmi_world_to_grid(_b._ptr(w), w.numel(), mn, self.resolution, _b._ptr(o), _b._stream()),
                       "_world_to_grid_batch")
            out.append(o[:w.numel()].cpu().numpy())
        return out[0], out[1]

    @staticmethod
    def _bresenham(x0, y0, x1, y1):
        """Cells from (x0,y0) towards (x1,y1), end point excluded — mapping.py:68-89 — as a list of tuples."""
        cells = bresenham_cells(np.array([[x0, y0, x1, y1]], dtype=np.int64))[0]
        return [(int(x), int(y)) for x, y in cells]

    # ── update, mapping.py:103-141 ───────────────────────────────────────────
    def update_scan(self, origin_xy, hit_points):
        """Trace a ray from ``origin_xy`` (2,) to every row of ``hit_points`` (N, 2), world frame."""
        if isinstance(hit_points, torch.Tensor):
            if hit_points.numel() == 0:
                return
            self.update_scans(torch.as_tensor(origin_xy, dtype=torch.float64).reshape(1, 2), [hit_points])
            return
        hit_points = np.asarray(hit_points, dtype=np.float64)
        if hit_points.size == 0:                                   # mapping.py:113-114
            return
        if hit_points.ndim != 2 or hit_points.shape[1] != 2:
            raise ValueError("hit_points must have shape (N, 2)")
        # the call slam.py:557 makes once per scan: origin and hits go up in ONE asynchronous copy from a pinned buffer
        # (two buffers in turn: the previous call's copy may still be in flight), the cell box comes from the host rows
        n = hit_points.shape[0]
        st = self._stage(n + 1)
        h = st[0].numpy()
        h[0] = np.asarray(origin_xy, dtype=np.float64).reshape(2)
        h[1:n + 1] = hit_points
        st[1][:n + 1].copy_(st[0][:n + 1], non_blocking=True)
        st[2].record()
        rows = h[:n + 1]
        self._off1[1] = n
        self._apply(st[1][:1], st[1][1:n + 1], self._off1, None, self._box_of(*_minmax_rows(rows)))

    def _stage(self, rows):
        """(pinned host rows, device rows, event of the last copy out of the host rows) — two sets used in turn."""
        if self._stages is None or self._stages[0][0].shape[0] < rows:
            cap = max(4096, 2 * rows)
            self._stages = [(torch.empty((cap, 2), dtype=torch.float64).pin_memory(),
                             torch.empty((cap, 2), dtype=torch.float64, device=self._dev), torch.cuda.Event()) for _ in range(2)]
            self._stage_i = 0
            self._off1 = np.zeros(2, dtype=np.int32)
        self._stage_i ^= 1
        st = self._stages[self._stage_i]
        st[2].synchronize()                                        # its previous upload has left the pinned rows
        return st

    def update_scans(self, origins, hits, rows=None):
        """Apply several scans in order (the replay of slam.py:271-277) without returning to the host.

        origins: (S, 2); hits: list of S arrays (N_s, 2) or one packed (sum N_s, 2)
        torch tensor with ``hit_offsets``-style list semantics.
        rows=(begin, end): write only that band of grid rows — one rank's share of a sharded
        replay (``icpmi.dist.replay_scans_sharded``); every other row is left untouched.
        """
        L = _lib.lib()
        S = len(hits)
        if S == 0:
            return
        if isinstance(origins, torch.Tensor):
            org = origins.to(self._dev, torch.float64).contiguous()
        else:
            org = torch.from_numpy(np.ascontiguousarray(origins, dtype=np.float64).reshape(S, 2)).to(self._dev)
        sizes = [int(h.shape[0]) for h in hits]
        off = np.zeros(S + 1, dtype=np.int32)
        np.cumsum(sizes, out=off[1:])
        box = None
        if all(isinstance(h, torch.Tensor) for h in hits):
            packed = torch.cat([h.to(self._dev, torch.float64).reshape(-1, 2) for h in hits]) if off[-1] else None
        else:
            host = np.concatenate([np.asarray(h, dtype=np.float64).reshape(-1, 2) for h in hits]) if off[-1] else None
            packed = torch.from_numpy(np.ascontiguousarray(host)).to(self._dev) if host is not None else None
            if host is not None and not isinstance(origins, torch.Tensor):       # everything is on the host: no read-back
                o_host = np.asarray(origins, dtype=np.float64).reshape(S, 2)
                both = np.vstack([o_host, host])
                box = self._box_of(*_minmax_rows(both))
                # A long trajectory in one call: the box of all scans is far larger than any scan's reach, and the tile
                # pass of the library enumerates the tiles of the box per scan.  Consecutive scans lie close together, so
                # the replay goes down in pieces of _REPLAY_PIECE scans, each with its own box (same order, same result).
                if box is not None and S > self._REPLAY_PIECE and self._box_tiles(box) > 64:
                    for c0 in range(0, S, self._REPLAY_PIECE):
                        c1 = min(S, c0 + self._REPLAY_PIECE)
                        if off[c1] == off[c0]:
                            continue
                        piece = np.vstack([o_host[c0:c1], host[off[c0]:off[c1]]])
                        self._apply(org[c0:c1], packed[off[c0]:off[c1]], off[c0:c1 + 1] - off[c0], rows,
                                    self._box_of(*_minmax_rows(piece)))
                    return
        self._apply(org, packed, off, rows, box)

    _REPLAY_PIECE = 64

    def replay_history(self, history, poses, ids=None, rows=None):
        """``update_scans`` of scans resident in an ``icpmi.ScanHistory``, by id: scan ids[k] (``None``: every scan in
        order) at poses[k] (3 x 3 matrices).  Origins are the poses' translations, hits the scans' world rows — transformed
        on the device (``icpmi_history_world_rows``: NumPy's ``pts @ T[:2, :2].T + T[:2, 2]`` bit for bit), so the cells are
        those of the host replay and nothing but ids, poses and offsets is uploaded.  ``rows`` as in ``update_scans``.

        Pieces of ``_REPLAY_PIECE`` scans as there, each one transform launch into a scratch of the largest piece's size
        (reused: everything runs on one stream) and one ``_apply``; a piece's cell box comes from the host
        (``reach_cell_box``), with no read-back."""
        self._replay(self._replay_args(history, poses, ids), rows)

    def _replay_args(self, history, poses, ids):
        if history.device != self._dev:
            raise ValueError(f"the history lives on {history.device}, the grid on {self._dev}")
        return (history,) + history.world_row_args(poses, ids)

    def _replay(self, args, rows):
        history, ids, pose6, off = args
        S = len(ids)
        if S == 0:
            return
        org = torch.from_numpy(np.ascontiguousarray(pose6[:, 4:6])).to(self._dev)
        if off[-1] == 0:                                           # no beam at all: what update_scans does with that
            self._apply(org, None, off, rows, None)
            return
        P = self._REPLAY_PIECE
        starts = range(0, S, P)
        piece_off = [off[c0:min(S, c0 + P) + 1] - off[c0] for c0 in starts]       # each piece's offsets into the scratch
        need = max(int(o[-1]) for o in piece_off)
        if self._replay_scratch is None or self._replay_scratch.shape[0] < need:
            self._replay_scratch = torch.empty((need, 2), dtype=torch.float64, device=self._dev)
        scratch = self._replay_scratch
        ids_d, pose_d = torch.from_numpy(ids).to(self._dev), torch.from_numpy(pose6).to(self._dev)
        off_d = torch.from_numpy(np.concatenate(piece_off)).to(self._dev)
        reach = history.reach[ids]
        at = 0
        for c0, o in zip(starts, piece_off):
            k = len(o) - 1
            if o[-1] > 0:
                history.world_rows_into(scratch, ids_d[c0:c0 + k], pose_d[c0:c0 + k], off_d[at:at + k + 1], k)
                self._apply(org[c0:c0 + k], scratch[:int(o[-1])], o, rows,
                            reach_cell_box(self, pose6[c0:c0 + k], reach[c0:c0 + k]))
            at += k + 1

    def rebuild_from_history(self, history, poses):
        """``_rebuild_map`` (slam.py:271-277) from a resident history: ``reset()`` and the replay of every scan at its pose."""
        args = self._replay_args(history, poses, None)             # refused before anything is zeroed
        self.reset()
        self._replay(args, None)

    @staticmethod
    def _box_tiles(box):
        """Tiles of 64 x 64 cells a cell box spans."""
        return ((int(box[2]) - int(box[0])) // 64 + 1) * ((int(box[3]) - int(box[1])) // 64 + 1)

    def _cell_box(self, org, packed):
        """Inclusive cell bounds {x0, y0, x1, y1} of the origins and hits (host int32[4]): every ray stays inside
        (Bresenham never leaves the rectangle of its end points).  Device tensors cost one small read-back."""
        if packed is None or packed.numel() == 0:
            return None
        pts = torch.cat([org.reshape(-1, 2), packed.reshape(-1, 2)])
        lo_hi = torch.stack([pts.amin(dim=0), pts.amax(dim=0)]).cpu().numpy()
        return self._box_of(lo_hi[0], lo_hi[1])

    def _box_of(self, lo, hi):
        # four scalars: plain float arithmetic (the same IEEE operations as the array expression, a fifth of its time —
        # this runs once per live scan)
        x0, y0, x1, y1 = float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])
        if not (math.isfinite(x0) and math.isfinite(y0) and math.isfinite(x1) and math.isfinite(y1)):
            return None                                         # a NaN / inf coordinate somewhere: no promise
        res, lim = self.resolution, 2.0 ** 29
        # same expression as the cell index, monotone in the coordinate; clamped before the floor, which refuses a quotient that
        # overflowed to infinity (a finite coordinate near 1.8e308: the library drops that beam, the box only has to hold it)
        c = [math.floor(min(max((v - m) / res, -lim), lim)) for v, m in ((x0, self.min_x), (y0, self.min_y), (x1, self.min_x), (y1, self.min_y))]
        return np.array([c[0] - 1, c[1] - 1, c[2] + 1, c[3] + 1], dtype=np.int32)

    def _apply(self, org, packed, off, rows=None, box=None):
        """org (S,2) and packed hits (sum N,2) are float64 device tensors; off is a host int32 array.
        box: int32[4] cell bounds of all rays (``_cell_box``), computed here when not given.

        This is the per-scan call of a SLAM loop, so the host side is kept short: the function pointer and the grid's and
        the workspace's addresses are converted once, the raw stream handle is read without
        building a torch.cuda.Stream."""
        S = len(off) - 1
        r0, r1 = (0, self.ny) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= r0 <= r1 <= self.ny:
            raise ValueError("rows must satisfy 0 <= begin <= end <= ny")
        c = self._call
        if c is None:
            L = _lib.lib()
            if self._ws is None:
                self._ws = torch.zeros(L.icpmi_grid_workspace_bytes(self.ny, self.nx), dtype=torch.uint8, device=self._dev)
            c = self._call = (L.icpmi_grid_update_scans_box, C.c_void_p(self._grid.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                              self._dev.index)
        if box is None:
            box = self._cell_box(org, packed)
        # (the scalars are the object's public attributes, as in the reference: read at every call)
        code = c[0](c[1], c[2], self.ny, self.nx, self.min_x, self.min_y, self.resolution, org.data_ptr(),
                    packed.data_ptr() if packed is not None else None, off.ctypes.data, S, float(self.l_hit), float(self.l_miss),
                    self.log_odds_min, self.log_odds_max, self._seq, 1 if self._full_clip else 0, r0, r1,
                    box.ctypes.data if box is not None else None, torch._C._cuda_getCurrentRawStream(c[3]))
        if code != 0:
            _lib.check(code, "update_scan")
        applied = (1 if off[1] > off[0] else 0) if S == 1 else int(np.count_nonzero(np.diff(off)))
        if r1 > r0:
            self._seq += applied
        if applied and (r0, r1) == (0, self.ny):
            self._full_clip = False        # every cell is inside [min, max] after a clipped scan
        self._host = None

    def reset(self):
        """Zero every cell (mapping.py:143-145)."""
        self._grid.zero_()
        self._host = None
        self._full_clip = not (self.log_odds_min <= 0.0 <= self.log_odds_max)

    # ── reading the map: correlative scan-to-map matching (icpmi.gridmatch; no counterpart in the reference) ─────────
    def score_field(self):
        """-> (field, k): the log-odds as the matcher reads them, an int16 (ny, nx) device tensor
        clip(rint(log_odds * 2^k), -32767, 32767), and k = ``icpmi.gridmatch.shift_bits`` of the clamps (12 for +-5).
        Built anew at every call — there is no cache, so no update has to invalidate one.  The matching methods build one
        per call too, unless one is passed back as ``field=``: they then score against the map as it was when that field
        was made, whatever has been applied since."""
        from icpmi import gridmatch
        k = gridmatch.shift_bits(self.log_odds_min, self.log_odds_max)
        return gridmatch.score_field(self._grid, k), k

    def _lf_radius(self, radius):
        from icpmi import gridmatch
        R = int(np.ceil(radius / self.resolution))
        if not 0 <= R <= gridmatch.LF_MAX_RADIUS:
            raise ValueError(f"a radius of {radius} m is {R} cells at {self.resolution} m; at most {gridmatch.LF_MAX_RADIUS} are supported")
        return R

    def distance_field(self, radius, occupied_log_odds=0.5, field=None):
        """-> the squared distance, in cells, of every cell to the nearest occupied one — log-odds >= ``occupied_log_odds`` in
        ``field`` (a ``(tensor, k)`` of ``score_field()``; None: the map as it is now) — exact where it is at most R^2,
        R = int(np.ceil(radius / resolution)) for ``radius`` in metres, and R^2 + 1 elsewhere: an int16 (ny, nx) device tensor
        (``icpmi.gridmatch.distance_field``).  Built anew at every call, like the field."""
        from icpmi import gridmatch
        q, k = self.score_field() if field is None else field
        return gridmatch.distance_field(q, int(np.rint(occupied_log_odds * 2.0 ** k)), self._lf_radius(radius))

    def likelihood_field(self, sigma=None, radius=None, occupied_log_odds=0.5, keep_free=True, field=None):
        """-> (field, k): the map as a likelihood field, for ``field=`` of every matching method (and ``bound_field(field=...)``
        for the wide search).  A cell scores rint(peak * exp(-d^2 / (2 sigma^2))) with d its exact distance to the nearest
        occupied cell — log-odds >= ``occupied_log_odds`` — and peak = rint(log_odds_max * 2^k): a hit half a cell off a wall
        one cell wide still scores.  ``sigma`` in metres (None: one cell); ``radius`` in metres (None: 3 sigma), R =
        int(np.ceil(radius / resolution)) cells — the float quotient as it comes, so 6 * 0.05 m at 0.05 m is 7 cells and 0.3 m is
        6: never fewer than asked for — ValueError above ``icpmi.gridmatch.LF_MAX_RADIUS``.  Beyond the radius a cell
        keeps min(raw field, 0), the penalty of observed free space, with ``keep_free``; else 0.  ``field``: the raw
        ``(tensor, k)`` of ``score_field()`` to start from (None: the map as it is now); k is that field's.
        Built anew at every call — there is no cache, so no update has to invalidate one; a field passed to a matcher scores
        against the map as it was when the field was made, whatever has been applied since."""
        from icpmi import gridmatch
        q, k = self.score_field() if field is None else field
        sigma = self.resolution if sigma is None else float(sigma)
        R = self._lf_radius(3.0 * sigma if radius is None else radius)
        table = gridmatch.likelihood_table(np.rint(self.log_odds_max * 2.0 ** k), sigma / self.resolution, R)
        return gridmatch.likelihood_field(q, int(np.rint(occupied_log_odds * 2.0 ** k)), R, table, keep_free), k

    @staticmethod
    def _xytheta(poses, n=None):
        """Predicted poses as (n, 3) rows [x, y, theta]: given as such, or as a stack of 3 x 3 matrices (theta as
        slam.py:131-132)."""
        p = np.asarray(poses, dtype=np.float64)
        if p.ndim == 3 and p.shape[1:] == (3, 3):
            p = np.stack([p[:, 0, 2], p[:, 1, 2], np.arctan2(p[:, 1, 0], p[:, 0, 0])], axis=1)
        elif p.ndim > 2 or p.size % 3:
            raise ValueError("poses must be rows [x, y, theta] or a stack of 3 x 3 matrices")
        p = p.reshape(-1, 3)
        if n is not None and len(p) != n:
            raise ValueError(f"{n} scans but {len(p)} predicted poses")
        return p

    @staticmethod
    def _one_pose(pose):
        """One pose ([x, y, theta] or a 3 x 3 matrix) as the stack of one the batched methods take."""
        p = np.asarray(pose, dtype=np.float64)
        return p[None] if p.ndim == 2 else p.reshape(1, 3)

    @staticmethod
    def _first(info):
        """The ``info`` of a batch of one as the single-scan methods return it: entry 0 of every array and list."""
        return {k: (v[0] if isinstance(v, (np.ndarray, list)) else v) for k, v in info.items()}

    def _named(self, clouds=None, voxel_size=None, scan=None, poses=None, history=None, ids=None):
        """-> (cloud set, pair_clouds) of the three ways the pair methods name their scans: ``clouds``, one pair each (through
        the voxel filter when a size is given); one ``scan``, uploaded once, at every pose of ``poses``; scans resident in a
        ``history`` by ``ids``, read where they are (``_history_rows`` chooses the rows)."""
        from icpmi import gridmatch, history as _h
        if history is not None:
            ids = _h._scan_ids(ids, ("ids", "scan ids"), history.n_scans)
            return self._history_rows(history, voxel_size), ids
        if scan is not None:
            return gridmatch.cloud_set_of([scan]), np.zeros(len(self._xytheta(poses)), dtype=np.int32)
        cs = gridmatch.cloud_set_of(clouds, voxel_size)
        return cs, np.arange(cs.n_clouds)

    def _pairs(self, cs, pair_clouds, poses):
        """What every pair method starts with -> (pair_clouds int32 [B], the poses as (B, 3) rows [x, y, theta]): the clouds
        on this grid's device, a pose per pair."""
        if cs.pts.device != self._dev:
            raise ValueError(f"the clouds live on {cs.pts.device}, the grid on {self._dev}")
        pair_clouds = np.ascontiguousarray(pair_clouds, dtype=np.int32).reshape(-1)
        return pair_clouds, self._xytheta(poses, len(pair_clouds))

    @staticmethod
    def _cos_sin(theta):
        """(cos, sin) rows of the headings ``theta``, by NumPy on the host: the rotations the cast, the check and the beam model take."""
        return np.stack([np.cos(theta), np.sin(theta)], axis=1)

    def _match_set(self, cs, pair_clouds, poses, linear_window, angular_window, angular_step, field, want_scores=False, half_log_odds=None):
        from icpmi import gridmatch
        pair_clouds, xyt = self._pairs(cs, pair_clouds, poses)
        if angular_step is None:                                   # score_poses: the pose itself and nothing around it
            angles, centre, W = xyt[:, 2:3], 0, 0
        else:
            angles, centre = gridmatch.angle_grid(xyt[:, 2], angular_window, angular_step)
            W = int(round(linear_window / self.resolution))
        job = gridmatch.GridMatchBatch(self, cs, pair_clouds, xyt[:, :2], angles, W, centre, field=field, want_scores=want_scores,
                                       half_log_odds=half_log_odds)
        job.run()
        return job

    def match_scans(self, clouds, predicted_poses, linear_window=0.6, angular_window=12.0, angular_step=1.0, voxel_size=None,
                    field=None, half_log_odds=None):
        """Localise every scan of ``clouds`` (sensor frame, (n, 2) arrays or a device ``CloudSet``) in this map around its
        predicted pose ([x, y, theta] or a 3 x 3 matrix): the pose among theta + np.deg2rad(np.arange(-angular_window,
        angular_window + angular_step, angular_step)) (slam.py:146-148's expression) and shifts of whole cells up to
        W = int(round(linear_window / resolution)) each way that puts the scan's hits on the largest sum of log-odds.
        ``voxel_size``: the scans pass through ``voxel_downsample`` first.  One chain of launches for all scans.
        ``half_log_odds`` (None: off): the drop of the mean log-odds under the hits that halves a candidate's weight; ``info``
        then carries the moments of the score volume about the winner, the sub-cell pose (``t_refined``, ``angle_refined``,
        ``R_refined``) and its ``covariance``, with ``edge_weight`` to show a distribution the window cut off.
        -> (R [B,2,2], t [B,2], score [B], info) as ``icpmi.gridmatch.GridMatchBatch.unpack`` forms them."""
        return self._match_set(*self._named(clouds, voxel_size), predicted_poses, linear_window, angular_window, angular_step, field,
                               half_log_odds=half_log_odds).unpack()

    def match_scan(self, points_local, predicted_pose, linear_window=0.6, angular_window=12.0, angular_step=1.0, voxel_size=None,
                   field=None, half_log_odds=None):
        """``match_scans`` of one scan -> (R (2,2), t (2,), score, info) with scalar entries in ``info``."""
        R, t, score, info = self.match_scans([points_local], [predicted_pose], linear_window, angular_window, angular_step,
                                             voxel_size, field, half_log_odds)
        return R[0], t[0], int(score[0]), self._first(info)

    def score_poses(self, points_local, poses, field=None):
        """The score of one scan at every pose of ``poses`` ((P, 3) rows [x, y, theta] or 3 x 3 matrices): the same kernel
        with one angle and no shifts per pose (pass one matrix as a stack of one) — weights for a particle filter, or a check of a loop closure before its edge
        goes into the graph -> (score [P], info)."""
        _, _, score, info = self._match_set(*self._named(scan=points_local, poses=poses), poses, 0.0, 0.0, None, field).unpack()
        return score, info

    # ── the map read back as ranges (icpmi.gridmatch.cast_rays; no counterpart in the reference) ─────────────────────
    def occupancy_planes(self, occupied_log_odds=0.5, field=None):
        """-> (planes, k): the map as the two bit planes the cast reads — a cell is occupied where its log-odds are >=
        ``occupied_log_odds`` in ``field`` (a ``(tensor, k)`` of ``score_field()`` or ``likelihood_field()``; None: the map as
        it is now), unknown where its field value is 0 — for ``planes=`` of ``cast_scans``.  Built anew at every call; a cast
        against kept planes reads the map as it was when they were made, whatever has been applied since."""
        from icpmi import gridmatch
        q, k = self.score_field() if field is None else field
        return gridmatch.occupancy_planes(q, int(np.rint(occupied_log_odds * 2.0 ** k))), k

    def _cast_map(self, occupied_log_odds, field, planes):
        """-> (what the cast and the check read, k, the threshold): kept ``planes`` as they are, else ``field`` or the map as it
        is now, with ``occupied_log_odds`` in that field's units."""
        from icpmi import gridmatch
        if field is not None and planes is not None:
            raise ValueError("pass field= or planes=, not both")
        if planes is not None:
            src, k = planes
            if not isinstance(src, gridmatch.OccupancyPlanes) or (src.ny, src.nx) != (self.ny, self.nx):
                raise ValueError("planes must be what occupancy_planes() returned for this grid")
            return src, k, src.threshold
        src, k = self.score_field() if field is None else field
        if tuple(src.shape) != (self.ny, self.nx):
            raise ValueError("field must be the int16 (ny, nx) tensor score_field() returned for this grid")
        return src, k, int(np.rint(occupied_log_odds * 2.0 ** k))

    def cast_scans(self, poses, angles, max_range, occupied_log_odds=0.5, field=None, planes=None):
        """The scan this map predicts at every pose of ``poses`` ((P, 3) rows [x, y, theta] or 3 x 3 matrices): along each
        sensor-frame bearing of ``angles`` (radians, A of them) up to ``max_range`` metres, the first occupied cell — log-odds
        >= ``occupied_log_odds`` — among exactly the cells ``update_scan`` would lower for a hit at that range, end cell
        included, and the first unknown cell before it.  One launch for all P x A rays.  ``field``: a ``(tensor, k)`` to read
        instead of the map as it is now; ``planes``: what ``occupancy_planes()`` returned (``occupied_log_odds`` is then the
        planes' own).  -> (ranges (P, A) float64, info).  ``ranges``: the distance from the pose to the CENTRE of the hit cell,
        hypot((x_hit + 0.5) * resolution + min_x - x, (y_hit + 0.5) * resolution + min_y - y); inf where nothing was hit, nan
        where the ray has no cells (a pose or end point that is not finite).  info: ``k_hit`` (P, A) (the step of the hit; -1
        none, -2 no cells), ``cells`` (P, A, 2) the hit cell (x, y) (the end cell without a hit), ``k_unknown`` (P, A) (-1: none),
        ``unknown_range`` (the same distance to the first unknown cell, inf without one) and ``shift_bits``."""
        from icpmi import gridmatch
        src, k, threshold = self._cast_map(occupied_log_odds, field, planes)
        xyt = self._xytheta(poses)
        ang = np.asarray(angles, dtype=np.float64).reshape(-1)
        pose_cs, beam_cs = self._cos_sin(xyt[:, 2]), self._cos_sin(ang)
        rec = gridmatch.cast_rays(src, threshold, self.min_x, self.min_y, self.resolution, xyt[:, :2], pose_cs, beam_cs, max_range)
        rec = rec.cpu().numpy().astype(np.int64)
        k_hit, k_unknown = rec[..., _lib.GC_K_HIT], rec[..., _lib.GC_K_UNKNOWN]
        cells = rec[..., _lib.GC_X_HIT:_lib.GC_Y_HIT + 1]
        segs, _ = gridmatch.ray_end_cells(self.min_x, self.min_y, self.resolution, xyt[:, :2], pose_cs, beam_cs, float(max_range))
        ux, uy = gridmatch.step_cells(segs, np.maximum(k_unknown, 0))
        px, py = xyt[:, None, 0], xyt[:, None, 1]
        centre = lambda cx, cy: np.hypot((cx + 0.5) * self.resolution + self.min_x - px, (cy + 0.5) * self.resolution + self.min_y - py)  # noqa: E731
        with np.errstate(invalid="ignore", over="ignore"):
            ranges = np.where(k_hit >= 0, centre(cells[..., 0], cells[..., 1]), np.where(k_hit == _lib.GC_NONE, np.inf, np.nan))
            unknown_range = np.where(k_unknown >= 0, centre(ux, uy), np.inf)
        return ranges, {"k_hit": k_hit, "cells": cells, "k_unknown": k_unknown, "unknown_range": unknown_range, "shift_bits": k}

    def cast_scan(self, pose, angles, max_range, occupied_log_odds=0.5, field=None, planes=None):
        """``cast_scans`` from one pose ([x, y, theta] or a 3 x 3 matrix) -> (ranges (A,), info) with (A, ...) entries."""
        ranges, info = self.cast_scans(self._one_pose(pose), angles, max_range, occupied_log_odds, field, planes)
        return ranges[0], self._first(info)

    # ── measured scans held against the map along their beams (icpmi.gridmatch.check_pairs; no counterpart in the reference) ──
    def _check_set(self, cs, pair_clouds, poses, tolerance, occupied_log_odds, field, planes, want_rows):
        from icpmi import gridmatch
        src, k, threshold = self._cast_map(occupied_log_odds, field, planes)
        pair_clouds, xyt = self._pairs(cs, pair_clouds, poses)
        cos_sin = self._cos_sin(xyt[:, 2])
        records, rows = gridmatch.check_pairs(src, threshold, self.min_x, self.min_y, self.resolution, cs, pair_clouds, xyt[:, :2], cos_sin,
                                              tolerance, want_rows=want_rows)
        rec = records.cpu().numpy().astype(np.int64)
        info = {key: rec[:, slot].copy() for key, slot in (
            ("status", _lib.GK_REC_STATUS), ("rows", _lib.GK_REC_ROWS), ("confirmed", _lib.GK_REC_CONFIRMED), ("violated", _lib.GK_REC_VIOLATED),
            ("in_free", _lib.GK_REC_IN_FREE), ("unexplored", _lib.GK_REC_UNEXPLORED), ("through_unknown", _lib.GK_REC_THROUGH_UNKNOWN))}
        some = np.maximum(info["rows"], 1)
        info["violated_share"] = np.where(info["rows"] > 0, info["violated"] / some, 0.0)
        info["in_free_share"] = np.where(info["rows"] > 0, info["in_free"] / some, 0.0)
        info["shift_bits"] = k
        if want_rows:
            info["classes"] = self._rows_per_pair(cs, pair_clouds, rows, info["status"] == _lib.GK_ST_CAPACITY)
        return info

    @staticmethod
    def _rows_per_pair(cs, pair_clouds, rows, refused):
        """The rows' records of the check or the beam model, per pair, cut to the cloud's count (none where the count was
        ``refused``: nothing was read)."""
        n = np.diff(cs.off_host).astype(np.int64)
        if cs.cnt is not None:
            n = np.minimum(n, cs.cnt.cpu().numpy().astype(np.int64))
        n = np.where(refused, 0, n[pair_clouds])
        host = rows.cpu().numpy()
        return [host[b, :n[b]].copy() for b in range(len(pair_clouds))]

    def check_scans(self, clouds, poses, tolerance=2, occupied_log_odds=0.5, voxel_size=None, field=None, planes=None, want_rows=False):
        """Does each scan of ``clouds`` (sensor frame, (n, 2) arrays or a device ``CloudSet``), held at its pose of ``poses``
        ([x, y, theta] rows or 3 x 3 matrices), contradict the free space and the walls this map already holds?  Every
        measured beam is walked from the pose's cell to the cell of its own hit — exactly the cells ``update_scan`` would
        touch for it — and falls in one class: ``confirmed``, the map has an occupied cell (log-odds >= ``occupied_log_odds``)
        within ``tolerance`` steps of the beam's end; ``violated``, the first occupied cell lies more than ``tolerance`` steps
        before the end — the beam came back from behind a wall of the map, which is what a false loop closure between
        similar rooms looks like —; ``in_free``, nothing occupied and the end in observed free space (something new, or
        something that moved in); ``unexplored``, nothing occupied and the end in unknown space or off the grid.  A sum of
        log-odds under the hits (``score_poses``) sees none of this.  One launch for all scans; only a few integers per scan
        come back.  ``tolerance`` is in steps (cells along the beam's major axis); at 0 a true pose fails, because a noisy
        return lands a cell behind the first occupied layer of a mapped wall.  A return just IN FRONT of a thin wall counts
        as ``in_free``; the remedy is thicker walls: pass ``planes=occupancy_planes(lower_occupied_log_odds,
        field=likelihood_field(...))`` — planes packed from a likelihood field with a lower ``occupied_log_odds`` hold every
        cell near a wall occupied.  ``voxel_size``: the scans pass through ``voxel_downsample`` first.  ``field``: a
        ``(tensor, k)`` to read instead of the map as it is now; ``planes``: what ``occupancy_planes()`` returned
        (``occupied_log_odds`` is then the planes' own); both show the map as it was when they were made.
        -> info: int64 arrays ``rows`` (the rows with cells), ``confirmed``, ``violated``, ``in_free``, ``unexplored`` (these
        four sum to ``rows``), ``through_unknown`` (rows whose beam crossed an unknown cell before its hit or end) and
        ``status`` (``icpmi._lib.GK_ST_*``); ``violated_share`` and ``in_free_share`` (count / rows, 0.0 where rows is 0);
        ``shift_bits``.  With ``want_rows``, ``classes``: per scan an (n, 4) int32 array [class, k_hit, K, k_unknown] per row
        (``icpmi._lib.GK_CLASS_*``; ``GK_NO_CELLS`` for a row without cells)."""
        return self._check_set(*self._named(clouds, voxel_size), poses, tolerance, occupied_log_odds, field, planes, want_rows)

    def check_scan(self, points_local, pose, tolerance=2, occupied_log_odds=0.5, voxel_size=None, field=None, planes=None, want_rows=False):
        """``check_scans`` of one scan at one pose ([x, y, theta] or a 3 x 3 matrix) -> info with scalar entries (``classes``:
        the one (n, 4) array)."""
        return self._first(self.check_scans([points_local], self._one_pose(pose), tolerance, occupied_log_odds, voxel_size, field, planes,
                                            want_rows))

    def check_poses(self, points_local, poses, tolerance=2, occupied_log_odds=0.5, field=None, planes=None, want_rows=False):
        """``check_scans`` of ONE scan at every pose of ``poses`` ((P, 3) rows [x, y, theta] or 3 x 3 matrices), as
        ``score_poses`` scores one: the scan is uploaded once and every hypothesis names it — a particle filter's free-space
        test, or a gate on loop-closure candidates -> info with (P,) entries."""
        return self._check_set(*self._named(scan=points_local, poses=poses), poses, tolerance, occupied_log_odds, field, planes, want_rows)

    def check_history(self, history, ids, poses, tolerance=2, occupied_log_odds=0.5, voxel_size=None, field=None, planes=None,
                      want_rows=False):
        """``check_scans`` of scans resident in an ``icpmi.ScanHistory``, by id: the rows are read where they are and no scan
        is uploaded; ``voxel_size`` chooses them as in ``match_history``."""
        return self._check_set(*self._named(history=history, ids=ids, voxel_size=voxel_size), poses, tolerance, occupied_log_odds, field,
                               planes, want_rows)

    # ── the beam model: measured scans scored against the ranges the map expects (icpmi.gridmatch.beam_pairs) ───────────
    def _beam_set(self, cs, pair_clouds, poses, sigma, half_width, beyond, table, occupied_log_odds, field, planes, want_histogram, want_rows):
        from icpmi import gridmatch
        src, k, threshold = self._cast_map(occupied_log_odds, field, planes)
        pair_clouds, xyt = self._pairs(cs, pair_clouds, poses)
        cos_sin = self._cos_sin(xyt[:, 2])
        if table is None:
            table = gridmatch.beam_table(self.resolution, self.resolution if sigma is None else sigma, half_width)
        if beyond is None:
            beyond = 1.5 * (int(half_width) + 2) * self.resolution
        records, hist, rows = gridmatch.beam_pairs(src, threshold, self.min_x, self.min_y, self.resolution, cs, pair_clouds, xyt[:, :2], cos_sin,
                                                   table, half_width, beyond, want_hist=want_histogram, want_rows=want_rows)
        rec = records.cpu().numpy().astype(np.int64)
        info = {key: rec[:, slot].copy() for key, slot in (
            ("status", _lib.GB_REC_STATUS), ("rows", _lib.GB_REC_ROWS), ("score", _lib.GB_REC_SCORE), ("expected", _lib.GB_REC_EXPECTED),
            ("novel", _lib.GB_REC_NOVEL), ("unexplored", _lib.GB_REC_UNEXPLORED))}
        info["mean_score"] = np.where(info["rows"] > 0, info["score"] / np.maximum(info["rows"], 1), 0.0)
        info["shift_bits"] = k
        if want_histogram:
            info["histogram"] = hist.cpu().numpy().astype(np.int64)
        if want_rows:
            info["classes"] = self._rows_per_pair(cs, pair_clouds, rows, info["status"] == _lib.GB_ST_CAPACITY)
        return info

    def beam_scans(self, clouds, poses, sigma=None, half_width=8, beyond=None, table=None, occupied_log_odds=0.5, voxel_size=None, field=None,
                   planes=None, want_histogram=False, want_rows=False):
        """The beam model: how well does each scan of ``clouds`` (sensor frame, (n, 2) arrays or a device ``CloudSet``), held at
        its pose of ``poses`` ([x, y, theta] rows or 3 x 3 matrices), agree with the ranges this map expects?  Every measured
        beam is walked from the pose's cell through the cell of its own hit to ``beyond`` metres behind it; the signed number
        of steps d between the map's first occupied cell (log-odds >= ``occupied_log_odds``) and the step at which the beam
        returned picks ``table[clamp(d, -H, H) + H]``, H = ``half_width``: d > 0, the beam came back short of the map's wall;
        d < 0, from behind it.  A beam without a wall on its walk reads ``table[2H + 1]`` where it returned out of observed
        free space and ``table[2H + 2]`` where it returned from unexplored space or off the grid.  The score of a scan is the
        sum over its beams — a log-likelihood in units of 1 / 1024 with the default table, which falls smoothly where
        ``check_scans`` counts four classes with a hard tolerance and ``score_poses`` cannot see the free space a beam
        crossed; ``icpmi.gridmatch.pose_weights`` turns scores into a particle filter's weights.  One launch for all scans.
        ``sigma``: the Gaussian's width in metres (None: one cell); ``beyond``: None for 1.5 * (half_width + 2) * resolution,
        enough for H + 1 major steps past the return on any bearing; ``table``: int32 [2H + 3] to read instead of
        ``icpmi.gridmatch.beam_table(resolution, sigma, half_width)``.  Differences are steps along a beam's major axis: a
        cell along an axis, up to sqrt(2) cells in metres along a diagonal.  ``voxel_size``, ``field``, ``planes`` as for
        ``check_scans``.
        -> info: int64 arrays ``status`` (``icpmi._lib.GB_ST_*``), ``rows`` (the rows with cells), ``score``, ``expected`` (rows
        with a wall of the map on their walk), ``novel`` (index 2H + 1), ``unexplored`` (index 2H + 2; the three sum to
        ``rows``); ``mean_score`` (score / rows, 0.0 where rows is 0); ``shift_bits``.  With ``want_histogram``,
        ``histogram`` (B, 2H + 3): the rows per index.  With ``want_rows``, ``classes``: per scan an (n, 4) int32 array [index,
        k_hit, k_z, k_unknown] per row (``GB_NO_CELLS`` for a row without cells)."""
        return self._beam_set(*self._named(clouds, voxel_size), poses, sigma, half_width, beyond, table, occupied_log_odds, field, planes,
                              want_histogram, want_rows)

    def beam_scan(self, points_local, pose, sigma=None, half_width=8, beyond=None, table=None, occupied_log_odds=0.5, voxel_size=None,
                  field=None, planes=None, want_histogram=False, want_rows=False):
        """``beam_scans`` of one scan at one pose ([x, y, theta] or a 3 x 3 matrix) -> info with scalar entries (``histogram``:
        the one (2H + 3,) array; ``classes``: the one (n, 4) array)."""
        return self._first(self.beam_scans([points_local], self._one_pose(pose), sigma, half_width, beyond, table, occupied_log_odds,
                                           voxel_size, field, planes, want_histogram, want_rows))

    def beam_poses(self, points_local, poses, sigma=None, half_width=8, beyond=None, table=None, occupied_log_odds=0.5, field=None,
                   planes=None, want_histogram=False, want_rows=False):
        """``beam_scans`` of ONE scan at every pose of ``poses`` ((P, 3) rows [x, y, theta] or 3 x 3 matrices): the scan is
        uploaded once and every hypothesis names it — a particle filter's measurement update (``icpmi.gridmatch.pose_weights``
        of ``score`` and ``status``), or a ranking of loop-closure candidates -> info with (P,) entries."""
        return self._beam_set(*self._named(scan=points_local, poses=poses), poses, sigma, half_width, beyond, table, occupied_log_odds,
                              field, planes, want_histogram, want_rows)

    def beam_history(self, history, ids, poses, sigma=None, half_width=8, beyond=None, table=None, occupied_log_odds=0.5, voxel_size=None,
                     field=None, planes=None, want_histogram=False, want_rows=False):
        """``beam_scans`` of scans resident in an ``icpmi.ScanHistory``, by id: the rows are read where they are and no scan
        is uploaded; ``voxel_size`` chooses them as in ``match_history``."""
        return self._beam_set(*self._named(history=history, ids=ids, voxel_size=voxel_size), poses, sigma, half_width, beyond, table,
                              occupied_log_odds, field, planes, want_histogram, want_rows)

    def particle_filter(self, n, **kw):
        """An ``icpmi.particles.ParticleFilter`` of ``n`` particles bound to this grid: localisation in the map as it is now
        (its bit planes are packed once; ``refresh_map()`` after the grid has changed).  ``kw``: ``seed``, ``temperature`` and
        the beam model's ``sigma``, ``half_width``, ``beyond``, ``table``, ``occupied_log_odds``, ``field``, ``planes``.  The
        filter starts about a known pose (``init_gaussian``) or over the free cells of this map (``init_uniform``, ``free_cells``)
        and recovers by injection (``resample(inject=)``, ``maybe_resample(recovery=)``)."""
        from icpmi.particles import ParticleFilter
        return ParticleFilter(self, n, **kw)

    @staticmethod
    def _history_rows(history, voxel_size):
        """The cloud set of a history's scans at ``voxel_size``: the raw rows (None), the history's own filtered copies where
        it is one of the history's voxel sizes, any other size filters every resident scan first."""
        from icpmi.batch import voxel_downsample_set
        if voxel_size is None:
            return history.raw
        if float(voxel_size) == history.voxel_size:
            return history.vox
        if float(voxel_size) == history.rotation_voxel_size:
            return history.rs_vox
        return voxel_downsample_set(history.raw, voxel_size)

    def match_history(self, history, ids, predicted_poses, linear_window=0.6, angular_window=12.0, angular_step=1.0, voxel_size=None,
                      field=None, half_log_odds=None):
        """``match_scans`` of scans resident in an ``icpmi.ScanHistory``, by id: the raw rows are read where they are and no
        scan is uploaded.  ``voxel_size``: the history's own filtered copies where it is one of the history's voxel sizes;
        any other size filters every resident scan first."""
        return self._match_set(*self._named(history=history, ids=ids, voxel_size=voxel_size), predicted_poses, linear_window, angular_window,
                               angular_step, field, half_log_odds=half_log_odds).unpack()

    # ── the same search over a wide window (icpmi.gridmatch.GridSearchBatch): metres and the full circle ─────────────
    def bound_field(self, field=None, block=8):
        """-> the bound field of ``field`` (a ``(tensor, k)`` of ``score_field()``; None: of the map as it is now) for blocks of
        ``block`` x ``block`` shifts: what the ``search_*`` methods prune with.  Built anew at every call, like the field; a
        caller who keeps one passes it back as ``bounds=`` together with the ``field=`` it was made from."""
        from icpmi import gridmatch
        return gridmatch.bound_field((self.score_field() if field is None else field)[0], block)

    def _search_set(self, cs, pair_clouds, poses, linear_window, angular_window, angular_step, block, field, bounds):
        from icpmi import gridmatch
        if bounds is not None and field is None:
            raise ValueError("bounds= belongs to the field it was made from: pass that field= too")
        pair_clouds, xyt = self._pairs(cs, pair_clouds, poses)
        angles, centre = gridmatch.angle_grid(xyt[:, 2], angular_window, angular_step)
        W = int(round(linear_window / self.resolution))
        job = gridmatch.GridSearchBatch(self, cs, pair_clouds, xyt[:, :2], angles, W, centre, block=block, field=field, bounds=bounds)
        job.run()
        return job

    def search_scans(self, clouds, predicted_poses, linear_window=5.0, angular_window=180.0, angular_step=1.0, voxel_size=None,
                     block=8, field=None, bounds=None):
        """``match_scans`` over a wide window — localising in a saved or rebuilt map, recovering when ICP and the submap both
        reject, checking a loop closure: the same arguments, angle grid and result (the first maximum of the exhaustive
        search, bit for bit), up to ``icpmi.gridmatch.WIDE_MAX_WINDOW`` cells each way.  The shifts are cut into blocks of
        ``block`` x ``block`` (4, 8 or 16); only blocks whose upper bound reaches a seed score are scored.  ``info`` adds
        ``blocks``, ``survivors``, ``seed_score`` and ``max_bound``.  ``bounds``: a ``bound_field(field, block)`` kept by the
        caller, with the ``field`` it was made from."""
        return self._search_set(*self._named(clouds, voxel_size), predicted_poses, linear_window, angular_window, angular_step, block, field,
                                bounds).unpack()

    def search_scan(self, points_local, predicted_pose, linear_window=5.0, angular_window=180.0, angular_step=1.0, voxel_size=None,
                    block=8, field=None, bounds=None):
        """``search_scans`` of one scan -> (R (2,2), t (2,), score, info) with scalar entries in ``info``."""
        R, t, score, info = self.search_scans([points_local], [predicted_pose], linear_window, angular_window, angular_step,
                                              voxel_size, block, field, bounds)
        return R[0], t[0], int(score[0]), self._first(info)

    def search_history(self, history, ids, predicted_poses, linear_window=5.0, angular_window=180.0, angular_step=1.0, voxel_size=None,
                       block=8, field=None, bounds=None):
        """``search_scans`` of scans resident in an ``icpmi.ScanHistory``, by id, with ``match_history``'s choice of rows."""
        return self._search_set(*self._named(history=history, ids=ids, voxel_size=voxel_size), predicted_poses, linear_window, angular_window,
                                angular_step, block, field, bounds).unpack()

    # ── probability / display, mapping.py:150-166 (NumPy on the host copy) ───
    def to_probability(self):
        return 1.0 / (1.0 + np.exp(-self.log_odds))

    def to_display(self):
        lo = self.log_odds
        display = 1.0 - self.to_probability()
        display[lo == 0.0] = 1.0      # unexplored -> white
        display[lo < 0.0] = 0.85      # free -> light grey
        return display

    def _flat_cell_data(self):
        return self.to_display().ravel(order="C")

    # ── PyVista helpers, mapping.py:168-178 (display only; pyvista optional) ─
    def create_pyvista_grid(self):
        import pyvista as pv
        grid = pv.ImageData(dimensions=(self.nx + 1, self.ny + 1, 1),
                            spacing=(self.resolution, self.resolution, 1e-6),
                            origin=(self.min_x, self.min_y, 0.0))
        grid.cell_data["occ"] = self._flat_cell_data()
        return grid

    def update_pyvista_grid(self, grid):
        grid.cell_data["occ"] = self._flat_cell_data()

    # ── export, mapping.py:183-187 ───────────────────────────────────────────
    def save_csv(self, file_path):
        np.savetxt(file_path, self.to_probability(), delimiter=",")

    def save_npy(self, file_path):
        np.save(file_path, self.to_probability())


def _minmax_rows(rows):
    """(min, max) over the rows of an (n, 2) array — on a transposed copy: NumPy reduces axis 0 of a two-column array
    with an inner loop of length two (90 us for a 2 048-beam scan), and the contiguous axis of the copy in 5."""
    t = np.ascontiguousarray(rows.T)
    return t.min(axis=1), t.max(axis=1)


def reach_cell_box(grid, poses, reach):
    """Inclusive cell bounds (host int32[4], through ``grid._box_of``) that hold every ray of scans whose world rows exist on
    the device only: scan s has the pose poses[s] = {R row-major, t} (six doubles) and no raw row longer than reach[s]
    (``ScanHistory.reach``).  A superset of the exact box of origins and world rows; ``None`` (no promise: the caller reads
    the bounds back from the device) when a reach or a pose is not finite.  ``grid``: anything with min_x, min_y and
    resolution.  Host arithmetic only.

    A world coordinate is w = fl(fl(fma(y, b, fl(x a))) + t) with (a, b) a row of R, exactly x a + y b + t but for three
    roundings.  |x a + y b| <= |(a, b)| |(x, y)| <= F r, with F the Frobenius norm of R and r the reach.  With u = 2^-53,
    the product and the fma put at most (1 + u)^2 on that, and the last addition at most u |w| <= u (|t| + F r (1 + u)^2)
    more, so |w - t| <= F r (1 + 4u) + 2u |t|.  F and r are themselves computed here: two nested hypots, the reach's hypot
    and their product are each within an ulp or two, under 8u relative together, and t -+ d below rounds once more,
    u (|t| + d).  Where an intermediate is subnormal a rounding is absolute, at most 2^-1074 each.  The margin taken,
    d = F r (1 + 2^-40) + 2^-40 |t| + 1e-300, covers all of that some thousand times over and is a relative 1e-12 of the
    distances involved: it moves a cell bound only for a coordinate that close to a cell edge."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    r = np.asarray(reach, dtype=np.float64).reshape(-1)
    if len(P) == 0 or len(P) != len(r) or not (np.isfinite(P).all() and np.isfinite(r).all()):
        return None
    F = np.hypot(np.hypot(P[:, 0], P[:, 1]), np.hypot(P[:, 2], P[:, 3]))
    eps = 2.0 ** -40
    t = P[:, 4:6]
    d = ((F * r) * (1.0 + eps))[:, None] + eps * np.abs(t) + 1e-300
    return OccupancyGrid2D._box_of(grid, (t - d).min(axis=0), (t + d).max(axis=0))


def bresenham_cells(segments):
    """Cells of ``_bresenham`` for every row ``[x0, y0, x1, y1]`` of ``segments`` -> list of (n_s, 2) int32 arrays."""
    _b.require_gpu()
    L = _lib.lib()
    seg = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 4)
    if len(seg) and np.abs(seg).max() >= 2 ** 29:
        raise OverflowError("cell coordinates beyond +-2^29 are not supported")
    n = np.maximum(np.abs(seg[:, 2] - seg[:, 0]), np.abs(seg[:, 3] - seg[:, 1]))
    off = np.zeros(len(seg) + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    dev = torch.device("cuda", torch.cuda.current_device())
    d_seg = torch.from_numpy(seg.astype(np.int32)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_out = torch.empty((max(int(off[-1]), 1), 2), dtype=torch.int32, device=dev)
    _lib.check(L.icpmi_bresenham_cells(_b._ptr(d_seg), _b._ptr(d_off), len(seg), _b._ptr(d_out), _b._stream()),
               "_bresenham")
    out = d_out.cpu().numpy()
    return [out[off[i]:off[i + 1]].copy() for i in range(len(seg))]
