"""A particle filter on the occupancy grid with its state resident on the device (``icpmi_pf_predict``, ``icpmi_pf_weights``,
``icpmi_pf_resample``, ``icpmi_pf_estimate``; the contract is include/icpmi.h's): localisation in a finished map.  The
particles are three float64 device tensors in the layout the beam model takes its poses in, so ``icpmi_grid_beam_batch``
scores one scan at every particle where the particles are; its integer scores become integer weights through a table
(``weight_table``), resampling is systematic over an integer prefix sum, and the random numbers are Philox4x32-10 at the
counter [particle, block, step, purpose]: a step is a function of (inputs, seed, step) to the bit.  A step reads four sums
back (``weigh``) and, when the caller asks for it, eight more (``estimate``); nothing else crosses to the host.

Without a prior the particles start over the map's free cells (``init_uniform``), and a filter that has lost the robot finds
it again by injection: ``resample(inject=m)`` draws m of the new generation from the free cells, and ``Recovery`` decides m
from the sums a step reads back anyway (``icpmi_pf_free_index``, ``icpmi_pf_draw_uniform``).
"""
import math

import numpy as np
import torch

from . import _lib, gridmatch
from ._lib import check
from .batch import _ptr, _stream, require_gpu

MAX_PARTICLES, ST_OK, ST_DEGENERATE, ST_NO_FREE = _lib.PF_MAX_PARTICLES, _lib.PF_ST_OK, _lib.PF_ST_DEGENERATE, _lib.PFG_ST_NO_FREE
INJECTED = _lib.PFG_INJECTED                                   # ``ancestors`` of a particle drawn from the free cells
NO_SCORE = -2 ** 63                                            # sums[PF_SUM_SMAX] when no record is OK
TWO_PI = 2.0 * math.pi


def weight_table(temperature, scale=1024, entries=4096, peak=2 ** 20):
    """The table ``icpmi_pf_weights`` reads, for scores of ``beam_pairs`` made with a table of that ``scale``: entry q is
    rint(peak * exp(-(q * 2^shift) / (scale * temperature))), the weight of a particle whose score lies q * 2^shift below
    the best one — ``pose_weights``' softmax about the maximum, in integers.  ``shift`` is the least non-negative integer
    for which the last entry's value lies below 0.5, so the table ends in a 0 and spans every distance that still has a
    weight.  ``temperature`` > 1 flattens the weights (see ``pose_weights``).  -> (uint32 [entries], shift)."""
    n, peak_i = int(entries), int(peak)
    if n != entries or not 1 <= n <= _lib.PF_MAX_ENTRIES or peak_i != peak or not 1 <= peak_i <= _lib.PF_MAX_WEIGHT:
        raise ValueError(f"entries must be a whole number in [1, {_lib.PF_MAX_ENTRIES}] and peak one in [1, {_lib.PF_MAX_WEIGHT}], "
                         f"got {entries}, {peak}")
    if not (np.isfinite(temperature) and temperature > 0.0 and np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"temperature and scale must be positive and finite, got {temperature}, {scale}")
    unit = float(scale) * float(temperature)
    value = lambda q, shift: peak_i * np.exp(-(q * 2.0 ** shift) / unit)          # noqa: E731
    shift = 0
    while n > 1 and value(n - 1.0, shift) >= 0.5:
        shift += 1
        if shift > _lib.PF_MAX_SHIFT:
            raise ValueError(f"temperature {temperature} at scale {scale} needs a shift above {_lib.PF_MAX_SHIFT}")
    return np.rint(value(np.arange(n, dtype=np.float64), shift)).astype(np.uint32), shift


class FreeCells:
    """The free index of a map's bit planes inside a cell box (``icpmi_pf_free_index``; include/icpmi.h has the layout):
    ``index``, the uint8 device buffer — its layout is csrc/particles.hpp's alone and is not restated here —; ``cells`` = (x0,
    y0, x1, y1), the half-open box as it was asked for.  ``build()`` enqueues the launches again, into the same buffer;
    ``count()`` reads the number of free cells, the buffer's first word, back."""

    def __init__(self, planes, cells):
        self.planes, self.cells = planes, tuple(int(v) for v in cells)
        need = _lib.lib().icpmi_pf_free_index_bytes(planes.ny, planes.nx)
        if not need:
            raise ValueError(f"a grid of {planes.ny} x {planes.nx} cells has more than {_lib.PFG_FREE_MAX_WORDS} plane words: no free index")
        self.index = torch.zeros(need, dtype=torch.uint8, device=planes.buf.device)
        self.build()

    def build(self):
        p = self.planes
        check(_lib.lib().icpmi_pf_free_index(_ptr(p.buf), p.ny, p.nx, *self.cells, _ptr(self.index), self.index.numel(), _stream()),
              "pf_free_index")
        return self

    def count(self):
        """The number of free cells (synchronises)."""
        return int(self.index[:4].view(torch.int32).item())


class Recovery:
    """How many particles to inject, by the rule of augmented MCL (Thrun, Burgard, Fox, "Probabilistic Robotics", table 8.3),
    on the host, from numbers a step reads back anyway.  ``update(s_max, rows)`` forms q = exp(s_max / (scale * rows)) — the
    best particle's mean likelihood per beam, ``s_max`` = ``sums[PF_SUM_SMAX]`` of the beam model's scores at that ``scale``,
    ``rows`` the scan's rows; no OK record: q = 0 —, moves ``w_slow`` and ``w_fast`` towards q by ``alpha_slow`` and
    ``alpha_fast`` (both start at the first q) and returns max(0, 1 - w_fast / w_slow), the share to inject: 0 while the
    short average keeps up with the long one, and 0 where the long one is 0."""

    def __init__(self, alpha_slow=0.05, alpha_fast=0.6, scale=1024):
        if not (0.0 < alpha_slow <= alpha_fast <= 1.0 and math.isfinite(scale) and scale > 0.0):
            raise ValueError(f"0 < alpha_slow <= alpha_fast <= 1 and a positive scale, got {alpha_slow}, {alpha_fast}, {scale}")
        self.alpha_slow, self.alpha_fast, self.scale = float(alpha_slow), float(alpha_fast), float(scale)
        self.w_slow = self.w_fast = None

    def update(self, s_max, rows):
        q = 0.0 if int(s_max) == NO_SCORE or rows <= 0 else math.exp(int(s_max) / (self.scale * int(rows)))
        if self.w_slow is None:
            self.w_slow = self.w_fast = q
        else:
            self.w_slow += self.alpha_slow * (q - self.w_slow)
            self.w_fast += self.alpha_fast * (q - self.w_fast)
        return max(0.0, 1.0 - self.w_fast / self.w_slow) if self.w_slow > 0.0 else 0.0


class ParticleFilter:
    """``n`` pose hypotheses [x, y, theta] in the map of ``grid`` (a ``utilities.mapping.OccupancyGrid2D``), kept on the
    grid's device: ``predict`` moves them by a control with noise, ``weigh`` scores a scan at each of them with the beam
    model and turns the scores into integer weights, ``resample`` / ``maybe_resample`` draw the next generation, ``estimate``
    reads the weighted mean and spread.  The particles start at ``set_poses`` rows, about a known pose (``init_gaussian``) or
    over the map's free cells (``init_uniform``); ``resample(inject=m)`` and ``maybe_resample(recovery=Recovery())`` bring a
    lost filter back.

    ``seed``: the generator's 64-bit key; with the step counter (``step``: one more after every ``predict`` and every
    ``resample``) it fixes every draw.  ``temperature``: of ``weight_table`` — the beams of a scan are not independent, and
    weights that multiply hundreds of them as if they were collapse onto one particle; the default 8 keeps tens of a few
    hundred particles alive on a 64-beam scan.  ``sigma``, ``half_width``, ``beyond``, ``table``, ``occupied_log_odds``,
    ``field``, ``planes``: of ``OccupancyGrid2D.beam_scans``.  The bit planes of the map are packed once, here (or are the
    caller's ``planes``); ``refresh_map()`` packs them again after the grid has changed.

    Every method enqueues on the current stream; ``weigh`` (four sums), ``estimate`` (eight), ``poses`` and ``resample``'s
    status are the read-backs.  ``ancestors``: the int32 device tensor of the last resampling (particle j of the present
    generation was particle ``ancestors[j]`` of the one before)."""

    def __init__(self, grid, n, seed=0, temperature=8.0, sigma=None, half_width=8, beyond=None, table=None, occupied_log_odds=0.5, field=None,
                 planes=None):
        require_gpu()
        N = int(n)
        if N != n or not 1 <= N <= MAX_PARTICLES:
            raise ValueError(f"n must be a whole number of particles in [1, {MAX_PARTICLES}], got {n}")
        if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be a whole number in [0, 2^64), got {seed}")
        H = int(half_width)
        if H != half_width or not 0 <= H <= _lib.GB_MAX_HALF_WIDTH:
            raise ValueError(f"half_width must be a whole number in [0, {_lib.GB_MAX_HALF_WIDTH}], got {half_width}")
        self.grid, self.n, self.seed, self.step, self.half_width = grid, N, int(seed), 0, H
        self.beyond = 1.5 * (H + 2) * grid.resolution if beyond is None else float(beyond)
        if not (np.isfinite(self.beyond) and self.beyond >= 0.0):
            raise ValueError(f"beyond must be finite and not negative, got {beyond}")
        self._map_args = (occupied_log_odds, field)
        self._own_planes = planes is None
        self._free = {}                                            # the FreeCells of free_cells(), by cell box
        if planes is not None:
            self.planes, self.shift_bits, _ = grid._cast_map(occupied_log_odds, field, planes)       # (refuses field= with planes=)
        else:
            self.refresh_map()
        dev = self.planes.buf.device
        if table is None:
            table = gridmatch.beam_table(grid.resolution, grid.resolution if sigma is None else sigma, H)
        table = np.ascontiguousarray(table)
        if table.dtype.kind not in "iu" or table.shape != (2 * H + 3,) or np.abs(table.astype(np.int64)).max() >= 2 ** 31:
            raise ValueError(f"table must hold int32 [{2 * H + 3}] for a half width of {H}")
        self.beam_table_host = table.astype(np.int32)
        self.weight_table_host, self.weight_shift = weight_table(temperature)
        self.temperature = float(temperature)
        self._beam_table = torch.from_numpy(self.beam_table_host).to(dev)
        self._weight_table = torch.from_numpy(self.weight_table_host.view(np.int32)).to(dev)     # (uint32 on the device; torch copies the bits)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)          # noqa: E731
        self._state, self._spare = [(f64(N, 2), f64(N), f64(N, 2)) for _ in range(2)]
        self._state[2][:, 0] = 1.0                                 # every particle at the origin, heading 0, until set_poses
        self._spare[2][:, 0] = 1.0
        self.records = torch.zeros((N, _lib.GB_INTS), dtype=torch.int32, device=dev)
        self.w = torch.ones(N, dtype=torch.int32, device=dev)     # (uint32 on the device: weights are at most 2^20)
        self.sums = torch.zeros(_lib.PF_SUMS, dtype=torch.int64, device=dev)
        self.ancestors = torch.arange(N, dtype=torch.int32, device=dev)
        self.info = torch.zeros(_lib.PF_INFO_INTS, dtype=torch.int32, device=dev)
        self.draw_info = torch.zeros(_lib.PF_INFO_INTS, dtype=torch.int32, device=dev)      # [status, F, 0, 0] of the last draw from free cells
        self.moments = torch.zeros(_lib.PF_EST_DOUBLES, dtype=torch.float64, device=dev)
        self._ws = torch.empty(max(_lib.lib().icpmi_pf_workspace_bytes(N), 256), dtype=torch.uint8, device=dev)
        self._pairs = None                                         # the GridPairs of the last scan index: N entries, all that index
        self.last_sums = None
        self.last_rows = None                                      # the rows of the last weigh's scan, read back with its sums
        self.last_injected = 0                                     # the slots the last maybe_resample asked to inject

    # ── the map ──────────────────────────────────────────────────────────────
    def refresh_map(self):
        """Pack the grid's bit planes again (after the grid has changed); the free indexes of ``free_cells`` are dropped with
        the old planes.  Planes the caller gave are the caller's to renew."""
        if not self._own_planes:
            raise ValueError("this filter reads the caller's planes: pass new ones to a new filter")
        occupied, field = self._map_args
        self.planes, self.shift_bits = self.grid.occupancy_planes(occupied, field)
        self._free = {}
        return self

    def free_cells(self, box=None):
        """The ``FreeCells`` of the filter's planes: the cells that are neither occupied nor unknown, inside ``box`` = (x_lo,
        y_lo, x_hi, y_hi) in metres (None: the whole map).  The box becomes cells by world_to_cell — floor((w - min) /
        resolution) — and is half-open: the cells of x_hi and y_hi are outside.  Built once per box and kept until
        ``refresh_map()``."""
        g = self.grid
        if box is None:
            cells = (0, 0, g.nx, g.ny)
        else:
            b = np.asarray(box, dtype=np.float64).reshape(-1)
            if b.shape != (4,) or not np.isfinite(b).all():
                raise ValueError(f"box must be four finite numbers (x_lo, y_lo, x_hi, y_hi), got {box}")
            cell = lambda w, mn: int(np.clip(np.floor((w - mn) / g.resolution), -2 ** 31, 2 ** 31 - 1))       # noqa: E731
            cells = (cell(b[0], g.min_x), cell(b[1], g.min_y), cell(b[2], g.min_x), cell(b[3], g.min_y))
        if cells not in self._free:
            self._free[cells] = FreeCells(self.planes, cells)
        return self._free[cells]

    # ── the state ────────────────────────────────────────────────────────────
    @property
    def pair_t(self):
        return self._state[0]

    @property
    def theta(self):
        return self._state[1]

    @property
    def cos_sin(self):
        return self._state[2]

    def set_poses(self, poses):
        """The particles from the host: one pose [x, y, theta] for all of them, or (n, 3) rows.  cos and sin by NumPy.  The
        weights become uniform."""
        p = np.asarray(poses, dtype=np.float64)
        if p.shape not in ((3,), (1, 3), (self.n, 3)) or not np.isfinite(p).all():
            raise ValueError(f"poses must be one finite [x, y, theta] or ({self.n}, 3) rows of them")
        p = np.ascontiguousarray(np.broadcast_to(p.reshape(-1, 3), (self.n, 3)))
        dev = self.pair_t.device
        self.pair_t.copy_(torch.from_numpy(np.ascontiguousarray(p[:, :2])).to(dev))
        self.theta.copy_(torch.from_numpy(np.ascontiguousarray(p[:, 2])).to(dev))
        self.cos_sin.copy_(torch.from_numpy(np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], axis=1)).to(dev))
        self.w.fill_(1)
        return self

    def init_gaussian(self, pose, sigma3):
        """Every particle at ``pose``, then ``predict`` with no control and the deviations ``sigma3`` = (sigma_x, sigma_y,
        sigma_theta), x and y in the pose's own frame."""
        return self.set_poses(np.asarray(pose, dtype=np.float64).reshape(3)).predict((0.0, 0.0, 0.0), sigma3)

    def _draw(self, m, box, heading, span, ancestors):
        """``icpmi_pf_draw_uniform`` of ``m`` of the ``n`` slots of the present state at the present ``step``."""
        theta0, span = 0.0 if heading is None else float(heading), float(span)
        if not (math.isfinite(theta0) and 0.0 <= span <= TWO_PI):
            raise ValueError(f"heading must be finite and span lie in [0, 2 pi], got {heading}, {span}")
        free, g = self.free_cells(box), self.grid
        check(_lib.lib().icpmi_pf_draw_uniform(self.n, m, _ptr(free.index), g.min_x, g.min_y, g.resolution, theta0, span, _ptr(self.pair_t),
                                               _ptr(self.theta), _ptr(self.cos_sin), ancestors, _ptr(self.draw_info), self.seed, self.step,
                                               _stream()), "pf_draw_uniform")

    def enqueue_uniform(self, box=None, heading=None, span=TWO_PI):
        """Every particle drawn anew (``icpmi_pf_draw_uniform`` with m = n), nothing read back: uniformly over the free cells
        of ``box`` (of ``free_cells``; None: the whole map) and uniformly inside its cell, the heading uniform over ``span``
        radians about ``heading`` (None: about 0; the default span is the full circle).  The weights become uniform.
        Advances ``step``.  A region without a free cell leaves the particles where they were — the weights are uniform and
        the step has advanced all the same — and ``draw_info`` says so."""
        self._draw(self.n, box, heading, span, None)
        self.w.fill_(1)
        self.step += 1
        return self

    def init_uniform(self, box=None, heading=None, span=TWO_PI):
        """``enqueue_uniform``, then the draw's status read back: ``ValueError`` when the region has no free cell."""
        self.enqueue_uniform(box, heading, span)
        if int(self.draw_info[0].item()) == ST_NO_FREE:
            raise ValueError(f"no free cell in {'the map' if box is None else box}: the particles are where they were")
        return self

    def predict(self, control, sigma3):
        """``icpmi_pf_predict``: every particle moved by ``control`` = (dx, dy, dtheta) in the robot's frame plus noise of the
        deviations ``sigma3``; theta is not wrapped.  Advances ``step``."""
        u, s = (tuple(float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)) for a in (control, sigma3))
        if len(u) != 3 or len(s) != 3 or not np.isfinite(u + s).all() or min(s) < 0.0:
            raise ValueError(f"control and sigma3 must be three finite numbers each, no deviation below zero, got {control}, {sigma3}")
        check(_lib.lib().icpmi_pf_predict(self.n, _ptr(self.pair_t), _ptr(self.theta), _ptr(self.cos_sin), *u, *s, self.seed, self.step,
                                          _stream()), "pf_predict")
        self.step += 1
        return self

    # ── the measurement ──────────────────────────────────────────────────────
    def scan_pairs(self, cs, cloud):
        """Every particle of the present generation paired with cloud ``cloud`` of ``cs`` against the filter's planes -> the
        prepared ``gridmatch.MapPairs``, on the filter's own pose tensors.  The pair list is made once per scan index and
        kept: a fresh cloud set costs neither an upload nor a pass over the particles."""
        cloud = int(cloud)
        if self._pairs is None or int(self._pairs.clouds[0]) != cloud:
            self._pairs = gridmatch.GridPairs(np.full(self.n, cloud, dtype=np.int32), self.planes.buf.device)
        g = self.grid
        return gridmatch.MapPairs(self.planes, None, g.min_x, g.min_y, g.resolution, cs, self._pairs, self.pair_t, self.cos_sin)

    def beam(self, pairs):
        """Enqueue the beam model of ``scan_pairs``' call into ``records``, with the filter's table, half width and beyond."""
        return pairs.beam(self._beam_table, self.half_width, self.beyond, out=self.records)[0]

    def enqueue_weights(self, pairs):
        """The two launches of a measurement update on the current stream, nothing read back: the beam model of
        ``scan_pairs``' call into ``records``, then ``icpmi_pf_weights`` into ``w`` and ``sums``."""
        self.beam(pairs)
        check(_lib.lib().icpmi_pf_weights(self.n, _ptr(self.records), _ptr(self._weight_table), len(self.weight_table_host), self.weight_shift,
                                          _ptr(self.w), _ptr(self.sums), _stream()), "pf_weights")

    def _weigh(self, cs, cloud):
        """The beam model with every particle naming cloud ``cloud`` of ``cs``, then the weights -> (ess, OK records)."""
        self.enqueue_weights(self.scan_pairs(cs, cloud))
        # a filtered set keeps its counts on the device: the scan's rows are then one more word of the same read-back
        rows = None if cs.cnt is None else cs.cnt[cloud:cloud + 1].to(torch.int64)
        back = [int(v) for v in (self.sums if rows is None else torch.cat([self.sums, rows])).cpu().numpy()]      # the step's one synchronisation
        self.last_sums = back[:_lib.PF_SUMS]
        self.last_rows = int(cs.off_host[cloud + 1] - cs.off_host[cloud]) if rows is None else back[_lib.PF_SUMS]
        W, WW, ok = self.last_sums[_lib.PF_SUM_W], self.last_sums[_lib.PF_SUM_WW], self.last_sums[_lib.PF_SUM_OK]
        self.ess = W * W / WW if WW else 0.0
        return self.ess, ok

    def weigh(self, points_local, voxel_size=None):
        """The measurement update: ``points_local`` ((n, 2), sensor frame; through ``voxel_downsample`` when a size is given)
        scored at every particle by the beam model, the scores turned into the integer weights ``w``.  Reads the four sums
        back -> (ess = W^2 / sum w^2, the particles whose record is OK); ess is 0.0 when no particle has a weight."""
        return self._weigh(gridmatch.cloud_set_of([np.asarray(points_local, dtype=np.float64)], voxel_size), 0)

    def weigh_history(self, history, scan_id, voxel_size=None):
        """``weigh`` of a scan resident in an ``icpmi.ScanHistory``, by id: the rows are read where they are
        (``voxel_size`` chooses them as in ``OccupancyGrid2D.beam_history``)."""
        from .history import _scan_ids
        scan = _scan_ids(scan_id, ("scan_id", "scan ids"), history.n_scans, one=True)
        return self._weigh(self.grid._history_rows(history, voxel_size), scan)

    # ── resampling ───────────────────────────────────────────────────────────
    def resample(self, inject=0, box=None, heading=None, span=TWO_PI):
        """``icpmi_pf_resample``: systematic resampling by the weights of the last ``weigh``; ``ancestors`` names each new
        particle's parent, the weights become uniform.  Advances ``step``.  Does not synchronise (``degenerate()`` reads the
        status).  ``inject`` = m > 0: after the same resampling, m slots of the new generation, spread evenly, are drawn from
        the free cells instead (``icpmi_pf_draw_uniform`` at the same step — the purposes differ; ``box``, ``heading``,
        ``span`` of ``init_uniform``) and have ``INJECTED`` for an ancestor; ``draw_info`` holds that draw's status."""
        m = int(inject)
        if m != inject or not 0 <= m <= self.n:
            raise ValueError(f"inject must be a whole number in [0, {self.n}], got {inject}")
        out = self._spare
        check(_lib.lib().icpmi_pf_resample(self.n, _ptr(self.w), _ptr(self.pair_t), _ptr(self.theta), _ptr(self.cos_sin), _ptr(out[0]), _ptr(out[1]),
                                           _ptr(out[2]), _ptr(self.ancestors), _ptr(self.info), self.seed, self.step, _ptr(self._ws),
                                           self._ws.numel(), _stream()), "pf_resample")
        self._state, self._spare = out, self._state
        if m:
            self._draw(m, box, heading, span, _ptr(self.ancestors))
        self.w.fill_(1)
        self.step += 1
        return self

    def degenerate(self):
        """Whether the last ``resample`` found no weight at all (it then copied the particles unchanged).  Synchronises."""
        return int(self.info[0].item()) == ST_DEGENERATE

    def maybe_resample(self, threshold=0.5, recovery=None, **region):
        """``resample()`` when the last ``weigh``'s ess lies below ``threshold`` * n -> whether it did.  With a ``Recovery``:
        its ``update`` with the last ``weigh``'s best score and the scan's rows gives the share to inject, m = int(share * n)
        (``last_injected``), and the filter resamples when the ess is low or m > 0, with ``resample(inject=m, **region)``."""
        if self.last_sums is None:
            raise ValueError("maybe_resample needs the sums of a weigh() before it")
        m = 0
        if recovery is not None:
            m = int(recovery.update(self.last_sums[_lib.PF_SUM_SMAX], self.last_rows) * self.n)
        self.last_injected = m
        if not (self.ess < float(threshold) * self.n or m > 0):
            return False
        self.resample(inject=m, **region)
        return True

    # ── reading the filter ───────────────────────────────────────────────────
    def enqueue_estimate(self):
        """``icpmi_pf_estimate`` on the current stream, nothing read back -> ``moments``, the device tensor of the eight sums."""
        check(_lib.lib().icpmi_pf_estimate(self.n, _ptr(self.w), _ptr(self.pair_t), _ptr(self.cos_sin), _ptr(self.moments), _ptr(self._ws),
                                           self._ws.numel(), _stream()), "pf_estimate")
        return self.moments

    def estimate(self):
        """``icpmi_pf_estimate`` of the present particles and weights (synchronises) -> a dict: ``mean`` [x, y, theta] — the
        weighted means of x and y, theta = atan2(sum w sin, sum w cos) —, ``covariance`` (2, 2) of (x, y), ``resultant`` in
        [0, 1] (1: every heading equal) and ``sums``, the eight float64 sums themselves.  Every entry NaN but ``sums`` when no
        particle has a weight."""
        S = self.enqueue_estimate().cpu().numpy().copy()
        if not S[0] > 0.0:
            return {"mean": np.full(3, np.nan), "covariance": np.full((2, 2), np.nan), "resultant": float("nan"), "sums": S}
        W = S[0]
        mx, my = S[1] / W, S[2] / W
        cxy = S[6] / W - mx * my
        return {"mean": np.array([mx, my, np.arctan2(S[4], S[3])]), "covariance": np.array([[S[5] / W - mx * mx, cxy], [cxy, S[7] / W - my * my]]),
                "resultant": float(np.hypot(S[3], S[4]) / W), "sums": S}

    def poses(self):
        """The particles as (n, 3) float64 rows [x, y, theta] on the host (synchronises)."""
        return np.concatenate([self.pair_t.cpu().numpy(), self.theta.cpu().numpy()[:, None]], axis=1)

    def weights(self):
        """The integer weights as int64 [n] on the host (synchronises): the last ``weigh``'s, or ones after a resampling."""
        return self.w.cpu().numpy().astype(np.int64)
