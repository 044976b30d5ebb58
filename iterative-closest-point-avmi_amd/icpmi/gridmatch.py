"""Correlative scan-to-map matching: clouds scored against the occupancy grid itself over a window of rotations and
whole-cell shifts (``icpmi_grid_score_field``, ``icpmi_grid_match_batch``; the contract is include/icpmi.h's), and the same
search over a wide window (``icpmi_grid_bound_field``, ``icpmi_grid_search_batch``): blocks of shifts bounded from above by
a max-pooled field, pruned against a seed score, the exhaustive winner returned.  ``icpmi_grid_match_moments`` reads the
volume of a match once more: the integer-weighted moments of the candidates about the winner, from which
``gaussian_of_moments`` forms a sub-cell pose and a covariance on the host.  ``icpmi_grid_likelihood_field`` makes the field
the matchers read while the map's walls are one cell wide: the exact truncated distance to the nearest occupied cell
(``distance_field``), mapped to a score through a table (``likelihood_table``, ``likelihood_field``).  The cast reads the
same field back as ranges (``icpmi_grid_occupancy_planes``, ``icpmi_grid_cast_segments``, ``icpmi_grid_cast_rays``:
``occupancy_planes``, ``cast_segments``, ``cast_rays``): along the cells the map's update would lower, the first occupied
cell and the first unknown cell before it.  The check (``icpmi_grid_check_batch``: ``check_pairs``) walks measured beams over
the same planes, from the pose to the cell of each row's own hit, and counts per pair the beams the map confirms, the beams
that came back from behind a wall of the map, and the returns out of observed free or unexplored space.  The beam model
(``icpmi_grid_beam_batch``: ``beam_pairs``, ``beam_table``, ``pose_weights``) walks each beam a little past its own hit and
scores the signed steps between the map's first wall and the beam's return through a table: one number per pair that falls
smoothly where the check counts classes.

The reference registers a scan against a cloud only (slam.py:53-98, 111-183); this reads the map ``utilities.mapping``
builds.  The log-odds are quantised to int16 and a candidate's score is the integer sum of the field under the scan's
cells, so a result is the same bits whatever the launch looks like — and equal to a NumPy restatement of the contract.
The angles' cos / sin are computed here on the host with NumPy (as ``prealign.AngleTables`` does), and the pose of the
winner is formed on the host from the record: R from that cos / sin, t = predicted + whole cells.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .batch import CloudSet, _ptr, _stream, require_gpu

ST_OK, ST_EMPTY, ST_CAPACITY = _lib.GM_ST_OK, _lib.GM_ST_EMPTY, _lib.GM_ST_CAPACITY
MAX_WINDOW, MAX_ANGLES, MAX_ROWS = _lib.GM_MAX_WINDOW, _lib.GM_MAX_ANGLES, _lib.GM_MAX_ROWS
WIDE_MAX_WINDOW, WIDE_MAX_ANGLES, BLOCKS = _lib.GMW_MAX_WINDOW, _lib.GMW_MAX_ANGLES, (4, 8, 16)
LF_MAX_RADIUS = _lib.LF_MAX_RADIUS


def shift_bits(log_odds_min, log_odds_max):
    """The largest k in [0, GM_MAX_SHIFT_BITS] with max(|log_odds_min|, |log_odds_max|) * 2^k <= 32767 (0 when none is)."""
    m = max(abs(float(log_odds_min)), abs(float(log_odds_max)))
    for k in range(_lib.GM_MAX_SHIFT_BITS, 0, -1):
        if m * 2.0 ** k <= 32767.0:
            return k
    return 0


def score_field(log_odds, k, out=None):
    """``icpmi_grid_score_field`` of a float32 (ny, nx) device tensor -> the int16 (ny, nx) field (``out`` when given)."""
    ny, nx = log_odds.shape
    if log_odds.dtype != torch.float32 or not log_odds.is_contiguous():
        raise ValueError("log_odds must be a contiguous float32 (ny, nx) device tensor")
    if out is None:
        out = torch.empty((ny, nx), dtype=torch.int16, device=log_odds.device)
    check(_lib.lib().icpmi_grid_score_field(_ptr(log_odds), ny, nx, int(k), _ptr(out), _stream()), "grid_score_field")
    return out


def bound_field(field, block=8, out=None):
    """``icpmi_grid_bound_field`` of an int16 (ny, nx) device field -> the int16 (ny + block - 1, nx + block - 1) bound field:
    entry [y + block - 1, x + block - 1] is the largest field value in rows [y, y + block) and columns [x, x + block), cells
    outside the grid counting 0."""
    if block not in BLOCKS:
        raise ValueError(f"block must be one of {BLOCKS}, got {block}")
    if field.dtype != torch.int16 or field.dim() != 2 or not field.is_contiguous():
        raise ValueError("field must be a contiguous int16 (ny, nx) device tensor")
    ny, nx = field.shape
    if out is None:
        out = torch.empty((ny + block - 1, nx + block - 1), dtype=torch.int16, device=field.device)
    check(_lib.lib().icpmi_grid_bound_field(_ptr(field), ny, nx, int(block), _ptr(out), _stream()), "grid_bound_field")
    return out


def _int16_field(field, out, what):
    if field.dtype != torch.int16 or field.dim() != 2 or not field.is_contiguous():
        raise ValueError("field must be a contiguous int16 (ny, nx) device tensor")
    if out is None:
        return torch.empty_like(field)
    if out.dtype != torch.int16 or out.shape != field.shape or not out.is_contiguous() or out.device != field.device:
        raise ValueError(f"{what} must be a contiguous int16 tensor of the field's shape on its device")
    return out


def _radius(radius):
    R = int(radius)
    if R != radius or not 0 <= R <= LF_MAX_RADIUS:
        raise ValueError(f"radius must be a whole number of cells in [0, {LF_MAX_RADIUS}], got {radius}")
    return R


def distance_field(field, threshold, radius, out=None):
    """The exact squared distance, in cells, of every cell of an int16 (ny, nx) device field to the nearest occupied one —
    a cell with ``field >= threshold`` — where that is at most radius^2, and radius^2 + 1 elsewhere
    (``icpmi_grid_likelihood_field``'s ``d2_out``) -> an int16 (ny, nx) tensor (``out`` when given)."""
    R = _radius(radius)
    out = _int16_field(field, out, "out")
    ny, nx = field.shape
    check(_lib.lib().icpmi_grid_likelihood_field(_ptr(field), ny, nx, int(threshold), R, None, 0, _ptr(out), None, None, 0, _stream()),
          "grid_likelihood_field")
    return out


def likelihood_table(peak, sigma_cells, radius):
    """The int16 table of ``likelihood_field`` for a Gaussian of the distance: entry d2 — a SQUARED distance in cells — is
    rint(peak * exp(-d2 / (2 sigma_cells^2))), clipped to +-32767, formed in float64 on the host; radius^2 + 1 entries."""
    R = _radius(radius)
    if not float(sigma_cells) > 0.0:
        raise ValueError(f"sigma_cells must be positive, got {sigma_cells}")
    return np.clip(np.rint(peak * np.exp(-np.arange(R * R + 1) / (2 * sigma_cells**2))), -32767, 32767).astype(np.int16)


def likelihood_field(field, threshold, radius, table, keep_free=True, out=None, d2_out=None, workspace=None):
    """``icpmi_grid_likelihood_field``: ``table[d2]`` wherever ``distance_field``'s d2 is within the radius; beyond it
    min(field, 0) — the raw field's penalty for a hit in observed free space — with ``keep_free``, else 0.  ``table``: radius^2
    + 1 int16 on the host (``likelihood_table``), none of them -32768.  ``d2_out``: an int16 tensor that receives the distance
    field of the same launch; ``workspace``: a uint8 tensor of ``icpmi_grid_likelihood_workspace_bytes`` to use instead of
    a fresh one.  -> the int16 (ny, nx) field (``out`` when given), which every matcher takes as
    ``field=(tensor, k)`` and ``bound_field`` as its input."""
    R = _radius(radius)
    table = np.ascontiguousarray(table)
    if table.dtype != np.int16 or table.shape != (R * R + 1,):
        raise ValueError(f"table must hold radius^2 + 1 = {R * R + 1} int16, got {table.dtype} {table.shape}")
    if int(table.min()) == -32768:
        raise ValueError("the table holds -32768: the matchers' score bound needs |field| <= 32767")
    out = _int16_field(field, out, "out")
    if d2_out is not None:
        d2_out = _int16_field(field, d2_out, "d2_out")
    ny, nx = field.shape
    L = _lib.lib()
    need = L.icpmi_grid_likelihood_workspace_bytes(ny, nx, R)
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=field.device)
    if ws.dtype != torch.uint8 or ws.numel() < need or ws.device != field.device:
        raise ValueError(f"workspace must be a uint8 tensor of at least {need} bytes on the field's device")
    check(L.icpmi_grid_likelihood_field(_ptr(field), ny, nx, int(threshold), R, table.ctypes.data_as(C.c_void_p), int(bool(keep_free)),
                                        None if d2_out is None else _ptr(d2_out), _ptr(out), _ptr(ws), ws.numel(), _stream()),
          "grid_likelihood_field")
    return out


class OccupancyPlanes:
    """What ``occupancy_planes`` returns and the casts take instead of a field: ``buf``, the uint8 device buffer of the two
    bit planes (occupied, unknown; include/icpmi.h has the layout), with the grid's ``ny``, ``nx`` and the ``threshold`` they
    were packed with.  Kept by the caller, they show the map as it was when they were made."""

    def __init__(self, buf, ny, nx, threshold):
        self.buf, self.ny, self.nx, self.threshold = buf, int(ny), int(nx), int(threshold)


def _cast_grid(ny, nx):
    if max(ny, nx) > 2 ** 29 or ny * nx >= 2 ** 31:
        raise ValueError(f"a grid of {ny} x {nx} cells cannot be cast: at most 2^29 per axis and fewer than 2^31 cells")


def occupancy_planes(field, threshold):
    """``icpmi_grid_occupancy_planes`` of an int16 (ny, nx) device field: one bit per cell for "occupied" — ``field >=
    threshold`` — and one for "unknown" — ``field == 0`` -> ``OccupancyPlanes``, for ``cast_segments`` and ``cast_rays``."""
    if not isinstance(field, torch.Tensor) or field.dtype != torch.int16 or field.dim() != 2 or not field.is_contiguous():
        raise ValueError("field must be a contiguous int16 (ny, nx) device tensor")
    ny, nx = field.shape
    _cast_grid(ny, nx)
    L = _lib.lib()
    buf = torch.empty(L.icpmi_grid_occupancy_planes_bytes(ny, nx), dtype=torch.uint8, device=field.device)
    check(L.icpmi_grid_occupancy_planes(_ptr(field), ny, nx, int(threshold), _ptr(buf), buf.numel(), _stream()), "grid_occupancy_planes")
    return OccupancyPlanes(buf, ny, nx, threshold)


def _cast_source(field_or_planes, threshold):
    """-> (field, planes buffer, workspace, ny, nx, threshold, device) as the cast entries take them: kept planes as they
    are, a field with a workspace the entry packs it into."""
    if isinstance(field_or_planes, OccupancyPlanes):
        p = field_or_planes
        return None, p.buf, None, p.ny, p.nx, p.threshold, p.buf.device
    f = field_or_planes
    if not isinstance(f, torch.Tensor) or f.dtype != torch.int16 or f.dim() != 2 or not f.is_contiguous():
        raise ValueError("the map must be a contiguous int16 (ny, nx) device field or the OccupancyPlanes of one")
    ny, nx = f.shape
    _cast_grid(ny, nx)
    ws = torch.empty(_lib.lib().icpmi_grid_occupancy_planes_bytes(ny, nx), dtype=torch.uint8, device=f.device)
    return f, None, ws, ny, nx, int(threshold), f.device


def _cast_out(out, shape, dev):
    if out is None:
        return torch.empty(shape, dtype=torch.int32, device=dev)
    if out.dtype != torch.int32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous int32 tensor of shape {tuple(shape)} on the map's device")
    return out


def _rows_f64(rows, cols, what, dev, n=None):
    t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, cols)))
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != cols or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what} must be float64 rows of {cols}" + (f", {n} of them" if n is not None else ""))
    return t.to(dev).contiguous()


def cast_segments(field_or_planes, threshold, segs, out=None):
    """``icpmi_grid_cast_segments``: the (n, 4) int32 cell segments (x0, y0, x1, y1), each coordinate within +-2^29, walked over
    an int16 (ny, nx) device field (occupied: ``field >= threshold``) or over kept ``OccupancyPlanes`` (``threshold`` is then
    the planes' own) -> the (n, GC_INTS) int32 device tensor of records [k_hit, x_hit, y_hit, k_unknown] (``out`` when given).
    Enqueues and does not synchronise."""
    field, planes, ws, ny, nx, thr, dev = _cast_source(field_or_planes, threshold)
    if not isinstance(segs, torch.Tensor):
        host = np.asarray(segs)
        if host.dtype.kind not in "iu" or host.ndim != 2 or host.shape[1] != 4:
            raise ValueError("segs must be (n, 4) integer rows (x0, y0, x1, y1)")
        if host.size and np.abs(host.astype(np.int64)).max() > 2 ** 29:
            raise ValueError("a segment's coordinates must lie within +-2^29 cells")
        segs = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32))
    if segs.dtype != torch.int32 or segs.dim() != 2 or segs.shape[1] != 4:
        raise ValueError("segs must be (n, 4) int32 rows (x0, y0, x1, y1)")
    n = segs.shape[0]
    if n >= 2 ** 29:
        raise ValueError(f"{n} segments: fewer than 2^29 fit one call")
    segs = segs.to(dev).contiguous()
    out = _cast_out(out, (n, _lib.GC_INTS), dev)
    check(_lib.lib().icpmi_grid_cast_segments(_ptr(field), _ptr(planes), ny, nx, thr, _ptr(segs), n, _ptr(out), _ptr(ws),
                                              0 if ws is None else ws.numel(), _stream()), "grid_cast_segments")
    return out


def cast_rays(field_or_planes, threshold, min_x, min_y, resolution, poses_xy, pose_cs, beam_cs, reach, out=None):
    """``icpmi_grid_cast_rays``: from every pose — ``poses_xy`` (P, 2) in metres, ``pose_cs`` (P, 2) the (cos, sin) of its
    heading — along every beam — ``beam_cs`` (A, 2), the (cos, sin) of its bearing in the sensor frame — to ``reach`` metres,
    over the map as ``cast_segments`` takes it -> the (P, A, GC_INTS) int32 device tensor of records (``out`` when given).
    The rows are the caller's own float64 (arrays or device tensors).  Enqueues and does not synchronise."""
    field, planes, ws, ny, nx, thr, dev = _cast_source(field_or_planes, threshold)
    for name, v in (("resolution", resolution), ("reach", reach)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    xy = _rows_f64(poses_xy, 2, "poses_xy", dev)
    P = xy.shape[0]
    pcs, bcs = _rows_f64(pose_cs, 2, "pose_cs", dev, P), _rows_f64(beam_cs, 2, "beam_cs", dev)
    A = bcs.shape[0]
    if P * A >= 2 ** 29:
        raise ValueError(f"{P} poses x {A} beams: fewer than 2^29 rays fit one call")
    out = _cast_out(out, (P, A, _lib.GC_INTS), dev)
    check(_lib.lib().icpmi_grid_cast_rays(_ptr(field), _ptr(planes), ny, nx, thr, float(min_x), float(min_y), float(resolution),
                                          _ptr(xy), _ptr(pcs), P, _ptr(bcs), A, float(reach), _ptr(out), _ptr(ws),
                                          0 if ws is None else ws.numel(), _stream()), "grid_cast_rays")
    return out


class GridPairs:
    """The pair list every pair entry takes: ``host`` (int32 [B], the cloud of each pair), ``dev`` (its device copy, made
    here, once) and what the checks need of it: ``clouds``, the different clouds it names in rising order, and ``times``, the
    pairs that name each.  ``on(cloud_set)`` judges the list against a cloud set from those two alone — no pass over the B
    entries, no upload — so one list serves every cloud set that has the clouds it names."""

    def __init__(self, pair_clouds, device):
        self.host = np.ascontiguousarray(pair_clouds, dtype=np.int32).reshape(-1)
        self.B = len(self.host)
        self.clouds, self.times = np.unique(self.host, return_counts=True)
        self._ends = self.clouds + 1                               # (the named clouds' entries of a set's offsets, for ``on``)
        self._host_ptr = C.c_void_p(self.host.ctypes.data)
        self.dev = torch.from_numpy(self.host).to(device)

    @classmethod
    def of(cls, pair_clouds, device):
        """``pair_clouds`` itself when it is a GridPairs already, else a new one on ``device``."""
        return pair_clouds if isinstance(pair_clouds, cls) else cls(pair_clouds, device)

    def on(self, cs):
        """The refusals of a pair list against the grid — a 2-D cloud set on the list's device, every pair naming one of its
        clouds, none of them above ``MAX_ROWS`` rows -> (the rows of the largest named cloud, the rows of all pairs)."""
        if cs.dim != 2:
            raise ValueError("pairs against the grid are 2-D")
        if cs.pts.device != self.dev.device:
            raise ValueError(f"the clouds live on {cs.pts.device}, the pair list on {self.dev.device}")
        if not self.B:
            return 0, 0
        if self.clouds[0] < 0 or self.clouds[-1] >= cs.n_clouds:
            raise ValueError("pair_clouds must index the cloud set")
        named = cs.off_host[self._ends] - cs.off_host[self.clouds]
        stride = int(named.max())
        if stride > MAX_ROWS:
            raise ValueError(f"a cloud above {MAX_ROWS} rows cannot be scored (int32 sums): filter it first")
        return stride, int(named @ self.times)                      # (int32 rows by int64 times: an int64 sum)

    def args(self, cs):
        """The pair-list arguments of the four C entries (``pts`` ... ``n_pairs``) for this list on ``cs``."""
        return (_ptr(cs.pts), _ptr(cs.off), C.c_void_p(cs.off_host.ctypes.data), _ptr(cs.cnt), cs.n_clouds, _ptr(self.dev),
                self._host_ptr, self.B)


class MapPairs:
    """Pairs of a cloud set against a map, checked and uploaded once and then run many times: what ``check_pairs`` and
    ``beam_pairs`` prepare on every call.  The arguments are theirs.  The object holds what its C calls point into — the
    planes, or the field with the workspace it is packed into; the cloud set's tensors; the pair list (``pairs``, a
    ``GridPairs``; one given as ``pair_clouds`` is used as it is); the pose tensors ``t`` and ``rot`` — with ``B``, ``stride``
    (the rows of the largest named cloud) and ``dev``.  float64 contiguous pose tensors on the map's device are used in place,
    and ``point_at`` aims the same object at another pair of them.  ``head`` is what the two C entries begin with (``field`` ...
    ``cos_sin``), ``tail()`` what they end with (workspace, bytes, stream): the stream is the current one of every call."""

    def __init__(self, field_or_planes, threshold, min_x, min_y, resolution, cloud_set, pair_clouds, translations, cos_sin):
        self.field, self.planes, self.ws, self.ny, self.nx, self.threshold, self.dev = _cast_source(field_or_planes, threshold)
        cs = self.cs = cloud_set
        if cs.pts.device != self.dev:
            raise ValueError(f"the clouds live on {cs.pts.device}, the map on {self.dev}")
        self.world = (float(min_x), float(min_y), float(resolution))
        if not (all(map(math.isfinite, self.world)) and resolution > 0.0):
            raise ValueError(f"resolution must be positive and finite and the map's corner finite, got {resolution}, ({min_x}, {min_y})")
        self.pairs = GridPairs.of(pair_clouds, self.dev)
        self.stride, rows = self.pairs.on(cs)
        if rows >= 2 ** 29:
            raise ValueError(f"{rows} rows: fewer than 2^29 fit one call")
        self.B = self.pairs.B
        self._clouds = (cs.pts, cs.off, cs.off_host, cs.cnt)       # head points into these, whatever becomes of the set
        self.point_at(translations, cos_sin)

    def point_at(self, translations, cos_sin):
        """Aim the calls at these poses (B rows of 2 each, as the constructor takes them) -> self.  Nothing else is looked at
        again: the pair list is neither checked nor uploaded."""
        self.t, self.rot = _rows_f64(translations, 2, "translations", self.dev, self.B), _rows_f64(cos_sin, 2, "cos_sin", self.dev, self.B)
        self.head = (_ptr(self.field), _ptr(self.planes), self.ny, self.nx, self.threshold, *self.world, *self.pairs.args(self.cs),
                     _ptr(self.t), _ptr(self.rot))
        return self

    def tail(self):
        return _ptr(self.ws), 0 if self.ws is None else self.ws.numel(), _stream()

    def check(self, tolerance, want_rows=False, out=None):
        """``check_pairs`` of the prepared pairs -> (records, rows).  With ``out`` given, nothing is allocated."""
        tol = int(tolerance)
        if tol != tolerance or not 0 <= tol <= _lib.GK_MAX_TOLERANCE:
            raise ValueError(f"tolerance must be a whole number of steps in [0, 2^30], got {tolerance}")
        rec_out, rows_out = (out if want_rows else (out, None)) if out is not None else (None, None)
        records = _cast_out(rec_out, (self.B, _lib.GK_INTS), self.dev)
        rows = _cast_out(rows_out, (self.B, self.stride, _lib.GK_ROW_INTS), self.dev) if want_rows else None
        check(_lib.lib().icpmi_grid_check_batch(*self.head, tol, _ptr(records), _ptr(rows), self.stride, *self.tail()), "grid_check")
        return records, rows

    def beam(self, table, half_width, beyond, want_hist=False, want_rows=False, out=None):
        """``beam_pairs`` of the prepared pairs -> (records, hist, rows).  An int32 [2H + 3] ``table`` on the map's device is
        read where it is; with ``out`` given as well, nothing is allocated."""
        H = int(half_width)
        if H != half_width or not 0 <= H <= _lib.GB_MAX_HALF_WIDTH:
            raise ValueError(f"half_width must be a whole number in [0, {_lib.GB_MAX_HALF_WIDTH}], got {half_width}")
        if not (math.isfinite(beyond) and beyond >= 0.0):
            raise ValueError(f"beyond must be finite and not negative, got {beyond}")
        if not isinstance(table, torch.Tensor):
            host = np.asarray(table)
            if host.dtype.kind not in "iu" or host.size and np.abs(host.astype(np.int64)).max() >= 2 ** 31:
                raise ValueError("table must hold int32 entries")
            table = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32))
        if table.dtype != torch.int32 or tuple(table.shape) != (2 * H + 3,):
            raise ValueError(f"table must be int32 [{2 * H + 3}] for a half width of {H}, got {table.dtype} {tuple(table.shape)}")
        table = table.to(self.dev).contiguous()
        rec_out, hist_out, rows_out = (out, None, None) if out is None or isinstance(out, torch.Tensor) else out
        records = _cast_out(rec_out, (self.B, _lib.GB_INTS), self.dev)
        hist = _cast_out(hist_out, (self.B, 2 * H + 3), self.dev) if want_hist else None
        rows = _cast_out(rows_out, (self.B, self.stride, _lib.GB_ROW_INTS), self.dev) if want_rows else None
        check(_lib.lib().icpmi_grid_beam_batch(*self.head, float(beyond), H, _ptr(table), _ptr(records), _ptr(hist), _ptr(rows), self.stride,
                                               *self.tail()), "grid_beam")
        return records, hist, rows


def check_pairs(field_or_planes, threshold, min_x, min_y, resolution, cloud_set, pair_clouds, translations, cos_sin, tolerance,
                want_rows=False, out=None):
    """``icpmi_grid_check_batch``: pair b holds cloud ``pair_clouds[b]`` of ``cloud_set`` (sensor frame, 2-D) at the
    translation ``translations[b]`` and the rotation ``cos_sin[b]`` = (cos, sin) against the map as ``cast_segments`` takes it.
    Every row's beam is walked from the pose's cell to the cell of its own hit and falls in one class (include/icpmi.h):
    confirmed — the map has a wall within ``tolerance`` steps of the beam's end —, violated — the beam came back from behind
    a wall of the map —, in free space or unexplored.  -> (records, rows): the (B, GK_INTS) int32 device tensor of records
    [status, rows with cells, confirmed, violated, in_free, unexplored, through_unknown, 0] and, with ``want_rows``, the (B,
    stride, GK_ROW_INTS) int32 device tensor of [class, k_hit, K, k_unknown] per row (else None) — stride the largest named
    cloud; what lies at or behind a cloud's count is not written.  ``out``: a records tensor, or with ``want_rows`` the pair
    (records, rows), to write into.  The rows are the caller's own float64 (arrays or device tensors).  Enqueues and does not
    synchronise."""
    return MapPairs(field_or_planes, threshold, min_x, min_y, resolution, cloud_set, pair_clouds, translations, cos_sin).check(
        tolerance, want_rows, out)


def beam_table(resolution, sigma, half_width, z_hit=0.8, z_short=0.1, z_rand=0.1, unexplored=None, scale=1024):
    """The table ``beam_pairs`` reads, from the beam model's mixture: for a difference of d steps, d = -half_width ...
    half_width, p(d) = z_hit * exp(-(d * resolution)^2 / (2 sigma^2)) + z_short * [d > 0] + z_rand — a Gaussian about the
    map's wall, a floor for returns short of it (something in the way) and a floor for anything at all; the two tail entries
    (a return out of observed free space with no wall near, a return from unexplored space) are z_short + z_rand, the
    last one ``unexplored`` when that is given.  An entry is max(-32767, rint(scale * ln(p / max p))): 0 at the best
    difference, negative elsewhere -> int32 [2 * half_width + 3].  ``resolution`` and ``sigma`` in metres; a step is a cell
    along the beam's major axis, so on a diagonal the same table is up to sqrt(2) wider in metres."""
    H = int(half_width)
    if H != half_width or not 0 <= H <= _lib.GB_MAX_HALF_WIDTH:
        raise ValueError(f"half_width must be a whole number in [0, {_lib.GB_MAX_HALF_WIDTH}], got {half_width}")
    if not (np.isfinite(resolution) and resolution > 0.0 and np.isfinite(sigma) and sigma > 0.0 and np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"resolution, sigma and scale must be positive and finite, got {resolution}, {sigma}, {scale}")
    tail = z_short + z_rand
    weights = [z_hit, z_short, z_rand, tail if unexplored is None else unexplored]
    if not all(np.isfinite(w) and w >= 0.0 for w in weights) or not z_hit + z_rand > 0.0:
        raise ValueError("the mixture's weights must be finite and not negative, and z_hit + z_rand positive")
    d = np.arange(-H, H + 1, dtype=np.float64)
    p = z_hit * np.exp(-(d * resolution) ** 2 / (2.0 * float(sigma) ** 2)) + z_short * (d > 0) + z_rand
    p = np.concatenate([p, [tail, weights[3]]])
    with np.errstate(divide="ignore"):
        return np.maximum(-float(_lib.GB_TABLE_CLIP), np.rint(scale * np.log(p / p.max()))).astype(np.int32)


def pose_weights(score, temperature=1.0, scale=1024, status=None):
    """Scores of ``beam_pairs`` (made with a table of that ``scale``) as normalised weights, in NumPy on the host:
    w = softmax(score / (scale * temperature)), computed about the maximum, and the effective sample size ess = 1 / sum(w^2)
    -> (w float64, ess).  ``temperature`` > 1 flattens the weights: the beams of a scan are not independent, and a filter
    that multiplies hundreds of them as if they were collapses onto one particle.  ``status``: the records' statuses; a pose
    whose status is not OK gets weight 0 (all of them: every weight 0 and ess 0.0)."""
    s = np.asarray(score, dtype=np.float64).reshape(-1)
    if not (np.isfinite(temperature) and temperature > 0.0 and np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"temperature and scale must be positive and finite, got {temperature}, {scale}")
    keep = np.ones(len(s), dtype=bool) if status is None else np.asarray(status).reshape(-1) == _lib.GB_ST_OK
    if len(keep) != len(s):
        raise ValueError(f"{len(s)} scores but {len(keep)} statuses")
    w = np.zeros(len(s))
    if not keep.any():
        return w, 0.0
    z = s[keep] / (float(scale) * float(temperature))
    e = np.exp(z - z.max())
    w[keep] = e / e.sum()
    return w, float(1.0 / np.sum(w * w))


def beam_pairs(field_or_planes, threshold, min_x, min_y, resolution, cloud_set, pair_clouds, translations, cos_sin, table, half_width,
               beyond, want_hist=False, want_rows=False, out=None):
    """``icpmi_grid_beam_batch``: the beam model.  Pair b holds cloud ``pair_clouds[b]`` of ``cloud_set`` (sensor frame, 2-D)
    at the translation ``translations[b]`` and the rotation ``cos_sin[b]`` = (cos, sin) against the map as ``cast_segments``
    takes it.  Every row's beam is walked from the pose's cell through the cell of its own hit to a far end ``beyond`` metres
    behind it; k_hit is the step of the map's first occupied cell on that walk and k_z the step at which the beam returned,
    both on the walk's major axis.  The row adds ``table[i]`` (clipped to +-32767) to the pair's score, i =
    clamp(k_hit - k_z, -H, H) + H where the map has a wall on the walk (positive differences: the beam came back short of
    it; negative: from behind it), else 2H + 1 for a return out of observed free space and 2H + 2 for one from unexplored
    space or off the grid; H = ``half_width``, ``table`` int32 [2H + 3] (``beam_table``; an array or a device tensor).
    Differences are in steps along the major axis — cells along an axis, up to sqrt(2) cells in metres along a diagonal —
    as the check's tolerance is.  -> (records, hist, rows): the (B, GB_INTS) int32 device tensor of records [status, rows
    with cells, score, expected (rows with k_hit >= 0), novel (index 2H + 1), unexplored (index 2H + 2), 0, 0]; with
    ``want_hist`` the (B, 2H + 3) int32 rows per index (else None); with ``want_rows`` the (B, stride, GB_ROW_INTS) int32
    [i, k_hit, k_z, k_unknown] per row (else None) — stride the largest named cloud, a row without cells is [GB_NO_CELLS, 0,
    0, -1], and what lies at or behind a cloud's count is not written.  ``out``: a records tensor, or the triple (records,
    hist, rows) with None for what is not asked for, to write into.  The rows are the caller's own float64 (arrays or device
    tensors).  Enqueues and does not synchronise."""
    return MapPairs(field_or_planes, threshold, min_x, min_y, resolution, cloud_set, pair_clouds, translations, cos_sin).beam(
        table, half_width, beyond, want_hist, want_rows, out)


def ray_end_cells(min_x, min_y, resolution, poses_xy, pose_cs, beam_cs, reach):
    """The origin and end cells ``icpmi_grid_cast_rays`` forms, in NumPy on the host with the same float64 operations ->
    (segments (P, A, 4) int64 [x0, y0, x1, y1], clamped to +-2^29; has_cells (P, A) bool)."""
    xy, pcs, bcs = (np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in (poses_xy, pose_cs, beam_cs))
    px, py, ct, st = xy[:, None, 0], xy[:, None, 1], pcs[:, None, 0], pcs[:, None, 1]
    ca, sa = bcs[None, :, 0], bcs[None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        c, s = ct * ca - st * sa, st * ca + ct * sa
        ex, ey = px + reach * c, py + reach * s
        f = [np.floor((np.broadcast_to(w, ex.shape) - m) / resolution) for w, m in ((px, min_x), (py, min_y), (ex, min_x), (ey, min_y))]
        ok = np.all([np.abs(v) < 1e300 for v in f], axis=0)
        seg = np.stack([np.clip(np.where(ok, v, 0.0), -2.0 ** 29, 2.0 ** 29).astype(np.int64) for v in f], axis=-1)
    return seg, ok


def step_cells(segs, k):
    """The cell of step ``k`` of every segment of ``segs`` (..., 4) — include/icpmi.h's closed form, in NumPy int64 ->
    (x, y); ``k`` outside [0, K] gives the cell the formula gives."""
    segs, k = np.asarray(segs, dtype=np.int64), np.asarray(k, dtype=np.int64)
    x0, y0, x1, y1 = (segs[..., i] for i in range(4))
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.where(x0 < x1, 1, -1), np.where(y0 < y1, 1, -1)
    xmajor = dx >= dy
    dmaj, dmin = np.where(xmajor, dx, dy), np.where(xmajor, dy, dx)
    q = (2 * k * dmin + dmaj - 1) // np.maximum(2 * dmaj, 1)
    q = np.where(dmaj > 0, q, 0)
    return np.where(xmajor, x0 + sx * k, x0 + sx * q), np.where(xmajor, y0 + sy * q, y0 + sy * k)


def angle_grid(theta, angular_window, angular_step):
    """theta + np.deg2rad(np.arange(-range, range + step, step)), the expression of slam.py:146-148, for every theta
    -> (angles [B, A], index of the offset nearest to zero)."""
    offsets = np.deg2rad(np.arange(-angular_window, angular_window + angular_step, angular_step))
    if len(offsets) == 0:
        raise ValueError("the angle grid is empty: angular_window and angular_step must be positive")
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    return theta[:, None] + offsets[None, :], int(np.argmin(np.abs(offsets)))


def half_step(half_log_odds, k):
    """``half_log_odds`` — the drop of the mean log-odds under a scan's hits that halves a candidate's weight — in the field
    units of shift ``k``: int(np.rint(half_log_odds * 2^k)), the ``half_step`` of ``icpmi_grid_match_moments``.  ValueError
    unless it lies in [1, GMOM_MAX_HALF_STEP]."""
    h = int(np.rint(float(half_log_odds) * 2.0 ** int(k)))
    if not 1 <= h <= _lib.GMOM_MAX_HALF_STEP:
        raise ValueError(f"half_log_odds {half_log_odds} at shift {k} is a half_step of {h}, outside [1, {_lib.GMOM_MAX_HALF_STEP}]")
    return h


def match_moments(volume, records, n_pairs, n_angles, window, half_step, out=None):
    """``icpmi_grid_match_moments`` of a match's (B, A, S, S) int32 device volume and its (B, 8) int32 device records, as
    ``GridMatchBatch.run()`` left them on the current stream -> the (B, GMOM_INTS) int64 device tensor of moments (``out``
    when given).  Enqueues and does not synchronise."""
    S = 2 * int(window) + 1
    for name, ten, cols in (("volume", volume, n_angles * S * S), ("records", records, _lib.GMREC_INTS)):
        if ten.dtype != torch.int32 or not ten.is_contiguous() or ten.numel() < n_pairs * cols:
            raise ValueError(f"{name} must be a contiguous int32 device tensor of at least {n_pairs} x {cols} values")
    if out is None:
        out = torch.empty((max(n_pairs, 1), _lib.GMOM_INTS), dtype=torch.int64, device=volume.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() < n_pairs * _lib.GMOM_INTS:
        raise ValueError(f"out must be a contiguous int64 device tensor of at least {n_pairs} x {_lib.GMOM_INTS} values")
    check(_lib.lib().icpmi_grid_match_moments(_ptr(volume), _ptr(records), int(n_pairs), int(n_angles), int(window), int(half_step),
                                              _ptr(out), _stream()), "grid_match_moments")
    return out


def gaussian_of_moments(moments, resolution, angular_step):
    """The Gaussian a (B, GMOM_INTS) integer array of moments describes, in NumPy on the host -> a dict:

    ``offset`` (B, 3): (resolution * mu_I, resolution * mu_J, angular_step * mu_A), the weighted mean of the candidates
    relative to the winner, mu_X = M_X / M_W; ``covariance`` (B, 3, 3), symmetric, of the pose's own parameters (t_x, t_y,
    theta) with world = R(theta) p + t: the index-unit central moments (M_XY M_W - M_X M_Y) / M_W^2 — the numerator formed
    exactly in Python integers, one float64 division — plus 1/12 on the diagonal (a candidate is a bin one cell or one step
    wide, so a single surviving candidate does not claim zero variance), reordered to [x, y, theta] = [I, J, A] and scaled by
    diag(resolution, resolution, angular_step); ``support`` (B,), the candidates with a non-zero weight; ``edge_weight``
    (B,), the share of the weight on the faces of the volume — near 1 the window cut the distribution off.

    ``angular_step``: radians, one value or one per pair.  A search over one angle has no step: pass 0, and the theta row
    and column of the covariance and the theta offset are zero.  A pair with M_W = 0 (``ST_CAPACITY``: nothing was read) gets
    NaN offset, covariance and edge_weight."""
    M = np.asarray(moments).reshape(-1, _lib.GMOM_INTS)
    B = len(M)
    res = float(resolution)
    steps = np.broadcast_to(np.asarray(angular_step, dtype=np.float64), (B,))
    first = (_lib.GMOM_I, _lib.GMOM_J, _lib.GMOM_A)                                   # [x, y, theta] = [I, J, A]
    second = ((_lib.GMOM_II, _lib.GMOM_JI, _lib.GMOM_AI), (_lib.GMOM_JI, _lib.GMOM_JJ, _lib.GMOM_AJ), (_lib.GMOM_AI, _lib.GMOM_AJ, _lib.GMOM_AA))
    offset, cov, edge = np.full((B, 3), np.nan), np.full((B, 3, 3), np.nan), np.full(B, np.nan)
    for b in range(B):
        m = [int(v) for v in M[b]]
        W = m[_lib.GMOM_W]
        if W == 0:
            continue
        D = (res, res, float(steps[b]))
        for p in range(3):
            offset[b, p] = D[p] * (float(m[first[p]]) / float(W))
            for q in range(p, 3):
                central = float(m[second[p][q]] * W - m[first[p]] * m[first[q]]) / float(W * W)
                cov[b, p, q] = cov[b, q, p] = (D[p] * D[q]) * (central + (1.0 / 12.0 if p == q else 0.0))
        edge[b] = float(m[_lib.GMOM_EDGE]) / float(W)
    return {"offset": offset, "covariance": cov, "support": M[:, _lib.GMOM_SUPPORT].astype(np.int64), "edge_weight": edge}


class GridMatchBatch:
    """Pair b: cloud ``pair_clouds[b]`` of ``cloud_set`` scored against ``grid`` at the translation ``translations[b]``
    under the rotations ``angle_rows[b]`` (radians, [B, A]) and every shift of whole cells within ``window``.

    ``grid``: anything with ``device_log_odds`` (float32 (ny, nx) device tensor), ``min_x``, ``min_y``, ``resolution``,
    ``log_odds_min`` and ``log_odds_max`` — a ``utilities.mapping.OccupancyGrid2D``.  ``field``: a ``(tensor, k)`` an earlier
    ``score_field`` returned, to score against the map as it was then; ``None``: the field is rebuilt by every ``run()``.
    ``run()`` enqueues the launches on the current stream and returns the (B, 8) int32 record tensor, without a
    synchronisation; ``want_scores``: ``scores`` then holds the full (B, A, S, S) int32 volume.  ``unpack()`` reads the
    records back and forms the poses.

    ``half_log_odds`` (None: off): ``run()`` also enqueues ``match_moments`` of the volume into ``moments``, with
    ``half_step(half_log_odds, k)``, and ``unpack()`` adds the sub-cell pose and its covariance to ``info``.  The volume is
    then kept as with ``want_scores``, and every angle row must be evenly spaced (its step scales the theta moments)."""

    def __init__(self, grid, cloud_set, pair_clouds, translations, angle_rows, window, centre_angle=-1, field=None, want_scores=False,
                 half_log_odds=None):
        self._setup(grid, cloud_set, pair_clouds, translations, angle_rows, window, centre_angle, field, MAX_WINDOW, MAX_ANGLES)
        B, dev = self.B, cloud_set.pts.device
        self.half_step = self.moments = None
        if half_log_odds is not None:
            self.half_step = half_step(half_log_odds, self.k)
            gaps = np.diff(self.angles, axis=1)
            if self.A > 1 and not all(np.allclose(g, g.mean()) for g in gaps):
                raise ValueError("half_log_odds needs evenly spaced angle rows: the step scales the moments in theta")
            self.angular_step = (self.angles[:, -1] - self.angles[:, 0]) / (self.A - 1) if self.A > 1 else np.zeros(B)
            self.moments = torch.zeros((max(B, 1), _lib.GMOM_INTS), dtype=torch.int64, device=dev)
            want_scores = True
        self.records = torch.zeros((max(B, 1), _lib.GMREC_INTS), dtype=torch.int32, device=dev)
        self.scores = torch.zeros((max(B, 1), self.A, self.S, self.S), dtype=torch.int32, device=dev) if want_scores else None
        need = _lib.lib().icpmi_grid_match_workspace_bytes(B, self.A, self.W)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)

    def _setup(self, grid, cloud_set, pair_clouds, translations, angle_rows, window, centre_angle, field, max_window, max_angles):
        """The pairs, their angles and the refusals the two searches share; everything but the outputs and the workspace."""
        require_gpu()
        self.grid, self.cs, self.field = grid, cloud_set, field
        dev = cloud_set.pts.device
        self.pairs = GridPairs.of(pair_clouds, dev)
        self.pairs.on(cloud_set)
        self.B = B = self.pairs.B
        self.t_host = np.ascontiguousarray(np.asarray(translations, dtype=np.float64).reshape(B, 2))
        self.angles = np.ascontiguousarray(np.asarray(angle_rows, dtype=np.float64).reshape(B, -1))
        self.A, self.W, self.centre_angle = self.angles.shape[1], int(window), int(centre_angle)
        self.S = 2 * self.W + 1
        if not 0 <= self.W <= max_window:
            raise ValueError(f"window must lie in [0, {max_window}] cells, got {self.W}")
        if not 1 <= self.A <= max_angles:
            raise ValueError(f"between 1 and {max_angles} angles per pair, got {self.A}")
        if self.centre_angle >= self.A:
            raise ValueError("centre_angle must be negative (none) or an index into the angle rows")
        self.cos_sin_host = np.ascontiguousarray(np.stack([np.cos(self.angles), np.sin(self.angles)], axis=2))
        self.t = torch.from_numpy(self.t_host).to(dev)
        self.cos_sin = torch.from_numpy(self.cos_sin_host).to(dev)
        self.k = shift_bits(grid.log_odds_min, grid.log_odds_max) if field is None else int(field[1])
        self._field_buf = None

    def _field(self):
        """The field a run scores against: the caller's, or the grid's log-odds quantised now."""
        lo = self.grid.device_log_odds
        if self.field is not None:
            fld = self.field[0]
            if tuple(fld.shape) != tuple(lo.shape) or fld.dtype != torch.int16:
                raise ValueError("field must be the int16 (ny, nx) tensor score_field() returned for this grid")
            return fld
        self._field_buf = score_field(lo, self.k, self._field_buf)
        return self._field_buf

    def _pair_args(self):
        """The arguments the two searches' C entries share: the world, the cloud set and the pairs (``min_x`` ... ``n_angles``)."""
        g = self.grid
        return (float(g.min_x), float(g.min_y), float(g.resolution), *self.pairs.args(self.cs), _ptr(self.t), _ptr(self.cos_sin), self.A)

    def run(self):
        fld = self._field()
        ny, nx = fld.shape
        check(_lib.lib().icpmi_grid_match_batch(_ptr(fld), ny, nx, *self._pair_args(), self.W, self.centre_angle, _ptr(self.records),
                                                _ptr(self.scores), _ptr(self.ws), self.ws.numel(), _stream()), "grid_match")
        if self.moments is not None:
            match_moments(self.scores, self.records, self.B, self.A, self.W, self.half_step, out=self.moments)
        return self.records

    def unpack(self, records=None):
        """-> (R [B,2,2], t [B,2], score [B] int, info) on the host (synchronises).  t = translation + ((i - W), (j - W)) *
        resolution, R from the caller's cos / sin at a.  info: ``status``, ``rows``, ``index``, ``a``, ``j``, ``i``,
        ``centre_score``, ``shift_bits``, ``angle`` and ``mean_log_odds`` = score / (rows * 2^k), the mean log-odds under the
        hits (0 where no row was scored).  With ``half_log_odds`` (R, t, score stay the whole-cell winner) also ``moments``
        (B, GMOM_INTS) int64, ``gaussian_of_moments``' ``offset``, ``covariance``, ``support`` and ``edge_weight``, and the
        refined pose: ``t_refined`` = t + offset[:, :2], ``angle_refined`` = angle + offset[:, 2], ``R_refined`` from NumPy's cos
        and sin of it."""
        rec = (self.records if records is None else records).cpu().numpy()[:self.B].astype(np.int64)
        col = lambda s: rec[:, s].copy()                       # noqa: E731
        a, j, i, score, rows = (col(s) for s in (_lib.GMREC_A, _lib.GMREC_J, _lib.GMREC_I, _lib.GMREC_SCORE, _lib.GMREC_ROWS))
        b = np.arange(self.B)
        co, si = self.cos_sin_host[b, a, 0], self.cos_sin_host[b, a, 1]
        R = np.stack([np.stack([co, -si], axis=1), np.stack([si, co], axis=1)], axis=1)
        res = float(self.grid.resolution)
        t = np.stack([self.t_host[:, 0] + (i - self.W) * res, self.t_host[:, 1] + (j - self.W) * res], axis=1)
        info = {"status": col(_lib.GMREC_STATUS), "rows": rows, "index": col(_lib.GMREC_INDEX), "a": a, "j": j, "i": i,
                "centre_score": col(_lib.GMREC_CENTRE), "shift_bits": self.k, "angle": self.angles[b, a],
                "mean_log_odds": np.where(rows > 0, score / (np.maximum(rows, 1) * 2.0 ** self.k), 0.0)}
        if self.moments is not None:
            info["moments"] = self.moments.cpu().numpy()[:self.B]
            info.update(gaussian_of_moments(info["moments"], res, self.angular_step))
            info["t_refined"], info["angle_refined"] = t + info["offset"][:, :2], info["angle"] + info["offset"][:, 2]
            co, si = np.cos(info["angle_refined"]), np.sin(info["angle_refined"])
            info["R_refined"] = np.stack([np.stack([co, -si], axis=1), np.stack([si, co], axis=1)], axis=1)
        return R, t, score, info


class GridSearchBatch(GridMatchBatch):
    """``GridMatchBatch`` over a window of up to ``WIDE_MAX_WINDOW`` cells: the shifts are cut into blocks of ``block`` x
    ``block``, every block gets an upper bound from the bound field, and only the blocks whose bound reaches a seed score
    are scored — the record's first eight slots are those of the exhaustive search all the same.

    ``bounds``: a tensor an earlier ``bound_field(field, block)`` returned, handed back like ``field=`` (no cache: without it
    the bound field is rebuilt by every ``run()``).  ``run()`` returns the (B, 12) int32 record tensor; ``want_bounds``:
    ``bounds_volume`` then holds the (B, A, NB, NB) int32 upper bounds of the blocks.  ``half_log_odds`` is refused: this
    search forms no volume to take moments of."""

    def __init__(self, grid, cloud_set, pair_clouds, translations, angle_rows, window, centre_angle=-1, block=8, field=None, bounds=None,
                 want_bounds=False, half_log_odds=None):
        if half_log_odds is not None:
            raise ValueError("the wide search forms no score volume, so it has no moments: run GridMatchBatch (match_scans) with "
                             "half_log_odds around the wide search's winner")
        self.half_step = self.moments = None
        self._setup(grid, cloud_set, pair_clouds, translations, angle_rows, window, centre_angle, field, WIDE_MAX_WINDOW, WIDE_MAX_ANGLES)
        if block not in BLOCKS:
            raise ValueError(f"block must be one of {BLOCKS}, got {block}")
        if self.A * self.S * self.S >= 2 ** 31:
            raise ValueError(f"{self.A} angles x {self.S}^2 shifts do not fit an int32 index")
        self.block, self.bounds = int(block), bounds
        self.NB = NB = -(-self.S // self.block)
        if self.B * self.A * NB * NB >= 2 ** 31:
            raise ValueError(f"{self.B} pairs x {self.A} angles x {NB}^2 blocks do not fit an int32 index")
        ny, nx = grid.device_log_odds.shape
        if bounds is not None and (tuple(bounds.shape) != (ny + block - 1, nx + block - 1) or bounds.dtype != torch.int16):
            raise ValueError(f"bounds must be the int16 ({ny + block - 1}, {nx + block - 1}) tensor bound_field() returned for this grid and block")
        dev = cloud_set.pts.device
        self.records = torch.zeros((max(self.B, 1), _lib.GMW_REC_INTS), dtype=torch.int32, device=dev)
        self.bounds_volume = torch.zeros((max(self.B, 1), self.A, NB, NB), dtype=torch.int32, device=dev) if want_bounds else None
        need = _lib.lib().icpmi_grid_search_workspace_bytes(self.B, self.A, self.W, self.block)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self._bound_buf = None

    def run(self):
        fld = self._field()
        if self.bounds is not None:
            bnd = self.bounds
        else:
            bnd = self._bound_buf = bound_field(fld, self.block, self._bound_buf)
        ny, nx = fld.shape
        check(_lib.lib().icpmi_grid_search_batch(_ptr(fld), _ptr(bnd), ny, nx, *self._pair_args(), self.W, self.block, self.centre_angle,
                                                 _ptr(self.records), _ptr(self.bounds_volume), _ptr(self.ws), self.ws.numel(), _stream()),
              "grid_search")
        return self.records

    def unpack(self, records=None):
        """``GridMatchBatch.unpack`` with, in ``info``: ``blocks`` (A * NB^2), ``survivors`` (the blocks scored exactly),
        ``seed_score`` (the score they had to reach) and ``max_bound`` (the largest upper bound of a block)."""
        R, t, score, info = super().unpack(records)
        rec = (self.records if records is None else records).cpu().numpy()[:self.B].astype(np.int64)
        for key, slot in (("blocks", _lib.GMW_REC_BLOCKS), ("survivors", _lib.GMW_REC_SURVIVORS), ("seed_score", _lib.GMW_REC_SEED),
                          ("max_bound", _lib.GMW_REC_MAX_BOUND)):
            info[key] = rec[:, slot].copy()
        return R, t, score, info


def cloud_set_of(clouds, voxel_size=None):
    """The clouds as a device ``CloudSet`` (one as it is), through the voxel filter of icp.py:117-129 when a size is given."""
    from .batch import voxel_downsample_set
    cs = clouds if isinstance(clouds, CloudSet) else CloudSet.from_numpy(clouds)
    return voxel_downsample_set(cs, voxel_size) if voxel_size is not None else cs
