"""Batched scan-pair registration on one MI355X.

The reference runs its scan pairs one after another (loop-closure candidates,
slam.py:575-597; scan-to-submap, slam.py:505-510).  Here a batch of independent
pairs is one pipeline of three launches on the current HIP stream — voxel
filter of every cloud, normals of every target cloud, one fused ICP workgroup
per pair — with device-side cloud sizes in between, so nothing returns to the
host until the results are read.  ``utilities.icp.ICP`` is this with one pair.

torch is used for device memory and streams only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import IcpmiError, IcpParams, check


PREP_MAX_POINTS = 4096      # clouds up to this many rows take the sorted-sweep kernels (prep.hip, icp2.hip)
VOXEL_KEY_RANGE_ERROR = "voxel key range does not fit in 64 bits"      # a count of -1 from the voxel filter, on the host


def require_gpu():
    if not torch.cuda.is_available():
        raise IcpmiError("libicpmi needs an AMD GPU (gfx950); torch.cuda.is_available() is False "
                         "and there is no CPU fallback")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class CloudSet:
    """Point clouds packed row-major in one float64 device buffer.

    off_host/off: first row of each cloud (C+1 entries, capacity based);
    cnt: valid rows per cloud on the device (None = full capacity).
    """

    def __init__(self, pts, off_host, cnt=None, off=None):
        self.pts = pts
        self.off_host = np.ascontiguousarray(off_host, dtype=np.int32)
        self.off = off if off is not None else torch.from_numpy(self.off_host).to(pts.device)
        self.cnt = cnt
        self.dim = int(pts.shape[1])

    @property
    def n_clouds(self):
        return len(self.off_host) - 1

    @property
    def total_rows(self):
        return int(self.off_host[-1])

    @property
    def max_n(self):
        return int(np.diff(self.off_host).max()) if self.n_clouds else 0

    @classmethod
    def from_numpy(cls, clouds, device=None):
        require_gpu()
        device = device or torch.device("cuda", torch.cuda.current_device())
        arrs = [np.ascontiguousarray(c, dtype=np.float64) for c in clouds]
        dim = arrs[0].shape[1] if arrs else 2
        if dim not in (2, 3) or any(a.ndim != 2 or a.shape[1] != dim for a in arrs):
            raise ValueError("clouds must be (n, 2) or (n, 3) arrays of one dimensionality")
        off = np.zeros(len(arrs) + 1, dtype=np.int64)
        np.cumsum([len(a) for a in arrs], out=off[1:])
        if off[-1] >= 2 ** 31:
            raise ValueError("cloud set too large for 32-bit row offsets")
        host = np.concatenate(arrs, axis=0) if arrs and off[-1] > 0 else np.empty((0, dim))
        pts = torch.from_numpy(host).to(device)
        if pts.shape[0] == 0:
            pts = torch.empty((1, dim), dtype=torch.float64, device=device)   # never hand out a null pointer
        return cls(pts, off.astype(np.int32))

    def counts_host(self):
        if self.cnt is None:
            return np.diff(self.off_host)
        return self.cnt.cpu().numpy()

    def to_numpy(self):
        """List of (cnt_c, dim) arrays (synchronises).  A negative count is the voxel filter's "key range does not fit"
        (csrc/voxel.hip): OverflowError, as from ``utilities.icp.voxel_downsample``."""
        host = self.pts.cpu().numpy()
        cnt = self.counts_host()
        if (cnt[:self.n_clouds] < 0).any():
            raise OverflowError(VOXEL_KEY_RANGE_ERROR)
        return [host[self.off_host[c]:self.off_host[c] + cnt[c]].copy() for c in range(self.n_clouds)]


class PairList:
    """The pairs of a batch: the cloud index of the source and of the target of every pair, int32, on the host
    (``src_host`` / ``tgt_host``) and — after ``to(device)`` — on the device (``src`` / ``tgt``).  The parts of one job
    (ICP, rotation search, feature alignment) share one."""

    def __init__(self, pair_src, pair_tgt):
        self.src_host = np.ascontiguousarray(pair_src, dtype=np.int32)
        self.tgt_host = np.ascontiguousarray(pair_tgt, dtype=np.int32)
        self.B = len(self.src_host)
        if len(self.tgt_host) != self.B:
            raise ValueError("pair_src and pair_tgt differ in length")
        self.src = self.tgt = None

    @classmethod
    def of(cls, pair_src, pair_tgt=None):
        """``pair_src`` itself when it is a PairList already (``pair_tgt`` is not looked at), else a new one."""
        return pair_src if isinstance(pair_src, cls) else cls(pair_src, pair_tgt)

    def to(self, dev):
        """Upload the two lists (once) -> self."""
        if self.src is None:
            self.src = torch.from_numpy(self.src_host).to(dev)
            self.tgt = torch.from_numpy(self.tgt_host).to(dev)
        elif self.src.device != dev:
            raise ValueError(f"this pair list lives on {self.src.device}, not on {dev}")
        return self


class _Paired:
    """The names under which every batch object shows its ``pairs`` (a PairList)."""
    pair_src_host = property(lambda self: self.pairs.src_host)
    pair_tgt_host = property(lambda self: self.pairs.tgt_host)
    pair_src = property(lambda self: self.pairs.src)
    pair_tgt = property(lambda self: self.pairs.tgt)
    B = property(lambda self: self.pairs.B)


def pair_lists(sources, targets):
    """(clouds, pair_src, pair_tgt) for sources[i] -> targets[i]; ``sources`` may be one array shared by every pair (the
    loop-closure shape, slam.py:576-579), which is then stored once."""
    targets = list(targets)
    B = len(targets)
    if isinstance(sources, np.ndarray) and sources.ndim == 2:
        return [sources] + targets, np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32)
    sources = list(sources)
    if len(sources) != B:
        raise ValueError("sources and targets differ in length")
    return sources + targets, np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)


ICP_METHODS = ("point_to_point", "point_to_line")


def icp_params(error_threshold, max_corr_dist, max_iterations, method, have_init, dim, strict=False):
    """The ICP problem record of include/icpmi.h with the reference's rules: point_to_line is 2-D only (icp.py:162) and
    ``max_corr_dist=None`` keeps every correspondence (-1).  A method string that is neither of ``ICP_METHODS`` is
    point_to_point, as the reference's else-branch (icp.py:196) — or, with ``strict``, a ValueError."""
    if method not in ICP_METHODS:
        if strict:
            raise ValueError(f"method must be 'point_to_point' or 'point_to_line', got {method!r}")
        method = "point_to_point"
    use_p2l = method == "point_to_line" and dim == 2
    return IcpParams(float(error_threshold), -1.0 if max_corr_dist is None else float(max_corr_dist), int(max_iterations),
                     _lib.POINT_TO_LINE if use_p2l else _lib.POINT_TO_POINT, 1 if have_init else 0, int(dim))


def init_rows(R_init, t_init, B, dim):
    """The start of every pair as [B, d*d + d] float64 rows {R row major, t}: one (d, d) / (d,) start for all pairs or one
    per pair.  None unless both are given: R_init is used only together with t_init (icp.py:153)."""
    if R_init is None or t_init is None:
        return None
    d = dim
    R = np.broadcast_to(np.asarray(R_init, dtype=np.float64), (B, d, d)).reshape(B, d * d)
    t = np.broadcast_to(np.asarray(t_init, dtype=np.float64), (B, d))
    return np.ascontiguousarray(np.concatenate([R, t], axis=1))


def filtered_rows(out, c=0):
    """Rows the voxel filter left in cloud ``c`` of its output set (synchronises); OverflowError for its count of -1 — as a
    slice bound that count would silently drop the cloud's last row."""
    n = int(out.cnt[c].item())
    if n < 0:
        raise OverflowError(VOXEL_KEY_RANGE_ERROR)
    return n


def voxel_downsample_set(cs, voxel_size, out=None, workspace=None):
    """voxel_downsample (reference icp.py:117-129) of every cloud of the set."""
    L = _lib.lib()
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    if out is None:
        out = CloudSet(torch.empty_like(cs.pts), cs.off_host,
                       cnt=torch.empty(max(cs.n_clouds, 1), dtype=torch.int32, device=cs.pts.device), off=cs.off)
    need = L.icpmi_voxel_workspace_bytes(cs.max_n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=cs.pts.device)
    check(L.icpmi_voxel_downsample_batch(_ptr(cs.pts), _ptr(cs.off), cs.off_host.ctypes.data_as(C.c_void_p),
                                         cs.n_clouds, cs.dim, float(voxel_size), _ptr(out.pts), _ptr(out.cnt),
                                         _ptr(workspace), workspace.numel(), _stream()), "voxel_downsample")
    return out


def normals_set(cs, k, cloud_ids=None, out=None, workspace=None, cloud_ids_dev=None, return_workspace=False):
    """estimate_normals_2d (reference icp.py:51-76) for the selected clouds of a 2-D set.  ``cloud_ids_dev``: the int32 device
    copy of ``cloud_ids`` when the caller keeps one (else it is uploaded here, and the host waits for the stream);
    ``return_workspace``: -> (normals, the workspace used), to hand back at the next call.  With ``out``, a workspace and
    device ids (or every cloud) the call only enqueues."""
    L = _lib.lib()
    if cs.dim != 2:
        raise ValueError("normals are defined for 2-D clouds only")
    if out is None:
        out = torch.zeros((max(cs.total_rows, 1), 2), dtype=torch.float64, device=cs.pts.device)
    if cloud_ids is None:
        n_sel, ids_t, max_n = cs.n_clouds, None, cs.max_n
    else:
        ids = np.ascontiguousarray(cloud_ids, dtype=np.int32)
        n_sel = len(ids)
        max_n = int(np.diff(cs.off_host)[ids].max()) if n_sel else 0
        ids_t = cloud_ids_dev if cloud_ids_dev is not None else torch.from_numpy(ids).to(cs.pts.device)
        if ids_t.dtype != torch.int32 or ids_t.numel() != n_sel or ids_t.device != cs.pts.device:
            raise ValueError("cloud_ids_dev must be the int32 device copy of cloud_ids")
    if max_n <= PREP_MAX_POINTS or k > 31:
        # sweep search on the axis-sorted copy (prep.hip; clouds above 4096 rows through global memory); the sorted copy
        # is a by-product.  Any k (the exhaustive kernel below holds its lists in registers: k <= 31).
        need = L.icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, max_n)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=cs.pts.device)
        ids_host = None if cloud_ids is None else np.ascontiguousarray(cloud_ids, dtype=np.int32)
        check(L.icpmi_prepare_targets_ex(_ptr(cs.pts), _ptr(cs.off), cs.off_host.ctypes.data_as(C.c_void_p), _ptr(cs.cnt),
                                         _ptr(ids_t), None if ids_host is None else ids_host.ctypes.data_as(C.c_void_p), n_sel,
                                         cs.n_clouds, cs.total_rows, max_n, int(k), _ptr(out), _ptr(workspace),
                                         workspace.numel(), 1, _stream()), "estimate_normals_2d")
        return (out, workspace) if return_workspace else out
    need = L.icpmi_normals_workspace_bytes(cs.total_rows, max_n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=cs.pts.device)
    check(L.icpmi_normals_2d_batch(_ptr(cs.pts), _ptr(cs.off), _ptr(cs.cnt), _ptr(ids_t), n_sel, cs.total_rows,
                                   max_n, int(k), _ptr(out), _ptr(workspace), workspace.numel(), _stream()),
          "estimate_normals_2d")
    return (out, workspace) if return_workspace else out


def nn_set(cs, pair_src, pair_tgt=None, out=None):
    """1-NN of every row of cloud pair_src[b] in cloud pair_tgt[b] -> (dist, idx) device tensors [B, stride].  With a
    ``PairList`` already on the device as ``pair_src`` and ``out`` = the (dist, idx) of an earlier call, the call allocates
    and uploads nothing: one launch on the current stream."""
    L = _lib.lib()
    p = PairList.of(pair_src, pair_tgt).to(cs.pts.device)
    B = p.B
    stride = max(int(np.diff(cs.off_host)[p.src_host].max()) if B else 0, 1)
    if out is None:
        out = (torch.empty((max(B, 1), stride), dtype=torch.float64, device=cs.pts.device),
               torch.empty((max(B, 1), stride), dtype=torch.int32, device=cs.pts.device))
    dist, idx = out
    if tuple(dist.shape) != (max(B, 1), stride) or tuple(idx.shape) != (max(B, 1), stride):
        raise ValueError(f"out must be (dist, idx) of shape {(max(B, 1), stride)}")
    check(L.icpmi_nn_batch(_ptr(cs.pts), _ptr(cs.off), _ptr(cs.cnt), _ptr(p.src), _ptr(p.tgt), B, stride, cs.dim,
                           _ptr(idx), _ptr(dist), stride, _stream()), "nn")
    return dist, idx


class SweepWorkspace:
    """What ``nn_set_sweep`` allocates for a cloud set and a pair list — the prepared targets, the target ids on the device
    and the outputs — kept, so that a repeated call only enqueues its two launches."""

    def __init__(self, cs, p, return_second):
        dev = cs.pts.device
        B = p.B
        sizes = np.diff(cs.off_host)
        self.tgt_ids = np.unique(p.tgt_host)
        self.max_tgt = int(sizes[self.tgt_ids].max()) if B else 0
        if self.max_tgt > PREP_MAX_POINTS:
            raise ValueError(f"target clouds above {PREP_MAX_POINTS} rows need the exhaustive search (nn_set)")
        self.stride = max(int(sizes[p.src_host].max()) if B else 0, 1)
        self.prepared = torch.empty(_lib.lib().icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, self.max_tgt),
                                    dtype=torch.uint8, device=dev)
        self.ids = torch.from_numpy(self.tgt_ids.astype(np.int32)).to(dev)
        self.idx = torch.empty((max(B, 1), self.stride), dtype=torch.int32, device=dev)
        self.dist = torch.empty((max(B, 1), self.stride), dtype=torch.float64, device=dev)
        self.second = torch.empty((max(B, 1), self.stride), dtype=torch.float64, device=dev) if return_second else None


def nn_set_sweep(cs, pair_src, pair_tgt=None, return_second=False, workspace=None):
    """Same result as ``nn_set`` by the sorted-sweep search (2-D, target clouds of at most 4096 rows):
    prepares the target clouds (axis choice + sort), then binary search + outward sweep per query.  ``workspace``: the
    ``SweepWorkspace`` of the same set and (device-resident ``PairList``) pairs — the call then allocates and uploads nothing."""
    L = _lib.lib()
    if cs.dim != 2:
        raise ValueError("the sweep search is 2-D only")
    dev = cs.pts.device
    p = PairList.of(pair_src, pair_tgt)
    B = p.B
    w = workspace if workspace is not None else SweepWorkspace(cs, p, return_second)
    if return_second and w.second is None:
        raise ValueError("this workspace holds no tensor for the second distances")
    check(L.icpmi_prepare_targets(_ptr(cs.pts), _ptr(cs.off), None, _ptr(cs.cnt), _ptr(w.ids), None, len(w.tgt_ids),
                                  cs.n_clouds, cs.total_rows, w.max_tgt, -1, None, _ptr(w.prepared), w.prepared.numel(),
                                  _stream()), "prepare_targets")
    p.to(dev)
    second = w.second if return_second else None
    check(L.icpmi_nn_prepared_batch(_ptr(cs.pts), _ptr(cs.off), _ptr(cs.cnt), _ptr(w.prepared), _ptr(p.src), _ptr(p.tgt), B,
                                    w.stride, w.max_tgt, cs.total_rows, _ptr(w.idx), _ptr(w.dist), _ptr(second), w.stride,
                                    _stream()), "nn (sweep)")
    return (w.dist, w.idx, second) if return_second else (w.dist, w.idx)


class IcpBatch(_Paired):
    """A batch of scan pairs resident in HBM, ready to be registered repeatedly.

    clouds: list of arrays; pair_src/pair_tgt: cloud indices per pair (a source
    shared by many pairs is stored once), or a ``PairList`` as pair_src.  ``run()`` performs exactly what the
    reference's ``ICP()`` does per pair — voxel filter of source and target,
    target normals for point_to_line, the ICP loop — and leaves a
    (B, 16) float64 result tensor on the device.
    """
    strict_method = False       # a method string the reference does not know: point_to_point (icp_params)

    def __init__(self, clouds, pair_src, pair_tgt, error_threshold, max_iterations, voxel_size,
                 R_init=None, t_init=None, method="point_to_point", normal_k=10, max_corr_dist=None,
                 force_exhaustive=False):
        require_gpu()
        raw = clouds if isinstance(clouds, CloudSet) else CloudSet.from_numpy(clouds)
        self._init_common(raw, pair_src, pair_tgt, error_threshold, max_iterations, voxel_size, R_init, t_init, method,
                          normal_k, max_corr_dist)
        self._init_buffers(force_exhaustive)

    def _init_common(self, raw, pair_src, pair_tgt, error_threshold, max_iterations, voxel_size, R_init, t_init, method,
                     normal_k, max_corr_dist):
        """What every variant needs: the pairs, the problem, the start of every pair, the ICP workspace, the results and
        the gate state.  The clouds' own buffers are ``_init_buffers``' (a resident variant points at a history's)."""
        self.raw, self.dim = raw, raw.dim
        dev = raw.pts.device
        self.pairs = PairList.of(pair_src, pair_tgt)
        rows = init_rows(R_init, t_init, self.B, self.dim)
        self.set_problem(error_threshold, max_iterations, voxel_size, method, normal_k, max_corr_dist, rows is not None)
        self.pairs.to(dev)
        self.init = None if rows is None else torch.from_numpy(rows).to(dev)
        # parked pairs (csrc/icp2.hip): a large batch runs in two stages — the pairs still running after 12
        # iterations are continued together by a second launch — and pairs that start metres from their target
        # are continued by the kernel for far queries
        self.icp_ws = torch.empty(_lib.lib().icpmi_icp_workspace_bytes(self.B, self.max_src_n, self.dim),
                                  dtype=torch.uint8, device=dev)
        self.results = torch.zeros((max(self.B, 1), _lib.RES_DOUBLES), dtype=torch.float64, device=dev)
        self.gate = None
        self.first_accepted_dev = None
        self.info_normals = None          # row-order normals of the targets information() was asked about (made on first use)

    def set_problem(self, error_threshold, max_iterations, voxel_size, method, normal_k, max_corr_dist, have_init):
        """Aim the batch at the clouds now in ``raw`` (their row counts) with these ICP arguments; buffers stay as they
        are, so a cached batch (``PairContext``) may only be re-aimed at clouds within the capacity it was built for."""
        self.voxel_size, self.normal_k = float(voxel_size), int(normal_k)
        self.params = icp_params(error_threshold, max_corr_dist, max_iterations, method, have_init, self.dim,
                                 strict=self.strict_method)
        self.use_p2l = self.params.method == _lib.POINT_TO_LINE
        sizes = np.diff(self.raw.off_host)
        self.max_src_n = int(sizes[self.pair_src_host].max()) if self.B else 0
        self.max_tgt_n = int(sizes[self.pair_tgt_host].max()) if self.B else 0

    def _init_buffers(self, force_exhaustive):
        """The buffers a batch owns for its clouds (persistent: nothing is allocated inside run())."""
        L = _lib.lib()
        dev = self.raw.pts.device
        self.tgt_ids = np.unique(self.pair_tgt_host)          # (sorted, contiguous, int32 as the pair list)
        self.vox = CloudSet(torch.empty_like(self.raw.pts), self.raw.off_host,
                            cnt=torch.zeros(max(self.raw.n_clouds, 1), dtype=torch.int32, device=dev), off=self.raw.off)
        self.vox_ws = torch.empty(L.icpmi_voxel_workspace_bytes(self.raw.max_n), dtype=torch.uint8, device=dev)
        self.tgt_ids_dev = torch.from_numpy(self.tgt_ids).to(dev)
        # fast path: 2-D, every cloud small enough for the on-chip kernels
        # (targets above PREP_MAX_POINTS rows — a rolling submap — are sorted through global memory and searched via L2)
        self.fast = self.dim == 2 and self.max_src_n <= PREP_MAX_POINTS and not force_exhaustive
        self.prepared = self.normals = None
        if self.fast:
            self.prepared = torch.empty(L.icpmi_prepared_bytes(self.raw.total_rows, self.raw.n_clouds, self.max_tgt_n),
                                        dtype=torch.uint8, device=dev)
        elif self.use_p2l:
            self.normals = torch.zeros((max(self.raw.total_rows, 1), 2), dtype=torch.float64, device=dev)
            self.nrm_ws = torch.empty(L.icpmi_normals_workspace_bytes(self.raw.total_rows, self.max_tgt_n),
                                      dtype=torch.uint8, device=dev)

    @property
    def layout_rows(self):
        """The row count ``prepared`` is laid out for: the set's rows (a resident history: its row capacity)."""
        return self.raw.total_rows

    def direction_words(self):
        """The sort order the last ``prepare()`` chose for every target cloud (``tgt_ids`` order): the int32 words behind the
        row arrays of ``prepared`` (csrc/prep_common.hpp, PreparedView) — 0..3 the projections x, y, x + y, x - y, 4 the
        bearing (csrc/sweep.hpp).  Read-only, on the host (synchronises); fast path only."""
        if self.prepared is None:
            raise IcpmiError("no prepared targets: this batch takes the exhaustive kernels")
        at = self.layout_rows * 40
        words = self.prepared[at:at + 4 * self.raw.n_clouds].view(torch.int32)
        return words.cpu().numpy()[self.tgt_ids].copy()

    def set_gate(self, error_accept, search_records=None, index_base=0, index_stride=1):
        """Stop after the first accepted pair (slam.py:582-597; include/icpmi.h, icpmi_icp_batch_gated): from now on
        ``run()`` lets pairs after the first one with err < error_accept (and, with ``search_records``, a rotation-search
        status below 2) stop early with status ST_SKIPPED, and leaves that pair's index in ``first_accepted_dev``
        (device int32, -1: none).  Every record up to it equals the ungated run's bit for bit.  None: ungated again."""
        if error_accept is None:
            self.gate = None
            return
        if index_base < 0 or index_stride < 1:
            raise ValueError("index_base must be >= 0 and index_stride >= 1")
        self.gate = (float(error_accept), search_records, int(index_base), int(index_stride))
        if self.first_accepted_dev is None:
            self.first_accepted_dev = torch.full((1,), -1, dtype=torch.int32, device=self.results.device)

    def run(self, events=None):
        """Enqueue voxel filter -> normals -> fused ICP on the current stream; returns the device result tensor.

        events: optional (start, end) torch.cuda.Event pair recorded around the fused ICP launch only."""
        self.prepare()
        return self.launch_icp(events)

    def prepare(self):
        """The per-cloud half of ``run()``: voxel filter of every cloud, search order (and normals) of the targets."""
        L = _lib.lib()
        st = _stream()
        voxel_downsample_set(self.raw, self.voxel_size, out=self.vox, workspace=self.vox_ws)
        if self.fast:
            # allow_polar: the sort order (a projection, or the bearing about the frame origin) is the library's choice
            check(L.icpmi_prepare_targets_ex(_ptr(self.vox.pts), _ptr(self.vox.off),
                                             self.raw.off_host.ctypes.data_as(C.c_void_p), _ptr(self.vox.cnt),
                                             _ptr(self.tgt_ids_dev), self.tgt_ids.ctypes.data_as(C.c_void_p),
                                             len(self.tgt_ids), self.raw.n_clouds, self.raw.total_rows, self.max_tgt_n,
                                             self.normal_k if self.use_p2l else -1, None, _ptr(self.prepared),
                                             self.prepared.numel(), 1, st), "prepare_targets")
        elif self.use_p2l and self.normal_k > 31:
            normals_set(self.vox, self.normal_k, cloud_ids=self.tgt_ids, out=self.normals)      # any k: the prepare path
        elif self.use_p2l:
            check(L.icpmi_normals_2d_batch(_ptr(self.vox.pts), _ptr(self.vox.off), _ptr(self.vox.cnt),
                                           _ptr(self.tgt_ids_dev), len(self.tgt_ids), self.raw.total_rows,
                                           self.max_tgt_n, self.normal_k, _ptr(self.normals), _ptr(self.nrm_ws),
                                           self.nrm_ws.numel(), st), "estimate_normals_2d")

    def launch_icp(self, events=None):
        """The per-pair half of ``run()``: the fused ICP on the filtered clouds and prepared targets -> the result tensor."""
        L = _lib.lib()
        st = _stream()
        if events is not None:
            events[0].record()
        args = (_ptr(self.vox.pts), _ptr(self.vox.off), _ptr(self.vox.cnt), _ptr(self.normals), _ptr(self.prepared),
                _ptr(self.pair_src), _ptr(self.pair_tgt), self.B, self.max_src_n, self.max_tgt_n, self.layout_rows,
                C.byref(self.params), _ptr(self.init), _ptr(self.results), _ptr(self.icp_ws),
                self.icp_ws.numel() if self.icp_ws is not None else 0)
        if self.gate is None:
            check(L.icpmi_icp_batch(*args, st), "ICP")
        else:
            accept, search, base, stride = self.gate
            check(L.icpmi_icp_batch_gated(*args, accept, _ptr(search), base, stride, _ptr(self.first_accepted_dev), st),
                  "ICP (gated)")
        if events is not None:
            events[1].record()
        return self.results

    def information(self, pairs=None, results=None):
        """The Gauss-Newton information records (icpmi.information; include/icpmi.h, icpmi_icp_information_batch) of the pairs
        ``pairs`` (indices into the pair list; None: all) at the transforms in ``results`` (None: those of the last ``run()``),
        with the batch's method and ``max_corr_dist`` -> a device (len(pairs), 16) tensor; does not synchronise.  2-D only."""
        from .information import batch_information
        return batch_information(self, pairs, results)

    def unpack(self, results=None):
        """(R [B,d,d], t [B,d], err [B], info) on the host (synchronises)."""
        res = (self.results if results is None else results).cpu().numpy()[:self.B]
        return unpack_results(res, self.dim)


def unpack_results(res, dim):
    d = dim
    R = res[:, _lib.RES_R:_lib.RES_R + d * d].reshape(-1, d, d).copy()
    t = res[:, _lib.RES_T:_lib.RES_T + d].copy()
    err = res[:, _lib.RES_ERR].copy()
    info = dict(iters=res[:, _lib.RES_ITERS].astype(np.int64), status=res[:, _lib.RES_STATUS].astype(np.int64),
                delta=res[:, _lib.RES_DELTA].copy())
    return R, t, err, info


def pack_results(R, t, err, info):
    """The inverse of ``unpack_results``: [B, RES_DOUBLES] records."""
    res = np.zeros((len(err), _lib.RES_DOUBLES))
    d = R.shape[1]
    res[:, _lib.RES_R:_lib.RES_R + d * d] = R.reshape(len(err), d * d)
    res[:, _lib.RES_T:_lib.RES_T + d] = t
    res[:, _lib.RES_ERR] = err
    res[:, _lib.RES_DELTA] = info["delta"]
    res[:, _lib.RES_ITERS] = info["iters"]
    res[:, _lib.RES_STATUS] = info["status"]
    return res


class PairContext:
    """One scan pair at a time through buffers that stay allocated (one context per device).

    ``utilities.icp.ICP`` is called once per scan by a SLAM loop (slam.py:90, 217, 471); building an ``IcpBatch`` per
    call — a dozen allocations, uploads of offsets and pair lists — cost more than its kernels.  Here the device
    buffers are sized for a capacity (grown when a larger cloud arrives) and a call is: one pinned upload of the
    two clouds and their offsets, the three launches of ``IcpBatch.run``, one 128-byte read-back.  2-D clouds of at
    most 4096 rows each (the on-chip kernels); anything else builds a fresh ``IcpBatch``."""
    _per_device = {}

    @classmethod
    def get(cls):
        require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in cls._per_device:
            cls._per_device[dev] = cls(dev)
        return cls._per_device[dev]

    def __init__(self, dev):
        self.dev = dev
        self.cap_s = self.cap_t = 0
        self.batch = None

    def _grow(self, ns, nt):
        # source and target capacities grow independently, each at most PREP_MAX_POINTS rows, so the batch object always
        # takes the on-chip kernels (a 2 100-row scan against a 3 000-row target: 5 100 rows in all, both halves fit)
        self.cap_s = min(PREP_MAX_POINTS, max(2048, self.cap_s, 2 * ns))
        self.cap_t = min(PREP_MAX_POINTS, max(2048, self.cap_t, 2 * nt))
        cap = self.cap_s + self.cap_t
        dummy = CloudSet(torch.zeros((cap, 2), dtype=torch.float64, device=self.dev),
                         np.array([0, self.cap_s, cap], dtype=np.int32))
        self.batch = IcpBatch(dummy, [0], [1], 1e-6, 1, 1.0, np.eye(2), np.zeros(2), "point_to_line", 1, None)
        assert self.batch.fast, "PairContext must stay on the sorted-sweep kernels"
        self.stage = torch.empty((cap, 2), dtype=torch.float64).pin_memory()
        self.off_stage = torch.zeros(3, dtype=torch.int32).pin_memory()
        self.init_stage = torch.zeros((1, 6), dtype=torch.float64).pin_memory()
        self.res_host = torch.zeros((1, _lib.RES_DOUBLES), dtype=torch.float64).pin_memory()

    def solve(self, source, target, error_threshold, max_iterations, voxel_size, R_init, t_init, method, normal_k,
              max_corr_dist):
        """-> one (RES_DOUBLES,) float64 result record on the host."""
        ns, nt = len(source), len(target)
        if ns > self.cap_s or nt > self.cap_t:
            self._grow(ns, nt)
        b = self.batch
        h = self.stage.numpy()
        h[:ns] = source
        h[ns:ns + nt] = target
        b.raw.pts[:ns + nt].copy_(self.stage[:ns + nt], non_blocking=True)
        b.raw.off_host[:] = (0, ns, ns + nt)
        self.off_stage.numpy()[:] = b.raw.off_host
        b.raw.off.copy_(self.off_stage, non_blocking=True)
        rows = init_rows(R_init, t_init, 1, 2)
        b.set_problem(error_threshold, max_iterations, voxel_size, method, normal_k, max_corr_dist, rows is not None)
        if rows is not None:
            self.init_stage.numpy()[:] = rows
            b.init.copy_(self.init_stage, non_blocking=True)
        res = b.run()
        self.res_host.copy_(res[:1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.res_host.numpy()[0].copy()


def icp_pair(source, target, error_threshold, max_iterations, voxel_size, R_init=None, t_init=None,
             method="point_to_point", normal_k=10, max_corr_dist=None):
    """One registration with the semantics of the reference ``ICP`` -> (R, t, err, info) like ``icp_batch``."""
    d = source.shape[1]
    if d == 2 and len(source) <= PREP_MAX_POINTS and len(target) <= PREP_MAX_POINTS and method in ICP_METHODS:
        res = PairContext.get().solve(source, target, error_threshold, max_iterations, voxel_size, R_init, t_init, method,
                                      normal_k, max_corr_dist)
        return unpack_results(res[None, :], 2)
    return icp_batch([source], [target], error_threshold, max_iterations, voxel_size, R_init, t_init, method, normal_k,
                     max_corr_dist)


def icp_batch(sources, targets, error_threshold, max_iterations, voxel_size, R_init=None, t_init=None,
              method="point_to_point", normal_k=10, max_corr_dist=None, force_exhaustive=False):
    """Register sources[i] onto targets[i] for every i; same per-pair semantics as the reference ``ICP``.

    ``sources`` may be one array shared by every pair (the loop-closure shape,
    slam.py:576-579).  Returns (R [B,d,d], t [B,d], err [B], info).
    """
    clouds, ps, pt = pair_lists(sources, targets)
    batch = IcpBatch(clouds, ps, pt, error_threshold, max_iterations, voxel_size, R_init, t_init,
                     method, normal_k, max_corr_dist, force_exhaustive)
    batch.run()
    return batch.unpack()
