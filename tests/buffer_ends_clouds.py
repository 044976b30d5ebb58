"""The cases of tests/test_buffer_ends_clouds_gpu.py: the voxel filter, the searches, the normals, target preparation, the
ICP and its information matrix, with every workspace and prepared buffer exactly as large as include/icpmi.h states
(tests/buffer_ends.py has the runner, DESIGN.md the inventory).  The cloud a pair reads last lies in the last rows of
``pts``, ``out_stride == max_src_n``.  No test in here."""
import ctypes as C

import numpy as np

import information_ref as info
import nn_ref
import voxel_ref
from buffer_ends import ROW_SETS, SCRATCH, Case, host

CASES = []
VOXEL = 0.3


def _add(fn, id, **kw):
    CASES.append(Case(f"{fn.__name__}[{id}]", lambda b: fn(b, **kw)))


def scan_like(n, seed, dim=2, moved=False):
    """n returns from the walls of a 6 m x 4 m room seen from near its middle, 5 mm of noise; ``moved``: the same room
    from a pose 0.05 rad and a decimetre away."""
    rng = np.random.default_rng(600 + seed + n)
    a = np.sort(rng.uniform(-np.pi, np.pi, n))
    c, s = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore"):
        r = np.minimum(np.where(c > 0, 3.2 / c, -2.8 / c), np.where(s > 0, 2.1 / s, -1.9 / s))
    p = np.stack([r * c, r * s], axis=1) + rng.normal(0.0, 0.005, (n, 2))
    if moved:
        th = 0.05
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        p = (p - [0.1, -0.05]) @ R
    if dim == 3:
        p = np.concatenate([p, rng.uniform(-0.5, 0.5, (n, 1))], axis=1)
    return np.ascontiguousarray(p)


class Set:
    """A cloud set of ``rows`` rows per cloud, packed; pairs whose first reads the last cloud as its target."""

    def __init__(self, b, rows, dim, n_pairs):
        self.clouds = [scan_like(n, k, dim, moved=k % 2 == 0) for k, n in enumerate(rows)]
        self.rows, self.dim, self.n_clouds, self.n_pairs = rows, dim, len(rows), n_pairs
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        self.total = int(self.off[-1])
        last = len(rows) - 1
        pairs = np.array([(0, last), (last, 0), (last, last)][:n_pairs], dtype=np.int32).reshape(-1, 2)
        self.src, self.tgt = pairs[:, 0].copy(), pairs[:, 1].copy()
        self.max_src = int(max([rows[c] for c in self.src], default=0))
        self.max_tgt = int(max([rows[c] for c in self.tgt], default=0))
        self.max_n = int(max(rows))
        self.ids = np.arange(self.n_clouds, dtype=np.int32)
        self.p_pts, self.p_off = b.place(np.concatenate(self.clouds), "pts"), b.place(self.off, "off_dev")

    def place_pairs(self, b):
        self.p_src, self.p_tgt = b.place(self.src, "pair_src"), b.place(self.tgt, "pair_tgt")

    def rows_mask(self, tail=()):
        """[B][max_src] (+ tail): the rows of each pair's source."""
        m = np.zeros((self.n_pairs, self.max_src) + tuple(tail), dtype=bool)
        for k, c in enumerate(self.src):
            m[k, :self.rows[c]] = True
        return m


# ── icpmi_voxel_downsample_batch ─────────────────────────────────────────────
def voxel_downsample(b, rows, dim):
    s = Set(b, rows, dim, 0)
    want = [voxel_ref.voxel_ref(c, VOXEL) for c in s.clouds]
    mask = np.zeros((s.total, dim), dtype=bool)
    for c, w in enumerate(want):
        mask[s.off[c]:s.off[c] + len(w)] = True
    p_o = b.out((s.total, dim), np.float64, "out_pts", mask=mask)
    p_c = b.out((s.n_clouds,), np.int32, "out_cnt")
    # (clouds of at most 8 192 rows do not use the workspace and the entry does not look at its size: no refusal)
    p_ws = b.query("workspace", "icpmi_voxel_workspace_bytes", (s.max_n,), refusal=0)
    b.call = lambda short=None: b.L.icpmi_voxel_downsample_batch(s.p_pts, s.p_off, host(s.off), s.n_clouds, dim, VOXEL, p_o, p_c, p_ws,
                                                                 b.size("workspace", short), b.stream())

    def expected():
        out = np.zeros((s.total, dim))
        for c, w in enumerate(want):
            out[s.off[c]:s.off[c] + len(w)] = w
        return {"out_pts": out, "out_cnt": np.array([len(w) for w in want], dtype=np.int32)}
    b.expected = expected


# ── icpmi_nn_batch ───────────────────────────────────────────────────────────
def _nn_expected(s, want_second=False):
    idx, dist, second = (np.zeros((s.n_pairs, s.max_src), dtype=t) for t in (np.int32, np.float64, np.float64))
    for k, (a, t) in enumerate(zip(s.src, s.tgt)):
        i, d, d2 = nn_ref.reference(s.clouds[a], s.clouds[t])
        idx[k, :len(i)], dist[k, :len(i)], second[k, :len(i)] = i, d, d2
    out = {"out_idx": idx, "out_dist": dist}
    if want_second:
        out["out_second_sq"] = second
    return out


def nn_batch(b, rows, dim, n_pairs):
    s = Set(b, rows, dim, n_pairs)
    s.place_pairs(b)
    m = s.rows_mask()
    p_i = b.out((n_pairs, s.max_src), np.int32, "out_idx", mask=m, untouched=~m)
    p_d = b.out((n_pairs, s.max_src), np.float64, "out_dist", mask=m, untouched=~m)
    b.call = lambda short=None: b.L.icpmi_nn_batch(s.p_pts, s.p_off, None, s.p_src, s.p_tgt, n_pairs, s.max_src, dim, p_i, p_d, s.max_src, b.stream())
    b.expected = lambda: _nn_expected(s)


# ── icpmi_normals_2d_batch ───────────────────────────────────────────────────
def normals_2d(b, rows):
    s = Set(b, rows, 2, 0)
    p_n = b.out((s.total, 2), np.float64, "out_normals")
    # the workspace is NULL with size 0, which the header allows for max_n <= 8192
    b.call = lambda short=None: b.L.icpmi_normals_2d_batch(s.p_pts, s.p_off, None, None, s.n_clouds, s.total, s.max_n, 10, p_n, None, 0, b.stream())
    b.twin = ("out_normals",)                                    # the sign of a normal is arbitrary: the same bits as on roomy buffers


# ── icpmi_prepare_targets(_ex) and what reads the prepared buffer ────────────
def _prepare(b, s, k, want_normals, polar):
    """-> prepare(): the call that fills ``prepared`` — exactly icpmi_prepared_bytes — and freezes it for what follows."""
    p_pr = b.query("prepared", "icpmi_prepared_bytes", (s.total, s.n_clouds, s.max_n))
    p_ids = b.place(s.ids, "cloud_ids")
    p_n = b.out((s.total, 2), np.float64, "out_normals") if want_normals else None
    if want_normals:
        b.twin = b.twin + ("out_normals",)

    def prepare(short=None):
        args = (s.p_pts, s.p_off, host(s.off), None, p_ids, host(s.ids), s.n_clouds, s.n_clouds, s.total, s.max_n, k, p_n, p_pr,
                b.size("prepared", short))
        rc = b.L.icpmi_prepare_targets_ex(*args, 1, b.stream()) if polar else b.L.icpmi_prepare_targets(*args, b.stream())
        if rc == 0 and short is None:
            b.sync()
            b.arena.freeze("prepared")                            # the searches and the ICP only read it
        return rc
    return prepare, p_pr


def prepare_nn(b, rows, n_pairs, k, want_normals, want_second):
    s = Set(b, rows, 2, n_pairs)
    s.place_pairs(b)
    prepare, p_pr = _prepare(b, s, k, want_normals, False)
    m = s.rows_mask()
    p_i = b.out((n_pairs, s.max_src), np.int32, "out_idx", mask=m, untouched=~m)
    p_d = b.out((n_pairs, s.max_src), np.float64, "out_dist", mask=m, untouched=~m)
    p_2 = b.out((n_pairs, s.max_src), np.float64, "out_second_sq", mask=m, untouched=~m) if want_second else None

    def call(short=None):
        return prepare(short) or b.L.icpmi_nn_prepared_batch(s.p_pts, s.p_off, None, p_pr, s.p_src, s.p_tgt, n_pairs, s.max_src, s.max_tgt, s.total,
                                                            p_i, p_d, p_2, s.max_src, b.stream())
    b.call = call
    b.expected = lambda: _nn_expected(s, want_second)


def _params(b, method, dim, has_init, gate=0.5):
    from icpmi import _lib
    return _lib.IcpParams(1e-9, gate, 30, _lib.POINT_TO_LINE if method == "point_to_line" else _lib.POINT_TO_POINT, 1 if has_init else 0, dim)


def prepare_icp(b, rows, n_pairs, method, polar, with_ws, want_normals=False):
    """The fused path on the exact prepared buffer; ``want_normals``: the row-order normals beside it (point_to_line)."""
    s = Set(b, rows, 2, n_pairs)
    s.place_pairs(b)
    prepare, p_pr = _prepare(b, s, 10 if method == "point_to_line" else -1, want_normals, polar)
    params = _params(b, method, 2, False)
    p_res = b.out((n_pairs, 16), np.float64, "results")
    p_ws = b.query("workspace", "icpmi_icp_workspace_bytes", (n_pairs, s.max_src, 2), refusal=0) if with_ws else None   # (optional here: not checked)

    def call(short=None):
        return prepare(short) or b.L.icpmi_icp_batch(s.p_pts, s.p_off, None, None, p_pr, s.p_src, s.p_tgt, n_pairs, s.max_src, s.max_tgt, s.total,
                                                     C.byref(params), None, p_res, p_ws, b.size("workspace") if with_ws else 0, b.stream())
    b.call = call
    b.twin = b.twin + ("results",)


def _chain_normals(b, s):
    """Row-order normals of every cloud, made in the arena by icpmi_normals_2d_batch and frozen."""
    p_n = b.place(16 * s.total, "normals", SCRATCH, dtype="float64")

    def make():
        rc = b.L.icpmi_normals_2d_batch(s.p_pts, s.p_off, None, None, s.n_clouds, s.total, s.max_n, 10, p_n, None, 0, b.stream())
        b.sync()
        b.arena.freeze("normals")
        return rc
    return make, p_n


def icp_exhaustive(b, rows, n_pairs, dim, method):
    s = Set(b, rows, dim, n_pairs)
    s.place_pairs(b)
    make, p_n = _chain_normals(b, s) if method == "point_to_line" else ((lambda: 0), None)
    params = _params(b, method, dim, dim == 2)
    init = None
    if dim == 2:
        th = 0.02
        init = np.tile(np.array([np.cos(th), -np.sin(th), np.sin(th), np.cos(th), 0.03, -0.02]), (n_pairs, 1))
    p_init = b.place(init, "init") if init is not None else None
    p_res = b.out((n_pairs, 16), np.float64, "results")
    p_ws = b.query("workspace", "icpmi_icp_workspace_bytes", (n_pairs, s.max_src, dim))

    def call(short=None):
        return (make() if short is None else 0) or b.L.icpmi_icp_batch(
            s.p_pts, s.p_off, None, p_n, None, s.p_src, s.p_tgt, n_pairs, s.max_src, s.max_tgt, s.total, C.byref(params), p_init, p_res, p_ws,
            b.size("workspace", short), b.stream())
    b.call = call
    b.twin = ("results",)


# ── icpmi_icp_information_batch ──────────────────────────────────────────────
def information(b, rows, n_pairs, method, gate=0.5):
    from icpmi import _lib
    s = Set(b, rows, 2, n_pairs)
    s.place_pairs(b)
    make, p_n = _chain_normals(b, s)
    th = 0.05
    T6 = np.tile(np.array([np.cos(th), -np.sin(th), np.sin(th), np.cos(th), 0.1, -0.05]), (n_pairs, 1))
    p_T = b.place(T6, "transforms")
    p_o = b.out((n_pairs, 16), np.float64, "out")
    code = _lib.POINT_TO_LINE if method == "point_to_line" else _lib.POINT_TO_POINT
    b.call = lambda short=None: make() or b.L.icpmi_icp_information_batch(s.p_pts, s.p_off, None, p_n, s.p_src, s.p_tgt, n_pairs, s.max_src, p_T,
                                                                         code, gate, p_o, b.stream())
    b.twin = ("out",)                                            # one fixed tree: the same bits as on roomy buffers

    def after(pattern):
        nrm, out = b.arena.read("normals").reshape(-1, 2), b.arena.read("out")
        for k, (a, t) in enumerate(zip(s.src, s.tgt)):
            ref = info.ref_of_pair(s.clouds[a], s.clouds[t], nrm[s.off[t]:s.off[t + 1]], T6[k], method, gate)
            info.check_record(out[k], ref, (k, method))
    b.after = after


for _rows, _B in zip(ROW_SETS, (1, 3, 1)):
    _id = f"rows{_rows[0]}+{_rows[1]}"
    for _dim in (2, 3):
        _add(voxel_downsample, f"{_id}-{_dim}d", rows=_rows, dim=_dim)
        _add(nn_batch, f"{_id}-{_dim}d-B{_B}", rows=_rows, dim=_dim, n_pairs=_B)
        _add(icp_exhaustive, f"{_id}-{_dim}d-B{_B}-point_to_point", rows=_rows, n_pairs=_B, dim=_dim, method="point_to_point")
    _add(icp_exhaustive, f"{_id}-2d-B{_B}-point_to_line", rows=_rows, n_pairs=_B, dim=2, method="point_to_line")
    _add(normals_2d, _id, rows=_rows)
    for _k, _nrm in ((-1, False), (10, False), (10, True)):
        for _second in (False, True):
            _add(prepare_nn, f"{_id}-B{_B}-k{_k}-{'normals' if _nrm else 'nonormals'}-{'second' if _second else 'nosecond'}", rows=_rows, n_pairs=_B, k=_k,
                 want_normals=_nrm, want_second=_second)
    for _method in ("point_to_line", "point_to_point"):
        for _polar, _ws in ((True, True), (True, False), (False, True)):
            _add(prepare_icp, f"{_id}-B{_B}-{_method}-{'polar' if _polar else 'projection'}-{'ws' if _ws else 'nows'}", rows=_rows, n_pairs=_B,
                 method=_method, polar=_polar, with_ws=_ws)
        _add(information, f"{_id}-B{_B}-{_method}", rows=_rows, n_pairs=_B, method=_method)
    # icpmi_prepare_targets_ex with out_normals: the row-order normals beside a bearing-ordered (up to 2 048 rows) or a
    # projection-ordered prepared buffer, which only the ICP may read
    for _polar in (True, False):
        _add(prepare_icp, f"{_id}-B{_B}-point_to_line-{'polar' if _polar else 'projection'}-ws-normals", rows=_rows, n_pairs=_B,
             method="point_to_line", polar=_polar, with_ws=True, want_normals=True)
