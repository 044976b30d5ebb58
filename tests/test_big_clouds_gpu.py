"""The two large routes of the normals on clouds above 4 096 and 8 192 rows: csrc/normals.hip (icpmi_normals_2d_batch: TopK
widths 8, 16, 32; x-sorted index in LDS up to 8 192 slots, in global memory above) and csrc/prep_big.hip
(icpmi_prepare_targets_ex: radix sort, gather, big_normals_kernel in widths 8, 13, 16, 32).  Clouds, references and bounds come
from tests/big_cloud_cases.py and are checked on the host by tests/test_big_clouds_cpu.py; nothing here is measured from a
kernel.  The clouds are uniform or nearly so: one wrong neighbour moves a normal by more than 1e9 units, the bound is below 20.

Which test reaches what:
  TopK<8>, <16>, <32> of normals.hip on the LDS index (4 097, 8 192 rows) and on the global index (8 193, 16 384, 16 385):
      test_normals_hip_every_size_and_k;
  big_normals_kernel<8>, <13>, <16>, <32>: test_prepare_big_every_width (k = 1, 7 | 8, 12 | 13, 15 | 16, 31), and
      through a registration test_submap_registration_at_other_list_widths (7, 16, 31; 10 is in test_gpu_parity.py);
  a device count below the capacity, on both routes, and several large clouds of one call through one scratch (the
      8 193- and 12 000-row clouds of the set: 2 x rows slots each of one workspace in normals.hip, one sort scratch in
      prep_big.hip): test_one_set_counts_and_a_selection.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from big_cloud_cases import (DECOYS, DUP_KS, DUP_N, FAMILY, KS, PREP_KS, SIZES, big_bound, cloud, compared, decoys, reference, ties,
                             uniform)
from conftest import rot_err
from test_p2l_step_cpu import U, normal_angle_units

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
LDS_SLOTS = 8192                      # NRM_LDS_MAX of normals.hip


class _Set:
    """A cloud set on the device with optional counts, and the two entries called as icpmi.batch.normals_set calls them."""

    def __init__(self, clouds, counts=None):
        import torch
        from icpmi import _lib, batch
        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.torch, self.L, self.batch = torch, _lib.lib(), batch
        self.cs = batch.CloudSet.from_numpy(clouds)
        self.cap = np.diff(self.cs.off_host)
        self.counts = self.cap if counts is None else np.asarray(counts, dtype=np.int32)
        if counts is not None:
            self.cs.cnt = torch.from_numpy(self.counts.astype(np.int32)).to(self.cs.pts.device)

    def _selection(self, ids):
        cs = self.cs
        if ids is None:
            return cs.n_clouds, None, None, cs.max_n
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        return len(ids), self.torch.from_numpy(ids).to(cs.pts.device), ids, int(self.cap[ids].max())

    def _out(self):
        return self.torch.full((self.cs.total_rows, 2), SENTINEL, dtype=self.torch.float64, device=self.cs.pts.device)

    def normals_hip(self, k, ids=None):
        """icpmi_normals_2d_batch -> normals [total rows, 2]; rows it does not write keep SENTINEL.  No workspace at all where
        the largest selected cloud fits the LDS index."""
        cs, _ptr, _stream = self.cs, self.batch._ptr, self.batch._stream
        n_sel, ids_t, _, max_n = self._selection(ids)
        ws = None
        if max_n > LDS_SLOTS:
            ws = self.torch.empty(self.L.icpmi_normals_workspace_bytes(cs.total_rows, max_n), dtype=self.torch.uint8, device=cs.pts.device)
        out = self._out()
        rc = self.L.icpmi_normals_2d_batch(_ptr(cs.pts), _ptr(cs.off), _ptr(cs.cnt), _ptr(ids_t), n_sel, cs.total_rows, max_n, int(k),
                                           _ptr(out), _ptr(ws), 0 if ws is None else ws.numel(), _stream())
        assert rc == 0, rc
        return out.cpu().numpy()

    def prepare(self, k, ids=None):
        """icpmi_prepare_targets_ex with the host offsets and out_normals, as the first branch of normals_set ->
        (normals in row order, sorted xy, sorted normals, sorted -> row map, axis word per cloud)."""
        cs, _ptr, _stream = self.cs, self.batch._ptr, self.batch._stream
        n_sel, ids_t, ids_host, max_n = self._selection(ids)
        need = self.L.icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, max_n)
        ws = self.torch.zeros(need, dtype=self.torch.uint8, device=cs.pts.device)
        out = self._out()
        rc = self.L.icpmi_prepare_targets_ex(_ptr(cs.pts), _ptr(cs.off), cs.off_host.ctypes.data_as(C.c_void_p), _ptr(cs.cnt), _ptr(ids_t),
                                             None if ids_host is None else ids_host.ctypes.data_as(C.c_void_p), n_sel, cs.n_clouds,
                                             cs.total_rows, max_n, int(k), _ptr(out), _ptr(ws), need, 1, _stream())
        assert rc == 0, rc
        T, raw = cs.total_rows, ws.cpu().numpy()                             # PreparedView, csrc/prep_common.hpp
        return (out.cpu().numpy(), raw[:T * 16].view(np.float64).reshape(T, 2), raw[T * 16:T * 32].view(np.float64).reshape(T, 2),
                raw[T * 32:T * 36].view(np.int32), raw[T * 40:T * 40 + 4 * cs.n_clouds].view(np.int32))


@functools.lru_cache(maxsize=None)
def _single(name, n):
    return _Set([cloud(name, n)])


def _check_normals(label, got, name, n, k):
    """finite, unit length to 8 u, every compared point within its family's bound of the longdouble eigenvector"""
    ref, gap, _ = reference(name, n, k)
    assert got.shape == ref.shape and np.isfinite(got).all(), label
    assert np.abs(np.sum(got * got, axis=1) - 1.0).max() <= 8 * U, label
    ok = compared(name, n, k)
    units = normal_angle_units(got, ref, gap)
    worst = int(np.argmax(np.where(ok, units, 0)))
    assert units[ok].max() <= big_bound(FAMILY[name]), (label, float(units[worst]), worst, big_bound(FAMILY[name]))
    return units


NORMALS_CASES = [("uniform", n, k) for n in SIZES for k in KS]
NORMALS_CASES += [(name, n, k) for name in ("uniform_far", "columns", "ties") for n in (8193, 16385) for k in KS]
NORMALS_CASES += [("duplicates", DUP_N, k) for k in DUP_KS]


@pytest.mark.parametrize("name, n, k", NORMALS_CASES, ids=[f"{a}-{b}-k{c}" for a, b, c in NORMALS_CASES])
def test_normals_hip_every_size_and_k(name, n, k):
    s = _single(name, n)
    got = s.normals_hip(k)
    units = _check_normals(("normals.hip", name, n, k), got, name, n, k)
    if name == "ties":                                                    # the planted queries took the lower row's normal:
        q = ties(n)[1][k][:, 0]                                           # the other candidate's lies 1e6 bounds away
        assert units[q].max() <= big_bound("ties"), (n, k, float(units[q].max()))
    assert s.normals_hip(k).tobytes() == got.tobytes(), (name, n, k)      # run again: the same bytes


def _projection(d, p):
    a = 0.0 if d == 1 else 1.0
    b = 0.0 if d == 0 else (-1.0 if d == 3 else 1.0)
    return p[:, 0] * a + p[:, 1] * b                                       # csrc/sweep.hpp, proj: x, y, x + y or x - y


PREP_CASES = [(name, n, k) for name, n in (("uniform", 4097), ("uniform", 8193), ("uniform", 16385), ("columns", 8193)) for k in PREP_KS]
PREP_CASES += [("ties", 8193, k) for k in KS]          # the tie rule of TopKP (rows read through the row map), planted for these k


@pytest.mark.parametrize("name, n, k", PREP_CASES, ids=[f"{a}-{b}-k{c}" for a, b, c in PREP_CASES])
def test_prepare_big_every_width(name, n, k):
    pts = cloud(name, n)
    nrm, sxy, snrm, sorig, dirs = _single(name, n).prepare(k)
    units = _check_normals(("prep_big.hip", name, n, k), nrm, name, n, k)
    if name == "ties":
        q = ties(n)[1][k][:, 0]
        assert units[q].max() <= big_bound("ties"), (n, k, float(units[q].max()))
    d = int(dirs[0])
    assert 0 <= d <= 3, d
    assert np.array_equal(np.sort(sorig), np.arange(n))                   # a permutation of the rows
    assert sxy.tobytes() == pts[sorig].tobytes()
    u = _projection(d, sxy)
    step = np.diff(u)
    assert (step >= 0).all(), (name, n, k, d)
    assert (np.diff(sorig)[step == 0] > 0).all(), (name, n, k, d)         # the radix sort is stable: equal keys in row order
    if name == "columns" and d == 0:
        assert int((step == 0).sum()) >= n - 64
    assert snrm.tobytes() == nrm[sorig].tobytes()


def test_the_two_routes_on_one_cloud():
    s = _single("uniform", 8193)
    a, b = s.normals_hip(12), s.prepare(12)[0]
    _check_normals(("normals.hip", 12), a, "uniform", 8193, 12)
    _check_normals(("prep_big.hip", 12), b, "uniform", 8193, 12)
    same = a.tobytes() == b.tobytes()
    print(f"\nuniform(8193), k = 12: normals.hip and prep_big.hip bit-equal: {same}; rows that differ: {int((a != b).any(axis=1).sum())}")


# ── one set, counts, a selection ─────────────────────────────────────────────────────────────────────────────────────────────
SET_ROWS = (1, 2, 5, 300, 4096, 4097, 8192, 8193, 12000)
SELECTION = (9, 7, 3, 10, 0, 8, 4)           # decoys (8193, 8192) | 8 193 | 300 | decoys (12000, 5000) | 1 | 12 000 | 4 096 rows


@functools.lru_cache(maxsize=None)
def _the_set():
    clouds = [uniform(n) for n in SET_ROWS] + [decoys(*pair) for pair in DECOYS]
    counts = [len(c) for c in clouds[:len(SET_ROWS)]] + [count for _, count in DECOYS]
    return clouds, counts, _Set(clouds, counts)


@pytest.mark.parametrize("k", (7, 16))
@pytest.mark.parametrize("entry", ("normals_hip", "prepare"))
def test_one_set_counts_and_a_selection(entry, k):
    clouds, counts, s = _the_set()
    off = s.cs.off_host

    def run(target, ids=None):
        out = getattr(target, entry)(k, ids)
        return out if entry == "normals_hip" else out[0]
    alone = [run(_Set([c[:m]])) for c, m in zip(clouds, counts)]          # the counted rows of every cloud as a one-cloud set
    for i, pair in enumerate(DECOYS):                                      # nothing behind the count was read
        _check_normals((entry, "decoys", pair, k), alone[len(SET_ROWS) + i], "decoys", pair, k)
    for ids in (SELECTION, None):
        got = run(s, ids)
        for c in range(len(clouds)):
            rows = got[off[c]:off[c + 1]]
            if ids is not None and c not in ids:
                assert (rows == SENTINEL).all(), (entry, k, c)
                continue
            assert rows[:counts[c]].tobytes() == alone[c].tobytes(), (entry, k, c, "selected" if ids else "all")
            assert (rows[counts[c]:] == SENTINEL).all(), (entry, k, c)
    for i, pair in enumerate(DECOYS):                                      # (and in the set, by the bits above: stated for itself)
        c = len(SET_ROWS) + i
        _check_normals((entry, "decoys in the set", pair, k), got[off[c]:off[c] + counts[c]], "decoys", pair, k)


# ── through the fused ICP ────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def submap():
    """The maze submap of test_gpu_parity.py::test_submap_10k_target_on_sweep_path, its scan and its initial guess."""
    from icpmi import synth
    segs = synth.maze_segments()
    poses = synth.trajectory(90, step=0.35)
    sub = np.vstack([synth.to_world(synth.scan(p, 500 + i, segs=segs), p) for i, p in enumerate(poses)])
    sub = oracle.voxel_downsample(sub, 0.04)
    assert 8192 < len(sub) < 16000, len(sub)
    pose = poses[-1]
    cur = synth.scan(pose, 999, segs=segs)
    th = pose[2] + np.deg2rad(1.0)
    R0 = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return cur, sub, R0, np.array([pose[0] + 0.05, pose[1] - 0.04])


@pytest.mark.parametrize("normal_k", (7, 16, 31))
def test_submap_registration_at_other_list_widths(submap, normal_k):
    """The fast path (prep_big.hip), force_exhaustive (normals.hip) and the oracle on a submap of 9 946 rows of which the voxel
    filter keeps 5 375: the host routes by the capacity (a workspace for normals.hip, the sort scratch for prep_big.hip), the
    kernels work on the count.  The tolerances are those of test_submap_10k_target_on_sweep_path."""
    from icpmi import batch
    from test_gpu_parity import FRO_TOL
    cur, sub, R0, t0 = submap
    kw = dict(method="point_to_line", normal_k=normal_k)
    f = batch.IcpBatch([cur, sub], [0], [1], 1e-10, 30, 0.04, R_init=R0, t_init=t0, **kw)
    assert f.fast and f.max_tgt_n > 8192
    f.run()
    R, t, err, info = f.unpack()
    Ro, to, eo, io = oracle.icp(cur, sub, 1e-10, 30, 0.04, R_init=R0, t_init=t0, **kw)
    assert 4096 < io["n_tgt"] < len(sub)          # the voxel filter leaves fewer rows than the capacity the host routes by
    assert info["iters"][0] == io["iters"] and info["status"][0] == io["status"], (normal_k, info, io)
    assert rot_err(R[0], t[0], Ro, to) < FRO_TOL, normal_k
    e = batch.IcpBatch([cur, sub], [0], [1], 1e-10, 30, 0.04, R_init=R0, t_init=t0, force_exhaustive=True, **kw)
    assert not e.fast
    e.run()
    Re, te, ee, ie = e.unpack()
    assert ie["iters"][0] == info["iters"][0] and ie["status"][0] == info["status"][0], normal_k
    assert rot_err(R[0], t[0], Re[0], te[0]) < 1e-11, normal_k
