"""The per-cloud kernels that sort first (voxel.hip, prep.hip, normals.hip; shared pieces in sort.hpp) at the sizes where their
LDS layout or their launch changes: the 512- and the 1 024-thread voxel launch on all three sort forms, the prepare kernel on
both sides of every register-sort width, of its pair-sort fallback and of the hand-over to the global-memory path, and the
return codes of the two entry points for calls that launch nothing.  Everything against the project's own oracle, bit for
bit where no bound is stated.

The voxel clouds here are uniform: a voxel holds one point, or two at the largest voxel size, so these tests cross the switches
between the sort forms but cannot see the order in which a run of equal keys is summed (a + b commutes).  Runs of three and
more points on every one of these paths, keys on the rounding boundary of the divide and the clouds the filter refuses are
tested in tests/test_voxel_edges_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle
from test_gpu_parity import _assert_normals_are_the_eigenvectors

pytestmark = pytest.mark.gpu

# voxel sizes as test_voxel_all_three_sort_paths picks them, for a box of 20 m x 12 m (x 3 m): packed (key, row) values of a
# 1 025 .. 2 048-row cloud (2 048 slots) below 4e9 -> one 32-bit word on registers; between 4e9 and 9e18 -> the register path
# declines, 64-bit packed sort; above 9e18 -> (key, row) pairs
VOXELS = {2: (0.04, 0.002, 1e-7), 3: (0.2, 0.01, 1e-5)}
BOX = np.array([20.0, 12.0, 3.0])
# one cycle of the 257-cloud set; it starts at 2 048 rows so that member 0 (path independence) is a cloud the register path
# takes on 512 threads (four elements a thread) and on 1 024 (two)
CYCLE = (2048, 2049, 4097, 1, 64, 65, 512, 513, 1024, 1025)
SINGLES = (1024, 1025, 2048, 2049, 4096, 4097, 8192)


def _cloud(rng, n, dim):
    return rng.uniform(-0.5, 0.5, size=(n, dim)) * BOX[:dim] + np.array([3.0, -2.0, 1.0])[:dim]


@pytest.fixture(scope="module")
def cloud_sets():
    """dim -> (the 257 clouds: 256 through CYCLE and an empty one, their oracle outputs per voxel size); built once."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    sets = {}
    for dim in (2, 3):
        rng = np.random.default_rng(300 + dim)
        clouds = [_cloud(rng, CYCLE[i % len(CYCLE)], dim) for i in range(256)]
        clouds.insert(100, np.empty((0, dim)))
        ref = {v: [oracle.voxel_downsample(c, v) if len(c) else np.empty((0, dim)) for c in clouds] for v in VOXELS[dim]}
        sets[dim] = (clouds, ref)
    return sets


def _packed_range(cloud, voxel):
    """cells x slots of the kernel's packed sort: product of the key extents floor((max - min) / voxel) + 1, times 2 048"""
    ext = np.floor((cloud.max(0) - cloud.min(0)) / voxel) + 1.0
    return float(np.prod(ext)) * 2048.0


def _filter(clouds, voxel):
    from icpmi import batch
    return batch.voxel_downsample_set(batch.CloudSet.from_numpy(clouds), voxel).to_numpy()


@pytest.mark.parametrize("dim", [2, 3])
def test_voxel_512_thread_launch_on_all_three_sort_forms(cloud_sets, dim):
    """257 clouds: the smallest set whose launch takes 512 threads a workgroup."""
    clouds, ref = cloud_sets[dim]
    assert len(clouds) == 257
    mid = [c for c in clouds if 1025 <= len(c) <= 2048]
    assert len(mid) >= 25
    for voxel, (lo, hi) in zip(VOXELS[dim], ((0.0, 4.0e9), (4.0e9, 9.0e18), (9.0e18, np.inf))):
        ranges = [_packed_range(c, voxel) for c in mid]
        print(f"dim {dim} voxel {voxel}: packed range {min(ranges):.3g} .. {max(ranges):.3g}")
        assert all(lo <= r < hi for r in ranges), (dim, voxel, min(ranges), max(ranges))
        # (the pair sort still needs the keys themselves below 9e18: else the filter reports a cloud it cannot key)
        assert max(ranges) / 2048.0 < 9.0e18
        out = _filter(clouds, voxel)
        for i, (o, r) in enumerate(zip(out, ref[voxel])):
            assert o.shape == r.shape and np.array_equal(o, r), (dim, voxel, i, len(clouds[i]))


@pytest.mark.parametrize("n", SINGLES)
def test_voxel_1024_thread_launch_on_all_three_sort_forms(n):
    """A lone cloud runs on 1 024 threads: both register-sort widths (1 025 .. 2 048 and 2 049 .. 4 096 rows), the LDS sorts
    on either side of them, and the largest cloud of the one-workgroup path."""
    cloud = _cloud(np.random.default_rng(1000 + n), n, 2)
    for voxel in VOXELS[2]:
        got, ref = _filter([cloud], voxel)[0], oracle.voxel_downsample(cloud, voxel)
        assert got.shape == ref.shape and np.array_equal(got, ref), (n, voxel)


@pytest.mark.parametrize("dim", [2, 3])
def test_voxel_output_does_not_depend_on_the_launch(cloud_sets, dim):
    """The same cloud alone (1 024 threads, LDS sized to it) and as a member of the 257-cloud set (512 threads, LDS sized to
    the largest member): the same bits.  Member 0, and with it one cloud of every size of the cycle."""
    clouds, _ = cloud_sets[dim]
    for voxel in VOXELS[dim]:
        in_set = _filter(clouds, voxel)
        for i in range(len(CYCLE)):
            alone = _filter([clouds[i]], voxel)[0]
            assert alone.shape == in_set[i].shape and np.array_equal(alone, in_set[i]), (dim, voxel, i, len(clouds[i]))


# ── prepare kernel ──────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("n", (511, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097))
def test_prepare_layout_switches(libopt, n):
    """estimate_normals_2d, k = 12, around every size at which the prepare kernel lays its LDS out differently: register sort
    of 512, 1 024, 2 048 slots, the pair sort for 4 096, and beyond 4 096 rows the kernels that work in global memory.  The grid
    search (scratch behind the sorted copy) and the sweep (scratch on it) find the same neighbours in the same order."""
    from utilities import icp as uicp
    pts = np.random.default_rng(2000 + n).uniform(-4, 4, size=(n, 2))
    got = {}
    for mode in ("grid", "sweep"):
        libopt.setenv("ICPMI_PREP_KNN", mode)
        got[mode] = uicp.estimate_normals_2d(pts, 12)
    assert np.array_equal(got["grid"], got["sweep"]), n
    ref = oracle.normals_2d(pts, 12)
    for mode in ("grid", "sweep"):
        worst = np.abs(np.abs(np.sum(got[mode] * ref, axis=1)) - 1).max()
        print(f"n {n} {mode}: ||n.n_ref| - 1| <= {worst:.3g}")
        assert worst < 1e-9, (n, mode, worst)                        # the bound of test_normals_sizes


def test_prepare_sort_only_then_any_k():
    """k = 40 at 2 049 rows: the sort-only instantiation (pair sort of 4 096 slots on the sorted copy), then the any-k launch
    on what it wrote; held to the bound of test_normals_and_icp_with_more_than_31_neighbours."""
    from utilities import icp as uicp
    pts = np.random.default_rng(2049).uniform(-4, 4, size=(2049, 2))
    _assert_normals_are_the_eigenvectors(uicp.estimate_normals_2d(pts, 40), pts, 40, (2049, 40), False)


# ── return codes of calls that launch nothing ───────────────────────────────────────────────────────────────────────
OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -2, -4           # include/icpmi.h


@pytest.fixture(scope="module")
def raw():
    """Device buffers for calls through the C ABI: 16 rows of points, outputs, and a host offset array to fill in."""
    import torch
    from icpmi import _lib
    from icpmi.batch import _ptr, _stream
    dev = torch.device("cuda", torch.cuda.current_device())

    class Raw:
        L = _lib.lib()
        pts = torch.zeros((16, 2), dtype=torch.float64, device=dev)
        out = torch.zeros((16, 2), dtype=torch.float64, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        off = torch.zeros(4, dtype=torch.int32, device=dev)

        def voxel(self, off_host, n_clouds, dim, voxel, workspace=None):
            off_host = np.ascontiguousarray(off_host, dtype=np.int32)
            return self.L.icpmi_voxel_downsample_batch(_ptr(self.pts), _ptr(self.off), off_host.ctypes.data_as(C.c_void_p), n_clouds, dim,
                                                       voxel, _ptr(self.out), _ptr(self.cnt), _ptr(workspace),
                                                       0 if workspace is None else workspace.numel(), _stream())

        def prepare(self, off_host, n_clouds, total_rows, max_n, k, prepared, prepared_bytes):
            oh = None if off_host is None else np.ascontiguousarray(off_host, dtype=np.int32).ctypes.data_as(C.c_void_p)
            return self.L.icpmi_prepare_targets_ex(_ptr(self.pts), _ptr(self.off), oh, None, None, None, n_clouds, n_clouds, total_rows,
                                                   max_n, k, None, _ptr(prepared), prepared_bytes, 1, _stream())
    return Raw()


def test_voxel_return_codes(raw):
    assert raw.voxel([0, 16], 1, 4, 0.1) == ERR_ARG                    # dim = 4
    assert raw.voxel([0, 16], 1, 2, 0.0) == ERR_ARG                    # voxel_size = 0
    assert raw.voxel([0, 16, 8], 2, 2, 0.1) == ERR_ARG                 # a negative row count
    assert raw.voxel([0, 8193], 1, 2, 0.1) == ERR_WORKSPACE            # a cloud for the large path, no workspace
    assert raw.voxel([0], 0, 2, 0.1) == OK                             # no clouds


def test_prepare_return_codes(raw):
    import torch
    L = raw.L
    big = L.icpmi_prepared_bytes(5000, 1, 5000)
    prepared = torch.empty(big, dtype=torch.uint8, device=raw.pts.device)
    assert raw.prepare(None, 1, 5000, 5000, 12, prepared, big) == ERR_ARG                # max_n > 4 096 needs the host offsets
    need = L.icpmi_prepared_bytes(16, 1, 16)
    assert raw.prepare([0, 16], 1, 16, 16, 7000, prepared, need) == ERR_UNSUPPORTED       # k beyond 6 143
    assert raw.prepare([0, 16], 1, 16, 16, 12, prepared, need - 1) == ERR_WORKSPACE       # one byte short
