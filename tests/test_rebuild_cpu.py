"""Host side of the rebuild from the resident scan history (``ScanHistory.world_rows``, ``OccupancyGrid2D.replay_history``).

(i)  The contract of ``icpmi_history_world_rows`` is NumPy's ``p @ T[:2, :2].T + T[:2, 2]`` (slam.py:46-50) bit for bit, and
     that expression is BLAS: two or more rows are a gemm, whose element is fma(y, R[c][1], x * R[c][0]) + t[c]; exactly one
     row is a gemv, fma(x, R[c][0], y * R[c][1]) + t[c].  Both forms are evaluated here in exact rational arithmetic with one
     rounding per operation and held against NumPy on this platform: if its BLAS accumulated otherwise, this is where it
     would show.
(ii) ``reach_cell_box``, the cell box a replay piece gets from the host (pose and reach, no read-back), encloses the exact box
     of the piece's origins and NumPy-transformed rows."""
import ctypes
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest


def fl(q):
    """One rounding: the double nearest to a rational (int / int division is correctly rounded)."""
    return float(q)


def gemm_form(x, y, a, b, t):
    return fl(Fraction(fl(Fraction(y) * Fraction(b) + Fraction(fl(Fraction(x) * Fraction(a))))) + Fraction(t))


def gemv_form(x, y, a, b, t):
    return fl(Fraction(fl(Fraction(x) * Fraction(a) + Fraction(fl(Fraction(y) * Fraction(b))))) + Fraction(t))


def both_forms(p, T):
    out = {}
    for name, form in (("gemm", gemm_form), ("gemv", gemv_form)):
        out[name] = np.array([[form(float(x), float(y), float(T[c, 0]), float(T[c, 1]), float(T[c, 2])) for c in (0, 1)] for x, y in p])
    return out


def random_pose(rng):
    th = rng.uniform(-np.pi, np.pi)
    T = np.eye(3)
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:2, 2] = rng.uniform(-30.0, 30.0, size=2)
    return T


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_numpy_transform_is_the_gemm_form_and_one_row_the_gemv_form(n):
    rng = np.random.default_rng(100 + n)
    differ = 0
    for _ in range(40 if n == 1 else 6):
        p = rng.uniform(-12.0, 12.0, size=(n, 2))
        T = random_pose(rng)
        got = p @ T[:2, :2].T + T[:2, 2]                          # transform_points_2d, slam.py:46-50
        forms = both_forms(p, T)
        assert np.array_equal(got, forms["gemv" if n == 1 else "gemm"]), n
        differ += int((forms["gemm"] != forms["gemv"]).sum())
    assert differ > 0, "the two forms never differed: the cases tell nothing apart"


# ── (ii) the cell box from the host ──────────────────────────────────────────
GRID = SimpleNamespace(min_x=-20.0, min_y=-15.0, resolution=0.05)


def pose6(T):
    return np.array([T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 2], T[1, 2]])


def exact_box(grid, scans, poses):
    from utilities.mapping import OccupancyGrid2D, _minmax_rows
    rows = [np.array([T[:2, 2] for T in poses])] + [s @ T[:2, :2].T + T[:2, 2] for s, T in zip(scans, poses)]
    return OccupancyGrid2D._box_of(grid, *_minmax_rows(np.vstack(rows)))


def host_box(grid, scans, poses):
    from icpmi.history import scan_reach
    from utilities.mapping import reach_cell_box
    return reach_cell_box(grid, np.array([pose6(T) for T in poses]), [scan_reach(s) for s in scans])


def assert_encloses(grid, scans, poses):
    from icpmi.history import scan_reach
    box, exact = host_box(grid, scans, poses), exact_box(grid, scans, poses)
    assert box is not None and box.dtype == np.int32 and box.shape == (4,)
    assert box[0] <= exact[0] and box[1] <= exact[1] and box[2] >= exact[2] and box[3] >= exact[3], (box, exact)
    # and it is a reach box, not the plane: no further out than the longest reach (times the pose's norm) and a cell
    far = max(np.linalg.norm(T[:2, :2]) * scan_reach(s) for s, T in zip(scans, poses)) / grid.resolution + 2
    assert box[0] >= exact[0] - far and box[1] >= exact[1] - far and box[2] <= exact[2] + far and box[3] <= exact[3] + far, (box, exact)
    return box, exact


def test_scan_reach():
    from icpmi.history import scan_reach
    assert scan_reach(np.zeros((0, 2))) == 0.0
    assert scan_reach(np.array([[3.0, -4.0], [1.0, 1.0]])) == 5.0
    assert scan_reach(np.array([[1e-200, 0.0]])) == 1e-200 and scan_reach(np.array([[1e200, 1e200]])) > 1e200     # no under- or overflow
    assert np.isnan(scan_reach(np.array([[1.0, 2.0], [np.nan, 0.0], [5.0, 5.0]])))
    assert not np.isfinite(scan_reach(np.array([[np.inf, np.nan]]))) and scan_reach(np.array([[0.0, -np.inf]])) == np.inf


def test_host_box_encloses_the_exact_box_of_random_scans_and_poses():
    rng = np.random.default_rng(7)
    for trial in range(200):
        res = float(rng.choice([0.05, 0.1, 0.013, 1.0]))
        grid = SimpleNamespace(min_x=float(rng.uniform(-60, 0)), min_y=float(rng.uniform(-60, 0)), resolution=res)
        S = int(rng.integers(1, 6))
        scans, poses = [], []
        for _ in range(S):
            n = int(rng.choice([0, 1, 2, 17, 90]))
            ang = rng.uniform(-np.pi, np.pi, size=n) if trial % 3 else np.sort(rng.uniform(-0.3, 0.3, size=n))     # all round / a narrow fan
            rad = rng.uniform(0.1, 25.0, size=n)
            scans.append(np.column_stack([rad * np.cos(ang), rad * np.sin(ang)]))
            poses.append(random_pose(rng))
        assert_encloses(grid, scans, poses)


def test_host_box_with_an_accumulated_pose_and_a_row_at_the_origin():
    rng = np.random.default_rng(11)
    step = random_pose(rng)
    step[:2, 2] *= 0.002
    T = np.eye(3)
    for _ in range(500):                                           # 500 products: no longer orthonormal to the last bit
        T = T @ step
    assert not np.array_equal(T[:2, :2] @ T[:2, :2].T, np.eye(2))
    ang = rng.uniform(-np.pi, np.pi, size=360)
    scan = np.column_stack([12.0 * np.cos(ang), 12.0 * np.sin(ang)])
    assert_encloses(GRID, [scan], [T])
    S = np.diag([1.5, 0.25, 1.0]) @ T                             # and a pose that is not a rotation at all
    assert_encloses(GRID, [scan, scan[:1]], [S, T])
    # one row at the origin: reach 0, the box is the origin's own
    P = random_pose(rng)
    box, exact = assert_encloses(GRID, [np.zeros((1, 2))], [P])
    assert np.array_equal(box, exact)
    # rows exactly as far as the reach, along the axes, on a cell edge of the grid
    E = np.eye(3)
    E[:2, 2] = (GRID.min_x + 100 * GRID.resolution, GRID.min_y + 100 * GRID.resolution)
    r = 40 * GRID.resolution
    assert_encloses(GRID, [np.array([[r, 0.0], [-r, 0.0], [0.0, r], [0.0, -r]])], [E])


def test_host_box_gives_no_promise_for_a_nan():
    from utilities.mapping import reach_cell_box
    good = pose6(random_pose(np.random.default_rng(3)))
    assert reach_cell_box(GRID, [good, good], [1.0, 2.0]) is not None
    assert reach_cell_box(GRID, [good, good], [1.0, np.nan]) is None
    assert reach_cell_box(GRID, [good, good], [np.inf, 1.0]) is None
    for slot in range(6):
        bad = good.copy()
        bad[slot] = np.nan
        assert reach_cell_box(GRID, [good, bad], [1.0, 2.0]) is None, slot


def test_pose_rows_layout_and_refusals():
    from icpmi.history import pose_rows
    T = np.arange(18, dtype=np.float64).reshape(2, 3, 3)
    assert np.array_equal(pose_rows(list(T), 2), [[0, 1, 3, 4, 2, 5], [9, 10, 12, 13, 11, 14]])
    assert pose_rows([], 0).shape == (0, 6)
    for bad, n in ((T, 3), (T[:, :2], 2), (T[0], 1), (np.zeros((2, 6)), 2)):
        with pytest.raises(ValueError, match="poses"):
            pose_rows(bad, n)


def test_world_rows_entry_is_exported_bound_and_refuses_on_the_host():
    """No launch is reached below (no GPU is touched): a null argument is refused, an empty list is done."""
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    L = icpmi.lib()
    assert hasattr(ctypes.CDLL(path), "icpmi_history_world_rows") and "icpmi_history_world_rows" in _lib.EXPORTS
    fake = 4096                                                    # a non-null address that is never dereferenced
    h = _lib.History(fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, 0, 0, 0.06, 0.3, 4, 8192, 10, 1)
    assert L.icpmi_history_world_rows(ctypes.byref(h), None, 0, None, None, None, None) == 0
    assert L.icpmi_history_world_rows(ctypes.byref(_lib.History()), fake, 0, fake, fake, fake, None) == -1
    assert L.icpmi_history_world_rows(ctypes.byref(h), fake, -1, fake, fake, fake, None) == -1
    assert L.icpmi_history_world_rows(ctypes.byref(h), fake, 2 ** 31 - 1, fake, fake, fake, None) == -1
    for missing in range(4):
        args = [fake] * 4
        args[missing] = None
        assert L.icpmi_history_world_rows(ctypes.byref(h), args[0], 1, args[1], args[2], args[3], None) == -1, missing
