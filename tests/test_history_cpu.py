"""Host side of the resident scan history (icpmi.history): ``find_loop_candidates`` against the reference's
``_find_loop_candidates`` (slam.py:230-268; tests/golden/loop_candidates.npz, written by make_golden_history.py), and the
C ABI of the history as the header declares it."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

CASES = ("loop", "far_travel", "still", "few", "tie", "idx_n_none", "idx_n_some", "interval", "drive")
EMPTY = ("far_travel", "still", "idx_n_none", "interval")


def golden_case(z, name):
    xy = z[name + "_xy"]
    if xy.dtype.kind == "U":                                  # the name of the entry that holds the same trajectory
        xy = z[str(xy)]
    idx, thr, interval, max_c, travel = z[name + "_args"]
    return xy, z[name + "_cur"], int(idx), float(thr), int(interval), int(max_c), float(travel), z[name + "_ids"], z[name + "_dist"]


def pose_matrices(xy):
    th = np.linspace(0.0, 3.0, len(xy))                       # (the heading plays no part, slam.py:241, 258)
    P = np.tile(np.eye(3), (len(xy), 1, 1))
    P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    P[:, :2, 2] = xy
    return P


def test_fixture_holds_every_case():
    z = load_golden("loop_candidates")
    assert tuple(z["cases"]) == CASES
    for name in CASES:
        xy, _, _, _, _, _, _, ids, dist = golden_case(z, name)
        assert 60 <= len(xy) <= 200 and len(ids) == len(dist)
        assert (len(ids) == 0) == (name in EMPTY), name


@pytest.mark.parametrize("as_matrices", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_find_loop_candidates_equals_the_reference(name, as_matrices):
    """Ids and their order exactly; distances to rtol 1e-12 (thousands of ulps, far below the 1e-6 by which the fixture keeps
    every comparison of the reference away from equality)."""
    from icpmi import find_loop_candidates
    xy, cur, idx, thr, interval, max_c, travel, ids, dist = golden_case(load_golden("loop_candidates"), name)
    poses = pose_matrices(xy) if as_matrices else xy
    current = np.array([[1.0, 0.0, cur[0]], [0.0, 1.0, cur[1]], [0.0, 0.0, 1.0]]) if as_matrices else cur
    got = find_loop_candidates(current, list(poses) if as_matrices else poses, idx, thr, interval, max_c, travel)
    assert [k for k, _ in got] == [int(k) for k in ids], name
    assert all(isinstance(k, int) and isinstance(d, float) for k, d in got)
    np.testing.assert_allclose([d for _, d in got], dist, rtol=1e-12, atol=0.0)


def test_the_tie_keeps_scan_order():
    """Two poses at bit-identical positions: equal distances come back in scan order (the reference's list.sort is stable)."""
    from icpmi import find_loop_candidates
    xy, cur, idx, thr, interval, max_c, travel, ids, dist = golden_case(load_golden("loop_candidates"), "tie")
    assert np.array_equal(xy[19], xy[21])
    got = find_loop_candidates(cur, xy, idx, thr, interval, max_c, travel)
    pos = {k: i for i, (k, _) in enumerate(got)}
    assert pos[21] == pos[19] + 1 and got[pos[19]][1] == got[pos[21]][1]


def test_default_travel_gate_and_empty_history():
    from icpmi import find_loop_candidates
    xy, cur, idx, thr, interval, max_c, _, ids, _ = golden_case(load_golden("loop_candidates"), "loop")
    assert [k for k, _ in find_loop_candidates(cur, xy, idx, thr, interval, max_c)] == [int(k) for k in ids]   # 10.0, slam.py:232
    assert find_loop_candidates(cur, np.zeros((0, 2)), 0, thr, interval, max_c) == []


def test_history_entries_are_declared_exported_and_bound():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    icpmi.lib()
    L = ctypes.CDLL(path)
    for name in ("icpmi_history_add", "icpmi_history_search", "icpmi_prepared_relayout"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert icpmi.ScanHistory is icpmi.history.ScanHistory
    # the struct the three share, field by field as the header lists them
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    body = re.search(r"typedef struct icpmi_history \{(.*?)\} icpmi_history;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.History._fields_]
    assert ctypes.sizeof(_lib.History) == 11 * 8 + 2 * 8 + 2 * 8 + 4 * 4


def test_history_entries_refuse_bad_arguments_on_the_host():
    """Every refusal below is decided before any launch (no GPU is touched)."""
    import icpmi
    from icpmi import _lib
    L = icpmi.lib()
    off = np.zeros(5, dtype=np.int32)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    empty = _lib.History()
    assert L.icpmi_history_add(ctypes.byref(empty), offp, 0, 1, 1, None) == -1
    assert L.icpmi_history_search(ctypes.byref(empty), None, None, 0, 0, None, 1, None, None, 0, 0, None, None, None) == -1
    nbytes = L.icpmi_prepared_bytes(8192, 4, 0)
    fake = 4096                                                # a non-null address that is never dereferenced
    h = _lib.History(fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, nbytes, 256, 0.06, 0.3, 4, 8192, 10, 1)
    assert L.icpmi_history_add(ctypes.byref(h), offp, 0, 0, 1, None) == 0            # nothing to do
    assert L.icpmi_history_add(ctypes.byref(h), offp, 3, 2, 1, None) == -1           # beyond the scan capacity
    off[:] = (0, 4097, 4097, 4097, 4097)
    assert L.icpmi_history_add(ctypes.byref(h), offp, 0, 1, 1, None) == -4           # a scan above 4096 rows
    off[:] = (0, 4000, 8000, 12000, 12000)
    assert L.icpmi_history_add(ctypes.byref(h), offp, 2, 1, 1, None) == -1           # beyond the row capacity
    h.prepared_bytes = nbytes - 1
    off[:] = (0, 10, 10, 10, 10)
    assert L.icpmi_history_add(ctypes.byref(h), offp, 0, 1, 1, None) == -1           # prepared buffers too small for the capacities
    assert L.icpmi_prepared_relayout(None, 0, 0, 1, 0, fake, nbytes, 8192, 4, None) == -1       # rows in use, no source
    assert L.icpmi_prepared_relayout(fake, 100, 2, 50, 1, fake, nbytes, 40, 4, None) == -1      # shrinking
    assert L.icpmi_prepared_relayout(fake, 100, 2, 50, 1, fake, nbytes - 1, 8192, 4, None) == -2
