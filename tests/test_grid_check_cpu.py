"""Host side of the check (include/icpmi.h: icpmi_grid_check_batch): the C ABI as the header declares it, every refusal the
entry decides on the host — before anything is enqueued, so no GPU is touched (the device pointers are fakes that are never
dereferenced) — and the NumPy restatement the device test compares against (tests/gridcheck_ref.py): its hand-made rows
against literal records, a room in which every beam is confirmed exactly, and the room map of the grid-matching suite, where
the rule separates true poses from displaced ones."""
import ctypes
import os
import re

import numpy as np

import gridcast_ref as cref
import gridcheck_ref as ref
import gridmatch_ref as gref
from conftest import REPO

FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


def test_entry_and_constants_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    name = "icpmi_grid_check_batch"
    assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"\b" + name + r"\(", hdr)
    proto = re.search(r"^int " + name + r"\((.*?)\);", hdr, flags=re.S | re.M).group(1)
    assert len(proto.split(",")) == 25 == len(lib.icpmi_grid_check_batch.argtypes)
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GK_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"GK_THREADS": 256, "GK_CHUNK_ROWS": 256, "GK_MAX_TOLERANCE": 2 ** 30, "GK_INTS": 8, "GK_REC_STATUS": 0, "GK_REC_ROWS": 1,
                       "GK_REC_CONFIRMED": 2, "GK_REC_VIOLATED": 3, "GK_REC_IN_FREE": 4, "GK_REC_UNEXPLORED": 5, "GK_REC_THROUGH_UNKNOWN": 6,
                       "GK_ST_OK": 0, "GK_ST_EMPTY": 1, "GK_ST_CAPACITY": 2, "GK_CLASS_CONFIRMED": 0, "GK_CLASS_VIOLATED": 1,
                       "GK_CLASS_IN_FREE": 2, "GK_CLASS_UNEXPLORED": 3, "GK_NO_CELLS": -2, "GK_ROW_INTS": 4, "GK_ROW_CLASS": 0,
                       "GK_ROW_K_HIT": 1, "GK_ROW_K": 2, "GK_ROW_K_UNKNOWN": 3}
    assert defines == {k: getattr(_lib, k) for k in defines}
    assert sorted(k for k in vars(_lib) if k.startswith("GK_")) == sorted(defines)
    assert (ref.INTS, ref.ROW_INTS, ref.STATUS, ref.ROWS, ref.CONFIRMED, ref.VIOLATED, ref.IN_FREE, ref.UNEXPLORED, ref.THROUGH_UNKNOWN) == (
        _lib.GK_INTS, _lib.GK_ROW_INTS, _lib.GK_REC_STATUS, _lib.GK_REC_ROWS, _lib.GK_REC_CONFIRMED, _lib.GK_REC_VIOLATED, _lib.GK_REC_IN_FREE,
        _lib.GK_REC_UNEXPLORED, _lib.GK_REC_THROUGH_UNKNOWN)
    assert (ref.ST_OK, ref.ST_EMPTY, ref.ST_CAPACITY, ref.CLASS_CONFIRMED, ref.CLASS_VIOLATED, ref.CLASS_IN_FREE, ref.CLASS_UNEXPLORED, ref.NO_CELLS) == (
        _lib.GK_ST_OK, _lib.GK_ST_EMPTY, _lib.GK_ST_CAPACITY, _lib.GK_CLASS_CONFIRMED, _lib.GK_CLASS_VIOLATED, _lib.GK_CLASS_IN_FREE,
        _lib.GK_CLASS_UNEXPLORED, _lib.GK_NO_CELLS)
    assert (ref.MAX_ROWS, ref.MAX_TOLERANCE) == (_lib.GM_MAX_ROWS, _lib.GK_MAX_TOLERANCE)
    # nothing new matches the cast's prefix: its set is what it was
    cast = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GC_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert cast == {"GC_INTS": 4, "GC_K_HIT": 0, "GC_X_HIT": 1, "GC_Y_HIT": 2, "GC_K_UNKNOWN": 3, "GC_NONE": -1, "GC_NO_CELLS": -2, "GC_THREADS": 256}


def test_entry_refuses_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    need = L.icpmi_grid_occupancy_planes_bytes(400, 560)
    inf, nan = float("inf"), float("nan")

    def check(field=FAKE, kept=None, ny=400, nx=560, min_x=-14.0, min_y=-10.0, res=0.1, pts=FAKE, off_dev=FAKE, off=(0, 100, 100, 360),
              off_host=True, cnt=None, pair_dev=FAKE, pair=(0, 2, 1, 2), pair_host=True, n_clouds=None, n_pairs=None, pair_t=FAKE,
              cos_sin=FAKE, tolerance=2, out=FAKE, out_rows=None, row_stride=0, ws=FAKE, ws_bytes=need):
        off_a, pair_a = np.array(off, dtype=np.int32), np.array(pair, dtype=np.int32)
        return L.icpmi_grid_check_batch(field, kept, ny, nx, 2048, min_x, min_y, res, pts, off_dev, off_a.ctypes.data if off_host else None,
                                        cnt, len(off_a) - 1 if n_clouds is None else n_clouds, pair_dev, pair_a.ctypes.data if pair_host else None,
                                        len(pair_a) if n_pairs is None else n_pairs, pair_t, cos_sin, tolerance, out, out_rows, row_stride,
                                        ws, ws_bytes, None)

    # the grid limits are the cast's
    assert check(ny=-1) == ERR_ARG and check(nx=(1 << 29) + 1, ny=1) == ERR_ARG and check(ny=1 << 16, nx=1 << 15) == ERR_ARG
    # the map: a field with a workspace, or kept planes
    assert check(field=None) == ERR_ARG and check(field=FAKE + 2) == ERR_ARG and check(kept=FAKE + 4) == ERR_ARG
    assert check(ws=None) == ERR_WORKSPACE and check(ws_bytes=need - 1) == ERR_WORKSPACE and check(ws=FAKE + 4) == ERR_WORKSPACE
    # the cloud set and the pairs are the matcher's
    assert check(n_pairs=-1) == ERR_ARG and check(n_clouds=-1) == ERR_ARG and check(off_host=False) == ERR_ARG and check(pair_host=False) == ERR_ARG
    assert check(pair=(0, 3)) == ERR_ARG and check(pair=(-1,)) == ERR_ARG and check(off=(0, 100, 90, 360)) == ERR_ARG
    assert check(off=(0, 65536), pair=(0,)) == ERR_UNSUPPORTED and check(off=(0, 65535), pair=(0,) * 8193) == ERR_UNSUPPORTED
    for name in ("pts", "off_dev", "pair_dev", "pair_t", "cos_sin", "out"):
        assert check(**{name: None}) == ERR_ARG, name
    assert check(pts=FAKE + 8) == ERR_ARG
    # the tolerance
    assert check(tolerance=-1) == ERR_ARG and check(tolerance=(1 << 30) + 1) == ERR_ARG
    # the rows' records
    assert check(out_rows=FAKE + 4, row_stride=260) == ERR_ARG and check(out_rows=FAKE, row_stride=259) == ERR_ARG
    assert check(out_rows=FAKE, row_stride=99, pair=(0, 0)) == ERR_ARG and check(out_rows=FAKE, row_stride=-1) == ERR_ARG
    for bad in (0.0, -0.1, inf, nan):
        assert check(res=bad) == ERR_ARG
    assert check(min_x=nan) == ERR_ARG and check(min_y=inf) == ERR_ARG
    # nothing to do is no refusal, whatever else is passed
    assert check(pair=(), field=None, ws=None, out=None, pts=None) == 0 and check(n_pairs=0, tolerance=-1, res=nan) == 0


def test_the_largest_sum_of_rows_that_is_refused_is_two_to_the_29():
    """65 535 rows named 8 193 times are 536 928 255 >= 2^29 rows: refused; 8 192 times are 536 862 720 < 2^29: those pass the
    host's checks — seen here through the NEXT refusal in line, a null output, instead of a launch."""
    import icpmi
    L = icpmi.lib()
    off = np.array([0, 65535], dtype=np.int32)

    def check(times, out):
        pair = np.zeros(times, dtype=np.int32)
        return L.icpmi_grid_check_batch(None, FAKE, 400, 560, 2048, -14.0, -10.0, 0.1, FAKE, FAKE, off.ctypes.data, None, 1, FAKE, pair.ctypes.data,
                                        times, FAKE, FAKE, 2, out, None, 0, None, 0, None)

    assert 65535 * 8193 >= 2 ** 29 > 65535 * 8192
    assert check(8193, FAKE) == ERR_UNSUPPORTED and check(8192, None) == ERR_ARG
    # 2^23 pairs of an empty cloud and one of 65 535 rows: few rows, but 2^31 (pair, chunk) workgroups and more
    off = np.array([0, 0, 65535], dtype=np.int32)
    pair = np.zeros(2 ** 23 + 1, dtype=np.int32)
    pair[-1] = 1
    call = lambda n, out: L.icpmi_grid_check_batch(None, FAKE, 400, 560, 2048, -14.0, -10.0, 0.1, FAKE, FAKE, off.ctypes.data, None, 2, FAKE,   # noqa: E731
                                                   pair[-n:].ctypes.data, n, FAKE, FAKE, 2, out, None, 0, None, 0, None)
    assert call(2 ** 23 + 1, FAKE) == ERR_UNSUPPORTED and call(2 ** 23 - 1, None) == ERR_ARG


def test_hand_made_rows_have_their_literal_records():
    field, cases = ref.hand_made()
    assert field.shape == (1, 200)
    for case in cases:
        pts, t, cs = ref.hand_made_pair(case)
        rec, rows = ref.check_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, case[2])
        assert rec.tolist() == case[3] and rows.tolist() == case[4], case
        assert rec[ref.CONFIRMED:ref.UNEXPLORED + 1].sum() == rec[ref.ROWS]
    # the matcher's rule for a device count: shortened, negative, over-long
    pts, t, cs = ref.hand_made_pair(cases[11])
    rec, rows = ref.check_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, 0, cnt=3)
    assert rec.tolist() == [ref.ST_OK, 2, 1, 1, 0, 0, 0, 0] and len(rows) == 3
    for cnt in (-1, 7):
        rec, rows = ref.check_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, 0, cnt=cnt)
        assert rec.tolist() == [ref.ST_CAPACITY, 0, 0, 0, 0, 0, 0, 0] and len(rows) == 0


def room_scan(field, centre):
    """The centres of the first wall cells gridcast_ref.cast_rays finds from the centre of ``centre`` along 360 bearings, in
    the sensor frame of that pose under heading 0 -> (pts (360, 2), the hit cells (360, 2))."""
    xy = [[centre[0] + 0.5, centre[1] + 0.5]]
    bearings = np.deg2rad(np.arange(360.0))
    rec, _, ok = cref.cast_rays(field, cref.THRESHOLD, 0.0, 0.0, 1.0, xy, [[1.0, 0.0]], gref.cos_sin_of(bearings), 40.0)
    assert ok.all() and (rec[0, :, 0] >= 0).all()
    cells = rec[0, :, 1:3].astype(np.int64)
    return (cells + 0.5) - np.array(xy[0]), cells


def test_an_exact_room_is_confirmed_beam_for_beam_and_a_shifted_pose_is_not():
    """Walls two cells thick, the pose at the centre of the centre cell: every beam to the centre of the first wall cell on
    its bearing is major-axis towards its wall and reaches the wall's coordinate only at its last step, so at tolerance 0
    all 360 are confirmed.  From a pose 4 cells along +x the beams that ended on the +x wall (off the corners) now end
    behind it — violated — and those of the -x wall end inside the room — in free space."""
    field, (cx, cy) = ref.exact_room()
    n = field.shape[0]
    lo, hi = 5, n - 6                                              # the first and last free column: the inner layers are lo - 1, hi + 1
    assert field[cy, lo] == -9 and field[cy, lo - 1] == cref.THRESHOLD and field[cy, hi] == -9 and field[cy, hi + 1] == cref.THRESHOLD
    pts, cells = room_scan(field, (cx, cy))
    assert set(np.abs(cells - [cx, cy]).max(axis=1).tolist()) == {hi + 1 - cx}                      # every hit lies on the inner layer
    rec, rows = ref.check_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, (cx + 0.5, cy + 0.5), (1.0, 0.0), 0)
    print("centre:", rec.tolist())
    assert rec.tolist() == [ref.ST_OK, 360, 360, 0, 0, 0, 0, 0] and (rows[:, 1] == rows[:, 2]).all()
    off_corner = (cells[:, 1] >= lo) & (cells[:, 1] <= hi)
    plus_x, minus_x = int((off_corner & (cells[:, 0] == hi + 1)).sum()), int((off_corner & (cells[:, 0] == lo - 1)).sum())
    rec, _ = ref.check_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, (cx + 4.5, cy + 0.5), (1.0, 0.0), 0)
    print("shifted:", rec.tolist(), "beams on the +x wall", plus_x, "on the -x wall", minus_x)
    assert plus_x > 40 and minus_x > 40
    assert rec[ref.ROWS] == 360 and rec[ref.VIOLATED] >= plus_x and rec[ref.IN_FREE] >= minus_x


DISPLACEMENTS = ((0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, np.deg2rad(10.0)), (2.0, 1.0, 0.3))


def test_the_rule_separates_true_from_displaced_poses_in_the_room_map():
    """The room map of tests/test_grid_cast_cpu.py::room_field, scans synth.scan(SCENE_POSES[n], 50 + n)[::4] for n = 0, 5,
    11, threshold rint(0.5 * 2^12).  At tolerance 2 a true pose has at most 15 of 512 beams violated (3 %; 10, 3, 5 when this
    was written) and each of five displacements at least 102 (20 %; the least was 113); at tolerance 0 the true poses fail with
    more than 100, because a noisy return lands a cell behind the first occupied layer of a mapped wall."""
    from icpmi import synth
    from test_grid_cast_cpu import room_field
    q, g = room_field()
    threshold = int(np.rint(0.5 * 2.0 ** 12))

    def walks(pts, pose):
        return ref.walk_rows(q, threshold, g["min_x"], g["min_y"], 0.1, pts, pose[:2], (np.cos(pose[2]), np.sin(pose[2])))

    for n in (0, 5, 11):
        pose = gref.SCENE_POSES[n]
        pts = synth.scan(pose, 50 + n)[::4]
        assert len(pts) == 512
        at_pose = walks(pts, pose)
        rec, rec0 = ref.classify(at_pose, 2)[0], ref.classify(at_pose, 0)[0]
        print(f"pose {n}: tolerance 2 {rec.tolist()}, tolerance 0 violated {rec0[ref.VIOLATED]}")
        assert rec[ref.ROWS] == 512 and rec[ref.VIOLATED] <= 15 and rec0[ref.VIOLATED] > 100
        for d in DISPLACEMENTS:
            moved = ref.classify(walks(pts, (pose[0] + d[0], pose[1] + d[1], pose[2] + d[2])), 2)[0]
            print(f"pose {n} + {d}: {moved.tolist()}")
            assert moved[ref.ROWS] == 512 and moved[ref.VIOLATED] >= 102
