"""Host side of the beam model (include/icpmi.h: icpmi_grid_beam_batch): the C ABI as the header declares it, every refusal
the entry decides on the host — before anything is enqueued, so no GPU is touched (the device pointers are fakes that are
never dereferenced) — the table and the weights the Python layer forms on the host, and the NumPy restatement the device test
compares against (tests/gridbeam_ref.py): its hand-made rows against literal records, its walks at beyond = 0 against the
check's restatement, and the room map of the grid-matching suite, where the score separates true poses from displaced ones
down to one cell and two degrees."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridbeam_ref as ref
import gridcast_ref as cref
import gridcheck_ref as kref
import gridmatch_ref as gref
from conftest import REPO

FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
TABLE_0P1_0P1_8 = [-2250, -2250, -2250, -2250, -2247, -2163, -1499, -441, 0, -279, -1097, -1496, -1539, -1540, -1540, -1540, -1540, -1540, -1540]


def test_entry_and_constants_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    name = "icpmi_grid_beam_batch"
    assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name)
    proto = re.search(r"^int " + name + r"\((.*?)\);", hdr, flags=re.S | re.M).group(1)
    assert len(proto.split(",")) == 28 == len(lib.icpmi_grid_beam_batch.argtypes)
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GB_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"GB_THREADS": 256, "GB_CHUNK_ROWS": 256, "GB_MAX_HALF_WIDTH": 127, "GB_TABLE_CLIP": 32767, "GB_INTS": 8, "GB_REC_STATUS": 0,
                       "GB_REC_ROWS": 1, "GB_REC_SCORE": 2, "GB_REC_EXPECTED": 3, "GB_REC_NOVEL": 4, "GB_REC_UNEXPLORED": 5, "GB_ST_OK": 0,
                       "GB_ST_EMPTY": 1, "GB_ST_CAPACITY": 2, "GB_NO_CELLS": -2, "GB_ROW_INTS": 4, "GB_ROW_INDEX": 0, "GB_ROW_K_HIT": 1,
                       "GB_ROW_K_Z": 2, "GB_ROW_K_UNKNOWN": 3}
    assert defines == {k: getattr(_lib, k) for k in defines}
    assert sorted(k for k in vars(_lib) if k.startswith("GB_")) == sorted(defines)
    assert (ref.INTS, ref.ROW_INTS, ref.STATUS, ref.ROWS, ref.SCORE, ref.EXPECTED, ref.NOVEL, ref.UNEXPLORED) == (
        _lib.GB_INTS, _lib.GB_ROW_INTS, _lib.GB_REC_STATUS, _lib.GB_REC_ROWS, _lib.GB_REC_SCORE, _lib.GB_REC_EXPECTED, _lib.GB_REC_NOVEL,
        _lib.GB_REC_UNEXPLORED)
    assert (ref.ST_OK, ref.ST_EMPTY, ref.ST_CAPACITY, ref.NO_CELLS, ref.MAX_HALF_WIDTH, ref.TABLE_CLIP, ref.MAX_ROWS) == (
        _lib.GB_ST_OK, _lib.GB_ST_EMPTY, _lib.GB_ST_CAPACITY, _lib.GB_NO_CELLS, _lib.GB_MAX_HALF_WIDTH, _lib.GB_TABLE_CLIP, _lib.GM_MAX_ROWS)
    assert ref.TABLE_CLIP * ref.MAX_ROWS < 2 ** 31 and max(ref.HALF_WIDTHS) == ref.MAX_HALF_WIDTH


def test_entry_refuses_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    need = L.icpmi_grid_occupancy_planes_bytes(400, 560)
    inf, nan = float("inf"), float("nan")

    def beam(field=FAKE, kept=None, ny=400, nx=560, min_x=-14.0, min_y=-10.0, res=0.1, pts=FAKE, off_dev=FAKE, off=(0, 100, 100, 360),
             off_host=True, cnt=None, pair_dev=FAKE, pair=(0, 2, 1, 2), pair_host=True, n_clouds=None, n_pairs=None, pair_t=FAKE,
             cos_sin=FAKE, beyond=1.5, H=8, table=FAKE, out=FAKE, out_hist=None, out_rows=None, row_stride=0, ws=FAKE, ws_bytes=need):
        off_a, pair_a = np.array(off, dtype=np.int32), np.array(pair, dtype=np.int32)
        return L.icpmi_grid_beam_batch(field, kept, ny, nx, 2048, min_x, min_y, res, pts, off_dev, off_a.ctypes.data if off_host else None,
                                       cnt, len(off_a) - 1 if n_clouds is None else n_clouds, pair_dev, pair_a.ctypes.data if pair_host else None,
                                       len(pair_a) if n_pairs is None else n_pairs, pair_t, cos_sin, beyond, H, table, out, out_hist, out_rows,
                                       row_stride, ws, ws_bytes, None)

    # the grid limits are the cast's
    assert beam(ny=-1) == ERR_ARG and beam(nx=(1 << 29) + 1, ny=1) == ERR_ARG and beam(ny=1 << 16, nx=1 << 15) == ERR_ARG
    # the map: a field with a workspace, or kept planes
    assert beam(field=None) == ERR_ARG and beam(field=FAKE + 2) == ERR_ARG and beam(kept=FAKE + 4) == ERR_ARG
    assert beam(ws=None) == ERR_WORKSPACE and beam(ws_bytes=need - 1) == ERR_WORKSPACE and beam(ws=FAKE + 4) == ERR_WORKSPACE
    # the cloud set and the pairs are the matcher's
    assert beam(n_pairs=-1) == ERR_ARG and beam(n_clouds=-1) == ERR_ARG and beam(off_host=False) == ERR_ARG and beam(pair_host=False) == ERR_ARG
    assert beam(pair=(0, 3)) == ERR_ARG and beam(pair=(-1,)) == ERR_ARG and beam(off=(0, 100, 90, 360)) == ERR_ARG
    assert beam(off=(0, 65536), pair=(0,)) == ERR_UNSUPPORTED and beam(off=(0, 65535), pair=(0,) * 8193) == ERR_UNSUPPORTED
    for name in ("pts", "off_dev", "pair_dev", "pair_t", "cos_sin", "out", "table"):
        assert beam(**{name: None}) == ERR_ARG, name
    assert beam(pts=FAKE + 8) == ERR_ARG and beam(table=FAKE + 4) == ERR_ARG
    # beyond and the half width
    for bad in (-0.0001, -inf, inf, nan):
        assert beam(beyond=bad) == ERR_ARG, bad
    assert beam(H=-1) == ERR_ARG and beam(H=128) == ERR_ARG
    # the histograms and the rows' records
    assert beam(out_hist=FAKE + 4) == ERR_ARG
    assert beam(out_rows=FAKE + 4, row_stride=260) == ERR_ARG and beam(out_rows=FAKE, row_stride=259) == ERR_ARG
    assert beam(out_rows=FAKE, row_stride=99, pair=(0, 0)) == ERR_ARG and beam(out_rows=FAKE, row_stride=-1) == ERR_ARG
    for bad in (0.0, -0.1, inf, nan):
        assert beam(res=bad) == ERR_ARG
    assert beam(min_x=nan) == ERR_ARG and beam(min_y=inf) == ERR_ARG
    # what is allowed passes every check up to the last one in line (the workspace), with each output, at the limits
    for ok in (dict(), dict(beyond=0.0), dict(beyond=1e300), dict(H=0), dict(H=127), dict(out_hist=FAKE), dict(out_rows=FAKE, row_stride=260)):
        assert beam(ws_bytes=need - 1, **ok) == ERR_WORKSPACE, ok
    # nothing to do is no refusal, whatever else is passed
    assert beam(pair=(), field=None, ws=None, out=None, pts=None, table=None) == 0 and beam(n_pairs=0, beyond=nan, H=-1, res=nan) == 0


def test_the_largest_sum_of_rows_that_is_refused_is_two_to_the_29():
    """The check's two limits, seen through the NEXT refusal in line, a null output, instead of a launch: 65 535 rows named
    8 193 times reach 2^29 rows and 8 192 times do not; 2^23 + 1 pairs with a cloud of 65 535 rows among them reach 2^31
    (pair, chunk) workgroups and 2^23 - 1 do not."""
    import icpmi
    L = icpmi.lib()
    off = np.array([0, 65535], dtype=np.int32)

    def beam(times, out):
        pair = np.zeros(times, dtype=np.int32)
        return L.icpmi_grid_beam_batch(None, FAKE, 400, 560, 2048, -14.0, -10.0, 0.1, FAKE, FAKE, off.ctypes.data, None, 1, FAKE, pair.ctypes.data,
                                       times, FAKE, FAKE, 1.5, 8, FAKE, out, None, None, 0, None, 0, None)

    assert 65535 * 8193 >= 2 ** 29 > 65535 * 8192
    assert beam(8193, FAKE) == ERR_UNSUPPORTED and beam(8192, None) == ERR_ARG
    off2 = np.array([0, 0, 65535], dtype=np.int32)
    pair = np.zeros(2 ** 23 + 1, dtype=np.int32)
    pair[-1] = 1
    call = lambda n, out: L.icpmi_grid_beam_batch(None, FAKE, 400, 560, 2048, -14.0, -10.0, 0.1, FAKE, FAKE, off2.ctypes.data, None, 2, FAKE,   # noqa: E731
                                                  pair[-n:].ctypes.data, n, FAKE, FAKE, 1.5, 8, FAKE, out, None, None, 0, None, 0, None)
    assert call(2 ** 23 + 1, FAKE) == ERR_UNSUPPORTED and call(2 ** 23 - 1, None) == ERR_ARG


def test_the_table_of_the_mixture():
    from icpmi import gridmatch
    t = gridmatch.beam_table(0.1, 0.1, 8)
    assert t.dtype == np.int32 and t.tolist() == TABLE_0P1_0P1_8
    t_peak = lambda res, sigma: max(0.9, 0.8 * np.exp(-res ** 2 / (2.0 * sigma ** 2)) + 0.2)          # noqa: E731  (p at d = 0 and at d = 1)
    for res, sigma, H in ((0.1, 0.1, 8), (0.05, 0.12, 20), (0.25, 0.1, 0), (0.1, 0.3, 127), (0.1, 0.01, 3)):
        t = gridmatch.beam_table(res, sigma, H)
        assert t.shape == (2 * H + 3,) and t.max() == 0 and (t <= 0).all() and (t >= -32767).all()
        # non-increasing away from d = 0 on each side; d = 0 itself is the best difference while the Gaussian loses more
        # over one step than the floor of short returns adds: 0.8 * (1 - exp(-res^2 / (2 sigma^2))) >= 0.1, res >= 0.517 sigma
        # (the second and the fourth case are wider than that: there d = 1 is the best, in the second d = 0 scores
        # rint(1024 ln(0.9 / 0.934)) = -37)
        assert (np.diff(t[:H + 1]) >= 0).all() and (np.diff(t[H + 1:2 * H + 1]) <= 0).all()
        assert t[H] == int(np.rint(1024 * np.log(0.9 / t_peak(res, sigma)))) and (t[H] == 0) == (res >= 0.517 * sigma)
        assert res >= 0.517 * sigma or (t[H + 1] == 0 and ((res, sigma) != (0.05, 0.12) or t[H] == -37))
        assert t[2 * H + 1] == t[2 * H + 2] == int(np.rint(1024 * np.log(0.2 / t_peak(res, sigma))))
    # the last entry on its own; an impossible class is the clip, not -inf; another scale
    assert gridmatch.beam_table(0.1, 0.1, 8, unexplored=0.9)[-1] == 0 and gridmatch.beam_table(0.1, 0.1, 8, unexplored=0.0)[-1] == -32767
    assert gridmatch.beam_table(0.1, 0.1, 8, unexplored=0.9)[:-1].tolist() == TABLE_0P1_0P1_8[:-1]
    assert gridmatch.beam_table(0.1, 0.1, 2, scale=100).tolist() == [int(np.rint(100 * np.log(p / 0.9))) for p in (
        0.8 * np.exp(-2.0) + 0.1, 0.8 * np.exp(-0.5) + 0.1, 0.9, 0.8 * np.exp(-0.5) + 0.2, 0.8 * np.exp(-2.0) + 0.2, 0.2, 0.2)]
    for bad in (dict(half_width=-1), dict(half_width=128), dict(half_width=1.5), dict(sigma=0.0), dict(resolution=float("nan")), dict(z_hit=-0.1),
                dict(z_hit=0.0, z_rand=0.0), dict(scale=0)):
        with pytest.raises(ValueError):
            gridmatch.beam_table(**{**dict(resolution=0.1, sigma=0.1, half_width=8), **bad})


def test_pose_weights_are_a_softmax_about_the_maximum():
    from icpmi import gridmatch
    w, ess = gridmatch.pose_weights(np.full(7, -123456))
    assert np.allclose(w, 1.0 / 7.0) and abs(w.sum() - 1.0) < 1e-15 and abs(ess - 7.0) < 1e-12
    w, ess = gridmatch.pose_weights([-100000, -500000, -520000, -2 ** 31])                        # (exp(-390) about the maximum: no underflow to 0 / 0)
    assert abs(w.sum() - 1.0) < 1e-15 and w[0] > 1.0 - 1e-12 and abs(ess - 1.0) < 1e-12
    s = np.array([-1024.0, -2048.0, 0.0])
    w, ess = gridmatch.pose_weights(s)
    e = np.exp([-1.0, -2.0, 0.0])
    assert np.allclose(w, e / e.sum(), rtol=1e-15) and np.isclose(ess, 1.0 / np.sum((e / e.sum()) ** 2))
    assert np.allclose(gridmatch.pose_weights(s, temperature=4.0)[0], np.exp(np.array([-0.25, -0.5, 0.0])) / np.exp(np.array([-0.25, -0.5, 0.0])).sum())
    assert np.allclose(gridmatch.pose_weights(s * 2, scale=2048)[0], w)
    # statuses: a pose that is not OK has weight 0, whatever its score
    w, ess = gridmatch.pose_weights([0, -1024, 0, -1024], status=[ref.ST_EMPTY, ref.ST_OK, ref.ST_CAPACITY, ref.ST_OK])
    assert w.tolist() == [0.0, 0.5, 0.0, 0.5] and ess == 2.0
    w, ess = gridmatch.pose_weights([0, 0], status=[ref.ST_EMPTY, ref.ST_EMPTY])
    assert w.tolist() == [0.0, 0.0] and ess == 0.0
    with pytest.raises(ValueError):
        gridmatch.pose_weights([0, 0], status=[0])
    with pytest.raises(ValueError):
        gridmatch.pose_weights([0, 0], temperature=0.0)


def sums_agree(rec, hist, table):
    clipped = np.clip(np.asarray(table, dtype=np.int64), -ref.TABLE_CLIP, ref.TABLE_CLIP)
    return int(rec[ref.SCORE]) == int(hist.astype(np.int64) @ clipped) and hist.sum() == rec[ref.ROWS] and \
        rec[ref.EXPECTED] + rec[ref.NOVEL] + rec[ref.UNEXPLORED] == rec[ref.ROWS] and hist[-2] == rec[ref.NOVEL] and hist[-1] == rec[ref.UNEXPLORED]


def test_hand_made_rows_have_their_literal_records():
    field, cases = ref.hand_made()
    assert field.shape == (1, 200)
    for case in cases:
        pts, t, cs, table, H, beyond = ref.hand_made_pair(case)
        rec, hist, rows = ref.beam_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, table, H, beyond)
        assert rec.tolist() == case[5] and np.array_equal(hist, ref.hist_of(case)) and rows.tolist() == case[7], case
        assert sums_agree(rec, hist, table)
    # the matcher's rule for a device count: shortened, negative, over-long
    pts, t, cs, table, H, beyond = ref.hand_made_pair(cases[12])
    rec, hist, rows = ref.beam_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, table, H, beyond, cnt=3)
    assert rec.tolist() == [ref.ST_OK, 1, -3, 1, 0, 0, 0, 0] and len(rows) == 3 and hist.tolist() == [0, 0, 1, 0, 0, 0, 0]
    for cnt in (-1, 7):
        rec, hist, rows = ref.beam_pair(field, cref.THRESHOLD, 0.0, 0.0, 1.0, pts, t, cs, table, H, beyond, cnt=cnt)
        assert rec.tolist() == [ref.ST_CAPACITY, 0, 0, 0, 0, 0, 0, 0] and len(rows) == 0 and not hist.any()


def test_without_beyond_the_walks_are_the_checks():
    """beyond = 0: s = r / r = 1, the far end is the hit, the walk is the check's and k_z its K — for every row of the
    check's own clouds and poses, those on cell borders, off the grid and without cells included.  A row at the origin (r =
    0, s = 0 / 0) alone has cells there and none here; the clouds hold some."""
    field = cref.wall_field(*cref.SIZES[0], 0)
    ny, nx = field.shape
    clouds = kref.clouds(ny, nx, 0)
    pair, t, rot = kref.poses(ny, nx, 65, 0)
    rows = at_origin = 0
    for b in range(0, 65, 4):
        pts = clouds[pair[b]]
        zero = (pts == 0.0).all(axis=1)
        mine = ref.walk_rows(field, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, pts, t[b], rot[b], 0.0)
        theirs = kref.walk_rows(field, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, pts, t[b], rot[b])
        assert np.array_equal(mine[~zero], theirs[~zero]) and not mine[zero, 0].any(), b
        rows += int(mine[:, 0].sum())
        at_origin += int(theirs[zero, 0].sum())
    assert rows > 1000 and at_origin > 0


def test_sums_agree_in_every_shared_case():
    """score == hist . clip(table) and hist.sum() == rows, for every half width and beyond of the device suite, on a table
    with entries beyond the clip."""
    field = cref.wall_field(*cref.SIZES[1], 1)
    ny, nx = field.shape
    clouds = kref.clouds(ny, nx, 1)
    pair, t, rot = kref.poses(ny, nx, 3, 1)
    seen = set()
    for H in ref.HALF_WIDTHS:
        table = ref.table_of(H).astype(np.int64) * 2 + 20000                  # in [-40 000, 20 000]
        for beyond in ref.BEYONDS:
            for b in range(3):
                rec, hist, rows = ref.beam_pair(field, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, clouds[pair[b]], t[b], rot[b], table, H, beyond)
                assert sums_agree(rec, hist, table) and len(rows) == len(clouds[pair[b]])
                seen |= {name for name, some in (("behind", hist[:H].sum()), ("on", hist[H]), ("short", hist[H + 1:2 * H + 1].sum()), ("novel", hist[-2]),
                                                 ("unexplored", hist[-1]), ("no cells", (rows[:, 0] == ref.NO_CELLS).sum())) if some}
    assert seen == {"behind", "on", "short", "novel", "unexplored", "no cells"}                  # (a condition on the inputs)


def test_the_score_separates_true_from_displaced_poses_in_the_room_map():
    """The room map of tests/test_grid_cast_cpu.py::room_field, scans synth.scan(SCENE_POSES[n], 50 + n)[::4] for n = 0, 5,
    11, threshold rint(0.5 * 2^12), H = 8, sigma = 0.1 m, beyond = 1.5 m, the default table.  Each of the five displacements
    of test_grid_check_cpu.DISPLACEMENTS scores at most 3 x the true pose's (negative) score — 3.67 x was the least ratio
    seen —, a displacement of one cell and one of 2 degrees, which the check cannot see, score strictly below the true
    pose, and at the true poses at least 85 % of the rows fall on d = -1 or d = 0 (91 % was the least seen)."""
    from icpmi import gridmatch, synth
    from test_grid_cast_cpu import room_field
    from test_grid_check_cpu import DISPLACEMENTS
    q, g = room_field()
    threshold = int(np.rint(0.5 * 2.0 ** 12))
    H, beyond = 8, 1.5
    table = gridmatch.beam_table(0.1, 0.1, H)
    assert table.tolist() == TABLE_0P1_0P1_8

    def scored(pts, pose):
        return ref.score(ref.walk_rows(q, threshold, g["min_x"], g["min_y"], 0.1, pts, pose[:2], (np.cos(pose[2]), np.sin(pose[2])), beyond), table, H)

    for n in (0, 5, 11):
        pose = gref.SCENE_POSES[n]
        pts = synth.scan(pose, 50 + n)[::4]
        assert len(pts) == 512
        rec, hist, _ = scored(pts, pose)
        true, near = int(rec[ref.SCORE]), int(hist[H - 1] + hist[H])
        print(f"pose {n}: {rec.tolist()}, rows on d = -1 or 0: {near}, histogram {hist.tolist()}")
        assert rec[ref.ROWS] == 512 and true < 0 and near >= 0.85 * 512
        for d in DISPLACEMENTS:
            moved = int(scored(pts, (pose[0] + d[0], pose[1] + d[1], pose[2] + d[2]))[0][ref.SCORE])
            print(f"pose {n} + {d}: {moved} = {moved / true:.2f} x")
            assert moved <= 3 * true
        for d in ((0.1, 0.0, 0.0), (0.0, 0.0, np.deg2rad(2.0))):
            moved = int(scored(pts, (pose[0] + d[0], pose[1] + d[1], pose[2] + d[2]))[0][ref.SCORE])
            print(f"pose {n} + {d}: {moved} = {moved / true:.2f} x")
            assert moved < true
