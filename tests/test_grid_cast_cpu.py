"""Host side of the cast (include/icpmi.h: icpmi_grid_occupancy_planes, icpmi_grid_cast_segments, icpmi_grid_cast_rays): the C
ABI as the header declares it, the size of the planes against literal values, every refusal the entries decide on the host —
before any launch, so no GPU is touched (the device pointers are fakes that are never dereferenced) — and the NumPy
restatement the device test compares against (tests/gridcast_ref.py): its steps against the 1 209 segments walked by the
reference (tests/golden/bresenham.npz), its hand-made records, and the scans it predicts in the room map against the scans
that built the map."""
import ctypes
import os
import re

import numpy as np

import gridcast_ref as ref
import gridmatch_ref as gref
from conftest import REPO, load_golden

NEW_SYMBOLS = ("icpmi_grid_occupancy_planes_bytes", "icpmi_grid_occupancy_planes", "icpmi_grid_cast_segments", "icpmi_grid_cast_rays")
FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


def test_entries_and_record_slots_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\(", hdr), name
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GC_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"GC_INTS": 4, "GC_K_HIT": 0, "GC_X_HIT": 1, "GC_Y_HIT": 2, "GC_K_UNKNOWN": 3, "GC_NONE": -1, "GC_NO_CELLS": -2,
                       "GC_THREADS": 256}
    assert defines == {k: getattr(_lib, k) for k in defines}
    assert (ref.K_HIT, ref.X_HIT, ref.Y_HIT, ref.K_UNKNOWN, ref.NONE, ref.NO_CELLS) == (0, 1, 2, 3, -1, -2)
    assert lib.icpmi_grid_occupancy_planes_bytes.restype is ctypes.c_size_t
    assert len(lib.icpmi_grid_cast_segments.argtypes) == 11 and len(lib.icpmi_grid_cast_rays.argtypes) == 18


def test_planes_bytes_against_literal_values():
    """csrc/gridcast.hip, GcPlanes: two planes of ny rows of ceil(nx / 32) uint32, each rounded up to 256 bytes."""
    import icpmi
    q = icpmi.lib().icpmi_grid_occupancy_planes_bytes
    assert q(1, 1) == 512 and q(1, 32) == 512 and q(64, 32) == 512 and q(65, 32) == 1024        # 4, 4, 256, 260 bytes a plane
    assert q(70, 100) == 2 * 1280                                                              # 70 x 4 words = 1120 -> 1280
    assert q(2242, 2402) == 2 * 681728                                                         # 2242 x 76 words = 681 568 -> 681 728
    assert q(0, 10) == 0 and q(10, 0) == 0
    assert q(-1, 10) == 0 and q(1 << 16, 1 << 15) == 0 and q((1 << 29) + 1, 1) == 0


def test_entries_refuse_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    need = L.icpmi_grid_occupancy_planes_bytes(400, 560)

    def planes(field=FAKE, ny=400, nx=560, thr=2048, out=FAKE, nbytes=need):
        return L.icpmi_grid_occupancy_planes(field, ny, nx, thr, out, nbytes, None)

    def segments(field=FAKE, kept=None, ny=400, nx=560, segs=FAKE, n=100, out=FAKE, ws=FAKE, ws_bytes=need):
        return L.icpmi_grid_cast_segments(field, kept, ny, nx, 2048, segs, n, out, ws, ws_bytes, None)

    def rays(field=FAKE, kept=None, ny=400, nx=560, res=0.1, poses=FAKE, pose_cs=FAKE, n_poses=3, beam_cs=FAKE, n_beams=360, reach=30.0,
             out=FAKE, ws=FAKE, ws_bytes=need):
        return L.icpmi_grid_cast_rays(field, kept, ny, nx, 2048, -14.0, -10.0, res, poses, pose_cs, n_poses, beam_cs, n_beams, reach, out, ws,
                                      ws_bytes, None)

    assert planes(field=None) == ERR_ARG and planes(out=None) == ERR_ARG and planes(field=FAKE + 2) == ERR_ARG and planes(out=FAKE + 4) == ERR_ARG
    assert planes(ny=-1) == ERR_ARG and planes(ny=1 << 16, nx=1 << 15) == ERR_ARG and planes(nbytes=need - 1) == ERR_WORKSPACE
    assert planes(ny=0) == 0 and planes(nx=0, field=None, out=None, nbytes=0) == 0                 # an empty grid: nothing to pack
    for call in (segments, rays):
        assert call(ny=-1) == ERR_ARG and call(nx=(1 << 29) + 1, ny=1) == ERR_ARG and call(ny=1 << 16, nx=1 << 15) == ERR_ARG
        assert call(out=None) == ERR_ARG and call(out=FAKE + 8) == ERR_ARG
        assert call(field=None) == ERR_ARG and call(field=FAKE + 2) == ERR_ARG                     # no planes: the field is needed
        assert call(ws=None) == ERR_WORKSPACE and call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws=FAKE + 4) == ERR_WORKSPACE
        assert call(kept=FAKE + 4) == ERR_ARG
    assert segments(segs=None) == ERR_ARG and segments(segs=FAKE + 4) == ERR_ARG and segments(n=-1) == ERR_ARG
    assert segments(n=1 << 29) == ERR_UNSUPPORTED and segments(n=0, segs=None, out=None, field=None, ws=None) == 0
    assert rays(n_poses=-1) == ERR_ARG and rays(n_beams=-1) == ERR_ARG
    assert rays(poses=None) == ERR_ARG and rays(pose_cs=None) == ERR_ARG and rays(beam_cs=None) == ERR_ARG
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        assert rays(res=bad) == ERR_ARG and rays(reach=bad) == ERR_ARG
    assert rays(n_poses=1 << 15, n_beams=1 << 14) == ERR_UNSUPPORTED and rays(n_poses=1 << 28, n_beams=2) == ERR_UNSUPPORTED
    assert rays(n_poses=0, poses=None, pose_cs=None, out=None) == 0 and rays(n_beams=0, beam_cs=None, out=None) == 0


def test_python_layer_restates_the_cells_of_a_ray():
    """icpmi.gridmatch.ray_end_cells and step_cells — what cast_scans forms ``unknown_range`` with on the host — against the
    restatement's scalar loops, NaN, infinite and far poses among them."""
    from icpmi import gridmatch
    rng = np.random.default_rng(3)
    xy = rng.uniform(-20, 20, size=(7, 2))
    xy[2, 0], xy[3, 1], xy[4, 0], xy[5, 1] = np.nan, np.inf, 1e305, -3e8
    th, ang = rng.uniform(-4, 4, size=7), rng.uniform(-4, 4, size=33)
    pcs, bcs = gref.cos_sin_of(th), gref.cos_sin_of(ang)
    for reach in (30.0, 1e9, 1e308):
        segs, ok = gridmatch.ray_end_cells(-14.0, -10.0, 0.1, xy, pcs, bcs, reach)
        want, want_ok = ref.ray_segments(-14.0, -10.0, 0.1, xy, pcs, bcs, reach)
        assert np.array_equal(ok, want_ok) and np.array_equal(segs[ok], want[ok]) and not ok[2].any() and ok[0].all() == (reach < 1e300)
    z = load_golden("bresenham")
    segs = z["segs"][::7]
    for k in (0, 1, 2, 5, 16, 700):
        x, y = gridmatch.step_cells(segs, np.full(len(segs), k))
        assert [(int(a), int(b)) for a, b in zip(x, y)] == [ref.step_cell(s, k) for s in segs]


def test_steps_are_the_reference_walk_and_the_end_cell():
    """Every golden segment against a field in which only its end cell is occupied (another non-zero value elsewhere): the hit
    is at step K = len(golden cells) and nothing is unknown.  With golden cell j occupied as well the hit is at j, for three j
    per segment: step j of the restatement is the reference's j-th cell, for every j that is tried — and step_cell gives it."""
    z = load_golden("bresenham")
    segs, cells, off = z["segs"], z["cells"], z["off"]
    assert len(segs) == 1209 and int(np.diff(off).max()) == 5707
    field = np.full((6016, 6016), 3, dtype=np.int16)               # every segment shifted by 3008 fits
    shift = 3008
    tried = 0
    for s, a, b in zip(segs, off[:-1], off[1:]):
        walk = cells[a:b].astype(np.int64) + shift
        seg = s + shift
        K = len(walk)
        assert K == max(abs(s[2] - s[0]), abs(s[3] - s[1]))
        field[seg[3], seg[2]] = ref.THRESHOLD
        assert ref.cast_segment(field, ref.THRESHOLD, seg) == [K, seg[2], seg[3], ref.NONE], s
        assert ref.step_cell(seg, K) == (seg[2], seg[3])
        for j in sorted({0, K // 2, K - 1} if K else ()):
            x, y = (int(v) for v in walk[j])
            field[y, x] = 32767
            assert ref.cast_segment(field, ref.THRESHOLD, seg) == [j, x, y, ref.NONE] and ref.step_cell(seg, j) == (x, y), (s, j)
            field[y, x] = 3
            tried += 1
        field[seg[3], seg[2]] = 3
    assert tried >= 3 * 1200 - 100 and (field == 3).all()


def test_hand_made_records():
    field, segs, records = ref.unknown_row()
    assert np.array_equal(ref.cast_segments(field, ref.THRESHOLD, segs), records)
    # a threshold at or below 0 makes an unknown cell occupied as well: it is the hit, not an unknown cell before it
    assert ref.cast_segment(field, 0, (51, 0, 90, 0)) == [0, 51, 0, ref.NONE]
    assert ref.cast_segment(field, -40000, (-5, 0, 9, 0)) == [5, 0, 0, ref.NONE]
    empty = np.zeros((0, 7), dtype=np.int16)
    assert ref.cast_segment(empty, 1, (1, 2, 3, 4)) == [ref.NONE, 3, 4, ref.NONE]
    far = ref.cast_segment(field, ref.THRESHOLD, (-2 ** 30, 0, 2 ** 30, 0))                        # clamped to +-2^29
    assert far == [2 ** 29 + 50, 50, 0, 2 ** 29 + 49]


def test_shared_cases_exercise_what_they_are_for():
    """Conditions on the inputs of the device test, decided by the restatement: each family meets the situation it is there
    for, so a generator that falls short fails here."""
    for (ny, nx), seed in zip(ref.SIZES, range(len(ref.SIZES))):
        f, segs = ref.wall_field(ny, nx, seed), ref.star_segments(ny, nx, seed)
        assert len(segs) == 257 == max(ref.BATCHES)
        rec = ref.cast_segments(f, ref.THRESHOLD, segs)
        hit = rec[:, 0] >= 0
        if ny * nx > 1:
            assert hit.any() and (~hit).any() and ((rec[:, 3] >= 0).any() or nx == 1)             # (nx = 1: the one column is a wall)
        if (ny, nx) == (70, 100):
            assert {31, 32, 63, 64, 99} <= set(rec[hit, 1].tolist())                              # every wall stops some ray
            assert ((rec[:, 0] > 0) & ((segs[:, 0] < 0) | (segs[:, 0] >= nx))).any()              # a ray from outside that hits inside
            dx, dy = np.abs(segs[:, 2] - segs[:, 0]), np.abs(segs[:, 3] - segs[:, 1])
            assert (hit & (dx > dy)).any() and (hit & (dy > dx)).any() and (hit & (dx == dy) & (dx > 0)).any()
    f, segs = ref.between_field_and_segments()
    rec = ref.cast_segments(f, ref.THRESHOLD, segs)
    passed = 0
    for s, r in zip(segs, rec):                                    # a diagonal move with both side cells occupied, before any hit
        last = r[0] if r[0] >= 0 else max(abs(s[2] - s[0]), abs(s[3] - s[1]))
        walk = [ref.step_cell(s, k) for k in range(last + 1)]
        passed += any(a[0] != b[0] and a[1] != b[1] and f[a[1], b[0]] >= ref.THRESHOLD and f[b[1], a[0]] >= ref.THRESHOLD
                      for a, b in zip(walk[:-1], walk[1:]))
    assert passed >= 16, passed
    f, segs = ref.fuzz()
    assert abs((f >= ref.THRESHOLD).mean() - 0.03) < 0.01 and abs((f == 0).mean() - 0.30) < 0.02 and len(segs) == 4000


def room_field():
    """The room of tests/gridmatch_ref.py at 0.1 m: 12 scans mapped by the oracle, the field at k = 12."""
    import oracle
    g = gref.SCENE
    lo = np.zeros((200, 280), dtype=np.float32)
    l_hit, l_miss = float(np.log(0.7 / 0.3)), float(np.log(0.4 / 0.6))
    for o, h in zip(*gref.scene_scans()):
        oracle.grid_update_scan(lo, g["min_x"], g["min_y"], 0.1, o, h, l_hit, l_miss, -5.0, 5.0)
    k = gref.shift_bits(-5.0, 5.0)
    assert k == 12
    return gref.quantise(lo, k), g


def test_predicted_scans_of_the_room_are_the_scans_that_built_it():
    """From the scan poses 0, 5 and 11 along each scan's own 2 048 bearings, reach 30 m, threshold rint(0.5 * 2^12): the
    median |range - the scan's range| is below one cell (0.1 m), at least 0.9 of the beams are within two cells and at most
    1 % hit nothing.  Measured when this was written: medians 0.056, 0.053, 0.056 m; shares 0.952, 0.990, 0.985; 2, 0 and 0
    beams without a hit."""
    from icpmi import synth
    q, g = room_field()
    threshold = int(np.rint(0.5 * 2.0 ** 12))
    for n in (0, 5, 11):
        pose = gref.SCENE_POSES[n]
        pts = synth.scan(pose, 50 + n)
        assert len(pts) == 2048
        bearings, measured = np.arctan2(pts[:, 1], pts[:, 0]), np.hypot(pts[:, 0], pts[:, 1])
        xy, pcs = [pose[:2]], gref.cos_sin_of(np.array([pose[2]]))
        rec, segs, ok = ref.cast_rays(q, threshold, g["min_x"], g["min_y"], 0.1, xy, pcs, gref.cos_sin_of(bearings), 30.0)
        ranges, _ = ref.ranges_of(rec, segs, xy, g["min_x"], g["min_y"], 0.1)
        assert ok.all()
        none = int(np.isinf(ranges).sum())
        err = np.abs(ranges[0] - measured)
        median, share = float(np.median(err[np.isfinite(err)])), float((err <= 0.2).mean())
        print(f"pose {n}: median |dr| {median:.3f} m, within two cells {share:.3f}, no hit {none}")
        assert median < 0.1 and share >= 0.9 and none <= 0.01 * 2048
