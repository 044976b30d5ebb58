"""The check on the device (csrc/gridcheck.hip; icpmi.gridmatch.check_pairs; check_scans, check_scan, check_poses and
check_history of utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract (tests/gridcheck_ref.py,
itself held to literal records by tests/test_grid_check_cpu.py).  Records and rows are integers, so every comparison is
array_equal: on small grids with walls on both sides of a word of the planes, with clouds around a wave and around a chunk
of rows, poses inside, on the border of, outside and without a cell of the grid, rows on cell borders and rows that are not
finite, every rule for a device count, field against kept planes, the rows against the cast of the same segments, a second
run into the same buffers, and through the Python layers on a small map."""
import numpy as np
import pytest

import gridcast_ref as cref
import gridcheck_ref as ref
import gridmatch_ref as gref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
FIELDS = [f"{ny}x{nx}" for ny, nx in cref.SIZES] + ["fuzz"]
PAIRS = {0: (1, 3, 65)}                                        # 65 pairs on the first field only; 1 and 3 everywhere


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def field_of(n):
    return cref.wall_field(*cref.SIZES[n], n) if n < len(cref.SIZES) else cref.fuzz()[0]


def device_check(src, cs, pair, t, rot, tolerance, out=None, threshold=cref.THRESHOLD):
    """check_pairs with the rows' records, into buffers full of a sentinel (or the caller's) -> (records, rows, the buffers)"""
    import torch
    from icpmi import gridmatch
    stride = int(np.diff(cs.off_host)[pair].max()) if len(pair) else 0
    if out is None:
        out = (torch.full((len(pair), ref.INTS), SENTINEL, dtype=torch.int32, device="cuda"),
               torch.full((len(pair), stride, ref.ROW_INTS), SENTINEL, dtype=torch.int32, device="cuda"))
    got = gridmatch.check_pairs(src, threshold, ref.MIN_X, ref.MIN_Y, ref.RES, cs, pair, t, rot, tolerance, want_rows=True, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out


def expected(walks, counts, stride, tolerance):
    """The restated (records (B, 8), rows (B, stride, 4)) of pairs whose walks are given: what lies at or behind a pair's count
    keeps the sentinel, a pair with a refused count (-1) reads nothing."""
    B = len(walks)
    recs = np.zeros((B, ref.INTS), dtype=np.int32)
    rows = np.full((B, stride, ref.ROW_INTS), SENTINEL, dtype=np.int32)
    for b, (w, n) in enumerate(zip(walks, counts)):
        if n < 0:
            recs[b, ref.STATUS] = ref.ST_CAPACITY
            continue
        recs[b], rows[b, :n] = ref.classify(w[:n], tolerance)
    return recs, rows


def same(got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        print(what, "differs at", bad[:5].tolist(), "got", [int(got[tuple(i)]) for i in bad[:5]], "want", [int(want[tuple(i)]) for i in bad[:5]])
    return len(bad) == 0


@pytest.mark.parametrize("n", range(len(FIELDS)), ids=FIELDS)
def test_records_and_rows_equal_the_restatement(gpu, n):
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field = field_of(n)
    ny, nx = field.shape
    clouds = ref.clouds(ny, nx, n)
    cs = CloudSet.from_numpy(clouds)
    fd = on_device(field)
    planes = gridmatch.occupancy_planes(fd, cref.THRESHOLD)
    for B in PAIRS.get(n, (1, 3)):
        pair, t, rot = ref.poses(ny, nx, B, n)
        walks = [ref.walk_rows(field, cref.THRESHOLD, ref.MIN_X, ref.MIN_Y, ref.RES, clouds[c], t[b], rot[b]) for b, c in enumerate(pair)]
        counts = [len(clouds[c]) for c in pair]
        stride = max(counts)
        for tolerance in ref.TOLERANCES:
            want_rec, want_rows = expected(walks, counts, stride, tolerance)
            rec, rows, out = device_check(fd, cs, pair, t, rot, tolerance)
            assert same(rec, want_rec, "records") and same(rows, want_rows, "rows"), (B, tolerance)
            assert (rec[:, ref.CONFIRMED:ref.UNEXPLORED + 1].sum(axis=1) == rec[:, ref.ROWS]).all() and not rec[:, 7].any()
        # kept planes give the bytes the field gave, and a second call into the same buffers changes nothing
        kept_rec, kept_rows, _ = device_check(planes, cs, pair, t, rot, ref.TOLERANCES[-1])
        assert kept_rec.tobytes() == rec.tobytes() and kept_rows.tobytes() == rows.tobytes()
        again_rec, again_rows, _ = device_check(fd, cs, pair, t, rot, ref.TOLERANCES[-1], out=out)
        assert again_rec.tobytes() == rec.tobytes() and again_rows.tobytes() == rows.tobytes()
        if B >= 3:                                                 # (conditions on the inputs: every class is met, and rows without cells)
            tol1 = expected(walks, counts, stride, 1)[0]
            print(FIELDS[n], B, "tolerance 1:", tol1[:, 1:7].sum(axis=0).tolist())
            assert min(ny, nx) == 1 or (tol1[:, ref.CONFIRMED:ref.THROUGH_UNKNOWN + 1].sum(axis=0) > 0).all()
        if B == 65:
            assert (want_rec[:, ref.STATUS] == ref.ST_EMPTY).sum() >= 3 and (want_rows[..., 0] == ref.NO_CELLS).any()
        # the records alone, without the rows' buffer
        only, none = gridmatch.check_pairs(fd, cref.THRESHOLD, ref.MIN_X, ref.MIN_Y, ref.RES, cs, pair, t, rot, ref.TOLERANCES[-1])
        assert none is None and only.cpu().numpy().tobytes() == rec.tobytes()


def test_the_rows_agree_with_the_cast_of_the_same_segments(gpu):
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field = field_of(0)
    ny, nx = field.shape
    clouds = ref.clouds(ny, nx, 0)
    pair, t, rot = ref.poses(ny, nx, 3, 0)
    planes = gridmatch.occupancy_planes(on_device(field), cref.THRESHOLD)
    _, rows, _ = device_check(planes, CloudSet.from_numpy(clouds), pair, t, rot, 1)
    segs, at = [], []
    for b, c in enumerate(pair):
        origin = ref.cell_of(0.0, 0.0, 1.0, 0.0, t[b, 0], t[b, 1], ref.MIN_X, ref.MIN_Y, ref.RES)
        for i, (x, y) in enumerate(clouds[c]):
            end = ref.cell_of(x, y, rot[b, 0], rot[b, 1], t[b, 0], t[b, 1], ref.MIN_X, ref.MIN_Y, ref.RES)
            if origin is not None and end is not None:
                segs.append(origin + end)
                at.append((b, i))
    assert len(segs) > 500
    cast = gridmatch.cast_segments(planes, cref.THRESHOLD, np.array(segs, dtype=np.int32)).cpu().numpy()
    mine = np.array([rows[b, i] for b, i in at])
    assert np.array_equal(mine[:, 1], cast[:, cref.K_HIT]) and np.array_equal(mine[:, 3], cast[:, cref.K_UNKNOWN])
    assert np.array_equal(mine[:, 2], np.abs(np.array(segs)[:, 2:] - np.array(segs)[:, :2]).max(axis=1))


def test_every_rule_for_a_device_count(gpu):
    """cnt_dev: a full count, shortened ones (to 0, into a wave, onto a chunk boundary), a negative one and an over-long one
    (both CAPACITY: nothing is read, nothing is written); NULL is every other test."""
    import torch
    from icpmi.batch import CloudSet
    field = field_of(0)
    ny, nx = field.shape
    clouds = ref.clouds(ny, nx, 0)
    full = CloudSet.from_numpy(clouds)
    cnt = np.array([0, 1, 10, -1, 66, 0, 200, 256, 514], dtype=np.int32)
    cs = CloudSet(full.pts, full.off_host, cnt=on_device(cnt))
    pair = np.arange(9, dtype=np.int32)
    _, t, rot = ref.poses(ny, nx, 9, 5)
    t[5:8] = t[0] + 0.1                                            # (poses with cells, so that the counts decide)
    counts = [ref.rows_of(len(clouds[c]), cnt[c]) for c in pair]
    assert counts == [0, 1, 10, -1, -1, 0, 200, 256, -1]
    walks = [ref.walk_rows(field, cref.THRESHOLD, ref.MIN_X, ref.MIN_Y, ref.RES, clouds[c][:max(counts[c], 0)], t[b], rot[b]) for b, c in enumerate(pair)]
    want_rec, want_rows = expected(walks, counts, 513, 1)
    rec, rows, out = device_check(on_device(field), cs, pair, t, rot, 1)
    assert same(rec, want_rec, "records") and same(rows, want_rows, "rows")
    assert rec[:, ref.STATUS].tolist() == [ref.ST_EMPTY, ref.ST_OK, ref.ST_OK, ref.ST_CAPACITY, ref.ST_CAPACITY, ref.ST_EMPTY, ref.ST_OK, ref.ST_OK,
                                           ref.ST_CAPACITY]
    assert torch.equal(cs.cnt.cpu(), torch.from_numpy(cnt))


def test_hand_made_rows_on_the_device(gpu):
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field, cases = ref.hand_made()
    fd = on_device(field)
    for case in cases:
        pts, t, rot = ref.hand_made_pair(case)
        cs = CloudSet.from_numpy([pts])
        rec, rows = gridmatch.check_pairs(fd, cref.THRESHOLD, 0.0, 0.0, 1.0, cs, [0], [t], [rot], case[2], want_rows=True)
        assert rec.cpu().numpy().tolist() == [case[3]] and rows.cpu().numpy().tolist() == [case[4]], case
    # an empty grid: nothing is packed, every row with cells ends in unexplored space
    pts, t, rot = ref.hand_made_pair(cases[11])
    empty = np.zeros((0, 9), dtype=np.int16)
    rec, rows = gridmatch.check_pairs(on_device(empty), 1, 0.0, 0.0, 1.0, CloudSet.from_numpy([pts]), [0], [t], [rot], 0, want_rows=True)
    want = ref.check_pair(empty, 1, 0.0, 0.0, 1.0, pts, t, rot, 0)
    assert np.array_equal(rec.cpu().numpy()[0], want[0]) and np.array_equal(rows.cpu().numpy()[0], want[1]) and want[0][ref.UNEXPLORED] == 3
    # no pair: nothing to do is no refusal
    rec, rows = gridmatch.check_pairs(fd, cref.THRESHOLD, 0.0, 0.0, 1.0, CloudSet.from_numpy([pts]), [], np.zeros((0, 2)), np.zeros((0, 2)), 0, want_rows=True)
    assert rec.shape == (0, ref.INTS) and rows.shape == (0, 0, ref.ROW_INTS)


# ── through the Python layers ────────────────────────────────────────────────
@pytest.fixture(scope="module")
def small_map(gpu):
    """(the scene's grid at 0.1 m built by update_scan from three thinned scans of the synthetic room, the scans, their poses)"""
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    poses = [gref.SCENE_POSES[k] for k in (0, 3, 6)]
    scans = [synth.scan(p, 50 + k)[::8] for k, p in zip((0, 3, 6), poses)]
    for p, s in zip(poses, scans):
        grid.update_scan(np.array(p[:2]), synth.to_world(s, p))
    return grid, scans, np.array(poses)


def restated_info(grid, scans, poses, tolerance, occupied=0.5):
    k = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    q = gref.quantise(grid.log_odds, k)
    out = [ref.check_pair(q, int(np.rint(occupied * 2.0 ** k)), grid.min_x, grid.min_y, grid.resolution, s, p[:2], (np.cos(p[2]), np.sin(p[2])), tolerance)
           for s, p in zip(scans, poses)]
    return np.array([r for r, _ in out]).astype(np.int64), [rows for _, rows in out]


KEYS = (("status", ref.STATUS), ("rows", ref.ROWS), ("confirmed", ref.CONFIRMED), ("violated", ref.VIOLATED), ("in_free", ref.IN_FREE),
        ("unexplored", ref.UNEXPLORED), ("through_unknown", ref.THROUGH_UNKNOWN))


def info_equals(info, rec, classes=None):
    ok = all(info[key].dtype == np.int64 and np.array_equal(info[key], rec[:, slot]) for key, slot in KEYS)
    some = np.maximum(rec[:, ref.ROWS], 1)
    ok = ok and np.array_equal(info["violated_share"], np.where(rec[:, ref.ROWS] > 0, rec[:, ref.VIOLATED] / some, 0.0))
    ok = ok and np.array_equal(info["in_free_share"], np.where(rec[:, ref.ROWS] > 0, rec[:, ref.IN_FREE] / some, 0.0))
    if classes is not None:
        ok = ok and len(info["classes"]) == len(classes) and all(np.array_equal(a, b) for a, b in zip(info["classes"], classes))
    return ok


def test_check_methods_of_the_grid_agree_with_check_pairs_and_the_restatement(small_map):
    from icpmi import gridmatch
    grid, scans, poses = small_map
    rec, classes = restated_info(grid, scans, poses, 2)
    info = grid.check_scans(scans, poses, want_rows=True)
    print("true poses:", rec[:, 1:7].tolist())
    assert info["shift_bits"] == 12 and info_equals(info, rec, classes) and "classes" not in grid.check_scans(scans, poses)
    assert (rec[:, ref.VIOLATED] < rec[:, ref.CONFIRMED]).all()
    # ... and with the layer below on the same field
    field, k = grid.score_field()
    cos_sin = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
    below, _ = gridmatch.check_pairs(field, int(np.rint(0.5 * 2.0 ** k)), grid.min_x, grid.min_y, grid.resolution, gridmatch.cloud_set_of(scans),
                                     np.arange(3), poses[:, :2], cos_sin, 2)
    assert np.array_equal(below.cpu().numpy(), rec)
    # one scan; one scan at many poses (a matrix among the ways to give one); another tolerance and threshold
    one = grid.check_scan(scans[1], poses[1], want_rows=True)
    assert all(int(one[key]) == rec[1, slot] for key, slot in KEYS) and np.array_equal(one["classes"], classes[1])
    th = poses[1, 2]
    matrix = np.array([[np.cos(th), -np.sin(th), poses[1, 0]], [np.sin(th), np.cos(th), poses[1, 1]], [0, 0, 1.0]])
    assert grid.check_scan(scans[1], matrix)["rows"] == rec[1, ref.ROWS]
    hyp = np.concatenate([poses, poses + [0.7, -0.4, 0.2], [[np.nan, 0.0, 0.0]]])
    want, want_classes = restated_info(grid, [scans[0]] * len(hyp), hyp, 0, occupied=1.0)
    got = grid.check_poses(scans[0], hyp, tolerance=0, occupied_log_odds=1.0, want_rows=True)
    assert info_equals(got, want, want_classes) and got["status"][-1] == ref.ST_EMPTY and got["violated_share"][-1] == 0.0
    assert want[3, ref.VIOLATED] > want[0, ref.VIOLATED]
    # field= and planes= as in cast_scans: the same bytes, and both together or planes of another grid are refused
    for kw in (dict(field=(field, k)), dict(planes=grid.occupancy_planes()), dict(planes=grid.occupancy_planes(field=(field, k)))):
        assert info_equals(grid.check_scans(scans, poses, **kw), rec)
    from utilities.mapping import OccupancyGrid2D
    other = OccupancyGrid2D(-1.0, 1.0, -1.0, 1.0)
    with pytest.raises(ValueError):
        grid.check_scans(scans, poses, field=(field, k), planes=grid.occupancy_planes())
    with pytest.raises(ValueError):
        other.check_scans(scans, poses, planes=grid.occupancy_planes())
    with pytest.raises(ValueError):
        other.check_poses(scans[0], poses, field=(field, k))
    with pytest.raises(ValueError):
        grid.check_scans(scans, poses, tolerance=-1)
    with pytest.raises(ValueError):
        grid.check_scans(scans, poses[:2])


def test_check_history_equals_check_scans(small_map):
    from icpmi import ScanHistory
    grid, scans, poses = small_map
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=4, row_capacity=1024)
    hist.add_many(scans)
    ids = [2, 0, 2, 1]
    p4 = poses[[2, 0, 1, 1]]
    got = grid.check_history(hist, ids, p4, want_rows=True)
    want = grid.check_scans([scans[i] for i in ids], p4, want_rows=True)
    assert all(np.array_equal(got[key], want[key]) for key, _ in KEYS) and all(np.array_equal(a, b) for a, b in zip(got["classes"], want["classes"]))
    rec, classes = restated_info(grid, [scans[i] for i in ids], p4, 2)
    assert info_equals(got, rec, classes)
    for voxel in (0.05, 0.3, 0.17):                                # the history's own filtered copies (device counts), or a fresh filter
        got = grid.check_history(hist, ids, p4, voxel_size=voxel, want_rows=True)
        want = grid.check_scans([scans[i] for i in ids], p4, voxel_size=voxel, want_rows=True)
        assert all(np.array_equal(got[key], want[key]) for key, _ in KEYS), voxel
        assert [len(c) for c in got["classes"]] == [len(c) for c in want["classes"]] and (got["rows"] == [len(c) for c in got["classes"]]).all()
        assert (got["rows"] <= 256).all() and (got["rows"] > 0).all()
    with pytest.raises(ValueError, match="scan ids must lie in"):
        grid.check_history(hist, [7], [poses[0]])
