"""The beam model on the device (csrc/gridbeam.hip; icpmi.gridmatch.beam_pairs; beam_scans, beam_scan, beam_poses and
beam_history of utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract (tests/gridbeam_ref.py,
itself held to literal records by tests/test_grid_beam_cpu.py).  Records, histograms and rows are integers, so every
comparison is array_equal: on the check's small grids with walls on both sides of a word of the planes, with its clouds
around a wave and around a chunk of rows and its poses inside, on the border of, outside and without a cell of the grid,
for half widths from 0 to the widest table and far ends from the hit itself to 10 km behind it, every rule for a device
count, field against kept planes, a second run into the same buffers, the rows against the check's at beyond = 0, and
through the Python layers on a small map."""
import numpy as np
import pytest

import gridbeam_ref as ref
import gridcast_ref as cref
import gridcheck_ref as kref
import gridmatch_ref as gref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
FIELDS = [f"{ny}x{nx}" for ny, nx in cref.SIZES] + ["fuzz"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def field_of(n):
    return cref.wall_field(*cref.SIZES[n], n) if n < len(cref.SIZES) else cref.fuzz()[0]


def device_beam(src, cs, pair, t, rot, table, H, beyond, out=None, threshold=cref.THRESHOLD):
    """beam_pairs with histograms and rows, into buffers full of a sentinel (or the caller's) -> (records, hist, rows, the buffers)"""
    import torch
    from icpmi import gridmatch
    stride = int(np.diff(cs.off_host)[pair].max()) if len(pair) else 0
    if out is None:
        out = tuple(torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
                    for shape in ((len(pair), ref.INTS), (len(pair), 2 * H + 3), (len(pair), stride, ref.ROW_INTS)))
    got = gridmatch.beam_pairs(src, threshold, kref.MIN_X, kref.MIN_Y, kref.RES, cs, pair, t, rot, table, H, beyond, want_hist=True, want_rows=True,
                               out=out)
    assert all(g is o for g, o in zip(got, out))
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), out


def expected(walks, counts, stride, table, H):
    """The restated (records (B, 8), hist (B, 2H + 3), rows (B, stride, 4)) of pairs whose walks are given: rows at or behind a
    pair's count keep the sentinel, a pair with a refused count (-1) reads nothing and its histogram is the memset's zeros."""
    B = len(walks)
    recs = np.zeros((B, ref.INTS), dtype=np.int32)
    hist = np.zeros((B, 2 * H + 3), dtype=np.int32)
    rows = np.full((B, stride, ref.ROW_INTS), SENTINEL, dtype=np.int32)
    for b, (w, n) in enumerate(zip(walks, counts)):
        if n < 0:
            recs[b, ref.STATUS] = ref.ST_CAPACITY
            continue
        recs[b], hist[b], rows[b, :n] = ref.score(w[:n], table, H)
    return recs, hist, rows


def same(got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        print(what, "differs at", bad[:5].tolist(), "got", [int(got[tuple(i)]) for i in bad[:5]], "want", [int(want[tuple(i)]) for i in bad[:5]])
    return len(bad) == 0


def all_walks(field, clouds, pair, t, rot, beyond):
    return [ref.walk_rows(field, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, clouds[c], t[b], rot[b], beyond) for b, c in enumerate(pair)]


def compare_everything(n, B):
    """Every half width and every beyond on field n with B pairs; kept planes, a second run and the records alone at the last.
    -> what occurred among the restated rows, for the conditions on the inputs."""
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field = field_of(n)
    ny, nx = field.shape
    clouds = kref.clouds(ny, nx, n)
    cs = CloudSet.from_numpy(clouds)
    fd = on_device(field)
    pair, t, rot = kref.poses(ny, nx, B, n)
    counts = [len(clouds[c]) for c in pair]
    stride = max(counts)
    seen = set()
    for beyond in ref.BEYONDS:
        walks = all_walks(field, clouds, pair, t, rot, beyond)
        for H in ref.HALF_WIDTHS:
            table = ref.table_of(H, n)
            want = expected(walks, counts, stride, table, H)
            rec, hist, rows, out = device_beam(fd, cs, pair, t, rot, table, H, beyond)
            assert same(rec, want[0], "records") and same(hist, want[1], "histograms") and same(rows, want[2], "rows"), (B, H, beyond)
            assert not rec[:, 6:].any() and (hist.sum(axis=1) == rec[:, ref.ROWS]).all()
            assert (hist.astype(np.int64) @ table.astype(np.int64) == rec[:, ref.SCORE]).all()
            tails = hist[:, 2 * H + 1:].sum(axis=0)
            seen |= {name for name, some in (("novel", tails[0]), ("unexplored", tails[1]), ("behind", hist[:, :H].sum()), ("short", hist[:, H + 1:2 * H + 1].sum()),
                                             ("on", hist[:, H].sum()), ("no cells", (want[2][..., 0] == ref.NO_CELLS).sum()),
                                             ("empty", (rec[:, ref.STATUS] == ref.ST_EMPTY).sum())) if some}
    # kept planes give the bytes the field gave, and a second call into the same buffers changes nothing
    planes = gridmatch.occupancy_planes(fd, cref.THRESHOLD)
    kept = device_beam(planes, cs, pair, t, rot, table, H, beyond)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kept[:3], (rec, hist, rows)))
    again = device_beam(fd, cs, pair, t, rot, table, H, beyond, out=out)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (rec, hist, rows)))
    # the records alone, and with one of the two other outputs
    only, no_hist, no_rows = gridmatch.beam_pairs(fd, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, cs, pair, t, rot, table, H, beyond)
    assert no_hist is None and no_rows is None and only.cpu().numpy().tobytes() == rec.tobytes()
    r2, h2, none = gridmatch.beam_pairs(planes, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, cs, pair, t, rot, table, H, beyond, want_hist=True)
    assert none is None and r2.cpu().numpy().tobytes() == rec.tobytes() and h2.cpu().numpy().tobytes() == hist.tobytes()
    return seen


@pytest.mark.parametrize("n", range(len(FIELDS)), ids=FIELDS)
def test_records_histograms_and_rows_equal_the_restatement(gpu, n):
    seen = compare_everything(n, 1) | compare_everything(n, 3)
    print(FIELDS[n], sorted(seen))
    # (conditions on the inputs: every class of index and rows without cells are met on the grids that are not a single line)
    assert min(field_of(n).shape) == 1 or seen >= {"novel", "unexplored", "behind", "short", "on", "no cells"}


def test_sixty_five_pairs(gpu):
    """More pairs than a status workgroup's waves hold, every cloud named, poses without a cell among them."""
    seen = compare_everything(0, 65)
    assert seen == {"novel", "unexplored", "behind", "short", "on", "no cells", "empty"}


def test_every_rule_for_a_device_count(gpu):
    """cnt_dev: a full count, shortened ones (to 0, into a wave, onto a chunk boundary), a negative one and an over-long one
    (both CAPACITY: nothing is read, nothing is written but the memset's zeros); NULL is every other test."""
    import torch
    from icpmi.batch import CloudSet
    field = field_of(0)
    ny, nx = field.shape
    clouds = kref.clouds(ny, nx, 0)
    full = CloudSet.from_numpy(clouds)
    cnt = np.array([0, 1, 10, -1, 66, 0, 200, 256, 514], dtype=np.int32)
    cs = CloudSet(full.pts, full.off_host, cnt=on_device(cnt))
    pair = np.arange(9, dtype=np.int32)
    _, t, rot = kref.poses(ny, nx, 9, 5)
    t[5:8] = t[0] + 0.1                                            # (poses with cells, so that the counts decide)
    counts = [kref.rows_of(len(clouds[c]), cnt[c]) for c in pair]
    assert counts == [0, 1, 10, -1, -1, 0, 200, 256, -1]
    H, beyond, table = 8, 2.0, ref.table_of(8)
    walks = [ref.walk_rows(field, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, clouds[c][:max(counts[c], 0)], t[b], rot[b], beyond)
             for b, c in enumerate(pair)]
    want = expected(walks, counts, 513, table, H)
    rec, hist, rows, _ = device_beam(on_device(field), cs, pair, t, rot, table, H, beyond)
    assert same(rec, want[0], "records") and same(hist, want[1], "histograms") and same(rows, want[2], "rows")
    assert rec[:, ref.STATUS].tolist() == [ref.ST_EMPTY, ref.ST_OK, ref.ST_OK, ref.ST_CAPACITY, ref.ST_CAPACITY, ref.ST_EMPTY, ref.ST_OK, ref.ST_OK,
                                           ref.ST_CAPACITY]
    assert torch.equal(cs.cnt.cpu(), torch.from_numpy(cnt))


def test_hand_made_rows_on_the_device(gpu):
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field, cases = ref.hand_made()
    fd = on_device(field)
    for case in cases:
        pts, t, rot, table, H, beyond = ref.hand_made_pair(case)
        cs = CloudSet.from_numpy([pts])
        rec, hist, rows = gridmatch.beam_pairs(fd, cref.THRESHOLD, 0.0, 0.0, 1.0, cs, [0], [t], [rot], table, H, beyond, want_hist=True, want_rows=True)
        assert rec.cpu().numpy().tolist() == [case[5]] and rows.cpu().numpy().tolist() == [case[7]], case
        assert np.array_equal(hist.cpu().numpy()[0], ref.hist_of(case)), case
    # an empty grid: nothing is packed, every row with cells returned from off the grid
    pts, t, rot, table, H, beyond = ref.hand_made_pair(cases[12])
    empty = np.zeros((0, 9), dtype=np.int16)
    rec, hist, rows = gridmatch.beam_pairs(on_device(empty), 1, 0.0, 0.0, 1.0, CloudSet.from_numpy([pts]), [0], [t], [rot], table, H, beyond,
                                           want_hist=True, want_rows=True)
    want = ref.beam_pair(empty, 1, 0.0, 0.0, 1.0, pts, t, rot, table, H, beyond)
    assert all(np.array_equal(got.cpu().numpy()[0], w) for got, w in zip((rec, hist, rows), want)) and want[0][ref.UNEXPLORED] == 2
    # no pair: nothing to do is no refusal
    rec, hist, rows = gridmatch.beam_pairs(fd, cref.THRESHOLD, 0.0, 0.0, 1.0, CloudSet.from_numpy([pts]), [], np.zeros((0, 2)), np.zeros((0, 2)), table, H,
                                           beyond, want_hist=True, want_rows=True)
    assert rec.shape == (0, ref.INTS) and hist.shape == (0, 2 * H + 3) and rows.shape == (0, 0, ref.ROW_INTS)
    # what the entry would refuse raises before it is called
    cs = CloudSet.from_numpy([pts])
    for bad in (dict(beyond=-1.0), dict(beyond=float("nan")), dict(beyond=float("inf")), dict(half_width=-1), dict(half_width=128),
                dict(table=table[:-1]), dict(table=table.astype(np.float64))):
        kw = {**dict(table=table, half_width=H, beyond=beyond), **bad}
        with pytest.raises(ValueError):
            gridmatch.beam_pairs(fd, cref.THRESHOLD, 0.0, 0.0, 1.0, cs, [0], [t], [rot], **kw)


def test_without_beyond_the_rows_are_the_checks(gpu):
    """beyond = 0: [k_hit, k_z, k_unknown] of every row with cells equal check_pairs' [k_hit, K, k_unknown] on the same inputs;
    a row at the origin alone has cells there and none here."""
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    field = field_of(0)
    ny, nx = field.shape
    clouds = kref.clouds(ny, nx, 0)
    cs = CloudSet.from_numpy(clouds)
    pair, t, rot = kref.poses(ny, nx, 65, 0)
    planes = gridmatch.occupancy_planes(on_device(field), cref.THRESHOLD)
    _, _, rows = gridmatch.beam_pairs(planes, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, cs, pair, t, rot, ref.table_of(8), 8, 0.0, want_rows=True)
    _, check = gridmatch.check_pairs(planes, cref.THRESHOLD, kref.MIN_X, kref.MIN_Y, kref.RES, cs, pair, t, rot, 2, want_rows=True)
    rows, check = rows.cpu().numpy(), check.cpu().numpy()
    compared = 0
    for b, c in enumerate(pair):
        n = len(clouds[c])
        zero = (clouds[c] == 0.0).all(axis=1)
        mine, theirs = rows[b, :n][~zero], check[b, :n][~zero]
        assert np.array_equal(mine[:, 1:], theirs[:, 1:]) and np.array_equal(mine[:, 0] == ref.NO_CELLS, theirs[:, 0] == kref.NO_CELLS), b
        assert (rows[b, :n][zero, 0] == ref.NO_CELLS).all()
        compared += int((mine[:, 0] >= 0).sum())
    assert compared > 5000


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


def restated_info(grid, scans, poses, table, H, beyond, occupied=0.5):
    k = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    q = gref.quantise(grid.log_odds, k)
    out = [ref.beam_pair(q, int(np.rint(occupied * 2.0 ** k)), grid.min_x, grid.min_y, grid.resolution, s, p[:2], (np.cos(p[2]), np.sin(p[2])), table, H, beyond)
           for s, p in zip(scans, poses)]
    return np.array([r for r, _, _ in out]).astype(np.int64), np.array([h for _, h, _ in out]).astype(np.int64), [rows for _, _, rows in out]


KEYS = (("status", ref.STATUS), ("rows", ref.ROWS), ("score", ref.SCORE), ("expected", ref.EXPECTED), ("novel", ref.NOVEL), ("unexplored", ref.UNEXPLORED))


def info_equals(info, rec, hist=None, classes=None):
    ok = all(info[key].dtype == np.int64 and np.array_equal(info[key], rec[:, slot]) for key, slot in KEYS)
    ok = ok and np.array_equal(info["mean_score"], np.where(rec[:, ref.ROWS] > 0, rec[:, ref.SCORE] / np.maximum(rec[:, ref.ROWS], 1), 0.0))
    if hist is not None:
        ok = ok and info["histogram"].dtype == np.int64 and np.array_equal(info["histogram"], hist)
    if classes is not None:
        ok = ok and len(info["classes"]) == len(classes) and all(np.array_equal(a, b) for a, b in zip(info["classes"], classes))
    return ok


def test_beam_methods_of_the_grid_agree_with_beam_pairs_and_the_restatement(small_map):
    from icpmi import gridmatch
    grid, scans, poses = small_map
    H = 8
    default, beyond = gridmatch.beam_table(grid.resolution, grid.resolution, H), 1.5 * (H + 2) * grid.resolution
    rec, hist, classes = restated_info(grid, scans, poses, default, H, beyond)
    info = grid.beam_scans(scans, poses, want_histogram=True, want_rows=True)
    print("true poses:", rec[:, :6].tolist())
    assert info["shift_bits"] == 12 and info_equals(info, rec, hist, classes)
    plain = grid.beam_scans(scans, poses)
    assert info_equals(plain, rec) and "classes" not in plain and "histogram" not in plain
    assert (rec[:, ref.EXPECTED] > 0.75 * rec[:, ref.ROWS]).all()
    # ... and with the layer below on the same field
    field, k = grid.score_field()
    cos_sin = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
    below, _, _ = gridmatch.beam_pairs(field, int(np.rint(0.5 * 2.0 ** k)), grid.min_x, grid.min_y, grid.resolution, gridmatch.cloud_set_of(scans),
                                       np.arange(3), poses[:, :2], cos_sin, default, H, beyond)
    assert np.array_equal(below.cpu().numpy(), rec)
    # one scan; one scan at many poses (a matrix among the ways to give one); another table, half width, beyond and threshold
    one = grid.beam_scan(scans[1], poses[1], want_histogram=True, want_rows=True)
    assert all(int(one[key]) == rec[1, slot] for key, slot in KEYS) and np.array_equal(one["classes"], classes[1]) and np.array_equal(one["histogram"], hist[1])
    assert one["mean_score"] == rec[1, ref.SCORE] / rec[1, ref.ROWS]
    th = poses[1, 2]
    matrix = np.array([[np.cos(th), -np.sin(th), poses[1, 0]], [np.sin(th), np.cos(th), poses[1, 1]], [0, 0, 1.0]])
    assert grid.beam_scan(scans[1], matrix)["score"] == rec[1, ref.SCORE]
    hyp = np.concatenate([poses, poses + [0.7, -0.4, 0.2], [[np.nan, 0.0, 0.0]]])
    table3 = gridmatch.beam_table(grid.resolution, 0.25, 3, unexplored=0.05)
    want = restated_info(grid, [scans[0]] * len(hyp), hyp, table3, 3, 0.4, occupied=1.0)
    got = grid.beam_poses(scans[0], hyp, sigma=0.25, half_width=3, beyond=0.4, table=table3, occupied_log_odds=1.0, want_histogram=True, want_rows=True)
    assert info_equals(got, *want) and got["status"][-1] == ref.ST_EMPTY and got["mean_score"][-1] == 0.0
    assert want[0][3, ref.SCORE] < want[0][0, ref.SCORE] < 0
    want = restated_info(grid, [scans[0]] * len(hyp), hyp, gridmatch.beam_table(grid.resolution, 0.25, 3), 3, 1.5 * 5 * grid.resolution)
    assert info_equals(grid.beam_poses(scans[0], hyp, sigma=0.25, half_width=3), want[0])        # the defaults follow sigma and half_width
    w, ess = gridmatch.pose_weights(got["score"], temperature=20.0, status=got["status"])
    assert w[-1] == 0.0 and abs(w.sum() - 1.0) < 1e-12 and np.argmax(w) == 0 and 1.0 <= ess < 6.0
    # field= and planes= as in check_scans: the same bytes, and both together or planes of another grid are refused
    for kw in (dict(field=(field, k)), dict(planes=grid.occupancy_planes()), dict(planes=grid.occupancy_planes(field=(field, k)))):
        assert info_equals(grid.beam_scans(scans, poses, **kw), rec)
    from utilities.mapping import OccupancyGrid2D
    other = OccupancyGrid2D(-1.0, 1.0, -1.0, 1.0)
    with pytest.raises(ValueError):
        grid.beam_scans(scans, poses, field=(field, k), planes=grid.occupancy_planes())
    with pytest.raises(ValueError):
        other.beam_scans(scans, poses, planes=grid.occupancy_planes())
    with pytest.raises(ValueError):
        other.beam_poses(scans[0], poses, field=(field, k))
    with pytest.raises(ValueError):
        grid.beam_scans(scans, poses, beyond=-1.0)
    with pytest.raises(ValueError):
        grid.beam_scans(scans, poses, half_width=128)
    with pytest.raises(ValueError):
        grid.beam_scans(scans, poses, table=default[:-1])
    with pytest.raises(ValueError):
        grid.beam_scans(scans, poses[:2])


def test_beam_history_equals_beam_scans(small_map):
    from icpmi import ScanHistory, gridmatch
    grid, scans, poses = small_map
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=4, row_capacity=1024)
    hist.add_many(scans)
    ids = [2, 0, 2, 1]
    p4 = poses[[2, 0, 1, 1]]
    got = grid.beam_history(hist, ids, p4, want_histogram=True, want_rows=True)
    want = grid.beam_scans([scans[i] for i in ids], p4, want_histogram=True, want_rows=True)
    assert all(np.array_equal(got[key], want[key]) for key, _ in KEYS) and all(np.array_equal(a, b) for a, b in zip(got["classes"], want["classes"]))
    assert np.array_equal(got["histogram"], want["histogram"])
    H = 8
    assert info_equals(got, *restated_info(grid, [scans[i] for i in ids], p4, gridmatch.beam_table(grid.resolution, grid.resolution, H), H,
                                           1.5 * (H + 2) * grid.resolution))
    for voxel in (0.05, 0.3, 0.17):                                # the history's own filtered copies (device counts), or a fresh filter
        got = grid.beam_history(hist, ids, p4, voxel_size=voxel, want_histogram=True, want_rows=True)
        want = grid.beam_scans([scans[i] for i in ids], p4, voxel_size=voxel, want_histogram=True, want_rows=True)
        assert all(np.array_equal(got[key], want[key]) for key, _ in KEYS) and np.array_equal(got["histogram"], want["histogram"]), voxel
        assert [len(c) for c in got["classes"]] == [len(c) for c in want["classes"]] and (got["rows"] == [len(c) for c in got["classes"]]).all()
        assert (got["rows"] <= 256).all() and (got["rows"] > 0).all() and (got["histogram"].sum(axis=1) == got["rows"]).all()
    with pytest.raises(ValueError, match="scan ids must lie in"):
        grid.beam_history(hist, [7], [poses[0]])
