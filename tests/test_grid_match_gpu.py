"""Correlative scan-to-map matching on the device (csrc/gridmatch.hip; icpmi.gridmatch; the matching methods of
utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract (tests/gridmatch_ref.py).  Every score is
an integer sum, so everything is compared with array_equal: the field, the full score volume, the records, and the poses the
host layer forms from them.

Volume cases run on a 64 x 48 grid at 0.25 m; the Python layer on the room of tests/test_grid_match_cpu.py, whose map is
built once on the device."""
import types

import numpy as np
import pytest

import gridmatch_ref as ref

pytestmark = pytest.mark.gpu

SMALL = dict(min_x=-6.0, min_y=-8.0, resolution=0.25, log_odds_min=-5.0, log_odds_max=5.0)     # nx = 48, ny = 64
CHUNK = 256


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert _lib.GM_CHUNK_ROWS == CHUNK


def small_grid(values):
    """A stand-in for an OccupancyGrid2D over a (64, 48) float32 array: what GridMatchBatch reads of a grid."""
    import torch
    return types.SimpleNamespace(device_log_odds=torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).cuda(), **SMALL)


@pytest.fixture(scope="module")
def small(gpu):
    """(grid stand-in, its field by the restatement): random log-odds inside the clamp."""
    lo = np.random.default_rng(11).uniform(-5.0, 5.0, size=(64, 48)).astype(np.float32)
    return small_grid(lo), ref.quantise(lo, ref.shift_bits(-5.0, 5.0))


def run_device(grid, clouds, pair_clouds, translations, angles, W, centre, cnt=None):
    """One launch -> (volume [B, A, S, S], records [B, 8]) on the host, and the job."""
    import torch
    from icpmi.batch import CloudSet
    from icpmi.gridmatch import GridMatchBatch
    cs = CloudSet.from_numpy(clouds)
    if cnt is not None:
        cs.cnt = torch.tensor(cnt, dtype=torch.int32, device=cs.pts.device)
    job = GridMatchBatch(grid, cs, pair_clouds, translations, angles, W, centre, want_scores=True)
    rec = job.run()
    torch.cuda.synchronize()
    return job.scores.cpu().numpy()[:len(pair_clouds)], rec.cpu().numpy()[:len(pair_clouds)], job


def run_ref(q, clouds, pair_clouds, translations, angles, W, centre):
    vols, recs = [], []
    for b, c in enumerate(pair_clouds):
        vol, rows = ref.volume(q, clouds[c], translations[b], ref.cos_sin_of(np.asarray(angles, dtype=np.float64)[b]), W,
                               SMALL["min_x"], SMALL["min_y"], SMALL["resolution"])
        vols.append(vol)
        recs.append(ref.record(vol, rows, centre, W))
    return np.stack(vols), np.stack(recs)


def disc(rng, n, radius=5.0):
    r, a = radius * np.sqrt(rng.uniform(size=n)), rng.uniform(-np.pi, np.pi, size=n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


# ── 1. the field ─────────────────────────────────────────────────────────────
def test_field_equals_the_restatement(gpu):
    import torch
    from icpmi import gridmatch
    rng = np.random.default_rng(3)
    lo = rng.uniform(-9.0, 9.0, size=(37, 53)).astype(np.float32)                   # beyond +-8: saturating at k = 12
    lo.ravel()[:12] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e30, -1e30, 8.0, -8.0, 7.99993, 1e-30, -1e-40]
    lo[5, :9] = (np.arange(9) - 4 + 0.5) / 4096.0                                   # x.5 / 2^k: half to even
    lo[36, 52] = np.nan                                                              # the last cell, in the ragged tail
    for k in (12, 0, 14, 5):
        got = gridmatch.score_field(torch.from_numpy(lo).cuda(), k)
        assert got.dtype == torch.int16 and tuple(got.shape) == (37, 53)
        assert np.array_equal(got.cpu().numpy(), ref.quantise(lo, k)), k
    for shape in ((1, 1), (1, 7), (1, 8), (3, 3), (2048, 1), (256, 8), (257, 8)):    # below, at and across a thread's eight cells
        a = rng.uniform(-6.0, 6.0, size=shape).astype(np.float32)
        assert np.array_equal(gridmatch.score_field(torch.from_numpy(a).cuda(), 12).cpu().numpy(), ref.quantise(a, 12)), shape


# ── 2. volume and record ─────────────────────────────────────────────────────
VOLUME_CASES = ([(n, 6, 2, c) for n, c in zip((1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 4097), (-1, 1, -1, 0, 1, -1, 0, 1))] +
                [(65, 0, 1, 0), (CHUNK + 1, 0, 2, -1), (65, 1, 1, -1), (CHUNK + 1, 1, 65, 33), (64, 0, 65, -1), (300, 6, 65, 64),
                 (CHUNK + 1, 31, 2, 1), (65, 31, 1, -1), (4097, 31, 1, 0), (4097, 0, 1, 0), (700, 3, 2, 0), (700, 8, 2, -1),
                 (300, 15, 1, 0), (300, 22, 2, -1)])


@pytest.mark.parametrize("n,W,A,centre", VOLUME_CASES)
def test_volume_and_record_equal_the_restatement(small, n, W, A, centre):
    grid, q = small
    rng = np.random.default_rng(1000 * n + 10 * W + A)
    clouds = [disc(rng, n)]
    t = rng.uniform(-2.0, 2.0, size=(1, 2))
    angles = rng.uniform(-np.pi, np.pi, size=(1, A))
    vol, rec, _ = run_device(grid, clouds, [0], t, angles, W, centre)
    want_vol, want_rec = run_ref(q, clouds, [0], t, angles, W, centre)
    assert vol.dtype == np.int32 and vol.shape == (1, A, 2 * W + 1, 2 * W + 1)
    assert np.array_equal(vol, want_vol)
    assert np.array_equal(rec, want_rec), (rec, want_rec)
    assert rec[0, 0] == ref.ST_OK and rec[0, 1] == n


# ── 3. edges ─────────────────────────────────────────────────────────────────
def test_clouds_across_the_borders_bad_rows_and_an_empty_cloud(small):
    """The grid spans x in [-6, 6), y in [-8, 8).  Clouds partly outside, wholly outside and straddling each side, with
    negative cells and windows that cross a corner; rows with NaN and inf; a row at 1e12; an empty cloud."""
    grid, q = small
    rng = np.random.default_rng(5)
    blob = disc(rng, 300, 1.5)
    bad = np.vstack([disc(rng, 40, 2.0), [[np.nan, 0.0], [0.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [1e12, 0.0], [0.0, -1e12],
                                         [1e300, 1e300], [2.0 ** 29 * 0.25, 0.0]], disc(rng, 30, 2.0)])
    only_bad = np.array([[np.nan, np.nan], [np.inf, 0.0], [1e12, 1e12]])
    clouds = [blob, bad, np.zeros((0, 2)), only_bad]
    W, A = 6, 3
    cases = [(0, (-6.0, 0.0)), (0, (6.0, 0.0)), (0, (0.0, -8.0)), (0, (0.0, 8.0)),          # straddling each side
             (0, (-6.2, -8.2)), (0, (5.9, 7.9)), (0, (-6.1, 7.9)), (0, (6.0, -8.0)),        # the corners
             (0, (-8.5, 0.0)), (0, (8.5, 9.0)),                                             # only the window reaches the grid
             (0, (100.0, -100.0)), (0, (-1e7, 0.0)),                                        # wholly outside
             (0, (0.0, 0.0)), (1, (0.0, 0.0)), (1, (-5.0, 7.0)), (2, (0.0, 0.0)), (3, (0.0, 0.0))]
    pair = [c for c, _ in cases]
    t = np.array([tt for _, tt in cases])
    angles = rng.uniform(-np.pi, np.pi, size=(len(cases), A))
    angles[:, 0] = 0.0
    vol, rec, _ = run_device(grid, clouds, pair, t, angles, W, 0)
    want_vol, want_rec = run_ref(q, clouds, pair, t, angles, W, 0)
    assert np.array_equal(vol, want_vol)
    assert np.array_equal(rec, want_rec), (rec, want_rec)
    assert vol[:10].any(axis=(1, 2, 3)).all()                                       # the border cases do reach the grid
    for b in (10, 11):                                                              # wholly outside: rows with cells, all scores 0
        assert not vol[b].any() and list(rec[b]) == [ref.ST_OK, 300, 0, 0, 0, 0, 0, 0]
    assert rec[13, 1] in (70, 71) and rec[13, 0] == ref.ST_OK                       # the bad rows drop out (the cell at 2^29 + 24 at angle 0)
    for b in (15, 16):                                                              # no row, and no row with a cell: EMPTY
        assert not vol[b].any() and list(rec[b]) == [ref.ST_EMPTY, 0, 0, 0, 0, 0, 0, 0]


def test_a_count_beyond_the_cloud_is_capacity(small):
    from icpmi import _lib
    grid, q = small
    rng = np.random.default_rng(6)
    clouds = [disc(rng, 50), disc(rng, 60), disc(rng, 70)]
    vol, rec, _ = run_device(grid, clouds, [0, 1, 2], np.zeros((3, 2)), np.zeros((3, 1)), 2, 0, cnt=[-1, 40, 71])
    want_vol, want_rec = run_ref(q, [clouds[1][:40]], [0], np.zeros((1, 2)), np.zeros((1, 1)), 2, 0)
    assert np.array_equal(vol[1:2], want_vol) and np.array_equal(rec[1:2], want_rec)          # a device count below the capacity
    for b in (0, 2):
        assert not vol[b].any() and list(rec[b]) == [_lib.GM_ST_CAPACITY, 0, 0, 0, 0, 0, 0, 0]


# ── 4. ties ──────────────────────────────────────────────────────────────────
def test_ties_go_to_the_lowest_flat_index(gpu):
    zero = small_grid(np.zeros((64, 48)))
    rng = np.random.default_rng(8)
    clouds = [disc(rng, 500)]
    vol, rec, _ = run_device(zero, clouds, [0], [[0.3, -0.2]], rng.uniform(-1, 1, size=(1, 5)), 6, 2)
    assert not vol.any() and list(rec[0]) == [ref.ST_OK, 500, 0, 0, 0, 0, 0, 0]
    # two equal isolated peaks, reached by one point at two different (a, j, i): angle 0 puts the point (1.1, 0.6) into cell
    # (28, 34), a quarter turn puts it into cell (21, 36); the peaks lie two cells right of the first and one above the second
    lo = np.zeros((64, 48), dtype=np.float32)
    lo[34, 30] = lo[37, 21] = 3.25
    peaks = small_grid(lo)
    q = ref.quantise(lo, 12)
    # (a half turn puts it far from both)
    for angles, first, second in (([[np.pi, 0.0, np.pi / 2]], (1, 3, 5), (2, 4, 3)), ([[np.pi / 2, np.pi, 0.0]], (0, 4, 3), (2, 3, 5))):
        vol, rec, _ = run_device(peaks, [np.array([[1.1, 0.6]])], [0], [[0.0, 0.0]], angles, 3, -1)
        want_vol, want_rec = run_ref(q, [np.array([[1.1, 0.6]])], [0], [[0.0, 0.0]], angles, 3, -1)
        assert np.array_equal(vol, want_vol) and np.array_equal(rec, want_rec)
        best = np.flatnonzero(vol.ravel() == vol.max())
        assert len(best) == 2 and vol.max() == 3.25 * 4096
        assert [tuple(int(v) for v in np.unravel_index(f, vol.shape[1:])) for f in best] == [first, second]
        assert rec[0, 2] == best[0] and tuple(rec[0, 3:6]) == first


# ── 5. batches ───────────────────────────────────────────────────────────────
def test_a_batch_equals_its_pairs_alone_and_a_second_run(small):
    grid, q = small
    rng = np.random.default_rng(21)
    B, W, A = 70, 2, 3
    sizes = rng.integers(1, 600, size=B)
    sizes[:4] = (1, CHUNK, CHUNK + 1, 599)
    clouds = [disc(rng, int(n), rng.uniform(1.0, 6.0)) for n in sizes]
    t = rng.uniform(-5.0, 5.0, size=(B, 2))
    angles = rng.uniform(-np.pi, np.pi, size=(B, A))
    pair = rng.permutation(B)
    vol, rec, job = run_device(grid, clouds, pair, t, angles, W, 1)
    for b in range(B):                                             # 70 launches, each over its own cloud set: max_n differs
        v1, r1, _ = run_device(grid, [clouds[pair[b]]], [0], t[b:b + 1], angles[b:b + 1], W, 1)
        assert np.array_equal(v1[0], vol[b]) and np.array_equal(r1[0], rec[b]), b
    want_vol, want_rec = run_ref(q, clouds, pair, t, angles, W, 1)
    assert np.array_equal(vol, want_vol) and np.array_equal(rec, want_rec)
    # the same job again, on the same workspace and volume: zeroed per call, so nothing accumulates
    import torch
    rec2 = job.run()
    torch.cuda.synchronize()
    assert np.array_equal(job.scores.cpu().numpy(), vol) and np.array_equal(rec2.cpu().numpy(), rec)
    # and without the volume handed out (it then lives in the workspace): the same records
    from icpmi.batch import CloudSet
    from icpmi.gridmatch import GridMatchBatch
    plain = GridMatchBatch(grid, CloudSet.from_numpy(clouds), pair, t, angles, W, 1)
    assert plain.scores is None
    for _ in range(2):
        assert np.array_equal(plain.run().cpu().numpy(), rec)


# ── 6. the Python layer ──────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def room(gpu):
    """(grid built by update_scans on the device, its field by the restatement, the queries)."""
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**ref.SCENE)
    assert (grid.ny, grid.nx) == (200, 280)
    origins, hits = ref.scene_scans()
    grid.update_scans(origins, hits)
    k = ref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    return grid, ref.quantise(grid.log_odds, k), ref.scene_queries(), k


def ref_match(grid, q, scan, pred, W=6, angular_window=12.0, angular_step=1.0):
    angles = ref.angle_rows(pred[2], angular_window, angular_step)
    cs = ref.cos_sin_of(angles)
    vol, rows = ref.volume(q, scan, pred[:2], cs, W, grid.min_x, grid.min_y, grid.resolution)
    rec = ref.record(vol, rows, len(angles) // 2, W)
    return rec, ref.pose(rec, pred[:2], cs, W, grid.resolution)


def test_match_scan_returns_the_restatements_pose(room):
    grid, q, queries, k = room
    field, kk = grid.score_field()
    assert kk == k == 12 and np.array_equal(field.cpu().numpy(), q)
    for true, pred, scan in queries[:4]:
        R, t, score, info = grid.match_scan(scan, pred)
        rec, (want_R, want_t) = ref_match(grid, q, scan, pred)
        assert (info["a"], info["j"], info["i"]) == (rec[3], rec[4], rec[5]) and info["index"] == rec[2]
        assert np.array_equal(R, want_R) and np.array_equal(t, want_t)
        assert score == rec[6] and info["centre_score"] == rec[7] and info["rows"] == rec[1] == len(scan) and info["status"] == 0
        assert info["shift_bits"] == 12 and info["mean_log_odds"] == rec[6] / (len(scan) * 4096.0)
        assert np.abs(t - np.array(true[:2])).max() <= 0.1 and abs(np.rad2deg(info["angle"] - true[2])) <= 1.0
        T = np.array([[np.cos(pred[2]), -np.sin(pred[2]), pred[0]], [np.sin(pred[2]), np.cos(pred[2]), pred[1]], [0.0, 0.0, 1.0]])
        if np.arctan2(T[1, 0], T[0, 0]) == pred[2]:                                  # the pose as a matrix: the same call
            R2, t2, score2, _ = grid.match_scan(scan, T)
            assert np.array_equal(R2, R) and np.array_equal(t2, t) and score2 == score


def test_match_scans_equals_match_scan_and_other_windows(room):
    grid, q, queries, _ = room
    scans, preds = [s for _, _, s in queries[:5]], [p for _, p, _ in queries[:5]]
    scans[2] = scans[2][:301]
    R, t, score, info = grid.match_scans(scans, preds)
    for b in range(5):
        R1, t1, s1, i1 = grid.match_scan(scans[b], preds[b])
        assert np.array_equal(R[b], R1) and np.array_equal(t[b], t1) and score[b] == s1
        assert all(info[key][b] == i1[key] for key in ("status", "rows", "index", "a", "j", "i", "centre_score", "angle", "mean_log_odds"))
    R, t, score, info = grid.match_scans(scans[:2], preds[:2], linear_window=0.34, angular_window=5.0, angular_step=2.5)
    for b in range(2):                                             # W = int(round(3.4)) = 3; offsets -5, -2.5, 0, 2.5, 5
        rec, (want_R, want_t) = ref_match(grid, q, scans[b], preds[b], 3, 5.0, 2.5)
        assert (info["a"][b], info["j"][b], info["i"][b], score[b]) == (rec[3], rec[4], rec[5], rec[6])
        assert np.array_equal(R[b], want_R) and np.array_equal(t[b], want_t)
    # through the voxel filter: the restatement on the filtered rows
    from utilities.icp import voxel_downsample
    R, t, score, info = grid.match_scan(scans[0], preds[0], voxel_size=0.2)
    filtered = voxel_downsample(scans[0], 0.2)
    rec, (want_R, want_t) = ref_match(grid, q, filtered, preds[0])
    assert info["rows"] == len(filtered) < len(scans[0]) and score == rec[6] and info["index"] == rec[2]
    assert np.array_equal(R, want_R) and np.array_equal(t, want_t)


def test_score_poses_equals_the_restatement(room):
    grid, q, queries, _ = room
    true, _, scan = queries[0]
    rng = np.random.default_rng(4)
    poses = np.array(true) + rng.uniform(-1.0, 1.0, size=(300, 3)) * np.array([0.6, 0.6, 0.3])
    poses[:3] = ((true[0], true[1], true[2]), (100.0, 0.0, 0.0), (-13.9, -9.9, 1.0))      # the true pose; off the map; across a corner
    score, info = grid.score_poses(scan, poses)
    want = np.array([ref.volume(q, scan, p[:2], ref.cos_sin_of(p[2:3]), 0, grid.min_x, grid.min_y, grid.resolution)[0][0, 0, 0]
                     for p in poses])
    assert score.shape == (300,) and np.array_equal(score, want)
    assert np.array_equal(info["centre_score"], want) and (info["rows"] == len(scan)).all() and not info["index"].any()
    assert score[0] > 0 and score[1] == 0


def test_match_history_equals_match_scans(room):
    from icpmi import ScanHistory
    grid, q, queries, _ = room
    scans, preds = [s for _, _, s in queries], [p for _, p, _ in queries]
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=2, row_capacity=1500)
    hist.add_many(scans[:2])
    ids = [1, 0, 1]
    got = grid.match_history(hist, ids, [preds[1], preds[0], preds[3]])
    want = grid.match_scans([scans[i] for i in ids], [preds[1], preds[0], preds[3]])
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert all(np.array_equal(got[3][key], want[3][key]) for key in want[3])
    cap = (hist.scan_capacity, hist.row_capacity)
    hist.add_many(scans[2:7])                                      # the history grows: new buffers, the same answers
    assert (hist.scan_capacity, hist.row_capacity) != cap
    ids = [6, 0, 3, 3]
    p4 = [preds[6], preds[0], preds[3], preds[4]]
    got = grid.match_history(hist, ids, p4, linear_window=0.4)
    want = grid.match_scans([scans[i] for i in ids], p4, linear_window=0.4)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert all(np.array_equal(got[3][key], want[3][key]) for key in want[3])
    # the history's own filtered copies serve its two voxel sizes; any other size filters the resident rows
    for voxel in (0.05, 0.3, 0.17):
        got = grid.match_history(hist, ids, p4, voxel_size=voxel)
        want = grid.match_scans([scans[i] for i in ids], p4, voxel_size=voxel)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w), voxel
        assert np.array_equal(got[3]["rows"], want[3]["rows"]) and (got[3]["rows"] <= 1024).all()
    with pytest.raises(ValueError, match="scan ids must lie in"):
        grid.match_history(hist, [7], [preds[0]])


def test_a_field_passed_back_scores_the_map_as_it_was():
    """field= from an earlier score_field() gives the result of rebuilding; after a further update_scan it keeps scoring the old
    map until it is refreshed.  (A grid of its own: the module's map stays as it is.)"""
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**ref.SCENE)
    origins, hits = ref.scene_scans()
    grid.update_scans(origins[:6], hits[:6])
    true, pred, scan = ref.scene_queries()[1]
    field = grid.score_field()
    fresh = grid.match_scan(scan, pred)
    kept = grid.match_scan(scan, pred, field=field)
    assert np.array_equal(fresh[0], kept[0]) and np.array_equal(fresh[1], kept[1]) and fresh[2] == kept[2]
    before = field[0].cpu().numpy().copy()
    p = (2.0, 0.2, 0.4)
    grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 77), p))
    stale = grid.match_scan(scan, pred, field=field)
    rebuilt = grid.match_scan(scan, pred)
    assert np.array_equal(field[0].cpu().numpy(), before) and stale[2] == kept[2] and stale[3]["index"] == kept[3]["index"]
    assert rebuilt[2] != kept[2]
    k = field[1]
    q_old, q_new = before, ref.quantise(grid.log_odds, k)
    for got, q in ((stale, q_old), (rebuilt, q_new)):
        rec, (want_R, want_t) = ref_match(grid, q, scan, pred)
        assert got[2] == rec[6] and got[3]["index"] == rec[2] and np.array_equal(got[1], want_t)
    s_old, _ = grid.score_poses(scan, [pred, true], field=field)
    s_new, _ = grid.score_poses(scan, [pred, true])
    assert s_old[1] > s_old[0] and s_new[1] > s_new[0] and s_new[1] != s_old[1]
