"""The moments of a scan-to-map match on the device (csrc/gridmoments.hip; icpmi.gridmatch.match_moments, GridMatchBatch(...,
half_log_odds=), the matching methods of utilities.mapping.OccupancyGrid2D) against the NumPy restatement
(tests/gridmoments_ref.py).  Every weight and every sum is an integer, so everything is compared with array_equal.

The raw entry runs on synthetic volumes and hand-made records, so that the edges of the weight rule — a drop of exactly m h / 8
and one either side of it, the whole int32 range, h = 1 and h = 65 535 * 32 767 — are hit on purpose; the layers run on the
small random grid and on the room of tests/test_grid_match_gpu.py."""
import types

import numpy as np
import pytest

import gridmatch_ref as ref
import gridmoments_ref as mref

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SHAPES = [(1, 0), (1, 1), (2, 6), (25, 6), (3, 31), (65, 1), (1024, 0)]        # (angles, window): 1 ... 11 907 candidates
HALF_STEPS = (1, 1024, 32767)
ROWS = (0, 1, 1430, 65535)
SMALL = dict(min_x=-6.0, min_y=-8.0, resolution=0.25, log_odds_min=-5.0, log_odds_max=5.0)     # nx = 48, ny = 64


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def device_moments(vols, recs, A, W, hs, out=None):
    """One call of the raw entry -> ((B, 12) int64 on the host, the device tensor)."""
    import torch
    from icpmi import gridmatch
    v = torch.from_numpy(np.ascontiguousarray(vols, dtype=np.int32)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(recs, dtype=np.int32)).cuda()
    m = gridmatch.match_moments(v, r, len(recs), A, W, hs, out)
    torch.cuda.synchronize()
    assert m.dtype == torch.int64 and m.shape[1] == 12
    return m.cpu().numpy()[:len(recs)], m


def record(rows, a, j, i, best, S, status=0):
    return [status, rows, (a * S + j) * S + i, a, j, i, best, 0]


def winners(A, S):
    """Corners, faces and the interior of the volume (fewer where the volume is too small to tell them apart)."""
    return sorted({(0, 0, 0), (A - 1, S - 1, S - 1), (A // 2, 0, S // 2), (0, S // 2, S // 2), (A // 2, S // 2, S // 2)})


def uniform_volume(rng, shape, at):
    """Scores uniform over the whole int32 range, INT32_MIN among them, INT32_MAX at the winner."""
    vol = rng.integers(I32_MIN, I32_MAX, size=shape, endpoint=True).astype(np.int32)
    vol.ravel()[:1] = I32_MIN
    vol[at] = I32_MAX
    return vol, I32_MAX


def ladder_volume(rng, shape, at, h):
    """Scores best - floor(m h / 8) + {-1, 0, 1} for m = 0 ... 170 (clipped to int32): a drop at every step of the weight rule,
    one short of it and one past it, up to and beyond the drop where the weight becomes 0; the one above `best` is clamped."""
    best = I32_MAX - 1
    steps = best - (np.arange(171, dtype=np.int64) * h) // 8
    vals = np.clip((steps[:, None] + np.array([-1, 0, 1])).ravel(), I32_MIN, I32_MAX)
    n = int(np.prod(shape))
    vol = np.resize(vals, max(n, len(vals)))[rng.permutation(max(n, len(vals)))[:n]].reshape(shape).astype(np.int32)
    vol[at] = best
    return vol, best


# ── 1, 2. shapes, scores, records ────────────────────────────────────────────
@pytest.mark.parametrize("hs", HALF_STEPS)
@pytest.mark.parametrize("A,W", SHAPES)
def test_moments_equal_the_restatement(gpu, A, W, hs):
    S = 2 * W + 1
    rng = np.random.default_rng(100 * A + W + hs)
    vols, recs = [], []
    for at in winners(A, S):
        for rows in ROWS:
            h = max(1, rows * hs)
            for vol, best in (uniform_volume(rng, (A, S, S), at), ladder_volume(rng, (A, S, S), at, h)):
                vols.append(vol)
                recs.append(record(rows, *at, best, S))
    got, _ = device_moments(np.stack(vols), recs, A, W, hs)
    want = np.stack([mref.moments(v, r, hs) for v, r in zip(vols, recs)])
    assert got.dtype == np.int64 and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (got[:, 0] >= 1 << 20).all() and (got[:, 10] >= 1).all() and (got[:, 10] <= A * S * S).all()    # the winner always counts
    if A * S * S > 600:
        assert got[:, 10].max() > 100                                           # the ladders do spread their weight


def test_headroom_at_the_capacities(gpu):
    """1 024 angles x 63^2 shifts, every score equal, the winner at index 0: every weight 2^20, the largest sums the entry
    can be asked for."""
    A, W = 1024, 31
    vol = np.full((1, A, 63, 63), 7, dtype=np.int32)
    rec = record(1430, 0, 0, 0, 7, 63)
    got, _ = device_moments(vol, [rec], A, W, 1024)
    assert np.array_equal(got[0], mref.moments(vol[0], rec, 1024))
    assert got[0, 4] == 1487384306207686656 and got[0, 0] == (A * 3969) << 20 and got[0, 10] == A * 3969
    assert got[0, 4] == got[0].max() < 2 ** 61


# ── 3. batches ───────────────────────────────────────────────────────────────
def test_a_batch_equals_its_pairs_alone_and_a_second_run(gpu):
    import torch
    B, A, W, hs = 70, 7, 6, 1024                                                # 1 183 candidates: two workgroups a pair
    S = 2 * W + 1
    rng = np.random.default_rng(31)
    vols, recs = [], []
    for b in range(B):
        rows = ROWS[b % 4] if b % 5 else int(rng.integers(1, 3000))
        h = max(1, rows * hs)
        at = (int(rng.integers(A)), int(rng.integers(S)), int(rng.integers(S)))
        best = I32_MAX - 1 - int(rng.integers(0, 1000))
        drop = rng.integers(0, min(25 * h, 2 ** 32 - 2000), size=(A, S, S))     # weights from 2^20 down to 0
        vol = (best - drop).astype(np.int32)
        vol[at] = best
        vols.append(vol)
        recs.append(record(rows, *at, best, S))
    recs[3][0] = mref.ST_CAPACITY                                               # nothing was read for this pair: twelve zeros
    recs[5][6] = int(np.median(vols[5]))                                        # a `best` below half of the scores: d clamps at 0
    recs[6][6] = I32_MIN
    vols = np.stack(vols)
    out = torch.full((B, 12), -1, dtype=torch.int64, device="cuda")             # the call zeroes it itself
    got, dev = device_moments(vols, recs, A, W, hs, out)
    assert dev is out
    want = np.stack([mref.moments(v, r, hs) for v, r in zip(vols, recs)])
    assert np.array_equal(got, want)
    assert not got[3].any() and got[6, 0] == (A * S * S) << 20 and got[5, 10] > A * S * S // 2
    for b in range(B):
        alone, _ = device_moments(vols[b:b + 1], recs[b:b + 1], A, W, hs)
        assert np.array_equal(alone[0], got[b]), b
    again, _ = device_moments(vols, recs, A, W, hs, out)                        # the same buffer, not cleared by the caller
    assert np.array_equal(again, got)


# ── 4. through the layers ────────────────────────────────────────────────────
def disc(rng, n, radius=5.0):
    r, a = radius * np.sqrt(rng.uniform(size=n)), rng.uniform(-np.pi, np.pi, size=n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def check_info_against(info, want_m, t, angle, res, step):
    from icpmi.gridmatch import gaussian_of_moments
    assert info["moments"].dtype == np.int64 and np.array_equal(info["moments"], want_m)
    g = gaussian_of_moments(want_m, res, step)
    for key in ("offset", "covariance", "support", "edge_weight"):
        assert np.array_equal(info[key], g[key]), key
    assert np.array_equal(info["t_refined"], t + g["offset"][:, :2]) and np.array_equal(info["angle_refined"], angle + g["offset"][:, 2])
    co, si = np.cos(info["angle_refined"]), np.sin(info["angle_refined"])
    assert np.array_equal(info["R_refined"], np.stack([np.stack([co, -si], axis=1), np.stack([si, co], axis=1)], axis=1))
    assert np.array_equal(info["covariance"], np.swapaxes(info["covariance"], 1, 2))


def test_match_batch_with_moments_on_the_small_grid(gpu):
    import torch
    from icpmi.batch import CloudSet
    from icpmi.gridmatch import GridMatchBatch, GridSearchBatch
    lo = np.random.default_rng(11).uniform(-5.0, 5.0, size=(64, 48)).astype(np.float32)
    grid = types.SimpleNamespace(device_log_odds=torch.from_numpy(lo).cuda(), **SMALL)
    q = ref.quantise(lo, 12)
    rng = np.random.default_rng(12)
    clouds = [disc(rng, 300), disc(rng, 1), disc(rng, 700, 3.0)]
    t = rng.uniform(-2.0, 2.0, size=(3, 2))
    angles = rng.uniform(-np.pi, np.pi, size=(3, 1)) + np.deg2rad(np.arange(-4.0, 5.0, 2.0))[None, :]
    W, centre, res = 3, 2, SMALL["resolution"]
    cs = CloudSet.from_numpy(clouds)
    job = GridMatchBatch(grid, cs, [0, 1, 2], t, angles, W, centre, half_log_odds=0.25)
    assert job.half_step == 1024 and job.scores is not None
    rec = job.run()
    R, tt, score, info = job.unpack()
    vols, recs, rows_of = [], [], []
    for b in range(3):
        vol, rows = ref.volume(q, clouds[b], t[b], ref.cos_sin_of(angles[b]), W, SMALL["min_x"], SMALL["min_y"], res)
        vols.append(vol)
        rows_of.append(rows)
        recs.append(ref.record(vol, rows, centre, W))
    assert np.array_equal(job.scores.cpu().numpy(), np.stack(vols)) and np.array_equal(rec.cpu().numpy(), np.stack(recs))
    want_m = np.stack([mref.moments(v, r, 1024) for v, r in zip(vols, recs)])
    check_info_against(info, want_m, tt, info["angle"], res, (angles[:, -1] - angles[:, 0]) / 4)
    assert (info["support"] >= 1).all() and np.isfinite(info["covariance"]).all()
    # without the argument: the same winner, record for record, and nothing about moments
    plain = GridMatchBatch(grid, cs, [0, 1, 2], t, angles, W, centre)
    assert plain.moments is None and plain.scores is None
    assert np.array_equal(plain.run().cpu().numpy(), rec.cpu().numpy())
    R0, t0, s0, i0 = plain.unpack()
    assert np.array_equal(R0, R) and np.array_equal(t0, tt) and np.array_equal(s0, score) and "moments" not in i0
    assert all(np.array_equal(i0[key], info[key]) for key in i0)
    # one angle: no step, the theta row and column are zero
    one = GridMatchBatch(grid, cs, [0, 2], t[[0, 2]], angles[[0, 2], 2:3], W, 0, half_log_odds=0.25)
    one.run()
    _, t1, _, i1 = one.unpack()
    want_1 = np.stack([mref.moments(vols[b][2:3], ref.record(vols[b][2:3], rows_of[b][2:3], 0, W), 1024) for b in (0, 2)])
    check_info_against(i1, want_1, t1, i1["angle"], res, 0.0)
    assert not i1["covariance"][:, 2, :].any() and not i1["covariance"][:, :, 2].any() and np.array_equal(i1["angle_refined"], i1["angle"])
    # an uneven angle row has no step; the wide search has no volume
    uneven = angles.copy()
    uneven[1, 3] += 1e-3
    with pytest.raises(ValueError, match="evenly spaced"):
        GridMatchBatch(grid, cs, [0, 1, 2], t, uneven, W, centre, half_log_odds=0.25)
    GridMatchBatch(grid, cs, [0, 1, 2], t, uneven, W, centre)                   # fine without moments, as before
    with pytest.raises(ValueError, match="no score volume"):
        GridSearchBatch(grid, cs, [0, 1, 2], t, angles, 40, centre, half_log_odds=0.25)
    with pytest.raises(ValueError, match="half_step"):
        GridMatchBatch(grid, cs, [0, 1, 2], t, angles, W, centre, half_log_odds=8.0)


@pytest.fixture(scope="module")
def room(gpu):
    """(grid built by update_scans on the device, its field by the restatement, the queries)."""
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**ref.SCENE)
    origins, hits = ref.scene_scans()
    grid.update_scans(origins, hits)
    k = ref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    assert k == 12
    return grid, ref.quantise(grid.log_odds, k), ref.scene_queries()


RECORD_KEYS = ("status", "rows", "index", "a", "j", "i", "centre_score")
MOMENT_KEYS = ("moments", "offset", "covariance", "support", "edge_weight", "t_refined", "angle_refined", "R_refined")


def test_match_methods_with_moments_in_the_room(room):
    from icpmi import ScanHistory
    grid, q, queries = room
    scans, preds = [s for _, _, s in queries[:3]], [p for _, p, _ in queries[:3]]
    R, t, score, info = grid.match_scans(scans, preds, half_log_odds=0.25)
    want_m, steps = [], []
    for b in range(3):
        angles = ref.angle_rows(preds[b][2])
        vol, rows = ref.volume(q, scans[b], preds[b][:2], ref.cos_sin_of(angles), 6, grid.min_x, grid.min_y, grid.resolution)
        rec = ref.record(vol, rows, 12, 6)
        assert [info[key][b] for key in RECORD_KEYS[:6]] == list(rec[:6]) and score[b] == rec[6] and info["centre_score"][b] == rec[7]
        want_m.append(mref.moments(vol, rec, 1024))
        steps.append((angles[-1] - angles[0]) / 24)
    check_info_against(info, np.stack(want_m), t, info["angle"], grid.resolution, np.array(steps))
    assert (info["support"] > 100).all() and (info["edge_weight"] < 0.01).all()
    for b in range(3):
        assert np.linalg.eigvalsh(info["covariance"][b]).min() > 0.0
    # the whole-cell winner is today's, with and without the argument
    R0, t0, s0, i0 = grid.match_scans(scans, preds)
    assert np.array_equal(R0, R) and np.array_equal(t0, t) and np.array_equal(s0, score) and not set(MOMENT_KEYS) & set(i0)
    assert all(np.array_equal(i0[key], info[key]) for key in i0)
    # match_scan and match_history agree with match_scans
    R1, t1, s1, i1 = grid.match_scan(scans[1], preds[1], half_log_odds=0.25)
    assert np.array_equal(R1, R[1]) and np.array_equal(t1, t[1]) and s1 == score[1]
    assert all(np.array_equal(i1[key], info[key][1]) for key in RECORD_KEYS + MOMENT_KEYS)
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=4, row_capacity=4096)
    hist.add_many(scans)
    got = grid.match_history(hist, [2, 0], [preds[2], preds[0]], half_log_odds=0.25)
    assert np.array_equal(got[0], R[[2, 0]]) and np.array_equal(got[1], t[[2, 0]]) and np.array_equal(got[2], score[[2, 0]])
    assert all(np.array_equal(got[3][key], info[key][[2, 0]]) for key in RECORD_KEYS + MOMENT_KEYS)
