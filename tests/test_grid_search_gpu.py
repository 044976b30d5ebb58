"""The wide-window scan-to-map search on the device (csrc/gridmatch_wide.hip; icpmi.gridmatch.bound_field, GridSearchBatch; the
search methods of utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract
(tests/gridmatch_wide_ref.py).  Every quantity is an integer, so everything is compared with array_equal: the bound field, the
blocks' bounds (through want_bounds), all twelve slots of the records, and the poses the host layer forms from them.

Two grids at 0.25 m, 37 x 53 and 203 x 131 cells — no edge a multiple of 4, 8 or 16 — hold random int16 with runs of -32767
and 32767; the fields are handed in as they are (field=), so the grid stand-in only gives the geometry."""
import types

import numpy as np
import pytest

import gridmatch_ref as ref
import gridmatch_wide_ref as wide

pytestmark = pytest.mark.gpu

RES = 0.25
CHUNK = 256


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert _lib.GM_CHUNK_ROWS == CHUNK


def geometry(shape):
    """The grid centred on the origin: (min_x, min_y, resolution)."""
    return -shape[1] * RES / 2, -shape[0] * RES / 2, RES


def random_field(seed, shape):
    rng = np.random.default_rng(seed)
    q = rng.integers(-20000, 20001, size=shape).astype(np.int16)
    q[rng.uniform(size=shape) < 0.7] = -250                                         # mostly free space, some walls
    q[3, 5:25] = 32767
    q[10, :30] = -32767
    q[-1, -9:] = 32767
    q[:9, -1] = -32767
    q[0, 0] = q[-1, 0] = 32767
    return q


def stand_in(q):
    """(what GridSearchBatch reads of a grid, the field= to hand in): the int16 array as the field itself, k = 0."""
    import torch
    min_x, min_y, res = geometry(q.shape)
    grid = types.SimpleNamespace(device_log_odds=torch.zeros(q.shape, dtype=torch.float32, device="cuda"), min_x=min_x, min_y=min_y,
                                 resolution=res, log_odds_min=-5.0, log_odds_max=5.0)
    return grid, (torch.from_numpy(np.ascontiguousarray(q)).cuda(), 0)


@pytest.fixture(scope="module")
def small(gpu):
    q = random_field(11, (37, 53))
    return (q,) + stand_in(q)


@pytest.fixture(scope="module")
def big(gpu):
    q = random_field(12, (203, 131))
    return (q,) + stand_in(q)


def run_device(grid, field, clouds, pair_clouds, translations, angles, W, centre, D, cnt=None, bounds=None):
    """One chain of launches -> (U [B, A, NB, NB], records [B, 12]) on the host, and the job."""
    import torch
    from icpmi.batch import CloudSet
    from icpmi.gridmatch import GridSearchBatch
    cs = CloudSet.from_numpy(clouds)
    if cnt is not None:
        cs.cnt = torch.tensor(cnt, dtype=torch.int32, device=cs.pts.device)
    job = GridSearchBatch(grid, cs, pair_clouds, translations, angles, W, centre, block=D, field=field, bounds=bounds, want_bounds=True)
    rec = job.run()
    torch.cuda.synchronize()
    return job.bounds_volume.cpu().numpy()[:len(pair_clouds)], rec.cpu().numpy()[:len(pair_clouds)], job


def run_ref(q, clouds, pair_clouds, translations, angles, W, centre, D, M=None):
    M = wide.bound_field(q, D) if M is None else M
    out = [wide.search(q, D, clouds[c], translations[b], ref.cos_sin_of(np.asarray(angles, dtype=np.float64)[b]), W, centre,
                       *geometry(q.shape), M=M) for b, c in enumerate(pair_clouds)]
    return np.stack([u for _, u in out]), np.stack([r for r, _ in out])


def check(case, q, grid, field, clouds, pair, t, angles, W, centre, D):
    U, rec, job = run_device(grid, field, clouds, pair, t, angles, W, centre, D)
    want_U, want_rec = run_ref(q, clouds, pair, t, angles, W, centre, D)
    NB = -(-(2 * W + 1) // D)
    assert U.dtype == np.int32 and U.shape == (len(pair), np.shape(angles)[1], NB, NB), case
    assert np.array_equal(U, want_U), case
    assert np.array_equal(rec, want_rec), (case, rec, want_rec)
    return U, rec, job


def disc(rng, n, radius):
    r, a = radius * np.sqrt(rng.uniform(size=n)), rng.uniform(-np.pi, np.pi, size=n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


# ── 1. the bound field ───────────────────────────────────────────────────────
def test_bound_field_equals_the_restatement(small, big):
    import torch
    from icpmi import gridmatch
    rng = np.random.default_rng(3)
    shapes = [(1, 1), (1, 9), (7, 5), (3, 129), (33, 128), (40, 257)]               # below, at and across a tile of 32 x 128
    fields = [small[0], big[0]] + [rng.integers(-32767, 32768, size=s).astype(np.int16) for s in shapes]
    for q in fields:
        for D in wide.BLOCKS:
            got = gridmatch.bound_field(torch.from_numpy(q).cuda(), D)
            assert got.dtype == torch.int16 and tuple(got.shape) == (q.shape[0] + D - 1, q.shape[1] + D - 1)
            assert np.array_equal(got.cpu().numpy(), wide.bound_field(q, D)), (q.shape, D)


# ── 2. windows and blocks ────────────────────────────────────────────────────
@pytest.mark.parametrize("W,D", [(W, D) for W in (0, 1, 5, 31, 32, 63) for D in wide.BLOCKS])
def test_records_and_bounds_equal_the_restatement(small, W, D):
    """S not a multiple of D, a single block (W = 0, 1; W = 5 at D = 16), W = 32: the first window the exhaustive entry refuses.
    For W <= 31 the first eight slots are also those of GridMatchBatch on the same inputs, device against device."""
    q, grid, field = small
    rng = np.random.default_rng(100 * W + D)
    clouds = [disc(rng, 300, 4.0)]
    t = rng.uniform(-1.0, 1.0, size=(1, 2))
    angles = rng.uniform(-np.pi, np.pi, size=(1, 2))
    _, rec, _ = check((W, D), q, grid, field, clouds, [0], t, angles, W, 1, D)
    assert rec[0, 0] == ref.ST_OK and rec[0, 1] == 300
    from icpmi.batch import CloudSet
    from icpmi.gridmatch import GridMatchBatch
    if W <= 31:
        old = GridMatchBatch(grid, CloudSet.from_numpy(clouds), [0], t, angles, W, 1, field=field).run().cpu().numpy()
        assert np.array_equal(rec[:, :8], old[:1])
    else:
        with pytest.raises(ValueError, match="window must lie in"):
            GridMatchBatch(grid, CloudSet.from_numpy(clouds), [0], t, angles, W, 1, field=field)


def test_the_widest_window(big):
    q, grid, field = big
    rng = np.random.default_rng(7)
    clouds = [disc(rng, 40, 10.0)]
    for D in (16, 4):                                                               # NB = 32 and 128: 1 024 and 16 384 blocks per angle
        _, rec, _ = check(D, q, grid, field, clouds, [0], [[1.0, -2.0]], [[0.3, -2.0]], 255, 0, D)
        assert rec[0, 8] == 2 * (-(-511 // D)) ** 2


@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 600])
def test_clouds_of_one_and_several_chunks(big, n):
    q, grid, field = big
    rng = np.random.default_rng(n)
    clouds = [disc(rng, n, 12.0)]
    t, angles = rng.uniform(-3.0, 3.0, size=(1, 2)), rng.uniform(-np.pi, np.pi, size=(1, 3))
    for W, D in ((9, 8), (20, 4), (40, 16)):                                        # NB^2 = 9, 121 and 36; D = 4: more than 64 blocks
        _, rec, _ = check((n, W, D), q, grid, field, clouds, [0], t, angles, W, 2, D)
        assert rec[0, 1] == n


# ── 3. edges ─────────────────────────────────────────────────────────────────
def test_negative_cells_read_the_negative_part_of_the_bound_field(small):
    """A cloud centred on the grid's lower left corner: half its cells have a negative index on at least one axis, so
    M(y, x) is read at negative y and x; clouds wholly outside; rows with NaN, inf and cells beyond 2^29."""
    q, grid, field = small
    rng = np.random.default_rng(5)
    min_x, min_y, _ = geometry(q.shape)
    corner = disc(rng, 400, 2.0) + (min_x, min_y)
    bad = np.vstack([disc(rng, 40, 2.0), [[np.nan, 0.0], [0.0, np.inf], [1e12, 0.0], [1e300, 1e300], [2.0 ** 29 * RES, 0.0]], disc(rng, 30, 2.0)])
    clouds = [corner, bad]
    cx, cy = ref.cells(corner, 1.0, 0.0, 0.0, 0.0, *geometry(q.shape))
    assert 150 < int(((cx < 0) | (cy < 0)).sum()) < 350
    cases = [(0, (0.0, 0.0)), (0, (-1.0, -0.5)), (0, (-3.0, -3.0)), (0, (13.2, 9.2)), (0, (100.0, -100.0)), (1, (0.0, 0.0)), (1, (-6.0, 4.0))]
    pair, t = [c for c, _ in cases], np.array([tt for _, tt in cases])
    angles = np.zeros((len(cases), 2))
    angles[:, 1] = rng.uniform(-np.pi, np.pi, size=len(cases))
    for W, D in ((6, 4), (13, 8), (17, 16)):
        U, rec, _ = check((W, D), q, grid, field, clouds, pair, t, angles, W, 0, D)
        assert U[0].any() and U[2].any() and not U[4].any()
        assert list(rec[4, :8]) == [ref.ST_OK, 400, 0, 0, 0, 0, 0, 0] and rec[4, 9] == rec[4, 8]   # wholly outside: all scores 0


def test_an_all_zero_field_keeps_every_block(gpu):
    q = np.zeros((37, 53), dtype=np.int16)
    grid, field = stand_in(q)
    rng = np.random.default_rng(8)
    for W, D in ((6, 4), (40, 8), (40, 16)):
        A, NB = 3, -(-(2 * W + 1) // D)
        U, rec, _ = check((W, D), q, grid, field, [disc(rng, 500, 4.0)], [0], [[0.3, -0.2]], rng.uniform(-1, 1, size=(1, A)), W, 1, D)
        assert not U.any() and list(rec[0]) == [ref.ST_OK, 500, 0, 0, 0, 0, 0, 0, A * NB * NB, A * NB * NB, 0, 0]


def test_an_all_negative_field_pushes_rows_off_the_map(gpu):
    """Every cell costs, so the winner moves as many rows as it can off the map, where a cell counts 0 — in M too: a block
    that can push a row out has bound 0 for it, not the -77 of the cells inside."""
    q = np.full((37, 53), -77, dtype=np.int16)
    q[5:9, 7:30] = -32767
    grid, field = stand_in(q)
    rng = np.random.default_rng(9)
    clouds = [disc(rng, 200, 3.0)]
    for W, D in ((10, 4), (25, 8), (31, 16)):
        U, rec, _ = check((W, D), q, grid, field, clouds, [0], [[4.0, 2.5]], [[0.0, 2.0]], W, 0, D)
        vol, _ = wide.volume(q, clouds[0], (4.0, 2.5), ref.cos_sin_of(np.array([0.0, 2.0])), W, *geometry(q.shape))
        assert rec[0, 6] == vol.max() > rec[0, 7] and rec[0, 7] < -77 * 150 and U.max() <= 0


# ── 4. ties ──────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("on_the_edge", [False, True])
def test_plateaus_go_to_the_lowest_flat_index(gpu, on_the_edge):
    """The plateaus of tests/test_grid_search_cpu.py's counter-check: every candidate ties (index 0, every block survives), and
    the edge plateau whose first maximum lies in a block whose bound EQUALS the seed score — found only with >=."""
    q, pts, t, cs, W, D, g = wide.plateau(on_the_edge)
    import torch
    grid = types.SimpleNamespace(device_log_odds=torch.zeros(q.shape, dtype=torch.float32, device="cuda"), min_x=g["min_x"], min_y=g["min_y"],
                                 resolution=g["res"], log_odds_min=-5.0, log_odds_max=5.0)
    field = (torch.from_numpy(q).cuda(), 0)
    U, rec, _ = run_device(grid, field, [pts], [0], [t], [[0.0]], W, 0, D)
    want_rec, want_U = wide.search(q, D, pts, t, cs, W, 0, **g)
    vol, rows = wide.volume(q, pts, t, cs, W, **g)
    assert np.array_equal(U[0], want_U) and np.array_equal(rec[0], want_rec) and np.array_equal(rec[0, :8], ref.record(vol, rows, 0, W))
    if on_the_edge:
        later, _ = wide.search(q, D, pts, t, cs, W, 0, keep=np.greater, **g)
        assert rec[0, 2] == D < later[2] and rec[0, 6] == later[6] == rec[0, 10] == 180
    else:
        assert list(rec[0]) == [0, 40, 0, 0, 0, 0, 360, 360, 9, 9, 360, 360]


def test_two_equal_peaks_in_different_blocks(gpu):
    q = np.zeros((40, 30), dtype=np.int16)
    q[12, 9] = q[20, 22] = 500
    import torch
    grid = types.SimpleNamespace(device_log_odds=torch.zeros(q.shape, dtype=torch.float32, device="cuda"), min_x=0.0, min_y=0.0, resolution=1.0,
                                 log_odds_min=-5.0, log_odds_max=5.0)
    field = (torch.from_numpy(q).cuda(), 0)
    pts = np.array([[10.5, 15.5]])
    for D in wide.BLOCKS:
        U, rec, _ = run_device(grid, field, [pts], [0], [[0.0, 0.0]], [[0.0]], 13, 0, D)
        want_rec, want_U = wide.search(q, D, pts, (0.0, 0.0), np.array([[1.0, 0.0]]), 13, 0, 0.0, 0.0, 1.0)
        assert np.array_equal(U[0], want_U) and np.array_equal(rec[0], want_rec)
        assert tuple(rec[0, 2:7]) == (10 * 27 + 12, 0, 10, 12, 500) and rec[0, 9] == 2 and rec[0, 7] == 0
    # and at two angles: a quarter turn puts the point into another cell; the earlier angle wins whichever peak it reaches
    for angles in ([[np.pi / 2, 0.0]], [[0.0, np.pi / 2]]):
        U, rec, _ = run_device(grid, field, [pts], [0], [[20.0, 3.0]], angles, 13, -1, 8)
        want_rec, _ = wide.search(q, 8, pts, (20.0, 3.0), ref.cos_sin_of(np.array(angles[0])), 13, -1, 0.0, 0.0, 1.0)
        assert np.array_equal(rec[0], want_rec) and rec[0, 3] == 0 and rec[0, 6] == 500


# ── 5. statuses and batches ──────────────────────────────────────────────────
def test_empty_and_capacity_clouds_beside_ordinary_ones(small):
    from icpmi import _lib
    q, grid, field = small
    rng = np.random.default_rng(6)
    clouds = [disc(rng, 50, 3.0), disc(rng, 60, 3.0), disc(rng, 70, 3.0), np.zeros((0, 2)), np.array([[np.nan, 0.0], [1e12, 1e12]])]
    W, D, A = 9, 4, 2
    NB = 5
    angles = rng.uniform(-1.0, 1.0, size=(6, A))
    U, rec, _ = run_device(grid, field, clouds, [0, 1, 2, 3, 4, 1], np.zeros((6, 2)), angles, W, 0, D, cnt=[-1, 40, 71, 0, 2])
    want_U, want_rec = run_ref(q, [clouds[1][:40]], [0, 0], np.zeros((2, 2)), angles[[1, 5]], W, 0, D)
    assert np.array_equal(U[[1, 5]], want_U) and np.array_equal(rec[[1, 5]], want_rec)           # a device count below the capacity
    for b, status in ((0, _lib.GM_ST_CAPACITY), (2, _lib.GM_ST_CAPACITY), (3, _lib.GM_ST_EMPTY), (4, _lib.GM_ST_EMPTY)):
        assert not U[b].any() and list(rec[b]) == [status, 0, 0, 0, 0, 0, 0, 0, A * NB * NB, A * NB * NB, 0, 0], b


def test_a_batch_equals_its_pairs_alone_a_second_run_and_bounds_handed_back(small):
    import torch
    from icpmi import gridmatch
    q, grid, field = small
    rng = np.random.default_rng(21)
    B, W, D, A = 70, 10, 8, 2
    sizes = rng.integers(1, 600, size=B)
    sizes[:4] = (1, CHUNK, CHUNK + 1, 599)
    clouds = [disc(rng, int(n), rng.uniform(1.0, 5.0)) for n in sizes]
    t = rng.uniform(-4.0, 4.0, size=(B, 2))
    angles = rng.uniform(-np.pi, np.pi, size=(B, A))
    pair = rng.permutation(B)
    U, rec, job = run_device(grid, field, clouds, pair, t, angles, W, 1, D)
    for b in range(B):                                             # 70 chains, each over its own cloud set: max_n and the grids differ
        U1, r1, _ = run_device(grid, field, [clouds[pair[b]]], [0], t[b:b + 1], angles[b:b + 1], W, 1, D)
        assert np.array_equal(U1[0], U[b]) and np.array_equal(r1[0], rec[b]), b
    want_U, want_rec = run_ref(q, clouds, pair, t, angles, W, 1, D)
    assert np.array_equal(U, want_U) and np.array_equal(rec, want_rec)
    rec2 = job.run()                                               # the same workspace again: zeroed per call, nothing accumulates
    torch.cuda.synchronize()
    assert np.array_equal(job.bounds_volume.cpu().numpy(), U) and np.array_equal(rec2.cpu().numpy(), rec)
    kept = gridmatch.bound_field(field[0], D)                      # bounds= handed back: the records of rebuilding
    assert np.array_equal(kept.cpu().numpy(), wide.bound_field(q, D))
    U3, rec3, job3 = run_device(grid, field, clouds, pair, t, angles, W, 1, D, bounds=kept)
    assert job3._bound_buf is None and np.array_equal(U3, U) and np.array_equal(rec3, rec)
    from icpmi.batch import CloudSet
    plain = gridmatch.GridSearchBatch(grid, CloudSet.from_numpy(clouds), pair, t, angles, W, 1, block=D, field=field)
    assert plain.bounds_volume is None                             # without the bounds handed out they live in the workspace
    for _ in range(2):
        assert np.array_equal(plain.run().cpu().numpy(), rec)
    R, tt, score, info = plain.unpack()
    assert all(np.array_equal(info[key], rec[:, s]) for key, s in (("blocks", 8), ("survivors", 9), ("seed_score", 10), ("max_bound", 11)))
    assert np.array_equal(score, rec[:, 6]) and np.array_equal(info["index"], rec[:, 2])


def test_refusals_on_the_host(small):
    import torch
    from icpmi import gridmatch
    from icpmi.batch import CloudSet
    q, grid, field = small
    cs = CloudSet.from_numpy([np.zeros((5, 2))])
    make = lambda **kw: gridmatch.GridSearchBatch(grid, kw.pop("cs", cs), [0], [[0.0, 0.0]], kw.pop("angles", [[0.0]]), kw.pop("W", 3), **kw)  # noqa: E731
    make(), make(W=255, block=16)                                                   # what passes
    for kw, what in ((dict(W=256), "window must lie in"), (dict(W=-1), "window must lie in"),
                     (dict(angles=np.zeros((1, 16385))), "angles per pair"), (dict(angles=np.zeros((1, 8225)), W=255), "do not fit an int32"),
                     (dict(block=5), "block must be one of"), (dict(block=0), "block must be one of"), (dict(centre_angle=1), "centre_angle"),
                     (dict(cs=CloudSet.from_numpy([np.zeros((65536, 2))])), "rows cannot be scored"),
                     (dict(bounds=torch.zeros((37 + 7, 53 + 6), dtype=torch.int16, device="cuda")), "bounds must be the int16"),
                     (dict(bounds=torch.zeros((37 + 3, 53 + 3), dtype=torch.int16, device="cuda")), "bounds must be the int16"),
                     (dict(bounds=torch.zeros((37 + 7, 53 + 7), dtype=torch.int32, device="cuda")), "bounds must be the int16")):
        with pytest.raises(ValueError, match=what):
            make(**kw)
    with pytest.raises(ValueError, match="block must be one of"):
        gridmatch.bound_field(field[0], 12)
    with pytest.raises(ValueError, match="contiguous int16"):
        gridmatch.bound_field(field[0].float(), 8)


# ── 6. the Python layer ──────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def room(gpu):
    """(grid built by update_scans on the device, its field by the restatement, its bound field for D = 8)."""
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**ref.SCENE)
    origins, hits = ref.scene_scans()
    grid.update_scans(origins, hits)
    q = ref.quantise(grid.log_odds, ref.shift_bits(grid.log_odds_min, grid.log_odds_max))
    return grid, q, wide.bound_field(q, 8)


def test_search_scan_returns_the_restatements_pose(room):
    """The relocalisation queries of tests/test_grid_search_cpu.py: 3 m per axis and 40 degrees off, a 4 m window, +-45 degrees."""
    grid, q, M = room
    cfg = wide.RELOC
    assert np.array_equal(grid.bound_field(block=8).cpu().numpy(), M)
    field = grid.score_field()
    kept = grid.bound_field(field, 8)
    for n, (true, pred, scan) in enumerate(wide.reloc_queries()[:3]):
        angles = ref.angle_rows(pred[2], cfg["angular_window"], cfg["angular_step"])
        cs = ref.cos_sin_of(angles)
        rec, _ = wide.search(q, 8, scan, pred[:2], cs, cfg["W"], 45, grid.min_x, grid.min_y, grid.resolution, M=M)
        want_R, want_t = ref.pose(rec, pred[:2], cs, cfg["W"], grid.resolution)
        kw = dict(field=field, bounds=kept) if n == 1 else {}
        R, t, score, info = grid.search_scan(scan, pred, linear_window=4.0, angular_window=45.0, angular_step=1.0, **kw)
        assert np.array_equal(R, want_R) and np.array_equal(t, want_t) and score == rec[6]
        assert [info[key] for key in ("status", "rows", "index", "a", "j", "i", "centre_score", "blocks", "survivors", "seed_score",
                                      "max_bound")] == [rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[7], rec[8], rec[9], rec[10], rec[11]]
        assert np.abs(t - np.array(true[:2])).max() <= 0.1 + 1e-9 and abs(np.rad2deg(info["angle"] - true[2])) <= 1.0 + 1e-9
    with pytest.raises(ValueError, match="pass that field"):
        grid.search_scan(scan, pred, bounds=kept)


def test_search_scans_and_search_history_equal_search_scan(room):
    from icpmi import ScanHistory
    grid, q, M = room
    queries = wide.reloc_queries()[:3]
    scans, preds = [s for _, _, s in queries], [p for _, p, _ in queries]
    kw = dict(linear_window=2.0, angular_window=20.0, angular_step=2.0, block=16)
    R, t, score, info = grid.search_scans(scans, preds, **kw)
    for b in range(3):
        R1, t1, s1, i1 = grid.search_scan(scans[b], preds[b], **kw)
        assert np.array_equal(R[b], R1) and np.array_equal(t[b], t1) and score[b] == s1
        assert all(info[key][b] == i1[key] for key in ("status", "rows", "index", "a", "j", "i", "centre_score", "survivors", "seed_score"))
        old = grid.match_scan(scans[b], preds[b], linear_window=2.0, angular_window=20.0, angular_step=2.0)    # W = 20: both entries
        assert np.array_equal(old[0], R1) and np.array_equal(old[1], t1) and old[2] == s1 and old[3]["index"] == i1["index"]
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=4, row_capacity=2048)
    hist.add_many(scans)
    got = grid.search_history(hist, [2, 0], [preds[2], preds[0]], **kw)
    want = grid.search_scans([scans[2], scans[0]], [preds[2], preds[0]], **kw)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert all(np.array_equal(got[3][key], want[3][key]) for key in want[3])
