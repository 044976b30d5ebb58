"""The four entries that hold a list of (cloud, pose) pairs against the occupancy grid — the exhaustive match, the wide
search, the check and the beam model (icpmi.gridmatch: GridMatchBatch, GridSearchBatch, check_pairs, beam_pairs) — judge
ONE pair list alike: the same status for every pair, and the same rows with cells wherever a pair is read.  Each family's
own suite compares its records bit for bit against its restatement; this holds the four against each other on one cloud
set with device counts (a short one, the voxel filter's overflow mark, one above its cap), a cloud that crosses a chunk
of 256 rows, a pose that puts its scan off the grid and a pose that is not finite."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPS = (0, 1, 257, 300)                                        # rows of the four clouds; 257 crosses a chunk of 256
COUNTS = (1, -1, 257, 258)                                     # above its cap, the overflow mark, full, short
PAIRS = (2, 3, 0, 1, 2, 3, 2, 3)                               # every cloud is named
NY, NX, RES, MIN_X, MIN_Y, K, THRESHOLD = 64, 96, 0.1, -4.8, -3.2, 10, 1024


@pytest.fixture(scope="module")
def world():
    """(cloud set, field tensor, grid, pair, t, theta, cos_sin): the one pair list every test here reads"""
    import torch
    from icpmi.batch import CloudSet
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    rng = np.random.default_rng(58)
    # rows on a ring of 1 to 3 m about the sensor: none at its origin, where the beam model has no far end
    bearing, r = rng.uniform(-np.pi, np.pi, sum(CAPS)), rng.uniform(1.0, 3.0, sum(CAPS))
    pts = np.stack([r * np.cos(bearing), r * np.sin(bearing)], axis=1)
    off = np.concatenate([[0], np.cumsum(CAPS)]).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    cs = CloudSet(torch.from_numpy(pts).to(dev), off, cnt=torch.tensor(COUNTS, dtype=torch.int32, device=dev))
    # the map: observed free space, one wall, a band nobody has seen
    field = np.full((NY, NX), -512, dtype=np.int16)
    field[:, 70] = 4096
    field[:8] = 0
    fld = torch.from_numpy(field).to(dev)
    grid = types.SimpleNamespace(device_log_odds=torch.zeros((NY, NX), dtype=torch.float32, device=dev), min_x=MIN_X, min_y=MIN_Y,
                                 resolution=RES, log_odds_min=-5.0, log_odds_max=5.0)
    pair = np.array(PAIRS, dtype=np.int32)
    B = len(pair)
    t = rng.uniform(-1.0, 1.0, (B, 2))
    theta = rng.uniform(-np.pi, np.pi, (B, 1))
    t[4] = (1000.0, -1000.0)                                       # the whole scan off the grid: its rows still have cells
    t[5] = (np.nan, 0.0)                                           # no row has a cell
    cos_sin = np.concatenate([np.cos(theta), np.sin(theta)], axis=1)
    return cs, fld, grid, pair, t, theta, cos_sin


def test_the_four_entries_judge_one_pair_list_alike(world):
    from icpmi import _lib, gridmatch
    cs, fld, grid, pair, t, theta, cos_sin = world
    B = len(pair)

    match = gridmatch.GridMatchBatch(grid, cs, pair, t, theta, 0, field=(fld, K))
    search = gridmatch.GridSearchBatch(grid, cs, pair, t, theta, 0, block=4, field=(fld, K))
    checked, _ = gridmatch.check_pairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, pair, t, cos_sin, 2)
    beamed, _, _ = gridmatch.beam_pairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, pair, t, cos_sin, gridmatch.beam_table(RES, RES, 8), 8, 1.5)
    rec = {"match": match.run().cpu().numpy()[:B], "search": search.run().cpu().numpy()[:B], "check": checked.cpu().numpy(),
           "beam": beamed.cpu().numpy()}
    status = {"match": _lib.GMREC_STATUS, "search": _lib.GMREC_STATUS, "check": _lib.GK_REC_STATUS, "beam": _lib.GB_REC_STATUS}
    rows = {"match": _lib.GMREC_ROWS, "check": _lib.GK_REC_ROWS, "beam": _lib.GB_REC_ROWS}

    # what the counts imply: a count that is negative or above the cloud's cap is not read; else any row with a cell decides
    n = np.array([c if 0 <= c <= cap else -1 for c, cap in zip(COUNTS, CAPS)])[pair]
    with_cells = np.where(np.isfinite(t).all(axis=1), n, 0)
    want = np.where(n < 0, _lib.GM_ST_CAPACITY, np.where(with_cells > 0, _lib.GM_ST_OK, _lib.GM_ST_EMPTY))
    assert want.tolist() == [0, 0, 2, 2, 0, 1, 0, 0] == [_lib.GM_ST_OK] * 2 + [_lib.GM_ST_CAPACITY] * 2 + [_lib.GM_ST_OK, _lib.GM_ST_EMPTY] + [_lib.GM_ST_OK] * 2
    for name, slot in status.items():
        print(name, "status", rec[name][:, slot].tolist())
        assert np.array_equal(rec[name][:, slot], want), name
    ok = want == _lib.GM_ST_OK
    for name, slot in rows.items():
        print(name, "rows with cells", rec[name][:, slot].tolist())
        assert np.array_equal(rec[name][ok, slot], rec["match"][ok, rows["match"]]), name
    assert np.array_equal(rec["match"][ok, rows["match"]], with_cells[ok])


SENTINEL, H, BEYOND, TOLERANCE = -7, 8, 1.5, 2
ROWS_READ = [c if 0 <= c <= cap else 0 for c, cap in zip(COUNTS, CAPS)]       # a refused count reads nothing


def sentinels(*shapes):
    import torch
    return tuple(torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda") for shape in shapes)


def host(tensors):
    return [None if x is None else x.cpu().numpy() for x in tensors]


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_one_prepared_call_run_twice_gives_check_pairs_and_beam_pairs(world):
    """MapPairs: checked and uploaded once, then the check and the beam model twice each into buffers full of a sentinel —
    the records, histograms and rows of check_pairs and beam_pairs (into sentinel buffers of their own), byte for byte, and
    what lies at or behind a cloud's count untouched.  Pointed at other poses it gives beam_pairs' records for those, and the
    first records again when pointed back."""
    from icpmi import _lib, gridmatch
    cs, fld, _, pair, t, _, cos_sin = world
    B, stride, table = len(pair), max(CAPS), gridmatch.beam_table(RES, RES, H)
    map_args = (fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, pair)
    shapes_k = ((B, _lib.GK_INTS), (B, stride, _lib.GK_ROW_INTS))
    shapes_b = ((B, _lib.GB_INTS), (B, 2 * H + 3), (B, stride, _lib.GB_ROW_INTS))
    want_k = host(gridmatch.check_pairs(*map_args, t, cos_sin, TOLERANCE, want_rows=True, out=sentinels(*shapes_k)))
    want_b = host(gridmatch.beam_pairs(*map_args, t, cos_sin, table, H, BEYOND, want_hist=True, want_rows=True, out=sentinels(*shapes_b)))

    mp = gridmatch.MapPairs(*map_args, on_device(t), on_device(cos_sin))
    assert (mp.B, mp.stride) == (B, stride)
    table_dev = on_device(table)
    for _ in range(2):
        out_k, out_b = sentinels(*shapes_k), sentinels(*shapes_b)
        got_k = mp.check(TOLERANCE, want_rows=True, out=out_k)
        got_b = mp.beam(table_dev, H, BEYOND, want_hist=True, want_rows=True, out=out_b)
        assert all(g is o for g, o in zip(got_k + got_b, out_k + out_b))           # written where the caller said
        for got, want in zip(host(got_k) + host(got_b), want_k + want_b):
            assert np.array_equal(got, want)
        for rows in (got_k[1].cpu().numpy(), got_b[2].cpu().numpy()):
            for b, c in enumerate(pair):
                assert (rows[b, ROWS_READ[c]:] == SENTINEL).all(), b
    assert mp.beam(table_dev, H, BEYOND)[1:] == (None, None) and mp.check(TOLERANCE)[1] is None

    # other poses: a half turn and a shift, the off-grid and the NaN pose kept
    rng = np.random.default_rng(59)
    t2 = t + rng.uniform(-0.5, 0.5, t.shape)
    cos_sin2 = -cos_sin
    want2 = gridmatch.beam_pairs(*map_args, t2, cos_sin2, table, H, BEYOND)[0].cpu().numpy()
    assert not np.array_equal(want2, want_b[0])
    pairs_dev = mp.pairs.dev
    assert np.array_equal(mp.point_at(on_device(t2), on_device(cos_sin2)).beam(table_dev, H, BEYOND)[0].cpu().numpy(), want2)
    assert np.array_equal(mp.point_at(on_device(t), on_device(cos_sin)).beam(table_dev, H, BEYOND)[0].cpu().numpy(), want_b[0])
    assert mp.pairs.dev is pairs_dev


def test_a_kept_pair_list_serves_every_fresh_one_cloud_set(world):
    """The filter's pattern: B = 8 pairs that all name cloud 0, the GridPairs made once, a fresh one-cloud set per scan —
    beam_pairs' records for that scan."""
    import torch
    from icpmi import _lib, gridmatch
    _, fld, _, pair, t, _, cos_sin = world
    B, table = len(pair), gridmatch.beam_table(RES, RES, H)
    zeros = gridmatch.GridPairs(np.zeros(B, dtype=np.int32), fld.device)
    kept = zeros.dev
    rng = np.random.default_rng(60)
    t_dev, rot_dev = on_device(t), on_device(cos_sin)
    for rows in (257, 40):
        bearing, r = rng.uniform(-np.pi, np.pi, rows), rng.uniform(1.0, 3.0, rows)
        scan = np.stack([r * np.cos(bearing), r * np.sin(bearing)], axis=1)
        want = gridmatch.beam_pairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, gridmatch.cloud_set_of([scan]), np.zeros(B, dtype=np.int32), t, cos_sin,
                                    table, H, BEYOND)[0].cpu().numpy()
        mp = gridmatch.MapPairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, gridmatch.cloud_set_of([scan]), zeros, t_dev, rot_dev)
        assert mp.pairs is zeros and zeros.dev is kept and mp.stride == rows and mp.t is t_dev and mp.rot is rot_dev
        assert np.array_equal(mp.beam(table, H, BEYOND)[0].cpu().numpy(), want)
        assert want[:, _lib.GB_REC_ROWS].max() == rows             # (the scan was read: rows with cells)
    torch.cuda.synchronize()


def test_the_filter_weighs_both_generations_through_the_prepared_call():
    """One ParticleFilter step at N = 300 (more than one block of 256): predict, weigh, resample, weigh.  After each weigh the
    filter's records are beam_pairs' at the particles read back — the second time those of the swapped generation."""
    from icpmi import gridmatch, synth
    from utilities.mapping import OccupancyGrid2D
    import gridmatch_ref as gref
    grid = OccupancyGrid2D(**gref.SCENE)
    for k, p in enumerate(gref.SCENE_POSES[:4]):
        grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 50 + k), p))
    N, pose = 300, gref.SCENE_POSES[1]
    scan = synth.scan(pose, 51)[::32]
    pf = grid.particle_filter(N, seed=77, half_width=H)
    pf.init_gaussian(pose, (0.2, 0.2, 0.05)).predict((0.02, 0.0, 0.005), (0.01, 0.01, 0.002))

    def weigh_and_compare():
        t, rot = pf.pair_t.cpu().numpy(), pf.cos_sin.cpu().numpy()
        ess, ok = pf.weigh(scan)
        want = gridmatch.beam_pairs(pf.planes, None, grid.min_x, grid.min_y, grid.resolution, gridmatch.cloud_set_of([scan]),
                                    np.zeros(N, dtype=np.int32), t, rot, pf.beam_table_host, H, pf.beyond)[0].cpu().numpy()
        assert np.array_equal(pf.records.cpu().numpy(), want) and ok == N and ess > 0.0
        return t

    first = weigh_and_compare()
    state = pf.pair_t
    pf.resample()
    assert pf.pair_t is not state and not pf.degenerate()          # the generations were swapped
    second = weigh_and_compare()
    assert np.array_equal(second, first[pf.ancestors.cpu().numpy()]) and not np.array_equal(second, first)
