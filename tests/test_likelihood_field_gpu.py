"""The likelihood field on the device (csrc/gridfield.hip; icpmi.gridmatch.distance_field, likelihood_field; the methods of
utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract (tests/likelihood_ref.py).  Everything is an
integer, so both outputs are compared with array_equal: at grids smaller than a halo, at the seams of the kernel's tiles of
LF_TILE_Y x LF_TILE_X outputs with occupied cells exactly R and R + 1 cells away, with nothing and with everything occupied,
on a sparse field whose nearest cells lie across seams, at thresholds the field holds and with a table of negative entries.
The room map of tests/test_likelihood_field_cpu.py then goes through OccupancyGrid2D.likelihood_field into the existing
matchers as field=, whose records must be those of the restatements of those matchers on the restated field."""
import functools

import numpy as np
import pytest

import gridmatch_ref as gref
import gridmatch_wide_ref as wide
import likelihood_ref as ref

pytestmark = pytest.mark.gpu

TILE_Y, TILE_X = 64, 128
CASES = ref.cases(TILE_Y, TILE_X)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert (_lib.LF_TILE_Y, _lib.LF_TILE_X, _lib.LF_MAX_RADIUS) == (TILE_Y, TILE_X, ref.MAX_RADIUS)


@functools.lru_cache(maxsize=None)
def restated(n):
    _, q, threshold, R, table, keep_free = CASES[n]
    d2, lf = ref.likelihood_field(q, threshold, R, table, keep_free)
    d2.setflags(write=False)
    lf.setflags(write=False)
    return d2, lf


def on_device(q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q)).cuda()


@pytest.mark.parametrize("n", range(len(CASES)), ids=[c[0] for c in CASES])
def test_both_fields_equal_the_restatement(gpu, n):
    import torch
    from icpmi import gridmatch
    name, q, threshold, R, table, keep_free = CASES[n]
    want_d2, want_lf = restated(n)
    if name.startswith("nothing"):
        assert (want_d2 == R * R + 1).all() and np.array_equal(want_lf, np.minimum(q, 0) if keep_free else np.zeros_like(q))
    if name.startswith("everything"):
        assert not want_d2.any() and (want_lf == table[0]).all()
    if name.startswith("sparse"):
        assert (want_d2 <= R * R).mean() > 0.9                     # nearly every cell has a neighbour, most across a seam
    qd = on_device(q)
    d2 = torch.full(q.shape, 21845, dtype=torch.int16, device="cuda")
    lf = gridmatch.likelihood_field(qd, threshold, R, table, keep_free, d2_out=d2)
    got_d2, got_lf = d2.cpu().numpy(), lf.cpu().numpy()
    print(name, "cells that differ: d2", int((got_d2 != want_d2).sum()), "lf", int((got_lf != want_lf).sum()))
    assert np.array_equal(got_d2, want_d2) and np.array_equal(got_lf, want_lf)
    assert np.array_equal(qd.cpu().numpy(), q)                     # the input is left as it was


def test_each_output_alone_and_a_second_run_write_the_same_bytes(gpu):
    import torch
    from icpmi import gridmatch
    for n, case in enumerate(CASES):
        name, q, threshold, R, table, keep_free = case
        if not (name.startswith("sparse random, free kept") or name == "tile edges R=64"):
            continue
        want_d2, want_lf = restated(n)
        qd = on_device(q)
        alone_d2 = gridmatch.distance_field(qd, threshold, R)
        alone_lf = gridmatch.likelihood_field(qd, threshold, R, table, keep_free)
        for run in range(2):
            d2 = torch.full(q.shape, -3, dtype=torch.int16, device="cuda")
            lf = torch.full(q.shape, -3, dtype=torch.int16, device="cuda")
            assert gridmatch.likelihood_field(qd, threshold, R, table, keep_free, out=lf, d2_out=d2) is lf
            assert torch.equal(d2, alone_d2) and torch.equal(lf, alone_lf), (name, run)
        assert np.array_equal(alone_d2.cpu().numpy(), want_d2) and np.array_equal(alone_lf.cpu().numpy(), want_lf)


def test_python_layer_refuses_what_the_entry_would(gpu):
    import torch
    from icpmi import gridmatch
    qd = on_device(np.zeros((8, 8), dtype=np.int16))
    tab = ref.table(100.0, 1.0, 2)
    for bad in (dict(radius=65), dict(radius=-1), dict(table=tab[:-1]), dict(table=tab.astype(np.int32)),
                dict(table=np.where(np.arange(5) == 3, -32768, tab).astype(np.int16)), dict(out=torch.zeros((8, 9), dtype=torch.int16, device="cuda"))):
        kw = dict(radius=2, table=tab)
        kw.update(bad)
        with pytest.raises(ValueError):
            gridmatch.likelihood_field(qd, 1, kw.pop("radius"), kw.pop("table"), **kw)
    with pytest.raises(ValueError):
        gridmatch.distance_field(qd.to(torch.int32), 1, 2)


# ── the room map through the Python layer into the existing matchers ─────────
@pytest.fixture(scope="module")
def room(gpu):
    """(grid of the scene's first scan at 0.05 m built on the device, its raw field restated, the likelihood field restated)."""
    from utilities.mapping import OccupancyGrid2D
    s = ref.SCENE
    grid = OccupancyGrid2D(**dict(gref.SCENE, resolution=s["resolution"]))
    origins, hits = gref.scene_scans()
    grid.update_scans(origins[:1], hits[:1])
    assert (grid.ny, grid.nx) == (400, 560)
    k = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    q = gref.quantise(grid.log_odds, k)
    tab = ref.table(np.rint(grid.log_odds_max * 2.0 ** k), s["sigma_cells"], s["radius"])
    d2, lf = ref.likelihood_field(q, int(np.rint(s["occupied_log_odds"] * 2.0 ** k)), s["radius"], tab, True)
    return grid, k, q, d2, lf


def room_fields(grid):
    s = ref.SCENE
    metres = dict(sigma=0.1, radius=0.3)                           # in metres; 6 * 0.05 is 0.30000000000000004, whose ceil is 7 cells
    assert metres["sigma"] / grid.resolution == s["sigma_cells"] and int(np.ceil(metres["radius"] / grid.resolution)) == s["radius"]
    return grid.likelihood_field(**metres), metres


def test_room_map_fields_equal_the_restatement(room):
    grid, k, q, d2, lf = room
    (field, got_k), metres = room_fields(grid)
    assert got_k == k == 12 and np.array_equal(field.cpu().numpy(), lf)
    assert np.array_equal(grid.distance_field(metres["radius"]).cpu().numpy(), d2)
    raw = grid.score_field()
    again, _ = grid.likelihood_field(field=raw, **metres)          # from a raw field kept by the caller
    assert np.array_equal(again.cpu().numpy(), lf)
    dropped, _ = grid.likelihood_field(keep_free=False, **metres)
    assert np.array_equal(dropped.cpu().numpy(), np.where(d2 <= 36, lf, 0))
    assert (lf[d2 > 36] <= 0).all() and (lf[d2 > 36] < 0).any() and lf.max() == 20480
    one_cell, _ = grid.likelihood_field()                          # the defaults: sigma one cell, radius 3 sigma
    R = int(np.ceil(3.0 * grid.resolution / grid.resolution))
    tab = ref.table(20480.0, 1.0, R)
    assert np.array_equal(one_cell.cpu().numpy(), ref.likelihood_field(q, 2048, R, tab, True)[1])
    with pytest.raises(ValueError, match="cells"):
        grid.likelihood_field(sigma=0.1, radius=64.5 * grid.resolution)
    with pytest.raises(ValueError, match="cells"):
        grid.distance_field(3.3)


def test_existing_matchers_take_the_likelihood_field_unchanged(room):
    """match_scans and search_scans (block 8) with field= the device's likelihood field: every record is, bit for bit, the
    restatement's of those matchers on the restated field, and the poses are within one cell and one step of the truth."""
    grid, k, q, d2, lf = room
    s = ref.SCENE
    field, _ = room_fields(grid)
    queries = ref.scene_queries()[:3]
    scans, preds = [scan for _, _, scan in queries], [pred for _, pred, _ in queries]
    W = s["W"]
    R, t, score, info = grid.match_scans(scans, preds, linear_window=W * s["resolution"], angular_window=12.0, angular_step=1.0, field=field)
    for b, (true, pred, scan) in enumerate(queries):
        angles = gref.angle_rows(pred[2])
        cs = gref.cos_sin_of(angles)
        vol, rows = gref.volume(lf, scan, pred[:2], cs, W, grid.min_x, grid.min_y, grid.resolution)
        rec = gref.record(vol, rows, 12, W)
        want_R, want_t = gref.pose(rec, pred[:2], cs, W, grid.resolution)
        assert [info[key][b] for key in ("status", "rows", "index", "a", "j", "i", "centre_score")] == [rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[7]]
        assert score[b] == rec[6] and np.array_equal(R[b], want_R) and np.array_equal(t[b], want_t) and info["shift_bits"] == k
        assert np.abs(t[b] - np.array(true[:2])).max() <= s["resolution"] and abs(np.rad2deg(info["angle"][b] - true[2])) <= 1.0
    Ww = 20                                                        # the wide search: 1 m each way, pruned with the field's own bounds
    M = wide.bound_field(lf, 8)
    bounds = grid.bound_field(field, 8)
    assert np.array_equal(bounds.cpu().numpy(), M)
    R, t, score, info = grid.search_scans(scans, preds, linear_window=Ww * s["resolution"], angular_window=12.0, angular_step=1.0, block=8,
                                          field=field, bounds=bounds)
    for b, (true, pred, scan) in enumerate(queries):
        cs = gref.cos_sin_of(gref.angle_rows(pred[2]))
        rec, _ = wide.search(lf, 8, scan, pred[:2], cs, Ww, 12, grid.min_x, grid.min_y, grid.resolution, M=M)
        want_R, want_t = gref.pose(rec, pred[:2], cs, Ww, grid.resolution)
        assert [info[key][b] for key in ("status", "rows", "index", "a", "j", "i", "centre_score", "blocks", "survivors", "seed_score",
                                         "max_bound")] == [rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[7], rec[8], rec[9], rec[10], rec[11]]
        assert score[b] == rec[6] and np.array_equal(R[b], want_R) and np.array_equal(t[b], want_t)
        assert np.abs(t[b] - np.array(true[:2])).max() <= s["resolution"]
