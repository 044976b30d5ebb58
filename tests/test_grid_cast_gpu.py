"""The cast on the device (csrc/gridcast.hip; icpmi.gridmatch.occupancy_planes, cast_segments, cast_rays; cast_scans, cast_scan
and occupancy_planes of utilities.mapping.OccupancyGrid2D) against the NumPy restatement of the contract
(tests/gridcast_ref.py, itself held to the reference's walk by tests/test_grid_cast_cpu.py).  A record is four integers, so
every comparison is array_equal: on small grids with walls on both sides of a word of the planes and in the pad of the last
one, at every batch size around a wave, between diagonal neighbours, around unknown cells, on a random field, on the golden
segments of the reference, and through the Python layers on the room map — where the ranges are compared bit for bit too."""
import numpy as np
import pytest

import gridcast_ref as ref
import gridmatch_ref as gref
import likelihood_ref as lref
from conftest import load_golden

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert (_lib.GC_K_HIT, _lib.GC_X_HIT, _lib.GC_Y_HIT, _lib.GC_K_UNKNOWN, _lib.GC_NONE, _lib.GC_NO_CELLS) == (
        ref.K_HIT, ref.X_HIT, ref.Y_HIT, ref.K_UNKNOWN, ref.NONE, ref.NO_CELLS)


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cast(field, threshold, segs, kept=False):
    """The device's records of ``segs`` over ``field`` (through kept planes when asked), into a tensor full of a sentinel."""
    import torch
    from icpmi import gridmatch
    fd, sd = on_device(field), on_device(segs)
    out = torch.full((len(segs), 4), SENTINEL, dtype=torch.int32, device="cuda")
    got = gridmatch.cast_segments(gridmatch.occupancy_planes(fd, threshold) if kept else fd, threshold, sd, out=out)
    assert got is out
    assert np.array_equal(fd.cpu().numpy(), field) and np.array_equal(sd.cpu().numpy(), segs)      # the inputs are left as they were
    return out.cpu().numpy()


def differing(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    print("records that differ:", len(bad), "of", len(want), [(got[b].tolist(), want[b].tolist()) for b in bad[:3]])
    return len(bad)


@pytest.mark.parametrize("n", range(len(ref.SIZES)), ids=[f"{ny}x{nx}" for ny, nx in ref.SIZES])
def test_small_grids_at_every_batch_size(gpu, n):
    ny, nx = ref.SIZES[n]
    field, segs = ref.wall_field(ny, nx, n), ref.star_segments(ny, nx, n)
    want = ref.cast_segments(field, ref.THRESHOLD, segs)
    for batch in ref.BATCHES:
        got = cast(field, ref.THRESHOLD, segs[:batch], kept=batch == 65)
        assert got.shape == (batch, 4) and differing(got, want[:batch]) == 0, batch
        assert np.array_equal(got, want[:batch])


def test_between_diagonal_neighbours_and_around_unknown_cells(gpu):
    field, segs = ref.between_field_and_segments()
    assert np.array_equal(cast(field, ref.THRESHOLD, segs), ref.cast_segments(field, ref.THRESHOLD, segs))
    field, segs, records = ref.unknown_row()
    assert np.array_equal(cast(field, ref.THRESHOLD, segs), records)
    assert np.array_equal(cast(field, 0, segs), ref.cast_segments(field, 0, segs))                # 0 is occupied AND unknown: the hit wins
    far = np.array([[-2 ** 29, 0, 2 ** 29, 0], [2 ** 29, 0, -2 ** 29, 0], [50, -2 ** 29, 50, 2 ** 29]], dtype=np.int32)
    assert np.array_equal(cast(field, ref.THRESHOLD, far), ref.cast_segments(field, ref.THRESHOLD, far))
    empty = np.zeros((0, 9), dtype=np.int16)                       # an empty grid: every ray has cells and none is hit
    assert np.array_equal(cast(empty, 1, segs), ref.cast_segments(empty, 1, segs))


def test_fuzz_and_a_second_run_writes_the_same_bytes(gpu):
    field, segs = ref.fuzz()
    want = ref.cast_segments(field, ref.THRESHOLD, segs)
    assert (want[:, 0] >= 0).mean() > 0.3 and (want[:, 3] >= 0).mean() > 0.3
    got = cast(field, ref.THRESHOLD, segs)
    assert differing(got, want) == 0
    assert np.array_equal(cast(field, ref.THRESHOLD, segs), got) and np.array_equal(cast(field, ref.THRESHOLD, segs, kept=True), got)
    ragged = np.ascontiguousarray(field[:71, :97])                 # rows that start at odd int16 offsets, a tail behind the last group
    assert np.array_equal(cast(ragged, ref.THRESHOLD, segs), ref.cast_segments(ragged, ref.THRESHOLD, segs))


def test_golden_segments_on_the_device(gpu):
    """Only end cells are occupied.  The short segments all leave one origin for every cell of a 33 x 33 square, so most of
    them stop at another segment's end cell, a step or two out; nearly every long one reaches its own, at step K, after up
    to 5 707 steps that were looked at and found free."""
    segs = load_golden("bresenham")["segs"]
    fits = (segs.min(axis=1) >= -50) & (segs.max(axis=1) <= 450)
    assert int(fits.sum()) == 1089
    for part, shift, size in ((segs[fits], 50, 512), (segs[~fits], 3008, 6016)):
        s = (part + shift).astype(np.int32)
        field = np.full((size, size), 3, dtype=np.int16)
        field[s[:, 3], s[:, 2]] = ref.THRESHOLD
        want = ref.cast_segments(field, ref.THRESHOLD, s)
        K = np.abs(part[:, 2:] - part[:, :2]).max(axis=1)
        assert (want[:, 0] >= 0).all() and K.max() == (5707 if size == 6016 else 16)
        assert size == 512 or (want[:, 0] == K).mean() > 0.9       # (a condition on the inputs: 0.975 when this was written)
        assert differing(cast(field, ref.THRESHOLD, s), want) == 0


# ── the room map through the Python layers ───────────────────────────────────
@pytest.fixture(scope="module")
def room(gpu):
    """(the grid of the scene's 12 scans at 0.1 m built on the device, its field restated, k, the threshold of 0.5)"""
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    origins, hits = gref.scene_scans()
    grid.update_scans(origins, hits)
    k = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    q = gref.quantise(grid.log_odds, k)
    q.setflags(write=False)
    return grid, q, k, int(np.rint(0.5 * 2.0 ** k))


def poses_and_angles(P, A):
    rng = np.random.default_rng(100 * P + A)
    poses = np.stack([rng.uniform(-3.0, 3.0, P), rng.uniform(-2.0, 2.0, P), rng.uniform(-np.pi, np.pi, P)], axis=1)
    return poses, np.linspace(-np.pi, np.pi, A, endpoint=False) + 0.01


def restated(grid, q, threshold, poses, angles, reach):
    args = (grid.min_x, grid.min_y, grid.resolution, poses[:, :2], gref.cos_sin_of(poses[:, 2]), gref.cos_sin_of(angles), reach)
    rec, segs, ok = ref.cast_rays(q, threshold, *args)
    ranges, unknown = ref.ranges_of(rec, segs, poses[:, :2], grid.min_x, grid.min_y, grid.resolution)
    return rec, ranges, unknown


def same(ranges, info, rec, want_ranges, want_unknown):
    return (np.array_equal(info["k_hit"], rec[..., 0]) and np.array_equal(info["cells"], rec[..., 1:3]) and np.array_equal(info["k_unknown"], rec[..., 3])
            and np.array_equal(ranges, want_ranges, equal_nan=True) and np.array_equal(info["unknown_range"], want_unknown))


@pytest.mark.parametrize("P", (1, 3, 65))
@pytest.mark.parametrize("A", (1, 65, 360))
def test_cast_scans_in_the_room(room, P, A):
    grid, q, k, threshold = room
    poses, angles = poses_and_angles(P, A)
    rec, want_ranges, want_unknown = restated(grid, q, threshold, poses, angles, 30.0)
    ranges, info = grid.cast_scans(poses, angles, 30.0)
    assert ranges.shape == (P, A) and ranges.dtype == np.float64 and info["shift_bits"] == k == 12
    print(P, A, "hits", int((rec[..., 0] >= 0).sum()), "unknown first", int((rec[..., 3] >= 0).sum()))
    assert same(ranges, info, rec, want_ranges, want_unknown)
    if A > 1:                                                      # (conditions on the inputs: most rays end at a wall, some cross unexplored space)
        assert (rec[..., 0] >= 0).mean() > 0.8 and (A < 360 or (rec[..., 3] >= 0).any())
    one, one_info = grid.cast_scan(poses[P - 1], angles, 30.0)
    assert one.shape == (A,) and same(one, one_info, rec[P - 1], want_ranges[P - 1], want_unknown[P - 1])
    matrix = np.array([[np.cos(poses[0, 2]), -np.sin(poses[0, 2]), poses[0, 0]], [np.sin(poses[0, 2]), np.cos(poses[0, 2]), poses[0, 1]], [0, 0, 1.0]])
    assert grid.cast_scan(matrix, angles, 30.0)[0].shape == (A,)


def test_poses_without_cells_and_ends_beyond_the_clamp(room):
    grid, q, k, threshold = room
    poses, angles = poses_and_angles(3, 65)
    poses[1, 0] = np.nan
    rec, want_ranges, want_unknown = restated(grid, q, threshold, poses, angles, 30.0)
    ranges, info = grid.cast_scans(poses, angles, 30.0)
    assert (info["k_hit"][1] == ref.NO_CELLS).all() and np.isnan(ranges[1]).all() and np.isinf(info["unknown_range"][1]).all()
    assert (info["cells"][1] == 0).all() and same(ranges, info, rec, want_ranges, want_unknown)
    poses[1, 0] = 0.5
    rec, want_ranges, want_unknown = restated(grid, q, threshold, poses, angles, 1e9)            # 1e10 cells: the end cells are clamped
    assert (np.abs(rec[rec[..., 0] == ref.NONE][:, 1:3]).max(axis=1) == 2 ** 29).all()
    ranges, info = grid.cast_scans(poses, angles, 1e9)
    assert same(ranges, info, rec, want_ranges, want_unknown)
    # the layer below, into a tensor full of a sentinel: every record is written, those of the rays without cells too
    import torch
    from icpmi import gridmatch
    poses[2, 1] = np.inf
    want, _, _ = ref.cast_rays(q, threshold, grid.min_x, grid.min_y, grid.resolution, poses[:, :2], gref.cos_sin_of(poses[:, 2]), gref.cos_sin_of(angles), 30.0)
    out = torch.full((3, 65, 4), SENTINEL, dtype=torch.int32, device="cuda")
    xy = on_device(poses[:, :2])
    got = gridmatch.cast_rays(on_device(q.copy()), threshold, grid.min_x, grid.min_y, grid.resolution, xy, gref.cos_sin_of(poses[:, 2]), gref.cos_sin_of(angles), 30.0,
                              out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want) and (want[2, :, 0] == ref.NO_CELLS).all()
    assert np.array_equal(xy.cpu().numpy(), poses[:, :2], equal_nan=True)


def test_kept_planes_and_fields_show_the_map_as_it_was(room):
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    origins, hits = gref.scene_scans()
    grid.update_scans(origins[:6], hits[:6])
    poses, angles = poses_and_angles(3, 360)
    before, before_info = grid.cast_scans(poses, angles, 30.0)
    field, planes = grid.score_field(), grid.occupancy_planes()
    for kw in (dict(field=field), dict(planes=planes), dict(planes=grid.occupancy_planes(field=field))):
        ranges, info = grid.cast_scans(poses, angles, 30.0, **kw)
        assert ranges.tobytes() == before.tobytes() and all(np.array_equal(info[key], before_info[key]) for key in before_info)
    grid.update_scans(origins[6:], hits[6:])
    after, _ = grid.cast_scans(poses, angles, 30.0)
    assert after.tobytes() != before.tobytes()                     # the map moved on ...
    for kw in (dict(field=field), dict(planes=planes)):            # ... what was kept did not
        assert grid.cast_scans(poses, angles, 30.0, **kw)[0].tobytes() == before.tobytes()
    other = OccupancyGrid2D(-1.0, 1.0, -1.0, 1.0)
    with pytest.raises(ValueError):
        other.cast_scans(poses, angles, 30.0, planes=planes)
    with pytest.raises(ValueError):
        grid.cast_scans(poses, angles, 30.0, field=field, planes=planes)


def test_a_likelihood_field_is_cast_through_as_well(room):
    grid, q, k, threshold = room
    field = grid.likelihood_field(sigma=0.1, radius=0.3)
    tab = lref.table(np.rint(grid.log_odds_max * 2.0 ** k), 1.0, 3)
    _, lf = lref.likelihood_field(q, threshold, 3, tab, True)
    assert np.array_equal(field[0].cpu().numpy(), lf)
    poses, angles = poses_and_angles(3, 65)
    rec, want_ranges, want_unknown = restated(grid, lf, threshold, poses, angles, 30.0)
    ranges, info = grid.cast_scans(poses, angles, 30.0, field=field)
    assert same(ranges, info, rec, want_ranges, want_unknown)
    assert (rec[..., 0] >= 0).mean() > 0.9


def test_python_layer_refuses_what_the_entries_would(gpu):
    import torch
    from icpmi import gridmatch
    fd = on_device(np.zeros((8, 8), dtype=np.int16))
    segs = np.zeros((3, 4), dtype=np.int32)
    pcs = np.array([[1.0, 0.0]])
    for bad in (lambda: gridmatch.occupancy_planes(fd.to(torch.int32), 1), lambda: gridmatch.occupancy_planes(fd[:, ::2], 1),
                lambda: gridmatch.cast_segments(fd.to(torch.float32), 1, segs), lambda: gridmatch.cast_segments(fd, 1, segs[:, :3]),
                lambda: gridmatch.cast_segments(fd, 1, segs.astype(np.float64)), lambda: gridmatch.cast_segments(fd, 1, segs + 2 ** 29 + 1),
                lambda: gridmatch.cast_segments(fd, 1, segs, out=torch.zeros((3, 3), dtype=torch.int32, device="cuda")),
                lambda: gridmatch.cast_segments(fd, 1, on_device(segs).to(torch.int64)),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.0, [[0.0, 0.0]], pcs, pcs, 5.0),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, [[0.0, 0.0]], pcs, pcs, -1.0),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, [[0.0, 0.0]], pcs, pcs, float("nan")),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, float("inf"), [[0.0, 0.0]], pcs, pcs, 5.0),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, [[0.0, 0.0], [1.0, 1.0]], pcs, pcs, 5.0),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, np.zeros((1 << 15, 2)), np.zeros((1 << 15, 2)), np.zeros((1 << 14, 2)), 5.0),
                lambda: gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, [[0.0, 0.0]], pcs, pcs, 5.0, out=torch.zeros((1, 1, 4), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    assert gridmatch.cast_segments(fd, 1, np.zeros((0, 4), dtype=np.int32)).shape == (0, 4)      # nothing to do is no refusal
    assert gridmatch.cast_rays(fd, 1, 0.0, 0.0, 0.1, np.zeros((0, 2)), np.zeros((0, 2)), pcs, 5.0).shape == (0, 1, 4)
