"""The rebuild that follows an accepted loop closure, from the resident scan history: ``ScanHistory.world_rows``
(icpmi_history_world_rows), ``OccupancyGrid2D.rebuild_from_history`` / ``replay_history`` and
``RollingSubmap.reset_from_history`` against the host path they replace — NumPy's ``pts @ T[:2, :2].T + T[:2, 2]`` per scan
(slam.py:46-50), ``update_scans`` of those arrays (slam.py:271-277) and ``reset`` with their tail (slam.py:612-615).  Everything
is compared bit for bit: the kernel reproduces NumPy's rounding (tests/test_rebuild_cpu.py pins what that is), and a cell box
that is a superset changes no cell.

Tiny scans on a 400 x 400 grid at 0.1 m; the 70-scan drive and its host replay are made once."""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOXEL, NORMAL_K, RS_VOXEL = 0.04, 12, 0.15
GRID = dict(min_x=-3.0, max_x=37.0, min_y=-15.0, max_y=25.0, resolution=0.1, p_hit=0.85, p_miss=0.42)
SIZES = (1, 2, 63, 64, 65, 257, 2048)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import features
    features.VERBOSE = False


def new_history(**kw):
    from icpmi import ScanHistory
    return ScanHistory(voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, **kw)


def new_grid(log_odds_min=-8.0, log_odds_max=8.0):
    from utilities.mapping import OccupancyGrid2D
    g = OccupancyGrid2D(log_odds_min=log_odds_min, log_odds_max=log_odds_max, **GRID)
    assert (g.ny, g.nx) == (400, 400)
    return g


def pose_matrix(x, y, th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]])


def numpy_worlds(scans, poses):
    return [pts @ T[:2, :2].T + T[:2, 2] for pts, T in zip(scans, poses)]


# ── 1. world_rows ────────────────────────────────────────────────────────────
def form_rows(pts, T):
    """The two forms of the contract, each operation rounded once (exact rationals): two or more rows as gemm has them,
    fma(y, R[c][1], x * R[c][0]) + t[c]; exactly one row as gemv has it, fma(x, R[c][0], y * R[c][1]) + t[c].  A coordinate
    whose pose entries are not all finite is NaN either way (the points are finite)."""
    out = np.empty((len(pts), 2))
    for c in (0, 1):
        a, b, t = float(T[c, 0]), float(T[c, 1]), float(T[c, 2])
        if not np.isfinite([a, b, t]).all():
            out[:, c] = pts[:, 0] * a + pts[:, 1] * b + t
            assert np.isnan(out[:, c]).all()
            continue
        A, B, Tq = Fraction(a), Fraction(b), Fraction(t)
        for i, (x, y) in enumerate(pts):
            x, y = float(x), float(y)
            if len(pts) == 1:
                inner = float(Fraction(x) * A + Fraction(y * b))
            else:
                inner = float(Fraction(y) * B + Fraction(x * a))
            out[i, c] = inner + t
    return out


@pytest.fixture(scope="module")
def sized(gpu):
    """A history of scans of SIZES rows, a pose per scan (identity, not orthonormal, one with a NaN, rotations) and the
    expected world rows of each scan under its pose."""
    rng = np.random.default_rng(21)
    scans = [rng.uniform(-9.0, 9.0, size=(n, 2)) for n in SIZES]
    poses = [pose_matrix(*rng.uniform(-3.0, 3.0, size=3)) for _ in SIZES]
    while np.array_equal(form_rows(scans[0], poses[0]), form_rows(np.vstack([scans[0]] * 2), poses[0])[:1]):
        poses[0] = pose_matrix(*rng.uniform(-3.0, 3.0, size=3))   # the one-row scan: a pose at which the two forms differ
    poses[1] = np.eye(3)
    poses[3] = np.array([[1.5, 0.2, -4.0], [-0.3, 0.25, 2.0], [0.0, 0.0, 1.0]])
    poses[4][0, 0] = np.nan
    h = new_history()
    assert h.add_many(scans) == list(range(len(SIZES)))
    want = [form_rows(s, T) for s, T in zip(scans, poses)]
    assert np.isnan(want[4][:, 0]).all() and np.isfinite(want[4][:, 1]).all()
    return h, scans, poses, want


@pytest.mark.parametrize("ids", [None, list(range(len(SIZES)))[::-1], [3, 0, 3, 6, 1, 0], [5, 2], [4], []],
                         ids=["all", "reversed", "repeat", "subset", "nan_pose", "empty"])
def test_world_rows_bit_for_bit(sized, ids):
    h, scans, poses, want = sized
    order = list(range(len(SIZES))) if ids is None else ids
    raw = h.raw.pts[:h.rows_used].clone()
    rows, off = h.world_rows([poses[k] for k in order], ids)
    assert rows.dtype.is_floating_point and rows.element_size() == 8 and rows.device == h.device and off.dtype == np.int32
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([SIZES[k] for k in order])]).astype(np.int32))
    assert tuple(rows.shape) == (int(off[-1]), 2)
    got = rows.cpu().numpy()
    for j, k in enumerate(order):
        assert np.array_equal(got[off[j]:off[j + 1]], want[k], equal_nan=True), (j, k)
        assert np.isnan(got[off[j]:off[j + 1]]).any() == (k == 4), (j, k)          # the NaN pose's scan and nothing else
    import torch
    assert torch.equal(h.raw.pts[:h.rows_used], raw)                                # the history is read, never written


def test_the_one_row_scan_takes_the_other_form(sized):
    """The one-row scan's pose is chosen so that the gemm form would give another double: the choice is per scan."""
    h, scans, poses, want = sized
    two = np.vstack([scans[0], scans[0]])
    assert not np.array_equal(form_rows(two, poses[0])[:1], want[0])
    assert np.array_equal(h.world_rows([poses[0]], [0])[0].cpu().numpy(), want[0])


def test_reach_is_recorded_per_scan(sized):
    h, scans, _, _ = sized
    assert h.reach.shape == (len(SIZES),)
    assert np.array_equal(h.reach, [np.hypot(s[:, 0], s[:, 1]).max() for s in scans])


# ── 2. the grid ──────────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def drive(gpu):
    """70 scans of 90 beams along a 30 m path through the maze, poses a little off the truth (as after an optimisation), the
    history holding them, and the host replay of all of them on a fresh grid."""
    from icpmi import synth
    segs = synth.maze_segments()
    rng = np.random.default_rng(5)
    truth = [(2.0 + 30.0 * k / 69, 5.0 + 0.4 * np.sin(0.3 * k), 0.05 * k) for k in range(70)]
    scans = [synth.scan(p, 600 + k, n_beams=90, segs=segs) for k, p in enumerate(truth)]
    poses = [pose_matrix(x + rng.normal(0, 0.02), y + rng.normal(0, 0.02), th + rng.normal(0, 0.01)) for x, y, th in truth]
    h = new_history()
    h.add_many(scans)
    worlds = numpy_worlds(scans, poses)
    return dict(scans=scans, poses=poses, history=h, worlds=worlds)


def host_replay(grid, scans, poses, rows=None, worlds=None):
    worlds = numpy_worlds(scans, poses) if worlds is None else worlds
    grid.update_scans(np.array([T[:2, 2] for T in poses]), worlds, rows=rows)
    return grid


def dirty(grid, drive):
    grid.update_scan(drive["poses"][3][:2, 2], drive["worlds"][3])
    return grid


@pytest.mark.parametrize("n", [1, 3, 70])
def test_grid_rebuild_equals_the_host_replay(drive, n):
    """1 scan: the single-launch owner path; 70 scans: two pieces.  rebuild_from_history resets a grid that held something."""
    import torch
    h = drive["history"]
    if n < 70:
        h = new_history()
        h.add_many(drive["scans"][:n])
    poses = drive["poses"][:n]
    want = host_replay(new_grid(), drive["scans"][:n], poses, worlds=drive["worlds"][:n])
    got = dirty(new_grid(), drive)
    got.rebuild_from_history(h, poses)
    assert torch.equal(got.device_log_odds, want.device_log_odds)
    assert int((want.device_log_odds != 0).sum()) > 100 * n
    assert np.array_equal(got.log_odds, want.log_odds)
    if n == 70:                                                   # the scratch is one piece's, not the history's
        assert got._replay_scratch.shape[0] == max(sum(len(s) for s in drive["scans"][:64]), sum(len(s) for s in drive["scans"][64:]))


def test_replay_by_id_on_a_band_of_rows(drive):
    """rows=(5, 200) and a list of ids (reversed, one repeated) on a grid that is not reset: only the band changes."""
    import torch
    ids = list(range(69, 40, -1)) + [7, 7]
    poses = [drive["poses"][k] for k in ids]
    want, got = dirty(new_grid(), drive), dirty(new_grid(), drive)
    before = got.device_log_odds.clone()
    host_replay(want, [drive["scans"][k] for k in ids], poses, rows=(5, 200))
    got.replay_history(drive["history"], poses, ids=ids, rows=(5, 200))
    assert torch.equal(got.device_log_odds, want.device_log_odds)
    assert torch.equal(got.device_log_odds[200:], before[200:]) and not torch.equal(got.device_log_odds[:200], before[:200])


def test_grid_rebuild_with_a_full_clip(drive):
    """log_odds_min > 0: 0 lies outside the range, so the first scan after a reset clips every cell."""
    import torch
    want = host_replay(new_grid(0.5, 5.0), drive["scans"], drive["poses"], worlds=drive["worlds"])
    got = new_grid(0.5, 5.0)
    got.rebuild_from_history(drive["history"], drive["poses"])
    assert torch.equal(got.device_log_odds, want.device_log_odds)
    assert float(got.device_log_odds.min()) == 0.5


def test_a_nan_pose_takes_the_read_back_route(drive):
    """No promise from the host for a piece with a NaN pose: the cell box is read back from the device, as for device
    tensors, and the result is still the host replay's."""
    import torch
    poses = [T.copy() for T in drive["poses"][:4]]
    poses[2][0, 0] = np.nan                                      # every x of scan 2: beams with a non-finite end are dropped
    want = host_replay(new_grid(), drive["scans"][:4], poses)
    got = new_grid()
    got.replay_history(drive["history"], poses, ids=[0, 1, 2, 3])
    assert torch.equal(got.device_log_odds, want.device_log_odds)


# ── 3. a history that has grown ──────────────────────────────────────────────
def test_rebuild_after_growth_and_after_the_large_scan(drive):
    """scan_capacity 2 and a row capacity the second scan exceeds: the buffers are replaced several times on the way to 70
    scans; then a 2 049-row scan switches the history out of bearing order (every earlier scan is prepared again).  The
    rebuilds equal the host replay each time, and match records before and after a rebuild are identical: the rebuild
    writes nothing into the history."""
    import torch
    from icpmi import synth
    from icpmi.submap import RollingSubmap
    scans, poses = list(drive["scans"]), list(drive["poses"])
    h = new_history(scan_capacity=2, row_capacity=100)
    h.add(scans[0])
    h.add_many(scans[1:30])
    for s in scans[30:33]:
        h.add(s)
    h.add_many(scans[33:])
    assert h.scan_capacity == 128 and h.row_capacity >= sum(len(s) for s in scans) and h.layout_generation > 3
    assert np.array_equal(h.reach, drive["history"].reach)
    want = host_replay(new_grid(), scans, poses, worlds=drive["worlds"])
    got = new_grid()

    def records():
        m = h.match(40, [38, 12, 39], error_threshold=1e-10, max_iterations=30)
        m.run()
        return m.icp.results.cpu().numpy()[:3].copy(), m.search.records.cpu().numpy()[:3].copy()

    before = records()
    got.rebuild_from_history(h, poses)
    RollingSubmap(window=8, voxel_size=0.04).reset_from_history(h, poses).build()
    after = records()
    assert torch.equal(got.device_log_odds, want.device_log_odds)
    assert np.array_equal(before[0], after[0], equal_nan=True) and np.array_equal(before[1], after[1], equal_nan=True)

    big = synth.scan((20.0, 5.0, 0.3), 77, n_beams=2049, segs=synth.maze_segments())
    assert len(big) == 2049 and h.allow_polar
    h.add(big)
    assert not h.allow_polar
    scans.append(big)
    poses.append(pose_matrix(20.05, 4.97, 0.31))
    want = host_replay(new_grid(), scans, poses)
    got.rebuild_from_history(h, poses)
    assert torch.equal(got.device_log_odds, want.device_log_odds)
    again = records()
    got.rebuild_from_history(h, poses)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, records()))


# ── 4. the submap ────────────────────────────────────────────────────────────
@pytest.mark.parametrize("window", [5, 100])
def test_submap_reset_from_history(drive, window):
    import torch
    from icpmi.submap import RollingSubmap
    h, poses, worlds = drive["history"], drive["poses"], drive["worlds"]
    want = RollingSubmap(window=window, voxel_size=0.04)
    want.reset(worlds[-window:])
    got = RollingSubmap(window=window, voxel_size=0.04).reset_from_history(h, poses)
    assert len(got) == len(want) == min(window, 70) and got.points_in == want.points_in
    held = torch.cat(got._scans).clone()
    assert torch.equal(held, torch.cat(want._scans))
    assert torch.equal(got.build()[0], want.build()[0])
    # later transforms and a map rebuild (its scratch is reused) leave the buffer alone
    moved = [pose_matrix(1.0, 2.0, 0.5) @ T for T in poses]
    h.world_rows(moved)
    new_grid().rebuild_from_history(h, moved)
    h.world_rows(moved[-window:], list(range(70))[-window:])
    assert torch.equal(torch.cat(got._scans), held)
    got._built = None
    assert torch.equal(got.build()[0], want.build()[0])
    # by id: the tail of the list given
    ids = [9, 3, 3, 60, 1, 30, 2]
    got.reset_from_history(h, [poses[k] for k in ids], ids)
    want.reset([worlds[k] for k in ids][-window:])
    assert torch.equal(got.build()[0], want.build()[0])


# ── 5. refusals ──────────────────────────────────────────────────────────────
def test_refusals(drive):
    import torch
    from icpmi.submap import RollingSubmap
    h, poses = drive["history"], drive["poses"]
    n = len(h)
    grid = new_grid()
    sub = RollingSubmap(window=5)
    zero = grid.device_log_odds.clone()
    h.match(drive["scans"][3][::2], [0, 1])                       # a staged source now sits in slot n
    assert h.sizes()[n] > 0
    for bad in ([n], [0, n + 7], [-1]):                           # n: the staged source's slot
        P = poses[:len(bad)]
        with pytest.raises(ValueError, match="scan ids"):
            h.world_rows(P, bad)
        with pytest.raises(ValueError, match="scan ids"):
            grid.replay_history(h, P, ids=bad)
        with pytest.raises(ValueError, match="scan ids"):
            sub.reset_from_history(h, P, bad)
    with pytest.raises(ValueError, match="1-D"):
        h.world_rows(poses[:1], [0.5])
    for P, ids in ((poses[:-1], None), (poses, [0, 1]), ([T[:2] for T in poses], None), (np.zeros((n, 6)), None), (poses[0], [0])):
        with pytest.raises(ValueError, match="poses"):
            h.world_rows(P, ids)
        with pytest.raises(ValueError, match="poses"):
            grid.rebuild_from_history(h, P) if ids is None else grid.replay_history(h, P, ids=ids)
        with pytest.raises(ValueError, match="poses"):
            sub.reset_from_history(h, P, ids)
    assert len(sub) == 0 and torch.equal(grid.device_log_odds, zero) and len(h) == n


def test_a_history_on_another_device_is_refused(drive):
    import torch
    from icpmi.submap import RollingSubmap
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    with torch.cuda.device(1):
        grid, sub = new_grid(), RollingSubmap(window=5)
    with pytest.raises(ValueError, match="lives on"):
        grid.rebuild_from_history(drive["history"], drive["poses"])
    with pytest.raises(ValueError, match="lives on"):
        sub.reset_from_history(drive["history"], drive["poses"])
