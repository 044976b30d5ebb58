"""NumPy restatement of the beam model's contract in include/icpmi.h (icpmi_grid_beam_batch): the far end of a row in
float64, the three cells by gridmatch_ref's expressions, the cast's record of the segment from the pose's cell to the far
end's by gridcast_ref.cast_segment, the step at which the beam returned on that walk's major axis, the table index of the
row, the sums of a pair — and the hand-made cases the CPU and the GPU suite share (tests/test_grid_beam_cpu.py,
tests/test_grid_beam_gpu.py).  The clouds, poses and fields are the check's (gridcheck_ref).  It uses nothing of the library."""
import numpy as np

import gridcast_ref as cref
import gridcheck_ref as kref

INTS, ROW_INTS = 8, 4
STATUS, ROWS, SCORE, EXPECTED, NOVEL, UNEXPLORED = range(6)
ST_OK, ST_EMPTY, ST_CAPACITY = 0, 1, 2
NO_CELLS, MAX_HALF_WIDTH, TABLE_CLIP, MAX_ROWS = -2, 127, 32767, 65535
NO_ROW = [NO_CELLS, 0, 0, -1]
HALF_WIDTHS = (0, 1, 8, 127)
BEYONDS = (0.0, 0.3, 2.0, 1e4)


def far_end(pts, beyond):
    """(fx, fy) of every row: r = sqrt(x * x + y * y), s = (r + beyond) / r, each operation rounded on its own."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        r = np.sqrt(x * x + y * y)
        s = (r + np.float64(beyond)) / r
        return np.stack([x * s, y * s], axis=1)


def walk_rows(field, threshold, min_x, min_y, res, pts, t, cs, beyond):
    """What does not depend on the table -> (n, 5) int64 [has cells, k_hit, k_z, k_unknown, the hit cell is observed]."""
    ny, nx = field.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    far = far_end(pts, beyond)
    out = np.zeros((len(pts), 5), dtype=np.int64)
    out[:, 3] = -1
    o = kref.cell_of(0.0, 0.0, 1.0, 0.0, t[0], t[1], min_x, min_y, res)
    if o is None:
        return out
    for i in range(len(pts)):
        h = kref.cell_of(pts[i, 0], pts[i, 1], cs[0], cs[1], t[0], t[1], min_x, min_y, res)
        f = kref.cell_of(far[i, 0], far[i, 1], cs[0], cs[1], t[0], t[1], min_x, min_y, res)
        if h is None or f is None:
            continue
        k_hit, _, _, k_unknown = cref.cast_segment(field, threshold, (o[0], o[1], f[0], f[1]))
        k_z = abs(h[0] - o[0]) if abs(f[0] - o[0]) >= abs(f[1] - o[1]) else abs(h[1] - o[1])
        observed = 0 <= h[0] < nx and 0 <= h[1] < ny and field[h[1], h[0]] != 0
        out[i] = [1, k_hit, k_z, k_unknown, observed]
    return out


def score(walks, table, H):
    """-> (record [8] int32 with status OK or EMPTY, hist [2H + 3] int32, rows (n, 4) int32 [index, k_hit, k_z, k_unknown])."""
    table = np.clip(np.asarray(table, dtype=np.int64), -TABLE_CLIP, TABLE_CLIP)
    assert table.shape == (2 * H + 3,)
    rows = np.tile(np.array(NO_ROW, dtype=np.int32), (len(walks), 1))
    rec, hist = np.zeros(INTS, dtype=np.int64), np.zeros(2 * H + 3, dtype=np.int32)
    for i, (cells, k_hit, k_z, k_unknown, observed) in enumerate(walks.tolist()):
        if not cells:
            continue
        idx = min(max(k_hit - k_z, -H), H) + H if k_hit >= 0 else (2 * H + 1 if observed else 2 * H + 2)
        rows[i] = [idx, k_hit, k_z, k_unknown]
        hist[idx] += 1
        rec[ROWS] += 1
        rec[SCORE] += table[idx]
        rec[EXPECTED] += k_hit >= 0
        rec[NOVEL] += idx == 2 * H + 1
        rec[UNEXPLORED] += idx == 2 * H + 2
    rec[STATUS] = ST_OK if rec[ROWS] else ST_EMPTY
    assert abs(rec[SCORE]) < 2 ** 31
    return rec.astype(np.int32), hist, rows


def beam_pair(field, threshold, min_x, min_y, res, pts, t, cs, table, H, beyond, cnt=None):
    """-> (record, hist, rows (n, 4)) of one pair; n the cloud's count (0 with CAPACITY, where nothing is read)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    n = kref.rows_of(len(pts), cnt)
    if n < 0:
        rec = np.zeros(INTS, dtype=np.int32)
        rec[STATUS] = ST_CAPACITY
        return rec, np.zeros(2 * H + 3, dtype=np.int32), np.zeros((0, ROW_INTS), dtype=np.int32)
    return score(walk_rows(field, threshold, min_x, min_y, res, pts[:n], t, cs, beyond), table, H)


def table_of(H, seed=0):
    """A table no two entries of which are equal, so a wrong index shows in the score: distinct values in [-30 000, 0]."""
    rng = np.random.default_rng(300 + 7 * H + seed)
    return -rng.choice(30001, size=2 * H + 3, replace=False).astype(np.int32)


def hand_made():
    """Hand-made pairs on gridcast_ref.unknown_row()'s 1 x 200 field (walls at 50 and 120, unknown cells at 49, 51 and 100),
    the grid's corner at (0, 0) and 1 m cells, every pose at the centre of its cell under the identity, the table
    TABLE[i] = -(i + 1) for its 2H + 3 entries (or the case's own) -> (field, cases): a case is (origin cell x, the rows' x
    offsets in cells, H, beyond, table or None, the literal record, the literal histogram as {index: rows}, the literal
    rows)."""
    field, _, _ = cref.unknown_row()
    nan, inf = float("nan"), float("inf")
    cases = [
        # a return exactly on the wall at 120: the walk goes on to 123, k_hit = k_z = 15, index H
        (105, [15], 2, 3.0, None, [ST_OK, 1, -3, 1, 0, 0, 0, 0], {2: 1}, [[2, 15, 15, -1]]),
        # one step short of the wall (d = +1) and one step behind it (d = -1: the walk ends at its first wall all the same)
        (105, [14], 2, 3.0, None, [ST_OK, 1, -4, 1, 0, 0, 0, 0], {3: 1}, [[3, 15, 14, -1]]),
        (105, [16], 2, 3.0, None, [ST_OK, 1, -2, 1, 0, 0, 0, 0], {1: 1}, [[1, 15, 16, -1]]),
        # differences clamped at +-H: five steps short under H = 2, seven behind
        (105, [10], 2, 6.0, None, [ST_OK, 1, -5, 1, 0, 0, 0, 0], {4: 1}, [[4, 15, 10, -1]]),
        (105, [22], 2, 1.0, None, [ST_OK, 1, -1, 1, 0, 0, 0, 0], {0: 1}, [[0, 15, 22, -1]]),
        # H = 0: three entries, every difference reads entry 0
        (105, [14, 15, 16], 0, 3.0, None, [ST_OK, 3, -3, 3, 0, 0, 0, 0], {0: 3}, [[0, 15, 14, -1], [0, 15, 15, -1], [0, 15, 16, -1]]),
        (105, [5], 0, 3.0, None, [ST_OK, 1, -2, 0, 1, 0, 0, 0], {1: 1}, [[1, -1, 5, -1]]),
        # a wall farther than `beyond`: the walk ends at 113, the hit cell 110 is observed free space (index 2H + 1)
        (105, [5], 2, 3.0, None, [ST_OK, 1, -6, 0, 1, 0, 0, 0], {5: 1}, [[5, -1, 5, -1]]),
        # ... and with beyond = 0 a return one step short of the wall does not see it
        (105, [14], 2, 0.0, None, [ST_OK, 1, -6, 0, 1, 0, 0, 0], {5: 1}, [[5, -1, 14, -1]]),
        # an unknown hit cell (100; the walk 90 -> 103 finds no wall) and a hit cell off the grid (205): index 2H + 2
        (90, [10], 2, 3.0, None, [ST_OK, 1, -7, 0, 0, 1, 0, 0], {6: 1}, [[6, -1, 10, 10]]),
        (190, [15], 2, 3.0, None, [ST_OK, 1, -7, 0, 0, 1, 0, 0], {6: 1}, [[6, -1, 15, -1]]),
        # towards -x through the unknown cell 51 to the wall at 50: k_hit = 10, the beam returned at step 8
        (60, [-8], 2, 3.0, None, [ST_OK, 1, -5, 1, 0, 0, 0, 0], {4: 1}, [[4, 10, 8, 9]]),
        # rows without cells among rows with: at the origin (s is not finite), NaN, inf and 1e305
        (105, [15, 0.0, nan, 14, inf, 1e305], 2, 3.0, None, [ST_OK, 2, -7, 2, 0, 0, 0, 0], {2: 1, 3: 1},
         [[2, 15, 15, -1], NO_ROW, NO_ROW, [3, 15, 14, -1], NO_ROW, NO_ROW]),
        (105, [0.0, nan, inf, 1e305], 2, 3.0, None, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], {}, [NO_ROW] * 4),
        # an origin without a cell
        (nan, [15, 16], 2, 3.0, None, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], {}, [NO_ROW, NO_ROW]),
        (1e305, [15, 16], 2, 3.0, None, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], {}, [NO_ROW, NO_ROW]),
        # table entries of +-40 000 count as +-32 767
        (105, [15, 15, 14], 1, 3.0, [7, 40000, -40000, 1, 2], [ST_OK, 3, 32767, 3, 0, 0, 0, 0], {1: 2, 2: 1},
         [[1, 15, 15, -1], [1, 15, 15, -1], [2, 15, 14, -1]]),
        (105, [14, 14, 15], 1, 3.0, [7, 40000, -40000, 1, 2], [ST_OK, 3, -32767, 3, 0, 0, 0, 0], {1: 1, 2: 2},
         [[2, 15, 14, -1], [2, 15, 14, -1], [1, 15, 15, -1]]),
    ]
    return field, cases


def hand_made_pair(case):
    """-> (pts (n, 2), translation, cos_sin, table, H, beyond) of a case of ``hand_made``."""
    origin, offsets, H, beyond, table = case[:5]
    table = -np.arange(1, 2 * H + 4, dtype=np.int32) if table is None else np.array(table, dtype=np.int32)
    return np.array([[dx, 0.0] for dx in offsets], dtype=np.float64), np.array([origin + 0.5, 0.5]), np.array([1.0, 0.0]), table, H, beyond


def hist_of(case):
    H = case[2]
    h = np.zeros(2 * H + 3, dtype=np.int32)
    for i, n in case[6].items():
        h[i] = n
    return h
