"""NumPy restatement of the check's contract in include/icpmi.h (icpmi_grid_check_batch): the cells of a row by
gridmatch_ref's expressions, the cast's record of the segment from the pose's cell to the row's cell by
gridcast_ref.cast_segment, the class of the row, the counts of a pair — and the cases the CPU and the GPU suite share
(tests/test_grid_check_cpu.py, tests/test_grid_check_gpu.py).  It uses nothing of the library."""
import numpy as np

import gridcast_ref as cref
import gridmatch_ref as gref

INTS, ROW_INTS = 8, 4
STATUS, ROWS, CONFIRMED, VIOLATED, IN_FREE, UNEXPLORED, THROUGH_UNKNOWN = range(7)
ST_OK, ST_EMPTY, ST_CAPACITY = 0, 1, 2
CLASS_CONFIRMED, CLASS_VIOLATED, CLASS_IN_FREE, CLASS_UNEXPLORED, NO_CELLS = 0, 1, 2, 3, -2
MAX_ROWS, MAX_TOLERANCE = 65535, 2 ** 30
NO_ROW = [NO_CELLS, 0, 0, -1]


def cell_of(x, y, c, s, tx, ty, min_x, min_y, res):
    """The cell (cx, cy) of one row, or None: gridmatch_ref.cells of that row alone."""
    cx, cy = gref.cells(np.array([[x, y]], dtype=np.float64), np.float64(c), np.float64(s), np.float64(tx), np.float64(ty), np.float64(min_x),
                        np.float64(min_y), np.float64(res))
    return (int(cx[0]), int(cy[0])) if len(cx) else None


def walk_rows(field, threshold, min_x, min_y, res, pts, t, cs):
    """What does not depend on the tolerance -> (n, 5) int64 [has cells, k_hit, K, k_unknown, the end cell is observed]: the
    origin cell comes from (tx, ty) by the rows' own rule (the row (0, 0) under the identity), and without it no row has cells."""
    ny, nx = field.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(pts), 5), dtype=np.int64)
    out[:, 3] = -1
    origin = cell_of(0.0, 0.0, 1.0, 0.0, t[0], t[1], min_x, min_y, res)
    if origin is None:
        return out
    for i, (x, y) in enumerate(pts):
        end = cell_of(x, y, cs[0], cs[1], t[0], t[1], min_x, min_y, res)
        if end is None:
            continue
        k_hit, _, _, k_unknown = cref.cast_segment(field, threshold, (origin[0], origin[1], end[0], end[1]))
        K = max(abs(end[0] - origin[0]), abs(end[1] - origin[1]))
        observed = 0 <= end[0] < nx and 0 <= end[1] < ny and field[end[1], end[0]] != 0
        out[i] = [1, k_hit, K, k_unknown, observed]
    return out


def classify(walks, tolerance):
    """-> (record [8] int32 with status OK or EMPTY, rows (n, 4) int32 [class, k_hit, K, k_unknown])."""
    rows = np.tile(np.array(NO_ROW, dtype=np.int32), (len(walks), 1))
    rec = np.zeros(INTS, dtype=np.int32)
    for i, (cells, k_hit, K, k_unknown, observed) in enumerate(walks.tolist()):
        if not cells:
            continue
        if k_hit >= 0:
            cls = CLASS_CONFIRMED if k_hit >= K - int(tolerance) else CLASS_VIOLATED
        else:
            cls = CLASS_IN_FREE if observed else CLASS_UNEXPLORED
        rows[i] = [cls, k_hit, K, k_unknown]
        rec[ROWS] += 1
        rec[CONFIRMED + cls] += 1
        rec[THROUGH_UNKNOWN] += k_unknown >= 0
    rec[STATUS] = ST_OK if rec[ROWS] else ST_EMPTY
    return rec, rows


def rows_of(cap, cnt):
    """The matcher's rule for a cloud's rows: the device count where there is one; -1 (CAPACITY) when it is negative, beyond
    the cloud's own rows or beyond MAX_ROWS."""
    n = cap if cnt is None else int(cnt)
    return -1 if n < 0 or n > cap or n > MAX_ROWS else n


def check_pair(field, threshold, min_x, min_y, res, pts, t, cs, tolerance, cnt=None):
    """-> (record, rows (n, 4)) of one pair; n the cloud's count (0 with CAPACITY, where nothing is read)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    n = rows_of(len(pts), cnt)
    if n < 0:
        rec = np.zeros(INTS, dtype=np.int32)
        rec[STATUS] = ST_CAPACITY
        return rec, np.zeros((0, ROW_INTS), dtype=np.int32)
    return classify(walk_rows(field, threshold, min_x, min_y, res, pts[:n], t, cs), tolerance)


# ── the shared cases ─────────────────────────────────────────────────────────
CLOUD_ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 513)            # around a wave (64) and around a chunk (256)
TOLERANCES = (0, 1, 5, 2 ** 30)
RES, MIN_X, MIN_Y = 0.25, -3.0, -2.0                           # 0.25 and its multiples are exact: a row can lie ON a cell border


def clouds(ny, nx, seed):
    """Nine sensor-frame clouds of CLOUD_ROWS rows whose beams, from poses in and around an (ny, nx) grid at RES, end inside
    the grid, on its border and outside it.  Every fourth row lies exactly on a cell border (a multiple of RES); cloud 4
    holds a NaN and an inf row, cloud 7 a row at 1e305."""
    rng = np.random.default_rng(1000 + seed)
    span = max(nx, ny) * RES
    out = []
    for n in CLOUD_ROWS:
        ang = np.sort(rng.uniform(-np.pi, np.pi, n))
        r = rng.uniform(0.0, 0.8 * span, n)
        p = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
        p[::4] = np.rint(p[::4] / RES) * RES
        out.append(p)
    out[4][7, 0], out[4][30, 1] = np.nan, np.inf
    out[7][100, 0] = 1e305
    return out


def poses(ny, nx, n_pairs, seed):
    """(pair_clouds, translations, cos_sin) of n_pairs pairs: poses inside the grid, on its border (a multiple of RES), outside
    it and — from the third pair on, once — without a cell; clouds repeat among the pairs and every cloud is named when
    there are nine pairs or more."""
    rng = np.random.default_rng(2000 + seed + n_pairs)
    w, h = nx * RES, ny * RES
    pair = (np.arange(n_pairs) * 5 + 8) % len(CLOUD_ROWS)        # 8, 4, 0, 5, 1, ...: the largest cloud first
    if n_pairs >= 3:
        pair[2] = pair[0]                                      # a repeated cloud
    t = np.stack([MIN_X + rng.uniform(0.0, w, n_pairs), MIN_Y + rng.uniform(0.0, h, n_pairs)], axis=1)
    th = rng.uniform(-np.pi, np.pi, n_pairs)
    if n_pairs >= 3:
        t[1] = [MIN_X, MIN_Y + RES * (ny // 2)]                # on the border of cell column 0, and of a cell row
        t[2] = [MIN_X - 1.3, MIN_Y + h + 0.7]                  # outside
    if n_pairs >= 9:
        t[5, 0] = np.nan                                       # no origin cell: no row of the pair has cells
        t[6] = [MIN_X + w, MIN_Y + h]                          # the first cell outside, exactly
        t[7, 1] = -1e12                                        # beyond 2^29 cells
    return pair.astype(np.int32), t, np.stack([np.cos(th), np.sin(th)], axis=1)


def exact_room(inner=21, wall=2, margin=3):
    """A square room of odd inner width with walls ``wall`` cells thick on a field that is 0 outside and a non-zero free value
    inside -> (field, the centre cell (cx, cy))."""
    n = inner + 2 * wall + 2 * margin
    f = np.zeros((n, n), dtype=np.int16)
    a, b = margin, n - margin
    f[a:b, a:b] = cref.THRESHOLD
    f[a + wall:b - wall, a + wall:b - wall] = -9
    c = n // 2
    return f, (c, c)


def hand_made():
    """Hand-made pairs on gridcast_ref.unknown_row()'s 1 x 200 field, the grid's corner at (0, 0) and 1 m cells, every pose at
    the centre of its cell under the identity -> (field, cases): a case is (origin cell x, the rows' x offsets in cells,
    tolerance, the literal record, the literal rows).  A hit exactly at K; a hit at K - 1 under the tolerances 0, 1 and 2^30; an
    occupied cell at K + 1, which is no hit, so the end cell decides; an end cell outside the grid; an unknown end cell; K = 0
    on an occupied, a free and an unknown cell; rows with NaN, inf and 1e305; an origin without a cell."""
    field, _, _ = cref.unknown_row()
    nan, inf = float("nan"), float("inf")
    cases = [
        (105, [15], 0, [ST_OK, 1, 1, 0, 0, 0, 0, 0], [[CLASS_CONFIRMED, 15, 15, -1]]),                 # the hit exactly at K
        (105, [16], 0, [ST_OK, 1, 0, 1, 0, 0, 0, 0], [[CLASS_VIOLATED, 15, 16, -1]]),                  # the hit at K - 1 ...
        (105, [16], 1, [ST_OK, 1, 1, 0, 0, 0, 0, 0], [[CLASS_CONFIRMED, 15, 16, -1]]),
        (105, [16], 2 ** 30, [ST_OK, 1, 1, 0, 0, 0, 0, 0], [[CLASS_CONFIRMED, 15, 16, -1]]),
        (105, [14], 0, [ST_OK, 1, 0, 0, 1, 0, 0, 0], [[CLASS_IN_FREE, -1, 14, -1]]),                   # occupied at K + 1: no hit, a free end
        (190, [15], 0, [ST_OK, 1, 0, 0, 0, 1, 0, 0], [[CLASS_UNEXPLORED, -1, 15, -1]]),                # the end cell 205 is outside
        (90, [10], 0, [ST_OK, 1, 0, 0, 0, 1, 1, 0], [[CLASS_UNEXPLORED, -1, 10, 10]]),                 # the end cell 100 is unknown
        (120, [0], 0, [ST_OK, 1, 1, 0, 0, 0, 0, 0], [[CLASS_CONFIRMED, 0, 0, -1]]),                    # K = 0 on an occupied cell
        (121, [0], 0, [ST_OK, 1, 0, 0, 1, 0, 0, 0], [[CLASS_IN_FREE, -1, 0, -1]]),                     # ... on a free one
        (100, [0], 5, [ST_OK, 1, 0, 0, 0, 1, 1, 0], [[CLASS_UNEXPLORED, -1, 0, 0]]),                   # ... on an unknown one
        (60, [-50], 2, [ST_OK, 1, 0, 1, 0, 0, 1, 0], [[CLASS_VIOLATED, 10, 50, 9]]),                   # through the wall at 50, unknown 51 before it
        (105, [15, nan, 16, inf, 14, 1e305], 0, [ST_OK, 3, 1, 1, 1, 0, 0, 0],
         [[CLASS_CONFIRMED, 15, 15, -1], NO_ROW, [CLASS_VIOLATED, 15, 16, -1], NO_ROW, [CLASS_IN_FREE, -1, 14, -1], NO_ROW]),
        (105, [nan, inf, 1e305], 0, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], [NO_ROW, NO_ROW, NO_ROW]),
        (nan, [15, 16], 0, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], [NO_ROW, NO_ROW]),                         # an origin without a cell
        (1e305, [15, 16], 0, [ST_EMPTY, 0, 0, 0, 0, 0, 0, 0], [NO_ROW, NO_ROW]),
    ]
    return field, cases


def hand_made_pair(case):
    """-> (pts (n, 2), translation, cos_sin) of a case of ``hand_made``."""
    origin, offsets = case[0], case[1]
    return np.array([[dx, 0.0] for dx in offsets], dtype=np.float64), np.array([origin + 0.5, 0.5]), np.array([1.0, 0.0])
