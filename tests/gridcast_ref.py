"""NumPy restatement of the cast's contract in include/icpmi.h (icpmi_grid_cast_segments, icpmi_grid_cast_rays): the steps of
a segment from the closed form, the first occupied cell, the first unknown cell before it, the float64 expressions of a ray's
end cells and the ranges the Python layer forms from a record — and the cases the CPU and the GPU suite share
(tests/test_grid_cast_cpu.py, tests/test_grid_cast_gpu.py).  It uses nothing of the library."""
import numpy as np

COORD_MAX = 2 ** 29
NONE, NO_CELLS = -1, -2
K_HIT, X_HIT, Y_HIT, K_UNKNOWN = 0, 1, 2, 3


def cast_segment(field, threshold, seg):
    """The record [k_hit, x_hit, y_hit, k_unknown] of one segment (x0, y0, x1, y1) over an int16 (ny, nx) field."""
    ny, nx = field.shape
    x0, y0, x1, y1 = (min(max(int(v), -COORD_MAX), COORD_MAX) for v in seg)
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    K = max(dx, dy)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    if dx >= dy:
        m0, n0, sm, sn, dmaj, dmin, nmaj, nmin = x0, y0, sx, sy, dx, dy, nx, ny
    else:
        m0, n0, sm, sn, dmaj, dmin, nmaj, nmin = y0, x0, sy, sx, dy, dx, ny, nx
    # the steps whose major coordinate m0 + sm * k lies in [0, nmaj): only those can be cells of the grid
    klo, khi = (max(0, -m0), min(K, nmaj - 1 - m0)) if sm > 0 else (max(0, m0 - (nmaj - 1)), min(K, m0))
    if klo > khi:
        return [NONE, x1, y1, NONE]
    k = np.arange(klo, khi + 1, dtype=np.int64)
    q = (2 * k * dmin + dmaj - 1) // (2 * dmaj) if dmaj else np.zeros_like(k)
    major, minor = m0 + sm * k, n0 + sn * q
    inside = (minor >= 0) & (minor < nmin)
    k, major, minor = k[inside], major[inside], minor[inside]
    x, y = (major, minor) if dx >= dy else (minor, major)
    v = field[y, x].astype(np.int64)
    hit = np.flatnonzero(v >= threshold)
    unknown = v == 0
    if len(hit):
        j = hit[0]
        k_hit, xh, yh, unknown = int(k[j]), int(x[j]), int(y[j]), unknown[:j]
    else:
        k_hit, xh, yh = NONE, x1, y1
    first = np.flatnonzero(unknown)
    return [k_hit, xh, yh, int(k[first[0]]) if len(first) else NONE]


def cast_segments(field, threshold, segs):
    segs = np.asarray(segs).reshape(-1, 4)
    return np.array([cast_segment(field, threshold, s) for s in segs], dtype=np.int32).reshape(len(segs), 4)


def step_cell(seg, k):
    """The cell of step k of a segment, from the closed form (Python integers)."""
    x0, y0, x1, y1 = (int(v) for v in seg)
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    dmaj, dmin = max(dx, dy), min(dx, dy)
    q = (2 * k * dmin + dmaj - 1) // (2 * dmaj) if dmaj else 0
    return (x0 + sx * k, y0 + sy * q) if dx >= dy else (x0 + sx * q, y0 + sy * k)


def ray_segments(min_x, min_y, res, xy, pose_cs, beam_cs, reach):
    """-> (segments (P, A, 4) int64 clamped to +-2^29, has_cells (P, A)): the float64 expressions of the contract, each
    operation rounded on its own, one ray at a time."""
    xy, pose_cs, beam_cs = (np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in (xy, pose_cs, beam_cs))
    P, A = len(xy), len(beam_cs)
    segs, ok = np.zeros((P, A, 4), dtype=np.int64), np.zeros((P, A), dtype=bool)
    reach, res, min_x, min_y = np.float64(reach), np.float64(res), np.float64(min_x), np.float64(min_y)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            px, py, ct, st = xy[p, 0], xy[p, 1], pose_cs[p, 0], pose_cs[p, 1]
            for a in range(A):
                ca, sa = beam_cs[a, 0], beam_cs[a, 1]
                c = ct * ca - st * sa
                s = st * ca + ct * sa
                ex = px + reach * c
                ey = py + reach * s
                f = [np.floor((px - min_x) / res), np.floor((py - min_y) / res), np.floor((ex - min_x) / res), np.floor((ey - min_y) / res)]
                ok[p, a] = all(abs(v) < 1e300 for v in f)                            # (NaN compares false)
                if ok[p, a]:
                    segs[p, a] = [int(min(max(v, -float(COORD_MAX)), float(COORD_MAX))) for v in f]
    return segs, ok


def cast_rays(field, threshold, min_x, min_y, res, xy, pose_cs, beam_cs, reach):
    """-> (records (P, A, 4) int32, segments, has_cells)"""
    segs, ok = ray_segments(min_x, min_y, res, xy, pose_cs, beam_cs, reach)
    P, A = ok.shape
    rec = np.zeros((P, A, 4), dtype=np.int32)
    for p in range(P):
        for a in range(A):
            rec[p, a] = cast_segment(field, threshold, segs[p, a]) if ok[p, a] else [NO_CELLS, 0, 0, NONE]
    return rec, segs, ok


def ranges_of(rec, segs, xy, min_x, min_y, res):
    """(ranges, unknown_range) (P, A) float64 as OccupancyGrid2D.cast_scans states them: the distance from the pose to the
    centre of the hit cell (inf: no hit, nan: no cells) and to the centre of the first unknown cell (inf: none)."""
    P, A = rec.shape[:2]
    ranges, unknown = np.full((P, A), np.inf), np.full((P, A), np.inf)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    centre = lambda cx, cy, p: np.hypot((cx + 0.5) * res + min_x - xy[p, 0], (cy + 0.5) * res + min_y - xy[p, 1])   # noqa: E731
    for p in range(P):
        for a in range(A):
            k_hit, xh, yh, k_unk = (int(v) for v in rec[p, a])
            if k_hit == NO_CELLS:
                ranges[p, a] = np.nan
            elif k_hit >= 0:
                ranges[p, a] = centre(xh, yh, p)
            if k_unk >= 0:
                unknown[p, a] = centre(*step_cell(segs[p, a], k_unk), p)
    return ranges, unknown


# ── the shared cases of icpmi_grid_cast_segments ─────────────────────────────
THRESHOLD = 2048
SIZES = [(70, 100), (40, 32), (1, 1), (1, 200), (200, 1)]
BATCHES = (1, 63, 64, 65, 257)


def wall_field(ny, nx, seed):
    """Known free space (a value below the threshold that is not 0) with walls at the columns x = 31, 32, 63, 64 and nx - 1
    — on the two sides of a word boundary and in the last word's pad — whose cells are threshold, 32767 or, as gaps,
    threshold - 1; a sprinkle of unknown cells (0) and of single occupied cells."""
    rng = np.random.default_rng(seed)
    f = np.full((ny, nx), 7, dtype=np.int16)
    f[rng.random((ny, nx)) < 0.15] = 0
    f[rng.random((ny, nx)) < 0.01] = 32767
    for x in (31, 32, 63, 64, nx - 1):
        if 0 <= x < nx:
            f[:, x] = np.array([THRESHOLD, 32767, THRESHOLD - 1], dtype=np.int16)[rng.integers(0, 3, size=ny)]
    return f


def star_segments(ny, nx, seed, n=257):
    """n segments: from origins inside, on the border and outside the grid, towards every octant, along both axes, exact
    diagonals, dx or dy = 0 and K = 0; rays that enter the grid, leave it and never touch it."""
    rng = np.random.default_rng(seed)
    origins = [(0, 0), (nx - 1, ny - 1), (nx // 2, ny // 2), (min(33, nx - 1), ny // 3), (-5, ny // 2), (nx + 4, -3), (nx // 3, ny + 6), (-9, -9)]
    offsets = [(0, 0), (9, 0), (-9, 0), (0, 9), (0, -9), (9, 9), (-9, 9), (9, -9), (-9, -9), (70, 3), (-70, 3), (70, -3), (-70, -3),
               (3, 70), (3, -70), (-3, 70), (-3, -70), (40, 20), (-40, 20), (40, -20), (-40, -20), (20, 40), (-20, 40), (20, -40), (-20, -40),
               (130, 0), (-130, 0), (0, 230), (0, -230), (33, 1), (-33, 1), (1, 33), (1, -33)]
    segs = [(ox, oy, ox + dx, oy + dy) for ox, oy in origins for dx, dy in offsets]
    while len(segs) < n:
        segs.append(tuple(int(v) for v in rng.integers(-12, max(nx, ny) + 12, size=4)))
    return np.array(segs[:n], dtype=np.int32)


def between_field_and_segments():
    """Two diagonally adjacent occupied cells with free cells on the other diagonal: a walk whose diagonal move falls there
    passes BETWEEN them.  Pairs on both diagonals all over a 48 x 48 field, and segments of slope 1/2, 2/5 and 2 in every
    direction through them, forwards and backwards, so both tie rules of mapping.py:68-89 (e2 > -dy and e2 < dx) decide
    in each direction."""
    f = np.full((48, 48), 5, dtype=np.int16)
    for y in range(2, 46, 4):
        for x in range(2, 46, 4):
            if (x + y) % 8 == 4:
                f[y, x] = f[y + 1, x + 1] = THRESHOLD
            else:
                f[y + 1, x] = f[y, x + 1] = THRESHOLD
    segs = []
    for ox, oy in ((24, 24), (23, 25), (10, 30), (31, 9)):
        for dx, dy in ((10, 5), (10, 4), (5, 10), (4, 10), (12, 6), (6, 12), (9, 9)):
            for sx in (1, -1):
                for sy in (1, -1):
                    segs.append((ox, oy, ox + sx * dx, oy + sy * dy))
                    segs.append((ox + sx * dx, oy + sy * dy, ox, oy))
    return f, np.array(segs, dtype=np.int32)


def unknown_row():
    """A 1 x 200 row and hand-made segments with their records: an unknown cell directly before the hit, one directly after
    it (which must not count), one at step 0; a hit exactly at step K; an occupied cell at step K + 1 (no hit); K = 0 on an
    occupied cell and on a free one."""
    f = np.full((1, 200), 9, dtype=np.int16)
    f[0, 50], f[0, 49], f[0, 51] = THRESHOLD, 0, 0
    f[0, 120], f[0, 100] = 32767, 0
    f[0, 150] = THRESHOLD - 1
    segs_and_records = [
        ((10, 0, 60, 0), (40, 50, 0, 39)),          # unknown at 49, directly before the hit at 50
        ((60, 0, 10, 0), (10, 50, 0, 9)),           # from the right: 51 is directly before the hit, 49 behind it
        ((52, 0, 90, 0), (NONE, 90, 0, NONE)),      # nothing
        ((51, 0, 90, 0), (NONE, 90, 0, 0)),         # unknown at step 0
        ((105, 0, 120, 0), (15, 120, 0, NONE)),     # the hit exactly at step K
        ((105, 0, 119, 0), (NONE, 119, 0, NONE)),   # occupied at step K + 1: no hit
        ((130, 0, 100, 0), (10, 120, 0, NONE)),     # the unknown cell 100 lies behind the hit
        ((120, 0, 120, 0), (0, 120, 0, NONE)),      # K = 0 on an occupied cell
        ((121, 0, 121, 0), (NONE, 121, 0, NONE)),   # K = 0 on a free cell
        ((100, 0, 100, 0), (NONE, 100, 0, 0)),      # K = 0 on an unknown cell
        ((140, 0, 160, 0), (NONE, 160, 0, NONE)),   # threshold - 1 is not occupied
        ((-30, 0, 230, 0), (80, 50, 0, 79)),        # starts outside the grid and would leave it on the far side
        ((10, 3, 60, 3), (NONE, 60, 3, NONE)),      # never touches the grid
    ]
    return f, np.array([s for s, _ in segs_and_records], dtype=np.int32), np.array([r for _, r in segs_and_records], dtype=np.int32)


def fuzz():
    """4 000 segments with ends in [-40, 140]^2 on a random 100 x 100 field: 3 % occupied, 30 % zero."""
    rng = np.random.default_rng(7)
    u = rng.random((100, 100))
    f = np.where(u < 0.03, rng.choice(np.array([THRESHOLD, 32767, 9000], dtype=np.int16), size=u.shape),
                 np.where(u < 0.33, 0, rng.choice(np.array([THRESHOLD - 1, -32767, 1, -1], dtype=np.int16), size=u.shape))).astype(np.int16)
    return f, rng.integers(-40, 141, size=(4000, 4)).astype(np.int32)
