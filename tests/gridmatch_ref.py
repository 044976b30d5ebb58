"""NumPy restatement of the grid-matching contract of include/icpmi.h (icpmi_grid_score_field, icpmi_grid_match_batch):
quantise, cells, the loop over shifts, np.argmax.  Shared by tests/test_grid_match_cpu.py and tests/test_grid_match_gpu.py;
it uses nothing of the library."""
import numpy as np

CELL_MAX = 2.0 ** 29
ST_OK, ST_EMPTY = 0, 1


def shift_bits(lo, hi):
    m = max(abs(lo), abs(hi))
    return max([k for k in range(15) if m * 2.0 ** k <= 32767.0], default=0)


def quantise(log_odds, k):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(log_odds, dtype=np.float32) * np.float32(2.0 ** k))        # float32 product, half to even
        return np.where(np.isnan(r), np.float32(0), np.clip(r, -32767, 32767)).astype(np.int16)


def cells(pts, c, s, tx, ty, min_x, min_y, res):
    """(cx, cy) int64 of the rows that have a cell."""
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        wx, wy = (c * x - s * y) + tx, (s * x + c * y) + ty
        fx, fy = np.floor((wx - min_x) / res), np.floor((wy - min_y) / res)
        ok = np.isfinite(wx) & np.isfinite(wy) & (np.abs(fx) <= CELL_MAX) & (np.abs(fy) <= CELL_MAX)
    return fx[ok].astype(np.int64), fy[ok].astype(np.int64)


def volume(q, pts, t, cos_sin, W, min_x, min_y, res):
    """-> (score [A, S, S] int32, rows with a cell [A])."""
    ny, nx = q.shape
    S = 2 * W + 1
    out, rows = np.zeros((len(cos_sin), S, S), dtype=np.int64), np.zeros(len(cos_sin), dtype=np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    for a, (c, s) in enumerate(cos_sin):
        cx, cy = cells(pts, c, s, t[0], t[1], min_x, min_y, res)
        rows[a] = len(cx)
        for j in range(S):
            for i in range(S):
                y, x = cy + (j - W), cx + (i - W)
                m = (y >= 0) & (y < ny) & (x >= 0) & (x < nx)
                out[a, j, i] = q[y[m], x[m]].astype(np.int64).sum()
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32), rows


def record(vol, rows, centre_angle, W):
    """The eight int32 of a record: status, rows, flat index, a, j, i, best score, centre score."""
    flat = int(np.argmax(vol.ravel()))                                                  # first maximum in C order
    a, j, i = np.unravel_index(flat, vol.shape)
    status = ST_OK if rows.any() else ST_EMPTY
    centre = int(vol[centre_angle, W, W]) if centre_angle >= 0 else 0
    return np.array([status, rows[a], flat, a, j, i, vol[a, j, i], centre], dtype=np.int32)


def pose(rec, t, cos_sin, W, res):
    """(R, t) of a record, formed as the library's host layer forms them."""
    a, j, i = int(rec[3]), int(rec[4]), int(rec[5])
    c, s = cos_sin[a]
    return np.array([[c, -s], [s, c]]), np.array([t[0] + (i - W) * res, t[1] + (j - W) * res])


def angle_rows(theta, angular_window=12.0, angular_step=1.0):
    return theta + np.deg2rad(np.arange(-angular_window, angular_window + angular_step, angular_step))


def cos_sin_of(angles):
    return np.stack([np.cos(angles), np.sin(angles)], axis=-1)


# ── the scene of the localisation check: the room of icpmi.synth, 12 scans along a short path, 12 queries ──────────────
SCENE = dict(min_x=-14.0, max_x=14.0, min_y=-10.0, max_y=10.0, resolution=0.1)
SCENE_POSES = [(-1.0 + 0.25 * k, -0.5 + 0.02 * k, 0.05 * k) for k in range(12)]


def scene_scans():
    """(origins [12, 2], world-frame hits) of the map's scans."""
    from icpmi import synth
    hits = [synth.to_world(synth.scan(p, 50 + k), p) for k, p in enumerate(SCENE_POSES)]
    return np.array([[p[0], p[1]] for p in SCENE_POSES]), hits


def scene_queries():
    """12 x (true pose, predicted pose, query scan), drawn from default_rng(0) in the order the issue fixes."""
    from icpmi import synth
    rng = np.random.default_rng(0)
    out = []
    for t in range(12):
        true = (rng.uniform(-1.0, 1.5), rng.uniform(-0.8, 0.3), rng.uniform(-0.2, 0.7))
        dx, dy = rng.uniform(-0.45, 0.45), rng.uniform(-0.45, 0.45)
        dth = np.deg2rad(rng.uniform(-9.0, 9.0))
        out.append((true, (true[0] + dx, true[1] + dy, true[2] + dth), synth.scan(true, 900 + t)[::2]))
    return out
