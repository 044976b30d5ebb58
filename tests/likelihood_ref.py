"""NumPy restatement of the likelihood-field contract of include/icpmi.h (icpmi_grid_likelihood_field): occupancy from the
threshold, the exact truncated squared distance by two shifted-minimum passes in int64, the sentinel, the table and
keep_free.  Shared by tests/test_likelihood_field_cpu.py and tests/test_likelihood_field_gpu.py; it uses nothing of the
library."""
import numpy as np

MAX_RADIUS = 64
FAR = 1 << 40                                                      # "no occupied cell within R": above every real sum


def occupancy(q, threshold):
    return np.asarray(q, dtype=np.int64) >= int(threshold)


def _shifted(a, d, axis, fill):
    """out[i] = a[i + d] along ``axis``, ``fill`` where i + d leaves the array."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(d, 0), n + min(d, 0))
    dst[axis] = slice(max(-d, 0), n - max(d, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def distance_field(q, threshold, R):
    """d2[y, x] = min (y - y')^2 + (x - x')^2 over the occupied cells where that is <= R^2, else R^2 + 1; int16."""
    assert 0 <= R <= MAX_RADIUS
    occ = occupancy(q, threshold)
    g = np.where(occ, 0, FAR).astype(np.int64)                     # the column distance to the nearest occupied cell within R
    for dy in range(1, R + 1):
        for d in (dy, -dy):
            g = np.minimum(g, np.where(_shifted(occ, d, 0, False), dy, FAR))
    g2 = np.where(g < FAR, g * g, FAR)
    d2 = g2.copy()
    for dx in range(1, R + 1):
        for d in (dx, -dx):
            d2 = np.minimum(d2, _shifted(g2, d, 1, FAR) + dx * dx)
    return np.where(d2 <= R * R, d2, R * R + 1).astype(np.int16)


def table(peak, sigma_cells, R):
    """The expression the issue fixes, in float64."""
    return np.clip(np.rint(peak * np.exp(-np.arange(R * R + 1) / (2 * sigma_cells ** 2))), -32767, 32767).astype(np.int16)


def likelihood_field(q, threshold, R, tab, keep_free=True):
    """-> (d2, lf): lf = tab[d2] within the radius; beyond it min(q, 0) (keep_free) or 0."""
    tab = np.asarray(tab, dtype=np.int16)
    assert tab.shape == (R * R + 1,) and tab.min() > -32768
    d2 = distance_field(q, threshold, R)
    near = d2 <= R * R
    beyond = np.minimum(np.asarray(q, dtype=np.int16), 0) if keep_free else np.zeros_like(d2)
    return d2, np.where(near, tab[np.where(near, d2, 0)], beyond).astype(np.int16)


# ── the cases the device is held to, and the restatement itself to scipy's transform ──────────────────────────────────
def cases(ty, tx):
    """[(name, q int16 (ny, nx), threshold, R, table int16, keep_free)]: the smallest shapes at which a kernel whose workgroups
    own tiles of ty x tx outputs with a halo of R can go wrong."""
    out = []
    gauss = lambda R: table(20480.0, max(R / 3.0, 0.5), R)                                     # noqa: E731
    for shape in ((1, 1), (1, 70), (70, 1)):                       # grids smaller than a halo, occupied at the ends
        q = np.zeros(shape, dtype=np.int16)
        q[shape[0] // 2, shape[1] // 2] = -7                       # a cell of free space (the only cell of 1 x 1: occupied below)
        q[0, 0] = q[-1, -1] = 100
        for R in (0, 1, 64):
            out.append((f"degenerate {shape} R={R}", q, 50, R, gauss(R), True))
    ny, nx = ty + 1, 2 * tx - 1                                    # two tiles each way, the last one row or ragged
    for R in (1, min(ty, tx) - 1, 64):
        q = np.full((ny, nx), -5, dtype=np.int16)
        q[0, 0] = q[0, -1] = q[-1, 0] = q[-1, -1] = 9
        q[20, tx - R] = q[45, tx - R - 1] = 9                      # R and R + 1 cells left of the seam's first column tx
        q[25, tx - 1 + R] = q[50, tx + R] = 9                      # R and R + 1 cells right of its last column tx - 1
        q[ty - R, 40] = 9                                          # R rows above the last row, ty
        if ty - R - 1 >= 0:
            q[ty - R - 1, 200] = 9                                 # and R + 1
        out.append((f"tile edges R={R}", q, 9, R, gauss(R), True))
    rng = np.random.default_rng(1)
    q = rng.integers(-3000, 100, size=(130, 200)).astype(np.int16)
    out.append(("nothing occupied, free kept", q, 100, 7, gauss(7), True))
    out.append(("nothing occupied, free dropped", q, 100, 7, gauss(7), False))
    out.append(("everything occupied", q, -3000, 7, gauss(7), True))
    q = np.where(np.random.default_rng(0).random((130, 200)) < 0.005, 3000, rng.integers(-3000, 100, size=(130, 200))).astype(np.int16)
    out.append(("sparse random, free kept", q, 2048, 64, gauss(64), True))
    out.append(("sparse random, free dropped", q, 2048, 64, gauss(64), False))
    q = rng.integers(-32767, 32768, size=(70, 150)).astype(np.int16)
    q[3, 5], q[40, 140], q[69, 0] = -32767, 0, 32767               # every threshold below is a value the field holds
    negative = (1000 - 37 * np.arange(3 * 3 + 1)).astype(np.int16)
    negative[-1] = -32767
    for threshold in (-32767, 0, 32767):
        out.append((f"threshold {threshold}, a table with negative entries", q, threshold, 3, negative, True))
    return out


# ── the scene of the localisation check: the room of gridmatch_ref at 0.05 m from its first scan alone, thin noisy queries ──
SCENE = dict(resolution=0.05, noise=0.05, every=8, W=12, sigma_cells=2.0, radius=6, occupied_log_odds=0.5, clamp=5.0)


def scene_queries():
    """gridmatch_ref.scene_queries with the scans redrawn at the scene's range noise, every 8th row of each:
    12 x (true pose, predicted pose, query scan)."""
    from icpmi import synth

    import gridmatch_ref
    return [(true, pred, synth.scan(true, 900 + t, noise=SCENE["noise"])[::2][::SCENE["every"]])
            for t, (true, pred, _) in enumerate(gridmatch_ref.scene_queries())]
