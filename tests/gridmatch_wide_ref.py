"""NumPy restatement of the wide-window search of include/icpmi.h (icpmi_grid_bound_field, icpmi_grid_search_batch): the
bound field by an explicit sliding maximum, the blocks' bounds, the seeds, the survivors, the 12-slot record — and the
exhaustive volume it must agree with, vectorised (tests/gridmatch_ref.py's loops over shifts take minutes at these windows).
Shared by tests/test_grid_search_cpu.py and tests/test_grid_search_gpu.py; it uses nothing of the library."""
import numpy as np

from gridmatch_ref import cells, quantise, record, scene_queries  # noqa: F401  (quantise: for the tests that import this module alone)

BLOCKS = (4, 8, 16)
SLAB_CELLS = 1 << 22                                               # gathered cells of one slab of the exhaustive volume


def bound_field(q, D):
    """M(y, x) = max of the 0-extended field over rows [y, y + D), columns [x, x + D), for y in [-(D - 1), ny) and x likewise,
    stored at [y + D - 1, x + D - 1]: int16 (ny + D - 1, nx + D - 1)."""
    ny, nx = q.shape
    pad = np.zeros((ny + 2 * (D - 1), nx + 2 * (D - 1)), dtype=np.int16)
    pad[D - 1:D - 1 + ny, D - 1:D - 1 + nx] = q
    out = np.full((ny + D - 1, nx + D - 1), -32768, dtype=np.int16)
    for dy in range(D):
        for dx in range(D):
            np.maximum(out, pad[dy:dy + ny + D - 1, dx:dx + nx + D - 1], out=out)
    return out


def gather(arr, y, x):
    """arr[y, x] as int64 with 0 wherever (y, x) lies outside arr: fancy indexing of arr padded by one ring of zeros."""
    pad = np.pad(arr.astype(np.int64), 1)
    return pad[np.clip(y + 1, 0, arr.shape[0] + 1), np.clip(x + 1, 0, arr.shape[1] + 1)]


def volume(q, pts, t, cos_sin, W, min_x, min_y, res):
    """gridmatch_ref.volume, vectorised: -> (score [A, S, S] int32, rows with a cell [A])."""
    S = 2 * W + 1
    d = np.arange(S) - W
    out, rows = np.zeros((len(cos_sin), S, S), dtype=np.int64), np.zeros(len(cos_sin), dtype=np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    for a, (c, s) in enumerate(cos_sin):
        cx, cy = cells(pts, c, s, t[0], t[1], min_x, min_y, res)
        rows[a] = n = len(cx)
        step = max(1, SLAB_CELLS // max(1, n * S))
        for j0 in range(0, S, step):                                # slabs of j: rows x js x S gathered cells at a time
            dj = d[j0:j0 + step]
            out[a, j0:j0 + step] = gather(q, cy[:, None, None] + dj[None, :, None], cx[:, None, None] + d[None, None, :]).sum(axis=0)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32), rows


def bounds(M, D, pts, t, cos_sin, W, min_x, min_y, res):
    """U[a, J, I] = sum over the rows with a cell at angle a of M(cy + J * D - W, cx + I * D - W) -> ([A, NB, NB] int32, rows [A])."""
    S = 2 * W + 1
    NB = -(-S // D)
    o = np.arange(NB) * D - W + (D - 1)                             # into the stored array: origin offset D - 1
    out, rows = np.zeros((len(cos_sin), NB, NB), dtype=np.int64), np.zeros(len(cos_sin), dtype=np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    for a, (c, s) in enumerate(cos_sin):
        cx, cy = cells(pts, c, s, t[0], t[1], min_x, min_y, res)
        rows[a] = len(cx)
        out[a] = gather(M, cy[:, None, None] + o[None, :, None], cx[:, None, None] + o[None, None, :]).sum(axis=0)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32), rows


def block_scores(q, cx, cy, W, D, J, I):
    """The exact scores of the shifts of block (J, I) at one angle, [dj, di] int64; shifts with j >= S or i >= S are cut off."""
    S = 2 * W + 1
    j, i = np.arange(J * D, min((J + 1) * D, S)), np.arange(I * D, min((I + 1) * D, S))
    return gather(q, cy[:, None, None] + (j - W)[None, :, None], cx[:, None, None] + (i - W)[None, None, :]).sum(axis=0)


def search(q, D, pts, t, cos_sin, W, centre_angle, min_x, min_y, res, M=None, keep=np.greater_equal):
    """The pruned search as the contract states it -> (the 12 int32 of a record, U [A, NB, NB]).  Only the seed blocks, the
    survivors and the centre's block are ever scored.  ``keep``: the survivor test against the seed score; with np.greater
    in its place (the counter-check) the seeds' own best result stands where no survivor beats it."""
    M = bound_field(q, D) if M is None else M
    S = 2 * W + 1
    NB = -(-S // D)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    U, rows = bounds(M, D, pts, t, cos_sin, W, min_x, min_y, res)
    cell = [cells(pts, c, s, t[0], t[1], min_x, min_y, res) for c, s in cos_sin]

    def best_of(a, J, I):
        """(score, lowest flat index attaining it) of a block"""
        sc = block_scores(q, cell[a][0], cell[a][1], W, D, J, I)
        dj, di = np.unravel_index(int(np.argmax(sc.ravel())), sc.shape)         # first maximum: lowest j, then lowest i
        return int(sc[dj, di]), (a * S + J * D + int(dj)) * S + I * D + int(di)

    def better(x, y):
        return y is None or x[0] > y[0] or (x[0] == y[0] and x[1] < y[1])

    seed = None
    for a in range(len(cos_sin)):
        J, I = np.unravel_index(int(np.argmax(U[a].ravel())), (NB, NB))          # first block in C order of maximal U
        got = best_of(a, int(J), int(I))
        if better(got, seed):
            seed = got
    best0 = seed[0]
    kept = np.argwhere(keep(U, best0))
    win = None if keep is np.greater_equal else seed
    for a, J, I in kept:
        got = best_of(int(a), int(J), int(I))
        if better(got, win):
            win = got
    score, flat = win
    a, rem = divmod(flat, S * S)
    j, i = divmod(rem, S)
    centre = 0
    if centre_angle >= 0:
        sc = block_scores(q, cell[centre_angle][0], cell[centre_angle][1], W, D, W // D, W // D)
        centre = int(sc[W % D, W % D])
    status = 0 if rows.any() else 1
    rec = np.array([status, rows[a], flat, a, j, i, score, centre, len(cos_sin) * NB * NB, len(kept), best0, U.max()], dtype=np.int32)
    return rec, U


# ── the plateaus of the tie and >= checks ────────────────────────────────────
def plateau(on_the_edge):
    """A constant positive field and 40 rows.  Inside: every row lies in the grid under every shift, so every score and every
    bound is 40 * 9.  On the edge (rows outside the grid allowed): 20 rows A at cell x = W - D, which are inside from i = D on,
    and 20 rows B at cell (nx + W - D, W - 1), inside for i < D and j >= 1.  No shift holds both groups, so the maximum is
    20 * 9, first at (j, i) = (0, D) — in block (0, 1), whose bound is 20 * 9 too — and the seed block (0, 0), first of that
    bound, has it only from (1, 0) on."""
    W, D = 5, 4
    q = np.full((40, 30), 9, dtype=np.int16)
    grid = dict(min_x=0.0, min_y=0.0, res=1.0)
    if not on_the_edge:
        pts = np.stack([np.linspace(8.5, 20.5, 40), np.linspace(10.5, 28.5, 40)], axis=1)
    else:
        A = np.stack([np.full(20, W - D + 0.5), np.linspace(W + 0.5, 30.5, 20)], axis=1)
        B = np.stack([np.full(20, 30 + W - D + 0.5), np.full(20, W - 1 + 0.5)], axis=1)
        pts = np.vstack([A, B])
    return q, pts, (0.0, 0.0), np.array([[1.0, 0.0]]), W, D, grid


# ── the relocalisation check: the scene of gridmatch_ref, predicted metres and tens of degrees off ─────────────────────
RELOC = dict(offset_m=3.0, offset_deg=40.0, W=40, angular_window=45.0, angular_step=1.0, queries=6, block=8)
SIGNS = ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))


def reloc_queries():
    """(true pose, predicted pose, scan) of the first RELOC['queries'] queries of gridmatch_ref.scene_queries, every second row
    of the scan, the prediction 3 m off on each axis and 40 degrees off in heading with the signs cycling."""
    out = []
    for k, (true, _, scan) in enumerate(scene_queries()[:RELOC["queries"]]):
        sx, sy, st = SIGNS[k % 4]
        pred = (true[0] + sx * RELOC["offset_m"], true[1] + sy * RELOC["offset_m"], true[2] + st * np.deg2rad(RELOC["offset_deg"]))
        out.append((true, pred, scan[::2]))
    return out
