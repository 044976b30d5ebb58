"""Clouds above 4 096 and 8 192 rows for the two large routes of the normals (csrc/normals.hip, csrc/prep_big.hip), their
references and their bounds.  No GPU: tests/test_big_clouds_cpu.py checks what is stated here, tests/test_big_clouds_gpu.py
holds the kernels to it.

Sizes: the first size of the large routes, both sides of the LDS / global switch of normals.hip (8 192 slots), a power of
two above it (the index fills its 2 x rows scratch exactly) and one more (32 768 slots).  Neighbour counts: both sides of
every list width of both files, k + 1 <= 8, 13, 16, 32.

Clouds.  A uniform cloud has no direction of its own, so the normal of a point follows its neighbour SET: with one
neighbour wrong it moves by more than 1e9 units (test_big_clouds_cpu.py measures it), where a wall keeps its normal.
  uniform(n)        uniform in [-4, 4]^2;
  uniform_far(n)    the same carried to (2e4, -1.5e4);
  columns(n)        x from 64 exact values (multiples of 2^-3), y uniform: n / 64 equal keys in an x-sorted index;
  duplicates(n)     every point four times, rows shuffled (compared at k >= 4);
  ties(n)           a cloud on a 2^-10 grid (squared distances are exact) with planted queries, each with two candidates for
                    its LAST list slot at bit-equal distance in perpendicular directions; the lower row takes the slot
                    (oracle.knn, TopK::push of normals.hip, TopKP::push of prep_common.hpp);
  decoys(cap, n)    n valid rows, and behind them cap - n rows that each lie nearer to a valid row than any valid row.

Bound: max(NORMALS_FLOOR, FACTOR x figure) as in tests/test_p2l_step_cpu.py, the figure being the largest angle of NumPy's
float64 eigh(np.cov) off the longdouble eigenvector on the reference's neighbours, in units of 2^-52 l1 / (l1 - l0), over
every cloud of the family and every k (to three digits, rounded up; test_big_clouds_cpu.py measures and prints them):

  family       NumPy eigh(np.cov)   bound
  uniform          1.59             12.72    (uniform, uniform_far and the counted rows of decoys)
  columns          1.64             13.12
  duplicates       2.26             18.08
  ties             1.96             15.68
"""
import functools

import numpy as np

from test_p2l_step_cpu import FACTOR, GAP_MIN, NORMALS_FLOOR, normals_reference

SIZES = (4097, 8192, 8193, 16384, 16385)
KS = (1, 2, 7, 8, 15, 16, 31)
PREP_KS = (1, 7, 8, 12, 13, 15, 16, 31)            # prep_big.hip: list widths 8, 13, 16, 32
DUP_N, DUP_KS = 8196, (7, 15, 31)
DECOYS = ((8193, 8192), (12000, 5000))             # (capacity, count)
FAR = np.array([2.0e4, -1.5e4])

# family: largest angle of float64 eigh(np.cov) off the longdouble eigenvector, units of 2^-52 l1 / (l1 - l0)
BIG_TABLE = {
    "uniform": 1.59,
    "columns": 1.64,
    "duplicates": 2.26,
    "ties": 1.96,
}
# share of a cloud's points that may go uncompared for an eigen-gap below GAP_MIN
GAP_SHARE = {"uniform": 0.001, "columns": 0.001, "ties": 0.001, "duplicates": 0.02}


def big_bound(family):
    return max(NORMALS_FLOOR, FACTOR * BIG_TABLE[family])


@functools.lru_cache(maxsize=None)
def uniform(n):
    pts = np.random.default_rng(n).uniform(-4, 4, size=(n, 2))
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def uniform_far(n):
    pts = uniform(n) + FAR
    pts.setflags(write=False)
    return pts


COLUMNS = 64


@functools.lru_cache(maxsize=None)
def columns(n):
    rng = np.random.default_rng(1000003 + n)
    col = rng.permutation(n) % COLUMNS                                  # n // 64 rows of every x, or one more
    pts = np.column_stack([-4.0 + col * 0.125, rng.uniform(-4, 4, size=n)])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def duplicates(n):
    assert n % 4 == 0
    rng = np.random.default_rng(2000003 + n)
    pts = np.repeat(rng.uniform(-4, 4, size=(n // 4, 2)), 4, axis=0)[rng.permutation(n)]
    pts.setflags(write=False)
    return pts


# ── ties ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
GRID = 2.0 ** -10
TIE_PER_K = 40                     # planted queries per k of KS: 280 in all
TIE_HOLE = 64                      # grid steps about a planted query that hold nothing but what is planted
TIE_PITCH = 320                    # grid steps between planted queries: no two holes meet


@functools.lru_cache(maxsize=None)
def ties(n):
    """-> (cloud, planted): planted[k] = int array [TIE_PER_K, 3] of (query row, candidate row a, candidate row b).

    A planted query q for k has k - 1 rows strictly nearer than D, two candidates a = q + (u, v) and b = q + (-v, u) at
    squared distance D^2 = u^2 + v^2 exactly, and no other row within TIE_HOLE > D grid steps: its k + 1 nearest are
    itself, the k - 1 inner rows and ONE of a, b.  Every other query is axis aligned (v = 0): there the gap along the
    sort axis alone equals the k-th best distance when the sweep meets the candidate.  The rows are shuffled, so either
    candidate is the lower row about half of the time."""
    rng = np.random.default_rng(3000003 + n)
    side = 20                                                           # 20 x 14 = 280 holes
    assert side * 14 == TIE_PER_K * len(KS)
    centres = np.array([(-3040 + TIE_PITCH * (i % side), -2080 + TIE_PITCH * (i // side)) for i in range(side * 14)], dtype=np.int64)
    centres = centres[rng.permutation(len(centres))]
    cells, planted_cells = [], {}
    for i, c in enumerate(centres):
        k = KS[i // TIE_PER_K]
        if i % 2 == 0:
            u, v = int(rng.integers(36, 44)), 0
        else:
            u, v = int(rng.integers(30, 40)), int(rng.integers(8, 20))
        if rng.integers(2):
            u, v = -v, u                                                # the pair turned by 90 degrees
        d2 = u * u + v * v
        inner = set()
        while len(inner) < k - 1:
            o = tuple(int(t) for t in rng.integers(-43, 44, size=2))
            if 0 < o[0] * o[0] + o[1] * o[1] < d2:
                inner.add(o)
        group = [(0, 0), (u, v), (-v, u)] + sorted(inner)
        planted_cells.setdefault(k, []).append(len(cells))
        cells += [(int(c[0]) + o[0], int(c[1]) + o[1]) for o in group]
    cells = np.array(cells, dtype=np.int64)
    # the rest: distinct grid cells of [-4, 4]^2 outside every hole
    cand = rng.integers(-4096, 4097, size=(2 * n, 2))
    near = np.stack([-3040 + TIE_PITCH * np.clip(np.rint((cand[:, 0] + 3040) / TIE_PITCH), 0, side - 1),
                     -2080 + TIE_PITCH * np.clip(np.rint((cand[:, 1] + 2080) / TIE_PITCH), 0, 13)], axis=1)
    cand = cand[((cand - near) ** 2).sum(axis=1) > TIE_HOLE ** 2]       # (near: the lattice point nearest to the cell)
    _, first = np.unique(cand, axis=0, return_index=True)
    rest = cand[np.sort(first)][:n - len(cells)]
    assert len(rest) == n - len(cells)
    allc = np.vstack([cells, rest])
    perm = rng.permutation(n)                                           # row r of the cloud = cell perm[r]
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)
    pts = allc[perm].astype(np.float64) * GRID
    planted = {k: np.array([[where[s], where[s + 1], where[s + 2]] for s in starts], dtype=np.int64) for k, starts in planted_cells.items()}
    pts.setflags(write=False)
    return pts, planted


def ties_cloud(n):
    return ties(n)[0]


# ── decoys ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
@functools.lru_cache(maxsize=None)
def decoys(cap, count):
    """-> [cap, 2]: rows 0 .. count - 1 are the cloud; row count + j lies at 1 / 4 (and, once every valid row has one, at
    1 / 8, 1 / 16, ...) of the way from valid row j % count to its nearest valid neighbour's distance, in a random
    direction: nearer to that row than any valid row is."""
    import oracle
    rng = np.random.default_rng(4000003 + cap)
    valid = rng.uniform(-4, 4, size=(count, 2))
    d2, _ = oracle.knn(valid, valid, 2)
    nearest = np.sqrt(d2[:, 1])
    assert (nearest > 0).all()
    j = np.arange(cap - count)
    ang = rng.uniform(0, 2 * np.pi, size=len(j))
    reach = nearest[j % count] * 0.25 / 2.0 ** (j // count)
    pts = np.vstack([valid, valid[j % count] + reach[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])])
    pts.setflags(write=False)
    return pts


# ── the cases and their references ───────────────────────────────────────────────────────────────────────────────────────────
CLOUDS = {"uniform": uniform, "uniform_far": uniform_far, "columns": columns, "duplicates": duplicates, "ties": ties_cloud}
FAMILY = {"uniform": "uniform", "uniform_far": "uniform", "columns": "columns", "duplicates": "duplicates", "ties": "ties",
          "decoys": "uniform"}


def cloud(name, n):
    """The rows a kernel is to work on: for ("decoys", (cap, count)) the counted rows."""
    if name == "decoys":
        return decoys(*n)[:n[1]]
    return CLOUDS[name](n)


def all_cases():
    """(name, n, ks) of everything either GPU route runs, for the table."""
    every = tuple(sorted(set(KS) | set(PREP_KS)))
    out = [("uniform", n, every) for n in SIZES]
    out += [(name, n, every) for name in ("uniform_far", "columns", "ties") for n in (8193, 16385)]
    out += [("duplicates", DUP_N, DUP_KS)]
    out += [("decoys", pair, (7, 16)) for pair in DECOYS]
    return out


@functools.lru_cache(maxsize=None)
def reference(name, n, k):
    """normals_reference of cloud(name, n): (longdouble unit eigenvectors, relative eigen-gaps, neighbour rows); computed
    once and shared, never written to."""
    ref, gap, nb = normals_reference(cloud(name, n), k)
    for a in (ref, gap, nb):
        a.setflags(write=False)
    return ref, gap, nb


def normals_of_sets(pts, nb):
    """The unit eigenvector of the smaller eigenvalue of the np.longdouble covariance of pts[nb[i]] for every i: the
    arithmetic of normals_reference on neighbour sets of the caller's choosing (a wrong one, to see what it costs)."""
    LD = np.longdouble
    pts = np.asarray(pts, dtype=np.float64)
    d = pts[nb].astype(LD) - pts[nb[:, 0]][:, None, :].astype(LD)
    d = d - d.mean(axis=1, keepdims=True)
    a, b, c = (d[..., 0] ** 2).sum(1), (d[..., 0] * d[..., 1]).sum(1), (d[..., 1] ** 2).sum(1)
    phi = 0.5 * np.arctan2(2 * b, a - c)
    return np.stack([-np.sin(phi), np.cos(phi)], axis=1)


def compared(name, n, k):
    """The points whose normal has a direction to compare: eigen-gap at least GAP_MIN."""
    return reference(name, n, k)[1] >= GAP_MIN
