"""The nearest-neighbour kernels' reference and cases (csrc/nn.hip, csrc/nn_sweep.hip), shared by test_nn_shapes_cpu.py and
test_nn_shapes_gpu.py.  NumPy only: no GPU, no torch.

The reference restates the operation, not the kernel: d2 = (sx-tx)*(sx-tx) + (sy-ty)*(sy-ty) [+ (sz-tz)*(sz-tz)], added
in axis order in float64, the lowest row among the smallest d2, sqrt of the winner, and the second-smallest d2 of a row
(counted with multiplicity: a duplicate of the winner is the second) for the sweep's third output.

The cases.  Every target cloud of a dimension is built round the same PLANTED points, which lie far from the generic
rows (a lattice in [1, side]^dim) and from each other, so one set of query points meets the planted rows of every target
whatever its size, and a source cloud is the same for every target: a window of one master source (`source`), whose
reference per target is evaluated once (`Cases.answer`).  Launch sizes are not restated here: the source sizes are taken
against the rows per workgroup the library's own plan reports (`source_sizes`).
"""
import numpy as np

CHUNK_ROWS = (15, 16)                  # a duplicated point across the border of two 16-row chunks
TARGET_SIZES = {2: (1, 15, 16, 17, 33, 2047, 2048, 2049, 4097, 4102), 3: (1, 16, 17, 33, 1359, 1360, 1361, 2721)}
SWEEP_MAX_ROWS = 4096                  # the sweep's limit on a prepared target (icpmi_nn_prepared_batch: UNSUPPORTED beyond)
MASTER_ROWS = 2560                     # rows of the master source: above any source a test takes a window of
IDX_SENTINEL, DIST_SENTINEL = -77, -123.25      # what the out buffers hold before a call: neither is ever an answer


MANY_PAIRS = 2 ** 30                   # a batch large enough for the largest rows per lane whatever the thresholds


def plan(L, n_pairs, max_src_n, dim=2):
    """icpmi_nn_batch_plan of the loaded library L: what icpmi_nn_batch starts for these arguments (no HIP call)."""
    import ctypes
    from icpmi import _lib
    p = _lib.NnPlan()
    code = L.icpmi_nn_batch_plan(n_pairs, max_src_n, dim, ctypes.byref(p))
    assert code == _lib.OK, code
    return p


def first_pairs_with(L, rows_per_lane, max_src_n, dim=2):
    """The smallest n_pairs whose plan has at least that many rows per lane, by bisection (the rule is monotone in
    n_pairs): the thresholds are read off the library, not restated."""
    lo, hi = 0, MANY_PAIRS                                            # lo: fewer rows per lane, hi: enough
    assert plan(L, hi, max_src_n, dim).rows_per_lane >= rows_per_lane
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(L, mid, max_src_n, dim).rows_per_lane >= rows_per_lane:
            hi = mid
        else:
            lo = mid
    return hi


def reference(src, tgt):
    """(idx int32, dist, second_d2) of every row of src in tgt; an empty target gives (-1, +inf, +inf)."""
    s, t = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    n, m = len(s), len(t)
    idx, best, second = np.full(n, -1, dtype=np.int32), np.full(n, np.inf), np.full(n, np.inf)
    if m == 0:
        return idx, best, second
    for r0 in range(0, n, 256):                                       # blocks of rows: the (n, m) table stays small
        blk = s[r0:r0 + 256]
        d2 = np.zeros((len(blk), m))
        for a in range(s.shape[1]):                                   # axis order, multiply and add separate
            diff = blk[:, a, None] - t[None, :, a]
            d2 = d2 + diff * diff
        j = np.argmin(d2, axis=1)                                     # the first occurrence: the lowest row
        idx[r0:r0 + 256] = j
        best[r0:r0 + 256] = d2[np.arange(len(blk)), j]
        if m > 1:
            second[r0:r0 + 256] = np.partition(d2, 1, axis=1)[:, 1]
    return idx, np.sqrt(best), second


# ── planted points ──────────────────────────────────────────────────────────────────────────────────────────────────
# Sites lie on the diagonal at 1000, 1100, ...: 100 apart, and hundreds from the generic rows, so a query at a site
# has its nearest rows among that site's planted ones in every target that holds them (and some generic or other
# planted row otherwise: the reference decides, the case stays a case).
def _site(k, dim):
    return np.full(dim, 1000.0 + 100.0 * k)


def _axis(dim, a, v):
    e = np.zeros(dim)
    e[a] = v
    return e


def tile_rows(dim):
    """Target rows per LDS tile as the tests plant them: the test modules check this against the plan's tile_points."""
    return 2048 if dim == 2 else 1360


def planted(dim, m):
    """{row: point} of a target of m rows (rows >= m left out).  T = rows per LDS tile."""
    T = tile_rows(dim)
    rows = {}
    rows[0] = _site(0, dim)                                           # a query beside it: the nearest is row 0
    for r in CHUNK_ROWS:
        rows[r] = _site(1, dim)                                       # the same point in two chunks
    for r in (T - 1, T):
        rows[r] = _site(2, dim)                                       # ... in two tiles
    for r in (5, T + 5, 2 * T + 5 if m > 2 * T + 5 else 2 * T):      # (a cloud that ends before 2T + 5: the third tile's first row)
        rows[r] = _site(3, dim)                                       # ... in three tiles
    rows[14], rows[17] = _site(4, dim) + _axis(dim, 0, 1.0), _site(4, dim) - _axis(dim, 0, 1.0)    # distinct, equidistant, two chunks
    rows[T - 2], rows[T + 1] = _site(5, dim) + _axis(dim, 1, 2.0), _site(5, dim) - _axis(dim, 1, 2.0)    # ... two tiles
    rows[3], rows[9] = _site(6, dim), _site(6, dim)                   # the same point twice inside one chunk
    rows[2], rows[12] = _site(7, dim) + _axis(dim, dim - 1, 3.0), _site(7, dim) - _axis(dim, dim - 1, 3.0)   # equidistant inside one chunk
    rows = {r: p for r, p in rows.items() if r < m}
    # the last row, alone in a padded chunk when m % 16 == 1: a point of its own (m = 33: the only minimum of its query)
    # unless a duplicate above sits there already (m = 17, T + 1, 2T + 1: the query on that site ties with an earlier row)
    if m > 0:
        rows.setdefault(m - 1, _site(8, dim))
    return rows


def queries(dim):
    """The query points that meet the planted rows: on every site and beside it, and beside the origin, where the rows a
    kernel pads a chunk with would lie if it padded with zeros (the generic rows keep off it)."""
    q = []
    for k in range(9):
        q += [_site(k, dim), _site(k, dim) + _axis(dim, 0, 0.25), _site(k, dim) - _axis(dim, dim - 1, 0.125)]
    q += [np.full(dim, 0.125), np.zeros(dim), _axis(dim, 0, -0.5)]
    return np.array(q)


def target(dim, m, seed=0):
    """A target of m rows: generic rows in [1, side]^dim — half of them lattice points (duplicates and equidistant rows
    everywhere, in shuffled row order), half real —, then the planted rows."""
    rng = np.random.default_rng(1000 * dim + 7 * m + seed)
    side = int(np.ceil(max(m, 1) ** (1.0 / dim))) + 2
    t = rng.integers(1, side + 1, size=(m, dim)).astype(np.float64)
    real = rng.random(m) < 0.5
    t[real] = rng.uniform(1.0, side, size=(int(real.sum()), dim))
    for r, p in planted(dim, m).items():
        t[r] = p
    return t


def master_source(dim):
    """MASTER_ROWS query rows: every fourth a planted query (in turn), the others spread over the boxes of all targets —
    lattice points (on a target: distance 0; several rows hold it), lattice points + 0.5 (four- or eight-way ties) and
    real points."""
    rng = np.random.default_rng(50 + dim)
    q = queries(dim)
    s = np.empty((MASTER_ROWS, dim))
    for i in range(MASTER_ROWS):
        side = (3, 6, 19, 47, 67)[rng.integers(0, 5)] if dim == 2 else (3, 5, 8, 13, 16)[rng.integers(0, 5)]
        kind = i % 4
        if kind == 0:
            s[i] = q[(i // 4) % len(q)]
        elif kind == 1:
            s[i] = rng.integers(1, side + 1, size=dim)
        elif kind == 2:
            s[i] = rng.integers(1, side + 1, size=dim) + 0.5
        else:
            s[i] = rng.uniform(0.0, side + 1.0, size=dim)
    return s


def lattice_case(seed=3):
    """A 50 x 50 integer lattice in shuffled row order, queried at +0.5: four-way ties everywhere, and the lowest ROW is
    not the first in any spatial order."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(50.0), np.arange(50.0), indexing="ij"), axis=-1).reshape(-1, 2)
    t = g[rng.permutation(len(g))]
    s = rng.integers(0, 49, size=(600, 2)) + 0.5                      # the centre of a cell with all four corners in the lattice
    return s, t


def source_sizes(rows_per_wg, threads):
    """Source sizes against the plan's rows per workgroup W and threads per workgroup: the borders of one row slot and of
    one workgroup, every number of row slots k = 1 .. W / threads a ragged last tile can hold (N mod W in
    (threads (k-1), threads k]) on the first and on the second tile, and two full tiles."""
    W, th = rows_per_wg, threads
    sizes = {1, th - 1, th, th + 1, W - 1, W, W + 1, 2 * W}
    for k in range(1, W // th + 1):
        for tile in (0, 1):
            sizes.add(tile * W + th * (k - 1) + 1 + (53 * k + 101 * tile) % (th - 1))     # N mod W in [th (k-1) + 1, th k - 1]
    return sorted(sizes)


def slots_reached(n, rows_per_wg, threads):
    """{(tile is the first, rows per lane of that tile)} over the workgroups a source of n rows keeps busy."""
    out = set()
    for first in range(0, n, rows_per_wg):
        out.add((first == 0, min(rows_per_wg // threads, -(-(n - first) // threads))))
    return out


class Cases:
    """The clouds of one dimension and their answers.  ``source(n, k)``: n rows of the master source from row 97 k on
    (cyclic), so that no two source clouds of a set start alike; ``answer(m, n, k)``: the reference of that source in
    ``target(m)`` — one evaluation per target, on the master source."""

    def __init__(self, dim):
        self.dim = dim
        self.master = master_source(dim)
        self._targets, self._answers = {}, {}

    def rows(self, n, k):
        assert n <= MASTER_ROWS
        return (97 * k + np.arange(n)) % MASTER_ROWS

    def source(self, n, k=0):
        return self.master[self.rows(n, k)]

    def target(self, m):
        if m not in self._targets:
            self._targets[m] = target(self.dim, m)
        return self._targets[m]

    def answer(self, m, n, k=0):
        if m not in self._answers:
            self._answers[m] = reference(self.master, self.target(m))
        r = self.rows(n, k)
        return tuple(a[r] for a in self._answers[m])


_cases = {}


def cases(dim):
    if dim not in _cases:
        _cases[dim] = Cases(dim)
    return _cases[dim]


def decoy_set(dim, seed=9):
    """Clouds whose capacity exceeds their count.  Targets: ``cnt`` valid rows, then decoy rows that are nearer to every
    source row than any valid one (the valid rows lie beyond 50, decoys and sources within [0, 4]).  Sources: ``cnt``
    rows, then rows behind the count (the same kind of point).  -> (clouds at capacity, cnt, source ids, target ids)."""
    rng = np.random.default_rng(seed + dim)
    clouds, cnt, src_ids, tgt_ids = [], [], [], []
    for n, cap in ((1, 4), (200, 300), (256, 257), (300, 700)):
        src_ids.append(len(clouds))
        clouds.append(rng.uniform(0.0, 4.0, size=(cap, dim)))
        cnt.append(n)
    for m, cap in ((1, 2), (16, 17), (17, 40), (700, 1500)):
        tgt_ids.append(len(clouds))
        t = rng.uniform(50.0, 60.0, size=(cap, dim))
        t[m:] = rng.uniform(0.0, 4.0, size=(cap - m, dim))
        clouds.append(t)
        cnt.append(m)
    return clouds, np.array(cnt, dtype=np.int32), src_ids, tgt_ids
