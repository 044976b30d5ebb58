"""NumPy restatement of the particle filter's global start and recovery in include/icpmi.h (icpmi_pf_free_index,
icpmi_pf_draw_uniform): the bit planes of a field and the free index of planes inside a cell box, formed cell by cell from
boolean arrays (not word by word, as the device forms them); the slots of a draw; the draw itself in float64 with every
operation rounded on its own; injection on top of tests/particles_ref.py's resampling; the host's ``Recovery``; and the
restated filter of tests/particles_ref.py with ``init_uniform`` and ``resample(inject=)``.  The CPU suite holds it to literal
values and to a kidnapped robot in the room map, the GPU suite compares the device with it bit for bit
(tests/test_particles_global_cpu.py, tests/test_particles_global_gpu.py).  It uses nothing of the library."""
import math

import numpy as np

import particles_ref as ref

PURPOSE_UNIFORM, FREE_HEADER, FREE_BLOCK, FREE_MAX_WORDS, INJECTED, ST_NO_FREE = 2, 64, 4096, 2 ** 22, -1, 2
TWO_PI = 2.0 * math.pi


# ── planes and the free index ────────────────────────────────────────────────
def pack_rows(cells):
    """Boolean (ny, nx) -> uint32 (ny, wpr): bit x & 31 of word x >> 5 of row y is cell (y, x); the pad bits are clear."""
    ny, nx = cells.shape
    wpr = (nx + 31) // 32
    padded = np.zeros((ny, wpr * 32), dtype=np.uint64)
    padded[:, :nx] = cells
    return (padded.reshape(ny, wpr, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def planes_of(field, threshold):
    """-> (occupied, unknown) uint32 (ny, wpr) of an int16 field: field >= threshold, field == 0."""
    field = np.asarray(field)
    return pack_rows(field >= threshold), pack_rows(field == 0)


def unpack_rows(words, nx):
    """uint32 (ny, wpr) -> boolean (ny, nx); a set pad bit is an error of the caller's."""
    ny, wpr = words.shape
    bits = ((words[:, :, None].astype(np.uint64) >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(ny, wpr * 32)
    assert not bits[:, nx:].any(), "a pad bit is set"
    return bits[:, :nx]


def index_bytes(ny, nx):
    """icpmi_pf_free_index_bytes: the header, free, rank and the build's block sums, each rounded up to 256 bytes."""
    words = ny * ((nx + 31) // 32)
    a = lambda v: (v + 255) // 256 * 256                       # noqa: E731
    return a(4 * FREE_HEADER) + 2 * a(4 * words) + a(4 * ((words + FREE_BLOCK - 1) // FREE_BLOCK))


def free_index(occupied, unknown, nx, box=None):
    """-> (header uint32 [FREE_HEADER], free uint32 [words], rank uint32 [words]) of planes (ny, wpr) inside the cell box
    (x0, y0, x1, y1), half-open and clipped to the grid (None: the whole grid)."""
    ny, wpr = occupied.shape
    free = ~unpack_rows(occupied, nx) & ~unpack_rows(unknown, nx)
    x0, y0, x1, y1 = (0, 0, nx, ny) if box is None else box
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, nx), min(y1, ny)
    inside = np.zeros((ny, nx), dtype=bool)
    if x1 > x0 and y1 > y0:
        inside[y0:y1, x0:x1] = True
    free &= inside
    padded = np.zeros((ny, wpr * 32), dtype=np.int64)
    padded[:, :nx] = free
    counts = padded.reshape(ny * wpr, 32).sum(axis=1)
    rank = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else np.zeros(0, dtype=np.int64)
    header = np.zeros(FREE_HEADER, dtype=np.uint32)
    header[:3] = int(counts.sum()), ny * wpr, wpr
    return header, pack_rows(free).reshape(-1), rank.astype(np.uint32)


def box_cells(box, min_x, min_y, res):
    """A box (x_lo, y_lo, x_hi, y_hi) in metres as cells by world_to_cell: floor((w - min) / res)."""
    cell = lambda w, mn: int(np.floor((np.float64(w) - np.float64(mn)) / np.float64(res)))      # noqa: E731
    return cell(box[0], min_x), cell(box[1], min_y), cell(box[2], min_x), cell(box[3], min_y)


# ── the slots, the draw ──────────────────────────────────────────────────────
def slots_ints(n, m):
    """Boolean [n]: slot j is drawn iff ((j + 1) m) div n > (j m) div n — Python integers."""
    return np.array([((j + 1) * m) // n > (j * m) // n for j in range(n)], dtype=bool)


def slots(n, m):
    """``slots_ints`` in uint64 arrays (n m < 2^64 for every n and m a draw can have)."""
    jm = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)
    return jm[1:] // np.uint64(n) > jm[:-1] // np.uint64(n)


def k_of(r0, F):
    """(uint64(r0) * F) >> 32"""
    return (np.asarray(r0, dtype=np.uint64) * np.uint64(F)) >> np.uint64(32)


def cell_of(k, free, rank, wpr):
    """-> (cx, cy, J) of free-cell numbers k (int64 arrays): J the largest word with rank[J] <= k, the (k - rank[J])-th set
    bit of free[J] counted from bit 0."""
    k = np.asarray(k, dtype=np.int64)
    J = np.searchsorted(rank.astype(np.int64), k, side="right") - 1
    fw, skip = free[J].astype(np.int64), k - rank[J].astype(np.int64)
    for s in range(32):
        fw = np.where(s < skip, fw & (fw - 1), fw)
    assert (fw != 0).all(), "k is not below F"
    bit = np.log2((fw & -fw).astype(np.float64)).astype(np.int64)
    return 32 * (J % wpr) + bit, J // wpr, J


def draw_uniform(index, n, m, min_x, min_y, res, theta0, span, seed, step):
    """icpmi_pf_draw_uniform -> (drawn boolean [n], pair_t (m, 2), theta (m,), cells (m, 2) int64 [cx, cy]) of the drawn slots
    in slot order; nothing is drawn (m rows of nothing: None) where the index has no free cell."""
    header, free, rank = index
    F, wpr = int(header[0]), int(header[2])
    drawn = slots(n, m)
    if F == 0:
        return drawn, None, None, None
    r = ref.draw(seed, np.flatnonzero(drawn), 0, step, PURPOSE_UNIFORM)
    cx, cy, _ = cell_of(k_of(r[:, 0], F), free, rank, wpr)
    ux = ((r[:, 1] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    uy = ((r[:, 2] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    min_x, min_y, res, theta0, span = (np.float64(v) for v in (min_x, min_y, res, theta0, span))
    x = min_x + (cx.astype(np.float64) + ux) * res
    y = min_y + (cy.astype(np.float64) + uy) * res
    theta = theta0 + ((r[:, 3].astype(np.float64) + 0.5) * 2.0 ** -32 - 0.5) * span
    return drawn, np.stack([x, y], axis=1), theta, np.stack([cx, cy], axis=1)


def inject(state, ancestors, index, m, min_x, min_y, res, theta0, span, seed, step):
    """The draw of m slots on top of a resampled generation ``state`` = (pair_t, theta, cos_sin) with its ``ancestors``
    -> (pair_t, theta, drawn, ancestors): cos_sin is the device library's and is not restated."""
    pair_t, theta, anc = state[0].copy(), state[1].copy(), np.array(ancestors, dtype=np.int32)
    drawn, new_t, new_theta, _ = draw_uniform(index, len(theta), m, min_x, min_y, res, theta0, span, seed, step)
    if new_t is not None:
        pair_t[drawn], theta[drawn], anc[drawn] = new_t, new_theta, INJECTED
    return pair_t, theta, drawn, anc


# ── the policy ───────────────────────────────────────────────────────────────
class Recovery:
    """icpmi.particles.Recovery restated: q = exp(s_max / (scale rows)), two running averages, max(0, 1 - fast / slow)."""

    def __init__(self, alpha_slow=0.05, alpha_fast=0.6, scale=1024):
        self.alpha_slow, self.alpha_fast, self.scale, self.w_slow, self.w_fast = alpha_slow, alpha_fast, float(scale), None, None

    def update(self, s_max, rows):
        q = 0.0 if int(s_max) == ref.NO_SCORE or rows <= 0 else math.exp(int(s_max) / (self.scale * int(rows)))
        if self.w_slow is None:
            self.w_slow = self.w_fast = q
        else:
            self.w_slow += self.alpha_slow * (q - self.w_slow)
            self.w_fast += self.alpha_fast * (q - self.w_fast)
        return max(0.0, 1.0 - self.w_fast / self.w_slow) if self.w_slow > 0.0 else 0.0


# ── the filter ───────────────────────────────────────────────────────────────
class Filter(ref.Filter):
    """tests/particles_ref.py's filter with a start over the free cells and injection at a resampling."""

    def free_index(self, box=None):
        field, threshold, min_x, min_y, res = self.map
        cells = None if box is None else box_cells(box, min_x, min_y, res)
        if not hasattr(self, "_free"):
            self._free = {}
        if cells not in self._free:
            self._free[cells] = free_index(*planes_of(field, threshold), field.shape[1], cells)
        return self._free[cells]

    def _draw(self, m, box, heading, span):
        _, _, min_x, min_y, res = self.map
        return draw_uniform(self.free_index(box), self.n, m, min_x, min_y, res, 0.0 if heading is None else heading, span, self.seed, self.step)

    def init_uniform(self, box=None, heading=None, span=TWO_PI):
        drawn, pair_t, theta, _ = self._draw(self.n, box, heading, span)
        if pair_t is None:
            raise ValueError("no free cell")
        self.pair_t, self.theta = pair_t, theta
        self.cos_sin = np.stack([np.cos(theta), np.sin(theta)], axis=1)
        self.w = np.ones(self.n, dtype=np.uint32)
        self.step += 1

    def resample(self, inject=0, box=None, heading=None, span=TWO_PI):
        anc, _, status = ref.resample(self.w, self.seed, self.step)
        self.pair_t, self.theta, self.cos_sin = self.pair_t[anc], self.theta[anc], self.cos_sin[anc]
        if inject:
            drawn, pair_t, theta, _ = self._draw(inject, box, heading, span)
            if pair_t is not None:
                anc = anc.copy()
                self.pair_t[drawn], self.theta[drawn], anc[drawn] = pair_t, theta, INJECTED
                self.cos_sin[drawn] = np.stack([np.cos(theta), np.sin(theta)], axis=1)
        self.step += 1
        self.w = np.ones(self.n, dtype=np.uint32)
        return anc, status

    def maybe_resample(self, ess, rows, threshold=0.5, recovery=None, **region):
        """-> the slots injected, or None where the filter did not resample."""
        m = int(recovery.update(int(self.sums[ref.SUM_SMAX]), rows) * self.n) if recovery is not None else 0
        if not (ess < threshold * self.n or m > 0):
            return None
        self.resample(inject=m, **region)
        return m
