"""Inputs of the ray-cast edge suites (csrc/raycast.hip), built by construction — TEST INFRASTRUCTURE ONLY.

tests/test_raycast_edges_cpu.py proves on the project's C oracle alone (oracle.grid_update_scan: the reference's loop, cell by
cell in int64) that every family has the property its GPU test relies on and takes the pass it is meant for;
tests/test_raycast_edges_gpu.py runs the library on the same inputs under its three counting passes.  Nothing here touches a
GPU, and nothing but ``apply_counts`` restates device code: the expected grids are the oracle's.

A grid is a ``Grid`` (name, minimum, cells, resolution; the maximum is put half a cell inside the last cell, so that
ceil((max - min) / res) is the cell count whatever the rounding of the quotient).  A scan is a ``Scan``: a name, an origin and
hits in WORLD coordinates.  Beams are built in cell space and converted with min + (cell + 0.5) * res — ``cells_of`` gives the
cells back through oracle.world_to_grid, and the CPU test asserts that they are the ones meant.

Families ("Edge tests" under K6/K7):
  A  ``border_cases``   hits on cell borders, where floor((w - min) * (1 / res)) and floor((w - min) / res) differ
  B  ``long_cases``     beams of 1 000 ... 2^29 cells: leaving the grid, crossing it from far outside, grazing it and its tiles
  C  ``clamp_case``     coordinates beyond +-2^29 cells (clamped) and quotients >= 1e300 (dropped)
  D  ``counter_cases``  65 535 / 65 536 / 65 537 beams through one cell: the limit of a packed 16-bit counter
  E  ``replay_cases``   the H / M replay on start values, clamps and probabilities that reach each of its exits
"""
import collections
import functools
import math

import numpy as np

import oracle

LIM = 2 ** 29                          # RC_COORD_MAX: cell indices are clamped to +-2^29
RC_WIDE = 65535                        # beams a packed 16-bit counter holds; more take the two-round route
DROP_QUOTIENT = 1e300                  # |floor((w - min) / res)| not below this: the beam is dropped

Grid = collections.namedtuple("Grid", "name min_x min_y nx ny res")
Scan = collections.namedtuple("Scan", "name origin hits")          # origin (2,), hits (n, 2): float64 world coordinates
Case = collections.namedtuple("Case", "name grid scans kw")        # kw: p_hit, p_miss, log_odds_min, log_odds_max


def bounds(g):
    """(min_x, max_x, min_y, max_y) for OccupancyGrid2D: exactly g.nx x g.ny cells"""
    return (g.min_x, g.min_x + (g.nx - 0.5) * g.res, g.min_y, g.min_y + (g.ny - 0.5) * g.res)


def shape(g):
    """(ny, nx) as the class computes them (mapping.py:44-45)"""
    b = bounds(g)
    return int(np.ceil((b[3] - b[2]) / g.res)), int(np.ceil((b[1] - b[0]) / g.res))


DEFAULT = Grid("default", 0.0, 0.0, 200, 150, 0.05)                # 4 x 3 tiles, neither extent a multiple of 64
OFFSET = Grid("offset", 500000.37, 5000000.11, 200, 150, 0.05)
SLIVER_X = Grid("sliver_130x1", 0.0, 0.0, 130, 1, 0.05)
SLIVER_Y = Grid("sliver_1x130", 0.0, 0.0, 1, 130, 0.05)
KW = dict(p_hit=0.55, p_miss=0.49, log_odds_min=-200.0, log_odds_max=200.0)     # no cell of A - C comes near a clamp: every count shows


def l_of(p):
    return np.log(p / (1.0 - p))                                   # mapping.py:49-50


def world(g, cx, cy):
    """centres of the cells (cx, cy) -> (n, 2) world rows"""
    cx, cy = np.asarray(cx, dtype=np.float64), np.asarray(cy, dtype=np.float64)
    return np.stack([g.min_x + (cx + 0.5) * g.res, g.min_y + (cy + 0.5) * g.res], axis=-1)


def cells_of(g, rows):
    """(n, 2) int64 cells of world rows: the oracle's floor((w - min) / res)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    return np.stack([oracle.world_to_grid(rows[:, 0], g.min_x, g.res), oracle.world_to_grid(rows[:, 1], g.min_y, g.res)], axis=1)


def cells_by_reciprocal(g, rows):
    """WRONG MODEL: the same index with one multiplication by 1 / res and no second look near an integer"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    rinv = 1.0 / g.res
    return np.stack([np.floor((rows[:, 0] - g.min_x) * rinv), np.floor((rows[:, 1] - g.min_y) * rinv)], axis=1).astype(np.int64)


def expected(case, start=None, snapshots=False):
    """The oracle's grid after the scans of ``case`` in order, from ``start`` (zeros) -> (ny, nx) float32, or one per scan."""
    case = ruled(case)                                             # C's rule; every other scan passes through unchanged
    g = case.grid
    ref = np.zeros((g.ny, g.nx), dtype=np.float32) if start is None else np.array(start, dtype=np.float32)
    out = []
    for s in case.scans:
        if len(s.hits):
            oracle.grid_update_scan(ref, g.min_x, g.min_y, g.res, s.origin, s.hits, l_of(case.kw["p_hit"]), l_of(case.kw["p_miss"]),
                                    case.kw["log_odds_min"], case.kw["log_odds_max"])
        out.append(ref.copy())
    return out if snapshots else ref


# ── A: borders ──────────────────────────────────────────────────────────────────────────────────────────────────────────
BORDER_RES = (0.05, 0.1, 0.03, 1.0 / 3.0, 0.07, 0.25)
BORDER_NX, BORDER_NY = 40, 30                                      # a beam is at most about 20 cells


TINY = np.array([-0.0, 0.0, 5e-324, -5e-324, 1e-290, -1e-290])     # relative to min: cell 0 for -0.0 and above, cell -1 below


def border_values(mn, res, n):
    """the five constructions of a border coordinate, for every k from -2 to n + 2 -> (5 * (n + 5),) float64"""
    k = np.arange(-2, n + 3, dtype=np.float64)
    b = mn + k * res
    return np.concatenate([b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), (k * res) + mn, mn + (k + 1.0) * res - res])


def border_grid(res):
    """minimum 0 — where the tiny coordinates below do not vanish in w - min — but for 0.07, which has more such borders elsewhere"""
    return Grid(f"border_{res:.4g}", -12.3 if res == 0.07 else 0.0, 3.7 if res == 0.07 else 0.0, BORDER_NX, BORDER_NY, res)


@functools.lru_cache(maxsize=None)
def border_case(res):
    """Two scans — the origin at a cell centre, then exactly on a cell corner — whose hits have a border coordinate on BOTH
    axes: every x construction paired with four y constructions that move over the grid, and the other way round; and the
    coordinates a rounding cannot see: min itself, -0.0, +-5e-324 and +-1e-290 away from it."""
    g = border_grid(res)
    bx, by = border_values(g.min_x, res, g.nx), border_values(g.min_y, res, g.ny)
    i, j = np.arange(len(bx)), np.arange(len(by))
    hx = np.concatenate([np.repeat(bx, 4), bx[(j[:, None] * 5 + np.array([3, 41, 97, 160])).ravel() % len(bx)]])
    hy = np.concatenate([by[(i[:, None] * 7 + np.array([1, 29, 83, 131])).ravel() % len(by)], np.repeat(by, 4)])
    mid = world(g, g.nx // 3, g.ny // 3)
    tx, ty = (TINY if g.min_x == 0.0 else g.min_x + TINY), (TINY if g.min_y == 0.0 else g.min_y + TINY)     # 0.0 + -0.0 is +0.0
    hx = np.concatenate([hx, tx, np.full(len(TINY), mid[0]), tx])
    hy = np.concatenate([hy, np.full(len(TINY), mid[1]), ty, ty[::-1]])
    hits = np.stack([hx, hy], axis=1)
    corner = np.array([g.min_x + (g.nx // 2) * res, g.min_y + (g.ny // 2) * res])
    return Case(g.name, g, (Scan("centre", world(g, g.nx // 2, g.ny // 2), hits), Scan("corner", corner, hits[::-1].copy())), KW)


def border_cases():
    return [border_case(r) for r in BORDER_RES]


# ── B: long beams ───────────────────────────────────────────────────────────────────────────────────────────────────────
LENGTHS = (1000, 65537, 10 ** 6, 2 * 10 ** 7, 4 * 10 ** 8 - 3, 4 * 10 ** 8 + 3)        # and 2^29 - 1 - origin cell
OCTANTS = ((1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))   # (sign major, sign minor, y major)
WALK_BUDGET = 9 * 10 ** 9              # cells the oracle walks in ONE pass over every scan of B and C (about 0.7 s per 2^29)


def minors(dmaj):
    """minor lengths of a beam of dmaj cells: none, one tie in the middle, one short of the diagonal, the diagonal, coprimes"""
    m = [0, 1, dmaj - 1, dmaj]
    for c in (dmaj * 3 // 7, dmaj * 5 // 11):
        while math.gcd(c, dmaj) != 1:
            c += 1
        m.append(c)
    return m


def _beam(o, dmaj, dmin, octant):
    sm, sn, ymaj = octant
    d = (sn * dmin, sm * dmaj) if ymaj else (sm * dmaj, sn * dmin)
    return (o[0] + d[0], o[1] + d[1])


def inside_scan(g, o):
    """(i) origin inside, the beam leaves: every length, every minor length; all octants for the two shortest lengths, four
    for the others — for the lengths from 4e8 on (half a second of oracle a beam) one beam an octant."""
    hits = []
    for n, dmaj in enumerate(LENGTHS):
        if dmaj <= 65537:
            hits += [_beam(o, dmaj, dmin, oc) for dmin in minors(dmaj) for oc in OCTANTS]
        elif dmaj <= 2 * 10 ** 7:
            hits += [_beam(o, dmaj, dmin, OCTANTS[(2 * k + n) % 8]) for k, dmin in enumerate(minors(dmaj))]
            hits += [_beam(o, dmaj, dmin, OCTANTS[(2 * k + n + 3) % 8]) for k, dmin in enumerate(minors(dmaj)[:4])]
        else:
            ms = minors(dmaj)
            ms = (ms[1], ms[2], ms[4], ms[5])
            hits += [_beam(o, dmaj, ms[(k + n) % 4], OCTANTS[(2 * k + n) % 8]) for k in range(4)]
    # 2^29 - 1 - (origin cell) to the last cell that is not clamped, and the same to the other three sides
    hits += [(LIM - 1, o[1] + 1), (o[0] - 1, -(LIM - 1)), (-(LIM - 1), o[1] - 5), (o[0] + 7, LIM - 1)]
    h = np.array(hits, dtype=np.int64)
    return Scan("inside", world(g, o[0], o[1]), world(g, h[:, 0], h[:, 1]))


def _through(o, t):
    """the hit that puts the cell t in the middle of the beam from o: Bresenham passes through t itself"""
    return (2 * t[0] - o[0], 2 * t[1] - o[1])


def outside_scan(g, dist, side):
    """(ii) an origin ``dist`` cells outside, on one of four sides and off the axes: beams through a lattice of cells of the grid
    (its corners and edges among them) to as far beyond it -> (origin cell, hit cells)"""
    nx, ny = g.nx, g.ny
    o = {0: (-dist, ny // 3), 1: (nx - 1 + dist, ny - 1 + dist * 3 // 7), 2: (nx // 2 - dist * 2 // 5, -dist), 3: (nx // 4 + dist // 9, ny - 1 + dist)}[side]
    targets = [(x, y) for x in sorted({0, nx // 7, nx // 2, nx - 1}) for y in sorted({0, ny // 3, ny - 1})]
    hits = [_through(o, t) for t in targets]
    return o, hits


def corner_scan(g, dist, ratio, corners):
    """(iii) - (v) beams through the cells on and just off the diagonal of corners that look the same way (sx, sy) — of the grid, of
    64 x 64 tiles, of 8 x 8 and 16 x 16 pieces — from c + (sx * dist, -sy * ratio * dist) for the first corner c: they come in
    across its diagonal and leave on the other side.  The oracle's walk sorts them into grazers, near misses and the rest
    (``classify``) -> (origin cell, hit cells)"""
    sx, sy = corners[0][2], corners[0][3]
    c0 = corners[0]
    o = (c0[0] + sx * dist, c0[1] - sy * int(ratio * dist))
    hits = []
    for cx, cy, _, _ in corners:
        for j in (0, 1, 2, 3):
            for ax, ay in ((1, 1), (1, 0), (0, 1), (2, 1)):
                hits.append(_through(o, (cx + sx * j * ax, cy + sy * j * ay)))
    return o, hits


def _scan_of(g, name, o, hits):
    h = np.array(hits, dtype=np.int64)
    return Scan(name, world(g, o[0], o[1]), world(g, h[:, 0], h[:, 1]))


@functools.lru_cache(maxsize=None)
def long_case(gname):
    g = {"default": DEFAULT, "offset": OFFSET, "sliver_130x1": SLIVER_X, "sliver_1x130": SLIVER_Y}[gname]
    nx, ny = g.nx, g.ny
    scans = []
    if g is DEFAULT:
        scans.append(inside_scan(g, (77, 41)))
    else:
        h = np.array([_beam((nx // 2, ny // 2), d, m, oc) for d in (1000, 65537) for m in minors(d) for oc in OCTANTS], dtype=np.int64)
        scans.append(Scan("inside", world(g, nx // 2, ny // 2), world(g, h[:, 0], h[:, 1])))
    dists = (10 ** 3, 65537, 10 ** 6, 2 * 10 ** 7) if g is DEFAULT else (10 ** 3, 65537, 10 ** 6)
    for n, dist in enumerate(dists):
        o, hits = outside_scan(g, dist, n % 4)
        scans.append(_scan_of(g, f"outside_{dist}", o, hits))
    corner_sets = {(-1, -1): [(0, 0)], (1, -1): [(nx - 1, 0)], (-1, 1): [(0, ny - 1)], (1, 1): [(nx - 1, ny - 1)]}
    for (sx, sy), cs in corner_sets.items():                       # the corners of the tiles and pieces that look the same way
        for t in (8, 16, 64):
            for x in range(t, nx, t):
                for y in range(t, ny, t):
                    if (x // t + y // t) % 5 == 0 and len(cs) < 6:
                        cs.append((x - (sx > 0), y - (sy > 0)))
    for n, ((sx, sy), cs) in enumerate(corner_sets.items()):
        for dist, ratio in ((10 ** 3, 0.37), (65537, 1.0), (10 ** 3, 2.3)):
            o, hits = corner_scan(g, dist, ratio, [(x, y, sx, sy) for x, y in cs])
            scans.append(_scan_of(g, f"corner_{sx}_{sy}_{dist}_{ratio}", o, hits))
    return Case(f"long_{g.name}", g, tuple(scans), KW)


def long_cases():
    return [long_case(n) for n in ("default", "offset", "sliver_130x1", "sliver_1x130")]


def walk_length(case):
    """cells the oracle walks for one pass over the scans of a case (clamped cells: what the device walks too)"""
    total = 0
    for s in case.scans:
        o = np.clip(cells_of(case.grid, s.origin)[0], -LIM, LIM)
        h = np.clip(cells_of(case.grid, keep_finite(case.grid, s.hits)), -LIM, LIM)
        total += int(np.abs(h - o).max(axis=1).sum()) if len(h) else 0
    return total


SUBFAMILIES = ("leaves", "crosses", "grazes", "near_miss", "tile_grazer")


@functools.lru_cache(maxsize=None)
def classify(gname):
    """-> {sub-family: number of beams} for long_case(gname), each beam walked on its own by the oracle, in cell space on the grid
    grown by two cells (l_hit = 0, l_miss = 1, wide clamps: a cell's value is the number of visits).
      leaves       origin inside, the beam leaves the grid                                    (i)
      crosses      origin 10^3 ... 2 * 10^7 cells outside, hit outside, >= 4 cells visited     (ii)
      grazes       1 to 3 cells of the grid visited                                           (iii)
      near_miss    none visited, but a cell of the two-cell margin                            (iv)
      tile_grazer  1 to 3 cells of an aligned 8 x 8, 16 x 16 or 64 x 64 rectangle visited       (v)"""
    case = long_case(gname)
    g = case.grid
    count = dict.fromkeys(SUBFAMILIES, 0)
    for s in case.scans:
        o = cells_of(g, s.origin)[0]
        o_in = 0 <= o[0] < g.nx and 0 <= o[1] < g.ny
        for h in cells_of(g, s.hits):
            grown = np.zeros((g.ny + 4, g.nx + 4), dtype=np.float32)
            oracle.grid_update_scan(grown, 0.0, 0.0, 1.0, (o[0] + 2.5, o[1] + 2.5), [(h[0] + 2.5, h[1] + 2.5)], 0.0, 1.0, -1e9, 1e9)
            inner = grown[2:-2, 2:-2] != 0
            n_in = int(inner.sum())
            h_in = 0 <= h[0] < g.nx and 0 <= h[1] < g.ny
            far = max(abs(int(h[0]) - int(o[0])), abs(int(h[1]) - int(o[1])))
            count["leaves"] += o_in and not h_in
            count["crosses"] += (not o_in) and (not h_in) and n_in >= 4 and far >= 1000
            count["grazes"] += (not o_in) and 1 <= n_in <= 3
            count["near_miss"] += n_in == 0 and bool((grown != 0).any())
            graze = False
            for t in (8, 16, 64):
                pad = np.zeros((-(-g.ny // t) * t, -(-g.nx // t) * t), dtype=np.int64)
                pad[:g.ny, :g.nx] = inner
                per = pad.reshape(pad.shape[0] // t, t, pad.shape[1] // t, t).sum(axis=(1, 3))
                graze |= bool(((per >= 1) & (per <= 3)).any())
            count["tile_grazer"] += graze
    return count


# ── C: beyond the clamp ─────────────────────────────────────────────────────────────────────────────────────────────────
def keep_finite(g, hits):
    """the rows the library keeps: both quotients finite and below 1e300 (raycast.hip: world_to_cell)"""
    hits = np.asarray(hits, dtype=np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.stack([np.floor((hits[:, 0] - g.min_x) / g.res), np.floor((hits[:, 1] - g.min_y) / g.res)], axis=1)
    return hits[(np.abs(q) < DROP_QUOTIENT).all(axis=1)]


def clamped(g, rows):
    """THE RULE: a kept coordinate whose cell lies beyond +-2^29 is the centre of the cell +-2^29; the others as they are"""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 2)
    for a, mn in ((0, g.min_x), (1, g.min_y)):
        q = np.floor((rows[:, a] - mn) / g.res)
        rows[:, a] = np.where(q > LIM, mn + (LIM + 0.5) * g.res, np.where(q < -LIM, mn + (-LIM + 0.5) * g.res, rows[:, a]))
    return rows


BEYOND = LIM + 1000


@functools.lru_cache(maxsize=None)
def clamp_case():
    """near: origin in the grid, three hits beyond the clamp whose clamped cells lie on a diagonal the true line is far from,
    two beams that are dropped (1e301 m and 1.7e308 m: quotients of 2e302 and infinity) and two ordinary ones;
    far: the origin itself beyond the clamp on both axes, two hits in the grid."""
    g = DEFAULT
    h = np.array([(BEYOND, 10 ** 10), (-10 ** 15, -BEYOND), (10 ** 10, -10 ** 15), (150, 149), (3, 100)], dtype=np.float64)
    hits = np.vstack([world(g, h[:, 0], h[:, 1]), [[1e301, 2.0], [3.0, 1.7e308]]])
    near = Scan("near", world(g, 100, 75), hits[[0, 5, 1, 3, 6, 2, 4]])
    far = Scan("far", world(g, BEYOND, 10 ** 10), world(g, [50, 120], [25, 140]))
    return Case("clamp", g, (near, far), KW)


def ruled(c):
    """the same scans as the rule restates them: dropped beams removed, coordinates beyond the clamp replaced"""
    return c._replace(scans=tuple(Scan(s.name, clamped(c.grid, s.origin)[0], clamped(c.grid, keep_finite(c.grid, s.hits))) for s in c.scans))


def clamp_expected_case():
    return ruled(clamp_case())


def replays():
    """Three scans in one update_scans call: the three longest scans of B on the default grid, and the two scans of C with a scan
    of B between them."""
    b, c = long_case("default"), clamp_case()
    by_walk = sorted(range(len(b.scans)), key=lambda i: -walk_length(b._replace(scans=(b.scans[i],))))[:3]
    return [Case("replay_long", b.grid, tuple(b.scans[i] for i in sorted(by_walk)), KW),
            Case("replay_clamp", c.grid, (c.scans[0], b.scans[1], c.scans[1]), KW)]


def unclamped_cells_in_grid(g, o, h, steps=LIM):
    """WRONG MODEL: the cells inside the grid of the Bresenham line between the UNCLAMPED cells o and h (Python integers), cut to
    its first 2^29 steps — by the closed form, over the steps whose major coordinate is inside the grid."""
    dx, dy = abs(h[0] - o[0]), abs(h[1] - o[1])
    sx, sy = (1 if o[0] < h[0] else -1), (1 if o[1] < h[1] else -1)
    xmaj = dx >= dy
    m0, n0, sm, sn = (o[0], o[1], sx, sy) if xmaj else (o[1], o[0], sy, sx)
    dmaj, dmin = (dx, dy) if xmaj else (dy, dx)
    size = g.nx if xmaj else g.ny
    klo, khi = (max(0, -m0), min(dmaj, size - m0)) if sm > 0 else (max(0, m0 - size + 1), min(dmaj, m0 + 1))
    out = set()
    for k in range(klo, min(khi, steps)):
        mj, mn = m0 + sm * k, n0 + sn * ((2 * k * dmin + dmaj - 1) // (2 * dmaj))
        x, y = (mj, mn) if xmaj else (mn, mj)
        if 0 <= x < g.nx and 0 <= y < g.ny:
            out.add((int(x), int(y)))
    return out


# ── D: counter limits ───────────────────────────────────────────────────────────────────────────────────────────────────
COUNTER_KW = dict(p_hit=0.5 + 1e-6, p_miss=0.5 - 1e-6, log_odds_min=-5.0, log_odds_max=5.0)
COUNTER_BEAMS = (65535, 65536, 65537)
COUNTER_ORIGIN, COUNTER_HIT = (100, 70), (104, 70)


def one_cell_scan(g, nb, origin=COUNTER_ORIGIN, hit=COUNTER_HIT, name=None):
    """nb equal beams: every cell from the origin's to the one before the hit's gets M = nb, the hit's cell H = nb"""
    return Scan(name or f"{nb}_beams", world(g, *origin), np.tile(world(g, *hit), (nb, 1)))


def fan_scan(g, seed):
    """100 ordinary beams around the cells of family D, so that the scans in front and behind leave something to add to"""
    k = np.arange(100)
    return Scan(f"fan_{seed}", world(g, 96 + seed, 66), world(g, 90 + (k * 7 + seed) % 23, 60 + (k * 5 + 3 * seed) % 19))


def counter_case(nb):
    return Case(f"counter_{nb}", DEFAULT, (one_cell_scan(DEFAULT, nb),), COUNTER_KW)


def counter_replay_case():
    g = DEFAULT
    return Case("counter_replay", g, (fan_scan(g, 0),) + tuple(one_cell_scan(g, nb) for nb in COUNTER_BEAMS) + (fan_scan(g, 1),), COUNTER_KW)


# ── E: replay arithmetic ────────────────────────────────────────────────────────────────────────────────────────────────
REPLAY_GRID = Grid("replay_8x8", 0.0, 0.0, 8, 8, 0.05)
F32_BIG = 3.4e38
START_VALUES = np.array([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 1e4, -1e4, 1e8, -1e8, F32_BIG, -F32_BIG, np.inf, -np.inf, np.nan],
                        dtype=np.float32)
CLAMPS = ((-5.0, 5.0), (0.5, 3.0), (-1e9, 1e9), (-F32_BIG, F32_BIG))
PROBS = ((0.5, 0.5), (0.5 + 1e-9, 0.5 - 1e-9), (0.7, 0.4), (1.0 - 1e-12, 1e-12), (0.4, 0.6))
# (M, H equal to M, row, shift of the start values, clamps, probabilities): a row of eight cells is crossed, so the shifts and
# rows bring every start value under every kind of count
REPLAY_COMBOS = (
    (1, False, 0, 0, 0, 0), (1, True, 1, 3, 1, 2), (1000, False, 2, 5, 0, 2), (1000, True, 3, 7, 2, 3),
    (65535, False, 4, 0, 2, 1), (65535, True, 5, 9, 3, 3), (65535, False, 6, 11, 0, 4), (1000, True, 7, 2, 3, 0),
    (65535, True, 0, 13, 1, 1), (1000, False, 1, 6, 1, 4), (65535, False, 2, 4, 2, 2), (1, True, 3, 1, 3, 1),
    (65535, True, 4, 8, 0, 0), (1000, False, 6, 14, 2, 4),
)
# One combination more than the lists above give, for the wrong model "saturate without the bound": from a start of 1, 65 535
# adds of l = -4e-6 each round to 67 steps of 2^-24 where the exact add is 67.1 of them, so the cell ends at 0.73829 while the
# exact sum is 0.73786 — a lower clamp of 0.738 lies between: the exact sum is beyond it, the cell is not.
DRIFT_COMBO = (65535, False, 5, 4, (0.738, 3.0), (0.5 + 1e-6, 0.5 - 1e-6))


def replay_start(shift):
    return START_VALUES[(np.arange(64) + shift) % len(START_VALUES)].reshape(8, 8).copy()


def replay_case(combo):
    """-> (Case, start grid).  Beams along row r from cell (0, r): M of them to the cell (7, r) — seven cells get M misses, (7, r) H
    = M hits — and, for "H equal to M", M more to the cell (8, r) outside the grid, which pass over (7, r): H = M there."""
    M, both, row, shift, clamps, probs = combo
    lo, hi = CLAMPS[clamps] if isinstance(clamps, int) else clamps
    p = PROBS[probs] if isinstance(probs, int) else probs
    g = REPLAY_GRID
    s = one_cell_scan(g, M, (0, row), (7, row), name="row")
    if both:
        s = Scan("row", s.origin, np.vstack([s.hits, np.tile(world(g, 8, row), (M, 1))]))
    name = f"M{M}_{'HM' if both else 'M'}_row{row}_s{shift}_clamp{lo:g}_{hi:g}_p{p[0]:.3g}"
    return Case(name, g, (s,), dict(p_hit=p[0], p_miss=p[1], log_odds_min=lo, log_odds_max=hi)), replay_start(shift)


def replay_cases():
    return [replay_case(c) for c in REPLAY_COMBOS + (DRIFT_COMBO,)]


def replay_counts(combo):
    """(H, M) per cell of the 8 x 8 grid, by construction (the CPU test checks them through the oracle)"""
    M, both, row = combo[:3]
    H_, M_ = np.zeros((8, 8), dtype=np.int64), np.zeros((8, 8), dtype=np.int64)
    M_[row, :7] = 2 * M if both else M
    M_[row, 7] = M if both else 0
    H_[row, 7] = M
    return H_, M_


SAT_LO, SAT_HI, FIXED, FULL, UNTOUCHED = "saturated low", "saturated high", "fixed point", "full loop", "untouched"


_LOOPS = {}


def _replay_loops(v0, H, M, l_hit, l_miss, keep_on_fixed):
    """the two loops of ``apply_counts`` over every counted cell, whatever the shortcut says about it (the shortcut only spares
    the device the loop) -> (values before the clip, whether a loop was left before its last add); kept per input: the wrong
    models share the loops of the right one"""
    key = (v0.tobytes(), H.tobytes(), M.tobytes(), l_hit, l_miss, keep_on_fixed)
    if key not in _LOOPS:
        v, early = v0.copy(), np.zeros(v0.shape, dtype=bool)
        for count, l in ((H, l_hit), (M, l_miss)):
            live = count > 0
            i = 0
            while live.any():
                with np.errstate(invalid="ignore", over="ignore"):
                    nv = (v.astype(np.float64) + l).astype(np.float32)
                fixed = live & (nv == v)
                v = np.where(live & ~fixed, nv, v) if keep_on_fixed else np.where(live, nv, v)
                i += 1
                early |= fixed & (i < count)
                live = live & ~fixed & (i < count)
        _LOOPS[key] = (v, early)
    return _LOOPS[key][0].copy(), _LOOPS[key][1].copy()


def apply_counts(v0, H, M, l_hit, l_miss, lo, hi, bound=True, keep_on_fixed=False, wrap16=False):
    """``apply_counts`` of csrc/raycast.hip restated for arrays: float32(float64(v) + l) H then M times and the clip, with its
    two shortcuts -> (values float32, branch per cell).  A cell without counts is only clipped (the whole-grid clip).
    Wrong models: ``bound=False`` saturates whenever the exact sum is beyond a clamp; ``keep_on_fixed`` leaves the loop with
    the value BEFORE the add that found the fixed point (-0.0 stays -0.0); ``wrap16`` keeps 16 bits of M."""
    shape = np.shape(v0)
    v0 = np.asarray(v0, dtype=np.float32).ravel()
    H, M = np.broadcast_to(np.asarray(H, dtype=np.int64), shape).ravel(), np.broadcast_to(np.asarray(M, dtype=np.int64), shape).ravel()
    if wrap16:
        M = M & 0xffff
    lo32, hi32 = np.float32(lo), np.float32(hi)
    branch = np.full(v0.shape, UNTOUCHED, dtype=object)
    with np.errstate(invalid="ignore"):
        out = np.where(v0 < lo32, lo32, v0)
        out = np.where(out > hi32, hi32, out).astype(np.float32)
    at = np.flatnonzero(H + M > 0)                                 # the loops run over the counted cells only
    v, H, M = v0[at], H[at], M[at]
    Hf, Mf = H.astype(np.float64), M.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = v.astype(np.float64) + Hf * l_hit + Mf * l_miss
        vmax = np.abs(v.astype(np.float64)) + Hf * abs(l_hit) + Mf * abs(l_miss)
        margin = ((Hf + Mf) * vmax * 1.2e-7 + 1e-30) if bound else 0.0
        sat_lo = exact + margin < np.float64(lo32)
        sat_hi = ~sat_lo & (exact - margin > np.float64(hi32))
    v, early = _replay_loops(v, H, M, float(l_hit), float(l_miss), keep_on_fixed)
    br = np.where(early, FIXED, FULL).astype(object)
    with np.errstate(invalid="ignore"):
        v = np.where(v < lo32, lo32, v)
        v = np.where(v > hi32, hi32, v).astype(np.float32)
    v[sat_lo], v[sat_hi] = lo32, hi32
    br[sat_lo], br[sat_hi] = SAT_LO, SAT_HI
    out[at], branch[at] = v, br
    return out.reshape(shape), branch.reshape(shape)


def same_bits(got, want):
    """bit patterns equal; a NaN cell is only required to be NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and bool(
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


# ── what the Python class hands the library, for the routing checks ─────────────────────────────────────────────────────
def box_of(g, scans):
    """the cell box OccupancyGrid2D computes for these scans (its own ``_box_of``, which needs no device)"""
    from utilities.mapping import OccupancyGrid2D, _minmax_rows
    rows = np.vstack([np.asarray(s.origin).reshape(1, 2) for s in scans] + [s.hits for s in scans])
    shim = collections.namedtuple("Shim", "min_x min_y resolution")(g.min_x, g.min_y, g.res)
    return OccupancyGrid2D._box_of(shim, *_minmax_rows(rows))
