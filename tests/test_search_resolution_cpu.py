"""Graded near-ties for the searches of the fused ICP kernel — the part that needs no GPU.

Every search of csrc/icp2.hip must return the exact float64 nearest neighbour.  Four implementations do so (sweep.hpp:
exact walks, float32 filter walks, packed float32 walks, the box hierarchy of the far continuation), and they can go
wrong only where a second candidate lies within the resolution of the float32 filter.  An ordinary scan has such a row in
a thousand, and the first step moves it away.  The pairs made here keep hundreds of such rows at every iteration:

  * the target is symmetric under x -> -x, y -> -y and both (one quadrant mirrored; negation is exact);
  * the source rows are probes placed at near-ties of the target, mirrored the same way, with no initial motion.

Matches are then mirror images of each other, centroids and cross terms cancel, and the step is the identity up to
rounding: the pair is stationary and the near-ties survive every iteration.  One row matched to its runner-up breaks
the symmetry and moves the transform by about (distance between the two candidates) / rows — ``observability`` measures
that for every row, with an extended-precision step.

A probe's relative gap in d^2 between its nearest and its second candidate is drawn log-uniformly, stratified by decade,
from [1e-9, 1e-2): below the 12 mantissa bits a packed word keeps, across the float32 margin, with two, three and four
candidates within 2^-12.  No exact ties: the row rule would break the symmetry, and exact ties are covered by
tests/test_gpu_parity.py::test_packed_walks_on_exact_ties_and_lattices.

Families: ``lattice`` (point-to-point; a jittered 0.25 m lattice whose upper cells are square to 2e-7, probes at
circumcentres and midpoints) and ``corridor`` (point-to-line; wall segments, probes mid-corridor and at a corner, the
nearest and the second candidate always on DIFFERENT walls — two candidates on one line give the same residual).

Measured census (``test_print_the_census``, run with -s; iteration 2 of six; rows with 2 / 3 / >= 4 candidates within
2^-12 of the nearest d^2; rows per decade of the gap 1e-9 .. 1e-3; smallest gap; largest row movement over all iterations
[m]; smallest transform movement when one row takes its runner-up, as a multiple of 1000 x FRO_TOL; rows lost to that
bound):

  pair               rows  target   2    3  >=4 | 1e-9 1e-8 1e-7 1e-6 1e-5 1e-4 1e-3 | smallest  movement  margin  lost
  lattice/base        616    384  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   5.6e-17     344  0.00
  lattice/rot45       616    384  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   2.9e-17     344  0.00
  lattice/rot90       616    384  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   5.6e-17     344  0.00
  lattice/rot135      616    384  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   1.1e-16     344  0.00
  lattice/long        600    384  252   64  120 |   60   72   80  108   80   76   64 |  1.1e-09   5.6e-17     360  0.00
  lattice/off35       616    384  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   2.1e-14     299  0.00
  lattice/off2e4      616    384  232   64   68 |    0    0  120  108   96   92  100 |  1.1e-07   9.1e-12 8.06e+03  0.00
  lattice/small        12    384    4    4    4 |    0    4    0    8    0    0    0 |  2.1e-08         0 1.97e+04  0.00
  lattice/pad2048     616   2048  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   5.6e-17     344  0.00
  lattice/pad2049     616   2049  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   5.6e-17     344  0.00
  lattice/pad4097     616   4097  256   56   96 |   64   88   68   88   68   68   76 |  1.1e-09   5.6e-17     344  0.00
  corridor/base       508   1448  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    83.6  0.00
  corridor/rot45      508   1448  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09   1.1e-16    83.6  0.00
  corridor/rot90      508   1448  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    83.6  0.00
  corridor/rot135     508   1448  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09   1.1e-16    83.6  0.00
  corridor/long       508   2008  148  120  120 |   72   60   72   88   76   64   72 |  1.3e-09   1.1e-16    46.4  0.00
  corridor/off35      508   1448  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    72.5  0.00
  corridor/small       12   1448    4    4    4 |    0    4    4    4    0    0    0 |  4.2e-08   3.7e-14 6.08e+04  0.00
  corridor/pad2048    508   2048  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    83.6  0.00
  corridor/pad2049    508   2049  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    83.6  0.00
  corridor/pad4097    508   4097  160  128  120 |   68   68   72   88   76   68   68 |  1.2e-09         0    83.6  0.00

The pair at (2e4, -1.5e4) has gaps from 1e-7 on: an ulp of its coordinates is 3.6e-12 m, which is 1e-10 relative in the
d^2 of a probe, so smaller gaps would lie within what two correct implementations may differ by.
"""
import functools

import numpy as np
import pytest

import oracle
from conftest import rot_err
from test_p2l_step_cpu import GAP_MIN, LD, normals_reference, numpy_step, step_reference

FRO_TOL = 1e-9                  # tests/test_gpu_parity.py
OBSERVABLE = 1000 * FRO_TOL     # what one swapped match must move the transform by
RES = 2.0 ** -12                # the resolution of a packed word, relative in d^2
DECADES = tuple(range(-9, -2))  # 10^k <= gap < 10^(k + 1)
ITERS = 6                       # iterations 0, 1: plain searches (the second seeded); 2 on: top-two from the kept match
VOXEL = 1e-3                    # every row its own voxel
NORMAL_K = 12
MOVE_MAX, GAP_FLOOR, LOST_MAX = 1e-12, 1e-10, 0.05


# ── generators ───────────────────────────────────────────────────────────────
def mirror(q):
    """The four images of a quadrant under the group D2 (exact)."""
    return np.vstack([q, q * [-1.0, 1.0], q * [1.0, -1.0], -q])


def _gaps(rng, n, lo):
    """n relative gaps, log-uniform inside a decade, the decades lo .. -3 dealt out in turn, in random order."""
    dec = np.arange(n) % (-2 - lo) + lo
    return rng.permutation(10.0 ** (dec + rng.uniform(0.02, 0.98, n)))


def _circumcentre(a, b, c):
    ab, ac = b - a, c - a
    d = 2.0 * (ab[0] * ac[1] - ab[1] * ac[0])
    ux = (ac[1] * (ab @ ab) - ab[1] * (ac @ ac)) / d
    uy = (ab[0] * (ac @ ac) - ac[0] * (ab @ ab)) / d
    return a + [ux, uy]


def _probe_centre(pts, first, second, gap, third=None):
    """A probe beside the circumcentre o of pts[first], pts[second] and pts[third] (a fourth point lies nearly on the same circle) that has
    pts[first] nearest and pts[second] second by ``gap`` relative in d^2.  Moved by eps along a unit vector u:
    d_i^2 = r^2 - 2 eps u.(q_i - o) + eps^2, so the order of the candidates is that of u.(q_i - o); u is the middle of
    the arc of directions that give the wanted two (the two must be neighbours on the circle)."""
    o = _circumcentre(pts[first], pts[second], pts[3 - first - second if third is None else third])
    w = pts - o
    ang = np.linspace(0.0, 2.0 * np.pi, 7200, endpoint=False)
    s = w @ np.array([np.cos(ang), np.sin(ang)])
    top = np.argsort(-s, axis=0)[:2]
    ok = (top[0] == first) & (top[1] == second)
    assert ok.any() and not ok.all(), (pts, first, second)
    start = int(np.flatnonzero(~ok)[0])                     # the arc may run through angle 0: count from outside it
    arc = (np.flatnonzero(np.roll(ok, -start)) + start) % len(ang)
    k = arc[len(arc) // 2]
    u = np.array([np.cos(ang[k]), np.sin(ang[k])])
    return o + u * (gap * (w[first] @ w[first]) / (2.0 * (s[first, k] - s[second, k])))


def _probe_pair(a, c, gap, across):
    """A probe ``across`` beside the midpoint of a and c (to the left of a -> c), nearer to a by ``gap`` relative in d^2."""
    e = c - a
    L = np.hypot(*e)
    e = e / L
    d2 = 0.25 * L * L + across * across
    return 0.5 * (a + c) - e * (gap * d2 / (2.0 * L)) + across * np.array([-e[1], e[0]])


def lattice_quadrant(seed, nx=12, ny=8, lo=-9):
    """-> (probes, kinds, points) of one quadrant.  Points: an nx x ny lattice of 0.25 m, jitter +-0.02 — +-2e-7 in the
    four upper rows, so the cells of the three upper rows are square to that.  Probes, per cell: the circumcentre of three
    corners moved by eps in a random direction (three candidates, four in a square cell) and the midpoint of the lower
    edge moved by eps along it and 0.01 across (two)."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    jit = np.where((j >= ny - 4)[..., None], 2e-7, 0.02) * rng.uniform(-1, 1, (ny, nx, 2))
    P = np.stack([(i + 0.5) * 0.25, (j + 0.5) * 0.25], -1) + jit
    cells = [(r, c) for r in range(ny - 1) for c in range(nx - 1)]
    g3, g2 = _gaps(rng, len(cells), lo), _gaps(rng, len(cells), lo)
    probes, kinds = [], []
    for n, (r, c) in enumerate(cells):
        corners = np.array([P[r, c], P[r, c + 1], P[r + 1, c], P[r + 1, c + 1]])
        o = _circumcentre(*corners[:3])
        w = corners[:3] - o
        u = rng.normal(size=2)
        u /= np.hypot(*u)
        s = np.sort(w @ u)
        probes.append(o + u * (g3[n] * (w[0] @ w[0]) / (2.0 * (s[2] - s[1]))))
        kinds.append("four" if r >= ny - 4 else "three")
        probes.append(_probe_pair(P[r, c], P[r, c + 1], g2[n] * rng.choice([-1.0, 1.0]), 0.01))
        kinds.append("two")
    return np.array(probes), kinds, P.reshape(-1, 2)


def corridor_quadrant(seed, n=161, half=40, lo=-9):
    """-> (probes, kinds, points) of one quadrant: a corridor 0.5 m wide along x (walls at y = 1 and y = 1.5, n points
    0.05 m apart each, so the 12 neighbours of a point inside a wall are points of that wall) and a corner behind its end.
      * the first ``half`` cells, upper points above the lower ones, jitter +-2e-7: the centre of a cell has two
        candidates on either wall; the probe is moved so that the nearest and the second lie on different walls;
      * from there on, upper points half a step on, jitter +-0.0005, probes in the next ``half`` cells: the circumcentre
        of two points of one wall and one of the other (three candidates, the single one nearest or second), and the
        midpoint of a diagonal (two);
      * a corner whose walls stop 0.1 m short of it: probes on its diagonal, one candidate on each wall (two).
    The walls run on without probes: the cloud is long and thin, so the prepare kernel sorts it along its length."""
    rng = np.random.default_rng(seed)
    x = 0.5 + 0.05 * np.arange(n)
    jit = np.where(np.arange(n) <= half, 2e-7, 0.0005)[:, None]
    low = np.column_stack([x, np.full(n, 1.0)]) + jit * rng.uniform(-1, 1, (n, 2))
    upp = np.column_stack([x + np.where(np.arange(n) <= half, 0.0, 0.025), np.full(n, 1.5)]) + jit * rng.uniform(-1, 1, (n, 2))
    cx, cy, r = x[-1] + 1.55, 1.5, 0.1 + 0.05 * np.arange(20)
    hw = np.column_stack([cx - r, np.full(20, cy)]) + rng.uniform(-0.004, 0.004, (20, 2))
    vw = np.column_stack([np.full(20, cx), cy - r]) + rng.uniform(-0.004, 0.004, (20, 2))
    probes, kinds = [], []
    g4, g3, g2, gc = _gaps(rng, half, lo), _gaps(rng, half, lo), _gaps(rng, half, lo), _gaps(rng, 7, lo)
    for k in range(half):
        # corners in the order lower left, lower right, upper left, upper right; (first, second) across the corridor
        # (the circle goes through the other point of the wall of ``first``: the fourth point, which is off it by the
        # jitter and may come in anywhere, lies across from ``first`` too)
        first, second, third = [(0, 2, 1), (2, 0, 3), (1, 3, 0), (3, 1, 2)][k % 4]
        probes.append(_probe_centre(np.array([low[k], low[k + 1], upp[k], upp[k + 1]]), first, second, g4[k], third))
        kinds.append("four")
    for j, k in enumerate(range(half + 1, 2 * half + 1)):
        first, second = [(2, 0), (2, 1), (0, 2), (1, 2)][k % 4]
        probes.append(_probe_centre(np.array([low[k], low[k + 1], upp[k]]), first, second, g3[j]))
        kinds.append("three")
        a, c = (low[k], upp[k]) if k % 2 else (upp[k], low[k + 1])
        probes.append(_probe_pair(a, c, g2[j], 0.0))
        kinds.append("two")
    for k in range(7):                                      # feet 0.2 .. 0.5 m from the corner, nearer to either wall in turn
        a, c, side = (hw[2 + k], vw[2 + k], -1.0) if k % 2 else (vw[2 + k], hw[2 + k], 1.0)
        probes.append(_probe_pair(a, c, gc[k], side * 0.5 * np.hypot(*(c - a))))
        kinds.append("two")
    return np.array(probes), kinds, np.vstack([low, upp, hw, vw])


def filler(count):
    """``count`` distant target rows, D2-symmetric: wall segments 20 m and more out (every point has a normal), and the
    origin — the one point that is its own image — when count is odd."""
    per, rest = divmod(count, 4)
    assert rest in (0, 1)
    k = np.arange(per)
    seg, along = k // 64, (k % 64) * 0.05
    q = np.column_stack([1.0 + along + 4.0 * (seg % 4), 20.0 + 0.5 * (seg // 4) + 0.003 * np.sin(1.0 + 7.0 * k)])
    return np.vstack([mirror(q)] + ([np.zeros((1, 2))] if rest else []))


def placed(pts, deg, shift):
    """The cloud turned by 0, 45, 90 or 135 degrees (90: exact) and shifted."""
    if deg in (90, 135):
        pts = pts[:, ::-1] * [-1.0, 1.0]
    if deg in (45, 135):
        h = np.sqrt(0.5)
        pts = pts @ np.array([[h, h], [-h, h]])
    return pts + np.asarray(shift, dtype=np.float64)


FAMILIES = {"lattice": ("point_to_point", lattice_quadrant), "corridor": ("point_to_line", corridor_quadrant)}
# name: (quadrant arguments, rotation, shift, small, target rows after padding)
VARIANTS = {
    "base": ({}, 0, (0, 0), False, None),
    "rot45": ({}, 45, (0, 0), False, None),
    "rot90": ({}, 90, (0, 0), False, None),
    "rot135": ({}, 135, (0, 0), False, None),
    "long": ({"long": True}, 0, (0, 0), False, None),
    "off35": ({}, 0, (35.0, -20.0), False, None),
    "off2e4": ({"lo": -7}, 0, (2.0e4, -1.5e4), False, None),
    "small": ({}, 0, (0, 0), True, None),
    "pad2048": ({}, 0, (0, 0), False, 2048),
    "pad2049": ({}, 0, (0, 0), False, 2049),
    "pad4097": ({}, 0, (0, 0), False, 4097),
}
LONG = {"lattice": dict(nx=16, ny=6), "corridor": dict(n=231)}      # the 2:1 elongated quadrants


@functools.lru_cache(maxsize=None)
def pair(family, variant):
    """-> (source, target, method, lowest gap decade): a stationary pair, rows shuffled (seeded) so that neither the row
    rule nor the order of the rows follows the geometry."""
    args, deg, shift, small, rows = VARIANTS[variant]
    args = dict(args)
    if args.pop("long", False):
        args.update(LONG[family])
    method, quadrant = FAMILIES[family]
    probes, kinds, pts = quadrant(11 if family == "lattice" else 12, **args)
    if small:                                               # one probe of each kind with a gap in [1e-8, 1e-5): twelve rows
        tgt0 = mirror(pts)
        d2 = np.sort(((probes[:, None, :] - tgt0[None]) ** 2).sum(-1), axis=1)
        gap = (d2[:, 1] - d2[:, 0]) / d2[:, 0]
        pick = [next(i for i, k in enumerate(kinds) if k == kind and 1e-8 <= gap[i] < 1e-5) for kind in ("two", "three", "four")]
        probes = probes[pick]
    src, tgt = mirror(probes), mirror(pts)
    if rows is not None:
        tgt = np.vstack([tgt, filler(rows - len(tgt))])
    rng = np.random.default_rng(7)
    src, tgt = src[rng.permutation(len(src))], tgt[rng.permutation(len(tgt))]
    src.flags.writeable = tgt.flags.writeable = False
    return placed(src, deg, shift), placed(tgt, deg, shift), method, args.get("lo", -9)


def all_pairs():
    """Every pair of the GPU test.  One pair lies 20 km out, and it is a point-to-point one: the point-to-line system is
    numerically singular there (the lever of the rotation; tests/test_p2l_step_cpu.py, family off2e4), so two correct
    kernels differ by more than the 1e-12 they are compared at (measured: 2e-10 in t)."""
    return [(f, v) for f in FAMILIES for v in VARIANTS if (f, v) != ("corridor", "off2e4")]


# ── the loop, restated in float64 NumPy ──────────────────────────────────────
def matches(cur, tgt, top=5):
    """Brute-force candidates of every row: the ``top`` smallest dx*dx + dy*dy (rounded as written) and their rows, the
    lowest row first among equals — the project's rule."""
    dx, dy = cur[:, None, 0] - tgt[None, :, 0], cur[:, None, 1] - tgt[None, :, 1]
    d2 = dx * dx + dy * dy
    part = np.sort(np.argpartition(d2, top, axis=1)[:, :top], axis=1)      # (no exact ties at the cut: asserted per pair)
    order = np.take_along_axis(part, np.argsort(np.take_along_axis(d2, part, 1), axis=1, kind="stable"), 1)
    return np.take_along_axis(d2, order, 1), order


def p2p_step(P, Q, dtype=np.float64):
    """One point-to-point step (Kabsch, icp.py:197-207) in 2-D closed form -> (R, t)."""
    P, Q = P.astype(dtype), Q.astype(dtype)
    mp, mq = P.mean(0), Q.mean(0)
    A, B = P - mp, Q - mq
    th = np.arctan2((A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]).sum(), (A[:, 0] * B[:, 0] + A[:, 1] * B[:, 1]).sum())
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], dtype=dtype)
    return R, mq - R @ mp


def p2l_step(P, tgt, normals, idx):
    x, _, _ = numpy_step(P, tgt, normals, idx)
    R = np.array([[np.cos(x[0]), -np.sin(x[0])], [np.sin(x[0]), np.cos(x[0])]])
    return R, x[1:]


def census_of(d2):
    """Of sorted candidate d^2 [N, top]: candidates within 2^-12 relative of the nearest (itself included) and the relative
    gap between the nearest and the second."""
    return (d2 <= d2[:, :1] * (1.0 + RES)).sum(1), (d2[:, 1] - d2[:, 0]) / d2[:, 0]


def run_loop(src, tgt, method, iters=ITERS, swap=None):
    """The ICP loop with error_threshold = 0 -> (R, t, err, per-iteration records).  swap = (iteration, row): that row
    takes its runner-up at that iteration."""
    normals = oracle.normals_2d(tgt, NORMAL_K) if method == "point_to_line" else None
    cur, R, t, err, rec = src.copy(), np.eye(2), np.zeros(2), np.inf, []
    for it in range(iters):
        d2, order = matches(cur, tgt)
        idx = order[:, 0].copy()
        if swap is not None and swap[0] == it:
            idx[swap[1]] = order[swap[1], 1]
        r, tt = p2p_step(cur, tgt[idx]) if normals is None else p2l_step(cur, tgt, normals, idx)
        new = cur @ r.T + tt
        within, gap = census_of(d2)
        rec.append(dict(move=float(np.abs(new - cur).max()), within=within, gap=gap, cur=cur, order=order, d2=d2))
        cur, R, t = new, r @ R, r @ t + tt
        err = float(((tgt[idx] - cur) ** 2).sum(1).mean())
    return R, t, err, rec


def observability(cur, tgt, order, method, rows, normals=None):
    """For each of ``rows``: how far (Frobenius, rot_err) one reference step moves when that row takes its runner-up —
    the longdouble Kabsch step for point_to_point, the exact ``step_reference`` for point_to_line."""
    def step(idx):
        if method == "point_to_point":
            R, t = p2p_step(cur, tgt[idx], LD)
            return R.astype(np.float64), t.astype(np.float64)
        ref = step_reference(cur, tgt, normals, idx)
        th = ref["theta"]
        return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), np.array([ref["tx"], ref["ty"]])
    base = step(order[:, 0])
    out = []
    for i in rows:
        idx = order[:, 0].copy()
        idx[i] = order[i, 1]
        out.append(rot_err(*step(idx), *base))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def measured(family, variant):
    """The census of one pair: per iteration the movement, the classes, the decades; the observability at iteration 2."""
    src, tgt, method, lo = pair(family, variant)
    _, _, _, rec = run_loop(src, tgt, method)
    normals = oracle.normals_2d(tgt, NORMAL_K) if method == "point_to_line" else None
    r2 = rec[2]
    rows = np.flatnonzero(r2["gap"] < 1e-2)
    moved = observability(r2["cur"], tgt, r2["order"], method, rows, normals)
    seen = rows[moved >= OBSERVABLE]
    out = dict(move=max(r["move"] for r in rec), margin=float(moved[moved >= OBSERVABLE].min() / OBSERVABLE), lo=lo, per_it=[])
    for r in rec:
        w, g = r["within"][seen], r["gap"][seen]
        out["per_it"].append(dict(classes=[int((w == 2).sum()), int((w == 3).sum()), int((w >= 4).sum())],
                                  decades=[int(((g >= 10.0 ** k) & (g < 10.0 ** (k + 1))).sum()) for k in DECADES],
                                  smallest=float(g[g > 0].min())))
    w_all = np.minimum(r2["within"][rows], 4)
    out["lost"] = [float(((w_all == c) & (moved < OBSERVABLE)).sum() / max(1, (w_all == c).sum())) for c in (2, 3, 4)]
    return out


# ── the conditions every pair of the GPU test meets ──────────────────────────
@pytest.mark.parametrize("family,variant", all_pairs())
def test_pairs_are_stationary_graded_and_observable(family, variant):
    src, tgt, method, lo = pair(family, variant)
    m = measured(family, variant)
    # (a coordinate that moves at all moves by an ulp: 3.6e-12 m at 2e4.  Product and sum of the step round at that size, and so
    # does the translation: four ulps there; every other pair has ulps far below MOVE_MAX)
    assert m["move"] <= max(MOVE_MAX, 4 * np.spacing(np.abs(tgt).max())), m["move"]
    assert max(m["lost"]) <= LOST_MAX, m["lost"]
    for it, c in enumerate(m["per_it"]):
        assert c["smallest"] >= (GAP_FLOOR if lo == -9 else 10.0 ** lo * 0.5), (it, c)
        assert min(c["classes"]) >= 1, (it, c)
        if variant != "small":
            assert len(src) <= 616 and min(c["decades"][lo + 9:]) >= 1, (it, c)
    if variant == "small":
        assert len(src) <= 12
    if VARIANTS[variant][4]:
        assert len(tgt) == VARIANTS[variant][4]
    d = np.sort(((tgt[:, None, :] - tgt[None]) ** 2).sum(-1), axis=1)[:, 1]
    assert d.min() > 2 * VOXEL ** 2                                       # no two rows share a voxel; no exact ties below
    d2, _ = matches(src, tgt)
    assert (d2[:, 1] > d2[:, 0]).all()


@pytest.mark.parametrize("variant", [v for f, v in all_pairs() if f == "corridor"])
def test_corridor_targets_have_normals(variant):
    _, tgt, _, _ = pair("corridor", variant)
    _, gap, _ = normals_reference(tgt, NORMAL_K)
    assert gap.min() >= GAP_MIN, gap.min()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_restated_loop_is_the_oracle(family):
    """The NumPy loop above against oracle.icp: same transform (FRO_TOL), same error, six iterations, not converged."""
    src, tgt, method, _ = pair(family, "base")
    R, t, err, _ = run_loop(src, tgt, method)
    Ro, to, eo, io = oracle.icp(src, tgt, 0.0, ITERS, VOXEL, method=method, normal_k=NORMAL_K)
    assert io["iters"] == ITERS and io["status"] == oracle.MAXITER and io["n_src"] == len(src) and io["n_tgt"] == len(tgt)
    assert rot_err(R, t, Ro, to) < FRO_TOL and abs(err - eo) <= 1e-9 * max(1.0, eo)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_one_swapped_match_fails_the_comparison_of_the_gpu_test(family):
    """What tests/test_search_resolution_gpu.py compares — the final transform against oracle.icp within FRO_TOL — when
    ONE row of the census takes its runner-up in ONE iteration: off by at least 1000 x FRO_TOL when that is the last
    iteration (the observability margin itself); an earlier one is printed (later steps do not heal it: the moved cloud
    re-decides every near-tie on one side)."""
    src, tgt, method, _ = pair(family, "base")
    Ro, to, _, _ = oracle.icp(src, tgt, 0.0, ITERS, VOXEL, method=method, normal_k=NORMAL_K)
    _, _, _, rec = run_loop(src, tgt, method)
    rows = np.flatnonzero(rec[2]["gap"] < 1e-2)
    rng = np.random.default_rng(3)
    for row in rng.choice(rows, 6, replace=False):
        for it in (1, 2, ITERS - 1):
            R, t, _, _ = run_loop(src, tgt, method, swap=(it, int(row)))
            off = rot_err(R, t, Ro, to)
            print(f"\n{family}: row {row} swapped at iteration {it}: final transform off by {off:.3g}", end="")
            assert off > FRO_TOL, (row, it, off)
            if it == ITERS - 1:
                assert off >= 0.5 * OBSERVABLE, (row, off)


def census_table():
    lines = ["  pair               rows  target   2    3  >=4 | " + " ".join(f"1e{k:+d}" for k in DECADES) +
             " | smallest  movement  margin  lost"]
    for f, v in all_pairs():
        src, tgt, _, _ = pair(f, v)
        m = measured(f, v)
        c = m["per_it"][2]
        lines.append(f"  {f + '/' + v:17s} {len(src):5d} {len(tgt):6d} {c['classes'][0]:4d} {c['classes'][1]:4d} {c['classes'][2]:4d} | " +
                     " ".join(f"{n:4d}" for n in c["decades"]) +
                     f" | {c['smallest']:8.2g} {m['move']:9.2g} {m['margin']:7.3g} {max(m['lost']):5.2f}")
    return "\n".join(lines)


def test_print_the_census():
    print("\n" + census_table())
