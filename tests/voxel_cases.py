"""Inputs of the voxel-filter edge suites, built from seeds or by construction — TEST INFRASTRUCTURE ONLY.

Every builder returns ``(name, points, voxel)``.  tests/test_voxel_edges_cpu.py proves on tests/voxel_ref.py alone that every
input has the property its GPU test relies on and takes the code path it is meant for; tests/test_voxel_edges_gpu.py runs the
library on the same inputs.  Nothing here touches a GPU.

The routing rules of csrc/voxel.hip are restated once, in ``route``: which of its code paths a cloud of n rows takes on a
launch of 512 or 1 024 threads.  There are eight names, ``ROUTES``: the four register-sort shapes, the three sort forms of the
LDS path (a register shape that declines a cloud hands it to the 64-bit or the pair form of the LDS path), and the
large path.

Out of scope: non-finite coordinates.  The reference returns NaN for the whole cloud there (the minimum is NaN), and the
device code has no defined answer; no case here holds one.
"""
import functools

import numpy as np

import voxel_ref as vr

SMALL_MAX = 8192                       # VOX_SMALL_MAX: more rows take the large path
SET_CLOUDS = 257                       # the smallest set whose launch takes 512 threads a workgroup
ROUTES = ("regs E=2 T=512", "regs E=4 T=512", "regs E=2 T=1024", "regs E=4 T=1024",
          "lds 32-bit", "lds 64-bit", "lds pairs", "large")
REFUSED = "refused"


# ── the kernel's routing, restated ──────────────────────────────────────────────────────────────────────────────────────
def npad_of(n):
    """slots of the sort: the next power of two at or above n, 64 at the least (sort_npad)"""
    npad = 64
    while npad < n:
        npad <<= 1
    return npad


def threads_of(n_clouds):
    """threads a workgroup of the one launch over a set (plan_voxel)"""
    return 512 if n_clouds > 256 else 1024


def extents(points, voxel):
    """key extent per axis, floor((max - min) / voxel) + 1, as the kernel's double arithmetic has it (key_extents)"""
    p = np.asarray(points, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.floor((p.max(axis=0) - p.min(axis=0)) / voxel) + 1.0


def fits(points, voxel):
    """False when the filter refuses the cloud (count -1): an extent or the product of the extents is not below 9e18"""
    ext = extents(points, voxel)
    prod = 1.0
    for e in ext:
        if not (e >= 1.0) or not (e < 9.0e18):
            return False
        prod *= e
    return prod < 9.0e18


def packed_range(points, voxel):
    """cells x slots: the bound of the packed (key, row) values (vox_packed_range), multiplied in the kernel's order"""
    cells = 1.0
    for e in extents(points, voxel):
        cells *= e
    return cells * float(npad_of(len(points)))


def route(points, voxel, threads):
    """The name (one of ROUTES, or REFUSED) of the path a cloud takes on a launch of ``threads`` threads a workgroup."""
    n = len(points)
    assert n >= 1 and threads in (512, 1024)
    if not fits(points, voxel):
        return REFUSED
    if n > SMALL_MAX:
        return "large"
    npad, rng = npad_of(n), packed_range(points, voxel)
    if npad in (2 * threads, 4 * threads) and rng < 4.0e9:
        return f"regs E={npad // threads} T={threads}"
    return "lds 32-bit" if rng < 4.0e9 else "lds 64-bit" if rng < 9.0e18 else "lds pairs"


def routes(points, voxel):
    """(alone, in a set of more than 256 clouds): the second is None for a cloud of the large path, which no launch width
    changes"""
    alone = route(points, voxel, 1024)
    return alone, (None if len(points) > SMALL_MAX else route(points, voxel, 512))


def _frozen(name, pts, voxel):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    assert np.isfinite(pts).all(), name
    pts.setflags(write=False)
    return name, pts, float(voxel)


# ── one voxel ───────────────────────────────────────────────────────────────────────────────────────────────────────────
# (1 024, 2 048 and 4 096 rows fill a register shape: the run ends at the slot behind the sorted array — 1 024 on 512 threads)
ONE_VOXEL_N = {2: (1024, 1025, 2047, 2048, 4095, 4096, 8192, 8193, 20000), 3: (2048, 4096, 8193)}
ONE_VOXEL_SIZE = 8.0


@functools.lru_cache(maxsize=None)
def one_voxel(n, dim):
    """n points of magnitudes 1e-6 .. 3, either sign, in shuffled order: less than 8 apart on every axis, so all in the one
    voxel of size 8, and a running sum that rounds at nearly every step."""
    rng = np.random.default_rng(7000 + 10 * n + dim)
    pts = rng.choice([-1.0, 1.0], size=(n, dim)) * 10.0 ** rng.uniform(-6.0, 0.5, size=(n, dim))
    return _frozen(f"one_voxel_{dim}d_{n}", rng.permutation(pts), ONE_VOXEL_SIZE)


# ── runs of every length and alignment ──────────────────────────────────────────────────────────────────────────────────
RUN_ROWS = (513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
RUN_VOXEL = 0.25
RUN_CYCLE = tuple(range(1, 10))
# 513 rows cannot hold 100 voxels of three or more members on the cycle (it spends 45 rows on 7 such voxels), and sums of
# three numbers of one binade depend on the order less than half of the time: there every length from 1 to 9 occurs once
# (6 twice), and 94 voxels of 4 or 5 members fill the rows, in an order drawn once
RUN_LENGTHS_513 = (1, 2, 3, 6, 6, 7, 8, 9) + (4,) * 39 + (5,) * 55
RUN_STRIPE = 32                        # voxels a stripe: the key extents stay small, so every case sorts 32-bit words


def run_lengths(n):
    """the member count of every voxel, in the order they are built: a few long runs (40 to 70) spread among the cycle, n
    rows in all"""
    long_runs = [40] if n < 1024 else [40, 55, 70] if n < 4096 else [40, 47, 55, 62, 70]
    lens, left, i = [], n - sum(long_runs), 0
    if n < 1024:
        assert left == sum(RUN_LENGTHS_513)
        lens, left = [int(c) for c in np.random.default_rng(513).permutation(RUN_LENGTHS_513)], 0
    while left > 0:
        lens.append(min(RUN_CYCLE[i % len(RUN_CYCLE)], left))
        left -= lens[-1]
        i += 1
    for j, run in enumerate(long_runs):                              # at odd places, so their starts differ mod 4
        lens.insert((2 * j + 1) * len(lens) // (2 * len(long_runs)) + j % 4, run)
    assert sum(lens) == n
    return lens


def run_lengths_in_key_order(n):
    """... as the filter meets them: voxel j has the second key 31 - j mod 32, so every stripe of 32 comes out backwards"""
    lens = run_lengths(n)
    return [c for s in range(0, len(lens), RUN_STRIPE) for c in lens[s:s + RUN_STRIPE][::-1]]


@functools.lru_cache(maxsize=None)
def runs(n, dim):
    """Voxel j has the key (j div 32, 31 - j mod 32[, j mod 7]): key order runs down one diagonal stripe after the other.
    Its members lie anywhere inside it, and a permutation scatters the members of every voxel through the input.  One member
    each of voxel 0 and of voxel 31 sits on the lower faces of the box, so the bounding box starts at 0 and the keys are
    the ones built."""
    rng = np.random.default_rng(8000 + 10 * n + dim)
    lens = run_lengths(n)
    J, W = len(lens), RUN_STRIPE
    assert J > W
    vox_of_row = np.repeat(np.arange(J), lens)
    key = np.stack([vox_of_row // W, W - 1 - vox_of_row % W, vox_of_row % 7][:dim], axis=1).astype(np.float64)
    pts = (key + rng.uniform(0.03, 0.97, size=(n, dim))) * RUN_VOXEL
    first = np.concatenate([[0], np.cumsum(lens)])                   # the first row of every voxel, before the permutation
    pts[first[0], 0] = 0.0
    pts[first[W - 1], 1] = 0.0
    if dim == 3:
        pts[first[0], 2] = 0.0
    return _frozen(f"runs_{dim}d_{n}", pts[rng.permutation(n)], RUN_VOXEL)


# ── clusters between two corner points ──────────────────────────────────────────────────────────────────────────────────
CLUSTER_ROWS = (1024, 2048, 4096)
CLUSTER_VOXEL = 0.5
CLUSTER_SIDES = ("below 4e9", "above 4e9", "exactly 4e9", "below 9e18", "above 9e18")
CLUSTER_FORM = {"below 4e9": "32-bit", "above 4e9": "64-bit", "exactly 4e9": "64-bit", "below 9e18": "64-bit",
                "above 9e18": "pairs"}


def cluster_extents(side, n, dim):
    """Key extents whose product times npad lies on the named side of a switch between sort forms, as near to it as whole
    extents allow: all axes but the last near the dim-th root of limit / npad, the last axis the smallest that reaches the
    limit (above), or one less (below).  2 048 rows, 2-D: 1 398 x 1 397 and 1 398 x 1 398.  The comparison is strict, so a
    product of exactly 4e9 is already a 64-bit case: 4e9 / npad in factors of 2 and 5, and None where that is no whole
    number (4 096 slots)."""
    npad = npad_of(n)
    if side == "exactly 4e9":
        cells = {1024: (1250, 3125) if dim == 2 else (125, 125, 250),
                 2048: (125, 15625) if dim == 2 else (125, 125, 125)}.get(npad)
        assert cells is None or int(np.prod(cells)) * npad == 4_000_000_000
        return cells
    limit = 4_000_000_000 if "4e9" in side else 9_000_000_000_000_000_000
    a = round((limit / npad) ** (1.0 / dim))
    rest = a ** (dim - 1)
    # the smallest b with rest * b * npad >= limit: the kernel asks "below the limit?", so a product of exactly the limit is
    # on the far side already (1 024 slots, 2-D: 93 750 000 squared times 1 024 is exactly 9e18)
    b = -(-limit // (npad * rest))
    ext = (a,) * (dim - 1) + ((b,) if side.startswith("above") else (b - 1,))
    prod = int(np.prod([int(e) for e in ext], dtype=object)) * npad
    assert (prod >= limit) if side.startswith("above") else (prod < limit), (side, n, dim, ext)
    return ext


@functools.lru_cache(maxsize=None)
def clusters(side, n, dim):
    """Two corner points fix the bounding box: the origin, and a point a quarter voxel inside the voxel with the largest key.
    A cluster in the voxel of key 0, one in the voxel with the largest key which holds the last row, and about 100 voxels
    spread over the box with up to about 60 members each; every row but the last is shuffled.  Voxel 0.5 and extents below
    2^27: every coordinate, difference and quotient of the corner points is exact, so the extents are the ones asked for.
    None where ``cluster_extents`` has no such extents."""
    ext = cluster_extents(side, n, dim)
    if ext is None:
        return None
    rng = np.random.default_rng(9000 + 100 * CLUSTER_SIDES.index(side) + 10 * CLUSTER_ROWS.index(n) + dim)
    ext = np.array(ext, dtype=np.int64)
    top = ext - 1
    v = CLUSTER_VOXEL
    n_first, n_last = 9, 7                                           # members of the key-0 and of the largest-key cluster
    raw = rng.integers(1, 61, size=100).astype(np.float64) ** 1.5    # three members each, the other rows shared out unevenly
    lens = 3 + np.floor(raw * ((n - n_first - n_last - 300) / raw.sum())).astype(np.int64)
    lens[np.argmax(lens)] += n - n_first - n_last - lens.sum()
    assert lens.sum() + n_first + n_last == n and lens.min() >= 3
    keys = np.stack([rng.integers(0, e, size=100) for e in ext], axis=1)
    bulk = (np.repeat(keys, lens, axis=0) + rng.uniform(0.0, 1.0, size=(lens.sum(), dim))) * v
    first = rng.uniform(0.0, 1.0, size=(n_first, dim)) * v
    first[0] = 0.0                                                   # the lower corner of the box
    last = (top + rng.uniform(0.0, 0.25, size=(n_last, dim))) * v
    last[0] = (top + 0.25) * v                                       # the upper corner of the box
    head = np.concatenate([bulk, first, last[:-1]])
    pts = np.concatenate([head[rng.permutation(len(head))], last[-1:]])
    assert len(pts) == n and np.array_equal(extents(pts, v), ext.astype(np.float64))
    return _frozen(f"clusters_{dim}d_{n}_{side.replace(' ', '_')}", pts, v)


# ── division lattices ───────────────────────────────────────────────────────────────────────────────────────────────────
LATTICE_V = (0.1, 0.05, 0.04, 0.3, 1.0 / 3.0)
LATTICE_OFF = (0.0, -7.3, 1.0e6 + 0.37)
LATTICE_SHIFTS = ("on", "ulp_down", "ulp_up")
LATTICE_K = 400
LATTICE_TILED = (1024, 2048, 4096, 4097, 8193)       # both register shapes of either launch, the LDS path, the large path
LATTICE_FAR = {"64-bit": 1.0e6, "pairs": 2.0e9}      # steps from the lattice to one far point: the other LDS sort forms
RECIPROCAL_V, RECIPROCAL_OFF = LATTICE_V[:3], LATTICE_OFF[:2]        # where the issue's floor of 20 points holds


def _lattice_points(v, off, shift):
    k = np.arange(LATTICE_K, dtype=np.float64)
    pts = np.stack([off + k * v, off + k[::-1] * v], axis=1)         # the two axes run in opposite directions
    if shift == "ulp_down":
        pts = np.nextafter(pts, -np.inf)
    elif shift == "ulp_up":
        pts = np.nextafter(pts, np.inf)
    return pts


def _lattice_name(v, off, shift):
    return f"lattice_v{v:.4g}_off{off:.7g}_{shift}"


@functools.lru_cache(maxsize=None)
def lattice(v, off, shift="on"):
    """400 points off + k v per axis (k = 0 .. 399), as float64 computes them, all of them moved one ulp down or up on
    request: the quotients (p - min) / v sit on or next to whole numbers, where the rounding of the divide decides the key."""
    return _frozen(_lattice_name(v, off, shift), _lattice_points(v, off, shift), v)


@functools.lru_cache(maxsize=None)
def lattice_tiled(v, off, n):
    """the lattice repeated to n rows (row i is lattice row i mod 400)"""
    return _frozen(_lattice_name(v, off, "on") + f"_x{n}", np.resize(_lattice_points(v, off, "on"), (n, 2)), v)


@functools.lru_cache(maxsize=None)
def lattice_far(v, off, form, n):
    """the lattice repeated to n - 1 rows and one point far out on both axes, off + K v: the minimum stays, so every lattice
    key stays, and the key extents ask for the 64-bit or the pair form of the sort"""
    far = off + LATTICE_FAR[form] * v
    pts = np.concatenate([np.resize(_lattice_points(v, off, "on"), (n - 1, 2)), [[far, far]]])
    return _frozen(_lattice_name(v, off, "on") + f"_far_{form}_x{n}", pts, v)


# ── refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────────
REFUSAL_ROWS = (64, 2048, 8193)                     # the LDS path, a register shape, the large path
REFUSAL_KINDS = ("apart", "tiny_voxel")


@functools.lru_cache(maxsize=None)
def refusal(kind, n):
    """Clouds whose key range does not fit 63 bits.  "apart": voxel 0.5 and two points 3.2e9 voxels apart on both axes (the
    extents' product is 1.02e19), the other rows near the first.  "tiny_voxel": a voxel of 1e-300 and a cloud some 1e10
    across, where (max - min) / voxel overflows and the extent is infinite."""
    rng = np.random.default_rng(9900 + n)
    pts = rng.uniform(-5.0, 5.0, size=(n, 2))
    if kind == "apart":
        pts[n // 3] = pts.min(axis=0) + 3.2e9 * 0.5
        return _frozen(f"refusal_apart_{n}", pts, 0.5)
    return _frozen(f"refusal_tiny_voxel_{n}", pts * 1.0e9, 1e-300)


# ── the families ────────────────────────────────────────────────────────────────────────────────────────────────────────
def one_voxel_cases():
    return [one_voxel(n, dim) for dim in (2, 3) for n in ONE_VOXEL_N[dim]]


def run_cases():
    return [runs(n, dim) for dim in (2, 3) for n in RUN_ROWS]


def cluster_cases():
    out = [clusters(side, n, dim) for dim in (2, 3) for n in CLUSTER_ROWS for side in CLUSTER_SIDES]
    return [c for c in out if c is not None]


def lattice_cases():
    out = [lattice(v, off, s) for v in LATTICE_V for off in LATTICE_OFF for s in LATTICE_SHIFTS]
    out += [lattice_tiled(v, off, n) for v in LATTICE_V for off in LATTICE_OFF for n in LATTICE_TILED]
    out += [lattice_far(v, off, form, n) for v in RECIPROCAL_V[:1] for off in RECIPROCAL_OFF for form in LATTICE_FAR
            for n in (401, 2048)]
    return out


def refusal_cases():
    return [refusal(kind, n) for kind in REFUSAL_KINDS for n in REFUSAL_ROWS]


FAMILIES = {"one_voxel": one_voxel_cases, "runs": run_cases, "clusters": cluster_cases, "lattices": lattice_cases}


def all_cases():
    """every case the filter answers (the refusals are apart: they have no output)"""
    return [c for fam in FAMILIES.values() for c in fam()]


@functools.lru_cache(maxsize=None)
def _reference(name):
    _, pts, voxel = BY_NAME[name]
    means = vr.voxel_ref(pts, voxel)
    means.setflags(write=False)
    return means


def reference(case):
    """voxel_ref of a case, computed once and shared (read-only)"""
    return _reference(case[0])


BY_NAME = {c[0]: c for c in all_cases()}
assert len(BY_NAME) == len(all_cases())
