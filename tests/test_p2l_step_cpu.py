"""One point-to-line step and the covariance normals, against extended precision — the part that needs no GPU.

This module holds
  * ``step_reference``: the normal equations of reference icp.py:88-104 formed and solved EXACTLY (integer arithmetic
    on the float64 inputs, rationals for the 3x3 solve), with a singularity verdict;
  * ``normals_reference``: the eigenvector of the np.longdouble covariance of the oracle's neighbour sets;
  * the case generators of both sweeps;
  * the table of what NumPy's own float64 formulas lose against those references, per family.  The GPU tests
    (tests/test_p2l_step_gpu.py) import the table: every bound there is 8 x a figure below, with a floor.

Measured tables (float64 NumPy against the references; units are defined at ``backward_error``, ``forward_multiple``
and ``normal_angle_units``; "NumPy" is the measured maximum, to three digits rounded up, "bound" is what the kernels
are held to: 8 x NumPy, with a floor of 4 for the backward error and of 8 for the normals):

  step family    NumPy backward  bound | NumPy forward  bound
  room                1.37       10.96 |   0.354        2.832
  hallway_2e-2        0.78        6.24 |   0.057        0.456
  hallway_1e-4        1.03        8.24 |   6.18e-05     4.944e-4
  hallway_1e-7        0.0147      4    |   (kappa 2^-52 >= 1e-6 throughout: not checked)
  off0                1.11        8.88 |   0.477        3.816
  off50               0.801       6.408|   0.0147       0.1176
  off2e3              4.22       33.76 |   (not checked)
  theta               1.97       15.76 |   0.34         2.72
  corner_a            1.42       11.36 |   0.442        3.536
  corner_b            1.53       12.24 |   0.249        1.992
  off2e4, wall_turned, dup, last_row: numerically singular (finite output and a proper rotation only);
  wall_axis and K = 0: exactly singular (identity).

  The pairs of the fused kernels (``fused_cases``) are other problems than the stand-alone cases of the same name: the
  normals are estimated from jittered geometry, the correspondences are nearest neighbours and leave a residual, and
  kappa differs by orders of magnitude (hallway_1e-4: 1e2 here, 1e8 above).  NumPy's float64 step is therefore measured
  on those pairs themselves, with the oracle's normals, and the fused kernels are held to that table:

  fused family   NumPy backward  bound | NumPy forward  bound
  room                0.867       6.936|   0.687        5.496
  hallway_2e-2        0.852       6.816|   0.0738       0.5904
  hallway_1e-4        0.209       4    |   0.0291       0.2328
  hallway_1e-7        0.112       4    |   0.0695       0.556
  off0                0.413       4    |   0.347        2.776
  off50               0.146       4    |   0.00262      0.02096
  theta               1.64       13.12 |   0.639        5.112

  normals family  NumPy eigh(np.cov)  bound
  thin                0.944            8
  axis                0.000113         8
  diag                0.000245         8
  corner              1.17             9.36
  small               1.9             15.2     (two or three rows, exact duplicates at 160 and 4200 rows)
  parity              1.54            12.32    (the clouds of tests/test_gpu_parity.py, k up to 5000)

The two tables are printed by ``test_print_the_measured_tables`` (run with -s) and asserted case by case.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import oracle
from conftest import load_golden

LD = np.longdouble
U = 2.0 ** -52
GAP_MIN = 1e-6                 # a normal is compared when (l1 - l0) / l1 of the longdouble covariance is at least this
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 511, 512, 513, 1025, 2049)
THETA_BANDS = (("tiny", 0.0, 1e-8), ("small", 1e-3, 0.2), ("below", 0.2499, 0.25), ("above", 0.25, 0.2501),
               ("mid", 0.25, 1.0), ("large", 1.0, np.pi), ("beyond", np.pi, np.inf))

# family: (largest backward error of NumPy's float64 step in units of 2^-52, largest forward error of it as a multiple
# of kappa * 2^-52 * |x|), as test_numpy_step_stays_within_the_table measures them, to three digits rounded up
P2L_TABLE = {
    "room": (1.37, 0.354),
    "hallway_2e-2": (0.78, 0.057),
    "hallway_1e-4": (1.03, 6.18e-05),
    "hallway_1e-7": (0.0147, 0.0),        # kappa * 2^-52 is never below 1e-6 here: no forward check
    "off0": (1.11, 0.477),
    "off50": (0.801, 0.0147),
    "off2e3": (4.22, 0.0),                # no forward check either
    "theta": (1.97, 0.34),
    "corner_a": (1.42, 0.442),
    "corner_b": (1.53, 0.249),
}
# the same two figures for the pairs of ``fused_cases``, measured on those pairs with the oracle's normals
# (test_numpy_step_on_the_fused_pairs_stays_within_its_table)
FUSED_TABLE = {
    "room": (0.867, 0.687),
    "hallway_2e-2": (0.852, 0.0738),
    "hallway_1e-4": (0.209, 0.0291),
    "hallway_1e-7": (0.112, 0.0695),
    "off0": (0.413, 0.347),
    "off50": (0.146, 0.00262),
    "theta": (1.64, 0.639),
}
BACKWARD_FLOOR, NORMALS_FLOOR, FACTOR = 4.0, 8.0, 8.0
# The tables hold the measured maxima themselves and the kernels' bounds are max(floor, 8 x table), nothing more.  This
# cap concerns only the self-check of this file, NumPy on the host against the table: A.T @ A goes through BLAS, whose
# order of summation differs between builds and processors, so another host may measure somewhat other maxima.
HOST_NUMPY_CAP = 2.0

# family: largest angle between float64 eigh(np.cov) and the longdouble eigenvector, in units of 2^-52 * l1 / (l1 - l0)
NORMALS_TABLE = {
    "thin": 0.944,
    "axis": 0.000113,
    "diag": 0.000245,
    "corner": 1.17,
    "small": 1.9,
    "parity": 1.54,
}


def backward_bound(family, table=P2L_TABLE):
    return max(BACKWARD_FLOOR, FACTOR * table[family][0])


def forward_bound(family, table=P2L_TABLE):
    return FACTOR * table[family][1]


def normals_bound(family):
    return max(NORMALS_FLOOR, FACTOR * NORMALS_TABLE[family])


# ── exact arithmetic on float64 data ─────────────────────────────────────────
def _exact_ints(*arrays):
    """float64 arrays -> (object arrays of Python ints, shift S): every value equals int / 2**S exactly."""
    arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
    emin = 0
    for a in arrays:
        nz = a[a != 0]
        if nz.size:
            emin = min(emin, int(np.frexp(nz)[1].min()))            # |v| = m 2^e with m in [0.5, 1): v 2^(53 - e) is whole
    S = 53 - emin
    assert S < 900, "values too small to scale exactly"
    out = []
    for a in arrays:
        ints = np.empty(a.size, dtype=object)
        ints[:] = [int(v) for v in np.ldexp(a.ravel(), S).tolist()]
        out.append(ints.reshape(a.shape))
    return out, S


def _isum(a):
    return sum(a.tolist(), 0)


def _to_ld(fr):
    """Fraction -> np.longdouble, correct to the longdouble's last bits."""
    fr = Fraction(fr)
    n, d = abs(fr.numerator), fr.denominator
    if n == 0:
        return LD(0)
    k = 90 - (n.bit_length() - d.bit_length())
    q = (n << k) // d if k >= 0 else n // (d << -k)                   # about 90 significant bits
    hi, lo = q >> 45, q & ((1 << 45) - 1)
    val = np.ldexp(np.ldexp(LD(float(hi)), 45) + LD(float(lo)), -k)
    return -val if fr < 0 else val


def _inverse3(M):
    """Exact inverse of a 3x3 matrix of Fractions by the adjugate, or None when it is singular."""
    (a, b, c), (d, e, f), (g, h, i) = M
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e],
           [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
    if det == 0:
        return None
    return [[v / det for v in row] for row in adj]


def _norm_inf(M):
    return max(sum(abs(v) for v in row) for row in M)


def pivot_trace(A, exact=False):
    """Replays LU with partial pivoting on a 3x3 matrix: (row chosen as first pivot, second-column swap?, a pivot
    exactly zero?).  ``exact`` eliminates in rationals, otherwise in float64 as the kernels do."""
    A = [[Fraction(float(v)) if exact else float(v) for v in row] for row in np.asarray(A, dtype=np.float64)]
    first, swapped = 0, False
    for c in range(3):
        piv = c
        for r in range(c + 1, 3):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        if c == 0:
            first = piv
        if c == 1:
            swapped = piv != c
        A[c], A[piv] = A[piv], A[c]
        if A[c][c] == 0:
            return first, swapped, True
        for r in range(c + 1, 3):
            f = A[r][c] / A[c][c]
            for q in range(c + 1, 3):
                A[r][q] -= f * A[c][q]
    return first, swapped, False


def numpy_step(src, tgt, normals, idx):
    """NumPy's float64 point-to-line step, rewritten from reference icp.py:88-115 -> (x or None, ATA, ATb); x is
    None where np.linalg.solve raises LinAlgError (the reference returns identity there, icp.py:107-108)."""
    q, nm, p = tgt[idx], normals[idx], src
    nx, ny = nm[:, 0], nm[:, 1]
    px, py = p[:, 0], p[:, 1]
    dx, dy = px - q[:, 0], py - q[:, 1]
    c = ny * px - nx * py
    A = np.column_stack([c, nx, ny])
    b = -(nx * dx + ny * dy)
    ATA, ATb = A.T @ A, A.T @ b
    try:
        x = np.linalg.solve(ATA, ATb)
    except np.linalg.LinAlgError:
        x = None
    return x, ATA, ATb


def step_reference(src, tgt, normals, idx, max_corr_dist=None, dists=None):
    """One point-to-line step (reference icp.py:88-115) without rounding.

    src (K, 2), tgt (M, 2), normals (M, 2) float64, idx (K,) rows of tgt.  With ``max_corr_dist`` only the rows with
    dists**2 < max_corr_dist**2 enter (icp.py:183-185; ``dists`` defaults to the float64 distance to the match).
    The sums M = A^T A and v = A^T b are exact (integers over a power of two); x = M^-1 v is exact (rationals).

    Returns a dict: theta, tx, ty (float64 nearest the exact solution; identity where the verdict is "exact"),
    x (the three Fractions, None when M is singular), M, v (Fractions), M_ld, v_ld (np.longdouble), kappa (exact
    infinity-norm condition number of M as a float, inf when singular), K (rows used) and verdict:
      "exact"     a pivot is exactly zero when LU with partial pivoting runs in exact arithmetic on the float64 sums:
                  NumPy raises LinAlgError there and the step is the identity;
      "numerical" kappa(M) * 2^-52 >= 1: the float64 answer carries no digits;
      "regular"   everything else.
    """
    src = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    tgt, normals = np.asarray(tgt, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    if max_corr_dist is not None:
        if dists is None:
            dists = np.sqrt(np.sum((src - tgt[idx]) ** 2, axis=1))
        keep = dists ** 2 < max_corr_dist ** 2
        src, idx = src[keep], idx[keep]
    (P, Q), sp = _exact_ints(src, tgt[idx])
    (N,), sn = _exact_ints(normals[idx])
    px, py, qx, qy, nx, ny = P[:, 0], P[:, 1], Q[:, 0], Q[:, 1], N[:, 0], N[:, 1]
    c = ny * px - nx * py                                               # icp.py:97, scale 2^(sp + sn)
    b = -(nx * (px - qx) + ny * (py - qy))                              # icp.py:101, same scale
    rows = [c, nx * (1 << sp), ny * (1 << sp)]
    den = 1 << (2 * (sp + sn))
    M = [[Fraction(_isum(rows[r] * rows[q]), den) for q in range(3)] for r in range(3)]
    v = [Fraction(_isum(rows[r] * b), den) for r in range(3)]
    inv = _inverse3(M)
    x = None if inv is None else [sum(inv[r][q] * v[q] for q in range(3)) for r in range(3)]
    kappa = float("inf") if inv is None else float(_norm_inf(M) * _norm_inf(inv))
    _, ATA, _ = numpy_step(src, tgt, normals, idx)
    if pivot_trace(ATA, exact=True)[2]:
        verdict, sol = "exact", (0.0, 0.0, 0.0)
    else:
        verdict = "numerical" if kappa * U >= 1.0 else "regular"
        sol = tuple(float(_to_ld(f)) for f in x) if x is not None else (float("nan"),) * 3
    return dict(theta=sol[0], tx=sol[1], ty=sol[2], x=x, M=M, v=v, kappa=kappa, K=len(src), verdict=verdict,
                M_ld=np.array([[_to_ld(f) for f in row] for row in M], dtype=LD),
                v_ld=np.array([_to_ld(f) for f in v], dtype=LD))


def backward_error(ref, x):
    """|M x - v|_inf / (|M|_inf |x|_inf + |v|_inf) in units of 2^-52 for a float64 x = (theta, tx, ty); M and v exact."""
    xf = [Fraction(float(t)) for t in x]
    res = max(abs(sum(ref["M"][r][q] * xf[q] for q in range(3)) - ref["v"][r]) for r in range(3))
    scale = _norm_inf(ref["M"]) * max(abs(t) for t in xf) + max(abs(t) for t in ref["v"])
    return float(res / scale) / U if scale else 0.0


def forward_multiple(ref, x):
    """|x - x_exact|_inf as a multiple of kappa * 2^-52 * |x_exact|_inf."""
    err = max(abs(Fraction(float(a)) - b) for a, b in zip(x, ref["x"]))
    return float(err / max(abs(b) for b in ref["x"])) / (ref["kappa"] * U)


def recover_theta(R, theta_ref):
    """atan2(R[1,0], R[0,0]), on the branch of ``theta_ref`` when that lies beyond +-pi."""
    th = float(np.arctan2(R[1, 0], R[0, 0]))
    if abs(theta_ref) > np.pi:
        th += 2 * np.pi * np.round((theta_ref - th) / (2 * np.pi))
    return th


def trig_ulps(R):
    """(ulps of R[0,0] off cos(theta), ulps of R[1,0] off sin(theta)) for theta = atan2(R[1,0], R[0,0]) in
    np.longdouble; an ulp is the spacing of float64 at the exact value.  cos and sin of that angle are R[0,0] / h and
    R[1,0] / h with h = hypot(R[0,0], R[1,0]): evaluated so, because an angle next to +-pi or +-pi/2 rounds, even in
    np.longdouble, by more than a float64 ulp of a sine or cosine next to zero."""
    c, s = LD(R[0, 0]), LD(R[1, 0])
    h = np.hypot(c, s)
    out = []
    for got, want in ((c, c / h), (s, s / h)):
        ulp = np.spacing(abs(float(want))) if want != 0 else np.spacing(0.0)
        out.append(float(abs(got - want) / LD(ulp)))
    return tuple(out)


def theta_band(theta):
    """Names of the bands of THETA_BANDS |theta| falls in: (0, 1e-8), (1e-3, 0.2), (0.2499, 0.25), [0.25, 0.2501),
    (0.25, 1), (1, pi), beyond pi."""
    a, names = abs(theta), []
    for name, lo, hi in THETA_BANDS:
        if name == "above":
            hit = lo <= a < hi
        else:
            hit = lo < a < hi
        if hit:
            names.append(name)
    return names


# ── the cases of the step sweep ──────────────────────────────────────────────
def _unit(angle):
    return np.column_stack([np.cos(angle), np.sin(angle)])


def _room(rng, m, noise, half=(5.0, 3.0)):
    """m points on the four walls of a room about the origin, with unit normals turned by N(0, noise)."""
    wall = np.arange(m) % 4
    s = rng.uniform(-1, 1, size=m)
    pts = np.where((wall < 2)[:, None], np.column_stack([s * half[0], np.where(wall == 0, -half[1], half[1])]),
                   np.column_stack([np.where(wall == 2, -half[0], half[0]), s * half[1]]))
    base = np.where(wall < 2, np.pi / 2, 0.0) + np.where(wall % 2 == 1, 0.0, np.pi)
    return pts, _unit(base + rng.normal(scale=noise, size=m))


def _hallway(rng, m, noise):
    wall = np.arange(m) % 2
    pts = np.column_stack([rng.uniform(-5, 5, size=m), np.where(wall == 0, -1.0, 1.0)])
    return pts, _unit(np.where(wall == 0, -np.pi / 2, np.pi / 2) + rng.normal(scale=noise, size=m))


def _small_corner(rng, m, heavy):
    """Two short walls 0.1 m from the origin.  c = ny px - nx py stays below 0.2 and keeps one sign on either wall, so
    sum(c nx) or sum(c ny) is the largest entry of the first column: with most points on the wall with normal (1, 0)
    (heavy = 0) row 1 is the first pivot, with most on the other (heavy = 1) row 2."""
    wall = (rng.uniform(size=m) < 0.15).astype(int) ^ heavy
    s = rng.uniform(0.05, 0.15, size=m)
    pts = np.where((wall == 0)[:, None], np.column_stack([np.full(m, 0.1), s]), np.column_stack([s, np.full(m, 0.02)]))
    return pts, _unit(np.where(wall == 0, 0.0, np.pi / 2) + rng.normal(scale=1e-2, size=m))


def _sources_for(rng, q, n, x_star, noise):
    """Sources whose exact least-squares step is x_star up to ``noise``: the matched target moved along its tangent,
    then along its normal by -(A x_star).  c = ny px - nx py does not change along the normal, so b = A x_star."""
    tang = np.column_stack([-n[:, 1], n[:, 0]])
    p0 = q + tang * rng.uniform(-0.02, 0.02, size=(len(q), 1)) + n * rng.normal(scale=noise, size=(len(q), 1))
    c = n[:, 1] * p0[:, 0] - n[:, 0] * p0[:, 1]
    return p0 - n * (c * x_star[0] + n[:, 0] * x_star[1] + n[:, 1] * x_star[2])[:, None]


def _case(rng, family, k, cloud, x_star=None, noise=1e-3, offset=0.0, idx_mode="any", name=None):
    m = max(k, 1) + 5                                                   # more target rows than matches: a real gather
    tgt, nrm = cloud(m)
    tgt = tgt + offset
    if idx_mode == "any":
        idx = rng.permutation(m)[:k]
    elif idx_mode == "dup":
        idx = np.full(k, int(rng.integers(m)))
    else:
        idx = np.full(k, m - 1)
    if x_star is None:
        x_star = (rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
    src = _sources_for(rng, tgt[idx], nrm[idx], x_star, noise)
    return dict(name=name or f"{family}/K{k}", family=family, src=src, tgt=tgt, normals=nrm, idx=idx.astype(np.int32))


@functools.lru_cache(maxsize=None)
def step_cases():
    """The sweep of the stand-alone step: every family at every size of SIZES, the pivot-order families and the
    theta bands.  Deterministic; the references are computed once (``step_references``)."""
    rng = np.random.default_rng(20260)
    out = []
    for k in SIZES:
        out.append(_case(rng, "room", k, lambda m: _room(rng, m, 1e-2)))
        for noise in ("2e-2", "1e-4", "1e-7"):
            out.append(_case(rng, f"hallway_{noise}", k, lambda m: _hallway(rng, m, float(noise))))
        # offsets: c = ny px - nx py grows with the offset and takes the first pivot.  At 2e4 m the column of c is
        # the offset's combination of the two normal columns up to 1 part in 4e3: kappa is about 1 / 2^-52, "numerical"
        for off, tag in ((0.0, "off0"), (50.0, "off50"), (2.0e3, "off2e3"), (2.0e4, "off2e4")):
            out.append(_case(rng, tag, k, lambda m: _room(rng, m, 1e-2), offset=np.array([off, -0.75 * off])))
        # one wall along an axis, normals exactly (0, +-1) or (+-1, 0): a zero column, exactly singular
        horiz = k % 2 == 0

        def axis_wall(m, horiz=horiz):
            s, sign = rng.uniform(-4, 4, size=m), np.where(rng.uniform(size=m) < 0.5, -1.0, 1.0)
            zero = np.zeros(m)
            return ((np.column_stack([s, np.full(m, 1.5)]), np.column_stack([zero, sign])) if horiz else
                    (np.column_stack([np.full(m, -2.5), s]), np.column_stack([sign, zero])))
        out.append(_case(rng, "wall_axis", k, axis_wall))
        ang = rng.uniform(0.2, 1.3)

        def turned_wall(m, ang=ang):
            s = rng.uniform(-4, 4, size=m)
            d, n = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
            return s[:, None] * d + 1.5 * n, np.tile(n, (m, 1))
        out.append(_case(rng, "wall_turned", k, turned_wall))
        out.append(_case(rng, "dup", k, lambda m: _room(rng, m, 1e-2), idx_mode="dup"))
        out.append(_case(rng, "last_row", k, lambda m: _room(rng, m, 1e-2), idx_mode="last"))
    for i in range(16):                                                  # rows 1 and 2 as first pivot
        for heavy, tag in ((0, "corner_a"), (1, "corner_b")):
            k = (63, 64, 65, 200, 511, 513)[i % 6]
            out.append(_case(rng, tag, k, lambda m: _small_corner(rng, m, heavy), name=f"{tag}/{i}"))
    spans = dict(tiny=(1e-10, 9e-9), small=(2e-3, 0.19), below=(0.24992, 0.24998), above=(0.25002, 0.25008),
                 mid=(0.3, 0.9), large=(1.2, 3.0), beyond=(3.3, 7.0))
    for band, (lo, hi) in spans.items():                                 # theta bands, both signs
        for i in range(12):
            th = rng.uniform(lo, hi) * (1 if i % 2 == 0 else -1)
            k = (63, 64, 65, 511, 513, 130)[i % 6]
            out.append(_case(rng, "theta", k, lambda m: _room(rng, m, 1e-2), noise=0.0,
                             x_star=(th, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)), name=f"theta/{band}/{i}"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def step_references():
    return tuple(step_reference(c["src"], c["tgt"], c["normals"], c["idx"]) for c in step_cases())


# ── one-iteration clouds for the fused kernels ───────────────────────────────
def _wall_points(rng, n, p0, p1, jitter):
    s = np.sort(rng.uniform(0, 1, size=n))
    d = np.asarray(p1, dtype=np.float64) - p0
    nrm = np.array([-d[1], d[0]]) / np.hypot(*d)
    return np.asarray(p0) + s[:, None] * d + nrm * rng.normal(scale=jitter, size=(n, 1)) if jitter else np.asarray(p0) + s[:, None] * d


def _room_cloud(rng, n, jitter=2e-3, half=(5.0, 3.0)):
    a, b = half
    q = max(n // 4, 1)
    walls = [((-a, -b), (a, -b)), ((a, -b), (a, b)), ((a, b), (-a, b)), ((-a, b), (-a, -b))]
    return np.vstack([_wall_points(rng, q if i else n - 3 * q, *w, jitter) for i, w in enumerate(walls)])


def _moved(rng, pts, ang, shift, keep=None):
    c, s = np.cos(ang), np.sin(ang)
    out = pts @ np.array([[c, -s], [s, c]]).T + shift
    return out if keep is None else out[rng.permutation(len(out))[:keep]]


def _turn_landing_on(tgt, shift, goal):
    """A turn of the source after which one step on nearest-neighbour correspondences solves theta = ``goal`` to 2e-5.
    The solved angle is not the turn (the matches of a turned room slide along its walls) but follows it piecewise
    continuously, so it is bracketed on a grid and bisected, in float64 with the oracle's normals."""
    T = oracle.voxel_downsample(tgt, FUSED_VOXEL)
    nrm = oracle.normals_2d(T, FUSED_NORMAL_K)

    def solved(ang):
        P = oracle.voxel_downsample(_moved(None, tgt, ang, shift), FUSED_VOXEL)
        return numpy_step(P, T, nrm, oracle.nn(P, T)[1])[0][0] - goal
    grid = np.linspace(0.2, 0.8, 61) * (-1 if goal > 0 else 1)
    for lo, hi in zip(grid[:-1], grid[1:]):
        if solved(lo) * solved(hi) > 0:
            continue
        for _ in range(45):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if solved(lo) * solved(mid) > 0 else (lo, mid)
        if abs(solved(lo)) < 2e-5:
            return lo
    raise AssertionError(f"no turn solves theta = {goal}")


@functools.lru_cache(maxsize=None)
def fused_cases():
    """(family, source, target[, max_corr_dist]) for one iteration of the fused kernels: the families of the
    stand-alone sweep built as geometry (the normals are the library's own), 4 to 400 points, a target above 4096
    rows, a source above 2048 rows and gated pairs."""
    rng = np.random.default_rng(20261)
    out = []
    for n in (4, 5, 17, 64, 130, 400):
        tgt = _room_cloud(rng, n)
        out.append(("room", _moved(rng, tgt, rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.05, 2)), tgt, None))
    for jitter, tag in ((3e-2, "hallway_2e-2"), (1e-4, "hallway_1e-4"), (1e-7, "hallway_1e-7")):
        for n in (40, 400):
            tgt = np.vstack([_wall_points(rng, n // 2, (-5, -1), (5, -1), jitter), _wall_points(rng, n - n // 2, (-5, 1), (5, 1), jitter)])
            out.append((tag, _moved(rng, tgt, rng.uniform(-0.01, 0.01), rng.uniform(-0.03, 0.03, 2)), tgt, None))
    for n in (9, 120):                                                   # one wall on an axis: exactly singular
        for horiz in (True, False):
            s = np.sort(rng.uniform(-4, 4, size=n))
            tgt = np.column_stack([s, np.full(n, 1.5)]) if horiz else np.column_stack([np.full(n, -2.5), s])
            out.append(("wall_axis", tgt + rng.uniform(-0.02, 0.02, size=2), tgt, None))
    for n in (9, 120):                                                   # the same wall turned: numerically singular
        tgt = _wall_points(rng, n, (-3, -1), (2.5, 1.7), 0.0)
        out.append(("wall_turned", tgt + rng.uniform(-0.02, 0.02, size=2), tgt, None))
    for off, tag in ((0.0, "off0"), (50.0, "off50"), (2.0e4, "off2e4")):
        for n in (30, 300):
            tgt = _room_cloud(rng, n) + np.array([off, -0.75 * off])
            out.append((tag, _moved(rng, tgt - [off, -0.75 * off], rng.uniform(-0.02, 0.02), rng.uniform(-0.05, 0.05, 2))
                        + [off, -0.75 * off], tgt, None))
    for ang in (1e-9, -1e-9, 0.05, -0.1, 0.2497, -0.2497, 0.2503, -0.2503, 0.4, -0.7, 1.3, -2.0, 3.0, -3.1):
        tgt = _room_cloud(rng, 200)                                      # sources turned so that theta spreads over the bands
        out.append(("theta", _moved(rng, tgt, ang, rng.uniform(-0.05, 0.05, 2)), tgt, None))
    tgt = _room_cloud(rng, 60)                                           # every source next to one target
    out.append(("dup", tgt[7] + rng.normal(scale=1e-3, size=(25, 2)), tgt, None))
    out.append(("last_row", tgt[-1] + rng.normal(scale=1e-3, size=(25, 2)), tgt, None))
    big = _room_cloud(rng, 4400)                                         # target above 4096 rows: streamed / through L2
    out.append(("room", _moved(rng, big, 0.01, np.array([0.02, -0.03]), keep=500), big, None))
    wide = _room_cloud(rng, 2300)                                        # source above 2048 rows: several row slots
    out.append(("room", _moved(rng, wide, -0.01, np.array([-0.02, 0.01])), _room_cloud(rng, 900), None))
    # gate: 300-row source of which 3..10 rows lie within max_corr_dist.  max(3, 300 // 10) = 30 inliers are required
    # (icp.py:186), so this pair stops before its first step, as the reference does
    tgt = _room_cloud(rng, 300)
    src = _moved(rng, tgt, 0.0, np.array([0.9, 0.7]))
    src[:6] = tgt[:6] + rng.normal(scale=1e-3, size=(6, 2))
    out.append(("gate_few", src, tgt, 0.05))
    # the same gate on 30 rows, where max(3, 30 // 10) = 3: the step runs on the survivors alone
    for n_in in (3, 6, 10):
        tgt = _room_cloud(rng, 120)
        pick = rng.permutation(120)[:30]
        src = tgt[pick] + np.array([0.9, 0.7])
        src[:n_in] = tgt[pick[:n_in]] + rng.normal(scale=2e-3, size=(n_in, 2)) + [0.004, -0.003]
        out.append(("room", src, tgt, 0.05))
    rng = np.random.default_rng(20262)                                   # theta on either side of the 0.25 rad switch
    for goal in (0.24995, -0.24995, 0.25005, -0.25005):
        tgt, shift = _room_cloud(rng, 200), rng.uniform(-0.03, 0.03, 2)
        out.append(("theta", _moved(rng, tgt, _turn_landing_on(tgt, shift, goal), shift), tgt, None))
    return tuple(out)


FUSED_VOXEL, FUSED_NORMAL_K = 1e-4, 12       # every point its own voxel; the default normal_k


def fused_step_inputs(src, tgt, gate, normals_of):
    """What one iteration of the fused kernels works on: the voxel-filtered clouds, the normals of the filtered target
    (``normals_of(T, k)``: the library's on the device, the oracle's here), the nearest neighbours and their distances,
    and the rows inside the gate (icp.py:183-185)."""
    P, T = oracle.voxel_downsample(src, FUSED_VOXEL), oracle.voxel_downsample(tgt, FUSED_VOXEL)
    d, idx = oracle.nn(P, T)
    keep = d ** 2 < gate ** 2 if gate is not None else np.ones(len(P), dtype=bool)
    return P, T, normals_of(T, FUSED_NORMAL_K), idx, d, keep


# ── normals ──────────────────────────────────────────────────────────────────
def normals_reference(pts, k):
    """Per point: the unit eigenvector of the smaller eigenvalue of the np.longdouble covariance of the oracle's
    k + 1 nearest neighbours (icp.py:61-73), the relative eigen-gap (l1 - l0) / l1 and the neighbour rows.
    One point alone has no covariance: (1, 0) with gap 0."""
    pts = np.asarray(pts, dtype=np.float64)
    m = len(pts)
    kk = min(k, m - 1) + 1
    if kk < 2:
        return np.tile(np.array([1.0, 0.0], dtype=LD), (m, 1)), np.zeros(m), np.zeros((m, 1), dtype=np.int32)
    _, nb = oracle.knn(pts, pts, kk)
    d = pts[nb].astype(LD) - pts[:, None, :].astype(LD)                 # shift by the query: exact or 2^-64 relative
    d = d - d.mean(axis=1, keepdims=True)
    a, b, c = (d[..., 0] ** 2).sum(1), (d[..., 0] * d[..., 1]).sum(1), (d[..., 1] ** 2).sum(1)
    rad2 = np.hypot(a - c, 2 * b)                                       # l1 - l0 (times kk - 1, which cancels)
    l1 = 0.5 * (a + c + rad2)
    gap = np.where(l1 > 0, rad2 / np.where(l1 > 0, l1, 1), 0).astype(np.float64)
    phi = 0.5 * np.arctan2(2 * b, a - c)                                 # direction of the larger eigenvalue
    return np.stack([-np.sin(phi), np.cos(phi)], axis=1), gap, nb


def numpy_normals(pts, nb):
    """float64 np.linalg.eigh on float64 np.cov of the same neighbours (icp.py:70-73)."""
    out = np.zeros((len(pts), 2))
    for i in range(len(pts)):
        out[i] = np.linalg.eigh(np.cov(pts[nb[i]].T))[1][:, 0]
    return out


def normal_angle_units(got, ref, gap):
    """Angle between ``got`` (float64, either sign) and the longdouble eigenvector, in units of 2^-52 l1 / (l1 - l0)."""
    g = np.asarray(got).astype(LD)
    cross = np.abs(g[:, 0] * ref[:, 1] - g[:, 1] * ref[:, 0])
    dot = np.abs(g[:, 0] * ref[:, 0] + g[:, 1] * ref[:, 1])
    return (np.arctan2(cross, dot) * gap / U).astype(np.float64)


def _thin_wall(rng, n, thickness, offset, ang=0.3):
    s = rng.uniform(-3, 3, size=n)
    d, nrm = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
    return s[:, None] * d + nrm * rng.uniform(-0.5, 0.5, size=(n, 1)) * thickness + np.array([offset, -0.75 * offset])


def normal_clouds(n, seed=5):
    """(name, table family or None, cloud, kind) for the normals sweep at about n rows.  kind "wall": every point
    with a defined direction is compared and at most 2 % may lack one; "free": isotropic, only finite unit output."""
    rng = np.random.default_rng(seed + n)
    out = []
    for th in (1e-3, 1e-6, 0.0):
        for off in (0.0, 50.0, 2.0e4):
            out.append((f"thin_{th:g}@{off:g}", "thin", _thin_wall(rng, n, th, off), "wall"))
    s = rng.uniform(-3, 3, size=n)
    out.append(("axis_x", "axis", np.column_stack([s, np.full(n, 0.5)]), "wall"))           # b == 0 exactly, a > c = 0
    out.append(("axis_y", "axis", np.column_stack([np.full(n, -1.25), s]), "wall"))         # b == 0 exactly, a < c
    out.append(("axis_x@2e4", "axis", np.column_stack([s + 2.0e4, np.full(n, 0.5)]), "wall"))
    out.append(("diag", "diag", np.column_stack([s, s]), "wall"))                            # a == c == b
    out.append(("diag@50", "diag", np.column_stack([s + 50.0, s + 50.0]), "wall"))
    h = n // 2
    corner = np.vstack([np.column_stack([rng.uniform(0, 3, h), rng.normal(scale=1e-3, size=h)]),
                        np.column_stack([rng.normal(scale=1e-3, size=n - h), rng.uniform(0, 3, n - h)])])
    out.append(("corner", "corner", corner, "wall"))
    out.append(("corner@2e4", "corner", corner @ _unit(np.array([0.4, 0.4 + np.pi / 2])).T + [2.0e4, -1.5e4], "wall"))
    return out


def small_normal_clouds():
    """The clouds whose size is the point: one, two and three rows, exact duplicates, the isotropic ones."""
    rng = np.random.default_rng(77)
    side = 12
    lattice = np.stack(np.meshgrid(np.arange(side) * 0.125, np.arange(side) * 0.125), -1).reshape(-1, 2)
    dup = np.repeat(_thin_wall(rng, 40, 1e-3, 0.0), 4, axis=0)
    return [("one", None, np.array([[0.3, -1.2]]), "one"),
            ("two", "small", rng.normal(size=(2, 2)), "wall"),
            ("three", "small", rng.normal(size=(3, 2)), "wall"),
            ("duplicates", "small", dup, "wall"),
            ("lattice", None, lattice, "free"),
            ("identical", None, np.full((9, 2), 0.75), "free")]


# ═════════════════════════════════════════════════════════════════════════════
def test_longdouble_is_extended():
    assert np.finfo(LD).nmant >= 63, "the trigonometric and eigenvector references need an extended np.longdouble"


def test_reference_reproduces_the_golden_step():
    z = load_golden("p2l_solve")
    ref = step_reference(z["src"], z["tgt"], z["normals"], z["idx"])
    assert ref["verdict"] == "regular"
    R = np.array([[np.cos(ref["theta"]), -np.sin(ref["theta"])], [np.sin(ref["theta"]), np.cos(ref["theta"])]])
    assert np.abs(R - z["R"]).max() <= 1e-12 and np.abs(np.array([ref["tx"], ref["ty"]]) - z["t"]).max() <= 1e-12
    assert np.abs(ref["M_ld"].astype(np.float64) - numpy_step(z["src"], z["tgt"], z["normals"], z["idx"])[1]).max() \
        <= 1e-12 * float(ref["M_ld"].max())
    zero = step_reference(z["src"], z["tgt"], z["zero_normals"], z["idx"])
    assert zero["verdict"] == "exact" and (zero["theta"], zero["tx"], zero["ty"]) == (0.0, 0.0, 0.0)


def test_gate_keeps_the_rows_inside_the_distance():
    rng = np.random.default_rng(3)
    tgt, nrm = _room(rng, 40, 1e-2)
    idx = np.arange(40)
    src = tgt + np.where((np.arange(40) < 7)[:, None], 0.01, 0.5)
    gated = step_reference(src, tgt, nrm, idx, max_corr_dist=0.1)
    plain = step_reference(src[:7], tgt, nrm, idx[:7])
    assert gated["K"] == 7 and gated["M"] == plain["M"] and gated["x"] == plain["x"]


def test_generator_covers_every_pivot_order():
    """Every row is first pivot and the rows of the second column are swapped, ten times each at least.  What this
    protects is the swap itself (rows and right-hand side moved together, in all three copies of the solve), not the
    choice of the second pivot: M = A^T A is positive definite, and with M = [[a, b, d], [b, e, f], [d, f, g]] and b
    the first pivot the entry that elimination WITHOUT the second swap creates is bounded by |f| + g, so its growth
    factor stays below 3 and it is backward stable too (an exactly zero second pivot needs kappa >= 2^52)."""
    first, second = [0, 0, 0], 0
    for c, ref in zip(step_cases(), step_references()):
        if ref["verdict"] != "regular":
            continue
        f, s, singular = pivot_trace(numpy_step(c["src"], c["tgt"], c["normals"], c["idx"])[1])
        assert not singular, c["name"]
        first[f] += 1
        second += s
    assert min(first) >= 10 and second >= 10, (first, second)


def test_generator_covers_every_theta_band_with_both_signs():
    count = {name: [0, 0] for name, _, _ in THETA_BANDS}
    for c, ref in zip(step_cases(), step_references()):
        if ref["verdict"] == "regular":
            for name in theta_band(ref["theta"]):
                count[name][ref["theta"] < 0] += 1
    for name, (pos, neg) in count.items():
        assert pos + neg >= 5 and pos >= 1 and neg >= 1, (name, pos, neg)


def test_exactly_singular_family_is_where_numpy_raises():
    n_exact = 0
    for c, ref in zip(step_cases(), step_references()):
        x, ATA, _ = numpy_step(c["src"], c["tgt"], c["normals"], c["idx"])
        if ref["verdict"] == "exact":
            n_exact += 1
            assert c["family"] == "wall_axis" or len(c["idx"]) == 0, c["name"]
            assert x is None, c["name"]                                  # LinAlgError
            assert not ATA.any(axis=0).all(), c["name"]                  # a zero column: singular in any order of summation
            assert (ref["theta"], ref["tx"], ref["ty"]) == (0.0, 0.0, 0.0)
        else:
            assert c["family"] != "wall_axis"
            assert ref["verdict"] == "numerical" or (ref["theta"], ref["tx"], ref["ty"]) != (0.0, 0.0, 0.0), c["name"]
        if c["family"] in ("wall_turned", "dup", "last_row", "off2e4") and len(c["idx"]):
            assert ref["verdict"] == "numerical", c["name"]
    assert n_exact >= len(SIZES)


@functools.lru_cache(maxsize=None)
def _measure_step():
    """family -> [largest NumPy backward error, largest NumPy forward multiple] over the regular cases."""
    seen = {}
    for c, ref in zip(step_cases(), step_references()):
        if ref["verdict"] != "regular":
            continue
        x = numpy_step(c["src"], c["tgt"], c["normals"], c["idx"])[0]
        m = seen.setdefault(c["family"], [0.0, 0.0])
        m[0] = max(m[0], backward_error(ref, x))
        if ref["kappa"] * U < 1e-6:
            m[1] = max(m[1], forward_multiple(ref, x))
    return seen


def test_numpy_step_stays_within_the_table():
    seen = _measure_step()
    assert set(seen) == set(P2L_TABLE), sorted(seen)
    for fam, (bwd, fwd) in seen.items():
        assert bwd <= HOST_NUMPY_CAP * P2L_TABLE[fam][0] and fwd <= HOST_NUMPY_CAP * P2L_TABLE[fam][1], (fam, bwd, fwd)


def test_oracle_step_agrees_with_the_reference_on_regular_cases():
    for c, ref in zip(step_cases(), step_references()):
        if ref["verdict"] != "regular":
            continue
        R, t = oracle.p2l_solve_2d(c["src"], c["tgt"], c["normals"], c["idx"])
        assert R[0, 0] == R[1, 1] and R[0, 1] == -R[1, 0]
        x = (recover_theta(R, ref["theta"]), t[0], t[1])
        assert backward_error(ref, x) <= backward_bound(c["family"]), (c["name"], backward_error(ref, x))
        if ref["kappa"] * U < 1e-6:
            assert forward_multiple(ref, x) <= forward_bound(c["family"]), (c["name"], forward_multiple(ref, x))


@functools.lru_cache(maxsize=None)
def _fused_cpu():
    """(family, inputs of the step, exact reference) of every fused pair that takes a regular step, with the oracle's
    normals.  The pair that stops on the inlier rule takes none."""
    out = []
    for fam, src, tgt, gate in fused_cases():
        P, T, nrm, idx, d, keep = fused_step_inputs(src, tgt, gate, oracle.normals_2d)
        ref = step_reference(P, T, nrm, idx, max_corr_dist=gate, dists=d)
        if fam != "gate_few" and ref["verdict"] == "regular":
            out.append((fam, (P[keep], T, nrm, idx[keep]), ref))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _measure_fused():
    seen = {}
    for fam, args, ref in _fused_cpu():
        x = numpy_step(*args)[0]
        m = seen.setdefault(fam, [0.0, 0.0])
        m[0] = max(m[0], backward_error(ref, x))
        if ref["kappa"] * U < 1e-6:
            m[1] = max(m[1], forward_multiple(ref, x))
    return seen


FUSED_SINGULAR = ("wall_turned", "off2e4", "dup", "last_row")   # fused families that take a step on a singular system
FUSED_BANDS = {("small", False), ("small", True), ("below", False), ("below", True), ("above", False), ("above", True),
               ("mid", False), ("mid", True)}                          # (band, theta < 0) the fused pairs reach


def test_fused_pairs_reach_their_bands_and_verdicts():
    """Nearest-neighbour matches of a turned room do not give the turn back: one step reaches at most 0.33 rad.  The
    pairs therefore cover both signs of the Taylor path, of either side of the switch at 0.25 rad and of the library
    path beyond it; larger angles belong to the stand-alone sweep."""
    bands = set()
    for fam, _, ref in _fused_cpu():
        bands.update((b, ref["theta"] < 0) for b in theta_band(ref["theta"]))
    assert FUSED_BANDS <= bands, sorted(FUSED_BANDS - bands)
    for fam, src, tgt, gate in fused_cases():
        if fam in FUSED_SINGULAR or fam == "wall_axis":
            P, T, nrm, idx, d, keep = fused_step_inputs(src, tgt, gate, oracle.normals_2d)
            assert step_reference(P, T, nrm, idx)["verdict"] == ("exact" if fam == "wall_axis" else "numerical"), fam


def test_numpy_step_on_the_fused_pairs_stays_within_its_table():
    seen = _measure_fused()
    assert set(seen) == set(FUSED_TABLE), sorted(seen)                   # the other families take no regular step
    for fam, (bwd, fwd) in seen.items():
        assert bwd <= HOST_NUMPY_CAP * FUSED_TABLE[fam][0] and fwd <= HOST_NUMPY_CAP * FUSED_TABLE[fam][1], (fam, bwd, fwd)
        assert fwd > 0, fam                                              # every fused family has a forward check


def test_oracle_step_agrees_with_the_reference_on_the_fused_pairs():
    for fam, args, ref in _fused_cpu():
        R, t = oracle.p2l_solve_2d(*args)
        x = (recover_theta(R, ref["theta"]), t[0], t[1])
        assert backward_error(ref, x) <= backward_bound(fam, FUSED_TABLE), (fam, ref["K"], backward_error(ref, x))
        if ref["kappa"] * U < 1e-6:
            assert forward_multiple(ref, x) <= forward_bound(fam, FUSED_TABLE), (fam, ref["K"], forward_multiple(ref, x))


def exhaustive_normal_clouds():
    """(k, clouds) of the route of normals.hip (above 4096 rows, k <= 31): the whole list at 4200 rows and exact
    duplicates, each point four times."""
    rng = np.random.default_rng(78)
    dup = ("duplicates", "small", np.repeat(_thin_wall(rng, 1050, 1e-3, 0.0), 4, axis=0), "wall")
    big = normal_clouds(4200)
    return ((12, big + [dup]), (31, [big[2], big[9], dup]))


def parity_normal_clouds():
    """The clouds of tests/test_gpu_parity.py::test_normals_grid_and_sweep_searches_agree, in its order: a filtered
    room scan, a random cloud, a line, exact duplicates, a lattice, five points, seven identical points."""
    from icpmi import synth
    rng = np.random.default_rng(8)
    a, _ = synth.config2_pair(3)
    line = np.column_stack([np.linspace(-2, 2, 300), np.full(300, 0.5)])               # collinear: a one-row grid
    dup = np.repeat(rng.uniform(-1, 1, size=(40, 2)), 5, axis=0)                         # exact duplicates: ties on the row
    lattice = np.stack(np.meshgrid(np.arange(30) * 0.1, np.arange(30) * 0.1), -1).reshape(-1, 2)   # many equal distances
    return [oracle.voxel_downsample(a, 0.04), rng.uniform(-4, 4, size=(3000, 2)), line, dup, lattice,
            rng.normal(size=(5, 2)), np.zeros((7, 2))]


def parity_scan_many_neighbours():
    """The filtered scan and the k of test_normals_and_icp_with_more_than_31_neighbours."""
    from icpmi import synth
    return oracle.voxel_downsample(synth.config2_pair(5)[1], 0.04), (32, 40, 100, 5000)


PARITY_DIRECTED = (0, 1, 2)      # scan, random cloud, line: (nearly) every point has a defined direction


@functools.lru_cache(maxsize=None)
def _measure_normals():
    """family -> largest angle of float64 eigh(np.cov) off the longdouble eigenvector; and the share of points of
    every wall cloud whose eigen-gap is below GAP_MIN."""
    seen, below = {}, {}
    sweep = [(12, normal_clouds(300)), (5, normal_clouds(120)), (32, normal_clouds(300)), (40, normal_clouds(300)),
             (1, normal_clouds(60)), (10, small_normal_clouds()), (12, small_normal_clouds()), (40, small_normal_clouds())]
    sweep += list(exhaustive_normal_clouds())
    par = parity_normal_clouds()
    sweep += [(k, [(f"parity{i}", "parity", par[i], "wall" if i in PARITY_DIRECTED else "some") for i in (0, 1, 2, 3, 5)])
              for k in (12, 5, 31)]
    scan, ks = parity_scan_many_neighbours()
    sweep += [(k, [("parity_scan", "parity", scan, "wall")]) for k in ks]
    for k, clouds in sweep:
        for name, fam, pts, kind in clouds:
            if kind not in ("wall", "some"):
                continue
            ref, gap, nb = normals_reference(pts, k)
            units = normal_angle_units(numpy_normals(pts, nb), ref, gap)
            ok = gap >= GAP_MIN
            if kind == "wall":
                below[(name, len(pts), k)] = 1.0 - ok.mean()
            if ok.any():
                seen[fam] = max(seen.get(fam, 0.0), float(units[ok].max()))
    return seen, below


def test_numpy_normals_stay_within_the_table_and_walls_have_a_direction():
    seen, below = _measure_normals()
    assert set(seen) == set(NORMALS_TABLE)
    for fam, units in seen.items():
        assert units <= HOST_NUMPY_CAP * NORMALS_TABLE[fam], (fam, units)
    for key, share in below.items():        # the cap of 2 % on every wall and corner cloud, those of normals.hip included
        assert share <= 0.02, (key, share)


def test_isotropic_and_single_point_references():
    for name, fam, pts, kind in small_normal_clouds():
        ref, gap, _ = normals_reference(pts, 12)                           # 12 neighbours of a lattice point: a symmetric set
        if kind == "one":
            assert np.array_equal(ref.astype(np.float64), [[1.0, 0.0]])
        if name == "identical":
            assert (gap == 0).all()
        if name == "lattice":
            assert (gap < GAP_MIN).any()                                 # interior points: no defined direction


def test_print_the_measured_tables():
    step, (nrm, below) = _measure_step(), _measure_normals()
    print("\nstep family      NumPy backward [2^-52]  bound | NumPy forward [kappa 2^-52 |x|]  bound")
    for fam in P2L_TABLE:
        print(f"  {fam:14s} {step[fam][0]:10.3g} {backward_bound(fam):14.3g} | {step[fam][1]:12.3g} {forward_bound(fam):18.3g}")
    fused = _measure_fused()
    print("fused family     NumPy backward [2^-52]  bound | NumPy forward [kappa 2^-52 |x|]  bound")
    for fam in FUSED_TABLE:
        print(f"  {fam:14s} {fused[fam][0]:10.3g} {backward_bound(fam, FUSED_TABLE):14.3g} | {fused[fam][1]:12.3g} "
              f"{forward_bound(fam, FUSED_TABLE):18.3g}")
    print("normals family   NumPy eigh(np.cov) [2^-52 l1/(l1-l0)]  bound")
    for fam in NORMALS_TABLE:
        print(f"  {fam:14s} {nrm[fam]:10.3g} {normals_bound(fam):14.3g}")
    print("largest share of wall points without a direction:", max(below.values()))
