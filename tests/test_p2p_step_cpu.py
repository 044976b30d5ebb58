"""One point-to-point step against exact arithmetic — the part that needs no GPU.

This module holds
  * ``p2p_step_reference``: the centroids, the centred cross-covariance W and, in 2-D, a = W00 + W11 and
    b = W01 - W10 of reference icp.py:197-201 formed EXACTLY (integers over a power of two, ``Fraction``), with the
    condition number of the angle and a verdict;
  * the measures a returned step (R, t, err) is held to, each against those exact values;
  * the deterministic case generators: the pairs of ``fused_cases`` of the point-to-line module as they are, sizes,
    rotation bands, gated pairs, the pairs that put rows exactly on the gate, and the 3-D clouds;
  * the table of what NumPy's float64 restatement of icp.py:197-207 and :215 loses against the exact values, per
    family.  The GPU tests (tests/test_p2p_step_gpu.py) import it: a kernel is held to max(4, 8 x figure), nothing
    here or there is measured from a kernel.

Units of the measures
  angle        |c b - s a| / hypot(a, b) with c = R[0,0], s = R[1,0] as exact rationals: |sin| of the angle between the
               returned rotation and the optimum.  Unit: kappa * 2^-52, kappa = sum_i |p_i - mp| |q_i - mq| / hypot(a, b)
               (at least 1; the condition number of the angle).  Regular verdict only.
  translation  |t - (mq - R mp)|_inf with the returned R's float64 entries used exactly.
               Unit: 2^-52 * (mean_i |p_i|_1 + mean_i |q_i|_1) over the rows of the step.  Every verdict.
  error        |err - exact mean over ALL rows of |q_i - (R p_i + t)|^2|, returned R and t used exactly (icp.py:212-215).
               Unit: 2^-52 * mean_i (|e_i|_1 + 2^-52 s_i) s_i with e_i the exact residual of row i and
               s_i = |p_i|_1 + |q_i|_1 + |t|_1: what rounding R p_i + t and q_i - (.) to float64 does to e_i^2 to first
               order, 2 |e_i| (2^-52 s_i), plus the second-order term (2^-52 s_i)^2, which is all that is left where a
               residual is itself rounding (one row; every row on one target).  Not scaled by err: a small residual far
               from the origin is not the kernel's fault.
  skew (3-D)   |(R W - (R W)^T) / 2|_F / |W|_F, W exact: an optimal rotation makes R W symmetric.  Unit 2^-52.
  orth (3-D)   |R^T R - I|_F.  Unit 2^-52.

Measured table (NumPy float64 against the exact reference, maxima to three digits rounded up; a kernel's bound is
max(4, 8 x figure); "-" = no regular step in the family, the figure is not checked).  The self-check of NumPy on the
host against the table allows HOST_NUMPY_CAP x the figure, or 0.5 where that is more: below 0.5 a figure moves no bound
(8 x 0.5 is the floor), and wall_axis's angle, for one, is NumPy being exact on b = 0, which another LAPACK need not be:

P2P_TABLE_BEGIN
  family           angle    translation  error
  room             0.869    2.94         0.254
  hallway_2e-2     0.296    1.38         0.137
  hallway_1e-4     0.0514   1.16         0.022
  hallway_1e-7     0.103    0.314        0.0314
  wall_axis        1.55e-15 2.65         0.000861
  wall_turned      0.497    0.469        0.0071
  off0             0.164    0.276        0.0345
  off50            0.32     1.36         0.0121
  off2e3           0.0365   0.437        0.00179
  off2e4           0.493    1.01         0.0439
  theta            0.749    1.98         0.0723
  dup              -        0.365        0.00546
  last_row         -        0.338        0.00482
  size             1.63     1.23         0.0733
  big_target       0.145    0.57         0.049
  band_tiny        0.0278   0.446        0.0293
  band_small       0.208    0.229        0.0215
  band_half        0.864    0.136        0.0261
  gate_need        0.205    0.237        0.159
  edge             1.06     0.181        0.0383
P2P_TABLE_END

P2P3_TABLE_BEGIN
  family           skew     orth         translation  error
  generic          0.511    5.07         0.399        0.0106
  planar           1.42     5.45         0.714        0.06
  line             1.37     4.66         1.21         0.0509
  one_row          -        0            0            0
  off2e3           0.567    7.69         0.972        0.017
P2P3_TABLE_END

Rotation bands.  With nearest-neighbour correspondences a >= 0 always, gated or not: q_i is the nearest target of p_i,
so |p_i - q_i| <= |p_i - q_s(i)| for every permutation s of the rows of the step; summed over the rows that is
sum p_i . q_i >= sum p_i . q_s(i), and averaged over all s it is sum p_i . (q_i - mq) >= 0, which is a.  One iteration
therefore never solves an angle beyond pi / 2, and the band next to pi cannot be reached through ``IcpBatch`` by any
cloud.  The band next to pi / 2 is reached by two-row clouds turned about their centroid (more rows no longer find
their own images there).  The band next to pi is covered here, on explicit correspondences, for NumPy and for the
oracle's step (``test_explicit_correspondences_reach_every_band``).
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

import oracle
from test_p2l_step_cpu import (FACTOR, FUSED_NORMAL_K, FUSED_VOXEL, HOST_NUMPY_CAP, U, _exact_ints, _isum, _moved,
                               backward_error, forward_multiple, fused_cases, fused_step_inputs, numpy_step, recover_theta,
                               step_reference)

FLOOR = 4.0                      # the floor of every bound, in units of its measure (BACKWARD_FLOOR of the point-to-line module)
SIZES = (1, 2, 3, 4, 63, 64, 65, 511, 512, 513, 1025, 2049, 2600)       # 2600 > 2048 + 512: a second trip of icp_nn_pass
GATE = 0.05                      # the gate of the gated pairs of ``fused_cases``
K = 2.0 ** -6                    # rows displaced by (3 K, 4 K) lie exactly 5 K from their match
EDGE_GATES = (float(np.nextafter(5 * K, 0.0)), 5 * K, float(np.nextafter(5 * K, 1.0)))      # d**2 < g**2: out, out, in
P2P_BAND_EDGES = (("tiny", 0.0, 1e-8), ("small", 1e-3, 0.2), ("half", np.pi / 2 - 2e-3, np.pi / 2 + 2e-3),
                  ("pi", np.pi - 1e-3, np.pi + 1e-9))
P2P_BANDS = {(b, neg) for b in ("tiny", "small", "half") for neg in (False, True)}       # what IcpBatch can reach (see above)

# family: NumPy's (angle, translation, error) figures in the units of the module docstring; None: not checked
P2P_TABLE = {
    "room": (0.869, 2.94, 0.254),
    "hallway_2e-2": (0.296, 1.38, 0.137),
    "hallway_1e-4": (0.0514, 1.16, 0.022),
    "hallway_1e-7": (0.103, 0.314, 0.0314),
    "wall_axis": (1.55e-15, 2.65, 0.000861),
    "wall_turned": (0.497, 0.469, 0.0071),
    "off0": (0.164, 0.276, 0.0345),
    "off50": (0.32, 1.36, 0.0121),
    "off2e3": (0.0365, 0.437, 0.00179),
    "off2e4": (0.493, 1.01, 0.0439),
    "theta": (0.749, 1.98, 0.0723),
    "dup": (None, 0.365, 0.00546),
    "last_row": (None, 0.338, 0.00482),
    "size": (1.63, 1.23, 0.0733),
    "big_target": (0.145, 0.57, 0.049),
    "band_tiny": (0.0278, 0.446, 0.0293),
    "band_small": (0.208, 0.229, 0.0215),
    "band_half": (0.864, 0.136, 0.0261),
    "gate_need": (0.205, 0.237, 0.159),
    "edge": (1.06, 0.181, 0.0383),
}
# family: NumPy's (skew, orth, translation, error) figures of the 3-D step
P2P3_TABLE = {
    "generic": (0.511, 5.07, 0.399, 0.0106),
    "planar": (1.42, 5.45, 0.714, 0.06),
    "line": (1.37, 4.66, 1.21, 0.0509),
    "one_row": (None, 0.0, 0.0, 0.0),
    "off2e3": (0.567, 7.69, 0.972, 0.017),
}
# the point-to-line step on the pairs of ``edge_pairs``: NumPy's (backward, forward) figures, in the units and the
# layout of FUSED_TABLE of the point-to-line module, measured on those pairs with the oracle's normals
EDGE_P2L_TABLE = {"edge": (0.177, 0.0645)}


def bound(family, which, table=None):
    """What a kernel is held to in ``family``: max(4, 8 x NumPy's figure); ``which`` indexes the family's tuple."""
    fig = (P2P_TABLE if table is None else table)[family][which]
    assert fig is not None, (family, which)
    return max(FLOOR, FACTOR * fig)


# ── the exact reference ──────────────────────────────────────────────────────
def p2p_step_reference(P, Q, keep=None):
    """icp.py:197-201 without rounding.  P (n, d), Q (n, d) float64 (Q: the matched target rows), ``keep`` an optional
    inlier mask.  Returns a dict: n, d, mp, mq (lists of Fractions), W (d x d Fractions), scale (the translation's
    unit without its 2^-52), kappa and verdict, and in 2-D a, b (Fractions) and hyp = hypot(a, b) as a float.
    kappa = sum |p_i - mp| |q_i - mq| / hypot(a, b) (3-D: / |W|_F) in float64 of the exact centred values.
    Verdict: "zero" where a == b == 0 (3-D: W == 0) exactly, "numerical" where kappa * 2^-52 >= 1, else "regular"."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    if keep is not None:
        P, Q = P[keep], Q[keep]
    n, d = P.shape
    assert n >= 1 and Q.shape == P.shape
    (Pi, Qi), S = _exact_ints(P, Q)
    sp, sq = [_isum(Pi[:, j]) for j in range(d)], [_isum(Qi[:, j]) for j in range(d)]
    den = n << S                                                        # n p - sum p: the centred row times n 2^S
    Pc = np.stack([Pi[:, j] * n - sp[j] for j in range(d)], axis=1)
    Qc = np.stack([Qi[:, j] * n - sq[j] for j in range(d)], axis=1)
    W = [[Fraction(_isum(Pc[:, i] * Qc[:, k]), den * den) for k in range(d)] for i in range(d)]
    out = dict(n=n, d=d, mp=[Fraction(v, den) for v in sp], mq=[Fraction(v, den) for v in sq], W=W,
               scale=float(np.abs(P).sum(axis=1).mean() + np.abs(Q).sum(axis=1).mean()))
    pc, qc = (Pc / den).astype(np.float64), (Qc / den).astype(np.float64)      # int / int: correctly rounded
    spread = float(np.sum(np.sqrt((pc * pc).sum(axis=1)) * np.sqrt((qc * qc).sum(axis=1))))
    if d == 2:
        a, b = W[0][0] + W[1][1], W[0][1] - W[1][0]
        hyp, zero = math.hypot(float(a), float(b)), a == 0 and b == 0
        out.update(a=a, b=b, hyp=hyp, theta=math.atan2(float(b), float(a)))
    else:
        hyp = math.sqrt(sum(float(v) ** 2 for row in W for v in row))
        zero = all(v == 0 for row in W for v in row)
        out.update(hyp=hyp)
    kappa = float("inf") if zero else spread / hyp
    out.update(kappa=kappa, verdict="zero" if zero else "numerical" if kappa * U >= 1.0 else "regular")
    return out


def _fr(M):
    return [[Fraction(float(v)) for v in row] for row in np.atleast_2d(M)]


def angle_units(ref, R):
    """(|c b - s a| / hypot(a, b) as a multiple of kappa * 2^-52, c a + s b > 0: the optimum and not its antipode)."""
    c, s = Fraction(float(R[0, 0])), Fraction(float(R[1, 0]))
    sine = float(abs(c * ref["b"] - s * ref["a"])) / ref["hyp"]
    return sine / (ref["kappa"] * U), c * ref["a"] + s * ref["b"] > 0


def translation_units(ref, R, t):
    """|t - (mq - R mp)|_inf in units of 2^-52 * (mean |p_i|_1 + mean |q_i|_1)."""
    Rf, d = _fr(R), ref["d"]
    off = max(abs(Fraction(float(t[i])) - (ref["mq"][i] - sum(Rf[i][k] * ref["mp"][k] for k in range(d)))) for i in range(d))
    return float(off) / (U * ref["scale"]) if ref["scale"] else float(off != 0) * np.inf


def error_units(P, Q, R, t, err):
    """|err - mean_i |q_i - (R p_i + t)|^2| over ALL rows, exact, in the unit of the module docstring."""
    P, Q, t = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if not np.isfinite(err):
        return float("inf")
    N, d = P.shape
    (Pi, Qi, ti), S = _exact_ints(P, Q, t)
    (Ri,), SR = _exact_ints(np.asarray(R, dtype=np.float64))
    res = [(Qi[:, i] - ti[i]) * (1 << SR) - sum(Ri[i, k] * Pi[:, k] for k in range(d)) for i in range(d)]     # scale 2^(S + SR)
    one = 1 << (S + SR)
    exact = Fraction(_isum(sum(r * r for r in res)), N * one * one)
    e1 = (sum(abs(r) for r in res) / one).astype(np.float64)
    s = np.abs(P).sum(axis=1) + np.abs(Q).sum(axis=1) + np.abs(t).sum()
    unit = U * float(np.mean((e1 + U * s) * s))
    off = float(abs(Fraction(float(err)) - exact))
    return off / unit if unit else float(off != 0) * np.inf


def skew_units(ref, R):
    """|(R W - (R W)^T) / 2|_F / |W|_F in units of 2^-52, and the sum of the two smallest eigenvalues of the symmetric
    part of R W over |W|_F (float64 of the exact product): negative beyond rounding at an improper optimum."""
    Rf, d = _fr(R), ref["d"]
    M = [[sum(Rf[i][k] * ref["W"][k][j] for k in range(d)) for j in range(d)] for i in range(d)]
    skew = math.sqrt(sum(float((M[i][j] - M[j][i]) / 2) ** 2 for i in range(d) for j in range(d)))
    sym = np.array([[float((M[i][j] + M[j][i]) / 2) for j in range(d)] for i in range(d)])
    return skew / ref["hyp"] / U, float(np.linalg.eigvalsh(sym)[:2].sum()) / ref["hyp"]


def orth_units(R):
    R = np.asarray(R, dtype=np.float64)
    return float(np.linalg.norm(R.T @ R - np.eye(len(R)))) / U


def structure_ok(R):
    """What kabsch2 owes bit for bit and to eight units: R = [[c, -s], [s, c]] with |c^2 + s^2 - 1| <= 8 * 2^-52."""
    c, s = Fraction(float(R[0, 0])), Fraction(float(R[1, 0]))
    return bool(R[0, 0] == R[1, 1] and R[0, 1] == -R[1, 0] and abs(c * c + s * s - 1) <= 8 * Fraction(U))


def p2p_band(theta):
    a = abs(theta)
    return [name for name, lo, hi in P2P_BAND_EDGES if lo < a < hi]


# ── NumPy's float64 step, and three wrong ones ───────────────────────────────
def _svd_rotation(w):
    u, s, vt = np.linalg.svd(w)                                         # icp.py:202-206
    r = np.dot(vt.T, u.T)
    if np.linalg.det(r) < 0:
        vt[-1, :] *= -1
        r = np.dot(vt.T, u.T)
    return r


def numpy_p2p_step(P, Q, wrong=None):
    """icp.py:197-207 restated -> (r, t).  ``wrong``: "uncentred" forms W = sum p q^T - n mp mq^T, "sign" turns the
    other way (b with the opposite sign), "centroid" composes t = mq - r mq."""
    mu_s, mu_t = np.mean(P, axis=0), np.mean(Q, axis=0)
    if wrong == "uncentred":
        w = np.dot(P.T, Q) - len(P) * np.outer(mu_s, mu_t)
    else:
        w = np.dot((P - mu_s).T, Q - mu_t)
    r = _svd_rotation(w)
    if wrong == "sign":
        r = r.T.copy()
    return r, mu_t - np.dot(r, mu_t if wrong == "centroid" else mu_s)


def numpy_error(P, Q, r, t):
    return float(np.mean(np.sum((Q - (np.dot(P, r.T) + t)) ** 2, axis=1)))     # icp.py:212, :215


# ── cases ────────────────────────────────────────────────────────────────────
Case = namedtuple("Case", "family name src tgt gate lone")
# the two pairs of ``fused_cases`` in which two rows share a voxel of FUSED_VOXEL (one of the 25 rows about a target; two
# of the 4400 random rows of the large target): taken as they are, on the filtered rows; every other row stands alone
SHARED_VOXELS = ("last_row#39", "room#40")


def _even_room(rng, n, half=(5.0, 3.0), jitter=1e-3):
    """n points along the walls of a room, evenly spaced up to a quarter of the spacing, up to ``jitter`` off the
    wall.  Neighbours along the walls stay half a spacing apart, so at 4400 rows (3.6 mm) every point has its voxel
    of FUSED_VOXEL to itself, turned or not."""
    a, b = half
    per = 4 * (a + b)
    s = np.mod((np.arange(n) + rng.uniform(-0.25, 0.25, size=n)) / n * per, per)
    j = rng.uniform(-jitter, jitter, size=n)
    x = np.select([s < 2 * a, s < 2 * a + 2 * b, s < 4 * a + 2 * b], [s - a, a + j, a - (s - 2 * a - 2 * b)], -a + j)
    y = np.select([s < 2 * a, s < 2 * a + 2 * b, s < 4 * a + 2 * b], [-b + j, s - 2 * a - b, b + j], b - (s - 4 * a - 2 * b))
    return np.column_stack([x, y])


def _rot(ang):
    return np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])


def _gated_pair(rng, n, n_in):
    """n source rows of which exactly n_in lie within GATE of a target; the others stand in the room, a metre from
    every wall."""
    tgt = _even_room(rng, 4 * n)
    pick = rng.permutation(len(tgt))[:n_in]
    near = tgt[pick] + rng.normal(scale=2e-3, size=(n_in, 2)).clip(-8e-3, 8e-3) + [0.004, -0.003]
    gx, gy = np.meshgrid(np.arange(-3.9, 3.95, 0.2), np.arange(-1.9, 1.95, 0.2))
    inner = np.column_stack([gx.ravel(), gy.ravel()])
    far = inner[rng.permutation(len(inner))[:n - n_in]] + rng.uniform(-0.05, 0.05, size=(n - n_in, 2))
    return np.vstack([near, far]), tgt


@functools.lru_cache(maxsize=None)
def p2p_cases():
    """The 2-D pairs of one iteration: ``fused_cases`` as they are, then the pairs built here, whose rows all keep
    their voxel to themselves (``lone``)."""
    out = [Case(fam if fam != "gate_few" else "gate_short", f"{fam}#{i}", src, tgt, gate, f"{fam}#{i}" not in SHARED_VOXELS)
           for i, (fam, src, tgt, gate) in enumerate(fused_cases())]
    rng = np.random.default_rng(20270)
    shift0 = np.array([2.0e3, -1.5e3])
    for n in (30, 300):                                                  # the offset between off50 and off2e4
        tgt = _even_room(rng, n)
        out.append(Case("off2e3", f"off2e3/{n}", _moved(None, tgt, rng.uniform(-0.02, 0.02), rng.uniform(-0.05, 0.05, 2)) + shift0,
                        tgt + shift0, None, True))
    for n in SIZES:
        m = n + 5 if n <= 65 else n
        tgt = _even_room(rng, m)
        pick = np.sort(rng.permutation(m)[:n])
        out.append(Case("size", f"size/{n}", _moved(None, tgt[pick], rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03, 2)),
                        tgt, None, True))
    big = _even_room(rng, 4400)                                          # the target above 4096 rows
    out.append(Case("big_target", "big_target", _moved(rng, big, 0.01, np.array([0.02, -0.03]), keep=500), big, None, True))
    for i, ang in enumerate((3e-9, -3e-9, 7e-10, -7e-10)):               # b: a small difference of W01 and W10
        tgt = _even_room(rng, (64, 65)[i % 2])
        out.append(Case("band_tiny", f"band_tiny/{ang:g}", _moved(None, tgt, ang, np.array([1e-3, -5e-4])), tgt, None, True))
    for i, ang in enumerate((0.03, -0.03, 0.15, -0.12)):
        tgt = _even_room(rng, (64, 130)[i % 2])
        out.append(Case("band_small", f"band_small/{ang:g}", _moved(None, tgt, ang, rng.uniform(-0.02, 0.02, 2)), tgt, None, True))
    for i, gap in enumerate((1e-3, -1e-3, 1e-5, -1e-5)):                 # two rows turned about their centroid: a about 0
        ang = np.sign(gap) * (np.pi / 2 - abs(gap))
        c0, phi = rng.uniform(-1, 1, 2), rng.uniform(0, np.pi)
        src = c0 + np.array([[np.cos(phi), np.sin(phi)]]) * np.array([[-1.0], [1.0]])
        tgt = (src - c0) @ _rot(ang).T + c0 + rng.uniform(-0.1, 0.1, 2) * abs(gap)     # a shift that leaves the images nearest
        out.append(Case("band_half", f"band_half/{gap:g}", src, tgt, None, True))
    for n in (30, 300):                                                  # exactly the inliers icp.py:186 asks for, and one fewer
        need = max(3, n // 10)
        out.append(Case("gate_need", f"gate_need/{n}", *_gated_pair(rng, n, need), GATE, True))
        out.append(Case("gate_short", f"gate_short/{n}", *_gated_pair(rng, n, need - 1), GATE, True))
    return tuple(out)


def p2p_inputs(case):
    """What one iteration works on: filtered source P, matched target rows Q = T[idx] for ALL rows, the inlier mask
    (icp.py:183-185), the inliers the reference asks for (icp.py:186) and the filtered target."""
    P, T, _, idx, d, keep = fused_step_inputs(case.src, case.tgt, case.gate, lambda T, k: None)
    need = max(3, len(P) // 10) if case.gate is not None else 0
    return P, T[idx], keep, need, T


@functools.lru_cache(maxsize=None)
def p2p_references():
    """Per case of ``p2p_cases``: (P, Q, keep, need, exact reference or None where icp.py:186 stops the pair)."""
    out = []
    for case in p2p_cases():
        P, Q, keep, need, _ = p2p_inputs(case)
        out.append((P, Q, keep, need, p2p_step_reference(P, Q, keep) if keep.sum() >= need else None))
    return tuple(out)


def check_2d(name, family, ref, P, Q, R, t, err, kernel=True, table=None):
    """The three figures of a 2-D step (angle: None where it is not owed), asserted against the family's bounds;
    ``kernel`` adds what kabsch2 owes bit for bit."""
    assert np.isfinite(R).all() and np.isfinite(t).all(), name
    if kernel:
        assert structure_ok(R), (name, R)
    ang = None
    if ref["verdict"] == "regular":
        ang, proper = angle_units(ref, R)
        assert proper, name
        assert ang <= bound(family, 0, table), (name, "angle", ang, bound(family, 0, table))
    tr, er = translation_units(ref, R, t), error_units(P, Q, R, t, err)
    assert tr <= bound(family, 1, table), (name, "translation", tr, bound(family, 1, table))
    assert er <= bound(family, 2, table), (name, "error", er, bound(family, 2, table))
    return ang, tr, er


# ── the gate at its own resolution ───────────────────────────────────────────
EDGE_ROWS = np.array(list(range(3, 18)) + list(range(23, 38)))      # the targets matched: 15 on either wall


@functools.lru_cache(maxsize=None)
def edge_pairs():
    """Two 30-row pairs on dyadic coordinates, max(3, 30 // 10) = 3 inliers asked for.  Targets: two walls, 1/4 m apart
    along them.  Every source row is its match plus an exact displacement: NEAR (K/4, -K/8), EDGE (3 K, 4 K) — exactly
    5 K away in float64 — or FAR (7 K, 7 K), beyond every gate of EDGE_GATES and still nearest to its own match.
      flip      2 NEAR + 1 EDGE + 27 FAR: the EDGE row decides between 2 and 3 inliers;
      minority  10 NEAR + 4 EDGE + 16 FAR: a step either way, but another one.
    -> ((name, source, target, rows that are EDGE), ...)"""
    tgt = np.array([[0.25 * i, 0.0] for i in range(20)] + [[-0.25, 0.25 * j] for j in range(1, 21)])
    rows = EDGE_ROWS
    near, edge, far = np.array([K / 4, -K / 8]), np.array([3 * K, 4 * K]), np.array([7 * K, 7 * K])
    out = []
    for name, n_near, n_edge in (("flip", 2, 1), ("minority", 10, 4)):
        disp = np.tile(far, (30, 1))
        order = np.array([0, 15, 7, 22, 3, 18, 11, 26, 13, 28, 5, 20, 9, 24])           # both walls in turn
        disp[order[:n_near]] = near
        disp[order[n_near:n_near + n_edge]] = edge
        is_edge = np.zeros(30, dtype=bool)
        is_edge[order[n_near:n_near + n_edge]] = True
        out.append((name, tgt[rows] + disp, tgt, is_edge))
    return tuple(out)


def edge_inputs(src, tgt, gate, le=False):
    """(P, T, idx, d, keep) of an edge pair under ``gate``; ``le`` decides with <= instead of the reference's <."""
    P, T, _, idx, d, _ = fused_step_inputs(src, tgt, None, lambda T, k: None)
    return P, T, idx, d, (d ** 2 <= gate ** 2) if le else (d ** 2 < gate ** 2)


# ── 3-D ──────────────────────────────────────────────────────────────────────
def _rot3(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
            @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


@functools.lru_cache(maxsize=None)
def cases_3d():
    """(family, name, source, target): generic clouds at the origin and 2 km from it, planes (rank 2: z = 0 exactly, and
    tilted), lines (rank 1: on an axis exactly, and turned), one row (rank 0); 4, 64, 65 and 513 rows."""
    rng = np.random.default_rng(20271)
    out = []
    for n in (4, 64, 65, 513):
        p = rng.uniform(-1, 1, size=(n, 3)) * [2.0, 1.5, 1.0]
        q = p @ _rot3(*rng.uniform(-0.05, 0.05, 3)).T + rng.uniform(-0.02, 0.02, 3)
        out.append(("generic", f"generic/{n}", p, q))
        off = np.array([2.0e3, -1.5e3, 40.0])
        out.append(("off2e3", f"off2e3/{n}", p + off, q + off))
        xy = rng.uniform(-1, 1, size=(n, 2)) * [2.0, 1.5]
        flat = np.column_stack([xy, np.zeros(n)])
        if n % 2 == 0:                                                   # z = 0, turned about z
            out.append(("planar", f"planar/{n}", flat, flat @ _rot3(0, 0, rng.uniform(-0.05, 0.05)).T + [0.01, -0.02, 0.0]))
        else:
            B = _rot3(*rng.uniform(-np.pi, np.pi, 3))
            out.append(("planar", f"planar/{n}", flat @ B.T, flat @ (_rot3(*rng.uniform(-0.05, 0.05, 3)) @ B).T + rng.uniform(-0.02, 0.02, 3)))
        s = (np.arange(n) + rng.uniform(-0.25, 0.25, size=n)) / n * 4.0 - 2.0          # no two rows in one voxel
        if n % 2 == 0:                                                   # on the x axis, moved along it
            line = np.column_stack([s, np.zeros(n), np.zeros(n)])
            out.append(("line", f"line/{n}", line, line + [0.01, 0.0, 0.0]))
        else:
            u, v = _rot3(*rng.uniform(-np.pi, np.pi, 3))[:, 0], None
            v = _rot3(*rng.uniform(-0.05, 0.05, 3)) @ u
            out.append(("line", f"line/{n}", s[:, None] * u, s[:, None] * v + rng.uniform(-0.02, 0.02, 3)))
    out.append(("one_row", "one_row", rng.uniform(-1, 1, size=(1, 3)), rng.uniform(-1, 1, size=(7, 3))))
    return tuple(out)


VOXEL_3D = 1e-4


def inputs_3d(src, tgt):
    P, T = oracle.voxel_downsample(src, VOXEL_3D), oracle.voxel_downsample(tgt, VOXEL_3D)
    return P, T[oracle.nn(P, T)[1]]


@functools.lru_cache(maxsize=None)
def references_3d():
    out = []
    for _, _, src, tgt in cases_3d():
        P, Q = inputs_3d(src, tgt)
        assert len(P) == len(src), len(P)                                # every row alone in its voxel
        out.append((P, Q, p2p_step_reference(P, Q)))
    return tuple(out)


def check_3d(name, family, ref, P, Q, R, t, err):
    """The four figures of a 3-D step (skew: None where W = 0), asserted against the family's bounds."""
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.linalg.det(R) > 0.5, name
    b = functools.partial(bound, family, table=P2P3_TABLE)
    sk = None
    if ref["verdict"] == "zero":
        assert np.array_equal(R, np.eye(3)), name                        # rank 0: the SVD of zero gives the identity
    else:
        sk, low = skew_units(ref, R)
        assert sk <= b(0), (name, "skew", sk, b(0))
        assert low >= -b(0) * U, (name, "improper optimum", low)
    orth, tr, er = orth_units(R), translation_units(ref, R, t), error_units(P, Q, R, t, err)
    assert orth <= b(1), (name, "orth", orth, b(1))
    assert tr <= b(2), (name, "translation", tr, b(2))
    assert er <= b(3), (name, "error", er, b(3))
    return sk, orth, tr, er


# ═════════════════════════════════════════════════════════════════════════════
def _lex(a):
    return a[np.lexsort(a.T[::-1])]


def _rows_of(kept, raw):
    """For every filtered row the raw row it is, bit for bit (the filter returns lone rows unchanged, in voxel order)."""
    where = {tuple(r): i for i, r in enumerate(np.asarray(raw, dtype=np.float64).tolist())}
    return np.array([where[tuple(r)] for r in kept.tolist()])


def test_rows_built_here_keep_their_voxels_and_the_sizes_are_reached():
    sizes, n_tgt = set(), 0
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        T = p2p_inputs(case)[4]
        n_tgt = max(n_tgt, len(T))
        if case.lone:
            for raw, kept in ((case.src, P), (case.tgt, T)):
                assert len(kept) == len(raw) and np.array_equal(_lex(kept), _lex(np.asarray(raw, dtype=np.float64))), case.name
            if case.family == "size":
                sizes.add(len(P))
        else:
            assert case.name in SHARED_VOXELS and len(P) + len(T) == len(case.src) + len(case.tgt) - (1 if len(P) < 100 else 2), case.name
    assert sizes == set(SIZES) and max(SIZES) > 2048 + 512 and n_tgt > 4096
    for name, src, tgt, _ in edge_pairs():
        P, T, idx, d, _ = edge_inputs(src, tgt, 1.0)
        assert np.array_equal(_lex(P), _lex(src)) and np.array_equal(_lex(T), _lex(tgt)), name


def test_reference_on_a_step_known_in_closed_form():
    """Dyadic rows turned by the 3-4-5 angle: every quantity is a rational that can be written down."""
    P = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 2.0], [0.0, -2.0]]) + [8.0, -4.0]
    Rt = np.array([[0.75, -1.0], [1.0, 0.75]])                           # 1.25 x a rotation: W = 1.25 sum |pc|^2 R^T-ish
    Q = (P - [8.0, -4.0]) @ Rt.T + [0.5, 0.25]
    ref = p2p_step_reference(P, Q)
    assert ref["mp"] == [8, -4] and ref["mq"] == [Fraction(1, 2), Fraction(1, 4)]
    assert (ref["a"], ref["b"]) == (Fraction(15, 2), 10) and ref["verdict"] == "regular"
    assert ref["W"] == [[Fraction(3, 2), 2], [-8, 6]]
    assert ref["kappa"] == pytest.approx(10 * 1.25 / 12.5)
    R = np.array([[0.6, -0.8], [0.8, 0.6]])
    ang, proper = angle_units(ref, R)
    assert proper and ang < 1.0 and not angle_units(ref, -R)[1] and angle_units(ref, R.T)[0] > 1e14
    t = np.array([0.5, 0.25]) - R @ [8.0, -4.0]
    assert translation_units(ref, R, t) < 4.0 and translation_units(ref, R, t + [0.0, 1e-12]) > 100.0
    err = numpy_error(P, Q, R, t)                                        # the scale 1.25 leaves a residual: |q - Rp|^2 = |pc|^2 / 16
    assert err == pytest.approx(10 / 4 / 16) and error_units(P, Q, R, t, err) < 4.0 and error_units(P, Q, R, t, err * (1 + 1e-11)) > 100.0
    half = p2p_step_reference(P, Q, np.array([True, True, False, False]))
    assert half["n"] == 2 and half["W"][1] == [0, 0] and half["verdict"] == "regular"


def test_verdicts_of_the_families():
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        if case.family == "gate_short":
            assert ref is None and len(P) in (30, 300), case.name
            assert keep.sum() == need - 1 or case.name.startswith("gate_few"), case.name
            continue
        assert ref is not None and ref["kappa"] >= 1.0 - 1e-12, case.name
        if case.family == "gate_need":
            assert keep.sum() == need == max(3, len(P) // 10) and len(P) in (30, 300), case.name
        if case.family in ("dup", "last_row") or len(P) == 1:
            assert ref["verdict"] == "zero", case.name                   # every row on one target: W = 0 exactly
        else:
            assert ref["verdict"] == "regular", (case.name, ref["kappa"])
        if case.family in ("off2e3", "off2e4"):
            assert ref["kappa"] < 2.0, (case.name, ref["kappa"])         # the centring keeps the offsets regular
        if len(P) == 2 and case.gate is None:
            assert ref["W"][0][0] * ref["W"][1][1] == ref["W"][0][1] * ref["W"][1][0], case.name    # rank 1
        if case.family == "band_half":                                    # the images are found: the turn is the solved angle
            assert np.array_equal(Q, case.tgt[_rows_of(P, case.src)]), case.name
            assert abs(abs(ref["theta"]) - np.pi / 2) < 2e-3, case.name


def test_nearest_neighbour_steps_never_turn_beyond_a_right_angle():
    """a >= 0 on every pair, as the module docstring derives; the bands IcpBatch can reach are reached, both signs."""
    bands = set()
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        if ref is None:
            continue
        assert ref["a"] >= 0, case.name
        if ref["verdict"] == "regular":
            bands.update((b, ref["theta"] < 0) for b in p2p_band(ref["theta"]))
    assert bands == P2P_BANDS, sorted(bands ^ P2P_BANDS)


@functools.lru_cache(maxsize=None)
def _measure_2d():
    """family -> NumPy's largest [angle, translation, error] figure; the edge pairs under every gate included."""
    seen = {}

    def take(fam, ref, P, Q, keep):
        r, t = numpy_p2p_step(P[keep], Q[keep])
        m = seen.setdefault(fam, [None, 0.0, 0.0])
        if ref["verdict"] == "regular":
            ang, proper = angle_units(ref, r)
            assert proper, fam
            m[0] = max(m[0] or 0.0, ang)
        m[1] = max(m[1], translation_units(ref, r, t))
        m[2] = max(m[2], error_units(P, Q, r, t, numpy_error(P, Q, r, t)))
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        if ref is not None:
            take(case.family, ref, P, Q, keep)
    for name, src, tgt, _ in edge_pairs():
        for gate in EDGE_GATES:
            P, T, idx, d, keep = edge_inputs(src, tgt, gate)
            if keep.sum() >= 3:
                take("edge", p2p_step_reference(P, T[idx], keep), P, T[idx], keep)
    return seen


@functools.lru_cache(maxsize=None)
def _measure_3d():
    seen = {}
    for (fam, name, _, _), (P, Q, ref) in zip(cases_3d(), references_3d()):
        r, t = numpy_p2p_step(P, Q)
        m = seen.setdefault(fam, [None, 0.0, 0.0, 0.0])
        if ref["verdict"] != "zero":
            sk, low = skew_units(ref, r)
            assert low >= -64 * U, name
            m[0] = max(m[0] or 0.0, sk)
        m[1] = max(m[1], orth_units(r))
        m[2] = max(m[2], translation_units(ref, r, t))
        m[3] = max(m[3], error_units(P, Q, r, t, numpy_error(P, Q, r, t)))
    return seen


def _within(seen, table):
    assert set(seen) == set(table), sorted(set(seen) ^ set(table))
    for fam, figs in seen.items():
        for got, want in zip(figs, table[fam]):
            assert (got is None) == (want is None), (fam, figs)
            # the floor of the kernels' bounds in NumPy's own terms: a figure of 0.0 in the table is a family in which
            # NumPy is exact here, and another host may round there
            assert got is None or got <= max(HOST_NUMPY_CAP * want, FLOOR / FACTOR), (fam, figs, table[fam])


def test_numpy_step_stays_within_the_table():
    _within(_measure_2d(), P2P_TABLE)


def test_numpy_step_3d_stays_within_its_table():
    _within(_measure_3d(), P2P3_TABLE)
    ranks = {}
    for (fam, name, _, _), (P, Q, ref) in zip(cases_3d(), references_3d()):
        W = np.array([[float(v) for v in row] for row in ref["W"]])
        ranks.setdefault(fam, set()).add(int(np.linalg.matrix_rank(W)))
        assert ref["verdict"] == ("zero" if fam == "one_row" else "regular"), name
    assert ranks == {"generic": {3}, "off2e3": {3}, "planar": {2}, "line": {1}, "one_row": {0}}, ranks
    assert {len(P) for P, _, _ in references_3d()} == {1, 4, 64, 65, 513}


def _fmt(v):
    return "-" if v is None else f"{v:.3g}"


def _table_lines(table, widths):
    return ["  " + "".join(f"{c:<{w}}" for c, w in zip([fam] + [_fmt(v) for v in figs], widths)).rstrip() for fam, figs in table.items()]


def test_docstring_tables_equal_the_dicts():
    for tag, table, widths in (("P2P_TABLE", P2P_TABLE, (17, 9, 13, 0)), ("P2P3_TABLE", P2P3_TABLE, (17, 9, 13, 13, 0))):
        block = __doc__.split(tag + "_BEGIN\n")[1].split(tag + "_END")[0].splitlines()
        assert block[1:] == _table_lines(table, widths), (tag, block[1:], _table_lines(table, widths))


def test_print_the_measured_tables():
    def up3(v):                                                          # three digits, rounded up
        if v is None or v == 0:
            return v
        q = 10.0 ** (math.floor(math.log10(v)) - 2)
        return float(f"{math.ceil(v / q - 1e-9) * q:.3g}")
    print("\nmeasured now (NumPy float64 against the exact reference), in the layout of the module docstring")
    for title, seen, widths in (("2-D: angle, translation, error", _measure_2d(), (17, 9, 13, 0)),
                                ("3-D: skew, orth, translation, error", _measure_3d(), (17, 9, 13, 13, 0))):
        print(title)
        print("\n".join(_table_lines({f: [up3(v) for v in figs] for f, figs in seen.items()}, widths)))
    p2l = _measure_edge_p2l()
    print("point-to-line on the edge pairs: backward, forward", [up3(v) for v in p2l])


def test_oracle_one_iteration_stays_within_the_bounds():
    """oracle.icp runs the same pipeline on the host (voxel filter, search, gate, step, error): it is held to the
    kernels' bounds, less what kabsch2 owes bit for bit (the oracle's 2-D step is a Jacobi SVD)."""
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        R, t, err, info = oracle.icp(case.src, case.tgt, 1e-30, 1, FUSED_VOXEL, max_corr_dist=case.gate)
        if ref is None:
            assert info["status"] == oracle.FEW_INLIERS and info["iters"] == 0 and np.array_equal(R, np.eye(2)) and not t.any()
            continue
        assert info["iters"] == 1 and info["status"] == oracle.MAXITER, case.name
        check_2d(case.name, case.family, ref, P, Q, R, t, err, kernel=False)
    for (fam, name, src, tgt), (P, Q, ref) in zip(cases_3d(), references_3d()):
        R, t, err, info = oracle.icp(src, tgt, 1e-30, 1, VOXEL_3D)
        assert info["iters"] == 1, name
        check_3d(name, fam, ref, P, Q, R, t, err)


def test_explicit_correspondences_reach_every_band():
    """The four bands with both signs on explicit correspondences (targets are the rows' own images, no search):
    NumPy's step and the oracle's, the band next to pi included, which no search reaches."""
    rng = np.random.default_rng(20272)
    seen = set()
    for ang in (4e-9, -4e-9, 0.07, -0.11, np.pi / 2 - 1e-4, -np.pi / 2 + 1e-4, np.pi / 2 + 1e-3, np.pi - 5e-4, -np.pi + 5e-4,
                np.pi - 1e-9, -np.pi + 1e-9):
        for n in (2, 3, 64, 513):
            P = _even_room(rng, n + 5)[:n] + rng.uniform(-1, 1, 2)
            Q = _moved(None, P, ang, rng.uniform(-0.05, 0.05, 2))
            ref = p2p_step_reference(P, Q)
            assert ref["verdict"] == "regular" and abs(ref["theta"] - ang) <= 1e-6 * abs(ang) + 1e-13, (ang, n)
            seen.update((b, ref["theta"] < 0) for b in p2p_band(ref["theta"]))
            for r, t in (numpy_p2p_step(P, Q), oracle.p2p_step(P, Q)):
                u, proper = angle_units(ref, r)
                assert proper and u <= FLOOR and translation_units(ref, r, t) <= FLOOR, (ang, n, u)
                assert abs(recover_theta(r, ang) - ang) <= 1e-12, (ang, n)
    assert seen == {(b, neg) for b, _, _ in P2P_BAND_EDGES for neg in (False, True)}, sorted(seen)


# ── the gate at its own resolution ───────────────────────────────────────────
def test_edge_rows_lie_exactly_on_the_gate():
    assert math.sqrt(9 * K * K + 16 * K * K) == 5 * K
    for name, src, tgt, is_edge in edge_pairs():
        P, T, idx, d, _ = edge_inputs(src, tgt, 1.0)
        order = _rows_of(P, src)                                         # the filter returns the rows in voxel order
        assert np.array_equal(T[idx], tgt[EDGE_ROWS][order]), name       # every row finds the target it was displaced from
        on_edge = is_edge[order]
        assert (d[on_edge] == 5 * K).all() and (np.abs(d[~on_edge] - 5 * K) > 0.02).all(), name
        counts = [int(edge_inputs(src, tgt, g)[4].sum()) for g in EDGE_GATES]
        assert counts == ([2, 2, 3] if name == "flip" else [10, 10, 14]), (name, counts)      # out, out, in
        assert [bool((d[on_edge] ** 2 < g ** 2).all()) for g in EDGE_GATES] == [False, False, True]


@functools.lru_cache(maxsize=None)
def _measure_edge_p2l():
    m = [0.0, 0.0]
    for name, src, tgt, _ in edge_pairs():
        for gate in EDGE_GATES:
            P, T, idx, d, keep = edge_inputs(src, tgt, gate)
            if keep.sum() < 3:
                continue
            nrm = oracle.normals_2d(T, FUSED_NORMAL_K)
            ref = step_reference(P, T, nrm, idx, max_corr_dist=gate, dists=d)
            assert ref["verdict"] == "regular" and ref["K"] == keep.sum() and ref["kappa"] * U < 1e-6, (name, gate, ref["kappa"])
            x = numpy_step(P[keep], T, nrm, idx[keep])[0]
            m[0], m[1] = max(m[0], backward_error(ref, x)), max(m[1], forward_multiple(ref, x))
    return tuple(m)


def test_numpy_point_to_line_step_on_the_edge_pairs_stays_within_its_table():
    bwd, fwd = _measure_edge_p2l()
    assert bwd <= HOST_NUMPY_CAP * EDGE_P2L_TABLE["edge"][0] and fwd <= HOST_NUMPY_CAP * EDGE_P2L_TABLE["edge"][1], (bwd, fwd)


def test_oracle_on_the_rows_exactly_on_the_gate():
    """The host twin of both kernels under the three gates, both methods: out, out, in."""
    for method in ("point_to_point", "point_to_line"):
        for gate in EDGE_GATES:
            for name, src, tgt, _ in edge_pairs():
                P, T, idx, d, keep = edge_inputs(src, tgt, gate)
                R, t, err, info = oracle.icp(src, tgt, 1e-30, 1, FUSED_VOXEL, method=method, normal_k=FUSED_NORMAL_K, max_corr_dist=gate)
                if keep.sum() < 3:
                    assert info["status"] == oracle.FEW_INLIERS and info["iters"] == 0 and np.array_equal(R, np.eye(2)) and not t.any()
                    continue
                assert info["iters"] == 1 and info["status"] == oracle.MAXITER, (name, gate)
                if method == "point_to_point":
                    check_2d(name, "edge", p2p_step_reference(P, T[idx], keep), P, T[idx], R, t, err, kernel=False)
                else:
                    ref = step_reference(P, T, oracle.normals_2d(T, FUSED_NORMAL_K), idx, max_corr_dist=gate, dists=d)
                    x = (recover_theta(R, ref["theta"]), t[0], t[1])
                    assert backward_error(ref, x) <= max(FLOOR, FACTOR * EDGE_P2L_TABLE["edge"][0]), (name, gate)
                    assert forward_multiple(ref, x) <= FACTOR * EDGE_P2L_TABLE["edge"][1], (name, gate)


# ── the tests can fail ───────────────────────────────────────────────────────
def _worst(wrong, families, which):
    """Largest figure ``which`` of a wrong NumPy step over ``families``, as a multiple of the kernels' bound there."""
    worst = 0.0
    for case, (P, Q, keep, need, ref) in zip(p2p_cases(), p2p_references()):
        if ref is None or ref["verdict"] != "regular" or case.family not in families:
            continue
        r, t = numpy_p2p_step(P[keep], Q[keep], wrong=wrong)
        fig = angle_units(ref, r)[0] if which == 0 else translation_units(ref, r, t)
        worst = max(worst, fig / bound(case.family, which))
    return worst


def test_wrong_steps_exceed_the_bounds():
    """Three plausible mistakes, in NumPy float64, against the bounds the kernels are held to."""
    uncentred = {f: _worst("uncentred", (f,), 0) for f in ("off0", "off2e3", "off2e4")}
    assert uncentred["off2e3"] > 10 and uncentred["off2e4"] > 10, uncentred              # the centring lost far from the origin
    assert uncentred["off0"] <= 1.0, uncentred                                            # and only there
    sign = {f: _worst("sign", (f,), 0) for f in ("theta", "band_small", "band_tiny", "band_half")}
    assert min(sign.values()) > 10, sign                                                  # b with the opposite sign: any turned pair
    families = tuple(f for f in P2P_TABLE if P2P_TABLE[f][0] is not None and f != "edge")
    assert all(_worst("centroid", (f,), 1) > 10 for f in families)                       # t = mq - R mq: every family
    print("\nwrong steps, worst figure over the bound: uncentred", uncentred, "sign", sign,
          "centroid", {f: _worst("centroid", (f,), 1) for f in families})


def test_a_gate_with_le_and_the_wrong_side_of_the_gate_show():
    (_, fsrc, ftgt, _), (_, msrc, mtgt, _) = edge_pairs()
    g = EDGE_GATES[1]                                                    # the gate equal to the distance: out
    assert edge_inputs(fsrc, ftgt, g)[4].sum() == 2 and edge_inputs(fsrc, ftgt, g, le=True)[4].sum() == 3     # status flips
    # minority pair: the exact step with the edge rows, taken for the one without them (and the reverse), misses
    # every bound by orders of magnitude, for either method
    P, T, idx, d, out_ = edge_inputs(msrc, mtgt, g)
    _, _, _, _, in_ = edge_inputs(msrc, mtgt, g, le=True)
    assert out_.sum() == 10 and in_.sum() == 14
    nrm = oracle.normals_2d(T, FUSED_NORMAL_K)
    for right, wrong in ((out_, in_), (in_, out_)):
        ref = p2p_step_reference(P, T[idx], right)
        r, t = numpy_p2p_step(P[wrong], T[idx][wrong])
        assert translation_units(p2p_step_reference(P, T[idx], wrong), r, t) <= bound("edge", 1)
        far = max(angle_units(ref, r)[0] / bound("edge", 0), translation_units(ref, r, t) / bound("edge", 1))
        assert far > 1e6, far
        ref_l = step_reference(P[right], T, nrm, idx[right])
        x = numpy_step(P[wrong], T, nrm, idx[wrong])[0]
        assert backward_error(ref_l, x) > 1e6 * max(4.0, FACTOR * EDGE_P2L_TABLE["edge"][0])
