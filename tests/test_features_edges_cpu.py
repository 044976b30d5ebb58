"""The extended-precision reference of the feature stages (tests/features_ref.py) and the inputs of the edge suite
(tests/features_cases.py), without a GPU: the reference reproduces what the reference project recorded in
tests/golden/features.npz, and every input has the property tests/test_features_edges_gpu.py relies on — so a GPU test
cannot pass because an input silently degenerated.  Decisions sit at least 1e-9 from their boundary, or exactly on it (or
2^-40 from it) by dyadic construction, where long double decides exactly as float64 does."""
from fractions import Fraction as F

import numpy as np
import pytest

import features_cases as fc
import features_ref as fr
from conftest import load_golden

CLOUDS = [f"c{i}" for i in range(8)] + ["s0", "s1", "s2", "s3", "few_t"]
LD = np.longdouble


@pytest.fixture(scope="module")
def g():
    return load_golden("features")


def test_long_double_is_wider_than_float64():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_reference_reproduces_the_golden_clouds(g):
    tol = float(g["curv_tol"])
    worst = 0.0
    for c in CLOUDS:
        pts, want = g[c + "_pts"], g[c + "_curv"]
        got, gap, _ = fr.curvature(pts, 10)
        assert (gap > 0).all(), c                                   # the generator's own condition: no tie at the k-th neighbour
        got = got.astype(np.float64)
        scale = np.maximum(np.abs(got), np.abs(want))
        rel = np.where(scale > 0, np.abs(got - want) / np.where(scale > 0, scale, 1.0), 0.0)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= tol, (c, rel.max(), tol)
        kp, margin = fr.keypoints(pts, want, 100, 0.3, order=g[c + "_order"])
        assert np.array_equal(kp, g[c + "_kp"]) and margin > 1e-12, c
        assert np.array_equal(fr.descriptors(pts, g[c + "_kp"], 30), g[c + "_desc"]), c
    print(f"curvature: largest relative difference to the fixture {worst:.3e} (recorded tolerance {tol:.3e})")


def test_reference_reproduces_the_golden_pairs(g):
    for i in range(4):
        m, margin = fr.matches(g[f"c{2 * i}_desc"], g[f"c{2 * i + 1}_desc"], 0.8)
        assert m == [tuple(int(x) for x in r) for r in g[f"p{i}_matches"]] and margin.min() > 1e-9, i
    m, _ = fr.matches(g["c2_desc"], g["few_t_desc"], 0.8)
    assert m == [tuple(int(x) for x in r) for r in g["few_matches"]]
    for p in [f"p{i}" for i in range(4)] + ["dup"]:
        r = fr.ransac(g[p + "_kp_s"], g[p + "_kp_t"], g[p + "_matches"], g[p + "_draws"], 0.5)
        assert np.array_equal(r["counts"], g[p + "_counts"]) and r["margin"] > 1e-9, p
        assert r["best"] == int(g[p + "_best"]) and r["inliers"] == int(g[p + "_n_inliers"]), p
        e = fr.rot_err_ld(g[p + "_R"], g[p + "_t"], r["R"], r["t"])
        print(p, "rot_err of the fixture against the long-double fit", e)
        assert e < 1e-12, p


# ── curvature and descriptors ────────────────────────────────────────────────────────────────────────
def test_curvature_inputs_and_yardstick():
    clouds = fc.curvature_clouds()
    assert 280 <= len(clouds["room"]) <= 300 and len(clouds["line"]) == 200 and len(clouds["lattice"]) == 120
    for n in fc.SMALL_N:
        assert len(clouds[f"small{n}"]) == n
    # the classes are what they are called
    p = clouds["line"]
    d = [(F(x) - F(p[0, 0]), F(y) - F(p[0, 1])) for x, y in p.tolist()]
    assert all(a * d[1][1] == b * d[1][0] for a, b in d) and np.hypot(*p[0]) > 100       # exactly collinear, away from the origin
    lat = clouds["lattice"]
    assert np.array_equal(lat * 4, np.round(lat * 4))                                     # dyadic: every d2 is exact
    seen = set()
    for name, pts in clouds.items():
        for k in fc.K_ALL:
            kk = min(k, len(pts) - 1) + 1
            want, gap, idx = fr.curvature(pts, k)
            y, tol = fr.curvature_tolerance(pts, idx, want)
            seen.add((8 if kk <= 8 else 16 if kk <= 16 else 32, kk in (8, 16, 32)))
            if name in ("room", "shifted"):
                assert (gap > 0).all(), (name, k)                 # tie-free: the set does not hang on the tie rule
            if name == "lattice" and k in (2, 6, 10, 15):
                assert (gap == 0).sum() > 60, k                   # a shell of equal distances cut by kk: true ties, most rows
            if name == "line":
                assert float(np.abs(want).max()) == 0.0           # exactly collinear: curvature exactly 0 in the reference
            assert tol < 1e-9 or name == "shifted"
            print(f"{name} k={k} kk={kk}: yardstick {y:.3e} tolerance {tol:.3e}")
    assert seen == {(8, False), (8, True), (16, False), (16, True), (32, False), (32, True)}
    for n in (2047, 2048):
        pts = fc.big_room(n)
        for k in (10, 31):
            want, gap, idx = fr.curvature(pts, k)
            y, tol = fr.curvature_tolerance(pts, idx, want)
            assert (gap > 0).all()
            print(f"room n={n} k={k}: yardstick {y:.3e} tolerance {tol:.3e}")


# ── keypoints ─────────────────────────────────────────────────────────────────────────────────────────
def test_keypoint_inputs():
    for n in fc.KP_LATTICE_N:
        pts = fc.keypoint_lattice(n)
        curv = fr.curvature(pts, 10)[0].astype(np.float64)
        assert len(np.unique(curv)) <= max(1, n // 8)                             # massive exact ties
        kp, margin = fr.keypoints(pts, curv, 256, 0.3)
        unlimited, _ = fr.keypoints(pts, curv, 4096, 0.3)
        assert margin > 1e-3                                                      # lattice distances: 0.25, 0.3535, ... never near 0.3
        assert len(kp) == min(256, len(unlimited))
        if n == 2048:
            assert len(kp) == 256 and len(unlimited) > 256                        # top_n binds, at the kernel's capacity
        print(f"lattice n={n}: {len(kp)} keypoints of {len(unlimited)} without a limit, {len(np.unique(curv))} distinct curvatures")
    for order, min_dist, kept in fc.TRIANGLE_CASES:
        kp, margin = fr.keypoints(fc.TRIANGLE, None, 3, min_dist, order=order)
        assert kp.tolist() == kept and margin == 0.0                              # a candidate exactly at min_dist, and kept
        a, b = fc.TRIANGLE[kept[0]], fc.TRIANGLE[kept[1]]
        assert (F(a[0]) - F(b[0])) ** 2 + (F(a[1]) - F(b[1])) ** 2 == F(min_dist) ** 2


# ── matching ──────────────────────────────────────────────────────────────────────────────────────────
def test_match_inputs():
    smallest = np.inf
    for q, length in enumerate(fc.MATCH_LENS):
        for empty in (None, 1 + q % 3):
            da, db, want = fc.match_descriptors_case(length, empty, seed=100 + q)
            m, margin = fr.matches(da, db, 0.8)
            src = np.array([i for i, _ in m])
            assert np.array_equal(np.flatnonzero(want), src) and margin.min() > 1e-9, (length, empty)
            smallest = min(smallest, float(margin.min()))
            per_wave = np.bincount(src // 64, minlength=4)
            assert (per_wave > 0).sum() == (4 if empty is None else 3) and (empty is None or per_wave[empty] == 0)
            assert {0, 63, 64, 127, 128, 191, 192, 255} - set(range(64 * empty, 64 * empty + 64) if empty is not None else ()) <= set(src)
            da2, db2, i_nan, j_nan = fc.with_nan_rows(da, db, m)
            m2, margin2 = fr.matches(da2, db2, 0.8)
            assert all(i != i_nan and j != j_nan for i, j in m2) and margin2.min() > 1e-9
            smallest = min(smallest, float(margin2.min()))
            keep = [x for x in m if x[0] != i_nan and x[1] != j_nan]                # every other match stays (a row halfway between the NaN
            assert set(keep) <= set(m2) and len(keep) == len(m) - 2 and len(m2) <= len(keep) + 2   # target and another may now match that one)
    print(f"smallest ratio-test margin |D0 - ratio^2 D1| / D1 of the 256 x 256 cases: {smallest:.3e}")
    da, db, _ = fc.match_descriptors_case(7, None, seed=120, ns=65, only=64)
    m, margin = fr.matches(da, db, 0.8)
    assert [i for i, _ in m] == [64] and margin.min() > 1e-9
    da, db, want = fc.match_descriptors_case(7, None, seed=121, ns=9, nt=2)
    m, margin = fr.matches(da, db, 0.8)
    assert 0 < len(m) < 9 and margin.min() > 1e-9
    for q, (a, db, ratio, want) in enumerate(fc.match_tie_cases()):
        m, margin = fr.matches(a, db, ratio)
        assert m == want, q
        if q < 6:
            assert margin[0] > 1e-9
    assert fr.matches(*fc.match_tie_cases()[6][:3])[1][0] == 0.0                   # exactly on the boundary: no match
    assert 0 < fr.matches(*fc.match_tie_cases()[7][:3])[1][0] < 1e-12 and F(2.0 ** -20) ** 2 + 4 == F(4 + 2.0 ** -40)


# ── RANSAC ────────────────────────────────────────────────────────────────────────────────────────────
def test_ransac_inputs():
    smallest = np.inf
    for n in (2, 64, 65, 256):
        kp_s, kp_t, m, good = fc.ransac_case(n, seed=200 + n)
        assert len(m) == len(kp_s) == len(kp_t) == n                                # 256: ICPMI_FT_MAX_KP matches fill S[] and D[]
        for n_iter in ((1, 255, 256, 257, 1000) if n == 256 else (257,)):
            r = fr.ransac(kp_s, kp_t, m, fc.random_hypotheses(n, n_iter, seed=n_iter), 0.5)
            assert r["margin"] > 1e-9, (n, n_iter)
            smallest = min(smallest, r["margin"])
            if n_iter > 1:
                assert r["inliers"] == int(good.sum()) and r["counts"].max() == r["inliers"]
        if n == 256:
            assert 200 <= good.sum() <= 202 and (np.bincount(np.flatnonzero(good) // 64, minlength=4) > 0).all()   # the refit: four lane trips
    kp_s, kp_t, m, good_pair, poor_pair = fc.winner_case()
    for name, (rows, planted) in fc.WINNER_TABLES.items():
        t = fc.winner_table(name, good_pair, poor_pair)
        r = fr.ransac(kp_s, kp_t, m, t, 0.5)
        c = r["counts"]
        assert len(t) == rows and r["margin"] > 1e-9
        smallest = min(smallest, r["margin"])
        assert r["best"] == planted[0] and (c[list(planted)] == c.max()).all() and (np.delete(c, planted) < c.max()).all()
        assert 0 < c[0] < c.max() and planted[0] > 0                              # a strictly smaller count before the winner
    for n in (2, 256):
        kp_s, kp_t, m, _ = fc.ransac_case(n, seed=200 + n)
        u, ij = fc.uniform_draws(n)
        assert (ij[:, 0] != ij[:, 1]).all() and ij.max() == n - 1 and ij.min() == 0 and u.max() < 1.0
        r = fr.ransac(kp_s, kp_t, m, ij, 0.5)
        assert r["margin"] > 1e-9
        smallest = min(smallest, r["margin"])
    print(f"smallest |err - thresh| of the seeded RANSAC cases: {smallest:.3e}")
    kp_s, kp_t, m, thresh = fc.threshold_case()
    r = fr.ransac(kp_s, kp_t, m, [[0, 1]], thresh)
    e = fr._errors(np.eye(2, dtype=LD), np.array([3.0, -2.0], dtype=LD), kp_s.astype(LD), kp_t.astype(LD))
    assert [float(v) for v in e] == [0.0, 0.0, 0.625, 0.625 - 2.0 ** -40, 0.0]    # exactly on the threshold, and 2^-40 under it
    assert r["counts"].tolist() == [4] and r["inliers"] == 4 and r["margin"] == 0.0      # (R, t is the refit on those four)


def test_rigid_inputs_and_yardstick():
    for name, (s, d) in fc.rigid_pairs().items():
        R, t = fr.rigid(s, d)
        y, tol = fr.rigid_tolerance(s, d)
        assert abs(float(R[0, 0] * R[1, 1] - R[0, 1] * R[1, 0]) - 1.0) < 1e-18
        if name.startswith("yaw180"):
            assert R[0, 0] == -1 and R[1, 0] == 0
        if name.startswith("yaw90"):
            assert R[0, 0] == 0 and R[1, 0] == 1
        if name.startswith("close"):
            assert abs(np.hypot(*(s[1] - s[0])) - 0.3) < 1e-9
        print(f"{name}: NumPy SVD rot_err {y:.3e} tolerance {tol:.3e}")
        r = fr.ransac(s, d, [[0, 0], [1, 1]], [[0, 1]], 0.5)
        assert r["inliers"] == 2 and r["margin"] > 0.4                            # both points on their own fit: err ~ 0
        if name.startswith("close"):
            r = fr.ransac(s, d, [[0, 0], [1, 0]], [[0, 1]], 0.5)                  # W = 0: identity, each source 0.15 from the mean
            assert r["inliers"] == 2 and r["margin"] > 0.3 and np.array_equal(r["R"], np.eye(2))
        assert tol < (1e-10 if name.endswith("far") else 1e-14)
    R, t = fr.rigid(np.array([[1.0, 2.0], [3.0, 5.0]]), np.array([[4.0, 4.0], [4.0, 4.0]]))      # W = 0
    assert np.array_equal(R, np.eye(2)) and t.tolist() == [2.0, 0.5]
