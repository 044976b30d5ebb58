"""Inputs of the feature-alignment edge suites, built from seeds or by construction — TEST INFRASTRUCTURE ONLY.

tests/test_features_edges_cpu.py proves on tests/features_ref.py alone that every input has the property its GPU test
relies on; tests/test_features_edges_gpu.py runs the kernels on the same inputs.  Nothing here touches a GPU.
"""
import functools

import numpy as np

from icpmi import synth

POSE = (0.5, -0.3, 0.1)
K_ALL = (2, 6, 7, 8, 10, 15, 16, 30, 31)          # kk = k + 1: below, at and above every template bound (8, 16, 32)
SMALL_N = (1, 2, 3, 8, 9, 16, 17, 32, 33)
MATCH_LENS = (1, 7, 8, 30, 31)


def lattice(nx, ny, step=0.25):
    """nx x ny rows on a dyadic lattice, row-major from (1, 2): every coordinate, difference and d2 is exact."""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.ascontiguousarray(np.stack([1.0 + step * i.ravel(), 2.0 + step * j.ravel()], axis=1))


@functools.lru_cache(maxsize=None)
def curvature_clouds():
    """name -> cloud of every input class of the curvature and descriptor tests."""
    room = synth.scan(POSE, 31, n_beams=300)
    steps = np.cumsum(np.random.default_rng(5).integers(1, 8, size=200)).astype(np.float64)
    line = np.stack([100.0 + 0.125 * steps, 50.0 + 0.0625 * steps], axis=1)      # exact: dyadic origin, direction and steps
    out = {"room": room, "shifted": room + np.array([1e4, -2e4]), "straight": synth.scan(POSE, 32, n_beams=300, noise=0.0),
           "line": line, "lattice": lattice(12, 10)}
    for n in SMALL_N:
        out[f"small{n}"] = np.ascontiguousarray(room[40:40 + n])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def big_room(n):
    """a noisy room scan of n <= 2048 rows (2048 beams, every one hits a wall)."""
    pts = synth.scan(POSE, 33, n_beams=2048)
    assert len(pts) == 2048
    pts = np.ascontiguousarray(pts[:n])
    pts.setflags(write=False)
    return pts


def keypoint_lattice(n):
    """the first n rows of the 64 x 32 lattice at 0.25 m: neighbours at 0.25 are suppressed by min_dist 0.3, diagonals kept."""
    return np.ascontiguousarray(lattice(64, 32)[:n])


KP_LATTICE_N = (2048, 1025, 1024, 65, 64, 1)
# three points of a 3-4-5 triangle scaled by 0.25: |AC| = 1.25, |AB| = 0.75, |BC| = 1, all exact
TRIANGLE = np.array([[0.75, 0.0], [0.0, 0.0], [0.0, 1.0]])          # A, B, C
TRIANGLE_CASES = (                                                  # (order, min_dist, kept)
    ([0, 2, 1], 1.25, [0, 2]),      # C at exactly min_dist of A: kept; B at 0.75: dropped
    ([1, 2, 0], 1.0, [1, 2]),       # C at exactly min_dist of B: kept; A at 0.75 of B: dropped
)


def match_descriptors_case(length, empty_wave, seed, ns=256, nt=256, only=None):
    """(da (ns, length), db (nt, length), intended mask): targets at least 1 apart in their first coordinate; a source row
    either sits on its target (noise 0.01: a match) or halfway between two targets (D0 ~ D1: none).  `empty_wave`: the wave
    of 64 source rows that has no match (None: matches in every wave); `only`: the single source row that matches."""
    rng = np.random.default_rng(seed)
    db = rng.uniform(0.0, 1.0, size=(nt, length))
    db[:, 0] += 2.0 * np.arange(nt)
    tgt = rng.permutation(nt)[np.arange(ns) % nt]
    want = rng.random(ns) < 0.5
    want[[i for i in (0, 63, 64, 127, 128, 191, 192, 255) if i < ns]] = True          # the first and last lane of every wave
    if empty_wave is not None:
        want[64 * empty_wave:64 * (empty_wave + 1)] = False
    if only is not None:
        want[:] = False
        want[only] = True
    other = np.where(tgt + 1 < nt, tgt + 1, tgt - 1)
    da = np.where(want[:, None], db[tgt], 0.5 * (db[tgt] + db[other])) + 0.01 * rng.normal(size=(ns, length))
    return da, db, want


def with_nan_rows(da, db, match_list):
    """-> (da, db, i, j) with source row i (a matched one) all NaN and one entry of target row j (another match's) NaN."""
    i, j = match_list[len(match_list) // 2][0], match_list[3][1]
    da, db = da.copy(), db.copy()
    da[i] = np.nan
    db[j, -1] = np.nan
    return da, db, i, j


def match_tie_cases():
    """(a, db, ratio, matches): two identical target rows — D0 == D1 is no match; with ratio > 1 it is one, to the lower index;
    a third row that is nearer makes the test pass — and the exact boundary of <: ratio^2 = 0.25, D0 = 1, D1 = 4 or 4 + 2^-40."""
    x, y = np.array([1.0, 2.0, 3.0]), np.array([9.0, 9.5, 8.0])
    ax, ay, z = (x + 0.01)[None, :], (y + 0.01)[None, :], np.zeros((1, 2))
    return [(ax, np.stack([x, x, y]), 0.8, []), (ax, np.stack([y, x, x]), 0.8, []),
            (ax, np.stack([x, x, y]), 1.5, [(0, 0)]), (ax, np.stack([y, x, x]), 1.5, [(0, 1)]),
            (ay, np.stack([x, x, y]), 0.8, [(0, 2)]), (ay, np.stack([x, y, x]), 0.8, [(0, 1)]),
            (z, np.array([[1.0, 0.0], [2.0, 0.0]]), 0.5, []), (z, np.array([[1.0, 0.0], [2.0, 2.0 ** -20]]), 0.5, [(0, 0)])]


def ransac_case(n, seed, inlier_share=0.78, centre=(0.0, 0.0), yaw_deg=30.0):
    """n matches (i, i) between n source keypoints and n target keypoints: a share of inliers (noise 0.01 under the
    rigid motion), the rest thrown far.  -> (kp_s, kp_t, matches, inlier mask)."""
    rng = np.random.default_rng(seed)
    kp_s = rng.uniform(-10.0, 10.0, size=(n, 2)) + np.asarray(centre)
    th = np.deg2rad(yaw_deg)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    kp_t = (kp_s - np.asarray(centre)) @ R.T + np.asarray(centre) + np.array([1.5, -0.75]) + 0.01 * rng.normal(size=(n, 2))
    good = np.zeros(n, dtype=bool)
    good[rng.permutation(n)[:max(2, int(round(inlier_share * n)))]] = True
    good[[0, n - 1]] = True                                 # an inlier in the first and in the last lane trip
    kp_t[~good] += rng.uniform(3.0, 8.0, size=(int((~good).sum()), 2)) * rng.choice([-1.0, 1.0], size=(int((~good).sum()), 2))
    m = np.stack([np.arange(n), np.arange(n)], axis=1)
    return kp_s, kp_t, m, good


def random_hypotheses(n, n_iter, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n, size=n_iter)
    j = rng.integers(0, n - 1, size=n_iter)
    j += j >= i
    return np.stack([i, j], axis=1).astype(np.int64)


def uniform_draws(n):
    """-> (u (300, 2) in [0, 1) with the ends of both ranges, the index pairs i = floor(u0 n), j = floor(u1 (n - 1)), j += (j >= i))."""
    u = np.random.default_rng(n).random((300, 2))
    u[:4] = [[0.0, 0.0], [1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53], [0.5, 0.5], [1.0 / n, 0.0]]
    i = np.floor(u[:, 0] * n).astype(np.int64)
    j = np.floor(u[:, 1] * (n - 1)).astype(np.int64)
    j += j >= i
    return u, np.stack([i, j], axis=1)


# winner order: (rows of the table, rows where the good pair is planted); everywhere else the poor pair
WINNER_TABLES = {"a": (512, (44, 300)),        # one thread, first and second trip
                 "b": (512, (70, 261)),        # wave 1's candidate (70) below wave 0's (261 = thread 5, second trip)
                 "c": (512, (255, 256)),       # last thread of wave 3, first thread's second trip
                 "d": (1000, (999,))}          # only the last row


def winner_case():
    """-> (kp_s, kp_t, matches, good pair, poor pair): the good pair (two inliers) counts every inlier, the poor pair (an
    inlier and an outlier) strictly fewer but more than 0."""
    kp_s, kp_t, m, good = ransac_case(96, seed=77)
    gi = np.flatnonzero(good)
    bi = np.flatnonzero(~good)
    return kp_s, kp_t, m, (int(gi[3]), int(gi[40])), (int(gi[5]), int(bi[2]))


def winner_table(name, good, poor):
    rows, planted = WINNER_TABLES[name]
    t = np.tile(np.array(poor, dtype=np.int64), (rows, 1))
    for q, h in enumerate(planted):
        t[h] = good if q == 0 else good[::-1]              # the same two matches the other way round: the same fit, the same count
    return t


def threshold_case():
    """A pure translation by (3, -2) on dyadic coordinates, thresh 0.625: match 2 misses by exactly 0.625 along x (err ==
    thresh: no inlier), match 3 by 0.625 - 2^-40 (an inlier); matches 0, 1 and 4 are exact.  Every operation of the two-point
    fit on matches (0, 1) and of the errors is exact in float64."""
    kp_s = np.array([[1.0, 2.0], [5.0, -3.0], [2.5, 0.5], [-4.0, 1.25], [0.75, 6.0]])
    kp_t = kp_s + np.array([3.0, -2.0])
    kp_t[2, 0] += 0.625
    kp_t[3, 0] += 0.625 - 2.0 ** -40
    m = np.stack([np.arange(5), np.arange(5)], axis=1)
    return kp_s, kp_t, m, 0.625


def rigid_pairs():
    """name -> (src (2, 2), dst (2, 2)): two-point fits at the yaws where the closed form is at an edge, near the origin
    and 1e4 m away; the separation of the 'close' pairs is the minimum keypoint distance 0.3 m."""
    out = {}
    for where, c in (("near", np.array([2.0, -1.0])), ("far", np.array([1e4, -2e4]))):
        s = c + np.array([[0.5, 0.25], [-1.75, 2.0]])
        t = np.array([0.5, -0.25])
        rel = s - c
        out[f"yaw0_{where}"] = (s, s + t)
        out[f"yaw90_{where}"] = (s, c + np.stack([-rel[:, 1], rel[:, 0]], axis=1) + t)
        out[f"yaw-90_{where}"] = (s, c + np.stack([rel[:, 1], -rel[:, 0]], axis=1) + t)
        out[f"yaw180_{where}"] = (s, c - rel + t)                    # a < 0, b = 0 exactly
        th = np.deg2rad(179.999)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out[f"yaw179.999_{where}"] = (s, rel @ R.T + c + t)
        close = c + np.array([[0.0, 0.0], [0.18, 0.24]])             # 0.3 m apart
        th = np.deg2rad(37.0)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out[f"close_{where}"] = (close, (close - c) @ R.T + c + t)
    return out


def chain_clouds():
    """raw clouds of the chain test: a cloud whose 0.2 m filter keeps close to 2048 rows, its moved copy, a room scan pair,
    and ten rows far apart (exactly 10 filtered rows: the least the reference aligns)."""
    rng = np.random.default_rng(41)
    big = rng.uniform(-25.0, 25.0, size=(2030, 2))
    th = np.deg2rad(4.0)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    ten = np.stack([np.arange(10) * 0.9 - 3.0, np.cos(np.arange(10)) * 2.0], axis=1)
    a, b = synth.scan(POSE, 51, n_beams=700), synth.scan((0.8, -0.1, 0.3), 52, n_beams=650)
    return [big, big @ R.T + np.array([0.3, -0.2]), a, b, ten]


def many_pair_clouds():
    return [synth.scan((0.5 + 0.1 * i, -0.3, 0.1 + 0.05 * i), 60 + i, n_beams=260 + 7 * i) for i in range(4)]
