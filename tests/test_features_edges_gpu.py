"""The feature-alignment kernels (csrc/features.hip) at their edges, against the extended-precision reference of
tests/features_ref.py on the inputs of tests/features_cases.py (tests/test_features_edges_cpu.py proves, without a GPU,
that every input has the property relied on here).  Curvature: absolute error within 4 x the error of the reference's
own float64 expression on the same neighbour sets (not below 4 * 2^-52).  Rigid fits: rot_err within 4 x that of the
reference's NumPy SVD expression (not below 8 * 2^-52 * max(1, |mu|)).  Everything else — keypoints, descriptors, match
lists, inliers of every hypothesis, winners, statuses — is exact."""
import functools

import numpy as np
import pytest

import features_cases as fc
import features_ref as fr

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4
SENT = -77


@pytest.fixture(autouse=True)
def quiet():
    from utilities import features
    keep, features.VERBOSE = features.VERBOSE, False
    yield
    features.VERBOSE = keep


@functools.lru_cache(maxsize=None)
def _ref_curvature(name, k):
    pts = fc.big_room(int(name[3:])) if name.startswith("big") else fc.curvature_clouds()[name]
    want, _, idx = fr.curvature(pts, k)
    y, tol = fr.curvature_tolerance(pts, idx, want)
    return pts, want, idx, y, tol


def _i32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _check_curvature_and_descriptors(name, k):
    from utilities import features
    pts, want, idx, y, tol = _ref_curvature(name, k)
    n, kk = len(pts), idx.shape[1]
    got = features.compute_curvature(pts, k=k)
    err = float(np.abs(got.astype(fr.LD) - want).max())
    print(f"{name} n={n} k={k} kk={kk}: curvature error {err:.3e}, yardstick {y:.3e}, allowed {tol:.3e}")
    assert got.shape == (n,) and err <= tol, (name, k, err, tol)
    if kk < 3:
        assert (got == 0.0).all()
    groups = {}
    for i, s in enumerate(np.sort(idx, axis=1)):
        groups.setdefault(s.tobytes(), []).append(i)
    for v in groups.values():
        assert len(set(got[v].tolist())) == 1, (name, k, v)                   # one neighbour set, one value, bit for bit
    kp = np.unique(np.concatenate([np.arange(0, n, max(1, n // 97)), [n - 1]]))[:256]
    desc = features.compute_descriptors(pts, kp, k=k)
    assert desc.shape == (len(kp), min(k, n - 1)), (name, k, desc.shape)      # desc_len = min(k, n - 1)
    assert np.array_equal(desc, fr.descriptors(pts, kp, k)), (name, k)
    return err, y


@pytest.mark.parametrize("name", ["room", "shifted", "straight", "line", "lattice"] + [f"small{n}" for n in fc.SMALL_N])
def test_curvature_and_descriptors_every_instantiation_and_both_kk_branches(name):
    """k + 1 = 3, 7, 8 | 9, 11, 16 | 17, 31, 32: ft_curvature_rows / ft_descriptor_rows <8>, <16>, <32>, each with kk < KK
    and kk == KK; the small clouds put kk = n on both sides of each bound.  The lattice has true ties at the k-th neighbour
    (the set is decided by `d == dk && j <= pk`); the line is exactly collinear (mid - rad cancels completely)."""
    worst = (0.0, 0.0)
    for k in fc.K_ALL:
        worst = max(worst, _check_curvature_and_descriptors(name, k))
    print(f"{name}: worst curvature error {worst[0]:.3e} at a yardstick of {worst[1]:.3e}")


@pytest.mark.parametrize("n", [2047, 2048])
def test_curvature_and_descriptors_at_the_row_capacity(n):
    for k in (10, 31):
        _check_curvature_and_descriptors(f"big{n}", k)


# ── keypoints ─────────────────────────────────────────────────────────────────────────────────────────
def _keypoints_raw(clouds, curv, order, top_n, min_dist, kp_stride, cloud_ids=None, cnt=None):
    """icpmi_feature_keypoints_batch on a set of clouds -> (return code, kp (C, kp_stride), kp_cnt (C,)), both filled with
    SENT before the call."""
    import torch
    from icpmi import _lib, batch as _b
    cs = _b.CloudSet.from_numpy(clouds)
    dev = cs.pts.device
    d_curv = None if curv is None else torch.from_numpy(np.ascontiguousarray(np.concatenate(curv), dtype=np.float64)).to(dev)
    d_order = None if order is None else _i32(np.concatenate(order), dev)
    d_ids = None if cloud_ids is None else _i32(cloud_ids, dev)
    d_cnt = None if cnt is None else _i32(cnt, dev)
    kp = torch.full((len(clouds), kp_stride), SENT, dtype=torch.int32, device=dev)
    kc = torch.full((len(clouds),), SENT, dtype=torch.int32, device=dev)
    P = _b._ptr
    rc = _lib.lib().icpmi_feature_keypoints_batch(P(cs.pts), P(cs.off), P(d_cnt), P(d_ids), len(clouds) if cloud_ids is None else len(cloud_ids),
                                                  P(d_curv), P(d_order), top_n, float(min_dist), P(kp), P(kc), kp_stride, _b._stream())
    torch.cuda.synchronize()
    return rc, kp.cpu().numpy(), kc.cpu().numpy()


@pytest.mark.parametrize("n", fc.KP_LATTICE_N)
def test_keypoints_on_a_lattice_of_tied_curvatures(n):
    """n = 2048: the device sort at npad = 2048, the walk over a full LDS cloud, 256 keypoints = four lane trips of `kept`,
    top_n the binding limit.  1025: 1023 pad slots; 1024, 64: none; 65, 1: the smallest sorts."""
    pts = fc.keypoint_lattice(n)
    curv = fr.curvature(pts, 10)[0].astype(np.float64)
    want, _ = fr.keypoints(pts, curv, 256, 0.3)
    for order in (None, np.argsort(-curv, kind="stable")):
        rc, kp, kc = _keypoints_raw([pts], [curv], None if order is None else [order], 256, 0.3, 256)
        assert rc == 0 and kc[0] == len(want) and np.array_equal(kp[0, :kc[0]], want), (n, order is None)
        assert (kp[0, kc[0]:] == SENT).all()
    if n == 2048:
        assert len(want) == 256


def test_keypoint_at_exactly_min_dist_is_kept():
    for order, min_dist, kept in fc.TRIANGLE_CASES:
        rc, kp, kc = _keypoints_raw([fc.TRIANGLE], None, [np.array(order)], 3, min_dist, 8)
        assert rc == 0 and kp[0, :kc[0]].tolist() == kept, (order, min_dist)


def test_keypoint_limits_and_refusals():
    """top_n binds below what the cloud would yield; top_n above kp_stride or above 256 is refused before any launch
    (include/icpmi.h: top_n <= kp_stride, at most ICPMI_FT_MAX_KP keypoints) and nothing is written."""
    pts = fc.keypoint_lattice(2048)
    curv = fr.curvature(pts, 10)[0].astype(np.float64)
    for top_n, stride in ((8, 8), (100, 104), (255, 256)):
        want, _ = fr.keypoints(pts, curv, top_n, 0.3)
        rc, kp, kc = _keypoints_raw([pts], [curv], None, top_n, 0.3, stride)
        assert rc == 0 and kc[0] == top_n == len(want) and np.array_equal(kp[0, :top_n], want) and (kp[0, top_n:] == SENT).all()
    for top_n, stride in ((100, 8), (300, 304), (257, 264)):
        rc, kp, kc = _keypoints_raw([pts], [curv], None, top_n, 0.3, stride)
        assert rc == ERR_UNSUPPORTED and (kp == SENT).all() and (kc == SENT).all(), (top_n, stride)


def test_order_entries_that_are_no_row_are_ignored():
    pts = fc.curvature_clouds()["room"]
    n = len(pts)
    curv = fr.curvature(pts, 10)[0].astype(np.float64)
    order = np.argsort(-curv, kind="stable").astype(np.int64)
    want, _ = fr.keypoints(pts, curv, 100, 0.3, order=order)
    bad = order.copy()
    bad[[0, 5, n // 2, n - 1]] = [n, -1, 2 ** 31 - 1, -(2 ** 31)]
    want_bad, _ = fr.keypoints(pts, curv, 100, 0.3, order=bad)
    rc, kp, kc = _keypoints_raw([pts], None, [bad], 100, 0.3, 104)
    assert rc == 0 and np.array_equal(kp[0, :kc[0]], want_bad) and not np.array_equal(want, want_bad)


def test_selected_clouds_and_counts_leave_the_rest_alone():
    """Three clouds, cloud_ids = [0, 2], cloud 2 with fewer valid rows than its capacity: clouds 0 and 2 as the reference on
    their valid rows; every slot of cloud 1, and every slot past a cloud's keypoints, keeps the fill."""
    import torch
    from icpmi import _lib, batch as _b
    room = fc.curvature_clouds()["room"]
    clouds = [room[:150], room[150:260], fc.big_room(500)]
    cnt = [150, 110, 333]
    S, k_c, k_d = 40, 10, 30
    cs = _b.CloudSet.from_numpy(clouds)
    dev = cs.pts.device
    P, st, L = _b._ptr, _b._stream(), _lib.lib()
    ids, d_cnt = _i32([0, 2], dev), _i32(cnt, dev)
    curv = torch.full((cs.total_rows,), float(SENT), dtype=torch.float64, device=dev)
    kp = torch.full((3, S), SENT, dtype=torch.int32, device=dev)
    kc = torch.full((3,), SENT, dtype=torch.int32, device=dev)
    desc = torch.full((3, S, 32), float(SENT), dtype=torch.float64, device=dev)
    dl = torch.full((3,), SENT, dtype=torch.int32, device=dev)
    assert L.icpmi_feature_curvature_batch(P(cs.pts), P(cs.off), P(d_cnt), P(ids), 2, k_c, P(curv), st) == 0
    assert L.icpmi_feature_keypoints_batch(P(cs.pts), P(cs.off), P(d_cnt), P(ids), 2, P(curv), None, S, 0.3, P(kp), P(kc), S, st) == 0
    assert L.icpmi_feature_descriptors_batch(P(cs.pts), P(cs.off), P(d_cnt), P(ids), 2, P(kp), P(kc), S, k_d, P(desc), P(dl), st) == 0
    curv, kp, kc, desc, dl = (x.cpu().numpy() for x in (curv, kp, kc, desc, dl))
    off = cs.off_host
    assert kc[1] == SENT and dl[1] == SENT and (kp[1] == SENT).all() and (desc[1] == SENT).all() and (curv[off[1]:off[2]] == SENT).all()
    assert (curv[off[2] + cnt[2]:off[3]] == SENT).all()                        # rows past the count of cloud 2
    for c in (0, 2):
        pts = clouds[c][:cnt[c]]
        want, _, idx = fr.curvature(pts, k_c)
        got = curv[off[c]:off[c] + cnt[c]]
        assert float(np.abs(got.astype(fr.LD) - want).max()) <= fr.curvature_tolerance(pts, idx, want)[1]
        want_kp, _ = fr.keypoints(pts, got, S, 0.3)
        assert 2 <= kc[c] == len(want_kp) and np.array_equal(kp[c, :kc[c]], want_kp) and (kp[c, kc[c]:] == SENT).all()
        assert dl[c] == k_d and np.array_equal(desc[c, :kc[c], :k_d], fr.descriptors(pts, want_kp, k_d)) and (desc[c, :kc[c], k_d:] == 0).all() and (desc[c, kc[c]:] == SENT).all()


# ── matching ──────────────────────────────────────────────────────────────────────────────────────────
def _match(da, db, ratio=0.8):
    from utilities import features
    got = features.match_descriptors(da, db, ratio=ratio)
    want, _ = fr.matches(da, db, ratio)
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("q,length", list(enumerate(fc.MATCH_LENS)))
def test_matches_in_every_wave_in_source_order(q, length):
    """256 x 256 descriptors: matches in all four waves of the ballot compaction, then with one wave empty; a NaN source row
    and a NaN target row match nothing and every other match keeps its place in the list."""
    for empty in (None, 1 + q % 3):
        da, db, want = fc.match_descriptors_case(length, empty, seed=100 + q)
        got = _match(da, db)
        assert [i for i, _ in got] == np.flatnonzero(want).tolist()
        da2, db2, i_nan, j_nan = fc.with_nan_rows(da, db, got)
        got2 = _match(da2, db2)
        assert all(i != i_nan and j != j_nan for i, j in got2) and set(m for m in got if m[0] != i_nan and m[1] != j_nan) <= set(got2)


def test_match_list_edges():
    da, db, _ = fc.match_descriptors_case(7, None, seed=120, ns=65, only=64)
    assert [i for i, _ in _match(da, db)] == [64]                               # the only match: first lane of the second wave
    da, db, _ = fc.match_descriptors_case(7, None, seed=121, ns=9, nt=2)
    assert 0 < len(_match(da, db)) < 9                                          # nt = 2: the least the ratio test takes
    for a, db, ratio, want in fc.match_tie_cases():                              # D0 == D1, the lower index, the boundary of <
        assert _match(a, db, ratio=ratio) == want


# ── RANSAC ────────────────────────────────────────────────────────────────────────────────────────────
def _ransac(kp_s, kp_t, m, hyp, thresh=0.5, what=""):
    """The kernel on an index table against the reference: counts of every hypothesis, winner, inliers exact; R, t within the
    rigid tolerance of the points the final fit was made on."""
    from test_features_gpu import _ransac_direct
    hyp = np.asarray(hyp, dtype=np.int64).reshape(-1, 2)
    rec, counts = _ransac_direct(kp_s, kp_t, m, len(hyp), hyp_idx=hyp, thresh=thresh)
    want = fr.ransac(kp_s, kp_t, m, hyp, thresh)
    assert np.array_equal(counts, want["counts"]), what
    assert int(rec[13]) == want["best"] and int(rec[5]) == want["inliers"] and int(rec[4]) == len(m) and int(rec[12]) == 0, what
    mm = np.asarray(m).reshape(-1, 2)
    if want["mask"] is not None:
        S, D = kp_s[mm[:, 0]][want["mask"]], kp_t[mm[:, 1]][want["mask"]]
    elif want["best"] >= 0:
        S, D = kp_s[mm[hyp[want["best"]], 0]], kp_t[mm[hyp[want["best"]], 1]]
    else:
        S = D = np.zeros((2, 2))
    y, tol = fr.rigid_tolerance(S, D)
    e = fr.rot_err_ld(rec[6:10], rec[10:12], want["R"], want["t"])
    print(f"{what}: {len(m)} matches, {len(hyp)} hypotheses, winner {want['best']}, {want['inliers']} inliers, rot_err {e:.3e} "
          f"(NumPy SVD {y:.3e}, allowed {tol:.3e})")
    assert e <= tol, (what, e, tol)
    return rec, counts, want


@pytest.mark.parametrize("n", [2, 64, 65, 256])
def test_ransac_at_capacity_and_lane_trip_edges(n):
    """256 matches fill S[] / D[] and take the refit's lane loop round four times (200 inliers); 64 and 65 are one trip and
    one row into the second.  n_iter on both sides of the 256 hypotheses a pass of the workgroup scores."""
    kp_s, kp_t, m, good = fc.ransac_case(n, seed=200 + n)
    for n_iter in ((1, 255, 256, 257, 1000) if n == 256 else (257,)):
        rec, _, want = _ransac(kp_s, kp_t, m, fc.random_hypotheses(n, n_iter, seed=n_iter), what=f"n={n} n_iter={n_iter}")
        if n_iter > 1:
            assert want["inliers"] == int(good.sum())


@pytest.mark.parametrize("name", sorted(fc.WINNER_TABLES))
def test_first_hypothesis_of_the_largest_count_wins(name):
    """Equal best counts planted (a) in one thread's first and second trip, (b) so that wave 1 holds the lower index than
    wave 0, (c) at 255 and 256, (d) only in the last row of 1000 rows: per thread, butterfly, take_first_best over waves."""
    kp_s, kp_t, m, good, poor = fc.winner_case()
    rec, counts, want = _ransac(kp_s, kp_t, m, fc.winner_table(name, good, poor), what=name)
    assert int(rec[13]) == fc.WINNER_TABLES[name][1][0]


def test_error_exactly_at_the_threshold_is_no_inlier():
    kp_s, kp_t, m, thresh = fc.threshold_case()
    rec, counts, _ = _ransac(kp_s, kp_t, m, [[0, 1]], thresh=thresh, what="threshold")
    assert counts.tolist() == [4] and int(rec[5]) == 4                          # 5 matches: the one at err == thresh is out


@pytest.mark.parametrize("name", sorted(fc.rigid_pairs()))
def test_two_point_fits_at_the_edges_of_the_closed_form(name):
    s, d = fc.rigid_pairs()[name]
    rec, _, want = _ransac(s, d, [[0, 0], [1, 1]], [[0, 1]], what=name)
    assert want["inliers"] == 2
    if name.startswith("close"):                                                # both matches on one target keypoint: W = 0, R = I
        rec, _, want = _ransac(s, d, [[0, 0], [1, 0]], [[0, 1]], what=name + " dup")
        assert np.array_equal(rec[6:10], [1.0, 0.0, 0.0, 1.0]) and want["inliers"] == 2


@pytest.mark.parametrize("n", [2, 256])
def test_uniform_draws_map_to_index_pairs(n):
    """i = floor(u0 n), j = floor(u1 (n - 1)), j += (j >= i): at n = 2 u1 decides nothing."""
    from test_features_gpu import _ransac_direct
    kp_s, kp_t, m, _ = fc.ransac_case(n, seed=200 + n)
    u, ij = fc.uniform_draws(n)
    rec_u, counts_u = _ransac_direct(kp_s, kp_t, m, len(u), hyp_u=u)
    rec_i, counts_i, _ = _ransac(kp_s, kp_t, m, ij, what=f"uniform n={n}")
    assert np.array_equal(counts_u, counts_i) and np.array_equal(rec_u, rec_i)


# ── chain ─────────────────────────────────────────────────────────────────────────────────────────────
class _Fixed:
    def __init__(self, u):
        self.u = u

    def random(self, shape):
        assert shape == self.u.shape
        return self.u


def test_chain_at_the_other_template_bounds_and_mixed_sizes():
    """k_curvature = 31 (<32>, kk == KK), k_descriptor = 7 (<8>, kk == KK), top_n = 256; a filtered cloud close to 2048 rows
    and one of exactly 10: the records equal the composition of the single-stage calls."""
    from icpmi.prealign import FEAT_DEFAULTS, FeatureAlignBatch
    from test_features_gpu import _compose
    cfg = dict(FEAT_DEFAULTS, k_curvature=31, k_descriptor=7, top_n=256, ransac_iterations=300)
    clouds = fc.chain_clouds()
    ps, pt = [0, 2, 4], [1, 3, 2]
    hyp_u = np.random.default_rng(12).random((300, 2))
    rec = FeatureAlignBatch(clouds, ps, pt, cfg, rng=_Fixed(hyp_u)).run().cpu().numpy()[:3]
    print("filtered rows", rec[:, 0], rec[:, 1], "keypoints", rec[:, 2], rec[:, 3], "matches", rec[:, 4], "status", rec[:, 12])
    assert 1900 <= rec[0, 0] <= 2048 and 1900 <= rec[0, 1] <= 2048 and rec[2, 0] == 10
    assert rec[0, 2] == 256 and (rec[:, 12] != 2).all() and (rec[:, 12] != 1).all()
    for q in range(3):
        want = _compose(clouds[ps[q]], clouds[pt[q]], None, hyp_u, cfg)
        assert np.array_equal(rec[q], want), (q, rec[q], want)


def test_chain_of_257_pairs():
    """The second workgroup of the finish kernel and, with a start per pair, 257 transformed copies: pairs naming the same
    clouds (and the same start) have identical records, and the last pair equals the composition."""
    import torch
    from icpmi.prealign import FEAT_DEFAULTS, FeatureAlignBatch
    from test_features_gpu import _compose
    cfg = dict(FEAT_DEFAULTS, ransac_iterations=100)
    clouds = fc.many_pair_clouds()
    B = 257
    ps, pt = [b % 4 for b in range(B)], [(b // 4) % 4 for b in range(B)]
    hyp_u = np.random.default_rng(13).random((100, 2))
    kind = np.array(ps) * 4 + np.array(pt)
    th = np.deg2rad(3.0 * kind - 20.0)
    init = np.stack([np.cos(th), -np.sin(th), np.sin(th), np.cos(th), 0.02 * kind, -0.01 * kind], axis=1)
    for with_init in (False, True):
        d_in = torch.from_numpy(init.copy()).cuda() if with_init else None
        d_out = torch.full((B, 6), -7.0, dtype=torch.float64, device="cuda")
        rec = FeatureAlignBatch(clouds, ps, pt, cfg, rng=_Fixed(hyp_u), init_in=d_in, init_out=d_out).run().cpu().numpy()[:B]
        out = d_out.cpu().numpy()
        for v in range(16):
            same = np.flatnonzero(kind == v)
            assert len(same) >= 16 and (rec[same] == rec[same[0]]).all() and (out[same] == out[same[0]]).all(), (with_init, v)
        assert (rec[:, 12] == 0).any() and (out != -7.0).all()
        want = _compose(clouds[ps[256]], clouds[pt[256]], init[256] if with_init else None, hyp_u, cfg)
        assert np.array_equal(rec[256], want), (with_init, rec[256], want)
