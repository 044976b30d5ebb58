"""GPU parity of the feature-based pre-alignment with the reference (utilities/features.py:35-160, 247-315), stage by
stage, every stage fed the input the reference recorded for it (tests/golden/features.npz, made by
tests/golden/make_golden_features.py).  The reference's end-to-end result is not reproducible — its keypoint order among
equal curvatures is an accident of np.argsort — so the chain is pinned to the composition of its own stages instead."""
import numpy as np
import pytest

from conftest import load_golden, rot_err

pytestmark = pytest.mark.gpu

CLOUDS = [f"c{i}" for i in range(8)] + ["s0", "s1", "s2", "s3", "few_t"]
PAIRS = [f"p{i}" for i in range(4)]


@pytest.fixture(scope="module")
def g():
    return load_golden("features")


@pytest.fixture(autouse=True)
def quiet():
    from utilities import features
    keep, features.VERBOSE = features.VERBOSE, False
    yield
    features.VERBOSE = keep


def test_curvature_within_the_references_own_rounding(g):
    """Tolerance: 10 x the largest relative difference between the reference and the reference's own code with the
    neighbours in row order (recorded by the generator: its sensitivity to summation order; the kernel adds a closed-form
    eigen solve).  Rows with one neighbour set: one value, bit for bit."""
    from scipy.spatial import KDTree
    from utilities import features
    tol = 10.0 * float(g["curv_tol"])
    worst = 0.0
    for c in CLOUDS:
        pts, want = g[c + "_pts"], g[c + "_curv"]
        got = features.compute_curvature(pts, k=10)
        scale = np.maximum(np.abs(got), np.abs(want))
        rel = np.where(scale > 0, np.abs(got - want) / np.where(scale > 0, scale, 1.0), 0.0)
        worst = max(worst, float(rel.max()))
        print(f"{c}: n={len(pts)} largest relative difference {rel.max():.3e} (allowed {tol:.3e})")
        assert rel.max() <= tol, c
        kc = min(10, len(pts) - 1)
        _, nn = KDTree(pts).query(pts, k=kc + 1)
        groups = {}
        for i, s in enumerate(np.sort(np.atleast_2d(nn), axis=1)):
            groups.setdefault(tuple(s), []).append(i)
        shared = [v for v in groups.values() if len(v) > 1]
        for v in shared:
            assert len(set(got[v].tolist())) == 1, (c, v)
        if c == "c0":
            assert len(shared) > 0
    print("largest relative difference over all clouds", worst)


def test_keypoints_identical_on_the_reference_curvature(g):
    from utilities import features
    for c in CLOUDS:
        got = features.extract_keypoints(g[c + "_pts"], g[c + "_curv"], top_n=100, min_dist=0.3)
        assert got.dtype == np.array([0], dtype=int).dtype and np.array_equal(got, g[c + "_kp"]), c
    got = features.extract_keypoints(g["c0_pts"], g["c0_curv"], top_n=7, min_dist=0.3)
    assert np.array_equal(got, g["c0_kp"][:7])


def test_descriptors_bit_equal(g):
    from utilities import features
    for c in CLOUDS:
        got = features.compute_descriptors(g[c + "_pts"], g[c + "_kp"], k=30)
        assert got.shape == g[c + "_desc"].shape and np.array_equal(got, g[c + "_desc"]), c


def test_matches_identical(g):
    from utilities import features
    for i, p in enumerate(PAIRS):
        got = features.match_descriptors(g[f"c{2 * i}_desc"], g[f"c{2 * i + 1}_desc"], ratio=0.8)
        assert isinstance(got, list) and got == [tuple(int(x) for x in m) for m in g[p + "_matches"]], p
    assert features.match_descriptors(g["c2_desc"], g["few_t_desc"], ratio=0.8) == [tuple(m) for m in g["few_matches"]]
    assert features.match_descriptors(g["c0_desc"][:0], g["c1_desc"]) == [] and features.match_descriptors(g["c0_desc"], g["c1_desc"][:1]) == []


def _ransac_direct(kp_s, kp_t, matches, n_iter, hyp_idx=None, hyp_u=None, thresh=0.5):
    """icpmi_feature_ransac_batch on one pair of keypoint lists -> (record, inliers of every hypothesis)."""
    import torch
    from icpmi import _lib, batch as _b
    cs = _b.CloudSet.from_numpy([kp_s, kp_t])
    dev = cs.pts.device
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    S = max(len(kp_s), len(kp_t), len(matches))
    kp = np.zeros((2, S), dtype=np.int32)
    kp[0, :len(kp_s)], kp[1, :len(kp_t)] = np.arange(len(kp_s)), np.arange(len(kp_t))
    mm = np.zeros((S, 2), dtype=np.int32)
    mm[:len(matches)] = matches
    d_kp, d_kc, d_ps, d_pt, d_m, d_mc = i32(kp), i32([len(kp_s), len(kp_t)]), i32([0]), i32([1]), i32(mm), i32([len(matches)])
    d_hi = i32(hyp_idx) if hyp_idx is not None else None
    d_hu = torch.from_numpy(np.ascontiguousarray(hyp_u, dtype=np.float64)).to(dev) if hyp_u is not None else None
    rec = torch.zeros((1, 16), dtype=torch.float64, device=dev)
    counts = torch.full((n_iter,), -1, dtype=torch.int32, device=dev)
    P = _b._ptr
    _lib.check(_lib.lib().icpmi_feature_ransac_batch(P(cs.pts), P(cs.off), None, P(d_kp), P(d_kc), S, P(d_ps), P(d_pt), 1, P(d_m), P(d_mc),
                                                     P(d_hi), P(d_hu), n_iter, 0, thresh, P(rec), P(counts), _b._stream()), "ransac")
    return rec.cpu().numpy()[0], counts.cpu().numpy().astype(np.int64)


def test_ransac_counts_winner_and_transform(g):
    from utilities import features
    for p in PAIRS + ["dup"]:
        draws = g[p + "_draws"]
        rec, counts = _ransac_direct(g[p + "_kp_s"], g[p + "_kp_t"], g[p + "_matches"], len(draws), hyp_idx=draws)
        assert np.array_equal(counts, g[p + "_counts"]), p                                    # every hypothesis of the reference
        assert int(rec[13]) == int(g[p + "_best"]) and int(rec[5]) == int(g[p + "_n_inliers"]), p
        np.random.seed(int(g[p + "_seed"]))
        R, t, n_in = features.ransac_align(g[p + "_kp_s"], g[p + "_kp_t"], [tuple(m) for m in g[p + "_matches"]],
                                           n_iter=len(draws), inlier_thresh=0.5)
        assert n_in == int(g[p + "_n_inliers"]), p
        assert np.array_equal(R.reshape(4), rec[6:10]) and np.array_equal(t, rec[10:12])      # the drop-in drew the same pairs
        e = rot_err(R, t, g[p + "_R"], g[p + "_t"])
        print(p, "rot_err", e)
        assert e < 1e-9, p
        st = np.random.get_state()
        assert np.array_equal(st[1], g[p + "_state_keys"]) and st[2] == int(g[p + "_state_pos"])


def test_uniform_draws_map_to_the_documented_index_pairs(g):
    """hyp_u -> (i, j): i = floor(u0 n), j = floor(u1 (n - 1)), j += (j >= i), taken on the host here and handed over as
    index pairs: the same inliers per hypothesis, the same winner, the same record."""
    kp_s, kp_t, m = g["p0_kp_s"], g["p0_kp_t"], g["p0_matches"]
    n = len(m)
    u = np.random.default_rng(21).random((500, 2))
    u[:4] = [[0.0, 0.0], [0.999999999, 0.999999999], [0.5, 0.5], [1.0 / n, 0.0]]            # the ends of both ranges
    i = np.floor(u[:, 0] * n).astype(np.int64)
    j = np.floor(u[:, 1] * (n - 1)).astype(np.int64)
    j += j >= i
    assert (i != j).all() and i.max() == n - 1 and j.max() == n - 1 and min(i.min(), j.min()) == 0
    rec_u, counts_u = _ransac_direct(kp_s, kp_t, m, len(u), hyp_u=u)
    rec_i, counts_i = _ransac_direct(kp_s, kp_t, m, len(u), hyp_idx=np.stack([i, j], axis=1))
    assert np.array_equal(counts_u, counts_i) and counts_u.max() >= 2 and np.array_equal(rec_u, rec_i)
    # a row that names a match the pair does not have, or one match twice, counts no inliers
    _, c = _ransac_direct(kp_s, kp_t, m, 3, hyp_idx=[[0, n], [2, 2], [-1, 1]])
    assert c.tolist() == [0, 0, 0]


def test_device_order_rule_is_a_stable_descending_sort(g):
    """order == NULL: descending curvature, ties by ascending row — the walk np.argsort(-curv, kind="stable") gives."""
    import torch
    from icpmi import _lib, batch as _b
    for c in ("c0", "c3", "s1", "few_t"):
        pts, curv = g[c + "_pts"], g[c + "_curv"].copy()
        if c == "c3":
            curv = np.round(curv, 2)                       # many exact ties, at every rank
            assert len(np.unique(curv)) < len(curv) // 2
        cs = _b.CloudSet.from_numpy([pts])
        dev = cs.pts.device
        out = []
        for order in (None, np.argsort(-curv, kind="stable")):
            d_curv = torch.from_numpy(curv).to(dev)
            d_order = None if order is None else torch.from_numpy(order.astype(np.int32)).to(dev)
            kp, cnt = torch.zeros(100, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().icpmi_feature_keypoints_batch(_b._ptr(cs.pts), _b._ptr(cs.off), None, None, 1, _b._ptr(d_curv),
                                                                _b._ptr(d_order), 100, 0.3, _b._ptr(kp), _b._ptr(cnt), 100,
                                                                _b._stream()), "keypoints")
            out.append(kp.cpu().numpy()[:int(cnt.item())])
        assert len(out[0]) >= 2 and np.array_equal(out[0], out[1]), c


def test_feature_based_alignment_runs_and_returns_early(g, capsys):
    from utilities import features
    features.VERBOSE = True
    np.random.seed(3)
    R, t, n = features.feature_based_alignment(g["p0_raw_s"], g["p0_raw_t"])
    assert R.shape == (2, 2) and t.shape == (2,) and isinstance(n, int) and abs(np.linalg.det(R) - 1) < 1e-9
    assert "Feature alignment:" in capsys.readouterr().out
    ident = lambda r: np.array_equal(r[0], np.eye(2)) and np.array_equal(r[1], np.zeros(2)) and r[2] == 0   # noqa: E731
    assert ident(features.feature_based_alignment(g["p0_raw_s"][:8], g["p0_raw_t"]))                     # under 10 rows, features.py:281
    blob = np.random.default_rng(1).uniform(0.0, 0.12, size=(200, 2))
    assert ident(features.feature_based_alignment(blob, g["p0_raw_t"], voxel_size=0.01))                # one keypoint, features.py:290
    assert ident(features.feature_based_alignment(g["p0_raw_s"], g["p0_raw_t"], ratio_threshold=1e-6))  # no match, features.py:299


def _compose(raw_s, raw_t, init, hyp_u, cfg):
    """One pair through the single-stage calls with the device order rule -> the record slots the chain must equal."""
    import torch
    from icpmi import _lib, batch as _b
    from utilities import icp as uicp
    L = _lib.lib()
    src = raw_s if init is None else None
    if init is not None:
        # the chain's own product, fma(y, R[c][1], x * R[c][0]) + t: the fused step in exact rational arithmetic, rounded once
        from fractions import Fraction as F
        r = [float(v) for v in init]
        fma = lambda a, b, c: float(F(a) * F(b) + F(c))   # noqa: E731
        src = np.array([[fma(y, r[1], x * r[0]) + r[4], fma(y, r[3], x * r[2]) + r[5]] for x, y in raw_s.tolist()])
    fs, ft = uicp.voxel_downsample(src, cfg["voxel_size"]), uicp.voxel_downsample(raw_t, cfg["voxel_size"])
    rec = np.zeros(16); rec[6] = rec[9] = 1.0; rec[13] = -1.0
    rec[0], rec[1] = len(fs), len(ft)
    if len(fs) < 10 or len(ft) < 10:
        rec[12] = 1
        return rec
    cs = _b.CloudSet.from_numpy([fs, ft])
    dev = cs.pts.device
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    S = (cfg["top_n"] + 7) // 8 * 8
    curv = torch.zeros(cs.total_rows, dtype=torch.float64, device=dev)
    kp, kpc = torch.zeros((2, S), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    desc, dl = torch.zeros((2, S, 32), dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    m, mc = torch.zeros((S, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros((1, 16), dtype=torch.float64, device=dev)
    ps, pt, hu = i32([0]), i32([1]), torch.from_numpy(hyp_u).to(dev)
    P, st = _b._ptr, _b._stream()
    _lib.check(L.icpmi_feature_curvature_batch(P(cs.pts), P(cs.off), None, None, 2, cfg["k_curvature"], P(curv), st), "curvature")
    _lib.check(L.icpmi_feature_keypoints_batch(P(cs.pts), P(cs.off), None, None, 2, P(curv), None, cfg["top_n"], cfg["min_kp_dist"],
                                               P(kp), P(kpc), S, st), "keypoints")
    _lib.check(L.icpmi_feature_descriptors_batch(P(cs.pts), P(cs.off), None, None, 2, P(kp), P(kpc), S, cfg["k_descriptor"], P(desc),
                                                 P(dl), st), "descriptors")
    _lib.check(L.icpmi_feature_match_batch(P(desc), P(dl), P(kpc), S, P(ps), P(pt), 1, cfg["ratio_threshold"] ** 2, P(m), P(mc), st), "match")
    _lib.check(L.icpmi_feature_ransac_batch(P(cs.pts), P(cs.off), None, P(kp), P(kpc), S, P(ps), P(pt), 1, P(m), P(mc), None, P(hu),
                                            len(hyp_u), 0, cfg["inlier_threshold"], P(out), None, st), "ransac")
    r = out.cpu().numpy()[0]
    k = kpc.cpu().numpy()
    rec[2], rec[3] = k
    if k.min() < 2:
        rec[12] = 3
        return rec
    rec[4:] = r[4:]
    if r[12] != 0:
        rec[5] = 0
    return rec


def test_chain_equals_the_composition_of_its_stages(g):
    """Mixed cloud sizes (full scans, halves, a tiny one), without and with a start per pair; init_out follows slam.py:83-88."""
    import torch
    from icpmi.prealign import FEAT_DEFAULTS, FeatureAlignBatch
    cfg = dict(FEAT_DEFAULTS, ransac_iterations=200)
    clouds = [g["p0_raw_s"], g["p0_raw_t"], g["p1_raw_s"][::2], g["p1_raw_t"], g["p2_raw_s"], g["p2_raw_t"][:700], g["p3_raw_s"][:6]]
    ps, pt = [0, 2, 4, 6, 0, 4], [1, 3, 5, 1, 5, 1]
    hyp_u = np.random.default_rng(11).random((200, 2))

    class Fixed:
        def random(self, shape):
            assert shape == (200, 2)
            return hyp_u
    th = np.deg2rad([5.0, -12.0, 0.0, 3.0, 20.0, -7.0])
    init = np.stack([np.cos(th), -np.sin(th), np.sin(th), np.cos(th), 0.1 * np.arange(6), -0.05 * np.arange(6)], axis=1)
    for with_init in (False, True):
        d_in = torch.from_numpy(init.copy()).cuda() if with_init else None
        d_out = torch.full((6, 6), -7.0, dtype=torch.float64, device="cuda")
        b = FeatureAlignBatch(clouds, ps, pt, cfg, rng=Fixed(), init_in=d_in, init_out=d_out)
        rec = b.run().cpu().numpy()[:6]
        out = d_out.cpu().numpy()
        assert int(rec[3, 12]) == 1 and (rec[:3, 12] == 0).all()                      # the 6-row source: under 10 rows
        for q in range(6):
            want = _compose(clouds[ps[q]], clouds[pt[q]], init[q] if with_init else None, hyp_u, cfg)
            assert np.array_equal(rec[q], want), (with_init, q, rec[q], want)
            start = init[q] if with_init else np.array([1.0, 0, 0, 1.0, 0, 0])
            if rec[q, 12] == 0 and rec[q, 5] >= cfg["min_inliers"]:
                Rf, tf = rec[q, 6:10].reshape(2, 2), rec[q, 10:12]
                R0, t0 = start[:4].reshape(2, 2), start[4:]
                e = rot_err(out[q, :4].reshape(2, 2), out[q, 4:], Rf @ R0, t0 @ Rf.T + tf)
                assert e < 1e-12, (q, e)                                              # two-term products of O(1) numbers: a few ulps
            else:
                assert np.array_equal(out[q], start), q
        assert (rec[:, 5] >= cfg["min_inliers"]).any()
    # a batch with min_inliers nobody reaches leaves every start as it was
    d_in = torch.from_numpy(init.copy()).cuda()
    b = FeatureAlignBatch(clouds, ps, pt, dict(cfg, min_inliers=10 ** 6), rng=Fixed(), init_in=d_in, init_out=d_in)
    b.run()
    assert np.array_equal(d_in.cpu().numpy(), init)


def test_rotation_search_method_is_unchanged(g):
    from icpmi.prealign import run_icp_pair_batch
    srcs, tgts = [g[f"p{i}_raw_s"] for i in range(4)], [g[f"p{i}_raw_t"] for i in range(4)]
    icp = dict(error_threshold=1e-9, max_iterations=60, voxel_size=0.08, method="point_to_line", normal_k=10)
    a = run_icp_pair_batch(srcs, tgts, icp, {}, error_accept=0.08)
    b = run_icp_pair_batch(srcs, tgts, icp, {}, error_accept=0.08, alignment_method="rotation_search")
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert a[3]["first_accepted"] == b[3]["first_accepted"] and np.array_equal(a[3]["iters"], b[3]["iters"])
    assert "feature_records" not in b[3]


def test_methods_features_and_both_run(g):
    """A reference configuration with method "features" or "both" runs through the batched _run_icp_pair."""
    from icpmi.prealign import run_icp_pair_batch
    srcs, tgts = [g[f"p{i}_raw_s"] for i in range(4)], [g[f"p{i}_raw_t"] for i in range(4)]
    icp = dict(error_threshold=1e-7, max_iterations=100, voxel_size=0.06, method="point_to_line", normal_k=10)
    for method in ("features", "both"):
        R, t, err, info = run_icp_pair_batch(srcs, tgts, icp, {}, alignment_method=method, rng=np.random.default_rng(5))
        assert np.isfinite(err).all() and info["feature_records"].shape == (4, 16)
        assert (info["feature_records"][:, 12] == 0).all(), method
        print(method, "errors", err, "inliers", info["feature_records"][:, 5])


def test_pairs_the_kernels_cannot_align_have_no_feature_start(g):
    """Status 2 (a filtered cloud above the 2 048 rows held on chip) and status 5 (descriptors of different lengths): identity,
    zeros, 0 inliers, init_out left as init_in — and the batch around them is unharmed."""
    import torch
    from icpmi.prealign import FEAT_DEFAULTS, FeatureAlignBatch, run_icp_pair_batch
    rng = np.random.default_rng(2)
    big = rng.uniform(-30.0, 30.0, size=(2600, 2))                        # 0.2 m voxels keep nearly all of them apart
    short = g["p1_raw_t"][:60]                                            # filters to fewer than 31 rows: descriptors of n - 1
    clouds = [g["p0_raw_s"], g["p0_raw_t"], big, short]
    init = np.tile([1.0, 0.0, 0.0, 1.0, 0.25, -0.5], (3, 1))
    d = torch.from_numpy(init.copy()).cuda()
    b = FeatureAlignBatch(clouds, [0, 2, 0], [1, 1, 3], dict(FEAT_DEFAULTS, ransac_iterations=100), init_in=d, init_out=d)
    R, t, n_in, rec = b.results(b.run())
    print("filtered rows", rec[:, 0], rec[:, 1], "status", rec[:, 12])
    assert rec[:, 12].astype(int).tolist() == [0, 2, 5]
    assert 10 <= rec[2, 1] < 31 and rec[1, 0] > 2048
    out = d.cpu().numpy()
    for q in (1, 2):
        assert np.array_equal(R[q], np.eye(2)) and np.array_equal(t[q], np.zeros(2)) and n_in[q] == 0
        assert np.array_equal(out[q], init[q])
    assert n_in[0] >= 3 and not np.array_equal(out[0], init[0])
    icp = dict(error_threshold=1e-7, max_iterations=60, voxel_size=0.1, method="point_to_line", normal_k=10)
    _, _, err, info = run_icp_pair_batch([clouds[0], big[:2048], clouds[0]], [clouds[1], clouds[1], short], icp, {}, alignment_method="features")
    assert np.isfinite(err[0]) and info["feature_records"][:, 12].astype(int)[0] == 0


def test_gate_and_early_stop_act_on_the_icp_stage_with_features(g):
    """error_accept / stop_after_first_accepted with "features" and "both": the first accepted candidate of the full run, and
    every record up to it bit for bit."""
    from icpmi.prealign import run_icp_pair_batch
    srcs = [g["e2e_src"][i] for i in range(4)] + [g[f"p{i}_raw_s"] for i in range(4)]
    tgts = [g["e2e_tgt"][i] for i in range(4)] + [g[f"p{i}_raw_t"] for i in range(4)]
    icp = dict(error_threshold=1e-7, max_iterations=100, voxel_size=0.06, method="point_to_line", normal_k=10)
    for method in ("features", "both"):
        kw = dict(alignment_method=method, rng=None, error_accept=0.08)
        full = run_icp_pair_batch(srcs, tgts, icp, {}, **kw)
        gated = run_icp_pair_batch(srcs, tgts, icp, {}, stop_after_first_accepted=True, **kw)
        first = full[3]["first_accepted"]
        print(method, "errors", full[2], "first accepted", first)
        assert first >= 0 and gated[3]["first_accepted"] == first
        for x, y in zip(full[:3], gated[:3]):
            assert np.array_equal(x[:first + 1], y[:first + 1])


def test_end_to_end_outcome_not_worse_than_the_reference(g):
    """Pairs with yaw up to 180 degrees that the reference's ICP registers ONLY from the reference's feature start (the
    generator requires 8 of them: error below the 0.08 gate with "features", above it without).  As many of them must end
    below the gate here as in the reference.  The reference's own draws are the hypotheses (a row naming a match this run
    does not have counts no inliers: the keypoints, hence the match lists, differ by the tie order of the curvatures)."""
    from icpmi.prealign import run_icp_pair_batch
    n = int(g["e2e_count"])
    assert n == 8 and (g["e2e_err_feat"] < 0.08).all() and (g["e2e_err_none"] >= 0.08).all()
    icp = dict(error_threshold=1e-7, max_iterations=100, voxel_size=0.06, method="point_to_line", normal_k=10)
    errs = []
    for i in range(n):
        _, _, err, info = run_icp_pair_batch([g["e2e_src"][i]], [g["e2e_tgt"][i]], icp, {}, alignment_method="features",
                                             hypotheses=g["e2e_draws"][i])
        errs.append(float(err[0]))
        print(i, "error", errs[-1], "reference", float(g["e2e_err_feat"][i]), "without a start", float(g["e2e_err_none"][i]),
              "matches / inliers", info["feature_records"][0, 4:6])
    assert np.isfinite(errs).all()
    assert sum(e < 0.08 for e in errs) >= int((g["e2e_err_feat"] < 0.08).sum())
