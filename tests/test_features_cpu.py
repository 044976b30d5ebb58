"""CPU-side checks of the feature-based pre-alignment (utilities/features.py:35-160, 247-315 of the reference): the fixture
tests/golden/features.npz is consistent with itself, libicpmi.so exports the new entry points, ``ransac_align`` draws its
hypotheses as the reference does (same draws, same state of the global stream afterwards), and the batched
``_run_icp_pair`` refuses an alignment method the reference does not have."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

NEW_SYMBOLS = ("icpmi_feature_curvature_batch", "icpmi_feature_keypoints_batch", "icpmi_feature_descriptors_batch",
               "icpmi_feature_match_batch", "icpmi_feature_ransac_batch", "icpmi_feature_align_batch",
               "icpmi_feature_align_batch_workspace_bytes")
CLOUDS = [f"c{i}" for i in range(8)] + ["s0", "s1", "s2", "s3", "few_t"]


def test_fixture_is_consistent():
    g = load_golden("features")
    cfg = dict(zip(g["cfg_keys"], g["cfg_values"]))
    assert int(g["n_pairs"]) == 4 and cfg["top_n"] == 100 and cfg["ransac_iterations"] == 1000
    ratio_margin, inlier_margin, walk_margin = g["margins"]
    assert ratio_margin > 1e-9 and inlier_margin > 1e-9 and walk_margin > 1e-12        # what the exact comparisons rest on
    assert 0 < float(g["curv_tol"]) < 1e-9
    for c in CLOUDS:
        pts, curv, order, kp, desc = (g[f"{c}_{k}"] for k in ("pts", "curv", "order", "kp", "desc"))
        n = len(pts)
        assert pts.shape == (n, 2) and curv.shape == (n,) and sorted(order) == list(range(n))
        assert (np.diff(curv[order]) <= 0).all()                                      # a descending order of the curvatures
        assert len(kp) <= 100 and len(set(kp)) == len(kp) and (kp < n).all()
        kd = min(30, n - 1)
        assert desc.shape == (len(kp), kd) and (np.diff(desc, axis=1) >= 0).all()
        d = np.linalg.norm(pts[kp][:, None, :] - pts[kp][None, :, :], axis=2) + np.eye(len(kp))
        assert (d >= cfg["min_kp_dist"]).all()                                        # the suppression held
    assert len(g["s0_pts"]) == 2 and (g["s0_curv"] == 0).all()                        # under 3 neighbours
    assert len(g["s1_pts"]) - 1 < 10 and len(g["s2_pts"]) < 10                        # k clamped; under 10 rows
    assert len(g["few_matches"]) < 2 and len(g["few_t_kp"]) >= 2
    assert int(g["e2e_count"]) == 8 and (g["e2e_err_feat"] < 0.08).all() and (g["e2e_err_none"] >= 0.08).all()   # the start matters
    assert g["e2e_draws"].shape == (8, 1000, 2)
    for p in [f"p{i}" for i in range(4)] + ["dup"]:
        m, draws, counts = g[p + "_matches"], g[p + "_draws"], g[p + "_counts"]
        assert draws.shape == (len(counts), 2) and (draws[:, 0] != draws[:, 1]).all() and draws.max() < len(m)
        best = int(g[p + "_best"])
        assert counts[best] == counts.max() and (counts[:best] < counts[best]).all()   # the first of the largest
        R = g[p + "_R"]
        assert abs(np.linalg.det(R) - 1) < 1e-12 and int(g[p + "_n_inliers"]) >= 2
    m, draws = g["dup_matches"], g["dup_draws"]
    assert (m[draws[:, 0], 1] == m[draws[:, 1], 1]).any()                             # a two-point fit with W = 0 is among them


def test_library_exports_the_feature_entry_points():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()                     # torch first, then the library: one HIP runtime in the process
    L = ctypes.CDLL(path)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS, s
    # the chain's workspace: described once (csrc/features.hip, FtWs); a start per pair adds a source copy per pair
    q = lib.icpmi_feature_align_batch_workspace_bytes
    assert q(-1, 1, 1, 1, 100, 0) == 0 and q(1000, 3, 500, 2, 100, 0) > 1000 * 24
    assert q(1000, 3, 500, 2, 100, 1) >= q(1000, 3, 500, 2, 100, 0) + 2 * 500 * 40


def test_ransac_draws_are_the_references(monkeypatch):
    """After np.random.seed(s), ransac_align must hand the kernel the index pairs the reference drew and leave the global
    stream in the state the reference leaves it in (the launch itself is replaced: no GPU here)."""
    import torch
    from utilities import features
    g = load_golden("features")
    seen = {}

    class Stop(Exception):
        pass

    def fake_from_numpy(cls, clouds, device=None):
        raise Stop()
    real_choice = np.random.choice

    def choice(*a, **k):
        r = real_choice(*a, **k)
        seen.setdefault("draws", []).append(np.array(r))
        return r
    monkeypatch.setattr(features._b.CloudSet, "from_numpy", classmethod(fake_from_numpy))
    monkeypatch.setattr(np.random, "choice", choice)
    for p in ("p0", "p2", "dup"):
        seen.clear()
        np.random.seed(int(g[p + "_seed"]))
        with pytest.raises(Stop):
            features.ransac_align(g[p + "_kp_s"], g[p + "_kp_t"], [tuple(m) for m in g[p + "_matches"]], n_iter=len(g[p + "_draws"]))
        st = np.random.get_state()
        assert np.array_equal(np.array(seen["draws"]), g[p + "_draws"])
        assert np.array_equal(st[1], g[p + "_state_keys"]) and st[2] == int(g[p + "_state_pos"])
    assert features.ransac_align(g["p0_kp_s"], g["p0_kp_t"], [(0, 1)]) == (None, None, 0)       # features.py:130-131


def test_unknown_alignment_method_is_refused():
    from icpmi.prealign import run_icp_pair_batch
    a = np.zeros((5, 2))
    with pytest.raises(ValueError, match="alignment_method"):
        run_icp_pair_batch([a], [a], alignment_method="ransac")


def test_numpy_helpers_match_their_definitions():
    from utilities import features
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(7, 5)), rng.normal(size=(4, 5))
    want = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    assert np.allclose(features._pairwise_sq(a, b), want, atol=1e-12)
    th = 0.7
    R0 = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    src = rng.normal(size=(6, 2))
    R, t = features._rigid_from_points(src, src @ R0.T + [1.0, -2.0])
    assert np.allclose(R, R0, atol=1e-12) and np.allclose(t, [1.0, -2.0], atol=1e-12)
