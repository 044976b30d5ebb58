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
    # the workspace of both chains: described once (csrc/features.hip, FtWs); a start per pair adds a source copy per pair
    q = lib.icpmi_feature_align_batch_workspace_bytes
    assert q(-1, 1, 1, 1, 100, 0) == 0 and q(1000, 3, 500, 2, 100, 0) > 1000 * 24
    assert q(1000, 3, 500, 2, 100, 1) >= q(1000, 3, 500, 2, 100, 0) + 2 * 500 * 40


FAKE = 4096                                                    # a non-null address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


def test_align_batch_refuses_bad_arguments_on_the_host():
    """Every refusal icpmi_feature_align_batch decides on the host, before any launch (the device pointers are fakes that
    are never dereferenced), and the order in which it decides when two faults coincide: a bad argument before an
    unsupported one, both before "no pairs: nothing to do", that before the host offsets, those before the workspace, and
    the workspace before the host sources of a start per pair."""
    import icpmi
    L = icpmi.lib()
    align = L.icpmi_feature_align_batch
    off = np.array([0, 300, 600], dtype=np.int32)
    src = np.array([0, 1], dtype=np.int32)
    offp, srcp = off.ctypes.data_as(ctypes.c_void_p), src.ctypes.data_as(ctypes.c_void_p)
    need = {w: L.icpmi_feature_align_batch_workspace_bytes(600, 2, 300, 2, 100, w) for w in (0, 1)}

    def call(pts=FAKE, off_dev=FAKE, off_host=offp, n_clouds=2, pair_src=FAKE, pair_src_host=srcp, pair_tgt=FAKE, n_pairs=2,
             voxel_size=0.2, k_curvature=10, top_n=100, k_descriptor=30, hyp_idx=None, hyp_u=FAKE, n_iter=10, init_in=FAKE,
             records=FAKE, ws=FAKE, ws_bytes=need[1]):
        return align(pts, off_dev, off_host, n_clouds, pair_src, pair_src_host, pair_tgt, n_pairs, voxel_size, k_curvature, top_n,
                     0.3, k_descriptor, 0.64, hyp_idx, hyp_u, n_iter, 0, 0.5, 3, init_in, FAKE, records, ws, ws_bytes, None)

    for kw in (dict(pts=None), dict(off_dev=None), dict(off_host=None), dict(pair_src=None), dict(pair_tgt=None), dict(records=None),
               dict(ws=None)):
        assert call(**kw) == ERR_ARG, kw
    for kw in (dict(n_clouds=0), dict(n_clouds=-1), dict(n_pairs=-1), dict(n_iter=-1), dict(k_curvature=-1), dict(k_descriptor=-1)):
        assert call(**kw) == ERR_ARG, kw
    assert call(hyp_idx=FAKE) == ERR_ARG and call(hyp_u=None) == ERR_ARG                # exactly one hypothesis table
    assert call(pair_src_host=None) == ERR_ARG                                          # a start per pair needs the host mirror
    assert call(voxel_size=0.0) == ERR_ARG and call(voxel_size=float("nan")) == ERR_ARG
    assert call(k_curvature=32) == ERR_UNSUPPORTED and call(k_descriptor=32) == ERR_UNSUPPORTED
    assert call(top_n=257) == ERR_UNSUPPORTED
    assert call(n_pairs=0) == 0                                                         # nothing to do
    assert call(n_pairs=0, n_iter=0, hyp_u=None, init_in=None, pair_src_host=None) == 0
    assert call(ws_bytes=need[1] - 1) == ERR_WORKSPACE
    assert call(init_in=None, ws_bytes=need[0] - 1) == ERR_WORKSPACE
    assert call(init_in=None, pair_src_host=None, ws_bytes=need[0] - 1) == ERR_WORKSPACE
    # two faults at once
    assert call(k_curvature=32, voxel_size=0.0) == ERR_ARG and call(top_n=257, n_iter=-1) == ERR_ARG
    assert call(k_descriptor=32, pts=None) == ERR_ARG and call(k_curvature=32, pair_src_host=None) == ERR_ARG
    assert call(n_pairs=0, pts=None) == ERR_ARG and call(n_pairs=0, voxel_size=0.0) == ERR_ARG
    assert call(n_pairs=0, k_curvature=32) == ERR_UNSUPPORTED and call(n_pairs=0, top_n=257) == ERR_UNSUPPORTED
    assert call(n_pairs=0, ws_bytes=0) == 0
    assert call(k_curvature=32, ws_bytes=0) == ERR_UNSUPPORTED
    src[:] = (0, 2)
    assert call() == ERR_ARG                                                            # a source that is no cloud of the set
    assert call(ws_bytes=need[1] - 1) == ERR_WORKSPACE                                  # the workspace is looked at first
    assert call(top_n=257) == ERR_UNSUPPORTED
    src[:] = (-1, 0)
    assert call() == ERR_ARG
    src[:] = (0, 1)
    off[:] = (0, 300, 200)
    assert call() == ERR_ARG and call(init_in=None) == ERR_ARG                          # decreasing host offsets
    assert call(ws_bytes=0) == ERR_ARG and call(n_pairs=0) == 0                         # before the workspace, after "no pairs"


def test_align_batch_workspace_bytes_against_literal_values():
    """csrc/features.hip, FtWs: every array rounded up to 256 bytes, 256 at the end.  Two clouds of 300 rows, 2 pairs, top_n
    100 (stride 104); V is the voxel scratch of a 300-row cloud, icpmi_voxel_workspace_bytes(300) rounded up to 256.
    Without a start the work set is the caller's clouds, on the caller's offsets and pair list: filtered rows 600 * 16 =
    9600 -> 9728, counts 256, curvature 4800 -> 4864, keypoints 2 * 104 * 4 = 832 -> 1024, their counts 256, descriptors
    2 * 104 * 256 = 53248, their lengths 256, matches 2 * 104 * 8 = 1664 -> 1792, their counts 256.
    With a start per pair it is 4 clouds of 1200 rows: two row arrays of 19200 each, offsets, counts and the pair list 256
    each, curvature 9600 -> 9728, keypoints 1664 -> 1792, their counts 256, descriptors 106496, their lengths 256, matches
    1792, their counts 256."""
    import icpmi
    L = icpmi.lib()
    q = L.icpmi_feature_align_batch_workspace_bytes
    V = -(-L.icpmi_voxel_workspace_bytes(300) // 256) * 256
    assert q(600, 2, 300, 2, 100, 0) == 9728 + 256 + 4864 + 1024 + 256 + 53248 + 256 + 1792 + 256 + V + 256 == 71936 + V
    assert q(600, 2, 300, 2, 100, 1) == 2 * 19200 + 3 * 256 + 9728 + 1792 + 256 + 106496 + 256 + 1792 + 256 + V + 256 == 160000 + V
    assert q(600, 2, 300, 2, 100, 7) == q(600, 2, 300, 2, 100, 1)                      # with_init is a flag
    assert q(-1, 2, 300, 2, 100, 0) == 0 and q(600, -1, 300, 2, 100, 0) == 0 and q(600, 2, -1, 2, 100, 0) == 0
    assert q(600, 2, 300, -1, 100, 1) == 0
    assert q(600, 2, 300, 2, 3, 0) == q(600, 2, 300, 2, 8, 0) == q(600, 2, 300, 2, 0, 0)   # top_n <= 0 or below 8: a stride of 8


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
