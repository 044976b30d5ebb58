"""Host side of the moments of a scan-to-map match (include/icpmi.h: icpmi_grid_match_moments; icpmi.gridmatch.half_step,
gaussian_of_moments): the entry in header, library and loader, every refusal it decides on the host — before anything is
enqueued, so no GPU is touched (the pointers are fakes that are never dereferenced) — the weight rule of the NumPy
restatement (tests/gridmoments_ref.py) against literal values, the Gaussian of hand-made moments, and on the room of
tests/gridmatch_ref.py the condition on the inputs: the weighted mean is closer to the truth than the whole-cell winner."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridmatch_ref as ref
import gridmoments_ref as mref
from conftest import REPO

FAKE = 4096                                                    # a non-null address that is never dereferenced
ERR_ARG, ERR_UNSUPPORTED = -1, -4
SLOTS = ("W", "A", "J", "I", "AA", "AJ", "AI", "JJ", "JI", "II", "SUPPORT", "EDGE")


def test_entry_and_defines_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    name = "icpmi_grid_match_moments"
    assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"\b" + name + r"\(", hdr)
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GMOM_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert len(defines) == 15                                  # 12 slots and INTS, WEIGHT_BITS, MAX_HALF_STEP
    for n, v in defines.items():
        assert getattr(_lib, n) == v, n
    assert [defines["GMOM_" + s] for s in SLOTS] == list(range(12)) and defines["GMOM_INTS"] == 12
    assert (defines["GMOM_WEIGHT_BITS"], defines["GMOM_MAX_HALF_STEP"]) == (20, 32767)
    args = lib.icpmi_grid_match_moments.argtypes
    assert len(args) == 8 and all(t is ctypes.c_int32 for t in args[2:6]) and lib.icpmi_grid_match_moments.restype is ctypes.c_int


def test_moments_refuses_bad_arguments_on_the_host():
    import icpmi
    entry = icpmi.lib().icpmi_grid_match_moments

    def call(volume=FAKE, records=FAKE, n_pairs=2, n_angles=25, window=6, half_step=1024, moments=FAKE):
        return entry(volume, records, n_pairs, n_angles, window, half_step, moments, None)

    assert call(n_pairs=0) == 0                                                # nothing to do
    assert call(n_pairs=0, volume=None, records=None, moments=None) == 0
    for kw in (dict(volume=None), dict(records=None), dict(moments=None), dict(n_pairs=-1), dict(n_angles=0), dict(n_angles=-3),
               dict(window=-1), dict(half_step=0), dict(half_step=-5), dict(half_step=32768), dict(moments=FAKE + 4),
               dict(moments=FAKE + 1)):
        assert call(**kw) == ERR_ARG, kw
    assert call(window=32) == ERR_UNSUPPORTED and call(n_angles=1025) == ERR_UNSUPPORTED
    assert call(window=255) == ERR_UNSUPPORTED and call(n_angles=16384) == ERR_UNSUPPORTED     # the wide search's capacities


def test_weight_rule_against_literal_values():
    from icpmi import gridmatch
    table = [1048576, 961548, 881744, 808563, 741455, 679917, 623487, 571740]
    assert list(mref.T) == table
    exact = 2.0 ** 20 * 2.0 ** (-np.arange(8) / 8.0)
    assert [int(v) for v in np.rint(exact)] == table
    assert np.abs(exact - np.floor(exact) - 0.5)[1:].min() > 0.05              # no entry near a tie (.43 the nearest)
    w = lambda d, h=8000, best=0: int(mref.weights(np.array([best - d]), best, h)[0])      # noqa: E731
    assert w(0) == 1048576 and w(8000) == 524288 and w(7999) == 571740 and w(16000) == 262144
    for f in range(8):
        assert w(1000 * f) == table[f], f
        if f:
            assert w(1000 * f - 1) == table[f - 1], f
    assert w(160000) == 1 and w(159999) == 571740 >> 19 == 1 and w(161000) == 0 and w(168000) == 0 and w(10 ** 9) == 0
    assert w(-1) == w(-10 ** 6) == 1048576                                     # a score above `best` counts as d = 0
    assert w(2 ** 32 - 1, 1, 2 ** 31 - 1) == 0 and w(20, 1) == 1 and w(19, 1) == 571740 >> 18 == 2 and w(21, 1) == 0 and w(2, 1) == 1048576 >> 2
    assert w(2 ** 32 - 1, 65535 * 32767, 2 ** 31 - 1) == 1048576 >> 2          # 8 d / h = 16.0000...: the largest d at the largest h
    assert mref.weights(np.array([[3, 5]], dtype=np.int32), 5, 1).dtype == np.int64
    assert gridmatch.half_step(0.25, 12) == 1024 and gridmatch.half_step(0.0625, 12) == 256 and gridmatch.half_step(7.9998, 12) == 32767
    assert gridmatch.half_step(1.0, 0) == 1
    for bad in ((0.0001, 12), (0.0, 12), (8.0, 12), (-0.25, 12), (3.0, 14)):   # 0, 0, 32 768, negative, 49 152
        with pytest.raises(ValueError, match="half_step"):
            gridmatch.half_step(*bad)


def hand_moments(cands):
    """The twelve moments of [(w, da, dj, di), ...], no candidate on a face."""
    m = np.zeros(12, dtype=np.int64)
    for w, da, dj, di in cands:
        m += np.array([w, w * da, w * dj, w * di, w * da * da, w * da * dj, w * da * di, w * dj * dj, w * dj * di, w * di * di, w > 0, 0])
    return m


def test_gaussian_of_hand_made_moments():
    from icpmi.gridmatch import gaussian_of_moments
    res, step = 0.1, np.deg2rad(1.0)
    one = 1 << 20
    M = np.stack([hand_moments([(one, 0, 0, 0)]),                              # one candidate: the winner itself
                  hand_moments([(one, 0, 0, 0), (one, 0, 0, 1)]),              # two equal weights one cell apart in i
                  np.zeros(12, dtype=np.int64),                                # no weight at all (CAPACITY)
                  hand_moments([(one, 0, 0, 0), (one >> 1, 1, 0, 0), (one >> 1, -1, 2, 0), (3, 0, -1, 1)])])
    M[3, 11] = M[3, 0] // 4
    g = gaussian_of_moments(M, res, step)
    assert g["offset"].shape == (4, 3) and g["covariance"].shape == (4, 3, 3) and g["support"].dtype == np.int64
    assert list(g["support"]) == [1, 2, 0, 4]
    assert np.array_equal(g["offset"][0], [0.0, 0.0, 0.0])
    assert np.array_equal(g["covariance"][0], np.diag([res * res * (1.0 / 12.0), res * res * (1.0 / 12.0), step * step * (1.0 / 12.0)]))
    assert np.array_equal(g["offset"][1], [res * 0.5, 0.0, 0.0])
    assert g["covariance"][1, 0, 0] == (res * res) * (0.25 + 1.0 / 12.0) and g["covariance"][1, 1, 1] == res * res * (1.0 / 12.0)
    assert not g["covariance"][1][~np.eye(3, dtype=bool)].any()
    assert np.isnan(g["offset"][2]).all() and np.isnan(g["covariance"][2]).all() and np.isnan(g["edge_weight"][2])
    assert g["edge_weight"][0] == 0.0 and g["edge_weight"][3] == float(M[3, 0] // 4) / float(M[3, 0])
    # the general pair against float64 moments formed directly: mean and covariance of the weighted candidates
    c = np.array([(one, 0, 0, 0), (one >> 1, 1, 0, 0), (one >> 1, -1, 2, 0), (3, 0, -1, 1)], dtype=np.float64)
    p, X = c[:, 0] / c[:, 0].sum(), c[:, [3, 2, 1]] * np.array([res, res, step])
    mu = p @ X
    want = (X - mu).T @ np.diag(p) @ (X - mu) + np.diag([res * res / 12.0, res * res / 12.0, step * step / 12.0])
    assert np.allclose(g["offset"][3], mu, rtol=1e-13, atol=0.0) and np.allclose(g["covariance"][3], want, rtol=1e-12, atol=1e-22)
    assert g["covariance"][3, 0, 1] != 0.0 and g["covariance"][3, 1, 2] != 0.0
    for b in (0, 1, 3):
        assert np.array_equal(g["covariance"][b], g["covariance"][b].T)        # symmetric bit for bit
        assert np.linalg.eigvalsh(g["covariance"][b]).min() > 0.0
    # one angle: no step, so the theta row and column and the theta offset are zero; a step per pair is taken per pair
    g1 = gaussian_of_moments(M[[0, 1, 3]], res, 0.0)
    assert not g1["covariance"][:, 2, :].any() and not g1["covariance"][:, :, 2].any() and not g1["offset"][:, 2].any()
    assert np.array_equal(g1["covariance"][:, :2, :2], g["covariance"][[0, 1, 3], :2, :2])
    g2 = gaussian_of_moments(M[[3, 3]], res, np.array([step, 2.0 * step]))
    assert np.array_equal(g2["covariance"][0], g["covariance"][3]) and np.array_equal(g2["covariance"][1, :2, :2], g["covariance"][3, :2, :2])
    assert g2["covariance"][1, 2, 2] == 4.0 * g["covariance"][3, 2, 2] and g2["covariance"][1, 0, 2] == 2.0 * g["covariance"][3, 0, 2]
    assert g2["offset"][1, 2] == 2.0 * g["offset"][3, 2]
    # moments as large as the capacities allow (1 024 angles x 63^2 shifts of weight 2^20 about index 0): the numerators are
    # Python integers, M_AA M_W alone is 6e30; the mean of a^2 over 0 ... 1023 is 349 013.5, the mean of a 511.5
    n = 1024 * 3969
    big = np.array([[n * one, 3969 * 523776 * one, 0, 0, 1487384306207686656, 0, 0, 3, 0, 5, n, 0]], dtype=np.int64)
    gb = gaussian_of_moments(big, 1.0, 1.0)
    assert gb["offset"][0, 2] == 511.5 and abs(gb["covariance"][0, 2, 2] - (349013.5 - 511.5 ** 2 + 1.0 / 12.0)) < 1e-9


def test_refined_pose_beats_the_winner_in_the_room():
    """The map, the 12 queries and the search of tests/test_grid_match_cpu.py (W = 6, 25 angles), half_log_odds = 0.25: per
    component the RMS error of the weighted mean over the 12 queries is below the whole-cell winner's, and every covariance
    is positive definite.  Measured when this was written: winner 0.0525 m, 0.0348 m, 0.264 deg; refined 0.0305 m, 0.0121 m,
    0.146 deg; 256 to 462 candidates with a weight; smallest eigenvalue of an index-unit covariance (the 1/12 included) 0.12."""
    import oracle
    from icpmi.gridmatch import gaussian_of_moments, half_step
    g = ref.SCENE
    lo = np.zeros((200, 280), dtype=np.float32)
    l_hit, l_miss = float(np.log(0.7 / 0.3)), float(np.log(0.4 / 0.6))
    for o, h in zip(*ref.scene_scans()):
        oracle.grid_update_scan(lo, g["min_x"], g["min_y"], 0.1, o, h, l_hit, l_miss, -5.0, 5.0)
    k = ref.shift_bits(-5.0, 5.0)
    q = ref.quantise(lo, k)
    hs = half_step(0.25, k)
    assert (k, hs) == (12, 1024)
    W, step = 6, np.deg2rad(1.0)
    err_win, err_ref, support, eig = [], [], [], []
    for true, pred, scan in ref.scene_queries():
        angles = ref.angle_rows(pred[2])
        cs = ref.cos_sin_of(angles)
        vol, rows = ref.volume(q, scan, pred[:2], cs, W, g["min_x"], g["min_y"], 0.1)
        rec = ref.record(vol, rows, 12, W)
        _, t = ref.pose(rec, pred[:2], cs, W, 0.1)
        m = mref.moments(vol, rec, hs)
        gm = gaussian_of_moments(m[None], 0.1, step)
        win = np.array([t[0], t[1], angles[rec[3]]])
        err_win.append(win - np.array(true))
        err_ref.append(win + gm["offset"][0] - np.array(true))
        support.append(int(gm["support"][0]))
        unit = gaussian_of_moments(m[None], 1.0, 1.0)["covariance"][0]
        eig.append(float(np.linalg.eigvalsh(unit).min()))
        assert np.linalg.eigvalsh(gm["covariance"][0]).min() > 0.0 and eig[-1] > 0.0
        assert m[0] >= 1 << 20 and 1 <= m[10] <= 25 * 169 and 0 <= m[11] <= m[0]
        print(f"true {true}: winner off {err_win[-1]}, refined off {err_ref[-1]}, support {support[-1]}, edge {gm['edge_weight'][0]:.4f}, "
              f"smallest index-unit eigenvalue {eig[-1]:.4f}")
    unit = np.array([1.0, 1.0, np.rad2deg(1.0)])
    rms_win, rms_ref = np.sqrt(np.mean(np.square(err_win), axis=0)) * unit, np.sqrt(np.mean(np.square(err_ref), axis=0)) * unit
    print("rms winner", rms_win, "rms refined", rms_ref, "support", min(support), max(support), "smallest eigenvalue", min(eig))
    assert (rms_ref < rms_win).all(), (rms_ref, rms_win)
