"""Resident feature alignment (``ScanHistory(..., feat_cfg=...)``, ``match(alignment_method="features" / "both")``;
include/icpmi.h icpmi_history_features_add / icpmi_history_feature_align) against the batch path it replaces:
``RunIcpPairBatch([src] + targets, alignment_method=..., hypotheses=...)`` on the same arrays.  The same kernels run on the
same filtered rows, so the ICP result records, the feature records (all 16 slots) and — for "both" — the search records
must agree BIT FOR BIT; nothing weaker than ``np.array_equal`` is accepted.

Every equality test first requires of the yardstick that at least half of its pairs were aligned (status 0 with at least
``min_inliers`` inliers) and that the pre-alignment moved their start: a batch in which every pair returns early would pass
vacuously.

Inputs: the pairs of tests/golden/features.npz (1024-row scans around one pose) and synthetic scans of 256, 360 and 512
beams — unequal clouds are what exposes a wrong offset or capacity."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOXEL, NORMAL_K, RS_VOXEL = 0.06, 10, 0.3                      # the reference's defaults: the fixture's pairs align at them
RUN = dict(error_threshold=1e-7, max_iterations=100, angle_step_coarse=2.0, angle_step_fine=0.2)
N_ITER = 400
PAIR_CFG = dict(ransac_iterations=N_ITER)                      # a pair-side key: given per match
MIN_INLIERS = 3                                                # FEAT_DEFAULTS
SRC = 2                                                        # the source scan of the matches by id
CANDS = [3, 6, 0, 3, 4, 7, 1]                                  # unordered, not contiguous, one repeated, three sizes
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from conftest import load_golden
    from utilities import features
    features.VERBOSE = False
    return load_golden("features")


@pytest.fixture(scope="module")
def scans(g):
    from icpmi import synth
    syn = [synth.scan((0.5 + 0.3 * i, -0.3, 0.1 + 0.1 * i), 5200 + i, n_beams=b) for i, b in enumerate((256, 512, 360))]
    return [g["p0_raw_t"], g["p1_raw_t"], g["p0_raw_s"], g["p2_raw_t"], g["p3_raw_t"]] + syn + [g["p3_raw_s"]]


@pytest.fixture(scope="module")
def staged_source():
    from icpmi import synth
    return synth.scan((0.4, -0.2, 0.3), 977, n_beams=300)


def new_history(feat_cfg={}, **kw):
    from icpmi import ScanHistory
    return ScanHistory(voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, feat_cfg=feat_cfg, **kw)


@pytest.fixture(scope="module")
def history(scans):
    h = new_history()
    assert h.add_many(scans) == list(range(len(scans)))
    return h


def hypotheses(kind):
    """An explicit table of match-index pairs (rows with two equal indices or an index the pair does not have count no
    inliers), or a generator seeded the same for both paths."""
    if kind == "table":
        return dict(hypotheses=np.random.default_rng(21).integers(0, 16, size=(N_ITER, 2)))
    return dict(rng=np.random.default_rng(5))


def device_records(b):
    """What the device wrote: ICP result records, feature records, search records (None without a search), the ICP's starts."""
    B = b.B
    return (b.icp.results.cpu().numpy()[:B].copy(), b.features.records.cpu().numpy()[:B].copy(),
            b.search.records.cpu().numpy()[:B].copy() if b.search is not None else None, b.icp.init.cpu().numpy()[:B].copy())


def batch_path(src, tgts, method, hyp, **kw):
    """The yardstick: the existing batch path on the same arrays."""
    from icpmi import prealign
    B = len(tgts)
    b = prealign.RunIcpPairBatch([src] + list(tgts), np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32),
                                 voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, alignment_method=method,
                                 feat_cfg=PAIR_CFG, **RUN, **hyp, **kw)
    b.run()
    return device_records(b) + (b,)


def search_starts(src, tgts):
    """The starts the rotation search alone leaves: what "both" hands to the feature alignment."""
    from icpmi import prealign
    B = len(tgts)
    b = prealign.RunIcpPairBatch([src] + list(tgts), np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32),
                                 voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, **RUN)
    b.search.run()
    return b.icp.init.cpu().numpy()[:B].copy()


def resident(h, source, cands, method, hyp, **kw):
    m = h.match(source, cands, alignment_method=method, feat_cfg=PAIR_CFG, **RUN, **hyp, **kw)
    m.run()
    return device_records(m) + (m,)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0], equal_nan=True), f"ICP records differ {what}"
    assert np.array_equal(got[1], want[1], equal_nan=True), f"feature records differ {what}"
    assert (got[2] is None) == (want[2] is None)
    if want[2] is not None:
        assert np.array_equal(got[2], want[2], equal_nan=True), f"search records differ {what}"
    assert np.array_equal(got[3], want[3], equal_nan=True), f"starts differ {what}"


def assert_not_vacuous(want, before, what=""):
    """The yardstick's feature records: at least half of the pairs aligned, and their start moved from ``before``."""
    rec, init = want[1], want[3]
    good = (rec[:, 12] == 0) & (rec[:, 5] >= MIN_INLIERS)
    print(what, "status", rec[:, 12].astype(int), "inliers", rec[:, 5].astype(int))
    assert 2 * int(good.sum()) >= len(rec), (what, rec[:, 12], rec[:, 5])
    moved = (init != np.broadcast_to(before, init.shape)).any(axis=1)
    assert moved[good].all(), what


@pytest.fixture(scope="module")
def yardstick(scans, staged_source):
    """Yardstick records computed once per (method, source kind, hypothesis kind), checked not to be vacuous."""
    cache = {}

    def get(method, staged, kind):
        key = (method, staged, kind)
        if key not in cache:
            src = staged_source if staged else scans[SRC]
            tgts = [scans[k] for k in CANDS]
            want = batch_path(src, tgts, method, hypotheses(kind))[:4]
            if ("starts", staged) not in cache:
                cache[("starts", staged)] = search_starts(src, tgts)
            assert_not_vacuous(want, cache[("starts", staged)] if method == "both" else IDENTITY, str(key))
            cache[key] = want
        return cache[key]
    return get


@pytest.mark.parametrize("staged", [False, True], ids=["by_id", "staged"])
@pytest.mark.parametrize("method", ["features", "both"])
def test_match_equals_the_batch_path(history, staged_source, yardstick, method, staged):
    n, rows = len(history), history.rows_used
    for kind in ("table", "rng"):
        want = yardstick(method, staged, kind)
        got = resident(history, staged_source if staged else SRC, CANDS, method, hypotheses(kind))
        assert_same(got, want, f"{method} {kind}")
        assert np.array_equal(got[0][0], got[0][3]) and np.array_equal(got[1][0], got[1][3])        # the repeated candidate
        R, t, err, info = got[4].unpack()
        assert np.array_equal(info["feature_records"], want[1]) and np.array_equal(err, want[0][:, 12])
    assert len(history) == n and history.rows_used == rows                                          # staged, not added


@pytest.mark.parametrize("method", ["features", "both"])
def test_statuses_inside_a_healthy_batch(g, method):
    """A scan of 8 points (status 1), 2 600 scattered points that the 0.2 m filter keeps apart (status 2: above the 2 048 rows
    held on chip) and 60 rows of a scan (status 5: descriptors shorter than k_descriptor), between two regular targets: the
    same statuses as the batch path, their starts left as they were, the regular pairs unharmed.  The first scan is added
    on its own, so the scan above 2 048 rows makes the history put it in search order again — which must leave the feature
    store alone."""
    big = np.random.default_rng(2).uniform(-30.0, 30.0, size=(2600, 2))
    clouds = [g["p0_raw_t"], g["p3_raw_t"][:8], big, g["p1_raw_t"][:60], g["p1_raw_t"]]
    src = g["p0_raw_s"]
    h = new_history(scan_capacity=8)
    h.add(clouds[0])
    h.add_many(clouds[1:])
    assert not h.allow_polar
    cands = [0, 1, 2, 3, 4]
    hyp = hypotheses("rng")
    want = batch_path(src, clouds, method, hypotheses("rng"))[:4]
    status = want[1][:, 12].astype(int).tolist()
    print(method, "status", status, "filtered rows", want[1][:, 1], "inliers", want[1][:, 5])
    assert status == [0, 1, 2, 5, 0]
    before = search_starts(src, clouds) if method == "both" else np.tile(IDENTITY, (5, 1))
    assert_not_vacuous((want[0][[0, 4]], want[1][[0, 4]], None, want[3][[0, 4]]), before[[0, 4]], method)
    got = resident(h, src, cands, method, hyp)
    assert_same(got, want, method)
    assert got[1][:, 12].astype(int).tolist() == [0, 1, 2, 5, 0]
    for q in (1, 2, 3):
        assert np.array_equal(got[3][q], before[q]), q                                              # init left as it was
        assert np.array_equal(got[1][q, 5:12], [0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]), q              # 0 inliers, identity, zeros
    rows, kps = h.feature_counts()
    assert rows[2] > 2048 and kps[2] == 0 and rows[1] < 10 and 10 <= rows[3] < 31


def test_scans_added_in_two_calls(scans, history, yardstick):
    """Three scans, a match, then the rest: the first match, run again after the second add, still gives what it gave, and
    the final state equals the history built by one add_many."""
    hyp = lambda: hypotheses("table")    # noqa: E731
    h = new_history()
    assert h.add_many(scans[:3]) == [0, 1, 2]
    for method in ("features", "both"):
        first = resident(h, SRC, [1, 0, 1], method, hyp())
        assert_same(first, batch_path(scans[SRC], [scans[1], scans[0], scans[1]], method, hyp())[:4], f"{method} before the second add")
        if method == "features":
            kept = first
    assert h.add_many(scans[3:]) == list(range(3, len(scans)))
    again = kept[4]
    again.run()
    assert_same(device_records(again), kept, "after the second add")
    for method in ("features", "both"):
        assert_same(resident(h, SRC, CANDS, method, hyp()), yardstick(method, False, "table"), f"{method}, two adds")
    for a, b in zip(h.feature_counts(), history.feature_counts()):
        assert np.array_equal(a, b)


def test_growth_leaves_results_alone(scans, history, yardstick):
    """scan_capacity 2 and a row capacity the second scan exceeds: both double, more than once, and nothing changes."""
    hyp = lambda: hypotheses("table")    # noqa: E731
    h = new_history(scan_capacity=2, row_capacity=1500)
    h.add(scans[0]); h.add(scans[1])
    assert (h.scan_capacity, h.row_capacity) == (2, 3000)
    before = {m: resident(h, scans[SRC], [1, 0], m, hyp()) for m in ("features", "both")}           # the staged source grows it
    assert h.scan_capacity == 4 and h.row_capacity == 6000
    for m in ("features", "both"):
        assert_same(before[m], batch_path(scans[SRC], [scans[1], scans[0]], m, hyp())[:4], f"{m}, staged source, grown")
    for s in scans[2:]:
        h.add(s)
    assert h.scan_capacity == 16 and h.row_capacity >= sum(len(s) for s in scans)
    with pytest.raises(Exception, match="grown"):
        before["features"][4].run()
    for m in ("features", "both"):
        assert_same(resident(h, scans[SRC], [1, 0], m, hyp()), before[m], f"{m}, after growing")
        assert_same(resident(h, SRC, CANDS, m, hyp()), yardstick(m, False, "table"), f"{m}, grown")
    for a, b in zip(h.feature_counts(), history.feature_counts()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("method", ["features", "both"])
def test_stop_after_first_accepted(history, scans, yardstick, method):
    """The worst candidate first: it is rejected before a later one is accepted.  first_accepted() equals the full run's
    and the gated batch path's, and every record up to the accepted candidate equals the full run."""
    err = yardstick(method, False, "table")[0][:, 12]
    worst = int(np.argmax(err))
    cands = [CANDS[worst]] + CANDS[:worst] + CANDS[worst + 1:]
    tgts = [scans[k] for k in cands]
    full = batch_path(scans[SRC], tgts, method, hypotheses("table"))
    assert_not_vacuous(full, search_starts(scans[SRC], tgts) if method == "both" else IDENTITY, method)
    err = full[0][:, 12]
    gate = float(np.sqrt(err[0] * err[1:].min()))              # between the worst candidate's error and the best one's
    assert err[0] > gate > err[1:].min(), err
    F = int(np.flatnonzero(err < gate)[0])
    assert F >= 1
    gated = dict(error_accept=gate, stop_after_first_accepted=True)
    want = batch_path(scans[SRC], tgts, method, hypotheses("table"), **gated)
    got = resident(history, SRC, cands, method, hypotheses("table"), **gated)
    assert want[4].first_accepted() == F and got[4].first_accepted() == F
    assert np.array_equal(got[1], full[1], equal_nan=True)
    if method == "both":
        assert np.array_equal(got[2], full[2], equal_nan=True)
    assert np.array_equal(got[0][:F + 1], full[0][:F + 1], equal_nan=True)
    for i in range(F + 1, len(cands)):
        if got[0][i, 15] != 5:
            assert np.array_equal(got[0][i], full[0][i], equal_nan=True), i
    assert got[4].unpack()[3]["first_accepted"] == F
    ungated = resident(history, SRC, cands, method, hypotheses("table"), error_accept=gate)
    assert_same(ungated, full, "a gate without the early stop")
    assert ungated[4].unpack()[3]["first_accepted"] == F


def test_end_to_end_pairs_through_a_history(g):
    """The eight pairs with yaw up to 180 degrees that the reference's ICP registers only from its feature start: targets
    added, sources staged, the reference's own draws as hypotheses.  As many must end below the 0.08 gate as in the
    reference — all eight."""
    n = int(g["e2e_count"])
    assert n == 8 and int((g["e2e_err_feat"] < 0.08).sum()) == 8
    h = new_history(scan_capacity=8)
    ids = h.add_many([g["e2e_tgt"][i] for i in range(n)])
    errs = []
    for i in range(n):
        m = h.match(g["e2e_src"][i], [ids[i]], alignment_method="features", hypotheses=g["e2e_draws"][i], **RUN)
        m.run()
        _, _, err, info = m.unpack()
        errs.append(float(err[0]))
        print(i, "error", errs[-1], "reference", float(g["e2e_err_feat"][i]), "matches / inliers", info["feature_records"][0, 4:6])
    assert np.isfinite(errs).all()
    assert sum(e < 0.08 for e in errs) >= 8


def test_refusals(g, history):
    from icpmi import ScanHistory
    plain = ScanHistory(voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, scan_capacity=4)
    plain.add_many([g["p0_raw_t"], g["p0_raw_s"]])
    for method in ("features", "both"):
        with pytest.raises(ValueError, match="RunIcpPairBatch"):
            plain.match(1, [0], alignment_method=method)
    with pytest.raises(ValueError, match="no features"):
        plain.feature_counts()
    for key, value in (("voxel_size", 0.25), ("k_curvature", 8), ("top_n", 50), ("min_kp_dist", 0.2), ("k_descriptor", 20)):
        with pytest.raises(ValueError, match=key):
            history.match(SRC, [0], alignment_method="features", feat_cfg={key: value})
    history.match(SRC, [0], alignment_method="features", feat_cfg=dict(top_n=100, voxel_size=0.2, min_inliers=5))   # equal: accepted
    with pytest.raises(ValueError, match="alignment_method"):
        history.match(SRC, [0], alignment_method="ransac")
    with pytest.raises(ValueError, match="hypotheses"):
        history.match(SRC, [0], alignment_method="features", hypotheses=np.zeros((7, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        ScanHistory(feat_cfg=dict(k_descriptor=32))
    with pytest.raises(ValueError):
        ScanHistory(feat_cfg=dict(top_n=257))
