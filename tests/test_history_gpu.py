"""The resident scan history (icpmi.history.ScanHistory, include/icpmi.h icpmi_history_*) against the batch path it
replaces: ``RunIcpPairBatch([src] + targets, ...)`` on the same arrays.  The same kernels run on the same filtered rows, and a
target's search order never changes a result, so the ICP result records and the search records must agree BIT FOR BIT
(a gated run: up to the accepted candidate; behind it a record is the full run's or SKIPPED, as tests/test_first_accepted.py
has it).

Scans of 256, 360 and 512 beams, mixed: unequal clouds are what exposes a wrong offset or capacity."""
import numpy as np
import pytest

from conftest import rot_err

pytestmark = pytest.mark.gpu

VOXEL, NORMAL_K, RS_VOXEL = 0.04, 12, 0.15
RUN = dict(error_threshold=1e-10, max_iterations=60, angle_step_coarse=2.0, angle_step_fine=0.2)
BEAMS = (256, 360, 512, 360, 512, 256, 512, 256, 360, 256, 512, 360)
CANDS = [7, 2, 9, 2, 0, 5]                     # unordered, not contiguous, one repeated


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import features
    features.VERBOSE = False


@pytest.fixture(scope="module")
def scans():
    from icpmi import synth
    poses = synth.trajectory(len(BEAMS), start=(-8.0, -0.5, 0.0), step=0.3)          # along the room, clear of its boxes
    return [synth.scan(p, 4100 + i, n_beams=b) for i, (p, b) in enumerate(zip(poses, BEAMS))]


def new_history(**kw):
    from icpmi import ScanHistory
    return ScanHistory(voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, **kw)


@pytest.fixture(scope="module")
def history(gpu, scans):
    h = new_history()
    assert h.add_many(scans) == list(range(len(scans))) and len(h) == len(scans)
    return h


def device_records(b):
    """(ICP result records, search records) of a RunIcpPairBatch / HistoryMatch after run(), as the device wrote them."""
    return b.icp.results.cpu().numpy()[:b.B].copy(), b.search.records.cpu().numpy()[:b.B].copy()


def batch_path(src, tgts, method="point_to_line", **kw):
    """The yardstick: the existing batch path on the same arrays -> (ICP records, search records, the batch)."""
    from icpmi import prealign
    B = len(tgts)
    b = prealign.RunIcpPairBatch([src] + list(tgts), np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32),
                                 voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, method=method, **RUN, **kw)
    b.run()
    return device_records(b) + (b,)


def resident(h, source, cands, method="point_to_line", **kw):
    m = h.match(source, cands, method=method, **RUN, **kw)
    m.run()
    return device_records(m) + (m,)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0], equal_nan=True), f"ICP records differ {what}"
    assert np.array_equal(got[1], want[1], equal_nan=True), f"search records differ {what}"


@pytest.fixture(scope="module")
def reference_p2l(gpu, scans):
    """The batch path's records of scan 11 against CANDS, computed once."""
    res, rec, _ = batch_path(scans[11], [scans[k] for k in CANDS])
    assert (rec[:, 11] == 0).all() and (res[:, 15] != 5).all()
    return res, rec


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
def test_match_by_id_equals_the_batch_path(history, scans, reference_p2l, method):
    want = reference_p2l if method == "point_to_line" else batch_path(scans[11], [scans[k] for k in CANDS], method)[:2]
    got = resident(history, 11, CANDS, method)
    assert_same(got, want, method)
    R, t, err, info = got[2].unpack()
    assert np.array_equal(err, want[0][:, 12]) and np.array_equal(info["iters"], want[0][:, 14].astype(np.int64))
    assert np.array_equal(got[0][1], got[0][3]) and np.array_equal(got[1][1], got[1][3])       # the repeated candidate


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
def test_match_with_a_source_that_is_not_in_the_history(history, scans, method):
    from icpmi import synth
    src = synth.scan((-6.0, 0.3, 0.4), 977, n_beams=300)
    n, rows = len(history), history.rows_used
    want = batch_path(src, [scans[k] for k in CANDS], method)[:2]
    got = resident(history, src, CANDS, method)
    assert_same(got, want, method)
    assert len(history) == n and history.rows_used == rows                                      # staged, not added
    # the next match by id is not disturbed by the staged rows, and the staged match refuses to run once they are gone
    m2 = history.match(src[::2], CANDS[:2], **RUN)
    with pytest.raises(Exception, match="overwritten"):
        got[2].run()
    m2.run()


def test_scans_added_in_two_calls(gpu, scans, history, reference_p2l):
    """Three scans, a match, then the rest: the final state equals the history built by one add_many, and the first match,
    run again after the second add, still gives what it gave — a later add leaves earlier prepared state alone."""
    h = new_history()
    assert h.add_many(scans[:3]) == [0, 1, 2]
    first = resident(h, 2, [0, 1, 0])
    assert_same(first, batch_path(scans[2], [scans[0], scans[1], scans[0]])[:2], "before the second add")
    assert h.add_many(scans[3:]) == list(range(3, len(scans)))
    again = first[2]
    again.run()
    assert_same(device_records(again), first, "after the second add")
    assert_same(resident(h, 11, CANDS), reference_p2l, "two adds")
    assert np.array_equal(h.counts(), history.counts()) and np.array_equal(h.search_counts(), history.search_counts())


def test_growth_leaves_results_alone(gpu, scans, history, reference_p2l):
    """scan_capacity 4 and a row capacity the fifth scan exceeds: both double, more than once, and nothing changes."""
    rows4 = sum(len(s) for s in scans[:4])
    h = new_history(scan_capacity=4, row_capacity=rows4 + 100)
    assert len(scans[4]) > 100
    for s in scans[:4]:
        h.add(s)
    assert (h.scan_capacity, h.row_capacity) == (4, rows4 + 100)
    before = resident(h, 3, [0, 2, 1])
    h.add(scans[4])
    assert h.scan_capacity == 8 and h.row_capacity == 2 * (rows4 + 100)
    with pytest.raises(Exception, match="grown"):
        before[2].run()
    assert_same(resident(h, 3, [0, 2, 1]), before, "after growing")
    for s in scans[5:]:
        h.add(s)
    assert h.scan_capacity == 16 and h.row_capacity >= sum(len(s) for s in scans)
    assert_same(resident(h, 11, CANDS), reference_p2l, "grown")
    assert np.array_equal(h.counts(), history.counts()) and np.array_equal(h.search_counts(), history.search_counts())
    src = scans[5][::2]                                       # a staged source may grow it too
    h2 = new_history(scan_capacity=2, row_capacity=len(scans[0]) + len(scans[1]))
    h2.add_many(scans[:2])
    assert_same(resident(h2, src, [1, 0]), batch_path(src, [scans[1], scans[0]])[:2], "staged source, grown")


def test_stop_after_first_accepted(history, scans):
    """A far candidate first: it is rejected before a later one is accepted.  first_accepted() and every record up to the
    accepted candidate equal the gated batch path; a gate nothing passes returns -1."""
    cands = [0, 10, 5, 9, 3, 8]                               # scan 0 is 3.3 m from scan 11, scan 10 its neighbour
    err = batch_path(scans[11], [scans[k] for k in cands])[0][:, 12]
    worst = int(np.argmax(err))                               # (by the batch path's own errors: the far one, in front)
    cands = [cands[worst]] + cands[:worst] + cands[worst + 1:]
    tgts = [scans[k] for k in cands]
    full, _, _ = batch_path(scans[11], tgts)
    err = full[:, 12]
    gate = float(np.sqrt(err[0] * err[1:].min()))             # between the far candidate's error and the best one's
    assert err[0] > gate > err[1:].min(), err
    F = int(np.flatnonzero(err < gate)[0])
    assert F >= 1
    wres, wrec, wb = batch_path(scans[11], tgts, error_accept=gate, stop_after_first_accepted=True)
    gres, grec, gm = resident(history, 11, cands, error_accept=gate, stop_after_first_accepted=True)
    assert wb.first_accepted() == F and gm.first_accepted() == F
    assert np.array_equal(grec, wrec, equal_nan=True)
    assert np.array_equal(gres[:F + 1], full[:F + 1], equal_nan=True) and np.array_equal(wres[:F + 1], full[:F + 1], equal_nan=True)
    for i in range(F + 1, len(cands)):
        if gres[i, 15] != 5:
            assert np.array_equal(gres[i], full[i], equal_nan=True), i
    assert gm.unpack()[3]["first_accepted"] == F
    none = history.match(11, cands, error_accept=float(err.min()) * 0.5, stop_after_first_accepted=True, **RUN)
    none.run()
    assert none.first_accepted() == -1
    assert np.array_equal(none.icp.results.cpu().numpy()[:len(cands)], full, equal_nan=True)    # nothing accepted: nothing skipped


def test_1100_pairs_take_the_two_stage_launch(gpu):
    """At least 1024 point_to_line pairs run in two stages (csrc/icp2.hip): 1100 pairs cycling over the history's targets."""
    from icpmi import synth
    poses = synth.trajectory(12, start=(-8.0, -0.5, 0.0), step=0.3)
    small = [synth.scan(p, 4300 + i, n_beams=256) for i, p in enumerate(poses)]
    h = new_history()
    h.add_many(small)
    cands = (np.arange(1100) * 7) % 11
    want = batch_path(small[11], [small[k] for k in cands])[:2]
    got = resident(h, 11, cands)
    assert_same(got, want, "1100 pairs")
    assert len(np.unique(want[0][:, 14])) > 1


def test_the_reference_pairs_through_the_history(gpu):
    """tests/golden/run_icp_pair.npz — the reference's own _run_icp_pair results (slam.py:53-98) — held to the fixture as
    tests/test_gpu_parity.py::test_run_icp_pair_equals_the_reference holds the batch path: equal iterations, FRO_TOL of that
    file, its error bound."""
    from icpmi import ScanHistory
    from test_gpu_parity import FRO_TOL
    from test_oracle_golden import run_icp_pair_cases
    cases = list(run_icp_pair_cases())
    icp_cfg, feat_cfg = cases[0][4], cases[0][5]
    h = ScanHistory(voxel_size=icp_cfg["voxel_size"], normal_k=icp_cfg["normal_k"], rotation_voxel_size=feat_cfg["rotation_voxel_size"],
                    scan_capacity=4, row_capacity=4096)                        # (and it grows on the way)
    ids = h.add_many([cases[0][1]] + [c[2] for c in cases])
    m = h.match(ids[0], ids[1:], error_threshold=icp_cfg["error_threshold"], max_iterations=icp_cfg["max_iterations"],
                method=icp_cfg["method"], angle_step_coarse=feat_cfg["angle_step_coarse"], angle_step_fine=feat_cfg["angle_step_fine"])
    m.run()
    R, t, err, info = m.unpack()
    for q, (i, s, tg, z, _, _) in enumerate(cases):
        assert int(info["iters"][q]) == int(z[f"p{i}__iters"]), i
        assert rot_err(R[q], t[q], z[f"p{i}__R"], z[f"p{i}__t"]) < FRO_TOL, i
        assert abs(err[q] - float(z[f"p{i}__err"])) <= 1e-9 * max(1.0, err[q]), i


def test_nothing_is_filtered_again(gpu, scans, reference_p2l):
    """After add, the raw rows of the candidates are overwritten on the device with another scan's (valid) points: a match
    that read them again would give that scan's records."""
    import torch
    h = new_history()
    h.add_many(scans)
    off = h.raw.off_host
    for k in set(CANDS):
        n = int(off[k + 1] - off[k])
        other = next(s for j, s in enumerate(scans) if j != k and j != 11 and len(s) >= n)
        h.raw.pts[int(off[k]):int(off[k + 1])].copy_(torch.from_numpy(np.ascontiguousarray(other[:n])))
    assert_same(resident(h, 11, CANDS), reference_p2l, "raw rows overwritten")


def test_refusals(history, scans):
    n = len(history)
    big = np.random.default_rng(0).normal(size=(4097, 2))
    with pytest.raises(ValueError, match="4096"):
        history.add(big)
    with pytest.raises(ValueError, match="4096"):
        history.match(big, [0])
    with pytest.raises(ValueError, match="RunIcpPairBatch"):
        history.match(11, [0], alignment_method="features")
    with pytest.raises(ValueError, match="RunIcpPairBatch"):
        history.match(11, [0], alignment_method="both")
    for bad in ([n], [0, n + 5], [-1]):
        with pytest.raises(ValueError, match="candidate ids"):
            history.match(11, bad)
    with pytest.raises(ValueError, match="source id"):
        history.match(n, [0])
    with pytest.raises(ValueError):
        history.match(11, [0], stop_after_first_accepted=True)
    from icpmi import ScanHistory
    with pytest.raises(ValueError, match="point_to_point"):
        h = ScanHistory(voxel_size=VOXEL, normal_k=None, rotation_voxel_size=RS_VOXEL, scan_capacity=4)
        h.add_many(scans[:2])
        h.match(1, [0])
    assert len(history) == n


def test_point_to_point_history(gpu, scans):
    """normal_k=None: no normals are computed; point_to_point matches equal the batch path."""
    from icpmi import ScanHistory
    h = ScanHistory(voxel_size=VOXEL, normal_k=None, rotation_voxel_size=RS_VOXEL, scan_capacity=4)
    h.add_many(scans[:4])
    want = batch_path(scans[3], [scans[1], scans[0]], "point_to_point")[:2]
    assert_same(resident(h, 3, [1, 0], "point_to_point"), want)


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
def test_icp_of_two_resident_scans_equals_icp_pair(history, scans, method):
    """The scan-to-scan step (slam.py:471) against the resident prepared target, with and without a start."""
    from icpmi.batch import icp_pair
    th = np.deg2rad(3.0)
    R0, t0 = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), np.array([0.25, -0.05])
    for s, t, init in ((4, 3, (None, None)), (6, 5, (R0, t0)), (1, 2, (R0, None))):
        want = icp_pair(scans[s], scans[t], 1e-10, 60, VOXEL, init[0], init[1], method, NORMAL_K, None)
        got = history.icp(s, t, init[0], init[1], error_threshold=1e-10, max_iterations=60, method=method)
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a, b, equal_nan=True), (method, s, t)
        for key in ("iters", "status", "delta"):
            assert np.array_equal(got[3][key], want[3][key], equal_nan=True), (method, key)
    with pytest.raises(ValueError, match="scan ids"):
        history.icp(0, len(history))
