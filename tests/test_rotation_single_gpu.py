"""The single-pair rotation search (icpmi_rotation_search) and its translation refinement (icpmi_rotation_refine) on the
device, at the edges tests/rotsingle_cases.py lists; that every case has its property is tests/test_rotation_single_cpu.py's
matter.

The refinement is called on a head written by hand, with a record of which only K, NF and J matter: all four outputs equal
the NumPy restatement bit for bit.  The search's K, NF and J are those its tables were built to give (np.argmin: the first
minimum, the first NaN), its scores are those of the stand-alone scoring entry bit for bit (one loop) and the oracle's to
the bound of test_rotation_scores_against_oracle; no other tolerance."""
import numpy as np
import pytest

import oracle
import rotsingle_cases as rc

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345e300


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


@pytest.fixture(scope="module")
def device_tables():
    """case -> (cos / sin of the coarse angles, of the fine grids, the grids' lengths) on the device, made once."""
    from utilities import features
    made = {}

    def get(case):
        if case.name not in made:
            made[case.name] = features._SearchContext.get().device_table(case.coarse, case.fine, case.fine_n)
        return made[case.name]
    return get


def _same(a, b):
    """Bit for bit, but for NaN, which equals NaN (and -0.0, which equals 0.0: neither occurs by construction)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ── icpmi_rotation_refine on a crafted head ─────────────────────────────────────────────────
def _refine_on_device(case):
    """Two runs into a sentinel-filled out4 -> [out4, out4]; the head must come back as it went."""
    import torch
    from icpmi import _lib
    from icpmi.batch import _ptr, _stream
    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    head = torch.from_numpy(case.head.copy()).to(dev)
    rec = np.full(_lib.RSREC_DOUBLES, -7.0)
    rec[_lib.RSREC_K], rec[_lib.RSREC_NF], rec[_lib.RSREC_J] = case.rec
    d_rec = torch.from_numpy(rec).to(dev)
    d_cs = torch.from_numpy(case.coarse_cs).to(dev)
    d_fcs = torch.from_numpy(case.fine_cs).to(dev) if case.max_fine else None
    scratch = torch.empty(L.icpmi_rotation_refine_workspace_bytes(case.raw[0]), dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    runs = []
    for _ in range(2):
        out.fill_(SENTINEL)
        _lib.check(L.icpmi_rotation_refine(_ptr(head), case.raw[0], case.raw[1], _ptr(d_rec), _ptr(d_cs), _ptr(d_fcs) if case.max_fine else None,
                                           case.max_fine, float(case.pred[0]), float(case.pred[1]), _ptr(out), _ptr(scratch), scratch.numel(),
                                           _stream()), "rotation_refine")
        runs.append(out.cpu().numpy())
    assert np.array_equal(head.cpu().numpy(), case.head), (case.name, "the refinement wrote into the search's workspace")
    return runs


@pytest.mark.parametrize("name", list(rc.refine_cases()))
def test_refinement_equals_the_restatement_bit_for_bit(name):
    """t, the inlier count and the 80th percentile of every refinement case, twice."""
    case = rc.refine_cases()[name]
    want = case.expected
    for run, got in enumerate(_refine_on_device(case)):
        print(f"{name} run {run}: device {got.tolist()} restatement {want.tolist()}")
        assert not (got == SENTINEL).any(), (name, run, got)
        assert _same(got[2:], want[2:]), (name, run, "inliers, threshold", got[2:], want[2:])
        assert _same(got[:2], want[:2]), (name, run, "t", got[:2], want[:2])


def test_the_head_gap_is_never_read():
    """180 of 300 and 120 of 200 rows valid, NaN or decoys nearer than any valid target behind the counts: the result of the
    head without a gap."""
    cases = rc.refine_cases()
    tight = _refine_on_device(cases["gap_tight"])[0]
    for name in ("gap_nan", "gap_decoy"):
        got = _refine_on_device(cases[name])[0]
        assert _same(got, tight) and _same(got, cases[name].expected), (name, got, tight)


# ── icpmi_rotation_search on crafted tables ───────────────────────────────────────────────
def _scores_in_workspace(ctx, n_src, n_tgt, n_coarse, max_fine):
    """The coarse and the fine scores the search left in its workspace (csrc/rotsearch.hip, RsWs: the head of
    RS_WS_CLOUDS bytes, n_src + n_tgt + 1 rows rounded up to 256 bytes, then n_coarse + max_fine scores)."""
    import torch
    at = rc.WS_CLOUDS + ((n_src + n_tgt + 1) * 16 + 255) // 256 * 256
    sc = ctx.ws[at:at + (n_coarse + max_fine) * 8].view(torch.float64).cpu().numpy()
    return sc[:n_coarse].copy(), sc[n_coarse:].copy()


@pytest.mark.parametrize("name", list(rc.search_cases()))
def test_search_record_is_np_argmin_of_its_own_scores(name, device_tables):
    """Every search case: the filter keeps the designed rows; MUS / MUT bit for bit; K, NF, J as the tables were built to
    give them (exact ties and NaN by index, the fine grid scored being the named row's); CSCORE, FSCORE and the scores left in
    the workspace equal the stand-alone entry's bit for bit and the oracle's to its bound; behind the winner's count +inf.
    The nan_* cases are the regression test of the NaN score: a NaN angle used to score +inf (the nearest-target scan's
    fmin drops NaN distances), so K named the finite minimum, 150, and the NaN rule of first_argmin was never reached."""
    from icpmi import _lib
    from utilities import features
    case = rc.search_cases()[name]
    ctx = features._SearchContext.get()
    rec = ctx.run(case.src, case.tgt, rc.VOXEL, case.coarse, case.fine, case.fine_n, device_tables(case), case.centred, case.shift)
    n_src, n_tgt, n_coarse = len(case.src), len(case.tgt), len(case.coarse)
    assert (rec[_lib.RSREC_NS], rec[_lib.RSREC_NT]) == (n_src, n_tgt), name                # the filter kept every row
    fs, ft = (c.cpu().numpy() for c in ctx.filtered_clouds(n_src, n_tgt, rec))
    sc_coarse, sc_fine = _scores_in_workspace(ctx, n_src, n_tgt, n_coarse, case.max_fine)
    assert np.array_equal(fs, case.filtered[0]) and np.array_equal(ft, case.filtered[1]), name

    # the means: np.mean(axis=0) of the filtered clouds, or zeros and the caller's shift, bit for bit
    rows, shift = case.frame(fs, ft)
    mu_s = np.mean(fs, axis=0) if case.centred else np.zeros(2)
    assert rec[_lib.RSREC_MUS:_lib.RSREC_MUS + 2].tobytes() == mu_s.tobytes(), (name, rec[2:4], mu_s)
    assert rec[_lib.RSREC_MUT:_lib.RSREC_MUT + 2].tobytes() == np.asarray(shift, dtype=np.float64).tobytes(), (name, rec[4:6], shift)

    k, nf, j = int(rec[_lib.RSREC_K]), int(rec[_lib.RSREC_NF]), int(rec[_lib.RSREC_J])
    print(f"{name}: K {k} NF {nf} J {j} CSCORE {rec[_lib.RSREC_CSCORE]!r} FSCORE {rec[_lib.RSREC_FSCORE]!r}; designed {case.K} {case.NF} {case.J}")
    assert (k, nf, j) == (case.K, case.NF, case.J), (name, (k, nf, j), (case.K, case.NF, case.J))

    def check(angles, win, score, left_behind, label):
        got = features.rotation_scores(rows, ft, angles, shift)
        ref = case.oracle_scores(angles)
        ok = ~np.isnan(angles)
        print(f"{name} {label}: record {score!r} stand-alone {got[win]!r} oracle {ref[win]!r} max |got - ref| {np.abs(got[ok] - ref[ok]).max():.3e} "
              f"bound {rc.score_bound(ref):.3e}")
        assert win == int(np.argmin(got)) and _same(got[win], score), (name, label, win, int(np.argmin(got)), got[win], score)
        assert _same(left_behind, got), (name, label, "the scores in the workspace are not the stand-alone entry's")
        assert np.isnan(got[~ok]).all() and not np.isnan(got[ok]).any(), (name, label)
        assert np.abs(got[ok] - ref[ok]).max() <= rc.score_bound(ref), (name, label)
        assert int(np.nanargmin(got)) == int(np.nanargmin(ref)), (name, label)               # decided by a margin above the bound, or by index

    check(case.coarse, k, rec[_lib.RSREC_CSCORE], sc_coarse, "coarse")
    assert np.isnan(rec[_lib.RSREC_CSCORE]) == bool(np.isnan(case.coarse).any()), name
    if nf > 0:
        check(case.fine[k, :nf], j, rec[_lib.RSREC_FSCORE], sc_fine[:nf], "fine")
    else:
        assert np.isnan(rec[_lib.RSREC_FSCORE]), (name, rec[_lib.RSREC_FSCORE])
    assert np.isposinf(sc_fine[nf:]).all(), (name, "an entry behind the winner's count was scored", sc_fine[nf:])


# ── through the Python layer: the device refinement and the host fallback on one input ────────────────────────
def test_2048_and_2049_raw_rows_refine_alike():
    """A scan of 2 048 raw rows refines on the device, the same scan with one row repeated (2 049 raw rows, the same
    filtered cloud) on the host: the same (R, t) bit for bit, and the oracle's."""
    from icpmi import submap
    submap.VERBOSE = False
    world = rc.lattice(2048, 500)
    pose_t = np.array([2.0, -1.0])
    scan = (world - pose_t) @ rc.rot(0.4) + np.random.default_rng(501).uniform(-0.01, 0.01, world.shape)
    th = 0.4 + np.deg2rad(3.0)
    pred = np.array([[np.cos(th), -np.sin(th), pose_t[0] + 0.05], [np.sin(th), np.cos(th), pose_t[1] - 0.04], [0.0, 0.0, 1.0]])
    kw = dict(angle_range=10.0, angle_step=2.0, fine_step=0.5, voxel_size=rc.VOXEL)
    longer = np.vstack([scan, scan[777:778]])
    assert len(scan) == rc.MAX_ROWS and len(longer) == rc.MAX_ROWS + 1
    assert np.array_equal(oracle.voxel_downsample(scan, rc.VOXEL), oracle.voxel_downsample(longer, rc.VOXEL))
    assert len(oracle.voxel_downsample(scan, rc.VOXEL)) == rc.MAX_ROWS
    R_dev, t_dev = submap.submap_rotation_search(scan, world, pred, **kw)
    R_host, t_host = submap.submap_rotation_search(longer, world, pred, **kw)
    R_ref, t_ref = oracle.submap_rotation_search(scan, world, pred, **kw)
    print(f"device t {t_dev.tolist()} host t {t_host.tolist()} oracle t {t_ref.tolist()}")
    assert np.array_equal(R_dev, R_host) and np.array_equal(t_dev, t_host)
    assert np.array_equal(R_dev, R_ref) and np.array_equal(t_dev, t_ref)
    assert not np.array_equal(t_dev, pred[:2, 2])                                            # the mean was taken, not the prediction
