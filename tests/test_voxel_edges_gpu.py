"""The voxel filter (csrc/voxel.hip) at its edges, bit for bit against the NumPy restatement tests/voxel_ref.py: runs of three
to 20 000 points, whose sums depend on the order of their members, on every code path — the four register-sort shapes, the
three sort forms of the LDS path from just below and just above their switches, the large path; division lattices, whose
keys depend on the rounding of the float64 divide; and the clouds the filter refuses, on the register, LDS and large path
and through both Python entry points.  The inputs are those of tests/voxel_cases.py; tests/test_voxel_edges_cpu.py proves
without a GPU that each has its property and takes the path it is meant for.  No tolerance anywhere: np.array_equal, shapes
included.  (tests/test_sort_layouts_gpu.py crosses the same switches with clouds whose voxels hold one or two points.)"""
import numpy as np
import pytest

import voxel_cases as vc
import voxel_ref as vr

pytestmark = pytest.mark.gpu


def _filter_set(clouds, voxel):
    from icpmi import batch
    return batch.voxel_downsample_set(batch.CloudSet.from_numpy(clouds), voxel)


def _assert_same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), what


def _ids(cases):
    return [c[0] for c in cases]


# ── lone clouds: the 1 024-thread launch, and the large path above 8 192 rows ───────────────────────────────────────────
@pytest.mark.parametrize("case", vc.all_cases(), ids=_ids(vc.all_cases()))
def test_lone_cloud(case):
    name, pts, voxel = case
    out = _filter_set([pts], voxel).to_numpy()
    assert len(out) == 1
    _assert_same(out[0], vc.reference(case), name)


# ── sets of 257 clouds: the 512-thread launch, LDS sized to the largest member ──────────────────────────────────────────
def _set_groups():
    """(id, the cases of one set): one set per family, dimensionality and voxel size (a set has one of each)"""
    groups = {}
    for fam, cases in vc.FAMILIES.items():
        for case in cases():
            if len(case[1]) <= vc.SMALL_MAX:
                groups.setdefault((fam, case[1].shape[1], case[2]), []).append(case)
    return [(f"{fam}_{dim}d_v{voxel:.4g}", cases) for (fam, dim, voxel), cases in groups.items()]


@pytest.mark.parametrize("cases", [g[1] for g in _set_groups()], ids=[g[0] for g in _set_groups()])
def test_set_of_257(cases):
    voxel, dim = cases[0][2], cases[0][1].shape[1]
    members = [cases[i % len(cases)] for i in range(vc.SET_CLOUDS - 1)]
    clouds = [c[1] for c in members]
    clouds.insert(100, np.empty((0, dim)))
    want = [vc.reference(c) for c in members]
    want.insert(100, np.empty((0, dim)))
    assert len(clouds) == vc.SET_CLOUDS and vc.threads_of(len(clouds)) == 512
    out = _filter_set(clouds, voxel).to_numpy()
    assert len(out) == len(want)
    for i, (o, w) in enumerate(zip(out, want)):
        _assert_same(o, w, (i, "empty" if i == 100 else members[i - (i > 100)][0]))


def test_every_small_case_is_in_a_set():
    in_sets = {c[0] for _, cases in _set_groups() for c in cases}
    assert in_sets == {c[0] for c in vc.all_cases() if len(c[1]) <= vc.SMALL_MAX}


# ── a large-path cloud between small ones ───────────────────────────────────────────────────────────────────────────────
def test_mixed_set():
    """One launch over the small clouds (which skips the large one), the large path for the cloud in between: every member
    compared.  The large cloud is two run cases one after the other, 12 289 rows with runs of up to 140."""
    voxel = vc.RUN_VOXEL
    big = np.concatenate([vc.runs(8192, 2)[1], vc.runs(4097, 2)[1]])
    assert vc.route(big, voxel, 1024) == "large"
    clouds = [vc.runs(513, 2)[1], vc.runs(2048, 2)[1], big, np.empty((0, 2)), vc.runs(4097, 2)[1], vc.runs(1024, 2)[1]]
    want = [vr.voxel_ref(c, voxel) if len(c) else np.empty((0, 2)) for c in clouds]
    out = _filter_set(clouds, voxel).to_numpy()
    for i, (o, w) in enumerate(zip(out, want)):
        _assert_same(o, w, i)


# ── the entry point users call ──────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", [vc.one_voxel(4096, 3), vc.one_voxel(20000, 2), vc.runs(2049, 2), vc.runs(1025, 3),
                                  vc.clusters("above 9e18", 2048, 2), vc.clusters("exactly 4e9", 1024, 3),
                                  vc.lattice(0.1, -7.3), vc.lattice_tiled(0.04, 0.0, 8193)], ids=lambda c: c[0])
def test_voxel_downsample_entry_point(case):
    from utilities import icp as uicp
    name, pts, voxel = case
    _assert_same(uicp.voxel_downsample(pts, voxel), vc.reference(case), name)


# ── refusals: counts and points are read back on the host only, no other kernel sees a negative count ───────────────────
@pytest.mark.parametrize("case", vc.refusal_cases(), ids=_ids(vc.refusal_cases()))
def test_refused_cloud_raises_from_both_entry_points(case):
    from icpmi import batch
    from utilities import icp as uicp
    name, pts, voxel = case
    with pytest.raises(OverflowError, match="voxel key range does not fit in 64 bits"):
        uicp.voxel_downsample(pts, voxel)
    out = _filter_set([pts], voxel)
    assert out.counts_host()[:1].tolist() == [-1], name
    with pytest.raises(OverflowError) as e:
        out.to_numpy()
    assert str(e.value) == batch.VOXEL_KEY_RANGE_ERROR


def test_refused_submap_raises():
    """The rolling submap and the rotation search's filter read the count back the same way: they raise too, where a slice
    bound of -1 dropped the last row of the unfiltered stack."""
    from icpmi import submap
    name, pts, voxel = vc.refusal("apart", 8193)
    sm = submap.RollingSubmap(window=2, voxel_size=voxel)
    sm.push(pts[:5000].copy())
    sm.push(pts[5000:].copy())
    with pytest.raises(OverflowError, match="voxel key range does not fit in 64 bits"):
        sm.build()
    with pytest.raises(OverflowError, match="voxel key range does not fit in 64 bits"):
        submap._voxel_rows(submap._device_rows(vc.refusal("tiny_voxel", 64)[1].copy()), 1e-300)


def _refusal_sets():
    """(id, clouds, voxel, refused): refused clouds of 64, 2 048 and 8 193 rows (LDS, register, large path) between clouds the
    filter answers.  At a voxel of 1e-300 those are clouds of one point, or of one point many times."""
    apart = [vc.clusters("below 4e9", 1024, 2)[1], vc.refusal("apart", 64)[1], vc.clusters("above 9e18", 2048, 2)[1],
             vc.refusal("apart", 2048)[1], vc.clusters("above 4e9", 4096, 2)[1], vc.refusal("apart", 8193)[1],
             vc.clusters("below 4e9", 2048, 2)[1]]
    small = [c for c in apart if len(c) <= vc.SMALL_MAX]
    tiny = [np.array([[0.3, -1.7]]), vc.refusal("tiny_voxel", 64)[1], np.full((70, 2), 0.3), vc.refusal("tiny_voxel", 2048)[1],
            np.full((2048, 2), -1.1), vc.refusal("tiny_voxel", 8193)[1], np.full((8193, 2), 0.7)]
    return [("apart", apart, 0.5), ("apart_257", [small[i % len(small)] for i in range(vc.SET_CLOUDS)], 0.5),
            ("tiny_voxel", tiny, 1e-300)]


@pytest.mark.parametrize("clouds,voxel", [s[1:] for s in _refusal_sets()], ids=[s[0] for s in _refusal_sets()])
def test_refused_cloud_in_a_set(clouds, voxel):
    refused = [vc.route(c, voxel, 1024) == vc.REFUSED for c in clouds]
    assert 2 <= sum(refused) < len(clouds) - 1
    out = _filter_set(clouds, voxel)
    cnt = out.counts_host()[:len(clouds)]
    host = out.pts.cpu().numpy()
    for i, (c, r) in enumerate(zip(clouds, refused)):
        if r:
            assert cnt[i] == -1, (i, len(c), int(cnt[i]))
        else:
            want = vr.voxel_ref(c, voxel)
            assert cnt[i] == len(want), (i, len(c), int(cnt[i]))
            _assert_same(host[out.off_host[i]:out.off_host[i] + cnt[i]], want, (i, len(c)))
    with pytest.raises(OverflowError):
        out.to_numpy()
