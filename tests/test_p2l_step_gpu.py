"""One point-to-line step and the covariance normals of the HIP kernels against extended precision.

The references, the case generators and every bound come from tests/test_p2l_step_cpu.py, whose table records what
NumPy's own float64 formulas lose against the same references; nothing here is measured from the kernels.
  a. the stand-alone entry (misc.hip) on explicit correspondences: sums, solve and trigonometry alone;
  b. one iteration of the fused kernels (icp2.hip, and icp.hip with force_exhaustive), correspondences from the
     oracle's voxel filter and nearest neighbours, normals as the library reports them;
  c. the normals of every route against the eigenvector of the longdouble covariance.
"""
import numpy as np
import pytest

import oracle
from test_p2l_step_cpu import (FUSED_BANDS, FUSED_NORMAL_K, FUSED_SINGULAR, FUSED_TABLE, FUSED_VOXEL, GAP_MIN, P2L_TABLE, U, backward_bound,
                               backward_error, exhaustive_normal_clouds, forward_bound, forward_multiple, fused_cases,
                               fused_step_inputs,
                               normal_angle_units, normal_clouds, normals_bound, normals_reference, recover_theta,
                               small_normal_clouds, step_cases, step_reference, step_references, theta_band, trig_ulps)

pytestmark = pytest.mark.gpu

NORMAL_K, VOXEL = FUSED_NORMAL_K, FUSED_VOXEL


@pytest.fixture(scope="module")
def uicp():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import icp
    icp.VERBOSE = False
    return icp


def _check_step(name, family, ref, R, t, table=P2L_TABLE):
    """What one step of a kernel owes the exact reference, by verdict; the bounds are those of ``family`` in ``table``."""
    assert R[0, 0] == R[1, 1] and R[0, 1] == -R[1, 0], name
    assert np.isfinite(R).all() and np.isfinite(t).all(), name
    if ref["verdict"] == "exact":
        assert np.array_equal(R, np.eye(2)) and np.array_equal(t, np.zeros(2)), name     # icp.py:107-108
        return None
    assert abs(float(R[0, 0]) ** 2 + float(R[1, 0]) ** 2 - 1.0) <= 8 * U, name            # a proper rotation
    identity = np.array_equal(R, np.eye(2)) and not t.any()
    if ref["verdict"] == "numerical":
        return None
    assert not identity, name
    theta = recover_theta(R, ref["theta"])
    c_ulp, s_ulp = trig_ulps(R)
    near = {"below", "above"} & set(theta_band(theta))
    assert max(c_ulp, s_ulp) <= (1.0 if near else 2.0), (name, theta, c_ulp, s_ulp)
    x = (theta, float(t[0]), float(t[1]))
    bwd = backward_error(ref, x)
    assert bwd <= backward_bound(family, table), (name, bwd, backward_bound(family, table))
    if ref["kappa"] * U < 1e-6:
        fwd = forward_multiple(ref, x)
        assert fwd <= forward_bound(family, table), (name, fwd, forward_bound(family, table))
    return theta


def test_standalone_step_against_the_exact_reference(uicp):
    seen = set()
    for c, ref in zip(step_cases(), step_references()):
        R, t = uicp._point_to_line_solve_2d(c["src"], c["tgt"], c["normals"], c["idx"])
        theta = _check_step(c["name"], c["family"], ref, R, t)
        if theta is not None:
            seen.update((b, theta < 0) for b in theta_band(theta))
    assert len(seen) == 14, sorted(seen)                                  # seven bands, both signs, on the device too


def _fused_reference(uicp, src, tgt, gate):
    P, T, nrm, idx, d, keep = fused_step_inputs(src, tgt, gate, uicp.estimate_normals_2d)
    return step_reference(P, T, nrm, idx, max_corr_dist=gate, dists=d), len(P), int(keep.sum())


@pytest.fixture(scope="module")
def fused_refs(uicp):
    return [_fused_reference(uicp, src, tgt, gate) for _, src, tgt, gate in fused_cases()]


@pytest.mark.parametrize("force_exhaustive", [False, True])
def test_fused_kernels_one_iteration_against_the_exact_reference(uicp, fused_refs, force_exhaustive):
    from icpmi import _lib, batch
    cases = fused_cases()
    assert max(len(c[2]) for c in cases) > 4096 and max(len(c[1]) for c in cases) > 2048
    bands = set()
    for gate in (None, 0.05):
        sel = [i for i, c in enumerate(cases) if c[3] == gate]
        clouds = [cases[i][1] for i in sel] + [cases[i][2] for i in sel]
        B = len(sel)
        b = batch.IcpBatch(clouds, np.arange(B), np.arange(B, 2 * B), 1e-30, 1, VOXEL, method="point_to_line",
                           normal_k=NORMAL_K, max_corr_dist=gate, force_exhaustive=force_exhaustive)
        assert b.fast == (not force_exhaustive)
        R_all, t_all, _, info = batch.unpack_results(b.run().cpu().numpy()[:B], 2)
        for k, i in enumerate(sel):
            family, name = cases[i][0], f"{cases[i][0]}#{i}"
            ref, n_src, n_in = fused_refs[i]
            if family == "gate_few":                                      # 3..10 of 300 rows inside the gate: icp.py:186 stops
                assert n_src == 300 and 3 <= n_in <= 10
                assert info["status"][k] == _lib.ST_FEW_INLIERS, name
                assert np.array_equal(R_all[k], np.eye(2)) and not t_all[k].any(), name
                continue
            if gate is not None:
                assert n_src == 30 and 3 <= n_in <= 10 and ref["K"] == n_in, name
            assert info["iters"][k] == 1, name
            if family in FUSED_SINGULAR or family == "wall_axis":         # no row of the table: no regular step is owed
                assert ref["verdict"] == ("exact" if family == "wall_axis" else "numerical"), name
            theta = _check_step(name, family, ref, R_all[k], t_all[k], FUSED_TABLE)
            if theta is not None:
                bands.update((band, theta < 0) for band in theta_band(theta))
    assert FUSED_BANDS <= bands, sorted(FUSED_BANDS - bands)              # both sides of the switch at 0.25 rad, both signs


def _check_normals(label, got, pts, k, fam, kind):
    assert got.shape == pts.shape and np.isfinite(got).all(), label
    assert np.abs(np.sum(got * got, axis=1) - 1.0).max() <= 8 * U, label
    if kind == "one":
        assert np.array_equal(got, [[1.0, 0.0]]), label
    if kind != "wall":
        return
    ref, gap, _ = normals_reference(pts, k)
    ok = gap >= GAP_MIN
    units = normal_angle_units(got, ref, gap)
    assert units[ok].max() <= normals_bound(fam), (label, float(units[ok].max()), int(np.argmax(np.where(ok, units, 0))))


@pytest.mark.parametrize("mode", ["grid", "sweep"])
def test_prepare_normals_against_the_longdouble_eigenvector(uicp, libopt, mode):
    libopt.setenv("ICPMI_PREP_KNN", mode)
    for k, clouds in ((12, normal_clouds(300)), (5, normal_clouds(120)), (1, normal_clouds(60)), (10, small_normal_clouds()),
                      (12, small_normal_clouds())):
        for name, fam, pts, kind in clouds:
            _check_normals((mode, name, k), uicp.estimate_normals_2d(pts, k), pts, k, fam, kind)


def test_exhaustive_normals_against_the_longdouble_eigenvector(uicp):
    """normals.hip: clouds above 4096 rows with k <= 31; the whole list of clouds and exact duplicates."""
    for k, clouds in exhaustive_normal_clouds():
        for name, fam, pts, kind in clouds:
            assert 4097 <= len(pts) <= 5000
            _check_normals(("normals.hip", name, k), uicp.estimate_normals_2d(pts, k), pts, k, fam, kind)


@pytest.mark.parametrize("k", [32, 40])
def test_drawn_normals_against_the_longdouble_eigenvector(uicp, k):
    """More than 31 neighbours: a wave draws them one by one."""
    for name, fam, pts, kind in normal_clouds(300) + small_normal_clouds():
        _check_normals(("draw", name, k), uicp.estimate_normals_2d(pts, k), pts, k, fam, kind)
