"""One point-to-point step of the HIP kernels against exact arithmetic, and the correspondence gate at its own resolution.

The exact reference, the measures and their units, the cases and every bound come from tests/test_p2p_step_cpu.py, whose
tables record what NumPy's float64 restatement of the reference loses against the same exact values; a kernel is held to
max(4, 8 x NumPy), and nothing here is measured from a kernel.  One iteration of ``IcpBatch`` returns the step itself:
  a. the 2-D step through the fused kernel (icp2.hip) and the exhaustive one (icp.hip, ``force_exhaustive``);
  b. rows exactly on ``max_corr_dist``, for both methods and both kernels;
  c. the 3-D step (kabsch3), which only the exhaustive kernel takes.
"""
import numpy as np
import pytest

from test_p2l_step_cpu import FUSED_NORMAL_K, FUSED_VOXEL, step_reference
from test_p2l_step_gpu import _check_step
from test_p2p_step_cpu import (EDGE_GATES, EDGE_P2L_TABLE, GATE, P2P3_TABLE, P2P_BANDS, P2P_TABLE, VOXEL_3D, cases_3d, check_2d,
                               check_3d, edge_inputs, edge_pairs, p2p_band, p2p_cases, p2p_references, p2p_step_reference,
                               references_3d)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uicp():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import icp
    icp.VERBOSE = False
    return icp


def _one_iteration(clouds, dim, voxel, **kw):
    """One iteration of every pair (cloud k onto cloud B + k) -> (R, t, err, info) on the host."""
    from icpmi import batch
    B = len(clouds) // 2
    b = batch.IcpBatch(clouds, np.arange(B), np.arange(B, 2 * B), 1e-30, 1, voxel, **kw)
    assert b.fast == (dim == 2 and not kw.get("force_exhaustive", False))
    return batch.unpack_results(b.run().cpu().numpy()[:B], dim)


def _stopped(name, R, t, info, k, dim=2):
    """icp.py:186-187: too few rows inside the gate, the pair stops before its first step."""
    from icpmi import _lib
    assert info["status"][k] == _lib.ST_FEW_INLIERS and info["iters"][k] == 0, (name, info["status"][k], info["iters"][k])
    assert np.array_equal(R, np.eye(dim)) and not t.any(), name


def _took_a_step(name, info, k):
    from icpmi import _lib
    assert info["iters"][k] == 1 and info["status"][k] == _lib.ST_MAXITER, (name, info["iters"][k], info["status"][k])


def _report(title, names, worst, table):
    print(f"\n{title}: worst figure per family ({', '.join(names)}), the bound in brackets")
    for fam, figs in worst.items():
        print(f"  {fam:14s}" + "".join(f" {'-':>10s}       " if v is None else f" {v:10.3g} [{max(4.0, 8 * table[fam][j]):5.3g}]"
                                      for j, v in enumerate(figs)))


def _keep_worst(worst, family, figs):
    m = worst.setdefault(family, [None] * len(figs))
    for j, v in enumerate(figs):
        if v is not None:
            m[j] = v if m[j] is None else max(m[j], v)


@pytest.mark.parametrize("force_exhaustive", [False, True])
def test_one_iteration_2d_against_the_exact_reference(uicp, force_exhaustive):
    cases, refs = p2p_cases(), p2p_references()
    worst, bands, stopped = {}, set(), 0
    for gate in (None, GATE):
        sel = [i for i, c in enumerate(cases) if c.gate == gate]
        R_all, t_all, err_all, info = _one_iteration([cases[i].src for i in sel] + [cases[i].tgt for i in sel], 2, FUSED_VOXEL,
                                                     method="point_to_point", max_corr_dist=gate, force_exhaustive=force_exhaustive)
        for k, i in enumerate(sel):
            case, (P, Q, keep, need, ref) = cases[i], refs[i]
            if ref is None:                                              # need - 1 inliers, or the 3..10 of 300 of gate_few
                _stopped(case.name, R_all[k], t_all[k], info, k)
                stopped += 1
                continue
            _took_a_step(case.name, info, k)
            _keep_worst(worst, case.family, check_2d(case.name, case.family, ref, P, Q, R_all[k], t_all[k], err_all[k]))
            if ref["verdict"] == "regular":
                theta = float(np.arctan2(R_all[k][1, 0], R_all[k][0, 0]))
                bands.update((b, theta < 0) for b in p2p_band(theta))
    _report(f"2-D, force_exhaustive={force_exhaustive}", ("angle", "translation", "error"), worst, P2P_TABLE)
    assert stopped == 3 and set(worst) == set(P2P_TABLE) - {"edge"}
    assert bands == P2P_BANDS, sorted(bands ^ P2P_BANDS)                  # tiny, small and next to pi / 2, both signs


@pytest.mark.parametrize("force_exhaustive", [False, True])
@pytest.mark.parametrize("method", ["point_to_point", "point_to_line"])
def test_rows_exactly_on_the_gate(uicp, method, force_exhaustive):
    """d**2 < g**2 (icp.py:183-186) for g one ulp below, at and one ulp above the distance of the edge rows: out, out,
    in.  The flip pair changes its status with them, the minority pair its step; the step owed is the exact one on
    the rows the reference keeps."""
    pairs = edge_pairs()
    worst, outcomes = {}, []
    for gate in EDGE_GATES:
        R_all, t_all, err_all, info = _one_iteration([p[1] for p in pairs] + [p[2] for p in pairs], 2, FUSED_VOXEL, method=method,
                                                     normal_k=FUSED_NORMAL_K, max_corr_dist=gate, force_exhaustive=force_exhaustive)
        for k, (name, src, tgt, _) in enumerate(pairs):
            P, T, idx, d, keep = edge_inputs(src, tgt, gate)
            label = f"{name}@{gate!r}"
            outcomes.append(int(keep.sum()))
            if keep.sum() < 3:
                _stopped(label, R_all[k], t_all[k], info, k)
                continue
            _took_a_step(label, info, k)
            if method == "point_to_point":
                ref = p2p_step_reference(P, T[idx], keep)
                _keep_worst(worst, "edge", check_2d(label, "edge", ref, P, T[idx], R_all[k], t_all[k], err_all[k]))
            else:
                ref = step_reference(P, T, uicp.estimate_normals_2d(T, FUSED_NORMAL_K), idx, max_corr_dist=gate, dists=d)
                assert ref["verdict"] == "regular" and ref["K"] == keep.sum(), label
                assert _check_step(label, "edge", ref, R_all[k], t_all[k], EDGE_P2L_TABLE) is not None, label
    assert outcomes == [2, 10, 2, 10, 3, 14], outcomes
    if worst:
        _report(f"edge pairs, force_exhaustive={force_exhaustive}", ("angle", "translation", "error"), worst, P2P_TABLE)


def test_one_iteration_3d_against_the_exact_reference(uicp):
    cases, refs = cases_3d(), references_3d()
    R_all, t_all, err_all, info = _one_iteration([c[2] for c in cases] + [c[3] for c in cases], 3, VOXEL_3D)
    worst = {}
    for k, ((fam, name, _, _), (P, Q, ref)) in enumerate(zip(cases, refs)):
        _took_a_step(name, info, k)
        _keep_worst(worst, fam, check_3d(name, fam, ref, P, Q, R_all[k], t_all[k], err_all[k]))
    _report("3-D", ("skew", "orth", "translation", "error"), worst, P2P3_TABLE)
    assert set(worst) == set(P2P3_TABLE)
