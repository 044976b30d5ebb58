"""Pins tests/pose_graph_ref.py and proves the conditions its cases must meet, without a GPU.

The GPU tests (tests/test_pose_graph_step_gpu.py) ask the kernel for ``step_bound``; here the oracle — the float64
restatement of the reference, solved by LAPACK — is held to the same bound on every case, the extended-precision step is
shown to have converged far below it, and the bound is shown to be a real demand (3n kappa 2^-53 <= 1e-5).
"""
import numpy as np
import pytest

import pose_graph_ref as ref
from oracle import pose_graph as opg

STEP, MULTI, SINGULAR = ref.case_names("step"), ref.case_names("multi"), ref.case_names("singular")


def _oracle_step(name):
    c = ref.cases()[name]
    g = c["graph"]
    out, it, st, norm = opg.optimize(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], 1, c["fix"], 0.0)
    return ref.step_difference(out, g["nodes"]), it, st, norm


def test_case_list_covers_what_it_claims():
    cs = ref.cases()
    assert len(STEP) == 23 + 4 + 1 + 2 + 5 + 3 + 9 and len(MULTI) == 4 and len(SINGULAR) == 2
    g = cs["closures_171"]["graph"]
    far = np.abs(g["ei"] - g["ej"]) != 1
    assert 3 * int(far.sum()) > 512 and (g["ei"] == g["ej"]).sum() == 1          # closure system wider than the workgroup
    assert ((g["ei"] == 7) | (g["ej"] == 7))[far].sum() >= 2                        # closures that end on the anchor
    for name in ("dense_540", "dense_540_gap", "info_indef_dense", "singular_dense"):
        g = cs[name]["graph"]
        linked = {min(a, b) for a, b in zip(g["ei"], g["ej"]) if abs(a - b) == 1}
        assert len(linked) < len(g["nodes"]) - 1, name                             # no chain numbering: the dense path
    assert 3 * len(cs["dense_540"]["graph"]["nodes"]) > 512
    for name in STEP:
        if cs[name]["family"] not in ("dense wider than 512",) and not name.endswith("_dense"):
            g = cs[name]["graph"]
            linked = {min(a, b) for a, b in zip(g["ei"], g["ej"]) if abs(a - b) == 1}
            assert len(linked) == len(g["nodes"]) - 1, name                        # a full chain: the split path
    g = cs["angles_out_of_range"]["graph"]
    assert g["nodes"][:, 2].max() > np.pi and g["nodes"][:, 2].min() < -np.pi
    g = cs["branch_cut"]["graph"]
    assert np.abs(np.abs(g["nodes"][:, 2]) - np.pi).min() < 0.06


@pytest.mark.parametrize("name", STEP)
def test_oracle_step_is_within_the_bound(name):
    r = ref.step_reference(name)
    n3 = r["H"].shape[0]
    assert n3 * r["kappa"] * ref.U <= 1e-5, (name, r["kappa"])                     # the bound is a real demand
    assert r["last_correction"] <= r["bound"] / 1024, (name, r["last_correction"], r["bound"])
    d, it, st, norm = _oracle_step(name)
    err = float(np.abs(d - r["dx"]).max())
    print(f"{name}: kappa {r['kappa']:.2e} bound {r['bound']:.2e} oracle error/bound {err / r['bound']:.2e}")
    assert err <= r["bound"], (name, err, r["bound"])
    assert (it, st) == (1, opg.MAX_ITERATIONS)
    assert abs(norm - r["norm"]) <= r["bound"] * np.sqrt(n3), name


@pytest.mark.parametrize("name", [n for n in STEP if 3 * len(ref.cases()[n]["graph"]["nodes"]) <= 120])
def test_refinement_agrees_with_long_double_lu(name):
    r = ref.step_reference(name)
    x = ref.lu_ld(r["H"], r["b"])
    scale = float(np.abs(x).max())
    assert float(np.abs(x - r["dx_ld"]).max()) <= 64 * float(np.finfo(ref.LD).eps) * r["kappa"] * scale + 1e-300, name
    assert float(np.abs(x - r["dx_ld"]).max()) <= r["bound"] / 1024, name


def test_assembly_restates_the_oracle():
    """H and b in long double against the oracle's float64 assembly, on a graph with every edge form."""
    for name in ("chain_twice_and_reversed", "info_indef", "closures_171", "angles_out_of_range"):
        c = ref.cases()[name]
        g = c["graph"]
        H, b = ref.assemble_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["fix"])
        n = len(g["nodes"])
        e, A, B = opg.linearise(g["nodes"], g["ei"], g["ej"], g["z"])
        H4 = np.zeros((n, n, 3, 3))
        At, Bt = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
        for idx, blk in (((g["ei"], g["ei"]), At @ g["omega"] @ A), ((g["ei"], g["ej"]), At @ g["omega"] @ B),
                         ((g["ej"], g["ei"]), Bt @ g["omega"] @ A), ((g["ej"], g["ej"]), Bt @ g["omega"] @ B)):
            np.add.at(H4, idx, blk)
        H64 = H4.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
        f = 3 * c["fix"]
        H64[f:f + 3, :] = 0.0
        H64[:, f:f + 3] = 0.0
        H64[f:f + 3, f:f + 3] = np.eye(3) * 1e10
        mag = float(np.abs(H64[H64 < 1e9]).max())
        assert float(np.abs(np.asarray(H, dtype=np.float64) - H64).max()) <= 1e-12 * mag * len(g["ei"]), name


@pytest.mark.parametrize("name", MULTI)
def test_iteration_counts_do_not_hinge_on_rounding(name):
    c = ref.cases()[name]
    run = ref.run_reference(name)
    assert run["status"] == ref.OK and 4 <= run["iterations"] < c["n_iterations"], (name, run["iterations"], run["steps"])
    for s in run["steps"]:
        assert s > 10 * c["eps"] or s < c["eps"] / 10, (name, run["steps"])
    g = c["graph"]
    out, it, st, _ = opg.optimize(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["n_iterations"], c["fix"], c["eps"])
    assert (it, st) == (run["iterations"], opg.OK), name
    d = ref.step_difference(out, np.asarray(run["iterates"][-1], dtype=np.float64))
    assert float(np.abs(d).max()) <= sum(run["bounds"]), (name, float(np.abs(d).max()), sum(run["bounds"]))


@pytest.mark.parametrize("name", SINGULAR)
def test_singular_cases_are_singular_for_the_oracle(name):
    c = ref.cases()[name]
    g = c["graph"]
    out, it, st, _ = opg.optimize(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], 1, c["fix"], 0.0)
    assert (it, st) == (0, opg.SINGULAR) and np.array_equal(out, g["nodes"])


def test_total_error_reference():
    g = ref.exact_single_edge()
    tot, bound = ref.total_error_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"])
    assert tot == 48.625 and 0 < bound < 1e-13 and len(g["ei"]) == 1
    assert abs(opg.total_error(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"]) - tot) <= bound
    g = ref.cases()["circle_n600_fix300"]["graph"]
    tot, bound = ref.total_error_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"])
    assert abs(opg.total_error(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"]) - tot) <= bound and len(g["ei"]) > 512


def test_weak_chain_edges_get_room_in_the_workspace():
    """The library's size query with the information matrices reserves room for the twins of weak chain edges (host only);
    a graph without weak chain edges needs what it needed before."""
    import ctypes
    import icpmi
    lib = icpmi.lib()

    def sizes(g):
        ij = np.ascontiguousarray(np.stack([g["ei"], g["ej"]], axis=1).astype(np.int32))
        om = np.ascontiguousarray(g["omega"], dtype=np.float64)
        n, m = len(g["nodes"]), len(ij)
        return (lib.icpmi_pose_graph_workspace_bytes(ij.ctypes.data_as(ctypes.c_void_p), n, m),
                lib.icpmi_pose_graph_weighted_workspace_bytes(ij.ctypes.data_as(ctypes.c_void_p), om.ctypes.data_as(ctypes.c_void_p), n, m))

    for name in ("circle_n600_fix300", "circle_n513_fix256", "dense_540"):
        plain, weighted = sizes(ref.cases()[name]["graph"])
        assert plain == weighted > 0, name
    for name in ("weak_eps1", "weak_eps0.0001", "weak_eps1e-08"):
        plain, weighted = sizes(ref.cases()[name]["graph"])
        assert weighted > plain > 0, name
    # a chain edge with a null direction gets no twin: such a graph is left to the dense elimination
    for name in ("weak_eps1e-12", "weak_eps0", "weak_zero_matrix", "weak_last_node", "singular_chain"):
        plain, weighted = sizes(ref.cases()[name]["graph"])
        assert weighted == plain > 0, name


@pytest.mark.parametrize("entry, size_query", [("icpmi_pose_graph_optimize", "icpmi_pose_graph_workspace_bytes"),
                                               ("icpmi_pose_graph_optimize_dense", "icpmi_pose_graph_dense_workspace_bytes")])
def test_host_refusals_come_before_any_launch(entry, size_query):
    """Fake device pointers on a 6-node chain with one closure: every refusal below is decided on the host before the first
    HIP call, so none of the pointers is ever touched."""
    import ctypes as C
    import os
    import re
    import icpmi
    from conftest import REPO
    header = open(os.path.join(REPO, "include", "icpmi.h")).read()
    ERR_ARG, ERR_WORKSPACE = (int(re.search(r"^#define ICPMI_ERR_%s \((-\d+)\)" % k, header, flags=re.M).group(1)) for k in ("ARG", "WORKSPACE"))
    L = icpmi.lib()
    ij = np.ascontiguousarray(np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], dtype=np.int32))
    n, m = 6, len(ij)
    ijp = ij.ctypes.data_as(C.c_void_p)
    nodes, z, omega, info, ws = [C.c_void_p(0x1000 * (k + 1)) for k in range(5)]
    least = getattr(L, size_query)(ijp, n, m)
    assert least > 0

    def call(nodes=nodes, ijp=ijp, z=z, omega=omega, n=n, m=m, iters=5, fix=0, info=info, ws=ws, ws_bytes=least):
        return getattr(L, entry)(nodes, ijp, z, omega, n, m, iters, fix, 1e-6, info, ws, ws_bytes, None)

    assert call(nodes=None) == ERR_ARG and call(info=None) == ERR_ARG
    assert call(n=-1) == ERR_ARG and call(m=-1) == ERR_ARG and call(iters=-1) == ERR_ARG
    assert call(ijp=None) == ERR_ARG and call(z=None) == ERR_ARG and call(omega=None) == ERR_ARG
    assert call(fix=6) == ERR_ARG and call(fix=-1) == ERR_ARG
    for bad in ((0, 6), (-1, 2)):
        bad_ij = ij.copy()
        bad_ij[2] = bad
        assert call(ijp=bad_ij.ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert getattr(L, size_query)(bad_ij.ctypes.data_as(C.c_void_p), n, m) == 0
    assert call(ws=None) == ERR_WORKSPACE
    assert call(ws_bytes=least - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE
