"""Single Gauss-Newton steps of the pose-graph kernel (csrc/posegraph.hip) against extended precision.

Running to convergence hides a solve that is only good to a few digits: the next iteration corrects it.  Here ONE step is
compared with the long-double step of tests/pose_graph_ref.py, within ``step_bound`` — what a backward-stable float64
solve of the same system owes, nothing measured on the kernel — at the smallest shapes where each part of the kernel can
go wrong.  tests/test_pose_graph_step_cpu.py holds the oracle to the same bound on the same cases and records its share.

Weak chain edges are the cases the chain + closures split cannot solve by itself: the chain alone is (nearly) singular
while the closures keep the whole system healthy.  The kernel has to notice and take the dense matrix.

Before the plan gave weak chain edges a twin among the closures, the device missed the bound of 2.6e-10 on the weak-chain
cases from eps = 1e-4 down (2.7e-8, 1.6e-6, 1.4e-4, 0.41, 1.1; 7.4 with zero matrices) and reported "singular H" for
weak_last_node.
"""
import numpy as np
import pytest

import pose_graph_ref as ref

pytestmark = pytest.mark.gpu

STEP, MULTI, SINGULAR = ref.case_names("step"), ref.case_names("multi"), ref.case_names("singular")


@pytest.fixture(scope="module")
def upg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import pose_graph
    pose_graph.VERBOSE = False
    return pose_graph


def _graph(upg, g):
    pg = upg.PoseGraph2D()
    for v in g["nodes"]:
        pg.add_node(v)
    for i, j, z, om in zip(g["ei"], g["ej"], g["z"], g["omega"]):
        pg.add_edge(int(i), int(j), z, om)
    return pg


@pytest.mark.parametrize("name", STEP)
def test_one_step_against_extended_precision(upg, name):
    c = ref.cases()[name]
    g, r = c["graph"], ref.step_reference(name)
    pg = _graph(upg, g)
    pg.optimize(n_iterations=1, fix_node=c["fix"], convergence_eps=0.0)
    info = pg.last_info
    d = ref.step_difference(np.array(pg.nodes), g["nodes"])
    err = float(np.abs(d - r["dx"]).max())
    print(f"{name} [{c['family']}]: bound {r['bound']:.3e} error/bound {err / r['bound']:.3e} "
          f"status {info['status']} iterations {info['iterations']} split refused at {info.get('split_refused_at')}")
    assert (info["status"], info["iterations"]) == (upg.MAX_ITERATIONS, 1), (name, info)
    assert err <= r["bound"], (name, err, r["bound"])
    assert abs(info["step_norm"] - r["norm"]) <= r["bound"] * np.sqrt(3 * len(g["nodes"])), (name, info["step_norm"], r["norm"])


@pytest.mark.parametrize("name", SINGULAR)
def test_singular_stays_singular(upg, name):
    """A node no edge with information holds: the reference's LAPACK call fails at iteration 0, the poses stay."""
    c = ref.cases()[name]
    pg = _graph(upg, c["graph"])
    pg.optimize(n_iterations=1, fix_node=c["fix"], convergence_eps=0.0)
    print(f"{name}: {pg.last_info}")
    assert (pg.last_info["status"], pg.last_info["iterations"]) == (upg.SINGULAR, 0), (name, pg.last_info)
    assert np.array_equal(np.array(pg.nodes), c["graph"]["nodes"]), name


@pytest.mark.parametrize("name", MULTI)
def test_several_iterations(upg, name):
    c = ref.cases()[name]
    g, run = c["graph"], ref.run_reference(name)
    kw = dict(n_iterations=c["n_iterations"], fix_node=c["fix"], convergence_eps=c["eps"])
    pg = _graph(upg, g)
    pg.optimize(**kw)
    out = np.array(pg.nodes)
    d = ref.step_difference(out, np.asarray(run["iterates"][-1], dtype=np.float64))
    err, bound = float(np.abs(d).max()), sum(run["bounds"])
    print(f"{name}: bound {bound:.3e} error/bound {err / bound:.3e} {pg.last_info} reference iterations {run['iterations']}")
    assert (pg.last_info["status"], pg.last_info["iterations"]) == (run["status"], run["iterations"]), (name, pg.last_info)
    assert err <= bound, (name, err, bound)
    again = _graph(upg, g)
    again.optimize(**kw)
    assert np.array_equal(np.array(again.nodes), out), name                      # fixed summation orders: bit-identical
    assert again.last_info["step_norm"] == pg.last_info["step_norm"], name


def test_total_error_against_extended_precision(upg):
    for label, g in (("one exact edge", ref.exact_single_edge()), ("n = 600", ref.cases()["circle_n600_fix300"]["graph"])):
        tot, bound = ref.total_error_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"])
        got = _graph(upg, g).total_error()
        print(f"total_error {label}: m {len(g['ei'])} reference {tot!r} device {got!r} error/bound {abs(got - tot) / bound:.3e}")
        assert abs(got - tot) <= bound, (label, got, tot, bound)


@pytest.mark.parametrize("entry", ["optimize", "optimize_robust", "marginals"])
def test_refused_without_room_for_the_twins_writes_nothing(upg, entry):
    """The three entries that run on a plan share one host front.  On the smallest graph with a twin and a closure — a
    6-node chain, the closure (5, 0), chain edge 2 with Omega = diag(1e-8, 1e4, 1e4), every other Omega = 1e4 I — a
    workspace sized without the information matrices has no room for the twin: ICPMI_OK, status REFUSED, and the nodes and
    every output keep the bytes they held.  Sized with the matrices the call proceeds.  With fewer than two nodes the
    status is NOTHING and again nothing is written."""
    import ctypes as C
    import torch
    from icpmi import _lib
    from icpmi import batch as _b
    L = _lib.lib()
    n, dev = 6, torch.device("cuda", torch.cuda.current_device())
    ij = np.ascontiguousarray(np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], dtype=np.int32))
    m = len(ij)
    t = 2.0 * np.pi * np.arange(n) / n
    nodes = np.ascontiguousarray(np.stack([np.cos(t), np.sin(t), t + np.pi / 2], axis=1))
    nodes[1:] += 0.01 * np.array([[1.0, -2.0, 0.5], [-1.5, 0.5, 1.0], [0.5, 1.0, -1.0], [2.0, -0.5, 0.5], [-1.0, 1.5, -0.5]])
    c, s = np.cos(np.pi / 3), np.sin(np.pi / 3)                                     # consecutive poses of the regular hexagon
    z = np.ascontiguousarray(np.tile([s, 1.0 - c, np.pi / 3], (m, 1)))
    om = np.ascontiguousarray(np.tile(1e4 * np.eye(3), (m, 1, 1)))
    om[2] = np.diag([1e-8, 1e4, 1e4])
    mask = np.ascontiguousarray(np.array([0, 0, 0, 0, 0, 1], dtype=np.uint8))
    ijp, omp, maskp = (a.ctypes.data_as(C.c_void_p) for a in (ij, om, mask))
    d_nodes, d_z, d_om = (torch.from_numpy(a).to(dev) for a in (nodes, z, om))
    doubles, status_slot = {"optimize": (_lib.PGINFO_DOUBLES, _lib.PGINFO_STATUS), "optimize_robust": (_lib.ROB_DOUBLES, _lib.PGINFO_STATUS),
                            "marginals": (_lib.MARG_DOUBLES, _lib.MARG_STATUS)}[entry]
    d_info = torch.full((doubles,), -1.0, dtype=torch.float64, device=dev)
    # what the entry writes besides nodes and info: nothing; chi2 and weights per edge; the diagonal blocks
    outs = [torch.full((k,), 7.0, dtype=torch.float64, device=dev) for k in {"optimize": (), "optimize_robust": (m, m), "marginals": (n * 9,)}[entry]]
    if entry == "optimize":
        small, full = L.icpmi_pose_graph_workspace_bytes(ijp, n, m), L.icpmi_pose_graph_weighted_workspace_bytes(ijp, omp, n, m)
    elif entry == "optimize_robust":
        small, full = (L.icpmi_pose_graph_robust_workspace_bytes(ijp, o, maskp, n, m, 0) for o in (None, omp))
    else:
        small, full = (L.icpmi_pose_graph_marginals_workspace_bytes(ijp, o, n, m, 0, 1, 0) for o in (None, omp))
    assert 0 < small < full
    ws = torch.empty(full, dtype=torch.uint8, device=dev)

    def call(n_nodes, ws_bytes):
        common = (_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om))
        tail = (_b._ptr(d_info), _b._ptr(ws), ws_bytes, _b._stream())
        if entry == "optimize":
            rc = L.icpmi_pose_graph_optimize(*common, n_nodes, m, 5, 0, 1e-6, *tail)
        elif entry == "optimize_robust":
            rc = L.icpmi_pose_graph_optimize_robust(*common, maskp, n_nodes, m, 5, 0, 1e-6, _lib.ROB_KERNEL_HUBER, 2.0, 0,
                                                    _b._ptr(outs[0]), _b._ptr(outs[1]), *tail)
        else:
            rc = L.icpmi_pose_graph_marginals(*common, n_nodes, m, 0, None, 0, _b._ptr(outs[0]), None, 0, *tail)
        torch.cuda.synchronize()
        return rc, int(d_info.cpu()[status_slot])

    def untouched():
        return d_nodes.cpu().numpy().tobytes() == nodes.tobytes() and all(bool((o == 7.0).all()) for o in outs)

    assert call(n, small) == (_lib.OK, _lib.PG_ST_REFUSED)
    assert untouched()
    assert call(1, full) == (_lib.OK, _lib.PG_ST_NOTHING)
    assert untouched()
    rc, status = call(n, full)
    assert rc == _lib.OK and status in (_lib.PG_ST_CONVERGED, _lib.PG_ST_MAXITER), (rc, status)
    assert all(bool(torch.isfinite(o).all()) and not bool((o == 7.0).all()) for o in outs)
    assert entry == "marginals" or d_nodes.cpu().numpy().tobytes() != nodes.tobytes()
