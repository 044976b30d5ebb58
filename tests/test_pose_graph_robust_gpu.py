"""The robust pose-graph optimiser (icpmi_pose_graph_optimize_robust, csrc/posegraph.hip) against extended precision.

Every reference and bound comes from tests/pose_graph_robust_ref.py (long double; tests/test_pose_graph_robust_cpu.py
holds a NumPy float64 restatement to the same bounds on the same cases).  Where the loss never leaves the quadratic the
robust kernel must return the plain kernel's bits: it is the same iteration with the same summation orders."""
import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_robust_ref as rref

pytestmark = pytest.mark.gpu

CASES = sorted(rref.cases())
MULTI = [k for k in CASES if rref.cases()[k]["multi"]]
# split, twins, dense (a numbering optimize cannot split either), refused-then-dense
EQUAL = ["n3_one_closure", "n65_false_closure", "n200_chain_three_times", "weak_twins", "n33_permuted", "weak_refused"]


@pytest.fixture(scope="module")
def upg():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import pose_graph
    pose_graph.VERBOSE = False
    return pose_graph


def _graph(upg, g, weights=None):
    pg = upg.PoseGraph2D()
    for v in g["nodes"]:
        pg.add_node(v)
    for q, (i, j, z, om) in enumerate(zip(g["ei"], g["ej"], g["z"], g["omega"])):
        pg.add_edge(int(i), int(j), z, om if weights is None else om * weights[q])
    return pg


def _worst_ratio(err, bound):
    """max |err| / bound for printing, over the entries whose bound is not 0 (an edge without information, an unmasked edge's weight)."""
    some = bound > 0
    return float((np.abs(err)[some] / bound[some]).max()) if some.any() else 0.0


@pytest.mark.parametrize("name", CASES)
def test_evaluation_only(upg, name):
    c = rref.cases()[name]
    g = c["graph"]
    for kernel in rref.KERNELS:
        ev = rref.evaluation(name, kernel)
        pg = _graph(upg, g)
        cost, chi2, w = pg.robust_cost(kernel, rref.DELTA, edges=c["mask"])
        e_chi2 = _worst_ratio(chi2 - np.asarray(ev["chi2"], dtype=np.float64), ev["chi2_bound"])
        e_w = _worst_ratio(w - np.asarray(ev["w"], dtype=np.float64), ev["w_bound"])
        print(f"{name} {kernel}: chi2 error/bound {e_chi2:.3e} weight error/bound {e_w:.3e} "
              f"cost {cost!r} reference {ev['cost']!r} error/bound {abs(cost - ev['cost']) / ev['cost_bound']:.3e}")
        assert np.all(np.abs(chi2 - np.asarray(ev["chi2"], dtype=np.float64)) <= ev["chi2_bound"]), (name, kernel)
        assert np.all(np.abs(w - np.asarray(ev["w"], dtype=np.float64)) <= ev["w_bound"]), (name, kernel)
        assert np.all(w[~c["mask"]] == 1.0) and np.all((w > 0) & (w <= 1)), (name, kernel)
        assert abs(cost - ev["cost"]) <= ev["cost_bound"], (name, kernel, cost, ev["cost"])
        assert np.array_equal(np.array(pg.nodes), g["nodes"]), name                  # nothing moved, to the bit


@pytest.mark.parametrize("name", CASES)
def test_one_step_against_extended_precision(upg, name):
    c = rref.cases()[name]
    g = c["graph"]
    for kernel in rref.KERNELS:
        run = rref.run(name, kernel, 1, 0.0)
        want = ref.step_difference(np.asarray(run["iterates"][0], dtype=np.float64), g["nodes"])
        pg = _graph(upg, g)
        pg.optimize_robust(n_iterations=1, fix_node=c["fix"], convergence_eps=0.0, kernel=kernel, delta=rref.DELTA, edges=c["mask"])
        info = pg.last_info
        err = float(np.abs(ref.step_difference(np.array(pg.nodes), g["nodes"]) - want).max())
        print(f"{name} {kernel}: bound {run['bounds'][0]:.3e} error/bound {err / run['bounds'][0]:.3e} path {info['path']} "
              f"split refused at {info['split_refused_at']} weights {info['weights_us']:.1f} us")
        assert (info["status"], info["iterations"]) == (upg.MAX_ITERATIONS, 1), (name, kernel, info)
        assert err <= run["bounds"][0], (name, kernel, err, run["bounds"][0])
        assert abs(info["step_norm"] - run["steps"][0]) <= run["bounds"][0] * np.sqrt(3 * len(g["nodes"])), (name, kernel)
        assert info["path"] == c["path"] and (info["split_refused_at"] == 0) == c["refused"], (name, info)
        ev = rref.evaluation(name, kernel)
        assert abs(info["cost_before"] - ev["cost"]) <= ev["cost_bound"], (name, kernel)


@pytest.mark.parametrize("name", EQUAL)
def test_a_quadratic_loss_is_optimize_to_the_bit(upg, name):
    """Huber with delta = 1e150 never leaves its quadratic part, and an empty mask leaves no robust edge: every weight is
    exactly 1.0, so nodes and step_norm are those of ``optimize`` — the same sums in the same order."""
    c = rref.cases()[name]
    g = c["graph"]
    kw = dict(n_iterations=4, fix_node=c["fix"], convergence_eps=1e-9)
    plain = _graph(upg, g)
    plain.optimize(**kw)
    m = len(g["ei"])
    runs = [("huber", dict(delta=1e150, edges=c["mask"]))] + [(k, dict(delta=rref.DELTA, edges=np.zeros(m, dtype=bool))) for k in rref.KERNELS]
    for kernel, more in runs:
        pg = _graph(upg, g)
        pg.optimize_robust(kernel=kernel, **kw, **more)
        assert np.all(pg.last_robust["weights"] == 1.0), (name, kernel)
        assert (pg.last_info["status"], pg.last_info["iterations"]) == (plain.last_info["status"], plain.last_info["iterations"])
        assert pg.last_info["path"] == c["path"], (name, kernel)
        assert np.array_equal(np.array(pg.nodes), np.array(plain.nodes)), (name, kernel)
        assert pg.last_info["step_norm"] == plain.last_info["step_norm"], (name, kernel)
        assert pg.last_info["split_refused_at"] == plain.last_info["split_refused_at"], (name, kernel)
        assert pg.last_info["cost_after"] <= pg.last_info["cost_before"], (name, kernel)


@pytest.mark.parametrize("kernel", rref.KERNELS)
@pytest.mark.parametrize("name", MULTI)
def test_several_iterations(upg, name, kernel):
    c = rref.cases()[name]
    g = c["graph"]
    run = rref.run(name, kernel, c["multi"]["n_iterations"], c["multi"]["eps"])
    kw = dict(n_iterations=c["multi"]["n_iterations"], fix_node=c["fix"], convergence_eps=c["multi"]["eps"], kernel=kernel,
              delta=rref.DELTA, edges=c["mask"])
    pg = _graph(upg, g)
    pg.optimize_robust(**kw)
    out, info, fin = np.array(pg.nodes), pg.last_info, run["final"]
    err = float(np.abs(ref.step_difference(out, np.asarray(run["iterates"][-1], dtype=np.float64))).max())
    bound = sum(run["bounds"])
    e_w = np.abs(pg.last_robust["weights"] - np.asarray(fin["w"], dtype=np.float64))
    print(f"{name} {kernel}: bound {bound:.3e} error/bound {err / bound:.3e} weights error/bound "
          f"{_worst_ratio(e_w, fin['w_bound']):.3e} cost {info['cost_before']:.6g} -> {info['cost_after']:.6g} "
          f"(reference {run['costs'][0]:.6g} -> {fin['cost']:.6g}) status {info['status']} iterations {info['iterations']} path {info['path']}")
    assert (info["status"], info["iterations"]) == (run["status"], run["iterations"]), (name, kernel, info)
    assert err <= bound, (name, kernel, err, bound)
    assert info["path"] == c["path"]
    assert np.all(e_w <= fin["w_bound"]), (name, kernel)
    assert np.all(np.abs(pg.last_robust["chi2"] - np.asarray(fin["chi2"], dtype=np.float64)) <= fin["chi2_bound"]), (name, kernel)
    assert abs(info["cost_after"] - fin["cost"]) <= fin["cost_bound"], (name, kernel)
    assert info["cost_after"] <= info["cost_before"], (name, kernel, info)
    assert np.array_equal(pg.last_robust["mask"], c["mask"]) and pg.last_robust["kernel"] == kernel
    again = _graph(upg, g)
    again.optimize_robust(**kw)
    assert np.array_equal(np.array(again.nodes), out), (name, kernel)               # fixed summation orders: bit-identical
    assert again.last_info["step_norm"] == info["step_norm"] and again.last_info["cost_after"] == info["cost_after"]
    assert np.array_equal(again.last_robust["weights"], pg.last_robust["weights"])


def test_default_mask_is_every_edge_between_nodes_that_are_not_consecutive(upg):
    g = rref.cases()["n33_false_closure"]["graph"]
    pg = _graph(upg, g)
    _, _, w_default = pg.robust_cost("cauchy", rref.DELTA)
    _, _, w_mask = pg.robust_cost("cauchy", rref.DELTA, edges=rref.default_mask(g))
    _, _, w_index = pg.robust_cost("cauchy", rref.DELTA, edges=[int(q) for q in np.flatnonzero(rref.default_mask(g))])
    assert np.array_equal(w_default, w_mask) and np.array_equal(w_default, w_index) and np.any(w_default < 1)
    with pytest.raises(ValueError):
        pg.optimize_robust(kernel="tukey")
    with pytest.raises(ValueError):
        pg.optimize_robust(delta=0.0)
    with pytest.raises(IndexError):
        pg.robust_cost("huber", 1.0, edges=[len(g["ei"])])


def test_marginals_with_edge_weights(upg):
    """marginals(edge_weights=w) is the marginals of the graph whose information matrices are Omega w, to the bit; without
    the argument, and with weights of 1.0, nothing changes."""
    c = rref.cases()["scenario_false_closure"]
    g = c["graph"]
    pg = _graph(upg, g)
    pg.optimize_robust(n_iterations=8, kernel="cauchy")
    w = pg.last_robust["weights"]
    assert np.any(w < 1)
    got = pg.marginals(nodes=[5, 39], edge_weights=w)
    twin = _graph(upg, dict(g, nodes=np.array(pg.nodes)), weights=w)
    want = twin.marginals(nodes=[5, 39])
    assert np.array_equal(got.diagonal, want.diagonal) and np.array_equal(got.columns, want.columns)
    plain = _graph(upg, dict(g, nodes=np.array(pg.nodes))).marginals(nodes=[5, 39])
    same = pg.marginals(nodes=[5, 39])
    ones = pg.marginals(nodes=[5, 39], edge_weights=np.ones(len(w)))
    for other in (same, ones):
        assert np.array_equal(other.diagonal, plain.diagonal) and np.array_equal(other.columns, plain.columns)
    assert not np.array_equal(got.diagonal, plain.diagonal)
    with pytest.raises(ValueError):
        pg.marginals(edge_weights=w[:-1])
