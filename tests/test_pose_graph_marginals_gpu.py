"""Marginals of the pose graph (icpmi_pose_graph_marginals, csrc/posegraph.hip) against extended precision.

Blocks of H^-1, H the matrix the reference's optimize assembles, against the long-double inverse of
tests/pose_graph_marginals_ref.py within ``bound`` — what a backward-stable float64 solve of H X = E owes a block column,
3n kappa 2^-53 max |column|; nothing measured on the kernels — on the step cases of tests/pose_graph_ref.py: one and two
levels of the chain, more nodes than threads, a closure system wider than 512, both dense cases, non-symmetric and
indefinite information, the branch cut, the 1e5 offset and every weak-chain case.
tests/test_pose_graph_marginals_cpu.py holds LAPACK's float64 inverse to the same bound on the same cases.
"""
import numpy as np
import pytest

import pose_graph_marginals_ref as mref
import pose_graph_ref as ref

pytestmark = pytest.mark.gpu

STEP, SINGULAR = ref.case_names("step"), ref.case_names("singular")
# no chain numbering (permuted), a gap in the chain, or a chain edge without information along some direction (the plan refuses)
DENSE = {"dense_540", "dense_540_gap", "info_indef_dense", "weak_eps1e-12", "weak_eps0", "weak_zero_matrix", "weak_last_node"}
FORCE_DENSE_MAX_N = 33


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


def _check(name, what, r, m, sel):
    """Every known block of ``m`` within its bound; the worst error / bound of the diagonal and of the columns."""
    n, fix = r["n"], r["fix"]
    assert m.diagonal.shape == (n, 3, 3) and m.columns.shape == (len(sel), n, 3, 3) and m.nodes == sel
    diag = max(mref.worst_ratio(r, m.diagonal, [v], v) for v in r["nodes"])
    cols = max(mref.worst_ratio(r, m.columns[a], range(n), w) for a, w in enumerate(sel))
    print(f"{name} [{what}, {m.path}]: n {n} kappa {r['kappa']:.2e} error/bound diagonal {diag:.3e} columns {cols:.3e}")
    assert diag <= 1.0, (name, what, diag)
    assert cols <= 1.0, (name, what, cols)
    assert np.array_equal(m.columns[3], m.columns[4]), name                       # the selection's duplicate
    for a, w in enumerate(sel):                                                   # the anchor is uncorrelated with every other node
        others = np.arange(n) != fix
        if w == fix:
            assert np.all(m.columns[a][others] == 0.0), (name, what, a)
        else:
            assert np.all(m.columns[a][fix] == 0.0), (name, what, a)


@pytest.mark.parametrize("name", STEP)
def test_marginals_against_extended_precision(upg, name):
    c = ref.cases()[name]
    g, r = c["graph"], mref.reference(name)
    assert r["last_correction"] < 1e-13, (name, r["last_correction"])
    n, fix = r["n"], r["fix"]
    sel = mref.selection(n, fix)
    pg = _graph(upg, g)
    m = pg.marginals(nodes=sel, fix_node=fix)
    assert np.array_equal(np.array(pg.nodes), g["nodes"]), name                   # nothing is iterated
    assert m.status == upg.CONVERGED and m.path == ("dense" if name in DENSE else "split"), (name, m.status, m.path)
    _check(name, "both outputs", r, m, sel)
    again = pg.marginals(nodes=sel, fix_node=fix)                                 # fixed summation orders: bit-identical
    assert np.array_equal(again.diagonal, m.diagonal) and np.array_equal(again.columns, m.columns), name
    if m.path == "split" and n <= FORCE_DENSE_MAX_N:
        d = pg.marginals(nodes=sel, fix_node=fix, force_dense=True)
        assert d.status == upg.CONVERGED and d.path == "dense", (name, d.status, d.path)
        _check(name, "forced dense", r, d, sel)


@pytest.mark.parametrize("name", SINGULAR)
def test_singular_raises(upg, name):
    c = ref.cases()[name]
    pg = _graph(upg, c["graph"])
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        pg.marginals(nodes=[0], fix_node=c["fix"])
    assert np.array_equal(np.array(pg.nodes), c["graph"]["nodes"]), name


def test_each_output_alone_and_the_accessors(upg):
    name = "cr_n9_fix4"
    c = ref.cases()[name]
    r, pg = mref.reference(name), _graph(upg, c["graph"])
    both = pg.marginals(nodes=[-1, 2, 4], fix_node=c["fix"])
    assert both.nodes == [8, 2, 4]                                                # Python's negative index
    only_diag = pg.marginals(fix_node=c["fix"])
    only_cols = pg.marginals(nodes=[-1, 2, 4], fix_node=c["fix"], diagonal=False)
    assert only_diag.columns is None and only_cols.diagonal is None
    for v in range(9):
        assert mref.worst_ratio(r, only_diag.diagonal, [v], v) <= 1.0
    for a, w in enumerate([8, 2, 4]):
        assert mref.worst_ratio(r, only_cols.columns[a], range(9), w) <= 1.0
    assert np.array_equal(both.block(3, 8), both.columns[0, 3]) and np.array_equal(only_diag.block(3, 3), only_diag.diagonal[3])
    j = both.joint(2, 8)
    assert j.shape == (6, 6) and np.array_equal(j[:3, 3:], both.columns[0, 2]) and np.array_equal(j[3:, :3], both.columns[1, 8])
    assert both.relative(2, 8).shape == (3, 3)
    with pytest.raises(KeyError):
        only_diag.block(3, 8)
    with pytest.raises(KeyError):
        both.joint(2, 5)
    empty = upg.PoseGraph2D()
    empty.add_node([0.0, 0.0, 0.0])
    assert empty.marginals() is None                                              # as optimize: nothing to do
