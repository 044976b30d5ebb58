"""Marginals of the pose graph without a GPU: the two entries exist at every layer, the host refuses what it must before
anything is enqueued, the extended-precision helper (tests/pose_graph_marginals_ref.py) is right and its bound leaves
room — LAPACK's float64 inverse is held to it on every case, which is the condition on the inputs — and the host
arithmetic of ``Marginals`` agrees with a long-double evaluation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_graph_marginals_ref as mref
import pose_graph_ref as ref
from conftest import REPO

LD = np.longdouble
HEADER = os.path.join(REPO, "include", "icpmi.h")
ENTRIES = ("icpmi_pose_graph_marginals_workspace_bytes", "icpmi_pose_graph_marginals")
STEP = ref.case_names("step")


def _defines():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return txt, {n: int(v) for n, v in re.findall(r"^#define ICPMI_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}


def test_entries_are_declared_exported_listed_and_bound():
    import icpmi
    from icpmi import _lib
    txt, defines = _defines()
    path = icpmi.build()
    lib = icpmi.lib()                     # torch first, then the library: one HIP runtime in the process
    raw = C.CDLL(path)                    # the same mapping, seen through a plain handle
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/icpmi.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.icpmi_pose_graph_marginals_workspace_bytes.restype is C.c_size_t and len(lib.icpmi_pose_graph_marginals.argtypes) == 16
    marg = {n: v for n, v in defines.items() if n.startswith("MARG_")}
    assert {"MARG_STATUS", "MARG_PATH", "MARG_DOUBLES"} <= set(marg)
    for n, v in marg.items():
        assert getattr(_lib, n) == v, n
    slots = sorted(v for n, v in marg.items() if n not in ("MARG_DOUBLES", "MARG_PATH_SPLIT", "MARG_PATH_DENSE"))
    assert slots == list(range(marg["MARG_DOUBLES"]))                            # every slot of the record has one name
    assert not any(n.startswith(("PG_MARG", "PGINFO_MARG")) for n in defines)


def _tiny():
    """A 6-node chain with one closure, host arrays only."""
    ij = np.ascontiguousarray(np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], dtype=np.int32))
    om = np.ascontiguousarray(np.tile(100.0 * np.eye(3), (len(ij), 1, 1)))
    return ij, om


def test_host_refusals_come_before_any_launch():
    """Fake device pointers: every refusal below is decided on the host, so none of them is ever touched."""
    import icpmi
    _, defines = _defines()
    ERR_ARG, ERR_WORKSPACE = defines["ERR_ARG"], defines["ERR_WORKSPACE"]
    L = icpmi.lib()
    ij, om = _tiny()
    n, m = 6, len(ij)
    ijp, omp = ij.ctypes.data_as(C.c_void_p), om.ctypes.data_as(C.c_void_p)
    fake = [C.c_void_p(0x1000 * (k + 1)) for k in range(7)]
    nodes, z, omega, diag, cols, info, ws = fake
    sel = np.array([0, 5, 5], dtype=np.int32)
    selp = sel.ctypes.data_as(C.c_void_p)
    size = L.icpmi_pose_graph_marginals_workspace_bytes
    need = size(ijp, omp, n, m, 3, 1, 0)
    assert need > 0

    def call(nodes=nodes, ijp=ijp, n=n, m=m, fix=0, selp=selp, s=3, diag=diag, cols=cols, dense=0, info=info, ws=ws, ws_bytes=need):
        return L.icpmi_pose_graph_marginals(nodes, ijp, z, omega, n, m, fix, selp, s, diag, cols, dense, info, ws, ws_bytes, None)

    assert call(nodes=None) == ERR_ARG and call(info=None) == ERR_ARG
    assert call(diag=None, cols=None) == ERR_ARG
    assert call(s=-1) == ERR_ARG and call(selp=None) == ERR_ARG
    assert call(n=-1) == ERR_ARG and call(m=-1) == ERR_ARG and call(ijp=None) == ERR_ARG
    assert call(fix=6) == ERR_ARG and call(fix=-1) == ERR_ARG
    for bad in (6, -1):
        bad_sel = np.array([0, bad, 5], dtype=np.int32)
        assert call(selp=bad_sel.ctypes.data_as(C.c_void_p)) == ERR_ARG
    for bad in ((0, 6), (-1, 2)):
        bad_ij = ij.copy()
        bad_ij[2] = bad
        assert call(ijp=bad_ij.ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert size(bad_ij.ctypes.data_as(C.c_void_p), omp, n, m, 3, 1, 0) == 0
    for dense in (0, 1):
        least = size(ijp, None, n, m, 3, 1, dense)
        assert call(dense=dense, ws=None, ws_bytes=least) == ERR_WORKSPACE
        assert call(dense=dense, ws_bytes=least - 1) == ERR_WORKSPACE and call(dense=dense, ws_bytes=0) == ERR_WORKSPACE
    # the size query: 0 for sizes below zero or edges without a list; more room for more selected nodes and for the diagonal
    assert size(ijp, omp, -1, m, 3, 1, 0) == 0 and size(ijp, omp, n, -1, 3, 1, 0) == 0 and size(ijp, omp, n, m, -1, 1, 0) == 0
    assert size(None, None, n, m, 3, 1, 0) == 0
    for dense in (0, 1):
        assert size(ijp, omp, n, m, 0, 0, dense) < size(ijp, omp, n, m, 1, 0, dense) < size(ijp, omp, n, m, 40, 0, dense)
        assert size(ijp, omp, n, m, 3, 0, dense) < size(ijp, omp, n, m, 3, 1, dense)
    assert size(ijp, omp, n, m, 3, 1, 0) < size(ijp, omp, 60, m, 3, 1, 1)         # the dense path holds two 3n x 3n arrays
    weak = om.copy()
    weak[2] = np.diag([1e-8, 100.0, 100.0])                                       # a weak chain edge: room for its twin
    assert size(ijp, weak.ctypes.data_as(C.c_void_p), n, m, 3, 1, 0) > need == size(ijp, None, n, m, 3, 1, 0)


SMALL = [k for k in STEP if len(ref.cases()[k]["graph"]["nodes"]) <= 9]


@pytest.mark.parametrize("name", SMALL)
def test_reference_inverse_against_long_double_elimination(name):
    """Two routes to H^-1 in long double — Newton on LAPACK's inverse, and plain LU with partial pivoting — agree to what
    long double allows: the form of the float64 bound with long double's unit roundoff, once for each route."""
    r = mref.reference(name)
    X = np.concatenate([r["cols_ld"][w] for w in range(r["n"])], axis=1)
    Y = mref.lu_inverse_ld(r["H"])
    u_ld = float(np.finfo(LD).eps) / 2
    tol = 2 * 3 * r["n"] * r["kappa"] * u_ld * float(np.abs(X).max())
    assert r["last_correction"] < 1e-13
    assert float(np.abs(X - Y).max()) <= tol, (name, float(np.abs(X - Y).max()), tol)
    assert float(np.abs(r["H"] @ X - np.eye(3 * r["n"], dtype=LD)).max()) <= tol * float(np.abs(r["H"]).sum(axis=1).max())


def test_lapack_float64_inverse_is_within_the_bound_on_every_case():
    """The condition on the inputs: a backward-stable float64 inverse of the same H meets the bound the kernels are held
    to, with room, on every case (every block column the reference holds)."""
    worst = {}
    for name in STEP:
        r = mref.reference(name)
        assert r["last_correction"] < 1e-13, (name, r["last_correction"])
        X = np.linalg.inv(np.asarray(r["H"], dtype=np.float64))
        worst[name] = max(mref.worst_ratio(r, {v: X[3 * v:3 * v + 3, 3 * w:3 * w + 3] for v in range(r["n"])}, range(r["n"]), w)
                          for w in r["nodes"])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("LAPACK float64 inverse, error / bound, worst cases: " + ", ".join(f"{k} {v:.3g}" for k, v in top))
    assert max(worst.values()) <= 1.0, top


@pytest.mark.parametrize("name", [k for k in STEP if len(ref.cases()[k]["graph"]["nodes"]) <= mref.FULL_INVERSE_MAX_N])
def test_anchor_is_uncorrelated_in_the_reference(name):
    """H's anchor rows and columns are zero but for 1e10 I: every block of H^-1 between the anchor and another node is 0."""
    r = mref.reference(name)
    f, n = r["fix"], r["n"]
    others = np.ones(3 * n, dtype=bool)
    others[3 * f:3 * f + 3] = False
    assert np.all(r["cols_ld"][f][others] == 0)
    for w in range(n):
        if w != f:
            assert np.all(r["cols_ld"][w][3 * f:3 * f + 3] == 0), (name, w)
    assert float(np.abs(r["cols_ld"][f][3 * f:3 * f + 3] - np.eye(3, dtype=LD) / LD(1e10)).max()) <= 1e-10 * 2.0 ** -60


def test_marginals_host_arithmetic_against_long_double():
    """block / joint / relative on hand-made blocks.  relative is J S J^T with J = [A B] (3 x 6) and S the 6 x 6 joint:
    two products of 6 terms each way, held entrywise to 32 * 2^-53 |J| |S| |J|^T against the same product in long double;
    the Jacobians themselves against tests/pose_graph_ref.linearise_ld."""
    from utilities.pose_graph import Marginals
    rng = np.random.default_rng(11)
    n = 7
    poses = np.column_stack([rng.normal(0, 30, n), rng.normal(0, 30, n), rng.uniform(-np.pi, np.pi, n)])
    sel = [5, 1, 5, 3]
    diagonal = rng.normal(size=(n, 3, 3))
    columns = rng.normal(size=(len(sel), n, 3, 3)) * 10.0 ** rng.integers(-6, 3, size=(len(sel), n, 1, 1))
    columns[2] = columns[0]
    m = Marginals(poses, 0, sel, diagonal, columns, 1, "split")
    assert np.array_equal(m.block(2, 5), columns[0, 2]) and np.array_equal(m.block(-1, 1), columns[1, 6])
    assert np.array_equal(m.block(4, 4), diagonal[4]) and np.array_equal(m.block(3, 3), columns[3, 3])
    with pytest.raises(KeyError):
        m.block(1, 2)
    with pytest.raises(KeyError):
        m.joint(1, 2)
    with pytest.raises(IndexError):
        m.block(7, 5)
    for i, j in ((1, 5), (5, 3), (3, 3), (-2, 1)):
        ii, jj = i % n, j % n
        S = m.joint(i, j)
        want = np.block([[columns[sel.index(ii), ii], columns[sel.index(jj), ii]], [columns[sel.index(ii), jj], columns[sel.index(jj), jj]]])
        assert S.shape == (6, 6) and np.array_equal(S, want)
        A, B = m.relative_jacobians(i, j)
        _, A_ld, B_ld = ref.linearise_ld(poses, np.array([ii]), np.array([jj]), np.zeros((1, 3)))
        scale = 4 * ref.U * (1.0 + float(np.abs(poses[:, :2]).max()) * 2)                     # cos, sin and one difference times them
        assert float(np.abs(A - A_ld[0]).max()) <= scale and float(np.abs(B - B_ld[0]).max()) <= scale
        J = np.hstack([A, B])
        exact = np.asarray(J, dtype=LD) @ np.asarray(S, dtype=LD) @ np.asarray(J, dtype=LD).T
        tol = 32 * ref.U * (np.abs(J) @ np.abs(S) @ np.abs(J).T)
        got = m.relative(i, j)
        assert got.shape == (3, 3) and np.all(np.abs(got - exact) <= tol), (i, j)
    only_diag = Marginals(poses, 0, [], diagonal, None, 1, "dense")
    assert np.array_equal(only_diag.block(2, 2), diagonal[2])
    with pytest.raises(KeyError):
        only_diag.relative(1, 2)
