"""The information matrix of an ICP result, host side (no GPU): the header, the library and the loader agree on
icpmi_icp_information_batch; ``edge_information`` is the first-order map it claims to be; ``residual_variance`` refuses what
has no degrees of freedom; ``constraint_spectrum`` finds the free direction of a corridor; the example's default is the
reference's isotropic weighting."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "icpmi.h")


def test_header_library_and_loader_agree():
    import icpmi
    from icpmi import _lib
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+icpmi_icp_information_batch\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/icpmi.h does not declare icpmi_icp_information_batch"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const double* pts", "const int32_t* off_dev", "const int32_t* cnt_dev", "const double* normals",
                      "const int32_t* pair_src", "const int32_t* pair_tgt", "int32_t n_pairs", "int32_t max_src_n",
                      "const double* transforms", "int32_t method", "double max_corr_dist", "double* out", "void* stream"]
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(INFO_\w+)[ \t]+(\d+)[ \t]*$", txt, flags=re.M)}
    assert defines == dict(INFO_DOUBLES=16, INFO_H=0, INFO_G=6, INFO_SSE=9, INFO_INLIERS=10, INFO_ROWS=11, INFO_STATUS=12,
                           INFO_THREADS=defines["INFO_THREADS"], INFO_TILE_ROWS=defines["INFO_TILE_ROWS"])
    for n, v in defines.items():
        assert getattr(_lib, n) == v, n
    assert defines["INFO_THREADS"] % 64 == 0 and defines["INFO_TILE_ROWS"] % 16 == 0
    assert len(_lib.INFO_SLOTS) == 13 and _lib.INFO_SLOTS[_lib.INFO_SSE] == "sse" and _lib.INFO_SLOTS[_lib.INFO_STATUS] == "status"
    # the moved row is stated in the header, so that a test can reproduce its bits
    assert "(R00 * sx + R01 * sy) + tx" in raw and "(R10 * sx + R11 * sy) + ty" in raw and "icp.py:92-104" in raw
    path = icpmi.build()
    assert hasattr(icpmi.lib(), "icpmi_icp_information_batch")       # (torch first, then the library: one HIP runtime)
    assert hasattr(ctypes.CDLL(path), "icpmi_icp_information_batch") and "icpmi_icp_information_batch" in _lib.EXPORTS
    res, args = _lib._SIGS["icpmi_icp_information_batch"]
    V, I, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert res is ctypes.c_int and args == [V, V, V, V, V, V, I, I, V, I, D, V, V] and len(args) == 13


def test_entry_point_refuses_on_the_host():
    """Decided before any launch, so no GPU is touched (the pointers are fakes that are never read)."""
    import icpmi
    from icpmi import _lib
    icpmi.build()
    L = icpmi.lib()
    f = L.icpmi_icp_information_batch
    p = ctypes.c_void_p(4096)
    ok = (p, p, None, p, p, p, 1, 10, p, _lib.POINT_TO_LINE, -1.0, p, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    assert call(a9=2) == -4 and call(a9=-1) == -4                               # not one of the two methods: unsupported
    assert call(a6=-1) == -1 and call(a7=-1) == -1                              # negative counts
    assert call(a6=0) == 0 and call(a6=0, a0=None) == 0                         # nothing to do: no launch, nothing read
    assert call(a3=None) == -1                                                  # point_to_line without normals
    for k in (0, 1, 4, 5, 8, 11):
        assert call(**{f"a{k}": None}) == -1, k
    assert call(a10=float("nan")) == -1


def test_lazy_exports():
    import icpmi
    from icpmi import information
    for name in ("information_set", "icp_information", "unpack_information", "edge_information", "residual_variance",
                 "constraint_spectrum"):
        assert getattr(icpmi, name) is getattr(information, name)
    assert icpmi.information is information
    from icpmi.batch import IcpBatch
    from icpmi.prealign import RunIcpPairBatch
    from icpmi.history import HistoryMatch, _ResidentIcp
    assert callable(IcpBatch.information) and _ResidentIcp.information is IcpBatch.information
    assert callable(RunIcpPairBatch.information) and HistoryMatch.information is RunIcpPairBatch.information


def _D(delta):
    th, tx, ty = delta
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s, tx], [s, c, ty], [0.0, 0.0, 1.0]])


def _G(R):
    return -np.array([[0.0, 0.0, 1.0], [R[0, 0], R[0, 1], 0.0], [R[1, 0], R[1, 1], 0.0]])


def test_edge_information_is_the_first_order_map():
    """z = pose_matrix_to_vec(inv(T)); z + h e corresponds to D(G h e) T up to second order: halving h divides the
    mismatch by 4 (3.5 .. 4.5: the next term is O(h) relative), and at h = 0 nothing is left at all.  The bounds follow
    from the order of the error term; nothing is measured."""
    from icpmi.information import edge_information
    from utilities.pose_graph import pose_matrix_to_vec, pose_vec_to_matrix
    rng = np.random.default_rng(0)
    for trial in range(20):
        z = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-3, 3)])
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)

        def T_of(h):
            return np.linalg.inv(pose_vec_to_matrix(z + h * e))

        T = T_of(0.0)
        assert np.allclose(pose_matrix_to_vec(np.linalg.inv(T)), z, atol=1e-12)
        G = _G(T[:2, :2])

        def mismatch(h):
            return float(np.linalg.norm(T_of(h) - _D(G @ (h * e)) @ T))

        assert mismatch(0.0) == 0.0
        m1, m2 = mismatch(1e-3), mismatch(5e-4)
        assert m1 > 1e-9, (trial, m1)                   # a generic direction does have a second-order term (rounding is ~1e-15)
        assert 3.5 < m1 / m2 < 4.5, (trial, m1, m2)
        # and the matrix the function applies is this G
        H = rng.normal(size=(3, 3))
        H = H @ H.T
        assert np.allclose(edge_information(H, T[:2, :2], 1.0), G.T @ H @ G, rtol=0, atol=1e-12 * np.abs(H).max())


def test_edge_information_is_symmetric_psd_and_reorders_at_identity():
    from icpmi.information import edge_information
    rng = np.random.default_rng(1)
    for trial in range(20):
        A = rng.normal(size=(int(rng.integers(1, 40)), 3)) * rng.uniform(0.1, 10.0, size=3)
        H = A.T @ A
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        sigma2 = rng.uniform(1e-4, 1.0)
        om = edge_information(H, R, sigma2)
        assert om.shape == (3, 3) and np.array_equal(om, om.T)
        lam = np.linalg.eigvalsh(om)
        assert lam.min() >= -1e-12 * max(lam.max(), 1.0), lam       # eigvalsh is backward stable: an error of a few ulp of |om|
        # x^T Omega x = |A G x|^2 / sigma2: the quadratic form of the residual rows themselves
        x = rng.normal(size=3)
        assert np.isclose(x @ om @ x, np.sum((A @ (_G(R) @ x)) ** 2) / sigma2, rtol=1e-10)
        # at R = I the map only moves theta last (and flips all three signs, which a quadratic form does not see)
        perm = [1, 2, 0]
        assert np.allclose(edge_information(H, np.eye(2), 1.0), H[np.ix_(perm, perm)], rtol=0, atol=1e-13 * np.abs(H).max())
    assert np.array_equal(edge_information(np.diag([1.0, 2.0, 3.0]), np.eye(2), 1.0), np.diag([2.0, 3.0, 1.0]))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            edge_information(np.eye(3), np.eye(2), bad)
    with pytest.raises(ValueError):
        edge_information(np.eye(2), np.eye(2), 1.0)


def test_residual_variance_refuses_without_degrees_of_freedom():
    from icpmi.information import residual_variance
    info = dict(sse=0.5, inliers=3)
    with pytest.raises(ValueError):
        residual_variance(info, "point_to_line")                    # 3 residuals, 3 unknowns
    with pytest.raises(ValueError):
        residual_variance(dict(sse=0.5, inliers=3))                 # point_to_line is the default
    with pytest.raises(ValueError):
        residual_variance(dict(sse=0.5, inliers=1), "point_to_point")   # 2 residuals
    with pytest.raises(ValueError):
        residual_variance(dict(sse=0.5, inliers=0, method="point_to_point"))
    assert residual_variance(dict(sse=0.5, inliers=4), "point_to_line") == 0.5
    assert residual_variance(dict(sse=0.5, inliers=2), "point_to_point") == 0.5
    assert residual_variance(dict(sse=3.0, inliers=5, method="point_to_point")) == 3.0 / 7
    assert residual_variance(dict(sse=3.0, inliers=5, method="point_to_point"), "point_to_line") == 1.5
    with pytest.raises(ValueError):
        residual_variance(dict(sse=1.0, inliers=10), "plane")


def test_unpack_information_layout():
    from icpmi import _lib
    from icpmi.information import unpack_information
    rec = np.arange(32.0).reshape(2, 16)
    u = unpack_information(rec)
    assert np.array_equal(u["H"][0], [[0, 1, 2], [1, 3, 4], [2, 4, 5]]) and np.array_equal(u["H"][1], u["H"][1].T)
    assert np.array_equal(u["g"], [[6, 7, 8], [22, 23, 24]]) and list(u["sse"]) == [9, 25]
    assert list(u["inliers"]) == [10, 26] and list(u["rows"]) == [11, 27] and list(u["status"]) == [12, 28]
    assert u["inliers"].dtype == np.int64
    one = unpack_information(rec[1])
    assert one["H"].shape == (3, 3) and one["sse"] == 25.0 and one["status"] == 28
    assert _lib.INFO_DOUBLES == 16


def test_constraint_spectrum_of_a_corridor():
    """Rows whose normals are all parallel (two walls of a corridor along the direction w): nothing constrains a
    translation along w.  One eigenvalue of the scaled Hessian is zero to rounding; its eigenvector has no theta component
    and its translation part points along the walls."""
    from icpmi.information import constraint_spectrum
    rng = np.random.default_rng(2)
    for ang in (0.0, 0.4, 1.3, -2.0):
        w = np.array([np.cos(ang), np.sin(ang)])
        n = np.array([-w[1], w[0]])
        s = rng.uniform(-8, 8, size=200)
        side = np.where(rng.random(200) < 0.5, 1.0, -1.0)
        p = s[:, None] * w + (side * 1.1)[:, None] * n + rng.normal(scale=0.01, size=(200, 2))
        nrm = np.tile(n, (200, 1)) * side[:, None]                       # both signs: immaterial
        A = np.column_stack([nrm[:, 1] * p[:, 0] - nrm[:, 0] * p[:, 1], nrm[:, 0], nrm[:, 1]])
        H = A.T @ A
        lam, V = constraint_spectrum(H)
        assert lam.shape == (3,) and np.all(np.diff(lam) >= 0)
        d = np.sqrt(np.diag(H))
        assert np.isclose(lam.sum(), np.count_nonzero(d), rtol=1e-12)    # unit diagonal (a wall along x leaves H_xx = 0 as it is)
        assert abs(lam[0]) < 1e-12 * lam[-1], lam
        v = V[:, 0]
        x = v / np.where(d > 0, d, 1.0)                                                     # back to [theta, tx, ty] units: H x = 0
        x /= np.linalg.norm(x[1:])
        assert abs(x[0]) < 1e-9, x
        assert abs(abs(x[1:] @ w) - 1.0) < 1e-9, (x, w)
    # a room (normals in every direction) has no such direction
    th = rng.uniform(-np.pi, np.pi, size=200)
    nrm = np.column_stack([np.cos(th), np.sin(th)])
    p = rng.uniform(-5, 5, size=(200, 2))
    A = np.column_stack([nrm[:, 1] * p[:, 0] - nrm[:, 0] * p[:, 1], nrm[:, 0], nrm[:, 1]])
    lam, _ = constraint_spectrum(A.T @ A)
    assert lam[0] / lam[-1] > 0.1


def test_example_defaults_to_the_isotropic_weighting():
    spec = importlib.util.spec_from_file_location("slam_loop", os.path.join(REPO, "examples", "slam_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert inspect.signature(m.run).parameters["edge_information"].default == "isotropic"
    assert m.EDGE_INFORMATION == ("isotropic", "icp")
    with pytest.raises(ValueError, match="edge_information must be one of"):
        m.run(3, verbose=False, edge_information="anisotropic")

    class NoCalls:                        # a backend without the calls is refused before anything runs
        pass
    with pytest.raises(ValueError, match="needs a backend with icp_information"):
        m.run(3, verbose=False, edge_information="icp", backend=NoCalls)
    for name in ("icp_information", "History", "match_history_information"):
        assert hasattr(m.GpuBackend, name)
    # edge_omega keeps the isotropic weight (None) for a record that cannot give one
    assert m.edge_omega(None, np.eye(2)) is None
    assert m.edge_omega(dict(status=3, H=np.eye(3), sse=1.0, inliers=50), np.eye(2)) is None
    assert m.edge_omega(dict(status=0, H=np.eye(3), sse=1.0, inliers=3), np.eye(2)) is None
    om = m.edge_omega(dict(status=0, H=np.diag([1.0, 2.0, 3.0]), sse=0.0, inliers=50), np.eye(2), 10.0)
    assert np.allclose(om, np.diag([2.0, 3.0, 1.0]) * 10.0 / 1e-6, rtol=1e-14, atol=0)   # sigma2 floored at 1e-6
