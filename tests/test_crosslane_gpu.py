"""The cross-lane reductions of csrc/common.hpp (DPP moves inside the 16-lane rows, permlane swaps across them) through the
kernels that use them, at the smallest shapes where a wrong lane or a wrong row would show: the voxel filter (wave_min /
wave_max of the bounds, the wave scan of block_exscan), prepare_targets (the same min / max in choose_axis, wave_sum of the
bin costs, the scan of the grid build) and the fused ICP (row_sum in wave_totals, the wave maximum of the staging).

The clouds lie on a fixed, sheared lattice.  The unique minimum and the unique maximum of x and of y are moved through rows
0, 15, 16, 31, 32, 47, 48, 63, 64, 511, 512 and 1 023 (those a cloud has): every DPP row, both halves of a wave, a first
and a last wave hold each extreme once.  A bound taken from the wrong lane moves every voxel key and every grid cell.

Everything against the project's oracle: the voxel filter bit for bit, the normals to the bound of test_normals_sizes
(tests/test_gpu_parity.py), the sorted copy against its restatement here (rows in (key, row) order), the registrations to
FRO_TOL with equal iteration counts."""
import numpy as np
import pytest

import oracle
from conftest import rot_err

pytestmark = pytest.mark.gpu

FRO_TOL = 1e-9                  # tests/test_gpu_parity.py, the fast path
NORMALS_TOL = 1e-9              # test_normals_sizes, test_prepare_layout_switches
SIZES = (1, 63, 64, 65, 513, 1024)
ROWS = (0, 15, 16, 31, 32, 47, 48, 63, 64, 511, 512, 1023)
VOXEL = 0.12                    # a few lattice sites per voxel: the means depend on which rows share a key
NORMAL_K = 12
# lattice: site (i, j) at (0.05 i + 0.011 j, 0.035 j) + origin — sheared and anisotropic, so that no neighbourhood is
# isotropic (its normal would be undefined); 48 x 40 sites, taken in a fixed pseudo-random order
LAT_NI, LAT_NJ = 48, 40
ORIGIN = np.array([1.013, -0.687])


def _site(i, j):
    return np.array([0.05 * i + 0.011 * j, 0.035 * j]) + ORIGIN


def _lattice(n, seed=0):
    order = np.random.default_rng(seed).permutation(LAT_NI * LAT_NJ)[:n]
    i, j = order % LAT_NI, order // LAT_NI
    return np.column_stack([0.05 * i + 0.011 * j, 0.035 * j]) + ORIGIN


def extreme_clouds():
    """[(label, cloud)]: per size and per row r_j of ROWS the cloud has, the lattice cloud with the unique min x in row r_j,
    the unique max x in r_(j+1), the unique min y in r_(j+2) and the unique max y in r_(j+3) (cyclically; one row holds them
    all where the cloud has a single point).  The extremes are lattice sites outside the box of the others."""
    out = []
    for n in SIZES:
        base = _lattice(n)
        rows = [r for r in ROWS if r < n]
        for j in range(len(rows)):
            c = base.copy()
            r = [rows[(j + q) % len(rows)] for q in range(4)]
            if n > 1:
                c[r[0]] = _site(-6, 20)                    # min x (y inside)
                c[r[1]] = _site(LAT_NI + 14, 21)           # max x
                c[r[2]] = _site(20, -5)                    # min y
                c[r[3]] = _site(21, LAT_NJ + 4)            # max y
            out.append((f"n{n}_r{'_'.join(str(q) for q in r)}", c))
    return out


def test_the_clouds_have_their_property():
    clouds = extreme_clouds()
    assert len(clouds) == 1 + 7 + 8 + 9 + 11 + 12
    seen = {n: [set(), set(), set(), set()] for n in SIZES}
    for label, c in clouds:
        n = len(c)
        if n == 1:
            continue
        for q, (col, f) in enumerate(((0, np.argmin), (0, np.argmax), (1, np.argmin), (1, np.argmax))):
            v = c[:, col]
            at = int(f(v))
            assert (v == v[at]).sum() == 1, (label, q)                 # unique
            seen[n][q].add(at)
    for n in SIZES[1:]:
        want = {r for r in ROWS if r < n}
        assert all(s == want for s in seen[n]), n                      # every extreme in every row


# ── voxel filter ────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def voxel_ref():
    return [oracle.voxel_downsample(c, VOXEL) for _, c in extreme_clouds()]


@pytest.mark.parametrize("copies", [1, 6], ids=["1024_threads", "512_threads"])
def test_voxel_filter_bit_equal(voxel_ref, copies):
    """All clouds as one set: 48 clouds run on 1 024 threads a workgroup, 288 on 512 (the launch of a large batch)."""
    from icpmi import batch
    clouds = [c for _, c in extreme_clouds()] * copies
    out = batch.voxel_downsample_set(batch.CloudSet.from_numpy(clouds), VOXEL).to_numpy()
    assert len(out) == len(clouds)
    labels = [l for l, _ in extreme_clouds()] * copies
    for i, o in enumerate(out):
        w = voxel_ref[i % len(voxel_ref)]
        assert o.shape == w.shape and np.array_equal(o, w), (copies, labels[i])


# ── prepare_targets ─────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def normals_ref():
    return [oracle.normals_2d(c, NORMAL_K) for _, c in extreme_clouds()]


def _prepare(clouds, k):
    """icpmi_prepare_targets_ex over the set -> (normals in row order, sorted xy, sorted->row map, bearing keys, axis per cloud)"""
    import torch
    from icpmi import _lib, batch
    cs = batch.CloudSet.from_numpy(clouds)
    L = _lib.lib()
    ws = torch.zeros(L.icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, cs.max_n), dtype=torch.uint8, device=cs.pts.device)
    nrm = batch.normals_set(cs, k, workspace=ws).cpu().numpy()
    T = cs.total_rows
    raw = ws.cpu().numpy()
    sxy = raw[:T * 16].view(np.float64).reshape(T, 2)
    sorig = raw[T * 32:T * 36].view(np.int32)
    skey = raw[T * 36:T * 40].view(np.float32)
    dirs = raw[T * 40:T * 40 + 4 * cs.n_clouds].view(np.int32)
    return cs.off_host, nrm, sxy, sorig, skey, dirs


def _projection(d, p):
    a = 0.0 if d == 1 else 1.0
    b = 0.0 if d == 0 else (-1.0 if d == 3 else 1.0)
    return p[:, 0] * a + p[:, 1] * b                                   # csrc/sweep.hpp, proj: two products, one sum


@pytest.mark.parametrize("polar, knn", [("2", None), ("0", None), ("0", "grid"), ("0", "sweep")],
                         ids=["bearing", "projections", "projections_grid", "projections_sweep"])
def test_prepare_targets(libopt, normals_ref, polar, knn):
    cases = extreme_clouds()
    clouds = [c for _, c in cases]
    libopt.setenv("ICPMI_POLAR", polar)
    if knn:
        libopt.setenv("ICPMI_PREP_KNN", knn)
    off, nrm, sxy, sorig, skey, dirs = _prepare(clouds, NORMAL_K)
    for i, (label, c) in enumerate(cases):
        lo, hi = int(off[i]), int(off[i + 1])
        n = hi - lo
        # normals, as test_normals_sizes compares them
        worst = np.abs(np.abs(np.sum(nrm[lo:hi] * normals_ref[i], axis=1)) - 1).max()
        assert worst < NORMALS_TOL, (label, polar, knn, worst)
        # the sorted copy: a permutation of the cloud, row by row the bits of the input
        rows = sorig[lo:hi]
        assert np.array_equal(np.sort(rows), np.arange(n)), (label, "not a permutation")
        assert np.array_equal(sxy[lo:hi], c[rows]), (label, "sorted copy")
        d = int(dirs[i])
        if polar == "2":
            assert d == 4, (label, d)
            key = skey[lo:hi].astype(np.float64)                       # the quantised bearing: equal keys keep row order
        else:
            assert 0 <= d < 4, (label, d)
            key = _projection(d, c)[rows]
            assert np.array_equal(rows, np.lexsort((np.arange(n), _projection(d, c)))), (label, d, "order")
        step = np.diff(key)
        assert (step >= 0).all() and (np.diff(rows)[step == 0] > 0).all(), (label, d, "(key, row) order")


def test_prepare_targets_orders_agree(libopt):
    """bearing order and projections: the same normals bit for bit (test_bearing_order_gives_identical_results)"""
    clouds = [c for _, c in extreme_clouds()]
    got = {}
    for polar in ("0", "2"):
        libopt.setenv("ICPMI_POLAR", polar)
        got[polar] = _prepare(clouds, NORMAL_K)[1]
    assert np.array_equal(got["0"], got["2"])


# ── fused ICP ───────────────────────────────────────────────────────────────────────────────────────────────────────────
ICP_ROWS = (1, 64, 65, 768, 769, 1536)      # one lane, a full wave, one row into the second wave, a full slot of the
ICP_VOXEL = 0.01                            # 768-thread shape, one row into the second slot, both slots full
ICP_ITERS = 3


def icp_pairs():
    """(sources, target): the target is 1 536 lattice sites (one per voxel at ICP_VOXEL; what two workgroups a CU can hold), a source the first n
    sites of another fixed order, turned by 1.5 degrees about the box and shifted: three iterations do not settle it.
    The error threshold is 0: a one-row source sits on its match after the first step and would meet any positive
    threshold in the second iteration; the others run all three at 1e-10 as well."""
    tgt = _lattice(1536, seed=1)
    th = np.deg2rad(1.5)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    mid = tgt.mean(0)
    srcs = [(_lattice(n, seed=2) - mid) @ R.T + mid + np.array([0.012, -0.009]) for n in ICP_ROWS]
    return srcs, tgt


@pytest.fixture(scope="module")
def icp_ref():
    srcs, tgt = icp_pairs()
    ref = {}
    for method in ("point_to_line", "point_to_point"):
        for s in srcs:
            ref[method, len(s)] = oracle.icp(s, tgt, 0.0, ICP_ITERS, ICP_VOXEL, method=method, normal_k=NORMAL_K)
    return ref


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
@pytest.mark.parametrize("n_pairs", [6, 1026], ids=["1024_threads", "768_threads"])
def test_icp_batch(icp_ref, method, n_pairs):
    """Six pairs run one to a workgroup of 1 024 threads; from 1 024 pairs on the launch takes 768 threads and two rows a
    thread (csrc/icp2.hip, plan_icp2), the shape of a large batch: the same six pairs over and over."""
    from icpmi import batch
    srcs, tgt = icp_pairs()
    for s in srcs:
        Ro, to, eo, io = icp_ref[method, len(s)]
        # the filter keeps every row (the shapes are what they are meant to be), and the oracle runs all three iterations
        assert io["n_src"] == len(s) and io["n_tgt"] == len(tgt) and io["iters"] == ICP_ITERS, (method, len(s), io)
    ps = np.arange(n_pairs) % len(srcs)
    b = batch.IcpBatch(srcs + [tgt], ps, np.full(n_pairs, len(srcs)), 0.0, ICP_ITERS, ICP_VOXEL, method=method, normal_k=NORMAL_K)
    assert b.fast
    b.run()
    R, t, err, info = b.unpack()
    for i in range(n_pairs):
        Ro, to, eo, io = icp_ref[method, len(srcs[ps[i]])]
        assert info["iters"][i] == io["iters"], (method, n_pairs, i, int(info["iters"][i]))
        fro = rot_err(R[i], t[i], Ro, to)
        assert fro < FRO_TOL, (method, n_pairs, i, len(srcs[ps[i]]), fro)
