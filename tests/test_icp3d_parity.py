"""3-D ICP on the MI355X (the fused kernel with DIM = 3 and the Jacobi kabsch3) against the reference's 3-D runs
(tests/golden/icp3d.npz, make_golden.py gold_icp3d), the CPU oracle, and NumPy's SVD as an independent reference of
the Kabsch step in 2-D and 3-D, rank-deficient cross-covariances included."""
import numpy as np
import pytest

import oracle
from conftest import rot_err
from test_oracle_golden import assert_proper_rotation, assert_rank_deficient_case, icp3d_cases, odometry3d_stream

pytestmark = pytest.mark.gpu

FRO_TOL = 1e-9
CASES = list(icp3d_cases())


@pytest.fixture(scope="module")
def uicp():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import icp
    icp.VERBOSE = False
    return icp


@pytest.mark.parametrize("name", CASES)
def test_icp3d_golden(uicp, name):
    from icpmi import synth
    s, t, kw, z = icp3d_cases()[name]
    R, tt, err = uicp.ICP(s, t, **kw)
    info = uicp.last_icp_info
    Ro, to, eo, io = oracle.icp(s, t, kdtree=True, **kw)
    assert info["status"] == io["status"] and info["iterations"] == io["iters"], (name, info, io)
    if name in synth.ICP3D_RANK_DEFICIENT:
        assert_rank_deficient_case(R, tt, err, info["iterations"], s, kw, z, name)
        assert rot_err(R, tt, Ro, to) < FRO_TOL                    # same completion as the oracle
        if name in ("line_x", "single_point"):                      # u1 = v1 / W = 0: the reference's R is I
            assert rot_err(R, tt, z[f"{name}__R"], z[f"{name}__t"]) < FRO_TOL
        return
    assert_proper_rotation(R)
    assert rot_err(R, tt, z[f"{name}__R"], z[f"{name}__t"]) < FRO_TOL, name
    assert rot_err(R, tt, Ro, to) < FRO_TOL, name
    ref = float(z[f"{name}__err"])
    assert (np.isinf(err) and np.isinf(ref)) or abs(err - ref) <= 1e-11 * max(1.0, abs(err)), name
    if int(z[f"{name}__conv"]):
        assert info["status"] == oracle.CONVERGED and info["iterations"] == int(z[f"{name}__iters"]), name


def test_icp3d_exact_ties_across_a_target_tile_boundary(uicp):
    """Sources exactly midway between z neighbours of a 2 197-row lattice (two target tiles; rows 2047 | 2048 are
    neighbours): the lower index wins, as in the oracle.  The reference's k-d tree breaks such ties by its tree."""
    from icpmi import synth
    g = synth.lattice3d(13 ** 3, 0, jitter=0.0)
    for rows in ([2047], [2047, 2046, 30, 1000, 2100], list(range(0, 2196, 7))):
        mids = g[[r for r in rows if g[r, 2] < 12]] + np.array([0.0, 0.0, 0.5])
        R, t, err = uicp.ICP(mids, g, 1e-10, 100, 0.05)
        Ro, to, eo, io = oracle.icp(mids, g, 1e-10, 100, 0.05)
        assert rot_err(R, t, Ro, to) < FRO_TOL and uicp.last_icp_info["iterations"] == io["iters"], rows
        assert abs(err - eo) <= 1e-11 * max(1.0, eo)


def test_icp3d_batch_equals_single_pair_runs(uicp):
    """Every fixture case in IcpBatch launches of mixed sizes (one per parameter set), per-pair (B, 3, 3) R_init and
    (B, 3) t_init, identity where a case has none: bit for bit what the single-pair runs return."""
    from icpmi import batch
    cases = icp3d_cases()
    groups = {}
    for name, (s, t, kw, z) in cases.items():
        key = (kw["error_threshold"], kw["max_iterations"], kw["voxel_size"], kw.get("max_corr_dist"))
        groups.setdefault(key, []).append(name)
    # a pair with inliers beside the one that has none (teapot_break0)
    extra = ("teapot_init", cases["teapot_init"][0], cases["teapot_init"][1], cases["teapot_init"][2])
    n_runs = 0
    for (thr, maxit, vox, corr), names in groups.items():
        items = [(n, cases[n][0], cases[n][1], cases[n][2]) for n in names]
        if "teapot_break0" in names:
            items.append(extra)
        B = len(items)
        Ri = np.stack([np.asarray(kw.get("R_init", np.eye(3))) if "t_init" in kw else np.eye(3) for _, _, _, kw in items])
        ti = np.stack([np.asarray(kw["t_init"]) if "t_init" in kw else np.zeros(3) for _, _, _, kw in items])
        clouds = [it[1] for it in items] + [it[2] for it in items]
        b = batch.IcpBatch(clouds, np.arange(B), np.arange(B, 2 * B), thr, maxit, vox, R_init=Ri, t_init=ti,
                           max_corr_dist=corr)
        res = b.run().cpu().numpy()[:B].copy()
        for k, (n, s, t, kw) in enumerate(items):
            one = batch.icp_batch([s], [t], thr, maxit, vox, R_init=Ri[k], t_init=ti[k], max_corr_dist=corr)
            R1, t1, e1, i1 = one
            assert np.array_equal(res[k, :9].reshape(3, 3), R1[0]) and np.array_equal(res[k, 9:12], t1[0]), n
            assert np.array_equal(res[k, 12], e1[0]) and int(res[k, 14]) == i1["iters"][0], n
            assert int(res[k, 15]) == i1["status"][0], n
            n_runs += 1
        if corr == 0.05:
            assert int(res[0, 15]) == oracle.FEW_INLIERS and int(res[0, 14]) == 0
            assert int(res[-1, 14]) >= 1
    assert n_runs == len(cases) + 1


# ── the Kabsch step against np.linalg.svd (reference icp.py:196-207) ──────────────────────────────────────────────
def _sweep_clouds(dim, seed=17):
    """(family, source, target) one-step registrations whose W is generic, planar, mirrored, has repeated singular
    values, rank 1 or rank 0."""
    from icpmi import synth
    rng = np.random.default_rng(seed + dim)
    out = []

    def rot():
        if dim == 2:
            a = rng.uniform(-0.6, 0.6)
            return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        return synth.rot3(*rng.uniform(-0.5, 0.5, size=3))

    def moved(p, noise=0.0):
        return p @ rot().T + rng.uniform(-0.3, 0.3, size=dim) + rng.normal(0.0, noise, size=p.shape)

    for _ in range(60):                                                          # generic, some noisy
        p = rng.normal(size=(int(rng.integers(4, 60)), dim)) * rng.uniform(0.2, 3.0, size=dim)
        out.append(("generic", p, moved(p, rng.choice([0.0, 0.05]))))
    for _ in range(40):                                                          # mirrored in the thin axis: det W < 0
        p = rng.normal(size=(int(rng.integers(5, 50)), dim)) * np.array([3.0, 2.0, 0.2][-dim:])
        m = np.ones(dim)
        m[-1] = -1.0
        a = rng.uniform(-0.05, 0.05)
        Rs = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) if dim == 2 else synth.rot3(0.0, 0.0, a)
        out.append(("mirrored", p, (p * m) @ Rs.T + rng.uniform(-0.05, 0.05, size=dim)))
    for _ in range(40):                                                          # collinear: rank 1
        n = int(rng.integers(2, 30))
        a = np.sort(rng.uniform(-2, 2, size=n))
        if rng.uniform() < 0.4:                                                  # along an axis, same direction
            k = int(rng.integers(dim))
            p = np.zeros((n, dim))
            p[:, k] = a
            q = p + np.eye(dim)[k] * rng.uniform(-0.05, 0.05)
        else:
            d, e = rng.normal(size=dim), rng.normal(size=dim)
            p = a[:, None] * d / np.linalg.norm(d)
            q = a[:, None] * e / np.linalg.norm(e) + rng.uniform(-1, 1, size=dim)
        out.append(("rank1", p, q))
    for _ in range(25):                                                          # one source point: W = 0
        out.append(("rank0", rng.uniform(-1, 1, size=(1, dim)), rng.uniform(-1, 1, size=(int(rng.integers(1, 20)), dim))))
    if dim == 3:
        for _ in range(50):                                                      # planar: W has rank 2
            n = int(rng.integers(4, 60))
            xy = rng.uniform(-1, 1, size=(n, 2))
            if rng.uniform() < 0.5:                                              # z = 0, turned about z: exact
                p = np.column_stack([xy, np.zeros(n)])
                a = rng.uniform(-0.6, 0.6)
                q = p @ synth.rot3(0.0, 0.0, a).T + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0])
                out.append(("planar", p, q))
            else:                                                                # a tilted plane: numerically rank 2
                Bm = synth.rot3(*rng.uniform(-np.pi, np.pi, size=3))
                p = xy @ Bm[:, :2].T
                out.append(("tilted", p, moved(p)))
        shapes = [np.stack(np.meshgrid([-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0], indexing="ij"), -1).reshape(-1, 3),
                  np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])]
        for k in range(3, 23):
            shapes.append(synth._fibonacci_sphere(10 * k))
        for _ in range(4):
            for sh in shapes[:2]:
                out.append(("repeated", sh, moved(sh)))
        for sh in shapes[2:]:
            out.append(("repeated", sh, moved(sh)))
    else:
        sq = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
        for k in range(40):                                                      # square, regular polygons
            a = 2 * np.pi * np.arange(3 + k % 9) / (3 + k % 9)
            sh = sq if k % 5 == 0 else np.stack([np.cos(a), np.sin(a)], 1)
            out.append(("repeated", sh, moved(sh)))
    return out


def _kabsch_reference(src, tgt, vox):
    """W from the correspondences the kernel must have used (oracle.nn is bit-exact to it), solved by NumPy."""
    P = oracle.voxel_downsample(src, vox)
    T = oracle.voxel_downsample(tgt, vox)
    _, idx = oracle.nn(P, T)
    Q = T[idx]
    W = (P - P.mean(axis=0)).T @ (Q - Q.mean(axis=0))
    u, s, vt = np.linalg.svd(W)
    r = vt.T @ u.T
    flipped = np.linalg.det(r) < 0
    if flipped:
        vt[-1, :] *= -1
        r = vt.T @ u.T
    # the size of W's rounding: |W| can be that small when every source finds the same target
    noise = 1e-14 * float(np.sum(np.linalg.norm(P, axis=1) * np.linalg.norm(Q, axis=1)))
    return W, s, r, flipped, noise


def _run_sweep(dim, force_exhaustive=False):
    from icpmi import batch
    cases = _sweep_clouds(dim)
    vox = 1e-4                                     # every point its own voxel; 3-D keys need range / voxel < 2^21
    clouds = [c[1] for c in cases] + [c[2] for c in cases]
    B = len(cases)
    b = batch.IcpBatch(clouds, np.arange(B), np.arange(B, 2 * B), 1e-30, 1, vox, force_exhaustive=force_exhaustive)
    assert b.fast == (dim == 2 and not force_exhaustive)
    res = b.run().cpu().numpy()[:B]
    R_all, _, _, info = batch.unpack_results(res, dim)
    seen, n_flip, n_unique = set(), 0, 0
    for k, (fam, src, tgt) in enumerate(cases):
        R = R_all[k]
        W, s, Rr, flipped, noise = _kabsch_reference(src, tgt, vox)
        assert info["iters"][k] == 1, (fam, k)
        assert_proper_rotation(R)
        wn = np.linalg.norm(W)
        assert np.trace(R @ W) >= np.trace(Rr @ W) - 1e-12 * wn - noise, (fam, k)
        unique = s[0] > 1e6 * noise and s[dim - 2] > 1e-8 * s[0] and (not flipped or s[dim - 2] - s[dim - 1] > 1e-8 * s[0])
        if unique:
            assert np.linalg.norm(R - Rr) <= 1e-10, (fam, k, np.linalg.norm(R - Rr))
            n_unique += 1
        if fam == "rank0":
            assert np.array_equal(R, np.eye(dim)), (fam, k)
        if fam == "rank1" and np.count_nonzero(W) == 1 and W.max() > 0:
            assert np.abs(R - np.eye(dim)).max() <= 1e-15, (fam, k)           # u1 = v1 on an axis: R = I
        n_flip += flipped and fam == "mirrored"
        seen.add(fam)
    assert n_flip >= 10                                                       # the det < 0 fix is really exercised
    assert n_unique >= B // 2
    return seen


def test_kabsch3_sweep_against_numpy_svd(uicp):
    seen = _run_sweep(3)
    assert seen == {"generic", "mirrored", "rank1", "rank0", "planar", "tilted", "repeated"}


@pytest.mark.parametrize("force_exhaustive", [False, True])
def test_kabsch2_sweep_against_numpy_svd(uicp, force_exhaustive):
    seen = _run_sweep(2, force_exhaustive)
    assert seen == {"generic", "mirrored", "rank1", "rank0", "repeated"}


def test_run_icp3d_odometry_equals_the_reference(uicp, capsys):
    """icp.py:225-250, the legacy odometry, on a 3-D stream with its defaults."""
    stream, z = odometry3d_stream()
    pose, traj = uicp.run_icp(iter(stream))
    out = capsys.readouterr().out
    assert np.abs(pose - z["odo__pose"]).max() < 1e-8
    assert np.abs(np.array(traj) - z["odo__traj"]).max() < 1e-8
    errs = [float(line.split()[-1]) for line in out.splitlines() if line.startswith("Scan:")]
    assert np.allclose(errs, z["odo__errs"], rtol=1e-11, atol=0)
