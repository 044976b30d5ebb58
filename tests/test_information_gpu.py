"""icpmi_icp_information_batch and the layers above it against a NumPy restatement of include/icpmi.h's contract.

The yardstick is tests/information_ref.py: the moved row from the stated expression (elementwise float64: the same bits the
kernel forms), a brute-force ``argmin`` of ``dx*dx + dy*dy`` (first minimum: the kernel's tie rule), the stated inlier test, and
the ten sums of a record in ``np.longdouble``.  ``inliers``, ``rows`` and ``status`` must be EQUAL; each sum must lie within

    (m + 16) * 2**-53 * sum_i |term_i|_abs

of the long-double value, m the number of summed terms and |term|_abs the term with every subtraction turned into a sum
of absolute values: the first-order running-error bound of ANY summation order of m float64 terms (m - 1 additions), plus
16 roundings for forming a term (the longest chain, c * c of point_to_line, has 11).  Nothing in the bound is measured.

Shapes are the smallest at which the kernel can go wrong: T the threads of a workgroup (rows l, l + T, ... belong to lane
l), L the rows of an LDS target tile, 16 the padding unit of a tile (NN_CHUNK)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from information_ref import LD, U, brute_match, check_record, moved, ref_of_pair, restate      # noqa: F401

pytestmark = pytest.mark.gpu

METHODS = ("point_to_line", "point_to_point")
GATES = (None, 0.04, 0.0015)              # keep all; reject the far third; reject all but rows 0 and 1
T_ID = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
T_ROT = np.array([np.cos(0.3), -np.sin(0.3), np.sin(0.3), np.cos(0.3), 0.6, -0.8])      # 0.3 rad, one metre


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import features, icp as uicp
    features.VERBOSE = uicp.VERBOSE = False


# ── the kernel's shapes, clouds built directly ───────────────────────────────
def target_cloud(M, rng, shift=0.0):
    """M points at least 0.6 apart: cells of a unit grid in random order, jittered by 0.2."""
    g = int(np.ceil(np.sqrt(M)))
    cells = rng.permutation(g * g)[:M]
    xy = np.stack([cells % g, cells // g], axis=1).astype(np.float64) - g / 2.0
    return np.ascontiguousarray(xy + rng.uniform(-0.2, 0.2, size=(M, 2)) + shift)


def source_cloud(N, Q, T6, rng):
    """N rows that land, moved by T6, beside rows of Q: rows 0 and 1 at 0.0005, every third row at 0.06 .. 0.1 and the
    others at 0.005 .. 0.02 — so that GATES[1] rejects about a third and GATES[2] all but two."""
    k = rng.integers(0, len(Q), size=N)
    r = rng.uniform(0.005, 0.02, size=N)
    far = np.arange(N) % 3 == 2
    r[far] = rng.uniform(0.06, 0.1, size=int(far.sum()))
    r[:2] = 0.0005
    a = rng.uniform(-np.pi, np.pi, size=N)
    w = Q[k] + r[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
    R, t = T6[:4].reshape(2, 2), T6[4:]
    return np.ascontiguousarray((w - t) @ R)                     # R^T (w - t), row-wise


@pytest.fixture(scope="module")
def shapes(gpu):
    """One cloud set with every shape, its pairs, and the brute-force match of every pair (computed once)."""
    import torch
    from icpmi import _lib
    from icpmi.batch import CloudSet
    T, L = _lib.INFO_THREADS, _lib.INFO_TILE_ROWS
    rng = np.random.default_rng(20240611)
    src_rows = (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
    tgt_rows = (1, 15, 16, 17, L - 1, L, L + 1, 2 * L + 3)
    clouds = [target_cloud(M, rng) for M in tgt_rows]
    pairs = []                                              # (source cloud, target cloud, transform, what)
    for ti, M in enumerate(tgt_rows):
        for N in src_rows:
            for T6, name in ((T_ID, "identity"), (T_ROT, "rotated")):
                clouds.append(source_cloud(N, clouds[ti], T6, rng))
                pairs.append((len(clouds) - 1, ti, T6, f"{N} rows -> {M} rows, {name}"))
    # exact ties: two targets mirrored about the moved source row (0, 0); the lower index must win.  Once inside one
    # 16-row chunk, once across two LDS tiles.
    tie_small = target_cloud(20, rng, shift=40.0)
    tie_small[3], tie_small[9] = (0.5, 0.25), (-0.5, -0.25)
    tie_tiles = target_cloud(L + 10, rng, shift=100.0)
    tie_tiles[5], tie_tiles[L + 7] = (0.5, 0.25), (-0.5, -0.25)
    tie_src = np.array([[0.0, 0.0], [40.3, 39.9], [0.0, 0.0]])
    clouds += [tie_small, tie_tiles, tie_src, np.zeros((0, 2))]
    i_small, i_tiles, i_src, i_empty = range(len(clouds) - 4, len(clouds))
    ties = [len(pairs), len(pairs) + 1]
    pairs += [(i_src, i_small, T_ID, "tie inside a chunk"), (i_src, i_tiles, T_ID, "tie across tiles")]
    empties = [len(pairs), len(pairs) + 1]
    pairs += [(i_empty, 1, T_ID, "empty source"), (len(tgt_rows) + 4, i_empty, T_ROT, "empty target")]
    cs = CloudSet.from_numpy(clouds)
    ang = rng.uniform(-np.pi, np.pi, size=cs.total_rows)
    normals = np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))     # unit rows, any direction
    match = []
    for s, t, T6, _ in pairs:
        P = moved(clouds[s], T6)
        match.append((P,) + (brute_match(P, clouds[t]) if len(P) and len(clouds[t]) else (np.zeros(0, dtype=np.int64), np.zeros(0))))
    off = cs.off_host
    return dict(cs=cs, clouds=clouds, pairs=pairs, match=match, normals=normals, normals_dev=torch.from_numpy(normals).to(cs.pts.device),
                nrm_of=lambda c: normals[off[c]:off[c + 1]], ties=ties, empties=empties,
                src=np.array([p[0] for p in pairs], dtype=np.int32), tgt=np.array([p[1] for p in pairs], dtype=np.int32),
                T=np.stack([p[2] for p in pairs]))


def run_set(sh, method, gate, which=None):
    from icpmi.information import information_set
    which = np.arange(len(sh["pairs"])) if which is None else np.asarray(which)
    return information_set(sh["cs"], sh["normals_dev"], sh["src"][which], sh["tgt"][which], sh["T"][which], method, gate).cpu().numpy()


@pytest.mark.parametrize("gate", GATES, ids=("no gate", "a third rejected", "all but two rejected"))
@pytest.mark.parametrize("method", METHODS)
def test_every_shape_against_the_restatement(shapes, method, gate):
    sh = shapes
    rec = run_set(sh, method, gate)
    assert rec.shape == (len(sh["pairs"]), 16)
    rejected = []
    for b, (s, t, T6, what) in enumerate(sh["pairs"]):
        P, j, d2 = sh["match"][b]
        ref = restate(P, sh["clouds"][t], sh["nrm_of"](t), j, d2, method, gate, len(sh["clouds"][s]))
        check_record(rec[b], ref, f"{what}, {method}, gate {gate}")
        if ref["status"] != 4 and b not in sh["ties"]:
            rejected.append((ref["rows"] - ref["inliers"], ref["rows"], ref["status"]))
    # the gates do what the cases were built for (a property of the inputs, checked on the restatement's counts)
    rej, rows, status = (np.array(v) for v in zip(*rejected))
    if gate is None:
        assert not rej.any() and not status.any()
    elif gate == GATES[1]:
        assert np.array_equal(rej, rows // 3)
    else:
        assert np.array_equal(rows - rej, np.minimum(rows, 2)) and (status == 3).all()
    for b in sh["empties"]:
        assert rec[b, 12] == 4 and not rec[b, :12].any() and not rec[b, 13:].any()


def test_exact_tie_takes_the_lower_index(shapes):
    """Both tie pairs: the two mirrored targets are exactly as far, the restatement (np.argmin: the first minimum) takes the
    lower index, the record agrees with it — and would not agree with the other choice, by far more than the bound."""
    from icpmi import _lib
    sh = shapes
    L = _lib.INFO_TILE_ROWS
    rec = run_set(sh, "point_to_point", None, sh["ties"])
    for k, (b, lo, hi) in enumerate(zip(sh["ties"], (3, 5), (9, L + 7))):
        s, t, T6, what = sh["pairs"][b]
        P, j, d2 = sh["match"][b]
        Q = sh["clouds"][t]
        assert np.array_equal(P[0], [0.0, 0.0]) and j[0] == lo and j[2] == lo
        assert (Q[lo] ** 2).sum() == (Q[hi] ** 2).sum() == d2[0]
        ref = restate(P, Q, sh["nrm_of"](t), j, d2, "point_to_point", None, len(P))
        check_record(rec[k], ref, what)
        other = j.copy()
        other[[0, 2]] = hi
        wrong = restate(P, Q, sh["nrm_of"](t), other, d2, "point_to_point", None, len(P))
        assert abs(LD(rec[k, _lib.INFO_G + 1]) - wrong["sums"][7]) > 1e6 * wrong["bound"][7]


def test_batch_of_70_equals_its_pairs_one_by_one_and_itself(shapes):
    """70 pairs that mix every kind (each size class, both transforms, shared targets, the ties, the empties) in one launch,
    against the same pairs in 70 launches of one, and the same launch again: bit for bit.  The lanes' rows, the tile
    sequence and the reduction tree of a pair do not depend on its batch."""
    sh = shapes
    n = len(sh["pairs"])
    which = list(range(0, n - 4, 3))[:64] + sh["ties"] + sh["empties"]
    which = (which + list(range(1, n, 7)))[:70]
    assert len(which) == 70 and len(set(sh["tgt"][which])) < 12          # targets are shared
    for method, gate in (("point_to_line", GATES[1]), ("point_to_point", None)):
        both = run_set(sh, method, gate, which)
        again = run_set(sh, method, gate, which)
        assert both.tobytes() == again.tobytes()
        for k, b in enumerate(which):
            one = run_set(sh, method, gate, [b])
            assert one.tobytes() == both[k:k + 1].tobytes(), sh["pairs"][b][3]
    full = run_set(sh, "point_to_line", GATES[1])
    assert full[which].tobytes() == run_set(sh, "point_to_line", GATES[1], which).tobytes()


def test_wrapper_refusals(shapes):
    from icpmi.batch import CloudSet
    from icpmi.information import information_set
    from icpmi import IcpmiError
    sh = shapes
    with pytest.raises(ValueError, match="normals"):
        information_set(sh["cs"], None, [8], [0], T_ID[None], "point_to_line")
    with pytest.raises(ValueError, match="method"):
        information_set(sh["cs"], None, [8], [0], T_ID[None], "plane")
    with pytest.raises(ValueError, match="pair lists"):
        information_set(sh["cs"], None, [len(sh["clouds"])], [0], T_ID[None], "point_to_point")
    with pytest.raises(IcpmiError, match="2-D only"):
        information_set(CloudSet.from_numpy([np.zeros((3, 3))]), None, [0], [0], T_ID[None], "point_to_point")
    assert tuple(information_set(sh["cs"], None, [], [], np.zeros((0, 6)), "point_to_point").shape) == (0, 16)


# ── through the public layers, on scans of 200 beams ─────────────────────────
VOXEL, NORMAL_K, RS_VOXEL = 0.04, 12, 0.15
ICP_KW = dict(error_threshold=1e-10, max_iterations=60)


@pytest.fixture(scope="module")
def scans(gpu):
    from icpmi import synth
    poses = synth.trajectory(8, start=(-8.0, -0.5, 0.0), step=0.3)
    return [synth.scan(p, 7300 + i, n_beams=200) for i, p in enumerate(poses)]


def restate_batch(b, rec, pairs=None, results=None):
    """The records ``rec`` of the pairs ``pairs`` of an IcpBatch against the restatement, on the inputs ``information()``
    itself uses: the rows voxel_downsample_set left in ``b.vox`` and the normals normals_set gives for the targets."""
    from icpmi.batch import normals_set
    idx = np.arange(b.B) if pairs is None else np.asarray(pairs)
    rows = b.vox.to_numpy()
    off = b.vox.off_host
    method = "point_to_line" if b.use_p2l else "point_to_point"
    nrm = normals_set(b.vox, b.normal_k, cloud_ids=np.unique(b.pair_tgt_host[idx])).cpu().numpy() if b.use_p2l else None
    res = (b.results if results is None else results).cpu().numpy()
    gate = None if b.params.max_corr_dist < 0 else b.params.max_corr_dist
    assert rec.shape == (len(idx), 16)
    for k, i in enumerate(idx):
        s, t = int(b.pair_src_host[i]), int(b.pair_tgt_host[i])
        T6 = res[i, [0, 1, 2, 3, 9, 10]]
        N = nrm[off[t]:off[t] + len(rows[t])] if b.use_p2l else None
        check_record(rec[k], ref_of_pair(rows[s], rows[t], N, T6, method, gate), f"pair {i} ({s} -> {t}), {method}")


@pytest.mark.parametrize("method,force,gate", [("point_to_line", False, None), ("point_to_line", True, None),
                                               ("point_to_line", False, 0.3), ("point_to_point", False, 0.3),
                                               ("point_to_point", True, None)])
def test_icp_batch_information(scans, method, force, gate):
    from icpmi.batch import IcpBatch
    b = IcpBatch(scans[:5], [0, 1, 2, 0], [3, 4, 3, 1], voxel_size=VOXEL, method=method, normal_k=NORMAL_K, max_corr_dist=gate,
                 force_exhaustive=force, **ICP_KW)
    assert b.fast == (not force)
    b.run()
    rec = b.information().cpu().numpy()
    assert gate is not None or ((rec[:, 12] == 0).all() and np.array_equal(rec[:, 10], rec[:, 11]))
    restate_batch(b, rec)
    some = b.information([2, 0]).cpu().numpy()                    # listed pairs, in the order listed
    assert some.tobytes() == rec[[2, 0]].tobytes()
    # at transforms handed in: the records of another result tensor
    other = b.results.clone()
    other[:, 9] += 0.01
    restate_batch(b, b.information([1, 3], results=other).cpu().numpy(), [1, 3], results=other)
    with pytest.raises(ValueError):
        b.information([4])


def test_history_batch_and_single_pair_agree_bit_for_bit(scans):
    """hist.match(...).information([first]) == RunIcpPairBatch.information([first]) on the same arrays == icp_information at
    that result; a point_to_line match on a history without normals is refused as before."""
    from icpmi import ScanHistory, prealign
    from icpmi.information import icp_information, unpack_information
    run = dict(angle_step_coarse=2.0, angle_step_fine=0.2, **ICP_KW)
    hist = ScanHistory(voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL)
    hist.add_many(scans)
    cands = [2, 0, 4, 1]
    for method in METHODS:
        m = hist.match(7, cands, method=method, error_accept=0.5, stop_after_first_accepted=True, **run)
        m.run()
        first = m.first_accepted()
        assert first >= 0, m.unpack()[2]
        b = prealign.RunIcpPairBatch([scans[7]] + [scans[k] for k in cands], np.zeros(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32),
                                     voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, method=method,
                                     error_accept=0.5, stop_after_first_accepted=True, **run)
        b.run()
        assert b.first_accepted() == first
        rec_h, rec_b = m.information([first]).cpu().numpy(), b.information([first]).cpu().numpy()
        assert rec_h.shape == (1, 16) and rec_h.tobytes() == rec_b.tobytes()
        assert rec_h[0, 12] == 0 and rec_h[0, 10] > 50
        restate_batch(b.icp, rec_b, [first])
        R, t, _, _ = m.unpack()
        one = icp_information(scans[7], scans[cands[first]], R[first], t[first], VOXEL, method=method, normal_k=NORMAL_K)
        u = unpack_information(rec_h[0])
        assert one["method"] == method and np.array_equal(one["H"], one["H"].T)
        for key in ("H", "g", "sse", "inliers", "rows", "status"):
            assert np.array_equal(one[key], u[key]), (method, key)
        # every candidate of an ungated match, the resident path against the batch path
        m2 = hist.match(7, cands, method=method, **run)
        m2.run()
        b2 = prealign.RunIcpPairBatch([scans[7]] + [scans[k] for k in cands], np.zeros(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32),
                                      voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, method=method, **run)
        b2.run()
        assert m2.information().cpu().numpy().tobytes() == b2.information().cpu().numpy().tobytes()
    p2p = ScanHistory(voxel_size=VOXEL, normal_k=None, rotation_voxel_size=RS_VOXEL)
    p2p.add_many(scans[:3])
    with pytest.raises(ValueError, match="holds no normals"):
        p2p.match(2, [0], method="point_to_line")
    m = p2p.match(2, [0, 1], method="point_to_point", **run)
    m.run()
    restate_batch(m.icp, m.information().cpu().numpy())


def test_corridor_is_less_constrained_than_a_room(gpu):
    """Two parallel walls: a match is free along them.  The smallest relative eigenvalue of the scaled Hessian of a corridor
    pair lies below that of a room pair by the factor the restatement's own Hessians give.  Eigenvalues of a symmetric
    matrix move by at most the norm of its perturbation (Weyl), and the scaled Hessians of kernel and restatement differ by
    no more than 3 * max(bound_ij / sqrt(H_ii H_jj)), which the restatement supplies."""
    from icpmi import synth
    from icpmi.batch import IcpBatch, normals_set
    from icpmi.information import constraint_spectrum, unpack_information
    corridor = np.array([[-60.0, -1.2, 60.0, -1.2], [-60.0, 1.2, 60.0, 1.2]])
    # (seen from a heading of 0.6 rad: walls oblique to the sensor frame, the case the per-axis scaling is made for)
    pairs = {"corridor": [synth.scan((0.0, 0.1, 0.62), 1, n_beams=200, segs=corridor), synth.scan((0.25, 0.0, 0.6), 2, n_beams=200, segs=corridor)],
             "room": [synth.scan((-8.0, -0.5, 0.0), 3, n_beams=200), synth.scan((-7.7, -0.45, 0.02), 4, n_beams=200)]}
    ratio, ratio_ref, slack = {}, {}, {}
    for name, (a, c) in pairs.items():
        b = IcpBatch([a, c], [0], [1], voxel_size=VOXEL, method="point_to_line", normal_k=NORMAL_K, **ICP_KW)
        b.run()
        rec = b.information().cpu().numpy()
        restate_batch(b, rec)
        lam = constraint_spectrum(unpack_information(rec[0])["H"])[0]
        rows = b.vox.to_numpy()
        nrm = normals_set(b.vox, NORMAL_K, cloud_ids=[1]).cpu().numpy()[b.vox.off_host[1]:][:len(rows[1])]
        ref = ref_of_pair(rows[0], rows[1], nrm, b.results.cpu().numpy()[0, [0, 1, 2, 3, 9, 10]], "point_to_line", None)
        Href = unpack_information(np.concatenate([ref["sums"].astype(np.float64), np.zeros(6)]))["H"]
        Bnd = unpack_information(np.concatenate([ref["bound"].astype(np.float64), np.zeros(6)]))["H"]
        lam_ref = constraint_spectrum(Href)[0]
        d = np.sqrt(np.diag(Href))
        slack[name] = 3.0 * float((Bnd / np.outer(d, d)).max()) + 16 * U          # (+ the scaling's and eigh's own rounding)
        assert np.all(np.abs(lam - lam_ref) <= slack[name] * 4), (name, lam, lam_ref)
        ratio[name], ratio_ref[name] = lam[0] / lam[-1], lam_ref[0] / lam_ref[-1]
    want = ratio_ref["corridor"] / ratio_ref["room"]
    assert want < 0.2, ratio_ref                                    # the corridor IS the degenerate one (the restatement says so)
    rel = 8 * (slack["corridor"] / (ratio_ref["corridor"] * 1.0) + slack["room"] / ratio_ref["room"])
    assert abs(ratio["corridor"] / ratio["room"] - want) <= rel * want, (ratio, ratio_ref)


def test_example_loop_with_icp_edge_information(gpu):
    spec = importlib.util.spec_from_file_location("slam_loop", os.path.join(REPO, "examples", "slam_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.run(40, verbose=False, loop=True, edge_information="icp")
    g = out["graph"]
    assert len(g.nodes) == 40 and len(g.edges) == 39 + len(out["accepted"])
    assert len(out["spectra"]) == len(out["accepted"]) and all(0.0 <= r <= 1.0 for _, _, r in out["spectra"])
    anisotropic = 0
    for i, j, z, om in g.edges:
        assert om.shape == (3, 3) and np.array_equal(om, om.T), (i, j)
        lam = np.linalg.eigvalsh(om)
        assert lam.min() >= -1e-12 * lam.max(), (i, j, lam)         # eigvalsh: backward stable, a few ulp of |om|
        anisotropic += not np.array_equal(om, np.eye(3) * om[0, 0])
    assert anisotropic >= 39 - len(out["rejected"])                 # every accepted scan-to-scan step brought its own matrix
    assert np.isfinite(out["drift"]).all()
    # the default is the reference's weighting, and naming it changes nothing: same poses, same edges, bit for bit
    a = m.run(40, verbose=False, loop=True)
    b = m.run(40, verbose=False, loop=True, edge_information="isotropic")
    assert len(a["history"]) == len(b["history"]) == 40
    for (pa, Ta), (pb, Tb) in zip(a["history"], b["history"]):
        assert np.array_equal(pa, pb) and Ta.tobytes() == Tb.tobytes()
    assert all(ea[:2] == eb[:2] and ea[2].tobytes() == eb[2].tobytes() and ea[3].tobytes() == eb[3].tobytes()
               for ea, eb in zip(a["graph"].edges, b["graph"].edges))
    assert all(np.array_equal(om, np.eye(3) * om[0, 0]) for _, _, _, om in a["graph"].edges) and a["spectra"] == []
