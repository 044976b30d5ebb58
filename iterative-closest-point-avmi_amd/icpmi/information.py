"""The information matrix of an ICP result, and its conversion to a pose-graph edge.

The reference weights every pose-graph edge isotropically — ``np.eye(3) / max(error, 1e-6)`` for odometry (slam.py:548),
``np.eye(3) * lc_info_scale / max(err_lc, 1e-6)`` for a closure (slam.py:592) — although a scan match in a corridor is
well determined across it and almost free along it.  The matcher knows better: the matrix ``ATA`` of the last
point-to-line step (icp.py:100-104) is the Gauss-Newton Hessian of the registration in ``[theta, tx, ty]``.
``icpmi_icp_information_batch`` (csrc/information.hip) evaluates it — and the right-hand side, the residual sum and the
inlier count — once, at a finished transform, as a pass of its own after the ICP:

    m = hist.match(sid, cands, error_accept=0.05, stop_after_first_accepted=True)
    m.run(); first = m.first_accepted()
    info = unpack_information(m.information([first]).cpu().numpy())
    R = m.unpack()[0][first]
    omega = edge_information(info["H"][0], R, residual_variance({k: v[0] for k, v in info.items()}))

``information_set`` is the thin wrapper of the entry point, ``IcpBatch.information`` / ``RunIcpPairBatch.information``
(icpmi.batch, icpmi.prealign) answer for pairs of a batch at the transforms of its results, ``icp_information`` for one
pair of arrays.  The rest is host NumPy on 3 x 3 matrices.

torch is used for device memory and streams only.
"""
import numpy as np
import torch

from . import _lib
from ._lib import IcpmiError, check
from .batch import ICP_METHODS, CloudSet, PairList, _ptr, _stream, normals_set, voxel_downsample_set

_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # the order of the six H slots: theta, x, y


def _method_code(method):
    if method in (_lib.POINT_TO_POINT, "point_to_point"):
        return _lib.POINT_TO_POINT
    if method in (_lib.POINT_TO_LINE, "point_to_line"):
        return _lib.POINT_TO_LINE
    raise ValueError(f"method must be one of {ICP_METHODS}, got {method!r}")


def information_set(cs, normals, pair_src, pair_tgt, transforms, method, max_corr_dist=None, out=None):
    """``icpmi_icp_information_batch`` for the pairs (pair_src[b], pair_tgt[b]) of a 2-D cloud set — filtered or not: the
    valid rows are ``cs.cnt``'s — at ``transforms`` ([B, 6]: R row major, t; a device tensor, or an array that is
    uploaded) -> a device (B, INFO_DOUBLES) float64 tensor of records (slots ``_lib.INFO_*``; ``unpack_information``).
    ``normals``: row layout of ``cs.pts`` (``normals_set``), needed for point_to_line only.  ``max_corr_dist=None`` keeps
    every correspondence.  Enqueued on the current stream.  With a ``PairList`` already on the device as ``pair_src``, a
    device tensor of transforms and ``out`` (a (B, INFO_DOUBLES) float64 tensor to write into) the call uploads and
    allocates nothing and does not synchronise; an upload from an array makes the host wait for the stream."""
    L = _lib.lib()
    if cs.dim != 2:
        raise IcpmiError("the information matrix is 2-D only (ICPMI_ERR_UNSUPPORTED)")
    code = _method_code(method)
    if code == _lib.POINT_TO_LINE and normals is None:
        raise ValueError("point_to_line needs the normals of the target clouds")
    dev = cs.pts.device
    p = PairList.of(pair_src, pair_tgt)
    B = p.B
    for ids in (p.src_host, p.tgt_host):
        if B and (ids.min() < 0 or ids.max() >= cs.n_clouds):
            raise ValueError(f"pair lists must name clouds in [0, {cs.n_clouds})")
    p.to(dev)
    if not isinstance(transforms, torch.Tensor):
        transforms = torch.from_numpy(np.ascontiguousarray(transforms, dtype=np.float64).reshape(B, 6)).to(dev)
    if transforms.dtype != torch.float64 or tuple(transforms.shape) != (B, 6) or transforms.device != dev:
        raise ValueError(f"transforms must be ({B}, 6) float64 on {dev}")
    transforms = transforms.contiguous()
    if normals is not None and (normals.dtype != torch.float64 or normals.shape[0] < cs.total_rows or normals.device != dev):
        raise ValueError("normals must be float64, on the set's device, one row per row of the set")
    max_src_n = int(np.diff(cs.off_host)[p.src_host].max()) if B else 0
    if out is None:
        out = torch.empty((B, _lib.INFO_DOUBLES), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B, _lib.INFO_DOUBLES) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({B}, {_lib.INFO_DOUBLES}) float64 tensor on {dev}")
    check(L.icpmi_icp_information_batch(_ptr(cs.pts), _ptr(cs.off), _ptr(cs.cnt), _ptr(normals), _ptr(p.src), _ptr(p.tgt), B,
                                        max_src_n, _ptr(transforms), code, -1.0 if max_corr_dist is None else float(max_corr_dist),
                                        _ptr(out), _stream()), "icp_information")
    return out


def batch_information(batch, pairs=None, results=None):
    """``IcpBatch.information``: the records of the pairs ``pairs`` (indices into the batch's pair list; None: all) at the
    transforms held in ``results`` (None: the batch's own result tensor, as the last ``run()`` left it), with the batch's
    method and ``max_corr_dist``, on its filtered clouds.  The transforms are gathered on the device (slots RES_R..RES_R + 3
    and RES_T, RES_T + 1 of each record).  For ``pairs=None`` the call keeps the target ids and the normals' workspace on
    the device (an ``IcpBatch`` has the ids there already; a resident batch uploads them at its first call) and only
    enqueues, without a synchronisation.  A selection of pairs is uploaded at every call, and the host waits for the stream
    while it is.

    Row-order normals of the targets: on the sorted-sweep path they exist only inside the prepared buffer, in sorted order,
    so they are computed here — ``normals_set`` on the filtered clouds, for the targets of the listed pairs, into a buffer
    the batch keeps from the first call on.  Normals enter H, g and sse in products of two only: their sign is immaterial."""
    if batch.dim != 2:
        raise IcpmiError("the information matrix is 2-D only (ICPMI_ERR_UNSUPPORTED)")
    idx = np.arange(batch.B, dtype=np.int64) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1)
    if len(idx) and (idx.min() < 0 or idx.max() >= batch.B):
        raise ValueError(f"pairs must lie in [0, {batch.B})")
    vox = batch.vox
    dev = vox.pts.device
    res = batch.results if results is None else results
    if batch.use_p2l and (batch.info_normals is None or batch.info_normals.shape[0] < vox.pts.shape[0]):
        batch.info_normals = torch.zeros((max(vox.pts.shape[0], 1), 2), dtype=torch.float64, device=dev)
    mcd = batch.params.max_corr_dist
    mcd = None if mcd < 0 else mcd
    if pairs is None and batch.B:
        # every pair: the batch's own pair list, and buffers kept from the first call on
        kept = getattr(batch, "_info_all", None)
        if kept is None:
            ids, ids_dev = getattr(batch, "tgt_ids", None), getattr(batch, "tgt_ids_dev", None)
            if ids_dev is None:                                    # a resident batch keeps no list of its targets: one upload, once
                ids = np.unique(batch.pair_tgt_host)
                ids_dev = torch.from_numpy(ids).to(dev)
            kept = batch._info_all = dict(ids=ids, ids_dev=ids_dev, ws=None)
        T = torch.cat([res[:batch.B, _lib.RES_R:_lib.RES_R + 4], res[:batch.B, _lib.RES_T:_lib.RES_T + 2]], dim=1)
        normals = None
        if batch.use_p2l:
            normals, kept["ws"] = normals_set(vox, batch.normal_k, cloud_ids=kept["ids"], out=batch.info_normals,
                                              workspace=kept["ws"], cloud_ids_dev=kept["ids_dev"], return_workspace=True)
        return information_set(vox, normals, batch.pairs, None, T, batch.params.method, mcd)
    transforms = torch.cat([res[:, _lib.RES_R:_lib.RES_R + 4], res[:, _lib.RES_T:_lib.RES_T + 2]], dim=1)[torch.from_numpy(idx).to(dev)]
    src, tgt = batch.pair_src_host[idx], batch.pair_tgt_host[idx]
    normals = None
    if batch.use_p2l:
        if len(idx):
            normals = normals_set(vox, batch.normal_k, cloud_ids=np.unique(tgt), out=batch.info_normals)
        else:
            normals = batch.info_normals
    return information_set(vox, normals, src, tgt, transforms.contiguous(), batch.params.method, mcd)


def unpack_information(rec):
    """Records ((B, INFO_DOUBLES), or one (INFO_DOUBLES,) record) on the host -> dict: ``H`` ((B,) 3 x 3, symmetric, in
    [theta, tx, ty]), ``g`` ((B,) 3), ``sse``, ``inliers``, ``rows``, ``status`` (0, ST_FEW_INLIERS or ST_EMPTY)."""
    rec = np.asarray(rec, dtype=np.float64)
    one = rec.ndim == 1
    rec = rec.reshape(-1, _lib.INFO_DOUBLES)
    H = np.zeros((len(rec), 3, 3))
    for k, (i, j) in enumerate(_UPPER):
        H[:, i, j] = H[:, j, i] = rec[:, _lib.INFO_H + k]
    out = dict(H=H, g=rec[:, _lib.INFO_G:_lib.INFO_G + 3].copy(), sse=rec[:, _lib.INFO_SSE].copy(),
               inliers=rec[:, _lib.INFO_INLIERS].astype(np.int64), rows=rec[:, _lib.INFO_ROWS].astype(np.int64),
               status=rec[:, _lib.INFO_STATUS].astype(np.int64))
    return {k: v[0] for k, v in out.items()} if one else out


def icp_information(source, target, R, t, voxel_size, method="point_to_line", normal_k=10, max_corr_dist=None):
    """The information of one registration, beside ``icp_pair``: both clouds are uploaded and voxel-filtered as ``ICP``
    does (icp.py:150-151), the target's normals estimated (point_to_line), and the normal equations evaluated at (R, t) —
    the result of ``ICP(source, target, ...)`` with the same ``voxel_size`` / ``normal_k`` / ``max_corr_dist`` -> dict: ``H``
    (3 x 3, symmetric), ``g``, ``sse``, ``inliers``, ``rows``, ``status`` (synchronises), plus ``method``."""
    code = _method_code(method)
    source, target = np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if source.ndim != 2 or source.shape[1] != 2 or target.ndim != 2 or target.shape[1] != 2:
        raise IcpmiError("the information matrix is 2-D only (ICPMI_ERR_UNSUPPORTED)")
    vox = voxel_downsample_set(CloudSet.from_numpy([source, target]), voxel_size)
    normals = normals_set(vox, normal_k, cloud_ids=[1]) if code == _lib.POINT_TO_LINE else None
    T = np.concatenate([np.asarray(R, dtype=np.float64).reshape(4), np.asarray(t, dtype=np.float64).reshape(2)])[None, :]
    rec = information_set(vox, normals, [0], [1], T, code, max_corr_dist).cpu().numpy()[0]
    out = unpack_information(rec)
    out["method"] = ICP_METHODS[code]
    return out


def edge_information(H, R, sigma2):
    """The 3 x 3 information matrix, in ``[x, y, theta]`` (the order of PoseGraph2D's error, pose_graph.py:138-182), of the
    pose-graph measurement ``z = pose_matrix_to_vec(inv(T))`` that slam.py:545-549 and slam.py:586-593 store, from the
    registration's Hessian ``H`` in ``[theta, tx, ty]``, its rotation ``R`` and the residual variance ``sigma2``.

    A left perturbation delta = [theta, tx, ty] of T — T' = D(delta) T — moves z additively by eps, and to first order
    delta = G eps with G = -[[0, 0, 1], [R00, R01, 0], [R10, R11, 0]] (z holds -R^T t and -theta_T; rotating T by theta adds
    R^T d to R^T t and nothing else at first order: no lever arm).  So Omega = G^T H G / sigma2."""
    H, R = np.asarray(H, dtype=np.float64), np.asarray(R, dtype=np.float64)
    if H.shape != (3, 3) or R.shape != (2, 2):
        raise ValueError("H must be 3 x 3 and R 2 x 2")
    if not sigma2 > 0:
        raise ValueError("sigma2 must be positive")
    G = -np.array([[0.0, 0.0, 1.0], [R[0, 0], R[0, 1], 0.0], [R[1, 0], R[1, 1], 0.0]])
    omega = G.T @ H @ G / float(sigma2)
    return 0.5 * (omega + omega.T)


def residual_variance(info, method=None):
    """sse / (residual rows - 3): ``sse / (inliers - 3)`` for point_to_line (one residual per inlier), ``sse / (2 * inliers
    - 3)`` for point_to_point (two).  ``info``: one pair's dict (``unpack_information`` of one record, ``icp_information``);
    ``method`` overrides / supplies ``info["method"]``.  ValueError when the denominator is not positive."""
    code = _method_code(method if method is not None else info.get("method", "point_to_line"))
    n = int(info["inliers"])
    dof = (n if code == _lib.POINT_TO_LINE else 2 * n) - 3
    if dof <= 0:
        raise ValueError(f"{n} inliers leave no degrees of freedom for a residual variance ({ICP_METHODS[code]})")
    return float(info["sse"]) / dof


def constraint_spectrum(H):
    """Eigenvalues (ascending) and eigenvectors (columns, in [theta, tx, ty]) of D H D with D = diag(1 / sqrt(H_ii)) — H
    scaled to a unit diagonal, so that radians and metres compare (a zero diagonal entry keeps scale 1).  The smallest
    eigenvalue relative to the largest is the corridor diagnostic: ~0 when one direction (along the walls) is unconstrained.

    What the scaling can and cannot see: a free direction that MIXES the coordinates — walls oblique to the target's frame,
    tx and ty almost perfectly correlated — gives an eigenvalue near zero; a free direction along a coordinate axis is a small
    diagonal entry, which the unit diagonal normalises away unless it is exactly zero.  Compare H_xx with H_yy as well when
    the walls may lie along the frame's axes."""
    H = np.asarray(H, dtype=np.float64)
    if H.shape != (3, 3):
        raise ValueError("H must be 3 x 3")
    d = np.diag(H)
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
    return np.linalg.eigh(H * s[:, None] * s[None, :])
