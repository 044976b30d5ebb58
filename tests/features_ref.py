"""Extended-precision reference of the feature-alignment stages (utilities/features.py:35-160) — TEST INFRASTRUCTURE ONLY.

Restates the five stages of csrc/features.hip one by one from their float64 inputs: what the kernels DECIDE (neighbour
order, suppression, ratio test, inliers, winner) by the documented rule, with the margin of every decision so a test can
say the decision is not a matter of rounding; what they COMPUTE (curvature, rigid fits) in np.longdouble.  NumPy only.
Used by tests/test_features_edges_cpu.py (which pins this helper to tests/golden/features.npz and proves the conditions
on the cases of tests/features_cases.py) and by tests/test_features_edges_gpu.py (the kernels against it).
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def _rows(pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    assert pts.ndim == 2 and pts.shape[1] == 2 and len(pts) >= 1
    return pts


def d2_matrix(q, pts):
    """float64 squared distances as the kernels take them: dx = q - c; s = dx*dx; s += dy*dy (no contraction)."""
    dx = q[:, None, 0] - pts[None, :, 0]
    dy = q[:, None, 1] - pts[None, :, 1]
    s = dx * dx
    s += dy * dy
    return s


def knn_sets(pts, kk, queries=None):
    """The kk nearest rows of every row (itself included), ordered by (float64 d2, row) ascending — the kernels' rule.

    -> (idx (n, kk) int64, d2 (n, kk) float64, gap (n,)): gap = d2 of list entry kk (the first one left out) minus d2 of
    entry kk - 1, inf when nothing is left out; gap > 0 says the SET does not depend on the tie rule."""
    pts = _rows(pts)
    q = pts if queries is None else pts[np.asarray(queries, dtype=np.int64)]
    n = len(pts)
    assert 1 <= kk <= n
    idx = np.empty((len(q), kk), dtype=np.int64)
    d2 = np.empty((len(q), kk))
    gap = np.full(len(q), np.inf)
    for lo in range(0, len(q), 256):                      # blocks: an (n, n) float64 matrix at n = 2048 is 32 MiB
        D = d2_matrix(q[lo:lo + 256], pts)
        o = np.argsort(D, axis=1, kind="stable")          # stable over ascending rows = ties by the lower row
        Ds = np.take_along_axis(D, o, axis=1)
        idx[lo:lo + 256], d2[lo:lo + 256] = o[:, :kk], Ds[:, :kk]
        if kk < n:
            gap[lo:lo + 256] = Ds[:, kk] - Ds[:, kk - 1]
    return idx, d2, gap


def curvature_of_sets(pts, idx):
    """ev0 / (ev1 + 1e-10) of np.cov (ddof 1) of every neighbour set, in long double.  The set is centred on its first
    entry first (the query point: differences of nearby float64 numbers are exact in long double), and the smaller
    eigenvalue is det / ev1, so neither a far origin nor exactly collinear neighbours cost the reference digits."""
    pts = _rows(pts)
    n, kk = idx.shape
    if kk < 3:
        return np.zeros(n, dtype=LD)
    nb = pts[idx].astype(LD) - pts[idx[:, 0]].astype(LD)[:, None, :]
    dev = nb - nb.mean(axis=1, keepdims=True)
    f = LD(kk - 1)
    a = (dev[:, :, 0] * dev[:, :, 0]).sum(axis=1) / f
    b = (dev[:, :, 0] * dev[:, :, 1]).sum(axis=1) / f
    c = (dev[:, :, 1] * dev[:, :, 1]).sum(axis=1) / f
    h, mid = (a - c) / 2, (a + c) / 2
    ev1 = mid + np.sqrt(h * h + b * b)
    det = a * c - b * b
    ev0 = np.where(ev1 > 0, det / np.where(ev1 > 0, ev1, LD(1)), LD(0))
    return ev0 / (ev1 + LD(1e-10))


def curvature(pts, k):
    """compute_curvature, features.py:35-54 -> (curvature (n,) long double, gap (n,) at the k-th neighbour, idx (n, kk))."""
    pts = _rows(pts)
    kk = min(int(k), len(pts) - 1) + 1
    idx, _, gap = knn_sets(pts, kk)
    return curvature_of_sets(pts, idx), gap, idx


def curvature_numpy(pts, idx):
    """The reference's own float64 expression (np.cov + np.linalg.eigvalsh, features.py:51-53) over the given sets, in the
    list's order (distance order, as KDTree.query hands them over): the yardstick of the curvature tolerance."""
    pts = _rows(pts)
    out = np.zeros(len(idx))
    if idx.shape[1] < 3:
        return out
    for i, s in enumerate(idx):
        ev = np.linalg.eigvalsh(np.cov(pts[s].T))
        out[i] = ev[0] / (ev[-1] + 1e-10)
    return out


def curvature_tolerance(pts, idx, want):
    """-> (yardstick, tolerance): the worst absolute error of the reference's float64 expression against `want` on these
    sets; the kernel may be 4 x that and not below 4 * 2^-52 (another summation order, a closed-form eigen solve)."""
    y = float(np.abs(curvature_numpy(pts, idx).astype(LD) - want).max())
    return y, max(4.0 * y, 4.0 * EPS)


def keypoints(pts, curv, top_n, min_dist, order=None):
    """extract_keypoints, features.py:57-71: the sequential walk with the float64 sqrt(dx*dx + dy*dy) < min_dist.
    order None: descending curvature, ties by ascending row.  Entries of `order` that are no row are ignored.
    -> (rows kept (int64), smallest |distance - min_dist| met in the walk)."""
    pts = _rows(pts)
    n = len(pts)
    if order is None:
        order = np.argsort(-np.asarray(curv, dtype=np.float64), kind="stable")
    kept, margin = [], np.inf
    for idx in np.asarray(order, dtype=np.int64)[:n]:
        if len(kept) >= top_n:
            break
        if idx < 0 or idx >= n:
            continue
        if kept:
            d = pts[kept] - pts[idx]
            s = d[:, 0] * d[:, 0]
            s = s + d[:, 1] * d[:, 1]
            dist = np.sqrt(s)
            margin = min(margin, float(np.abs(dist - min_dist).min()))
            if (dist < min_dist).any():
                continue
        kept.append(int(idx))
    return np.array(kept, dtype=np.int64), margin


def descriptors(pts, kp, k):
    """compute_descriptors, features.py:76-87: sqrt of the float64 d2 of list entries 1 .. kk-1 -> (n_kp, min(k, n-1))."""
    pts = _rows(pts)
    kk = min(int(k), len(pts) - 1) + 1
    kp = np.asarray(kp, dtype=np.int64)
    if len(kp) == 0:
        return np.zeros((0, kk - 1))
    _, d2, _ = knn_sets(pts, kk, queries=kp)
    return np.sqrt(d2[:, 1:])


def matches(da, db, ratio):
    """match_descriptors, features.py:92-106, by direct differences in long double: the two smallest squared distances
    of every source row (the lower index on ties; a NaN distance is never one of them), D0 < ratio^2 * D1 with the
    float64 ratio ** 2 the caller forms.
    -> (list of (i, j), margin (ns,) = |D0 - ratio^2 D1| / D1 (0 where D1 == 0, inf where a row has no two distances))."""
    da, db = np.asarray(da, dtype=np.float64), np.asarray(db, dtype=np.float64)
    ns, nt = len(da), len(db)
    if ns == 0 or nt < 2:
        return [], np.full(ns, np.inf)
    r2 = LD(float(ratio) ** 2)
    diff = da.astype(LD)[:, None, :] - db.astype(LD)[None, :, :]
    D = (diff * diff).sum(axis=2)
    D = np.where(np.isnan(D), LD(np.inf), D)
    o = np.argsort(D, axis=1, kind="stable")
    out, margin = [], np.full(ns, np.inf)
    for i in range(ns):
        j0, j1 = o[i, 0], o[i, 1]
        D0, D1 = D[i, j0], D[i, j1]
        if not np.isfinite(D1):
            continue                                       # no two distances to compare (a NaN row): no match
        margin[i] = float(abs(D0 - r2 * D1) / D1) if D1 > 0 else 0.0
        if D0 < r2 * D1:
            out.append((i, int(j0)))
    return out, margin


def rigid(src, dst):
    """_rigid_from_points, features.py:111-122, in long double: the optimal rotation has the angle
    atan2(W01 - W10, W00 + W11), written as cos = a / hypot(a, b), sin = b / hypot(a, b); the identity when both are 0.
    t = mu_d - R mu_s.  -> (R (2, 2), t (2,)) long double."""
    s, d = np.asarray(src, dtype=np.float64).astype(LD), np.asarray(dst, dtype=np.float64).astype(LD)
    s0, d0 = s[0].copy(), d[0].copy()                      # centred on the first point first: exact, see curvature_of_sets
    ms, md = (s - s0).mean(axis=0), (d - d0).mean(axis=0)
    p, q = (s - s0) - ms, (d - d0) - md
    W = p.T @ q
    a, b = W[0, 0] + W[1, 1], W[0, 1] - W[1, 0]
    nrm = np.sqrt(a * a + b * b)
    c, sn = (a / nrm, b / nrm) if nrm > 0 else (LD(1), LD(0))
    R = np.array([[c, -sn], [sn, c]], dtype=LD)
    t = (md + d0) - R @ (ms + s0)
    return R, t


def _errors(R, t, S, D):
    e = S @ R.T + t - D
    return np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def ransac(kp_s, kp_t, match_list, hyp_idx, thresh):
    """ransac_align, features.py:125-160, the hypotheses an input (rows (i, j) of match indices; a row outside [0, n) or
    with i == j counts 0).  -> dict: counts (n_iter,), best (-1: none), inliers, R, t (long double), margin = smallest
    |err - thresh| met, few = fewer than 2 matches, mask = the inliers the final fit was made on (None: a two-point fit or none)."""
    m = np.asarray(match_list, dtype=np.int64).reshape(-1, 2)
    n = len(m)
    out = dict(counts=np.zeros(len(hyp_idx), dtype=np.int64), best=-1, inliers=0, R=np.eye(2, dtype=LD), t=np.zeros(2, dtype=LD),
               margin=np.inf, few=n < 2, mask=None)
    if n < 2:
        return out
    S = np.asarray(kp_s, dtype=np.float64)[m[:, 0]].astype(LD)
    D = np.asarray(kp_t, dtype=np.float64)[m[:, 1]].astype(LD)
    th = LD(float(thresh))
    fits = {}
    for h, (i, j) in enumerate(np.asarray(hyp_idx, dtype=np.int64).reshape(-1, 2)):
        if i < 0 or j < 0 or i >= n or j >= n or i == j:
            continue
        key = (int(i), int(j))
        if key not in fits:
            R, t = rigid(S[[i, j]], D[[i, j]])
            err = _errors(R, t, S, D)
            fits[key] = (R, t, int((err < th).sum()), float(np.abs(err - th).min()))
        out["counts"][h] = fits[key][2]
        out["margin"] = min(out["margin"], fits[key][3])
    c = out["counts"]
    if c.max() <= 0:
        return out
    best = int(np.argmax(c))                               # the first of the largest, features.py:148 (strict >)
    i, j = (int(v) for v in np.asarray(hyp_idx).reshape(-1, 2)[best])
    R, t, inl, _ = fits[(i, j)]
    if inl >= 2:                                           # features.py:153-158
        err = _errors(R, t, S, D)
        mask = err < th
        out["margin"] = min(out["margin"], float(np.abs(err - th).min()))
        if mask.sum() >= 2:
            R, t = rigid(S[mask], D[mask])
            inl = int(mask.sum())
            out["mask"] = mask
    out.update(best=best, inliers=inl, R=R, t=t)
    return out


def rot_err_ld(R, t, Rw, tw):
    """Frobenius distance of a float64 transform from a long-double one."""
    dR = np.asarray(R, dtype=np.float64).astype(LD).reshape(2, 2) - Rw
    dt = np.asarray(t, dtype=np.float64).astype(LD).reshape(2) - tw
    return float(np.sqrt((dR * dR).sum() + (dt * dt).sum()))


def rigid_tolerance(src, dst):
    """-> (yardstick, tolerance) of a rigid fit: the rot_err of the reference's NumPy SVD expression on these points
    against `rigid`; the kernel may be 4 x that and not below 8 * 2^-52 * max(1, |mu|) (t carries the offset's rounding)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    W = (src - mu_s).T @ (dst - mu_d)
    U, _, Vt = np.linalg.svd(W)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[-1] *= -1
        R = Vt.T @ U.T
    t = mu_d - R @ mu_s
    Rw, tw = rigid(src, dst)
    y = rot_err_ld(R, t, Rw, tw)
    mu = max(1.0, float(np.hypot(*mu_s)), float(np.hypot(*mu_d)))
    return y, max(4.0 * y, 8.0 * EPS * mu)
