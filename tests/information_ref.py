"""NumPy restatement of the record of icpmi_icp_information_batch (include/icpmi.h) and its bound, shared by
tests/test_information_gpu.py — whose docstring derives the bound — and the buffer-end cases of tests/buffer_ends_clouds.py:
the moved row from the stated expression (elementwise float64: the same bits the kernel forms), a brute-force ``argmin`` of
``dx*dx + dy*dy`` (first minimum: the kernel's tie rule), the stated inlier test, the ten sums of a record in
``np.longdouble``, and the check of a device record against them.  It uses nothing of the library but the slot numbers."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


# ── the restatement ──────────────────────────────────────────────────────────
def moved(S, T6):
    r00, r01, r10, r11, tx, ty = (np.float64(v) for v in T6)
    return np.stack([(r00 * S[:, 0] + r01 * S[:, 1]) + tx, (r10 * S[:, 0] + r11 * S[:, 1]) + ty], axis=1)


def brute_match(P, Q):
    """-> (j, d2): the first minimum of dx*dx + dy*dy over the rows of Q, for every row of P."""
    j = np.empty(len(P), dtype=np.int64)
    d2 = np.empty(len(P))
    for a in range(0, len(P), 256):
        dx = P[a:a + 256, None, 0] - Q[None, :, 0]
        dy = P[a:a + 256, None, 1] - Q[None, :, 1]
        D = dx * dx + dy * dy
        j[a:a + 256] = np.argmin(D, axis=1)
        d2[a:a + 256] = D[np.arange(D.shape[0]), j[a:a + 256]]
    return j, d2


def restate(P, Q, Nrm, j, d2, method, gate, n_src):
    """The record include/icpmi.h describes -> dict(sums [10] longdouble, bound [10] longdouble, inliers, rows, status)."""
    if n_src == 0 or len(Q) == 0:
        return dict(sums=np.zeros(10, dtype=LD), bound=np.zeros(10, dtype=LD), inliers=0, rows=0, status=4)
    if gate is None:
        keep = np.ones(len(P), dtype=bool)
    else:
        dist = np.sqrt(d2)
        keep = dist * dist < np.float64(gate) * np.float64(gate)
    px, py = P[keep, 0].astype(LD), P[keep, 1].astype(LD)
    qx, qy = Q[j[keep], 0].astype(LD), Q[j[keep], 1].astype(LD)
    one, zero = np.ones_like(px), np.zeros_like(px)
    if method == "point_to_line":
        nx, ny = Nrm[j[keep], 0].astype(LD), Nrm[j[keep], 1].astype(LD)
        rows = [(ny * px - nx * py, nx, ny, -(nx * (px - qx) + ny * (py - qy)))]
        rows_abs = [(abs(ny * px) + abs(nx * py), abs(nx), abs(ny), abs(nx) * (abs(px) + abs(qx)) + abs(ny) * (abs(py) + abs(qy)))]
    else:
        rows = [(-py, one, zero, -(px - qx)), (px, zero, one, -(py - qy))]
        rows_abs = [(abs(py), one, zero, abs(px) + abs(qx)), (abs(px), zero, one, abs(py) + abs(qy))]

    def ten(rr):
        out = np.zeros(10, dtype=LD)
        for a0, a1, a2, b in rr:
            for k, term in enumerate((a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2, a0 * b, a1 * b, a2 * b, b * b)):
                out[k] += np.sum(term, dtype=LD)
        return out

    n_in = int(keep.sum())
    m = n_in * len(rows)
    status = 3 if gate is not None and n_in < max(3, n_src // 10) else 0
    return dict(sums=ten(rows), bound=LD(m + 16) * LD(U) * ten(rows_abs), inliers=n_in, rows=n_src, status=status)


def check_record(rec, ref, what):
    from icpmi import _lib
    assert rec.shape == (16,)
    assert (rec[_lib.INFO_INLIERS], rec[_lib.INFO_ROWS], rec[_lib.INFO_STATUS]) == (ref["inliers"], ref["rows"], ref["status"]), what
    assert np.all(rec[13:] == 0.0), what
    err = np.abs(rec[:10].astype(LD) - ref["sums"])
    assert np.all(err <= ref["bound"]), (what, _lib.INFO_SLOTS[int(np.argmax(err - ref["bound"]))], err, ref["bound"])


def ref_of_pair(S, Q, Nrm, T6, method, gate):
    P = moved(S, T6)
    if len(S) and len(Q):
        j, d2 = brute_match(P, Q)
    else:
        j, d2 = np.zeros(0, dtype=np.int64), np.zeros(0)
    return restate(P, Q, Nrm, j, d2, method, gate, len(S))
