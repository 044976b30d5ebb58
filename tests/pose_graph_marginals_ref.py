"""Extended-precision reference for the marginals of the pose graph (blocks of H^-1) — TEST INFRASTRUCTURE ONLY.

The reference project has no marginals; the yardstick is the inverse of ITS matrix H (tests/pose_graph_ref.assemble_ld: the
edges' blocks, the anchor's rows and columns zeroed, 1e10 I on its block) in np.longdouble, and the bound is what a
backward-stable float64 solve of H X = E owes each block column (``block_bound``, of the form of ``step_bound``).  NumPy only.
Used by tests/test_pose_graph_marginals_cpu.py (which pins this helper and proves the condition on the cases) and by
tests/test_pose_graph_marginals_gpu.py (the kernels against the same references and bounds).
"""
import functools

import numpy as np

import pose_graph_ref as R

LD = np.longdouble
U = R.U
NEWTON_ROUNDS = 3
FULL_INVERSE_MAX_N = 200            # above: only the needed unit columns (a long-double matrix product is too slow)


def inverse_ld(H):
    """H^-1 in long double: LAPACK's float64 inverse, then NEWTON_ROUNDS rounds X <- X + X (I - H X) in long double.
    -> (X, max |last correction| / max |X|)."""
    H = np.asarray(H, dtype=LD)
    X = np.asarray(np.linalg.inv(np.asarray(H, dtype=np.float64)), dtype=LD)
    I = np.eye(H.shape[0], dtype=LD)
    rows, nz = np.nonzero(H)                                # H is sparse: its zeros are skipped in H X
    vals = H[rows, nz][:, None]
    last = np.inf
    for _ in range(NEWTON_ROUNDS):
        HX = np.zeros_like(X)
        np.add.at(HX, rows, vals * X[nz])
        d = X @ (I - HX)
        X = X + d
        last = float(np.abs(d).max() / np.abs(X).max())
    return X, last


def columns_ld(H, cols):
    """The columns ``cols`` of H^-1 in long double by the refinement loop of pose_graph_ref.step_ld (float64 inverse as
    the approximate solver, long-double residuals; H's zeros are skipped in the residual).  -> (X (3n, len(cols)), last
    correction relative to max |X|)."""
    H = np.asarray(H, dtype=LD)
    N = H.shape[0]
    Hinv = np.linalg.inv(np.asarray(H, dtype=np.float64))
    rows, nz = np.nonzero(H)
    vals = H[rows, nz]
    E = np.zeros((N, len(cols)), dtype=LD)
    E[np.asarray(cols), np.arange(len(cols))] = 1
    x = np.zeros_like(E)
    last = np.inf
    for _ in range(R.REFINE_ROUNDS + 1):
        Hx = np.zeros_like(E)
        np.add.at(Hx, rows, vals[:, None] * x[nz])
        d = Hinv @ np.asarray(E - Hx, dtype=np.float64)
        x = x + d
        last = float(np.abs(d).max() / np.abs(x).max())
    return x, last


def lu_inverse_ld(H):
    """The cross-check: column by column with pose_graph_ref.lu_ld (small systems only)."""
    N = H.shape[0]
    return np.stack([R.lu_ld(H, -np.eye(N, dtype=LD)[:, c]) for c in range(N)], axis=1)


def sample_nodes(n, fix):
    """The nodes whose blocks are checked where the whole inverse is not formed: at most 16."""
    want = [0, n - 1, fix - 1, fix, fix + 1, 255, 256, 511, 512, n // 2, n // 3, 1]
    out = []
    for v in want:
        if 0 <= v < n and v not in out:
            out.append(v)
    return out[:16]


def selection(n, fix):
    """S of the columns tests: the anchor, both ends, the middle twice."""
    return [fix, 0, n - 1, n // 2, n // 2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(n, fix, H, kappa, nodes (the nodes whose block columns are known), cols {w: (3n, 3) float64 of the long-double
    H^-1[:, 3w:3w+3]}, bound {w: block_bound}, last_correction).  Every node for n <= FULL_INVERSE_MAX_N."""
    c = R.cases()[name]
    g = c["graph"]
    n, fix = len(g["nodes"]), c["fix"]
    H, _ = R.assemble_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], fix)
    kappa = R.kappa_inf(H, fix)
    if n <= FULL_INVERSE_MAX_N:
        nodes = list(range(n))
        X, last = inverse_ld(H)
    else:
        nodes = sorted(set(sample_nodes(n, fix) + selection(n, fix)))
        X, last = columns_ld(H, [3 * w + c for w in nodes for c in range(3)])
    cols = {w: X[:, 3 * a:3 * a + 3] for a, w in enumerate(nodes)}
    bound = {w: 3 * n * kappa * U * float(np.abs(cols[w]).max()) for w in nodes}
    return dict(n=n, fix=fix, H=H, kappa=kappa, nodes=nodes, last_correction=last, bound=bound,
                cols={w: np.asarray(x, dtype=np.float64) for w, x in cols.items()}, cols_ld=cols)


def block(ref, v, w):
    """Block (v, w) of the reference inverse, float64 of the long-double value."""
    return ref["cols"][w][3 * v:3 * v + 3]


def worst_ratio(ref, got, v_list, w):
    """max over v of max |got[v] - block(v, w)| / bound[w]; got: {v: (3, 3)} or an (n, 3, 3) array indexed by v."""
    worst = 0.0
    for v in v_list:
        err = np.abs(np.asarray(got[v], dtype=LD) - ref["cols_ld"][w][3 * v:3 * v + 3]).max()
        worst = max(worst, float(err) / ref["bound"][w])
    return worst
