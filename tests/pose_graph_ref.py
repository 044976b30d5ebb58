"""Extended-precision reference for ONE Gauss-Newton step of the pose-graph optimiser — TEST INFRASTRUCTURE ONLY.

Restates oracle/pose_graph.py edge by edge in np.longdouble from the float64 inputs, solves the step to well below
float64 rounding, and states what a backward-stable float64 solver owes that step (``step_bound``).  NumPy only.
Used by tests/test_pose_graph_step_cpu.py (which pins this helper against the oracle and proves the conditions on the
cases) and by tests/test_pose_graph_step_gpu.py (the kernel against the same references and bounds).
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI_LD = LD(np.pi)                       # the reference wraps with float64 np.pi; carried exactly
OK, MAX_ITERATIONS, SINGULAR = 1, 2, 3
REFINE_ROUNDS = 4


def wrap64(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def wrap_ld(a):
    return (a + PI_LD) % (2 * PI_LD) - PI_LD


def linearise_ld(nodes, ei, ej, z):
    """oracle.pose_graph.linearise in long double: e (m,3), A (m,3,3), B (m,3,3)."""
    nodes, z = np.asarray(nodes, dtype=LD), np.asarray(z, dtype=LD)
    xi, xj = nodes[ei], nodes[ej]
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    m = len(ei)
    e = np.empty((m, 3), dtype=LD)
    e[:, 0] = (c * dx + s * dy) - z[:, 0]
    e[:, 1] = (-s * dx + c * dy) - z[:, 1]
    e[:, 2] = wrap_ld(wrap_ld(xj[:, 2] - xi[:, 2]) - z[:, 2])
    A = np.zeros((m, 3, 3), dtype=LD)
    B = np.zeros((m, 3, 3), dtype=LD)
    A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1] = -c, -s, s, -c
    A[:, 0, 2] = -s * dx + c * dy
    A[:, 1, 2] = -c * dx - s * dy
    A[:, 2, 2] = -1
    B[:, 0, 0], B[:, 0, 1], B[:, 1, 0], B[:, 1, 1] = c, s, -s, c
    B[:, 2, 2] = 1
    return e, A, B


def assemble_ld(nodes, ei, ej, z, omega, fix):
    """H (3n,3n) and b (3n) of oracle.pose_graph.optimize's iteration, in long double, edge by edge, with its anchor."""
    n = len(nodes)
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    om = np.asarray(omega, dtype=LD).reshape(-1, 3, 3)
    e, A, B = linearise_ld(nodes, ei, ej, z)
    H = np.zeros((3 * n, 3 * n), dtype=LD)
    b = np.zeros(3 * n, dtype=LD)
    for q in range(len(ei)):
        i, j = 3 * int(ei[q]), 3 * int(ej[q])
        AtO, BtO = A[q].T @ om[q], B[q].T @ om[q]
        H[i:i + 3, i:i + 3] += AtO @ A[q]
        H[i:i + 3, j:j + 3] += AtO @ B[q]
        H[j:j + 3, i:i + 3] += BtO @ A[q]
        H[j:j + 3, j:j + 3] += BtO @ B[q]
        b[i:i + 3] += AtO @ e[q]
        b[j:j + 3] += BtO @ e[q]
    f = 3 * fix
    H[f:f + 3, :] = 0
    H[:, f:f + 3] = 0
    H[f:f + 3, f:f + 3] = np.eye(3, dtype=LD) * LD(1e10)
    b[f:f + 3] = 0
    return H, b


def step_ld(H, b):
    """dx with H dx = -b: float64 inverse as the approximate solver, REFINE_ROUNDS rounds of refinement with long-double
    residuals.  Returns (dx in long double, max |last correction|)."""
    Hinv = np.linalg.inv(np.asarray(H, dtype=np.float64))
    rhs = -b
    x = np.zeros(len(b), dtype=LD)
    last = np.inf
    for _ in range(REFINE_ROUNDS + 1):                   # the first round is the float64 solve itself
        r = rhs - H @ x
        d = Hinv @ np.asarray(r, dtype=np.float64)
        x = x + d
        last = float(np.abs(d).max())
    return x, last


def lu_ld(H, b):
    """The cross-check: plain long-double LU with partial pivoting (small systems only)."""
    a = np.array(H, dtype=LD)
    x = np.array(-b, dtype=LD)
    N = len(x)
    for p in range(N):
        r = p + int(np.argmax(np.abs(a[p:, p])))
        if a[r, p] == 0:
            raise np.linalg.LinAlgError("singular")
        if r != p:
            a[[p, r]] = a[[r, p]]
            x[[p, r]] = x[[r, p]]
        l = a[p + 1:, p] / a[p, p]
        a[p + 1:, p:] -= l[:, None] * a[p, p:][None, :]
        x[p + 1:] -= l * x[p]
    for r in range(N - 1, -1, -1):
        x[r] = (x[r] - a[r, r + 1:] @ x[r + 1:]) / a[r, r]
    return x


def kappa_inf(H, fix):
    """Infinity-norm condition number of H without the anchor's rows and columns (float64 is plenty for a factor)."""
    keep = np.ones(H.shape[0], dtype=bool)
    keep[3 * fix:3 * fix + 3] = False
    Hr = np.asarray(H, dtype=np.float64)[np.ix_(keep, keep)]
    return float(np.linalg.cond(Hr, np.inf))


def step_bound(H, fix, dx_ref, nodes):
    """What a backward-stable float64 solve of this 3n x 3n system owes the exact step (the textbook forward bound), plus
    the rounding of reading a step back as nodes_after - nodes_before.  Nothing here comes from the code under test."""
    n3 = H.shape[0]
    return (n3 * kappa_inf(H, fix) * U * float(np.abs(dx_ref).max())
            + 4 * U * float(np.abs(np.asarray(nodes, dtype=np.float64)).max()))


def run_ld(nodes, ei, ej, z, omega, n_iterations, fix, eps):
    """oracle.pose_graph.optimize's loop wholly in long double.
    -> dict(iterates [nodes after every iteration], steps [norms], bounds [step_bound per iteration], status, iterations)."""
    x = np.array(nodes, dtype=LD).reshape(-1, 3)
    out = dict(iterates=[], steps=[], bounds=[], status=MAX_ITERATIONS, iterations=n_iterations)
    for it in range(n_iterations):
        H, b = assemble_ld(x, ei, ej, z, omega, fix)
        dx, _ = step_ld(H, b)
        out["bounds"].append(step_bound(H, fix, dx, x))
        d = dx.reshape(-1, 3)
        x = x.copy()
        x[:, :2] += d[:, :2]
        x[:, 2] = wrap_ld(x[:, 2] + d[:, 2])
        out["iterates"].append(x)
        out["steps"].append(float(np.sqrt(np.sum(dx * dx))))
        if out["steps"][-1] < eps:
            out["status"], out["iterations"] = OK, it + 1
            break
    return out


def total_error_ld(nodes, ei, ej, z, omega):
    """sum of e^T Omega e in edge order, and the bound m 2^-53 sum |e|^T |Omega| |e| on a float64 evaluation."""
    e, _, _ = linearise_ld(nodes, np.asarray(ei), np.asarray(ej), z)
    om = np.asarray(omega, dtype=LD).reshape(-1, 3, 3)
    tot = np.einsum("ma,mab,mb->", e, om, e)
    mag = np.einsum("ma,mab,mb->", np.abs(e), np.abs(om), np.abs(e))
    return float(tot), len(ei) * U * float(mag)


# ── graphs ───────────────────────────────────────────────────────────────────────────────────────────────────────────
def _rel(a, b):
    """z_ab = a^-1 b for poses [x, y, theta]."""
    c, s = np.cos(a[2]), np.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, wrap64(b[2] - a[2])])


def _compose(a, z):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * z[0] - s * z[1], a[1] + s * z[0] + c * z[1], wrap64(a[2] + z[2])])


def _information(rng, kind):
    if kind == "iso":
        return np.eye(3) * rng.uniform(100, 1e4)
    g = rng.normal(size=(3, 3))
    if kind == "full":                                   # symmetric positive definite, not diagonal
        return g @ g.T * 300 + np.eye(3) * 100
    if kind == "nonsym":                                 # symmetric positive definite plus a skew part
        k = rng.normal(size=(3, 3)) * 20
        return g @ g.T * 300 + np.eye(3) * 100 + (k - k.T)
    if kind == "indef":                                  # anything the reference accepts
        return g * 100
    raise ValueError(kind)


def make_graph(shape, n, seed, closures=(), info="iso", special_every=0, weak=None, angle_offset=0.0, xy_offset=0.0,
               angle_add=None, extra_chain=(), drop_chain=(), permute=False, guess_noise=0.0, noise_scale=1.0):
    """A chain 0-1-...-(n-1) with closure edges, seeded and deterministic.
    shape: "drive" (a wandering chain) or "circle" (heading advances 2 pi / 64 per node, steps of 0.3: bounded extent).
    info: information kind of every ``special_every``-th edge (all other edges "iso"); weak: {c: Omega} replaces the
    information of chain edge (c, c + 1); extra_chain: (i, j) pairs of adjacent nodes listed once more; drop_chain:
    chain edges left out; permute: renumber the nodes at random (no chain numbering left: the dense path)."""
    rng = np.random.default_rng(seed)
    if shape == "drive":
        th = np.cumsum(rng.normal(0.0, 0.1, n))
    elif shape == "circle":
        th = 2 * np.pi / 64 * np.arange(n)
    else:
        raise ValueError(shape)
    th = th + angle_offset
    xy = np.cumsum(np.stack([0.3 * np.cos(th), 0.3 * np.sin(th)], axis=1), axis=0) + xy_offset
    truth = np.column_stack([xy, wrap64(th)])
    est = [truth[0].copy()]
    edges = []
    weak = weak or {}
    for k in range(1, n):
        zt = _rel(truth[k - 1], truth[k]) + rng.normal(0.0, 0.01 * noise_scale, 3)
        est.append(_compose(est[-1], zt))
        om = np.eye(3) * rng.uniform(100, 1e4)
        if (k - 1) in weak:
            om = np.array(weak[k - 1], dtype=np.float64)
        if (k - 1) not in drop_chain:
            edges.append([k - 1, k, zt, om])
    for a, b in extra_chain:
        edges.append([a, b, _rel(truth[a], truth[b]) + rng.normal(0.0, 0.01, 3), np.eye(3) * rng.uniform(100, 1e4)])
    for a, b in closures:
        edges.append([a, b, _rel(truth[a], truth[b]) + rng.normal(0.0, 0.003 * noise_scale, 3), np.eye(3) * 2e4])
    if special_every:
        for q in range(2, len(edges), special_every):
            if edges[q][0] + 1 == edges[q][1] and edges[q][0] in weak:
                continue
            edges[q][3] = _information(rng, info)
    nodes = np.array(est)
    if guess_noise:
        nodes = nodes + rng.normal(0.0, guess_noise, nodes.shape)
    for k, v in (angle_add or {}).items():
        nodes[k, 2] += v
    ei = np.array([e[0] for e in edges], dtype=np.int64)
    ej = np.array([e[1] for e in edges], dtype=np.int64)
    z = np.array([e[2] for e in edges]).reshape(-1, 3)
    om = np.array([e[3] for e in edges]).reshape(-1, 3, 3)
    perm = np.arange(n)
    if permute:
        perm = rng.permutation(n)                        # node k of the chain is node perm[k]
        shuffled = np.empty_like(nodes)
        shuffled[perm] = nodes
        nodes, ei, ej = shuffled, perm[ei], perm[ej]
    return dict(nodes=nodes, ei=ei, ej=ej, z=z, omega=om, perm=perm)


def _closures_for(n):
    c = []
    if n >= 4:
        c.append((n - 1, 0))
    if n >= 7:
        c += [(n - 2, 1), (n // 2, n // 2 - 2)]
    return c


def _circle_closures(n):
    return [(k, k - 64) for k in range(64, n, 16)] + [(n - 1, 0)]


def _wide_closures(n, fix, count, seed):
    """``count`` closures, none between consecutive nodes: a self-edge, a duplicate, one pair in both directions, two
    that end on the anchor, the rest random."""
    rng = np.random.default_rng(seed)
    c = [(50, 50), (120, 30), (120, 30), (60, 140), (140, 60), (fix, 100), (150, fix)]
    while len(c) < count:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) >= 2:
            c.append((a, b))
    return c


WEAK_EPS = (1.0, 1e-2, 1e-4, 1e-6, 1e-8, 1e-12, 0.0)
WEAK_CLOSURES = [(32, 0), (15, 5), (28, 18)]


def _weak(eps):
    return np.diag([eps, 1e4, 1e4])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(family, kind ("step" | "singular" | "multi" ), graph, fix).  ``fix`` is in the graph's own numbering."""
    out = {}

    def add(name, family, graph, fix, kind="step", **kw):
        out[name] = dict(family=family, kind=kind, graph=graph, fix=int(graph["perm"][fix]), **kw)

    for n in (2, 3, 4, 5, 7, 8, 9, 33):
        for fix in sorted({0, n // 2, n - 1}):
            add(f"cr_n{n}_fix{fix}", "cyclic reduction", make_graph("drive", n, 100 + n, _closures_for(n)), fix)
    for n in (513, 600):
        for fix in (n // 2, n - 1):
            add(f"circle_n{n}_fix{fix}", "more nodes than threads", make_graph("circle", n, 200 + n, _circle_closures(n)), fix)
    add("closures_171", "closure system wider than 512", make_graph("circle", 200, 301, _wide_closures(200, 7, 171, 302)), 7)
    add("dense_540", "dense wider than 512", make_graph("circle", 180, 401, _circle_closures(180), permute=True), 11)
    add("dense_540_gap", "dense wider than 512",
        make_graph("circle", 180, 401, _circle_closures(180) + [(99, 101)], drop_chain=(100,), permute=True), 11)
    add("chain_twice_and_reversed", "edge forms", make_graph("drive", 12, 501, _closures_for(12), extra_chain=[(3, 4), (6, 5)]), 2)
    for kind in ("full", "nonsym", "indef"):
        add(f"info_{kind}", "edge forms", make_graph("drive", 12, 510, _closures_for(12), info=kind, special_every=3), 4)
    add("info_indef_dense", "edge forms",
        make_graph("drive", 12, 510, _closures_for(12), info="indef", special_every=3, permute=True), 4)
    add("branch_cut", "angles and magnitudes", make_graph("drive", 20, 601, _closures_for(20), angle_offset=np.pi - 0.05), 0)
    add("angles_out_of_range", "angles and magnitudes",
        make_graph("drive", 20, 602, _closures_for(20), angle_add={3: 7.0, 11: -100.0, 19: 7.0}), 5)
    add("offset_1e5", "angles and magnitudes", make_graph("drive", 20, 603, _closures_for(20), xy_offset=1e5), 0)
    for eps in WEAK_EPS:
        add(f"weak_eps{eps:g}", "weak chain edges",
            make_graph("drive", 33, 700, WEAK_CLOSURES, weak={10: _weak(eps), 22: _weak(eps)}), 0)
    add("weak_zero_matrix", "weak chain edges",
        make_graph("drive", 33, 700, WEAK_CLOSURES, weak={10: np.zeros((3, 3)), 22: np.zeros((3, 3))}), 0)
    add("weak_last_node", "weak chain edges", make_graph("drive", 33, 700, WEAK_CLOSURES, weak={31: np.zeros((3, 3))}), 0)
    for name, permute in (("singular_chain", False), ("singular_dense", True)):
        add(name, "singular", make_graph("drive", 33, 800, WEAK_CLOSURES, weak={19: np.zeros((3, 3)), 20: np.zeros((3, 3))},
                                         permute=permute), 0, kind="singular")
    # measurement noise scaled down: Gauss-Newton then converges fast enough for a step above 1e-8 to be followed by one
    # below 1e-10 (seeds chosen for that; tests/test_pose_graph_step_cpu.py proves it), so eps = 1e-9 decides nothing by rounding
    for n, seed in ((9, 912), (33, 934)):
        cl = _closures_for(n) if n == 9 else WEAK_CLOSURES
        add(f"multi_n{n}_healthy", "several iterations",
            make_graph("drive", n, seed, cl, guess_noise=0.1, noise_scale=0.03), 0, kind="multi", n_iterations=25, eps=1e-9)
        add(f"multi_n{n}_weak", "several iterations",
            make_graph("drive", n, seed, cl, weak={n // 3: _weak(1e-8), 2 * n // 3: _weak(1e-8)}, guess_noise=0.1,
                       noise_scale=0.03), 0, kind="multi", n_iterations=25, eps=1e-9)
    return out


def exact_single_edge():
    """m = 1 for total_error.  Its bound, 1 * 2^-53 * |e|^T |Omega| |e|, leaves no room for the rounding of e itself, so
    this graph is one whose float64 evaluation is exact: headings 0 (cos = 1, sin = 0, the wraps return 0), dyadic
    coordinates and a small-integer information matrix.  A correct evaluation returns 48.625 to the bit."""
    return dict(nodes=np.array([[0.5, -0.25, 0.0], [2.0, 1.0, 0.0]]), ei=np.array([0]), ej=np.array([1]),
                z=np.array([[0.25, 0.5, 0.0]]), omega=np.array([[[16.0, 3.0, 1.0], [3.0, 32.0, -2.0], [1.0, -2.0, 8.0]]]))


def case_names(kind):
    return [k for k, c in cases().items() if c["kind"] == kind]


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """The exact first step of a case: dict(dx (n,3) float64 of the long-double step, norm, bound, kappa, last_correction, H, b)."""
    c = cases()[name]
    g = c["graph"]
    H, b = assemble_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["fix"])
    dx, last = step_ld(H, b)
    return dict(dx=np.asarray(dx, dtype=np.float64).reshape(-1, 3), norm=float(np.sqrt(np.sum(dx * dx))),
                bound=step_bound(H, c["fix"], dx, g["nodes"]), kappa=kappa_inf(H, c["fix"]), last_correction=last,
                H=H, b=b, dx_ld=dx)


@functools.lru_cache(maxsize=None)
def run_reference(name):
    c = cases()[name]
    g = c["graph"]
    return run_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["n_iterations"], c["fix"], c["eps"])


def step_difference(after, before):
    """A step read back from the poses, the angle difference wrapped."""
    d = np.asarray(after, dtype=np.float64) - np.asarray(before, dtype=np.float64)
    d[:, 2] = wrap64(d[:, 2])
    return d
