"""Extended-precision reference for the robust pose-graph optimiser — TEST INFRASTRUCTURE ONLY.

Built on tests/pose_graph_ref.py: the losses and their weights in np.longdouble, ``run_robust_ld`` (``ref.run_ld`` with
every masked edge's Omega re-weighted by rho'(chi2) at the start of every iteration) and the bounds a float64 evaluation
in the stated order owes them.  Nothing here comes from the code under test.  NumPy only.

The loss (include/icpmi.h has the same table), s = chi2 = e^T Omega e, c = delta^2:
    huber           rho = s (s <= c), 2 delta sqrt(s) - c     w = 1 (s <= c), delta / sqrt(s)
    cauchy          rho = c log1p(s / c)                      w = c / (c + s)
    geman_mcclure   rho = c s / (c + s)                       w = (c / (c + s))^2

Bounds
  chi2   e = (c dx + s dy) - z: the two differences, cos and sin (a few ulp on the device), two products, a sum and a
         difference — |de_k| <= 8 u (|dx| + |dy| + |z_k|) for the translation rows, and for the angle row, two wraps of
         sums that stay below |theta_i| + |theta_j| + |z_2| + 2 pi, |de_2| <= 8 u of that.  Then Omega e and e . (Omega e),
         two three-term dot products on top of each other (at most 6 roundings on any product):
             |d chi2| <= 8 u |e|^T |Omega| |e| + |de|^T |Omega| |e| + |e|^T |Omega| |de|,
         as total_error_ld bounds the sum.  Where the poses themselves are only known to ``pose_error`` (a device result after
         several iterations), the first-order term pose_error * || d chi2 / d(x_i, x_j) ||_1 is added.
  w      |w'(chi2)| taken at the end of [chi2 - bound, chi2 + bound] where it is largest (every |w'| decreases in s;
         Huber's is 0 below c), times the chi2 bound, plus 4 u w for its own two or three operations.
  cost   per edge w * (chi2 bound) (rho' = w) + 8 u of the magnitude of rho's terms (log1p and sqrt to a few ulp, one
         division; log1p(x) >= x / (1 + x) keeps the division's share below rho), plus m u sum |rho| for any summation order.
  step   ref.step_bound of the re-weighted system, plus the first-order effect of the weight bounds through H_w^-1:
         d(dx) = -H_w^-1 sum_q dw_q J_q^T Omega_q (e_q + J_q dx), bounded by sum_q wb_q || H_w^-1 J_q^T Omega_q (e_q + J_q dx) ||_inf.
"""
import functools

import numpy as np

import pose_graph_ref as ref

LD = ref.LD
U = ref.U
KERNELS = ("huber", "cauchy", "geman_mcclure")
DELTA = 2.7955                          # sqrt(7.8147): the 95 % quantile of chi-square with 3 degrees of freedom


def rho_ld(kernel, s, delta):
    s, d = np.asarray(s, dtype=LD), LD(delta)
    c = d * d
    if kernel == "huber":
        return np.where(s <= c, s, 2 * d * np.sqrt(np.maximum(s, 0)) - c)
    if kernel == "cauchy":
        return c * np.log1p(s / c)
    if kernel == "geman_mcclure":
        return c * s / (c + s)
    raise ValueError(kernel)


def weight_ld(kernel, s, delta):
    s, d = np.asarray(s, dtype=LD), LD(delta)
    c = d * d
    if kernel == "huber":
        return np.where(s <= c, LD(1), d / np.sqrt(np.maximum(s, c)))
    if kernel == "cauchy":
        return c / (c + s)
    if kernel == "geman_mcclure":
        return (c / (c + s)) ** 2
    raise ValueError(kernel)


def weight_slope_ld(kernel, s, delta):
    """|w'(s)|, by hand."""
    s, d = np.asarray(s, dtype=LD), LD(delta)
    c = d * d
    if kernel == "huber":
        return np.where(s < c, LD(0), d / (2 * np.maximum(s, c) ** LD(1.5)))
    if kernel == "cauchy":
        return c / (c + s) ** 2
    if kernel == "geman_mcclure":
        return 2 * c * c / (c + s) ** 3
    raise ValueError(kernel)


def chi2_ld(nodes, ei, ej, z, omega, pose_error=0.0):
    """chi2 per edge in long double and the bound on a float64 evaluation of it (module docstring)."""
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    x, zz = np.asarray(nodes, dtype=LD), np.asarray(z, dtype=LD)
    om = np.asarray(omega, dtype=LD).reshape(-1, 3, 3)
    e, A, B = ref.linearise_ld(x, ei, ej, zz)
    chi2 = np.einsum("ma,mab,mb->m", e, om, e)
    xi, xj = x[ei], x[ej]
    span = np.abs(xj[:, 0] - xi[:, 0]) + np.abs(xj[:, 1] - xi[:, 1])
    de = np.empty_like(e)
    de[:, 0] = 8 * U * (span + np.abs(zz[:, 0]))
    de[:, 1] = 8 * U * (span + np.abs(zz[:, 1]))
    de[:, 2] = 8 * U * (np.abs(xi[:, 2]) + np.abs(xj[:, 2]) + np.abs(zz[:, 2]) + 2 * ref.PI_LD)
    ae, ao = np.abs(e), np.abs(om)
    bound = (8 * U * np.einsum("ma,mab,mb->m", ae, ao, ae) + np.einsum("ma,mab,mb->m", de, ao, ae)
             + np.einsum("ma,mab,mb->m", ae, ao, de))
    if pose_error:
        r = np.einsum("mab,mb->ma", om + om.transpose(0, 2, 1), e)                       # d chi2 / d e
        grad = np.abs(np.einsum("mab,ma->mb", A, r)).sum(axis=1) + np.abs(np.einsum("mab,ma->mb", B, r)).sum(axis=1)
        bound = bound + pose_error * grad
    return chi2, np.asarray(bound, dtype=np.float64)


def evaluate_ld(kernel, delta, nodes, ei, ej, z, omega, mask, pose_error=0.0):
    """-> dict(chi2, chi2_bound, w, w_bound, cost, cost_bound) at ``nodes``; chi2 and w in long double."""
    mask = np.asarray(mask, dtype=bool)
    chi2, cb = chi2_ld(nodes, ei, ej, z, omega, pose_error)
    w = np.where(mask, weight_ld(kernel, chi2, delta), LD(1))
    lo = np.maximum(chi2 - cb, 0)
    if kernel == "huber":                                        # 0 wherever the whole interval is quadratic
        slope = np.where(chi2 + cb <= LD(delta) * LD(delta), LD(0), weight_slope_ld(kernel, np.maximum(lo, LD(delta) * LD(delta)), delta))
    else:
        slope = weight_slope_ld(kernel, lo, delta)
    wb = np.where(mask, np.asarray(slope * cb + 4 * U * w, dtype=np.float64), 0.0)
    rho = np.where(mask, rho_ld(kernel, chi2, delta), chi2)
    mag = np.abs(rho)
    if kernel == "huber":
        c = LD(delta) * LD(delta)
        mag = np.where(mask & (chi2 > c), 2 * LD(delta) * np.sqrt(np.maximum(chi2, 0)) + c, mag)
    cost_bound = float(np.sum(w * cb + 8 * U * mag) + len(chi2) * U * np.sum(np.abs(rho)))
    return dict(chi2=chi2, chi2_bound=cb, w=w, w_bound=wb, cost=float(np.sum(rho)), cost_bound=cost_bound)


def weight_effect_bound(H, dx, nodes, ei, ej, z, omega, wb, fix):
    """sum_q wb_q || H^-1 J_q^T Omega_q (e_q + J_q dx) ||_inf, float64 (a factor of a bound)."""
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    e, A, B = ref.linearise_ld(nodes, ei, ej, z)
    Hinv = np.linalg.inv(np.asarray(H, dtype=np.float64))
    d = np.asarray(dx, dtype=LD).reshape(-1, 3)
    om = np.asarray(omega, dtype=LD).reshape(-1, 3, 3)
    total = 0.0
    for q in np.flatnonzero(np.asarray(wb) > 0):
        i, j = int(ei[q]), int(ej[q])
        r = om[q] @ (e[q] + A[q] @ d[i] + B[q] @ d[j])
        g = np.zeros(H.shape[0])
        if i != fix:
            g[3 * i:3 * i + 3] += np.asarray(A[q].T @ r, dtype=np.float64)
        if j != fix:
            g[3 * j:3 * j + 3] += np.asarray(B[q].T @ r, dtype=np.float64)
        total += float(wb[q]) * float(np.abs(Hinv @ g).max())
    return total


def run_robust_ld(kernel, delta, nodes, ei, ej, z, omega, mask, n_iterations, fix, eps):
    """ref.run_ld with w_q Omega_q of the current poses in every iteration.
    -> dict(iterates, steps, bounds, status, iterations, costs [at the start of every iteration], final [evaluate_ld at the
    last iterate, its bounds widened by the sum of the step bounds])."""
    x = np.array(nodes, dtype=LD).reshape(-1, 3)
    om = np.asarray(omega, dtype=LD).reshape(-1, 3, 3)
    out = dict(iterates=[], steps=[], bounds=[], costs=[], status=ref.MAX_ITERATIONS, iterations=n_iterations)
    for it in range(n_iterations):
        ev = evaluate_ld(kernel, delta, x, ei, ej, z, omega, mask)
        out["costs"].append(ev["cost"])
        omw = om * ev["w"][:, None, None]
        H, b = ref.assemble_ld(x, ei, ej, z, omw, fix)
        dx, _ = ref.step_ld(H, b)
        out["bounds"].append(ref.step_bound(H, fix, dx, x) + weight_effect_bound(H, dx, x, ei, ej, z, omega, ev["w_bound"], fix))
        d = dx.reshape(-1, 3)
        x = x.copy()
        x[:, :2] += d[:, :2]
        x[:, 2] = ref.wrap_ld(x[:, 2] + d[:, 2])
        out["iterates"].append(x)
        out["steps"].append(float(np.sqrt(np.sum(dx * dx))))
        if out["steps"][-1] < eps:
            out["status"], out["iterations"] = ref.OK, it + 1
            break
    out["final"] = evaluate_ld(kernel, delta, x, ei, ej, z, omega, mask, pose_error=sum(out["bounds"]))
    return out


# ── float64 restatement: the condition on the inputs ─────────────────────────────────────────────────────────────────
def step64(kernel, delta, g, mask, fix):
    """One robust step in plain NumPy float64 (weights, assembly edge by edge, LAPACK solve): -> dx (n, 3)."""
    x, z, om = (np.asarray(g[k], dtype=np.float64) for k in ("nodes", "z", "omega"))
    ei, ej = np.asarray(g["ei"], dtype=np.int64), np.asarray(g["ej"], dtype=np.int64)
    xi, xj = x[ei], x[ej]
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    e = np.stack([(c * dx + s * dy) - z[:, 0], (-s * dx + c * dy) - z[:, 1],
                  ref.wrap64(ref.wrap64(xj[:, 2] - xi[:, 2]) - z[:, 2])], axis=1)
    chi2 = np.einsum("ma,mab,mb->m", e, om, e)
    cc = delta * delta
    if kernel == "huber":
        w = np.where(chi2 <= cc, 1.0, delta / np.sqrt(np.maximum(chi2, cc)))
    elif kernel == "cauchy":
        w = cc / (cc + chi2)
    else:
        w = (cc / (cc + chi2)) ** 2
    w = np.where(mask, w, 1.0)
    n = len(x)
    H, b = np.zeros((3 * n, 3 * n)), np.zeros(3 * n)
    for q in range(len(ei)):
        A = np.array([[-c[q], -s[q], -s[q] * dx[q] + c[q] * dy[q]], [s[q], -c[q], -c[q] * dx[q] - s[q] * dy[q]], [0, 0, -1.0]])
        B = np.array([[c[q], s[q], 0], [-s[q], c[q], 0], [0, 0, 1.0]])
        O = om[q] * w[q]
        i, j = 3 * int(ei[q]), 3 * int(ej[q])
        H[i:i + 3, i:i + 3] += A.T @ O @ A
        H[i:i + 3, j:j + 3] += A.T @ O @ B
        H[j:j + 3, i:i + 3] += B.T @ O @ A
        H[j:j + 3, j:j + 3] += B.T @ O @ B
        b[i:i + 3] += A.T @ O @ e[q]
        b[j:j + 3] += B.T @ O @ e[q]
    f = 3 * fix
    H[f:f + 3, :] = 0
    H[:, f:f + 3] = 0
    H[f:f + 3, f:f + 3] = np.eye(3) * 1e10
    b[f:f + 3] = 0
    return np.linalg.solve(H, -b).reshape(-1, 3)


# ── graphs ───────────────────────────────────────────────────────────────────────────────────────────────────────────
def default_mask(g):
    return np.abs(np.asarray(g["ei"]) - np.asarray(g["ej"])) != 1


def false_closure_scenario():
    """A closed loop of 40 nodes (radius about 1.9 m), odometry with noise, four true closures and one false one whose
    measurement is moved by metres; every closure has the same information.  -> (graph, truth (40, 3), index of the false edge)."""
    n = 40
    rng = np.random.default_rng(4040)
    th = 2 * np.pi / n * np.arange(n)
    xy = np.cumsum(np.stack([0.3 * np.cos(th), 0.3 * np.sin(th)], axis=1), axis=0)
    truth = np.column_stack([xy, ref.wrap64(th)])
    est, edges = [truth[0].copy()], []
    for k in range(1, n):
        zt = ref._rel(truth[k - 1], truth[k]) + rng.normal(0.0, 0.01, 3)
        est.append(ref._compose(est[-1], zt))
        edges.append([k - 1, k, zt, np.eye(3) * rng.uniform(100, 1e4)])
    for a, b in ((39, 0), (38, 1), (37, 3), (25, 5)):
        edges.append([a, b, ref._rel(truth[a], truth[b]) + rng.normal(0.0, 0.003, 3), np.eye(3) * 2e4])
    false_edge = len(edges)
    edges.append([30, 10, ref._rel(truth[30], truth[10]) + np.array([3.0, -2.0, 0.5]), np.eye(3) * 2e4])
    g = dict(nodes=np.array(est), ei=np.array([e[0] for e in edges], dtype=np.int64), ej=np.array([e[1] for e in edges], dtype=np.int64),
             z=np.array([e[2] for e in edges]).reshape(-1, 3), omega=np.array([e[3] for e in edges]).reshape(-1, 3, 3), perm=np.arange(n))
    return g, truth, false_edge


def _with_false_closure(g, q, shift):
    g = dict(g)
    g["z"] = g["z"].copy()
    g["z"][q] += shift
    return g


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(graph, fix, mask (bool per edge), path ("split" | "dense"), refused (the split is refused: the call
    continues densely), multi (dict(n_iterations, eps) where the case is also run for several iterations))."""
    out = {}

    def add(name, g, fix, mask=None, path="split", refused=False, multi=None):
        out[name] = dict(graph=g, fix=fix, mask=default_mask(g) if mask is None else np.asarray(mask, dtype=bool), path=path,
                         refused=refused, multi=multi)

    add("n2_masked_chain_edge", ref.make_graph("drive", 2, 1102, guess_noise=0.05), 0, mask=[True], path="dense")
    add("n3_one_closure", ref.make_graph("drive", 3, 1103, [(2, 0)], guess_noise=0.05), 0)
    add("n33_no_closure", ref.make_graph("drive", 33, 1133, guess_noise=0.02), 16)                   # k = 0: an empty mask
    for n in (33, 64, 65):                                       # the odd and even ends of the cyclic reduction
        g = ref.make_graph("drive", n, 1100 + n, ref._closures_for(n))
        add(f"n{n}_false_closure", _with_false_closure(g, len(g["ei"]) - 1, np.array([1.5, -1.0, 0.3])), n // 2)
    g = ref.make_graph("drive", 33, 1134, ref._closures_for(33))
    mask = default_mask(g)
    mask[7] = True                                               # a robust chain edge: the dense path
    add("n33_masked_chain_edge", _with_false_closure(g, 7, np.array([0.5, 0.2, -0.1])), 0, mask=mask, path="dense",
        multi=dict(n_iterations=6, eps=1e-9))
    g = ref.make_graph("drive", 33, 1135, ref._closures_for(33), permute=True)                       # no chain numbering: dense for optimize too
    add("n33_permuted", g, int(g["perm"][4]), path="dense")
    chain = [(k, k + 1) for k in range(199)]
    g = ref.make_graph("circle", 200, 1200, [(199, 0), (150, 20)], extra_chain=chain + chain)       # 599 edges: more than a workgroup
    add("n200_chain_three_times", _with_false_closure(g, len(g["ei"]) - 1, np.array([2.0, 1.0, -0.4])), 100,
        multi=dict(n_iterations=3, eps=1e-9))
    add("weak_twins", ref.cases()["weak_eps1e-08"]["graph"], ref.cases()["weak_eps1e-08"]["fix"])
    add("weak_refused", ref.cases()["weak_zero_matrix"]["graph"], ref.cases()["weak_zero_matrix"]["fix"], path="dense", refused=True)
    g, _, _ = false_closure_scenario()
    add("scenario_false_closure", g, 0, multi=dict(n_iterations=8, eps=1e-8))
    return out


@functools.lru_cache(maxsize=None)
def evaluation(name, kernel):
    c = cases()[name]
    g = c["graph"]
    return evaluate_ld(kernel, DELTA, g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["mask"])


@functools.lru_cache(maxsize=None)
def run(name, kernel, n_iterations, eps):
    c = cases()[name]
    g = c["graph"]
    return run_robust_ld(kernel, DELTA, g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["mask"], n_iterations, c["fix"], eps)
