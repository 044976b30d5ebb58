"""utilities.pose_graph — the reference's 2-D pose-graph optimiser
(/root/reference/utilities/pose_graph.py) with the same names and behaviour; the
Gauss-Newton optimisation runs on the MI355X in one launch (csrc/posegraph.hip).

Nodes are poses [x, y, theta]; edges are relative-pose measurements with 3x3
information matrices.  After ``optimize()`` read ``nodes`` or
``get_poses_as_matrices()``.  ``last_info`` holds what the reference only
prints: iterations run, status and the norm of the last step, and in
``phase_us`` the kernel's device clocks in microseconds, summed over the
iterations, under ``PHASE_KEYS``.  Two keys are older than what they time:
``chain_lu`` is the building of the closure columns W and ``chain_sweeps`` the
whole chain solve (the cyclic reduction of T, which is its factorisation, and
the back substitution).  On the dense path the four clocks between
``assemble`` and ``dx`` stay 0 and the whole elimination is in ``dx``.  The private
per-edge helper ``_error_and_jacobians`` (pose_graph.py:138-182) has no host
counterpart here: edges are linearised inside the kernels.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from icpmi import _lib
from icpmi import batch as _b

VERBOSE = True      # the reference prints one line per optimisation

NOTHING_TO_DO, CONVERGED, MAX_ITERATIONS, SINGULAR = _lib.PG_ST_NOTHING, _lib.PG_ST_CONVERGED, _lib.PG_ST_MAXITER, _lib.PG_ST_SINGULAR
_SPLIT_REFUSED = _lib.PG_ST_REFUSED   # device status only: the chain part of the split is exactly singular, go on with the dense matrix
_ITERATIONS, _STATUS, _STEP = _lib.PGINFO_ITERATIONS, _lib.PGINFO_STATUS, _lib.PGINFO_STEP
_PHASES = slice(_lib.PGINFO_PHASE_US, _lib.PGINFO_PHASE_US + _lib.PGINFO_PHASES)
PHASE_KEYS = ("assemble", "chain_lu", "chain_sweeps", "closure_system", "closure_solve", "dx", "apply")    # in slot order
ROBUST_KERNELS = {"huber": _lib.ROB_KERNEL_HUBER, "cauchy": _lib.ROB_KERNEL_CAUCHY, "geman_mcclure": _lib.ROB_KERNEL_GEMAN_MCCLURE}


def normalize_angle(a):
    """pose_graph.py:15-17: wrap to [-pi, pi)."""
    return (a + np.pi) % (2 * np.pi) - np.pi


def pose_matrix_to_vec(T):
    """pose_graph.py:20-22: 3x3 homogeneous matrix -> [x, y, theta]."""
    return np.array([T[0, 2], T[1, 2], np.arctan2(T[1, 0], T[0, 0])])


def pose_vec_to_matrix(v):
    """pose_graph.py:25-31."""
    x, y, theta = v
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, x], [s, c, y], [0, 0, 1]])


def relative_transform_vec(T_i, T_j):
    """pose_graph.py:34-37: z_ij = T_i^-1 T_j as [dx, dy, dtheta]."""
    return pose_matrix_to_vec(np.linalg.inv(T_i) @ T_j)


def _print_outcome(status, iters, step, n_iterations):
    """The reference's one line per optimisation (pose_graph.py:118, 131-134)."""
    if status == SINGULAR:
        print(f"  PoseGraph: singular H at iter {iters}, stopping")
    elif status == CONVERGED:
        print(f"  PoseGraph converged: iter={iters - 1}, ||Δx||={step:.2e}")
    elif status == MAX_ITERATIONS:
        print(f"  PoseGraph max iterations: iter={n_iterations}, ||Δx||={step:.2e}")


def _continued(launch, n_iterations=None, dense=False, status_slot=_STATUS):
    """``launch(dense, iterations)`` -> info record, run with the continuation every plan entry has: a split that is
    refused (``_SPLIT_REFUSED``: before its first iteration by the plan, or in one where a block turns out exactly singular)
    leaves the poses of the iteration before, and the remaining iterations take the dense matrix.  Returns (record, the
    refused launch's record or None); the two records of an optimiser (``n_iterations`` given) are merged here:
    iterations and clocks add up, the step is the split's where the dense run is singular at once, and a robust record
    keeps the cost of the poses given unless the split was refused at once, where the dense launch has it."""
    info = launch(dense, n_iterations)
    if int(info[status_slot]) != _SPLIT_REFUSED:
        return info, None
    if n_iterations is None:
        return launch(True, None), info
    first, info = info, launch(True, n_iterations - int(info[_ITERATIONS]))
    info[_ITERATIONS] += first[_ITERATIONS]
    info[_PHASES] += first[_PHASES]
    if int(info[_ITERATIONS]) == int(first[_ITERATIONS]):
        info[_STEP] = first[_STEP]
    if len(info) == _lib.ROB_DOUBLES:
        info[_lib.ROB_WEIGHTS_US] += first[_lib.ROB_WEIGHTS_US]
        if int(first[_ITERATIONS]) > 0:
            info[_lib.ROB_COST_BEFORE] = first[_lib.ROB_COST_BEFORE]
    return info, first


def _info_dict(info, first):
    """``last_info`` of an optimiser's (merged) record."""
    return dict(iterations=int(info[_ITERATIONS]), status=int(info[_STATUS]), step_norm=float(info[_STEP]),
                split_refused_at=None if first is None else int(first[_ITERATIONS]),
                phase_us=dict(zip(PHASE_KEYS, info[_PHASES].tolist())))


class Marginals:
    """What ``PoseGraph2D.marginals`` returns: blocks of H^-1 (no counterpart in the reference).
    ``diagonal``: (n, 3, 3) block (v, v) of every node, or None; ``nodes``: the selected nodes, negative indices resolved;
    ``columns``: (s, n, 3, 3), ``columns[a, v]`` is block (v, nodes[a]), or None; ``status``; ``path``: "split" or "dense"."""

    def __init__(self, poses, fix_node, nodes, diagonal, columns, status, path):
        self.poses, self.fix_node, self.nodes = poses, fix_node, list(nodes)
        self.diagonal, self.columns, self.status, self.path = diagonal, columns, status, path

    def _node(self, v):
        n = len(self.poses)
        v = int(v)
        v = v + n if v < 0 else v
        if not 0 <= v < n:
            raise IndexError("list index out of range")
        return v

    def block(self, v, w):
        """Block (v, w) of H^-1: needs ``w`` among ``nodes``, or ``v == w`` and the diagonal."""
        v, w = self._node(v), self._node(w)
        if self.columns is not None and w in self.nodes:
            return self.columns[self.nodes.index(w), v]
        if v == w and self.diagonal is not None:
            return self.diagonal[v]
        raise KeyError(f"block ({v}, {w}) was not computed: pass nodes=[..., {w}] to marginals()")

    def joint(self, i, j):
        """The 6 x 6 joint marginal [[S_ii, S_ij], [S_ji, S_jj]] of two selected nodes."""
        i, j = self._node(i), self._node(j)
        if self.columns is None or i not in self.nodes or j not in self.nodes:
            raise KeyError(f"joint({i}, {j}) needs both nodes among marginals(nodes=...)")
        return np.block([[self.block(i, i), self.block(i, j)], [self.block(j, i), self.block(j, j)]])

    def relative_jacobians(self, i, j):
        """A = d z_ij / d x_i and B = d z_ij / d x_j at the poses the marginals were taken at (pose_graph.py:165-178)."""
        xi, xj = self.poses[self._node(i)], self.poses[self._node(j)]
        c, s = np.cos(xi[2]), np.sin(xi[2])
        dx, dy = xj[0] - xi[0], xj[1] - xi[1]
        A = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
        B = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        return A, B

    def relative(self, i, j):
        """Covariance A S_ii A^T + A S_ij B^T + B S_ji A^T + B S_jj B^T of the predicted measurement z_ij (3 x 3)."""
        J = np.hstack(self.relative_jacobians(i, j))
        return J @ self.joint(i, j) @ J.T


class PoseGraph2D:
    """pose_graph.py:42-194.  ``nodes`` is a list of (3,) arrays and ``edges`` a list of
    ``(i, j, z_ij, omega)`` tuples, as in the reference; both may be edited freely between calls."""

    def __init__(self):
        self.nodes = []
        self.edges = []
        self.last_info = {}
        self.last_robust = {}

    def add_node(self, pose_vec):
        self.nodes.append(np.asarray(pose_vec, dtype=float).copy())
        return len(self.nodes) - 1

    def add_edge(self, i, j, measurement, information=None):
        z = np.asarray(measurement, dtype=float).copy()
        omega = np.eye(3) if information is None else np.asarray(information, dtype=float).copy()
        self.edges.append((i, j, z, omega))

    # ── device staging ────────────────────────────────────────────────────
    def _edge_arrays(self):
        m, n = len(self.edges), len(self.nodes)
        ij = np.empty((m, 2), dtype=np.int32)
        z = np.empty((m, 3))
        om = np.empty((m, 3, 3))
        for q, (i, j, zz, o) in enumerate(self.edges):
            i, j = int(i), int(j)
            if i < 0:                    # Python list indexing semantics of the reference
                i += n
            if j < 0:
                j += n
            if not (0 <= i < n and 0 <= j < n):
                raise IndexError("list index out of range")
            ij[q] = (i, j)
            z[q] = zz
            om[q] = o
        return ij, z, om

    def _stage(self, fix_node=0, edge_weights=None):
        """What every device entry takes, staged once: the sizes, the anchor (a negative index counts from the end), the
        device, the poses / z / Omega on the host and on the device, and the host pointers of the edge list and of Omega
        (``edge_weights``: Omega times one weight per edge)."""
        _b.require_gpu()
        t = SimpleNamespace(n=len(self.nodes), dev=torch.device("cuda", torch.cuda.current_device()))
        t.ij, t.z, t.om = self._edge_arrays()
        t.m = len(t.ij)
        if edge_weights is not None:
            w = np.asarray(edge_weights, dtype=np.float64)
            if w.shape != (t.m,):
                raise ValueError(f"edge_weights needs one weight per edge ({t.m}), got shape {w.shape}")
            t.om = np.ascontiguousarray(t.om * w[:, None, None])
        t.fix = int(fix_node + t.n if fix_node < 0 else fix_node)
        t.poses = np.ascontiguousarray(np.array(self.nodes, dtype=np.float64).reshape(t.n, 3))
        t.d_nodes, t.d_z, t.d_om = (torch.from_numpy(a).to(t.dev) for a in (t.poses, t.z, t.om))
        t.ijp, t.omp = t.ij.ctypes.data_as(C.c_void_p), t.om.ctypes.data_as(C.c_void_p)
        return t

    @staticmethod
    def _launch(t, what, entry, size, d_info, *args):
        """One call of a plan entry — ``entry(nodes, edges, z, Omega, *args, info, workspace, its size, stream)`` — in a
        workspace of ``size`` bytes.  Returns the info record."""
        ws = torch.empty(max(int(size), 256), dtype=torch.uint8, device=t.dev)
        _lib.check(entry(_b._ptr(t.d_nodes), t.ijp, _b._ptr(t.d_z), _b._ptr(t.d_om), *args, _b._ptr(d_info), _b._ptr(ws), ws.numel(),
                         _b._stream()), what)
        return d_info.cpu().numpy()

    def _take(self, t):
        out = t.d_nodes.cpu().numpy()
        for k in range(t.n):                                 # in place, like pose_graph.py:122-125
            self.nodes[k][:] = out[k]

    def optimize(self, n_iterations=20, fix_node=0, convergence_eps=1e-6):
        """pose_graph.py:83-134: Gauss-Newton with the pose at ``fix_node`` held constant."""
        if len(self.nodes) < 2 or len(self.edges) == 0:
            return
        t, L = self._stage(fix_node), _lib.lib()
        d_info = torch.zeros(_lib.PGINFO_DOUBLES, dtype=torch.float64, device=t.dev)

        def launch(dense, iterations):
            # sized with the information matrices: room for the twins of weak chain edges
            size = (L.icpmi_pose_graph_dense_workspace_bytes(t.ijp, t.n, t.m) if dense
                    else L.icpmi_pose_graph_weighted_workspace_bytes(t.ijp, t.omp, t.n, t.m))
            return self._launch(t, "PoseGraph2D.optimize", L.icpmi_pose_graph_optimize_dense if dense else L.icpmi_pose_graph_optimize,
                                size, d_info, t.n, t.m, iterations, t.fix, float(convergence_eps))

        info, first = _continued(launch, int(n_iterations))
        self._take(t)
        self.last_info = _info_dict(info, first)
        if VERBOSE:
            _print_outcome(int(info[_STATUS]), int(info[_ITERATIONS]), info[_STEP], n_iterations)

    # ── robust edges (no counterpart in the reference) ────────────────────
    def _robust_mask(self, ij, edges):
        """uint8 mask over the edge list: ``edges`` is an iterable of edge indices or a boolean mask; None = every edge that
        does not join consecutive nodes (the loop closures)."""
        m = len(ij)
        if edges is None:
            return np.ascontiguousarray((np.abs(ij[:, 0] - ij[:, 1]) != 1).astype(np.uint8))
        e = np.asarray(list(edges) if not isinstance(edges, np.ndarray) else edges)
        mask = np.zeros(m, dtype=np.uint8)
        if e.dtype == np.bool_:
            if e.shape != (m,):
                raise ValueError(f"a boolean edge mask needs one entry per edge ({m}), got shape {e.shape}")
            mask[e] = 1
        elif e.size:
            idx = e.astype(np.int64)
            if e.ndim != 1 or np.any(idx != e) or np.any(idx < -m) or np.any(idx >= m):
                raise IndexError("edge index out of range")
            mask[idx] = 1
        return mask

    def _run_robust(self, what, n_iterations, fix_node, convergence_eps, kernel, delta, edges):
        """The robust entry on the current graph.  -> (the staging, merged info record, the refused launch's record or
        None, chi2, weights, mask)."""
        if kernel not in ROBUST_KERNELS:
            raise ValueError(f"unknown robust kernel {kernel!r}: one of {sorted(ROBUST_KERNELS)}")
        if not float(delta) > 0.0:
            raise ValueError(f"delta must be > 0, got {delta!r}")
        t, L = self._stage(fix_node), _lib.lib()
        mask = self._robust_mask(t.ij, edges)
        maskp = mask.ctypes.data_as(C.c_void_p)
        d_info = torch.zeros(_lib.ROB_DOUBLES, dtype=torch.float64, device=t.dev)
        d_chi2, d_wgt = (torch.zeros(t.m, dtype=torch.float64, device=t.dev) for _ in range(2))

        def launch(dense, iterations):
            return self._launch(t, what, L.icpmi_pose_graph_optimize_robust,
                                L.icpmi_pose_graph_robust_workspace_bytes(t.ijp, t.omp, maskp, t.n, t.m, int(dense)), d_info,
                                maskp, t.n, t.m, iterations, t.fix, float(convergence_eps), ROBUST_KERNELS[kernel], float(delta),
                                int(dense), _b._ptr(d_chi2), _b._ptr(d_wgt))

        info, first = _continued(launch, int(n_iterations))
        return t, info, first, d_chi2.cpu().numpy(), d_wgt.cpu().numpy(), mask.astype(bool)

    def optimize_robust(self, n_iterations=20, fix_node=0, convergence_eps=1e-6, kernel="huber", delta=2.7955, edges=None):
        """``optimize`` with a robust loss on some edges: Gauss-Newton on sum of chi2 over the plain edges plus sum of
        rho(chi2) over the robust ones, chi2 = e^T Omega e, by re-weighting every robust edge's Omega with rho'(chi2) at the
        start of every iteration.  ``kernel``: "huber", "cauchy" or "geman_mcclure" (include/icpmi.h has the table);
        ``delta``: chi2 = delta^2 is where the loss leaves the quadratic — the default is sqrt(7.8147), the 95 % quantile of
        chi-square with 3 degrees of freedom; ``edges``: indices or a boolean mask of the robust edges, None = every edge that
        does not join consecutive nodes.  A robust edge between consecutive nodes sends the graph down the dense path.
        Sets ``last_info`` as ``optimize`` does, plus ``cost_before`` / ``cost_after`` (the loss at the poses given and
        returned), ``weights_us`` and ``path``; and ``last_robust`` = dict(chi2, weights, mask, kernel, delta), chi2 and
        weights per edge at the returned poses."""
        n = len(self.nodes)
        if n < 2 or len(self.edges) == 0:
            return
        t, info, first, chi2, weights, mask = self._run_robust("PoseGraph2D.optimize_robust", n_iterations, fix_node,
                                                               convergence_eps, kernel, delta, edges)
        self._take(t)
        # the plan's path rule (pg_plan, csrc/posegraph.hip) restated: the split needs every pair of consecutive nodes joined
        # by an edge, none of those edges robust; a refused split went on densely
        chained = np.abs(t.ij[:, 0] - t.ij[:, 1]) == 1
        dense = (first is not None or bool(mask[chained].any())
                 or len(set(np.minimum(t.ij[chained, 0], t.ij[chained, 1]).tolist())) < n - 1)
        self.last_info = dict(_info_dict(info, first),
                              cost_before=float(info[_lib.ROB_COST_BEFORE]), cost_after=float(info[_lib.ROB_COST_AFTER]),
                              weights_us=float(info[_lib.ROB_WEIGHTS_US]), path="dense" if dense else "split")
        self.last_robust = dict(chi2=chi2, weights=weights, mask=mask, kernel=kernel, delta=float(delta))
        if VERBOSE:
            _print_outcome(int(info[_STATUS]), int(info[_ITERATIONS]), info[_STEP], n_iterations)

    def robust_cost(self, kernel, delta, edges=None):
        """(cost, chi2, weights) of the robust loss at the current poses (``optimize_robust`` names the arguments): the
        evaluation-only call, nothing is moved.  (0.0, empty, empty) for a graph without edges."""
        if len(self.nodes) < 2 or len(self.edges) == 0:
            return 0.0, np.zeros(0), np.zeros(0)
        _, info, _, chi2, weights, _ = self._run_robust("PoseGraph2D.robust_cost", 0, 0, 0.0, kernel, delta, edges)
        return float(info[_lib.ROB_COST_AFTER]), chi2, weights

    def marginals(self, nodes=None, fix_node=0, diagonal=True, force_dense=False, edge_weights=None):
        """3 x 3 blocks of the inverse of the matrix ``optimize`` factorises (pose_graph.py:93-114) at the current poses:
        for symmetric positive definite information, the covariance of the poses given the pose at ``fix_node``.
        ``diagonal``: the block of every node; ``nodes``: a list of node indices (negative ones count from the end,
        repeats allowed) whose block columns are returned too, which holds every joint marginal among them.  Nothing is
        iterated and ``self.nodes`` stay as they are.  ``force_dense``: the dense elimination whatever the graph (it is
        taken anyway where the chain + closures split does not apply or is refused).  ``edge_weights``: one weight per edge
        (``last_robust["weights"]``), every Omega is multiplied by its weight on the host before upload: the covariances at
        a robust optimum.  Returns a ``Marginals``, or None where ``optimize`` would return
        at once (fewer than two nodes, no edges); raises ``np.linalg.LinAlgError`` where the reference's solve would."""
        n = len(self.nodes)
        if n < 2 or len(self.edges) == 0:
            return None
        sel = []
        for v in ([] if nodes is None else nodes):
            v = int(v)
            v = v + n if v < 0 else v
            if not 0 <= v < n:
                raise IndexError("list index out of range")
            sel.append(v)
        if not sel and not diagonal:
            raise ValueError("marginals: nothing asked for (diagonal=False and no nodes)")
        t, L, s = self._stage(fix_node, edge_weights), _lib.lib(), len(sel)
        d_info = torch.zeros(_lib.MARG_DOUBLES, dtype=torch.float64, device=t.dev)
        d_diag = torch.empty((n, 3, 3), dtype=torch.float64, device=t.dev) if diagonal else None
        d_cols = torch.empty((s, n, 3, 3), dtype=torch.float64, device=t.dev) if s else None
        sel_host = np.ascontiguousarray(np.array(sel, dtype=np.int32))

        def launch(dense, _):
            return self._launch(t, "PoseGraph2D.marginals", L.icpmi_pose_graph_marginals,
                                L.icpmi_pose_graph_marginals_workspace_bytes(t.ijp, t.omp, n, t.m, s, int(bool(diagonal)), int(dense)),
                                d_info, n, t.m, t.fix, sel_host.ctypes.data_as(C.c_void_p), s, _b._ptr(d_diag) if diagonal else None,
                                _b._ptr(d_cols) if s else None, int(dense))

        info, _ = _continued(launch, dense=bool(force_dense), status_slot=_lib.MARG_STATUS)
        status = int(info[_lib.MARG_STATUS])
        if status == SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        return Marginals(t.poses, t.fix, sel, d_diag.cpu().numpy() if diagonal else None, d_cols.cpu().numpy() if s else None,
                         status, "dense" if int(info[_lib.MARG_PATH]) == _lib.MARG_PATH_DENSE else "split")

    def get_poses_as_matrices(self):
        return [pose_vec_to_matrix(v) for v in self.nodes]

    def total_error(self):
        """pose_graph.py:189-194: sum of e^T Omega e over the edges."""
        if not self.edges:
            return 0.0
        t = self._stage()
        d_i, d_j = (torch.from_numpy(np.ascontiguousarray(t.ij[:, c])).to(t.dev) for c in (0, 1))
        scratch = torch.empty(t.m + 1, dtype=torch.float64, device=t.dev)
        _lib.check(_lib.lib().icpmi_pose_graph_error(_b._ptr(t.d_nodes), _b._ptr(d_i), _b._ptr(d_j), _b._ptr(t.d_z), _b._ptr(t.d_om),
                                                     t.m, _b._ptr(scratch), _b._ptr(scratch[t.m:]), _b._stream()),
                   "PoseGraph2D.total_error")
        return float(scratch[t.m].item())
