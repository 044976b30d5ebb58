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

    def optimize(self, n_iterations=20, fix_node=0, convergence_eps=1e-6):
        """pose_graph.py:83-134: Gauss-Newton with the pose at ``fix_node`` held constant."""
        n = len(self.nodes)
        if n < 2 or len(self.edges) == 0:
            return
        _b.require_gpu()
        L = _lib.lib()
        dev = torch.device("cuda", torch.cuda.current_device())
        ij, z, om = self._edge_arrays()
        m = len(ij)
        fix = fix_node + n if fix_node < 0 else fix_node
        d_nodes = torch.from_numpy(np.ascontiguousarray(np.array(self.nodes, dtype=np.float64).reshape(n, 3))).to(dev)
        d_z, d_om = torch.from_numpy(z).to(dev), torch.from_numpy(om).to(dev)
        d_info = torch.zeros(_lib.PGINFO_DOUBLES, dtype=torch.float64, device=dev)
        ijp = ij.ctypes.data_as(C.c_void_p)

        def launch(size_query, entry, iterations):
            ws = torch.empty(max(int(size_query(ijp, n, m)), 256), dtype=torch.uint8, device=dev)
            _lib.check(entry(_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om), n, m, iterations, int(fix),
                             float(convergence_eps), _b._ptr(d_info), _b._ptr(ws), ws.numel(), _b._stream()),
                       "PoseGraph2D.optimize")
            return d_info.cpu().numpy()

        omp = om.ctypes.data_as(C.c_void_p)                 # with the information matrices: room for the twins of weak chain edges
        info = launch(lambda *a: L.icpmi_pose_graph_weighted_workspace_bytes(a[0], omp, *a[1:]),
                      L.icpmi_pose_graph_optimize, int(n_iterations))
        split_refused_at = None
        if int(info[_STATUS]) == _SPLIT_REFUSED:
            # the chain part of the split turned out exactly singular: the remaining iterations take the dense matrix
            split_refused_at, first = int(info[_ITERATIONS]), info
            info = launch(L.icpmi_pose_graph_dense_workspace_bytes, L.icpmi_pose_graph_optimize_dense,
                          int(n_iterations) - split_refused_at)
            info[_ITERATIONS] += first[_ITERATIONS]
            info[_PHASES] += first[_PHASES]
            if int(info[_ITERATIONS]) == split_refused_at:
                info[_STEP] = first[_STEP]                         # singular at once: the last step applied is the split's
        out = d_nodes.cpu().numpy()
        iters, status, step = int(info[_ITERATIONS]), int(info[_STATUS]), info[_STEP]
        for k in range(n):                                   # in place, like pose_graph.py:122-125
            self.nodes[k][:] = out[k]
        self.last_info = dict(iterations=iters, status=status, step_norm=float(step), split_refused_at=split_refused_at,
                              phase_us=dict(zip(PHASE_KEYS, info[_PHASES].tolist())))
        if VERBOSE:
            if status == SINGULAR:
                print(f"  PoseGraph: singular H at iter {iters}, stopping")
            elif status == CONVERGED:
                print(f"  PoseGraph converged: iter={iters - 1}, ||Δx||={step:.2e}")
            elif status == MAX_ITERATIONS:
                print(f"  PoseGraph max iterations: iter={n_iterations}, ||Δx||={step:.2e}")

    def marginals(self, nodes=None, fix_node=0, diagonal=True, force_dense=False):
        """3 x 3 blocks of the inverse of the matrix ``optimize`` factorises (pose_graph.py:93-114) at the current poses:
        for symmetric positive definite information, the covariance of the poses given the pose at ``fix_node``.
        ``diagonal``: the block of every node; ``nodes``: a list of node indices (negative ones count from the end,
        repeats allowed) whose block columns are returned too, which holds every joint marginal among them.  Nothing is
        iterated and ``self.nodes`` stay as they are.  ``force_dense``: the dense elimination whatever the graph (it is
        taken anyway where the chain + closures split does not apply or is refused).  Returns a ``Marginals``, or None where ``optimize`` would return
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
        _b.require_gpu()
        L = _lib.lib()
        dev = torch.device("cuda", torch.cuda.current_device())
        ij, z, om = self._edge_arrays()
        m, s = len(ij), len(sel)
        fix = fix_node + n if fix_node < 0 else fix_node
        poses = np.ascontiguousarray(np.array(self.nodes, dtype=np.float64).reshape(n, 3))
        d_nodes = torch.from_numpy(poses).to(dev)
        d_z, d_om = torch.from_numpy(z).to(dev), torch.from_numpy(om).to(dev)
        d_info = torch.zeros(_lib.MARG_DOUBLES, dtype=torch.float64, device=dev)
        d_diag = torch.empty((n, 3, 3), dtype=torch.float64, device=dev) if diagonal else None
        d_cols = torch.empty((s, n, 3, 3), dtype=torch.float64, device=dev) if s else None
        sel_host = np.ascontiguousarray(np.array(sel, dtype=np.int32))
        ijp, omp, selp = (a.ctypes.data_as(C.c_void_p) for a in (ij, om, sel_host))

        def launch(dense):
            size = L.icpmi_pose_graph_marginals_workspace_bytes(ijp, omp, n, m, s, int(bool(diagonal)), int(dense))
            ws = torch.empty(max(int(size), 256), dtype=torch.uint8, device=dev)
            _lib.check(L.icpmi_pose_graph_marginals(_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om), n, m, int(fix), selp, s,
                                                    _b._ptr(d_diag) if diagonal else None, _b._ptr(d_cols) if s else None,
                                                    int(dense), _b._ptr(d_info), _b._ptr(ws), ws.numel(), _b._stream()),
                       "PoseGraph2D.marginals")
            return d_info.cpu().numpy()

        info = launch(bool(force_dense))
        if int(info[_lib.MARG_STATUS]) == _SPLIT_REFUSED:          # as optimize: go on with the dense matrix
            info = launch(True)
        status = int(info[_lib.MARG_STATUS])
        if status == SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        return Marginals(poses, fix, sel, d_diag.cpu().numpy() if diagonal else None, d_cols.cpu().numpy() if s else None,
                         status, "dense" if int(info[_lib.MARG_PATH]) == _lib.MARG_PATH_DENSE else "split")

    def get_poses_as_matrices(self):
        return [pose_vec_to_matrix(v) for v in self.nodes]

    def total_error(self):
        """pose_graph.py:189-194: sum of e^T Omega e over the edges."""
        if not self.edges:
            return 0.0
        _b.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        n = len(self.nodes)
        ij, z, om = self._edge_arrays()
        m = len(ij)
        d_nodes = torch.from_numpy(np.ascontiguousarray(np.array(self.nodes, dtype=np.float64).reshape(n, 3))).to(dev)
        d_i = torch.from_numpy(np.ascontiguousarray(ij[:, 0])).to(dev)
        d_j = torch.from_numpy(np.ascontiguousarray(ij[:, 1])).to(dev)
        d_z, d_om = torch.from_numpy(z).to(dev), torch.from_numpy(om).to(dev)
        scratch = torch.empty(m + 1, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().icpmi_pose_graph_error(_b._ptr(d_nodes), _b._ptr(d_i), _b._ptr(d_j), _b._ptr(d_z), _b._ptr(d_om),
                                                     m, _b._ptr(scratch), _b._ptr(scratch[m:]), _b._stream()),
                   "PoseGraph2D.total_error")
        return float(scratch[m].item())
