#!/usr/bin/env python3
"""Marginals of the pose graph (icpmi_pose_graph_marginals) on chains of 1 000 and 10 000 nodes with 20 closures, one
process on one GPU, device events around the whole call (its host plan, its copies and every launch), the variants
alternating:

  (d) the diagonal: block (v, v) of every node;
  (c) the block columns of 6 selected nodes (first, last, the middle and three others);
  (o) for scale: one Gauss-Newton iteration of icpmi_pose_graph_optimize on the same graph (its nodes restored before
      every sample, outside the events).

All three take the split path (the status and path of every variant are printed).  A sample is one call; SAMPLES samples
per variant after one warm-up of each.  The marginals' sweeps along the chain are serial in the number of nodes, so their
time grows with it where the optimiser's cyclic reduction does not.

usage: time_marginals.py [samples]   (prints one JSON line)"""
import ctypes as C
import json
import sys

from timing import stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import _lib
from icpmi import batch as _b

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SIZES, CLOSURES, SELECTED = (1000, 10000), 20, 6


def chain_graph(n, seed):
    """A drive of n poses (0.3 m steps, heading a random walk), odometry edges with noise, CLOSURES closures."""
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0.0, 0.05, n))
    xy = np.cumsum(np.stack([0.3 * np.cos(th), 0.3 * np.sin(th)], axis=1), axis=0)
    truth = np.column_stack([xy, (th + np.pi) % (2 * np.pi) - np.pi])

    def rel(a, b):
        c, s = np.cos(a[2]), np.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, (b[2] - a[2] + np.pi) % (2 * np.pi) - np.pi])

    pairs = [(k, k + 1) for k in range(n - 1)]
    while len(pairs) < n - 1 + CLOSURES:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) >= 2:
            pairs.append((a, b))
    ij = np.ascontiguousarray(np.array(pairs, dtype=np.int32))
    z = np.array([rel(truth[a], truth[b]) for a, b in pairs]) + rng.normal(0.0, 0.005, (len(pairs), 3))
    om = np.ascontiguousarray(np.eye(3)[None] * rng.uniform(100.0, 1e4, len(pairs))[:, None, None])
    nodes = truth + rng.normal(0.0, 0.01, truth.shape)
    return nodes, ij, z, om


assert torch.cuda.is_available(), "time_marginals.py measures on the GPU: there is nothing to time without one"
L = _lib.lib()
dev = torch.device("cuda", torch.cuda.current_device())
out = {"closures": CLOSURES, "selected": SELECTED}
for n in SIZES:
    nodes, ij, z, om = chain_graph(n, 77 + n)
    m = len(ij)
    sel = np.ascontiguousarray(np.array([0, n - 1, n // 2, n // 3, n // 5, 7], dtype=np.int32))
    ijp, omp, selp = (a.ctypes.data_as(C.c_void_p) for a in (ij, om, sel))
    d_nodes0 = torch.from_numpy(np.ascontiguousarray(nodes)).to(dev)
    d_nodes = d_nodes0.clone()
    d_z, d_om = torch.from_numpy(np.ascontiguousarray(z)).to(dev), torch.from_numpy(om).to(dev)
    d_minfo = torch.zeros(_lib.MARG_DOUBLES, dtype=torch.float64, device=dev)
    d_oinfo = torch.zeros(_lib.PGINFO_DOUBLES, dtype=torch.float64, device=dev)
    d_diag = torch.empty((n, 9), dtype=torch.float64, device=dev)
    d_cols = torch.empty((SELECTED, n, 9), dtype=torch.float64, device=dev)
    ws_d = torch.empty(L.icpmi_pose_graph_marginals_workspace_bytes(ijp, omp, n, m, 0, 1, 0), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(L.icpmi_pose_graph_marginals_workspace_bytes(ijp, omp, n, m, SELECTED, 0, 0), dtype=torch.uint8, device=dev)
    ws_o = torch.empty(L.icpmi_pose_graph_weighted_workspace_bytes(ijp, omp, n, m), dtype=torch.uint8, device=dev)

    def marginals(diag, cols, ws, s):
        _lib.check(L.icpmi_pose_graph_marginals(_b._ptr(d_nodes0), ijp, _b._ptr(d_z), _b._ptr(d_om), n, m, 0, selp, s,
                                                _b._ptr(diag) if diag is not None else None, _b._ptr(cols) if cols is not None else None,
                                                0, _b._ptr(d_minfo), _b._ptr(ws), ws.numel(), _b._stream()), "marginals")

    def optimize():
        _lib.check(L.icpmi_pose_graph_optimize(_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om), n, m, 1, 0, 0.0,
                                               _b._ptr(d_oinfo), _b._ptr(ws_o), ws_o.numel(), _b._stream()), "optimize")

    variants = {"d_diagonal": (lambda: marginals(d_diag, None, ws_d, 0), d_minfo, _lib.MARG_STATUS),
                "c_columns_of_6": (lambda: marginals(None, d_cols, ws_c, SELECTED), d_minfo, _lib.MARG_STATUS),
                "o_optimize_one_iteration": (optimize, d_oinfo, _lib.PGINFO_STATUS)}

    def sample(fn):
        d_nodes.copy_(d_nodes0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res = {}
    for name, (fn, info, slot) in variants.items():
        sample(fn)
        res[name] = {"status": int(info.cpu()[slot])}
        if info is d_minfo:
            res[name]["path"] = "dense" if int(info.cpu()[_lib.MARG_PATH]) == _lib.MARG_PATH_DENSE else "split"
    times = {name: [] for name in variants}
    for _ in range(SAMPLES):
        for name, (fn, _, _) in variants.items():
            times[name].append(sample(fn))
    for name in variants:
        res[name].update(stats(times[name]))
    res["diagonal_finite"] = bool(torch.isfinite(d_diag).all())
    res["largest_position_variance_m2"] = float(d_diag[:, [0, 4]].max())
    out[f"n_{n}"] = res
print(json.dumps(out))
