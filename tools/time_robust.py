#!/usr/bin/env python3
"""icpmi_pose_graph_optimize against icpmi_pose_graph_optimize_robust, per Gauss-Newton iteration, one process on one GPU,
device events around the whole call (its host plan, its copies and the launch), the variants alternating:

  (o)  optimize, ITERATIONS iterations with convergence_eps = 0 (so every call runs them all);
  (o2) the same variant sampled a second time: the difference of its median from (o)'s is the spread of the measurement;
  (h) (c) (g) optimize_robust with Huber, Cauchy and Geman-McClure on the closures, delta = 2.7955.

on a chain of 1 000 nodes with 10 closures and on one of 64 nodes with 3.  One closure of each graph is false (its
measurement moved by metres), so that the robust weights are not all 1.  The nodes are restored before every sample,
outside the events.  Besides the events, the kernels' own clocks: the sum of the phase clocks per iteration, and the
weights phase per pass (ITERATIONS + 1 passes).

usage: time_robust.py [samples] [library]   (prints one JSON line)
``library``: another build of libicpmi.so (the parent commit's, to compare ``optimize`` across builds); the robust
variants are left out where it does not export them."""
import ctypes as C
import json
import os
import sys

from timing import stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import _lib
from icpmi import batch as _b

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
ITERATIONS, DELTA = 5, 2.7955
SIZES = ((1000, 10), (64, 3))                  # (nodes, closures)
KERNELS = (("h_huber", _lib.ROB_KERNEL_HUBER), ("c_cauchy", _lib.ROB_KERNEL_CAUCHY), ("g_geman_mcclure", _lib.ROB_KERNEL_GEMAN_MCCLURE))


def chain_graph(n, closures, seed):
    """A drive of n poses (0.3 m steps, heading a random walk), odometry edges with noise, ``closures`` closures, the last one false."""
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0.0, 0.05, n))
    xy = np.cumsum(np.stack([0.3 * np.cos(th), 0.3 * np.sin(th)], axis=1), axis=0)
    truth = np.column_stack([xy, (th + np.pi) % (2 * np.pi) - np.pi])

    def rel(a, b):
        c, s = np.cos(a[2]), np.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, (b[2] - a[2] + np.pi) % (2 * np.pi) - np.pi])

    pairs = [(k, k + 1) for k in range(n - 1)]
    while len(pairs) < n - 1 + closures:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) >= 2:
            pairs.append((a, b))
    ij = np.ascontiguousarray(np.array(pairs, dtype=np.int32))
    z = np.array([rel(truth[a], truth[b]) for a, b in pairs]) + rng.normal(0.0, 0.005, (len(pairs), 3))
    z[-1] += (3.0, -2.0, 0.5)
    om = np.ascontiguousarray(np.eye(3)[None] * rng.uniform(100.0, 1e4, len(pairs))[:, None, None])
    nodes = truth + rng.normal(0.0, 0.01, truth.shape)
    return nodes, ij, np.ascontiguousarray(z), om


assert torch.cuda.is_available(), "time_robust.py measures on the GPU: there is nothing to time without one"
if len(sys.argv) > 2:                           # another build: bind what it exports (torch, and with it the HIP runtime, is loaded)
    L = _lib.bind(os.path.abspath(sys.argv[2]), exported_only=True)
else:
    L = _lib.lib()
robust = hasattr(L, "icpmi_pose_graph_optimize_robust")
dev = torch.device("cuda", torch.cuda.current_device())
out = {"iterations": ITERATIONS, "library": sys.argv[2] if len(sys.argv) > 2 else "libicpmi.so"}
for n, closures in SIZES:
    nodes, ij, z, om = chain_graph(n, closures, 91 + n)
    m = len(ij)
    mask = np.ascontiguousarray((np.abs(ij[:, 0] - ij[:, 1]) != 1).astype(np.uint8))
    ijp, omp, maskp = (a.ctypes.data_as(C.c_void_p) for a in (ij, om, mask))
    d_nodes0 = torch.from_numpy(np.ascontiguousarray(nodes)).to(dev)
    d_nodes = d_nodes0.clone()
    d_z, d_om = torch.from_numpy(z).to(dev), torch.from_numpy(om).to(dev)
    d_info = torch.zeros(_lib.ROB_DOUBLES, dtype=torch.float64, device=dev)
    d_chi2, d_wgt = (torch.zeros(m, dtype=torch.float64, device=dev) for _ in range(2))
    ws = torch.empty(L.icpmi_pose_graph_weighted_workspace_bytes(ijp, omp, n, m), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(L.icpmi_pose_graph_robust_workspace_bytes(ijp, omp, maskp, n, m, 0), dtype=torch.uint8, device=dev) if robust else None

    def optimize():
        _lib.check(L.icpmi_pose_graph_optimize(_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om), n, m, ITERATIONS, 0, 0.0,
                                               _b._ptr(d_info), _b._ptr(ws), ws.numel(), _b._stream()), "optimize")

    def optimize_robust(kernel):
        _lib.check(L.icpmi_pose_graph_optimize_robust(_b._ptr(d_nodes), ijp, _b._ptr(d_z), _b._ptr(d_om), maskp, n, m, ITERATIONS, 0, 0.0,
                                                      kernel, DELTA, 0, _b._ptr(d_chi2), _b._ptr(d_wgt), _b._ptr(d_info), _b._ptr(ws_r),
                                                      ws_r.numel(), _b._stream()), "optimize_robust")

    variants = {"o_optimize": optimize, "o2_optimize_again": optimize}
    if robust:
        variants.update({name: (lambda k=k: optimize_robust(k)) for name, k in KERNELS})

    def sample(fn):
        d_nodes.copy_(d_nodes0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res, times, clocks, weights = {}, {}, {}, {}
    for name, fn in variants.items():
        sample(fn)
        info = d_info.cpu().numpy()
        res[name] = {"status": int(info[_lib.PGINFO_STATUS]), "iterations": int(info[_lib.PGINFO_ITERATIONS])}
        times[name], clocks[name], weights[name] = [], [], []
    for _ in range(SAMPLES):
        for name, fn in variants.items():
            times[name].append(sample(fn))
            info = d_info.cpu().numpy()
            clocks[name].append(float(info[_lib.PGINFO_PHASE_US:_lib.PGINFO_PHASE_US + _lib.PGINFO_PHASES].sum()) / ITERATIONS)
            if name not in ("o_optimize", "o2_optimize_again"):
                weights[name].append(float(info[_lib.ROB_WEIGHTS_US]) / (ITERATIONS + 1))
    for name in variants:
        res[name].update(stats(times[name]))
        res[name]["per_iteration_ms"] = round(res[name]["median_ms"] / ITERATIONS, 4)
        res[name]["kernel_clock_us_per_iteration"] = round(float(np.median(clocks[name])), 2)
        if weights[name]:
            res[name]["weights_us_per_pass"] = round(float(np.median(weights[name])), 2)
    if robust:
        res["smallest_weight"] = float(d_wgt.min())
    out[f"n_{n}"] = res
print(json.dumps(out))
