#!/usr/bin/env python3
"""Diagnostic: batched _run_icp_pair on B loop-closure candidates with each alignment method — "rotation_search" (the
default), "features" and "both" — on the same build: device time of the pre-alignment and of the whole run (events, median
of the repeats after warm-up).  usage: time_features.py [B] [max_offset max_yaw_deg]
With REFERENCE=<path of the reference checkout> it also times the reference's feature_based_alignment per pair on the CPU."""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "iterative-closest-point-avmi_amd"))
import numpy as np, torch
from icpmi import synth
from icpmi.prealign import RunIcpPairBatch
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
off = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
yaw = float(sys.argv[3]) if len(sys.argv) > 3 else 20.0
WARMUP, REPEATS = 3, 10
srcs, tgts = synth.loop_closure_batch(B, seed0=7000, shared_source=True, max_offset=off, max_yaw_deg=yaw)
kw = dict(error_threshold=1e-10, max_iterations=150, voxel_size=0.04, method="point_to_line", normal_k=12)
clouds, ps, pt = [srcs[0]] + tgts, np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32)
for method in ("rotation_search", "features", "both"):
    b = RunIcpPairBatch(clouds, ps, pt, rotation_voxel_size=0.15, angle_step_coarse=1.5, angle_step_fine=0.1,
                        max_rows_hint=1024, alignment_method=method,
                        rng=np.random.default_rng(1), **kw)
    for _ in range(WARMUP):
        b.run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        if b.use_search:
            b.search.run()
        e[1].record()
        if b.features is not None:
            b.features.run()
        e[2].record(); b.icp.run(); e[3].record(); torch.cuda.synchronize()
        ts.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), e[0].elapsed_time(e[3])))
    ts = np.median(np.array(ts), axis=0)
    res = b.icp.results.cpu().numpy()[:B]
    line = (f"B={B} offset<={off} yaw<={yaw} {method:16s}: search {ts[0]:.3f} ms, features {ts[1]:.3f} ms, voxel+prepare+icp {ts[2]:.3f} ms, "
            f"total {ts[3]:.3f} ms (median of {REPEATS}); registered {(res[:, 12] < 0.05).mean():.3f}")
    if b.features is not None:
        fr = b.features.records.cpu().numpy()[:B]
        line += (f"; feature status counts {np.bincount(fr[:, 12].astype(int), minlength=6).tolist()}, matches {fr[:, 4].mean():.1f}, "
                 f"inliers {fr[:, 5].mean():.1f}, filtered rows {fr[:, 1].mean():.0f}")
    print(line, flush=True)
ref = os.environ.get("REFERENCE")
if ref:
    import importlib, types
    sys.path.insert(0, ref)
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    for m in [m for m in sys.modules if m == "utilities" or m.startswith("utilities.")]:
        del sys.modules[m]
    ref_feat = importlib.import_module("utilities.features")
    import contextlib, io
    n = min(B, 16)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(n):
            ref_feat.feature_based_alignment(srcs[0], tgts[i])
    print(f"reference feature_based_alignment on this CPU: {(time.perf_counter() - t0) / n * 1e3:.1f} ms per pair ({n} pairs)")
