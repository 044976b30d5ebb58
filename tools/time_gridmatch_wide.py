#!/usr/bin/env python3
"""The wide-window scan-to-map search (icpmi.gridmatch.GridSearchBatch behind OccupancyGrid2D.search_scan) on bench.py's
config-4 grid (2 242 x 2 402 cells at 0.05 m, 32 scans applied), one process on one GPU, device events around run(), the
variants alternating:

  case 1, one 1 430-row scan, 25 angles, W = 31 (1.55 m), the field kept (field=):
    (e)  the exhaustive search, GridMatchBatch: 25 x 63^2 candidates;
    (s8) the pruned search, block 8, the bound field kept (bounds=);  (s4), (s16): blocks 4 and 16;
    (r8) block 8 with the bound field rebuilt by every run;
  case 2, the same scan predicted 3.2 m and 75 degrees off, W = 100 (5 m), the full circle at 1 degree: 361 x 201^2 candidates,
  which no other entry can search:
    (w8) block 8, field and bound field kept;  (w4), (w16): blocks 4 and 16;
  (m) the bound field of the 5.4 M-cell grid alone, block 8.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  (s8) is sampled twice, as s8 and s8b, in the same alternation: |median s8 - median s8b| is the run-to-run spread a
difference has to exceed.  The survivor fraction is what the records report (slot 9 / slot 8): a function of the inputs.

usage: time_gridmatch_wide.py [samples] [block]   (prints one JSON line)"""
import json
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import synth
from icpmi.batch import CloudSet
from icpmi.gridmatch import GridMatchBatch, GridSearchBatch, angle_grid, bound_field

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ROWS, W_NEAR, W_WIDE = 1430, 31, 100


assert torch.cuda.is_available(), "time_gridmatch_wide.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
field = grid.score_field()
kept = {D: bound_field(field[0], D) for D in (4, 8, 16)}

true = (0.5, -0.1, np.deg2rad(14.0))
full = synth.scan(true, 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
one = CloudSet.from_numpy([scan])
near = (true[0] + 0.9, true[1] - 0.7, true[2] + np.deg2rad(8.0))
far = (true[0] + 3.2, true[1] - 3.2, true[2] + np.deg2rad(75.0))
angles, centre = angle_grid([near[2]], 12.0, 1.0)
circle, ccentre = angle_grid([far[2]], 180.0, 1.0)

e = GridMatchBatch(grid, one, [0], [near[:2]], angles, W_NEAR, centre, field=field)
s = {D: GridSearchBatch(grid, one, [0], [near[:2]], angles, W_NEAR, centre, block=D, field=field, bounds=kept[D]) for D in (4, 8, 16)}
r8 = GridSearchBatch(grid, one, [0], [near[:2]], angles, W_NEAR, centre, block=8, field=field)
w = {D: GridSearchBatch(grid, one, [0], [far[:2]], circle, W_WIDE, ccentre, block=D, field=field, bounds=kept[D]) for D in (4, 8, 16)}

variants = {"s8": s[8].run, "e": e.run, "s4": s[4].run, "s16": s[16].run, "r8": r8.run, "w8": w[8].run, "w4": w[4].run, "w16": w[16].run,
            "m": lambda: bound_field(field[0], 8, kept[8]), "s8b": s[8].run}
times = alternate({name: (fn, BLOCK) for name, fn in variants.items()}, SAMPLES, 2)


def found(job, pred):
    _, t, score, info = job.unpack()
    out = {"err_m": [round(float(abs(t[0, i] - true[i])), 4) for i in (0, 1)], "err_deg": round(float(np.rad2deg(abs(info["angle"][0] - true[2]))), 3),
           "score": int(score[0]), "centre_score": int(info["centre_score"][0]), "index": int(info["index"][0])}
    if "blocks" in info:
        out.update(blocks=int(info["blocks"][0]), survivors=int(info["survivors"][0]), seed_score=int(info["seed_score"][0]),
                   max_bound=int(info["max_bound"][0]), survivor_fraction=round(float(info["survivors"][0] / info["blocks"][0]), 6))
    return out


what = {"e": found(e, near), **{f"s{D}": found(s[D], near) for D in s}, **{f"w{D}": found(w[D], far) for D in w}}
what["near_equal_to_exhaustive"] = bool(all(np.array_equal(s[D].records.cpu().numpy()[:, :8], e.records.cpu().numpy()) for D in s))
what["wide_blocks_agree"] = bool(all(np.array_equal(w[D].records.cpu().numpy()[:, :8], w[8].records.cpu().numpy()[:, :8]) for D in w))
out = {"grid": [grid.ny, grid.nx], "resolution": grid.resolution, "block": BLOCK, "rows": ROWS,
       "near": {"W": W_NEAR, "angles": int(angles.shape[1]), "candidates": int(angles.shape[1]) * (2 * W_NEAR + 1) ** 2},
       "wide": {"W": W_WIDE, "angles": int(circle.shape[1]), "candidates": int(circle.shape[1]) * (2 * W_WIDE + 1) ** 2},
       "found": what, "s8_spread_ms": round(abs(float(np.median(times["s8"]) - np.median(times["s8b"]))), 4),
       **{name: stats(v) for name, v in times.items()}}
print(json.dumps(out))
