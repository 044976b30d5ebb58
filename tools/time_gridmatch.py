#!/usr/bin/env python3
"""Correlative scan-to-map matching (icpmi.gridmatch.GridMatchBatch behind OccupancyGrid2D.match_scan / match_history /
score_poses) on bench.py's config-4 grid (2 242 x 2 402 cells at 0.05 m, 32 scans applied), one process on one GPU, device
events around run(), the variants alternating:

  (a) one 1 430-row scan, 25 angles x 13^2 shifts (W = 6), the field rebuilt by every run — what match_scan enqueues;
  (k) the same with the field kept (field=): scoring and arg-max alone;
  (m) (k) plus the moments of the volume about the winner (half_log_odds=0.25): one more memset and launch — reported as the
      time it adds to (k) of the same run;
  (f) the field alone (icpmi_grid_score_field of the whole grid);
  (b) 512 resident 2 048-beam scans of a ScanHistory by id, 25 angles x 13^2 shifts each, field kept;
  (c) 4 096 poses of the 1 430-row scan through the score_poses shape (one angle, no shifts), field kept.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  (a) is sampled twice, as a1 and a2, in the same alternation: |median a1 - median a2| is the run-to-run spread a
difference has to exceed.  There is no earlier capability to compare a time against: the numbers stand on their own.

usage: time_gridmatch.py [samples] [block]   (prints one JSON line)"""
import json
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import ScanHistory, synth
from icpmi.batch import CloudSet
from icpmi.gridmatch import GridMatchBatch, angle_grid

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N_HIST, N_POSES, ROWS, W = 512, 4096, 1430, 6


assert torch.cuda.is_available(), "time_gridmatch.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
field = grid.score_field()

rng = np.random.default_rng(0)
true = (0.5, -0.1, np.deg2rad(14.0))
full = synth.scan(true, 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
pred = (true[0] + 0.12, true[1] - 0.08, true[2] + np.deg2rad(3.0))
angles, centre = angle_grid([pred[2]], 12.0, 1.0)
one = CloudSet.from_numpy([scan])
a = GridMatchBatch(grid, one, [0], [pred[:2]], angles, W, centre)
k = GridMatchBatch(grid, one, [0], [pred[:2]], angles, W, centre, field=field)
m = GridMatchBatch(grid, one, [0], [pred[:2]], angles, W, centre, field=field, half_log_odds=0.25)

poses = [(0.3 + 0.02 * (i % 32) + rng.uniform(-0.1, 0.1), -0.2 + 0.01 * (i % 32) + rng.uniform(-0.1, 0.1),
          np.deg2rad(10.0 + 0.5 * (i % 32) + rng.uniform(-3.0, 3.0))) for i in range(N_HIST)]
hist = ScanHistory(scan_capacity=N_HIST, row_capacity=N_HIST * 2048)
ids = hist.add_many([synth.scan(p, 6000 + i) for i, p in enumerate(poses)])
P = np.array(poses)
hangles, hcentre = angle_grid(P[:, 2] + np.deg2rad(2.0), 12.0, 1.0)
b = GridMatchBatch(grid, hist.raw, ids, P[:, :2] + 0.1, hangles, W, hcentre, field=field)

hyp = np.array(true) + rng.uniform(-1.0, 1.0, size=(N_POSES, 3)) * np.array([0.5, 0.5, 0.2])
c = GridMatchBatch(grid, one, np.zeros(N_POSES, dtype=np.int32), hyp[:, :2], hyp[:, 2:3], 0, 0, field=field)

variants = {"a1": a.run, "k": k.run, "m": m.run, "f": grid.score_field, "b": b.run, "c": c.run, "a2": a.run}
times = alternate({name: (fn, BLOCK) for name, fn in variants.items()}, SAMPLES, 3)
# what the runs found, once: the single scan's error against its true pose, the batch's statuses
_, t, score, info = a.unpack()
minfo = m.unpack()[3]
found = {"err_m": [round(float(abs(t[0, i] - true[i])), 4) for i in (0, 1)], "err_deg": round(float(np.rad2deg(abs(info["angle"][0] - true[2]))), 3),
         "score": int(score[0]), "centre_score": int(info["centre_score"][0]), "equal_with_field_kept": bool(np.array_equal(a.records.cpu().numpy(), k.records.cpu().numpy())),
         "refined_err_m": [round(float(abs(v - true[i])), 4) for i, v in enumerate(minfo["t_refined"][0])],
         "refined_err_deg": round(float(np.rad2deg(abs(minfo["angle_refined"][0] - true[2]))), 3),
         "support": int(minfo["support"][0]), "edge_weight": round(float(minfo["edge_weight"][0]), 5),
         "history_status_ok": int((b.unpack()[3]["status"] == 0).sum()), "poses_status_ok": int((c.unpack()[3]["status"] == 0).sum())}
both = np.array(times["a1"] + times["a2"])
out = {"grid": [grid.ny, grid.nx], "resolution": grid.resolution, "block": BLOCK, "found": found,
       "a_one_scan_25x13x13_field_rebuilt": stats(both), "a1": stats(times["a1"]), "a2": stats(times["a2"]),
       "a_spread_ms": round(abs(float(np.median(times["a1"]) - np.median(times["a2"]))), 4),
       "k_one_scan_field_kept": stats(times["k"]), "m_one_scan_field_kept_with_moments": stats(times["m"]),
       "m_added_ms": round(float(np.median(times["m"]) - np.median(times["k"])), 4), "f_field_alone": stats(times["f"]),
       f"b_{N_HIST}_history_scans_25x13x13": stats(times["b"]), f"c_{N_POSES}_poses": stats(times["c"]),
       "b_candidates_per_s": round(N_HIST * 25 * 169 * 1e3 / float(np.median(times["b"]))),
       "c_poses_per_s": round(N_POSES * 1e3 / float(np.median(times["c"])))}
print(json.dumps(out))
