#!/usr/bin/env python3
"""The map rebuild that follows an accepted loop closure (slam.py:271-277), from host arrays and from the resident scan
history, one process on one GPU, device events around reset() ... the last launch plus a final synchronise, the variants
alternating:

  (a) the host path as examples/slam_loop.py runs it for a backend without a resident rebuild: NumPy transforms of every
      scan (`pts @ T[:2, :2].T + T[:2, 2]`), reset(), update_scans of the host arrays (concatenate, upload, replay);
  (b) OccupancyGrid2D.rebuild_from_history: ids and poses go up, the scans are transformed on the device piece by piece;
  (t) the transform alone: one icpmi_history_world_rows launch for the whole history (arguments already on the device),
      BLOCK launches between two events.

512 synthetic 2 048-beam scans along a drive through the room, on BASELINE config 4's grid (2 242 x 2 402 cells at 0.05 m).
(a) is sampled twice, as a1 and a2, in the same alternation: |median a1 - median a2| is the run-to-run spread a difference
has to exceed.  Before any timing the two grids are compared bit for bit.

usage: time_rebuild.py [samples] [scans]   (prints one JSON line)"""
import json
import sys

from timing import alternate, sample, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import ScanHistory, synth
from utilities.mapping import OccupancyGrid2D

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
BLOCK = 20


def pose_matrix(x, y, th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]])


assert torch.cuda.is_available(), "time_rebuild.py measures on the GPU: there is nothing to time without one"
truth = [(-8.5 + 17.0 * k / max(N - 1, 1), -0.5 + 0.2 * np.sin(0.05 * k), 0.3 * np.sin(0.02 * k)) for k in range(N)]
scans = [synth.scan(p, 5000 + k) for k, p in enumerate(truth)]
rng = np.random.default_rng(1)
poses = [pose_matrix(x + rng.normal(0, 0.02), y + rng.normal(0, 0.02), th + rng.normal(0, 0.01)) for x, y, th in truth]
history = list(zip(scans, poses))

p0 = (0.3, -0.2, np.deg2rad(10.0))                       # the grid of bench.py's raycast_workload (BASELINE config 4)
first = synth.to_world(synth.scan(p0, 2), p0)
bounds = (first[:, 0].min() - 50, first[:, 0].max() + 50, first[:, 1].min() - 50, first[:, 1].max() + 50)
kw = dict(resolution=0.05, p_hit=0.85, p_miss=0.42, log_odds_min=-8.0, log_odds_max=8.0)
grid_a, grid_b = OccupancyGrid2D(*bounds, **kw), OccupancyGrid2D(*bounds, **kw)

resident = ScanHistory(voxel_size=0.04, normal_k=12, rotation_voxel_size=0.15, scan_capacity=N,
                       row_capacity=sum(len(s) for s in scans))
resident.add_many(scans)


def host_path():
    worlds = [pts @ T[:2, :2].T + T[:2, 2] for pts, T in history]
    grid_a.reset()
    grid_a.update_scans(np.array([T[:2, 2] for _, T in history]), worlds)


def resident_path():
    grid_b.rebuild_from_history(resident, poses)


ids, pose6, off = resident.world_row_args(poses)
d_ids, d_pose, d_off = (torch.from_numpy(a).to(resident.device) for a in (ids, pose6, off))
rows = torch.empty((int(off[-1]), 2), dtype=torch.float64, device=resident.device)


def transform_alone():
    resident.world_rows_into(rows, d_ids, d_pose, d_off, len(ids))


host_path(); resident_path(); transform_alone()
torch.cuda.synchronize()
equal = bool(torch.equal(grid_a.device_log_odds, grid_b.device_log_odds))
rows_equal = bool(np.array_equal(rows.cpu().numpy(), np.concatenate([pts @ T[:2, :2].T + T[:2, 2] for pts, T in history])))

variants = {"a1": host_path, "b": resident_path, "a2": host_path}
times = alternate({k: (fn, 1) for k, fn in variants.items()}, SAMPLES, 1)
sample(transform_alone, 3)
t_rows = [sample(transform_alone, BLOCK) for _ in range(SAMPLES)]

a = np.array(times["a1"] + times["a2"])
out = {"shape": f"{N} scans x 2048 beams ({int(off[-1])} rows), grid {grid_a.ny}x{grid_a.nx} at 0.05 m",
       "grids_equal": equal, "world_rows_equal_numpy": rows_equal,
       "a_host": stats(a), "a1": stats(times["a1"]), "a2": stats(times["a2"]),
       "a_spread_ms": round(abs(float(np.median(times["a1"]) - np.median(times["a2"]))), 4),
       "b_resident": stats(times["b"]), "transform_launch": stats(t_rows),
       "b_minus_a_ms": round(float(np.median(times["b"]) - np.median(a)), 4)}
print(json.dumps(out))
