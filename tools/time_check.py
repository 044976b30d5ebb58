#!/usr/bin/env python3
"""The check (icpmi.gridmatch.check_pairs behind OccupancyGrid2D.check_scans / check_poses / check_history) on bench.py's
config-4 grid (2 242 x 2 402 cells at 0.05 m, 32 scans applied), one process on one GPU, device events, the variants
alternating:

  (k4k)   4 096 poses x one 360-row scan over kept planes, the library's prepared call (gridmatch.MapPairs.check, outputs
          given): checked and uploaded once, then run; sampled twice (k4k_again);
  (k4f)   the same through the field: the call packs the planes first;
  (k4r)   (k4k) with the rows' records written as well;
  (kh)    512 scans of 2 048 rows resident in a ScanHistory, checked by id at the poses they were taken from, kept planes;
  (r4k)   icpmi_grid_cast_rays of 4 096 poses x 360 beams over the same planes, reach 30 m, the entry called directly;
  (sp)    OccupancyGrid2D.score_poses of the 360-row scan at the 4 096 poses (synchronises: what a caller waits for);
  (c4k)   (k4k) through OccupancyGrid2D.check_poses with kept planes: upload of the poses, the launches and the records
          read back — what a caller waits for.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  |median(k4k) - median(k4k_again)| is the run-to-run spread a difference has to exceed.  The walk's rate is rows x mean
steps looked at (to the hit, or all the steps inside the grid up to the end cell) per second; the check's beams end at the
scan's own returns, the cast's at its reach, so the check looks at fewer steps per ray.  No hardware counters are collected.
There is no earlier capability to compare a time against.

usage: time_check.py [samples] [block]   (prints one JSON line)"""
import json
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import ScanHistory, _lib, gridmatch, synth
from icpmi.batch import _ptr, _stream

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 21
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
REACH, POSES, ROWS, RESIDENT, TOLERANCE = 30.0, 4096, 360, 512, 2

assert torch.cuda.is_available(), "time_check.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
raw, k = grid.score_field()
ny, nx = raw.shape
threshold = int(np.rint(0.5 * 2.0 ** k))
dev = raw.device
L = _lib.lib()
planes = grid.occupancy_planes(field=(raw, k))
ws = torch.empty_like(planes[0].buf)
up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)                                    # noqa: E731

rng = np.random.default_rng(11)
poses = np.stack([rng.uniform(-3.0, 3.0, POSES), rng.uniform(-2.0, 2.0, POSES), rng.uniform(-np.pi, np.pi, POSES)], axis=1)
full = synth.scan((0.5, -0.1, np.deg2rad(14.0)), 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
one = gridmatch.cloud_set_of([scan])

drive = [(0.3 + 0.0012 * i, -0.2 + 0.0006 * i, np.deg2rad(10.0 + 0.03 * i)) for i in range(RESIDENT)]       # inside the mapped drive
hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=RESIDENT, row_capacity=RESIDENT * 2048)
hist.add_many([synth.scan(p, 7000 + i) for i, p in enumerate(drive)])
drive = np.array(drive)


def check_of(cs, pair_host, xyt, source, want_rows):
    """The library's prepared call over one set of pairs, its outputs made once -> (run, records, rows)"""
    pairs = gridmatch.MapPairs(source, threshold, grid.min_x, grid.min_y, grid.resolution, cs, pair_host, up(xyt[:, :2]),
                               up(np.stack([np.cos(xyt[:, 2]), np.sin(xyt[:, 2])], axis=1)))
    rec = torch.empty((pairs.B, _lib.GK_INTS), dtype=torch.int32, device=dev)
    rows = torch.empty((pairs.B, pairs.stride, _lib.GK_ROW_INTS), dtype=torch.int32, device=dev) if want_rows else None
    out = (rec, rows) if want_rows else rec
    return (lambda: pairs.check(TOLERANCE, want_rows, out)), rec, rows


k4k, rec4k, _ = check_of(one, np.zeros(POSES, dtype=np.int32), poses, planes[0], False)
k4f, rec4f, _ = check_of(one, np.zeros(POSES, dtype=np.int32), poses, raw, False)
k4r, rec4r, rows4r = check_of(one, np.zeros(POSES, dtype=np.int32), poses, planes[0], True)
kh, rech, rowsh = check_of(hist.raw, np.arange(RESIDENT), drive, planes[0], True)
for fn in (k4k, k4f, k4r, kh):
    fn()
want = rec4k.cpu().numpy()
assert np.array_equal(rec4f.cpu().numpy(), want) and np.array_equal(rec4r.cpu().numpy(), want)
info = grid.check_poses(scan, poses, tolerance=TOLERANCE, planes=planes)
assert np.array_equal(info["violated"], want[:, _lib.GK_REC_VIOLATED]) and np.array_equal(info["rows"], want[:, _lib.GK_REC_ROWS])

xy, pcs = up(poses[:, :2]), up(np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1))
angles = np.linspace(-np.pi, np.pi, ROWS, endpoint=False)
bcs = up(np.stack([np.cos(angles), np.sin(angles)], axis=1))
cast_out = torch.empty((POSES, ROWS, 4), dtype=torch.int32, device=dev)
cast_args = (None, _ptr(planes[0].buf), ny, nx, threshold, grid.min_x, grid.min_y, grid.resolution, _ptr(xy), _ptr(pcs), POSES, _ptr(bcs), ROWS, REACH,
             _ptr(cast_out), _ptr(ws), ws.numel(), _stream())


def r4k():
    rc = L.icpmi_grid_cast_rays(*cast_args)
    assert rc == 0, rc


host_bound = {"sp", "c4k"}                                      # these synchronise per call: a shorter block is enough
variants = {"k4k": k4k, "k4f": k4f, "k4r": k4r, "kh": kh, "r4k": r4k,
            "sp": lambda: grid.score_poses(scan, poses, field=(raw, k)),
            "c4k": lambda: grid.check_poses(scan, poses, tolerance=TOLERANCE, planes=planes),
            "k4k_again": k4k}
times = alternate({name: (fn, 2 if name in host_bound else BLOCK) for name, fn in variants.items()}, SAMPLES, 2)


def looked_at(rows, counts):
    """Mean steps a row's walk looked at — to the hit, else to the end cell (an upper bound where the beam leaves the grid) —
    over the rows with cells, and the classes' shares."""
    r = np.concatenate([rows[b, :n] for b, n in enumerate(counts)]).astype(np.int64)
    r = r[r[:, _lib.GK_ROW_CLASS] >= 0]
    steps = np.where(r[:, _lib.GK_ROW_K_HIT] >= 0, r[:, _lib.GK_ROW_K_HIT], r[:, _lib.GK_ROW_K]) + 1
    share = {name: round(float((r[:, _lib.GK_ROW_CLASS] == c).mean()), 4) for name, c in (
        ("confirmed", _lib.GK_CLASS_CONFIRMED), ("violated", _lib.GK_CLASS_VIOLATED), ("in_free", _lib.GK_CLASS_IN_FREE),
        ("unexplored", _lib.GK_CLASS_UNEXPLORED))}
    return {"rows": int(len(r)), "mean_steps": round(float(steps.mean()), 2), **share}


cast = cast_out.cpu().numpy().astype(np.int64)
segs, _ = gridmatch.ray_end_cells(grid.min_x, grid.min_y, grid.resolution, poses[:, :2], np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1),
                                  np.stack([np.cos(angles), np.sin(angles)], axis=1), REACH)
K = np.abs(segs[..., 2:] - segs[..., :2]).max(axis=-1)
walked = {"4k": looked_at(rows4r.cpu().numpy(), [ROWS] * POSES), "h": looked_at(rowsh.cpu().numpy(), hist.raw.counts_host()[:RESIDENT]),
          "r4k": {"rows": int(K.size), "mean_steps": round(float((np.where(cast[..., 0] >= 0, cast[..., 0], K) + 1).mean()), 2),
                  "hit_share": round(float((cast[..., 0] >= 0).mean()), 4)}}
out = {"grid": [ny, nx], "resolution": grid.resolution, "block": BLOCK, "tolerance": TOLERANCE, "reach_m": REACH, "counters": "none collected",
       "walked": walked}
for name in variants:
    out[name] = stats(times[name])
for name, w in (("k4k", "4k"), ("kh", "h"), ("r4k", "r4k")):
    out[name + "_giga_steps_per_s"] = round(walked[w]["rows"] * walked[w]["mean_steps"] / (float(np.median(times[name])) * 1e-3) / 1e9, 3)
out["k4k_spread_ms"] = round(abs(float(np.median(times["k4k"]) - np.median(times["k4k_again"]))), 4)
print(json.dumps(out))
