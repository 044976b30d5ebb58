#!/usr/bin/env python3
"""The beam model (icpmi.gridmatch.beam_pairs behind OccupancyGrid2D.beam_scans / beam_poses / beam_history) beside the check
(check_pairs) on the same inputs in the same run: bench.py's config-4 grid (2 242 x 2 402 cells at 0.05 m, 32 scans applied),
one process on one GPU, device events, the variants alternating:

  (k4k)   the check: 4 096 poses x one 360-row scan over kept planes, the library's prepared call (gridmatch.MapPairs.check
          and .beam, outputs given): checked and uploaded once, then run — the yardstick; sampled twice (k4k_again);
  (b4k)   the beam model on those pairs: half width 8, the default table, beyond = 1.5 * (8 + 2) cells;
  (b4h)   (b4k) with the histograms written as well;
  (b4r)   (b4k) with the rows' records written as well;
  (b4z)   (b4k) with beyond = 0: the check's own walks, so what is left is the table, the sum and the third cell;
  (kh)    the check: 512 scans of 2 048 rows resident in a ScanHistory, by id at the poses they were taken from, kept planes,
          the rows' records written (as tools/time_check.py's kh);
  (bh)    the beam model on those pairs, the rows' records written;
  (p4k)   (b4k) through OccupancyGrid2D.beam_poses with kept planes: upload of the poses, the launches and the records read
          back — what a caller waits for.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  |median(k4k) - median(k4k_again)| is the run-to-run spread a difference has to exceed.  The expectation for b4k / k4k
is the check's time plus the extra steps of `beyond`: `walked` gives the mean steps a row's walk looked at in each.  No
hardware counters are collected.

usage: time_beam.py [samples] [block]   (prints one JSON line)"""
import json
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import ScanHistory, _lib, gridmatch, synth

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 21
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
POSES, ROWS, RESIDENT, TOLERANCE, HALF_WIDTH = 4096, 360, 512, 2, 8

assert torch.cuda.is_available(), "time_beam.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
raw, k = grid.score_field()
ny, nx = raw.shape
threshold = int(np.rint(0.5 * 2.0 ** k))
dev = raw.device
planes = grid.occupancy_planes(field=(raw, k))
up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)                                    # noqa: E731
BEYOND = 1.5 * (HALF_WIDTH + 2) * grid.resolution
table_host = gridmatch.beam_table(grid.resolution, grid.resolution, HALF_WIDTH)
table = up(table_host)

rng = np.random.default_rng(11)                                 # tools/time_check.py's poses, scan and history
poses = np.stack([rng.uniform(-3.0, 3.0, POSES), rng.uniform(-2.0, 2.0, POSES), rng.uniform(-np.pi, np.pi, POSES)], axis=1)
full = synth.scan((0.5, -0.1, np.deg2rad(14.0)), 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
one = gridmatch.cloud_set_of([scan])

drive = [(0.3 + 0.0012 * i, -0.2 + 0.0006 * i, np.deg2rad(10.0 + 0.03 * i)) for i in range(RESIDENT)]       # inside the mapped drive
hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=RESIDENT, row_capacity=RESIDENT * 2048)
hist.add_many([synth.scan(p, 7000 + i) for i, p in enumerate(drive)])
drive = np.array(drive)


def entry_of(cs, pair_host, xyt, beyond=None, want_hist=False, want_rows=False):
    """The library's prepared call over one set of pairs over the kept planes, its outputs made once: the check (beyond None)
    or the beam model -> (run, records, hist, rows)"""
    pairs = gridmatch.MapPairs(planes[0], threshold, grid.min_x, grid.min_y, grid.resolution, cs, pair_host, up(xyt[:, :2]),
                               up(np.stack([np.cos(xyt[:, 2]), np.sin(xyt[:, 2])], axis=1)))
    rec = torch.empty((pairs.B, _lib.GB_INTS), dtype=torch.int32, device=dev)
    bins = torch.empty((pairs.B, 2 * HALF_WIDTH + 3), dtype=torch.int32, device=dev) if want_hist else None
    rows = torch.empty((pairs.B, pairs.stride, _lib.GB_ROW_INTS), dtype=torch.int32, device=dev) if want_rows else None
    if beyond is None:
        out = (rec, rows) if want_rows else rec
        return (lambda: pairs.check(TOLERANCE, want_rows, out)), rec, bins, rows
    return (lambda: pairs.beam(table, HALF_WIDTH, beyond, want_hist, want_rows, (rec, bins, rows))), rec, bins, rows


assert _lib.GB_INTS == _lib.GK_INTS and _lib.GB_ROW_INTS == _lib.GK_ROW_INTS
zeros = np.zeros(POSES, dtype=np.int32)
k4k, krec, _, _ = entry_of(one, zeros, poses)
k4r, _, _, krows = entry_of(one, zeros, poses, want_rows=True)       # (not timed: the check's steps for `walked`)
b4k, brec, _, _ = entry_of(one, zeros, poses, BEYOND)
b4h, bhrec, bbins, _ = entry_of(one, zeros, poses, BEYOND, want_hist=True)
b4r, brrec, _, brows = entry_of(one, zeros, poses, BEYOND, want_rows=True)
b4z, _, _, _ = entry_of(one, zeros, poses, 0.0)
kh, _, _, khrows = entry_of(hist.raw, np.arange(RESIDENT), drive, want_rows=True)
bh, bhist_rec, _, bhrows = entry_of(hist.raw, np.arange(RESIDENT), drive, BEYOND, want_rows=True)
for fn in (k4k, k4r, b4k, b4h, b4r, b4z, kh, bh):
    fn()
want = brec.cpu().numpy()
assert np.array_equal(bhrec.cpu().numpy(), want) and np.array_equal(brrec.cpu().numpy(), want)
assert np.array_equal(bbins.cpu().numpy().astype(np.int64) @ table_host.astype(np.int64), want[:, _lib.GB_REC_SCORE])
info = grid.beam_poses(scan, poses, half_width=HALF_WIDTH, planes=planes)
assert np.array_equal(info["score"], want[:, _lib.GB_REC_SCORE]) and np.array_equal(info["rows"], want[:, _lib.GB_REC_ROWS])

variants = {"k4k": k4k, "b4k": b4k, "b4h": b4h, "b4r": b4r, "b4z": b4z, "kh": kh, "bh": bh,
            "p4k": lambda: grid.beam_poses(scan, poses, half_width=HALF_WIDTH, planes=planes),
            "k4k_again": k4k}
host_bound = {"p4k"}                                            # synchronises per call: a shorter block is enough
times = alternate({name: (fn, 2 if name in host_bound else BLOCK) for name, fn in variants.items()}, SAMPLES, 2)


def looked_at(rows, counts, k_end):
    """Mean steps a row's walk looked at — to the hit, else to the end cell of the walk (an upper bound where the beam leaves
    the grid; ``k_end`` the slot that holds it, or None where the rows do not: then the hit rows alone) — over the rows with
    cells, and the share of rows with a hit."""
    r = np.concatenate([rows[b, :n] for b, n in enumerate(counts)]).astype(np.int64)
    r = r[r[:, 0] >= 0]
    hit = r[:, 1] >= 0
    out = {"rows": int(len(r)), "hit_share": round(float(hit.mean()), 4), "mean_steps_to_hit": round(float((r[hit, 1] + 1).mean()), 2)}
    if k_end is not None:
        out["mean_steps"] = round(float((np.where(hit, r[:, 1], r[:, k_end]) + 1).mean()), 2)
    return out


counts_h = hist.raw.counts_host()[:RESIDENT]
walked = {"k4k": looked_at(krows.cpu().numpy(), [ROWS] * POSES, _lib.GK_ROW_K), "b4k": looked_at(brows.cpu().numpy(), [ROWS] * POSES, None),
          "kh": looked_at(khrows.cpu().numpy(), counts_h, _lib.GK_ROW_K), "bh": looked_at(bhrows.cpu().numpy(), counts_h, None)}
rec = want.astype(np.int64)
out = {"grid": [ny, nx], "resolution": grid.resolution, "block": BLOCK, "tolerance": TOLERANCE, "half_width": HALF_WIDTH, "beyond_m": BEYOND,
       "counters": "none collected", "walked": walked,
       "b4k_records": {"rows": int(rec[:, _lib.GB_REC_ROWS].sum()), "expected": int(rec[:, _lib.GB_REC_EXPECTED].sum()),
                       "novel": int(rec[:, _lib.GB_REC_NOVEL].sum()), "unexplored": int(rec[:, _lib.GB_REC_UNEXPLORED].sum())}}
for name in variants:
    out[name] = stats(times[name])
med = lambda name: float(np.median(times[name]))                                                    # noqa: E731
out["b4k_over_k4k"] = round(med("b4k") / med("k4k"), 3)
out["b4z_over_k4k"] = round(med("b4z") / med("k4k"), 3)
out["bh_over_kh"] = round(med("bh") / med("kh"), 3)
out["k4k_spread_ms"] = round(abs(med("k4k") - med("k4k_again")), 4)
print(json.dumps(out))
