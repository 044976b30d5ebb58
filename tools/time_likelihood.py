#!/usr/bin/env python3
"""The likelihood field (icpmi.gridmatch.likelihood_field behind OccupancyGrid2D.likelihood_field) on bench.py's config-4 grid
(2 242 x 2 402 cells at 0.05 m, 32 scans applied), one process on one GPU, device events, the variants alternating:

  (f)    the raw field alone (icpmi_grid_score_field of the whole grid), for scale;
  (lR)   the likelihood field of the kept raw field at a radius of R cells, R in 3, 6, 20, 64 (sigma R / 3 cells, free space
         kept): the copy of the table and lf_field_kernel, the entry called with arguments prepared once — a launch this
         short is otherwise hidden behind the Python wrapper's own time per call; l6 is sampled twice;
  (p6)   l6 through icpmi.gridmatch.likelihood_field (checks, workspace, table pointer per call): what a caller waits for;
  (d6)   the distance field alone at R = 6 (no table, one output), the entry called directly;
  (mr), (ml)   one 1 430-row scan, 25 angles x 13^2 shifts (W = 6), against the raw field and against the likelihood field
         (R = 6) kept as field=: the same kernels on another field;
  (sr), (sl)   the same scan through the wide search (W = 31, block 8), field and bound field kept, raw and likelihood.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  l6 is sampled twice, as l6 and l6_again, in the same alternation: |median - median| is the run-to-run spread a
difference has to exceed.  The build's byte floor is 4 B per cell (2 read, 2 written); its share is floor / time at
ICPMI_HBM_TBS (default 8.0, the MI355X's HBM3E peak in TB/s).  There is no earlier capability to compare a time against.

usage: time_likelihood.py [samples] [block]   (prints one JSON line)"""
import json
import os
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

import ctypes as C

from icpmi import _lib, gridmatch, synth
from icpmi.batch import CloudSet, _ptr, _stream
from icpmi.gridmatch import GridMatchBatch, GridSearchBatch, angle_grid

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
RADII, ROWS, W, W_WIDE = (3, 6, 20, 64), 1430, 6, 31
HBM_TBS = float(os.environ.get("ICPMI_HBM_TBS", "8.0"))


assert torch.cuda.is_available(), "time_likelihood.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
raw, k = grid.score_field()
threshold = int(np.rint(0.5 * 2.0 ** k))
peak = np.rint(grid.log_odds_max * 2.0 ** k)
tables = {R: gridmatch.likelihood_table(peak, R / 3.0, R) for R in RADII}
out_lf, out_d2 = torch.empty_like(raw), torch.empty_like(raw)


L = _lib.lib()
ny, nx = raw.shape
workspaces = {R: torch.empty(L.icpmi_grid_likelihood_workspace_bytes(ny, nx, R), dtype=torch.uint8, device=raw.device) for R in RADII}


def build(R, d2_only=False):
    """The entry with its arguments made once (everything runs on the current stream)"""
    ws, tab = workspaces[R], tables[R].ctypes.data_as(C.c_void_p)
    if d2_only:
        args = (_ptr(raw), ny, nx, threshold, R, None, 0, _ptr(out_d2), None, None, 0, _stream())
    else:
        args = (_ptr(raw), ny, nx, threshold, R, tab, 1, None, _ptr(out_lf), _ptr(ws), ws.numel(), _stream())
    entry = L.icpmi_grid_likelihood_field

    def run():
        rc = entry(*args)
        assert rc == 0, rc
    return run


like = (gridmatch.likelihood_field(raw, threshold, 6, tables[6], True), k)
true = (0.5, -0.1, np.deg2rad(14.0))
full = synth.scan(true, 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
pred = (true[0] + 0.12, true[1] - 0.08, true[2] + np.deg2rad(3.0))
angles, centre = angle_grid([pred[2]], 12.0, 1.0)
one = CloudSet.from_numpy([scan])
match = {n: GridMatchBatch(grid, one, [0], [pred[:2]], angles, W, centre, field=f) for n, f in (("mr", (raw, k)), ("ml", like))}
search = {n: GridSearchBatch(grid, one, [0], [pred[:2]], angles, W_WIDE, centre, block=8, field=f, bounds=gridmatch.bound_field(f[0], 8))
          for n, f in (("sr", (raw, k)), ("sl", like))}

variants = {"f": grid.score_field, "l6": build(6)}
variants.update({f"l{R}": build(R) for R in RADII if R != 6})
variants["p6"] = lambda: gridmatch.likelihood_field(raw, threshold, 6, tables[6], True, out=out_lf)
variants["d6"] = build(6, d2_only=True)
variants.update({n: j.run for n, j in match.items()})
variants.update({n: j.run for n, j in search.items()})
variants["l6_again"] = build(6)
times = alternate({name: (fn, BLOCK) for name, fn in variants.items()}, SAMPLES, 3)
found = {}
for n, job in list(match.items()) + list(search.items()):
    _, t, score, info = job.unpack()
    found[n] = {"err_m": [round(float(abs(t[0, i] - true[i])), 4) for i in (0, 1)], "err_deg": round(float(np.rad2deg(abs(info["angle"][0] - true[2]))), 3),
                "score": int(score[0])}
d2 = gridmatch.distance_field(raw, threshold, 6).cpu().numpy()
found["occupied_cells"] = int((d2 == 0).sum())
found["cells_within_6"] = int((d2 <= 36).sum())
cells = grid.ny * grid.nx
floor_ms = 4.0 * cells / (HBM_TBS * 1e12) * 1e3
out = {"grid": [grid.ny, grid.nx], "resolution": grid.resolution, "block": BLOCK, "found": found, "hbm_tbs": HBM_TBS,
       "byte_floor_ms": round(floor_ms, 5), "f_raw_field_alone": stats(times["f"])}
for R in RADII:
    out[f"l{R}_likelihood_field"] = stats(times[f"l{R}"])
    out[f"l{R}_share_of_byte_floor"] = round(floor_ms / float(np.median(times[f"l{R}"])), 4)
out.update({"l6_again": stats(times["l6_again"]),
            "l6_spread_ms": round(abs(float(np.median(times["l6"]) - np.median(times["l6_again"]))), 4),
            "p6_through_the_python_wrapper": stats(times["p6"]), "d6_distance_field_alone": stats(times["d6"]),
            "mr_match_raw_field": stats(times["mr"]), "ml_match_likelihood_field": stats(times["ml"]),
            "sr_search_raw_field": stats(times["sr"]), "sl_search_likelihood_field": stats(times["sl"])})
print(json.dumps(out))
