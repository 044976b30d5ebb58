#!/usr/bin/env python3
"""The cast (icpmi.gridmatch.occupancy_planes / cast_rays behind OccupancyGrid2D.cast_scans) on bench.py's config-4 grid
(2 242 x 2 402 cells at 0.05 m, 32 scans applied), one process on one GPU, device events, the variants alternating:

  (pl)    the planes pass alone (icpmi_grid_occupancy_planes of the kept raw field), the entry called with arguments prepared
          once — a launch this short is otherwise hidden behind the Python wrapper's own time per call;
  (r1)    one pose x 2 048 beams over kept planes, reach 30 m, the entry called directly;
  (r4k)   4 096 poses x 360 beams over kept planes, the entry called directly; sampled twice (r4k_again);
  (r4f)   the same from the field: the call packs the planes first;
  (s1), (s4k)   (r1) and (r4k) through OccupancyGrid2D.cast_scans with kept planes: upload of the poses, the launch, the
          records read back and the ranges formed on the host — what a caller waits for;
  (s4f)   (s4k) without kept planes: score_field and the packing per call as well;
  (f), (sp)   the raw field alone and score_poses of one 1 430-row scan at 4 096 poses, for scale.

Further libraries named on the command line (built by `make variant VSRC=gridcast NAME=... DEFS=...` into lib/) add (pl), (r1)
and (r4k) of their own under their name: other chunk lengths of the walk (-DICPMI_GC_CHUNK=1, 8, 16) — and, when the kernel
was chosen, the walk by runs of one row and a transposed second pair of planes (DESIGN.md has their times).  Every variant's
records are compared with the shipped library's before anything is timed.

A sample is BLOCK runs back to back between two events, divided by BLOCK; SAMPLES samples per variant after a warm-up of
each.  |median(r4k) - median(r4k_again)| is the run-to-run spread a difference has to exceed.  The planes pass's byte floor
is 2.25 B per cell (2 read, 2 bits written); its share is floor / time at ICPMI_HBM_TBS (default 8.0, the MI355X's HBM3E peak
in TB/s).  The walk's rate is rays x mean steps looked at (to the hit, or all the steps inside the grid) per second.  No
hardware counters are collected.  There is no earlier capability to compare a time against.

usage: time_cast.py [samples] [block] [libicpmi_variant.so ...]   (prints one JSON line)"""
import json
import os
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import _lib, gridmatch, synth
from icpmi.batch import _ptr, _stream

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
EXTRA = sys.argv[3:]
HBM_TBS = float(os.environ.get("ICPMI_HBM_TBS", "8.0"))
REACH, POSES, BEAMS, ROWS = 30.0, 4096, 360, 1430


def library(name):
    """A variant library of lib/ (every object but one is the shipped library's), with the shipped loader's signatures."""
    return _lib.bind(os.path.join(os.path.dirname(_lib.LIB_PATH), name))


assert torch.cuda.is_available(), "time_cast.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
raw, k = grid.score_field()
ny, nx = raw.shape
threshold = int(np.rint(0.5 * 2.0 ** k))
dev = raw.device
rng = np.random.default_rng(11)
poses = np.stack([rng.uniform(-3.0, 3.0, POSES), rng.uniform(-2.0, 2.0, POSES), rng.uniform(-np.pi, np.pi, POSES)], axis=1)
sets = {"1": (poses[:1], np.linspace(-np.pi, np.pi, 2048, endpoint=False)), "4k": (poses, np.linspace(-np.pi, np.pi, BEAMS, endpoint=False))}


def device_rows(p, a):
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)                                # noqa: E731
    return up(p[:, :2]), up(np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], axis=1)), up(np.stack([np.cos(a), np.sin(a)], axis=1))


rows = {n: device_rows(p, a) for n, (p, a) in sets.items()}
outs = {n: torch.empty((len(p), len(a), 4), dtype=torch.int32, device=dev) for n, (p, a) in sets.items()}


def entries(L):
    """(the planes pass, {set: the cast over kept planes}, the cast that packs first) of one library, arguments made once"""
    buf = torch.empty(L.icpmi_grid_occupancy_planes_bytes(ny, nx), dtype=torch.uint8, device=dev)
    ws = torch.empty_like(buf)
    pack_args = (_ptr(raw), ny, nx, threshold, _ptr(buf), buf.numel(), _stream())

    def pack():
        rc = L.icpmi_grid_occupancy_planes(*pack_args)
        assert rc == 0, rc

    def cast_of(n, kept):
        xy, pcs, bcs = rows[n]
        args = (None if kept else _ptr(raw), _ptr(buf) if kept else None, ny, nx, threshold, grid.min_x, grid.min_y, grid.resolution, _ptr(xy),
                _ptr(pcs), xy.shape[0], _ptr(bcs), bcs.shape[0], REACH, _ptr(outs[n]), _ptr(ws), ws.numel(), _stream())

        def run():
            rc = L.icpmi_grid_cast_rays(*args)
            assert rc == 0, rc
        return run
    pack()
    return pack, {n: cast_of(n, True) for n in sets}, cast_of("4k", False), buf


shipped = _lib.lib()
pack, kept, from_field, _ = entries(shipped)
variants = {"pl": pack, "r1": kept["1"], "r4k": kept["4k"], "r4f": from_field}
records = {}
for n in sets:
    kept[n]()
    records[n] = outs[n].cpu().numpy().copy()
from_field()
assert np.array_equal(outs["4k"].cpu().numpy(), records["4k"])
for name in EXTRA:
    tag = os.path.splitext(name)[0].replace("libicpmi_", "")
    v_pack, v_kept, _, _ = entries(library(name))
    for n in sets:
        outs[n].fill_(-7)
        v_kept[n]()
        assert np.array_equal(outs[n].cpu().numpy(), records[n]), f"{name}: records differ from the shipped library's"
    variants.update({f"pl_{tag}": v_pack, f"r1_{tag}": v_kept["1"], f"r4k_{tag}": v_kept["4k"]})
planes = grid.occupancy_planes(field=(raw, k))
variants["s1"] = lambda: grid.cast_scans(sets["1"][0], sets["1"][1], REACH, planes=planes)
variants["s4k"] = lambda: grid.cast_scans(sets["4k"][0], sets["4k"][1], REACH, planes=planes)
variants["s4f"] = lambda: grid.cast_scans(sets["4k"][0], sets["4k"][1], REACH)
full = synth.scan((0.5, -0.1, np.deg2rad(14.0)), 4242)
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
variants["f"] = grid.score_field
variants["sp"] = lambda: grid.score_poses(scan, poses, field=(raw, k))
variants["r4k_again"] = kept["4k"]
host_bound = {"s1", "s4k", "s4f", "sp"}                          # these synchronise per call: a shorter block is enough
times = alternate({name: (fn, 2 if name in host_bound else BLOCK) for name, fn in variants.items()}, SAMPLES, 2)

# what the walks looked at: the steps to the hit, or every step inside the grid (the origins are inside it)
steps = {}
for n, (p, a) in sets.items():
    rec = records[n].astype(np.int64)
    segs, _ = gridmatch.ray_end_cells(grid.min_x, grid.min_y, grid.resolution, p[:, :2], np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], axis=1),
                                      np.stack([np.cos(a), np.sin(a)], axis=1), REACH)
    dx, dy = segs[..., 2] - segs[..., 0], segs[..., 3] - segs[..., 1]
    xmajor = np.abs(dx) >= np.abs(dy)
    m0, d, size = np.where(xmajor, segs[..., 0], segs[..., 1]), np.where(xmajor, dx, dy), np.where(xmajor, nx, ny)
    inside = np.minimum(np.abs(d), np.where(d > 0, size - 1 - m0, m0)) + 1
    looked = np.where(rec[..., 0] >= 0, rec[..., 0] + 1, inside)
    steps[n] = {"rays": int(rec[..., 0].size), "hit_share": round(float((rec[..., 0] >= 0).mean()), 4), "mean_steps": round(float(looked.mean()), 2),
                "x_major_share": round(float(xmajor.mean()), 4), "unknown_first_share": round(float((rec[..., 3] >= 0).mean()), 4)}
cells = ny * nx
floor_ms = 2.25 * cells / (HBM_TBS * 1e12) * 1e3
out = {"grid": [ny, nx], "resolution": grid.resolution, "block": BLOCK, "reach_m": REACH, "hbm_tbs": HBM_TBS, "counters": "none collected",
       "planes_bytes": int(shipped.icpmi_grid_occupancy_planes_bytes(ny, nx)), "field_bytes": 2 * cells, "walked": steps,
       "planes_byte_floor_ms": round(floor_ms, 5)}
for name in variants:
    out[name] = stats(times[name])
for name in variants:
    if name.startswith("pl"):
        out[name + "_share_of_byte_floor"] = round(floor_ms / float(np.median(times[name])), 4)
    if name.startswith("r1") or name.startswith("r4k"):
        w = steps["1" if name.startswith("r1") else "4k"]
        out[name + "_giga_steps_per_s"] = round(w["rays"] * w["mean_steps"] / (float(np.median(times[name])) * 1e-3) / 1e9, 3)
out["r4k_spread_ms"] = round(abs(float(np.median(times["r4k"]) - np.median(times["r4k_again"]))), 4)
print(json.dumps(out))
