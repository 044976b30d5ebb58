#!/usr/bin/env python3
"""The resident particle filter (icpmi.particles.ParticleFilter: icpmi_pf_predict, icpmi_grid_beam_batch, icpmi_pf_weights,
icpmi_pf_resample, icpmi_pf_estimate) beside the path a caller had without it, in the same run: bench.py's config-4 grid
(2 242 x 2 402 cells at 0.05 m, 32 scans applied) with kept planes, one 360-row scan, N = 512, 4 096 and 65 536 particles,
one process on one GPU, device events, the variants alternating.  Per N:

  (predict, beam, weights, resample, estimate)
            each stage's C entry alone on the filter's own tensors, arguments prepared once; `beam` is the beam model's
            launch on the resident particles as the filter makes it (ParticleFilter.scan_pairs once, .beam per run) — the
            yardstick the step is held against;
  (step)    the five stages enqueued back to back, resampling every time, nothing read back: what the device does per scan;
  (filter)  ParticleFilter.predict / weigh / maybe_resample / estimate with their read-backs (the four sums, the eight
            moments) and the scan's upload: what a caller waits for per scan;
  (host)    the path of a caller without the filter: OccupancyGrid2D.beam_poses (poses up, records back), pose_weights,
            systematic resampling and the motion model in NumPy, and the poses with their cos / sin uploaded again.

A sample is BLOCK runs back to back between two events, divided by BLOCK (2 for the variants that synchronise per run);
SAMPLES samples per variant after a warm-up of each.  `beam_again` samples the yardstick twice: |median(beam) -
median(beam_again)| is the run-to-run spread a difference has to exceed.  No hardware counters are collected.

With --global the same grid serves the start over the free cells and the recovery by injection instead (icpmi_pf_free_index,
icpmi_pf_draw_uniform):

  (index)   the free index of the whole grid, built again into its buffer (FreeCells.build: three launches);
  (draw_n)  every one of n = 4 096, 65 536 and 2^20 slots drawn from it;
  (step, step_inject)
            per N = 4 096 and 65 536, the five-stage step above and the same step with n / 4 slots of the resampled
            generation drawn anew, ancestors marked;
  (host_start)
            what the parent of this feature could offer for a start: the field read back, np.nonzero of its free cells,
            NumPy draws and ParticleFilter.set_poses, at n = 4 096;

and, once and without a clock, a whole-map start in the room map of the test suite (200 x 280 cells at 0.1 m, twelve scans
of 64 rows) at 2^18 particles over the full circle: the error of the estimate at every scan.

usage: time_particles.py [--global] [samples] [block]   (prints one JSON line)"""
import json
import sys

from timing import alternate, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import _lib, gridmatch, synth
from icpmi.batch import _ptr, _stream

GLOBAL = "--global" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--global"]
SAMPLES = int(ARGS[0]) if len(ARGS) > 0 else 21
BLOCK = int(ARGS[1]) if len(ARGS) > 1 else 20
SIZES, ROWS, HALF_WIDTH, TEMPERATURE = (4096, 512, 65536), 360, 8, 8.0
CONTROL, MOTION = (0.02, 0.0, 0.005), (0.01, 0.01, 0.002)

assert torch.cuda.is_available(), "time_particles.py measures on the GPU: there is nothing to time without one"
import bench
grid, org, hits, _ = bench.raycast_workload(synth, 32)
grid.update_scans(org, hits)
planes = grid.occupancy_planes()
L = _lib.lib()
full = synth.scan((0.5, -0.1, np.deg2rad(14.0)), 4242)           # tools/time_beam.py's scan
scan = full[np.linspace(0, len(full) - 1, ROWS).astype(np.int64)]
one = gridmatch.cloud_set_of([scan])
start = np.array([0.5, -0.1, np.deg2rad(14.0)])


def variants_of(n):
    """-> {name: (run, runs per sample)} for n particles, started as a cloud about the scan's pose"""
    pf = grid.particle_filter(n, seed=n, temperature=TEMPERATURE, half_width=HALF_WIDTH, planes=planes)
    pf.init_gaussian(start, (0.2, 0.2, 0.05))
    pf.weigh(scan)                                                 # leaves real weights
    pairs = pf.scan_pairs(one, 0)                                  # the prepared call weigh() makes, on the present generation
    p, st = pf.planes, _stream()
    spare = pf._spare

    def call(fn, *args):
        def run():
            rc = fn(*args)
            assert rc == 0, rc
        return run

    state = (_ptr(pf.pair_t), _ptr(pf.theta), _ptr(pf.cos_sin))
    predict = call(L.icpmi_pf_predict, n, *state, *CONTROL, *MOTION, pf.seed, 1, st)
    beam = lambda: pf.beam(pairs)                                  # noqa: E731
    weights = call(L.icpmi_pf_weights, n, _ptr(pf.records), _ptr(pf._weight_table), len(pf.weight_table_host), pf.weight_shift, _ptr(pf.w),
                   _ptr(pf.sums), st)
    # (the resampled generation goes to the spare buffers and is not swapped in: every run reads the same particles)
    resample = call(L.icpmi_pf_resample, n, _ptr(pf.w), *state, _ptr(spare[0]), _ptr(spare[1]), _ptr(spare[2]), _ptr(pf.ancestors), _ptr(pf.info),
                    pf.seed, 2, _ptr(pf._ws), pf._ws.numel(), st)
    estimate = call(L.icpmi_pf_estimate, n, _ptr(pf.w), state[0], state[2], _ptr(pf.moments), _ptr(pf._ws), pf._ws.numel(), st)
    # the motion noise is small and the control is undone every other run, so the cloud stays where the map is
    back = call(L.icpmi_pf_predict, n, *state, *(-v for v in CONTROL), *MOTION, pf.seed, 3, st)
    flip = [0]

    def move():
        flip[0] ^= 1
        (predict if flip[0] else back)()

    def step():
        move()
        beam()
        weights()
        resample()
        estimate()

    if GLOBAL:
        # (as the resampled generation, the injected slots go to the spare buffers)
        inject = call(L.icpmi_pf_draw_uniform, n, n // 4, _ptr(pf.free_cells().index), grid.min_x, grid.min_y, grid.resolution, 0.0, 2.0 * np.pi,
                      _ptr(spare[0]), _ptr(spare[1]), _ptr(spare[2]), _ptr(pf.ancestors), _ptr(pf.draw_info), pf.seed, 2, st)

        def step_inject():
            step()
            inject()

        return {"step": (step, BLOCK), "step_inject": (step_inject, BLOCK), "step_again": (step, BLOCK)}, (pf,)

    own = grid.particle_filter(n, seed=n + 1, temperature=TEMPERATURE, half_width=HALF_WIDTH, planes=planes)
    own.init_gaussian(start, (0.2, 0.2, 0.05))

    def filter_step():
        flip[0] ^= 1
        own.predict(CONTROL if flip[0] else tuple(-v for v in CONTROL), MOTION)
        own.weigh(scan)
        own.maybe_resample(0.5)
        return own.estimate()

    rng = np.random.default_rng(n)
    host_poses = [start + rng.normal(size=(n, 3)) * (0.2, 0.2, 0.05)]
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(p.buf.device)            # noqa: E731

    def host_step():
        poses = host_poses[0]
        flip[0] ^= 1
        u = np.array(CONTROL if flip[0] else tuple(-v for v in CONTROL)) + rng.normal(size=(n, 3)) * MOTION
        c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
        poses = poses + np.stack([c * u[:, 0] - s * u[:, 1], s * u[:, 0] + c * u[:, 1], u[:, 2]], axis=1)
        info = grid.beam_poses(scan, poses, half_width=HALF_WIDTH, planes=planes)
        w, ess = gridmatch.pose_weights(info["score"], temperature=TEMPERATURE, status=info["status"])
        if ess < 0.5 * n:
            anc = np.minimum(np.searchsorted(np.cumsum(w), (rng.random() + np.arange(n)) / n), n - 1)
            poses = poses[anc]
        host_poses[0] = poses
        mean = (w[:, None] * poses[:, :2]).sum(axis=0)
        keep = (up(poses[:, :2]), up(np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)))      # the next step's upload
        return mean, keep

    return {"predict": (move, BLOCK), "beam": (beam, BLOCK), "weights": (weights, BLOCK), "resample": (resample, BLOCK), "estimate": (estimate, BLOCK),
            "step": (step, BLOCK), "filter": (filter_step, 2), "host": (host_step, 2), "beam_again": (beam, BLOCK)}, (pf, own)


def room_start(n):
    """A start over every free cell of the suite's room map and the full circle, n particles, the twelve scans of the track
    thinned to 64 rows -> what the filter settles on, scan by scan (run once: nothing is timed)."""
    from utilities.mapping import OccupancyGrid2D
    poses = np.array([(-1.0 + 0.25 * k, -0.5 + 0.02 * k, 0.05 * k) for k in range(12)])             # tests/gridmatch_ref.py: SCENE_POSES
    room = OccupancyGrid2D(min_x=-14.0, max_x=14.0, min_y=-10.0, max_y=10.0, resolution=0.1)
    for k, p in enumerate(poses):
        room.update_scan(p[:2].copy(), synth.to_world(synth.scan(tuple(p), 50 + k), tuple(p)))
    pf = room.particle_filter(n, seed=1, temperature=TEMPERATURE, half_width=HALF_WIDTH)
    free = pf.free_cells().count()
    pf.init_uniform()
    track = []
    for k, p in enumerate(poses):
        if k:
            a, d = poses[k - 1], p[:2] - poses[k - 1, :2]
            c, s = np.cos(a[2]), np.sin(a[2])
            pf.predict((c * d[0] + s * d[1], -s * d[0] + c * d[1], p[2] - a[2]), (0.05, 0.05, np.deg2rad(1.0)))
        ess, ok = pf.weigh(synth.scan(tuple(p), 50 + k)[::32])
        did = pf.maybe_resample(0.5)
        est = pf.estimate()
        track.append({"scan": k, "ess": round(ess, 1), "ok": ok, "resampled": did, "best_score": pf.last_sums[_lib.PF_SUM_SMAX],
                      "error_m": round(float(np.hypot(*(est["mean"][:2] - p[:2]))), 3),
                      "error_deg": round(float(np.degrees(abs((est["mean"][2] - p[2] + np.pi) % (2 * np.pi) - np.pi))), 2),
                      "resultant": round(est["resultant"], 4)})
    return {"particles": n, "free_cells": free, "track": track}


def global_report():
    pf = grid.particle_filter(2 ** 20, seed=5, planes=planes)
    free = pf.free_cells()
    frame = (grid.min_x, grid.min_y, grid.resolution, 0.0, 2.0 * np.pi)

    def draw(n):
        def run():
            rc = L.icpmi_pf_draw_uniform(n, n, _ptr(free.index), *frame, _ptr(pf.pair_t), _ptr(pf.theta), _ptr(pf.cos_sin), None, _ptr(pf.draw_info),
                                         pf.seed, 1, _stream())
            assert rc == 0, rc
        return run

    small = grid.particle_filter(4096, seed=6, planes=planes)
    rng = np.random.default_rng(6)
    threshold = planes[0].threshold

    def host_start():
        f = grid.score_field()[0].cpu().numpy()                    # the field read back
        ys, xs = np.nonzero((f != 0) & (f < threshold))
        pick = rng.integers(0, len(xs), size=small.n)
        small.set_poses(np.stack([grid.min_x + (xs[pick] + rng.random(small.n)) * grid.resolution,
                                  grid.min_y + (ys[pick] + rng.random(small.n)) * grid.resolution, rng.uniform(-np.pi, np.pi, small.n)], axis=1))

    variants = {"index": (free.build, BLOCK), "draw_4096": (draw(4096), BLOCK), "draw_65536": (draw(65536), BLOCK), "draw_1048576": (draw(2 ** 20), BLOCK),
                "host_start": (host_start, 2), "index_again": (free.build, BLOCK)}
    times = alternate(variants, SAMPLES, 2)
    res = {name: stats(times[name]) for name in variants}
    res["free_cells"] = free.count()
    for n in (4096, 65536):
        steps, _ = variants_of(n)
        times = alternate(steps, SAMPLES, 2)
        res[f"n{n}"] = {name: stats(times[name]) for name in steps}
        res[f"n{n}"]["inject_adds_ms"] = round(float(np.median(times["step_inject"]) - np.median(times["step"])), 4)
        res[f"n{n}"]["step_spread_ms"] = round(abs(float(np.median(times["step"]) - np.median(times["step_again"]))), 4)
    res["room_start"] = room_start(2 ** 18)
    return res


out = {"grid": [grid.ny, grid.nx], "resolution": grid.resolution, "rows": ROWS, "block": BLOCK, "half_width": HALF_WIDTH, "temperature": TEMPERATURE,
       "counters": "none collected"}
if GLOBAL:
    out.update(global_report())
    print(json.dumps(out))
    sys.exit(0)
for n in SIZES:
    variants, keep = variants_of(n)
    times = alternate(variants, SAMPLES, 2)
    med = lambda name: float(np.median(times[name]))                                              # noqa: E731
    res = {name: stats(times[name]) for name in variants}
    res["stages_sum_ms"] = round(sum(med(s) for s in ("predict", "beam", "weights", "resample", "estimate")), 4)
    res["step_over_beam"] = round(med("step") / med("beam"), 3)
    res["filter_over_beam"] = round(med("filter") / med("beam"), 3)
    res["host_over_filter"] = round(med("host") / med("filter"), 3)
    res["beam_spread_ms"] = round(abs(med("beam") - med("beam_again")), 4)
    res["ess_of_the_last_filter_step"] = round(float(keep[1].ess), 1)
    out[f"n{n}"] = res
print(json.dumps(out))
