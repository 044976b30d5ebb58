#!/usr/bin/env python3
"""The resident scan history (icpmi.history.ScanHistory) against the batch path it replaces, one process on one GPU,
device events around run(), the variants alternating:

  (a) RunIcpPairBatch.run() on bench.py's config5_run_icp_pair_512 shape: 512 loop-closure candidates (2048-beam scans
      within 0.6 m / 6 degrees) of one current scan — filter, means, both search orders, search, ICP;
  (b) ScanHistory.match(...).run() on the same 512 targets already resident — search, ICP;
  (c) the same 512 targets inside a history of 4096 scans (the query must not scale with the history);
  (d) add() of one 2048-beam scan (upload, both filters, means, both search orders).

A sample is BLOCK runs back to back between two events, divided by BLOCK (one run is about a millisecond: too short a
window by itself); SAMPLES samples per variant after a warm-up of each.  (a) is sampled twice, as a1 and a2, in the same
alternation: |median a1 - median a2| and their quartiles are the run-to-run spread a difference has to exceed.  Before any
timing the records of (b) and (c) are compared with (a)'s, bit for bit.

--alignment features | both: the same protocol for the resident feature alignment (a history built with feat_cfg) — (a)
and (b) only, the feature records compared too, and (d) is an add() with the per-scan features.  The default,
rotation_search, is the measurement described above, unchanged.

usage: time_history.py [samples] [block] [--alignment {rotation_search,features,both}]   (prints one JSON line)"""
import json
import sys

from timing import alternate, sample, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

from icpmi import ScanHistory, synth
from icpmi.prealign import RunIcpPairBatch

ICP = dict(error_threshold=1e-10, max_iterations=150, method="point_to_line")
VOXEL, NORMAL_K, RS_VOXEL = 0.04, 12, 0.15
STEPS = dict(angle_step_coarse=1.5, angle_step_fine=0.1, max_rows_hint=1024)
ALIGNMENT = "rotation_search"
if "--alignment" in sys.argv:
    k = sys.argv.index("--alignment")
    ALIGNMENT = sys.argv[k + 1]
    assert ALIGNMENT in ("rotation_search", "features", "both"), ALIGNMENT
    del sys.argv[k:k + 2]
SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, BIG = 512, 4096


def records(b):
    return b.icp.results.cpu().numpy()[:b.B].copy(), b.search.records.cpu().numpy()[:b.B].copy()


def time_add(hist, samples, block):
    """(d): add() of one 2048-beam scan, cycling over eight scans."""
    extra = [synth.scan((0.1 * (i % 7), -0.05 * (i % 5), 0.01 * i), 8800 + i) for i in range(8)]
    k = [0]

    def add_one():
        hist.add(extra[k[0] % len(extra)])
        k[0] += 1
    capacity = hist.scan_capacity
    sample(add_one, 3)
    t = [sample(add_one, block) for _ in range(samples)]
    assert hist.scan_capacity == capacity, "the history grew while add() was timed"
    return t


def feature_alignment(method):
    """(a) against (b) for "features" / "both": the reference's feature configuration, one hypothesis table for both."""
    srcs, tgts = synth.loop_closure_batch(N, seed0=7000, shared_source=True, max_offset=0.6, max_yaw_deg=6.0)
    src = srcs[0]
    draws = np.random.default_rng(0).random((1000, 2))

    class Fixed:
        def random(self, shape):
            return draws
    batch = RunIcpPairBatch([src] + list(tgts), np.zeros(N, dtype=np.int32), np.arange(1, N + 1, dtype=np.int32),
                            voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, alignment_method=method, rng=Fixed(),
                            **ICP, **STEPS)
    rows = sum(len(t) for t in tgts)
    hist = ScanHistory(VOXEL, NORMAL_K, RS_VOXEL, scan_capacity=1024, row_capacity=rows + 600 * 2048, feat_cfg={})
    ids = hist.add_many(list(tgts))
    m = hist.match(hist.add(src), ids, alignment_method=method, rng=Fixed(), **ICP, **STEPS)
    batch.run(); m.run()
    parts = lambda b: [b.icp.results, b.features.records] + ([b.search.records] if b.search is not None else [])   # noqa: E731
    equal = all(np.array_equal(x.cpu().numpy()[:N], y.cpu().numpy()[:N], equal_nan=True) for x, y in zip(parts(m), parts(batch)))
    rec = batch.features.records.cpu().numpy()[:N]
    variants = {"a1": batch.run, "b": m.run, "a2": batch.run}
    times = alternate({k: (fn, BLOCK) for k, fn in variants.items()}, SAMPLES, 3)
    t_add = time_add(hist, SAMPLES, BLOCK)
    a = np.array(times["a1"] + times["a2"])
    return {"alignment": method, "shape": f"{N} candidates of 2048-beam scans, one source", "block": BLOCK,
            "records_equal_to_batch": bool(equal), "pairs_aligned": int(((rec[:, 12] == 0) & (rec[:, 5] >= 3)).sum()),
            "a_batch": stats(a), "a1": stats(times["a1"]), "a2": stats(times["a2"]),
            "a_spread_ms": round(abs(float(np.median(times["a1"]) - np.median(times["a2"]))), 4),
            "b_resident": stats(times["b"]), "d_add_one_scan_with_features": stats(t_add),
            "b_minus_a_ms": round(float(np.median(times["b"]) - np.median(a)), 4)}


assert torch.cuda.is_available(), "time_history.py measures on the GPU: there is nothing to time without one"
if ALIGNMENT != "rotation_search":
    print(json.dumps(feature_alignment(ALIGNMENT)))
    sys.exit(0)
srcs, tgts = synth.loop_closure_batch(N, seed0=7000, shared_source=True, max_offset=0.6, max_yaw_deg=6.0)
src = srcs[0]
batch = RunIcpPairBatch([src] + list(tgts), np.zeros(N, dtype=np.int32), np.arange(1, N + 1, dtype=np.int32),
                        voxel_size=VOXEL, normal_k=NORMAL_K, rotation_voxel_size=RS_VOXEL, **ICP, **STEPS)

rows = sum(len(t) for t in tgts)
small = ScanHistory(VOXEL, NORMAL_K, RS_VOXEL, scan_capacity=1024, row_capacity=rows + 600 * 2048)
ids = small.add_many(list(tgts))
m_small = small.match(small.add(src), ids, **ICP, **STEPS)

big = ScanHistory(VOXEL, NORMAL_K, RS_VOXEL, scan_capacity=BIG + 8, row_capacity=(BIG // N) * rows + 8 * 2048)
big.add_many(list(tgts) * (BIG // N))                                     # target j again at j + 512, j + 1024, ...
spread = np.array([(j % (BIG // N)) * N + j for j in range(N)])            # the same 512 targets, all over the history
m_big = big.match(big.add(src), spread, **ICP, **STEPS)

batch.run(); m_small.run(); m_big.run()
want = records(batch)
equal = {name: bool(np.array_equal(records(m)[0], want[0], equal_nan=True) and np.array_equal(records(m)[1], want[1], equal_nan=True))
         for name, m in (("b", m_small), ("c", m_big))}

variants = {"a1": batch.run, "b": m_small.run, "c": m_big.run, "a2": batch.run}
times = alternate({k: (fn, BLOCK) for k, fn in variants.items()}, SAMPLES, 3)

t_add = time_add(small, SAMPLES, BLOCK)

a = np.array(times["a1"] + times["a2"])
out = {"shape": f"{N} candidates of 2048-beam scans, one source; history of (c): {len(big)} scans", "block": BLOCK,
       "records_equal_to_batch": equal,
       "a_batch": stats(a), "a1": stats(times["a1"]), "a2": stats(times["a2"]),
       "a_spread_ms": round(abs(float(np.median(times["a1"]) - np.median(times["a2"]))), 4),
       "b_resident": stats(times["b"]), "c_resident_in_4096": stats(times["c"]), "d_add_one_scan": stats(t_add),
       "b_minus_a_ms": round(float(np.median(times["b"]) - np.median(a)), 4),
       "c_minus_b_ms": round(float(np.median(times["c"]) - np.median(times["b"])), 4)}
print(json.dumps(out))
