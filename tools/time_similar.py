#!/usr/bin/env python3
"""The appearance signatures of the resident scan history (ScanHistory(signature=...), ScanHistory.similar), one process on
one GPU, device events around the runs (tools/timing.py), medians with quartiles:

  (i)   add() of one 720-beam scan into a history with and without a signature store, alternating: what
        icpmi_history_signatures_add adds to the chain of icpmi_history_add;
  (ii)  one query against 4096 resident scans, top_k 10: on the device alone (BLOCK runs back to back between two events)
        and as a caller waits for it (run() and unpack() — the synchronisation and the read-back of the records — on the
        host's clock);
  (iii) all pairs of the 4096 scans with every score kept (all_scores: the similarity matrix of the run), one run per sample;
  (iv)  the host's way to (ii)'s answer: signatures() read back and the NumPy restatement of tests/signatures_ref.py.

The history holds 256 distinct scans of the single room of icpmi.synth, each sixteen times (the kernels do the same work
whatever the words hold).  Before any timing the records of (ii) are compared with the restatement's, bit for bit.

usage: time_similar.py [samples] [block]   (prints one JSON line)"""
import json
import os
import sys
import time

from timing import REPO, alternate, sample, stats  # (first: it puts the repository on sys.path)
import numpy as np
import torch

sys.path.insert(0, os.path.join(REPO, "tests"))
import signatures_ref as ref  # noqa: E402
from icpmi import ScanHistory, synth  # noqa: E402

SAMPLES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
BLOCK = int(sys.argv[2]) if len(sys.argv) > 2 else 20
DISTINCT, COPIES, BEAMS, TOP = 256, 16, 720, 10
N = DISTINCT * COPIES
VOXEL, NORMAL_K, RS_VOXEL = 0.04, 12, 0.15

assert torch.cuda.is_available(), "time_similar.py measures on the GPU: there is nothing to time without one"
rng = np.random.default_rng(11)
poses = []
while len(poses) < DISTINCT + 8:
    x, y = rng.uniform(synth.ROOM[0], synth.ROOM[2]), rng.uniform(synth.ROOM[1], synth.ROOM[3])
    if synth._free_pose(x, y):
        poses.append((x, y, rng.uniform(-np.pi, np.pi)))
scans = [synth.scan(p, 9100 + i, n_beams=BEAMS) for i, p in enumerate(poses)]
extra = scans[DISTINCT:]

with_sig = ScanHistory(VOXEL, NORMAL_K, RS_VOXEL, scan_capacity=N + 1024, row_capacity=(N + 1024) * BEAMS, signature={})
without = ScanHistory(VOXEL, NORMAL_K, RS_VOXEL, scan_capacity=1024, row_capacity=1024 * BEAMS)
for _ in range(COPIES):
    with_sig.add_many(scans[:DISTINCT])
torch.cuda.synchronize()
assert len(with_sig) == N

# (ii), and its check
one = with_sig.similar(N - 1, top_k=TOP, hi=N)
one.run()
one.unpack()
words, bits = with_sig.signatures()
want, _ = ref.similar(words, bits, [N - 1], [0], [N], N, TOP)
equal = bool(np.array_equal(one.records, want))


def waited():
    t0 = time.perf_counter()
    one.run()
    one.unpack()
    return (time.perf_counter() - t0) * 1e3


for _ in range(5):
    waited()
t_waited = [waited() for _ in range(SAMPLES * 4)]
t_one = alternate({"one": (one.run, BLOCK)}, SAMPLES, 3)["one"]

# (iii)
every = with_sig.similar(list(range(N)), top_k=TOP, hi=N, all_scores=True)
t_all = alternate({"all": (every.run, 1)}, SAMPLES, 2)["all"]
every.unpack()
diagonal = bool((every.all[np.arange(N), np.arange(N)] == (65535 << 8)).all())
del every

# (iv)
def on_the_host():
    t0 = time.perf_counter()
    w, b = with_sig.signatures()
    ref.similar(w, b, [N - 1], [0], [N], N, TOP)
    return (time.perf_counter() - t0) * 1e3


t_host = [on_the_host() for _ in range(max(SAMPLES // 3, 3))]

# (i)
k = {"with": 0, "without": 0}


def adder(hist, name):
    def add_one():
        hist.add(extra[k[name] % len(extra)])
        k[name] += 1
    return add_one


capacities = (with_sig.scan_capacity, without.scan_capacity)
t_add = alternate({"with": (adder(with_sig, "with"), BLOCK), "without": (adder(without, "without"), BLOCK)}, SAMPLES, 3)
assert (with_sig.scan_capacity, without.scan_capacity) == capacities, "a history grew while add() was timed"

pairs = N * N
out = {"shape": f"{N} resident scans of {BEAMS} beams ({DISTINCT} distinct), top_k {TOP}", "block": BLOCK,
       "records_equal_to_restatement": equal, "all_pairs_diagonal_is_65535": diagonal,
       "i_add_with_signatures": stats(t_add["with"]), "i_add_without": stats(t_add["without"]),
       "i_difference_ms": round(float(np.median(t_add["with"]) - np.median(t_add["without"])), 4),
       "ii_one_query_device": stats(t_one), "ii_one_query_waited_host_clock": stats(t_waited),
       "iii_all_pairs": stats(t_all),
       "iii_pairs_per_second": round(pairs / (float(np.median(t_all)) * 1e-3)),
       "iii_lane_operations_per_second": round(pairs * 128 * 64 / (float(np.median(t_all)) * 1e-3)),
       "iv_host_readback_and_numpy": stats(t_host)}
print(json.dumps(out))
