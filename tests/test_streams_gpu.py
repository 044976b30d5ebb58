"""The stream side of the library on the device: include/icpmi.h promises that every call is asynchronous on the stream
it is given and that calls may come from several host threads, and the resident classes repeat it (``run()`` enqueues on
the current stream without a synchronisation).  Everywhere else in the suite the current stream is the null stream, where
a dropped or wrong stream argument changes nothing.  The workloads are those of tests/stream_cases.py.

A. Ordered behind the stream it was given, one test per workload.  A reference object runs twice on the default stream
   (the two runs must agree: the workload is repeatable).  A second object is built from the same arrays and every device
   tensor it owns is poisoned.  Then, on a stream of its own: a delay kernel, an event ``gate`` behind it, the restoring
   copies, ``run`` twice, copies of the outputs.  When the last of these has been enqueued the delay must still be
   running (``not gate.query()``) — otherwise some call waited for the stream, or the delay was too short to tell; the
   delay starts at 20 ms and is doubled up to five times, and a run that never gets there fails as inconclusive.  After
   the stream has drained the copies must equal the reference bit for bit.  A launch, memset, copy or sort that went to
   any other stream ran during the delay, on poison; the second of the two runs catches a stray memset, which would clear
   a counter before the first run has dirtied it.

B. In flight together: the objects of bench.py's pipelined mode and their neighbours, enqueued round-robin over three
   streams for five rounds, and the same from three host threads; every object's outputs must equal what it gave alone.
   ICP2_SIDE is left unset, so every caller stream shares the library's side stream, its events and its lock.

The far continuation cannot be observed from the records.  The far pairs of the large batches are built as
test_far_pairs_finish_on_the_far_continuation_with_the_same_bits builds its pairs; that some of them took the path is read
from the third counter of the ICP workspace (stream_cases.icp_counters), which the preconditions below assert."""
import threading

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

DELAY_MS = 20.0                      # the first delay; doubled while the enqueueing outlasts it
DOUBLINGS = 5
delays_needed = {}                   # workload -> the delay (ms) behind which its enqueueing finished


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import features, pose_graph
    keep = features.VERBOSE, pose_graph.VERBOSE
    features.VERBOSE = pose_graph.VERBOSE = False                 # (set once here: three threads call the pose graph at a time)
    yield torch
    features.VERBOSE, pose_graph.VERBOSE = keep


@pytest.fixture(scope="module")
def cycles_per_ms(gpu):
    """What ``torch.cuda._sleep`` takes as a millisecond, measured once on a long sleep."""
    torch = gpu
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)                                  # the first launch loads the kernel
    torch.cuda.synchronize()
    start.record()
    torch.cuda._sleep(20_000_000)
    end.record()
    torch.cuda.synchronize()
    rate = 20_000_000 / start.elapsed_time(end)
    print(f"torch.cuda._sleep: {rate:.0f} cycles per ms")
    return rate


def host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def set_options(libopt, w):
    for name, value in w.options.items():
        libopt.setenv(name, value)


def reference(torch, w, seed=0):
    """(object, outputs after one run, after a second) on the default stream."""
    obj = w.build(seed)
    torch.cuda.synchronize()
    w.run(obj)
    torch.cuda.synchronize()
    first = host(w.outputs(obj))
    w.run(obj)
    torch.cuda.synchronize()
    return obj, first, host(w.outputs(obj))


@pytest.mark.parametrize("name", list(sc.WORKLOADS))
def test_ordered_behind_its_stream(gpu, cycles_per_ms, libopt, name):
    torch = gpu
    w = sc.WORKLOADS[name]
    set_options(libopt, w)
    ref, first, want = reference(torch, w)
    w.compare(first, want)                                        # the precondition: the workload repeats itself
    preconditions(name, ref, want)
    s = torch.cuda.Stream()
    for attempt in range(DOUBLINGS + 1):
        delay = DELAY_MS * 2 ** attempt
        dut = w.build(0)                                          # has never run: its scratch holds nothing valid
        torch.cuda.synchronize()
        owned = sc.owned_tensors(dut)
        assert owned, name
        clean = {path: t.clone() for path, t in owned.items()}
        sc.poison_(owned.values())
        torch.cuda.synchronize()
        gate = torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(delay * cycles_per_ms))
            gate.record()
            for path, t in owned.items():
                t.copy_(clean[path])
            w.run(dut)
            w.run(dut)
            snapshots = [t.clone() for t in w.outputs(dut)]
            still_delayed = not gate.query()
        s.synchronize()
        torch.cuda.synchronize()
        if still_delayed:
            break
        print(f"{name}: the enqueueing outlasted a delay of {delay:.0f} ms")
    else:
        pytest.fail(f"{name}: inconclusive — after a delay of {delay:.0f} ms the gate had passed when the last call returned: "
                    "a call waits for its stream, or the host side takes longer than that")
    delays_needed[name] = delay
    print(f"{name}: enqueued behind a delay of {delay:.0f} ms; {len(owned)} tensors poisoned and restored")
    w.compare(want, host(snapshots))


def large_batch_preconditions(batch, results, counters):
    """The conditions the batch's numbers stand for, asserted from a solo run: pairs in the second stage, clouds in the wide
    launch, pairs sent to the far continuation."""
    from icpmi import _lib
    B = sc.LARGE_B
    iters, status = results[:B, _lib.RES_ITERS], results[:B, _lib.RES_STATUS]
    cnt = batch.vox.cnt.cpu().numpy()
    print(f"large batch: {(iters > 12).sum()} pairs beyond 12 iterations, {(cnt > 1536).sum()} clouds above 1 536 rows, "
          f"statuses {sorted(set(status.astype(int).tolist()))}, counters (second stage, wide, far) {counters.tolist()}")
    assert (iters > 12).sum() >= 8 and counters[0] >= 8           # they took the second stage
    assert (cnt > 1536).sum() >= 8 and counters[1] >= 8           # the wide launch ran (on the side stream)
    assert counters[2] >= 1                                       # the far continuation had pairs to finish
    assert (iters >= 1).all() and set(status.astype(int).tolist()) <= {1, 2, 3}       # every pair registered, nobody left parked


def preconditions(name, ref, want):
    from icpmi import _lib
    if name in ("icp_two_stage_wide", "icp_p2p_two_stage"):
        large_batch_preconditions(ref, *want)
    elif name == "icp_big_target":
        assert int(ref.vox.cnt[1].item()) == sc.BIG_TARGET_ROWS   # the target keeps every row: the prep_big.hip path
        assert want[0][0, _lib.RES_ITERS] >= 2
    elif name == "icp_gated":
        assert int(want[2][0]) == sc.GATED_FIRST                  # the third pair is the first accepted
    elif name == "history_match":
        print("history_match: first accepted", int(want[2][0]))
        assert int(want[2][0]) >= 0
    elif name == "voxel_large":
        assert 0 < int(want[1][0]) < sc.VOXEL_LARGE_ROWS
    elif name == "particle_round":
        assert int(want[6][0]) == 0 and want[4][_lib.PF_SUM_W] > 0        # the resampling was not degenerate: particles had weights
    elif name in ("grid_match", "grid_search"):
        assert (want[0][:, _lib.GMREC_STATUS] == _lib.GM_ST_OK).all()


# ── B. in flight together ────────────────────────────────────────────────────
IN_FLIGHT = (("icp_two_stage_wide", 0), ("icp_two_stage_wide", 1), ("icp_gated", 0), ("history_match", 0), ("grid_search", 0),
             ("particle_round", 0))
ROUNDS = 5


@pytest.fixture(scope="module")
def solo(gpu):
    """[(workload, object, its outputs alone)] of the objects of part B, and the results of the three pose-graph calls, each
    run alone on the default stream."""
    torch = gpu
    objects = []
    for name, seed in IN_FLIGHT:
        w = sc.WORKLOADS[name]
        assert not w.options
        obj = w.build(seed)
        w.run(obj)
        torch.cuda.synchronize()
        want = host(w.outputs(obj))
        if name == "icp_two_stage_wide":
            large_batch_preconditions(obj, *want)
        objects.append((w, obj, want))
    assert objects[0][2][0].tobytes() != objects[1][2][0].tobytes()                  # the two large batches are different batches
    graphs = {kind: sc.pose_graph_call(kind) for kind in sc.POSE_GRAPH_CASES}
    return objects, graphs


def compare_all(torch, objects):
    torch.cuda.synchronize()
    for w, obj, want in objects:
        try:
            w.compare(want, host(w.outputs(obj)))
        except AssertionError as e:
            raise AssertionError(f"{w.name}: {e}") from None


def test_batches_in_flight_on_three_streams(gpu, solo):
    torch = gpu
    objects, graphs = solo
    streams = [torch.cuda.Stream() for _ in range(3)]
    last = [None] * len(objects)                                  # the event behind each object's latest run
    kinds = list(sc.POSE_GRAPH_CASES)
    for r in range(ROUNDS):
        for k, (w, obj, _) in enumerate(objects):
            s = streams[(k + r) % 3]                              # the assignment rotates: an object changes streams every round
            with torch.cuda.stream(s):
                if last[k] is not None:
                    s.wait_event(last[k])                         # one object is run by one stream at a time
                w.run(obj)
                last[k] = torch.cuda.Event()
                last[k].record()
        kind = kinds[r % 3]
        with torch.cuda.stream(streams[(r + 1) % 3]):             # synchronises that stream, the others stay in flight
            sc.compare_bits(graphs[kind], sc.pose_graph_call(kind))
    compare_all(torch, objects)


def test_calls_from_three_host_threads(gpu, solo):
    torch = gpu
    objects, graphs = solo
    kinds = list(sc.POSE_GRAPH_CASES)
    barrier = threading.Barrier(3)
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            barrier.wait(timeout=60)
            with torch.cuda.stream(s):
                for _ in range(ROUNDS):
                    for w, obj, _ in objects[k::3]:
                        w.run(obj)
                    sc.compare_bits(graphs[kinds[k]], sc.pose_graph_call(kinds[k]))
            s.synchronize()
        except BaseException as e:                                # re-raised in the main thread
            errors.append((k, e))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise AssertionError(f"thread {errors[0][0]}: {errors[0][1]!r}") from errors[0][1]
    compare_all(torch, objects)
