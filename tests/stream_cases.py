"""The workloads of the stream tests (tests/test_streams_cpu.py, tests/test_streams_gpu.py): every path of the library that
takes a stream, as a small record that can be built twice from the same arrays, run on whatever stream is current, and read.

A ``Workload`` has

- ``inputs(seed)``: the host arrays, a dict of NumPy arrays (lists of them), made by seeded generators only and cached —
  treat them as read-only;
- ``build(seed)``: a fresh object on the device — a resident object of the library, or a ``SimpleNamespace`` that holds one
  with the preallocated buffers of a set-style function.  Building may upload, allocate and synchronise;
- ``run(obj)``: enqueues the work on the current stream.  It uploads nothing, reads nothing back and, from its second call
  on, allocates nothing (a few wrappers allocate a scratch tensor per call from torch's caching allocator, which is
  ordered by the stream; none of them is an output);
- ``outputs(obj)``: the device tensors that hold the results, asked for after a ``run``;
- ``compare(want, got)``: both lists of host arrays in the order of ``outputs``.  Bit for bit unless the workload says
  otherwise: the gated runs are compared by the gate's contract, as tests/test_first_accepted.py compares them, because the
  candidates after the accepted one stop wherever the gate word reaches them;
- ``options``: switches of the library (``libopt``) the workload needs; ``entries`` / ``classes``: the C entries and the
  classes with a ``run`` method it reaches.

``owned_tensors`` and ``poison_`` are what part A of the GPU test stands on.  The poison is NaN in floating tensors and
zero bytes in integer and byte tensors, on purpose: a launch that runs too early then sees empty clouds (counts and
offsets of zero), pair lists that name cloud 0, and NaN coordinates.  Nothing it reads can send an index out of range,
so a stream bug in the library shows as wrong bits and never as a fault.

Importable without a GPU: torch and the library are imported inside the functions that need them.

The far continuation of the fused ICP cannot be observed from the records.  The far pairs of ``icp_two_stage_wide`` are
built as test_far_pairs_finish_on_the_far_continuation_with_the_same_bits builds its pairs (``loop_closure_batch`` with
offsets up to 3 m and 20 degrees), thinned to 128 beams; how many pairs took the path is the third of the workspace's
counters (``icp_counters``), which the large batches list among their outputs and the GPU test asserts to be positive.

The inventory — every ``extern "C"`` entry of include/icpmi.h with the workloads that reach it or the reason it is left
out, and every class of icpmi/ with a ``run`` method — is appended to this docstring when the module is imported
(``inventory_text``); tests/test_streams_cpu.py holds it complete.
"""
import collections
import ctypes as C
import functools
import types

import numpy as np

Workload = collections.namedtuple("Workload", "name inputs build run outputs compare options entries classes")

WORKLOADS = collections.OrderedDict()

NO_STREAM = "takes no stream: sizes, plans, options or text, answered on the host"
POSE_GRAPH = ("synchronises its stream by contract (csrc/posegraph.hip: the plan's vectors live on the call's stack frame), so it "
              "cannot sit behind a delay: part B only (test_batches_in_flight_on_three_streams, test_calls_from_three_host_threads)")

# entries no workload reaches, with the reason
EXCLUDED_ENTRIES = dict(
    {name: NO_STREAM for name in (
        "icpmi_version", "icpmi_strerror", "icpmi_set_option", "icpmi_shutdown", "icpmi_runtime_check", "icpmi_voxel_workspace_bytes",
        "icpmi_nn_batch_plan", "icpmi_normals_workspace_bytes", "icpmi_icp_workspace_bytes", "icpmi_prepared_bytes",
        "icpmi_rotation_search_workspace_bytes", "icpmi_rotation_refine_workspace_bytes", "icpmi_rotation_search_batch_workspace_bytes",
        "icpmi_feature_align_batch_workspace_bytes", "icpmi_history_feature_align_workspace_bytes", "icpmi_grid_workspace_bytes",
        "icpmi_grid_update_plan", "icpmi_grid_match_workspace_bytes", "icpmi_grid_search_workspace_bytes",
        "icpmi_grid_likelihood_workspace_bytes", "icpmi_grid_occupancy_planes_bytes", "icpmi_pf_workspace_bytes",
        "icpmi_pose_graph_workspace_bytes", "icpmi_pose_graph_weighted_workspace_bytes", "icpmi_pose_graph_dense_workspace_bytes",
        "icpmi_pose_graph_marginals_workspace_bytes", "icpmi_pose_graph_robust_workspace_bytes")},
    icpmi_pose_graph_optimize=POSE_GRAPH, icpmi_pose_graph_optimize_robust=POSE_GRAPH, icpmi_pose_graph_marginals=POSE_GRAPH,
    icpmi_pose_graph_optimize_dense="synchronises its stream like icpmi_pose_graph_optimize; taken only where a split is refused, which "
                                    "the chain cases of part B never are: not reached by the stream tests",
)
# classes of icpmi/ with a run method that no workload builds, with the reason
EXCLUDED_CLASSES = {
    "RunIcpPairSharded": "icpmi.dist: one batch over the GPUs of a node — multi-GPU is out of scope here",
}


def workload(name, entries, classes=(), options=None, compare=None):
    """Decorator of a class with ``inputs``, ``build``, ``run`` and ``outputs`` as static methods -> its Workload, registered."""
    def register(cls):
        inputs = functools.lru_cache(maxsize=None)(cls.inputs)
        w = Workload(name, inputs, lambda seed=0: cls.build(inputs(seed)), cls.run, cls.outputs, compare or compare_bits,
                     dict(options or {}), tuple(entries), tuple(classes))
        WORKLOADS[name] = w
        return w
    return register


# ── the two helpers of part A ────────────────────────────────────────────────
_LEAVES = (str, bytes, int, float, complex, bool, type(None), np.ndarray, np.generic, C._SimpleCData, C.Structure, C.Array)


def owned_tensors(obj, device_type="cuda"):
    """Every torch tensor on ``device_type`` that ``obj`` holds, once, keyed by its attribute path: the walk goes through
    the attributes of objects (the nested resident objects), lists, tuples and dicts.  A tensor met again under another
    path — or a second tensor over exactly the same memory — is listed under the first path only."""
    import torch
    found, seen_objects, seen_memory = collections.OrderedDict(), set(), set()

    def walk(x, path):
        if isinstance(x, torch.Tensor):
            key = (x.data_ptr(), x.dtype, tuple(x.shape), tuple(x.stride()))
            if x.device.type == device_type and x.numel() and key not in seen_memory:
                seen_memory.add(key)
                found[path] = x
            return
        if isinstance(x, _LEAVES) or isinstance(x, type) or callable(x) or isinstance(x, types.ModuleType):
            return
        if id(x) in seen_objects:
            return
        seen_objects.add(id(x))
        if isinstance(x, dict):
            for k, v in x.items():
                walk(v, f"{path}[{k!r}]")
        elif isinstance(x, (list, tuple)):
            for k, v in enumerate(x):
                walk(v, f"{path}[{k}]")
        elif hasattr(x, "__dict__") and not type(x).__module__.split(".")[0] in ("torch", "numpy", "ctypes", "builtins", "threading"):
            for k, v in vars(x).items():
                walk(v, f"{path}.{k}" if path else k)

    walk(obj, "")
    return found


def poison_(tensors):
    """NaN into every floating tensor, zero bytes into every integer, byte and bool tensor (the module docstring says why)."""
    for t in tensors:
        if t.dtype.is_floating_point or t.dtype.is_complex:
            t.fill_(float("nan"))
        else:
            t.zero_()


# ── comparisons ──────────────────────────────────────────────────────────────
def compare_bits(want, got):
    assert len(want) == len(got), (len(want), len(got))
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            av, bv = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
            bad = np.flatnonzero(av != bv)
            at = int(bad[0]) // a.dtype.itemsize
            raise AssertionError(f"output {k}: {len(bad)} bytes differ, first at element {at} of {a.size}: "
                                 f"want {a.reshape(-1)[at]!r}, got {b.reshape(-1)[at]!r}")


def compare_gated(want, got):
    """Outputs [full results, gated results, first accepted] by the contract of icpmi_icp_batch_gated, as
    tests/test_first_accepted.py::check_contract: the ungated run and the first accepted index bit for bit, every gated
    record up to the accepted one bit for bit, every later one either the ungated run's or SKIPPED (status 5)."""
    from icpmi import _lib
    compare_bits([want[0], want[2]], [got[0], got[2]])
    first = int(want[2].reshape(-1)[0])
    upto = len(want[1]) if first < 0 else first + 1
    compare_bits([want[1][:upto]], [got[1][:upto]])
    for i in range(upto, len(got[1])):
        if got[1][i, _lib.RES_STATUS] != _lib.ST_SKIPPED:
            assert got[1][i].tobytes() == got[0][i].tobytes(), f"gated record {i} is neither skipped nor the ungated run's"
    compare_bits(want[3:], got[3:])


# ── generators ───────────────────────────────────────────────────────────────
BASE = (0.5, -0.3, 0.1)              # the source pose of icpmi.synth.loop_closure_batch
FAR_POSES = ((-8.0, 4.0, 2.5), (8.5, -4.8, -2.0))      # other corners of the synthetic room: scans that match no scan near BASE


def near_pairs(n, seed0, beams, max_offset=0.6, max_yaw_deg=6.0, shared_source=False):
    """``synth.loop_closure_batch`` with ``beams[i]`` beams in pair i (the same draws per pair: distance, direction, yaw)."""
    from icpmi import synth
    srcs, tgts = [], []
    shared = synth.scan(BASE, seed0 - 1, n_beams=int(beams[0]))
    for i in range(n):
        rng = np.random.default_rng(seed0 + i)
        while True:
            d, a = rng.uniform(0.0, max_offset), rng.uniform(-np.pi, np.pi)
            th = np.deg2rad(rng.uniform(-max_yaw_deg, max_yaw_deg))
            pose = (BASE[0] + d * np.cos(a), BASE[1] + d * np.sin(a), BASE[2] + th)
            if synth._free_pose(pose[0], pose[1]):
                break
        srcs.append(shared if shared_source else synth.scan(BASE, seed0 + 7919 * (i + 1), n_beams=int(beams[i])))
        tgts.append(synth.scan(pose, seed0 + i, n_beams=int(beams[i])))
    return srcs, tgts


def jittered_lattice2d(n, seed, spacing=0.1, jitter=0.2):
    """The first n nodes of a square lattice, each moved by at most jitter * spacing per axis: two rows differ by at least
    (1 - 2 jitter) spacing along an axis, so a voxel filter finer than that keeps every row."""
    k = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((g + rng.uniform(-jitter, jitter, size=(n, 2))) * spacing)


def rot2(a):
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


SMALL_ROOM = dict(min_x=0.0, max_x=6.4, min_y=0.0, max_y=6.4, resolution=0.1, p_hit=0.85, p_miss=0.42, log_odds_min=-8.0,
                  log_odds_max=8.0)                                       # 64 x 64 cells
SMALL_ROOM_POSES = ((2.0, 2.0, 0.3), (2.6, 3.0, 1.0), (1.5, 4.5, -0.5))


def small_room_segments():
    from icpmi import synth
    segs = synth._rect_segments((0.6, 0.6, 5.8, 5.8)) + synth._rect_segments((3.6, 3.4, 4.4, 4.2))
    return np.array([[a[0], a[1], b[0], b[1]] for a, b in segs], dtype=np.float64)


def small_room_scans(seed, beams=128):
    from icpmi import synth
    segs = small_room_segments()
    return [synth.scan(p, 9100 + 10 * seed + k, n_beams=beams, segs=segs) for k, p in enumerate(SMALL_ROOM_POSES)]


def build_small_room(scans):
    """The 64 x 64 grid of the small room, built by two ``update_scan`` of each scan at its true pose (synchronised)."""
    import torch
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    g = OccupancyGrid2D(**SMALL_ROOM)
    assert (g.ny, g.nx) == (64, 64)
    for _ in range(2):
        for p, s in zip(SMALL_ROOM_POSES, scans):
            g.update_scan(np.array(p[:2]), synth.to_world(s, p))
    torch.cuda.synchronize()
    return g


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def calm(*scratch):
    """Zero-fill the scratch tensors of an object that has never run (``torch.empty`` workspaces; None is skipped) -> the
    first of them.  Part A restores behind its delay what the object held when it was built; with this that is zeros and
    not whatever the allocation held, so that under a stray memset a counter starts at zero or at what a run left — never at
    a value that could send an index out of range."""
    for t in scratch:
        if t is not None:
            t.zero_()
    return scratch[0] if scratch else None


def calm_icp(b):
    """``calm`` of an ``IcpBatch``'s own workspaces (a resident one points at its history's prepared targets: left alone)."""
    calm(b.icp_ws, getattr(b, "vox_ws", None), getattr(b, "nrm_ws", None), None if hasattr(b, "history") else b.prepared)
    return b


# ── fused ICP ────────────────────────────────────────────────────────────────
LARGE_B = 1024                       # the two-stage threshold of csrc/icp2.hip (plan_icp2: many)
WIDE_PAIRS = tuple(range(5, LARGE_B, 64))        # 16 pairs of 2 048-beam clouds: more than 1 536 rows at voxel 0.005
FAR_PAIRS = tuple(range(9, LARGE_B, 64))         # 16 pairs offset by up to 3 m and 20 degrees


def large_batch_inputs(seed):
    from icpmi import synth
    seed0 = 810000 + 5000 * seed
    beams = 64 + (np.arange(LARGE_B) * 37) % 65                       # 64 .. 128
    srcs, tgts = near_pairs(LARGE_B, seed0, beams)
    ws, wt = synth.loop_closure_batch(len(WIDE_PAIRS), seed0=seed0 + 2000)
    fs, ft = synth.loop_closure_batch(len(FAR_PAIRS), seed0=seed0 + 3000, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
    for k, i in enumerate(WIDE_PAIRS):
        srcs[i], tgts[i] = ws[k], wt[k]
    for k, i in enumerate(FAR_PAIRS):
        srcs[i], tgts[i] = fs[k][::16], ft[k][::16]
    return {"clouds": srcs + tgts}


def build_large_batch(inp, method):
    from icpmi import batch
    B = LARGE_B
    return calm_icp(batch.IcpBatch(inp["clouds"], np.arange(B), np.arange(B, 2 * B), error_threshold=1e-10, max_iterations=40,
                                   voxel_size=0.005, method=method, normal_k=12))


def run_batch(b):
    b.run()


def batch_results(b):
    return [b.results]


def icp_counters(b):
    """The three int32 counters at the end of a fast batch's ICP workspace (csrc/icp2.hip, Icp2Ws: parked rows 16 B +
    positions 4 B per source row | three lists of B | the counters): the pairs the last run parked for its second stage,
    listed for the wide launch and sent to the far continuation.  The launcher clears them with a memset on its stream; pairs
    listed twice are registered twice with the same result, so only the counters show a memset that ran too early."""
    import torch
    off = b.B * b.max_src_n * 20 + 3 * b.B * 4
    return b.icp_ws[off:off + 12].view(torch.int32)


def batch_results_and_counters(b):
    return [b.results, icp_counters(b)]


ICP_FAST = ("icpmi_voxel_downsample_batch", "icpmi_prepare_targets_ex", "icpmi_icp_batch")


@workload("icp_two_stage_wide", ICP_FAST, ("IcpBatch",))
class _IcpTwoStageWide:
    inputs = staticmethod(large_batch_inputs)
    build = staticmethod(lambda inp: build_large_batch(inp, "point_to_line"))
    run, outputs = staticmethod(run_batch), staticmethod(batch_results_and_counters)


@workload("icp_p2p_two_stage", ICP_FAST, ("IcpBatch",), options={"ICP2_STAGES": "2"})
class _IcpP2pTwoStage:
    inputs = staticmethod(large_batch_inputs)
    build = staticmethod(lambda inp: build_large_batch(inp, "point_to_point"))
    run, outputs = staticmethod(run_batch), staticmethod(batch_results_and_counters)


@workload("icp_exhaustive_3d", ("icpmi_voxel_downsample_batch", "icpmi_icp_batch"), ("IcpBatch",))
class _IcpExhaustive3d:
    @staticmethod
    def inputs(seed):
        from icpmi import synth
        R, t = synth.rot3(0.02, -0.015, 0.03), np.array([0.12, -0.08, 0.05])
        sizes = [(200, 260), (257, 300), (300, 257), (333, 400), (256, 256), (389, 211), (211, 389), (400, 333)]
        srcs = [synth.lattice3d(n, 100 + 20 * seed + k) @ R.T + t for k, (n, _) in enumerate(sizes)]
        tgts = [synth.lattice3d(m, 500 + 20 * seed + k) for k, (_, m) in enumerate(sizes)]
        return {"clouds": srcs + tgts}

    @staticmethod
    def build(inp):
        from icpmi import batch
        b = batch.IcpBatch(inp["clouds"], np.arange(8), np.arange(8, 16), error_threshold=1e-10, max_iterations=30, voxel_size=0.05)
        assert b.dim == 3 and not b.fast
        return calm_icp(b)

    run, outputs = staticmethod(run_batch), staticmethod(batch_results)


@workload("icp_exhaustive_p2l", ("icpmi_voxel_downsample_batch", "icpmi_normals_2d_batch", "icpmi_icp_batch"), ("IcpBatch",))
class _IcpExhaustiveP2l:
    @staticmethod
    def inputs(seed):
        srcs, tgts = near_pairs(8, 820000 + 100 * seed, [256] * 8)
        return {"clouds": srcs + tgts}

    @staticmethod
    def build(inp):
        from icpmi import batch
        b = batch.IcpBatch(inp["clouds"], np.arange(8), np.arange(8, 16), error_threshold=1e-10, max_iterations=30, voxel_size=0.04,
                           method="point_to_line", normal_k=10, force_exhaustive=True)
        assert not b.fast and b.use_p2l
        return calm_icp(b)

    run, outputs = staticmethod(run_batch), staticmethod(batch_results)


BIG_TARGET_ROWS = 4097               # one row above PREP_MAX_POINTS: the target is prepared through global memory (prep_big.hip)


@workload("icp_big_target", ICP_FAST, ("IcpBatch",))
class _IcpBigTarget:
    @staticmethod
    def inputs(seed):
        tgt = jittered_lattice2d(BIG_TARGET_ROWS, 830 + seed)
        src = (tgt[::8][:500] - tgt.mean(axis=0)) @ rot2(0.02).T + tgt.mean(axis=0) + np.array([0.03, -0.02])
        return {"clouds": [np.ascontiguousarray(src), tgt]}

    @staticmethod
    def build(inp):
        from icpmi import batch
        b = batch.IcpBatch(inp["clouds"], [0], [1], error_threshold=1e-10, max_iterations=30, voxel_size=0.02, method="point_to_line",
                           normal_k=10)
        assert b.fast and b.max_tgt_n == BIG_TARGET_ROWS > batch.PREP_MAX_POINTS
        return calm_icp(b)

    run, outputs = staticmethod(run_batch), staticmethod(batch_results)


GATE = 0.01                          # m^2: far above the residual of two scans of one place, far below that of two places
GATED_B, GATED_FIRST = 64, 2


def gated_targets(n, seed0, beams):
    """n candidate scans: the first GATED_FIRST taken in other corners of the room, the others near BASE."""
    from icpmi import synth
    _, near = near_pairs(n, seed0, [beams] * n, max_offset=0.3, max_yaw_deg=3.0, shared_source=True)
    for k in range(GATED_FIRST):
        near[k] = synth.scan(FAR_POSES[k], seed0 + 500 + k, n_beams=beams)
    return near


@workload("icp_gated", ICP_FAST + ("icpmi_icp_batch_gated",), ("IcpBatch",), compare=compare_gated)
class _IcpGated:
    @staticmethod
    def inputs(seed):
        from icpmi import synth
        seed0 = 840000 + 1000 * seed
        return {"clouds": [synth.scan(BASE, seed0 - 1, n_beams=256)] + gated_targets(GATED_B, seed0, 256)}

    @staticmethod
    def build(inp):
        from icpmi import batch
        B = GATED_B
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        kw = dict(error_threshold=1e-10, max_iterations=40, voxel_size=0.04, method="point_to_line", normal_k=12)
        full = batch.IcpBatch(cs, np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32), **kw)
        gated = batch.IcpBatch(cs, full.pairs, None, **kw)
        gated.set_gate(GATE)
        return types.SimpleNamespace(full=calm_icp(full), gated=calm_icp(gated))

    @staticmethod
    def run(o):
        o.full.run()
        o.gated.run()

    @staticmethod
    def outputs(o):
        return [o.full.results, o.gated.results, o.gated.first_accepted_dev]


@workload("information", ICP_FAST + ("icpmi_icp_information_batch",), ("IcpBatch",))
class _Information:
    @staticmethod
    def inputs(seed):
        srcs, tgts = near_pairs(16, 850000 + 100 * seed, [256] * 16)
        return {"clouds": srcs + tgts}

    @staticmethod
    def build(inp):
        from icpmi import batch
        b = batch.IcpBatch(inp["clouds"], np.arange(16), np.arange(16, 32), error_threshold=1e-10, max_iterations=30, voxel_size=0.04,
                           method="point_to_line", normal_k=12)
        return types.SimpleNamespace(batch=calm_icp(b), records=None)

    @staticmethod
    def run(o):
        o.batch.run()
        o.records = o.batch.information()

    @staticmethod
    def outputs(o):
        return [o.batch.results, o.records]


# ── the set functions ────────────────────────────────────────────────────────
VOXEL_LARGE_ROWS = 8193              # above the 8 192 rows the voxel filter sorts on chip: the rocPRIM path of csrc/voxel.hip


@workload("voxel_large", ("icpmi_voxel_downsample_batch",))
class _VoxelLarge:
    @staticmethod
    def inputs(seed):
        return {"clouds": [np.random.default_rng(860 + seed).uniform(-10.0, 10.0, size=(VOXEL_LARGE_ROWS, 2))]}

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, batch
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        out = batch.CloudSet(torch.zeros_like(cs.pts), cs.off_host, cnt=torch.zeros(1, dtype=torch.int32, device=cs.pts.device), off=cs.off)
        ws = torch.zeros(_lib.lib().icpmi_voxel_workspace_bytes(cs.max_n), dtype=torch.uint8, device=cs.pts.device)
        return types.SimpleNamespace(cs=cs, out=out, ws=ws)

    @staticmethod
    def run(o):
        from icpmi import batch
        batch.voxel_downsample_set(o.cs, 0.25, out=o.out, workspace=o.ws)

    @staticmethod
    def outputs(o):
        return [o.out.pts, o.out.cnt]


def dozen_clouds(seed):
    from icpmi import synth
    sizes = (40, 64, 65, 100, 128, 129, 200, 255, 256, 257, 300, 90)
    return {"clouds": [synth.scan((0.3 * k - 1.5, 0.1 * k, 0.2 * k), 870 + 20 * seed + k, n_beams=n) for k, n in enumerate(sizes)]}


def dozen_pairs():
    return np.arange(12, dtype=np.int32), ((np.arange(12) + 5) % 12).astype(np.int32)


@workload("nn_set", ("icpmi_nn_batch",))
class _NnSet:
    inputs = staticmethod(dozen_clouds)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import batch
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        pairs = batch.PairList(*dozen_pairs()).to(cs.pts.device)
        stride = int(np.diff(cs.off_host).max())
        out = (torch.zeros((12, stride), dtype=torch.float64, device=cs.pts.device), torch.zeros((12, stride), dtype=torch.int32, device=cs.pts.device))
        return types.SimpleNamespace(cs=cs, pairs=pairs, out=out)

    @staticmethod
    def run(o):
        from icpmi import batch
        batch.nn_set(o.cs, o.pairs, out=o.out)

    @staticmethod
    def outputs(o):
        return list(o.out)


@workload("nn_set_sweep", ("icpmi_prepare_targets", "icpmi_nn_prepared_batch"))
class _NnSetSweep:
    inputs = staticmethod(dozen_clouds)

    @staticmethod
    def build(inp):
        from icpmi import batch
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        pairs = batch.PairList(*dozen_pairs()).to(cs.pts.device)
        w = batch.SweepWorkspace(cs, pairs, return_second=True)
        for t in (w.idx, w.dist, w.second):
            t.zero_()
        return types.SimpleNamespace(cs=cs, pairs=pairs, w=w)

    @staticmethod
    def run(o):
        from icpmi import batch
        batch.nn_set_sweep(o.cs, o.pairs, return_second=True, workspace=o.w)

    @staticmethod
    def outputs(o):
        return [o.w.dist, o.w.idx, o.w.second]


@workload("normals_set", ("icpmi_prepare_targets_ex",))
class _NormalsSet:
    inputs = staticmethod(dozen_clouds)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, batch
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        dev = cs.pts.device
        ws = torch.zeros(_lib.lib().icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, cs.max_n), dtype=torch.uint8, device=dev)
        return types.SimpleNamespace(cs=cs, out=torch.zeros((cs.total_rows, 2), dtype=torch.float64, device=dev), ws=ws)

    @staticmethod
    def run(o):
        from icpmi import batch
        batch.normals_set(o.cs, 8, out=o.out, workspace=o.ws)

    @staticmethod
    def outputs(o):
        return [o.out]


# ── pre-alignment ────────────────────────────────────────────────────────────
def candidate_inputs(n, seed0, step):
    from icpmi import synth
    srcs, tgts = synth.loop_closure_batch(n, seed0=seed0, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
    return {"clouds": [srcs[0][::step]] + [t[::step] for t in tgts]}


def candidate_pairs(n):
    return np.zeros(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)


@workload("rotation_search_batch", ("icpmi_rotation_search_batch",), ("RotationSearchBatch",))
class _RotationSearchBatch:
    inputs = staticmethod(lambda seed: candidate_inputs(8, 880000 + 100 * seed, 8))

    @staticmethod
    def build(inp):
        from icpmi import prealign
        b = prealign.RotationSearchBatch(inp["clouds"], *candidate_pairs(8))
        calm(b.ws)
        return b

    run = staticmethod(run_batch)

    @staticmethod
    def outputs(b):
        return [b.records, b.init]


@workload("feature_align_batch", ("icpmi_feature_align_batch",), ("FeatureAlignBatch",))
class _FeatureAlignBatch:
    inputs = staticmethod(lambda seed: candidate_inputs(8, 881000 + 100 * seed, 4))

    @staticmethod
    def build(inp):
        import torch
        from icpmi import prealign
        start = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
        b = prealign.FeatureAlignBatch(inp["clouds"], *candidate_pairs(8), init_out=start)
        calm(b.ws)
        return b

    run = staticmethod(run_batch)

    @staticmethod
    def outputs(b):
        return [b.records, b.init_out]


@workload("run_icp_pair_batch", ICP_FAST + ("icpmi_rotation_search_batch", "icpmi_feature_align_batch"),
          ("RunIcpPairBatch", "IcpBatch", "RotationSearchBatch", "FeatureAlignBatch"))
class _RunIcpPairBatch:
    inputs = staticmethod(lambda seed: candidate_inputs(32, 882000 + 100 * seed, 8))

    @staticmethod
    def build(inp):
        from icpmi import prealign
        b = prealign.RunIcpPairBatch(inp["clouds"], *candidate_pairs(32), error_threshold=1e-10, max_iterations=40, voxel_size=0.04,
                                     normal_k=12, alignment_method="both")
        calm_icp(b.icp)
        calm(b.search.ws, b.features.ws)
        return b

    run = staticmethod(run_batch)

    @staticmethod
    def outputs(b):
        return [b.icp.results, b.search.records, b.features.records]


@workload("submap_rotation_search", ("icpmi_rotation_search", "icpmi_rotation_refine"))
class _SubmapRotationSearch:
    """``submap.submap_rotation_search`` up to its read-back: ``enqueue_submap_search`` on the tables and the device clouds the
    function itself would make.  The search context is the library's one per device, so a second object shares its buffers
    (``rec``, ``ref_out``) with the first: the outputs are read before the next object runs."""

    @staticmethod
    def inputs(seed):
        from icpmi import synth
        pose = (0.9, -0.1, 0.35)
        world = np.vstack([synth.to_world(synth.scan(p, 890 + 10 * seed + k, n_beams=512), p)
                           for k, p in enumerate(((0.5, -0.3, 0.1), (1.2, 0.1, 0.3), (0.2, 0.4, -0.2)))])
        return {"clouds": [synth.scan(pose, 899 + 10 * seed, n_beams=512), world], "pose": np.array(pose)}

    @staticmethod
    def build(inp):
        from icpmi import submap
        from icpmi.prealign import arange_rows
        from utilities.features import _SearchContext
        x, y, th = inp["pose"]
        guess = th + np.deg2rad(8.0)
        angles = guess + np.deg2rad(np.arange(-60.0, 60.0 + 2.0, 2.0))                                # slam.py:146-151
        fine, fine_n = arange_rows(angles - np.deg2rad(2.0), angles + np.deg2rad(2.0), np.deg2rad(0.5))
        ctx = _SearchContext.get()
        o = types.SimpleNamespace(ctx=ctx, src=submap._device_rows(inp["clouds"][0]), tgt=submap._device_rows(inp["clouds"][1]),
                                  dtab=ctx.device_table(angles, fine, fine_n), n_coarse=len(angles), max_fine=int(fine.shape[1]),
                                  pred_t=(float(x) + 0.1, float(y) - 0.05))
        if ctx.cap < 8192:                                       # the context grows (and allocates) outside run()
            ctx.upload(np.zeros((1, 2)), np.zeros((1, 2)))
        calm(ctx.workspace(len(o.src), len(o.tgt), o.n_coarse, o.max_fine), getattr(ctx, "ref_ws", None))
        return o

    @staticmethod
    def run(o):
        from icpmi import submap
        assert submap.enqueue_submap_search(o.ctx, o.src, o.tgt, o.dtab, o.n_coarse, o.max_fine, o.pred_t, 0.3)

    @staticmethod
    def outputs(o):
        return [o.ctx.rec, o.ctx.ref_out]


# ── the resident history ─────────────────────────────────────────────────────
HISTORY_SCANS = 8


def history_inputs(seed):
    from icpmi import synth
    seed0 = 900000 + 1000 * seed
    return {"clouds": gated_targets(HISTORY_SCANS - 1, seed0, 256) + [synth.scan(BASE, seed0 - 1, n_beams=256)]}


def build_history(inp):
    from icpmi import ScanHistory
    h = ScanHistory(voxel_size=0.04, normal_k=12, rotation_voxel_size=0.3, scan_capacity=16, row_capacity=4096, feat_cfg={})
    for t in (h.icp_prepared, h.rs_prepared):                     # the row arrays (40 bytes a row, csrc/prep_common.hpp): rows behind a
        t[:h.row_capacity * 40].zero_()                           # filtered cloud's count are never written — zero, so two histories agree
    calm(h.voxel_ws)
    assert h.add_many(inp["clouds"]) == list(range(HISTORY_SCANS))
    return h


@workload("history_match", ("icpmi_history_add", "icpmi_history_features_add", "icpmi_history_search", "icpmi_history_feature_align",
                            "icpmi_icp_batch", "icpmi_icp_batch_gated"),
          ("HistoryMatch", "_ResidentIcp", "_ResidentSearch", "_ResidentFeatures", "RunIcpPairBatch"), compare=compare_gated)
class _HistoryMatch:
    """``ScanHistory.add_many`` of 8 scans when the object is built (it uploads, so it cannot sit behind a delay); ``run``
    processes the resident scans again — the two launches of ``add_many``, ``icpmi_history_add`` and
    ``icpmi_history_features_add`` — and then matches the last scan against the others, ungated and gated."""
    inputs = staticmethod(history_inputs)

    @staticmethod
    def build(inp):
        h = build_history(inp)
        kw = dict(error_threshold=1e-10, max_iterations=40, alignment_method="both")
        cands = np.arange(HISTORY_SCANS - 1)
        o = types.SimpleNamespace(history=h, full=h.match(HISTORY_SCANS - 1, cands, **kw),
                                  gated=h.match(HISTORY_SCANS - 1, cands, error_accept=GATE, stop_after_first_accepted=True, **kw))
        for m in (o.full, o.gated):
            calm_icp(m.icp)
            calm(m.features.ws)
        return o

    @staticmethod
    def run(o):
        o.history._process(0, HISTORY_SCANS, True)
        o.full.run()
        o.gated.run()

    @staticmethod
    def outputs(o):
        return [o.full.icp.results, o.gated.icp.results, o.gated.icp.first_accepted_dev, o.full.search.records, o.full.features.records,
                o.gated.search.records, o.gated.features.records]


@workload("history_world_rows", ("icpmi_history_world_rows", "icpmi_prepared_relayout"))
class _HistoryWorldRows:
    """``ScanHistory.world_rows_into`` as ``world_rows`` calls it (the wrapper of tests/test_rebuild_gpu.py), on ids, poses and
    offsets uploaded when the object is built; and ``icpmi_prepared_relayout`` as ``ScanHistory._allocate`` calls it when a
    history grows, into a buffer for twice the scans and rows."""
    inputs = staticmethod(history_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib
        h = build_history(inp)
        rng = np.random.default_rng(17)
        order = [3, 0, 7, 7, 5, 1]
        poses = []
        for _ in order:
            x, y, th = rng.uniform(-3.0, 3.0, size=3)
            poses.append(np.array([[np.cos(th), -np.sin(th), x], [np.sin(th), np.cos(th), y], [0.0, 0.0, 1.0]]))
        ids, pose6, off = h.world_row_args(poses, order)
        S, R = 2 * h.scan_capacity, 2 * h.row_capacity
        nbytes = _lib.lib().icpmi_prepared_bytes(R, S, 0)
        return types.SimpleNamespace(history=h, n=len(ids), ids=_dev(ids), poses=_dev(pose6), off=_dev(off),
                                     rows=torch.zeros((int(off[-1]), 2), dtype=torch.float64, device=h.device), S=S, R=R, nbytes=nbytes,
                                     grown=torch.zeros(nbytes, dtype=torch.uint8, device=h.device))

    @staticmethod
    def run(o):
        from icpmi import _lib
        from icpmi.batch import _ptr, _stream
        h = o.history
        h.world_rows_into(o.rows, o.ids, o.poses, o.off, o.n)
        _lib.check(_lib.lib().icpmi_prepared_relayout(_ptr(h.icp_prepared), h.row_capacity, h.scan_capacity, h.rows_used, h.n_scans,
                                                      _ptr(o.grown), o.nbytes, o.R, o.S, _stream()), "prepared_relayout")

    @staticmethod
    def outputs(o):
        return [o.rows, o.grown]


# ── the occupancy grid: matching, searching, the pair entries, the filter, the update ───────────────────────────────────
def room_inputs(seed):
    return {"clouds": small_room_scans(seed)}


def match_arguments(seed, window_deg, step_deg):
    from icpmi import gridmatch
    rng = np.random.default_rng(910 + seed)
    truth = np.array(SMALL_ROOM_POSES)
    angles, centre = gridmatch.angle_grid(truth[:, 2] + np.deg2rad(rng.uniform(-2.0, 2.0, size=3)), window_deg, step_deg)
    return truth[:, :2] + rng.uniform(-0.15, 0.15, size=(3, 2)), angles, centre


@workload("grid_match", ("icpmi_grid_score_field", "icpmi_grid_match_batch", "icpmi_grid_match_moments"), ("GridMatchBatch",))
class _GridMatch:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        from icpmi import batch, gridmatch
        t, angles, centre = match_arguments(0, 6.0, 1.0)
        b = gridmatch.GridMatchBatch(build_small_room(inp["clouds"]), batch.CloudSet.from_numpy(inp["clouds"]), [0, 1, 2], t, angles, 4,
                                     centre, half_log_odds=1.0)
        calm(b.ws)
        return b

    run = staticmethod(run_batch)

    @staticmethod
    def outputs(b):
        return [b.records, b.scores, b.moments, b._field_buf]


@workload("grid_search", ("icpmi_grid_score_field", "icpmi_grid_bound_field", "icpmi_grid_search_batch"), ("GridSearchBatch",))
class _GridSearch:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        from icpmi import batch, gridmatch
        t, angles, centre = match_arguments(1, 20.0, 2.0)
        b = gridmatch.GridSearchBatch(build_small_room(inp["clouds"]), batch.CloudSet.from_numpy(inp["clouds"]), [0, 1, 2], t, angles, 20,
                                      centre, block=8, want_bounds=True)
        calm(b.ws)
        return b

    run = staticmethod(run_batch)

    @staticmethod
    def outputs(b):
        return [b.records, b.bounds_volume, b._field_buf, b._bound_buf]


def room_field(inp):
    """(grid, its int16 field, k, the threshold of an occupied cell) of the small room, synchronised."""
    import torch
    g = build_small_room(inp["clouds"])
    field, k = g.score_field()
    torch.cuda.synchronize()
    return g, field, k, int(np.rint(0.5 * 2.0 ** k))


@workload("grid_likelihood_field", ("icpmi_grid_likelihood_field",))
class _GridLikelihood:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, gridmatch
        g, field, k, thr = room_field(inp)
        ws = torch.zeros(_lib.lib().icpmi_grid_likelihood_workspace_bytes(64, 64, 3), dtype=torch.uint8, device=field.device)
        return types.SimpleNamespace(field=field, thr=thr, table=gridmatch.likelihood_table(2.0 ** k, 1.0, 3), ws=ws,
                                     lf=torch.zeros_like(field), d2=torch.zeros_like(field), alone=torch.zeros_like(field))

    @staticmethod
    def run(o):
        from icpmi import gridmatch
        gridmatch.likelihood_field(o.field, o.thr, 3, o.table, True, out=o.lf, d2_out=o.d2, workspace=o.ws)
        gridmatch.distance_field(o.field, o.thr, 3, out=o.alone)

    @staticmethod
    def outputs(o):
        return [o.lf, o.d2, o.alone]


@workload("grid_occupancy_planes", ("icpmi_grid_occupancy_planes",))
class _GridPlanes:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        g, field, k, thr = room_field(inp)
        return types.SimpleNamespace(field=field, thr=thr, planes=None)

    @staticmethod
    def run(o):
        from icpmi import gridmatch
        o.planes = gridmatch.occupancy_planes(o.field, o.thr)

    @staticmethod
    def outputs(o):
        return [o.planes.buf]


def pair_poses(seed, n):
    """n poses near the true ones of the small room -> (clouds named, translations (n, 2), cos / sin (n, 2))."""
    rng = np.random.default_rng(920 + seed)
    which = np.arange(n) % 3
    truth = np.array(SMALL_ROOM_POSES)[which]
    th = truth[:, 2] + np.deg2rad(rng.uniform(-3.0, 3.0, size=n))
    return which.astype(np.int32), truth[:, :2] + rng.uniform(-0.1, 0.1, size=(n, 2)), np.stack([np.cos(th), np.sin(th)], axis=1)


@workload("grid_cast", ("icpmi_grid_cast_segments", "icpmi_grid_cast_rays"))
class _GridCast:
    """``cast_segments`` over the field (packed into a workspace by the entry) and ``cast_rays`` over kept planes."""
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, gridmatch
        g, field, k, thr = room_field(inp)
        planes = gridmatch.occupancy_planes(field, thr)
        rng = np.random.default_rng(921)
        segs = rng.integers(-4, 68, size=(65, 4)).astype(np.int32)
        _, xy, cs = pair_poses(1, 5)
        beams = np.linspace(-np.pi, np.pi, 33, endpoint=False)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=field.device)             # noqa: E731
        torch.cuda.synchronize()
        return types.SimpleNamespace(field=field, thr=thr, planes=planes, grid=g, segs=_dev(segs), xy=_dev(xy), pcs=_dev(cs),
                                     bcs=_dev(np.stack([np.cos(beams), np.sin(beams)], axis=1)), seg_out=i32(65, _lib.GC_INTS),
                                     ray_out=i32(5, 33, _lib.GC_INTS))

    @staticmethod
    def run(o):
        from icpmi import gridmatch
        g = o.grid
        gridmatch.cast_segments(o.field, o.thr, o.segs, out=o.seg_out)
        gridmatch.cast_rays(o.planes, o.thr, g.min_x, g.min_y, g.resolution, o.xy, o.pcs, o.bcs, 4.0, out=o.ray_out)

    @staticmethod
    def outputs(o):
        return [o.seg_out, o.ray_out]


def build_map_pairs(inp, kept):
    import torch
    from icpmi import batch, gridmatch
    g, field, k, thr = room_field(inp)
    src = gridmatch.occupancy_planes(field, thr) if kept else field
    which, xy, cs = pair_poses(2, 7)
    mp = gridmatch.MapPairs(src, thr, g.min_x, g.min_y, g.resolution, batch.CloudSet.from_numpy(inp["clouds"]), which, _dev(xy), _dev(cs))
    torch.cuda.synchronize()
    return mp


@workload("grid_check", ("icpmi_grid_check_batch",))
class _GridCheck:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib
        mp = build_map_pairs(inp, kept=False)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=mp.dev)                   # noqa: E731
        return types.SimpleNamespace(mp=mp, out=(i32(mp.B, _lib.GK_INTS), i32(mp.B, mp.stride, _lib.GK_ROW_INTS)))

    @staticmethod
    def run(o):
        o.mp.check(2, want_rows=True, out=o.out)

    @staticmethod
    def outputs(o):
        return list(o.out)


BEAM_H = 4


@workload("grid_beam", ("icpmi_grid_beam_batch",))
class _GridBeam:
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, gridmatch
        mp = build_map_pairs(inp, kept=True)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=mp.dev)                   # noqa: E731
        return types.SimpleNamespace(mp=mp, table=_dev(gridmatch.beam_table(0.1, 0.1, BEAM_H)),
                                     out=(i32(mp.B, _lib.GB_INTS), i32(mp.B, 2 * BEAM_H + 3), i32(mp.B, mp.stride, _lib.GB_ROW_INTS)))

    @staticmethod
    def run(o):
        o.mp.beam(o.table, BEAM_H, 0.9, want_hist=True, want_rows=True, out=o.out)

    @staticmethod
    def outputs(o):
        return list(o.out)


PARTICLES = 257                      # one above a block of 256 weights


@workload("particle_round", ("icpmi_pf_predict", "icpmi_grid_beam_batch", "icpmi_pf_weights", "icpmi_pf_resample", "icpmi_pf_estimate"))
class _ParticleRound:
    """One round of the filter without its read-backs: the particles put back where they started (device copies), then
    predict, the beam model and the weights, resample, the estimate's sums."""
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import ParticleFilter, batch
        g = build_small_room(inp["clouds"])
        pf = ParticleFilter(g, PARTICLES, seed=0x51CA5E5, half_width=BEAM_H)
        rng = np.random.default_rng(930)
        p = np.array(SMALL_ROOM_POSES[0]) + rng.normal(0.0, 1.0, size=(PARTICLES, 3)) * np.array([0.1, 0.1, 0.03])
        pf.set_poses(p)
        cs = batch.CloudSet.from_numpy([inp["clouds"][0][::2]])
        pf.scan_pairs(cs, 0)                                      # the pair list is uploaded here, once
        start = [t.clone() for t in pf._state]
        calm(pf._ws)
        torch.cuda.synchronize()
        return types.SimpleNamespace(pf=pf, cs=cs, start=start)

    @staticmethod
    def run(o):
        pf = o.pf
        for dst, src in zip(pf._state, o.start):
            dst.copy_(src)
        pf.w.fill_(1)
        pf.step = 0
        pf.predict((0.05, 0.0, 0.01), (0.05, 0.05, 0.02))
        pf.enqueue_weights(pf.scan_pairs(o.cs, 0))
        pf.resample()
        pf.enqueue_estimate()

    @staticmethod
    def outputs(o):
        pf = o.pf
        return [pf.pair_t, pf.theta, pf.cos_sin, pf.records, pf.sums, pf.ancestors, pf.info, pf.moments, pf.w]


class _GridUpdate:
    """``OccupancyGrid2D.update_scan`` of a NumPy scan — its pinned staging copy and ``icpmi_grid_update_scans_box`` on the
    stream ``mapping.py`` reads through ``torch._C._cuda_getCurrentRawStream`` — on a grid that ``run`` zeroes first; and the
    entry's two other forms, ``icpmi_grid_update_scans`` and ``icpmi_grid_update_scans_band``, called as ``_apply`` calls the
    first, each on a grid of its own."""
    inputs = staticmethod(room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import _lib, synth
        from utilities.mapping import OccupancyGrid2D
        pose = SMALL_ROOM_POSES[1]
        world = synth.to_world(inp["clouds"][1], pose)
        g = OccupancyGrid2D(**SMALL_ROOM)
        ws = lambda: torch.zeros(_lib.lib().icpmi_grid_workspace_bytes(64, 64), dtype=torch.uint8, device="cuda")       # noqa: E731
        o = types.SimpleNamespace(grid=g, origin=np.array(pose[:2]), world=world, org=_dev(np.array([pose[:2]])), hits=_dev(world),
                                  off=np.array([0, len(world)], dtype=np.int32), plain=torch.zeros_like(g._grid), plain_ws=ws(),
                                  band=torch.zeros_like(g._grid), band_ws=ws())
        torch.cuda.synchronize()
        return o

    @staticmethod
    def run(o):
        from icpmi import _lib
        from icpmi.batch import _ptr, _stream
        g, L = o.grid, _lib.lib()
        g.reset()
        g._seq = 0
        g.update_scan(o.origin, o.world)
        head = (64, 64, g.min_x, g.min_y, g.resolution, _ptr(o.org), _ptr(o.hits), o.off.ctypes.data_as(C.c_void_p), 1, float(g.l_hit),
                float(g.l_miss), g.log_odds_min, g.log_odds_max, 0, 0)
        o.plain.zero_()
        _lib.check(L.icpmi_grid_update_scans(_ptr(o.plain), _ptr(o.plain_ws), *head, _stream()), "grid_update_scans")
        o.band.zero_()
        _lib.check(L.icpmi_grid_update_scans_band(_ptr(o.band), _ptr(o.band_ws), *head, 8, 56, _stream()), "grid_update_scans_band")

    @staticmethod
    def outputs(o):
        return [o.grid._grid, o.plain, o.band]


for _pass in ("tiles", "atomic", "owner"):
    workload(f"grid_update_{_pass}", ("icpmi_grid_update_scans_box", "icpmi_grid_update_scans", "icpmi_grid_update_scans_band"),
             options={"ICPMI_RAYCAST": _pass})(_GridUpdate)


# ── entries behind wrappers that upload and read back in one call ────────────
@workload("helper_entries", ("icpmi_p2l_solve_2d", "icpmi_rotation_scores", "icpmi_world_to_grid", "icpmi_bresenham_cells",
                             "icpmi_pose_graph_error"))
class _HelperEntries:
    """Five entries whose Python wrappers (utilities.icp._point_to_line_solve_2d, utilities.features.rotation_scores,
    OccupancyGrid2D._world_to_grid_batch, utilities.mapping.bresenham_cells, PoseGraph2D.total_error) upload, launch and read
    back in one call: here each entry is called as its wrapper calls it, on buffers uploaded when the object is built."""

    @staticmethod
    def inputs(seed):
        from icpmi import synth
        rng = np.random.default_rng(940 + seed)
        src, tgt = synth.scan(BASE, 941 + seed, n_beams=300), synth.scan((0.55, -0.25, 0.12), 942 + seed, n_beams=257)
        nrm = rng.normal(size=(257, 2))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        seg = rng.integers(-40, 40, size=(33, 4))
        nodes = rng.uniform(-2.0, 2.0, size=(9, 3))
        ij = np.stack([np.arange(8), np.arange(1, 9)], axis=1)
        om = rng.uniform(0.5, 2.0, size=(8, 1, 1)) * np.eye(3)
        return {"src": src, "tgt": tgt, "nrm": nrm, "idx": rng.integers(0, 257, size=300), "angles": np.deg2rad(np.arange(-30.0, 30.0, 0.5)),
                "seg": seg, "world": rng.uniform(-5.0, 5.0, size=1000), "nodes": nodes, "ij": ij, "z": rng.normal(size=(8, 3)), "om": om}

    @staticmethod
    def build(inp):
        import torch
        seg = inp["seg"].astype(np.int64)
        n = np.maximum(np.abs(seg[:, 2] - seg[:, 0]), np.abs(seg[:, 3] - seg[:, 1]))
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        a = inp["angles"]
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")                  # noqa: E731
        o = types.SimpleNamespace(
            src=_dev(inp["src"]), tgt=_dev(inp["tgt"]), nrm=_dev(inp["nrm"]), idx=_dev(inp["idx"].astype(np.int32)), solve=f64(6),
            cs=_dev(np.stack([np.cos(a), np.sin(a)], axis=1)), n_angles=len(a), scores=f64(len(a)),
            world=_dev(inp["world"]), cells=torch.zeros(1000, dtype=torch.int64, device="cuda"),
            seg=_dev(seg.astype(np.int32)), seg_off=_dev(off), n_seg=len(seg), seg_cells=torch.zeros((int(off[-1]), 2), dtype=torch.int32, device="cuda"),
            nodes=_dev(inp["nodes"]), ei=_dev(inp["ij"][:, 0].astype(np.int32)), ej=_dev(inp["ij"][:, 1].astype(np.int32)), z=_dev(inp["z"]),
            om=_dev(inp["om"]), scratch=f64(9))
        torch.cuda.synchronize()
        return o

    @staticmethod
    def run(o):
        from icpmi import _lib
        from icpmi.batch import _ptr as P, _stream
        L, st = _lib.lib(), _stream()
        _lib.check(L.icpmi_p2l_solve_2d(P(o.src), len(o.src), P(o.tgt), P(o.nrm), P(o.idx), P(o.solve), st), "p2l_solve_2d")
        _lib.check(L.icpmi_rotation_scores(P(o.src), len(o.src), P(o.tgt), len(o.tgt), P(o.cs), o.n_angles, 0.05, -0.02, P(o.scores), st),
                   "rotation_scores")
        _lib.check(L.icpmi_world_to_grid(P(o.world), o.world.numel(), -5.0, 0.05, P(o.cells), st), "world_to_grid")
        _lib.check(L.icpmi_bresenham_cells(P(o.seg), P(o.seg_off), o.n_seg, P(o.seg_cells), st), "bresenham_cells")
        _lib.check(L.icpmi_pose_graph_error(P(o.nodes), P(o.ei), P(o.ej), P(o.z), P(o.om), 8, P(o.scratch), P(o.scratch[8:]), st),
                   "pose_graph_error")

    @staticmethod
    def outputs(o):
        return [o.solve, o.scores, o.cells, o.seg_cells, o.scratch]


@workload("feature_stages", ("icpmi_feature_curvature_batch", "icpmi_feature_keypoints_batch", "icpmi_feature_descriptors_batch",
                             "icpmi_feature_match_batch", "icpmi_feature_ransac_batch"))
class _FeatureStages:
    """The five stage entries behind utilities.features' one-call functions, chained on one pair of clouds as
    tests/test_features_gpu.py chains them."""

    @staticmethod
    def inputs(seed):
        inp = candidate_inputs(1, 950000 + 100 * seed, 4)
        inp["hyp_u"] = np.random.default_rng(951 + seed).random((200, 2))
        return inp

    @staticmethod
    def build(inp):
        import torch
        from icpmi import batch
        from icpmi.prealign import FEAT_DEFAULTS
        cs = batch.CloudSet.from_numpy(inp["clouds"])
        S = (FEAT_DEFAULTS["top_n"] + 7) // 8 * 8
        z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=cs.pts.device)                # noqa: E731
        o = types.SimpleNamespace(cs=cs, S=S, curv=z(torch.float64, cs.total_rows), kp=z(torch.int32, 2, S), kpc=z(torch.int32, 2),
                                  desc=z(torch.float64, 2, S, 32), dl=z(torch.int32, 2), m=z(torch.int32, S, 2), mc=z(torch.int32, 1),
                                  out=z(torch.float64, 1, 16), ps=_dev(np.array([0], dtype=np.int32)), pt=_dev(np.array([1], dtype=np.int32)),
                                  hu=_dev(inp["hyp_u"]))
        torch.cuda.synchronize()
        return o

    @staticmethod
    def run(o):
        from icpmi import _lib
        from icpmi.batch import _ptr as P, _stream
        from icpmi.prealign import FEAT_DEFAULTS as cfg
        L, st, cs, S = _lib.lib(), _stream(), o.cs, o.S
        _lib.check(L.icpmi_feature_curvature_batch(P(cs.pts), P(cs.off), None, None, 2, cfg["k_curvature"], P(o.curv), st), "curvature")
        _lib.check(L.icpmi_feature_keypoints_batch(P(cs.pts), P(cs.off), None, None, 2, P(o.curv), None, cfg["top_n"], cfg["min_kp_dist"],
                                                   P(o.kp), P(o.kpc), S, st), "keypoints")
        _lib.check(L.icpmi_feature_descriptors_batch(P(cs.pts), P(cs.off), None, None, 2, P(o.kp), P(o.kpc), S, cfg["k_descriptor"], P(o.desc),
                                                     P(o.dl), st), "descriptors")
        _lib.check(L.icpmi_feature_match_batch(P(o.desc), P(o.dl), P(o.kpc), S, P(o.ps), P(o.pt), 1, cfg["ratio_threshold"] ** 2, P(o.m),
                                               P(o.mc), st), "match")
        _lib.check(L.icpmi_feature_ransac_batch(P(cs.pts), P(cs.off), None, P(o.kp), P(o.kpc), S, P(o.ps), P(o.pt), 1, P(o.m), P(o.mc), None,
                                                P(o.hu), o.hu.shape[0], 0, cfg["inlier_threshold"], P(o.out), None, st), "ransac")

    @staticmethod
    def outputs(o):
        return [o.curv, o.kp, o.kpc, o.desc, o.dl, o.mc, o.out]


# ── part B: the pose-graph calls ─────────────────────────────────────────────
POSE_GRAPH_CASES = {"optimize": "cr_n33_fix0", "robust": "multi_n33_healthy", "marginals": "cr_n9_fix4"}


def pose_graph_call(kind):
    """One pose-graph call on the current stream (it synchronises that stream by contract), on a chain case of
    tests/pose_graph_ref.py -> the host arrays of its result.  The info records hold clock readings and are left out."""
    import pose_graph_ref
    from utilities import pose_graph
    case = pose_graph_ref.cases()[POSE_GRAPH_CASES[kind]]
    g = case["graph"]
    pg = pose_graph.PoseGraph2D()
    for v in g["nodes"]:
        pg.add_node(v)
    for i, j, z, om in zip(g["ei"], g["ej"], g["z"], g["omega"]):
        pg.add_edge(int(i), int(j), z, om)
    if kind == "optimize":
        pg.optimize(n_iterations=5, fix_node=case["fix"])
        return [np.array(pg.nodes)]
    if kind == "robust":
        pg.optimize_robust(n_iterations=5, fix_node=case["fix"], kernel="huber")
        return [np.array(pg.nodes), pg.last_robust["chi2"], pg.last_robust["weights"]]
    m = pg.marginals(nodes=[0, 3, -1], fix_node=case["fix"])
    return [m.diagonal, m.columns]


# ── the inventory ────────────────────────────────────────────────────────────
def reached_entries():
    """entry -> the names of the workloads that reach it."""
    out = collections.OrderedDict()
    for w in WORKLOADS.values():
        for e in w.entries:
            out.setdefault(e, []).append(w.name)
    return out


def reached_classes():
    out = collections.OrderedDict()
    for w in WORKLOADS.values():
        for c in w.classes:
            out.setdefault(c, []).append(w.name)
    return out


def inventory_text():
    from icpmi import _lib
    reached, lines = reached_entries(), ["", "Inventory of include/icpmi.h:", ""]
    for name in _lib.EXPORTS:
        what = ", ".join(reached[name]) if name in reached else "left out — " + EXCLUDED_ENTRIES.get(name, "NOT ACCOUNTED FOR")
        lines.append(f"- {name}: {what}")
    lines += ["", "Classes of icpmi/ with a run method:", ""]
    for name, ws in reached_classes().items():
        lines.append(f"- {name}: {', '.join(ws)}")
    for name, why in EXCLUDED_CLASSES.items():
        lines.append(f"- {name}: left out — {why}")
    return "\n".join(lines) + "\n"


__doc__ += inventory_text()
