"""CPU-side checks: the C-ABI library builds, loads and exports every symbol the
header declares; the product path refuses to run without a GPU (no CPU
fallback); the multi-rank sharding/gather logic works under gloo with
world_size 2 (the oracle is injected as the local solver — test only)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "icpmi.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(icpmi_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_header_symbols():
    import ctypes
    import icpmi
    path = icpmi.build()
    lib = icpmi.lib()                     # torch first, then the library: ONE HIP runtime in the process (icpmi_runtime_check)
    L = ctypes.CDLL(path)                 # the same mapping, seen through a plain handle
    syms = declared_symbols()
    assert len(syms) >= 14
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/icpmi.h but not exported"
    # and the Python binding knows every one of them
    from icpmi import _lib
    assert sorted(_lib.EXPORTS) == syms
    assert _lib.runtime_problem() == ""
    assert lib.icpmi_version().decode().startswith("icpmi")
    assert lib.icpmi_strerror(-2).decode() == "workspace missing or too small"
    # host-only size queries (no GPU touched)
    assert lib.icpmi_grid_workspace_bytes(10, 20) == 4 * 10 * 20 * 4 + 256 + 2 * 32 * 17 * 16   # four grids of counters (was 32) + box slots + per-scan cell boxes
    assert lib.icpmi_icp_workspace_bytes(2, 100, 2) == 2 * 100 * (16 + 8 + 4) + 256
    assert lib.icpmi_voxel_workspace_bytes(2048) == 256
    assert lib.icpmi_voxel_workspace_bytes(100000) > 100000 * 24
    # every size query against literal values: a layout is described once (a struct that walks icpmi::Carve) and its size
    # must not move when the description is edited — callers, utilities/features.py among them, index into these buffers
    import torch
    on_gpu = torch.cuda.is_available()
    for name, table in SIZE_TABLE.items():
        for args, want in table:
            if isinstance(want, tuple):
                want = want[1 if on_gpu else 0]
            assert getattr(lib, name)(*args) == want, (name, args)
    # The pose-graph workspace (PgWs in csrc/posegraph.hip), by hand.  a(x) = x rounded up to 256 bytes; n nodes, m edges
    # (with the twins), k non-chain edges, w twins:
    #   a(8m) + a(4(n+1)) + a(4(2m+1)) + a(4(m+1)) + a(4(k+1))       ei/ej, csr_ptr, csr_edge, loop_slot, loop_edge
    #   + 5 a(72n) + a(24n(1+3k)) + a(144(k+1)) + a(8(9k^2+1)) + a(8(3k+1)) + a(24n)     D U L Dinv G, X, AB, M, g, dx
    #   + [dense: a(72n^2)] + [w > 0: a(72m) + a(24m)] + 256
    # n = 50, m = 49, k = 0: 512 + 256 + 512 + 256 + 256 + 19200 + 1280 + 256 + 256 + 256 + 1280 + 256 = 24576
    # n = 50, m = 52, k = 3: 512 + 256 + 512 + 256 + 256 + 19200 + 12032 + 768 + 768 + 256 + 1280 + 256 = 36352
    # n = 50, m = 49, k = 0, dense: 24576 + a(180000) = 24576 + 180224 = 204800
    # n = 5, m = 0 (no chain either: dense, and a(0) = 0 for ei/ej): 9 x 256 + 5 x 512 + a(1800) + 256 = 7168
    # (Three arrays no kernel used — a(72n) + a(8(3k+1)) + a(8(m+1)), 4608 bytes for the 50-node graphs and 1024 for
    # n = 5 — were part of the layout before: 29184, 40960, 209408, 8192.)
    chain = [(i, i + 1) for i in range(49)]
    closures = [(0, 49), (10, 30), (5, 45)]
    for edges, n, want in ((chain, 50, 24576),                                              # sparse plan, no loop edge
                           (chain + closures, 50, 36352),                                   # sparse plan, k = 3
                           ([e for e in chain if e[0] != 20] + [(0, 49)], 50, 204800),      # a gap in the chain: dense plan
                           ([(0, 7)], 5, 0), ([], 5, 7168), ([], -1, 0)):
        ij = np.ascontiguousarray(np.array(edges, dtype=np.int32).reshape(-1, 2))
        assert lib.icpmi_pose_graph_workspace_bytes(ij.ctypes.data if len(edges) else None, n, len(edges)) == want, (edges, n)
    assert lib.icpmi_pose_graph_workspace_bytes(None, 5, 3) == 0
    # With the information matrices (S = 1e4, a chain edge is weak below S / (3n) = 66.7).  One weak chain edge gets a twin
    # among the closures: m = 53, k = 4, w = 1, the plain size of a graph with one more closure and one more edge row
    # (512 + 256 + 512 + 256 + 256 + 19200 + 15616 + 768 + 1280 + 256 + 1280 + 256 = 40448) plus the two twin arrays
    # (a(72 x 53) + a(24 x 53) = 3840 + 1280): 45568.  A chain edge of all zeros is a null edge: no twins, the plain 36352.
    ij = np.ascontiguousarray(np.array(chain + closures, dtype=np.int32))
    for weak, want in ((np.diag([1e-8, 1e4, 1e4]), 45568), (np.zeros((3, 3)), 36352), (None, 36352)):
        om = np.ascontiguousarray(np.tile(1e4 * np.eye(3), (len(ij), 1, 1)))
        if weak is not None:
            om[20] = weak
        assert lib.icpmi_pose_graph_weighted_workspace_bytes(ij.ctypes.data, om.ctypes.data, 50, len(ij)) == want, weak


# (arguments, bytes) of the host-only size queries; zero-sized inputs keep their fixed parts; negative ones give 0 where the
# query checks them.  A pair of values: the layout holds rocprim's temporary storage (clouds above 8192 rows in the voxel
# filter, above 4096 in the prepare path), whose size rocprim picks for the device it finds — (without a GPU, on gfx950).
SIZE_TABLE = {
    "icpmi_voxel_workspace_bytes": [((0,), 256), ((-1,), 256), ((2048,), 256), ((2049,), 256), ((4096,), 256), ((8192,), 256),
                                    ((8193,), (264192, 362752)), ((100000,), (3201024, 4401152))],
    "icpmi_prepared_bytes": [((0, 0, 0), 256), ((-1, 1, 1), 0), ((1, -1, 1), 0), ((1, 1, -1), 0), ((100, 1, 0), 4352),
                             ((1000, 3, 500), 40448), ((8192, 2, 4096), 328192), ((8193, 2, 4097), (427776, 477184)),
                             ((12000, 3, 10000), (721408, 841472))],
    "icpmi_icp_workspace_bytes": [((2, 100, 2), 5856), ((2, 100, 3), 7456), ((7, 333, 3), 84172), ((16384, 1400, 2), 642253056),
                                  ((0, 0, 2), 256), ((0, 100, 3), 256), ((-1, 100, 2), 0), ((2, -1, 2), 0), ((2, 100, 4), 0),
                                  ((2, 100, 1), 0)],
    "icpmi_normals_workspace_bytes": [((1000, 8192), 256), ((0, 0), 256), ((0, 9000), 512), ((20000, 8193), 480512),
                                      ((100000, 20000), 2400512)],
    "icpmi_rotation_search_workspace_bytes": [((1400, 1500, 72, 40), 48128), ((10000, 9000, 360, 64), (629504, 749568)), ((1, 1, 1, 0), 1024),
                                              ((0, 0, 0, 0), 1024), ((-1, 10, 10, 10), 0), ((10, -1, 10, 10), 0),
                                              ((10, 10, -1, 10), 0), ((10, 10, 10, -1), 0)],
    "icpmi_rotation_search_batch_workspace_bytes": [((20000, 16, 2048), 1121536), ((4096, 1, 4096), 230912), ((333, 7, 100), 20224),
                                                    ((0, 0, 0), 768), ((-1, 1, 1), 0), ((1, -1, 1), 0), ((1, 1, -1), 0)],
    "icpmi_rotation_refine_workspace_bytes": [((1,), 1024), ((1400,), 39680), ((4096,), 114944), ((0,), 256), ((-1,), 0)],
    "icpmi_grid_workspace_bytes": [((10, 20), 20864), ((480, 320), 2475264), ((4000, 4000), 256017664), ((0, 10), 0), ((10, 0), 0),
                                   ((-1, 10), 0), ((10, -5), 0)],
}


def test_record_layouts_are_named_once_in_the_header():
    """include/icpmi.h names the slots, statuses and capacities of the rotation-search and feature records and of the
    pose graph's info record; icpmi._lib mirrors every one of them (ICPMI_<NAME> -> _lib.<NAME>) and the names prealign /
    utilities.features / utilities.pose_graph exported before are aliases of them."""
    from icpmi import _lib, prealign
    from utilities import features, pose_graph
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    families = ("RSREC_", "RS_WS_", "RSR_", "RSBREC_", "RSB_", "FTREC_", "FT_", "PG_", "PGINFO_")
    named = {n for n in defines if n.startswith(families)}
    # search: 10 + 4 slots, 4 statuses, 2 offsets, 3 capacities; features: 11 slots, 6 statuses, 3 capacities;
    # pose graph: 5 statuses, the record's length, 4 slots, the number of phase clocks
    assert len(named) == 43 + 11
    for n in named:
        assert getattr(_lib, n) == defines[n], n
    pg = ("NOTHING", "CONVERGED", "MAXITER", "SINGULAR", "REFUSED")
    assert [defines["PG_ST_" + n] for n in pg] == list(range(5))
    assert (pose_graph.NOTHING_TO_DO, pose_graph.CONVERGED, pose_graph.MAX_ITERATIONS, pose_graph.SINGULAR) == (0, 1, 2, 3)
    assert [defines["PGINFO_" + n] for n in ("ITERATIONS", "STATUS", "STEP", "PHASE_US", "PHASES", "DOUBLES")] == [0, 1, 2, 3, 7, 10]
    assert len(pose_graph.PHASE_KEYS) == defines["PGINFO_PHASES"] == defines["PGINFO_DOUBLES"] - defines["PGINFO_PHASE_US"]
    for n, v in defines.items():                              # and whatever else the binding mirrors (RES_*, ST_*, ERR_*) agrees
        assert getattr(_lib, n, v) == v, n
    assert _lib.RES_DOUBLES == defines["RES_DOUBLES"] and _lib.ERR_HIP == defines["ERR_HIP"] == -3
    assert [defines[n] for n in ("RSBREC_STATUS", "RSBREC_DOUBLES", "FTREC_STATUS", "FTREC_DOUBLES", "RSREC_DOUBLES")] == [11, 16, 12, 16, 12]
    assert (prealign.ST_OK, prealign.ST_FEW, prealign.ST_CAPACITY, prealign.ST_NO_FINE) == tuple(
        defines[n] for n in ("RSB_ST_OK", "RSB_ST_FEW", "RSB_ST_CAPACITY", "RSB_ST_NO_FINE")) == (0, 1, 2, 3)
    assert prealign.REC_DOUBLES == defines["RSBREC_DOUBLES"] == defines["FTREC_DOUBLES"]
    assert prealign.RSB_MAX_ANGLES == defines["RSB_MAX_ANGLES"] == 1024
    feat = ("OK", "FEW_ROWS", "CAPACITY", "FEW_KP", "FEW_MATCHES", "DESC_LEN")
    assert [getattr(prealign, "FEAT_ST_" + n) for n in feat] == [defines["FT_ST_" + n] for n in feat] == list(range(6))
    assert (features.FEAT_MAX_ROWS, features.FEAT_MAX_KP, features.FEAT_DESC_STRIDE) == (
        defines["FT_MAX_ROWS"], defines["FT_MAX_KP"], defines["FT_DESC_STRIDE"]) == (2048, 256, 32)


def test_winning_angle_of_a_search_record():
    """icpmi.prealign.winning_angle: the fine angle a record names, for one record and for a batch of them; a winner
    without a fine grid raises as np.argmin does (features.py:231) or, for the submap search, falls back to the coarse
    angle (slam.py:157-159)."""
    from icpmi import _lib
    from icpmi.prealign import winning_angle
    coarse = np.array([0.1, 0.2, 0.3])
    fine = np.arange(12.0).reshape(3, 4)
    rec = np.zeros((3, _lib.RSBREC_DOUBLES))
    rec[:, _lib.RSREC_K], rec[:, _lib.RSREC_NF], rec[:, _lib.RSREC_J] = (2, 0, 1), (4, 3, 0), (3, 1, 0)
    assert np.array_equal(winning_angle(coarse, fine, rec[:2]), [11.0, 1.0])
    assert winning_angle(coarse, fine, rec[0]) == 11.0 and winning_angle(coarse, fine, rec[0], coarse_without_fine=True) == 11.0
    with pytest.raises(ValueError, match="argmin of an empty sequence"):
        winning_angle(coarse, fine, rec[2])
    assert winning_angle(coarse, fine, rec[2], coarse_without_fine=True) == 0.2
    assert winning_angle(coarse, np.zeros((3, 0)), rec[2], coarse_without_fine=True) == 0.2
    assert np.array_equal(winning_angle(coarse, fine, rec, coarse_without_fine=True), [11.0, 1.0, 0.2])


def test_two_hip_runtimes_in_one_process_are_named():
    """libicpmi.so loaded BEFORE torch maps /opt/rocm's libamdhip64 and torch then maps its own — every
    launch would fail with a bare ICPMI_ERR_HIP.  icpmi_runtime_check names the two copies; the Python loader raises with
    that message instead of handing out a library that cannot launch."""
    code = (f"import ctypes, sys; sys.path.insert(0, {PKG!r}); L = ctypes.CDLL({os.path.join(PKG, 'lib', 'libicpmi.so')!r});"
            "buf = ctypes.create_string_buffer(1024); L.icpmi_runtime_check.argtypes = [ctypes.c_char_p, ctypes.c_size_t];"
            "assert L.icpmi_runtime_check(buf, 1024) == 0, buf.value;"          # the library alone: one runtime
            "import torch;"
            "rc = L.icpmi_runtime_check(buf, 1024); print('RC', rc, buf.value.decode());"
            "from icpmi import _lib\n"
            "try:\n    _lib.lib(); print('LOADED')\nexcept _lib.IcpmiError as e:\n    print('RAISED', e)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if "RC 0" in r.stdout:                # torch resolved to the runtime already mapped (same SONAME): nothing to diagnose
        assert "LOADED" in r.stdout
    else:
        assert "RC -3 two HIP runtimes in one process" in r.stdout and "RAISED two HIP runtimes" in r.stdout, r.stdout


def test_struct_layout_matches_header():
    import ctypes
    from icpmi._lib import IcpParams
    assert ctypes.sizeof(IcpParams) == 32
    assert IcpParams.max_iterations.offset == 16 and IcpParams.dim.offset == 28


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from icpmi import IcpmiError
    from utilities import icp as uicp
    from utilities.mapping import OccupancyGrid2D
    pts = np.random.default_rng(0).normal(size=(100, 2))
    with pytest.raises(IcpmiError):
        uicp.ICP(pts, pts, 1e-6, 10, 0.1)
    with pytest.raises(IcpmiError):
        uicp.voxel_downsample(pts, 0.1)
    with pytest.raises(IcpmiError):
        OccupancyGrid2D(-1, 1, -1, 1)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package or bench's GPU legs may import it."""
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(import oracle|from oracle)", src, flags=re.M), f
                assert "liboracle" not in src, f


def test_shard_and_gather_single_process():
    import torch
    from icpmi import dist as idist
    assert list(idist.shard(10, 1, 4)) == [1, 5, 9]
    assert idist.slots_per_rank(10, 4) == 3
    loc = torch.arange(5 * 16, dtype=torch.float64).reshape(5, 16)
    out = idist.gather_results(loc, 5, 0, 1)
    assert torch.equal(out, loc)
    res = torch.zeros((4, 16), dtype=torch.float64)
    res[:, 12] = torch.tensor([0.5, 0.2, 0.01, 0.001])
    assert idist.first_accepted(res, 0.05) == 2 and idist.first_accepted(res, 1e-6) == -1


WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, {pkg!r})
import oracle
from icpmi import dist as idist, synth, _lib

def solver(src, tgt, Ri, ti):
    out = np.zeros((len(tgt), _lib.RES_DOUBLES))
    for i, (s, t) in enumerate(zip(src, tgt)):
        R, tt, err, info = oracle.icp(s, t, 1e-10, 60, 0.1, method="point_to_line", normal_k=8)
        out[i, :4] = R.ravel(); out[i, 9:11] = tt; out[i, 12] = err
        out[i, 14] = info["iters"]; out[i, 15] = info["status"]
    return torch.from_numpy(out)

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
srcs, tgts = synth.loop_closure_batch(5, seed0=77)
srcs = [s[::4] for s in srcs]; tgts = [t[::4] for t in tgts]
res = idist.icp_batch_sharded(srcs, tgts, 1e-10, 60, 0.1, method="point_to_line", normal_k=8, solver=solver)
full = solver(srcs, tgts, None, None)            # every pair locally, in order
assert res.shape == (5, _lib.RES_DOUBLES)
assert torch.equal(res, full), (rank, (res - full).abs().max())
shared = idist.icp_batch_sharded(srcs[0], tgts, 1e-10, 60, 0.1, solver=solver)
assert torch.equal(shared, solver([srcs[0]] * 5, tgts, None, None))
dist.barrier()
if rank == 0:
    print("GLOO_OK", world)
dist.destroy_process_group()
'''


def test_sharded_batch_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(repo=REPO, pkg=PKG))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29713", str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GLOO_OK 2" in r.stdout


RUN_ICP_PAIR_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, {pkg!r})
import oracle
from icpmi import dist as idist, synth, _lib

ICP = dict(error_threshold=1e-10, max_iterations=40, voxel_size=0.1, method="point_to_line", normal_k=8)
FEAT = dict(rotation_voxel_size=0.3, angle_step_coarse=6.0, angle_step_fine=1.0)

def solver(src, tgts):          # slam.py:53-98 with the oracle: rotation search, then ICP from its result
    out = np.zeros((len(tgts), _lib.RES_DOUBLES))
    for i, t in enumerate(tgts):
        R0, t0, _ = oracle.rotation_search(src, t, FEAT["rotation_voxel_size"], FEAT["angle_step_coarse"], FEAT["angle_step_fine"])
        R, tt, err, info = oracle.icp(src, t, 1e-10, 40, 0.1, R_init=R0, t_init=t0, method="point_to_line", normal_k=8)
        out[i, :4] = R.ravel(); out[i, 9:11] = tt; out[i, 12] = err
        out[i, 13] = info["delta"]; out[i, 14] = info["iters"]; out[i, 15] = info["status"]
    return torch.from_numpy(out)

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
srcs, tgts = synth.loop_closure_batch(7, seed0=311, shared_source=True, max_offset=2.0, max_yaw_deg=15.0)
src = srcs[0][::4]; tgts = [t[::4] for t in tgts]
job = idist.RunIcpPairSharded(src, tgts, ICP, FEAT, solver=solver)
assert list(job.mine) == list(range(rank, 7, world))
res = job.run()
full = solver(src, tgts)                                   # every candidate locally, in candidate order
assert res.shape == (7, _lib.RES_DOUBLES) and torch.equal(res, full), rank
err = full[:, 12].numpy()
gate = float(np.sort(err)[2]) * 1.0000001                  # three candidates pass: the FIRST in candidate order wins
want = int(np.flatnonzero(err < gate)[0])
assert job.first_accepted(gate) == want and job.first_accepted(0.0) == -1
R, t, e, info = idist.run_icp_pair_batch_sharded(src, tgts, ICP, FEAT, error_accept=gate, solver=solver)
assert info["first_accepted"] == want and np.array_equal(e, err) and np.array_equal(R.reshape(7, 4), full[:, :4].numpy())
assert np.array_equal(info["iters"], full[:, 14].numpy().astype(np.int64))
dist.barrier()
if rank == 0:
    print("GLOO_RUN_ICP_PAIR_OK", world)
dist.destroy_process_group()
'''


def test_sharded_run_icp_pair_gloo_world2(tmp_path):
    """icpmi.dist.RunIcpPairSharded / run_icp_pair_batch_sharded (slam.py:575-597 over ranks): candidates interleaved over two
    gloo ranks, the oracle injected as the local solver; gathered records in candidate order, first accepted candidate."""
    script = tmp_path / "worker.py"
    script.write_text(RUN_ICP_PAIR_WORKER.format(repo=REPO, pkg=PKG))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29733", str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GLOO_RUN_ICP_PAIR_OK 2" in r.stdout


def test_row_bands_cover_and_balance():
    import torch
    from icpmi import dist as idist, synth
    assert idist.row_bands(10, 4) == [0, 2, 5, 7, 10]
    assert idist.row_bands(7, 1) == [0, 7]
    segs = synth.room_segments()
    poses = [(0.0, 0.0, 0.0), (1.0, -0.5, 0.3), (-2.0, 1.0, -0.2)]
    hits = [synth.to_world(synth.scan(p, 50 + i, segs=segs), p) for i, p in enumerate(poses)]
    org = np.array([[p[0], p[1]] for p in poses])
    ny = 800
    cost = idist.row_costs(ny, -20.0, 0.05, org, hits)
    assert cost.shape == (ny,) and int(cost.min()) >= 0 and int(cost.sum()) > 0
    for world in (2, 3, 8):
        b = idist.row_bands(ny, world, cost)
        assert b[0] == 0 and b[-1] == ny and all(b[i] <= b[i + 1] for i in range(world))
        work = [int(cost[b[i]:b[i + 1]].sum()) for i in range(world)]
        assert max(work) < 1.5 * sum(work) / world, work           # near-equal shares of the estimated work
    # same numbers from torch tensors as from numpy arrays (every rank must agree)
    cost_t = idist.row_costs(ny, -20.0, 0.05, torch.from_numpy(org), [torch.from_numpy(h) for h in hits])
    assert torch.equal(cost, cost_t)


REPLAY_WORKER = r"""
import os, sys, types
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, {pkg!r})
import oracle
from icpmi import dist as idist, synth

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
segs = synth.room_segments()
poses = [(0.3 * i, -0.1 * i, 0.05 * i) for i in range(4)]
hits = [synth.to_world(synth.scan(p, 300 + i, segs=segs), p)[::8] for i, p in enumerate(poses)]
org = np.array([[p[0], p[1]] for p in poses])
g = types.SimpleNamespace(ny=300, nx=420, min_x=-10.5, min_y=-7.5, resolution=0.05)
l_hit, l_miss = float(np.log(0.85 / 0.15)), float(np.log(0.42 / 0.58))

def whole():
    lo = np.zeros((g.ny, g.nx), dtype=np.float32)
    for o, h in zip(org, hits):
        oracle.grid_update_scan(lo, g.min_x, g.min_y, g.resolution, o, h, l_hit, l_miss, -8.0, 8.0)
    return lo

def replay(r0, r1):          # stand-in for the GPU band replay: cells are independent, so a band is a slice
    return torch.from_numpy(whole()[r0:r1].copy())

bands, full = idist.replay_scans_sharded(g, org, hits, replay=replay)
assert len(bands) == world + 1 and bands[0] == 0 and bands[-1] == g.ny
assert 0 < bands[1] < g.ny                       # both ranks own rows the scans touch
assert np.array_equal(full.numpy(), whole())
bands2, full2 = idist.replay_scans_sharded(g, org, hits, replay=replay, balance=False)
assert bands2 == [0, 150, 300] and np.array_equal(full2.numpy(), whole())
dist.barrier()
if rank == 0:
    print("REPLAY_OK", world, bands)
dist.destroy_process_group()
"""


def test_sharded_replay_gloo_world2(tmp_path):
    script = tmp_path / "replay_worker.py"
    script.write_text(REPLAY_WORKER.format(repo=REPO, pkg=PKG))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29717", str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "REPLAY_OK 2" in r.stdout


def test_bench_self_launch_decision():
    """`python bench.py --gpus 2` without WORLD_SIZE (how the driver starts it) must decide to spawn child ranks
    under torch.distributed.run BEFORE torch is imported in the parent (never re-exec a process that touched the GPU)."""
    import json
    code = ("import sys, runpy\n"
            f"sys.argv = [{os.path.join(REPO, 'bench.py')!r}, '--gpus', '2', '--steps', '3', '--warmup', '1']\n"
            "try:\n"
            f"    runpy.run_path({os.path.join(REPO, 'bench.py')!r}, run_name='__main__')\n"
            "except SystemExit as e:\n"
            "    assert e.code == 0, e.code\n"
            "assert 'torch' not in sys.modules, 'the launching parent imported torch'\n"
            "print('PARENT_CLEAN')\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["ICPMI_BENCH_DRYLAUNCH"] = "1"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PARENT_CLEAN" in r.stdout
    cmd = json.loads(r.stdout.splitlines()[0])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    i = cmd.index(os.path.join(REPO, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]
    # under a launcher (WORLD_SIZE set) the same command line does not spawn again: it goes on to need a GPU
    env2 = dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                        env=env2, timeout=300)
    assert "launch" not in r2.stdout
    import torch
    if not torch.cuda.is_available():
        assert r2.returncode != 0 and "no CPU fallback" in (r2.stdout + r2.stderr)


def test_bench_refuses_stale_pmc_traffic(tmp_path, monkeypatch):
    """roofline.traffic comes from a committed rocprofv3 --pmc summary; one collected on other kernel sources is refused."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sig = bench.csrc_signature()
    assert re.fullmatch(r"[0-9a-f]{16}", sig)
    doc = {"csrc_sha256": sig, "kernels": {"void icpmi::icp2_fused_kernel<512, 2, true, true>(icpmi::Icp2Args) [64 workgroups]": {"hbm_bytes_per_launch": 123},
                                           "void icpmi::icp2_resume_rest_kernel<512, 2, true, true>(icpmi::Icp2Args, int) [256 workgroups]": {"hbm_bytes_per_launch": 7}}}
    f = tmp_path / "pmc.json"
    f.write_text(json.dumps(doc))
    monkeypatch.setattr(bench, "PMC_TRAFFIC", str(f))
    assert bench.pmc_traffic(64)[0] == 123
    assert bench.pmc_traffic(65)[0] is None
    doc["csrc_sha256"] = "0" * 16
    f.write_text(json.dumps(doc))
    t, why = bench.pmc_traffic(64)
    assert t is None and "stale" in why
    # the vector-issue roofline of a batch comes from the committed SQ-counter summary the same way
    k = "void icpmi::icp2_fused_kernel<512, 2, true, true> [64 workgroups]"
    mix = {"csrc_sha256": sig, "kernels": {k: {"SQ_ACTIVE_INST_VALU": 6.4e6, "SQ_BUSY_CYCLES": 1.0e6,
                                               "derived": {"valu_issue_frac": 0.8, "active_lanes_per_valu_instruction": 44.0}}}}
    g = tmp_path / "mix.json"
    g.write_text(json.dumps(mix))
    monkeypatch.setattr(bench, "PMC_MIX", str(g))
    issue, src = bench.pmc_issue(64)
    assert abs(issue["frac"] - 6.4e6 * 4 / (1024 * 1.0e6 / 32)) < 1e-4 and "same csrc" in src
    mix["csrc_sha256"] = "0" * 16
    g.write_text(json.dumps(mix))
    assert bench.pmc_issue(64)[0] is None and "stale" in bench.pmc_issue(64)[1]
    assert os.path.basename(bench.latest_profile("pmc_traffic.json")).startswith("r")


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs writes the last step's result records field by field as float64 .npy, every pair in pair order;
    past DUMP_MAX_PAIRS, the same seeded sample of pairs every time, with its indices."""
    import importlib.util
    from icpmi import _lib
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_MAX_PAIRS * 88 <= 64 * 2**20
    B = 10
    res = np.zeros((B, _lib.RES_DOUBLES))
    res[:, _lib.RES_R:_lib.RES_R + 4] = np.arange(4 * B).reshape(B, 4)
    res[:, _lib.RES_T:_lib.RES_T + 2] = -np.arange(2 * B).reshape(B, 2)
    res[:, _lib.RES_ERR], res[:, _lib.RES_DELTA] = np.arange(B) * 1e-3, np.arange(B) * 1e-6
    res[:, _lib.RES_ITERS], res[:, _lib.RES_STATUS] = np.arange(B) + 1, np.arange(B) % 4 + 1
    bench.dump_outputs(str(tmp_path / "all"), res)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["R", "delta", "error", "iterations", "status", "t"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["R"], np.arange(4 * B).reshape(B, 2, 2)) and np.array_equal(got["t"][:, 1], -np.arange(1, 2 * B, 2))
    assert np.array_equal(got["iterations"], np.arange(B) + 1) and np.array_equal(got["error"], np.arange(B) * 1e-3)
    assert np.array_equal(got["delta"], np.arange(B) * 1e-6) and np.array_equal(got["status"], np.arange(B) % 4 + 1)
    monkeypatch.setattr(bench, "DUMP_MAX_PAIRS", 4)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), res)
    idx = np.load(tmp_path / "s1" / "pair_index.npy")
    assert len(idx) == 4 and np.array_equal(idx, np.load(tmp_path / "s2" / "pair_index.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "iterations.npy"), idx + 1)
    assert np.array_equal(np.load(tmp_path / "s1" / "status.npy"), idx % 4 + 1)


def test_bench_pairs_equal_synth():
    """The bench builds its scan pairs in ranges, in spawned processes: the same arrays, bit for bit and in the same
    order, as icpmi.synth.loop_closure_batch makes in one call (the inputs of the measured path do not change)."""
    from icpmi import synth
    import bench
    for seed0 in (1000, 1000 + 100003):
        want = synth.loop_closure_batch(40, seed0=seed0)
        a, b = bench.pairs_chunk((0, 17, seed0)), bench.pairs_chunk((17, 40, seed0))
        got = (a[0] + b[0], a[1] + b[1])
        assert all(len(g) == 40 and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(g, w))
                   for g, w in zip(got, want))
    code = ("import sys, numpy as np\n"
            f"sys.path[:0] = [{REPO!r}, {PKG!r}]\n"
            "import bench\n"
            "from icpmi import synth\n"
            "if __name__ == '__main__':\n"
            "    got = bench.make_pairs(300, 1000, 3)\n"
            "    want = synth.loop_closure_batch(300, seed0=1000)\n"
            "    assert all(len(g) == 300 and all(np.array_equal(x, y) for x, y in zip(g, w)) for g, w in zip(got, want))\n"
            "    assert 'torch' not in sys.modules\n"
            "    print('PAIRS_EQUAL')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PAIRS_EQUAL" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_arange_rows_is_numpys_arange():
    """icpmi.prealign.arange_rows tabulates np.arange(lo[k], hi[k], step) for every k at once (the fine grids that can
    follow each coarse winner of a rotation search, features.py:227-229): the same numbers and lengths bit for bit."""
    from icpmi.prealign import arange_rows
    for cstep, fstep in ((2.0, 0.2), (1.5, 0.1), (2.0, 0.5), (7.0, 0.33), (1.0, 2.5)):
        coarse = np.deg2rad(np.arange(-180, 180, cstep))
        lo, hi = coarse - np.deg2rad(cstep), coarse + np.deg2rad(cstep)
        vals, n = arange_rows(lo, hi, np.deg2rad(fstep))
        for k in range(len(coarse)):
            ref = np.arange(lo[k], hi[k], np.deg2rad(fstep))
            assert n[k] == len(ref) and np.array_equal(vals[k, :n[k]], ref), (cstep, fstep, k)
    vals, n = arange_rows([1.0, 2.0], [1.0, 1.5], 0.1)                  # empty grids
    assert list(n) == [0, 0]


def test_candidate_poses_stay_out_of_obstacles():
    """synth.loop_closure_batch: the defaults are unchanged by the rejection of poses inside boxes (none of them is
    within reach at 0.6 m), the 3 m / 20 degree candidates all stand in free space."""
    from icpmi import synth
    rng_poses = []
    for i in range(64):
        rng = np.random.default_rng(500 + i)
        d, a, th = rng.uniform(0.0, 0.6), rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-6.0, 6.0))
        rng_poses.append((0.5 + d * np.cos(a), -0.3 + d * np.sin(a)))
    assert all(synth._free_pose(x, y) for x, y in rng_poses)            # first draws are always accepted at 0.6 m
    assert not synth._free_pose(3.0, 2.0) and not synth._free_pose(9.9, 0.0) and synth._free_pose(0.5, -0.3)
    srcs, tgts = synth.loop_closure_batch(3, seed0=500, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
    assert srcs[0] is srcs[1] and all(len(t) == 2048 for t in tgts)     # a scan from free space sees a wall on every beam


def test_pair_lists_of_the_batched_run_icp_pair():
    from icpmi.batch import pair_lists as _pair_lists
    a, b, c = np.zeros((5, 2)), np.ones((6, 2)), np.ones((7, 2))
    clouds, ps, pt = _pair_lists(a, [b, c])                              # one source shared by every pair (slam.py:576-579)
    assert len(clouds) == 3 and list(ps) == [0, 0] and list(pt) == [1, 2]
    clouds, ps, pt = _pair_lists([a, b], [b, c])
    assert len(clouds) == 4 and list(ps) == [0, 1] and list(pt) == [2, 3]
    with pytest.raises(ValueError):
        _pair_lists([a], [b, c])


def test_pair_list_refuses_lists_of_different_lengths():
    """icpmi.batch.PairList, its host half (no device): int32 copies, the number of pairs, the one length check."""
    from icpmi.batch import PairList
    p = PairList([0, 0, 1], (3, 4, 5))
    assert p.B == 3 and p.src_host.dtype == p.tgt_host.dtype == np.int32 and p.src is None and p.tgt is None
    assert list(p.src_host) == [0, 0, 1] and list(p.tgt_host) == [3, 4, 5]
    assert PairList.of(p) is p and PairList.of([1], [2]).B == 1 and PairList([], []).B == 0
    for ps, pt in (([0, 1], [2]), ([0], [1, 2]), ([], [0])):
        with pytest.raises(ValueError, match="pair_src and pair_tgt differ in length"):
            PairList(ps, pt)


def test_icp_params_builder():
    """icpmi.batch.icp_params: the reference's rules for the ICP problem record (icp.py:153, 162, 196), once."""
    from icpmi import _lib
    from icpmi.batch import icp_params, init_rows
    p = icp_params(1e-7, 0.5, 100, "point_to_line", True, 2)
    assert (p.error_threshold, p.max_corr_dist, p.max_iterations, p.method, p.has_init, p.dim) == (1e-7, 0.5, 100, _lib.POINT_TO_LINE, 1, 2)
    assert icp_params(1e-7, None, 100, "point_to_line", False, 3).method == _lib.POINT_TO_POINT       # 3-D: icp.py:162
    assert icp_params(1e-7, None, 100, "point_to_point", False, 2).method == _lib.POINT_TO_POINT
    assert icp_params(1e-7, None, 100, "plane", False, 2).method == _lib.POINT_TO_POINT                # IcpBatch: icp.py:196 else-branch
    for dim in (2, 3):
        with pytest.raises(ValueError, match="method must be 'point_to_point' or 'point_to_line', got 'plane'"):
            icp_params(1e-7, None, 100, "plane", False, dim, strict=True)                              # the history's policy
    assert icp_params(1e-7, None, 100, "point_to_line", False, 2, strict=True).method == _lib.POINT_TO_LINE
    assert icp_params(1e-7, None, 100, "point_to_point", False, 2).max_corr_dist == -1.0
    # an init counts only when both halves are given (icp.py:153)
    R, t = np.eye(2), np.zeros(2)
    for Ri, ti, want in ((R, t, 1), (R, None, 0), (None, t, 0), (None, None, 0)):
        rows = init_rows(Ri, ti, 1, 2)
        assert (rows is not None) == bool(want)
        assert icp_params(1e-7, None, 100, "point_to_point", rows is not None, 2).has_init == want


def test_init_rows_builder():
    """icpmi.batch.init_rows against the expression IcpBatch.__init__ held before: one start broadcast to every pair, one
    start per pair, and the 3-D case."""
    from icpmi.batch import init_rows
    rng = np.random.default_rng(3)

    def before(R_init, t_init, B, d):
        R = np.broadcast_to(np.asarray(R_init, dtype=np.float64), (B, d, d)).reshape(B, d * d)
        t = np.broadcast_to(np.asarray(t_init, dtype=np.float64), (B, d))
        return np.ascontiguousarray(np.concatenate([R, t], axis=1))

    for shape_R, shape_t, B, d in (((2, 2), (2,), 3, 2), ((3, 2, 2), (3, 2), 3, 2), ((3, 3), (3,), 3, 3), ((3, 3), (3,), 1, 3)):
        R, t = rng.normal(size=shape_R), rng.normal(size=shape_t)
        got = init_rows(R, t, B, d)
        assert got.shape == (B, d * d + d) and got.dtype == np.float64 and got.flags.c_contiguous
        assert np.array_equal(got, before(R, t, B, d))
    got = init_rows(R := rng.normal(size=(2, 2)), t := rng.normal(size=2), 3, 2)
    assert all(np.array_equal(row, np.concatenate([R.ravel(), t])) for row in got)               # R row major, then t
    per = init_rows(Rs := rng.normal(size=(3, 2, 2)), ts := rng.normal(size=(3, 2)), 3, 2)
    assert all(np.array_equal(per[b], np.concatenate([Rs[b].ravel(), ts[b]])) for b in range(3))
    with pytest.raises(ValueError):
        init_rows(np.eye(2), np.zeros(2), 3, 3)                                                 # a 2-D start for 3-D pairs


def test_scan_ids_validator():
    """icpmi.history._scan_ids: the one check of scan ids behind ScanHistory.match, world_row_args and icp, with the messages
    each of them raised before."""
    from icpmi.history import _scan_ids
    cand, ids = ("candidates", "candidate ids"), ("ids", "scan ids")
    for what, m1, m2 in ((cand, "candidates must be a 1-D sequence of scan ids", "candidate ids must lie in [0, 7): got "),
                         (ids, "ids must be a 1-D sequence of scan ids", "scan ids must lie in [0, 7): got ")):
        for bad in ([[0, 1], [2, 3]], [0.0, 1.0], [0.5], 3):                                      # 2-D, floats, a scalar
            with pytest.raises(ValueError) as e:
                _scan_ids(bad, what, 7)
            assert str(e.value) == m1
        for bad, got in (([0, -1, 3], "-1..3"), ([7], "7..7"), ([0, 12], "0..12"), (np.array([-2, 9]), "-2..9")):
            with pytest.raises(ValueError) as e:
                _scan_ids(bad, what, 7)
            assert str(e.value) == m2 + got
        out = _scan_ids([], what, 7)                                                               # an empty list is fine
        assert out.shape == (0,) and out.dtype == np.int32
        out = _scan_ids([6, 0, 6, 6, 3], what, 7)                                                  # and so are repeats
        assert out.dtype == np.int32 and out.flags.c_contiguous and list(out) == [6, 0, 6, 6, 3]
        assert list(_scan_ids(np.array([1, 2], dtype=np.int64), what, 7)) == [1, 2]
        with pytest.raises(ValueError, match="got 0..0"):
            _scan_ids([0], what, 0)                                                                # an empty history has no ids
    # one id, not a sequence (ScanHistory.icp, the source of ScanHistory.match)
    assert _scan_ids(6, ids, 7, one=True) == 6 and _scan_ids(np.int32(0), ids, 7, one=True) == 0
    for bad in (7, -1):
        with pytest.raises(ValueError) as e:
            _scan_ids(bad, ids, 7, one=True)
        assert str(e.value) == f"scan ids must lie in [0, 7): got {bad}"
    with pytest.raises(ValueError) as e:
        _scan_ids(9, ("source", "source id"), 7, one=True)
    assert str(e.value) == "source id must lie in [0, 7): got 9"


def test_cell_box_of_a_scan_matches_the_array_expression():
    """The live update_scan takes the cell box of a scan on the host: min / max of the rows on a transposed copy and the
    box in scalar arithmetic.  Both must equal the plain NumPy expressions they replace (same IEEE operations)."""
    import types
    from utilities import mapping
    rng = np.random.default_rng(5)
    grid = types.SimpleNamespace(min_x=-56.05, min_y=-60.0, resolution=0.05)
    for trial in range(300):
        scale = 10.0 ** rng.integers(-3, 11)
        rows = rng.normal(size=(int(rng.integers(1, 400)), 2)) * scale
        if trial % 50 == 7:
            rows[rng.integers(0, len(rows)), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, -np.inf])
        lo, hi = mapping._minmax_rows(rows)
        assert np.array_equal(lo, rows.min(axis=0), equal_nan=True) and np.array_equal(hi, rows.max(axis=0), equal_nan=True)
        got = mapping.OccupancyGrid2D._box_of(grid, lo, hi)
        lo_hi = np.array([rows.min(axis=0), rows.max(axis=0)])
        if not np.isfinite(lo_hi).all():
            assert got is None
            continue
        c = np.clip(np.floor((lo_hi - np.array([grid.min_x, grid.min_y])) / grid.resolution), -2.0 ** 29, 2.0 ** 29)
        want = np.array([c[0, 0] - 1, c[0, 1] - 1, c[1, 0] + 1, c[1, 1] + 1], dtype=np.int32)
        assert got.dtype == np.int32 and np.array_equal(got, want), trial


def test_cell_box_holds_a_coordinate_whose_quotient_overflows():
    """A finite coordinate near 1.8e308 has an infinite quotient: the library drops that beam, and the box — clamped before the
    floor — is the clamp on that side (math.floor(inf) raised OverflowError out of update_scan)."""
    import types
    from utilities import mapping
    grid = types.SimpleNamespace(min_x=0.0, min_y=0.0, resolution=0.05)
    got = mapping.OccupancyGrid2D._box_of(grid, np.array([-1.7e308, 1.0]), np.array([2.0, 1e301]))
    assert got.tolist() == [-2 ** 29 - 1, 19, 41, 2 ** 29 + 1]


def test_grid_update_plan_rows():
    """icpmi_grid_update_plan: the host-only view of what icpmi_grid_update_scans_box starts — its refusals, and the pass, group
    size, tiles, live scans and wide flag for the default RAYCAST option, and the rounds and kernel launches of the call
    (counted by hand from the launcher's rules), against literal values."""
    import ctypes
    import icpmi
    from icpmi import _lib
    icpmi.build()
    lib = icpmi.lib()
    ERR_ARG, NONE, OWNER, TILES, ATOMIC = -1, _lib.RC_PASS_NONE, _lib.RC_PASS_OWNER, _lib.RC_PASS_TILES, _lib.RC_PASS_ATOMIC
    assert ctypes.sizeof(_lib.GridPlan) == 32 and _lib.GridPlan.wide.offset == 20

    def call(ny=150, nx=200, res=0.05, off=(0, 2048), have_hits=1, full_clip=0, rows=None, box=(0, 0, 199, 149), out=True, n_scans=None):
        o = np.array(off, dtype=np.int32) if off is not None else None
        b = np.array(box, dtype=np.int32) if box is not None else None
        plan = _lib.GridPlan(-7, -7, -7, -7, -7, -7, -7, -7)
        r0, r1 = (0, ny) if rows is None else rows
        code = lib.icpmi_grid_update_plan(ny, nx, res, o.ctypes.data if o is not None else None, len(off) - 1 if n_scans is None else n_scans,
                                          have_hits, full_clip, r0, r1, b.ctypes.data if b is not None else None,
                                          ctypes.byref(plan) if out else None)
        return code, (plan.pass_, plan.group_max, plan.tiles_x, plan.tiles_y, plan.live_scans, plan.wide), (plan.rounds, plan.launches)

    # refusals, in the order of icpmi_grid_update_scans_box
    for kw in (dict(out=False), dict(off=None, n_scans=1), dict(ny=0), dict(nx=-1), dict(n_scans=-1), dict(rows=(-1, 10)), dict(rows=(0, 151)),
               dict(rows=(9, 8)), dict(ny=2 ** 29 + 1, rows=(0, 1)), dict(res=0.0), dict(res=float("nan")), dict(off=(0, 10, 5)),
               dict(have_hits=0), dict(off=(0, 2, 4, 6, 5), box=None)):            # the last: a bad count beyond the first group
        assert call(**kw)[0] == ERR_ARG, kw
    # (pass, group_max, tiles_x, tiles_y, live_scans, wide), (rounds, launches).  A group: the launch that counts it (and finalises
    # the group before it), one before it for its scan boxes (TILES, several live scans) unless a group went before, one after it to
    # finalise it unless a group follows; a wide scan: four.
    five = (0, 10, 20, 30, 40, 50)
    rows = [(dict(), (OWNER, 2, 4, 3, 1, 0), (1, 1)),                                  # the live update
            (dict(rows=(7, 7)), (NONE, 0, 0, 0, 0, 0), (0, 0)),                         # an empty band starts nothing
            (dict(full_clip=1), (ATOMIC, 2, 4, 3, 1, 0), (1, 2)),                       # the owner pass does no whole-grid clip: count + finalise
            (dict(box=None), (ATOMIC, 2, 4, 3, 1, 0), (1, 2)),                          # no promise about the rays
            (dict(off=(0, 65535)), (OWNER, 2, 4, 3, 1, 0), (1, 1)), (dict(off=(0, 65536)), (ATOMIC, 2, 4, 3, 1, 1), (1, 4)),
            (dict(off=(0, 100, 100, 300)), (TILES, 2, 4, 3, 2, 0), (1, 3)),             # a replay with a box: boxes + step + finalise
            (dict(off=(0, 100, 70000, 70100)), (TILES, 2, 4, 3, 3, 1), (3, 10)),        # a wide scan in the middle: 3 + 4 + 3
            (dict(off=(0, 70000, 70000, 70010)), (TILES, 2, 4, 3, 2, 1), (2, 7)),       # a wide scan first, a scan without beams: 4 + 3
            (dict(off=(0, 10, 20, 30, 100000), box=None), (ATOMIC, 2, 4, 3, 4, 1), (3, 7)),   # a wide scan last: 1 + 2 + 4
            (dict(off=(0, 100, 300), box=(10, 20, 70, 40)), (TILES, 32, 1, 1, 2, 0), (1, 3)),   # a small box: 32 scans a group
            (dict(off=(0, 100, 300), rows=(40, 97)), (TILES, 5, 4, 1, 2, 0), (1, 3)),   # a band: 200 x 57 cells
            (dict(off=(0, 100, 300), box=(300, 0, 400, 10)), (ATOMIC, 32, 1, 1, 2, 0), (1, 2)),  # a box beside the grid: an empty window
            (dict(off=(0, 0, 0)), (ATOMIC, 2, 4, 3, 0, 0), (0, 0)), (dict(off=(0, 0), have_hits=0), (ATOMIC, 2, 4, 3, 0, 0), (0, 0)),
            (dict(off=five, box=None), (ATOMIC, 2, 4, 3, 5, 0), (3, 4)),                # groups of 2: count + 2 steps + finalise
            (dict(off=five), (TILES, 2, 4, 3, 5, 0), (3, 5)),                           # boxes once + 3 steps + finalise
            (dict(ny=4000, nx=4000, box=(0, 0, 3999, 3999)), (ATOMIC, 2, 63, 63, 1, 0), (1, 2)),   # 3 969 tiles: too many for the owner pass
            (dict(ny=1200, nx=1200, box=(0, 0, 1199, 1199)), (ATOMIC, 2, 19, 19, 1, 0), (1, 2)),   # 361 > 320
            (dict(ny=1088, nx=1088, box=(0, 0, 1087, 1087)), (OWNER, 2, 17, 17, 1, 0), (1, 1))]    # 289 tiles
    for kw, want, issued in rows:
        code, got, got_issued = call(**kw)
        assert code == 0 and got == want and got_issued == issued, (kw, got, got_issued)


def test_the_four_pair_entries_judge_a_bad_pair_list_alike():
    """The exhaustive match, the wide search, the check and the beam model take one pair list (cloud set offsets on the host,
    a cloud index per pair) and refuse a bad one with the same code, decided on the host before anything is enqueued: the
    device pointers are fakes that are never dereferenced, and everything else about each call is in order."""
    import icpmi
    L = icpmi.lib()
    FAKE, BIG, ERR_ARG, ERR_UNSUPPORTED = 4096, 1 << 40, -1, -4

    def codes(off=(0, 100, 100, 360), pair=(0, 2, 1, 2), n_clouds=None, off_host=True):
        off_a, pair_a = np.array(off, dtype=np.int32), np.array(pair, dtype=np.int32)
        lst = (FAKE, FAKE, off_a.ctypes.data if off_host else None, None, len(off_a) - 1 if n_clouds is None else n_clouds, FAKE,
               pair_a.ctypes.data, len(pair_a), FAKE, FAKE)                  # pts ... cos_sin, as all four take them
        world = (-14.0, -10.0, 0.1)
        return (L.icpmi_grid_match_batch(FAKE, 400, 560, *world, *lst, 1, 0, -1, FAKE, None, FAKE, BIG, None),
                L.icpmi_grid_search_batch(FAKE, FAKE, 400, 560, *world, *lst, 1, 0, 4, -1, FAKE, None, FAKE, BIG, None),
                L.icpmi_grid_check_batch(None, FAKE, 400, 560, 2048, *world, *lst, 2, FAKE, None, 0, None, 0, None),
                L.icpmi_grid_beam_batch(None, FAKE, 400, 560, 2048, *world, *lst, 0.5, 8, FAKE, FAKE, None, None, 0, None, 0, None))

    assert codes(pair=(0, 3)) == (ERR_ARG,) * 4                              # an index beyond the set
    assert codes(off=(0, 100, 90, 360)) == (ERR_ARG,) * 4                    # a negative row count
    assert codes(n_clouds=-1) == (ERR_ARG,) * 4
    assert codes(off_host=False) == (ERR_ARG,) * 4
    assert codes(off=(0, 65536), pair=(0,)) == (ERR_UNSUPPORTED,) * 4        # a cloud above ICPMI_GM_MAX_ROWS


def test_map_pairs_forms_the_head_of_the_check_and_the_beam_model_once(monkeypatch):
    """icpmi.gridmatch.MapPairs over CPU tensors (nothing dereferences them) and a stand-in for the library that records
    its arguments: the head (``field`` ... ``cos_sin``) and the tail (workspace, bytes, stream) of both C calls equal a tuple
    written out here in include/icpmi.h's order; GridMatchBatch's pair part is the same GridPairs' output; the stream is
    asked for at every call and not at construction; re-pointing and a second cloud set leave the pair list alone; and every
    refusal ``_map_pairs`` raised is raised with its text."""
    import types
    import torch
    from icpmi import _lib, gridmatch
    from icpmi.batch import CloudSet
    from test_grid_pairs_gpu import CAPS, COUNTS, K, MIN_X, MIN_Y, NX, NY, PAIRS, RES, THRESHOLD
    value = lambda args: [getattr(a, "value", a) for a in args]                 # noqa: E731  (c_void_p -> its address, None for null)
    rng = np.random.default_rng(58)
    off = np.concatenate([[0], np.cumsum(CAPS)]).astype(np.int32)
    cs = CloudSet(torch.from_numpy(rng.normal(size=(sum(CAPS), 2))), off, cnt=torch.tensor(COUNTS, dtype=torch.int32))
    B = len(PAIRS)
    t, rot, t2, rot2 = (torch.from_numpy(rng.normal(size=(B, 2))) for _ in range(4))
    planes = gridmatch.OccupancyPlanes(torch.zeros(2 * NY * ((NX + 31) // 32) * 4, dtype=torch.uint8), NY, NX, THRESHOLD)
    asked, calls = [], []
    monkeypatch.setattr(gridmatch, "_stream", lambda: asked.append(1) or 1000 + len(asked))
    record = lambda name: lambda *a: calls.append((name, value(a))) or 0         # noqa: E731
    fake = types.SimpleNamespace(icpmi_grid_check_batch=record("check"), icpmi_grid_beam_batch=record("beam"),
                                 icpmi_grid_occupancy_planes_bytes=_lib.lib().icpmi_grid_occupancy_planes_bytes)

    mp = gridmatch.MapPairs(planes, None, MIN_X, MIN_Y, RES, cs, PAIRS, t, rot)
    assert asked == [] and (mp.B, mp.stride, mp.dev) == (B, 300, torch.device("cpu"))
    assert mp.t is t and mp.rot is rot                                           # float64, contiguous, on the map's device: in place
    assert mp.pairs.host.dtype == np.int32 and mp.pairs.host.tolist() == list(PAIRS) and mp.pairs.dev.tolist() == list(PAIRS)
    assert mp.pairs.clouds.tolist() == [0, 1, 2, 3] and mp.pairs.times.tolist() == [1, 1, 3, 3]
    pair_part = [cs.pts.data_ptr(), cs.off.data_ptr(), cs.off_host.ctypes.data, cs.cnt.data_ptr(), 4, mp.pairs.dev.data_ptr(),
                 mp.pairs.host.ctypes.data, B]
    head = [None, planes.buf.data_ptr(), NY, NX, THRESHOLD, MIN_X, MIN_Y, RES] + pair_part + [t.data_ptr(), rot.data_ptr()]
    assert value(mp.head) == head and value(mp.pairs.args(cs)) == pair_part
    rec, rows = torch.zeros((B, _lib.GK_INTS), dtype=torch.int32), torch.zeros((B, 300, _lib.GK_ROW_INTS), dtype=torch.int32)
    hist, table = torch.zeros((B, 19), dtype=torch.int32), torch.zeros(19, dtype=torch.int32)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    assert mp.check(2, want_rows=True, out=(rec, rows)) == (rec, rows)
    assert mp.beam(table, 8, 1.5, want_hist=True, out=(rec, hist, None)) == (rec, hist, None)
    assert calls[0] == ("check", head + [2, rec.data_ptr(), rows.data_ptr(), 300, None, 0, 1001])
    assert calls[1] == ("beam", head + [1.5, 8, table.data_ptr(), rec.data_ptr(), hist.data_ptr(), None, 300, None, 0, 1002])
    assert len(asked) == 2                                                       # once per call

    # through a field: the workspace the entry packs the planes into is made at construction and is the tail's
    fld = torch.zeros((NY, NX), dtype=torch.int16)
    mf = gridmatch.MapPairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, mp.pairs, t, rot)
    assert mf.pairs is mp.pairs and value(mf.head)[:5] == [fld.data_ptr(), None, NY, NX, THRESHOLD] and value(mf.head)[5:] == head[5:]
    assert value(mf.tail()) == [mf.ws.data_ptr(), mf.ws.numel(), 1003] and mf.ws.numel() > 0

    # re-pointed: the two pose pointers change, nothing else; pointed back, the head is the first one
    dev_before = mp.pairs.dev
    assert value(mp.point_at(t2, rot2).head) == head[:16] + [t2.data_ptr(), rot2.data_ptr()] and mp.pairs.dev is dev_before
    assert value(mp.point_at(t, rot).head) == head

    # an existing pair list against a second cloud set — the filter's pattern, all pairs naming cloud 0: judged from the clouds
    # it names; the B entries are not read (the host array is swapped for something that has an address and nothing else) and
    # nothing is uploaded
    zeros = gridmatch.GridPairs(np.zeros(B, dtype=np.int32), torch.device("cpu"))
    assert zeros.clouds.tolist() == [0] and zeros.times.tolist() == [B]
    zeros_dev, zeros.host = zeros.dev, types.SimpleNamespace(ctypes=zeros.host.ctypes)
    uploads = []
    monkeypatch.setattr(torch, "from_numpy", lambda a: uploads.append(a))
    for rows_of_scan in (5, 7):
        scan = CloudSet(torch.zeros((rows_of_scan, 2), dtype=torch.float64), np.array([0, rows_of_scan], dtype=np.int32),
                        off=torch.tensor([0, rows_of_scan], dtype=torch.int32))
        one = gridmatch.MapPairs(planes, None, MIN_X, MIN_Y, RES, scan, zeros, t, rot)
        assert one.pairs is zeros and zeros.dev is zeros_dev and (one.B, one.stride) == (B, rows_of_scan)
        assert value(one.head)[8:16] == [scan.pts.data_ptr(), scan.off.data_ptr(), scan.off_host.ctypes.data, None, 1, zeros_dev.data_ptr(),
                                         zeros.host.ctypes.data, B]
    assert uploads == []
    monkeypatch.undo()

    # GridMatchBatch hands the same object's output to the two searches
    monkeypatch.setattr(gridmatch, "require_gpu", lambda: None)
    grid = types.SimpleNamespace(device_log_odds=torch.zeros((NY, NX), dtype=torch.float32), min_x=MIN_X, min_y=MIN_Y, resolution=RES,
                                 log_odds_min=-5.0, log_odds_max=5.0)
    match = gridmatch.GridMatchBatch(grid, cs, mp.pairs, t.numpy(), np.zeros((B, 3)), 0, field=(fld, K))
    assert match.pairs is mp.pairs and match.B == B
    assert value(match._pair_args()) == [MIN_X, MIN_Y, RES] + pair_part + [match.t.data_ptr(), match.cos_sin.data_ptr(), 3]

    # the refusals, each with the text it had
    def refused(text, source=planes, min_x=MIN_X, cloud_set=cs, pair=PAIRS, tr=t):
        with pytest.raises(ValueError) as e:
            gridmatch.MapPairs(source, None, min_x, MIN_Y, RES, cloud_set, pair, tr, rot)
        assert str(e.value) == text
    set_of = lambda rows, dim=2: CloudSet(torch.zeros((4, dim), dtype=torch.float64), np.array([0, rows], dtype=np.int32),   # noqa: E731
                                          off=torch.zeros(2, dtype=torch.int32))
    refused("pairs against the grid are 2-D", cloud_set=set_of(4, 3), pair=[0] * B)
    refused("pair_clouds must index the cloud set", pair=(2, 3, 0, 1, 2, 4, 2, 3))
    refused("pair_clouds must index the cloud set", pair=(2, 3, 0, -1, 2, 3, 2, 3))
    refused("a cloud above 65535 rows cannot be scored (int32 sums): filter it first", cloud_set=set_of(65536), pair=[0] * B)
    assert gridmatch.MAX_ROWS == 65535 and 65535 * 8193 >= 2 ** 29 > 65535 * 8192
    many = torch.zeros((8193, 2), dtype=torch.float64)
    with pytest.raises(ValueError) as e:
        gridmatch.MapPairs(planes, None, MIN_X, MIN_Y, RES, set_of(65535), np.zeros(8193, dtype=np.int32), many, many)
    assert str(e.value) == f"{65535 * 8193} rows: fewer than 2^29 fit one call"
    assert gridmatch.MapPairs(planes, None, MIN_X, MIN_Y, RES, set_of(65535), np.zeros(8192, dtype=np.int32), many[:8192], many[:8192]).B == 8192
    refused(f"resolution must be positive and finite and the map's corner finite, got {RES}, (nan, {MIN_Y})", min_x=float("nan"))
    refused(f"translations must be float64 rows of 2, {B} of them", tr=t[:B - 1])
    refused(f"translations must be float64 rows of 2, {B} of them", tr=torch.zeros((B, 3), dtype=torch.float64))
    refused("the map must be a contiguous int16 (ny, nx) device field or the OccupancyPlanes of one", source=fld.float())
    with pytest.raises(ValueError) as e:
        mp.check(2.5)
    assert str(e.value) == "tolerance must be a whole number of steps in [0, 2^30], got 2.5"
    with pytest.raises(ValueError) as e:
        mp.point_at(t, rot[:3])
    assert str(e.value) == f"cos_sin must be float64 rows of 2, {B} of them" and mp.t is t and mp.rot is rot
