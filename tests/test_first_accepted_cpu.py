"""CPU side of stopping after the first accepted candidate (icpmi_icp_batch_gated): the C ABI, the arguments, and the
sharded form under gloo with an injected oracle solver that skips what the gate allows it to skip."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, REPO


def test_gated_entry_is_declared_exported_and_bound():
    import ctypes
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    icpmi.lib()
    assert hasattr(ctypes.CDLL(path), "icpmi_icp_batch_gated")
    assert "icpmi_icp_batch_gated" in _lib.EXPORTS
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    assert re.search(r"#define ICPMI_ST_SKIPPED 5\b", hdr)
    assert _lib.ST_SKIPPED == 5


def test_stop_without_a_gate_raises():
    from icpmi import dist, prealign
    with pytest.raises(ValueError):
        prealign.RunIcpPairBatch([], [], [], stop_after_first_accepted=True)
    with pytest.raises(ValueError):
        dist.RunIcpPairSharded(None, [], stop_after_first_accepted=True)


WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, {pkg!r})
import oracle
from icpmi import dist as idist, synth, _lib

ICP = dict(error_threshold=1e-10, max_iterations=40, voxel_size=0.1, method="point_to_line", normal_k=8)
FEAT = dict(rotation_voxel_size=0.3, angle_step_coarse=6.0, angle_step_fine=1.0)
N = {n}

def one(src, t):
    R0, t0, _ = oracle.rotation_search(src, t, FEAT["rotation_voxel_size"], FEAT["angle_step_coarse"], FEAT["angle_step_fine"])
    R, tt, err, info = oracle.icp(src, t, 1e-10, 40, 0.1, R_init=R0, t_init=t0, method="point_to_line", normal_k=8)
    r = np.zeros(_lib.RES_DOUBLES)
    r[:4] = R.ravel(); r[9:11] = tt; r[12] = err; r[13] = info["delta"]; r[14] = info["iters"]; r[15] = info["status"]
    return r

def full_solver(src, tgts):
    return torch.from_numpy(np.array([one(src, t) for t in tgts]).reshape(-1, _lib.RES_DOUBLES))

def gating_solver(src, tgts, gate):
    # what a gated rank may do: in local order, every candidate after the first one it accepts is skipped — with an error
    # far below the gate, which must never count
    out, accepted = np.zeros((len(tgts), _lib.RES_DOUBLES)), False
    for i, t in enumerate(tgts):
        if accepted:
            out[i, 0] = out[i, 3] = 1.0; out[i, 12] = 0.0; out[i, 15] = _lib.ST_SKIPPED
            continue
        out[i] = one(src, t)
        accepted = out[i, 12] < gate["error_accept"]
    assert gate["index_base"] == dist.get_rank() and gate["index_stride"] == dist.get_world_size()
    return torch.from_numpy(out)

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
srcs, tgts = synth.loop_closure_batch(N, seed0=311, shared_source=True, max_offset=2.0, max_yaw_deg=15.0)
src = srcs[0][::4]; tgts = [t[::4] for t in tgts]
full = full_solver(src, tgts)
err = full[:, 12].numpy()
gates = [float(np.sort(err)[min(2, N - 1)]) * 1.0000001, float(err.min()) * 1.0000001, 0.0]
for gate in gates:
    ok = np.flatnonzero(err < gate)
    want = int(ok[0]) if len(ok) else -1
    job = idist.RunIcpPairSharded(src, tgts, ICP, FEAT, solver=gating_solver, stop_after_first_accepted=True, error_accept=gate)
    res = job.run()
    F = job.first_accepted()
    assert F == want, (rank, gate, F, want)
    upto = N if F < 0 else F + 1
    assert torch.equal(res[:upto], full[:upto]), rank
    for i in range(upto, N):
        assert res[i, 15] == _lib.ST_SKIPPED or torch.equal(res[i], full[i]), (rank, i)
    R, t, e, info = idist.run_icp_pair_batch_sharded(src, tgts, ICP, FEAT, error_accept=gate, solver=gating_solver,
                                                     stop_after_first_accepted=True)
    assert info["first_accepted"] == want and np.array_equal(e[:upto], err[:upto])
dist.barrier()
if rank == 0:
    print("GLOO_GATED_OK", world)
dist.destroy_process_group()
'''


@pytest.mark.parametrize("world,n,port", [(2, 7, 29753), (3, 2, 29763)])
def test_sharded_gate_equals_the_unsharded_run(tmp_path, world, n, port):
    """Candidates interleaved over gloo ranks (world 3 with two candidates: one rank owns none), each rank gating its own
    share with the global candidate numbers: the gathered first accepted candidate and every record up to it are the
    unsharded run's."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(repo=REPO, pkg=PKG, n=n))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"GLOO_GATED_OK {world}" in r.stdout
