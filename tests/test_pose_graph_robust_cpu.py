"""Robust pose-graph edges without a GPU: the two entries exist at every layer, the host refuses what it must before
anything is enqueued, the workspace sizes are what the layout says, the extended-precision helper
(tests/pose_graph_robust_ref.py) is right and its bounds leave room — a NumPy float64 restatement of a robust step is held
to them on every case the GPU tests use, which is the condition on the inputs — and a robust loss does what it is for:
one false loop closure ruins the plain optimum and not the robust ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_robust_ref as rref
from conftest import REPO

LD = np.longdouble
HEADER = os.path.join(REPO, "include", "icpmi.h")
ENTRIES = ("icpmi_pose_graph_robust_workspace_bytes", "icpmi_pose_graph_optimize_robust")


def _defines():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return txt, {n: int(v) for n, v in re.findall(r"^#define ICPMI_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}


def test_entries_are_declared_exported_listed_and_bound():
    import icpmi
    from icpmi import _lib
    txt, _ = _defines()
    path = icpmi.build()
    lib = icpmi.lib()                     # torch first, then the library: one HIP runtime in the process
    raw = C.CDLL(path)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/icpmi.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.icpmi_pose_graph_robust_workspace_bytes.restype is C.c_size_t
    assert len(lib.icpmi_pose_graph_robust_workspace_bytes.argtypes) == 6 and len(lib.icpmi_pose_graph_optimize_robust.argtypes) == 19


def test_every_define_is_mirrored():
    from icpmi import _lib
    from utilities import pose_graph
    _, defines = _defines()
    rob = {n: v for n, v in defines.items() if n.startswith("ROB_")}
    assert set(rob) == {"ROB_KERNEL_HUBER", "ROB_KERNEL_CAUCHY", "ROB_KERNEL_GEMAN_MCCLURE", "ROB_DOUBLES", "ROB_COST_BEFORE",
                        "ROB_COST_AFTER", "ROB_WEIGHTS_US"}
    for n, v in rob.items():
        assert getattr(_lib, n) == v, n
    assert [rob["ROB_KERNEL_" + k] for k in ("HUBER", "CAUCHY", "GEMAN_MCCLURE")] == [0, 1, 2]
    assert rob["ROB_DOUBLES"] == defines["PGINFO_DOUBLES"] + 3
    assert [rob["ROB_" + k] for k in ("COST_BEFORE", "COST_AFTER", "WEIGHTS_US")] == [10, 11, 12]
    assert pose_graph.ROBUST_KERNELS == dict(huber=0, cauchy=1, geman_mcclure=2) and tuple(pose_graph.ROBUST_KERNELS) == rref.KERNELS


def _tiny():
    """A 6-node chain with one closure, host arrays only."""
    ij = np.ascontiguousarray(np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], dtype=np.int32))
    om = np.ascontiguousarray(np.tile(100.0 * np.eye(3), (len(ij), 1, 1)))
    mask = np.ascontiguousarray(np.array([0, 0, 0, 0, 0, 1], dtype=np.uint8))
    return ij, om, mask


def test_host_refusals_come_before_any_launch():
    """Fake device pointers: every refusal below is decided on the host, so none of them is ever touched."""
    import icpmi
    _, defines = _defines()
    ERR_ARG, ERR_WORKSPACE = defines["ERR_ARG"], defines["ERR_WORKSPACE"]
    L = icpmi.lib()
    ij, om, mask = _tiny()
    n, m = 6, len(ij)
    ijp, omp, maskp = (a.ctypes.data_as(C.c_void_p) for a in (ij, om, mask))
    nodes, z, omega, chi2, wgt, info, ws = [C.c_void_p(0x1000 * (k + 1)) for k in range(7)]
    size = L.icpmi_pose_graph_robust_workspace_bytes
    need = size(ijp, omp, maskp, n, m, 0)
    assert need > 0

    def call(nodes=nodes, ijp=ijp, z=z, omega=omega, maskp=maskp, n=n, m=m, iters=5, fix=0, kernel=0, delta=2.0, dense=0, chi2=chi2,
             wgt=wgt, info=info, ws=ws, ws_bytes=need):
        return L.icpmi_pose_graph_optimize_robust(nodes, ijp, z, omega, maskp, n, m, iters, fix, 1e-6, kernel, delta, dense, chi2, wgt,
                                                  info, ws, ws_bytes, None)

    for kernel in (-1, 3, 99):
        assert call(kernel=kernel) == ERR_ARG
    for delta in (0.0, -1.0, float("nan"), -float("inf")):
        assert call(delta=delta) == ERR_ARG
    assert call(maskp=None) == ERR_ARG
    assert call(chi2=None) == ERR_ARG and call(wgt=None) == ERR_ARG
    assert call(nodes=None) == ERR_ARG and call(info=None) == ERR_ARG                     # the argument checks of optimize
    assert call(n=-1) == ERR_ARG and call(m=-1) == ERR_ARG and call(iters=-1) == ERR_ARG
    assert call(ijp=None) == ERR_ARG and call(z=None) == ERR_ARG and call(omega=None) == ERR_ARG
    assert call(fix=6) == ERR_ARG and call(fix=-1) == ERR_ARG
    for bad in ((0, 6), (-1, 2)):
        bad_ij = ij.copy()
        bad_ij[2] = bad
        assert call(ijp=bad_ij.ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert size(bad_ij.ctypes.data_as(C.c_void_p), omp, maskp, n, m, 0) == 0
    for dense in (0, 1):
        least = size(ijp, None, maskp, n, m, dense)
        assert call(dense=dense, ws=None, ws_bytes=least) == ERR_WORKSPACE
        assert call(dense=dense, ws_bytes=least - 1) == ERR_WORKSPACE and call(dense=dense, ws_bytes=0) == ERR_WORKSPACE
    for iters in (0, 5):                                         # evaluation only is refused in the same way
        assert call(iters=iters, kernel=7) == ERR_ARG and call(iters=iters, ws_bytes=0) == ERR_WORKSPACE
    assert size(ijp, omp, maskp, -1, m, 0) == 0 and size(ijp, omp, maskp, n, -1, 0) == 0
    assert size(None, omp, maskp, n, m, 0) == 0 and size(ijp, omp, None, n, m, 0) == 0


def _a(x):
    return (x + 255) // 256 * 256


def test_workspace_sizes_by_hand():
    """PgRobWs (csrc/posegraph.hip) is PgWs — whose formula tests/test_host_cpu.py writes out — without its 256 spare
    bytes, then wgt a(8 (m + 1)), rob a(m + 1) and the 256.  a(x) = x rounded up to 256.
    n = 6, m = 6, k = 1 (the closure), split:
      a(48) + a(28) + a(52) + a(28) + a(8) = 5 x 256 = 1280                        ei/ej, csr_ptr, csr_edge, loop_slot, loop_edge
      5 a(432) = 2560; X a(24 x 6 x 4 = 576) = 768; AB a(288) = 512; M a(80) = 256; g a(32) = 256; dx a(144) = 256
      = 1280 + 2560 + 768 + 512 + 256 + 256 + 256 = 5888, + wgt a(56) = 256 + rob a(7) = 256 + 256 = 6656.
    The same graph with chain edge 2 masked is planned dense, k = 0:
      1280 + 2560 + X a(144) = 256 + AB a(144) = 256 + M a(8) = 256 + g a(8) = 256 + dx 256 + Hd a(8 x 18 x 18 = 2592) = 2816
      = 7936, + 256 + 256 + 256 = 8704; dense != 0 gives the same.
    m = 0, n = 5 (no chain: dense; a(0) = 0 for ei/ej): PgWs 7168 of test_host_cpu.py - 256 = 6912, + wgt a(8) + rob a(1) + 256 = 7680."""
    import icpmi
    L = icpmi.lib()
    ij, om, mask = _tiny()
    ijp, omp = ij.ctypes.data_as(C.c_void_p), om.ctypes.data_as(C.c_void_p)
    size = L.icpmi_pose_graph_robust_workspace_bytes
    assert size(ijp, omp, mask.ctypes.data_as(C.c_void_p), 6, 6, 0) == 6656 == 5888 + 3 * 256
    assert size(ijp, None, mask.ctypes.data_as(C.c_void_p), 6, 6, 0) == 6656
    chain_masked = mask.copy()
    chain_masked[2] = 1
    assert size(ijp, omp, chain_masked.ctypes.data_as(C.c_void_p), 6, 6, 0) == 8704
    assert size(ijp, omp, mask.ctypes.data_as(C.c_void_p), 6, 6, 1) == 8704
    assert size(None, None, None, 5, 0, 0) == 7680
    # and PgWs is where it was: the plain query on the same graph
    assert L.icpmi_pose_graph_workspace_bytes(ijp, 6, 6) == 5888 + 256


@pytest.mark.parametrize("kernel", rref.KERNELS)
def test_weight_is_the_derivative_of_the_loss(kernel):
    """w = d rho / d s by a long-double central difference, on both sides of c; the hand-made |w'| the same way; and the
    three properties the design rests on: w is continuous at c, in (0, 1], and exactly 1.0 where the loss is quadratic."""
    delta = LD(rref.DELTA)
    c = delta * delta
    for s in (LD(1e-3), c / 3, c * LD(0.999), c * LD(1.001), 3 * c, LD(1e3), LD(1e6)):
        # h = 2^-20 s: the truncation h^2 |rho'''| / 6 stays below 2^-38 w for these losses (1e-10 w allows it); what long
        # double's 2^-64 rho loses in the difference, over 2 h, is 2^-45 rho / s (allowed twice) — more than any share of
        # w once rho has flattened out (Geman-McClure at 1e6)
        h = s * LD(2.0) ** -20
        num = (rref.rho_ld(kernel, s + h, delta) - rref.rho_ld(kernel, s - h, delta)) / (2 * h)
        w = rref.weight_ld(kernel, s, delta)
        assert abs(num - w) <= 1e-10 * w + LD(2.0) ** -44 * rref.rho_ld(kernel, s, delta) / s, (kernel, float(s), float(num), float(w))
        slope = (rref.weight_ld(kernel, s + h, delta) - rref.weight_ld(kernel, s - h, delta)) / (2 * h)
        want = rref.weight_slope_ld(kernel, s, delta)
        # differencing w cancels more: 2^-64 w against 2 h |w'|, which is above 1e-7 w at every s here
        assert abs(abs(slope) - want) <= 1e-6 * want, (kernel, float(s))
        assert 0 < w <= 1
    eps = c * LD(2.0) ** -60
    assert abs(rref.weight_ld(kernel, c + eps, delta) - rref.weight_ld(kernel, c - eps, delta)) <= 1e-15
    if kernel == "huber":
        assert rref.weight_ld(kernel, c, delta) == 1 and rref.weight_ld(kernel, LD(0), delta) == 1
        assert rref.rho_ld(kernel, c / 2, delta) == c / 2
    assert rref.rho_ld(kernel, LD(0), delta) == 0 and rref.weight_ld(kernel, LD(0), delta) == 1


@pytest.mark.parametrize("name", ["n33_false_closure", "weak_twins", "scenario_false_closure"])
def test_a_loss_that_never_leaves_the_quadratic_is_the_plain_run(name):
    c = rref.cases()[name]
    g = c["graph"]
    plain = ref.run_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], 4, c["fix"], 1e-9)
    robust = rref.run_robust_ld("huber", 1e150, g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], c["mask"], 4, c["fix"], 1e-9)
    assert robust["iterations"] == plain["iterations"] and robust["status"] == plain["status"]
    for a, b in zip(plain["iterates"], robust["iterates"]):
        assert np.array_equal(a, b)
    assert robust["steps"] == plain["steps"]


CASES = sorted(rref.cases())


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_of_a_robust_step_is_within_the_bound(name):
    """The condition on the inputs: NumPy float64 — weights, assembly, LAPACK's solve — meets the bound the kernel is held
    to on every case, for every loss, and the evaluation's chi2 and weights meet theirs."""
    c = rref.cases()[name]
    g = c["graph"]
    for kernel in rref.KERNELS:
        run = rref.run(name, kernel, 1, 0.0)
        want = ref.step_difference(np.asarray(run["iterates"][0], dtype=np.float64), g["nodes"])
        got = rref.step64(kernel, rref.DELTA, g, c["mask"], c["fix"])
        err = float(np.abs(got - want).max())
        print(f"{name} {kernel}: step bound {run['bounds'][0]:.3e} float64 error/bound {err / run['bounds'][0]:.3e}")
        assert err <= run["bounds"][0], (name, kernel, err, run["bounds"][0])
        ev = rref.evaluation(name, kernel)
        assert np.all(ev["w"] > 0) and np.all(ev["w"] <= 1) and np.all(ev["w"][~c["mask"]] == 1)
        assert np.all(ev["chi2_bound"] <= 1e-9 * np.maximum(np.abs(ev["chi2"]), 1.0)), name        # the bounds say something


def test_runs_of_several_iterations_do_not_stop_by_rounding():
    """No step norm of a several-iteration reference run comes near its eps: status and iteration count are decided.  A
    step within the bounds of the reference's has a norm within sqrt(3 n) times them (as the one-step tests hold it); twice
    that, for what the earlier iterations' errors add, is the margin asked for."""
    for name, c in rref.cases().items():
        if c["multi"]:
            for kernel in rref.KERNELS:
                run = rref.run(name, kernel, c["multi"]["n_iterations"], c["multi"]["eps"])
                total = sum(run["bounds"])
                assert all(abs(s - c["multi"]["eps"]) > 2 * total * np.sqrt(3 * len(c["graph"]["nodes"])) for s in run["steps"]), (name, kernel)
                assert total < 1e-6, (name, kernel, total)


def test_one_false_closure_ruins_the_plain_optimum_and_not_the_robust_ones():
    """The scenario, in long double: a closed loop of 40 nodes, four true closures and one whose measurement is off by
    metres, all with the same information.  Largest position error against the generating poses, after 30 iterations:
    plain 1.619 m; huber 0.646 m, cauchy 0.185 m, geman_mcclure 0.183 m."""
    g, truth, false_edge = rref.false_closure_scenario()
    mask = rref.default_mask(g)
    assert mask[false_edge] and mask.sum() == 5

    def worst(x):
        return float(np.sqrt(np.sum((np.asarray(x, dtype=np.float64)[:, :2] - truth[:, :2]) ** 2, axis=1)).max())

    plain = worst(ref.run_ld(g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], 30, 0, 1e-12)["iterates"][-1])
    print(f"largest position error, plain optimum: {plain:.3e} m")
    for kernel in rref.KERNELS:
        run = rref.run_robust_ld(kernel, rref.DELTA, g["nodes"], g["ei"], g["ej"], g["z"], g["omega"], mask, 30, 0, 1e-12)
        robust = worst(run["iterates"][-1])
        print(f"largest position error, {kernel}: {robust:.3e} m, weight of the false closure {float(run['final']['w'][false_edge]):.3e}")
        assert plain > robust, (kernel, plain, robust)
