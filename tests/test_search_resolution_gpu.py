"""The searches of the fused ICP kernel (csrc/icp2.hip, csrc/sweep.hpp) at the resolution of their float32 filter.

The pairs come from tests/test_search_resolution_cpu.py: stationary, D2-symmetric, hundreds of source rows whose second
(third, fourth) candidate lies 1e-9 .. 1e-2 relative in d^2 behind the nearest — at every iteration, because nothing
moves.  With error_threshold = 0 all six iterations run: 0 and 1 search the plain nearest neighbour (centred, then
seeded), 2 on the top two (centred, then from the kept match; the rows whose third candidate is near search again every
iteration).  One wrong correspondence moves the transform by at least 1000 x FRO_TOL (measured there, row by row), so:
fused path = exhaustive kernel = oracle, in every sort order, alone and in company, through the far continuation, and
above the sizes where the float32 filter and the LDS copy end.  Nothing here is measured from the kernels."""
import numpy as np
import pytest

import oracle
from conftest import rot_err
from test_gpu_parity import FRO_TOL
from test_icp2_layout_gpu import _far_count
from test_search_resolution_cpu import FAMILIES, ITERS, NORMAL_K, VOXEL, all_pairs, pair
from test_search_resolution_cpu import FRO_TOL as CPU_FRO_TOL

pytestmark = pytest.mark.gpu

assert FRO_TOL == CPU_FRO_TOL            # the observability margin is a multiple of the suite's tolerance


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def _batch(family, variant, copies=1, **kw):
    from icpmi import batch
    src, tgt, method, _ = pair(family, variant)
    extra = dict(normal_k=NORMAL_K) if method == "point_to_line" else {}
    return batch.IcpBatch([src, tgt], [0] * copies, [1] * copies, 0.0, ITERS, VOXEL, method=method, **extra, **kw)


def _records(b):
    """One run -> the records on the host; every row kept by the voxel filter."""
    out = b.run().cpu().numpy()[:b.B].copy()
    assert b.vox.cnt.cpu().numpy().tolist() == np.diff(b.raw.off_host).tolist()
    return out


_REFERENCE = {}


def _reference(family, variant, b):
    """oracle.icp on the filtered clouds of ``b`` (the rows in the order the kernels see them), once per pair."""
    if (family, variant) not in _REFERENCE:
        src, tgt = b.vox.to_numpy()
        method = FAMILIES[family][0]
        _REFERENCE[family, variant] = oracle.icp(src, tgt, 0.0, ITERS, VOXEL, method=method, normal_k=NORMAL_K)
    return _REFERENCE[family, variant]


def _against_oracle(rec, ref, label):
    from icpmi import batch
    R, t, err, info = batch.unpack_results(rec, 2)
    Ro, to, eo, io = ref
    assert io["iters"] == ITERS and io["status"] == oracle.MAXITER
    for i in range(len(rec)):
        assert int(info["iters"][i]) == io["iters"] and int(info["status"][i]) == io["status"], (label, i, info, io)
        assert rot_err(R[i], t[i], Ro, to) < FRO_TOL, (label, i, rot_err(R[i], t[i], Ro, to))
        assert abs(err[i] - eo) <= 1e-9 * max(1.0, eo), (label, i, err[i], eo)


@pytest.mark.parametrize("family,variant", all_pairs())
def test_fused_exhaustive_and_oracle_agree_in_every_sort_order(libopt, family, variant):
    """A batch of one — every lane searches, so the full-size pairs take the packed walks and the twelve rows of ``small``
    the branching ones; the targets of 2 049 and 4 097 rows the exact walks (LDS copy, then L2).  Sorted along a
    projection (ICPMI_POLAR=0), by bearing (2; the library sorts targets above 2 048 rows along a projection whatever the
    option says, csrc/prep.hip) and as the library chooses: the same bytes, twice."""
    from icpmi import batch
    rows = len(pair(family, variant)[1])
    got = {}
    for mode in ("0", "2", None):
        libopt.setenv("ICPMI_POLAR", mode) if mode else libopt.delenv("ICPMI_POLAR")
        b = _batch(family, variant)
        assert b.fast
        got[mode] = _records(b)
        word = int(b.direction_words()[0])
        bearing_allowed = mode != "0" and rows <= 2048
        assert (word == 4) if (mode == "2" and bearing_allowed) else (0 <= word <= (4 if bearing_allowed else 3)), (mode, word)
        assert _records(b).tobytes() == got[mode].tobytes(), mode              # a run repeated
    assert got["0"].tobytes() == got["2"].tobytes() and got["0"].tobytes() == got[None].tobytes()
    ref = _reference(family, variant, b)
    slow = _batch(family, variant, force_exhaustive=True)
    assert not slow.fast
    exh = _records(slow)
    Rf, tf, _, inf_ = batch.unpack_results(got["0"], 2)
    Rs, ts, _, ins = batch.unpack_results(exh, 2)
    assert np.array_equal(inf_["iters"], ins["iters"]) and np.array_equal(inf_["status"], ins["status"])
    diffs = (np.abs(Rf - Rs).max(), np.abs(tf - ts).max())
    print(f"\n{family}/{variant}: fused - exhaustive R {diffs[0]:.3g} t {diffs[1]:.3g}; fused - oracle "
          f"{rot_err(Rf[0], tf[0], ref[0], ref[1]):.3g}; exhaustive - oracle {rot_err(Rs[0], ts[0], ref[0], ref[1]):.3g}")
    assert diffs[0] < 1e-12 and diffs[1] < 1e-12, diffs
    _against_oracle(got["0"], ref, "fused")
    _against_oracle(exh, ref, "exhaustive")


def test_the_pairs_are_sorted_along_every_projection(libopt):
    """What the run above covers: with ICPMI_POLAR=0 the prepare kernel picks each of x, y, x + y, x - y for some pair."""
    libopt.setenv("ICPMI_POLAR", "0")
    seen = {}
    for family, variant in all_pairs():
        b = _batch(family, variant)
        b.prepare()
        seen[family, variant] = int(b.direction_words()[0])
    assert set(seen.values()) == {0, 1, 2, 3}, seen


@pytest.mark.parametrize("family", list(FAMILIES))
def test_company_does_not_matter(family):
    """Twelve rows search in a wave of their own (the branching filter walks); eighty such pairs in one batch give the
    record of the single run bit for bit."""
    single = _batch(family, "small")
    one = _records(single)
    many = _records(_batch(family, "small", copies=80))
    assert many.shape[0] == 80 and all(many[i].tobytes() == one[0].tobytes() for i in range(80))
    _against_oracle(many, _reference(family, "small", single), "80 copies")


@pytest.mark.parametrize("variant", ["base", "pad2048"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_far_continuation_keeps_every_near_tie(libopt, family, variant):
    """The box hierarchy of the far continuation (sweepf_top2_far) runs iterations 2 on when the first step leaves a mean
    squared error above ICP2_FAR: 1e-12 sends these pairs (the workspace counter shows it).  The records of the plain
    path (ICP2_FAR = 0), byte for byte, on the smallest target and on the largest the continuation holds.  (The 616 rows
    of the lattice pair are two rows for some threads of the 512-thread launch and one row each for the continuation's
    1 024: the sums of a step must still be taken in the same order, csrc/icp2.hip, Icp2Args::far_row_threads.)"""
    out, sent = {}, {}
    for far in ("0", "1e-12"):
        libopt.setenv("ICP2_FAR", far)
        b = _batch(family, variant)
        b.icp_ws.zero_()                                                    # a launch that parks nobody leaves the counters alone
        out[far] = _records(b)
        sent[far] = _far_count(b)
    assert sent == {"0": 0, "1e-12": 1}, sent
    assert out["0"].tobytes() == out["1e-12"].tobytes()
    _against_oracle(out["1e-12"], _reference(family, variant, b), "far")
