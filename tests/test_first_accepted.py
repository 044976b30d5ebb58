"""Stopping batched loop-closure matching after the first accepted candidate (slam.py:582-597, include/icpmi.h
icpmi_icp_batch_gated).  Every batch runs twice, ungated and gated, and the gated run must keep the contract:

- the same first accepted index F (err < gate, rotation search usable; -1: none);
- every candidate up to F (all of them when F = -1) equal to the full run in all 16 doubles of its record;
- every candidate after F either equal to the full run or SKIPPED (status 5).
"""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

ICP = dict(error_threshold=1e-10, max_iterations=150, voxel_size=0.04, method="point_to_line", normal_k=12)
FEAT = dict(rotation_voxel_size=0.15, angle_step_coarse=1.5, angle_step_fine=0.1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import features
    features.VERBOSE = False


def records(R, t, err, info):
    from icpmi.dist import _pack_results
    return _pack_results(R, t, err, info)


def run_icp_pairs(src, tgts, gate, stop, max_rows_hint=1024, feat=FEAT, icp=ICP):
    """(records [B,16], first_accepted, RunIcpPairBatch) of the candidates tgts of one current scan."""
    from icpmi import prealign
    B = len(tgts)
    b = prealign.RunIcpPairBatch([src] + list(tgts), np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32),
                                 max_rows_hint=max_rows_hint, stop_after_first_accepted=stop, error_accept=gate, **feat, **icp)
    b.run()
    R, t, err, info = b.unpack()
    return records(R, t, err, info), info["first_accepted"], b


def check_contract(full, gated, F_full, F_gated):
    assert F_gated == F_full, (F_gated, F_full)
    upto = len(full) if F_full < 0 else F_full + 1
    assert np.array_equal(full[:upto], gated[:upto], equal_nan=True)
    for i in range(upto, len(full)):
        if gated[i, 15] != 5:
            assert np.array_equal(full[i], gated[i], equal_nan=True), i
    return int((gated[:, 15] == 5).sum())


def test_512_far_candidates_stop_after_the_first_accepted(gpu):
    """The bench's 3 m / 20 degree candidates (config5_run_icp_pair_512_3m_20deg) under config.yaml's gate 0.08: the gate
    must act — candidates are skipped and the batch does fewer iterations in all."""
    from icpmi import synth
    srcs, tgts = synth.loop_closure_batch(512, seed0=7000, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
    full, F, _ = run_icp_pairs(srcs[0], tgts, 0.08, False)
    gated, Fg, b = run_icp_pairs(srcs[0], tgts, 0.08, True)
    assert F >= 0
    skipped = check_contract(full, gated, F, Fg)
    assert skipped >= 1
    assert gated[:, 14].sum() < full[:, 14].sum()
    assert b.first_accepted() == F
    b.run()                                                            # repeated: the gate word starts afresh
    assert b.first_accepted() == F


def test_five_candidates_as_slam_py_tries_them(gpu):
    """The slam.py shape (config.yaml max_candidates 5) over several seeds, among them ones where candidate 0 is rejected
    and a later one accepted."""
    from icpmi import synth
    seen = set()
    for seed in (100, 197, 294, 391, 682, 1749, 2040, 2913):          # the reference's F: 0, 2, 1, 0, 4, 4, 2, 2
        srcs, tgts = synth.loop_closure_batch(5, seed0=seed, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
        full, F, _ = run_icp_pairs(srcs[0], tgts, 0.08, False)
        gated, Fg, _ = run_icp_pairs(srcs[0], tgts, 0.08, True)
        check_contract(full, gated, F, Fg)
        seen.add("later" if F > 0 else ("first" if F == 0 else "none"))
    assert {"later", "first"} <= seen, seen


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
def test_two_stages_and_far_continuation(gpu, libopt, method):
    """About 1 100 pairs with the two-stage run forced on (ICP2_STAGES=2) and the far continuation on (ICP2_FAR 0.04):
    first stage, second stage and far kernel all honour the gate; no rotation search (every pair eligible)."""
    import torch
    from icpmi import batch, synth
    B = 1100
    srcs, tgts = synth.loop_closure_batch(B, seed0=4300, shared_source=True, max_offset=2.0, max_yaw_deg=12.0)
    srcs, tgts = [c[::4] for c in srcs], [c[::4] for c in tgts]
    libopt.setenv("ICP2_STAGES", "2")
    libopt.setenv("ICP2_FAR", "0.04")
    clouds = [srcs[0]] + tgts
    b = batch.IcpBatch(clouds, np.zeros(B, dtype=np.int32), np.arange(1, B + 1, dtype=np.int32), 1e-10, 40, 0.04,
                       None, None, method, 12)
    full = b.run().cpu().numpy()[:B].copy()
    err = full[:, 12]
    gate = float(np.median(err))
    F = int(np.flatnonzero(err < gate)[0])
    b.set_gate(gate)
    gated = b.run().cpu().numpy()[:B].copy()
    Fg = int(b.first_accepted_dev.item())
    assert check_contract(full, gated, F, Fg) >= 1, method
    b.set_gate(None)                                                   # ungated again: the same bits as before
    assert np.array_equal(b.run().cpu().numpy()[:B], full)
    torch.cuda.synchronize()


def test_nothing_accepted_skips_nothing(gpu):
    from icpmi import synth
    srcs, tgts = synth.loop_closure_batch(64, seed0=7000, shared_source=True, max_offset=3.0, max_yaw_deg=20.0)
    full, F, _ = run_icp_pairs(srcs[0], tgts, 0.0, False)
    gated, Fg, _ = run_icp_pairs(srcs[0], tgts, 0.0, True)
    assert F == -1 and Fg == -1
    assert np.array_equal(full, gated, equal_nan=True)


def test_capacity_candidates_are_redone_up_to_the_first_accepted(gpu):
    """Every candidate beyond the capacity hint of the batched search (status 2): their device ICP starts from the wrong
    pose and never counts; unpack() redoes them on the host in order and stops at the first accepted one."""
    from icpmi import synth
    srcs, tgts = synth.loop_closure_batch(6, seed0=300, shared_source=True)
    feat = dict(rotation_voxel_size=0.05, angle_step_coarse=4.0, angle_step_fine=0.5)
    icp = dict(error_threshold=1e-10, max_iterations=60, voxel_size=0.04, method="point_to_line", normal_k=12)
    full, _, b = run_icp_pairs(srcs[0], tgts, 1.0, False, max_rows_hint=256, feat=feat, icp=icp)
    assert (b.search.records.cpu().numpy()[:6, 11] == 2).all()
    err = full[:, 12]
    gate = float(err.min()) * 1.0000001
    F = int(np.flatnonzero(err < gate)[0])
    full2, F2, _ = run_icp_pairs(srcs[0], tgts, gate, False, max_rows_hint=256, feat=feat, icp=icp)
    assert F2 == F and np.array_equal(full, full2)
    gated, Fg, bg = run_icp_pairs(srcs[0], tgts, gate, True, max_rows_hint=256, feat=feat, icp=icp)
    check_contract(full, gated, F, Fg)
    assert (gated[F + 1:, 15] == 5).all()                              # not redone after the accepted one
    assert bg.first_accepted() == F


def test_reference_cases_first_accepted(gpu):
    """tests/golden/run_icp_pair.npz: the gated run's first accepted candidate is the first whose REFERENCE error is below
    the gate of config.yaml (0.08)."""
    from icpmi import prealign
    from test_oracle_golden import run_icp_pair_cases
    cases = list(run_icp_pair_cases())
    z = load_golden("run_icp_pair")
    ref = np.array([float(z[f"p{c[0]}__err"]) for c in cases])
    ok = np.flatnonzero(ref < 0.08)
    want = int(ok[0]) if len(ok) else -1
    icp_cfg, feat_cfg = cases[0][4], cases[0][5]
    tg = [c[2] for c in cases]
    Rf, tf, ef, inf_ = prealign.run_icp_pair_batch(cases[0][1], tg, icp_cfg, feat_cfg, error_accept=0.08)
    Rg, tgt_, eg, ing = prealign.run_icp_pair_batch(cases[0][1], tg, icp_cfg, feat_cfg, error_accept=0.08,
                                                    stop_after_first_accepted=True)
    assert inf_["first_accepted"] == want and ing["first_accepted"] == want
    check_contract(records(Rf, tf, ef, inf_), records(Rg, tgt_, eg, ing), want, ing["first_accepted"])
