"""A rotation-search record is the same bits run after run.  The pruned coarse sweep scores a few angles more or fewer
depending on when the waves of a workgroup see each other's results (csrc/rotsearch.hip), so the record counts the angles
every schedule scores — those whose bound does not exceed the winning score, and the first of each wave — not the ones a
run happened to score.  With
the count of a run in that slot, one pair in some hundreds changed it from one run to the next (14 or 15), and every test
that compares two runs' records bit for bit failed now and then.

The 1 100 pairs of tests/test_history_gpu.py::test_1100_pairs_take_the_two_stage_launch, 256-beam scans; built once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUNS = 12


def test_search_records_do_not_change_from_run_to_run():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib, synth
    from utilities import features
    import test_history_gpu as T
    features.VERBOSE = False
    poses = synth.trajectory(12, start=(-8.0, -0.5, 0.0), step=0.3)
    small = [synth.scan(p, 4300 + i, n_beams=256) for i, p in enumerate(poses)]
    h = T.new_history()
    h.add_many(small)
    cands = (np.arange(1100) * 7) % 11
    _, first, batch = T.batch_path(small[11], [small[k] for k in cands])
    _, rec, match = T.resident(h, 11, cands)
    assert np.array_equal(rec, first, equal_nan=True)
    evals, n_coarse = first[:, _lib.RSBREC_EVALS], len(batch.search.tables.coarse)
    assert (first[:, _lib.RSBREC_STATUS] == _lib.RSB_ST_OK).all()
    assert (evals >= 1).all() and (evals < n_coarse).all()                  # pruned
    # the same target gives the same record wherever it stands in the batch
    for k in range(11):
        same = first[cands == k]
        assert np.array_equal(same, np.broadcast_to(same[0], same.shape), equal_nan=True), k
    for run in range(RUNS):
        batch.search.run()
        match.search.run()
        torch.cuda.synchronize()
        for what, job in (("batch", batch), ("resident", match)):
            again = job.search.records.cpu().numpy()[:1100]
            bad = np.argwhere(~((again == first) | (np.isnan(again) & np.isnan(first))))
            assert len(bad) == 0, (what, run, [(int(r), int(c), again[r, c], first[r, c]) for r, c in bad[:5]])
