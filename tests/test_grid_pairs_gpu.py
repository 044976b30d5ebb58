"""The four entries that hold a list of (cloud, pose) pairs against the occupancy grid — the exhaustive match, the wide
search, the check and the beam model (icpmi.gridmatch: GridMatchBatch, GridSearchBatch, check_pairs, beam_pairs) — judge
ONE pair list alike: the same status for every pair, and the same rows with cells wherever a pair is read.  Each family's
own suite compares its records bit for bit against its restatement; this holds the four against each other on one cloud
set with device counts (a short one, the voxel filter's overflow mark, one above its cap), a cloud that crosses a chunk
of 256 rows, a pose that puts its scan off the grid and a pose that is not finite."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPS = (0, 1, 257, 300)                                        # rows of the four clouds; 257 crosses a chunk of 256
COUNTS = (1, -1, 257, 258)                                     # above its cap, the overflow mark, full, short
PAIRS = (2, 3, 0, 1, 2, 3, 2, 3)                               # every cloud is named
NY, NX, RES, MIN_X, MIN_Y, K, THRESHOLD = 64, 96, 0.1, -4.8, -3.2, 10, 1024


def test_the_four_entries_judge_one_pair_list_alike():
    import torch
    from icpmi import _lib, gridmatch
    from icpmi.batch import CloudSet
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    rng = np.random.default_rng(58)
    # rows on a ring of 1 to 3 m about the sensor: none at its origin, where the beam model has no far end
    bearing, r = rng.uniform(-np.pi, np.pi, sum(CAPS)), rng.uniform(1.0, 3.0, sum(CAPS))
    pts = np.stack([r * np.cos(bearing), r * np.sin(bearing)], axis=1)
    off = np.concatenate([[0], np.cumsum(CAPS)]).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    cs = CloudSet(torch.from_numpy(pts).to(dev), off, cnt=torch.tensor(COUNTS, dtype=torch.int32, device=dev))
    # the map: observed free space, one wall, a band nobody has seen
    field = np.full((NY, NX), -512, dtype=np.int16)
    field[:, 70] = 4096
    field[:8] = 0
    fld = torch.from_numpy(field).to(dev)
    grid = types.SimpleNamespace(device_log_odds=torch.zeros((NY, NX), dtype=torch.float32, device=dev), min_x=MIN_X, min_y=MIN_Y,
                                 resolution=RES, log_odds_min=-5.0, log_odds_max=5.0)
    pair = np.array(PAIRS, dtype=np.int32)
    B = len(pair)
    t = rng.uniform(-1.0, 1.0, (B, 2))
    theta = rng.uniform(-np.pi, np.pi, (B, 1))
    t[4] = (1000.0, -1000.0)                                       # the whole scan off the grid: its rows still have cells
    t[5] = (np.nan, 0.0)                                           # no row has a cell
    cos_sin = np.concatenate([np.cos(theta), np.sin(theta)], axis=1)

    match = gridmatch.GridMatchBatch(grid, cs, pair, t, theta, 0, field=(fld, K))
    search = gridmatch.GridSearchBatch(grid, cs, pair, t, theta, 0, block=4, field=(fld, K))
    checked, _ = gridmatch.check_pairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, pair, t, cos_sin, 2)
    beamed, _, _ = gridmatch.beam_pairs(fld, THRESHOLD, MIN_X, MIN_Y, RES, cs, pair, t, cos_sin, gridmatch.beam_table(RES, RES, 8), 8, 1.5)
    rec = {"match": match.run().cpu().numpy()[:B], "search": search.run().cpu().numpy()[:B], "check": checked.cpu().numpy(),
           "beam": beamed.cpu().numpy()}
    status = {"match": _lib.GMREC_STATUS, "search": _lib.GMREC_STATUS, "check": _lib.GK_REC_STATUS, "beam": _lib.GB_REC_STATUS}
    rows = {"match": _lib.GMREC_ROWS, "check": _lib.GK_REC_ROWS, "beam": _lib.GB_REC_ROWS}

    # what the counts imply: a count that is negative or above the cloud's cap is not read; else any row with a cell decides
    n = np.array([c if 0 <= c <= cap else -1 for c, cap in zip(COUNTS, CAPS)])[pair]
    with_cells = np.where(np.isfinite(t).all(axis=1), n, 0)
    want = np.where(n < 0, _lib.GM_ST_CAPACITY, np.where(with_cells > 0, _lib.GM_ST_OK, _lib.GM_ST_EMPTY))
    assert want.tolist() == [0, 0, 2, 2, 0, 1, 0, 0] == [_lib.GM_ST_OK] * 2 + [_lib.GM_ST_CAPACITY] * 2 + [_lib.GM_ST_OK, _lib.GM_ST_EMPTY] + [_lib.GM_ST_OK] * 2
    for name, slot in status.items():
        print(name, "status", rec[name][:, slot].tolist())
        assert np.array_equal(rec[name][:, slot], want), name
    ok = want == _lib.GM_ST_OK
    for name, slot in rows.items():
        print(name, "rows with cells", rec[name][:, slot].tolist())
        assert np.array_equal(rec[name][ok, slot], rec["match"][ok, rows["match"]]), name
    assert np.array_equal(rec["match"][ok, rows["match"]], with_cells[ok])
