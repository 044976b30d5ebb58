"""The ray-cast (csrc/raycast.hip) outside the envelope of tests/test_gpu_parity.py — hits on cell borders, beams of up to 2^29
cells, coordinates beyond the clamp, scans at the limit of a 16-bit counter, and the H / M replay on start values, clamps and
probabilities that reach each of its exits — under its three counting passes, bit for bit against the project's C oracle
(oracle.grid_update_scan).  The inputs are those of tests/raycast_cases.py; tests/test_raycast_edges_cpu.py proves without a
GPU that each has its property and takes the pass its id names.  No tolerance anywhere: the comparison is of bit patterns
(``raycast_cases.same_bits``; a NaN cell is only required to be NaN).  Expected grids are computed once per module."""
import functools

import numpy as np
import pytest

import raycast_cases as rc

pytestmark = pytest.mark.gpu

PASSES = ("tiles", "atomic", "owner")


@pytest.fixture(scope="module")
def umap():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from utilities import mapping
    return mapping


@pytest.fixture(params=PASSES)
def raypath(request, libopt):
    """tiles: counters per 64 x 64 tile in LDS; atomic: an atomic per (wave, cell) on the scan's counter region; owner: the
    single launch of a live scan (replays, bands and uploaded grids take their default pass under it)"""
    libopt.setenv("ICPMI_RAYCAST", request.param)
    return request.param


want = functools.lru_cache(maxsize=None)(lambda key: EXPECTED[key]())
EXPECTED = {}                          # key -> a function that computes the oracle's answer; evaluated once, shared by the passes
SEEN = {}                              # (family, case) -> {pass: bytes of the grid}, for the agreement tests at the end


def _grid(umap, case, start=None):
    g = umap.OccupancyGrid2D(*rc.bounds(case.grid), resolution=case.grid.res, **case.kw)
    assert (g.ny, g.nx) == (case.grid.ny, case.grid.nx)
    if start is not None:
        g.log_odds = start
    return g


def _note(family, name, raypath, grid):
    grid = np.where(np.isnan(grid), np.float32(np.nan), grid)           # a NaN cell is only required to be NaN
    SEEN.setdefault((family, name), {})[raypath] = np.ascontiguousarray(grid, dtype=np.float32).tobytes()


def _ids(cases):
    return [c.name for c in cases]


# ── A, B, C: the live path, scan by scan ────────────────────────────────────────────────────────────────────────────────
LIVE = rc.border_cases() + rc.long_cases() + [rc.clamp_case()]
for _c in LIVE:
    EXPECTED["live", _c.name] = functools.partial(rc.expected, _c, snapshots=True)


@pytest.mark.parametrize("case", LIVE, ids=_ids(LIVE))
def test_live_scans(umap, raypath, case):
    g = _grid(umap, case)
    for s, ref in zip(case.scans, want(("live", case.name))):
        g.update_scan(s.origin, s.hits)
        assert rc.same_bits(g.log_odds, ref), (case.name, s.name)
    _note("live", case.name, raypath, g.log_odds)


# ── B in bands: rows outside the band untouched ─────────────────────────────────────────────────────────────────────────
def _band_start(g, rows):
    """random values (inside KW's clamps) outside the band, where nothing may be written; zeros inside it, so that the band's
    rows are those of the live test's last grid — cells are independent, and the oracle walks the long beams once"""
    start = np.random.default_rng(11).uniform(-150.0, 150.0, size=(g.ny, g.nx)).astype(np.float32)
    start[rows[0]:rows[1]] = 0.0
    return start


@pytest.mark.parametrize("rows", [(40, 97), (0, 1)], ids=["rows40_97", "rows0_1"])
@pytest.mark.parametrize("case", rc.long_cases(), ids=_ids(rc.long_cases()))
def test_long_beams_in_a_band(umap, raypath, case, rows):
    if rows[1] > case.grid.ny:
        rows = (0, 1)                                                    # the 130 x 1 sliver has one row: its band is the grid
    start = _band_start(case.grid, rows)
    g = _grid(umap, case, start)
    g.update_scans(np.array([s.origin for s in case.scans]), [s.hits for s in case.scans], rows=rows)
    ref = start.copy()
    ref[rows[0]:rows[1]] = want(("live", case.name))[-1][rows[0]:rows[1]]
    got = g.log_odds
    outside = np.ones(case.grid.ny, dtype=bool)
    outside[rows[0]:rows[1]] = False
    assert rc.same_bits(got[outside], start[outside]), "rows outside the band were written"
    assert rc.same_bits(got, ref)
    _note("band", f"{case.name}_{rows}", raypath, got)


# ── B and C in a replay: three scans, one call ──────────────────────────────────────────────────────────────────────────
for _c in rc.replays():
    EXPECTED["replay", _c.name] = functools.partial(rc.expected, _c)


@pytest.mark.parametrize("case", rc.replays(), ids=_ids(rc.replays()))
def test_replay_of_the_longest_scans(umap, raypath, case):
    g = _grid(umap, case)
    g.update_scans(np.array([s.origin for s in case.scans]), [s.hits for s in case.scans])
    assert rc.same_bits(g.log_odds, want(("replay", case.name)))
    _note("replay", case.name, raypath, g.log_odds)


# ── D: 65 535, 65 536 and 65 537 beams through one cell ─────────────────────────────────────────────────────────────────
COUNTERS = [rc.counter_case(nb) for nb in rc.COUNTER_BEAMS]
for _c in COUNTERS + [rc.counter_replay_case()]:
    EXPECTED["counter", _c.name] = functools.partial(rc.expected, _c)


@pytest.mark.parametrize("case", COUNTERS, ids=_ids(COUNTERS))
def test_counter_limit_alone(umap, raypath, case):
    g = _grid(umap, case)
    g.update_scan(case.scans[0].origin, case.scans[0].hits)
    assert rc.same_bits(g.log_odds, want(("counter", case.name)))
    _note("counter", case.name, raypath, g.log_odds)


def test_counter_limits_in_one_replay(umap, raypath):
    case = rc.counter_replay_case()
    g = _grid(umap, case)
    g.update_scans(np.array([s.origin for s in case.scans]), [s.hits for s in case.scans])
    assert rc.same_bits(g.log_odds, want(("counter", case.name)))
    _note("counter", case.name, raypath, g.log_odds)


# ── E: the replay arithmetic ────────────────────────────────────────────────────────────────────────────────────────────
REPLAYS = rc.replay_cases()
for _c, _s in REPLAYS:
    EXPECTED["arith", _c.name] = functools.partial(rc.expected, _c, _s)


@pytest.mark.parametrize("case,start", REPLAYS, ids=[c.name for c, _ in REPLAYS])
def test_replay_arithmetic(umap, raypath, case, start):
    g = _grid(umap, case, start)
    assert rc.same_bits(g.log_odds, start)                               # the upload keeps -0.0, the infinities and NaN
    g.update_scan(case.scans[0].origin, case.scans[0].hits)
    assert rc.same_bits(g.log_odds, want(("arith", case.name))), case.name
    _note("arith", case.name, raypath, g.log_odds)


# ── a refusal comes before the first launch ─────────────────────────────────────────────────────────────────────────────
def test_a_bad_last_scan_is_refused_before_anything_is_started(umap, raypath):
    """Four scans of two beams inside an 8 x 8 grid, no box (groups of two), and offsets whose LAST count is negative: the
    entry refuses the call as a whole, so the grid keeps its start values bit for bit and the workspace stays all zero (a
    refusal met after the first group was counted left its counters and a box slot behind).  All 8 rows of `hits` exist, so
    whatever reads them reads inside the allocation."""
    import torch
    import icpmi
    L = icpmi.lib()
    rng = np.random.default_rng(23)
    start = torch.from_numpy(rng.uniform(-4.0, 4.0, size=(8, 8)).astype(np.float32)).cuda()
    grid = start.clone()
    ws = torch.zeros(L.icpmi_grid_workspace_bytes(8, 8), dtype=torch.uint8, device="cuda")
    origins = torch.from_numpy(rng.uniform(1.0, 7.0, size=(4, 2))).cuda()
    hits = torch.from_numpy(rng.uniform(1.0, 7.0, size=(8, 2))).cuda()
    off = np.array([0, 2, 4, 6, 5], dtype=np.int32)
    code = L.icpmi_grid_update_scans_box(grid.data_ptr(), ws.data_ptr(), 8, 8, 0.0, 0.0, 1.0, origins.data_ptr(), hits.data_ptr(),
                                         off.ctypes.data, 4, 0.9, -0.4, -8.0, 8.0, 0, 0, 0, 8, None,
                                         torch._C._cuda_getCurrentRawStream(grid.device.index))
    torch.cuda.synchronize()
    assert code == -1                                                    # ICPMI_ERR_ARG
    assert torch.equal(grid.view(torch.int32), start.view(torch.int32)), "a refused call wrote the grid"
    assert int(ws.count_nonzero()) == 0, "a refused call left counts or a box in the workspace"


# ── the three passes agree: a failure above names the pass, this one names the family ───────────────────────────────────
@pytest.mark.parametrize("family", ["live", "band", "replay", "counter", "arith"])
def test_the_three_passes_wrote_the_same_bytes(family):
    runs = {k: v for k, v in SEEN.items() if k[0] == family}
    assert runs, "runs after the tests of the family, in the same session"
    for key, by_pass in runs.items():
        assert set(by_pass) == set(PASSES), (key, sorted(by_pass))
        assert len(set(by_pass.values())) == 1, key
