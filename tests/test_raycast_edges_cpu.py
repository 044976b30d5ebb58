"""The inputs of tests/raycast_cases.py have the properties tests/test_raycast_edges_gpu.py relies on — shown here without a
GPU, from the project's C oracle alone (oracle.grid_update_scan walks every cell in int64 with the reference's loop) — and
take the counting pass their test id names (icpmi_grid_update_plan: the library's own plan, no HIP call).  Five wrong
models, NumPy restatements only, each differ from the oracle on the family meant to catch them.  A minimum count is a
condition on the inputs: a generator that falls short fails here, nothing is skipped."""
import ctypes as C

import numpy as np
import pytest

import oracle
import raycast_cases as rc


def _cells(pairs):
    return np.array(pairs, dtype=np.int64).reshape(-1, 2)


# ── the grids and the conversion ────────────────────────────────────────────────────────────────────────────────────────
def test_grids_have_the_cells_they_name():
    for g in [rc.DEFAULT, rc.OFFSET, rc.SLIVER_X, rc.SLIVER_Y, rc.REPLAY_GRID] + [rc.border_grid(r) for r in rc.BORDER_RES]:
        assert rc.shape(g) == (g.ny, g.nx), g.name
    assert rc.bounds(rc.DEFAULT)[0] == 0.0 and rc.shape(rc.DEFAULT) == (150, 200)
    assert (rc.DEFAULT.nx % 64, rc.DEFAULT.ny % 64) == (8, 22)           # neither extent a multiple of the tile


def test_cell_centres_convert_to_their_cells():
    """min + (cell + 0.5) * res is that cell for the oracle, on every grid, up to 10^15 cells away"""
    far = [0, 1, -1, 199, 1000, -65537, 10 ** 6, -2 * 10 ** 7, 4 * 10 ** 8 + 3, -(4 * 10 ** 8 - 3), rc.LIM - 1, -(rc.LIM - 1), rc.LIM,
           -rc.LIM, rc.BEYOND, -rc.BEYOND, 10 ** 10, -10 ** 15]
    for g in (rc.DEFAULT, rc.OFFSET, rc.SLIVER_X):
        c = _cells([(a, b) for a in far for b in far])
        assert np.array_equal(rc.cells_of(g, rc.world(g, c[:, 0], c[:, 1])), c), g.name


# ── A ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", rc.border_cases(), ids=lambda c: c.name)
def test_border_hits_change_cell_under_the_reciprocal(case):
    g = case.grid
    changed = sum(int((rc.cells_of(g, s.hits) != rc.cells_by_reciprocal(g, s.hits)).any(axis=1).sum()) for s in case.scans)
    if g.res == 0.25:
        assert changed == 0                                              # a power of two: the reciprocal is exact
        return
    assert changed >= 100, changed
    # wrong model: the grid the reciprocal index gives is not the oracle's
    want = rc.expected(case)
    wrong = np.zeros_like(want)
    for s in case.scans:
        o = rc.cells_by_reciprocal(g, s.origin)[0]
        oracle.grid_update_scan(wrong, 0.0, 0.0, 1.0, o + 0.5, rc.cells_by_reciprocal(g, s.hits) + 0.5, rc.l_of(case.kw["p_hit"]),
                                rc.l_of(case.kw["p_miss"]), case.kw["log_odds_min"], case.kw["log_odds_max"])
    assert not rc.same_bits(wrong, want)


def test_border_origins_and_tiny_coordinates():
    for case in rc.border_cases():
        g = case.grid
        centre, corner = case.scans
        assert np.array_equal(rc.cells_of(g, centre.origin)[0], [g.nx // 2, g.ny // 2])
        assert corner.origin[0] == g.min_x + (g.nx // 2) * g.res and corner.origin[1] == g.min_y + (g.ny // 2) * g.res
        beams = np.abs(rc.cells_of(g, centre.hits) - rc.cells_of(g, centre.origin)).max(axis=1)
        assert beams.max() <= 25                                         # hits spread over the grid, short beams
        inside = rc.cells_of(g, centre.hits)
        assert len(np.unique(inside, axis=0)) > 300
    g = rc.border_grid(0.05)
    assert g.min_x == 0.0
    assert oracle.world_to_grid(rc.TINY, 0.0, 0.05).tolist() == [0, 0, 0, -1, 0, -1]
    hits = rc.border_case(0.05).scans[0].hits
    for t in rc.TINY:                                                    # present on both axes, bit for bit
        for a in (0, 1):
            assert (hits[:, a].view(np.uint64) == np.float64(t).view(np.uint64)).any(), (t, a)


# ── B ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_long_beams_have_every_length_and_octant():
    case = rc.long_case("default")
    g = case.grid
    inside = case.scans[0]
    o = rc.cells_of(g, inside.origin)[0]
    d = rc.cells_of(g, inside.hits) - o
    dmaj, dmin = np.abs(d).max(axis=1), np.abs(d).min(axis=1)
    octant = (d[:, 0] > 0).astype(int) + 2 * (d[:, 1] > 0) + 4 * (np.abs(d[:, 1]) > np.abs(d[:, 0]))
    for n in rc.LENGTHS + (rc.LIM - 1 - int(o[0]),):
        assert (dmaj == n).any(), n
    for n in rc.LENGTHS[:4]:
        assert {0, 1, n - 1, n} <= set(dmin[dmaj == n].tolist()), n
        assert any(np.gcd(int(m), n) == 1 and 1 < m < n - 1 for m in dmin[dmaj == n]), n
    for n in rc.LENGTHS:
        assert len(set(octant[(dmaj == n) & (dmin > 0) & (dmin < n)].tolist())) >= (8 if n <= 65537 else 4), n
    assert (dmaj >= rc.LIM - 1 - 77).sum() == 4                          # to the last unclamped cell on each side
    assert np.abs(rc.cells_of(g, inside.hits)).max() < rc.LIM           # nothing of B is clamped
    for c in rc.long_cases():
        for s in c.scans:
            assert np.abs(rc.cells_of(c.grid, s.hits)).max() < rc.LIM and np.abs(rc.cells_of(c.grid, s.origin)).max() < rc.LIM


def test_long_beam_subfamilies_hold_32_beams_each():
    """counted from the oracle's walk of each beam on its own (raycast_cases.classify)"""
    total = dict.fromkeys(rc.SUBFAMILIES, 0)
    for name in ("default", "offset", "sliver_130x1", "sliver_1x130"):
        for k, v in rc.classify(name).items():
            total[k] += int(v)
    for k in rc.SUBFAMILIES:
        assert rc.classify("default")[k] >= 32, (k, rc.classify("default"))
        assert total[k] >= 32
    for name in ("sliver_130x1", "sliver_1x130"):                        # a sliver is mostly grazed
        assert rc.classify(name)["grazes"] >= 32 and rc.classify(name)["near_miss"] >= 32


def test_oracle_walks_stay_within_the_budget():
    """one pass over every scan of B and C; the GPU module makes about two (the live path, the replay of the longest scans)"""
    total = sum(rc.walk_length(c) for c in rc.long_cases()) + rc.walk_length(rc.clamp_case())
    assert total <= rc.WALK_BUDGET, total
    long_beams = 0
    for c in rc.long_cases() + [rc.clamp_case()]:
        for s in c.scans:
            o = np.clip(rc.cells_of(c.grid, s.origin)[0], -rc.LIM, rc.LIM)
            h = np.clip(rc.cells_of(c.grid, rc.keep_finite(c.grid, s.hits)), -rc.LIM, rc.LIM)
            long_beams += int((np.abs(h - o).max(axis=1) >= 4 * 10 ** 8 - 3).sum())
    assert long_beams <= 17, long_beams


# ── C ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_clamp_case_is_what_it_says():
    case, want_case = rc.clamp_case(), rc.clamp_expected_case()
    g = case.grid
    near, far = case.scans
    kept = rc.keep_finite(g, near.hits)
    assert len(kept) == len(near.hits) - 2                               # 1e301 m and 1.7e308 m: quotients not below 1e300
    with np.errstate(over="ignore"):
        dropped = [h for h in near.hits if not (np.abs(np.floor((h - [g.min_x, g.min_y]) / g.res)) < rc.DROP_QUOTIENT).all()]
    assert sorted(float(np.abs(h).max()) for h in dropped) == [1e301, 1.7e308]
    cells = rc.cells_of(g, kept)
    assert sorted(np.abs(cells).max(axis=1).tolist())[-3:] == [10 ** 10, 10 ** 15, 10 ** 15]
    assert (np.abs(cells) == rc.BEYOND).sum() == 2
    assert rc.cells_of(g, far.origin)[0].tolist() == [rc.BEYOND, 10 ** 10]
    # the replacement is the cell +-2^29 and leaves every other coordinate alone
    for s, w in zip(case.scans, want_case.scans):
        c, cw = rc.cells_of(g, rc.keep_finite(g, s.hits)), rc.cells_of(g, w.hits)
        assert np.array_equal(cw, np.clip(c, -rc.LIM, rc.LIM))
        assert np.array_equal(w.hits[np.abs(c) <= rc.LIM], rc.keep_finite(g, s.hits)[np.abs(c) <= rc.LIM])
        assert np.array_equal(rc.cells_of(g, w.origin)[0], np.clip(rc.cells_of(g, s.origin)[0], -rc.LIM, rc.LIM))
    assert rc.cells_of(g, want_case.scans[1].origin)[0].tolist() == [rc.LIM, rc.LIM]


def _tiles(cells):
    return {(x // 64, y // 64) for x, y in cells}


def test_clamped_and_true_lines_cross_different_tiles():
    """wrong model: the unclamped direction, cut to the first 2^29 steps, against the oracle on the clamped cells"""
    case, want_case = rc.clamp_case(), rc.clamp_expected_case()
    g = case.grid
    differing = 0
    for s, w in zip(case.scans, want_case.scans):
        o, ow = rc.cells_of(g, s.origin)[0], rc.cells_of(g, w.origin)[0]
        for h, hw in zip(rc.cells_of(g, rc.keep_finite(g, s.hits)), rc.cells_of(g, w.hits)):
            if np.abs(h).max() <= rc.LIM and np.abs(o).max() <= rc.LIM:
                continue
            one = np.zeros((g.ny, g.nx), dtype=np.float32)
            oracle.grid_update_scan(one, 0.0, 0.0, 1.0, ow + 0.5, [hw + 0.5], 0.0, 1.0, -1e9, 1e9)
            clamped = {(int(x), int(y)) for y, x in zip(*np.nonzero(one))}
            true = rc.unclamped_cells_in_grid(g, [int(v) for v in o], [int(v) for v in h])
            assert clamped and _tiles(clamped) != _tiles(true), (o, h)
            differing += 1
    assert differing == 5


# ── D ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_counter_limits_show_in_the_grid():
    grids = {nb: rc.expected(rc.counter_case(nb)) for nb in (65534,) + rc.COUNTER_BEAMS + (65538,)}
    for nb in rc.COUNTER_BEAMS:                                          # one beam more or less changes bits
        assert not rc.same_bits(grids[nb], grids[nb - 1]) and not rc.same_bits(grids[nb], grids[nb + 1])
        case = rc.counter_case(nb)
        H, M = np.zeros((150, 200), dtype=np.int64), np.zeros((150, 200), dtype=np.int64)
        M[70, 100:104], H[70, 104] = nb, nb
        args = (np.zeros((150, 200), dtype=np.float32), H, M, rc.l_of(case.kw["p_hit"]), rc.l_of(case.kw["p_miss"]), -5.0, 5.0)
        assert rc.same_bits(rc.apply_counts(*args)[0], grids[nb])        # four cells with M = nb, one with H = nb
        wrapped = rc.apply_counts(*args, wrap16=True)[0]                 # wrong model: 16 bits of M
        assert rc.same_bits(wrapped, grids[nb]) == (nb == 65535), nb
        carried = rc.apply_counts(args[0], H + (M >> 16), M & 0xffff, *args[3:])[0]     # wrong model: M carries into H
        assert rc.same_bits(carried, grids[nb]) == (nb == 65535), nb
    replay = rc.counter_replay_case()
    assert [len(s.hits) for s in replay.scans] == [100, 65535, 65536, 65537, 100]
    snaps = rc.expected(replay, snapshots=True)
    assert all(not rc.same_bits(a, b) for a, b in zip(snaps[:-1], snaps[1:]))


# ── E ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _replay_runs():
    for combo, (case, start) in zip(rc.REPLAY_COMBOS + (rc.DRIFT_COMBO,), rc.replay_cases()):
        H, M = rc.replay_counts(combo)
        kw = case.kw
        yield combo, case, start, (start, H, M, rc.l_of(kw["p_hit"]), rc.l_of(kw["p_miss"]), kw["log_odds_min"], kw["log_odds_max"])


def test_replay_restatement_is_the_oracle_and_reaches_every_exit():
    seen, starts = set(), set()
    for combo, case, start, args in _replay_runs():
        want = rc.expected(case, start)
        got, branch = rc.apply_counts(*args)
        assert rc.same_bits(got, want), case.name
        counted = branch != rc.UNTOUCHED
        assert counted.sum() == 8
        seen |= set(branch[counted].tolist())
        starts |= set(start[counted].view(np.uint32).tolist())
    assert seen == {rc.SAT_LO, rc.SAT_HI, rc.FIXED, rc.FULL}, seen
    assert len(starts) == len(rc.START_VALUES)                           # every start value under a count
    used = rc.REPLAY_COMBOS
    assert {c[0] for c in used} == {1, 1000, 65535} and {c[1] for c in used} == {False, True}
    assert {c[4] for c in used} == set(range(len(rc.CLAMPS))) and {c[5] for c in used} == set(range(len(rc.PROBS)))


def test_replay_wrong_models_differ():
    no_bound = keep = zero_case = 0
    for combo, case, start, args in _replay_runs():
        want = rc.expected(case, start)
        no_bound += not rc.same_bits(rc.apply_counts(*args, bound=False)[0], want)
        # (its loops are run where they are short: up to 1 000 adds, or l == 0.0, where the first add is the fixed point)
        differs = (combo[0] <= 1000 or case.kw["p_hit"] == 0.5) and not rc.same_bits(rc.apply_counts(*args, keep_on_fixed=True)[0], want)
        keep += differs
        if case.kw["p_hit"] == 0.5 and differs:                          # l == 0.0: a counted -0.0 ends as +0.0 in the oracle
            counted = rc.apply_counts(*args)[1] != rc.UNTOUCHED
            cell = counted & (start.view(np.uint32) == 0x80000000)
            assert cell.any() and (want.view(np.uint32)[cell] == 0).all()
            zero_case += 1
    assert no_bound >= 1 and keep >= 1 and zero_case >= 1, (no_bound, keep, zero_case)


# ── routing: every case takes the pass its id names ─────────────────────────────────────────────────────────────────────
NONE, OWNER, TILES, ATOMIC = 0, 1, 2, 3


@pytest.fixture(scope="module")
def plan_of():
    import icpmi
    from icpmi import _lib
    icpmi.build()
    L = _lib.lib()
    assert (_lib.RC_PASS_NONE, _lib.RC_PASS_OWNER, _lib.RC_PASS_TILES, _lib.RC_PASS_ATOMIC) == (NONE, OWNER, TILES, ATOMIC)

    def plan(case, scans, option, rows=None, full_clip=False):
        """the plan of the call OccupancyGrid2D makes for these scans of a case (one scan: update_scan; more: update_scans)"""
        g = case.grid
        off = np.zeros(len(scans) + 1, dtype=np.int32)
        np.cumsum([len(s.hits) for s in scans], out=off[1:])
        box = rc.box_of(g, scans)
        assert box is not None and box.dtype == np.int32
        r0, r1 = (0, g.ny) if rows is None else rows
        out = _lib.GridPlan()
        _lib.set_option("ICPMI_RAYCAST", option)
        try:
            code = L.icpmi_grid_update_plan(g.ny, g.nx, g.res, off.ctypes.data, len(scans), 1, 1 if full_clip else 0, r0, r1,
                                            box.ctypes.data, C.byref(out))
        finally:
            _lib.set_option("ICPMI_RAYCAST", None)
        assert code == 0
        return out
    return plan


LIVE = {None: OWNER, "owner": OWNER, "tiles": TILES, "atomic": ATOMIC}
REPLAY = {None: TILES, "owner": TILES, "tiles": TILES, "atomic": ATOMIC}


@pytest.mark.parametrize("option", [None, "owner", "tiles", "atomic"])
def test_every_case_takes_the_pass_its_id_names(plan_of, option):
    # A - C live: one scan, a box, no whole-grid clip
    for case in rc.border_cases() + rc.long_cases() + [rc.clamp_case()]:
        for s in case.scans:
            p = plan_of(case, [s], option)
            assert (p.pass_, p.wide, p.live_scans) == (LIVE[option], 0, 1), (case.name, s.name)
            assert 1 <= p.tiles_x * p.tiles_y <= 12                      # the window: the scan's box cut to the grid
    # B in bands and the replays: several scans in one call
    for case in rc.long_cases():
        for rows in ((40, 97), (0, 1)):
            if rows[1] <= case.grid.ny:
                p = plan_of(case, case.scans, option, rows=rows, full_clip=True)
                assert (p.pass_, p.wide, p.live_scans) == (REPLAY[option], 0, len(case.scans)), case.name
    for case in rc.replays():
        p = plan_of(case, case.scans, option)
        assert (p.pass_, p.wide, p.live_scans, p.group_max) == (REPLAY[option], 0, 3, 2), case.name
    # D: 65 535 beams fit the packed counter, one more goes the wide way under every option
    for nb in rc.COUNTER_BEAMS:
        p = plan_of(rc.counter_case(nb), rc.counter_case(nb).scans, option)
        assert p.wide == (1 if nb > rc.RC_WIDE else 0), nb
        assert p.pass_ == (LIVE[option] if nb <= rc.RC_WIDE else (TILES if option == "tiles" else ATOMIC)), nb
    replay = rc.counter_replay_case()
    p = plan_of(replay, replay.scans, option)
    assert (p.pass_, p.wide, p.live_scans) == (REPLAY[option], 1, 5)
    # E: an uploaded grid asks for the whole-grid clip, which the owner pass does not do
    for case, _ in rc.replay_cases():
        p = plan_of(case, case.scans, option, full_clip=True)
        assert p.pass_ == (TILES if option == "tiles" else ATOMIC) and p.wide == (1 if len(case.scans[0].hits) > rc.RC_WIDE else 0)
    assert any(len(c.scans[0].hits) > rc.RC_WIDE for c, _ in rc.replay_cases())      # H = M = 65 535: the two-round route
