"""Host side of the particle filter's global start and recovery (include/icpmi.h: icpmi_pf_free_index, icpmi_pf_draw_uniform,
icpmi_pf_free_index_bytes): the C ABI as the header declares it, every refusal the entries decide on the host — with fake
device pointers that are never dereferenced, and no call here is one the library would accept —, and the NumPy restatement
the device test compares against (tests/particles_global_ref.py): the free index on hand-made fields against literal words
and ranks, the draw at the ends of its range and over every free cell of the room map, the slots, and the restated filter
alone starting over a region of the room map and finding a kidnapped robot again."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridmatch_ref as gref
import particles_global_ref as gl
import particles_ref as ref
import stream_cases_particles_global  # noqa: F401  (registers the stream workload: tests/test_streams_cpu.py, tests/test_streams_gpu.py)
from conftest import REPO

FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
ENTRIES = {"icpmi_pf_free_index_bytes": 2, "icpmi_pf_free_index": 10, "icpmi_pf_draw_uniform": 16}
inf, nan = float("inf"), float("nan")
FREE, WALL, UNKNOWN, THRESHOLD = -100, 3000, 0, 2048           # field values of the hand-made maps


# ── the ABI ──────────────────────────────────────────────────────────────────
def test_entries_and_constants_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib, particles
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name, args in ENTRIES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        proto = re.search(r"^(?:int|size_t) " + name + r"\((.*?)\);", hdr, flags=re.S | re.M).group(1)
        assert len(proto.split(",")) == args == len(getattr(lib, name).argtypes), name
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(PFG_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"PFG_PURPOSE_UNIFORM": 2, "PFG_FREE_HEADER": 64, "PFG_FREE_BLOCK": 4096, "PFG_FREE_MAX_WORDS": 2 ** 22, "PFG_INJECTED": -1,
                       "PFG_ST_NO_FREE": 2}
    assert defines == {k: getattr(_lib, k) for k in defines} and sorted(k for k in vars(_lib) if k.startswith("PFG_")) == sorted(defines)
    assert defines == {"PFG_" + k: getattr(gl, k) for k in ("PURPOSE_UNIFORM", "FREE_HEADER", "FREE_BLOCK", "FREE_MAX_WORDS", "INJECTED", "ST_NO_FREE")}
    # the purpose and the status are new values beside the filter's own; one workgroup scans every block sum of the largest index
    assert gl.PURPOSE_UNIFORM not in (ref.PURPOSE_PREDICT, ref.PURPOSE_RESAMPLE) and gl.ST_NO_FREE not in (ref.ST_OK, ref.ST_DEGENERATE)
    assert gl.FREE_MAX_WORDS == gl.FREE_BLOCK * ref.THREADS * ref.SUMS_PER_LANE and gl.FREE_BLOCK % (4 * ref.THREADS) == 0
    assert icpmi.Recovery is particles.Recovery and (particles.ST_NO_FREE, particles.INJECTED) == (gl.ST_NO_FREE, gl.INJECTED)
    assert not any(hasattr(c, "run") for c in (particles.Recovery, particles.FreeCells))


def test_index_bytes_against_literal_values():
    """256 (the header) + 2 a(4 words) + a(4 blocks), a(x) = x rounded up to 256, words = ny ceil(nx / 32), blocks =
    ceil(words / 4096); 0 for a grid the build refuses."""
    import icpmi
    L = icpmi.lib()
    for (ny, nx), want in (((200, 280), 256 + 2 * 7424 + 256), ((1, 1), 256 + 2 * 256 + 256), ((0, 0), 256), ((5, 0), 256), ((0, 5), 256),
                           ((2242, 2402), 256 + 2 * 681728 + 256), ((65536, 2048), 256 + 2 * 2 ** 24 + 4096), ((65537, 2048), 0),
                           ((-1, 5), 0), ((5, -1), 0), ((2 ** 29 + 1, 1), 0), ((65536, 32768), 0)):
        assert L.icpmi_pf_free_index_bytes(ny, nx) == want, (ny, nx)
        if want:
            assert gl.index_bytes(ny, nx) == want, (ny, nx)


def test_entries_refuse_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    need = L.icpmi_pf_free_index_bytes(200, 280)

    def index(planes=FAKE, ny=200, nx=280, box=(0, 0, 280, 200), out=FAKE, out_bytes=need - 1):
        return L.icpmi_pf_free_index(planes, ny, nx, *box, out, out_bytes, None)

    def draw(n=1000, m=250, ix=FAKE, min_x=-14.0, min_y=-10.0, res=0.1, theta0=0.0, span=2.0 * np.pi, pair_t=FAKE, theta=FAKE, cos_sin=FAKE,
             ancestors=None, info=FAKE):
        return L.icpmi_pf_draw_uniform(n, m, ix, min_x, min_y, res, theta0, span, pair_t, theta, cos_sin, ancestors, info, 7, 3, None)

    # the index: the grid first (as icpmi_grid_occupancy_planes refuses it), then its size, then the planes, the index last
    for ny, nx in ((-1, 280), (200, -1), (2 ** 29 + 1, 1), (1, 2 ** 29 + 1), (65536, 32768)):
        assert index(ny=ny, nx=nx, planes=None, out=None) == ERR_ARG, (ny, nx)
    assert index(ny=65537, nx=2048, planes=None, out=None) == ERR_UNSUPPORTED                  # 2^22 + 64 words, before a null pointer is seen
    assert index(ny=65536, nx=2048, out_bytes=L.icpmi_pf_free_index_bytes(65536, 2048) - 1) == ERR_WORKSPACE      # the capacity itself is allowed
    assert index(planes=None) == ERR_ARG and index(planes=FAKE + 8) == ERR_ARG and index(planes=None, out=None) == ERR_ARG
    assert index() == ERR_WORKSPACE and index(out=None, out_bytes=need) == ERR_WORKSPACE and index(out=FAKE + 8, out_bytes=need) == ERR_WORKSPACE
    for box in ((-5, -5, 1000, 1000), (300, 0, 400, 10), (10, 10, 5, 5), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert index(box=box) == ERR_WORKSPACE, box            # any box is legal: the refusal is the short index's
    # the draw: n as in every entry of the filter, then m, the pointers, the numbers
    assert draw(n=-1) == ERR_ARG and draw(n=2 ** 20 + 1, ix=None) == ERR_UNSUPPORTED and draw(n=0, ix=None, m=5, res=nan) == 0
    assert draw(m=-1) == ERR_ARG and draw(m=1001) == ERR_ARG
    for name in ("ix", "pair_t", "theta", "cos_sin", "info"):
        assert draw(**{name: None}) == ERR_ARG, name
    assert draw(ix=FAKE + 8) == ERR_ARG and draw(pair_t=FAKE + 8) == ERR_ARG and draw(cos_sin=FAKE + 8) == ERR_ARG and draw(theta=FAKE + 4) == ERR_ARG
    for bad in (0.0, -0.1, nan, inf):
        assert draw(res=bad) == ERR_ARG, bad
    for bad in (-1e-300, np.nextafter(2.0 * np.pi, 7.0), nan, inf):
        assert draw(span=bad) == ERR_ARG, bad
    for name in ("theta0", "min_x", "min_y"):
        for bad in (nan, inf, -inf):
            assert draw(**{name: bad}) == ERR_ARG, (name, bad)
    assert draw(m=0, info=None) == ERR_ARG and draw(m=1000, ancestors=FAKE, info=None) == ERR_ARG       # (m = 0, m = n and ancestors are legal)


def test_the_python_layer_needs_no_gpu_for_its_policy():
    from icpmi import particles
    mine, theirs = particles.Recovery(), gl.Recovery()
    scores = [-900, -950, -900, -20000, -30000, -25000, -1200, -900, -900, ref.NO_SCORE, -900]
    got = [mine.update(s, 64) for s in scores]
    assert got == [theirs.update(s, 64) for s in scores]
    # nothing while the best score holds, a share when it falls, nothing again once the short average has caught up
    assert got[0] == 0.0 and 0.0 < got[2] < got[1] < 1e-3         # (-950 against -900 over 64 beams: below a slot in a thousand)
    assert got[3] > 0.1 and got[4] > got[3] and got[8] == 0.0 and got[9] > 0.5 and all(0.0 <= v < 1.0 for v in got)
    first = particles.Recovery(0.05, 0.6, scale=512)
    e1, e2 = float(np.exp(-1.0)), float(np.exp(-2.0))
    assert first.update(-512 * 64, 64) == 0.0 and first.w_slow == first.w_fast and abs(first.w_slow - e1) < 1e-15
    assert abs(first.update(-1024 * 64, 64) - (1.0 - (e1 + 0.6 * (e2 - e1)) / (e1 + 0.05 * (e2 - e1)))) < 1e-14       # (a few units of the last place)
    assert particles.Recovery().update(ref.NO_SCORE, 64) == 0.0            # nothing known yet: nothing to compare with
    for bad in (dict(alpha_slow=0.0), dict(alpha_slow=0.7), dict(alpha_fast=1.5), dict(scale=0), dict(scale=nan)):
        with pytest.raises(ValueError):
            particles.Recovery(**bad)


# ── the free index, restated ─────────────────────────────────────────────────
def hand_made_fields():
    """name -> (field int16 (ny, nx), box or None, F, the literal free words, the literal ranks)"""
    all_free = lambda ny, nx: np.full((ny, nx), FREE, dtype=np.int16)                                   # noqa: E731
    last_bit = np.full((2, 70), WALL, dtype=np.int16)
    last_bit[1, 69] = FREE
    gaps = np.full((1, 160), WALL, dtype=np.int16)
    gaps[0, 64:128:2] = UNKNOWN                                   # words 2 and 3: walls and unknown cells
    gaps[0, [35, 63, 96]] = FREE                                  # word 1: bits 3 and 31; word 3: bit 0
    mixed = all_free(2, 40)
    mixed[0, 0], mixed[0, 5], mixed[1, 39], mixed[1, 38] = WALL, UNKNOWN, WALL, THRESHOLD            # (the threshold itself is occupied)
    mixed[1, 37] = THRESHOLD - 1                                  # just below it: free
    return {
        "nx = 70: six valid bits in a row's last word": (all_free(2, 70), None, 140, [0xffffffff, 0xffffffff, 0x3f] * 2, [0, 32, 64, 70, 102, 134]),
        "a box that cuts two words in the middle": (all_free(3, 70), (10, 1, 40, 2), 30, [0, 0, 0, 0xfffffc00, 0xff, 0, 0, 0, 0], [0, 0, 0, 0, 22, 30, 30, 30, 30]),
        "a box that reaches over the grid's edges": (all_free(2, 70), (64, -7, 5000, 1), 6, [0, 0, 0x3f, 0, 0, 0], [0, 0, 0, 6, 6, 6]),
        "a box outside the grid": (all_free(3, 70), (100, 0, 200, 3), 0, [0] * 9, [0] * 9),
        "a box before the grid": (all_free(3, 70), (-50, -50, 0, 3), 0, [0] * 9, [0] * 9),
        "a box turned inside out": (all_free(3, 70), (40, 2, 10, 1), 0, [0] * 9, [0] * 9),
        # the ends of int32: x1 - 32 wx must not wrap for the words behind the first
        "a box that ends at the least int32 in x": (all_free(3, 70), (0, 0, -2 ** 31, 3), 0, [0] * 9, [0] * 9),
        "a box that ends at the least int32": (all_free(3, 70), (0, 0, -2 ** 31, -2 ** 31), 0, [0] * 9, [0] * 9),
        "a box that starts at the largest int32": (all_free(3, 70), (2 ** 31 - 1, 0, 2 ** 31 - 1, 3), 0, [0] * 9, [0] * 9),
        "a box from the least to the largest int32": (all_free(2, 70), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), 140,
                                                      [0xffffffff, 0xffffffff, 0x3f] * 2, [0, 32, 64, 70, 102, 134]),
        "nothing known": (np.zeros((2, 70), dtype=np.int16), None, 0, [0] * 6, [0] * 6),
        "walls everywhere": (np.full((2, 70), WALL, dtype=np.int16), None, 0, [0] * 6, [0] * 6),
        "one free cell, the last valid bit of the last word": (last_bit, None, 1, [0, 0, 0, 0, 0, 0x20], [0] * 6),
        "zero words in front of, between and behind free ones": (gaps, None, 3, [0, 0x80000008, 0, 1, 0], [0, 0, 2, 2, 3]),
        "walls, unknown cells and the threshold": (mixed, None, 76, [0xffffffde, 0xff, 0xffffffff, 0x3f], [0, 30, 38, 70]),
    }


def test_planes_restated_against_literal_words():
    field = hand_made_fields()["walls, unknown cells and the threshold"][0]
    occ, unk = gl.planes_of(field, THRESHOLD)
    assert occ.dtype == np.uint32 and occ.tolist() == [[0x1, 0x0], [0x0, 0xc0]] and unk.tolist() == [[0x20, 0x0], [0x0, 0x0]]
    assert np.array_equal(gl.unpack_rows(occ, 40), field >= THRESHOLD) and np.array_equal(gl.unpack_rows(unk, 40), field == 0)
    with pytest.raises(AssertionError):
        gl.unpack_rows(np.array([[0, 0x100]], dtype=np.uint32), 40)                                    # a pad bit


@pytest.mark.parametrize("name", list(hand_made_fields()))
def test_the_free_index_restated_against_literal_words_and_ranks(name):
    field, box, F, free, rank = hand_made_fields()[name]
    ny, nx = field.shape
    header, got_free, got_rank = gl.free_index(*gl.planes_of(field, THRESHOLD), nx, box)
    wpr = (nx + 31) // 32
    assert header.dtype == got_free.dtype == got_rank.dtype == np.uint32 and header.shape == (gl.FREE_HEADER,)
    assert header[:3].tolist() == [F, ny * wpr, wpr] and not header[3:].any()
    assert got_free.tolist() == free and got_rank.tolist() == rank, ([hex(v) for v in got_free], got_rank.tolist())
    # every free cell by its number, and the cells in word order
    if F:
        cx, cy, J = gl.cell_of(np.arange(F), got_free, got_rank, wpr)
        cells = set(zip(cx.tolist(), cy.tolist()))
        x0, y0, x1, y1 = box or (0, 0, nx, ny)
        want = {(x, y) for y in range(ny) for x in range(nx) if field[y, x] != 0 and field[y, x] < THRESHOLD and x0 <= x < x1 and y0 <= y < y1}
        assert len(cells) == F and cells == want and (np.diff(J) >= 0).all() and (np.diff(cy * 100000 + cx) > 0).all()


def test_the_single_free_cells_and_the_gaps_are_drawn_where_they_are():
    field, _, _, _, _ = hand_made_fields()["one free cell, the last valid bit of the last word"]
    index = gl.free_index(*gl.planes_of(field, THRESHOLD), 70)
    drawn, pair_t, theta, cells = gl.draw_uniform(index, 100, 100, 5.0, -3.0, 0.5, 1.0, 0.0, 9, 4)
    assert drawn.all() and (cells == [69, 1]).all() and (theta == 1.0).all()
    assert (pair_t[:, 0] > 5.0 + 69 * 0.5).all() and (pair_t[:, 0] < 5.0 + 70 * 0.5).all() and (pair_t[:, 1] > -2.5).all() and (pair_t[:, 1] < -2.0).all()
    field = hand_made_fields()["zero words in front of, between and behind free ones"][0]
    header, free, rank = gl.free_index(*gl.planes_of(field, THRESHOLD), 160)
    cx, cy, J = gl.cell_of([0, 1, 2], free, rank, 5)
    assert cx.tolist() == [35, 63, 96] and cy.tolist() == [0, 0, 0] and J.tolist() == [1, 1, 3]
    # no free cell: nothing is drawn
    assert gl.draw_uniform(gl.free_index(*gl.planes_of(np.zeros((2, 70), dtype=np.int16), THRESHOLD), 70), 10, 10, 0.0, 0.0, 0.1, 0.0, 1.0, 0, 0)[1] is None


# ── the draw ─────────────────────────────────────────────────────────────────
def test_k_covers_the_free_cells_exactly():
    for F in (1, 2, 3, 441, 17039, 2 ** 31 - 1):
        assert int(gl.k_of(0, F)) == 0 and int(gl.k_of(2 ** 32 - 1, F)) == F - 1, F
        # the least r0 of every k below 100: k r0-steps of 2^32 / F, without a gap
        ks = np.arange(min(F, 100))
        least = [(k * 2 ** 32 + F - 1) // F for k in ks.tolist()]
        assert gl.k_of(np.array(least, dtype=np.uint64), F).tolist() == ks.tolist()
        assert gl.k_of(np.array([v - 1 for v in least[1:]], dtype=np.uint64), F).tolist() == ks[:-1].tolist()


@pytest.fixture(scope="module")
def room():
    """(the room's field at k = 12, its threshold, the grid's frame, the whole map's free index)"""
    from test_grid_cast_cpu import room_field
    q, g = room_field()
    threshold = int(np.rint(0.5 * 2.0 ** 12))
    return q, threshold, g, gl.free_index(*gl.planes_of(q, threshold), q.shape[1])


def world_to_cell(w, mn, res):
    return np.floor((w - np.float64(mn)) / np.float64(res)).astype(np.int64)


def test_every_drawn_pose_lies_in_its_drawn_cell(room):
    q, threshold, g, index = room
    for min_x, min_y in ((g["min_x"], g["min_y"]), (-1e4, 3e3)):
        drawn, pair_t, theta, cells = gl.draw_uniform(index, 50000, 50000, min_x, min_y, 0.1, 0.3, 1.0, 77, 5)
        assert np.array_equal(world_to_cell(pair_t[:, 0], min_x, 0.1), cells[:, 0]) and np.array_equal(world_to_cell(pair_t[:, 1], min_y, 0.1), cells[:, 1])
        assert (theta > 0.3 - 0.5).all() and (theta < 0.3 + 0.5).all() and 0.95 < np.ptp(theta) < 1.0
    # the ends of the three uniform numbers: strictly inside the cell and the span
    lo, hi = (0 + 0.5) * 2.0 ** -24, (2 ** 24 - 1 + 0.5) * 2.0 ** -24
    assert 0.0 < lo and hi < 1.0 and (2 ** 32 - 1 + 0.5) * 2.0 ** -32 - 0.5 < 0.5 and (0 + 0.5) * 2.0 ** -32 - 0.5 > -0.5


def test_every_free_cell_of_the_room_map_is_drawn_and_no_other(room):
    q, threshold, g, index = room
    F = int(index[0][0])
    print(f"the room map: {F} free cells of {q.size}")
    assert q.shape == (200, 280) and F == 17039                  # (a condition on the inputs)
    n = 64 * F
    drawn, pair_t, theta, cells = gl.draw_uniform(index, n, n, g["min_x"], g["min_y"], 0.1, 0.0, gl.TWO_PI, 1, 0)
    free = (q != 0) & (q < threshold)
    hits = np.zeros(q.shape, dtype=np.int64)
    np.add.at(hits, (cells[:, 1], cells[:, 0]), 1)
    print(f"{n} draws: between {hits[free].min()} and {hits[free].max()} per free cell")
    assert drawn.all() and hits.sum() == n and (hits[free] > 0).all() and not hits[~free].any()
    assert hits[free].min() >= 64 - 6 * 8 and hits[free].max() <= 64 + 8 * 8                    # Poisson(64): the deviation is 8


def test_the_slots():
    n = 1000
    for m in (0, 1, 7, 999, 1000):
        s = gl.slots(n, m)
        where = np.flatnonzero(s)
        assert s.shape == (n,) and len(where) == m and np.array_equal(s, gl.slots_ints(n, m)), m
        if m > 1:
            gaps = np.diff(where)
            assert gaps.max() - gaps.min() <= 1 and gaps.min() >= n // m, (m, gaps.min(), gaps.max())
    assert gl.slots(1, 1).tolist() == [True] and gl.slots(1, 0).tolist() == [False] and gl.slots(4, 2).tolist() == [False, True, False, True]
    big = 2 ** 20
    assert gl.slots(big, big // 4).sum() == big // 4 and gl.slots(big, big - 1).sum() == big - 1


def test_injection_on_top_of_a_resampling(room):
    q, threshold, g, index = room
    n, m, seed, step = 1000, 250, 5, 9
    w = ref.weight_cases(n)["runs of zeros"]
    anc, _, status = ref.resample(w, seed, step)
    rng = np.random.default_rng(3)
    state = (rng.normal(size=(n, 2)), rng.normal(size=n), rng.normal(size=(n, 2)))
    gathered = tuple(v[anc] for v in state)
    pair_t, theta, drawn, anc2 = gl.inject(gathered, anc, index, m, g["min_x"], g["min_y"], 0.1, 0.25, 2.0, seed, step)
    assert status == ref.ST_OK and drawn.sum() == m and np.array_equal(drawn, gl.slots(n, m))
    assert (anc2[drawn] == gl.INJECTED).all() and np.array_equal(anc2[~drawn], anc[~drawn])
    assert np.array_equal(pair_t[~drawn], gathered[0][~drawn]) and np.array_equal(theta[~drawn], gathered[1][~drawn])
    free = (q != 0) & (q < threshold)
    assert (np.abs(theta[drawn] - 0.25) < 1.0).all() and free[world_to_cell(pair_t[drawn, 1], g["min_y"], 0.1), world_to_cell(pair_t[drawn, 0], g["min_x"], 0.1)].all()
    # the draw of slot j does not depend on m or n: the same slot in another draw has the same pose
    all_t = gl.draw_uniform(index, n, n, g["min_x"], g["min_y"], 0.1, 0.25, 2.0, seed, step)[1]
    assert np.array_equal(pair_t[drawn], all_t[drawn])


# ── the restated filter ──────────────────────────────────────────────────────
N = 1024


def room_filter(seed, n=N):
    """tests/test_particles_cpu.py::room_filter with the filter of tests/particles_global_ref.py and ``n`` particles."""
    from icpmi import gridmatch, synth
    from test_grid_cast_cpu import room_field
    from test_particles_cpu import CHAIN
    q, g = room_field()
    H = CHAIN["half_width"]
    wtable, shift = ref.weight_table(CHAIN["temperature"])
    f = gl.Filter(q, int(np.rint(0.5 * 2.0 ** 12)), g["min_x"], g["min_y"], 0.1, n, seed, wtable, shift, gridmatch.beam_table(0.1, 0.1, H), H,
                  1.5 * (H + 2) * 0.1)
    return f, [synth.scan(p, 50 + k)[::CHAIN["thin"]] for k, p in enumerate(gref.SCENE_POSES)]


def errors(mean, truth):
    return float(np.hypot(*(mean[:2] - truth[:2]))), float(abs((mean[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi))


def box_about(pose, half):
    return (pose[0] - half, pose[1] - half, pose[0] + half, pose[1] + half)


KIDNAP = dict(scan=3, shift=(1.5, 0.8, np.deg2rad(40.0)), box=box_about(gref.SCENE_POSES[5], 2.5), heading=0.25, span=np.deg2rad(120.0), settled=8)


def kidnapped_chain(f, scans, recovery, report):
    """The chain of test_the_restated_filter_localises_in_the_room_map from init_gaussian; before the weights of scan
    KIDNAP["scan"] every particle is moved by KIDNAP["shift"] -> [(|dxy|, |dtheta|, slots injected or None)] per scan."""
    from test_particles_cpu import CHAIN, controls
    truth = np.array(gref.SCENE_POSES)
    f.init_gaussian(truth[0], CHAIN["init_sigma"])
    out = []
    for k, scan in enumerate(scans):
        if k:
            f.predict(controls()[k - 1], CHAIN["motion_sigma"])
        if k == KIDNAP["scan"]:
            f.pair_t, f.theta = f.pair_t + np.array(KIDNAP["shift"][:2]), f.theta + KIDNAP["shift"][2]
            f.cos_sin = np.stack([np.cos(f.theta), np.sin(f.theta)], axis=1)
        ess, ok = f.weigh(scan)
        region = dict(box=KIDNAP["box"], heading=KIDNAP["heading"], span=KIDNAP["span"]) if recovery is not None else {}
        injected = f.maybe_resample(ess, len(scan), 0.5, recovery, **region)
        e_xy, e_th = errors(f.estimate()[0], truth[k])
        print(f"{report} scan {k}: ess {ess:.1f}, ok {ok}, injected {injected}, |dxy| {e_xy:.3f} m, |dtheta| {np.degrees(e_th):.2f} deg")
        out.append((e_xy, e_th, injected))
    return out


def test_a_start_over_a_region_of_the_room_map_localises():
    """init_uniform over the box of +-1 m about SCENE_POSES[0] (400 free cells: 20 x 20, the box being half-open; counted with
    the cells of x_hi and y_hi it would be 21 x 21 = 441) with headings within 60 degrees about the true one, N = 1 024, then the chain of test_the_restated_filter_localises_in_the_room_map: from the fourth scan on the
    estimate lies within 0.3 m and 5 degrees.  Seen when this was written, seed 0, with the restated Philox draws: 0.102,
    0.132 and 0.081 m at the first three scans (the ess of the first is 4.8 of 1 024), at most 0.047 m and 0.10 degrees from
    the fourth on, 0.009 m at the last."""
    from test_particles_cpu import CHAIN, controls
    f, scans = room_filter(0)
    truth = np.array(gref.SCENE_POSES)
    box = box_about(truth[0], 1.0)
    assert int(f.free_index(box)[0][0]) == 400                    # (a condition on the inputs)
    f.init_uniform(box, heading=truth[0, 2], span=np.deg2rad(60.0))
    assert f.step == 1 and (np.abs(f.pair_t - truth[0, :2]) < 1.0 + 0.1).all() and (np.abs(f.theta - truth[0, 2]) < np.deg2rad(30.0)).all()
    for k, scan in enumerate(scans):
        if k:
            f.predict(controls()[k - 1], CHAIN["motion_sigma"])
        ess, ok = f.weigh(scan)
        if ess < 0.5 * f.n:
            f.resample()
        e_xy, e_th = errors(f.estimate()[0], truth[k])
        print(f"scan {k}: ess {ess:.1f}, ok {ok}, |dxy| {e_xy:.3f} m, |dtheta| {np.degrees(e_th):.2f} deg")
        assert ok == f.n
        if k >= 3:
            assert e_xy < 0.3 and e_th < np.deg2rad(5.0), k
    with pytest.raises(ValueError):
        f.init_uniform((100.0, 100.0, 101.0, 101.0))


def test_a_kidnapped_robot_is_found_again_by_injection():
    """N = 1 024 from init_gaussian, every particle moved by (+1.5 m, +0.8 m, +40 degrees) before the weights of scan 3.
    The condition on the inputs: without injection the estimate stays more than 1 m off at every scan from 3 on.  The
    assertion: with Recovery(0.05, 0.6) and injection over the box of +-2.5 m about SCENE_POSES[5] (2 423 free cells of 50 x 50; 2 505 of 51 x 51 with the cells of x_hi and y_hi), headings
    within 120 degrees about 0.25, the estimate lies within 0.3 m and 5 degrees from scan 8 on.  Seeds tried with the restated
    Philox draws when this was written: 0, 1 and 2, all within the bound at N = 1 024; seed 0 runs here.  Seen without
    injection, seed 0: 1.72 to 2.28 m off from scan 3 on, the ess between 570 and 990 of 1 024.  Seen with injection, the
    worst of scans 8 to 11 and the slots injected at scans 3 to 9: seed 0: 0.190 m, 2.16 degrees, 431 578 550 508 420 199 0;
    seed 1: 0.029 m, 0.15 degrees, 435 551 581 500 329 67 0; seed 2: 0.089 m, 1.44 degrees, 419 573 529 467 411 251 27.  The
    estimate is formed after the resampling, so a scan at which slots are injected carries their spread: seed 0's 0.190 m
    is scan 8, with 199 injected, and seed 2's 0.089 m scan 9, with 27; from scan 10 on every seed is within 0.06 m."""
    f, scans = room_filter(0)
    assert int(f.free_index(KIDNAP["box"])[0][0]) == 2423         # (a condition on the inputs)
    lost = kidnapped_chain(f, scans, None, "without injection,")
    assert all(e_xy > 1.0 for e_xy, _, _ in lost[KIDNAP["scan"]:]), [round(e[0], 2) for e in lost]
    f, scans = room_filter(0)
    found = kidnapped_chain(f, scans, gl.Recovery(0.05, 0.6), "with injection,")
    assert found[KIDNAP["scan"]][2] and found[KIDNAP["scan"]][2] > N // 8              # the loss is seen at once: slots are injected
    for k in range(KIDNAP["settled"], len(scans)):
        assert found[k][0] < 0.3 and found[k][1] < np.deg2rad(5.0), (k, found[k])
