"""Host side of the wide-window scan-to-map search (include/icpmi.h: icpmi_grid_bound_field, icpmi_grid_search_workspace_bytes,
icpmi_grid_search_batch): the C ABI as the header declares it, the workspace layout against literal sizes, every refusal the
entries decide on the host (fake pointers, never dereferenced: no GPU is touched) — and the NumPy restatement of the contract
(tests/gridmatch_wide_ref.py) against the exhaustive search it must reproduce: the bound is a bound, the record from the
survivors alone is the exhaustive record, the >= of the survivor test cannot be a >, and scans predicted metres and tens of
degrees off are relocalised in a map built by the oracle.  Everything is an integer: every comparison is array_equal."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridmatch_ref as ref
import gridmatch_wide_ref as wide
from conftest import REPO

NEW_SYMBOLS = ("icpmi_grid_bound_field", "icpmi_grid_search_workspace_bytes", "icpmi_grid_search_batch")
FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
GRID = dict(min_x=-3.0, min_y=-2.0, res=0.25)


def test_entries_and_defines_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib, gridmatch
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\(", hdr), name
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GMW_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert len(defines) == 8                                   # 2 capacities, the planned grid, 5 record names
    for n, v in defines.items():
        assert getattr(_lib, n) == v, n
    assert (defines["GMW_MAX_WINDOW"], defines["GMW_MAX_ANGLES"], defines["GMW_SCORE_GROUPS"]) == (255, 16384, 2048)
    assert [defines["GMW_REC_" + n] for n in ("BLOCKS", "SURVIVORS", "SEED", "MAX_BOUND", "INTS")] == [8, 9, 10, 11, 12]
    assert (gridmatch.WIDE_MAX_WINDOW, gridmatch.BLOCKS) == (255, wide.BLOCKS)
    assert lib.icpmi_grid_search_batch.argtypes[24] is ctypes.c_size_t and len(lib.icpmi_grid_search_batch.argtypes) == 26


def test_workspace_bytes_against_literal_values():
    """csrc/gridmatch_wide.hip, GmwWs: rows-with-a-cell counts (int32 per (pair, angle)), the pairs' words (32 bytes each), the
    list's count, the seeds (int32 per (pair, angle)), then the bounds and the survivor list (int32 per block each), every part
    rounded up to 256 bytes."""
    import icpmi
    q = icpmi.lib().icpmi_grid_search_workspace_bytes
    assert q(1, 91, 40, 8) == 512 + 256 + 256 + 512 + 2 * 44288 == 90112            # NB = 11: 91 * 121 * 4 = 44044 -> 44288
    assert q(1, 361, 100, 8) == 1536 + 256 + 256 + 1536 + 2 * 976384 == 1956352      # NB = 26: 361 * 676 * 4 = 976144 -> 976384
    assert q(70, 3, 5, 4) == 1024 + 2304 + 256 + 1024 + 2 * 7680 == 19968            # NB = 3: 70 * 3 * 9 * 4 = 7560 -> 7680
    assert q(1, 2, 255, 16) == 256 * 4 + 2 * 8192 == 17408                           # NB = 32
    assert q(1, 1, 0, 16) == 256 * 6 and q(0, 5, 3, 8) == 256
    assert q(-1, 5, 3, 8) == 0 and q(1, -1, 3, 8) == 0 and q(1, 5, -1, 8) == 0 and q(1, 5, 3, 5) == 0 and q(1, 5, 3, 0) == 0


def test_entries_refuse_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    search = L.icpmi_grid_search_batch
    off = np.array([0, 300, 600, 600], dtype=np.int32)
    pair = np.array([0, 1], dtype=np.int32)
    offp, pairp = off.ctypes.data_as(ctypes.c_void_p), pair.ctypes.data_as(ctypes.c_void_p)
    need = L.icpmi_grid_search_workspace_bytes(2, 25, 40, 8)

    def call(field=FAKE, bound=FAKE, ny=200, nx=280, res=0.1, pts=FAKE, off_dev=FAKE, off_host=offp, n_clouds=3, pair_cloud=FAKE,
             pair_host=pairp, n_pairs=2, pair_t=FAKE, cos_sin=FAKE, n_angles=25, window=40, block=8, centre=12, records=FAKE, bounds=None,
             ws=FAKE, ws_bytes=need):
        return search(field, bound, ny, nx, -14.0, -10.0, res, pts, off_dev, off_host, None, n_clouds, pair_cloud, pair_host, n_pairs,
                      pair_t, cos_sin, n_angles, window, block, centre, records, bounds, ws, ws_bytes, None)

    big = 1 << 40
    assert call(n_pairs=0) == 0 and call(n_pairs=0, off_host=None, pair_host=None, ws=None) == 0       # nothing to do
    assert call(window=256, ws_bytes=big) == ERR_UNSUPPORTED                   # W <= 255
    assert call(window=255, ws_bytes=0) == ERR_WORKSPACE                       # 255 passes the plan
    assert call(n_angles=16385, centre=-1, ws_bytes=big) == ERR_UNSUPPORTED    # A <= 16 384
    assert call(n_angles=8225, window=255, ws_bytes=big) == ERR_UNSUPPORTED    # 8 225 * 511^2 = 2^31 + 236 577
    assert call(n_angles=8224, window=255, ws_bytes=0) == ERR_WORKSPACE        # 8 224 * 511^2 < 2^31
    for block in (0, 1, 2, 5, 12, 32, -8):
        assert call(block=block, ws_bytes=big) == ERR_ARG, block
    for block in wide.BLOCKS:
        assert call(block=block, ws_bytes=0) == ERR_WORKSPACE, block
    off[:] = (0, 300, 300 + 65536, 300 + 65536)
    assert call(ws_bytes=big) == ERR_UNSUPPORTED                               # a cloud of 65 536 rows, by off_host
    off[:] = (0, 300, 600, 600)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(window=44) == ERR_WORKSPACE      # NB = 12, not 11
    for kw in (dict(field=None), dict(bound=None), dict(pts=None), dict(off_dev=None), dict(off_host=None), dict(pair_cloud=None),
               dict(pair_host=None), dict(pair_t=None), dict(cos_sin=None), dict(records=None), dict(ws=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(n_pairs=-1) == ERR_ARG and call(n_angles=0) == ERR_ARG and call(window=-1) == ERR_ARG and call(centre=25) == ERR_ARG
    assert call(ny=0) == ERR_ARG and call(nx=-3) == ERR_ARG and call(ny=1 << 16, nx=1 << 15) == ERR_ARG
    assert call(res=0.0) == ERR_ARG and call(res=float("nan")) == ERR_ARG
    pair[:] = (0, 3)
    assert call() == ERR_ARG                                                   # a pair's cloud beyond the set
    pair[:] = (0, 1)
    # the bound field's entry: a block of 4, 8 or 16, aligned non-null pointers; an empty grid is nothing to do
    boundf = L.icpmi_grid_bound_field
    assert boundf(None, 0, 10, 8, None, None) == 0 and boundf(None, 10, 0, 4, None, None) == 0
    assert boundf(FAKE, 10, 10, 7, FAKE, None) == ERR_ARG and boundf(FAKE, 10, 10, 32, FAKE, None) == ERR_ARG
    assert boundf(None, 10, 10, 8, FAKE, None) == ERR_ARG and boundf(FAKE, 10, 10, 8, None, None) == ERR_ARG
    assert boundf(FAKE + 2, 10, 10, 8, FAKE, None) == ERR_ARG and boundf(FAKE, 10, 10, 8, FAKE + 8, None) == ERR_ARG
    assert boundf(FAKE, -1, 10, 8, FAKE, None) == ERR_ARG and boundf(FAKE, 1 << 16, 1 << 15, 8, FAKE, None) == ERR_ARG


# ── the restatement against the exhaustive search ───────────────────────────
def test_bound_field_by_its_definition():
    rng = np.random.default_rng(2)
    q = rng.integers(-32767, 32768, size=(9, 13)).astype(np.int16)
    q[2, 3:9] = -32767
    for D in wide.BLOCKS:
        M = wide.bound_field(q, D)
        assert M.dtype == np.int16 and M.shape == (9 + D - 1, 13 + D - 1)
        for Y in range(M.shape[0]):
            for X in range(M.shape[1]):
                y, x = Y - (D - 1), X - (D - 1)
                win = [int(q[yy, xx]) if 0 <= yy < 9 and 0 <= xx < 13 else 0 for yy in range(y, y + D) for xx in range(x, x + D)]
                assert M[Y, X] == max(win), (D, Y, X)
    neg = np.full((20, 20), -7, dtype=np.int16)                 # "outside counts 0" holds in M: -7 only where the window is inside
    M = wide.bound_field(neg, 4)
    assert (M[3:-3, 3:-3] == -7).all() and not M[:3].any() and not M[-3:].any() and not M[:, :3].any() and not M[:, -3:].any()


def test_vectorised_volume_equals_the_loops():
    rng = np.random.default_rng(3)
    q = rng.integers(-3000, 3000, size=(17, 23)).astype(np.int16)
    pts = rng.uniform(-4.0, 4.0, size=(60, 2))
    pts[7] = (np.nan, 0.0)
    cs = ref.cos_sin_of(np.array([0.0, 0.7, -2.0]))
    for W in (0, 3, 9):
        got = wide.volume(q, pts, (0.2, -0.1), cs, W, **GRID)
        want = ref.volume(q, pts, (0.2, -0.1), cs, W, GRID["min_x"], GRID["min_y"], GRID["res"])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.int32


def random_case(seed, shape, n):
    rng = np.random.default_rng(seed)
    q = rng.integers(-20000, 20001, size=shape).astype(np.int16)
    q[rng.uniform(size=shape) < 0.7] = rng.integers(-300, 0)                    # mostly free space, some walls
    pts = rng.uniform(-1.0, 1.0, size=(n, 2)) * (shape[1] * 0.1, shape[0] * 0.1)
    t = rng.uniform(-0.5, 0.5, size=2) + (GRID["min_x"] + shape[1] * 0.125, GRID["min_y"] + shape[0] * 0.125)     # about the grid's centre
    return q, pts, t, ref.cos_sin_of(rng.uniform(-np.pi, np.pi, size=3))


@pytest.mark.parametrize("seed,W,D", [(s, W, D) for s, W in ((1, 0), (2, 1), (3, 5), (4, 11), (5, 16), (6, 21)) for D in wide.BLOCKS])
def test_the_bound_bounds_and_the_survivors_hold_the_winner(seed, W, D):
    q, pts, t, cs = random_case(seed, (37, 53), 80)
    vol, rows = wide.volume(q, pts, t, cs, W, **GRID)
    rec, U = wide.search(q, D, pts, t, cs, W, 1, **GRID)
    S, NB = 2 * W + 1, -(-(2 * W + 1) // D)
    assert U.shape == (3, NB, NB) and U.dtype == np.int32
    for J in range(NB):
        for I in range(NB):
            assert (U[:, J, I] >= vol[:, J * D:(J + 1) * D, I * D:(I + 1) * D].max(axis=(1, 2))).all(), (J, I)
    assert np.array_equal(rec[:8], ref.record(vol, rows, 1, W)), (rec, ref.record(vol, rows, 1, W))
    assert rec[8] == 3 * NB * NB and 1 <= rec[9] <= rec[8] and rec[10] <= rec[6] <= rec[11] == U.max()
    assert rec[9] == int((U >= rec[10]).sum())


def test_the_survivor_test_is_greater_or_equal():
    """Counter-check: with > in place of >= the restatement returns a different, later index.  On the plateau with every row
    inside the grid the two cannot differ — the first all-inside shift of an angle always lies in that angle's seed block
    (its (J, I) are the floors of the shift's (j, i) over D), so > merely prunes every block and the seed's result stands —
    which is why the second plateau pushes rows over the edge."""
    q, pts, t, cs, W, D, grid = wide.plateau(False)
    vol, rows = wide.volume(q, pts, t, cs, W, **grid)
    assert (vol == 360).all()
    rec, U = wide.search(q, D, pts, t, cs, W, 0, **grid)
    assert (U == 360).all() and list(rec) == [0, 40, 0, 0, 0, 0, 360, 360, 9, 9, 360, 360]        # every block survives, index 0
    strict, _ = wide.search(q, D, pts, t, cs, W, 0, keep=np.greater, **grid)
    assert strict[9] == 0 and strict[2] == 0                                                   # nothing survives >

    q, pts, t, cs, W, D, grid = wide.plateau(True)
    vol, rows = wide.volume(q, pts, t, cs, W, **grid)
    want = ref.record(vol, rows, 0, W)
    S = 2 * W + 1
    assert vol.max() == 180 and want[2] == D and vol[0, 1, 0] == 180 and (vol[0, 0, :D] < 180).all()
    rec, U = wide.search(q, D, pts, t, cs, W, 0, **grid)
    assert U[0, 0, 0] == U[0, 0, 1] == 180 == U.max() == rec[10]
    assert np.array_equal(rec[:8], want) and rec[2] == D
    strict, _ = wide.search(q, D, pts, t, cs, W, 0, keep=np.greater, **grid)
    assert strict[6] == 180 and strict[2] == S > D and strict[9] == 0                          # the same score, a later index


def test_two_equal_peaks_in_different_blocks():
    q = np.zeros((40, 30), dtype=np.int16)
    q[12, 9] = q[20, 22] = 500
    for D in wide.BLOCKS:
        rec, U = wide.search(q, D, np.array([[10.5, 15.5]]), (0.0, 0.0), ref.cos_sin_of(np.array([0.0])), 13, 0, 0.0, 0.0, 1.0)
        vol, rows = wide.volume(q, np.array([[10.5, 15.5]]), (0.0, 0.0), ref.cos_sin_of(np.array([0.0])), 13, 0.0, 0.0, 1.0)
        assert int((vol == 500).sum()) == 2 and np.array_equal(rec[:8], ref.record(vol, rows, 0, 13))
        assert tuple(rec[3:7]) == (0, 10, 12, 500) and rec[9] == 2                # (12 - 15 + 13, 9 - 10 + 13); the two blocks that see a peak


# ── relocalisation in the room ───────────────────────────────────────────────
def room_field():
    import oracle
    g = ref.SCENE
    lo = np.zeros((200, 280), dtype=np.float32)
    l_hit, l_miss = float(np.log(0.7 / 0.3)), float(np.log(0.4 / 0.6))
    for o, h in zip(*ref.scene_scans()):
        oracle.grid_update_scan(lo, g["min_x"], g["min_y"], 0.1, o, h, l_hit, l_miss, -5.0, 5.0)
    return ref.quantise(lo, ref.shift_bits(-5.0, 5.0))


def test_restatement_relocalises_in_the_room():
    """The map of tests/test_grid_match_cpu.py.  6 queries predicted 3 m per axis and 40 degrees off, W = 40 cells (4 m), +-45
    degrees in 1 degree steps: 91 x 81 x 81 candidates each.  First the condition on the inputs — the EXHAUSTIVE restatement
    lands within one cell per axis and one step of the truth with a unique maximum — then the assertion: the pruned record
    equals the exhaustive one.  Survivor fractions seen: 6 to 8 of 11 011 blocks (D = 8)."""
    g = ref.SCENE
    q = room_field()
    M = wide.bound_field(q, wide.RELOC["block"])
    W = wide.RELOC["W"]
    for true, pred, scan in wide.reloc_queries():
        angles = ref.angle_rows(pred[2], wide.RELOC["angular_window"], wide.RELOC["angular_step"])
        assert len(angles) == 91 and len(scan) == 512
        cs = ref.cos_sin_of(angles)
        vol, rows = wide.volume(q, scan, pred[:2], cs, W, g["min_x"], g["min_y"], 0.1)
        want = ref.record(vol, rows, 45, W)
        _, t = ref.pose(want, pred[:2], cs, W, 0.1)
        err_xy, err_th = np.abs(t - np.array(true[:2])), abs(np.rad2deg(angles[want[3]] - true[2]))
        assert err_xy.max() <= 0.1 + 1e-9 and err_th <= 1.0 + 1e-9 and want[6] > want[7]       # the condition on the inputs
        assert int((vol == want[6]).sum()) == 1
        rec, U = wide.search(q, wide.RELOC["block"], scan, pred[:2], cs, W, 45, g["min_x"], g["min_y"], 0.1, M=M)
        print(f"true {true} found {t} {angles[want[3]]}: best {want[6]} centre {want[7]}, survivors {rec[9]} of {rec[8]}")
        assert np.array_equal(rec[:8], want), (rec, want)
        assert rec[8] == 91 * 11 * 11 and 1 <= rec[9] <= rec[8]
