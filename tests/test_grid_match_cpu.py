"""Host side of the correlative scan-to-map matching (include/icpmi.h: icpmi_grid_score_field,
icpmi_grid_match_workspace_bytes, icpmi_grid_match_batch): the C ABI as the header declares it, the workspace layout against
literal sizes, every refusal the entry decides on the host — before any launch, so no GPU is touched (the pointers are fakes
that are never dereferenced) — the quantisation rule, and the NumPy restatement of the contract (tests/gridmatch_ref.py)
localising scans in a map built by the oracle: a condition on the inputs the device test then compares against bit for bit."""
import ctypes
import os
import re

import numpy as np

import gridmatch_ref as ref
from conftest import REPO

NEW_SYMBOLS = ("icpmi_grid_score_field", "icpmi_grid_match_workspace_bytes", "icpmi_grid_match_batch")
FAKE = 4096                                                    # a non-null address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


def test_entries_and_defines_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\(", hdr), name
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(GM_\w+|GMREC_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert len(defines) == 18                                  # 4 capacities, 2 kernel sizes, 3 statuses, 9 record names
    for n, v in defines.items():
        assert getattr(_lib, n) == v, n
    assert (defines["GM_MAX_WINDOW"], defines["GM_MAX_ANGLES"], defines["GM_MAX_ROWS"]) == (31, 1024, 65535)
    assert [defines["GMREC_" + n] for n in ("STATUS", "ROWS", "INDEX", "A", "J", "I", "SCORE", "CENTRE", "INTS")] == list(range(8)) + [8]
    assert (defines["GM_ST_OK"], defines["GM_ST_EMPTY"], defines["GM_ST_CAPACITY"]) == (0, 1, 2) and (ref.ST_OK, ref.ST_EMPTY) == (0, 1)
    assert lib.icpmi_grid_match_batch.argtypes[22] is ctypes.c_size_t and len(lib.icpmi_grid_match_batch.argtypes) == 24


def test_workspace_bytes_against_literal_values():
    """csrc/gridmatch.hip, GmWs: the rows-with-a-cell counts, one int32 per (pair, angle), then the score volume, one int32 per
    (pair, angle, shift), each rounded up to 256 bytes."""
    import icpmi
    q = icpmi.lib().icpmi_grid_match_workspace_bytes
    assert q(1, 25, 6) == 256 + 17152 == 17408                                 # 100 -> 256; 25 * 169 * 4 = 16900 -> 17152
    assert q(70, 65, 1) == 18432 + 163840 == 182272                            # 18200 -> 18432; 163800 -> 163840
    assert q(4096, 1, 0) == 16384 + 16384 == 32768
    assert q(1, 1024, 31) == 4096 + 1024 * 3969 * 4 == 16261120
    assert q(0, 5, 3) == 0
    assert q(-1, 25, 6) == 0 and q(1, -1, 6) == 0 and q(1, 25, -1) == 0


def test_match_refuses_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    match = L.icpmi_grid_match_batch
    off = np.array([0, 300, 600, 600], dtype=np.int32)
    pair = np.array([0, 1], dtype=np.int32)
    offp, pairp = off.ctypes.data_as(ctypes.c_void_p), pair.ctypes.data_as(ctypes.c_void_p)
    need = L.icpmi_grid_match_workspace_bytes(2, 25, 6)

    def call(field=FAKE, ny=200, nx=280, res=0.1, pts=FAKE, off_dev=FAKE, off_host=offp, n_clouds=3, pair_cloud=FAKE, pair_host=pairp,
             n_pairs=2, pair_t=FAKE, cos_sin=FAKE, n_angles=25, window=6, centre=12, records=FAKE, scores=None, ws=FAKE, ws_bytes=need):
        return match(field, ny, nx, -14.0, -10.0, res, pts, off_dev, off_host, None, n_clouds, pair_cloud, pair_host, n_pairs, pair_t,
                     cos_sin, n_angles, window, centre, records, scores, ws, ws_bytes, None)

    assert call(n_pairs=0) == 0                                                # nothing to do
    assert call(n_pairs=0, off_host=None, pair_host=None, ws=None) == 0
    assert call(window=32, ws_bytes=1 << 30) == ERR_UNSUPPORTED                # W <= 31
    assert call(n_angles=1025, ws_bytes=1 << 30) == ERR_UNSUPPORTED            # A <= 1 024
    off[:] = (0, 300, 300 + 65536, 300 + 65536)
    assert call(ws_bytes=1 << 30) == ERR_UNSUPPORTED                           # a cloud of 65 536 rows, by off_host
    off[:] = (0, 300, 300 + 65535, 300 + 65535)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE                            # 65 535 rows pass; a short workspace
    off[:] = (0, 300, 600, 600)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(window=7) == ERR_WORKSPACE
    for kw in (dict(field=None), dict(pts=None), dict(off_dev=None), dict(off_host=None), dict(pair_cloud=None), dict(pair_host=None),
               dict(pair_t=None), dict(cos_sin=None), dict(records=None), dict(ws=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(n_pairs=-1) == ERR_ARG and call(n_angles=0) == ERR_ARG and call(window=-1) == ERR_ARG and call(centre=25) == ERR_ARG
    assert call(ny=0) == ERR_ARG and call(nx=-3) == ERR_ARG and call(ny=1 << 16, nx=1 << 15) == ERR_ARG      # 2^31 cells
    assert call(res=0.0) == ERR_ARG and call(res=float("nan")) == ERR_ARG and call(res=float("inf")) == ERR_ARG
    pair[:] = (0, 3)
    assert call() == ERR_ARG                                                   # a pair's cloud beyond the set
    pair[:] = (-1, 0)
    assert call() == ERR_ARG
    pair[:] = (0, 1)
    off[:] = (0, 300, 200, 600)
    assert call() == ERR_ARG                                                   # a negative row count
    # the field entry: shift_bits in [0, 14], aligned non-null pointers; an empty grid is nothing to do
    fieldf = L.icpmi_grid_score_field
    assert fieldf(None, 0, 10, 12, None, None) == 0
    assert fieldf(FAKE, 10, 10, 15, FAKE, None) == ERR_ARG and fieldf(FAKE, 10, 10, -1, FAKE, None) == ERR_ARG
    assert fieldf(None, 10, 10, 12, FAKE, None) == ERR_ARG and fieldf(FAKE, 10, 10, 12, None, None) == ERR_ARG
    assert fieldf(FAKE + 4, 10, 10, 12, FAKE, None) == ERR_ARG and fieldf(FAKE, 10, 10, 12, FAKE + 2, None) == ERR_ARG
    assert fieldf(FAKE, -1, 10, 12, FAKE, None) == ERR_ARG


def test_quantisation_rule():
    from icpmi import gridmatch
    for clamp, k in ((5.0, 12), (8.0, 11), (0.5, 14), (40000.0, 0)):
        assert gridmatch.shift_bits(-clamp, clamp) == ref.shift_bits(-clamp, clamp) == k, clamp
    assert gridmatch.shift_bits(-5.0, 2.0) == 12 and gridmatch.shift_bits(-1.0, 7.999) == 12 and gridmatch.shift_bits(0.0, 0.0) == 14
    k = 12
    half = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 1000.5, 1001.5], dtype=np.float32) / np.float32(2.0 ** k)   # exact: x.5 / 2^k
    assert list(ref.quantise(half, k)) == [0, 2, 2, 4, 0, -2, -2, 1000, 1002]                   # half to even
    edge = np.array([7.99, 8.0, 9.0, -8.0, -9.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 5.0, -5.0, 1e-30], dtype=np.float32)
    assert list(ref.quantise(edge, k)) == [32727, 32767, 32767, -32767, -32767, 32767, -32767, 32767, -32767, 0, 0, 0, 20480, -20480, 0]
    assert list(ref.quantise(np.array([40000.0, -40000.0, 123.4, 0.5, 1.5], dtype=np.float32), 0)) == [32767, -32767, 123, 0, 2]
    assert ref.quantise(np.zeros((3, 4), dtype=np.float32), 3).dtype == np.int16


def test_restatement_record_and_ties():
    q = np.zeros((8, 9), dtype=np.int16)
    cs = ref.cos_sin_of(np.array([0.0, 0.3]))
    vol, rows = ref.volume(q, np.array([[0.3, 0.3]]), (0.0, 0.0), cs, 2, 0.0, 0.0, 0.25)
    assert vol.shape == (2, 5, 5) and not vol.any() and list(rows) == [1, 1]
    assert list(ref.record(vol, rows, 1, 2)) == [0, 1, 0, 0, 0, 0, 0, 0]                         # every candidate ties: flat index 0
    vol, rows = ref.volume(q, np.zeros((0, 2)), (0.0, 0.0), cs, 2, 0.0, 0.0, 0.25)
    assert list(ref.record(vol, rows, -1, 2)) == [1, 0, 0, 0, 0, 0, 0, 0]                        # an empty cloud
    q[3, 4] = 7
    vol, rows = ref.volume(q, np.array([[0.6, 0.3], [np.nan, 0.0], [1e12, 0.0]]), (0.0, 0.0), cs[:1], 2, 0.0, 0.0, 0.25)
    assert list(rows) == [1] and vol.sum() == 7 and vol[0, 4, 4] == 7                            # cell (2, 1) + (2, 2) = (4, 3)
    assert list(ref.record(vol, rows, 0, 2)) == [0, 1, 24, 0, 4, 4, 7, 0]


def test_restatement_localises_in_the_room():
    """The map: grid (-14, 14, -10, 10) at 0.1 m with default probabilities and clamps, 12 scans of icpmi.synth's room applied
    with the oracle.  12 queries up to 0.45 m and 9 degrees off, W = 6, +-12 degrees in 1 degree steps: every one is localised
    within one cell per axis and one step, scores above its predicted pose, and has a unique maximum."""
    import oracle
    g = ref.SCENE
    nx, ny = int(np.ceil((g["max_x"] - g["min_x"]) / 0.1)), int(np.ceil((g["max_y"] - g["min_y"]) / 0.1))
    assert (ny, nx) == (200, 280)
    lo = np.zeros((ny, nx), dtype=np.float32)
    l_hit, l_miss = float(np.log(0.7 / 0.3)), float(np.log(0.4 / 0.6))
    for o, h in zip(*ref.scene_scans()):
        oracle.grid_update_scan(lo, g["min_x"], g["min_y"], 0.1, o, h, l_hit, l_miss, -5.0, 5.0)
    k = ref.shift_bits(-5.0, 5.0)
    q = ref.quantise(lo, k)
    W = 6
    worst_xy = worst_th = 0.0
    for true, pred, scan in ref.scene_queries():
        angles = ref.angle_rows(pred[2])
        assert len(angles) == 25 and len(scan) == 1024
        cs = ref.cos_sin_of(angles)
        vol, rows = ref.volume(q, scan, pred[:2], cs, W, g["min_x"], g["min_y"], 0.1)
        rec = ref.record(vol, rows, 12, W)
        _, t = ref.pose(rec, pred[:2], cs, W, 0.1)
        err_xy, err_th = np.abs(t - np.array(true[:2])), abs(np.rad2deg(angles[rec[3]] - true[2]))
        print(f"true {true} found {t} {angles[rec[3]]}: err {err_xy} m {err_th:.3f} deg, best {rec[6]} centre {rec[7]}")
        worst_xy, worst_th = max(worst_xy, err_xy.max()), max(worst_th, err_th)
        assert err_xy.max() <= 0.1 and err_th <= 1.0
        assert rec[0] == ref.ST_OK and rec[6] > rec[7]
        assert int((vol == rec[6]).sum()) == 1                                                   # a unique maximum
    print("worst", worst_xy, worst_th)
