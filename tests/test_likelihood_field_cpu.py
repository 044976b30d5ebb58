"""Host side of the likelihood field (include/icpmi.h: icpmi_grid_likelihood_workspace_bytes, icpmi_grid_likelihood_field):
the C ABI as the header declares it, the workspace against literal sizes, every refusal the entry decides on the host — before
anything is enqueued, so no GPU is touched (the device pointers are fakes that are never dereferenced; the table is the one
host pointer and real) — the table's rule, the NumPy restatement (tests/likelihood_ref.py) against scipy's Euclidean
distance transform on the device test's cases, and the restatement localising thin, noisy scans in a map of one scan: a
condition on the inputs the device test then compares against bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridmatch_ref as gref
import gridmatch_wide_ref as wref
import likelihood_ref as ref
from conftest import REPO

NEW_SYMBOLS = ("icpmi_grid_likelihood_workspace_bytes", "icpmi_grid_likelihood_field")
FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


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
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(LF_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"LF_MAX_RADIUS": 64, "LF_TILE_X": 128, "LF_TILE_Y": 64}
    for n, v in defines.items():
        assert getattr(_lib, n) == v, n
    assert gridmatch.LF_MAX_RADIUS == ref.MAX_RADIUS == defines["LF_MAX_RADIUS"]
    args = lib.icpmi_grid_likelihood_field.argtypes
    assert len(args) == 12 and args[10] is ctypes.c_size_t and lib.icpmi_grid_likelihood_workspace_bytes.restype is ctypes.c_size_t


def test_workspace_bytes_against_literal_values():
    """csrc/gridfield.hip, LfWs: the device copy of the table, R^2 + 1 int16 rounded up to 256 bytes, whatever the grid."""
    import icpmi
    q = icpmi.lib().icpmi_grid_likelihood_workspace_bytes
    assert q(400, 560, 0) == 256                                               # 2 -> 256
    assert q(400, 560, 6) == 256                                               # 74 -> 256
    assert q(1, 1, 11) == 256 and q(1, 1, 12) == 512                           # 244 -> 256; 290 -> 512
    assert q(2242, 2402, 20) == 1024                                           # 802 -> 1024
    assert q(2242, 2402, 64) == 8448                                           # 8194 -> 8448
    assert q(10, 10, 65) == 0 and q(10, 10, -1) == 0 and q(0, 10, 3) == 0 and q(10, -1, 3) == 0
    assert q(1 << 16, 1 << 15, 3) == 0                                         # 2^31 cells


def test_entry_refuses_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    entry = L.icpmi_grid_likelihood_field
    tab = ref.table(20480.0, 2.0, 6)
    tabp = tab.ctypes.data_as(ctypes.c_void_p)
    need = L.icpmi_grid_likelihood_workspace_bytes(400, 560, 6)

    def call(field=FAKE, ny=400, nx=560, threshold=2048, radius=6, table=tabp, keep_free=1, d2=FAKE, lf=FAKE, ws=FAKE, ws_bytes=need):
        return entry(field, ny, nx, threshold, radius, table, keep_free, d2, lf, ws, ws_bytes, None)

    assert call(d2=None, lf=None) == ERR_ARG                                   # both outputs NULL
    assert call(table=None) == ERR_ARG and call(table=None, d2=None) == ERR_ARG    # a likelihood without a table
    assert call(radius=-1) == ERR_UNSUPPORTED and call(radius=65) == ERR_UNSUPPORTED
    assert call(radius=-1, lf=None, table=None, ws=None) == ERR_UNSUPPORTED and call(radius=65, lf=None, table=None, ws=None) == ERR_UNSUPPORTED
    assert call(ny=0) == ERR_ARG and call(nx=0) == ERR_ARG and call(ny=-4) == ERR_ARG and call(ny=0, radius=65) == ERR_ARG
    assert call(ny=1 << 16, nx=1 << 15) == ERR_ARG                             # 2^31 cells
    assert call(ny=65535 * 64 + 1, nx=1) == ERR_UNSUPPORTED                    # 65 536 rows of tiles
    assert call(field=None) == ERR_ARG
    for kw in (dict(field=FAKE + 2), dict(field=FAKE + 8), dict(d2=FAKE + 4), dict(lf=FAKE + 8), dict(lf=None, d2=FAKE + 2)):
        assert call(**kw) == ERR_ARG, kw                                       # 16-byte alignment of every device field
    assert call(ws=None) == ERR_WORKSPACE and call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE
    bad = tab.copy()
    bad[17] = -32768
    assert call(table=bad.ctypes.data_as(ctypes.c_void_p)) == ERR_ARG          # the matchers' score bound needs |field| <= 32767
    bad[17], bad[36] = 5, -32768
    assert call(table=bad.ctypes.data_as(ctypes.c_void_p)) == ERR_ARG          # ... up to the last entry


def test_workspace_of_another_radius_is_short():
    """145 entries are 290 bytes, two granules: the workspace of a radius of 6 (one granule) is refused for a radius of 12."""
    import icpmi
    L = icpmi.lib()
    tab = ref.table(20480.0, 4.0, 12)
    assert len(tab) == 145
    rc = L.icpmi_grid_likelihood_field(FAKE, 400, 560, 2048, 12, tab.ctypes.data_as(ctypes.c_void_p), 1, FAKE, FAKE, FAKE, 256, None)
    assert rc == ERR_WORKSPACE


@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5])
@pytest.mark.parametrize("R", [0, 1, 64])
def test_table_rule(sigma, R):
    from icpmi import gridmatch
    peak = float(np.rint(5.0 * 2.0 ** 12))
    tab = gridmatch.likelihood_table(peak, sigma, R)
    assert tab.dtype == np.int16 and tab.shape == (R * R + 1,)
    assert tab[0] == peak == 20480
    assert (np.diff(tab.astype(np.int64)) <= 0).all()                          # never rising with the distance
    assert tab.min() > -32768 and tab.min() >= 0
    assert np.array_equal(tab, ref.table(peak, sigma, R))                      # the restatement's expression, by construction
    if R == 64:
        assert tab[-1] == 0                                                    # 64 cells are beyond 25 sigma


def test_table_and_radius_arguments():
    from icpmi import gridmatch
    assert gridmatch.likelihood_table(40000.0, 1.0, 1)[0] == 32767 and gridmatch.likelihood_table(-40000.0, 1.0, 1)[0] == -32767
    for bad in (-1, 65, 2.5):
        with pytest.raises(ValueError):
            gridmatch.likelihood_table(100.0, 1.0, bad)
    with pytest.raises(ValueError):
        gridmatch.likelihood_table(100.0, 0.0, 3)


def test_restatement_by_hand():
    q = np.zeros((5, 7), dtype=np.int16)
    q[2, 3] = 10
    q[0, 6] = -4
    d2 = ref.distance_field(q, 10, 2)
    want = np.full((5, 7), 5, dtype=np.int16)
    want[2, 1:6] = (4, 1, 0, 1, 4)
    want[1, 2:5] = want[3, 2:5] = (2, 1, 2)
    want[0, 3] = want[4, 3] = 4
    assert np.array_equal(d2, want)
    tab = np.array([50, 40, 30, 20, 10], dtype=np.int16)
    _, lf = ref.likelihood_field(q, 10, 2, tab, True)
    assert lf[2, 3] == 50 and lf[1, 2] == 30 and lf[0, 3] == 10 and lf[0, 0] == 0 and lf[0, 6] == -4
    _, lf = ref.likelihood_field(q, 10, 2, tab, False)
    assert lf[0, 6] == 0 and lf[2, 3] == 50
    assert (ref.distance_field(q, 11, 2) == 5).all() and (ref.distance_field(q, -4, 0) == 0).sum() == 35
    assert np.array_equal(ref.distance_field(q, 10, 0), np.where(q >= 10, 0, 1))


def test_restatement_against_scipy():
    """The yardstick against something independent: scipy's exact Euclidean transform, squared, rounded and clamped to the
    sentinel, on every case the device test runs."""
    ndimage = pytest.importorskip("scipy.ndimage")
    from icpmi import _lib
    seen = 0
    for name, q, threshold, R, _, _ in ref.cases(_lib.LF_TILE_Y, _lib.LF_TILE_X):
        occ = ref.occupancy(q, threshold)
        if occ.any():
            e2 = np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.int64)
            want = np.where(e2 <= R * R, e2, R * R + 1)
        else:
            want = np.full(q.shape, R * R + 1)
        got = ref.distance_field(q, threshold, R)
        assert got.dtype == np.int16 and np.array_equal(got, want), name
        seen += 1
    assert seen == 20


def test_restatement_localises_thin_noisy_scans_in_a_map_of_one_scan():
    """The map: the room of tests/gridmatch_ref.py at 0.05 m, default probabilities and clamps, its FIRST scan alone applied
    with the oracle: walls one cell wide.  The 12 queries redrawn with 0.05 m of range noise, every 8th row; W = 12, +-12
    degrees in 1 degree steps.  With the likelihood field (sigma 2 cells, radius 6, free space kept) every query is localised
    within one cell per axis and one step; with the raw field the worst translation error is beyond one cell."""
    import oracle
    g, s = gref.SCENE, ref.SCENE
    res = s["resolution"]
    nx, ny = int(np.ceil((g["max_x"] - g["min_x"]) / res)), int(np.ceil((g["max_y"] - g["min_y"]) / res))
    assert (ny, nx) == (400, 560)
    lo = np.zeros((ny, nx), dtype=np.float32)
    l_hit, l_miss = float(np.log(0.7 / 0.3)), float(np.log(0.4 / 0.6))
    origins, hits = gref.scene_scans()
    oracle.grid_update_scan(lo, g["min_x"], g["min_y"], res, origins[0], hits[0], l_hit, l_miss, -s["clamp"], s["clamp"])
    k = gref.shift_bits(-s["clamp"], s["clamp"])
    q = gref.quantise(lo, k)
    tab = ref.table(np.rint(s["clamp"] * 2.0 ** k), s["sigma_cells"], s["radius"])
    _, lf = ref.likelihood_field(q, int(np.rint(s["occupied_log_odds"] * 2.0 ** k)), s["radius"], tab, True)
    W = s["W"]
    worst = {}
    for name, field in (("raw", q), ("likelihood", lf)):
        worst_xy = worst_th = 0.0
        for true, pred, scan in ref.scene_queries():
            angles = gref.angle_rows(pred[2])
            assert len(angles) == 25 and len(scan) == 128
            cs = gref.cos_sin_of(angles)
            vol, rows = wref.volume(field, scan, pred[:2], cs, W, g["min_x"], g["min_y"], res)
            rec = gref.record(vol, rows, 12, W)
            _, t = gref.pose(rec, pred[:2], cs, W, res)
            err_xy, err_th = np.abs(t - np.array(true[:2])).max(), abs(np.rad2deg(angles[rec[3]] - true[2]))
            print(f"{name}: true {true} found {t} {angles[rec[3]]}: err {err_xy:.4f} m {err_th:.3f} deg, best {rec[6]} centre {rec[7]}")
            worst_xy, worst_th = max(worst_xy, err_xy), max(worst_th, err_th)
            if name == "likelihood":
                assert err_xy <= res and err_th <= 1.0 and rec[0] == gref.ST_OK
        worst[name] = (worst_xy, worst_th)
    print("worst", worst)
    assert worst["raw"][0] > res                                               # 0.065 m: more than one cell
    assert worst["likelihood"][0] <= res                                       # 0.028 m
