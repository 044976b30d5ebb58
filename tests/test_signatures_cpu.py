"""Appearance signatures without a GPU (include/icpmi.h: icpmi_history_signatures_add, icpmi_history_similar;
icpmi/history.py: ``similar``, ``similar_loop_candidates``): the C ABI and every refusal the entries decide on the host; the
NumPy restatement (tests/signatures_ref.py) on hand-made clouds whose signatures are stated literally; the exact
quarter-turn property, which fixes the sign of ``yaw``; pairs of clouds for every shift; what the signatures are FOR —
stored scans of the query's place ranked first whatever the heading, in the single room of icpmi.synth — asserted on the
restatement, to which tests/test_signatures_gpu.py holds the device bit for bit; the host logic of the Python layer; and
the CPU half of tests/buffer_ends_signatures.py (exact sizes, one byte less refused)."""
import ctypes
import os
import re

import numpy as np
import pytest

import buffer_ends as be
import signatures_ref as ref
import stream_cases_signatures  # noqa: F401  (registers the stream workload: tests/test_streams_cpu.py counts on it)
from buffer_ends_signatures import CASES
from conftest import REPO

NEW_SYMBOLS = ("icpmi_history_signatures_add", "icpmi_history_similar_workspace_bytes", "icpmi_history_similar")
FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
TAB = ref.tables()


@pytest.fixture(scope="module")
def L():
    import icpmi
    icpmi.build()
    return icpmi.lib()


def sig_of(points):
    return ref.signature(points, TAB)


def cells_of(words):
    """{(ring, sector)} of a signature."""
    return {(int(r), int(s)) for r, s in np.argwhere(ref.unpack(words))}


# ── a. ABI and refusals ──────────────────────────────────────────────────────
def test_new_entries_are_declared_exported_and_bound(L):
    from icpmi import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b" + name + r"\(", hdr), name
    V, I = ctypes.c_void_p, ctypes.c_int32
    H = ctypes.POINTER(_lib.History)
    assert L.icpmi_history_signatures_add.argtypes == [H, V, V, V, V, I, I, V] and L.icpmi_history_signatures_add.restype is ctypes.c_int
    assert L.icpmi_history_similar_workspace_bytes.argtypes == [I, I, I] and L.icpmi_history_similar_workspace_bytes.restype is ctypes.c_size_t
    assert L.icpmi_history_similar.argtypes == [H, V, V, V, I, V, V, I, I, V, V, V, ctypes.c_size_t, V]
    assert (_lib.SIG_RINGS, _lib.SIG_SECTORS, _lib.SIG_MAX_TOP, _lib.SIG_TABLE_DOUBLES, _lib.SIG_REC_INTS) == (32, 64, 64, 63, 4)
    assert (ref.RINGS, ref.SECTORS, ref.MAX_TOP, ref.TABLE_DOUBLES) == (32, 64, 64, 63)
    assert (_lib.SIG_REC_ID, _lib.SIG_REC_SCORE, _lib.SIG_REC_SHIFT, _lib.SIG_REC_BEST) == (0, 1, 2, 3)


def fake_history(scans=4, rows=8192):
    from icpmi import _lib
    return _lib.History(pts=FAKE, off_dev=FAKE, scan_capacity=scans, row_capacity=rows)


def test_signatures_add_refuses_bad_arguments_on_the_host(L):
    from icpmi import _lib
    add = L.icpmi_history_signatures_add
    off = np.zeros(5, dtype=np.int32)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    B, h = ctypes.byref, fake_history()
    assert add(B(h), FAKE, FAKE, FAKE, offp, 0, 0, None) == 0                  # nothing to do: no launch
    assert add(None, FAKE, FAKE, FAKE, offp, 0, 1, None) == ERR_ARG
    assert add(B(_lib.History()), FAKE, FAKE, FAKE, offp, 0, 1, None) == ERR_ARG
    for k in range(3):
        args = [FAKE, FAKE, FAKE]
        args[k] = None
        assert add(B(h), *args, offp, 0, 1, None) == ERR_ARG, k
    assert add(B(h), FAKE, FAKE, FAKE, None, 0, 1, None) == ERR_ARG
    assert add(B(h), FAKE, FAKE, FAKE, offp, 3, 2, None) == ERR_ARG            # beyond the scan capacity
    assert add(B(h), FAKE, FAKE, FAKE, offp, -1, 1, None) == ERR_ARG and add(B(h), FAKE, FAKE, FAKE, offp, 0, -1, None) == ERR_ARG
    off[:] = (0, 4000, 8000, 12000, 12000)
    assert add(B(h), FAKE, FAKE, FAKE, offp, 2, 1, None) == ERR_ARG            # beyond the row capacity
    off[:] = (0, 10, 5, 5, 5)
    assert add(B(h), FAKE, FAKE, FAKE, offp, 1, 1, None) == ERR_ARG            # a negative row count


def test_similar_workspace_bytes_and_refusals_on_the_host(L):
    q = L.icpmi_history_similar_workspace_bytes
    assert q(1, 1, 1) == 256 and q(3, 64, 5) == 768 and q(3, 65, 5) == 1024 and q(4096, 4096, 10) == 4096 * 4096 * 4
    assert q(0, 100, 1) == 256 and q(5, 0, 1) == 256                             # nothing to hold: the least a buffer is
    assert q(1, 1, 0) == 0 and q(1, 1, 65) == 0 and q(-1, 1, 1) == 0 and q(1, -1, 1) == 0
    assert q(65536, 1, 1) == 0 and q(32768, 65536, 1) == 0                      # refused sizes
    sim = L.icpmi_history_similar
    B, h = ctypes.byref, fake_history(scans=64)
    need = q(3, 63, 5)

    def call(hh=h, sig=FAKE, bits=FAKE, ids=FAKE, n_queries=3, lo=FAKE, hi=FAKE, n_scans=63, top_k=5, rec=FAKE, rows=None, ws=FAKE,
             ws_bytes=need):
        return sim(B(hh) if hh is not None else None, sig, bits, ids, n_queries, lo, hi, n_scans, top_k, rec, rows, ws, ws_bytes, None)

    assert call(n_queries=0) == 0                                              # nothing to do: no launch
    assert call(n_queries=0, sig=None, rec=None, ws=None, ws_bytes=0) == 0
    assert call(top_k=0) == ERR_ARG and call(top_k=65) == ERR_ARG and call(n_queries=-1) == ERR_ARG and call(n_scans=-1) == ERR_ARG
    assert call(hh=None) == ERR_ARG and call(n_scans=65, ws_bytes=1 << 20) == ERR_ARG       # more scans than the store has
    for kw in (dict(sig=None), dict(bits=None), dict(ids=None), dict(lo=None), dict(hi=None), dict(rec=None), dict(ws=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(ws=FAKE + 8) == ERR_ARG                                        # 16-byte aligned
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(rows=FAKE, ws_bytes=need - 1) == ERR_WORKSPACE
    assert call(n_queries=65536, n_scans=1) == ERR_UNSUPPORTED


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_buffer_end_cases_have_exact_sizes_and_refuse_one_byte_less(case, L):
    import arena as ar
    b = be.build_on_cpu(case, L)
    assert b.call is not None and b.outputs and b.expected is not None
    for r in b.arena.regions.values():
        assert r.ptr % ar.ALIGN == ar.START, r.name
    for name, (query, args, refusal, on_host) in b.sized.items():
        need = getattr(L, query)(*args)
        assert need > 0 and b.arena.nbytes(name) == need == b.size(name) and b.size(name, short=name) == need - 1
        assert refusal == ERR_WORKSPACE and on_host and b.call(short=name) == ERR_WORKSPACE
    want = b.expected()                                                        # the stated sizes are the restatement's shapes
    for name in b.outputs:
        assert np.asarray(want[name]).nbytes == b.arena.nbytes(name), name
    if case.id.startswith("similar"):
        assert set(b.sized) == {"workspace"}
    else:
        assert b.arena.nbytes("sig") == 260 * b.arena.regions["sig_bits"].shape[0] - b.arena.nbytes("sig_bits")     # 260 bytes a scan


# ── b. literal signatures of hand-made clouds ────────────────────────────────
def test_tables_are_what_the_header_states():
    from icpmi import history
    edge2, bc, bs = TAB
    assert edge2[0] == 0.1 * 0.1 and edge2[1] == (0.1 + 0.5) * (0.1 + 0.5) and edge2[32] == (0.1 + 16.0) * (0.1 + 16.0)
    assert edge2.shape == (33,) and (np.diff(edge2) > 0).all()
    assert bc[8] == np.cos(np.pi / 4) and bs[8] == np.sin(np.pi / 4) and bc[0] == 1.0 and bs[0] == 0.0
    packed = ref.packed_tables()
    assert packed.shape == (63,) and packed.tobytes() == history.signature_tables(0.5, 0.1).tobytes()
    assert ref.packed_tables(0.25, 0.3).tobytes() == history.signature_tables(0.25, 0.3).tobytes()


def test_literal_signatures_of_the_edge_clouds():
    clouds = ref.edge_clouds()
    # squared ranges exactly edge2[0], [1], [31], [32] on the +x axis: rings 0, 1, 31 and out (>= is on the outer side)
    ring, sector, kept = ref.cells(clouds["ring_edges"], TAB)
    assert ring.tolist() == [0, 1, 31, 32] and kept.tolist() == [True, True, True, False] and sector.tolist() == [0, 0, 0, 0]
    assert cells_of(sig_of(clouds["ring_edges"])[0]) == {(0, 0), (1, 0), (31, 0)} and sig_of(clouds["ring_edges"])[1] == 3
    # the axes, range 1 (ring 1): +x -> 0, +y -> 16, -y -> 48 with either zero; -x -> 31 with either zero, because a row with
    # y == 0 (either sign: -0.0 >= 0) and x <= 0 belongs to the second quadrant, whose last sector is 31
    ring, sector, kept = ref.cells(clouds["axes"], TAB)
    assert kept.all() and (ring == 1).all() and sector.tolist() == [0, 0, 16, 16, 31, 31, 48, 48]
    w, bits = sig_of(clouds["axes"])
    assert w[1] == (1 << 0) | (1 << 16) | (1 << 31) | (1 << 48) and bits == 4 and not w[[0] + list(range(2, 32))].any()
    # exactly on the direction of boundary 5, and one ulp of y either side: on it and above it sector 5, below it sector 4
    _, sector, kept = ref.cells(clouds["sector_boundary"], TAB)
    assert kept.all() and sector.tolist() == [5, 5, 4]
    # NaN, inf, zero rows; rows below min_range; rows past the reach: nothing
    for name in ("not_finite", "below_min_range", "past_reach"):
        assert not ref.cells(clouds[name], TAB)[2].any(), name
        w, bits = sig_of(clouds[name])
        assert not w.any() and bits == 0, name
    assert sig_of(np.zeros((0, 2)))[1] == 0
    # every sector centre lands in its sector, in every ring
    for r in (0.3, 5.2, 16.0):
        _, sector, kept = ref.cells(np.array([ref.sector_centre(s, r) for s in range(64)]), TAB)
        assert kept.all() and sector.tolist() == list(range(64))


# ── c. the exact quarter-turn property, and the sign of yaw ──────────────────
def generic_cloud(seed, n=400):
    rng = np.random.default_rng(seed)
    ang, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, 17.0, n)
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)


@pytest.mark.parametrize("seed", range(4))
def test_a_quarter_turn_rotates_the_signature_by_sixteen_sectors(seed):
    from icpmi import history
    cloud = generic_cloud(seed)                                                # (no row on an axis: the -x axis is the one exception, above)
    w, bits = sig_of(cloud)
    assert bits > 100
    for k in range(1, 4):
        turned = ref.quarter_turn(cloud, k)
        wk, bk = sig_of(turned)
        assert wk.tobytes() == ref.rotl(w, 16 * k).tobytes() and bk == bits
        # query = the turned cloud, candidate = the original: rotl of the candidate by 16 k is the query
        score, shift, best = ref.compare(wk, bk, w[None], [bits])
        assert (score[0], shift[0], best[0]) == (65535, 16 * k, bits)
        # and the other way round
        score, shift, best = ref.compare(w, bits, wk[None], [bk])
        assert (score[0], shift[0], best[0]) == (65535, 64 - 16 * k, bits)
    # the sign of yaw: points turned by +90 degrees in the sensor frame are what a sensor turned by -90 degrees sees, so the
    # source (the turned cloud) has heading -pi / 2 relative to the candidate: yaw = -shift * 2 pi / 64
    assert ref.yaw_of(16) == -np.pi / 2 and ref.yaw_of(48) == np.pi / 2 and ref.yaw_of(0) == 0.0 and ref.yaw_of(32) == np.pi
    assert np.array_equal(history.shift_yaw(np.arange(64)), ref.yaw_of(np.arange(64)))
    assert (ref.yaw_of(np.arange(64)) > -np.pi).all() and (ref.yaw_of(np.arange(64)) <= np.pi).all()


# ── d. every shift wins once; ties; empty signatures ─────────────────────────
@pytest.mark.parametrize("s", range(64))
def test_every_shift_wins_once(s):
    query, cand = ref.shift_pair(s, seed=s)
    (wq, bq), (wc, bc) = sig_of(query), sig_of(cand)
    inter = ref.intersections(wq, wc[None])[0]
    assert inter[s] == bq == bc and (np.delete(inter, s) < bq).all()           # the unique best
    score, shift, best = ref.compare(wq, bq, wc[None], [bc])
    assert (score[0], shift[0], best[0]) == (65535, s, bq)


def test_ties_and_empty_signatures():
    full = sig_of(ref.full_ring())
    assert full[1] == 64
    score, shift, best = ref.compare(*full, full[0][None], [64])
    assert (score[0], shift[0], best[0]) == (65535, 0, 64)                     # every shift ties: the lowest
    # two identical scans at different ids: the lower id first; an empty signature scores 0 against anything
    q = sig_of(generic_cloud(9))
    other, empty = sig_of(generic_cloud(10)), sig_of(np.zeros((0, 2)))
    words = np.array([other[0], q[0], empty[0], q[0], q[0]])
    bits = np.array([other[1], q[1], 0, q[1], q[1]], dtype=np.int32)
    records, rows = ref.similar(words, bits, [4, 2], [0, 0], [4, 5], 5, 3)
    assert records[0, :, 0].tolist() == [1, 3, 0] and records[0, :2, 1].tolist() == [65535, 65535] and records[0, 2, 1] < 30000
    assert rows[0, 4] == -1 and rows[0, 2] == 0                                # outside the range; against the empty scan
    assert (records[1, :, 1] == 0).all() and records[1, :, 0].tolist() == [0, 1, 2] and (rows[1] == 0).all()     # the empty query
    assert (records[1, :, 2:] == 0).all()
    # padding, an empty range, a range cut on both sides
    records, rows = ref.similar(words, bits, [4, 4, 4], [0, 3, -7], [2, 3, 99], 5, 4)
    assert records[0, :, 0].tolist() == [1, 0, -1, -1] and (records[0, 2:, 1:] == 0).all()
    assert (records[1, :, 0] == -1).all() and (rows[1] == -1).all()
    assert records[2, :, 0].tolist() == [1, 3, 4, 0]


# ── e. ranking, on the restatement ───────────────────────────────────────────
STORED, QUERIES, BEAMS = 120, 60, 720


@pytest.fixture(scope="module")
def room_run():
    """120 stored scans at random free poses of the single room and 60 queries, each within 0.5 m of a stored pose under any
    heading -> (stored poses, query poses, records of every query against all stored scans)."""
    from icpmi import synth
    rng = np.random.default_rng(20260)
    segs = synth.room_segments()

    def free_pose(near=None):
        while True:
            if near is None:
                x, y = rng.uniform(synth.ROOM[0], synth.ROOM[2]), rng.uniform(synth.ROOM[1], synth.ROOM[3])
            else:
                d, a = rng.uniform(0.0, 0.5), rng.uniform(-np.pi, np.pi)
                x, y = near[0] + d * np.cos(a), near[1] + d * np.sin(a)
            if synth._free_pose(x, y):
                return (x, y, rng.uniform(-np.pi, np.pi))

    stored = [free_pose() for _ in range(STORED)]
    queries = [free_pose(stored[k]) for k in rng.permutation(STORED)[:QUERIES]]
    words, bits = ref.signatures([synth.scan(p, 5000 + k, n_beams=BEAMS, segs=segs) for k, p in enumerate(stored)], TAB)
    records = []
    for k, p in enumerate(queries):
        w, b = ref.signature(synth.scan(p, 7000 + k, n_beams=BEAMS, segs=segs), TAB)
        rec, _ = ref.similar(np.concatenate([words, w[None]]), np.append(bits, b), [STORED], [0], [STORED], STORED, 5)
        records.append(rec[0])
    return np.array(stored), np.array(queries), np.array(records)


def test_a_stored_scan_of_the_place_is_in_the_top_five(room_run):
    stored, queries, records = room_run
    hits = first = 0
    for q, rec in zip(queries, records):
        near = np.hypot(*(stored[rec[:, 0], :2] - q[:2]).T) <= 1.0
        hits += bool(near.any())
        first += bool(near[0])
    print(f"a stored scan within 1 m: first for {first} of {QUERIES} queries, in the top five for {hits}")
    assert hits >= 0.9 * QUERIES


def test_the_winning_shift_gives_the_heading_to_two_sectors(room_run):
    stored, queries, records = room_run
    errors = []
    for q, rec in zip(queries, records):
        k = rec[0, 0]
        if np.hypot(*(stored[k, :2] - q[:2])) <= 1.0:
            err = ref.yaw_of(rec[0, 2]) - (q[2] - stored[k, 2])
            errors.append(abs((err + np.pi) % (2.0 * np.pi) - np.pi))
    errors = np.rad2deg(errors)
    print(f"|yaw error| over {len(errors)} queries whose neighbour ranks first: median {np.median(errors):.2f}, max {errors.max():.2f} degrees")
    assert len(errors) >= QUERIES // 2 and errors.max() <= 11.25


# ── f. the host logic of the Python layer ────────────────────────────────────
def test_signature_config_and_similar_args():
    from icpmi import history
    assert history.signature_config({}) == {"ring_width": 0.5, "min_range": 0.1}
    assert history.signature_config({"ring_width": 1, "min_range": 0.25}) == {"ring_width": 1.0, "min_range": 0.25}
    for bad in ({"ring_width": 0.0}, {"ring_width": -1.0}, {"min_range": 0.0}, {"min_range": np.inf}, {"ring_width": np.nan},
                {"rings": 16}):
        with pytest.raises(ValueError):
            history.signature_config(bad)
    ids, lo, hi = history.similar_args([10, 3, 12], 12, top_k=5, min_interval=4)
    assert all(a.dtype == np.int32 for a in (ids, lo, hi))
    assert ids.tolist() == [10, 3, 12] and lo.tolist() == [0, 0, 0] and hi.tolist() == [7, 0, 9]      # i kept iff id - i >= min_interval
    assert history.similar_args([5], 12)[2].tolist() == [6]                                          # min_interval 0: itself included
    ids, lo, hi = history.similar_args([10, 3], 12, lo=2, hi=[9, 100])
    assert lo.tolist() == [2, 2] and hi.tolist() == [9, 100]
    _, lo, hi = history.similar_args([1], 12, lo=-2 ** 40, hi=2 ** 40)
    assert lo.tolist() == [-2 ** 31] and hi.tolist() == [2 ** 31 - 1]            # clipped into int32: the device clips to the scans
    for kw in (dict(top_k=0), dict(top_k=65), dict(min_interval=-1), dict(lo=[1, 2, 3]), dict(hi=1.5), dict(lo=[[1, 2]])):
        with pytest.raises(ValueError):
            history.similar_args([10, 3], 12, **kw)
    with pytest.raises(ValueError):
        history.similar_args([13], 12)                                           # 12 is the staged source, 13 nobody
    with pytest.raises(ValueError):
        history.similar_args([-1], 12)


def test_similar_loop_candidates_filters_and_keeps_the_shape():
    import icpmi
    from icpmi import history
    assert icpmi.similar_loop_candidates is history.similar_loop_candidates
    asked = {}

    class Query:
        def run(self):
            asked["ran"] = True

        def unpack(self):
            return [[(7, 0.9, 0.1), (2, 0.5, -3.0), (4, 0.29, 0.0)]]

    class Hist:
        def similar(self, source, **kw):
            asked.update(kw, source=source)
            return Query()

    got = history.similar_loop_candidates(Hist(), 40, min_interval=30, max_candidates=3, min_score=0.3)
    assert got == [(7, 0.9), (2, 0.5)] and asked == {"ran": True, "source": 40, "top_k": 3, "min_interval": 30}
    assert [k for k, _ in got] == [7, 2]
    with pytest.raises(ValueError):
        history.similar_loop_candidates(Hist(), [1, 2], min_interval=30, max_candidates=3, min_score=0.3)
