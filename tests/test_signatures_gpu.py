"""Appearance signatures on the device (include/icpmi.h: icpmi_history_signatures_add, icpmi_history_similar; icpmi/history.py:
``ScanHistory(signature=...)``, ``signatures``, ``similar``, ``similar_loop_candidates``): everything BIT-EQUAL to the NumPy
restatement of tests/signatures_ref.py, on which tests/test_signatures_cpu.py asserts what the signatures are good for.

The two entries are driven directly on small raw cloud sets and stores (every row count and every launch shape), and
through the Python layer (adding at once and one by one, growth, a staged source, the re-preparation after a scan above
2 048 rows, loop candidates into ``match``)."""
import ctypes as C
import functools

import numpy as np
import pytest

import signatures_ref as ref
import stream_cases_signatures  # noqa: F401  (registers the stream workload: tests/test_streams_gpu.py runs it behind a delay)
from buffer_ends_signatures import _store

pytestmark = pytest.mark.gpu

TAB = ref.tables()
TILE = 64                                                     # ICPMI_SIG_TILE: candidates a workgroup of the pair kernel takes


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert _lib.SIG_TILE == TILE
    return torch


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_signatures(clouds, first=0, n_new=None, tab_args=(0.5, 0.1)):
    """icpmi_history_signatures_add on a raw cloud set of exactly these clouds -> (words uint64 [n][32], bits int32 [n])."""
    import torch
    import icpmi
    from icpmi import _lib
    S = len(clouds)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    rows = max(int(off[-1]), 1)
    pts = dev(np.concatenate(list(clouds) + [np.zeros((rows - int(off[-1]), 2))], axis=0))
    off_dev, tables = dev(off), dev(ref.packed_tables(*tab_args))
    sig = torch.full((S, ref.RINGS), -1, dtype=torch.int64, device="cuda")
    bits = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    h = _lib.History(pts=pts.data_ptr(), off_dev=off_dev.data_ptr(), scan_capacity=S, row_capacity=rows)
    rc = icpmi.lib().icpmi_history_signatures_add(C.byref(h), P(sig), P(bits), P(tables), off.ctypes.data_as(C.c_void_p), first,
                                                  S - first if n_new is None else n_new, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sig.cpu().numpy().view(np.uint64), bits.cpu().numpy()


def device_similar(words, bits, q, lo, hi, n_scans, top_k, with_all=True):
    """icpmi_history_similar on a store uploaded as it is -> (records, rows or None); every output starts out as garbage."""
    import torch
    import icpmi
    from icpmi import _lib
    L = icpmi.lib()
    q, lo, hi = (np.ascontiguousarray(v, dtype=np.int32) for v in (q, lo, hi))
    sig, sb, dq, dlo, dhi = dev(words.view(np.int64)), dev(bits), dev(q), dev(lo), dev(hi)
    rec = torch.full((len(q), top_k, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rows = torch.full((len(q), n_scans), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if with_all else None
    ws = torch.full((L.icpmi_history_similar_workspace_bytes(len(q), n_scans, top_k),), 0x5a, dtype=torch.uint8, device="cuda")
    h = _lib.History(scan_capacity=len(words), row_capacity=1)
    rc = L.icpmi_history_similar(C.byref(h), P(sig), P(sb), P(dq), len(q), P(dlo), P(dhi), n_scans, top_k, P(rec), P(rows), P(ws), ws.numel(),
                                 stream())
    assert rc == 0
    torch.cuda.synchronize()
    return rec.cpu().numpy(), None if rows is None else rows.cpu().numpy()


def sized(points, n):
    """A scan cut or tiled to n rows (a tiled copy is moved a little: new rows, not repeats)."""
    reps = -(-n // len(points)) if n else 1
    return np.concatenate([points * (1.0 + 0.01 * k) for k in range(reps)], axis=0)[:n]


@pytest.fixture(scope="module")
def scans():
    from icpmi import synth
    poses = synth.trajectory(12, start=(-8.0, -0.5, 0.0), step=0.3)
    return [synth.scan(p, 4300 + i, n_beams=720) for i, p in enumerate(poses)]


# ── g. signatures ────────────────────────────────────────────────────────────
ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 2048, 4096)


def test_signatures_of_every_row_count(gpu, scans):
    clouds = [sized(scans[k % len(scans)], n) for k, n in enumerate(ROWS)] + [sized(scans[0], 9000)]     # nothing caps the rows
    words, bits = device_signatures(clouds)
    want_w, want_b = ref.signatures(clouds, TAB)
    assert np.array_equal(words, want_w) and np.array_equal(bits, want_b)
    assert bits[0] == 0 and not words[0].any() and bits[-1] > bits[2] > 0


def test_signatures_of_the_hand_made_clouds(gpu):
    made = ref.edge_clouds()
    clouds = list(made.values()) + [ref.full_ring(), np.concatenate(list(made.values()))]
    words, bits = device_signatures(clouds)
    want_w, want_b = ref.signatures(clouds, TAB)
    assert np.array_equal(words, want_w) and np.array_equal(bits, want_b)
    assert dict(zip(made, bits.tolist())) == {"ring_edges": 3, "axes": 4, "sector_boundary": 2, "not_finite": 0, "below_min_range": 0,
                                              "past_reach": 0}
    # other rings: the tables alone carry ring_width and min_range
    words, bits = device_signatures(clouds, tab_args=(0.25, 0.3))
    want_w, want_b = ref.signatures(clouds, ref.tables(0.25, 0.3))
    assert np.array_equal(words, want_w) and np.array_equal(bits, want_b)


def test_a_range_leaves_the_other_scans_alone(gpu, scans):
    clouds = [sized(s, n) for s, n in zip(scans, (100, 300, 64, 720, 5))]
    words, bits = device_signatures(clouds, first=1, n_new=3)
    want_w, want_b = ref.signatures(clouds, TAB)
    assert np.array_equal(words[1:4], want_w[1:4]) and np.array_equal(bits[1:4], want_b[1:4])
    assert (words[[0, 4]] == np.uint64(2 ** 64 - 1)).all() and (bits[[0, 4]] == -1).all()


def new_history(**kw):
    from icpmi import ScanHistory
    return ScanHistory(voxel_size=0.04, normal_k=12, rotation_voxel_size=0.15, signature={}, **kw)


def test_history_keeps_signatures_through_adds_growth_and_a_big_scan(gpu, scans):
    want_w, want_b = ref.signatures(scans, TAB)
    h = new_history(scan_capacity=2, row_capacity=2048)
    assert h.add_many(scans[:2]) == [0, 1]
    first = h.signatures()
    assert np.array_equal(first[0], want_w[:2]) and np.array_equal(first[1], want_b[:2]) and first[0].dtype == np.uint64
    generation = h.layout_generation
    h.add(scans[2])                                                              # grows: 2 -> 4 scans
    h.add_many(scans[3:7])                                                       # grows again: 4 -> 8
    assert h.layout_generation >= generation + 2 and h.scan_capacity == 8
    words, bits = h.signatures()
    assert np.array_equal(words, want_w[:7]) and np.array_equal(bits, want_b[:7])
    # a scan above 2 048 rows: the earlier scans are prepared again, their signatures are left alone
    big = sized(scans[7], 4096)
    h.sig[:7] += 1                                                               # marked: a rewrite would undo it
    assert h.add(big) == 7 and not h.allow_polar
    words, bits = h.signatures()
    assert np.array_equal(words[:7], want_w[:7] + np.uint64(1))
    assert np.array_equal(words[7], ref.signature(big, TAB)[0]) and bits[7] == ref.signature(big, TAB)[1]
    w, b = h.signatures([7, 0, 7])
    assert np.array_equal(w, words[[7, 0, 7]]) and np.array_equal(b, bits[[7, 0, 7]])
    # with signature=None nothing of this exists
    from icpmi import ScanHistory
    plain = ScanHistory(voxel_size=0.04, normal_k=12, rotation_voxel_size=0.15, scan_capacity=2)
    assert plain.sig_cfg is None and not hasattr(plain, "sig") and not hasattr(plain, "sig_tables")
    with pytest.raises(ValueError, match="signature=None"):
        plain.similar(0)
    with pytest.raises(ValueError, match="signature=None"):
        plain.signatures()


@pytest.fixture(scope="module")
def history(gpu, scans):
    h = new_history(scan_capacity=16)
    assert h.add_many(scans) == list(range(len(scans)))
    return h


def test_a_staged_source(gpu, scans, history):
    from icpmi import _lib, synth
    h, n = history, len(scans)
    words, bits = ref.signatures(scans, TAB)
    source = synth.scan((-6.1, -0.4, 2.0), 4400, n_beams=500)
    q = h.similar(source, top_k=4, all_scores=True)
    q.run()
    found = q.unpack()
    sw, sb = ref.signature(source, TAB)
    want_rec, want_rows = ref.similar(np.concatenate([words, sw[None]]), np.append(bits, sb), [n], [0], [n + 1], n, 4)
    assert np.array_equal(q.records, want_rec) and np.array_equal(q.all, want_rows)
    assert len(h) == n and np.array_equal(h.signatures()[0], words)              # not added, nobody's signature touched
    assert np.array_equal(h.sig[n].cpu().numpy().view(np.uint64), sw) and int(h.sig_bits[n]) == sb
    assert [k for k, _, _ in found[0]] == want_rec[0, :, 0].tolist()
    assert [s for _, s, _ in found[0]] == (want_rec[0, :, 1] / 65535.0).tolist()
    assert np.array_equal([y for _, _, y in found[0]], ref.yaw_of(want_rec[0, :, 2]))
    # staging again overwrites it: the first query refuses to run
    h.similar(scans[0][:100])
    with pytest.raises(_lib.IcpmiError, match="staged source"):
        q.run()


def test_similar_by_id_through_the_python_layer(gpu, scans, history):
    h, n = history, len(scans)
    words, bits = ref.signatures(scans, TAB)
    q = h.similar([n - 1, 4, 0], top_k=3, min_interval=2, all_scores=True)
    q.run()
    found = q.unpack()
    want_rec, want_rows = ref.similar(words, bits, [n - 1, 4, 0], [0, 0, 0], [n - 2, 3, -1], n, 3)
    assert np.array_equal(q.records, want_rec) and np.array_equal(q.all, want_rows)
    assert found[2] == [] and len(found[0]) == 3 and all(0.0 <= s <= 1.0 for _, s, _ in found[0])
    one = h.similar(5)                                                           # itself included: score 1, shift 0
    one.run()
    assert one.unpack()[0][0] == (5, 1.0, 0.0) and one.all is None and one.records.shape == (1, 10, 4)
    assert (one.records[0, 6:, 0] == -1).all() and (one.records[0, 6:, 1:] == 0).all()               # six candidates, four paddings


# ── h. query records ─────────────────────────────────────────────────────────
@functools.lru_cache(maxsize=None)
def store(n_scans):
    return _store(n_scans)


def queries_of(n_scans, n_queries, seed):
    """Query ids over [0, n_scans] (the staged slot included), with full ranges, ranges cut on both sides, empty ranges and
    ranges far outside, in turn."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, n_scans + 1, size=n_queries)
    q[0] = n_scans // 2                                                          # a self-match in range
    lo, hi = np.zeros(n_queries, dtype=np.int64), np.full(n_queries, n_scans, dtype=np.int64)
    for i in range(1, n_queries):
        kind = i % 5
        if kind == 1:
            lo[i], hi[i] = sorted(rng.integers(0, n_scans + 1, size=2))
        elif kind == 2:
            lo[i] = hi[i] = rng.integers(0, n_scans + 1)
        elif kind == 3:
            lo[i], hi[i] = -5, n_scans + 1000
        elif kind == 4:
            lo[i], hi[i] = n_scans // 3, n_scans // 3 + 1
    return q, lo, hi


@pytest.mark.parametrize("n_scans", [1, 2, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("n_queries", [1, 3, 65])
def test_records_and_rows(gpu, n_scans, n_queries):
    words, bits = store(n_scans)
    q, lo, hi = queries_of(n_scans, n_queries, 31 * n_scans + n_queries)
    for top_k in (1, 5, 64):
        want_rec, want_rows = ref.similar(words, bits, q, lo, hi, n_scans, top_k)
        rec, rows = device_similar(words, bits, q, lo, hi, n_scans, top_k)
        assert np.array_equal(rows, want_rows), (top_k, np.argwhere(rows != want_rows)[:4])
        assert np.array_equal(rec, want_rec), (top_k, np.argwhere(rec != want_rec)[:4])
        assert rec[0, 0].tolist()[:3] == [n_scans // 2, 65535, 0]                # the self-match
        if top_k > n_scans:
            assert (rec[:, n_scans:, 0] == -1).all() and (rec[:, n_scans:, 1:] == 0).all()           # padding records
    rec, rows = device_similar(words, bits, q, lo, hi, n_scans, 5, with_all=False)                   # the rows in the workspace
    assert rows is None and np.array_equal(rec, ref.similar(words, bits, q, lo, hi, n_scans, 5)[0])


def test_query_ids_that_name_no_cloud_have_no_candidates(gpu):
    words, bits = store(65)
    rec, rows = device_similar(words, bits, [-1, 66, 2 ** 31 - 1, 3], [0] * 4, [65] * 4, 65, 5)
    assert (rec[:3, :, 0] == -1).all() and (rec[:3, :, 1:] == 0).all() and (rows[:3] == -1).all()
    assert rec[3, 0].tolist()[:3] == [3, 65535, 0]


def test_the_pairs_of_every_shift_and_the_quarter_turns(gpu):
    clouds = []
    for s in range(64):
        clouds += list(ref.shift_pair(s, seed=s))                                # query 2 s, candidate 2 s + 1
    base = np.random.default_rng(77).uniform(-12.0, 12.0, size=(300, 2))
    clouds += [ref.quarter_turn(base, k) for k in range(4)] + [ref.full_ring(), ref.full_ring(), np.zeros((0, 2))]
    words, bits = device_signatures(clouds)
    want_w, want_b = ref.signatures(clouds, TAB)
    assert np.array_equal(words, want_w) and np.array_equal(bits, want_b)
    n = len(clouds)
    q = list(range(0, 128, 2)) + [128] * 3 + [133, 134]
    lo = list(range(1, 129, 2)) + [129, 130, 131] + [132, 0]
    hi = [v + 1 for v in lo[:-1]] + [n]
    rec, rows = device_similar(words, bits, q, lo, hi, n, 2)
    want_rec, want_rows = ref.similar(words, bits, q, lo, hi, n, 2)
    assert np.array_equal(rec, want_rec) and np.array_equal(rows, want_rows)
    assert rec[:64, 0, 2].tolist() == list(range(64)) and (rec[:64, 0, 1] == 65535).all()           # every shift wins once
    assert rec[64:67, 0, 2].tolist() == [48, 32, 16] and (rec[64:67, 0, 1] == 65535).all()           # the base against its turns
    assert rec[67, 0].tolist() == [132, 65535, 0, 64]                            # all 64 shifts tie: the lowest
    assert (rec[68, :, 1] == 0).all() and rec[68, :, 0].tolist() == [0, 1]       # the empty scan scores 0 against everything


# ── i. loop candidates ───────────────────────────────────────────────────────
def test_similar_loop_candidates_into_match(gpu):
    import icpmi
    from icpmi import synth
    poses = synth.loop_trajectory(40)
    segs = synth.maze_segments()
    loop = [synth.scan(p, 4500 + i, n_beams=360, segs=segs) for i, p in enumerate(poses)]
    h = new_history(scan_capacity=64)
    h.add_many(loop)
    sid = len(loop) - 1
    cands = icpmi.similar_loop_candidates(h, sid, min_interval=10, max_candidates=5, min_score=0.2)
    words, bits = ref.signatures(loop, TAB)
    rec, _ = ref.similar(words, bits, [sid], [0], [sid - 10 + 1], len(loop), 5)
    want = [(int(r[0]), r[1] / 65535.0) for r in rec[0] if r[0] >= 0 and r[1] / 65535.0 >= 0.2]
    assert cands == want and len(cands) >= 1
    print("loop candidates by appearance:", [(k, round(s, 3)) for k, s in cands])
    m = h.match(sid, [k for k, _ in cands], error_threshold=1e-10, max_iterations=40)
    m.run()
    R, t, err, info = m.unpack()
    assert len(err) == len(cands) and np.isfinite(err).all()
