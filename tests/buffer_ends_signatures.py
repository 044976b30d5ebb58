"""The cases of tests/test_buffer_ends_signatures_gpu.py: the appearance signatures' entries with the signature tables, the
records, the score rows and the workspace exactly as large as include/icpmi.h states (tests/buffer_ends.py has the runner).
tests/test_signatures_cpu.py runs the CPU half — exact sizes and the refusal of one byte less.  No test in here."""
import ctypes as C

import numpy as np

import signatures_ref as ref
from buffer_ends import Case, host

CASES = []
TAB = ref.tables()


def _add(fn, id, **kw):
    CASES.append(Case(f"{fn.__name__}[{id}]", lambda b: fn(b, **kw)))


def _clouds(rows, seed=0):
    """Clouds of ``rows`` rows around the sensor out to 20 m: past the reach of 16.1 m, with a NaN row and a zero row in each
    cloud of more than two rows."""
    rng = np.random.default_rng(600 + seed + sum(rows))
    out = []
    for n in rows:
        ang, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, 20.0, n)
        p = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
        if n > 2:
            p[n // 2], p[n // 3] = (np.nan, 1.0), (0.0, 0.0)
        out.append(p)
    return out


def _history(b, pts_ptr, off_ptr, scans, rows):
    from icpmi import _lib
    return _lib.History(pts=pts_ptr.value, off_dev=off_ptr.value, scan_capacity=scans, row_capacity=rows)


# ── icpmi_history_signatures_add ─────────────────────────────────────────────
def signatures_add(b, rows, first, n_new):
    """A store of exactly len(rows) scans over raw rows of exactly their number; the range [first, first + n_new) is written."""
    clouds = _clouds(rows)
    S = len(rows)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    total = max(int(off[-1]), 1)
    pts = np.concatenate(clouds + [np.zeros((total - int(off[-1]), 2))], axis=0)
    p_pts, p_off, p_tab = b.place(pts, "pts"), b.place(off, "off"), b.place(ref.packed_tables(), "tables")
    written = np.zeros(S, dtype=bool)
    written[first:first + n_new] = True
    p_sig = b.out((S, ref.RINGS), np.uint64, "sig", mask=written[:, None], untouched=~written[:, None])
    p_bits = b.out((S,), np.int32, "sig_bits", mask=written, untouched=~written)
    h = _history(b, p_pts, p_off, S, total)
    b.call = lambda short=None: b.L.icpmi_history_signatures_add(C.byref(h), p_sig, p_bits, p_tab, host(off), first, n_new, b.stream())

    def expected():
        words, bits = ref.signatures(clouds, TAB)
        return {"sig": words, "sig_bits": bits}
    b.expected = expected


# ── icpmi_history_similar ────────────────────────────────────────────────────
def _store(n_scans, seed=0):
    """Signatures of n_scans + 1 clouds (the last a staged source): a few places seen under several headings, so that scores tie
    and differ."""
    rng = np.random.default_rng(700 + seed + n_scans)
    places = [_clouds([200], seed=k)[0] for k in range(4)]
    clouds = []
    for c in range(n_scans + 1):
        p = places[c % 4][rng.random(200) < 0.8]
        a = rng.integers(0, 64) * 2.0 * np.pi / 64
        clouds.append(p @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]))
    return ref.signatures(clouds, TAB)


def similar(b, n_scans, queries, top_k, lo, hi, with_all):
    words, bits = _store(n_scans)
    S = n_scans + 1
    q = np.asarray(queries, dtype=np.int32)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.int32), q.shape).copy() for v in (lo, hi))
    p_sig, p_bits = b.place(words, "sig"), b.place(bits, "sig_bits")
    p_q, p_lo, p_hi = b.place(q, "query_ids"), b.place(lo, "lo"), b.place(hi, "hi")
    p_rec = b.out((len(q), top_k, 4), np.int32, "out_records")
    p_all = b.out((len(q), n_scans), np.int32, "out_all") if with_all else None
    p_ws = b.query("workspace", "icpmi_history_similar_workspace_bytes", (len(q), n_scans, top_k))
    from icpmi import _lib
    h = _lib.History(scan_capacity=S, row_capacity=1)
    b.call = lambda short=None: b.L.icpmi_history_similar(C.byref(h), p_sig, p_bits, p_q, len(q), p_lo, p_hi, n_scans, top_k, p_rec, p_all,
                                                          p_ws, b.size("workspace", short), b.stream())

    def expected():
        records, rows = ref.similar(words, bits, q, lo, hi, n_scans, top_k)
        return {"out_records": records, "out_all": rows} if with_all else {"out_records": records}
    b.expected = expected


_add(signatures_add, "one-scan-one-row", rows=(1,), first=0, n_new=1)
_add(signatures_add, "no-rows", rows=(0, 0), first=0, n_new=2)
_add(signatures_add, "all-of-five", rows=(257, 0, 64, 1, 4096), first=0, n_new=5)
_add(signatures_add, "middle-of-five", rows=(63, 255, 65, 2048, 7), first=1, n_new=3)
_add(signatures_add, "last", rows=(300, 256, 1025), first=2, n_new=1)
for _n, _q, _k in ((1, (0,), 1), (63, (62, 0, 63), 5), (64, (64,), 64), (65, (1, 64, 65), 5), (257, (256, 100, 257), 64)):
    _add(similar, f"n{_n}-q{len(_q)}-top{_k}-all", n_scans=_n, queries=_q, top_k=_k, lo=0, hi=_n, with_all=True)
    _add(similar, f"n{_n}-q{len(_q)}-top{_k}", n_scans=_n, queries=_q, top_k=_k, lo=0, hi=_n, with_all=False)
_add(similar, "n130-cut-ranges", n_scans=130, queries=(129, 5, 70, 130), top_k=5, lo=(60, 0, 70, -5), hi=(70, 0, 1000, 129), with_all=True)
