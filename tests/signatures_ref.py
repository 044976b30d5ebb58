"""NumPy restatement of the appearance signatures of include/icpmi.h (icpmi_history_signatures_add, icpmi_history_similar):
the row rule, the score, the shift and the selection, written from the header's contract and from nothing in csrc/.  The
device results are asserted bit-equal to this (tests/test_signatures_gpu.py), and what the signatures are good for —
ranking the scans of one place first, whatever the heading — is asserted on this alone, on a CPU
(tests/test_signatures_cpu.py).  No test in here; no torch, no library.

Everything is integers except the row rule, whose floating-point steps are single IEEE operations on float64 arrays
(NumPy fuses nothing), in the order the header gives them.
"""
import numpy as np

RINGS, SECTORS, MAX_TOP, TABLE_DOUBLES = 32, 64, 64, 63
REC_ID, REC_SCORE, REC_SHIFT, REC_BEST = 0, 1, 2, 3


def tables(ring_width=0.5, min_range=0.1):
    """(edge2 [33], bc [16], bs [16]) — bc[k] = cos(k pi / 32), bs[k] = sin(k pi / 32); index 0 is not part of the store."""
    edge = min_range + np.arange(RINGS + 1, dtype=np.float64) * ring_width
    a = np.arange(16, dtype=np.float64) * np.pi / 32
    return edge * edge, np.cos(a), np.sin(a)


def packed_tables(ring_width=0.5, min_range=0.1):
    """The store's 63 doubles: edge2, bc[1 .. 15], bs[1 .. 15]."""
    edge2, bc, bs = tables(ring_width, min_range)
    return np.concatenate([edge2, bc[1:], bs[1:]])


def cells(points, tab):
    """(ring, sector, kept) of every row: the row rule of the header."""
    edge2, bc, bs = tab
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = x * x + y * y
        ring = (d2[:, None] >= edge2[None, :]).sum(axis=1) - 1
        q = np.where(y >= 0, np.where(x > 0, 0, 1), np.where(x < 0, 2, 3))
        u = np.choose(q, [x, y, -x, -y])
        v = np.choose(q, [y, -x, -y, x])
        sector = 16 * q + (v[:, None] * bc[None, 1:] >= u[:, None] * bs[None, 1:]).sum(axis=1)
    return ring, sector, (ring >= 0) & (ring < RINGS)


def signature(points, tab):
    """(words uint64 [32], bits int) of one cloud."""
    ring, sector, kept = cells(points, tab)
    words = np.zeros(RINGS, dtype=np.uint64)
    np.bitwise_or.at(words, ring[kept], np.uint64(1) << sector[kept].astype(np.uint64))
    return words, int(unpack(words).sum())


def signatures(clouds, tab):
    """(words uint64 [n][32], bits int32 [n]) of a list of clouds."""
    got = [signature(c, tab) for c in clouds]
    return (np.array([w for w, _ in got], dtype=np.uint64).reshape(len(got), RINGS),
            np.array([b for _, b in got], dtype=np.int32))


def unpack(words):
    """(..., 32) uint64 -> (..., 32, 64) uint8: element [r][s] is bit s of word r."""
    w = np.asarray(words, dtype=np.uint64)
    return ((w[..., None] >> np.arange(SECTORS, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def rotl(words, s):
    w, s = np.asarray(words, dtype=np.uint64), np.uint64(int(s) % 64)
    return w if s == 0 else (w << s) | (w >> (np.uint64(64) - s))


def intersections(a_words, b_words):
    """inter[n][s] = sum over r of popcount(A[r] & rotl64(B[n][r], s)) for the candidates B (n, 32) -> int64 (n, 64).  Bit j
    of rotl(B, s) is bit j - s of B: inter(s) = sum over j of A[j + s] B[j], one exact float32 product of 0 / 1 matrices."""
    a = unpack(a_words).astype(np.float32)                                           # (32, 64)
    turned = np.stack([np.roll(a, -s, axis=1) for s in range(SECTORS)], axis=0)      # [s][r][j] = A[r][j + s]
    b = unpack(b_words).astype(np.float32).reshape(-1, RINGS * SECTORS)
    return np.rint(b @ turned.reshape(SECTORS, -1).T).astype(np.int64)


def compare(a_words, a_bits, b_words, b_bits):
    """(score, shift, best) int64 [n] of the query A against the candidates B: the header's best, lowest shift and score."""
    inter = intersections(a_words, np.asarray(b_words, dtype=np.uint64).reshape(-1, RINGS))
    best = inter.max(axis=1)
    shift = inter.argmax(axis=1)                                                     # the first of equal values
    union = int(a_bits) + np.asarray(b_bits, dtype=np.int64).reshape(-1) - best
    score = np.where(union != 0, (best * 65535) // np.where(union != 0, union, 1), 0)
    return score, shift.astype(np.int64), best


def similar(words, bits, query_ids, lo, hi, n_scans, top_k):
    """(records int32 [nq][top_k][4], rows int32 [nq][n_scans]) of icpmi_history_similar.  words / bits: the store, indexed by
    cloud (a staged source at n_scans included)."""
    nq = len(query_ids)
    records = np.zeros((nq, top_k, 4), dtype=np.int32)
    records[:, :, REC_ID] = -1
    rows = np.full((nq, n_scans), -1, dtype=np.int32)
    for i, q in enumerate(query_ids):
        a, b = max(int(lo[i]), 0), min(int(hi[i]), n_scans)
        if not 0 <= q < len(words) or a >= b:
            continue
        score, shift, best = compare(words[q], bits[q], words[a:b], bits[a:b])
        rows[i, a:b] = (score << 8) | shift
        ids = np.arange(a, b, dtype=np.int64)
        order = np.argsort(((65535 - score) << 32) | ids, kind="stable")[:top_k]
        records[i, :len(order)] = np.stack([ids[order], score[order], shift[order], best[order]], axis=1)
    return records, rows


def yaw_of(shift):
    """Heading of the query relative to the candidate, in (-pi, pi]: - shift * 2 pi / 64."""
    yaw = -(np.asarray(shift, dtype=np.float64) % SECTORS) * (2.0 * np.pi / SECTORS)
    return np.where(yaw <= -np.pi, yaw + 2.0 * np.pi, yaw)


# ── hand-made clouds ─────────────────────────────────────────────────────────
def sector_centre(s, r=1.0):
    """A row in the middle of sector s at range r."""
    a = (s + 0.5) * 2.0 * np.pi / SECTORS
    return np.array([r * np.cos(a), r * np.sin(a)])


def shift_pair(s, seed=0):
    """(query cloud, candidate cloud) whose unique best shift is s: one row per chosen sector centre in ring 1 — an
    irregular set of sectors, so that no other rotation maps it onto itself — the query's sectors being the candidate's
    moved on by s (rotl by s of the candidate's word is the query's)."""
    rng = np.random.default_rng(1000 + seed)
    base = np.flatnonzero(rng.random(SECTORS) < 0.4)
    if len(base) < 3:
        base = np.array([0, 1, 5])
    cand = np.array([sector_centre(j, 0.9) for j in base])
    query = np.array([sector_centre((j + s) % SECTORS, 0.9) for j in base])
    return query, cand


def full_ring(r=0.9):
    """One row in every sector of one ring: every rotation is as good as any."""
    return np.array([sector_centre(j, r) for j in range(SECTORS)])


def quarter_turn(points, k=1):
    """(x, y) -> (-y, x), k times: exact."""
    p = np.asarray(points, dtype=np.float64)
    for _ in range(k % 4):
        p = np.stack([-p[:, 1], p[:, 0]], axis=1)
    return p


def edge_clouds(ring_width=0.5, min_range=0.1):
    """The hand-made clouds of the CPU and GPU tests -> {name: (n, 2) array}.  tests/test_signatures_cpu.py states the literal
    signature of each."""
    edge2, bc, bs = tables(ring_width, min_range)
    e = np.sqrt(edge2)                                          # only to place rows NEAR a ring edge; the exact ones are below
    up, down = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)      # noqa: E731
    out = {}
    # rows on the x axis whose squared range is exactly edge2[j]: x = the edge itself, as x * x is how edge2 was made
    edge = min_range + np.arange(RINGS + 1, dtype=np.float64) * ring_width
    out["ring_edges"] = np.array([[edge[j], 0.0] for j in (0, 1, 31, 32)])
    out["axes"] = np.array([[1.0, 0.0], [1.0, -0.0], [0.0, 1.0], [-0.0, 1.0], [-1.0, 0.0], [-1.0, -0.0], [0.0, -1.0], [-0.0, -1.0]])
    k = 5
    on = np.array([bc[k], bs[k]]) * 2.0
    out["sector_boundary"] = np.array([on, [on[0], up(on[1])], [on[0], down(on[1])]])
    out["not_finite"] = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [0.0, 0.0], [-0.0, 0.0]])
    out["below_min_range"] = np.array([[down(min_range), 0.0], [0.0, -0.05]])
    out["past_reach"] = np.array([[up(e[32]), 0.0], [100.0, 100.0], [0.0, 1e200]])
    return out
