"""The cases of tests/test_buffer_ends_particles_gpu.py: the particle filter's entries with every state array exactly n rows
and every workspace, planes and index buffer exactly as large as include/icpmi.h states (tests/buffer_ends.py has the
runner, DESIGN.md the inventory).  No test in here."""
import numpy as np

import gridbeam_ref as bref
import particles_global_ref as pgref
import particles_ref as pref
from buffer_ends import GRIDS, MIN_X, MIN_Y, RES, STATE, THRESHOLD, Case, field_of, planes_bytes_of

CASES = []
SIZES = (1, 255, 257, 1025, 4097)
MAX_ENTRIES = 4096
SEED, STEP = 0x123456789abcdef, 7


def _add(fn, id, **kw):
    CASES.append(Case(f"{fn.__name__}[{id}]", lambda b: fn(b, **kw)))


def _state(n, seed=0):
    rng = np.random.default_rng(400 + seed + n)
    pair_t = rng.uniform(-5.0, 5.0, (n, 2))
    theta = rng.uniform(-np.pi, np.pi, n)
    return pair_t, theta, np.stack([np.cos(theta), np.sin(theta)], axis=1)


def _u32(a):
    return np.asarray(a).astype(np.uint32)


# ── icpmi_pf_predict ─────────────────────────────────────────────────────────
def predict(b, n):
    pair_t, theta, cs = _state(n)
    control, sigma3 = (0.3, -0.1, 0.05), (0.02, 0.01, 0.03)
    p_t, p_th, p_cs = b.place(pair_t, "pair_t", STATE), b.place(theta, "theta", STATE), b.place(cs, "cos_sin", STATE)
    b.outputs.update(pair_t=None, theta=None, cos_sin=None)
    b.call = lambda short=None: b.L.icpmi_pf_predict(n, p_t, p_th, p_cs, *control, *sigma3, SEED, STEP, b.stream())
    b.twin = ("cos_sin",)                                        # the device library's sincos: not restated

    def expected():
        t, th = pref.predict(pair_t, theta, cs, control, sigma3, SEED, STEP)
        return {"pair_t": t, "theta": th}
    b.expected = expected


# ── icpmi_pf_weights ─────────────────────────────────────────────────────────
def weights(b, n, entries):
    rng = np.random.default_rng(500 + n + entries)
    shift = 2
    rec = np.zeros((n, bref.INTS), dtype=np.int32)
    rec[:, bref.SCORE] = -rng.integers(0, (entries + entries // 4 + 1) << shift, size=n)
    rec[:, bref.ROWS] = 50
    rec[rng.random(n) < 0.1, bref.STATUS] = bref.ST_EMPTY
    rec[-1, bref.STATUS] = bref.ST_OK                              # the last record counts
    table = _u32(rng.integers(0, 2 ** 20 + 5000, size=entries))   # (some above ICPMI_PF_MAX_WEIGHT: clipped)
    p_r, p_tab = b.place(rec, "records"), b.place(table, "wtable")
    p_w, p_s = b.out((n,), np.uint32, "w"), b.out((4,), np.int64, "sums")
    b.call = lambda short=None: b.L.icpmi_pf_weights(n, p_r, p_tab, entries, shift, p_w, p_s, b.stream())

    def expected():
        w, sums = pref.weights(rec, table, shift)
        return {"w": w, "sums": sums}
    b.expected = expected


# ── icpmi_pf_resample ────────────────────────────────────────────────────────
def resample(b, n):
    pair_t, theta, cs = _state(n)
    w = pref.weight_cases(n)["runs of zeros"] if n > 1 else _u32([5])
    p_w, p_t, p_th, p_cs = b.place(w, "w"), b.place(pair_t, "pair_t"), b.place(theta, "theta"), b.place(cs, "cos_sin")
    o_t, o_th, o_cs = b.out((n, 2), np.float64, "out_pair_t"), b.out((n,), np.float64, "out_theta"), b.out((n, 2), np.float64, "out_cos_sin")
    p_a, p_i = b.out((n,), np.int32, "ancestors"), b.out((4,), np.int32, "info")
    p_ws = b.query("workspace", "icpmi_pf_workspace_bytes", (n,))
    b.call = lambda short=None: b.L.icpmi_pf_resample(n, p_w, p_t, p_th, p_cs, o_t, o_th, o_cs, p_a, p_i, SEED, STEP, p_ws, b.size("workspace", short),
                                                      b.stream())

    def expected():
        anc, _, status = pref.resample(w, SEED, STEP)
        return {"out_pair_t": pair_t[anc], "out_theta": theta[anc], "out_cos_sin": cs[anc], "ancestors": anc,
                "info": np.array([status, 0, 0, 0], dtype=np.int32)}
    b.expected = expected


# ── icpmi_pf_estimate ────────────────────────────────────────────────────────
def estimate(b, n):
    pair_t, _, cs = _state(n)
    w = pref.weight_cases(n)["runs of zeros"] if n > 1 else _u32([5])
    p_w, p_t, p_cs = b.place(w, "w"), b.place(pair_t, "pair_t"), b.place(cs, "cos_sin")
    p_o = b.out((8,), np.float64, "out")
    p_ws = b.query("workspace", "icpmi_pf_workspace_bytes", (n,))
    b.call = lambda short=None: b.L.icpmi_pf_estimate(n, p_w, p_t, p_cs, p_o, p_ws, b.size("workspace", short), b.stream())
    b.twin = ("out",)                                            # a fixed summation order: the same bits as on roomy buffers

    def after(pattern):
        sums, mag = pref.estimate(w, pair_t, cs)                    # and the right value: long double sums of the device's terms
        got = b.arena.read("out").astype(np.longdouble)
        assert (np.abs(got - sums) <= mag * n * np.finfo(np.float64).eps).all(), (got, sums)
    b.after = after


# ── icpmi_pf_free_index, icpmi_pf_draw_uniform ───────────────────────────────
def _planes(b, q, packed):
    """The planes of exactly their bytes -> (pack, pointer): packed by icpmi_grid_occupancy_planes into the arena — the
    padding behind each plane then holds the pattern — or written by the host with zeros there."""
    ny, nx = q.shape
    if packed:
        p_q = b.place(q, "field")
        p_pl = b.query("planes", "icpmi_grid_occupancy_planes_bytes", (ny, nx), host=False)

        def pack(short=None):
            if short is not None:                                 # a refusal is being tested: nothing is launched
                return 0
            rc = b.L.icpmi_grid_occupancy_planes(p_q, ny, nx, THRESHOLD, p_pl, b.size("planes"), b.stream())
            b.sync()
            b.arena.freeze("planes")
            return rc
        return pack, p_pl
    need = int(b.L.icpmi_grid_occupancy_planes_bytes(ny, nx))
    b.sized["planes"] = ("icpmi_grid_occupancy_planes_bytes", (ny, nx), 0, True)      # (icpmi_pf_free_index takes no byte count of them)
    return (lambda short=None: 0), b.place(planes_bytes_of(*pgref.planes_of(q, THRESHOLD), need)[0], "planes")


def _index_layout(ny, nx, total):
    """-> (offset of free, offset of rank, words, the mask of the bytes include/icpmi.h defines)"""
    words = ny * ((nx + 31) // 32)
    a = lambda v: (v + 255) // 256 * 256                           # noqa: E731
    free, rank = a(4 * pgref.FREE_HEADER), a(4 * pgref.FREE_HEADER) + a(4 * words)
    mask = np.zeros(total, dtype=bool)
    mask[:4 * pgref.FREE_HEADER] = mask[free:free + 4 * words] = mask[rank:rank + 4 * words] = True
    return free, rank, words, mask


def _index_bytes(q, box, total):
    ny, nx = q.shape
    free, rank, words, _ = _index_layout(ny, nx, total)
    h, f, r = pgref.free_index(*pgref.planes_of(q, THRESHOLD), nx, box)
    buf = np.zeros(total, dtype=np.uint8)
    buf[:h.nbytes], buf[free:free + 4 * words], buf[rank:rank + 4 * words] = h.view(np.uint8), f.view(np.uint8), r.view(np.uint8)
    return buf, (h, f, r)


def _boxes(ny, nx):
    """The whole grid, and a box that cuts two words of a row (or what the grid has of them)."""
    return {"whole": (0, 0, nx, ny), "cut": (min(3, nx - 1), min(1, ny - 1), max(nx - 2, 1) if nx <= 40 else 39, max(ny - 1, 1))}


def free_index(b, ny, nx, box, packed):
    q = field_of(ny, nx)
    cells = _boxes(ny, nx)[box]
    pack, p_pl = _planes(b, q, packed)
    p_ix = b.query("index", "icpmi_pf_free_index_bytes", (ny, nx))
    total = b.arena.nbytes("index")
    b.outputs["index"] = _index_layout(ny, nx, total)[3]

    def call(short=None):
        return pack(short) or b.L.icpmi_pf_free_index(p_pl, ny, nx, *cells, p_ix, b.size("index", short), b.stream())
    b.call = call
    b.expected = lambda: {"index": _index_bytes(q, cells, total)[0]}


def draw_uniform(b, n, m, ny=37, nx=53):
    q = field_of(ny, nx)
    cells = _boxes(ny, nx)["cut"]
    pair_t, theta, cs = _state(n, seed=1)
    anc = np.arange(n, dtype=np.int32)
    theta0, span = 0.4, 1.5
    pack, p_pl = _planes(b, q, False)
    p_ix = b.query("index", "icpmi_pf_free_index_bytes", (ny, nx), host=False)
    p_t, p_th, p_cs = b.place(pair_t, "pair_t", STATE), b.place(theta, "theta", STATE), b.place(cs, "cos_sin", STATE)
    p_a = b.place(anc, "ancestors", STATE)
    p_i = b.out((4,), np.int32, "info")
    b.outputs.update(pair_t=None, theta=None, cos_sin=None, ancestors=None)

    def call(short=None):
        rc = b.L.icpmi_pf_free_index(p_pl, ny, nx, *cells, p_ix, b.size("index"), b.stream())
        b.sync()
        b.arena.freeze("index")                                   # the draw only reads it
        return rc or b.L.icpmi_pf_draw_uniform(n, m, p_ix, MIN_X, MIN_Y, RES, theta0, span, p_t, p_th, p_cs, p_a, p_i, SEED, STEP, b.stream())
    b.call = call
    b.twin = ("cos_sin",)

    def expected():
        index = _index_bytes(q, cells, int(b.L.icpmi_pf_free_index_bytes(ny, nx)))[1]
        drawn, t, th, _ = pgref.draw_uniform(index, n, m, MIN_X, MIN_Y, RES, theta0, span, SEED, STEP)
        assert t is not None, "the case's box has no free cell"
        out_t, out_th, out_a = pair_t.copy(), theta.copy(), anc.copy()
        out_t[drawn], out_th[drawn], out_a[drawn] = t, th, -1
        return {"pair_t": out_t, "theta": out_th, "ancestors": out_a, "info": np.array([0, int(index[0][0]), 0, 0], dtype=np.int32)}
    b.expected = expected


# 4 096 particles and a 64 x 32 grid besides: every array of the workspace and of the index then ends exactly on a 256-byte
# granule of the layout, with no padding behind the last one
GRANULE_N, GRANULE_GRID = 4096, (64, 32)
for _n in SIZES:
    _add(predict, f"n{_n}", n=_n)
for _n in SIZES + (GRANULE_N,):
    _add(resample, f"n{_n}", n=_n)
    _add(estimate, f"n{_n}", n=_n)
for _n, _e in zip(SIZES, (1, 8, MAX_ENTRIES, 8, MAX_ENTRIES)):
    _add(weights, f"n{_n}-entries{_e}", n=_n, entries=_e)
for _ny, _nx in GRIDS + (GRANULE_GRID,):
    for _box in ("whole", "cut"):
        _add(free_index, f"{_ny}x{_nx}-{_box}-packed", ny=_ny, nx=_nx, box=_box, packed=True)
    _add(free_index, f"{_ny}x{_nx}-whole-zero-padding", ny=_ny, nx=_nx, box="whole", packed=False)
for _n, _m in ((1, 1), (257, 3), (1025, 1025)):
    _add(draw_uniform, f"n{_n}-m{_m}", n=_n, m=_m)
