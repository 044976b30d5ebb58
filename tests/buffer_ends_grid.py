"""The cases of tests/test_buffer_ends_grid_gpu.py: every grid entry with each device buffer exactly as large as
include/icpmi.h states (tests/buffer_ends.py has the runner, DESIGN.md the inventory).  No test in here."""
import numpy as np

import gridbeam_ref as bref
import gridcast_ref as cref
import gridcheck_ref as kref
import gridmatch_ref as gref
import gridmatch_wide_ref as wref
import gridmoments_ref as mref
import likelihood_ref as lref
import particles_global_ref as pgref
from buffer_ends import (GRIDS, MIN_X, MIN_Y, RES, ROW_SETS, SCRATCH, STATE, THRESHOLD, Case, clouds_of, field_of, host, pair_clouds_of,
                         planes_bytes_of, poses_of)

CASES = []


def _log_odds(ny, nx):
    rng = np.random.default_rng(ny * 1000 + nx)
    lo = rng.uniform(-9.0, 9.0, (ny, nx)).astype(np.float32)
    flat = lo.reshape(-1)
    flat[::5] = np.float32(0.0)
    flat[-1] = np.float32(np.inf)                                 # the last cell, in the last (partial) group of 8
    if flat.size > 2:
        flat[-2], flat[0] = np.float32(np.nan), np.float32(-np.inf)
    return lo


# ── icpmi_grid_score_field ───────────────────────────────────────────────────
def score_field(b, ny, nx):
    lo = _log_odds(ny, nx)
    p_lo, p_f = b.place(lo, "log_odds"), b.out((ny, nx), np.int16, "field")
    b.call = lambda short=None: b.L.icpmi_grid_score_field(p_lo, ny, nx, 11, p_f, b.stream())
    b.expected = lambda: {"field": gref.quantise(lo, 11)}


# ── icpmi_grid_bound_field ───────────────────────────────────────────────────
def bound_field(b, ny, nx, D):
    q = field_of(ny, nx)
    p_q, p_o = b.place(q, "field"), b.out((ny + D - 1, nx + D - 1), np.int16, "bound")
    b.call = lambda short=None: b.L.icpmi_grid_bound_field(p_q, ny, nx, D, p_o, b.stream())
    b.expected = lambda: {"bound": wref.bound_field(q, D)}


# ── icpmi_grid_likelihood_field ──────────────────────────────────────────────
def likelihood_field(b, ny, nx, R, want):
    q = field_of(ny, nx)
    tab = lref.table(4000, max(1.0, R / 3.0), R)                  # exactly R^2 + 1 int16, on the host
    p_q = b.place(q, "field")
    p_d2 = b.out((ny, nx), np.int16, "d2") if "d2" in want else None
    p_lf = b.out((ny, nx), np.int16, "lf") if "lf" in want else None
    if p_lf is not None:
        p_ws = b.query("workspace", "icpmi_grid_likelihood_workspace_bytes", (ny, nx, R))
    b.call = lambda short=None: b.L.icpmi_grid_likelihood_field(
        p_q, ny, nx, THRESHOLD, R, host(tab) if p_lf is not None else None, 1, p_d2, p_lf, p_ws if p_lf is not None else None,
        b.size("workspace", short) if p_lf is not None else 0, b.stream())

    def expected():
        d2, lf = lref.likelihood_field(q, THRESHOLD, R, tab, True)
        return {k: v for k, v in (("d2", d2), ("lf", lf)) if k in want}
    b.expected = expected


# ── icpmi_grid_occupancy_planes ──────────────────────────────────────────────
def _place_planes_output(b, ny, nx, name="planes"):
    """The planes buffer as an output: exactly the queried bytes; the words of the two planes are compared."""
    p = b.query(name, "icpmi_grid_occupancy_planes_bytes", (ny, nx), role=SCRATCH)
    total = b.arena.nbytes(name)
    mask = planes_bytes_of(*pgref.planes_of(np.zeros((ny, nx), np.int16), 1), total)[1]
    b.outputs[name] = mask
    return p, total


def occupancy_planes(b, ny, nx):
    q = field_of(ny, nx)
    p_q = b.place(q, "field")
    p_pl, total = _place_planes_output(b, ny, nx)
    b.call = lambda short=None: b.L.icpmi_grid_occupancy_planes(p_q, ny, nx, THRESHOLD, p_pl, b.size("planes", short), b.stream())
    b.expected = lambda: {"planes": planes_bytes_of(*pgref.planes_of(q, THRESHOLD), total)[0]}


def _map(b, q, kept):
    """The map of a cast, a check or a beam call -> (field, planes, workspace, bytes(short)) pointers: the field with a
    workspace of exactly the planes' bytes, or planes packed into the arena by the call itself and kept."""
    ny, nx = q.shape
    p_q = b.place(q, "field")
    if not kept:
        p_ws = b.query("workspace", "icpmi_grid_occupancy_planes_bytes", (ny, nx))
        return (lambda short=None: 0), p_q, None, p_ws, (lambda short: b.size("workspace", short))
    p_pl = b.query("planes", "icpmi_grid_occupancy_planes_bytes", (ny, nx), host=False)

    def pack(short=None):
        if short is not None:                                     # a refusal is being tested: nothing is launched
            return 0
        rc = b.L.icpmi_grid_occupancy_planes(p_q, ny, nx, THRESHOLD, p_pl, b.size("planes"), b.stream())
        b.sync()
        b.arena.freeze("planes")                                  # from here on the planes are an input
        return rc
    return pack, None, p_pl, None, (lambda short: 0)


# ── icpmi_grid_cast_segments, icpmi_grid_cast_rays ───────────────────────────
def cast_segments(b, ny, nx, n, kept):
    q = field_of(ny, nx)
    segs = cref.star_segments(ny, nx, 3, n=max(n, 40))[-n:]
    pack, p_q, p_pl, p_ws, ws_bytes = _map(b, q, kept)
    p_s, p_o = b.place(segs, "segs"), b.out((n, 4), np.int32, "records")

    def call(short=None):
        return pack(short) or b.L.icpmi_grid_cast_segments(p_q, p_pl, ny, nx, THRESHOLD, p_s, n, p_o, p_ws, ws_bytes(short), b.stream())
    b.call = call
    b.expected = lambda: {"records": cref.cast_segments(q, THRESHOLD, segs)}


def cast_rays(b, ny, nx, P, A, kept):
    q = field_of(ny, nx)
    xy, pcs = poses_of(P, ny, nx, seed=5)
    ang = np.linspace(-np.pi, np.pi, A, endpoint=False) + 0.01
    bcs = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    reach = 0.6 * max(ny, nx) * RES + 0.3
    pack, p_q, p_pl, p_ws, ws_bytes = _map(b, q, kept)
    p_xy, p_pcs, p_bcs = b.place(xy, "poses"), b.place(pcs, "pose_cs"), b.place(bcs, "beam_cs")
    p_o = b.out((P, A, 4), np.int32, "records")

    def call(short=None):
        return pack(short) or b.L.icpmi_grid_cast_rays(p_q, p_pl, ny, nx, THRESHOLD, MIN_X, MIN_Y, RES, p_xy, p_pcs, P, p_bcs, A, reach, p_o, p_ws,
                                                  ws_bytes(short), b.stream())
    b.call = call
    b.expected = lambda: {"records": cref.cast_rays(q, THRESHOLD, MIN_X, MIN_Y, RES, xy, pcs, bcs, reach)[0]}


# ── the pair entries: a cloud set whose last cloud is the one a single pair reads ─────────────────────────────────────
class Pairs:
    def __init__(self, b, ny, nx, rows, n_pairs, n_angles=1):
        self.clouds = clouds_of(rows, ny, nx)
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        self.pair = pair_clouds_of(n_pairs, len(rows))
        self.t, cs = poses_of(n_pairs, ny, nx)
        th = np.arctan2(cs[:, 1], cs[:, 0])[:, None] + 0.05 * np.arange(n_angles)[None, :]
        self.cs = np.stack([np.cos(th), np.sin(th)], axis=2)        # [B][A][2]
        self.n_pairs, self.n_clouds = n_pairs, len(rows)
        self.stride = int(max(rows[c] for c in self.pair))
        self.p_pts = b.place(np.concatenate(self.clouds), "pts")
        self.p_off, self.p_pair = b.place(self.off, "off_dev"), b.place(self.pair, "pair_cloud")
        self.p_t, self.p_cs = b.place(self.t, "pair_t"), b.place(self.cs if n_angles > 1 else self.cs[:, 0], "cos_sin")

    def args(self):
        """pts ... n_pairs, as the pair entries take them (cnt_dev NULL: every cloud full)."""
        return (self.p_pts, self.p_off, host(self.off), None, self.n_clouds, self.p_pair, host(self.pair), self.n_pairs)

    def rows_mask(self, ints):
        """[B][stride][ints]: the rows of each pair's cloud — what lies behind a cloud's count is not written."""
        m = np.zeros((self.n_pairs, self.stride, ints), dtype=bool)
        for k, c in enumerate(self.pair):
            m[k, :len(self.clouds[c])] = True
        return m


def match_batch(b, ny, nx, rows, n_pairs, W, A, want_scores):
    q = field_of(ny, nx)
    S = 2 * W + 1
    p_q = b.place(q, "field")
    pr = Pairs(b, ny, nx, rows, n_pairs, A)
    p_rec = b.out((n_pairs, 8), np.int32, "records")
    p_vol = b.out((n_pairs, A, S, S), np.int32, "scores") if want_scores else None
    p_ws = b.query("workspace", "icpmi_grid_match_workspace_bytes", (n_pairs, A, W))
    centre = A // 2
    b.call = lambda short=None: b.L.icpmi_grid_match_batch(p_q, ny, nx, MIN_X, MIN_Y, RES, *pr.args(), pr.p_t, pr.p_cs, A, W, centre, p_rec, p_vol,
                                                           p_ws, b.size("workspace", short), b.stream())

    def expected():
        vols = [gref.volume(q, pr.clouds[c], pr.t[k], pr.cs[k], W, MIN_X, MIN_Y, RES) for k, c in enumerate(pr.pair)]
        out = {"records": np.array([gref.record(v, r, centre, W) for v, r in vols])}
        if want_scores:
            out["scores"] = np.array([v for v, _ in vols])
        return out
    b.expected = expected


def search_batch(b, ny, nx, rows, n_pairs, W, D, A, want_bounds):
    q = field_of(ny, nx)
    M = wref.bound_field(q, D)
    NB = -(-(2 * W + 1) // D)
    p_q, p_m = b.place(q, "field"), b.place(M, "bound")
    pr = Pairs(b, ny, nx, rows, n_pairs, A)
    p_rec = b.out((n_pairs, 12), np.int32, "records")
    p_u = b.out((n_pairs, A, NB, NB), np.int32, "bounds") if want_bounds else None
    p_ws = b.query("workspace", "icpmi_grid_search_workspace_bytes", (n_pairs, A, W, D))
    centre = A - 1
    b.call = lambda short=None: b.L.icpmi_grid_search_batch(p_q, p_m, ny, nx, MIN_X, MIN_Y, RES, *pr.args(), pr.p_t, pr.p_cs, A, W, D, centre, p_rec,
                                                            p_u, p_ws, b.size("workspace", short), b.stream())

    def expected():
        got = [wref.search(q, D, pr.clouds[c], pr.t[k], pr.cs[k], W, centre, MIN_X, MIN_Y, RES, M=M) for k, c in enumerate(pr.pair)]
        out = {"records": np.array([r for r, _ in got])}
        if want_bounds:
            out["bounds"] = np.array([u for _, u in got])
        return out
    b.expected = expected


def match_moments(b, n_pairs, A, W):
    S = 2 * W + 1
    rng = np.random.default_rng(A * 100 + W)
    vol = rng.integers(-3000, 3000, size=(n_pairs, A, S, S)).astype(np.int32)
    rec = np.array([gref.record(v, np.full(A, 40 + k), -1, W) for k, v in enumerate(vol)], dtype=np.int32)
    if n_pairs > 1:
        rec[1, 0] = mref.ST_CAPACITY                               # twelve zeros
    p_v, p_r = b.place(vol, "volume"), b.place(rec, "records")
    p_m = b.out((n_pairs, 12), np.int64, "moments")
    b.call = lambda short=None: b.L.icpmi_grid_match_moments(p_v, p_r, n_pairs, A, W, 7, p_m, b.stream())
    b.expected = lambda: {"moments": np.array([mref.moments(v, r, 7) for v, r in zip(vol, rec)])}


def check_batch(b, ny, nx, rows, n_pairs, tolerance, want_rows, kept):
    q = field_of(ny, nx)
    pack, p_q, p_pl, p_ws, ws_bytes = _map(b, q, kept)
    pr = Pairs(b, ny, nx, rows, n_pairs)
    p_rec = b.out((n_pairs, 8), np.int32, "records")
    p_rows = None
    if want_rows:
        m = pr.rows_mask(4)
        p_rows = b.out((n_pairs, pr.stride, 4), np.int32, "rows", mask=m, untouched=~m)

    def call(short=None):
        return pack(short) or b.L.icpmi_grid_check_batch(p_q, p_pl, ny, nx, THRESHOLD, MIN_X, MIN_Y, RES, *pr.args(), pr.p_t, pr.p_cs, tolerance, p_rec,
                                                    p_rows, pr.stride, p_ws, ws_bytes(short), b.stream())
    b.call = call

    def expected():
        got = [kref.check_pair(q, THRESHOLD, MIN_X, MIN_Y, RES, pr.clouds[c], pr.t[k], pr.cs[k, 0], tolerance) for k, c in enumerate(pr.pair)]
        out = {"records": np.array([r for r, _ in got])}
        if want_rows:
            out["rows"] = np.zeros((n_pairs, pr.stride, 4), dtype=np.int32)
            for k, (_, r) in enumerate(got):
                out["rows"][k, :len(r)] = r
        return out
    b.expected = expected


def beam_batch(b, ny, nx, rows, n_pairs, H, want_hist, want_rows, kept):
    q = field_of(ny, nx)
    table = bref.table_of(H)                                       # exactly 2 H + 3 int32
    beyond = 0.6
    pack, p_q, p_pl, p_ws, ws_bytes = _map(b, q, kept)
    pr = Pairs(b, ny, nx, rows, n_pairs)
    p_tab = b.place(table, "table")
    p_rec = b.out((n_pairs, 8), np.int32, "records")
    p_hist = b.out((n_pairs, 2 * H + 3), np.int32, "hist") if want_hist else None
    p_rows = None
    if want_rows:
        m = pr.rows_mask(4)
        p_rows = b.out((n_pairs, pr.stride, 4), np.int32, "rows", mask=m, untouched=~m)

    def call(short=None):
        return pack(short) or b.L.icpmi_grid_beam_batch(p_q, p_pl, ny, nx, THRESHOLD, MIN_X, MIN_Y, RES, *pr.args(), pr.p_t, pr.p_cs, beyond, H, p_tab,
                                                   p_rec, p_hist, p_rows, pr.stride, p_ws, ws_bytes(short), b.stream())
    b.call = call

    def expected():
        got = [bref.beam_pair(q, THRESHOLD, MIN_X, MIN_Y, RES, pr.clouds[c], pr.t[k], pr.cs[k, 0], table, H, beyond) for k, c in enumerate(pr.pair)]
        out = {"records": np.array([g[0] for g in got])}
        if want_hist:
            out["hist"] = np.array([g[1] for g in got])
        if want_rows:
            out["rows"] = np.zeros((n_pairs, pr.stride, 4), dtype=np.int32)
            for k, g in enumerate(got):
                out["rows"][k, :len(g[2])] = g[2]
        return out
    b.expected = expected


# ── icpmi_grid_update_scans ──────────────────────────────────────────────────
def update_scans(b, ny, nx, n_scans, n_hits, behind="zeros"):
    """``behind``: what the bounding-box slots and the scan boxes behind the four counter grids hold when the call starts —
    "zeros", as the caller's first call finds them; "pattern", the byte pattern of the run; "left over", what an earlier call
    of the same entry left (the case calls twice, and the reference replays the scans twice)."""
    import oracle
    rng = np.random.default_rng(ny + n_scans * 7 + n_hits)
    res, min_x, min_y = 0.1, -1.0, -0.5
    lo0 = rng.uniform(-2.0, 2.0, (ny, nx)).astype(np.float32)
    origins = np.stack([min_x + rng.uniform(0.2, 0.8, n_scans) * nx * res, min_y + rng.uniform(0.2, 0.8, n_scans) * ny * res], axis=1)
    hits = np.stack([min_x + rng.uniform(-0.1, 1.1, n_scans * n_hits) * nx * res, min_y + rng.uniform(-0.1, 1.1, n_scans * n_hits) * ny * res], axis=1)
    hits[-1] = [min_x + nx * res - 1e-9, min_y + ny * res - 1e-9]  # the grid's last cell
    hit_off = (np.arange(n_scans + 1) * n_hits).astype(np.int32)
    l_hit, l_miss, lo, hi = 0.85, -0.4, -4.0, 4.0
    calls = 2 if behind == "left over" else 1
    p_lo = b.place(lo0, "log_odds", STATE)
    b.outputs["log_odds"] = None
    p_cnt = b.query("counts", "icpmi_grid_workspace_bytes", (ny, nx), refusal=0, zeros=True)     # (the entry takes no byte count)
    grids = 4 * 4 * ny * nx                                        # four grids of uint32 counters; the slots and boxes follow
    p_or, p_hits = b.place(origins, "origins"), b.place(hits, "hits")

    def call(short=None):
        if behind == "pattern":
            b.arena.view("counts")[grids:].fill_(b.arena.pattern)
            b.sync()
        rc = 0
        for _ in range(calls):
            rc = rc or b.L.icpmi_grid_update_scans(p_lo, p_cnt, ny, nx, min_x, min_y, res, p_or, p_hits, host(hit_off), n_scans, l_hit, l_miss, lo,
                                                   hi, 0, 0, b.stream())
        return rc
    b.call = call

    def after(pattern):
        raw = b.arena.read("counts")
        left = np.flatnonzero(raw[:grids])
        assert not len(left), f"the call must leave its counter grids all zero again: bytes {left[:4].tolist()} are not"
    b.after = after

    def expected():
        ref = lo0.copy()
        for _ in range(calls):
            for s in range(n_scans):
                oracle.grid_update_scan(ref, min_x, min_y, res, origins[s], hits[hit_off[s]:hit_off[s + 1]], l_hit, l_miss, lo, hi)
        return {"log_odds": ref}
    b.expected = expected


# ── the table of cases ───────────────────────────────────────────────────────
def _add(fn, id, **kw):
    CASES.append(Case(f"{fn.__name__}[{id}]", lambda b: fn(b, **kw)))


# Beside the shapes whose buffers end inside a vector group, one where a whole layout ends exactly on a 256-byte granule —
# no padding behind the last array, so a size query that is a few bytes short shows: 64 plane words (256 bytes a plane), and
# 64 (pair, angle) words with 64 shifts (256 bytes each in the matcher's workspace).
GRANULE_GRID = (64, 32)
for _ny, _nx in GRIDS + (GRANULE_GRID,):
    _add(score_field, f"{_ny}x{_nx}", ny=_ny, nx=_nx)
    _add(occupancy_planes, f"{_ny}x{_nx}", ny=_ny, nx=_nx)
for _i, _D in enumerate(wref.BLOCKS):
    for _ny, _nx in GRIDS:
        _add(bound_field, f"{_ny}x{_nx}-D{_D}", ny=_ny, nx=_nx, D=_D)
for _R in (0, 1, 64):
    for _ny, _nx in ((1, 1), (5, 33), (37, 53), (65, 129)):
        for _want in (("d2",), ("lf",), ("d2", "lf")):
            _add(likelihood_field, f"{_ny}x{_nx}-R{_R}-{'+'.join(_want)}", ny=_ny, nx=_nx, R=_R, want=_want)
for _n, (_ny, _nx) in zip((1, 63, 65), ((1, 7), (5, 33), (37, 53))):
    for _kept in (False, True):
        _add(cast_segments, f"{_ny}x{_nx}-n{_n}-{'planes' if _kept else 'field'}", ny=_ny, nx=_nx, n=_n, kept=_kept)
for (_P, _A), (_ny, _nx) in zip(((1, 1), (3, 65)), ((2, 65), (37, 53))):
    for _kept in (False, True):
        _add(cast_rays, f"{_ny}x{_nx}-{_P}x{_A}-{'planes' if _kept else 'field'}", ny=_ny, nx=_nx, P=_P, A=_A, kept=_kept)
for (_W, _A), _rows, _B, (_ny, _nx) in zip(((0, 1), (3, 3), (8, 2), (0, 64)), ROW_SETS + ROW_SETS[:1], (1, 3, 1, 1),
                                           ((5, 33), (37, 53), (65, 129), (4, 32))):
    for _vol in (True, False):
        _add(match_batch, f"W{_W}-A{_A}-rows{_rows[-1]}-B{_B}-{'scores' if _vol else 'workspace'}", ny=_ny, nx=_nx, rows=_rows, n_pairs=_B, W=_W, A=_A,
             want_scores=_vol)
for _W, _D, _rows, _B, (_ny, _nx) in zip((5, 33, 5), (4, 8, 16), ROW_SETS, (1, 3, 1), ((5, 33), (37, 53), (65, 129))):
    for _u in (True, False):
        _add(search_batch, f"W{_W}-D{_D}-rows{_rows[-1]}-B{_B}-{'bounds' if _u else 'plain'}", ny=_ny, nx=_nx, rows=_rows, n_pairs=_B, W=_W, D=_D, A=2,
             want_bounds=_u)
for (_A, _W), _B in zip(((1, 0), (3, 6), (65, 1)), (1, 3, 3)):
    _add(match_moments, f"A{_A}-W{_W}-B{_B}", n_pairs=_B, A=_A, W=_W)
for _H, _rows, _B, (_ny, _nx) in zip((0, 3, 3), ROW_SETS, (1, 3, 1), ((5, 33), (37, 53), (65, 129))):
    for _want_rows in (False, True):
        for _kept in (False, True):
            _add(check_batch, f"tol{_H}-rows{_rows[-1]}-B{_B}-{'rows' if _want_rows else 'norows'}-{'planes' if _kept else 'field'}", ny=_ny, nx=_nx,
                 rows=_rows, n_pairs=_B, tolerance=_H, want_rows=_want_rows, kept=_kept)
        for _want_hist in (False, True):
            _add(beam_batch, f"H{_H}-rows{_rows[-1]}-B{_B}-{'hist' if _want_hist else 'nohist'}-{'rows' if _want_rows else 'norows'}", ny=_ny, nx=_nx,
                 rows=_rows, n_pairs=_B, H=_H, want_hist=_want_hist, want_rows=_want_rows, kept=_want_hist != _want_rows)
# one-pair cases read the last cloud only (1, 15 rows); with three pairs both clouds of a set are read, the 2 049 rows too
_add(match_batch, "W0-A1-rows2049+15-B3-scores", ny=65, nx=129, rows=ROW_SETS[2], n_pairs=3, W=0, A=1, want_scores=True)
_add(check_batch, "tol3-rows2049+15-B3-rows-field", ny=65, nx=129, rows=ROW_SETS[2], n_pairs=3, tolerance=3, want_rows=True, kept=False)
_add(beam_batch, "H3-rows2049+15-B3-hist-rows", ny=65, nx=129, rows=ROW_SETS[2], n_pairs=3, H=3, want_hist=True, want_rows=True, kept=False)
for _ny, _nx in ((37, 53), (65, 129)):
    for _S, _h in ((1, 1), (1, 65), (3, 1), (3, 65)):
        _add(update_scans, f"{_ny}x{_nx}-{_S}scans-{_h}hits", ny=_ny, nx=_nx, n_scans=_S, n_hits=_h)
    # what include/icpmi.h says of the bytes behind the counter grids: no call depends on them
    for _S, _behind in ((1, "pattern"), (3, "pattern"), (1, "left over"), (3, "left over")):
        _add(update_scans, f"{_ny}x{_nx}-{_S}scans-65hits-{_behind.replace(' ', '-')}-behind", ny=_ny, nx=_nx, n_scans=_S, n_hits=65, behind=_behind)
