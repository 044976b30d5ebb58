"""The single-pair rotation search and its translation refinement (csrc/rotsearch.hip: icpmi_rotation_search,
icpmi_rotation_refine) at their edges: a NumPy restatement of the refinement, the workspace head the refinement reads, and
the cases of tests/test_rotation_single_cpu.py (which proves that every case has the property it is named for) and
tests/test_rotation_single_gpu.py (which compares the device with the restatement).  Importable without a GPU.

Refinement cases (``refine_cases``).  The head is written by hand, so no voxel filter stands between a case and the
kernels: the row counts are the designed ones.
* lerp_n5 .. lerp_n11    — (n - 1) * 0.8 has the fractions .2, 0, .8, .6, .4, .2, 0: the exact order statistic and both
                           branches of NumPy's _lerp.  Without ties four rows pass at n = 5 (the prediction returns) and
                           exactly five at n = 6.
* match_n255 .. n257     — the match kernel's workgroups of 256 source rows.
* finish_n1023 .. n1025  — the finishing workgroup's stride of 1 024.
* cap_n2047, cap_n2048   — ICPMI_RSR_MAX_ROWS.
* tile_m5 .. tile_m2049  — 300 source rows; 43 of them are nearest to the LAST target row (alone in the second tile of
                           2 048 at m = 2 049); ``_twin``: row 0 holds the same coordinates, so the lowest index wins the tie.
* few_n4, few_m4         — fewer than five rows on either side: (prediction, 0, NaN).
* zero, tie_n5, two_*, run_*  — exact ties among the squared distances: offsets q / 4096 along x from targets at even
                           integer coordinates under the identity rotation, so every d2 is (q / 4096)^2 exactly.
* gap_tight, gap_nan, gap_decoy — 180 valid source rows of 300 raw and 120 valid target rows of 200 raw; the rows behind
                           the counts hold NaN, or decoys nearer to every source row than any valid target.
* rec_fine, rec_nofine   — a record that names fine entry [2][1]; NF = 0 beside a fine table whose [K][0] is another angle.
Fewer than five inliers at n >= 6 cannot happen: lo = floor((n - 1) * 0.8) >= 4 and the threshold is at least the lo-th
order statistic, so lo + 1 >= 5 rows are at or below it (asserted on the restatement in the CPU file).

Search cases (``search_cases``).  Clouds are jittered lattices of spacing 0.5 (two rows are at least 0.46 apart, more
than the diagonal of a 0.3 voxel: the filter keeps every row in any frame); the angle tables are plain arrays, so a
repeated angle has bit-equal cos / sin and a bit-equal score, and a NaN angle a NaN score.  Out of reach: a score vector
that is +inf throughout (it needs coordinates whose squares overflow, and the voxel filter refuses such clouds first).
"""
import functools
import types

import numpy as np

import oracle
from icpmi import _lib

WS_COUNTS, WS_CLOUDS, MAX_ROWS = _lib.RS_WS_COUNTS, _lib.RS_WS_CLOUDS, _lib.RSR_MAX_ROWS
TILE = 2048                       # RS_TILE_POINTS: target rows per LDS tile of the nearest-target walk
THETA = 0.3                       # the rotation that aligns every generic pair
PRED = (1.5, -0.7)                # the predicted position / the caller's shift
VOXEL = 0.3


def rot(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s], [s, c]])


def cos_sin_table(angles):
    """cos / sin of an angle array as icpmi.prealign.device_angle_tables forms them ([..., 2])."""
    a = np.asarray(angles, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=a.ndim))


# ── the refinement, slam.py:161-181, in oracle.submap_rotation_search's steps ─────────────────────────────────────
def nearest(placed, tgt):
    """Brute force in float64: d2 = dx * dx + dy * dy of direct differences, the lowest row on ties -> (d2 [n, m], idx [n])."""
    dx = placed[:, None, 0] - tgt[None, :, 0]
    dy = placed[:, None, 1] - tgt[None, :, 1]
    d2 = dx * dx + dy * dy
    return d2, np.argmin(d2, axis=1)


def refine_parts(src, tgt, cos_sin, pred_t):
    """Every intermediate of ``refine`` (None below five rows)."""
    src, tgt = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
    pred_t = np.asarray(pred_t, dtype=np.float64)
    if len(src) < 5 or len(tgt) < 5:                                   # slam.py:128-129
        return None
    c, s = cos_sin
    R = np.array([[c, -s], [s, c]])
    rotated = src @ R.T                                                # slam.py:168
    all_d2, idx = nearest(rotated + pred_t, tgt)                       # slam.py:169-170
    d = np.sqrt(all_d2[np.arange(len(src)), idx])                      # what KDTree.query returns
    d2 = d * d                                                         # slam.py:171
    thresh = np.percentile(d2, 80)
    keep = d2 <= thresh
    k = int(keep.sum())
    t = np.mean(tgt[idx][keep] - rotated[keep], axis=0) if k >= 5 else pred_t.copy()
    return types.SimpleNamespace(rotated=rotated, all_d2=all_d2, idx=idx, d2=d2, thresh=thresh, keep=keep, k=k, t=t)


def refine(src, tgt, cos_sin, pred_t):
    """-> (t, inliers, thresh); (pred_t, 0, NaN) when either cloud has fewer than five rows."""
    p = refine_parts(src, tgt, cos_sin, pred_t)
    if p is None:
        return np.array(pred_t, dtype=np.float64), 0, np.nan
    return p.t, p.k, p.thresh


def lerp_position(n):
    """(lo, hi, t) of np.percentile(., 80) over n values: the virtual index (n - 1) * 0.8 split as NumPy splits it."""
    vi = (n - 1) * 0.8
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1), vi - lo


def lerp_forms(d2):
    """The two forms of NumPy's _lerp between the order statistics lo and hi of d2: A + (B - A) t, used below t = 0.5, and
    B - (B - A) (1 - t), used from there on."""
    s = np.sort(d2)
    lo, hi, t = lerp_position(len(s))
    A, B = s[lo], s[hi]
    return A + (B - A) * t, B - (B - A) * (1.0 - t)


# ── the workspace head icpmi_rotation_refine reads ──────────────────────────────────────────────────
def _gap_rows(gap_fill, count):
    g = np.asarray(gap_fill, dtype=np.float64)
    if g.ndim == 0:
        return np.full((count, 2), float(g))
    return np.resize(g.reshape(-1, 2), (count, 2)) if count else np.empty((0, 2))      # the rows, cycled


def head(src, tgt, n_src_raw, n_tgt_raw, gap_fill=np.nan):
    """The head of a search workspace as bytes: int32 offsets (0, n_src_raw, n_src_raw + n_tgt_raw) at byte 0, the counts
    (len(src), len(tgt)) at RS_WS_COUNTS, the rows at RS_WS_CLOUDS with the target n_src_raw rows in.  The rows behind
    each count hold ``gap_fill`` (a value, or rows that are repeated in turn); the head's other bytes hold 0xA5."""
    src, tgt = np.asarray(src, dtype=np.float64).reshape(-1, 2), np.asarray(tgt, dtype=np.float64).reshape(-1, 2)
    assert len(src) <= n_src_raw and len(tgt) <= n_tgt_raw
    buf = np.full(WS_CLOUDS + (n_src_raw + n_tgt_raw) * 16, 0xA5, dtype=np.uint8)
    buf[:12].view(np.int32)[:] = (0, n_src_raw, n_src_raw + n_tgt_raw)
    buf[WS_COUNTS:WS_COUNTS + 8].view(np.int32)[:] = (len(src), len(tgt))
    rows = buf[WS_CLOUDS:].view(np.float64).reshape(-1, 2)
    rows[:len(src)] = src
    rows[len(src):n_src_raw] = _gap_rows(gap_fill, n_src_raw - len(src))
    rows[n_src_raw:n_src_raw + len(tgt)] = tgt
    rows[n_src_raw + len(tgt):] = _gap_rows(gap_fill, n_tgt_raw - len(tgt))
    return buf


def read_head(buf):
    """-> (offsets, counts, valid source rows, valid target rows, source gap, target gap) by the documented offsets."""
    off = buf[:12].view(np.int32).copy()
    cnt = buf[WS_COUNTS:WS_COUNTS + 8].view(np.int32).copy()
    rows = buf[WS_CLOUDS:].view(np.float64).reshape(-1, 2)
    return (off, cnt, rows[:cnt[0]].copy(), rows[off[1]:off[1] + cnt[1]].copy(), rows[cnt[0]:off[1]].copy(),
            rows[off[1] + cnt[1]:off[2]].copy())


# ── refinement cases ──────────────────────────────────────────────────────────────
def lattice(n, seed, spacing=0.5, jitter=0.04):
    """n points of a square lattice, each moved by at most jitter x spacing along either axis."""
    w = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    return (np.stack([i % w, i // w], axis=1) + np.random.default_rng(seed).uniform(-jitter, jitter, (n, 2))) * spacing


class RefineCase:
    """Valid rows ``src`` / ``tgt``; the tables and the record slots (K, NF, J) that choose the angle; raw counts and gap."""

    def __init__(self, name, src, tgt, pred=PRED, coarse=None, fine=None, rec=(1, 0, 0), raw=None, gap=np.nan, **props):
        self.name = name
        self.src, self.tgt = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
        self.pred = np.array(pred, dtype=np.float64)
        self.coarse = np.array([THETA + 0.4, THETA, THETA - 0.7] if coarse is None else coarse, dtype=np.float64)
        self.fine = None if fine is None else np.ascontiguousarray(fine, dtype=np.float64)
        self.rec = rec
        self.raw = (len(self.src), len(self.tgt)) if raw is None else raw
        self.gap = gap
        self.props = types.SimpleNamespace(**props)

    n = property(lambda self: len(self.src))
    m = property(lambda self: len(self.tgt))
    max_fine = property(lambda self: 0 if self.fine is None else int(self.fine.shape[1]))
    coarse_cs = property(lambda self: cos_sin_table(self.coarse))
    fine_cs = property(lambda self: None if self.fine is None else cos_sin_table(self.fine))

    @property
    def cos_sin(self):
        """cos / sin of the angle the record names: the fine entry [K][J] if NF > 0, else coarse entry K (slam.py:157-159)."""
        k, nf, j = self.rec
        return tuple(self.fine_cs[k, j]) if nf > 0 else tuple(self.coarse_cs[k])

    @functools.cached_property
    def head(self):
        return head(self.src, self.tgt, self.raw[0], self.raw[1], self.gap)

    @functools.cached_property
    def parts(self):
        return refine_parts(self.src, self.tgt, self.cos_sin, self.pred)

    @functools.cached_property
    def expected(self):
        """[t_x, t_y, inliers, thresh] as the device writes them."""
        t, k, thresh = refine(self.src, self.tgt, self.cos_sin, self.pred)
        return np.array([t[0], t[1], float(k), thresh])


def _generic(name, n, m, seed, which=None, tgt=None, jitter=0.05, **kw):
    """Source row i a jittered copy of target row which[i] (i mod m unless given), taken back through the pose
    (THETA, PRED): rotated and placed it lies within ``jitter`` of its row along either axis, other rows 0.46 and more away."""
    rng = np.random.default_rng(seed)
    tgt = lattice(m, seed + 1) if tgt is None else tgt
    which = np.arange(n) % m if which is None else np.asarray(which)
    placed = tgt[which] + rng.uniform(-jitter, jitter, (n, 2))
    return RefineCase(name, (placed - np.array(PRED)) @ rot(THETA), tgt, which=which, **kw)


def _tile(m, twin, seed):
    """300 source rows about the last min(m - 1, 7) target rows; ``twin``: row 0 repeats the last row's coordinates."""
    tgt = lattice(m, seed + 1)
    if twin:
        tgt[0] = tgt[m - 1]
    which = m - 1 - np.arange(300) % min(m - 1, 7)
    return _generic(f"tile_m{m}" + ("_twin" if twin else ""), 300, m, seed, which=which, tgt=tgt, twin=twin)


def _exact(name, q, seed, **props):
    """Identity rotation, integer prediction, targets at even integers, source row i placed q[i] / 4096 to the right of target
    row i mod 64 (q < 2048: below half a unit, the next target two units off): d2[i] = (q[i] / 4096)^2 with no rounding."""
    q = np.random.default_rng(seed).permutation(np.asarray(q, dtype=np.int64))
    assert q.min() >= 0 and q.max() < 2048
    i = np.arange(64)
    tgt = 2.0 * np.stack([i % 8, i // 8], axis=1)
    pred = np.array([3.0, -2.0])
    src = tgt[np.arange(len(q)) % 64] + np.stack([q / 4096.0, np.zeros(len(q))], axis=1) - pred
    return RefineCase(name, src, tgt, pred=pred, coarse=[0.4, 0.0, -0.7], q=q, **props)


def _tie_cases():
    out = [_exact("zero", np.zeros(9), 70, run=(0, 8)),
           _exact("tie_n5", [10, 20, 30, 40, 40], 71, run=(3, 4))]
    for n, seed in ((7, 72), (1025, 73)):
        lo, hi, _ = lerp_position(n)
        # two distinct distances, `low` rows of the smaller: the border between the two runs lies between lo and hi (the lower
        # run covers lo only, the upper hi only), below lo (both in the upper run), above hi (both in the lower run)
        for tag, low in (("split", lo + 1), ("upper", lo - 2), ("lower", hi + 2 if hi + 2 < n else n - 1)):
            out.append(_exact(f"two_{tag}_n{n}", [100] * low + [900] * (n - low), seed, run=None, low=low))
        # distinct distances but for one run of equal ones, which covers lo and not hi, hi and not lo, both
        w = 2 if n == 7 else 10
        for tag, first, last in (("lo", lo - w, lo), ("hi", hi, min(hi + w, n - 1)), ("both", lo - w // 2, hi + w // 2)):
            q = np.arange(1, n + 1)
            q[first:last + 1] = q[first]
            out.append(_exact(f"run_{tag}_n{n}", q, seed + 10, run=(first, last)))
    return out


def _gap_cases():
    """180 source rows in 60 clusters of three, each cluster (0.1 .. 0.12, 0.1 .. 0.12) off its target row: at least 0.14 from
    it and at most 0.015 from the cluster's decoy at (0.11, 0.11)."""
    rng = np.random.default_rng(80)
    tgt = lattice(120, 81)
    which = 2 * (np.arange(180) % 60)
    placed = tgt[which] + 0.1 + rng.uniform(0.0, 0.02, (180, 2))
    src = (placed - np.array(PRED)) @ rot(THETA)
    decoys = tgt[2 * np.arange(60)] + 0.11
    kw = dict(which=which, decoys=decoys)
    return [RefineCase("gap_tight", src, tgt, **kw),
            RefineCase("gap_nan", src, tgt, raw=(300, 200), gap=np.nan, **kw),
            RefineCase("gap_decoy", src, tgt, raw=(300, 200), gap=decoys, **kw)]


def _record_cases():
    base = _generic("", 40, 64, 90)
    coarse = [THETA + 0.4, THETA - 0.7, THETA + 0.9]
    fine = np.array([[THETA + 0.01 * (4 * k + j + 1) for j in range(4)] for k in range(3)])
    fine[2, 1] = THETA
    nofine = fine.copy()
    nofine[1, 0] = THETA + 0.3
    return [RefineCase("rec_fine", base.src, base.tgt, coarse=coarse, fine=fine, rec=(2, 3, 1)),
            RefineCase("rec_nofine", base.src, base.tgt, coarse=[THETA + 0.4, THETA, THETA - 0.7], fine=nofine, rec=(1, 0, 0))]


@functools.lru_cache(maxsize=None)
def refine_cases():
    """name -> RefineCase, in a fixed order."""
    cases = []
    for n in range(5, 12):
        # drawn again until the two forms of _lerp give different bits where the second applies (t >= 0.5: n = 7, 8)
        for seed in range(10 + n, 1000, 20):
            case = _generic(f"lerp_n{n}", n, 40, seed, which=np.random.default_rng(seed + 7).permutation(40)[:n])
            low_form, high_form = lerp_forms(case.parts.d2)
            if lerp_position(n)[2] < 0.5 or low_form != high_form:
                break
        cases.append(case)
    for fam, sizes in (("match", (255, 256, 257)), ("finish", (1023, 1024, 1025)), ("cap", (2047, 2048))):
        for n in sizes:
            cases.append(_generic(f"{fam}_n{n}", n, 64, 1000 + n))
    for m in (5, TILE - 1, TILE, TILE + 1):
        cases += [_tile(m, False, 40 + m), _tile(m, True, 50 + m)]
    cases += [_generic("few_n4", 4, 40, 60), _generic("few_m4", 40, 4, 61)]
    cases += _tie_cases() + _gap_cases() + _record_cases()
    return {c.name: c for c in cases}


LERP = tuple(f"lerp_n{n}" for n in range(5, 12))
TILES = tuple(f"tile_m{m}{t}" for m in (5, TILE - 1, TILE, TILE + 1) for t in ("", "_twin"))


# ── search cases ────────────────────────────────────────────────────────────────
class SearchCase:
    """Raw clouds, angle tables (``fine`` [K, L] with lengths ``fine_n``, or None: max_fine = 0, null tables), the mode,
    and the record slots the tables were built to give."""

    def __init__(self, name, src, tgt, coarse, fine, fine_n, centred, K, NF, J, tied=False):
        self.name, self.src, self.tgt = name, np.ascontiguousarray(src), np.ascontiguousarray(tgt)
        self.coarse = np.ascontiguousarray(coarse, dtype=np.float64)
        self.fine = np.zeros((len(self.coarse), 0)) if fine is None else np.ascontiguousarray(fine, dtype=np.float64)
        self.fine_n = np.zeros(len(self.coarse), dtype=np.int64) if fine_n is None else np.asarray(fine_n, dtype=np.int64)
        self.centred, self.shift = bool(centred), PRED
        self.K, self.NF, self.J, self.tied = K, NF, J, tied

    max_fine = property(lambda self: int(self.fine.shape[1]))

    @functools.cached_property
    def filtered(self):
        """The clouds the pinned voxel filter leaves (the designed rows, in the filter's order)."""
        fs, ft = oracle.voxel_downsample(self.src, VOXEL), oracle.voxel_downsample(self.tgt, VOXEL)
        assert (len(fs), len(ft)) == (len(self.src), len(self.tgt)), (self.name, len(fs), len(ft))
        return fs, ft

    def frame(self, fs, ft):
        """(centred source rows, shift) of the scoring loop: features.py:205-216 or slam.py:138-143."""
        if self.centred:
            return fs - np.mean(fs, axis=0), np.mean(ft, axis=0)
        return fs, np.array(self.shift)

    def oracle_scores(self, angles):
        """oracle.rotation_scores on the filtered clouds; NaN for a NaN angle (the oracle's tree is not asked)."""
        a = np.asarray(angles, dtype=np.float64)
        out = np.full(len(a), np.nan)
        ok = ~np.isnan(a)
        rows, shift = self.frame(*self.filtered)
        out[ok] = oracle.rotation_scores(rows, self.filtered[1], a[ok], shift)
        return out


def score_bound(ref):
    """The project's bound between a device score and the oracle's (tests/test_gpu_parity.py,
    test_rotation_scores_against_oracle): 1e-13 x max(1, the largest reference score)."""
    return 1e-13 * max(1.0, float(np.nanmax(ref)))


def _pair(n_src, n_tgt, seed, centred):
    """The target a lattice (jitter 0.02), the source n_src of its rows moved by up to 0.01 and taken back through the
    pose (THETA, PRED): at THETA a row lies within 0.015 of its own, and at 2 degrees and more off a row a metre from the pivot
    is 0.035 and more away.  Centred, the pivot is the source's mean, carried to the target's: n_src == n_tgt keeps them together."""
    rng = np.random.default_rng(seed)
    tgt = lattice(n_tgt, seed + 1, jitter=0.04)
    part = tgt[rng.permutation(n_tgt)[:n_src]] + rng.uniform(-0.01, 0.01, (n_src, 2))
    assert not centred or n_src == n_tgt
    return (part - np.array(PRED)) @ rot(THETA), tgt


def _others(n_coarse):
    """n_coarse distinct angles 2 to 358 degrees off THETA."""
    return THETA + np.deg2rad(2.0 + 356.0 * np.arange(n_coarse) / n_coarse)


def _fine_rows(base, fine_n, winner):
    """Row k: base[k] + step x (1 + a) + k x 1e-3 (no two rows alike), step 0.5 degrees or what keeps the longest row within
    350 degrees (a full turn further on an angle scores as its twin, to rounding); ``winner``'s row with THETA in the middle
    of its length."""
    L = int(fine_n.max())
    step = np.deg2rad(min(0.5, 350.0 / L))
    fine = base[:, None] + step * (1 + np.arange(L))[None, :] + 1e-3 * np.arange(len(base))[:, None]
    j = (int(fine_n[winner]) - 1) // 2
    fine[winner, j] = THETA
    return fine, j


def _table_case(name, n_coarse, winners, nans=()):
    """THETA at the coarse indices ``winners``, NaN at ``nans``; row k's fine grid has n_coarse - k entries (all lengths
    distinct: NF names the row that was scored).  The record names the first NaN, else the first winner."""
    src, tgt = _pair(300, 300, 200 + n_coarse + sum(winners), False)
    base = _others(n_coarse)
    coarse = base.copy()
    coarse[list(winners)] = THETA
    coarse[list(nans)] = np.nan
    fine_n = n_coarse - np.arange(n_coarse)
    K = min(nans) if nans else min(winners)
    fine, J = _fine_rows(base, fine_n, K)
    return SearchCase(name, src, tgt, coarse, fine, fine_n, False, K, int(fine_n[K]), J, tied=len(winners) > 1)


def _ragged_case(name, cnt, max_fine=6):
    """Twelve coarse angles, THETA at index 7; its fine row holds THETA + (cnt - a) degrees for a < cnt (the last is the
    nearest) and THETA itself, the decoy, behind the count."""
    src, tgt = _pair(300, 300, 300 + cnt, False)
    coarse = _others(12)
    coarse[7] = THETA
    if max_fine == 0:
        return SearchCase(name, src, tgt, coarse, None, None, False, 7, 0, 0)
    fine_n = np.full(12, max_fine)
    fine_n[7] = cnt
    fine, _ = _fine_rows(coarse, fine_n, 0)
    fine[7] = THETA
    fine[7, :cnt] = THETA + np.deg2rad(cnt - np.arange(cnt))
    return SearchCase(name, src, tgt, coarse, fine, fine_n, False, 7, cnt, max(cnt - 1, 0))


def _means_case(n, centred):
    src, tgt = _pair(n, n, 400 + n, centred)
    coarse = THETA + np.deg2rad([40.0, -25.0, 0.0, 3.0, 170.0])
    fine_n = np.full(5, 3)
    fine = coarse[:, None] + np.deg2rad([-1.5, 1.0, 0.0])[None, :]
    return SearchCase(f"means_n{n}_{'centred' if centred else 'shifted'}", src, tgt, coarse, fine, fine_n, centred, 2, 3, 2)


MEANS_ROWS = (5, 7, 8, 9, 255, 256, 257, 263, 520)


@functools.lru_cache(maxsize=None)
def search_cases():
    """name -> SearchCase, in a fixed order."""
    cases = [_table_case("tie_3_259", 300, (3, 259)), _table_case("tie_70_130", 300, (70, 130)),
             _table_case("tie_0_299", 300, (0, 299)), _table_case("tie_0_1024", 1025, (0, 1024)),
             _table_case("single_angle", 1, (0,)),
             _table_case("nan_after", 300, (150,), nans=(200,)), _table_case("nan_before", 300, (150,), nans=(100,)),
             _table_case("nan_twice", 300, (150,), nans=(120, 220)),
             _ragged_case("ragged_1", 1), _ragged_case("ragged_3", 3), _ragged_case("ragged_full", 6),
             _ragged_case("ragged_0", 0), _ragged_case("no_fine_tables", 0, max_fine=0)]
    cases += [_means_case(n, centred) for n in MEANS_ROWS for centred in (True, False)]
    return {c.name: c for c in cases}
