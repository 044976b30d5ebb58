"""That the cases of tests/rotsingle_cases.py have the properties they are named for, that the restatement of the
refinement is np.percentile's rule to within rounding of exact arithmetic, and the refusals icpmi_rotation_refine decides
on the host.  No GPU: a case that loses its property fails here, not silently on the device."""
from fractions import Fraction

import numpy as np
import pytest

import rotsingle_cases as rc

REFINE = rc.refine_cases()
SEARCH = rc.search_cases()


def _sorted_d2(case):
    return np.sort(case.parts.d2)


# ── the refinement cases ──────────────────────────────────────────────────────────
def test_the_families_have_the_row_counts_where_the_loops_change():
    assert [REFINE[name].n for name in rc.LERP] == [5, 6, 7, 8, 9, 10, 11] and all(REFINE[name].m == 40 for name in rc.LERP)
    for fam, sizes in (("match", (255, 256, 257)), ("finish", (1023, 1024, 1025)), ("cap", (2047, 2048))):
        assert [(REFINE[f"{fam}_n{n}"].n, REFINE[f"{fam}_n{n}"].m) for n in sizes] == [(n, 64) for n in sizes]
    assert rc.MAX_ROWS == 2048 and rc.TILE == 2048
    assert [(REFINE[name].n, REFINE[name].m) for name in rc.TILES] == [(300, m) for m in (5, 5, 2047, 2047, 2048, 2048, 2049, 2049)]
    assert (REFINE["few_n4"].n, REFINE["few_n4"].m, REFINE["few_m4"].n, REFINE["few_m4"].m) == (4, 40, 40, 4)


def test_the_lerp_family_reaches_the_exact_index_and_both_branches():
    """(n - 1) * 0.8 for n = 5 .. 11: t = .2, 0, .8, .6, .4, .2, 0 — zero is exact, and at t >= 0.5 the two forms of NumPy's
    _lerp give different bits on these rows, so a kernel without the second form returns another threshold."""
    want = {5: (3, 0.2), 6: (4, 0.0), 7: (4, 0.8), 8: (5, 0.6), 9: (6, 0.4), 10: (7, 0.2), 11: (8, 0.0)}
    for n, (lo_want, t_want) in want.items():
        lo, hi, t = rc.lerp_position(n)
        assert lo == lo_want and hi == lo + 1 and abs(t - t_want) < 1e-12 and (t == 0.0) == (t_want == 0.0), (n, lo, t)
        case = REFINE[f"lerp_n{n}"]
        s = _sorted_d2(case)
        assert len(np.unique(s)) == n, "no ties in this family"
        low_form, high_form = rc.lerp_forms(case.parts.d2)
        assert case.parts.thresh == (high_form if t >= 0.5 else low_form), n
        if t >= 0.5:
            assert low_form != high_form, (n, "the two forms of _lerp agree here: redraw the case")


def test_the_inlier_counts():
    """Four of five rows pass without ties (the prediction returns), exactly five of six, five of five when s[3] == s[4];
    every row when all distances are zero; and never fewer than five from six rows on."""
    five, six, tied, zero = REFINE["lerp_n5"], REFINE["lerp_n6"], REFINE["tie_n5"], REFINE["zero"]
    assert five.parts.k == 4 and np.array_equal(five.expected[:2], five.pred)
    assert six.parts.k == 5 and not np.array_equal(six.expected[:2], six.pred)
    s = _sorted_d2(tied)
    assert tied.parts.k == 5 and s[3] == s[4] and s[2] < s[3] and not np.array_equal(tied.expected[:2], [0.0, 0.0])
    assert zero.parts.k == zero.n == 9 and zero.parts.thresh == 0.0 and not zero.parts.d2.any()
    for case in REFINE.values():
        if case.parts is not None and case.n >= 6:
            assert case.parts.k >= 5, case.name
            assert case.parts.k >= rc.lerp_position(case.n)[0] + 1, case.name
    for name in ("few_n4", "few_m4"):
        case = REFINE[name]
        assert case.parts is None and np.array_equal(case.expected[:3], [*case.pred, 0.0]) and np.isnan(case.expected[3])


def test_the_tie_runs_sit_where_they_are_meant_to():
    """The exact cases' squared distances are (q / 4096)^2 with no rounding; a run of equal values covers lo and not hi,
    hi and not lo, or both; two distinct distances meet between lo and hi, below lo, above hi."""
    for n in (7, 1025):
        lo, hi, _ = rc.lerp_position(n)
        for tag in ("lo", "hi", "both"):
            case = REFINE[f"run_{tag}_n{n}"]
            s = _sorted_d2(case)
            assert np.array_equal(s, np.sort((case.props.q / 4096.0) ** 2)), case.name
            first, last = case.props.run
            assert first < last and (s[first:last + 1] == s[first]).all(), case.name
            assert (first == 0 or s[first - 1] < s[first]) and (last == n - 1 or s[last + 1] > s[last]), case.name
            others = np.delete(s, np.arange(first, last + 1))
            assert len(np.unique(others)) == len(others), case.name
            assert (first < lo <= last, first <= hi <= last) == {"lo": (True, False), "hi": (False, True), "both": (True, True)}[tag], case.name
        for tag, where in (("split", (True, False)), ("upper", (False, False)), ("lower", (True, True))):
            case = REFINE[f"two_{tag}_n{n}"]
            s = _sorted_d2(case)
            low = case.props.low
            assert len(np.unique(s)) == 2 and (s[:low] == s[0]).all() and (s[low:] == s[-1]).all() and 1 < low < n, case.name
            assert (lo < low, hi < low) == where, case.name                # which of lo, hi lie in the lower run
            assert case.parts.k == (n if tag == "upper" else low), case.name


def test_a_nearest_neighbour_tie_is_between_equal_rows_only():
    """Where two target rows are equally near a placed source row they hold the same coordinates: the matched row's
    coordinates, all the refinement uses of it, do not depend on the tie rule."""
    n_ties = 0
    for case in REFINE.values():
        p = case.parts
        if p is None:
            continue
        best = p.all_d2[np.arange(case.n), p.idx]
        i, j = np.nonzero(p.all_d2 == best[:, None])
        n_ties += len(i) - case.n
        assert np.array_equal(case.tgt[j], case.tgt[p.idx[i]]), case.name
    assert n_ties > 0                                                       # the twins of the tile family


def test_the_tile_family_matches_into_the_last_tile_or_its_twin():
    for name in rc.TILES:
        case = REFINE[name]
        m, p = case.m, case.parts
        last = case.props.which == m - 1
        assert last.sum() >= 40 and np.array_equal(p.idx[~last], case.props.which[~last]), name
        if case.props.twin:
            assert np.array_equal(case.tgt[0], case.tgt[m - 1]) and (p.idx[last] == 0).all(), name
            assert np.array_equal(p.all_d2[last, 0], p.all_d2[last, m - 1]), name
        else:
            assert (p.idx[last] == m - 1).all(), name
            # without the last tile the answer changes: the next best row is another one
            assert (np.sort(p.all_d2[last], axis=1)[:, 1] > p.all_d2[last, m - 1]).all(), name
    assert (rc.TILE + 1 - 1) // rc.TILE == 1                                # row 2 048 of 2 049 is alone in the second tile


def test_the_decoys_would_win_without_the_counts():
    tight, nan, decoy = REFINE["gap_tight"], REFINE["gap_nan"], REFINE["gap_decoy"]
    assert (tight.n, tight.m, tight.raw, nan.raw, decoy.raw) == (180, 120, (180, 120), (300, 200), (300, 200))
    assert np.array_equal(tight.expected, nan.expected) and np.array_equal(tight.expected, decoy.expected)
    _, _, _, _, src_gap, tgt_gap = rc.read_head(decoy.head)
    assert len(src_gap) == 120 and len(tgt_gap) == 80
    # every source row is nearer to a decoy of the target's gap than to any valid target row
    raw_tgt = np.vstack([decoy.tgt, tgt_gap])
    loose = rc.refine_parts(decoy.src, raw_tgt, decoy.cos_sin, decoy.pred)
    assert (loose.idx >= 120).all() and (loose.d2 < decoy.parts.d2).all()
    assert not np.array_equal(loose.t, decoy.expected[:2])
    # and reading the source's gap as rows changes the answer too
    raw_src = np.vstack([decoy.src, src_gap])
    assert not np.array_equal(rc.refine(raw_src, decoy.tgt, decoy.cos_sin, decoy.pred)[0], decoy.expected[:2])
    _, _, _, _, src_gap, tgt_gap = rc.read_head(nan.head)
    assert np.isnan(src_gap).all() and np.isnan(tgt_gap).all()


def test_the_record_variants_name_what_they_should():
    fine, nofine = REFINE["rec_fine"], REFINE["rec_nofine"]
    assert fine.rec == (2, 3, 1) and fine.cos_sin == (np.cos(rc.THETA), np.sin(rc.THETA))
    assert len(np.unique(np.concatenate([fine.fine.ravel(), fine.coarse]))) == fine.fine.size + 3     # any other entry is another angle
    assert nofine.rec == (1, 0, 0) and nofine.cos_sin == (np.cos(rc.THETA), np.sin(rc.THETA))
    assert nofine.fine[1, 0] != nofine.coarse[1] and nofine.max_fine == 4
    other = rc.refine(nofine.src, nofine.tgt, tuple(nofine.fine_cs[1, 0]), nofine.pred)
    assert not np.array_equal(other[0], nofine.expected[:2])


# ── the restatement against exact arithmetic ─────────────────────────────────────────────
@pytest.mark.parametrize("name", [n for n, c in REFINE.items() if c.parts is not None])
def test_the_threshold_against_exact_arithmetic(name):
    """The order statistics and A + (B - A) t in rationals (t: the float NumPy forms): np.percentile's value is within one
    ulp of it, and the rows at or below the one are the rows at or below the other."""
    p = REFINE[name].parts
    n = len(p.d2)
    exact_rows = [Fraction(float(x)) for x in p.d2]
    s = sorted(exact_rows)
    lo, hi, t = rc.lerp_position(n)
    exact = s[lo] + (s[hi] - s[lo]) * Fraction(t)
    assert abs(Fraction(float(p.thresh)) - exact) <= Fraction(float(np.spacing(p.thresh))), (name, p.thresh, float(exact))
    assert [x <= exact for x in exact_rows] == p.keep.tolist(), (name, "a row within rounding of the threshold: redraw the case")


def test_numpys_matmul_is_the_fma_form_on_these_rows():
    """The kernel forms a rotated row as fma(y, R[c][1], x * R[c][0]): one rounding of the exact y R[c][1] + fl(x R[c][0]).
    NumPy's (n, 2) @ (2, 2) must give that on every row of every case, or the GPU file's bit-for-bit comparison is with NumPy's
    product under the BLAS at hand and not with the formula."""
    rows = 0
    for case in REFINE.values():
        if case.parts is None:
            continue
        c, s = (float(v) for v in case.cos_sin)
        R = ((c, -s), (s, c))
        for (x, y), got in zip(case.src.tolist(), case.parts.rotated.tolist()):
            for col in (0, 1):
                want = float(Fraction(y) * Fraction(R[col][1]) + Fraction(x * R[col][0]))
                assert got[col] == want, (f"{case.name}: NumPy's matmul is not fma(y, R[c][1], x * R[c][0]) with this BLAS — the "
                                          "restatement follows NumPy, the kernel the formula", x, y, got[col], want)
            rows += 1
    assert rows > 10000


def test_the_head_round_trips():
    for name in ("gap_tight", "gap_nan", "gap_decoy", "cap_n2048", "few_n4"):
        case = REFINE[name]
        off, cnt, src, tgt, src_gap, tgt_gap = rc.read_head(case.head)
        assert off.tolist() == [0, case.raw[0], case.raw[0] + case.raw[1]] and cnt.tolist() == [case.n, case.m], name
        assert np.array_equal(src, case.src) and np.array_equal(tgt, case.tgt), name
        assert (len(src_gap), len(tgt_gap)) == (case.raw[0] - case.n, case.raw[1] - case.m), name
        assert len(case.head) == rc.WS_CLOUDS + 16 * sum(case.raw), name
    assert (rc.WS_COUNTS, rc.WS_CLOUDS) == (16, 256)
    decoy = REFINE["gap_decoy"]
    _, _, _, _, src_gap, tgt_gap = rc.read_head(decoy.head)
    assert np.array_equal(src_gap, np.resize(decoy.props.decoys, (120, 2))) and np.array_equal(tgt_gap, np.resize(decoy.props.decoys, (80, 2)))
    assert (decoy.head[12:16] == 0xA5).all() and (decoy.head[24:256] == 0xA5).all()


def test_refusals_of_the_refinement_decided_on_the_host():
    """Above ICPMI_RSR_MAX_ROWS, a scratch one byte short, a fine table announced and not given: refused before any launch
    (the device pointers are fakes that are never dereferenced)."""
    from icpmi import _lib
    L = _lib.lib()
    FAKE = 4096

    def call(n_src=300, fine_cs=None, max_fine=0, short=0):
        need = L.icpmi_rotation_refine_workspace_bytes(n_src)
        return L.icpmi_rotation_refine(FAKE, n_src, 200, FAKE, FAKE, fine_cs, max_fine, 0.0, 0.0, FAKE, FAKE, need - short, None)

    assert call(n_src=rc.MAX_ROWS + 1) == _lib.ERR_UNSUPPORTED
    assert call(short=1) == _lib.ERR_WORKSPACE
    assert call(n_src=rc.MAX_ROWS, short=1) == _lib.ERR_WORKSPACE
    assert call(max_fine=4, fine_cs=None) == _lib.ERR_ARG
    assert call(n_src=0) == _lib.ERR_ARG


# ── the search cases ─────────────────────────────────────────────────────────────
def _second_best(ref, angles, best):
    """The lowest reference score among the entries that are not the best entry's angle."""
    other = ~np.isnan(angles) & (angles != angles[best])
    return ref[other].min() if other.any() else np.inf


@pytest.mark.parametrize("name", list(SEARCH))
def test_the_search_tables_decide_by_construction(name):
    """The filter keeps every row; the designed winner is the oracle's arg-min of the coarse table (among the angles that
    are numbers) and of its fine row, with a margin above the bound between a device score and the oracle's — ties and
    NaN are then decided by index alone, as np.argmin decides them."""
    case = SEARCH[name]
    assert [len(c) for c in case.filtered] == [len(case.src), len(case.tgt)]
    ref = case.oracle_scores(case.coarse)
    bound = rc.score_bound(ref)
    finite_best = int(np.nanargmin(ref))
    assert ref[finite_best] + bound < _second_best(ref, case.coarse, finite_best), name
    assert case.coarse[finite_best] == rc.THETA
    assert case.K == int(np.argmin(ref)), (name, case.K, int(np.argmin(ref)))             # np.argmin: the first NaN, else the first minimum
    assert case.NF == (int(case.fine_n[case.K]) if case.max_fine else 0)
    if case.NF:
        fref = case.oracle_scores(case.fine[case.K, :case.NF])
        assert case.J == int(np.argmin(fref)) and fref[case.J] + rc.score_bound(fref) < _second_best(fref, case.fine[case.K, :case.NF], case.J), name
    else:
        assert case.J == 0


def test_the_tied_and_nan_tables_are_what_the_reduction_has_to_survive():
    where = {"tie_3_259": (3, 259), "tie_70_130": (70, 130), "tie_0_299": (0, 299), "tie_0_1024": (0, 1024)}
    for name, (a, b) in where.items():
        case = SEARCH[name]
        hits = np.nonzero(case.coarse == rc.THETA)[0].tolist()
        assert hits == [a, b] and case.K == a and case.tied and b == (len(case.coarse) - 1 if a == 0 else b), name
        assert len(np.unique(case.fine_n)) == len(case.coarse) and case.NF == case.fine_n[a] != case.fine_n[b], name
        assert len(case.src) == len(case.tgt) == 300
    # one thread's first and second trip at 256 threads; different waves at 256, another thread's later trip at 64
    assert 3 % 256 == 259 % 256 and 70 // 64 != 130 // 64 and (70 % 64, 70 // 64, 130 % 64, 130 // 64) == (6, 1, 2, 2)
    assert len(SEARCH["tie_0_1024"].coarse) == 1025 and len(SEARCH["single_angle"].coarse) == 1
    for name, nans, K in (("nan_after", [200], 200), ("nan_before", [100], 100), ("nan_twice", [120, 220], 120)):
        case = SEARCH[name]
        assert np.nonzero(np.isnan(case.coarse))[0].tolist() == nans and case.K == K, name
        assert np.nonzero(case.coarse == rc.THETA)[0].tolist() == [150] and not np.isnan(case.fine).any(), name


def test_the_ragged_tables_hide_the_true_rotation_behind_the_count():
    for name, cnt in (("ragged_1", 1), ("ragged_3", 3), ("ragged_full", 6), ("ragged_0", 0)):
        case = SEARCH[name]
        assert case.max_fine == 6 and case.fine_n[7] == cnt == case.NF and case.K == 7, name
        assert (case.fine[7, cnt:] == rc.THETA).all() and (case.fine[7, :cnt] != rc.THETA).all(), name
        if 0 < cnt < 6:
            row = case.oracle_scores(case.fine[7])
            assert int(np.argmin(row)) >= cnt > case.J, name                    # the decoy would win if the count were ignored
    assert SEARCH["no_fine_tables"].max_fine == 0 and SEARCH["no_fine_tables"].fine.size == 0


def test_the_means_family():
    for n in rc.MEANS_ROWS:
        for mode, centred in (("centred", True), ("shifted", False)):
            case = SEARCH[f"means_n{n}_{mode}"]
            assert len(case.src) == len(case.tgt) == n and case.centred == centred
    assert rc.MEANS_ROWS == (5, 7, 8, 9, 255, 256, 257, 263, 520)    # under, at and over the 8-way tail, a batch of 256 and one more, 256 + 7, two batches + 8
    assert not float(rc.PRED[0]).is_integer() and not float(rc.PRED[1]).is_integer()
