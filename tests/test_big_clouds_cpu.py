"""The clouds, references and bounds of tests/big_cloud_cases.py, checked without a GPU: the table of NumPy's figures holds,
the inputs meet the conditions the GPU tests rest on, a single wrong neighbour is visible at every compared point, and the
two host entries refuse large clouds they cannot serve before anything is enqueued.

That a cloud of 8 192 rows needs no workspace for icpmi_normals_2d_batch is a call that launches: it is made in
tests/test_big_clouds_gpu.py (icpmi_normals_workspace_bytes for it is pinned in tests/test_host_cpu.py).  That
icpmi_prepare_targets_ex refuses a cloud above 4 096 rows without the host offsets is pinned in
tests/test_sort_layouts_gpu.py."""
import functools

import numpy as np

import oracle
from big_cloud_cases import (BIG_TABLE, COLUMNS, DECOYS, FAMILY, GAP_SHARE, KS, TIE_PER_K, all_cases, big_bound, cloud, columns,
                             compared, decoys, normals_of_sets, reference, ties, uniform)
from test_p2l_step_cpu import GAP_MIN, normal_angle_units, numpy_normals


@functools.lru_cache(maxsize=None)
def _measure():
    """(name, n, k) -> (largest angle of NumPy's float64 eigh(np.cov) off the reference over the compared points, the same
    of the oracle's normals_2d, share of points not compared)."""
    out = {}
    for name, n, ks in all_cases():
        pts = cloud(name, n)
        for k in ks:
            if name == "duplicates" and k < 4:
                continue
            ref, gap, nb = reference(name, n, k)
            ok = compared(name, n, k)
            out[(name, n, k)] = (float(normal_angle_units(numpy_normals(pts, nb), ref, gap)[ok].max()),
                                 float(normal_angle_units(oracle.normals_2d(pts, k), ref, gap)[ok].max()), 1.0 - float(ok.mean()))
    return out


def test_numpy_stays_within_the_table_and_the_oracle_within_the_bound():
    seen = {}
    for (name, n, k), (numpy_units, oracle_units, _) in _measure().items():
        fam = FAMILY[name]
        row = seen.setdefault((fam, k), [0.0, 0.0])
        row[0], row[1] = max(row[0], numpy_units), max(row[1], oracle_units)
        assert numpy_units <= BIG_TABLE[fam], (name, n, k, numpy_units)
        assert oracle_units <= big_bound(fam), (name, n, k, oracle_units)
    print("\nfamily       k   NumPy eigh(np.cov)   oracle   [2^-52 l1 / (l1 - l0)]")
    for (fam, k), (a, b) in sorted(seen.items()):
        print(f"  {fam:11s} {k:2d} {a:12.3g} {b:14.3g}")
    print("family       NumPy, every k   table   bound")
    for fam in BIG_TABLE:
        worst = max(v[0] for (f, _), v in seen.items() if f == fam)
        print(f"  {fam:11s} {worst:10.3g} {BIG_TABLE[fam]:12.3g} {big_bound(fam):8.3g}")
        assert worst > 0.5 * BIG_TABLE[fam], fam                           # the entry is this family's figure, not a loose one


def test_nearly_every_point_has_a_direction():
    for (name, n, k), (_, _, share) in _measure().items():
        assert share <= GAP_SHARE[FAMILY[name]], (name, n, k, share)
        if name in ("uniform", "uniform_far"):
            assert share == 0.0, (name, n, k, share)


def test_columns_hold_a_hundred_rows_each():
    for n in (8193, 16385):
        x, count = np.unique(columns(n)[:, 0], return_counts=True)
        assert len(x) == COLUMNS and count.min() >= 100, (n, len(x), count.min())
        assert np.array_equal(x * 8, np.rint(x * 8))                      # multiples of 2^-3: exact keys


def test_decoys_lie_nearer_than_any_valid_row():
    for cap, count in DECOYS:
        pts = decoys(cap, count)
        assert pts.shape == (cap, 2)
        valid = pts[:count]
        d2, _ = oracle.knn(valid, valid, 2)
        target = np.arange(cap - count) % count                          # the valid row a decoy is placed at
        gap = ((pts[count:] - valid[target]) ** 2).sum(axis=1)
        assert (gap < d2[target, 1]).all() and (gap > 0).all(), (cap, count)


def test_planted_ties_are_exact_and_the_two_choices_far_apart():
    for n in (8193, 16385):
        pts, planted = ties(n)
        assert len(pts) == n and len(np.unique(pts, axis=0)) == n
        assert sorted(planted) == sorted(KS) and all(len(p) == TIE_PER_K for p in planted.values())
        for k, rows in planted.items():
            q, a, b = rows.T
            da = ((pts[a] - pts[q]) ** 2).sum(axis=1)
            db = ((pts[b] - pts[q]) ** 2).sum(axis=1)
            assert np.array_equal(da, db)                                  # bit-equal in float64
            assert (np.abs(np.sum((pts[a] - pts[q]) * (pts[b] - pts[q]), axis=1)) == 0).all()      # at right angles
            low, high = np.minimum(a, b), np.maximum(a, b)
            assert 5 <= int((a < b).sum()) <= TIE_PER_K - 5, (n, k)         # either candidate is the lower row often enough
            ref, gap, nb = reference("ties", n, k)
            sets = nb[q]
            # the reference's list: the query, the k - 1 inner rows, and the LOWER candidate in the last slot
            assert (sets[:, -1] == low).all() and not (sets == high[:, None]).any(), (n, k)
            assert (((pts[sets[:, -2]] - pts[q]) ** 2).sum(axis=1) < da).all(), (n, k)
            assert (gap[q] >= GAP_MIN).all(), (n, k)
            other = sets.copy()
            other[:, -1] = high
            units = normal_angle_units(normals_of_sets(pts, other), ref[q], gap[q])
            assert units.min() > 1e6 * big_bound("ties"), (n, k, float(units.min()))
            # and the helper is the reference's arithmetic
            assert normal_angle_units(normals_of_sets(pts, sets).astype(np.float64), ref[q], gap[q]).max() <= 1.0


def test_one_wrong_neighbour_exceeds_the_bound_at_every_compared_point():
    """The farthest neighbour swapped for the next one out: the GPU tests can see the search, not only the arithmetic."""
    pts = uniform(8193)
    for k in (1, 7, 15, 31):
        ref, gap, nb = reference("uniform", 8193, k)
        _, wider = oracle.knn(pts, pts, k + 2)
        assert np.array_equal(wider[:, :k + 1], nb)
        wrong = np.concatenate([nb[:, :k], wider[:, k + 1:]], axis=1)
        units = normal_angle_units(normals_of_sets(pts, wrong), ref, gap)
        ok = compared("uniform", 8193, k)
        print(f"k {k}: one wrong neighbour moves the normal by at least {units[ok].min():.3g} units")
        assert units[ok].min() > big_bound("uniform"), (k, float(units[ok].min()))


# ── host refusals at large sizes ─────────────────────────────────────────────────────────────────────────────────────────────
FAKE, OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 4096, 0, -1, -2, -4      # include/icpmi.h; the pointers are never dereferenced


def test_normals_entry_refuses_a_large_cloud_without_its_workspace():
    import icpmi
    L = icpmi.lib()
    total, max_n = 20000, 8193
    need = L.icpmi_normals_workspace_bytes(total, max_n)
    assert need > 256

    def call(k, ws, ws_bytes):
        return L.icpmi_normals_2d_batch(FAKE, FAKE, None, None, 2, total, max_n, k, FAKE, ws, ws_bytes, None)
    assert call(12, None, 0) == ERR_WORKSPACE
    assert call(12, None, need) == ERR_WORKSPACE                          # a size without a buffer
    assert call(12, FAKE, need - 1) == ERR_WORKSPACE                      # one byte short
    assert call(32, FAKE, need) == ERR_UNSUPPORTED                        # the lists are registers: k <= 31
    assert L.icpmi_normals_2d_batch(FAKE, FAKE, None, None, 0, total, max_n, 12, FAKE, None, 0, None) == OK    # no cloud selected


def test_prepare_entry_refuses_a_large_selection_it_cannot_route():
    import icpmi
    L = icpmi.lib()
    off = np.array([0, 8193, 8200], dtype=np.int32)
    ids = np.array([1, 0], dtype=np.int32)
    total, clouds, max_n = 8200, 2, 8193
    need = L.icpmi_prepared_bytes(total, clouds, max_n)
    assert need > L.icpmi_prepared_bytes(total, clouds, 4096)            # the scratch of the sort is part of it

    def call(ids_dev, ids_host, nbytes, off_host=off.ctypes.data):
        return L.icpmi_prepare_targets_ex(FAKE, FAKE, off_host, None, ids_dev, ids_host, 2, clouds, total, max_n, 12, FAKE, FAKE,
                                          nbytes, 1, None)
    assert call(FAKE, None, need) == ERR_ARG                              # a selection on the device alone: nothing to route by
    assert call(FAKE, ids.ctypes.data, need - 1) == ERR_WORKSPACE         # one byte short
    assert call(None, None, need - 1) == ERR_WORKSPACE
    assert call(None, None, need - 1, off_host=None) == ERR_WORKSPACE     # (the size is judged first)
