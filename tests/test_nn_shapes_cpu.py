"""The nearest-neighbour kernels' launch shapes, without a GPU: the reference of tests/nn_ref.py against the CPU oracle
(brute force and k-d tree) on the tie cases and a sample of the size cases; icpmi_nn_batch_plan — the library's own
launch rule, which icpmi_nn_batch itself goes by — on either side of both of its thresholds, read off by bisection; and
the refusals of icpmi_nn_batch / icpmi_nn_prepared_batch, decided on the host before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import nn_ref
import oracle
from nn_ref import MANY_PAIRS, first_pairs_with, plan

GRID_Y_MAX = 65535                     # HIP's limit on a grid's y extent: a batch beyond it goes down in slices


@pytest.fixture(scope="module")
def L():
    import icpmi
    icpmi.build()
    return icpmi.lib()


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in p._fields_)


# ── the reference against the oracle ────────────────────────────────────────────────────────────────────────────────
def both_oracles_equal(src, tgt, what):
    idx, dist, second = nn_ref.reference(src, tgt)
    for kdtree in (False, True):
        do, io = oracle.nn(src, tgt, kdtree=kdtree)
        assert np.array_equal(idx, io) and np.array_equal(dist, do), (what, kdtree)
    if len(tgt) > 1:                                                  # the second of a row: the smallest with the winner's row taken out
        for r in range(0, len(src), max(len(src) // 40, 1)):
            rest = np.delete(np.asarray(tgt, dtype=np.float64), idx[r], axis=0)
            assert np.sqrt(second[r]) == nn_ref.reference(src[r:r + 1], rest)[1][0], (what, r)
    else:
        assert np.all(np.isinf(second))
    return idx


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_equals_both_oracles_on_ties_and_sizes(dim):
    cs = nn_ref.cases(dim)
    T = nn_ref.tile_rows(dim)
    hits = {}
    for m in nn_ref.TARGET_SIZES[dim]:
        n = 400 if m > T + 1 else nn_ref.MASTER_ROWS                  # a sample of the rows on the large targets
        src = cs.source(n, k=m)
        idx = both_oracles_equal(src, cs.target(m), (dim, m))
        assert all(np.array_equal(a, b) for a, b in zip(cs.answer(m, n, k=m), nn_ref.reference(src, cs.target(m)))), (dim, m)
        hits[m] = set(idx.tolist())
    # the planted rows do what they are there for: the lower row of every duplicate wins and the higher never does
    big = max(nn_ref.TARGET_SIZES[dim])
    third = 2 * T + 5 if big > 2 * T + 5 else 2 * T
    assert {0, 15, 14, T - 1, T - 2, 5, 3, 2} <= hits[big] and not {16, 17, T, T + 5, third, 9} & hits[big]
    assert 32 in hits[33]                                             # the last row of a cloud with m % 16 == 1, alone in its chunk
    # a window of the master source is what it says
    assert np.array_equal(cs.source(5, k=3), cs.master[291:296]) and len(cs.source(nn_ref.MASTER_ROWS, k=9)) == nn_ref.MASTER_ROWS


def test_reference_on_the_shuffled_lattice_and_the_empty_target():
    s, t = nn_ref.lattice_case()
    idx = both_oracles_equal(s, t, "lattice")
    d2 = ((s[:, None, :] - t[None, :, :]) ** 2).sum(axis=2)
    assert np.all((d2 == 0.5).sum(axis=1) == 4)                       # four-way ties everywhere
    assert np.array_equal(idx, [int(np.flatnonzero(row == 0.5)[0]) for row in d2])
    idx, dist, second = nn_ref.reference(s[:3], np.empty((0, 2)))
    assert np.array_equal(idx, [-1, -1, -1]) and np.all(np.isinf(dist)) and np.all(np.isinf(second))
    for dim in (2, 3):
        clouds, cnt, src_ids, tgt_ids = nn_ref.decoy_set(dim)
        for si in src_ids:
            for ti in tgt_ids:
                valid = nn_ref.reference(clouds[si], clouds[ti][:cnt[ti]])[0]
                full = nn_ref.reference(clouds[si], clouds[ti])[0]
                assert np.all(valid < cnt[ti]) and np.all(full >= cnt[ti])    # a decoy is nearer to every row than any valid row


def test_source_sizes_reach_every_body():
    for threads, spl in ((256, 1), (256, 2), (256, 4), (64, 3)):
        W = threads * spl
        sizes = nn_ref.source_sizes(W, threads)
        assert {1, threads - 1, threads, threads + 1, W - 1, W, W + 1, 2 * W} <= set(sizes) and max(sizes) == 2 * W
        reached = set().union(*(nn_ref.slots_reached(n, W, threads) for n in sizes))
        assert reached == {(first, k) for first in (True, False) for k in range(1, spl + 1)}


# ── the plan ────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("dim", [2, 3])
def test_plan_on_either_side_of_both_thresholds(L, dim):
    top = plan(L, MANY_PAIRS, 1, dim)
    one = plan(L, 1, 1, dim)
    assert (one.rows_per_lane, top.rows_per_lane) == (1, 4) and one.threads == top.threads
    # what the planted rows of nn_ref.py go by
    assert top.tile_points == one.tile_points == nn_ref.tile_rows(dim) and top.chunk == nn_ref.CHUNK_ROWS[1] and top.tile_points % top.chunk == 0
    assert top.tile_points * dim * 8 <= 32768                         # the tile the kernel declares: 32 KiB of LDS
    W4, W2 = top.rows_per_wg, 2 * top.threads
    seen = set()
    for max_src_n in (1, top.threads, W2, W2 + 1, W4, W4 + 1, 3 * W4, 3 * W4 + 1, 1430, 8191):
        n2, n4 = first_pairs_with(L, 2, max_src_n, dim), first_pairs_with(L, 4, max_src_n, dim)
        assert 1 < n2 < n4
        for n_pairs, want in ((n2 - 1, 1), (n2, 2), (n4 - 1, 2), (n4, 4), (1, 1), (MANY_PAIRS, 4)):
            p = plan(L, n_pairs, max_src_n, dim)
            assert p.rows_per_lane == want, (max_src_n, n_pairs)
            assert p.rows_per_wg == p.threads * p.rows_per_lane
            assert p.grid_x == -(-max_src_n // p.rows_per_wg) and p.grid_x * p.rows_per_wg >= max_src_n
            assert p.launches == -(-n_pairs // GRID_Y_MAX)
            assert (p.threads, p.tile_points, p.chunk) == (top.threads, top.tile_points, top.chunk)
            seen.add(p.rows_per_lane)
        # both thresholds count workgroups: the first n_pairs falls as the tiles per pair rise
        t2, t4 = -(-max_src_n // W2), -(-max_src_n // W4)
        assert n2 == -(-first_pairs_with(L, 2, 1, dim) // t2) and n4 == -(-first_pairs_with(L, 4, 1, dim) // t4)
    assert seen == {1, 2, 4}
    # slices of pairs on either side of the grid's y extent
    assert [plan(L, n, 300, dim).launches for n in (1, GRID_Y_MAX, GRID_Y_MAX + 1, 2 * GRID_Y_MAX, 2 * GRID_Y_MAX + 1)] == [1, 1, 2, 2, 3]
    # dim changes the tile and nothing else
    assert as_tuple(plan(L, 700, 1430, 2))[:3] == as_tuple(plan(L, 700, 1430, 3))[:3]


def test_plan_refusals_and_the_plan_of_zeros(L):
    from icpmi import _lib
    p = _lib.NnPlan()
    for args in ((-1, 10, 2), (10, -1, 2), (10, 10, 1), (10, 10, 4), (10, 10, 0)):
        p.rows_per_lane = 99
        assert L.icpmi_nn_batch_plan(*args, C.byref(p)) == _lib.ERR_ARG, args
        assert p.rows_per_lane == 99                                  # a refusal leaves the plan alone
    assert L.icpmi_nn_batch_plan(10, 10, 2, None) == _lib.ERR_ARG
    for args in ((0, 10, 2), (10, 0, 3), (0, 0, 2)):
        p.rows_per_lane = p.launches = 99
        assert L.icpmi_nn_batch_plan(*args, C.byref(p)) == _lib.OK and as_tuple(p) == (0,) * 7, args
    assert [f for f, _ in _lib.NnPlan._fields_] == ["rows_per_lane", "threads", "rows_per_wg", "tile_points", "chunk", "grid_x", "launches"]


# ── refusals of the two entries ─────────────────────────────────────────────────────────────────────────────────────
def test_host_refusals_come_before_any_launch(L):
    """Fake device pointers: every refusal below, and every call that has nothing to launch, is decided on the host
    before the first HIP call, so none of the pointers is ever touched."""
    from icpmi import _lib
    pts, off, cnt, ps, pt, oi, od, prep, o2 = [C.c_void_p(0x1000 * (k + 1)) for k in range(9)]

    def nn(pts=pts, off=off, cnt=cnt, ps=ps, pt=pt, n_pairs=4, max_src_n=100, dim=2, oi=oi, od=od, stride=100):
        return L.icpmi_nn_batch(pts, off, cnt, ps, pt, n_pairs, max_src_n, dim, oi, od, stride, None)

    def swept(pts=pts, off=off, cnt=cnt, prep=prep, ps=ps, pt=pt, n_pairs=4, max_src_n=100, max_tgt_n=200, total=1000, oi=oi, od=od,
              o2=o2, stride=100):
        return L.icpmi_nn_prepared_batch(pts, off, cnt, prep, ps, pt, n_pairs, max_src_n, max_tgt_n, total, oi, od, o2, stride, None)

    for call in (nn, swept):
        for name in ("pts", "off", "ps", "pt", "oi", "od"):
            assert call(**{name: None}) == _lib.ERR_ARG, (call.__name__, name)
        assert call(n_pairs=-1) == _lib.ERR_ARG and call(max_src_n=-1) == _lib.ERR_ARG
        assert call(stride=99) == _lib.ERR_ARG and call(max_src_n=101) == _lib.ERR_ARG        # out_stride < max_src_n
        assert call(n_pairs=0) == _lib.OK and call(n_pairs=0, cnt=None) == _lib.OK
        assert call(max_src_n=0, stride=0) == _lib.OK
    for dim in (-1, 0, 1, 4):
        assert nn(dim=dim) == _lib.ERR_ARG
    assert nn(n_pairs=0, dim=3) == _lib.OK and nn(n_pairs=0, dim=4) == _lib.ERR_ARG
    assert swept(prep=None) == _lib.ERR_ARG and swept(max_tgt_n=-1) == _lib.ERR_ARG
    assert swept(n_pairs=0, o2=None) == _lib.OK
    assert swept(max_tgt_n=nn_ref.SWEEP_MAX_ROWS + 1) == _lib.ERR_UNSUPPORTED
    assert swept(max_tgt_n=nn_ref.SWEEP_MAX_ROWS, n_pairs=0) == _lib.OK
    assert swept(max_tgt_n=nn_ref.SWEEP_MAX_ROWS + 1, stride=99) == _lib.ERR_ARG             # a bad argument is named first
