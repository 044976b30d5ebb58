"""The nearest-neighbour kernels in every launch shape they take (csrc/nn.hip, csrc/nn_sweep.hip) against the NumPy
reference of tests/nn_ref.py, bit for bit.

icpmi_nn_batch picks the rows per lane S from the size of the launch and every workgroup then runs the body for
SE <= S rows: seven bodies per dimension.  The tests call the C entry directly, so n_pairs and max_src_n fix the launch
shape whatever the data, ask the library's own plan (icpmi_nn_batch_plan) which S a launch gets — no threshold is
restated here — and take the source sizes against the plan's rows per workgroup.  A handful of clouds is reused by
thousands of pairs; the reference is evaluated once per target."""
import numpy as np
import pytest

import nn_ref
from nn_ref import DIST_SENTINEL, IDX_SENTINEL, first_pairs_with, plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import icpmi
    from icpmi import batch
    return torch, icpmi.lib(), batch


def sentinel_outs(torch, rows, stride, dev, second=False):
    idx = torch.full((rows, stride), IDX_SENTINEL, dtype=torch.int32, device=dev)
    dist = torch.full((rows, stride), DIST_SENTINEL, dtype=torch.float64, device=dev)
    return (idx, dist, torch.full((rows, stride), DIST_SENTINEL, dtype=torch.float64, device=dev)) if second else (idx, dist)


def nn_batch(gpu, cs, cnt, ps, pt, max_src_n, stride, use_cnt=True):
    """icpmi_nn_batch itself on sentinel-filled out buffers -> (idx, dist) device tensors [n_pairs, stride]."""
    torch, L, batch = gpu
    from icpmi._lib import check
    p = batch.PairList(ps, pt).to(cs.pts.device)
    idx, dist = sentinel_outs(torch, p.B, stride, cs.pts.device)
    check(L.icpmi_nn_batch(batch._ptr(cs.pts), batch._ptr(cs.off), batch._ptr(cnt if use_cnt else None), batch._ptr(p.src),
                           batch._ptr(p.tgt), p.B, max_src_n, cs.dim, batch._ptr(idx), batch._ptr(dist), stride, batch._stream()), "nn")
    return idx, dist


def nn_prepared(gpu, cs, cnt, ps, pt, max_src_n, stride):
    """icpmi_prepare_targets + icpmi_nn_prepared_batch on sentinel-filled out buffers -> (idx, dist, second)."""
    torch, L, batch = gpu
    from icpmi._lib import check
    dev = cs.pts.device
    p = batch.PairList(ps, pt).to(dev)
    tgt_ids = np.unique(p.tgt_host).astype(np.int32)
    max_tgt = int(np.diff(cs.off_host)[tgt_ids].max())
    prepared = torch.empty(L.icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, max_tgt), dtype=torch.uint8, device=dev)
    ids = torch.from_numpy(tgt_ids).to(dev)
    check(L.icpmi_prepare_targets(batch._ptr(cs.pts), batch._ptr(cs.off), None, batch._ptr(cnt), batch._ptr(ids), None, len(tgt_ids),
                                  cs.n_clouds, cs.total_rows, max_tgt, -1, None, batch._ptr(prepared), prepared.numel(),
                                  batch._stream()), "prepare_targets")
    idx, dist, second = sentinel_outs(torch, p.B, stride, dev, second=True)
    check(L.icpmi_nn_prepared_batch(batch._ptr(cs.pts), batch._ptr(cs.off), batch._ptr(cnt), batch._ptr(prepared), batch._ptr(p.src),
                                    batch._ptr(p.tgt), p.B, max_src_n, max_tgt, cs.total_rows, batch._ptr(idx), batch._ptr(dist),
                                    batch._ptr(second), stride, batch._stream()), "nn (sweep)")
    return idx, dist, second


def expected_rows(answers, stride):
    """[(idx, dist) of the rows a pair writes] -> (idx, dist) arrays [len(answers), stride], the sentinel elsewhere."""
    idx = np.full((len(answers), stride), IDX_SENTINEL, dtype=np.int32)
    dist = np.full((len(answers), stride), DIST_SENTINEL)
    for c, (i, d) in enumerate(answers):
        idx[c, :len(i)], dist[c, :len(d)] = i, d
    return idx, dist


def assert_same(torch, got, want, combo_of_pair, what):
    """A device tensor [n_pairs, stride] against the expected rows of every pair's combination, bit for bit."""
    dev = got.device
    want = torch.from_numpy(want).to(dev)[torch.from_numpy(np.asarray(combo_of_pair, dtype=np.int64)).to(dev)]
    bits = (lambda t: t.view(torch.int64)) if got.dtype == torch.float64 else (lambda t: t)
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        b, n = (int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} entries differ, the first at pair {b} (combination {combo_of_pair[b]}) row {n}: "
                    f"{got[b, n].item()!r} for {want[b, n].item()!r}")


# ── every body ──────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("rows_per_lane", [1, 2, 4])
@pytest.mark.parametrize("dim", [2, 3])
def test_every_body_equals_the_reference(gpu, dim, rows_per_lane):
    """One launch whose plan says S = rows_per_lane: every source size of nn_ref.source_sizes (each SE <= S on a first and
    on a later tile) against every target size, with the planted ties; an empty source and an empty target among them.
    Indices and distances of every pair, and the sentinel on every row a pair does not own, bit for bit."""
    torch, L, batch = gpu
    cs = nn_ref.cases(dim)
    threads = plan(L, 1, 1, dim).threads
    W = threads * rows_per_lane
    sizes = [0] + nn_ref.source_sizes(W, threads)
    targets = [0] + list(nn_ref.TARGET_SIZES[dim])
    max_src_n = stride = max(sizes)
    reached = set().union(*(nn_ref.slots_reached(n, W, threads) for n in sizes))
    assert reached == {(first, k) for first in (True, False) for k in range(1, rows_per_lane + 1)}
    combos = [(si, ti) for ti in range(len(targets)) for si in range(len(sizes))]
    small = [c for c, (si, ti) in enumerate(combos) if targets[ti] <= 33]
    # the smallest batch the library gives this many rows per lane (S = 1: just the combinations)
    n_pairs = max(len(combos), first_pairs_with(L, rows_per_lane, max_src_n, dim) if rows_per_lane > 1 else 0)
    p = plan(L, n_pairs, max_src_n, dim)
    assert p.rows_per_lane == rows_per_lane and p.rows_per_wg == W and p.grid_x == 2 and p.launches == 1
    assert p.tile_points == nn_ref.tile_rows(dim) and p.chunk == nn_ref.CHUNK_ROWS[1]
    # every combination once, then the ones with small targets over again (the large targets go to a few pairs only)
    combo_of_pair = np.concatenate([np.arange(len(combos)), np.resize(small, n_pairs - len(combos))]).astype(np.int64)
    clouds = [cs.source(n, k) for k, n in enumerate(sizes)] + [cs.target(m) if m else np.empty((0, dim)) for m in targets]
    pairs = np.array(combos)[combo_of_pair]
    answers = []
    for si, ti in combos:
        n, m = sizes[si], targets[ti]
        answers.append(cs.answer(m, n, si)[:2] if m else nn_ref.reference(cs.source(n, si), np.empty((0, dim)))[:2])
    want_idx, want_dist = expected_rows(answers, stride)
    assert (want_idx[combos.index((1, 0))] == -1).sum() == sizes[1] and np.isinf(want_dist[combos.index((1, 0))]).sum() == sizes[1]
    cloud_set = batch.CloudSet.from_numpy(clouds)
    idx, dist = nn_batch(gpu, cloud_set, None, pairs[:, 0], len(sizes) + pairs[:, 1], max_src_n, stride)
    assert_same(torch, idx, want_idx, combo_of_pair, f"index, dim {dim}, S {rows_per_lane}")
    assert_same(torch, dist, want_dist, combo_of_pair, f"distance, dim {dim}, S {rows_per_lane}")


def test_shuffled_lattice_four_way_ties(gpu):
    torch, L, batch = gpu
    s, t = nn_ref.lattice_case()
    want = nn_ref.reference(s, t)
    cloud_set = batch.CloudSet.from_numpy([s, t])
    idx, dist = nn_batch(gpu, cloud_set, None, [0], [1], len(s), len(s))
    assert np.array_equal(idx.cpu().numpy()[0], want[0]) and np.array_equal(dist.cpu().numpy()[0], want[1])
    idx, dist, second = nn_prepared(gpu, cloud_set, None, [0], [1], len(s), len(s))
    assert np.array_equal(idx.cpu().numpy()[0], want[0]) and np.array_equal(dist.cpu().numpy()[0], want[1])
    assert np.array_equal(second.cpu().numpy()[0], want[2]) and np.all(want[2] == 0.5)


# ── the two count paths ─────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("dim, entry", [(2, "batch"), (3, "batch"), (2, "prepared")])       # (the sweep search is 2-D only)
def test_counts_on_the_device_and_capacity_counts(gpu, dim, entry):
    """Clouds whose capacity exceeds their count, decoy rows behind the count of every target that are nearer to every
    source row than any valid row.  With cnt_dev: decoys are ignored and rows behind the source count stay unwritten.
    With cnt_dev == NULL the same buffers are searched at full capacity: the decoys win."""
    torch, L, batch = gpu
    clouds, cnt, src_ids, tgt_ids = nn_ref.decoy_set(dim)
    cloud_set = batch.CloudSet.from_numpy(clouds)
    cnt_dev = torch.from_numpy(cnt).to(cloud_set.pts.device)
    combos = [(si, ti) for si in src_ids for ti in tgt_ids]
    ps, pt = [c[0] for c in combos], [c[1] for c in combos]
    max_src_n = stride = max(len(clouds[si]) for si in src_ids)
    for counted in (True, False):
        rows = (lambda c: clouds[c][:cnt[c]]) if counted else (lambda c: clouds[c])
        refs = [nn_ref.reference(rows(si), rows(ti)) for si, ti in combos]
        assert all(np.all((r[0] < cnt[ti]) == counted) for r, (si, ti) in zip(refs, combos))
        want_idx, want_dist = expected_rows([r[:2] for r in refs], stride)
        if entry == "batch":
            idx, dist = nn_batch(gpu, cloud_set, cnt_dev, ps, pt, max_src_n, stride, use_cnt=counted)
        else:
            idx, dist, second = nn_prepared(gpu, cloud_set, cnt_dev if counted else None, ps, pt, max_src_n, stride)
            want_second = expected_rows([(r[0], r[2]) for r in refs], stride)[1]
            assert_same(torch, second, want_second, np.arange(len(combos)), f"second, counted {counted}")
        assert_same(torch, idx, want_idx, np.arange(len(combos)), f"index, counted {counted}")
        assert_same(torch, dist, want_dist, np.arange(len(combos)), f"distance, counted {counted}")


# ── a cloud with more rows than max_src_n ───────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("entry, rows_per_lane", [("batch", 1), ("batch", 2), ("batch", 4), ("prepared", 1)])
def test_a_longer_cloud_is_truncated_to_max_src_n(gpu, entry, rows_per_lane):
    """max_src_n bounds the rows written per pair.  A source cloud of max_src_n + 150 rows — rows the grid covers —
    with out_stride == max_src_n: rows n < max_src_n of its pair hold the right answers and nothing at or beyond
    max_src_n is written, which would be the NEXT pair's rows.  The next pair has a three-row source, so nearly all its
    rows must still hold the sentinel; the batch ends on an ordinary pair, so even a library without the clamp stays
    inside the buffers."""
    torch, L, batch = gpu
    dim = 2
    cs = nn_ref.cases(dim)
    max_src_n = stride = 300
    long_n = max_src_n + 150
    m = 33
    n_pairs = max(8, first_pairs_with(L, rows_per_lane, max_src_n, dim) if rows_per_lane > 1 else 0)
    n_pairs += -n_pairs % 4
    p = plan(L, n_pairs, max_src_n, dim)
    assert p.rows_per_lane == rows_per_lane and max_src_n < long_n <= p.grid_x * p.rows_per_wg
    assert long_n <= -(-max_src_n // p.threads) * p.threads          # ... and the rows the sweep's grid covers (a row per lane)
    sizes = [max_src_n, long_n, 3, 200]                               # every group of four pairs: full, too long, short, ordinary
    clouds = [cs.source(n, k) for k, n in enumerate(sizes)] + [cs.target(m)]
    answers = [tuple(a[:max_src_n] for a in cs.answer(m, n, k)) for k, n in enumerate(sizes)]
    want_idx, want_dist = expected_rows([a[:2] for a in answers], stride)
    combo_of_pair = np.arange(n_pairs) % 4
    cloud_set = batch.CloudSet.from_numpy(clouds)
    pt = np.full(n_pairs, 4)
    if entry == "batch":
        idx, dist = nn_batch(gpu, cloud_set, None, combo_of_pair, pt, max_src_n, stride)
    else:
        idx, dist, second = nn_prepared(gpu, cloud_set, None, combo_of_pair, pt, max_src_n, stride)
        assert_same(torch, second, expected_rows([(a[0], a[2]) for a in answers], stride)[1], combo_of_pair, "second")
    assert_same(torch, idx, want_idx, combo_of_pair, "index")
    assert_same(torch, dist, want_dist, combo_of_pair, "distance")


# ── the sweep on the same cases ─────────────────────────────────────────────────────────────────────────────────────
def test_sweep_equals_the_reference_on_the_same_cases(gpu):
    """batch.nn_set_sweep on the 2-D combinations whose target the sweep takes: index, distance and the second-smallest
    squared distance (+inf for a one-row target).  One launch: the sweep kernel has one body."""
    torch, L, batch = gpu
    cs = nn_ref.cases(2)
    p = plan(L, nn_ref.MANY_PAIRS, 1, 2)
    sizes = nn_ref.source_sizes(p.rows_per_wg, p.threads)
    targets = [m for m in nn_ref.TARGET_SIZES[2] if m <= nn_ref.SWEEP_MAX_ROWS]
    assert {1, 2047, 2048, 2049} <= set(targets)
    clouds = [cs.source(n, k) for k, n in enumerate(sizes)] + [cs.target(m) for m in targets]
    combos = [(si, ti) for ti in range(len(targets)) for si in range(len(sizes))]
    dist, idx, second = batch.nn_set_sweep(batch.CloudSet.from_numpy(clouds), [c[0] for c in combos],
                                           [len(sizes) + c[1] for c in combos], return_second=True)
    dist, idx, second = dist.cpu().numpy(), idx.cpu().numpy(), second.cpu().numpy()
    for b, (si, ti) in enumerate(combos):
        n, m = sizes[si], targets[ti]
        want = cs.answer(m, n, si)
        assert np.array_equal(idx[b, :n], want[0]) and np.array_equal(dist[b, :n], want[1]), (n, m)
        assert np.array_equal(second[b, :n], want[2]) and (m > 1 or np.all(np.isinf(second[b, :n]))), (n, m)
