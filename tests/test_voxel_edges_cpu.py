"""The NumPy restatement of the voxel filter (tests/voxel_ref.py) and the inputs of its edge suite (tests/voxel_cases.py),
without a GPU: the restatement equals the C oracle bit for bit and its keys equal the keys of exact arithmetic on every
input; every input has the property tests/test_voxel_edges_gpu.py relies on — long runs whose sums depend on the order,
points whose key depends on the rounding of the divide, the code path named by the restated routing rules — so a GPU test
cannot pass because an input silently lost its point; and every wrong model of the filter differs from the right one on the
family meant to catch it.  Every floor below is a condition on the inputs, asserted against the restatement alone."""
import numpy as np
import pytest

import oracle
import voxel_cases as vc
import voxel_ref as vr

ORDER_FAMILIES = ("one_voxel", "runs", "clusters")


def _describe(case):
    """route alone / in a 257-cloud set, voxels, longest run, order-sensitive voxels, reciprocal-sensitive points: printed"""
    name, pts, voxel = case
    _, counts = vr.voxel_ref(pts, voxel, return_counts=True)
    d = dict(routes=vc.routes(pts, voxel), voxels=len(counts), longest=int(counts.max()), counts=counts,
             sensitive=vr.order_sensitive(pts, voxel), reciprocal=int(vr.reciprocal_sensitive(pts, voxel).sum()))
    print(f"{name}: n {len(pts)} route {d['routes'][0]} | {d['routes'][1]}, {d['voxels']} voxels, longest run {d['longest']}, "
          f"{int(d['sensitive'].sum())} order-sensitive voxels, {d['reciprocal']} reciprocal-sensitive points")
    return d


def _ids(cases):
    return [c[0] for c in cases]


# ── the reference, stated twice, and the oracle ─────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", vc.all_cases(), ids=_ids(vc.all_cases()))
def test_restatement_equals_the_oracle_and_exact_arithmetic(case):
    name, pts, voxel = case
    means, keys = vr.voxel_ref(pts, voxel, return_keys=True)
    want = oracle.voxel_downsample(pts, voxel)
    assert means.shape == want.shape and np.array_equal(means, want), name
    assert np.array_equal(keys, vr.exact_keys(pts, voxel)), name
    assert np.array_equal(means, vc.reference(case))


def test_exact_keys_by_hand():
    """0.3 / 0.1 rounds to 2.9999999999999996 and (0.1 + 0.2) / 0.1 to 3.0000000000000004 in float64"""
    pts = np.array([[0.0, 0.0], [0.3, 0.1 + 0.2], [0.25, 0.75]])
    assert vr.exact_keys(pts, 0.1).tolist() == [[0, 0], [2, 3], [2, 7]]
    assert vr.exact_keys(pts, 0.25).tolist() == [[0, 0], [1, 1], [1, 3]]
    assert vr.voxel_ref(pts, 0.1, return_keys=True)[1].tolist() == [[0, 0], [2, 3], [2, 7]]


def test_restatement_by_hand():
    pts = np.array([[1.0, 5.0], [0.0, 4.0], [1.25, 5.5], [0.5, 4.25], [1.75, 5.75]])          # dyadic: every sum is exact
    means, keys, counts = vr.voxel_ref(pts, 1.0, return_keys=True, return_counts=True)
    assert keys.tolist() == [[1, 1], [0, 0], [1, 1], [0, 0], [1, 1]] and counts.tolist() == [2, 3]
    assert means.tolist() == [[0.25, 4.125], [4.0 / 3.0, 16.25 / 3.0]]


# ── the routing rules ───────────────────────────────────────────────────────────────────────────────────────────────────
def test_routing_rules_by_hand():
    assert [vc.npad_of(n) for n in (1, 64, 65, 1024, 1025, 8192)] == [64, 64, 128, 1024, 2048, 8192]
    assert [vc.threads_of(c) for c in (1, 256, 257)] == [1024, 1024, 512]
    box = lambda n, e: np.array([[0.0, 0.0]] * (n - 1) + [[(e[0] - 1) * 0.5, (e[1] - 1) * 0.5]])
    assert vc.route(box(2048, (1397, 1398)), 0.5, 1024) == "regs E=2 T=1024"           # 3.99976e9
    assert vc.route(box(2048, (1397, 1398)), 0.5, 512) == "regs E=4 T=512"
    assert vc.route(box(2048, (1398, 1398)), 0.5, 1024) == "lds 64-bit"                # 4.00262e9
    assert vc.route(box(2048, (125, 15625)), 0.5, 1024) == "lds 64-bit"                # exactly 4e9: the comparison is strict
    assert vc.packed_range(box(2048, (125, 15625)), 0.5) == 4.0e9
    assert vc.route(box(2048, (66291000, 66291000)), 0.5, 512) == "lds 64-bit"         # 8.99993e18
    assert vc.route(box(2048, (66292000, 66292000)), 0.5, 512) == "lds pairs"          # 9.0002e18
    assert vc.route(box(1024, (10, 10)), 0.5, 1024) == "lds 32-bit" and vc.route(box(1024, (10, 10)), 0.5, 512) == "regs E=2 T=512"
    assert vc.route(box(4096, (10, 10)), 0.5, 1024) == "regs E=4 T=1024" and vc.route(box(4096, (10, 10)), 0.5, 512) == "lds 32-bit"
    assert vc.route(box(8192, (10, 10)), 0.5, 1024) == "lds 32-bit" and vc.route(box(8193, (10, 10)), 0.5, 1024) == "large"
    assert vc.route(box(64, (3.2e9, 3.2e9)), 0.5, 1024) == vc.REFUSED


# ── one voxel ───────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", vc.one_voxel_cases(), ids=_ids(vc.one_voxel_cases()))
def test_one_voxel_cases(case):
    name, pts, voxel = case
    d = _describe(case)
    assert d["voxels"] == 1 and d["longest"] == len(pts), name
    assert d["sensitive"].all(), name                               # the one mean changes bits under reversed order
    n = len(pts)
    want = ("large", None) if n > 8192 else ("lds 32-bit", "regs E=2 T=512") if n <= 1024 else \
        ("regs E=2 T=1024", "regs E=4 T=512") if n <= 2048 else \
        ("regs E=4 T=1024", "lds 32-bit") if n <= 4096 else ("lds 32-bit", "lds 32-bit")
    assert d["routes"] == want, name


def test_one_voxel_sizes():
    """the sizes the suite was asked for, and 1 024 rows: the full register shape of the 512-thread launch"""
    assert {(len(c[1]), c[1].shape[1]) for c in vc.one_voxel_cases()} == \
        {(n, 2) for n in (1024, 1025, 2047, 2048, 4095, 4096, 8192, 8193, 20000)} | {(n, 3) for n in (2048, 4096, 8193)}


# ── runs ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", vc.run_cases(), ids=_ids(vc.run_cases()))
def test_run_cases(case):
    name, pts, voxel = case
    n = len(pts)
    d = _describe(case)
    counts = d["counts"]
    assert counts.tolist() == vc.run_lengths_in_key_order(n), name               # the voxels are the ones built, in key order
    assert set(range(1, 10)) <= set(counts.tolist()) and ((counts >= 40) & (counts <= 70)).sum() >= 1, name
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ends = np.cumsum(counts) - 1
    assert set((starts % 4).tolist()) == {0, 1, 2, 3} and set((ends % 4).tolist()) == {0, 1, 2, 3}, name
    long_enough = counts >= 3
    assert long_enough.sum() >= 100, (name, int(long_enough.sum()))
    assert (d["sensitive"] & long_enough).sum() * 2 >= long_enough.sum(), (name, int((d["sensitive"] & long_enough).sum()))
    # key order is not input order: the first members of the voxels do not come in ascending row order
    _, keys = vr.voxel_ref(pts, voxel, return_keys=True)
    _, first_row = np.unique(keys, axis=0, return_index=True)
    assert (np.diff(first_row) < 0).sum() >= len(first_row) // 4, name
    # ... and the members of a voxel are scattered: those of the longest run span most of the input
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    rows = np.flatnonzero(np.asarray(inverse).reshape(-1) == int(np.argmax(counts)))
    assert rows.max() - rows.min() >= n // 2, name
    npad = vc.npad_of(n)
    want = ("lds 32-bit", "regs E=2 T=512") if npad == 1024 else ("regs E=2 T=1024", "regs E=4 T=512") if npad == 2048 else \
        ("regs E=4 T=1024", "lds 32-bit") if npad == 4096 else ("lds 32-bit", "lds 32-bit")
    assert d["routes"] == want, name


def test_run_sizes():
    assert {(len(c[1]), c[1].shape[1]) for c in vc.run_cases()} == \
        {(n, dim) for n in (513, 1024, 1025, 2048, 2049, 4096, 4097, 8192) for dim in (2, 3)}


# ── clusters ────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_cluster_extents_are_the_issue_table_at_2048_rows():
    assert vc.cluster_extents("below 4e9", 2048, 2) == (1398, 1397)
    assert vc.cluster_extents("above 4e9", 2048, 2) == (1398, 1398)
    assert vc.cluster_extents("exactly 4e9", 2048, 2) == (125, 15625)
    for side, lo, hi in (("below 9e18", 8.9999e18, 9.0e18), ("above 9e18", 9.0e18, 9.0001e18)):
        for n in vc.CLUSTER_ROWS:
            for dim in (2, 3):
                prod = float(np.prod(vc.cluster_extents(side, n, dim), dtype=np.float64)) * vc.npad_of(n)
                assert lo <= prod < hi, (side, n, dim, prod)         # (exactly 9e18 is "not below": above)
    assert vc.cluster_extents("exactly 4e9", 4096, 2) is None        # 4e9 / 4 096 is no whole number
    assert len(vc.cluster_cases()) == 2 * (3 * 5 - 1)


@pytest.mark.parametrize("case", vc.cluster_cases(), ids=_ids(vc.cluster_cases()))
def test_cluster_cases(case):
    name, pts, voxel = case
    n, dim = pts.shape
    side = next(s for s in vc.CLUSTER_SIDES if name.endswith(s.replace(" ", "_")))
    d = _describe(case)
    counts = d["counts"]
    means, keys = vr.voxel_ref(pts, voxel, return_keys=True)
    ext = vc.extents(pts, voxel)
    rng = vc.packed_range(pts, voxel)
    print(f"    extents {ext.astype(np.int64).tolist()} packed range {rng:.6g}")
    assert ext.tolist() == [float(e) for e in vc.cluster_extents(side, n, dim)], name
    lo, hi = {"below 4e9": (3.9e9, 4.0e9), "above 4e9": (4.0e9, 4.1e9), "exactly 4e9": (4.0e9, 4.0e9),
              "below 9e18": (8.9999e18, 9.0e18), "above 9e18": (9.0e18, 9.0001e18)}[side]
    assert (rng == lo) if lo == hi else (lo <= rng < hi), (name, rng)
    # a cluster in the voxel of key 0; one in the voxel with the largest key, which holds the last row
    assert (keys == 0).all(axis=1).sum() == counts[0] >= 3, name
    assert (keys == ext - 1).all(axis=1).sum() == counts[-1] >= 3 and (keys[n - 1] == ext - 1).all(), name
    assert (counts >= 3).sum() >= 80 and counts.max() >= 30, (name, int((counts >= 3).sum()), int(counts.max()))
    assert d["sensitive"].sum() >= 50, (name, int(d["sensitive"].sum()))
    form = vc.CLUSTER_FORM[side]
    shape = {1024: (None, "regs E=2 T=512"), 2048: ("regs E=2 T=1024", "regs E=4 T=512"), 4096: ("regs E=4 T=1024", None)}[n]
    want = tuple(s if s is not None and form == "32-bit" else "lds " + form for s in shape)
    assert d["routes"] == want, (name, d["routes"], want)


# ── division lattices ───────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("case", vc.lattice_cases(), ids=_ids(vc.lattice_cases()))
def test_lattice_cases(case):
    name, pts, voxel = case
    d = _describe(case)
    n = len(pts)
    if "_far_" in name:
        form = "64-bit" if "_far_64-bit" in name else "pairs"
        assert d["routes"] == ("lds " + form, "lds " + form), name
    else:
        npad = vc.npad_of(n)
        want = ("large", None) if n > 8192 else ("lds 32-bit", "regs E=2 T=512") if npad == 1024 else \
            ("regs E=2 T=1024", "regs E=4 T=512") if npad == 2048 else ("regs E=4 T=1024", "lds 32-bit") if npad == 4096 else \
            ("lds 32-bit", "lds 32-bit")
        assert d["routes"] == want, name
    on_lattice = not name.endswith(("_ulp_down", "_ulp_up"))         # (the floor is stated for the lattice itself)
    if on_lattice and voxel in vc.RECIPROCAL_V and any(f"_off{off:.7g}_" in name for off in vc.RECIPROCAL_OFF):
        assert d["reciprocal"] >= 20, (name, d["reciprocal"])
    if n > vc.LATTICE_K and "_far_" not in name:                     # a tiled lattice: the voxels of the lattice, more members each
        base = vc.lattice(voxel, next(off for off in vc.LATTICE_OFF if f"_off{off:.7g}_" in name))
        assert np.array_equal(vr.voxel_ref(base[1], voxel, return_keys=True)[1], vr.voxel_ref(pts, voxel, return_keys=True)[1][:400])


def test_lattice_points_are_the_ones_asked_for():
    assert len(vc.lattice_cases()) == 5 * 3 * 3 + 5 * 3 * len(vc.LATTICE_TILED) + 2 * 2 * 2
    for v in vc.LATTICE_V:
        for off in vc.LATTICE_OFF:
            on, down, up = (vc.lattice(v, off, s)[1] for s in vc.LATTICE_SHIFTS)
            k = np.arange(400.0)
            assert np.array_equal(on[:, 0], off + k * v) and np.array_equal(on[:, 1], (off + k * v)[::-1])
            assert (down < on).all() and (np.nextafter(down, np.inf) == on).all()
            assert (up > on).all() and (np.nextafter(up, -np.inf) == on).all()


# ── refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_refusal_cases():
    cases = vc.refusal_cases()
    assert sorted(len(c[1]) for c in cases) == [64, 64, 2048, 2048, 8193, 8193]
    for name, pts, voxel in cases:
        ext = vc.extents(pts, voxel)
        print(f"{name}: extents {ext.tolist()}")
        assert vc.routes(pts, voxel)[0] == vc.REFUSED, name
        assert (ext >= 3.2e9).all(), name
    name, pts, voxel = vc.refusal("apart", 64)
    assert vc.extents(pts, voxel).tolist() == [3.2e9 + 1.0] * 2
    assert np.isinf(vc.extents(vc.refusal("tiny_voxel", 64)[1], 1e-300)).all()
    # what the refusal tests put next to a refused cloud at a voxel of 1e-300 is not refused
    assert vc.route(np.full((70, 2), 0.3), 1e-300, 1024) == "lds 32-bit"


# ── every path is reached ───────────────────────────────────────────────────────────────────────────────────────────────
def test_every_path_meets_long_runs_and_a_lattice():
    """Every route of voxel.hip is taken by a case whose sums depend on the order (three or more members, different bits
    when reversed) and by a division lattice with reciprocal-sensitive points."""
    by_runs, by_lattice = {r: [] for r in vc.ROUTES}, {r: [] for r in vc.ROUTES}
    for fam in ORDER_FAMILIES:
        for case in vc.FAMILIES[fam]():
            _, counts = vr.voxel_ref(case[1], case[2], return_counts=True)
            if ((counts >= 3) & vr.order_sensitive(case[1], case[2])).any():
                for r in vc.routes(case[1], case[2]):
                    if r is not None:
                        by_runs[r].append(case[0])
    for case in vc.lattice_cases():
        if vr.reciprocal_sensitive(case[1], case[2]).sum() >= 20:
            for r in vc.routes(case[1], case[2]):
                if r is not None:
                    by_lattice[r].append(case[0])
    for r in vc.ROUTES:
        print(f"{r}: {len(by_runs[r])} cases with order-sensitive runs (e.g. {by_runs[r][:2]}), "
              f"{len(by_lattice[r])} lattices (e.g. {by_lattice[r][:2]})")
        assert by_runs[r] and by_lattice[r], r


# ── the wrong models ────────────────────────────────────────────────────────────────────────────────────────────────────
def _differs(case, **model):
    got = vr.voxel_ref(case[1], case[2], **model)
    ref = vc.reference(case)
    return got.shape != ref.shape or not np.array_equal(got, ref)


@pytest.mark.parametrize("model", ["reciprocal", "float32"])
def test_wrong_keys_are_caught_by_the_lattices(model):
    caught = [c[0] for c in vc.lattice_cases() if _differs(c, key_model=model)]
    print(f"{model} keys: {len(caught)} of {len(vc.lattice_cases())} lattices differ")
    assert caught
    if model == "reciprocal":                                        # every lattice with the floor of 20 such points
        for c in vc.lattice_cases():
            if vr.reciprocal_sensitive(c[1], c[2]).sum() >= 20:
                assert c[0] in caught, c[0]


@pytest.mark.parametrize("order", ["reversed", "by_value"])
@pytest.mark.parametrize("family", ORDER_FAMILIES)
def test_wrong_orders_are_caught(family, order):
    cases = vc.FAMILIES[family]()
    caught = [c[0] for c in cases if _differs(c, order=order)]
    print(f"{order} sums: {len(caught)} of {len(cases)} {family} cases differ")
    assert len(caught) == len(cases), sorted(set(c[0] for c in cases) - set(caught))


# ── CloudSet.to_numpy() on a refused cloud ──────────────────────────────────────────────────────────────────────────────
def test_to_numpy_raises_on_a_negative_count():
    """A hand-made CloudSet on CPU tensors (the class only stores them): a count of -1 is the filter's "key range does not
    fit", and reading the set back says so instead of slicing host[off : off - 1] into an empty cloud."""
    import torch
    from icpmi import batch
    pts = torch.arange(12, dtype=torch.float64).reshape(6, 2)
    good = batch.CloudSet(pts, [0, 2, 6], cnt=torch.tensor([1, 3], dtype=torch.int32))
    out = good.to_numpy()
    assert [o.tolist() for o in out] == [[[0.0, 1.0]], [[4.0, 5.0], [6.0, 7.0], [8.0, 9.0]]]
    assert [o.shape for o in batch.CloudSet(pts, [0, 2, 6]).to_numpy()] == [(2, 2), (4, 2)]
    bad = batch.CloudSet(pts, [0, 2, 6], cnt=torch.tensor([1, -1], dtype=torch.int32))
    with pytest.raises(OverflowError, match="voxel key range does not fit in 64 bits") as e:
        bad.to_numpy()
    assert str(e.value) == batch.VOXEL_KEY_RANGE_ERROR
    assert bad.counts_host().tolist() == [1, -1]                    # the counts themselves stay readable
    assert batch.filtered_rows(bad, 0) == 1
    with pytest.raises(OverflowError, match="voxel key range does not fit in 64 bits"):
        batch.filtered_rows(bad, 1)
