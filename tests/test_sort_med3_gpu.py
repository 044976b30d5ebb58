"""The 32-bit register sorting network (csrc/sort.hpp) with one median per cross-lane compare-exchange, driven through its
two callers.  The voxel filter, bit for bit against tests/voxel_ref.py: both register shapes of both launch widths, row counts one below, at and one above a padded size (pad
words in every lane position of the last wave), a cloud whose lowest packed word is exactly 0 (key 0, row 0: the
minimum's select word itself), clouds whose cells x slots lie just below 4e9 (real words with bit 31 set sort unsigned and
below the pad word), and voxels of three or more members scattered over all slots of different threads, so that a wrong
exchange changes an in-order sum.  The prepare kernel's bearing order (prep_sort_polar32; normal_k = 12 is an instantiation
that takes the median): targets of 64 .. 2 047 rows, a scan and a cloud of spokes through the origin (many rows per 21-bit
key) each — the sorted copy in (key, row) order, normals and registrations bit for bit those of the projection orders.
No tolerance: np.array_equal, shapes included."""
import functools

import numpy as np
import pytest

import voxel_cases as vc
import voxel_ref as vr

pytestmark = pytest.mark.gpu

VOXEL = 0.25
# 512 threads a workgroup (a set of 257): 513 .. 1 024 rows sort two words a thread, 1 025 .. 2 048 four
SET_ROWS = (513, 1023, 1024, 1025, 2047, 2048)
# 1 024 threads (a lone cloud): the same shapes at twice the rows
LONE_ROWS = tuple(2 * n for n in SET_ROWS) + (1025, 2049, 4095)


@functools.lru_cache(maxsize=None)
def scattered(n):
    """n rows in n / 5 voxels (700 at the most) of a 32 x 24 grid, the members anywhere inside their voxel (coordinates 0.007 .. 8) and
    shuffled through the input; row 0 is the origin and the lower corner of the box: key 0, row 0, the packed word 0."""
    rng = np.random.default_rng(6000 + n)
    cells = rng.choice(32 * 24, size=min(n // 5, 700), replace=False)
    of_row = cells[rng.integers(0, len(cells), size=n)]
    key = np.stack([of_row // 24, of_row % 24], axis=1).astype(np.float64)
    pts = (key + rng.uniform(0.03, 0.97, size=(n, 2))) * VOXEL
    pts = pts[rng.permutation(n)]
    pts[0] = 0.0
    pts.setflags(write=False)
    assert vc.fits(pts, VOXEL) and vc.packed_range(pts, VOXEL) < 4.0e9
    return pts


@functools.lru_cache(maxsize=None)
def scattered_ref(n):
    ref = vr.voxel_ref(scattered(n), VOXEL)
    ref.setflags(write=False)
    return ref


def _filter_set(clouds, voxel):
    from icpmi import batch
    return batch.voxel_downsample_set(batch.CloudSet.from_numpy(clouds), voxel).to_numpy()


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), what


def test_inputs_take_the_register_paths_and_are_order_sensitive():
    for n in SET_ROWS:
        assert vc.route(scattered(n), VOXEL, 512) == f"regs E={2 if n <= 1024 else 4} T=512", n
    for n in LONE_ROWS:
        assert vc.route(scattered(n), VOXEL, 1024) == f"regs E={2 if n <= 2048 else 4} T=1024", n
    for n in SET_ROWS + LONE_ROWS:
        assert vr.order_sensitive(scattered(n), VOXEL).sum() >= 20, n


def test_set_of_257():
    clouds = [scattered(SET_ROWS[i % len(SET_ROWS)]) for i in range(vc.SET_CLOUDS)]
    assert vc.threads_of(len(clouds)) == 512
    out = _filter_set(clouds, VOXEL)
    assert len(out) == len(clouds)
    for i, o in enumerate(out):
        _same(o, scattered_ref(SET_ROWS[i % len(SET_ROWS)]), (i, SET_ROWS[i % len(SET_ROWS)]))


@pytest.mark.parametrize("n", LONE_ROWS)
def test_lone_cloud(n):
    out = _filter_set([scattered(n)], VOXEL)
    _same(out[0], scattered_ref(n), n)


# cells x slots just below 4e9: the largest keys times the slots exceed 2^31
BIT31 = [vc.clusters("below 4e9", n, dim) for n in (1024, 2048, 4096) for dim in (2, 3)]


def test_bit31_inputs():
    for name, pts, voxel in BIT31:
        assert 2.0 ** 31 < vc.packed_range(pts, voxel) < 4.0e9, name


@pytest.mark.parametrize("case", [c for c in BIT31 if len(c[1]) >= 2048], ids=lambda c: c[0])
def test_bit31_lone(case):
    name, pts, voxel = case
    assert vc.route(pts, voxel, 1024).startswith("regs")
    _same(_filter_set([pts], voxel)[0], vc.reference(case), name)


@pytest.mark.parametrize("dim", (2, 3))
def test_bit31_set_of_257(dim):
    cases = [c for c in BIT31 if c[1].shape[1] == dim and len(c[1]) <= 2048]
    assert [vc.route(c[1], c[2], 512) for c in cases] == ["regs E=2 T=512", "regs E=4 T=512"]
    members = [cases[i % 2] for i in range(vc.SET_CLOUDS)]
    out = _filter_set([c[1] for c in members], cases[0][2])
    for i, (o, c) in enumerate(zip(out, members)):
        _same(o, vc.reference(c), (i, c[0]))


# ── the prepare side: bearing order ─────────────────────────────────────────────────────────────────────────────────────
# one, two and four words a thread (512 threads), a full and a nearly full last wave; not 2 048: ADVICE.md, the pad sentinel
PREP_ROWS = (64, 65, 1024, 1025, 1536, 2047)
PREP_K = 12


@functools.lru_cache(maxsize=None)
def prep_clouds():
    """per size a scan of that many beams, then a cloud of four spokes through the origin, two of them 2e-6 rad apart"""
    from icpmi import synth
    out = []
    for n in PREP_ROWS:
        out.append(synth.scan((0.3, -0.2, 0.1), 700 + n, n_beams=n))
    for n in PREP_ROWS:
        ang = np.resize(np.array([0.3, 0.3 + 2e-6, -2.9, np.pi]), n)
        r = np.random.default_rng(800 + n).permutation(np.linspace(0.5, 6.0, n))
        out.append(np.column_stack([r * np.cos(ang), r * np.sin(ang)]))
    for c in out:
        c.setflags(write=False)
    return out


def _prepare(clouds, k):
    """icpmi_prepare_targets_ex over the set -> (offsets, normals in row order, sorted xy, sorted -> row map, bearing keys, axis per cloud)"""
    import torch
    from icpmi import _lib, batch
    cs = batch.CloudSet.from_numpy(clouds)
    L = _lib.lib()
    ws = torch.zeros(L.icpmi_prepared_bytes(cs.total_rows, cs.n_clouds, cs.max_n), dtype=torch.uint8, device=cs.pts.device)
    nrm = batch.normals_set(cs, k, workspace=ws).cpu().numpy()
    T = cs.total_rows
    raw = ws.cpu().numpy()
    return (cs.off_host, nrm, raw[:T * 16].view(np.float64).reshape(T, 2), raw[T * 32:T * 36].view(np.int32),
            raw[T * 36:T * 40].view(np.float32), raw[T * 40:T * 40 + 4 * cs.n_clouds].view(np.int32))


@pytest.mark.parametrize("knn", ["sweep", "grid"])
def test_bearing_order_sorted_copy_and_normals(libopt, knn):
    clouds = prep_clouds()
    assert [len(c) for c in clouds] == list(PREP_ROWS) * 2
    libopt.setenv("ICPMI_PREP_KNN", knn)
    libopt.setenv("ICPMI_POLAR", "0")
    want = _prepare(clouds, PREP_K)[1]                                 # the projection orders: the 64-bit network
    libopt.setenv("ICPMI_POLAR", "2")
    off, nrm, sxy, sorig, skey, dirs = _prepare(clouds, PREP_K)
    assert np.array_equal(nrm, want), knn
    many = 0
    for i, c in enumerate(clouds):
        lo, hi = int(off[i]), int(off[i + 1])
        rows, key = sorig[lo:hi], skey[lo:hi].astype(np.float64)
        assert int(dirs[i]) == 4, (i, dirs[i])
        assert np.array_equal(np.sort(rows), np.arange(len(c))) and np.array_equal(sxy[lo:hi], c[rows]), (i, "sorted copy")
        step = np.diff(key)
        assert (step >= 0).all() and (np.diff(rows)[step == 0] > 0).all(), (i, "(key, row) order")
        if i >= len(PREP_ROWS):
            many += int((step == 0).sum() >= len(c) - 8)               # a spoke cloud: at most eight distinct keys
    assert many == len(PREP_ROWS)


def test_bearing_order_registrations(libopt):
    """a nearest-neighbour pass per iteration over the bearing-ordered targets: the records of the projection orders, bit
    for bit.  The voxel size is below every point distance, so the filter keeps every row."""
    from icpmi import batch
    tgts = prep_clouds()
    srcs = [t[::2] + np.array([0.03, 0.02]) for t in tgts]
    got = {}
    for mode in ("0", "2"):
        libopt.setenv("ICPMI_POLAR", mode)
        b = batch.IcpBatch(srcs + tgts, np.arange(len(tgts)), np.arange(len(tgts), 2 * len(tgts)), 1e-10, 6, 1e-5,
                           method="point_to_line", normal_k=PREP_K)
        got[mode] = b.run().cpu().numpy().copy()
        assert np.array_equal(b.vox.cnt.cpu().numpy()[len(tgts):], [len(t) for t in tgts])
    assert np.array_equal(got["0"], got["2"])
