"""The LDS layout of the fused ICP kernel (csrc/icp2.hip, Icp2Lds) at the target sizes where it can go wrong: the steps of
the LDS capacity (64, 65, 1024, 1025), the 1 536-point special case (1536, 1537), the limit of the float32 filter (2048,
2049), the limit of the LDS copy (4096, 4097), and every M == capacity, where the padding image behind the last point is
the last thing in its area.  The fast path must give what the exhaustive kernel gives; the far continuation (tree and
slots behind the images) must give what the plain path gives, byte for byte."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOXEL = 0.04
SIZES = [64, 65, 1024, 1025, 1536, 1537, 2048, 2049, 4096, 4097]
SEG = 32            # points of a wall segment


def _walls(n, seed):
    """n points on wall segments of 32 points 0.05 m apart (jitter 4 mm: neighbours stay more than one voxel apart, so the
    voxel filter keeps every point), alternately horizontal (x < 7) and vertical (x >= 8), walls 0.5 m apart: already 64
    points constrain both directions."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    seg, along = i // SEG, (i % SEG) * 0.05
    k = seg // 2                                            # k-th segment of its orientation: four to a wall
    u, v = along + 1.7 * (k % 4), 0.5 * (k // 4)
    horizontal = seg % 2 == 0
    pts = np.where(horizontal[:, None], np.stack([u, v], 1), np.stack([8.0 + v, u], 1))
    return pts + rng.uniform(-0.004, 0.004, size=(n, 2))


def _moved(pts, deg, shift):
    th = np.deg2rad(deg)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return pts @ R.T + np.asarray(shift)


N_SRC = 2 * SEG * 5


@pytest.fixture(scope="module")
def source():
    """320 rows: five copies 0.05 m apart of the first horizontal and the first vertical segment — close to every target
    here, the smallest included, so the errors stay small against the 1e-14 they are compared at — slightly moved."""
    base = _walls(2 * SEG, 77)
    band = [base + np.where(np.arange(2 * SEG)[:, None] < SEG, [0.0, 0.02 + 0.05 * k], [0.02 + 0.05 * k, 0.0]) for k in range(5)]
    return _moved(np.vstack(band), 0.3, (0.03, -0.02))


def _batch(source, target, method, **kw):
    from icpmi import batch
    extra = dict(normal_k=12) if method == "point_to_line" else {}
    return batch.IcpBatch([source, target], [0], [1], 1e-10, 20, VOXEL, method=method, **extra, **kw)


@pytest.mark.parametrize("method", ["point_to_line", "point_to_point"])
@pytest.mark.parametrize("m", SIZES)
def test_fast_path_equals_exhaustive_path_at_the_layout_edges(source, m, method):
    target = _walls(m, 1000 + m)
    fast, slow = _batch(source, target, method), _batch(source, target, method, force_exhaustive=True)
    assert fast.fast and not slow.fast
    fast.run(); slow.run()
    assert fast.vox.cnt.cpu().numpy().tolist() == [N_SRC, m]              # the filtered row counts are exact
    Rf, tf, ef, inf_ = fast.unpack()
    Rs, ts, es, ins = slow.unpack()
    assert np.array_equal(inf_["iters"], ins["iters"]) and np.array_equal(inf_["status"], ins["status"])
    diffs = (np.abs(Rf - Rs).max(), np.abs(tf - ts).max(), np.abs(ef - es).max())
    assert diffs[0] < 1e-12 and diffs[1] < 1e-12 and diffs[2] < 1e-14, diffs


def _far_count(b):
    """How many pairs the last launch handed to the far continuation: the third counter of the ICP workspace
    (csrc/icp2.hip, Icp2Ws: parked rows 16 B + positions 4 B per source row | three lists of B | three counters)."""
    off = b.B * b.max_src_n * 20 + 3 * b.B * 4 + 2 * 4
    return int(b.icp_ws[off:off + 4].view(torch.int32).item())


@pytest.mark.parametrize("m", [64, 2048])
def test_far_continuation_at_the_extremes_of_its_layout(source, libopt, m):
    """A source started 3 m off, finished by the far continuation, whose box hierarchy and slots lie behind the images:
    the smallest capacity and the largest.  The walls of the 2 048-row target are 0.5 m apart, so 3 m off is still beside
    a wall and the default threshold (1 m^2 after the first step) does not send that pair: the threshold 1e-12 does,
    and the workspace's counter shows that it did.  Same records as the plain path (option ICP2_FAR = 0), byte for byte."""
    target = _walls(m, 1000 + m)
    far_source = _moved(source, 2.0, (2.4, 1.8))
    out, sent = {}, {}
    for far in ("0", None, "1e-12"):
        libopt.setenv("ICP2_FAR", far) if far else libopt.delenv("ICP2_FAR")
        b = _batch(far_source, target, "point_to_line")
        b.icp_ws.zero_()                                                 # a launch that parks nobody leaves the counters alone
        out[far] = b.run().cpu().numpy().copy()
        sent[far] = _far_count(b)
        assert b.vox.cnt.cpu().numpy().tolist() == [N_SRC, m]
    assert sent["0"] == 0 and sent["1e-12"] == 1, sent
    assert out["0"][0, 14] > 2                                           # iterations are left for the continuation
    assert out["0"].tobytes() == out[None].tobytes() and out["0"].tobytes() == out["1e-12"].tobytes()
