"""The particle filter's global start and recovery on the device (csrc/particles.hip: icpmi_pf_free_index,
icpmi_pf_draw_uniform; icpmi.particles: FreeCells, init_uniform, resample(inject=), Recovery) against the NumPy restatement
of the contract (tests/particles_global_ref.py, itself held to literal values by tests/test_particles_global_cpu.py).  Bit
for bit, given the DEVICE's own inputs, so a difference names its stage: the index from the device's planes, the draw from
the device's index, the injection from the device's weights and state; cos and sin of a drawn heading to the 4 ulp
tests/test_particles_gpu.py grants the device library's sincos."""
import numpy as np
import pytest

import gridbeam_ref as bref
import gridmatch_ref as gref
import particles_global_ref as gl
import particles_ref as ref
import stream_cases_particles_global  # noqa: F401  (registers the stream workload: tests/test_streams_cpu.py, tests/test_streams_gpu.py)
from test_particles_global_cpu import KIDNAP, N, THRESHOLD, box_about, errors, hand_made_fields
from test_particles_gpu import SINCOS_ULPS, as_u32, call, on_device, state_of, stream

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


# ── the index ────────────────────────────────────────────────────────────────
def device_planes(field, threshold):
    """The device's planes of an int16 field -> (OccupancyPlanes, occupied, unknown as uint32 (ny, wpr) on the host)."""
    from icpmi import gridmatch
    planes = gridmatch.occupancy_planes(on_device(np.ascontiguousarray(field, dtype=np.int16)), threshold)
    return (planes,) + host_planes(planes)


def host_planes(planes):
    ny, wpr = planes.ny, (planes.nx + 31) // 32
    raw = planes.buf.cpu().numpy()
    unk_at = (4 * ny * wpr + 255) // 256 * 256
    return tuple(raw[at:at + 4 * ny * wpr].view(np.uint32).reshape(ny, wpr).copy() for at in (0, unk_at))


def device_index(planes, box):
    """icpmi_pf_free_index into a buffer full of a sentinel -> (header, free, rank, the whole buffer) on the host."""
    import icpmi
    import torch
    L = icpmi.lib()
    need = L.icpmi_pf_free_index_bytes(planes.ny, planes.nx)
    assert need == gl.index_bytes(planes.ny, planes.nx)
    buf = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    x0, y0, x1, y1 = (0, 0, planes.nx, planes.ny) if box is None else box
    call(L.icpmi_pf_free_index(planes.buf.data_ptr(), planes.ny, planes.nx, x0, y0, x1, y1, buf.data_ptr(), need, stream()), "free_index")
    return split_index(buf.cpu().numpy(), planes.ny, planes.nx) + (buf,)


def split_index(raw, ny, nx):
    words = ny * ((nx + 31) // 32)
    a = lambda v: (v + 255) // 256 * 256                       # noqa: E731
    part = lambda at, count: raw[at:at + 4 * count].view(np.uint32).copy()      # noqa: E731
    return part(0, gl.FREE_HEADER), part(a(4 * gl.FREE_HEADER), words), part(a(4 * gl.FREE_HEADER) + a(4 * words), words)


def check_index(planes, occ, unk, box, what):
    want = gl.free_index(occ, unk, planes.nx, box)
    got = device_index(planes, box)
    for name, a, b in zip(("header", "free", "rank"), got, want):
        assert np.array_equal(a, b), (what, name, np.flatnonzero(a != b)[:5].tolist())
    again = device_index(planes, box)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])), what                     # twice in a row: the same bits
    return got


@pytest.mark.parametrize("name", list(hand_made_fields()))
def test_the_index_of_the_hand_made_fields(gpu, name):
    field, box, F, free, rank = hand_made_fields()[name]
    planes, occ, unk = device_planes(field, THRESHOLD)
    want_occ, want_unk = gl.planes_of(field, THRESHOLD)
    assert np.array_equal(occ, want_occ) and np.array_equal(unk, want_unk)
    header, got_free, got_rank, _ = check_index(planes, occ, unk, box, name)
    assert int(header[0]) == F and got_free.tolist() == free and got_rank.tolist() == rank         # the literal values themselves


@pytest.fixture(scope="module")
def room(gpu):
    """(the scene's grid at 0.1 m built by update_scan from the twelve scans of the synthetic room, the restated field and its
    threshold, the twelve scans thinned to 64 rows, the true poses) — tests/test_particles_gpu.py's"""
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    truth = np.array(gref.SCENE_POSES)
    for k, p in enumerate(gref.SCENE_POSES):
        grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 50 + k), p))
    k_bits = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    scans = [synth.scan(p, 50 + k)[::32] for k, p in enumerate(gref.SCENE_POSES)]
    return grid, gref.quantise(grid.log_odds, k_bits), int(np.rint(0.5 * 2.0 ** k_bits)), scans, truth


def test_the_index_of_the_room_map_whole_and_boxed(room):
    grid, field, threshold, _, truth = room
    planes, _ = grid.occupancy_planes()
    occ, unk = host_planes(planes)
    want_occ, want_unk = gl.planes_of(field, threshold)
    assert (planes.ny, planes.nx) == (200, 280) and np.array_equal(occ, want_occ) and np.array_equal(unk, want_unk)
    for box in (None, gl.box_cells(box_about(truth[0], 1.0), grid.min_x, grid.min_y, grid.resolution),
                gl.box_cells(KIDNAP["box"], grid.min_x, grid.min_y, grid.resolution), (33, 7, 95, 8), (279, 199, 280, 200), (-10, 150, 5000, 5000)):
        header = check_index(planes, occ, unk, box, box)[0]
        print(f"the room map, box {box}: {int(header[0])} free cells")
    assert int(check_index(planes, occ, unk, None, "whole")[0][0]) > 10000


def test_the_index_of_a_grid_of_more_than_one_scan_block(gpu):
    """300 x 4 000 cells: 125 words a row, 37 500 words, ten scan blocks of 4 096, the last one short."""
    rng = np.random.default_rng(20)
    field = rng.choice(np.array([0, -100, 3000, 2047, 2048], dtype=np.int16), size=(300, 4000), p=[0.3, 0.4, 0.2, 0.05, 0.05])
    field[100:103] = 0                                             # whole rows, more than a row of words, without a free cell
    field[200:240, 1000:3000] = -5                                 # and a block of nothing but free cells
    planes, occ, unk = device_planes(field, 2048)
    assert occ.size == 37500 > 9 * gl.FREE_BLOCK
    for box in (None, (37, 11, 3901, 288), (0, 0, 4000, 1), (3999, 0, 4000, 300)):
        header, free, rank, _ = check_index(planes, occ, unk, box, box)
        assert int(header[0]) == int(rank[-1]) + bin(int(free[-1])).count("1")
    assert int(header[0]) > 100                                    # (the last column has free cells: the box is not empty)


# ── the draw ─────────────────────────────────────────────────────────────────
def device_draw(index_buf, n, m, frame, theta0, span, seed, step, with_ancestors=True):
    """icpmi_pf_draw_uniform into buffers full of a sentinel -> (pair_t, theta, cos_sin, ancestors or None, info) on the host."""
    import icpmi
    import torch
    f64 = lambda *shape: torch.full(shape, float(SENTINEL), dtype=torch.float64, device="cuda")      # noqa: E731
    pair_t, theta, cos_sin = f64(n, 2), f64(n), f64(n, 2)
    anc = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") if with_ancestors else None
    info = torch.full((ref.INFO_INTS,), SENTINEL, dtype=torch.int32, device="cuda")
    call(icpmi.lib().icpmi_pf_draw_uniform(n, m, index_buf.data_ptr(), *frame, theta0, span, pair_t.data_ptr(), theta.data_ptr(), cos_sin.data_ptr(),
                                           anc.data_ptr() if with_ancestors else None, info.data_ptr(), seed, step, stream()), "draw_uniform")
    return pair_t.cpu().numpy(), theta.cpu().numpy(), cos_sin.cpu().numpy(), anc.cpu().numpy() if with_ancestors else None, info.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 1000, 4097])
def test_the_draw_is_the_restated_one_bit_for_bit(room, n):
    grid, _, _, _, _ = room
    planes, _ = grid.occupancy_planes()
    header, free, rank, buf = device_index(planes, None)
    F = int(header[0])
    frame, worst = (grid.min_x, grid.min_y, grid.resolution), 0.0
    for k, m in enumerate(sorted({0, 1, n - 1, n})):
        seed, step, theta0, span = (0x0123456789ABCDEF, 2 ** 32 - 1, 0.25, 2.0) if k % 2 else (7 + n, k, -3.0, gl.TWO_PI)
        pair_t, theta, cos_sin, anc, info = device_draw(buf, n, m, frame, theta0, span, seed, step, with_ancestors=k != 1)
        drawn, want_t, want_theta, _ = gl.draw_uniform((header, free, rank), n, m, *frame, theta0, span, seed, step)
        assert info.tolist() == [ref.ST_OK, F, 0, 0] and drawn.sum() == m, (n, m)
        assert np.array_equal(pair_t[drawn].view(np.uint64), want_t.view(np.uint64)) and np.array_equal(theta[drawn].view(np.uint64), want_theta.view(np.uint64)), (n, m)
        assert (pair_t[~drawn] == SENTINEL).all() and (theta[~drawn] == SENTINEL).all() and (cos_sin[~drawn] == SENTINEL).all(), (n, m)
        if anc is not None:
            assert np.array_equal(anc, np.where(drawn, gl.INJECTED, SENTINEL)), (n, m)
        if m:
            worst = max(worst, float(ref.ulps(cos_sin[drawn], ref.cos_sin_ld(theta[drawn])).max()))
    print(f"n = {n}: largest error of the device's cos / sin: {worst:.3f} ulp")
    assert worst <= SINCOS_ULPS


def test_a_draw_without_a_free_cell_writes_its_status_and_nothing_else(gpu):
    field = hand_made_fields()["nothing known"][0]
    planes, occ, unk = device_planes(field, THRESHOLD)
    header, _, _, buf = device_index(planes, None)
    assert int(header[0]) == 0
    for n, m in ((1, 1), (1000, 1000), (1000, 250)):
        pair_t, theta, cos_sin, anc, info = device_draw(buf, n, m, (0.0, 0.0, 0.1), 0.0, 1.0, 3, 4)
        assert info.tolist() == [gl.ST_NO_FREE, 0, 0, 0]
        assert (pair_t == SENTINEL).all() and (theta == SENTINEL).all() and (cos_sin == SENTINEL).all() and (anc == SENTINEL).all()
    # an index of zero bytes — what the stream tests' poison leaves — is the same: no free cell, nothing written
    buf.zero_()
    assert device_draw(buf, 300, 300, (0.0, 0.0, 0.1), 0.0, 1.0, 3, 4)[4].tolist() == [gl.ST_NO_FREE, 0, 0, 0]


# ── the Python layer ─────────────────────────────────────────────────────────
def host_index(free_cells):
    """(header, free, rank) of a ``FreeCells``' buffer, by the layout as the restatement states it."""
    return split_index(free_cells.index.cpu().numpy(), free_cells.planes.ny, free_cells.planes.nx)


def test_init_uniform_is_the_restated_draw_of_every_slot(room):
    from icpmi import particles
    grid, field, threshold, _, truth = room
    pf = grid.particle_filter(N, seed=0xC0FFEE)
    box, span = box_about(truth[0], 1.0), np.deg2rad(60.0)
    free = pf.free_cells(box)
    assert isinstance(free, particles.FreeCells) and pf.free_cells(box) is free and pf.free_cells() is not free
    want_index = gl.free_index(*gl.planes_of(field, threshold), 280, gl.box_cells(box, grid.min_x, grid.min_y, grid.resolution))
    assert all(np.array_equal(a, b) for a, b in zip(host_index(free), want_index)) and free.count() == int(want_index[0][0]) == 400
    pf.w.fill_(5)
    assert pf.init_uniform(box, heading=truth[0, 2], span=span) is pf and pf.step == 1 and (pf.weights() == 1).all()
    drawn, want_t, want_theta, _ = gl.draw_uniform(want_index, N, N, grid.min_x, grid.min_y, grid.resolution, truth[0, 2], span, 0xC0FFEE, 0)
    pair_t, theta, cos_sin = state_of(pf)
    assert np.array_equal(pair_t.view(np.uint64), want_t.view(np.uint64)) and np.array_equal(theta.view(np.uint64), want_theta.view(np.uint64))
    assert float(ref.ulps(cos_sin, ref.cos_sin_ld(theta)).max()) <= SINCOS_ULPS and pf.draw_info.cpu().numpy().tolist() == [0, 400, 0, 0]
    # the whole map, the full circle, heading None: about 0, at the next step
    pf.init_uniform()
    whole = gl.free_index(*gl.planes_of(field, threshold), 280)
    _, want_t, want_theta, _ = gl.draw_uniform(whole, N, N, grid.min_x, grid.min_y, grid.resolution, 0.0, gl.TWO_PI, 0xC0FFEE, 1)
    assert pf.step == 2 and np.array_equal(state_of(pf)[0], want_t) and np.array_equal(state_of(pf)[1], want_theta)
    # a region without a free cell: refused after the status has been read — the particles are where they were, the step has
    # advanced (enqueue_uniform's rule, stated once); every other refusal comes before anything is enqueued
    before = pf.poses()
    assert pf.last_rows is None and pf.last_injected == 0         # nothing weighed yet
    for bad in (lambda: pf.init_uniform((100.0, 100.0, 101.0, 101.0)), lambda: pf.init_uniform((0.0, 0.0, np.nan, 1.0)), lambda: pf.init_uniform(span=7.0),
                lambda: pf.init_uniform(heading=np.inf), lambda: pf.resample(inject=N + 1), lambda: pf.resample(inject=-1), lambda: pf.resample(inject=1.5)):
        with pytest.raises(ValueError):
            bad()
    assert pf.step == 3 and np.array_equal(pf.poses().view(np.uint64), before.view(np.uint64)) and pf.draw_info.cpu().numpy().tolist() == [gl.ST_NO_FREE, 0, 0, 0]
    # a box beyond what a cell index holds: its cells are the ends of int32, the region is empty, and nothing lands outside it
    with pytest.raises(ValueError):
        pf.init_uniform((-2e10, -5.0, -1e10, 5.0))
    assert pf.step == 4 and np.array_equal(pf.poses().view(np.uint64), before.view(np.uint64)) and pf.free_cells((-2e10, -5.0, -1e10, 5.0)).cells[2] == -2 ** 31


def test_the_kidnapped_chain_stage_by_stage(room):
    """tests/test_particles_global_cpu.py's kidnapped chain on the device, N = 1 024: every stage against the restatement given
    the device's own inputs, the injected counts equal to the restated policy's, and the chain's own assertion at the end."""
    from icpmi import gridmatch, particles
    from test_particles_cpu import CHAIN, controls
    grid, field, threshold, scans, truth = room
    H, seed = CHAIN["half_width"], 0
    pf = grid.particle_filter(N, seed=seed, temperature=CHAIN["temperature"], half_width=H)
    table, beyond = gridmatch.beam_table(grid.resolution, grid.resolution, H), 1.5 * (H + 2) * grid.resolution
    wtable, shift = ref.weight_table(CHAIN["temperature"])
    frame = (grid.min_x, grid.min_y, grid.resolution)
    region = dict(box=KIDNAP["box"], heading=KIDNAP["heading"], span=KIDNAP["span"])
    index = host_index(pf.free_cells(KIDNAP["box"]))
    assert all(np.array_equal(a, b) for a, b in zip(index, gl.free_index(*gl.planes_of(field, threshold), 280, gl.box_cells(KIDNAP["box"], *frame))))
    mine, theirs = particles.Recovery(0.05, 0.6), gl.Recovery(0.05, 0.6)
    worst, injected = 0.0, []
    pf.init_gaussian(truth[0], CHAIN["init_sigma"])
    for k, scan in enumerate(scans):
        if k:
            before, step = state_of(pf), pf.step
            pf.predict(controls()[k - 1], CHAIN["motion_sigma"])
            want_t, want_theta = ref.predict(*before, controls()[k - 1], CHAIN["motion_sigma"], seed, step)
            assert np.array_equal(state_of(pf)[0], want_t) and np.array_equal(state_of(pf)[1], want_theta) and pf.step == step + 1
        if k == KIDNAP["scan"]:
            moved = pf.poses() + np.array(KIDNAP["shift"])
            pf.set_poses(moved)
        pair_t, theta, cos_sin = state_of(pf)
        ess, ok = pf.weigh(scan)
        records = pf.records.cpu().numpy()
        want_records = np.array([bref.beam_pair(field, threshold, *frame, scan, pair_t[i], cos_sin[i], table, H, beyond)[0] for i in range(N)])
        assert np.array_equal(records, want_records), k
        want_w, want_sums = ref.weights(records, wtable, shift)
        w = as_u32(pf.w)
        assert np.array_equal(w, want_w) and pf.last_sums == want_sums.tolist() and pf.last_rows == len(scan) == 64
        step = pf.step
        did = pf.maybe_resample(0.5, recovery=mine, **region)
        m = int(theirs.update(int(want_sums[ref.SUM_SMAX]), len(scan)) * N)
        assert pf.last_injected == m and did == (ess < 0.5 * N or m > 0) and (mine.w_slow, mine.w_fast) == (theirs.w_slow, theirs.w_fast)
        injected.append(m if did else None)
        if did:
            anc, _, status = ref.resample(w, seed, step)
            gathered = (pair_t[anc], theta[anc], cos_sin[anc])
            want_t, want_theta, drawn, want_anc = gl.inject(gathered, anc, index, m, *frame, KIDNAP["heading"], KIDNAP["span"], seed, step)
            got_t, got_theta, got_cs = state_of(pf)
            assert status == ref.ST_OK and not pf.degenerate() and pf.step == step + 1 and drawn.sum() == m
            assert np.array_equal(pf.ancestors.cpu().numpy(), want_anc) and (pf.weights() == 1).all()
            assert np.array_equal(got_t.view(np.uint64), want_t.view(np.uint64)) and np.array_equal(got_theta.view(np.uint64), want_theta.view(np.uint64))
            assert np.array_equal(got_cs[~drawn].view(np.uint64), gathered[2][~drawn].view(np.uint64))
            if m:
                worst = max(worst, float(ref.ulps(got_cs[drawn], ref.cos_sin_ld(got_theta[drawn])).max()))
                assert pf.draw_info.cpu().numpy().tolist() == [0, int(index[0][0]), 0, 0]
        else:
            assert pf.step == step
        e_xy, e_th = errors(pf.estimate()["mean"], truth[k])
        print(f"scan {k}: ess {ess:.1f}, injected {injected[-1]}, |dxy| {e_xy:.3f} m, |dtheta| {np.degrees(e_th):.2f} deg")
        if k >= KIDNAP["settled"]:
            assert e_xy < 0.3 and e_th < np.deg2rad(5.0), k
    print(f"injected per scan: {injected}; largest error of the device's cos / sin of a drawn heading: {worst:.3f} ulp")
    assert worst <= SINCOS_ULPS and injected[KIDNAP["scan"]] and injected[KIDNAP["scan"]] > N // 8 and not any(injected[:KIDNAP["scan"]])


def test_injecting_nothing_is_the_resampling_as_it_was(room):
    grid, _, _, scans, truth = room
    a, b = (grid.particle_filter(1000, seed=11) for _ in range(2))
    for pf in (a, b):
        pf.init_gaussian(truth[2], (0.2, 0.2, 0.05))
        pf.weigh(scans[2])
    a.resample()
    b.resample(inject=0, box=(0.0, 0.0, 1.0, 1.0), heading=1.0, span=0.5)
    for x, y in zip(state_of(a) + (a.ancestors.cpu().numpy(), a.info.cpu().numpy()), state_of(b) + (b.ancestors.cpu().numpy(), b.info.cpu().numpy())):
        assert x.tobytes() == y.tobytes()
    assert a.step == b.step == 2 and not b._free and (a.ancestors.cpu().numpy() >= 0).all()         # no index was built for nothing
    # the rows Recovery divides by: the scan's own, or what the voxel filter kept of it — read back with the sums
    from icpmi import gridmatch
    kept = int(gridmatch.cloud_set_of([scans[2]], 0.5).counts_host()[0])
    assert a.last_rows == 64
    a.weigh(scans[2], voxel_size=0.5)
    assert a.last_rows == kept and 0 < kept < 64


def test_refresh_map_drops_the_index_of_the_old_map(gpu):
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    k_bits = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    threshold = int(np.rint(0.5 * 2.0 ** k_bits))
    p = gref.SCENE_POSES[0]
    grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 50)[::64], p))                   # a thin scan: few free cells
    pf = grid.particle_filter(16)
    first = pf.free_cells()
    F1 = first.count()
    want = gl.free_index(*gl.planes_of(gref.quantise(grid.log_odds, k_bits), threshold), 280)
    assert all(np.array_equal(a, b) for a, b in zip(host_index(first), want)) and 0 < F1 == int(want[0][0])
    grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 50), p))                         # the full scan opens more
    assert pf.free_cells() is first and first.count() == F1       # the planes are the old map's until they are packed again
    second = pf.refresh_map().free_cells()
    want = gl.free_index(*gl.planes_of(gref.quantise(grid.log_odds, k_bits), threshold), 280)
    assert second is not first and all(np.array_equal(a, b) for a, b in zip(host_index(second), want)) and second.count() == int(want[0][0]) > F1
    print(f"free cells: {F1} after the thin scan, {second.count()} after the full one")
