"""The particle filter on the device (csrc/particles.hip; icpmi.particles.ParticleFilter; OccupancyGrid2D.particle_filter)
against the NumPy restatement of the contract (tests/particles_ref.py, itself held to Philox's known answers and to the
integer resampling's properties by tests/test_particles_cpu.py).  Every stage is compared given the DEVICE's own inputs, so
a difference names its stage: the motion model bit for bit (cos and sin to the 4 ulp OpenCL sets for double sincos, which
the device library follows), the weights and their sums bit for bit, the ancestors and the gathered state bit for bit at
every size where the prefix sum takes another path, the moments within the bound of any summation order and equal between
runs, and the whole chain on a twelve-scan track in the room map with the beam records held to tests/gridbeam_ref.py."""
import numpy as np
import pytest

import gridbeam_ref as bref
import gridmatch_ref as gref
import particles_ref as ref

pytestmark = pytest.mark.gpu

SINCOS_ULPS = 4.0                                              # OpenCL's bound for double sincos, which OCML follows
BLOCK = ref.SCAN_BLOCK                                         # weights of one scan workgroup (first level)
LANE = ref.SCAN_BLOCK * ref.SUMS_PER_LANE                      # weights behind one lane of the second-level workgroup
WAVE = LANE * 64                                               # ... behind one of its waves
RESAMPLE_SIZES = [1, 2, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, ref.MAX_PARTICLES]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def as_u32(t):
    """A device int32 tensor's bits as uint32 on the host."""
    return t.cpu().numpy().view(np.uint32)


def call(code, what):
    assert code == 0, (what, code)


def stream():
    from icpmi.batch import _stream
    return _stream()


def random_state(n, seed, spread=10.0, turn=95.0):
    rng = np.random.default_rng(seed)
    theta = rng.uniform(-turn, turn, size=n)
    return rng.uniform(-spread, spread, size=(n, 2)), theta, np.stack([np.cos(theta), np.sin(theta)], axis=1)


# ── predict ──────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_predict_is_the_restated_motion_model_bit_for_bit(gpu, n):
    import icpmi
    L = icpmi.lib()
    worst = 0.0
    for seed in (0, 0xFEEDFACECAFEBEEF):
        pair_t, theta, cos_sin = random_state(n, n + (seed & 0xff))
        d = [on_device(v) for v in (pair_t, theta, cos_sin)]
        control, sigma3 = (0.25, -0.02, 0.05), (0.05, 0.03, 0.01)
        for step in (0, 1, 2, 2 ** 32 - 1):
            before = [v.cpu().numpy() for v in d]
            call(L.icpmi_pf_predict(n, *(v.data_ptr() for v in d), *control, *sigma3, seed, step, stream()), "predict")
            got_t, got_theta, got_cs = (v.cpu().numpy() for v in d)
            want_t, want_theta = ref.predict(*before, control, sigma3, seed, step)
            assert np.array_equal(got_t, want_t) and np.array_equal(got_theta, want_theta), (seed, step)
            assert np.abs(got_theta).max() <= 100.0
            worst = max(worst, float(ref.ulps(got_cs, ref.cos_sin_ld(got_theta)).max()))
            control = (-control[0], control[1] * 3.0, -control[2] * 2.0)
    print(f"n = {n}: largest error of the device's cos / sin: {worst:.3f} ulp")
    assert worst <= SINCOS_ULPS


def test_predict_from_the_origin_with_unit_deviations_gives_the_deviates_themselves(gpu):
    """State (0, 0, 0; 1, 0), no control, deviations 1: x' = z0, y' = z1, theta' = z2 exactly, which pins S_m."""
    import icpmi
    L = icpmi.lib()
    n = 1000
    for seed, step in ((0, 0), (12345, 3), (2 ** 64 - 1, 77)):
        d = [on_device(v) for v in (np.zeros((n, 2)), np.zeros(n), np.tile([1.0, 0.0], (n, 1)))]
        call(L.icpmi_pf_predict(n, *(v.data_ptr() for v in d), 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, seed, step, stream()), "predict")
        z = ref.deviates(seed, n, step)
        assert np.array_equal(d[0].cpu().numpy(), z[:, :2]) and np.array_equal(d[1].cpu().numpy(), z[:, 2]), (seed, step)
        assert len(np.unique(z)) > 2000                        # (a condition on the inputs: the draws differ)
    # no deviation: the control alone, every particle alike
    d = [on_device(v) for v in (np.zeros((n, 2)), np.zeros(n), np.tile([0.0, 1.0], (n, 1)))]            # heading +90 degrees
    call(L.icpmi_pf_predict(n, *(v.data_ptr() for v in d), 2.0, 0.5, 0.25, 0.0, 0.0, 0.0, 1, 1, stream()), "predict")
    assert np.array_equal(d[0].cpu().numpy(), np.tile([-0.5, 2.0], (n, 1))) and np.array_equal(d[1].cpu().numpy(), np.full(n, 0.25))


# ── weights ──────────────────────────────────────────────────────────────────
def records_of(status, score):
    rec = np.zeros((len(status), bref.INTS), dtype=np.int32)
    rec[:, bref.STATUS], rec[:, bref.SCORE] = status, score
    rec[:, bref.ROWS] = np.where(rec[:, bref.STATUS] == bref.ST_OK, 64, 0)
    return rec


def weight_record_cases():
    """name -> (records, table, shift)"""
    rng = np.random.default_rng(41)
    table, shift = ref.weight_table(8.0)
    ok = lambda n: np.full(n, bref.ST_OK)                      # noqa: E731
    mixed = rng.choice([bref.ST_OK, bref.ST_EMPTY, bref.ST_CAPACITY], size=700, p=[0.8, 0.1, 0.1])
    lonely = np.full(257, bref.ST_EMPTY)
    lonely[200] = bref.ST_OK
    past = -rng.integers(0, 3 * 4096 * 2 ** shift, size=1000)
    extremes = np.array([2 ** 31 - 1, -2 ** 31, 0, 2 ** 31 - 1, -2 ** 31, -1, 2 ** 31 - 2, 1] * 40)
    huge = np.minimum(table.astype(np.int64) * 5000, 2 ** 32 - 1).astype(np.uint32)          # entries above the clip of 2^20
    return {"every score equal": (records_of(ok(300), np.full(300, -123456)), table, shift),
            "one OK record only": (records_of(lonely, rng.integers(-10 ** 6, 0, size=257)), table, shift),
            "no OK record": (records_of(np.where(np.arange(65) % 2, bref.ST_EMPTY, bref.ST_CAPACITY), np.zeros(65)), table, shift),
            "spread past the table's end": (records_of(ok(1000), past), table, shift),
            "mixed statuses": (records_of(mixed, -rng.integers(0, 4096 * 2 ** shift, size=700)), table, shift),
            "the best score is not OK": (records_of(np.array([bref.ST_EMPTY] + [bref.ST_OK] * 63), np.array([10 ** 6] + [-5 * k for k in range(63)])), table, shift),
            "int32 extremes, shift 0": (records_of(ok(320), extremes), table, 0),
            "int32 extremes, shift 20": (records_of(ok(320), extremes), table, 20),
            "int32 extremes, shift 32": (records_of(ok(320), extremes), table, 32),
            "a table of 8": (records_of(ok(513), -rng.integers(0, 12, size=513)), np.array([9, 8, 7, 6, 5, 4, 3, 2], dtype=np.uint32), 0),
            "a table of 1": (records_of(ok(64), -rng.integers(0, 3, size=64)), np.array([7], dtype=np.uint32), 1),
            "entries above the clip": (records_of(ok(1025), -rng.integers(0, 4096 * 2 ** shift, size=1025)), huge, shift)}


def device_weights(records, table, shift):
    import icpmi
    import torch
    n = len(records)
    rec, tab = on_device(records), on_device(np.asarray(table, dtype=np.uint32).view(np.int32))
    w = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sums = torch.full((ref.SUMS,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    call(icpmi.lib().icpmi_pf_weights(n, rec.data_ptr(), tab.data_ptr(), len(table), shift, w.data_ptr(), sums.data_ptr(), stream()), "weights")
    return as_u32(w), sums.cpu().numpy()


def test_weights_and_their_sums_are_the_restated_integers(gpu):
    seen = set()
    for name, (records, table, shift) in weight_record_cases().items():
        want_w, want_sums = ref.weights(records, table, shift)
        got_w, got_sums = device_weights(records, table, shift)
        print(f"{name}: sums {want_sums.tolist()}")
        assert np.array_equal(got_w, want_w) and np.array_equal(got_sums, want_sums), (name, got_sums.tolist(), want_sums.tolist())
        # a second run into the same kind of buffers: the same bits (the sums are started anew, not added to)
        again_w, again_sums = device_weights(records, table, shift)
        assert np.array_equal(again_w, got_w) and np.array_equal(again_sums, got_sums), name
        seen |= {what for what, some in (("zero weight of an OK record", ((want_w == 0) & (records[:, bref.STATUS] == bref.ST_OK)).any()),
                                        ("no weight at all", want_sums[ref.SUM_W] == 0), ("clipped", (want_w == ref.MAX_WEIGHT).any() and table[0] > ref.MAX_WEIGHT),
                                        ("distance of 2^32 - 1", np.ptp(records[:, bref.SCORE].astype(np.int64)) == 2 ** 32 - 1)) if some}
    assert seen == {"zero weight of an OK record", "no weight at all", "clipped", "distance of 2^32 - 1"}          # (conditions on the inputs)


# ── resample ─────────────────────────────────────────────────────────────────
def device_resample(w, state, seed, step):
    """-> (ancestors, info, gathered pair_t, theta, cos_sin) of icpmi_pf_resample into buffers full of a sentinel."""
    import icpmi
    import torch
    L = icpmi.lib()
    n = len(w)
    wd = on_device(np.asarray(w, dtype=np.uint32).view(np.int32))
    src = [on_device(v) for v in state]
    out = [torch.full_like(v, -7.0) for v in src]
    anc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((ref.INFO_INTS,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.icpmi_pf_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    call(L.icpmi_pf_resample(n, wd.data_ptr(), *(v.data_ptr() for v in src), *(v.data_ptr() for v in out), anc.data_ptr(), info.data_ptr(), seed, step,
                             ws.data_ptr(), ws.numel(), stream()), "resample")
    assert all(np.array_equal(v.cpu().numpy(), s) for v, s in zip(src, state))                 # the inputs are read only
    return (anc.cpu().numpy(), info.cpu().numpy()) + tuple(v.cpu().numpy() for v in out)


@pytest.mark.parametrize("n", RESAMPLE_SIZES)
def test_resampling_gives_the_restated_ancestors_and_state(gpu, n):
    """Sizes: 1, 2, around a workgroup of lanes (256), around one scan block (BLOCK = 1024 weights), around the four blocks
    one lane of the second-level workgroup owns (LANE = 4096), around the 64 lanes of its first wave (WAVE = 262 144), and
    the capacity 2^20, where all 1024 block sums are scanned."""
    state = random_state(n, 7 + n)
    cases = dict(ref.weight_cases(n))
    cases["no weight"] = np.zeros(n, dtype=np.uint32)
    for k, (name, w) in enumerate(cases.items()):
        seed, step = 0xA5A5A5A5DEADBEEF + k, 3 + k
        want_anc, _, want_status = ref.resample(w, seed, step)
        anc, info, pair_t, theta, cos_sin = device_resample(w, state, seed, step)
        assert info.tolist() == [want_status, 0, 0, 0] and np.array_equal(anc, want_anc), (name, np.argwhere(anc != want_anc)[:5].tolist())
        for got, src in zip((pair_t, theta, cos_sin), state):
            assert np.array_equal(got.view(np.uint64), src[want_anc].view(np.uint64)), name


# ── estimate ─────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("n", [1, 255, 257, 1024, 1025, 5000, ref.MAX_PARTICLES])
def test_the_moments_lie_within_the_bound_of_any_summation_order_and_repeat(gpu, n):
    import icpmi
    import torch
    L = icpmi.lib()
    rng = np.random.default_rng(n)
    pair_t, _, cos_sin = random_state(n, n, spread=100.0)
    pair_t[:, 0] += 50.0                                       # a mean away from zero: the second moments cancel less than they add
    w = rng.integers(0, ref.MAX_WEIGHT + 1, size=n).astype(np.uint32)
    w[rng.random(n) < 0.2] = 0
    w[0] = ref.MAX_WEIGHT
    d = [on_device(v) for v in (w.view(np.int32), pair_t, cos_sin)]
    ws = torch.empty(L.icpmi_pf_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        out = torch.full((ref.EST_DOUBLES,), np.nan, dtype=torch.float64, device="cuda")
        call(L.icpmi_pf_estimate(n, *(v.data_ptr() for v in d), out.data_ptr(), ws.data_ptr(), ws.numel(), stream()), "estimate")
        runs.append(out.cpu().numpy())
    want, absolute = ref.estimate(w, pair_t, cos_sin)
    err = np.abs(runs[0].astype(np.longdouble) - want)
    bound = (n + 2) * np.longdouble(2.0) ** -53 * absolute
    print(f"n = {n}: error / bound per sum: {[float(e / b) for e, b in zip(err, bound)]}")
    assert (err <= bound).all() and np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    assert runs[0][0] == float(w.astype(np.int64).sum())      # the weights' own sum is exact: integers below 2^53


# ── the chain, through the Python layers ─────────────────────────────────────
@pytest.fixture(scope="module")
def room(gpu):
    """(the scene's grid at 0.1 m built by update_scan from the twelve scans of the synthetic room, the restated field and its
    threshold, the twelve scans thinned to 64 rows, the true poses)"""
    from icpmi import synth
    from utilities.mapping import OccupancyGrid2D
    grid = OccupancyGrid2D(**gref.SCENE)
    truth = np.array(gref.SCENE_POSES)
    for k, p in enumerate(gref.SCENE_POSES):
        grid.update_scan(np.array(p[:2]), synth.to_world(synth.scan(p, 50 + k), p))
    k_bits = gref.shift_bits(grid.log_odds_min, grid.log_odds_max)
    scans = [synth.scan(p, 50 + k)[::32] for k, p in enumerate(gref.SCENE_POSES)]
    return grid, gref.quantise(grid.log_odds, k_bits), int(np.rint(0.5 * 2.0 ** k_bits)), scans, truth


def state_of(pf):
    return pf.pair_t.cpu().numpy(), pf.theta.cpu().numpy(), pf.cos_sin.cpu().numpy()


def test_the_chain_on_the_room_track_stage_by_stage(room):
    from icpmi import ParticleFilter, ScanHistory, gridmatch
    from test_particles_cpu import CHAIN, controls
    grid, field, threshold, scans, truth = room
    N, H, seed = CHAIN["n"], CHAIN["half_width"], 0x1234567887654321
    pf = grid.particle_filter(N, seed=seed, temperature=CHAIN["temperature"], half_width=H)
    twin = ParticleFilter(grid, N, seed=seed, temperature=CHAIN["temperature"], half_width=H, planes=grid.occupancy_planes())
    assert isinstance(pf, ParticleFilter) and pf.n == N and pf.step == 0
    hist = ScanHistory(voxel_size=0.05, normal_k=None, rotation_voxel_size=0.3, scan_capacity=12, row_capacity=64)
    hist.add_many(scans)
    table, beyond = gridmatch.beam_table(grid.resolution, grid.resolution, H), 1.5 * (H + 2) * grid.resolution
    wtable, shift = ref.weight_table(CHAIN["temperature"])
    assert np.array_equal(pf.weight_table_host, wtable) and pf.weight_shift == shift and np.array_equal(pf.beam_table_host, table)
    worst_ulps, resampled = 0.0, 0

    def check_predict(before, step, control, sigma3):
        nonlocal worst_ulps
        got = state_of(pf)
        want_t, want_theta = ref.predict(*before, control, sigma3, seed, step)
        assert np.array_equal(got[0], want_t) and np.array_equal(got[1], want_theta)
        worst_ulps = max(worst_ulps, float(ref.ulps(got[2], ref.cos_sin_ld(got[1])).max()))

    for f in (pf, twin):
        f.init_gaussian(truth[0], CHAIN["init_sigma"])
    p0 = np.tile(truth[0], (N, 1))
    check_predict((p0[:, :2], p0[:, 2], np.stack([np.cos(p0[:, 2]), np.sin(p0[:, 2])], axis=1)), 0, (0.0, 0.0, 0.0), CHAIN["init_sigma"])
    for k, scan in enumerate(scans):
        if k:
            before, step = state_of(pf), pf.step
            for f in (pf, twin):
                f.predict(controls()[k - 1], CHAIN["motion_sigma"])
            assert pf.step == step + 1
            check_predict(before, step, controls()[k - 1], CHAIN["motion_sigma"])
        # the measurement: the beam records against the beam model's restatement at the device's own particles, then the weights
        pair_t, theta, cos_sin = state_of(pf)
        ess, ok = pf.weigh(scan)
        records = pf.records.cpu().numpy()
        want_records = np.array([bref.beam_pair(field, threshold, grid.min_x, grid.min_y, grid.resolution, scan, pair_t[i], cos_sin[i], table, H, beyond)[0]
                                 for i in range(N)])
        assert np.array_equal(records, want_records), k
        want_w, want_sums = ref.weights(records, wtable, shift)
        w = as_u32(pf.w)
        assert np.array_equal(w, want_w) and pf.last_sums == want_sums.tolist() and ok == N
        assert ess == int(want_sums[0]) ** 2 / int(want_sums[1])
        # the same scan resident in a history: the same bits
        assert pf.weigh_history(hist, k) == (ess, ok) and np.array_equal(pf.records.cpu().numpy(), records) and np.array_equal(as_u32(pf.w), w)
        assert twin.weigh(scan) == (ess, ok)
        # resampling by the real weights
        step = pf.step
        did = pf.maybe_resample(0.5)
        assert did == (ess < 0.5 * N) == twin.maybe_resample(0.5)
        if did:
            resampled += 1
            want_anc, _, status = ref.resample(w, seed, step)
            assert status == ref.ST_OK and not pf.degenerate() and np.array_equal(pf.ancestors.cpu().numpy(), want_anc) and pf.step == step + 1
            for got, src in zip(state_of(pf), (pair_t, theta, cos_sin)):
                assert np.array_equal(got.view(np.uint64), src[want_anc].view(np.uint64))
            assert (pf.weights() == 1).all()
        # the estimate of what is there now
        est = pf.estimate()
        want, absolute = ref.estimate(as_u32(pf.w), *[state_of(pf)[i] for i in (0, 2)])
        assert (np.abs(est["sums"].astype(np.longdouble) - want) <= (N + 2) * np.longdouble(2.0) ** -53 * absolute).all()
        mean, cov, resultant = ref.pose_of(est["sums"])
        assert np.array_equal(est["mean"], mean) and np.array_equal(est["covariance"], cov) and est["resultant"] == resultant
        e_xy = float(np.hypot(*(mean[:2] - truth[k, :2])))
        e_th = float(abs((mean[2] - truth[k, 2] + np.pi) % (2 * np.pi) - np.pi))
        print(f"scan {k}: ess {ess:.1f}, resampled {did}, |dxy| {e_xy:.3f} m, |dtheta| {np.degrees(e_th):.2f} deg, resultant {resultant:.4f}")
        if k >= 3:
            assert e_xy < 0.3 and e_th < np.deg2rad(5.0), k
    print(f"largest error of the device's cos / sin over the chain: {worst_ulps:.3f} ulp; resampled at {resampled} of 12 scans")
    assert worst_ulps <= SINCOS_ULPS and resampled >= 3        # (a condition on the inputs: the chain does resample)
    # the filter made by the grid and the one made by hand, on kept planes: the same bits all the way
    assert np.array_equal(pf.poses().view(np.uint64), twin.poses().view(np.uint64)) and pf.step == twin.step
    assert np.array_equal(pf.poses(), np.concatenate([state_of(pf)[0], state_of(pf)[1][:, None]], axis=1))


def test_particles_off_every_map_have_no_weight_and_the_python_layer_refuses_what_it_must(room):
    from icpmi import ParticleFilter, particles
    grid, _, _, scans, truth = room
    pf = grid.particle_filter(100, seed=5)
    pf.set_poses([1e300, 0.0, 0.0])                                # no cell: every record EMPTY
    before = pf.poses()
    assert pf.weigh(scans[0]) == (0.0, 0) and pf.last_sums == [0, 0, 0, particles.NO_SCORE] and not pf.weights().any()
    assert pf.maybe_resample() and pf.degenerate() and np.array_equal(pf.ancestors.cpu().numpy(), np.arange(100))
    assert np.array_equal(pf.poses().view(np.uint64), before.view(np.uint64))
    assert np.isnan(pf.set_poses(truth[0]).estimate()["mean"]).sum() == 0 and np.isnan(grid.particle_filter(3).estimate()["mean"]).sum() == 0
    pf.w.fill_(0)
    assert np.isnan(pf.estimate()["mean"]).all()
    # set_poses: one pose for all, or a row each; an estimate of equal particles is the pose itself
    rows = np.tile(truth[3], (100, 1))
    est = pf.set_poses(rows).estimate()
    assert np.allclose(est["mean"], truth[3], rtol=0, atol=1e-12) and abs(est["resultant"] - 1.0) < 1e-12 and np.abs(est["covariance"]).max() < 1e-9
    assert not pf.refresh_map().maybe_resample(0.0)               # (ess < 0 never holds)
    for bad in (dict(n=0), dict(n=2 ** 20 + 1), dict(n=1.5), dict(seed=-1), dict(seed=2 ** 64), dict(half_width=128), dict(beyond=-1.0),
                dict(temperature=0.0), dict(table=np.zeros(5, dtype=np.int32)), dict(field=grid.score_field(), planes=grid.occupancy_planes())):
        with pytest.raises(ValueError):
            ParticleFilter(grid, **{**dict(n=10), **bad})
    for call_ in (lambda: pf.set_poses(np.zeros((99, 3))), lambda: pf.set_poses([np.nan, 0, 0]), lambda: pf.predict((0, 0), (0, 0, 0)),
                  lambda: pf.predict((0, 0, np.inf), (0, 0, 0)), lambda: pf.predict((0, 0, 0), (0, -1, 0)), lambda: pf.weigh(np.zeros((70000, 2))),
                  lambda: grid.particle_filter(4).maybe_resample(),
                  lambda: ParticleFilter(grid, 4, planes=grid.occupancy_planes()).refresh_map()):
        with pytest.raises(ValueError):
            call_()
