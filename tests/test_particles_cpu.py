"""Host side of the particle filter (include/icpmi.h: icpmi_pf_predict, icpmi_pf_weights, icpmi_pf_resample,
icpmi_pf_estimate, icpmi_pf_workspace_bytes): the C ABI as the header declares it, every refusal the entries decide on the
host — before anything is enqueued, so no GPU is touched (the device pointers are fakes that are never dereferenced, and no
call here is one the library would accept) — the weight table the Python layer forms, and the NumPy restatement the device
test compares against (tests/particles_ref.py): Philox against its known answers, the deviates at their ends, the integer
resampling at its edges, and the restated filter alone localising in the room map of the grid-matching suite."""
import ctypes
import os
import re

import numpy as np
import pytest

import gridmatch_ref as gref
import particles_ref as ref
from conftest import REPO

FAKE = 4096                                                    # a non-null, 16-byte aligned address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
ENTRIES = {"icpmi_pf_predict": 13, "icpmi_pf_weights": 8, "icpmi_pf_resample": 15, "icpmi_pf_estimate": 8, "icpmi_pf_workspace_bytes": 1}
inf, nan = float("inf"), float("nan")


def test_entries_and_constants_agree_in_header_library_and_loader():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name, args in ENTRIES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        proto = re.search(r"^(?:int|size_t) " + name + r"\((.*?)\);", hdr, flags=re.S | re.M).group(1)
        assert len(proto.split(",")) == args == len(getattr(lib, name).argtypes), name
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define ICPMI_(PF_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M)}
    assert defines == {"PF_MAX_PARTICLES": 2 ** 20, "PF_THREADS": 256, "PF_PREDICT_BLOCKS": 5, "PF_PURPOSE_PREDICT": 0, "PF_PURPOSE_RESAMPLE": 1,
                       "PF_MAX_ENTRIES": 4096, "PF_MAX_SHIFT": 32, "PF_MAX_WEIGHT": 2 ** 20, "PF_SUMS": 4, "PF_SUM_W": 0, "PF_SUM_WW": 1,
                       "PF_SUM_OK": 2, "PF_SUM_SMAX": 3, "PF_SCAN_BLOCK": 1024, "PF_SUMS_PER_LANE": 4, "PF_INFO_INTS": 4, "PF_ST_OK": 0,
                       "PF_ST_DEGENERATE": 1, "PF_EST_CHUNK": 1024, "PF_EST_DOUBLES": 8}
    assert defines == {k: getattr(_lib, k) for k in defines}
    assert sorted(k for k in vars(_lib) if k.startswith("PF_")) == sorted(defines)
    assert defines == {"PF_" + k: getattr(ref, k) for k in (
        "MAX_PARTICLES", "THREADS", "PREDICT_BLOCKS", "PURPOSE_PREDICT", "PURPOSE_RESAMPLE", "MAX_ENTRIES", "MAX_SHIFT", "MAX_WEIGHT", "SUMS", "SUM_W",
        "SUM_WW", "SUM_OK", "SUM_SMAX", "SCAN_BLOCK", "SUMS_PER_LANE", "INFO_INTS", "ST_OK", "ST_DEGENERATE", "EST_CHUNK", "EST_DOUBLES")}
    # one workgroup scans every block sum of the largest filter; W <= 2^40 and the squares' sum <= 2^60
    assert ref.MAX_PARTICLES == ref.SCAN_BLOCK * ref.THREADS * ref.SUMS_PER_LANE and ref.MAX_WEIGHT * ref.MAX_PARTICLES == 2 ** 40
    from icpmi import particles
    assert icpmi.ParticleFilter is particles.ParticleFilter and icpmi.weight_table is particles.weight_table
    assert (particles.MAX_PARTICLES, particles.NO_SCORE) == (ref.MAX_PARTICLES, ref.NO_SCORE)


def test_workspace_bytes_against_literal_values():
    """head 256 + a(8 blocks) + a(4 n) + a(64 chunks), a(x) = x rounded up to 256, blocks = chunks = ceil(n / 1024)."""
    import icpmi
    L = icpmi.lib()
    for n, want in ((1, 1024), (1024, 256 + 256 + 4096 + 256), (1025, 256 + 256 + 4352 + 256), (2 ** 20, 256 + 8192 + 4194304 + 65536),
                    (0, 0), (-1, 0), (2 ** 20 + 1, 0)):
        assert L.icpmi_pf_workspace_bytes(n) == want, n


def test_entries_refuse_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    N = 1000
    need = L.icpmi_pf_workspace_bytes(N)

    def predict(n=N, pair_t=FAKE, theta=FAKE, cos_sin=FAKE, u=(0.1, 0.0, 0.01), s=(0.1, 0.1, 0.01)):
        return L.icpmi_pf_predict(n, pair_t, theta, cos_sin, *u, *s, 7, 3, None)

    def weights(n=N, records=FAKE, wtable=FAKE, entries=4096, shift=3, w=FAKE, sums=FAKE):
        return L.icpmi_pf_weights(n, records, wtable, entries, shift, w, sums, None)

    def resample(n=N, w=FAKE, pair_t=FAKE, theta=FAKE, cos_sin=FAKE, out_pair_t=2 * FAKE, out_theta=2 * FAKE, out_cos_sin=2 * FAKE, ancestors=FAKE,
                 info=FAKE, ws=FAKE, ws_bytes=need - 1):
        return L.icpmi_pf_resample(n, w, pair_t, theta, cos_sin, out_pair_t, out_theta, out_cos_sin, ancestors, info, 7, 3, ws, ws_bytes, None)

    def estimate(n=N, w=FAKE, pair_t=FAKE, cos_sin=FAKE, out=FAKE, ws=FAKE, ws_bytes=need - 1):
        return L.icpmi_pf_estimate(n, w, pair_t, cos_sin, out, ws, ws_bytes, None)

    # the number of particles comes first, in every entry: negative, above the capacity (before a null pointer is seen),
    # and nothing to do is no refusal, whatever else is passed
    for entry, nulls in ((predict, dict(pair_t=None)), (weights, dict(records=None)), (resample, dict(w=None)), (estimate, dict(out=None))):
        assert entry(n=-1) == ERR_ARG and entry(n=2 ** 20 + 1, **nulls) == ERR_UNSUPPORTED and entry(n=0, **nulls) == 0, entry.__name__
    assert predict(n=0, u=(nan, 0, 0), s=(-1, 0, 0)) == 0 and weights(n=0, entries=0, shift=-1) == 0 and resample(n=0, ws=None, out_theta=None) == 0
    # predict: pointers, then finite numbers, then deviations not below zero
    for name in ("pair_t", "theta", "cos_sin"):
        assert predict(**{name: None}) == ERR_ARG, name
    assert predict(pair_t=FAKE + 8) == ERR_ARG and predict(cos_sin=FAKE + 8) == ERR_ARG and predict(theta=FAKE + 4) == ERR_ARG
    for bad in (nan, inf, -inf):
        for k in range(3):
            assert predict(u=tuple(bad if i == k else 0.0 for i in range(3))) == ERR_ARG
            assert predict(s=tuple(bad if i == k else 0.0 for i in range(3))) == ERR_ARG
    for k in range(3):
        assert predict(s=tuple(-1e-300 if i == k else 0.0 for i in range(3))) == ERR_ARG
    # weights: pointers, then the table's size and the shift
    for name in ("records", "wtable", "w", "sums"):
        assert weights(**{name: None}) == ERR_ARG, name
    assert weights(records=FAKE + 8) == ERR_ARG and weights(sums=FAKE + 4) == ERR_ARG
    assert weights(entries=0) == ERR_ARG and weights(entries=4097) == ERR_ARG and weights(shift=-1) == ERR_ARG and weights(shift=33) == ERR_ARG
    # resample: pointers, alignment, an output that is its input — all before the workspace, which is last in line
    for name in ("w", "pair_t", "theta", "cos_sin", "out_pair_t", "out_theta", "out_cos_sin", "ancestors", "info"):
        assert resample(**{name: None}) == ERR_ARG, name
    for name in ("pair_t", "cos_sin", "out_pair_t", "out_cos_sin"):
        assert resample(**{name: FAKE + 8}) == ERR_ARG, name
    assert resample(theta=FAKE + 4) == ERR_ARG and resample(out_theta=FAKE + 4) == ERR_ARG
    assert resample(out_pair_t=FAKE) == ERR_ARG and resample(out_theta=FAKE) == ERR_ARG and resample(out_cos_sin=FAKE) == ERR_ARG
    assert resample() == ERR_WORKSPACE and resample(ws=None, ws_bytes=need) == ERR_WORKSPACE and resample(ws=FAKE + 8, ws_bytes=need) == ERR_WORKSPACE
    assert resample(n=2 ** 20, ws_bytes=L.icpmi_pf_workspace_bytes(2 ** 20) - 1) == ERR_WORKSPACE          # the capacity itself is allowed
    # estimate likewise
    for name in ("w", "pair_t", "cos_sin", "out"):
        assert estimate(**{name: None}) == ERR_ARG, name
    assert estimate(pair_t=FAKE + 8) == ERR_ARG and estimate(cos_sin=FAKE + 8) == ERR_ARG and estimate(out=FAKE + 4) == ERR_ARG
    assert estimate() == ERR_WORKSPACE and estimate(ws=None, ws_bytes=need) == ERR_WORKSPACE and estimate(ws=FAKE + 8, ws_bytes=need) == ERR_WORKSPACE


def test_philox_gives_the_known_answers():
    for counter, key, want in ref.KNOWN_ANSWERS:
        got = ref.philox(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # a batch is its rows, and draw() places particle, block, step and purpose and splits the seed as the contract says
    batch = ref.philox(np.array([k[0] for k in ref.KNOWN_ANSWERS], dtype=np.uint32), np.array([k[1] for k in ref.KNOWN_ANSWERS], dtype=np.uint32))
    assert [tuple(int(v) for v in row) for row in batch] == [k[2] for k in ref.KNOWN_ANSWERS]
    counter, key, want = ref.KNOWN_ANSWERS[2]
    assert tuple(int(v) for v in ref.draw(key[0] | (key[1] << 32), np.array([counter[0]]), counter[1], counter[2], counter[3])[0]) == want


def test_deviates_at_their_ends_and_in_the_large():
    assert ref.deviate_of_halves([0] * 12) == -393210 * 2.0 ** -16 and ref.deviate_of_halves([65535] * 12) == 393210 * 2.0 ** -16
    assert ref.deviate_of_halves([65535] * 6 + [0] * 6) == 0.0 and 393210 * 2.0 ** -16 < 6.0
    z = ref.deviates(12345, 100000, 3)
    assert z.shape == (100000, 3) and np.array_equal(z * 65536.0, np.rint(z * 65536.0))          # multiples of 2^-16
    print("mean", z.mean(axis=0), "std", z.std(axis=0), "extremes", z.min(), z.max())
    # 1e5 draws of unit variance: the mean within 4 / sqrt(n), the deviation within 4 / sqrt(2 n)
    assert (np.abs(z.mean(axis=0)) < 4.0 / np.sqrt(1e5)).all() and (np.abs(z.std(axis=0) - 1.0) < 4.0 / np.sqrt(2e5)).all()
    assert abs(np.corrcoef(z.T)[0, 1]) < 4.0 / np.sqrt(1e5) and np.abs(z).max() < 6.0
    # a function of (seed, step, particle): other particles do not matter, another step or seed gives other draws
    assert np.array_equal(ref.deviates(12345, 10, 3), z[:10]) and not np.array_equal(ref.deviates(12345, 10, 4), z[:10])
    assert not np.array_equal(ref.deviates(12345 + 2 ** 32, 10, 3), z[:10])


def test_the_weight_table():
    from icpmi import particles
    for temperature in (1.0, 8.0, 1e4):
        table, shift = particles.weight_table(temperature)
        want, want_shift = ref.weight_table(temperature)
        assert table.dtype == np.uint32 and table.shape == (4096,) and shift == want_shift and np.array_equal(table, want)
        last = lambda s: 2 ** 20 * np.exp(-(4095 * 2.0 ** s) / (1024 * temperature))          # noqa: E731
        assert last(shift) < 0.5 and (shift == 0 or last(shift - 1) >= 0.5)                     # the least such shift
        assert table[0] == 2 ** 20 and (np.diff(table.astype(np.int64)) <= 0).all() and table[-1] == 0
        # the entry before the shift's bound — the last one whose value is at least 0.5 — is not 0
        q = np.arange(4096)
        assert table[q[2 ** 20 * np.exp(-(q * 2.0 ** shift) / (1024 * temperature)) >= 0.5].max()] > 0
    assert [particles.weight_table(t)[1] for t in (1.0, 8.0, 1e4)] == [2, 5, 16]               # 2^shift > 3.64 T: 3.64, 29.1, 36 400
    t, s = particles.weight_table(2.0, scale=100, entries=8, peak=1000)
    assert s == 8 and t.tolist() == [int(np.rint(1000 * np.exp(-q * 256 / 200.0))) for q in range(8)]          # 7 * 2^s / 200 > ln 2000
    assert particles.weight_table(1.0, entries=1)[0].tolist() == [2 ** 20] and particles.weight_table(1.0, entries=1)[1] == 0
    for bad in (dict(temperature=0.0), dict(temperature=nan), dict(scale=0), dict(entries=0), dict(entries=4097), dict(entries=1.5), dict(peak=0),
                dict(peak=2 ** 20 + 1), dict(temperature=1e12)):
        with pytest.raises(ValueError):
            particles.weight_table(**{**dict(temperature=1.0), **bad})


def offspring_are_fair(w, off, n):
    """Sum n; each count within 1 of n w_i / W (in integers: |count W - n w_i| <= W); no offspring of a zero weight."""
    w, off = w.astype(object), off.astype(object)
    W = int(w.sum())
    return int(off.sum()) == n and all(abs(int(c) * W - n * int(v)) <= W for c, v in zip(off, w)) and not off[w == 0].any()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_resampling_restated(n):
    for name, w in ref.weight_cases(n).items():
        for step in (0, 5):
            anc, off, status = ref.resample(w, 99, step)
            if not w.any():
                assert status == ref.ST_DEGENERATE and np.array_equal(anc, np.arange(n)), name
                continue
            assert status == ref.ST_OK and anc.dtype == np.int32 and len(anc) == n and (np.diff(anc) >= 0).all(), name
            assert np.array_equal(np.bincount(anc, minlength=n), off) and offspring_are_fair(w, off, n), name
            assert off.tolist() == ref.resample_ints(w, 99, step), name
    anc, _, status = ref.resample(np.zeros(n, dtype=np.uint32), 99, 0)
    assert status == ref.ST_DEGENERATE and np.array_equal(anc, np.arange(n))
    if n > 1:
        assert (ref.resample(ref.weight_cases(n)["first alone"], 1, 0)[0] == 0).all() and (ref.resample(ref.weight_cases(n)["last alone"], 1, 0)[0] == n - 1).all()


def test_resampling_at_the_capacity_with_every_weight_at_the_peak():
    """n = 2^20, w = 2^20 each: W = 2^40, n C_i + rho reaches 2^60 + rho < 2^61, and every particle has exactly one child."""
    n = ref.MAX_PARTICLES
    w = ref.weight_cases(n)["all at the peak"]
    anc, off, status = ref.resample(w, 7, 11)
    assert status == ref.ST_OK and int(w.astype(np.uint64).sum()) == 2 ** 40 and np.array_equal(anc, np.arange(n)) and (off == 1).all()
    assert 0 <= ref.rho_of(7, 11, 2 ** 40) < 2 ** 40 and ref.rho_of(7, 11, 2 ** 40) != ref.rho_of(7, 12, 2 ** 40)
    runs = ref.weight_cases(n)["runs of zeros"]
    anc, off, status = ref.resample(runs, 7, 11)
    W = int(runs.astype(np.uint64).sum())
    assert int(off.sum()) == n and not off[runs == 0].any() and (np.abs(off.astype(np.float64) - n * runs.astype(np.float64) / W) <= 1.0 + 1e-9).all()


CHAIN = dict(n=256, thin=32, temperature=8.0, seed=0, init_sigma=(0.3, 0.3, np.deg2rad(5.0)), motion_sigma=(0.05, 0.05, np.deg2rad(1.0)), half_width=8)


def controls():
    """The pose difference between consecutive scene poses, in the frame of the earlier one."""
    p = np.array(gref.SCENE_POSES)
    out = []
    for a, b in zip(p[:-1], p[1:]):
        c, s, d = np.cos(a[2]), np.sin(a[2]), b[:2] - a[:2]
        out.append((c * d[0] + s * d[1], -s * d[0] + c * d[1], b[2] - a[2]))
    return out


def room_filter(seed=CHAIN["seed"]):
    """-> (the restated filter in the room map at CHAIN's values, the twelve 64-row scans)."""
    from icpmi import gridmatch, synth
    from test_grid_cast_cpu import room_field
    q, g = room_field()
    H = CHAIN["half_width"]
    wtable, shift = ref.weight_table(CHAIN["temperature"])
    f = ref.Filter(q, int(np.rint(0.5 * 2.0 ** 12)), g["min_x"], g["min_y"], 0.1, CHAIN["n"], seed, wtable, shift, gridmatch.beam_table(0.1, 0.1, H), H,
                   1.5 * (H + 2) * 0.1)
    scans = [synth.scan(p, 50 + k)[::CHAIN["thin"]] for k, p in enumerate(gref.SCENE_POSES)]
    assert all(len(s) == 64 for s in scans)
    return f, scans


def test_the_restated_filter_localises_in_the_room_map():
    """The room map of tests/test_grid_cast_cpu.py::room_field, the scans synth.scan(SCENE_POSES[k], 50 + k)[::32] (64 rows),
    N = 256, init_gaussian about SCENE_POSES[0] with (0.3 m, 0.3 m, 5 degrees), the control the pose difference of consecutive
    scene poses with motion noise (0.05 m, 0.05 m, 1 degree), temperature 8, resampling below ess = N / 2, seed 0: the values
    the issue proposed, unchanged.  From the fourth scan on the estimate lies within the initial deviations of the true pose
    (0.3 m, 5 degrees).  Seen when this was written, seed 0: position errors 0.016, 0.008, 0.010, 0.025, 0.022, 0.013, 0.015,
    0.011, 0.009, 0.005, 0.006, 0.005 m, heading errors at most 0.11 degrees; the ess of the first scan is 3.2 of 256 — the
    prior is wide against a likelihood this sharp — and 80 to 130 afterwards.  Seeds 1, 2, 3 and 12345678901234567 were
    run by hand with the same outcome (errors below 0.05 m at every scan), so the condition does not hang on the seed."""
    f, scans = room_filter()
    truth = np.array(gref.SCENE_POSES)
    f.init_gaussian(truth[0], CHAIN["init_sigma"])
    for k, scan in enumerate(scans):
        if k:
            f.predict(controls()[k - 1], CHAIN["motion_sigma"])
        ess, ok = f.weigh(scan)
        if ess < 0.5 * f.n:
            f.resample()
        mean, cov, resultant = f.estimate()
        e_xy = float(np.hypot(*(mean[:2] - truth[k, :2])))
        e_th = float(abs((mean[2] - truth[k, 2] + np.pi) % (2 * np.pi) - np.pi))
        print(f"scan {k}: ess {ess:.1f}, ok {ok}, |dxy| {e_xy:.3f} m, |dtheta| {np.degrees(e_th):.2f} deg, resultant {resultant:.4f}")
        assert ok == f.n and ess >= 1.0
        if k >= 3:
            assert e_xy < 0.3 and e_th < np.deg2rad(5.0), k
