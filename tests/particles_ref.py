"""NumPy restatement of the particle filter's contract in include/icpmi.h (icpmi_pf_predict, icpmi_pf_weights,
icpmi_pf_resample, icpmi_pf_estimate): Philox4x32-10 and the deviates made of its halves, the motion model in float64 with
every operation rounded on its own, the weights and the resampling in integers (uint64 arrays; ``resample_ints`` restates
them once more in Python integers), the moments in long double — and a whole filter made of them over the beam model's
restatement (tests/gridbeam_ref.py), which the CPU suite localises in the room map and the GPU suite compares the device
with, stage by stage (tests/test_particles_cpu.py, tests/test_particles_gpu.py).  It uses nothing of the library."""
import numpy as np

import gridbeam_ref as bref

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MAX_PARTICLES, THREADS, PREDICT_BLOCKS, PURPOSE_PREDICT, PURPOSE_RESAMPLE = 2 ** 20, 256, 5, 0, 1
MAX_ENTRIES, MAX_SHIFT, MAX_WEIGHT = 4096, 32, 2 ** 20
SUMS, SUM_W, SUM_WW, SUM_OK, SUM_SMAX = 4, 0, 1, 2, 3
SCAN_BLOCK, SUMS_PER_LANE, INFO_INTS, ST_OK, ST_DEGENERATE, EST_CHUNK, EST_DOUBLES = 1024, 4, 4, 0, 1, 1024, 8
NO_SCORE = -2 ** 63
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(counter, key):
    """Philox4x32-10 of counters (..., 4) under keys (..., 2), uint32 words -> (..., 4) uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                   # (32-bit factors: the products fit a uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def draw(seed, particle, block, step, purpose):
    """The four words at counter [particle, block, step, purpose] under the key (seed low word, seed high word)."""
    particle = np.asarray(particle, dtype=np.uint64)
    ctr = np.stack([particle, np.full_like(particle, block), np.full_like(particle, step), np.full_like(particle, purpose)], axis=-1)
    return philox(ctr, np.broadcast_to(np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64), ctr.shape[:-1] + (2,)))


def deviate_of_halves(halves):
    """z = (S - 393 210) * 2^-16 of twelve 16-bit halves (..., 12)."""
    S = np.asarray(halves, dtype=np.int64).sum(axis=-1)
    return (S - 393210).astype(np.float64) * 2.0 ** -16


def deviates(seed, n, step):
    """-> (n, 3) float64: particle i's z0, z1, z2, from the 40 halves of its blocks 0 .. 4 (word order, low half first)."""
    words = np.concatenate([draw(seed, np.arange(n), b, step, PURPOSE_PREDICT) for b in range(PREDICT_BLOCKS)], axis=-1).astype(np.int64)
    halves = np.stack([words & 0xffff, words >> 16], axis=-1).reshape(n, 8 * PREDICT_BLOCKS)
    return np.stack([deviate_of_halves(halves[:, 12 * m:12 * m + 12]) for m in range(3)], axis=1)


def predict(pair_t, theta, cos_sin, control, sigma3, seed, step):
    """The motion model -> (pair_t', theta'): NumPy's float64 operations are rounded one by one.  (cos, sin) of theta' are
    the device library's own and are not restated: ``cos_sin_ld`` gives what they are compared with."""
    pair_t, theta, cos_sin = (np.asarray(v, dtype=np.float64) for v in (pair_t, theta, cos_sin))
    z = deviates(seed, len(theta), step)
    dx, dy, dth = (np.float64(v) for v in control)
    sx, sy, sth = (np.float64(v) for v in sigma3)
    ux, uy, ut = dx + sx * z[:, 0], dy + sy * z[:, 1], dth + sth * z[:, 2]
    c, s = cos_sin[:, 0], cos_sin[:, 1]
    return np.stack([pair_t[:, 0] + (c * ux - s * uy), pair_t[:, 1] + (s * ux + c * uy)], axis=1), theta + ut


def cos_sin_ld(theta):
    """(cos, sin) of float64 angles in long double, as long double (n, 2)."""
    t = np.asarray(theta, dtype=np.float64).astype(np.longdouble)
    return np.stack([np.cos(t), np.sin(t)], axis=1)


def ulps(got, want_ld):
    """|got - want| in units of the last place of float64 at |want| (at least the least normal's)."""
    want_ld = np.asarray(want_ld, dtype=np.longdouble)
    return np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - want_ld) / np.spacing(np.maximum(np.abs(want_ld.astype(np.float64)), 2.0 ** -1022))


def weight_table(temperature, scale=1024, entries=4096, peak=2 ** 20):
    """The rule of icpmi.particles.weight_table, restated: the least shift whose last entry rounds to 0."""
    shift = 0
    while peak * np.exp(-((entries - 1) * 2.0 ** shift) / (scale * temperature)) >= 0.5:
        shift += 1
    q = np.arange(entries, dtype=np.float64)
    return np.rint(peak * np.exp(-(q * 2.0 ** shift) / (float(scale) * float(temperature)))).astype(np.uint32), shift


def weights(records, wtable, shift):
    """-> (w uint32 [n], sums int64 [4]) of beam records (n, 8) int32."""
    rec = np.asarray(records).reshape(-1, bref.INTS).astype(np.int64)
    table = np.minimum(np.asarray(wtable).astype(np.int64), MAX_WEIGHT)
    ok = rec[:, bref.STATUS] == bref.ST_OK
    w = np.zeros(len(rec), dtype=np.int64)
    if not ok.any():
        return w.astype(np.uint32), np.array([0, 0, 0, NO_SCORE], dtype=np.int64)
    s_max = int(rec[ok, bref.SCORE].max())
    q = (s_max - rec[:, bref.SCORE]) >> shift
    inside = ok & (q < len(table))
    w[inside] = table[q[inside]]
    return w.astype(np.uint32), np.array([w.sum(), (w * w).sum(), ok.sum(), s_max], dtype=np.int64)


def rho_of(seed, step, W):
    r = draw(seed, np.array([0]), 0, step, PURPOSE_RESAMPLE)[0]
    return ((int(r[1]) << 32) + int(r[0])) % W


def resample(w, seed, step):
    """-> (ancestors int32 [n], offspring int64 [n], status): uint64 arithmetic, n * C_i + rho < 2^61."""
    w = np.asarray(w).astype(np.uint64)
    n = len(w)
    C = np.cumsum(w, dtype=np.uint64)
    W = int(C[-1])
    if W == 0:
        return np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int64), ST_DEGENERATE
    assert n * W + W < 2 ** 61
    E = (np.uint64(n) * C + np.uint64(rho_of(seed, step, W))) // np.uint64(W)
    off = np.diff(np.concatenate([[np.uint64(0)], E])).astype(np.int64)
    return np.repeat(np.arange(n, dtype=np.int32), off), off, ST_OK


def resample_ints(w, seed, step):
    """``resample``'s offspring once more, in Python integers."""
    w = [int(v) for v in w]
    n, W = len(w), sum(w)
    if W == 0:
        return [1] * n
    rho, C, before, out = rho_of(seed, step, W), 0, 0, []
    for v in w:
        C += v
        E = (n * C + rho) // W
        out.append(E - before)
        before = E
    return out


def weight_cases(n, seed=0):
    """The weights both suites resample, by name -> uint32 [n]: runs of zeros between runs of table-like weights, a single
    weight (the first, the last), every weight at the peak."""
    rng = np.random.default_rng(900 + seed + n)
    runs = rng.integers(0, MAX_WEIGHT + 1, size=n, dtype=np.int64)
    edges = np.sort(rng.integers(0, n + 1, size=8))
    for a, b in zip(edges[0::2], edges[1::2]):
        runs[a:b] = 0
    if n > 2:
        runs[0] = runs[-1] = 0                                 # a run of zeros at each end
        runs[n // 2] = MAX_WEIGHT                              # (and never all of them)
    first, last = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    first[0], last[-1] = 1, MAX_WEIGHT
    return {"runs of zeros": runs.astype(np.uint32), "first alone": first.astype(np.uint32), "last alone": last.astype(np.uint32),
            "all at the peak": np.full(n, MAX_WEIGHT, dtype=np.uint32)}


def estimate(w, pair_t, cos_sin):
    """-> (sums long double [8], sum of |term| long double [8]): the terms are the device's — every product rounded to
    float64 on its own — and only their sum is formed in long double."""
    wd = np.asarray(w).astype(np.float64)
    x, y, c, s = (np.asarray(v, dtype=np.float64) for v in (pair_t[:, 0], pair_t[:, 1], cos_sin[:, 0], cos_sin[:, 1]))
    wx, wy = wd * x, wd * y
    terms = np.stack([wd, wx, wy, wd * c, wd * s, wx * x, wx * y, wy * y], axis=1).astype(np.longdouble)
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def pose_of(sums):
    """The estimate's pose and spread of the eight sums (float64 arithmetic) -> (mean [x, y, theta], covariance (2, 2),
    resultant length)."""
    S = [float(v) for v in sums]
    W = S[0]
    mx, my = S[1] / W, S[2] / W
    cov = np.array([[S[5] / W - mx * mx, S[6] / W - mx * my], [S[6] / W - mx * my, S[7] / W - my * my]])
    return np.array([mx, my, np.arctan2(S[4], S[3])]), cov, float(np.hypot(S[3], S[4]) / W)


class Filter:
    """The filter restated on the host: the state in NumPy, the beam model by tests/gridbeam_ref.py, cos and sin by NumPy."""

    def __init__(self, field, threshold, min_x, min_y, res, n, seed, wtable, shift, beam_table, half_width, beyond):
        self.map = (field, threshold, min_x, min_y, res)
        self.n, self.seed, self.step = n, seed, 0
        self.wtable, self.shift, self.beam_table, self.H, self.beyond = wtable, shift, beam_table, half_width, beyond
        self.w = np.ones(n, dtype=np.uint32)

    def set_poses(self, poses):
        p = np.broadcast_to(np.asarray(poses, dtype=np.float64), (self.n, 3))
        self.pair_t, self.theta = p[:, :2].copy(), p[:, 2].copy()
        self.cos_sin = np.stack([np.cos(self.theta), np.sin(self.theta)], axis=1)
        self.w = np.ones(self.n, dtype=np.uint32)

    def init_gaussian(self, pose, sigma3):
        self.set_poses(pose)
        self.predict((0.0, 0.0, 0.0), sigma3)

    def predict(self, control, sigma3):
        self.pair_t, self.theta = predict(self.pair_t, self.theta, self.cos_sin, control, sigma3, self.seed, self.step)
        self.cos_sin = np.stack([np.cos(self.theta), np.sin(self.theta)], axis=1)
        self.step += 1

    def weigh(self, pts):
        self.records = np.array([bref.beam_pair(*self.map, pts, self.pair_t[i], self.cos_sin[i], self.beam_table, self.H, self.beyond)[0]
                                 for i in range(self.n)])
        self.w, self.sums = weights(self.records, self.wtable, self.shift)
        W, WW = int(self.sums[SUM_W]), int(self.sums[SUM_WW])
        return (W * W / WW if WW else 0.0), int(self.sums[SUM_OK])

    def resample(self):
        anc, _, status = resample(self.w, self.seed, self.step)
        self.step += 1
        self.pair_t, self.theta, self.cos_sin = self.pair_t[anc], self.theta[anc], self.cos_sin[anc]
        self.w = np.ones(self.n, dtype=np.uint32)
        return anc, status

    def estimate(self):
        return pose_of(estimate(self.w, self.pair_t, self.cos_sin)[0])
