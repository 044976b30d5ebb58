"""Extended-precision reference of the rotation search's score (features.py:213-218) and the probe construction of
tests/test_rotation_bound_cpu.py / tests/test_rotation_bound_gpu.py.  Nothing here imports the oracle's scoring.

The score of a table entry (c, s) for a pair of voxel-filtered clouds:

    mu_s, mu_t = np.mean(src, axis=0), np.mean(tgt, axis=0)          (float64, as the device record holds them)
    q_i        = ((x_i - mu_s.x) c - (y_i - mu_s.y) s, (x_i - mu_s.x) s + (y_i - mu_s.y) c) + mu_t
    score      = mean_i min_j |q_i - t_j|^2

evaluated in np.longdouble (64-bit mantissa here) from the float64 inputs, the table entries taken as they are.  The
minimum is the brute-force one: a float64 pass only sets aside targets that cannot be it — a target stays a candidate
unless its float64 distance exceeds the smallest by more than CANDIDATE_MARGIN times the rounding of the coordinates —
and ``Pair.score(..., exhaustive=True)`` skips that pass (the CPU test compares the two).

TAU — what a float64 evaluation of the same formula may differ by, relative to the score
------------------------------------------------------------------------------------
u = 2^-53.  S = max_i (|x_i| + |y_i|) of the centred source, Q = max(|mu_t.x|, |mu_t.y|) + rho, rho = max_i |(x_i, y_i)|.
* coordinates: the centring rounds once (u |x|), the two products once each (u (|x c| + |y s|)), their sum once and the
  shift once (u |q|): a coordinate of q is off by at most e_q = u (3 S + Q) (first order), the point by e = sqrt(2) e_q.
  The targets are inputs: exact.  A row's distance d_i moves by at most e, its square by 2 d_i e + e^2; over the rows
  sum 2 d_i e <= 2 e sqrt(n sum d_i^2) (Cauchy-Schwarz), so the score moves by at most (2 r + r^2) relative, with
  r = e / sqrt(score) — coordinate magnitude over distance, with the root-mean-square distance where the smallest one
  would be the cruder (and, for a row that lies on a target point, unbounded) divisor.  The minimum over targets of
  values each within a bound of the true ones is within that bound of the true minimum.
* a row's arithmetic: the two differences (u each, squared: 2 u), the two squares (u), their sum (u), the square root
  (u / 2 on d, u on d^2 ... counted whole: u), d * d (u): (1 + u)^7 — counted as 8 u.
* the sum: a lane of the batch kernel adds ceil(n / 64) terms in sequence, the wave tree adds 6 levels, every add
  rounds once and all terms are non-negative: (ceil(n / 64) + 6) u.  The division by n: u.
* the long-double reference itself: n 2^-63, added so that TAU bounds the distance between the two computations.

    TAU = u (ceil(n / 64) + 6 + 8 + 1) + 2 r + r^2 + n 2^-63

The oracle's float64 scoring adds the n rows in sequence ((n - 1) u in place of the lane-and-tree term): the CPU test
only asks it for the winner of a probe, whose margin is at least 100 TAU, never for a score within TAU.
"""
import numpy as np

try:                                                     # only to propose candidates faster; the answer does not depend on it
    from scipy.spatial import cKDTree
except ImportError:                                      # pragma: no cover
    cKDTree = None

LD = np.longdouble
U = 2.0 ** -53
CANDIDATES = 4
CANDIDATE_MARGIN = 64.0                                  # x u x (coordinate magnitudes): far above the 3 sqrt(2) of the derivation
MAX_DELTA = 0.05                                         # |A - B| of a probe, radians
GRADES = (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 3e-2)

assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"


class Pair:
    """A voxel-filtered pair (float64 (n, 2) and (m, 2) arrays) and its long-double scores."""

    def __init__(self, src, tgt):
        self.src = np.ascontiguousarray(src, dtype=np.float64)
        self.tgt = np.ascontiguousarray(tgt, dtype=np.float64)
        self.n, self.m = len(self.src), len(self.tgt)
        self.mu_s, self.mu_t = np.mean(self.src, axis=0), np.mean(self.tgt, axis=0)
        self.x = self.src[:, 0].astype(LD) - LD(self.mu_s[0])
        self.y = self.src[:, 1].astype(LD) - LD(self.mu_s[1])
        self.tx, self.ty = self.tgt[:, 0].astype(LD), self.tgt[:, 1].astype(LD)
        self.S = float(np.max(np.abs(self.x) + np.abs(self.y)))
        self.rho = float(np.max(np.sqrt(self.x * self.x + self.y * self.y)))
        self.Q = float(np.max(np.abs(self.mu_t))) + self.rho
        self.T = float(np.max(np.abs(self.tgt)))
        self._tree = cKDTree(self.tgt) if cKDTree is not None and self.m > CANDIDATES else None
        self._cache = {}

    def rotated(self, c, s):
        """The rows q_i in long double for the table entry (c, s)."""
        c, s = LD(c), LD(s)
        return self.x * c - self.y * s + LD(self.mu_t[0]), self.x * s + self.y * c + LD(self.mu_t[1])

    def _row_minima(self, qx, qy, rows):
        dx = qx[rows, None] - self.tx[None, :]
        dy = qy[rows, None] - self.ty[None, :]
        return np.min(dx * dx + dy * dy, axis=1)

    def row_d2(self, c, s, exhaustive=False):
        """min_j |q_i - t_j|^2 for every row, long double."""
        qx, qy = self.rotated(c, s)
        k = min(CANDIDATES, self.m)
        if exhaustive or k == self.m:
            out = np.empty(self.n, dtype=LD)
            for i0 in range(0, self.n, 256):                                  # (256 x m long doubles at a time)
                rows = np.arange(i0, min(i0 + 256, self.n))
                out[rows] = self._row_minima(qx, qy, rows)
            return out
        q64 = np.stack([qx.astype(np.float64), qy.astype(np.float64)], axis=1)
        if self._tree is not None:
            d64, idx = self._tree.query(q64, k=k)
        else:
            full = np.sqrt(((q64[:, None, :] - self.tgt[None, :, :]) ** 2).sum(axis=2))
            idx = np.argpartition(full, k - 1, axis=1)[:, :k]
            d64 = np.take_along_axis(full, idx, axis=1)
            o = np.argsort(d64, axis=1)
            d64, idx = np.take_along_axis(d64, o, axis=1), np.take_along_axis(idx, o, axis=1)
        dx = qx[:, None] - self.tx[idx]
        dy = qy[:, None] - self.ty[idx]
        out = np.min(dx * dx + dy * dy, axis=1)
        margin = CANDIDATE_MARGIN * U * (self.S + self.Q + self.T)
        crowded = np.flatnonzero(d64[:, k - 1] - d64[:, 0] <= margin)          # a fifth target could be the nearest: all of them
        if len(crowded):
            out[crowded] = self._row_minima(qx, qy, crowded)
        return out

    def score(self, c, s, exhaustive=False):
        return np.sum(self.row_d2(c, s, exhaustive)) / LD(self.n)

    def score_at(self, angle, exhaustive=False):
        """The score of the table entry NumPy makes of ``angle`` (features.py:214: np.cos / np.sin of the float64)."""
        a = float(angle)
        if exhaustive:
            return self.score(np.cos(a), np.sin(a), True)
        if a not in self._cache:
            self._cache[a] = self.score(np.cos(a), np.sin(a))
        return self._cache[a]

    def tau(self, score):
        """TAU of the module docstring at a score of this pair."""
        r = np.sqrt(2.0) * U * (3.0 * self.S + self.Q) / float(np.sqrt(LD(score)))
        return U * (np.ceil(self.n / 64.0) + 6 + 8 + 1) + 2.0 * r + r * r + self.n * 2.0 ** -63


def _ladder(sign):
    return [sign * MAX_DELTA * 2.0 ** -k for k in range(40, -1, -1)]            # 4.5e-14 ... 0.05


def find_delta(pair, B, eps):
    """delta, |delta| <= MAX_DELTA, with score(B + delta) = score(B) (1 + eps) as nearly as the float64 angle B + delta
    allows and never below: the smallest rung of a doubling ladder at which the score has risen that far brackets a root
    (the score is continuous in the angle), regula falsi (Illinois) closes in on it, and the side above is returned; of
    the two signs the smaller |delta|.  None when neither side rises that far within MAX_DELTA.
    -> (delta, achieved eps) or None."""
    sB = pair.score_at(B)
    want = sB * (LD(1) + LD(eps))
    best = None
    for sign in (1.0, -1.0):
        lo, flo = 0.0, sB - want
        hi = None
        for d in _ladder(sign):
            f = pair.score_at(B + d) - want
            if f > 0:
                hi, fhi, top = d, f, f
                break
            lo, flo = d, f
        if hi is None:
            continue
        side = 0
        for _ in range(80):
            if float(B + lo) == float(B + hi) or top <= want * LD(eps) * LD(1e-11):
                break
            mid = float(lo - (hi - lo) * float(flo / (fhi - flo)))
            if not (min(lo, hi) < mid < max(lo, hi)) or float(B + mid) in (float(B + lo), float(B + hi)):
                mid = 0.5 * (lo + hi)
                if float(B + mid) in (float(B + lo), float(B + hi)):
                    break
            f = pair.score_at(B + mid) - want
            if f > 0:
                hi, fhi, top = mid, f, f
                if side == 1:
                    flo = flo / 2
                side = 1
            else:
                lo, flo = mid, f
                if side == -1:
                    fhi = fhi / 2
                side = -1
        if best is None or abs(hi) < abs(best):
            best = hi
    if best is None:
        return None
    A = float(B + best)
    return A - B, float(pair.score_at(A) / sB - 1)


class Probe:
    """One (pair, B, eps): the second angle A, both long-double scores, the achieved eps and the pair's TAU there."""

    def __init__(self, pair, B, eps, A, achieved):
        self.B, self.eps, self.A, self.achieved = float(B), float(eps), float(A), float(achieved)
        self.sB, self.sA = pair.score_at(B), pair.score_at(A)
        self.tau = pair.tau(self.sB)

    def table(self, b_last):
        """The 16 coarse angles: [A] x 15 + [B], or [B] + [A] x 15."""
        return np.array([self.A] * 15 + [self.B] if b_last else [self.B] + [self.A] * 15)


def probes(pair, angles, grades=GRADES):
    """Every (B, eps) of angles x grades -> (kept [Probe], dropped [(B, eps)]).  A probe is dropped when no delta within
    MAX_DELTA reaches eps, or when the float64 angles are too coarse to land within a factor 2 of it."""
    kept, dropped = [], []
    for B in angles:
        for eps in grades:
            r = find_delta(pair, float(B), eps)
            if r is None or not (0.5 * eps <= r[1] <= 2.0 * eps):
                dropped.append((float(B), eps))
                continue
            kept.append(Probe(pair, B, eps, float(B) + r[0], r[1]))
    return kept, dropped


def grades_for(pair, angles):
    """The grades of GRADES that are at least 100 TAU at every angle of the pair: far from the origin a float64 coordinate
    no longer resolves 1e-9 of a squared distance, and a probe below the resolution of the reference's own inputs would
    test nothing."""
    t = max(pair.tau(pair.score_at(B)) for B in angles)
    return tuple(g for g in GRADES if g >= 100.0 * t)
