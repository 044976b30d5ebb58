"""NumPy restatement of icpmi_grid_match_moments (include/icpmi.h): the weight of a candidate and the twelve int64 moments
of a score volume about the winner its record names.  Shared by tests/test_grid_moments_cpu.py and
tests/test_grid_moments_gpu.py; it uses nothing of the library."""
import numpy as np

T = np.array([1048576, 961548, 881744, 808563, 741455, 679917, 623487, 571740], dtype=np.int64)
ST_CAPACITY = 2


def weights(scores, best, h):
    d = np.maximum(0, np.int64(best) - np.asarray(scores, dtype=np.int64))
    u = (8 * d) // np.int64(h)
    e, f = u >> 3, u & 7
    return np.where(e > 20, 0, T[f] >> np.minimum(e, 20))


def moments(vol, rec, half_step):
    """vol [A, S, S] int32, rec the eight int32 of the pair's record -> the twelve int64."""
    if rec[0] == ST_CAPACITY:
        return np.zeros(12, dtype=np.int64)
    rows, a0, j0, i0, best = (int(rec[s]) for s in (1, 3, 4, 5, 6))
    w = weights(vol, best, max(1, rows * int(half_step)))
    A, S = vol.shape[:2]
    a, j, i = np.meshgrid(np.arange(A), np.arange(S), np.arange(S), indexing="ij")
    da, dj, di = a - a0, j - j0, i - i0
    face = ((A > 1) & ((a == 0) | (a == A - 1))) | ((S > 1) & ((j == 0) | (j == S - 1) | (i == 0) | (i == S - 1)))
    return np.array([w.sum(), (w * da).sum(), (w * dj).sum(), (w * di).sum(), (w * da * da).sum(), (w * da * dj).sum(),
                     (w * da * di).sum(), (w * dj * dj).sum(), (w * dj * di).sum(), (w * di * di).sum(), (w > 0).sum(), w[face].sum()],
                    dtype=np.int64)
