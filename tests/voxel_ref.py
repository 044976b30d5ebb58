"""The voxel filter restated in NumPy, and its keys restated in exact arithmetic — TEST INFRASTRUCTURE ONLY.

Written from the contract at the top of csrc/voxel.hip, line by line:

    min_bound = points.min(0)
    key       = floor((p - min_bound) / voxel)     float64 IEEE divide, per axis
    rows      = np.unique(keys, axis=0)            lexicographic order of the keys
    mean      = bincount(weights=p) / bincount     sum taken in INPUT order

``voxel_ref`` is that, ``exact_keys`` says with ``fractions.Fraction`` what "IEEE divide" means: the difference rounded once
to double, the quotient rounded once to double, then the floor.  The wrong models at the end (``KEY_MODELS`` other than
"ieee", ``ORDERS`` other than "input") are variants of this function only; tests/test_voxel_edges_cpu.py uses them to show
that the inputs of tests/voxel_cases.py tell a right filter from a subtly wrong one.  Nothing here touches a GPU.
"""
import math
from fractions import Fraction

import numpy as np

KEY_MODELS = ("ieee", "reciprocal", "float32")
ORDERS = ("input", "reversed", "by_value")


def _keys(p, voxel, model):
    mn = p.min(axis=0)
    if model == "ieee":
        q = (p - mn) / voxel
    elif model == "reciprocal":                    # WRONG: what a fast-math flag makes of the divide
        q = (p - mn) * (1.0 / voxel)
    elif model == "float32":                       # WRONG: the whole key in single precision
        p32 = p.astype(np.float32)
        q = (p32 - p32.min(axis=0)) / np.float32(voxel)
    else:
        raise ValueError(model)
    return np.floor(q).astype(np.int64)


def _sums(p, inverse, n_voxels, order):
    """per-voxel, per-axis sums; np.bincount adds its weights one after the other, in the order of its arguments"""
    out = np.empty((n_voxels, p.shape[1]))
    for d in range(p.shape[1]):
        if order == "input":
            rows = np.arange(len(p))
        elif order == "reversed":                  # WRONG: last member first
            rows = np.arange(len(p))[::-1]
        elif order == "by_value":                  # WRONG: members in ascending order of the coordinate that is summed
            rows = np.argsort(p[:, d], kind="stable")
        else:
            raise ValueError(order)
        out[:, d] = np.bincount(inverse[rows], weights=p[rows, d], minlength=n_voxels)
    return out


def voxel_ref(points, voxel, return_keys=False, return_counts=False, key_model="ieee", order="input"):
    """Means of the voxels of ``points`` (n >= 1 rows, 2 or 3 columns), in lexicographic key order: (m, dim) float64.
    With ``return_keys`` also the (n, dim) int64 key of every point, with ``return_counts`` also the (m,) member counts.
    ``key_model`` / ``order`` other than the defaults give the wrong models named in the module text."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    keys = _keys(p, float(voxel), key_model)
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    counts = np.bincount(inverse, minlength=len(uniq))
    means = _sums(p, inverse, len(uniq), order) / counts[:, None]
    out = (means,)
    if return_keys:
        out += (keys,)
    if return_counts:
        out += (counts,)
    return out if len(out) > 1 else means


def exact_keys(points, voxel):
    """The same keys from exact arithmetic.  Per coordinate: Fraction(p) - Fraction(min) is the exact difference, float()
    rounds it once to the nearest double (the subtraction); that double as a Fraction over Fraction(voxel) is the exact
    quotient, float() rounds it once (the divide); then the floor.  Equal coordinates are worked out once."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    fv = Fraction(float(voxel))
    keys = np.empty(p.shape, dtype=np.int64)
    for d in range(p.shape[1]):
        vals, inverse = np.unique(p[:, d], return_inverse=True)
        fmn = Fraction(float(vals[0]))
        col = np.empty(len(vals), dtype=np.int64)
        for i, x in enumerate(vals):
            diff = float(Fraction(float(x)) - fmn)
            col[i] = math.floor(float(Fraction(diff) / fv))
        keys[:, d] = col[np.asarray(inverse).reshape(-1)]
    return keys


def order_sensitive(points, voxel):
    """(m,) bool: the voxels whose mean changes bits when their members are summed last to first."""
    fwd = voxel_ref(points, voxel)
    rev = voxel_ref(points, voxel, order="reversed")
    return np.any(fwd != rev, axis=1)


def reciprocal_sensitive(points, voxel):
    """(n,) bool: the points that multiply-by-reciprocal keys differently from the IEEE divide."""
    return np.any(_keys(np.ascontiguousarray(points, dtype=np.float64), float(voxel), "ieee")
                  != _keys(np.ascontiguousarray(points, dtype=np.float64), float(voxel), "reciprocal"), axis=1)
