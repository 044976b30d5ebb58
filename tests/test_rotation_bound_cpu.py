"""The probes of the batched rotation search's pruning bound (csrc/rotsearch.hip, rotation_search_batch_kernel), without a
GPU: that they are fair, and what they can and cannot see.

A probe is a pair, an angle B and a second angle A = B + delta whose long-double score is s(B) (1 + eps)
(tests/rotsearch_ref.py); the GPU test launches the search with the coarse table [A] x 15 + [B] (and reversed) and
expects B to win.  If the kernel's lower bound of B exceeded s(A), B would never be scored.  Here:

* every graded eps is at least 100 TAU (the derived float64-against-long-double error of a score), so a float64 kernel
  that sums in any order still has to pick B; the oracle's float64 scoring — another summation order — does;
* at most 5 % of the (geometry, angle, eps) probes are dropped for lack of a delta within 0.05 rad, and every geometry
  keeps a probe at each of its grades;
* a float32 NumPy MODEL of the kernel's steps 2 and 3 (field, look-up, margins) gives the census: the design gap
  s(B) / lb(B) a probe cannot look below, and which of four mutants of the model a probe would expose.  The model is never
  an expected value for the device.

Grades: 1e-9 ... 1e-3 by decades and 3e-2, less those below 100 TAU (20 km from the origin a float64 coordinate resolves
1e-10 of these squared distances: the grades start at 1e-8 and 1e-7 there) and, for ``speck``, those above 1e-6: a centred
cluster in a field that is linear across it keeps its score to first order in the angle (the rows' displacements sum to
zero), and the second order is (rho delta / d)^2 = (1 mm / 0.75 m)^2 = 1.8e-6.
"""
import numpy as np
import pytest

import oracle
import rotsearch_cases as rc
import rotsearch_ref as ref

F = np.float32
W = 64
MUTANTS = ("transposed", "sign", "corner", "no_offset")


def model_origin(pair):
    """The frame of the float32 images: the middle row of the target in its search order — here: sorted along x."""
    return pair.tgt[np.argsort(pair.tgt[:, 0], kind="stable")[pair.m >> 1]]


def model_field(pair, origin):
    """Step 2 of the kernel in float32 NumPy -> (field [W, W], fox, foy, g, shfx, shfy)."""
    t = (pair.tgt - origin).astype(F)
    rt = np.abs(t).max() * F(1.000001)
    c = (pair.src - pair.mu_s).astype(F)
    rho = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]).max()
    H = rho * F(1.00001) + F(1e-3)
    g = F(2.0) * H / F(W)
    shf = (pair.mu_t - origin).astype(F)
    fox, foy = shf[0] - H, shf[1] - H
    k = np.arange(W, dtype=F) + F(0.5)
    cx, cy = fox + k * g, foy + k * g
    mn = np.full((W, W), np.inf, dtype=F)
    for j0 in range(0, pair.m, 256):
        dx = cx[None, :, None] - t[None, None, j0:j0 + 256, 0]
        dy = cy[:, None, None] - t[None, None, j0:j0 + 256, 1]
        mn = np.minimum(mn, (dy * dy + dx * dx).min(axis=2))
    slack = F(1e-5) * (abs(shf[0]) + abs(shf[1]) + F(2.0) * H + rt) + F(1e-6)
    return np.sqrt(mn) * F(0.999999) - slack, fox, foy, g, shf[0], shf[1]


def model_bounds(pair, angles, origin=None, mutant=None):
    """Step 3 in float32 NumPy: the lower bound of the score of every angle (its float64 table entry rounded to float32, as
    the kernel reads it).  ``mutant``: one of MUTANTS — the field read at [jx][jy]; +s for -s in the rotation; the look-up
    grid's corner one cell further on in x and y; the query's offset from the cell centre not subtracted."""
    origin = model_origin(pair) if origin is None else origin
    field, fox, foy, g, shfx, shfy = model_field(pair, origin)
    if mutant == "corner":
        fox, foy = fox + g, foy + g
    inv_g = F(1.0) / g
    c64 = pair.src - pair.mu_s
    x, y = c64[:, 0].astype(F), c64[:, 1].astype(F)
    out = np.empty(len(angles), dtype=F)
    for k, a in enumerate(angles):
        c, s = F(np.cos(a)), F(np.sin(a))
        if mutant == "sign":
            s = -s
        qx, qy = (x * c - y * s) + shfx, (x * s + y * c) + shfy
        jx = np.clip(np.floor((qx - fox) * inv_g).astype(np.int64), 0, W - 1)
        jy = np.clip(np.floor((qy - foy) * inv_g).astype(np.int64), 0, W - 1)
        ox, oy = qx - (fox + (jx.astype(F) + F(0.5)) * g), qy - (foy + (jy.astype(F) + F(0.5)) * g)
        off = np.sqrt(ox * ox + oy * oy) * F(1.000001) + F(1e-5) * (np.abs(qx) + np.abs(qy)) + F(1e-6)
        if mutant == "no_offset":
            off = F(0.0)
        cell = field[jx, jy] if mutant == "transposed" else field[jy, jx]
        L = np.maximum(F(0.0), cell - off)
        out[k] = (L * L).sum(dtype=F) * F(0.9997) / F(pair.n)
    return out


def census(case):
    """What the probes of a case can see -> dict (rows, probes, eps range, design gap, share of probes that catch each
    mutant of the model)."""
    kept, dropped = case.probes
    pair = case.pair
    Bs = sorted({p.B for p in kept})
    lb = dict(zip(Bs, model_bounds(pair, Bs).astype(np.float64)))
    gap = np.array([float(pair.score_at(B)) / lb[B] if lb[B] > 0 else np.inf for B in Bs])
    caught = {}
    for m in MUTANTS:
        mb = dict(zip(Bs, model_bounds(pair, Bs, mutant=m).astype(np.float64)))
        caught[m] = sum(1 for p in kept if mb[p.B] > float(p.sA))
    return dict(n=pair.n, m=pair.m, kept=len(kept), dropped=len(dropped), eps=(min(p.achieved for p in kept), max(p.achieved for p in kept)),
                tau=max(p.tau for p in kept), gap_min=float(gap.min()), gap_median=float(np.median(gap)), caught=caught,
                sound=all(lb[p.B] <= float(p.sB) for p in kept))


def census_line(name, c):
    share = "  ".join(f"{c['caught'][m]:3d}" for m in MUTANTS)
    return (f"  {name:13s} {c['n']:5d} {c['m']:5d}  {c['kept']:3d} {c['dropped']:3d}  {c['eps'][0]:8.2g} {c['eps'][1]:8.2g}  {c['tau']:8.2g}  "
            f"{c['gap_min']:9.4g} {c['gap_median']:9.4g} | {share}")


@pytest.fixture(scope="module")
def table():
    return {name: census(case) for name, case in rc.cases().items()}


def test_the_census(table):
    """The table of DESIGN.md section 5 (-s shows it); the unmutated model's bound stays below every probe's score, and each
    of the four mutants is caught, in the model, by a probe of ``walls`` or ``speck``."""
    print("\n  geometry       rows   tgt  kept drop   eps min  eps max       tau    gap min    median | " + "  ".join(m[:4] for m in MUTANTS))
    for name, c in table.items():
        print(census_line(name, c))
        assert c["sound"], name
    for m in MUTANTS:
        assert table["walls"]["caught"][m] + table["speck"]["caught"][m] >= 1, m


def test_the_probes_are_fair():
    total = dropped = 0
    for name, case in rc.cases().items():
        kept, gone = case.probes
        total += len(kept) + len(gone)
        dropped += len(gone)
        assert len(case.angles) == 12 and len(set(case.angles)) == 12, name
        assert case.grades, name
        for g in case.grades:
            assert any(p.eps == g for p in kept), (name, g)
        for p in kept:
            assert p.achieved >= 100.0 * p.tau and p.eps >= 100.0 * p.tau, (name, p.B, p.eps, p.tau)
            assert 0.5 * p.eps <= p.achieved <= 2.0 * p.eps and abs(p.A - p.B) <= ref.MAX_DELTA, (name, p.B, p.eps)
            assert p.sA > p.sB
    assert dropped <= 0.05 * total, (dropped, total)
    full = [g for g in ref.GRADES]
    assert rc.cases()["room"].grades == tuple(full) and rc.cases()["walls"].grades == tuple(full)
    assert rc.cases()["speck"].grades == tuple(g for g in full if g <= 1e-6)


@pytest.mark.parametrize("name", list(rc.cases()))
def test_float64_scoring_picks_B(name):
    """oracle.rotation_scores (float64, k-d tree, rows added in sequence) on every probe, in both table orders: np.argmin
    names B.  The reference alone stays within the rule the device is held to."""
    case = rc.cases()[name]
    pair = case.pair
    src_c = pair.src - pair.mu_s
    for p in case.probes[0]:
        for b_last in (True, False):
            s = oracle.rotation_scores(src_c, pair.tgt, p.table(b_last), pair.mu_t)
            assert int(np.argmin(s)) == (15 if b_last else 0), (name, p.B, p.eps)
            assert abs(s.min() - float(p.sB)) <= (p.tau + pair.n * ref.U) * float(p.sB), (name, p.B)       # (n - 1) u: its sequential sum


@pytest.mark.parametrize("name", ["room", "walls", "speck", "inside", "dups", "line", "walls_off2e4", "walls_tgt5"])
def test_the_candidate_pass_changes_nothing(name):
    """The long-double score with and without the float64 pass that sets distant targets aside, and with that pass's
    candidates found either way: the same number."""
    case = rc.cases()[name]
    plain = ref.Pair(case.pair.src, case.pair.tgt)
    plain._tree = None                                                  # candidates from the full float64 matrix, not a k-d tree
    for p in case.probes[0][::7]:
        for a in (p.A, p.B):
            assert case.pair.score_at(a) == case.pair.score_at(a, exhaustive=True) == plain.score_at(a), (name, a)


def test_the_means_are_numpy_s():
    """The reference takes np.mean(axis=0) of the filtered clouds (the GPU test holds the record's MUS / MUT to them bit for
    bit): a row-by-row sum divided by the count."""
    pair = rc.cases()["room"].pair
    s = np.zeros(2)
    for row in pair.src:
        s = s + row
    assert np.array_equal(s / pair.n, pair.mu_s)
