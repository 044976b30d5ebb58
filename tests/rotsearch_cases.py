"""The geometries of the rotation-bound probes (tests/test_rotation_bound_cpu.py, tests/test_rotation_bound_gpu.py).

Deterministic, a few hundred rows unless a size edge says otherwise.  The designed clouds put ONE point into every voxel
they occupy (``on_cells``), so the voxel filter keeps every row and the filtered counts are the designed ones; ``room`` is
an ordinary scan pair, and a designed cloud that is turned or carried far away may merge a few rows (its count is then
whatever the pinned filter of the oracle gives — the GPU test compares NS / NT with that in every case).

* room   — synth.config2_pair(9): the generic case.
* walls  — the target a 16 m wall, two voxels thick, with a short stub at one end; the source a wall of the same length
           laid out at -31 degrees, so that B = +31 degrees aligns it and at most other angles its ends stick out by
           metres: the field's gradient is large, different in x and y, and different at B and -B.
* speck  — the target an L of two 3 m arms with its corner at the upper right, the source a cluster within 2 cm of its
           mean, which the search carries to the L's mean on the diagonal: 0.75 m below one arm and left of the other.
           The field half side is 2 cm, its cells 0.7 mm; the triangle term is below 1e-3 of a distance and only the float32
           margins separate bound and score.  The field is linear across the cluster and the rows' displacements under a
           turn sum to zero, so the score is stationary in the angle to first order; the second order is
           (rho delta / d)^2 <= (1 mm / 0.75 m)^2 = 1.8e-6: this geometry is graded up to 1e-6 (``top_grade``).
* inside — the source inside a dense lattice target: most bounds clamp to 0.
* dups   — a target of points repeated four times.
* line   — a collinear target (one y for every row).
* frames — room and walls turned by 45, 90, 135 degrees (the prepare kernel's four projections), carried to (35, -20) m and to
           (2e4, -3e4) m (float32 images about the middle target row; mu_t - origin rounded to float32).
* sizes  — on walls: 5, 63, 64, 65, 129 source rows (the stride-64 row loop, the first partial-sum give-up), 5, 16, 17, 33
           target rows (the box hierarchy's blocks of 16), 2 048 / 2 048 rows (the workgroup's capacity; one grade), and a
           pair above its capacity hint, which must report ICPMI_RSB_ST_CAPACITY and no winner.
"""
import functools

import numpy as np

import oracle
import rotsearch_ref as ref
from icpmi import synth

VOXEL = 0.3


def on_cells(cells, voxel, seed):
    """One point in every voxel of ``cells`` (distinct integer pairs): voxel x (cell + f), f = 0.2 in the lowest row and
    column (the filter's keys are floor((p - min) / voxel), min the cloud's own) and within [0.3, 0.7] elsewhere."""
    cells = np.asarray(cells, dtype=np.int64)
    assert len(np.unique(cells, axis=0)) == len(cells)
    f = np.random.default_rng(seed).uniform(0.3, 0.7, size=cells.shape)
    for d in (0, 1):
        f[cells[:, d] == cells[:, d].min(), d] = 0.2
    return voxel * (cells + f)


def moved(cloud, deg=0.0, offset=(0.0, 0.0)):
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return np.ascontiguousarray(cloud @ R.T + np.asarray(offset, dtype=np.float64))


def _spread(cells, n):
    """n of the cells, evenly through their order, both ends kept."""
    return cells[np.round(np.linspace(0, len(cells) - 1, n)).astype(np.int64)]


def _wall_cells(length, stub=True):
    wall = [(i, j) for i in range(length) for j in (0, 1)]
    if stub:
        wall += [(i, j) for i in (length - 8, length - 7) for j in range(2, 12)]
    return np.array(wall)


def _slanted_cells(length):
    """A wall two cells thick at atan(-0.6) = -30.96 degrees."""
    return np.array([(i, int(np.round(-0.6 * i)) + j) for i in range(length) for j in (0, 1)])


class Case:
    def __init__(self, name, src, tgt, voxel=VOXEL, designed=None, hint=0, top_grade=None, only_grade=None):
        self.name, self.voxel, self.designed, self.hint = name, float(voxel), designed, int(hint)
        self.src, self.tgt = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
        self.top_grade, self.only_grade = top_grade, only_grade

    @functools.cached_property
    def pair(self):
        """The long-double reference on the clouds the pinned voxel filter leaves."""
        p = ref.Pair(oracle.voxel_downsample(self.src, self.voxel), oracle.voxel_downsample(self.tgt, self.voxel))
        if self.designed is not None:
            assert (p.n, p.m) == self.designed, (self.name, p.n, p.m, self.designed)
        return p

    @functools.cached_property
    def field_half_side(self):
        """H of the kernel's field: rho x 1.00001 + 1e-3 in float32, rho the largest float32 radius of a centred row."""
        c = (self.pair.src - self.pair.mu_s).astype(np.float32)
        rho = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]).max()
        return np.float32(rho * np.float32(1.00001) + np.float32(1e-3))

    @functools.cached_property
    def angles(self):
        """Twelve values of B: 0, +-90, +-180 degrees, three generic ones (31 aligns the walls), and both sides of two
        cell borders of the field: the centred row of largest radius r at phase phi has q.x - mu_t.x = r cos(B + phi)
        and q.y - mu_t.y = r sin(B + phi); the borders are at -H + j g, g = 2 H / 64; column border 40 is reached at
        B = acos(0.25 H / r) - phi, row border 24 at B = asin(-0.25 H / r) - phi.  1e-7 rad to either side is within the
        float32 rounding of q (2^-24 of a coordinate)."""
        c = self.pair.src - self.pair.mu_s
        r = np.hypot(c[:, 0], c[:, 1])
        i = int(np.argmax(r))
        phi, H = np.arctan2(c[i, 1], c[i, 0]), float(self.field_half_side)
        bx = np.arccos(0.25 * H / r[i]) - phi
        by = np.arcsin(-0.25 * H / r[i]) - phi
        wrap = lambda a: float((a + np.pi) % (2 * np.pi) - np.pi)
        fixed = [np.deg2rad(d) for d in (0.0, 90.0, -90.0, 180.0, -180.0, 31.0, 7.0, 120.0)]
        return tuple(float(a) for a in fixed) + tuple(wrap(b + e) for b in (bx, by) for e in (-1e-7, 1e-7))

    @functools.cached_property
    def grades(self):
        g = ref.grades_for(self.pair, self.angles)
        if self.top_grade is not None:
            g = tuple(x for x in g if x <= self.top_grade)
        if self.only_grade is not None:
            g = tuple(x for x in g if x == self.only_grade)
        return g

    @functools.cached_property
    def probes(self):
        """(kept, dropped) of rotsearch_ref.probes, once per process."""
        return ref.probes(self.pair, self.angles, self.grades)


def _room():
    a, b = synth.config2_pair(9)
    return a, b


def _walls(voxel=0.125, length=128, n_src=None, n_tgt=None, stub=True, src_length=None):
    sc, tc = _slanted_cells(src_length or length - 18), _wall_cells(length, stub)
    if n_src is not None:
        sc = _spread(sc, n_src)
    if n_tgt is not None:
        tc = _spread(tc, n_tgt)
    return on_cells(sc, voxel, 11), on_cells(tc, voxel, 12) + np.array([-0.5 * length * voxel, 0.0]), (len(sc), len(tc))


def _speck():
    voxel = 0.0036
    tgt = np.array([(x, 3.0) for x in np.arange(0.0, 3.0, 0.05)] + [(3.0, y) for y in np.arange(0.0, 3.0, 0.05)])
    tgt = tgt + np.random.default_rng(21).uniform(-0.004, 0.004, size=tgt.shape)             # rows 0.05 m apart: a voxel each
    cells = np.array([(i, j) for i in range(-5, 6) for j in range(-5, 6) if (i * i + j * j) * 0.004 ** 2 <= 0.0185 ** 2])
    rng = np.random.default_rng(22)
    src = 0.004 * cells + rng.uniform(-0.0001, 0.0001, size=cells.shape) + np.array([1.0, -2.0])   # pitch 1.11 voxels: a voxel each
    assert np.hypot(*(src - src.mean(axis=0)).T).max() < 0.02
    return src, tgt, voxel, (len(src), len(tgt))


def _inside():
    tc = np.array([(i, j) for i in range(20) for j in range(20)])
    sc = np.array([(i, j) for i in range(5, 15) for j in range(5, 15)])
    return on_cells(sc, VOXEL, 31) + np.array([0.11, -0.07]), on_cells(tc, VOXEL, 32), (100, 400)


def _dups():
    rng = np.random.default_rng(41)
    tc = rng.permutation(np.array([(i, j) for i in range(24) for j in range(24)]))[:120]
    sc = rng.permutation(np.array([(i, j) for i in range(20) for j in range(20)]))[:90]
    return on_cells(sc, VOXEL, 42), np.repeat(on_cells(tc, VOXEL, 43), 4, axis=0), (90, 120)


def _line():
    tgt = on_cells(np.array([(i, 0) for i in range(80)]), VOXEL, 51)
    tgt[:, 1] = 1.0
    sc = np.array([(i, 0) for i in range(40)] + [(0, j) for j in range(1, 31)])
    return on_cells(sc, VOXEL, 52), tgt, (70, 80)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order."""
    out = {}

    def add(name, src, tgt, **kw):
        out[name] = Case(name, src, tgt, **kw)

    rs, rt = _room()
    ws, wt, wd = _walls()
    add("room", rs, rt)
    add("walls", ws, wt, voxel=0.125, designed=wd)
    ss, st, sv, sd = _speck()
    add("speck", ss, st, voxel=sv, designed=sd, top_grade=1e-6)
    s, t, d = _inside()
    add("inside", s, t, designed=d)
    s, t, d = _dups()
    add("dups", s, t, designed=d)
    s, t, d = _line()
    add("line", s, t, designed=d)
    for deg in (45, 90, 135):
        add(f"room_rot{deg}", moved(rs, deg), moved(rt, deg))
        add(f"walls_rot{deg}", moved(ws, deg), moved(wt, deg), voxel=0.125)
    for tag, off in (("off35", (35.0, -20.0)), ("off2e4", (2e4, -3e4))):
        add(f"room_{tag}", moved(rs, 0.0, off), moved(rt, 0.0, off))
        add(f"walls_{tag}", moved(ws, 0.0, off), moved(wt, 0.0, off), voxel=0.125)
    for n in (5, 63, 64, 65, 129):
        s, t, d = _walls(n_src=n)
        add(f"walls_src{n}", s, t, voxel=0.125, designed=d)
    for m in (5, 16, 17, 33):
        s, t, d = _walls(n_tgt=m)
        add(f"walls_tgt{m}", s, t, voxel=0.125, designed=d)
    s, t, d = _walls(voxel=1.0 / 64, length=1024, stub=False, src_length=1024)
    add("walls_2048", s, t, voxel=1.0 / 64, designed=(2048, 2048), only_grade=1e-6)
    return out


FRAMES = tuple(f"{g}_rot{d}" for g in ("room", "walls") for d in (45, 90, 135))
CARRIED = tuple(f"{g}_{t}" for t in ("off35", "off2e4") for g in ("room", "walls"))


def capacity_case():
    """walls with a capacity hint of 64 rows: 220 and 276 filtered rows do not fit."""
    ws, wt, wd = _walls()
    return Case("walls_hint64", ws, wt, voxel=0.125, designed=wd, hint=64)
