"""Synthetic 2-D LiDAR scans of a polygonal world.

The reference ships no sensor logs (``data/*.csv`` is git-ignored there), so
every measurement and parity input in this repo comes from this generator:
a world of wall segments, a 2 048-beam scanner, Gaussian range noise from
``np.random.default_rng(seed)``.  Pure NumPy, host side only.
"""
import numpy as np

# Outer room plus four boxes: (x0, y0, x1, y1) axis-aligned rectangles.
ROOM = (-10.0, -6.0, 10.0, 6.0)
BOXES = (
    (2.0, 1.0, 4.0, 3.0),
    (-6.0, -4.0, -4.0, -1.5),
    (-3.0, 3.0, -1.0, 4.5),
    (5.0, -4.0, 7.5, -3.0),
)


def _rect_segments(r):
    x0, y0, x1, y1 = r
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [(c[i], c[(i + 1) % 4]) for i in range(4)]


def room_segments():
    """(S, 4) array of wall segments ``[ax, ay, bx, by]`` of the single room."""
    segs = _rect_segments(ROOM)
    for b in BOXES:
        segs += _rect_segments(b)
    return np.array([[a[0], a[1], b[0], b[1]] for a, b in segs], dtype=np.float64)


def maze_segments(nx=6, ny=4, cell=10.0, door=2.0, seed=7):
    """A larger multi-room world (≈ ``nx*ny`` rooms of ``cell`` metres) used to
    grow a rolling submap to ~10 k points after voxel filtering (config 3)."""
    rng = np.random.default_rng(seed)
    segs = []
    W, H = nx * cell, ny * cell
    segs += _rect_segments((0.0, 0.0, W, H))
    for i in range(1, nx):            # vertical walls with a door per room
        x = i * cell
        for j in range(ny):
            y0, y1 = j * cell, (j + 1) * cell
            d = y0 + 1.0 + rng.uniform(0, cell - 2.0 - door)
            segs.append(((x, y0), (x, d)))
            segs.append(((x, d + door), (x, y1)))
    for j in range(1, ny):            # horizontal walls with a door per room
        y = j * cell
        for i in range(nx):
            x0, x1 = i * cell, (i + 1) * cell
            d = x0 + 1.0 + rng.uniform(0, cell - 2.0 - door)
            segs.append(((x0, y), (d, y)))
            segs.append(((d + door, y), (x1, y)))
    for i in range(nx):               # one pillar per room
        for j in range(ny):
            cx = i * cell + rng.uniform(2.5, cell - 2.5)
            cy = j * cell + rng.uniform(2.5, cell - 2.5)
            s = rng.uniform(0.4, 1.2)
            segs += _rect_segments((cx - s, cy - s, cx + s, cy + s))
    return np.array([[a[0], a[1], b[0], b[1]] for a, b in segs], dtype=np.float64)


def cast_ranges(segs, pose, n_beams=2048):
    """Exact ranges from ``pose=(x, y, theta)`` to the nearest wall per beam.

    Beam angles are ``theta + linspace(-pi, pi, n_beams, endpoint=False)``.
    Beams that hit nothing get ``inf``.
    """
    x, y, th = pose
    ang = th + np.linspace(-np.pi, np.pi, n_beams, endpoint=False)
    dx, dy = np.cos(ang)[:, None], np.sin(ang)[:, None]          # (B,1)
    ax, ay = segs[None, :, 0] - x, segs[None, :, 1] - y           # (1,S)
    ex, ey = segs[None, :, 2] - segs[None, :, 0], segs[None, :, 3] - segs[None, :, 1]
    den = dx * ey - dy * ex
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (ax * ey - ay * ex) / den                             # along the beam
        u = (ax * dy - ay * dx) / den                             # along the wall
    ok = (np.abs(den) > 1e-12) & (t > 1e-9) & (u >= 0.0) & (u <= 1.0)
    t = np.where(ok, t, np.inf)
    return t.min(axis=1), ang


def scan(pose, seed, n_beams=2048, noise=0.01, segs=None):
    """One scan in the SENSOR frame: ``(n_beams, 2) float64``."""
    if segs is None:
        segs = room_segments()
    rng = np.random.default_rng(seed)
    r, ang = cast_ranges(segs, pose, n_beams)
    r = r + rng.normal(0.0, noise, size=n_beams)
    keep = np.isfinite(r)
    a_local = ang - pose[2]
    pts = np.stack([r * np.cos(a_local), r * np.sin(a_local)], axis=1)
    return np.ascontiguousarray(pts[keep])


def to_world(pts, pose):
    """Sensor-frame points -> world frame for ``pose=(x, y, theta)``."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    R = np.array([[c, -s], [s, c]])
    return pts @ R.T + np.array([pose[0], pose[1]])


def config2_pair(seed=0):
    """BASELINE config 2: scans at (0,0,0) and (0.15,-0.08,3 deg)."""
    a = scan((0.0, 0.0, 0.0), seed)
    b = scan((0.15, -0.08, np.deg2rad(3.0)), seed + 1)
    return a, b


def _free_pose(x, y, clearance=0.25):
    """Inside the room and not inside (or within `clearance` of) one of its boxes."""
    if not (ROOM[0] + clearance < x < ROOM[2] - clearance and ROOM[1] + clearance < y < ROOM[3] - clearance):
        return False
    return not any(b[0] - clearance < x < b[2] + clearance and b[1] - clearance < y < b[3] + clearance for b in BOXES)


def loop_closure_batch(n_pairs, seed0=1000, shared_source=False, max_offset=0.6, max_yaw_deg=6.0):
    """Candidate scan pairs of a loop closure (BASELINE config 5): the target pose lies within ``max_offset`` metres
    (uniform distance, uniform direction) and ``max_yaw_deg`` degrees (uniform) of the source pose.

    The defaults, 0.6 m / 6 deg, are offsets ICP converges from WITHOUT pre-alignment (the `ICP iterations/s` batches of
    bench.py).  SURVEY section 8d / config.yaml:70 describe the candidates the reference gates — within 3 m / 20 deg:
    ``max_offset=3.0, max_yaw_deg=20.0``; those are only reachable through the rotation search of _run_icp_pair
    (icpmi.prealign), which is exactly why the reference pre-aligns."""
    srcs, tgts = [], []
    base = (0.5, -0.3, 0.1)
    src_shared = scan(base, seed0 - 1)
    for i in range(n_pairs):
        rng = np.random.default_rng(seed0 + i)
        while True:                          # a sensor cannot stand inside a box or a wall: such draws are taken again
            d = rng.uniform(0.0, max_offset)
            a = rng.uniform(-np.pi, np.pi)
            th = np.deg2rad(rng.uniform(-max_yaw_deg, max_yaw_deg))
            pose_t = (base[0] + d * np.cos(a), base[1] + d * np.sin(a), base[2] + th)
            if _free_pose(pose_t[0], pose_t[1]):
                break
        srcs.append(src_shared if shared_source else scan(base, seed0 + 7919 * (i + 1)))
        tgts.append(scan(pose_t, seed0 + i))
    return srcs, tgts


def trajectory(n, start=(5.0, 5.0, 0.0), step=0.25, segs=None, seed=3):
    """A smooth drive through the maze world: list of poses."""
    rng = np.random.default_rng(seed)
    poses = []
    x, y, th = start
    for _ in range(n):
        poses.append((x, y, th))
        th += rng.normal(0.0, 0.03)
        x += step * np.cos(th)
        y += step * np.sin(th)
    return poses


def loop_trajectory(n, center=(25.0, 15.0), radius=3.2, laps=1.2):
    """A closed circuit (counter-clockwise circle, heading along the tangent) that overlaps itself after one
    lap, for loop closures.  The default sits in a room of ``maze_segments()`` clear of its pillar."""
    poses = []
    for k in range(n):
        a = 2.0 * np.pi * laps * k / max(n - 1, 1)
        poses.append((center[0] + radius * np.cos(a), center[1] + radius * np.sin(a), a + np.pi / 2.0))
    return poses


# ── 3-D inputs (the (n, 3) path of ICP / IcpBatch and the reference's run_icp odometry) ─────────────────────────
ROOM3D = (-5.0, -4.0, 0.0, 5.0, 4.0, 3.0)        # x0, y0, z0, x1, y1, z1: floor, ceiling, four walls
BOXES3D = (
    (1.0, 0.5, 0.0, 2.2, 1.5, 1.1),
    (-3.5, -2.5, 0.0, -2.3, -1.0, 0.8),
    (-1.0, 2.2, 0.0, 0.4, 3.2, 1.9),
)


def rot3(rx, ry, rz):
    """Rz(rz) @ Ry(ry) @ Rx(rx), angles in radians."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


def lattice3d(n, seed, spacing=1.0, jitter=0.2):
    """The first ``n`` nodes (x-major order) of a cubic lattice, each moved by a uniform jitter of at most
    ``jitter * spacing`` per axis.  Distinct nodes differ by at least ``(1 - 2 jitter) spacing`` along some axis, so
    a voxel filter finer than that keeps every point: the filtered count is exactly ``n``."""
    k = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((g + rng.uniform(-jitter, jitter, size=(n, 3))) * spacing)


def _box_faces(b, rng, n):
    """n points uniform on the surface of the axis-aligned box b = (x0, y0, z0, x1, y1, z1)."""
    lo, hi = np.array(b[:3]), np.array(b[3:])
    ext = hi - lo
    areas = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = lo + rng.uniform(0.0, 1.0, size=(n, 3)) * ext
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = np.where(side == 1, hi[axis], lo[axis])
    return p


def room3d_world(n, seed, noise=0.01):
    """n surface points of a furnished room (world frame): the room's six faces and three boxes, Gaussian noise."""
    rng = np.random.default_rng(seed)
    parts = [ROOM3D] + list(BOXES3D)
    share = np.array([0.7, 0.1, 0.1, 0.1])
    counts = np.floor(share * n).astype(int)
    counts[0] += n - counts.sum()
    p = np.vstack([_box_faces(b, rng, c) for b, c in zip(parts, counts)])
    return p + rng.normal(0.0, noise, size=p.shape)


def scan3d(pose, seed, n=3000, noise=0.01):
    """One 3-D scan in the SENSOR frame of ``pose = (R (3, 3), t (3,))``: room points within 6 m of the sensor."""
    R, t = pose
    w = room3d_world(n, seed, noise)
    w = w[np.linalg.norm(w - t, axis=1) < 6.0]
    return np.ascontiguousarray((w - t) @ R)


def trajectory3d(n, step=0.2, yaw_step=np.deg2rad(2.0)):
    """A slow drive across the room at sensor height 1.2 m with a gentle pitch and roll: list of (R, t)."""
    out = []
    for k in range(n):
        R = rot3(np.deg2rad(0.5 * np.sin(k)), np.deg2rad(0.4 * np.cos(k)), -0.3 + yaw_step * k)
        out.append((R, np.array([-2.0 + step * k, -0.5 + 0.05 * k, 1.2 + 0.01 * k])))
    return out


def _tetrahedron():
    return np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])


def _fibonacci_sphere(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(1.0 - z * z)
    a = np.pi * (3.0 - np.sqrt(5.0)) * k
    return np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)


def icp3d_cases(teapot):
    """The 3-D registrations of tests/golden/icp3d.npz: name -> (source, target, ICP keyword arguments).

    ``teapot`` is the reference's teapot.csv (418 x 3; tests/golden/icp.npz holds it).  Lattice cases put the
    source counts around every branch of the 3-D ICP kernel (N mod 2048 in each quarter of a pass, several passes)
    and the target counts around its 2 048-row LDS tile; the small clouds make the cross-covariance W rank 0, 1
    or 2, mirrored, or with repeated singular values."""
    cases = {}
    lat = dict(error_threshold=1e-10, max_iterations=100, voxel_size=0.05)
    Rm, tm = rot3(0.02, -0.015, 0.03), np.array([0.12, -0.08, 0.05])
    for k, (n, m) in enumerate(((1200, 2048), (1800, 6000), (2348, 2048), (2848, 2049), (3900, 1500), (5396, 6000))):
        src = lattice3d(n, 100 + k) @ Rm.T + tm
        cases[f"lat_n{n}_m{m}"] = (src, lattice3d(m, 200 + k), dict(lat))
    # near ties across the boundary of two target tiles: targets are the plain 13^3 lattice (rows 2047 and 2048 are
    # the neighbours (12, 1, 6) and (12, 1, 7)); the sources sit 1e-7 off the midpoints of such z neighbours, on
    # either side (exact ties are left out: the reference's k-d tree breaks them by its tree, not by index)
    g = lattice3d(13 ** 3, 0, jitter=0.0)
    mids = g[[2047, 2046, 30, 1000, 2100]] + np.array([0.0, 0.0, 0.5])
    mids[:, 2] += np.array([1e-7, -1e-7, 1e-7, -1e-7, 1e-7])
    cases["tile_near_tie"] = (mids, g, dict(lat))
    # the teapot (icp.npz "teapot": Ry(25 deg), t = (0.25, 0.05, 0) undone)
    ang = np.radians(25.0)
    Ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    moved = teapot @ Ry.T + np.array([0.25, 0.05, 0.0])
    tp = dict(error_threshold=1e-12, max_iterations=300, voxel_size=0.005)
    Ri, ti = rot3(0.05, -0.3, 0.02), np.array([-0.2, -0.03, 0.05])
    cases["teapot_init"] = (moved, teapot, dict(tp, R_init=Ri, t_init=ti))
    cases["teapot_Ronly"] = (moved, teapot, dict(tp, R_init=Ri))
    cases["teapot_corr"] = (moved, teapot, dict(tp, max_corr_dist=0.08))
    cases["teapot_break0"] = (moved, teapot + np.array([30.0, 0.0, 0.0]), dict(tp, max_corr_dist=0.05))
    cases["teapot_maxit5"] = (moved, teapot, dict(tp, max_iterations=5))
    # break at iteration 1: 12 of 100 correspondences are inliers at first, the step then pushes 5 of them out
    rng = np.random.default_rng(31)
    gx, gy, gz = np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(4.0), indexing="ij")
    bsrc = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1) + rng.uniform(-0.1, 0.1, size=(100, 3))
    perm = rng.permutation(100)
    btgt = bsrc.copy()
    btgt[perm[:7]] += [0.05, 0.0, 0.0]
    btgt[perm[7:12]] -= [0.05, 0.0, 0.0]
    btgt[perm[12:]] += [0.0, 0.0, 30.0]
    cases["breakN"] = (bsrc, btgt, dict(error_threshold=1e-10, max_iterations=150, voxel_size=0.005, max_corr_dist=0.055))
    # geometry of W
    geo = dict(error_threshold=1e-12, max_iterations=100, voxel_size=1e-4)
    rng = np.random.default_rng(32)
    pl = np.column_stack([rng.uniform(-1, 1, size=(300, 2)), np.zeros(300)])
    cases["planar_z0"] = (pl, pl @ rot3(0.0, 0.0, np.deg2rad(12.0)).T + np.array([0.05, -0.03, 0.0]), dict(geo))
    B = rot3(0.4, -0.7, 1.1)
    tilt = rng.uniform(-1, 1, size=(300, 2)) @ B[:, :2].T + np.array([0.3, -0.1, 0.7])
    cases["tilted_plane"] = (tilt, tilt @ rot3(0.05, 0.1, -0.08).T + np.array([0.02, 0.04, -0.03]), dict(geo))
    an = rng.normal(size=(200, 3)) * np.array([3.0, 2.0, 1.0])
    cases["mirrored"] = (an, an * np.array([1.0, 1.0, -1.0]) + np.array([0.1, 0.0, 0.0]), dict(geo))
    cube = np.stack(np.meshgrid([-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0], indexing="ij"), -1).reshape(-1, 3)
    cases["cube"] = (cube, cube @ rot3(0.1, 0.2, 0.15).T + np.array([0.1, -0.2, 0.05]), dict(geo))
    cases["tetrahedron"] = (_tetrahedron(), _tetrahedron() @ rot3(-0.2, 0.1, 0.25).T + np.array([0.0, 0.1, 0.2]), dict(geo))
    sph = _fibonacci_sphere(200)
    cases["sphere"] = (sph, sph @ rot3(0.03, -0.04, 0.05).T + np.array([0.01, 0.0, -0.02]), dict(geo))
    lx = np.column_stack([np.linspace(0.0, 3.0, 20), np.zeros(20), np.zeros(20)])
    cases["line_x"] = (lx, lx + np.array([0.05, 0.0, 0.0]), dict(geo))
    d = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    e = np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
    a = np.linspace(-2.0, 3.0, 25)
    cases["line_general"] = (a[:, None] * d, a[:, None] * e + np.array([0.4, 0.1, -0.3]), dict(geo))
    cases["single_point"] = (np.array([[0.3, -0.2, 0.5]]), lattice3d(50, 9) * 0.2, dict(geo))
    return cases


# Cases whose W has rank <= 1 in some iteration: the optimal rotation is not unique there.
ICP3D_RANK_DEFICIENT = ("line_x", "line_general", "single_point")


def odometry3d_stream(n_scans=7):
    """(timestamp, points) scans along trajectory3d for the reference's legacy run_icp odometry."""
    return [(f"{k:04d}", scan3d(p, 300 + k)) for k, p in enumerate(trajectory3d(n_scans))]
