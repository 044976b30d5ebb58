"""What the three buffer-end modules share (tests/test_buffer_ends_{grid,particles,clouds}_gpu.py and, for the sizes and the
refusals, tests/test_buffer_ends_cpu.py): a case builds every device buffer of one call in a ``tests/arena.py`` arena, each
exactly as large as include/icpmi.h states, and the runner holds the call to three things — nothing outside a buffer is
written, the outputs are the same bits whatever the guards and the scratch held, and the outputs are right.

A case is a function ``build(b)`` over a ``Built``: it places the buffers, sets ``b.call`` and says what to compare.  It
runs on a CPU arena as well — nothing is launched there; the CPU module reads ``b.sized`` (every buffer whose size is a
query of the header) and calls ``b.call(short=name)`` for the refusals an entry decides before its first HIP call.

Reads outside a buffer that never reach a result — a load whose value is masked away — cannot be seen by this method.
"""
import numpy as np
import torch

import arena as ar
from arena import INPUT, OUTPUT, SCRATCH, STATE            # noqa: F401  (the case modules take them from here)

ERR_HIP = -3
ROOM = 4096                                               # what a roomy twin adds to every queried size


class Case:
    def __init__(self, id, build, capacity=8 << 20):
        self.id, self.build, self.capacity = id, build, capacity

    def __repr__(self):
        return self.id


class Built:
    """One case in one arena.  ``roomy``: the twin — every queried size gets ROOM bytes more, and the runner surrounds
    everything with zeros, as the Python layer's fresh allocations mostly are."""

    def __init__(self, arena, L, roomy=False):
        self.arena, self.L, self.roomy = arena, L, roomy
        self.sized = {}                # name -> (query name, its arguments, the refusal of one byte less, decided on the host)
        self.outputs = {}              # name -> boolean mask of the elements the header says are written (None: all)
        self.untouched = {}            # name -> boolean mask of the elements the header says are NOT written
        self.expected = None           # () -> {name: array}: the restatement's outputs
        self.twin = ()                 # names compared with the roomy twin instead
        self.after = None              # (pattern) -> None: further requirements after a run
        self.call = None               # (short=None) -> return code
        self.on_gpu = arena.device.type == "cuda"

    def place(self, a, name, role=None, **kw):
        return self.arena.place(a, name, role, **kw)[1]

    def out(self, shape, dtype, name, mask=None, untouched=None, role=OUTPUT):
        """An output of ``shape`` and ``dtype``, pre-filled with the pattern."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.arena.place(n, name, role, dtype=np.dtype(dtype).name)[1]
        r = self.arena.regions[name]
        r.shape = tuple(shape)
        self.outputs[name] = mask
        if untouched is not None:
            self.untouched[name] = untouched
        return p

    def query(self, name, query, args, refusal=None, host=True, role=SCRATCH, zeros=False, **kw):
        """The buffer ``name`` of exactly ``L.<query>(*args)`` bytes -> its pointer.  ``refusal``: what the entry returns
        for one byte less (ICPMI_ERR_WORKSPACE unless said; 0: the entry takes no byte count), ``host``: whether it decides so
        before its first HIP call.  ``zeros``: the contract asks the caller for a zeroed buffer (role STATE)."""
        need = int(getattr(self.L, query)(*args))
        assert need > 0, f"{query}{args} is 0: the case is refused"
        self.sized[name] = (query, tuple(args), -2 if refusal is None else refusal, host)
        n = need + (ROOM if self.roomy else 0)
        return self.place(np.zeros(n, dtype=np.uint8), name, STATE, **kw) if zeros else self.place(n, name, role, **kw)

    def size(self, name, short=None):
        """The byte count to hand the entry for ``name``: what was placed, one less when the refusal is being tested."""
        return self.arena.nbytes(name) - (1 if short == name else 0)

    def sync(self):
        if self.on_gpu:
            torch.cuda.synchronize()

    def stream(self):
        import ctypes as C
        return C.c_void_p(torch.cuda.current_stream().cuda_stream if self.on_gpu else 0)


def host(a):
    """A host array as the void* of a ``*_host`` parameter (the caller keeps ``a`` alive)."""
    import ctypes as C
    return C.c_void_p(a.ctypes.data)


def same_bits(a, b, mask=None):
    a, b = (np.ascontiguousarray(v if mask is None else v[np.broadcast_to(mask, v.shape)]) for v in (a, b))
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


def _runs(b, patterns):
    got = []
    for pattern in patterns:
        b.arena.poison(pattern)
        b.sync()
        try:
            rc = b.call()
            b.sync()
        except RuntimeError as e:                                  # a HIP error out of torch: the device may have faulted
            rc, why = ERR_HIP, str(e)
        else:
            why = f"the call returned {rc}"
        if rc == ERR_HIP:
            import pytest
            pytest.exit(f"{why} under pattern {pattern:#x}: nothing more is started on the GPU", returncode=3)
        assert rc == 0, f"the call returned {rc} under pattern {pattern:#x}"
        bad = b.arena.check()
        assert not bad, f"written outside a buffer under pattern {pattern:#x}: {bad}"
        for name, mask in b.untouched.items():
            assert b.arena.holds_pattern(name, mask), f"{name}: elements the header leaves unwritten were written"
        if b.after is not None:
            b.after(pattern)
        got.append({name: b.arena.read(name) for name in b.outputs})
    return got


def run(case, L, device="cuda"):
    """The runner of the three GPU modules: pattern A, check, pattern B in the same arena, check, both runs bit-equal, the
    outputs equal to the reference."""
    b = Built(ar.Arena(device, case.capacity), L)
    case.build(b)
    first, second = _runs(b, ar.PATTERNS)
    for name, mask in b.outputs.items():
        assert same_bits(first[name], second[name], mask), f"{name} depends on what the guards and the scratch held"
    want = dict(b.expected()) if b.expected is not None else {}
    if b.twin:
        t = Built(ar.Arena(device, case.capacity + 64 * ROOM), L, roomy=True)
        case.build(t)
        roomy = _runs(t, (0,))[0]
        want.update({name: roomy[name] for name in b.twin})
    assert set(want) == set(b.outputs), f"no reference for {set(b.outputs) - set(want)}"
    for name, mask in b.outputs.items():
        w = np.asarray(want[name]).reshape(first[name].shape).astype(first[name].dtype, copy=False)
        if not same_bits(first[name], w, mask):
            m = np.ones(w.shape, bool) if mask is None else np.broadcast_to(mask, w.shape)
            differ = np.argwhere(m & ~((first[name] == w) | ((first[name] != first[name]) & (w != w))))
            raise AssertionError(f"{name} differs from the reference at {differ[:4].tolist()} ({len(differ)} elements)")
    print(f"{case.id}: guards intact, {b.arena.watched_bytes()} bytes watched")
    return b


def build_on_cpu(case, L):
    b = Built(ar.Arena("cpu", case.capacity), L)
    case.build(b)
    return b


# ── inputs the grid and the particle cases share ─────────────────────────────
GRIDS = ((1, 1), (1, 7), (3, 3), (4, 32), (5, 33), (2, 65), (37, 53), (65, 129))
ROW_SETS = ((17, 1), (257, 255), (2049, 15))
THRESHOLD = 2048
RES, MIN_X, MIN_Y = 0.25, -3.0, -2.0


def field_of(ny, nx, seed=0):
    """An int16 (ny, nx) field with walls, free space (7), unknown cells (0) and single occupied cells; the last column — a
    row's last word — a wall."""
    rng = np.random.default_rng(50 + seed + 131 * ny + nx)
    f = np.full((ny, nx), 7, dtype=np.int16)
    f[rng.random((ny, nx)) < 0.15] = 0
    f[rng.random((ny, nx)) < 0.05] = 32767
    f[rng.random((ny, nx)) < 0.05] = -900
    f[:, nx - 1] = np.array([THRESHOLD, 32767, THRESHOLD - 1], dtype=np.int16)[rng.integers(0, 3, size=ny)]
    return f


def clouds_of(rows, ny, nx, seed=0):
    """Sensor-frame 2-D clouds of ``rows`` rows whose points, under the poses of ``poses_of``, fall in and around the grid."""
    rng = np.random.default_rng(70 + seed + sum(rows))
    span = max(nx, ny) * RES
    out = []
    for n in rows:
        ang, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.05, 0.8 * span, n)
        p = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
        p[::4] = np.rint(p[::4] / RES) * RES
        out.append(p)
    return out


def poses_of(n_pairs, ny, nx, seed=0):
    rng = np.random.default_rng(90 + seed + n_pairs)
    t = np.stack([MIN_X + rng.uniform(0.0, nx * RES, n_pairs), MIN_Y + rng.uniform(0.0, ny * RES, n_pairs)], axis=1)
    th = rng.uniform(-np.pi, np.pi, n_pairs)
    return t, np.stack([np.cos(th), np.sin(th)], axis=1)


def pair_clouds_of(n_pairs, n_clouds):
    """The last cloud first: the rows a one-pair call reads are the last rows of ``pts``."""
    return ((n_clouds - 1 - np.arange(n_pairs)) % n_clouds).astype(np.int32)


def planes_bytes_of(occupied, unknown, total):
    """The planes buffer as include/icpmi.h lays it out -> (uint8 [total], the mask of the bytes it defines)."""
    buf, mask = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=bool)
    n = occupied.nbytes
    second = (n + 255) // 256 * 256
    buf[:n], buf[second:second + n] = occupied.reshape(-1).view(np.uint8), unknown.reshape(-1).view(np.uint8)
    mask[:n] = mask[second:second + n] = True
    return buf, mask
