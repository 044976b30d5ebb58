"""Guard bands around device buffers: one ``torch.uint8`` allocation holds every buffer of a call as
``[guard | payload | guard | payload | ... | guard]``, each payload exactly as long as include/icpmi.h says and starting at
an address that is 16 (mod 256) — 16-byte aligned, as the entries check, and never 256-byte aligned, so a layout that is
only right from a 256-aligned base shows.  The guards (64 KiB each) and every byte nothing has been promised about are
filled with one of two byte patterns before a call; afterwards ``check()`` names what changed.  Everything lies inside
the one allocation, so a kernel that runs a little over its buffer lands in a guard, not in someone else's memory.

A helper, no test in it.  It works on CPU tensors as well (tests/test_buffer_ends_cpu.py tests it there).

What the method cannot see: a read outside a buffer whose value never reaches a result, such as a load that is masked
away afterwards.  Only writes, and reads that change an output under one of the two patterns, show.
"""
import ctypes as C

import numpy as np
import torch

GUARD = 64 * 1024                      # bytes of every guard: a condition, far above the 256-byte paddings and one grid row
START = 16                             # a payload's address modulo ALIGN
ALIGN = 256
PATTERNS = (0x7F, 0xFF)
# what a buffer full of a pattern reads as: 0x7F — a huge double, an occupied int16 cell with a large score, a large
# positive int32; 0xFF — NaN, -1
DECODED = {0x7F: {"int16": 32639, "int32": 2139062143, "uint32": 2139062143, "float64": 1.3824172084878715e306},
           0xFF: {"int16": -1, "int32": -1, "uint32": 4294967295, "float64": float("nan")}}

INPUT, OUTPUT, SCRATCH, STATE = "input", "output", "scratch", "state"

_TORCH = {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32, "uint32": torch.int32, "int64": torch.int64,
          "uint64": torch.int64, "float32": torch.float32, "float64": torch.float64}


def decode(pattern, dtype):
    """The value an element of ``dtype`` (a NumPy dtype or its name) has when every byte of it is ``pattern``."""
    dt = np.dtype(dtype)
    return np.full(dt.itemsize, pattern, dtype=np.uint8).view(dt)[0]


class Region:
    def __init__(self, name, role, offset, nbytes, dtype, shape, initial):
        self.name, self.role, self.offset, self.nbytes = name, role, offset, nbytes
        self.dtype, self.shape, self.initial = dtype, shape, initial
        self.frozen = None             # a snapshot taken by Arena.freeze: the payload is watched like an input from then on
        self.ptr = 0


class Arena:
    """``place`` hands out the payloads in order; ``poison`` writes the pattern and the initial contents; ``check`` compares.

    Roles: INPUT — the array's bytes, which must be unchanged after the call; STATE — the array's bytes, written again by
    every ``poison`` and free to change (a buffer whose contract asks the caller for initial contents, or one updated in
    place); OUTPUT and SCRATCH — filled with the pattern."""

    def __init__(self, device="cpu", capacity=8 << 20):
        self.device = torch.device(device)
        self.buf = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        self.end = 0                                               # one past the last payload
        self.regions = {}
        self.pattern = None
        self._image = None

    # ── placement ────────────────────────────────────────────────────────────
    def place(self, array_or_nbytes, name, role=None, dtype=None, start=START):
        """-> (view, pointer): ``view`` a typed tensor over exactly the payload's bytes (uint32 / uint64 as torch's signed type
        of the same width: the bits are what matters), ``pointer`` a ``ctypes.c_void_p``.  An array gives its bytes, dtype and
        shape (role INPUT unless said otherwise); a number gives that many bytes (role SCRATCH unless said otherwise; ``dtype``
        a NumPy dtype name for the view, uint8 by default).  ``start``: the payload's address modulo 256, for an entry that
        needs a stricter start than 16."""
        if name in self.regions:
            raise ValueError(f"{name} is placed already")
        if isinstance(array_or_nbytes, (int, np.integer)):
            nbytes, initial = int(array_or_nbytes), None
            dt = np.dtype(dtype or "uint8")
            if nbytes % dt.itemsize:
                dt = np.dtype("uint8")
            shape, role = (nbytes // dt.itemsize,), role or SCRATCH
        else:
            a = np.ascontiguousarray(array_or_nbytes)
            nbytes, dt, shape, role = a.nbytes, a.dtype, a.shape, role or INPUT
            initial = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(self.device)
        if role in (INPUT, STATE) and initial is None:
            raise ValueError(f"{name}: role {role} needs contents")
        first = self.end + GUARD
        offset = first + (start - (self.buf.data_ptr() + first)) % ALIGN
        if offset + nbytes + GUARD > self.buf.numel():
            raise ValueError(f"{name}: the arena's capacity of {self.buf.numel()} bytes is used up")
        r = Region(name, role, offset, nbytes, dt, shape, initial)
        r.ptr = self.buf.data_ptr() + offset
        self.regions[name] = r
        self.end = offset + nbytes
        self._image = None
        return self.view(name), C.c_void_p(r.ptr)

    def view(self, name):
        r = self.regions[name]
        return self.buf[r.offset:r.offset + r.nbytes].view(_TORCH[r.dtype.name]).reshape(r.shape)

    def ptr(self, name):
        return C.c_void_p(self.regions[name].ptr)

    def nbytes(self, name):
        return self.regions[name].nbytes

    @property
    def limit(self):
        """One past the last watched byte: the last payload's guard ends here."""
        return self.end + GUARD

    # ── patterns ─────────────────────────────────────────────────────────────
    def poison(self, pattern):
        """Every guard, every SCRATCH and every OUTPUT payload becomes ``pattern``; INPUT and STATE payloads get their
        contents.  Snapshots of ``freeze`` are dropped."""
        self.pattern = int(pattern)
        self.buf[:self.limit].fill_(self.pattern)
        for r in self.regions.values():
            r.frozen = None
            if r.initial is not None:
                self.buf[r.offset:r.offset + r.nbytes].copy_(r.initial)
        self._image = None

    def freeze(self, name):
        """From now until the next ``poison`` the payload ``name`` must keep the bytes it holds at this moment: a buffer one
        entry of a chain has written and the next ones only read."""
        r = self.regions[name]
        r.frozen = self.buf[r.offset:r.offset + r.nbytes].clone()
        self._image = None

    def _expected(self):
        """(image, watched): what every watched byte must hold, and which bytes are watched."""
        if self._image is None:
            image = torch.full((self.limit,), self.pattern, dtype=torch.uint8, device=self.device)
            watched = torch.ones(self.limit, dtype=torch.bool, device=self.device)
            for r in self.regions.values():
                keep = r.frozen if r.frozen is not None else (r.initial if r.role == INPUT else None)
                if keep is not None:
                    image[r.offset:r.offset + r.nbytes] = keep
                else:
                    watched[r.offset:r.offset + r.nbytes] = False
            self._image = (image, watched)
        return self._image

    def watched_bytes(self):
        return int(self._expected()[1].sum().item())

    def check(self, most=4):
        """-> a list of (name, where, offsets): ``where`` is "before" or "after" for the guard on that side of the payload
        ``name`` and "input" for the payload itself; ``offsets`` the first changed bytes, relative to the payload's first
        byte (negative in the guard before it, from its length on in the guard after it).  Empty: nothing outside was
        written.  One comparison on the device over all watched bytes; only what differs comes to the host."""
        image, watched = self._expected()
        bad = torch.nonzero((self.buf[:self.limit] != image) & watched).reshape(-1).cpu().numpy()
        if not len(bad):
            return []
        order = sorted(self.regions.values(), key=lambda r: r.offset)
        ends = [r.offset + r.nbytes for r in order]
        # a gap between two payloads is split in the middle: each half is the guard of the payload it touches
        cuts = [0] + [(ends[i] + order[i + 1].offset) // 2 for i in range(len(order) - 1)] + [self.limit]
        found = []
        for i, r in enumerate(order):
            for where, a, b in (("before", cuts[i], r.offset), ("input", r.offset, ends[i]), ("after", ends[i], cuts[i + 1])):
                hit = bad[(bad >= a) & (bad < b)]
                if len(hit):
                    found.append((r.name, where, [int(v) - r.offset for v in hit[:most]]))
        return found

    # ── reading back ─────────────────────────────────────────────────────────
    def read(self, name):
        """The payload on the host, as a NumPy array of the placed dtype and shape (a copy)."""
        r = self.regions[name]
        return self.buf[r.offset:r.offset + r.nbytes].cpu().numpy().copy().view(r.dtype).reshape(r.shape)

    def holds_pattern(self, name, mask=None):
        """Whether the elements of ``name`` selected by the boolean ``mask`` (all of them without one) still hold the pattern."""
        r = self.regions[name]
        raw = self.buf[r.offset:r.offset + r.nbytes].cpu().numpy().reshape(-1, r.dtype.itemsize)
        same = (raw == self.pattern).all(axis=1).reshape(r.shape)
        return bool(same.all() if mask is None else same[np.broadcast_to(mask, r.shape)].all())
