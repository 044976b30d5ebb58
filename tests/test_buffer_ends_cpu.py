"""Without a GPU: the arena of tests/arena.py itself, and for every case of the three buffer-end GPU modules that each
workspace, prepared, planes and index buffer is handed exactly what include/icpmi.h's size query returns for the case's
arguments, and that one byte less is refused wherever the entry decides that before its first HIP call (the size queries
are host functions; tests/test_host_cpu.py loads them the same way)."""
import numpy as np
import pytest

import arena as ar
import buffer_ends as be
import buffer_ends_clouds
import buffer_ends_grid
import buffer_ends_particles

ALL = buffer_ends_grid.CASES + buffer_ends_particles.CASES + buffer_ends_clouds.CASES
ERR_WORKSPACE = -2


@pytest.fixture(scope="module")
def L():
    import icpmi
    icpmi.build()
    return icpmi.lib()


# ── the arena ────────────────────────────────────────────────────────────────
def _three():
    a = ar.Arena("cpu", 1 << 20)
    src = np.arange(37, dtype=np.int16)
    a.place(src, "in")
    a.place(13, "scratch")
    a.place(np.full(5, 2.5), "state", ar.STATE)
    a.place(40, "out", ar.OUTPUT, dtype="int32")
    return a, src


def test_placement_arithmetic():
    a, src = _three()
    order = sorted(a.regions.values(), key=lambda r: r.offset)
    assert [r.name for r in order] == ["in", "scratch", "state", "out"]
    assert [r.nbytes for r in order] == [74, 13, 40, 40]
    for r in order:
        assert r.ptr % ar.ALIGN == ar.START and r.ptr == a.buf.data_ptr() + r.offset
        assert a.view(r.name).numel() * a.view(r.name).element_size() == r.nbytes      # the view is exactly the payload
    assert order[0].offset >= ar.GUARD
    for p, q in zip(order, order[1:]):
        gap = q.offset - (p.offset + p.nbytes)
        assert ar.GUARD <= gap < ar.GUARD + ar.ALIGN                                     # the guard begins on the next byte
    assert a.limit == order[-1].offset + 40 + ar.GUARD <= a.buf.numel()
    assert ar.GUARD == 64 * 1024
    a.poison(0x7F)
    assert np.array_equal(a.read("in"), src) and (a.read("state") == 2.5).all()
    assert a.holds_pattern("scratch") and a.holds_pattern("out")
    assert a.check() == []
    # everything but the free payloads is watched: the guards and the input
    assert a.watched_bytes() == a.limit - 13 - 40 - 40
    a.place(16, "strict", start=0)
    assert a.regions["strict"].ptr % ar.ALIGN == 0
    with pytest.raises(ValueError):
        a.place(8, "in")


@pytest.mark.parametrize("pattern", ar.PATTERNS)
def test_planted_bytes_are_reported_under_their_names(pattern):
    a, _ = _three()
    a.poison(pattern)
    r = a.regions["scratch"]
    for offset, where, rel in ((r.offset - 1, "before", -1), (r.offset + r.nbytes, "after", r.nbytes)):
        a.buf[offset] ^= 0x10
        assert a.check() == [("scratch", where, [rel])]
        a.buf[offset] ^= 0x10
    assert a.check() == []
    i = a.regions["in"]
    a.buf[i.offset + 5] ^= 1
    assert a.check() == [("in", "input", [5])]
    a.buf[i.offset + 5] ^= 1
    a.buf[r.offset + 3] = 0                                        # a scratch payload is free to change
    a.view("state")[0] = 9.0                                       # and so is a state payload
    assert a.check() == []
    a.freeze("scratch")                                            # until it is frozen
    a.buf[r.offset + 3] = 1
    assert a.check() == [("scratch", "input", [3])]
    a.poison(pattern)                                              # which poison undoes
    assert a.check() == [] and (a.read("state") == 2.5).all()
    o = a.regions["out"]
    a.buf[a.limit - 1] ^= 0xFF                                     # the last watched byte belongs to the last payload
    assert a.check() == [("out", "after", [a.limit - 1 - o.offset])]


def test_patterns_decode_to_the_listed_values():
    assert ar.PATTERNS == (0x7F, 0xFF)
    assert (ar.decode(0x7F, "int16"), ar.decode(0x7F, "int32"), ar.decode(0x7F, "uint32")) == (32639, 2139062143, 2139062143)
    assert 1.3e306 < ar.decode(0x7F, "float64") < 1.5e306
    assert (ar.decode(0xFF, "int16"), ar.decode(0xFF, "int32"), ar.decode(0xFF, "uint32")) == (-1, -1, 4294967295)
    assert np.isnan(ar.decode(0xFF, "float64"))
    for pattern, table in ar.DECODED.items():
        for name, value in table.items():
            got = ar.decode(pattern, name)
            assert (np.isnan(got) and np.isnan(value)) or got == value
    a = ar.Arena("cpu", 1 << 19)
    a.place(64, "d", ar.OUTPUT, dtype="float64")
    a.place(64, "h", ar.OUTPUT, dtype="int16")
    a.poison(0x7F)
    assert (a.read("d") == ar.decode(0x7F, "float64")).all() and (a.read("h") == 32639).all()
    a.poison(0xFF)
    assert np.isnan(a.read("d")).all() and (a.read("h") == -1).all() and (a.view("h") == -1).all()


def test_same_bits_is_bitwise():
    nan = np.array([np.nan, 1.0])
    assert be.same_bits(nan, nan.copy()) and not be.same_bits(np.array([0.0]), np.array([-0.0]))
    assert be.same_bits(np.array([1, 2]), np.array([1, 3]), np.array([True, False]))


# ── the cases of the GPU modules: exact sizes, and the refusal of one byte less ──────────────────────────────────────────
def test_case_ids_are_unique():
    ids = [c.id for c in ALL]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_exact_sizes_and_refusals(case, L):
    b = be.build_on_cpu(case, L)
    assert b.call is not None and b.outputs and (b.expected is not None or b.twin)
    for r in b.arena.regions.values():
        assert r.ptr % ar.ALIGN == ar.START, (r.name, "a start other than 16 (mod 256) belongs in the inventory")
    for name, (query, args, refusal, on_host) in b.sized.items():
        need = getattr(L, query)(*args)
        assert need > 0 and b.arena.nbytes(name) == need == b.size(name), (name, query, args)
        assert b.size(name, short=name) == need - 1
        if refusal and on_host:
            assert b.call(short=name) == refusal, (name, "one byte less must be refused before anything is started")
