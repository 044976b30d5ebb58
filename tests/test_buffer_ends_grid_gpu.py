"""Buffer ends of the grid entries — the score field, the bound field, the likelihood field, the bit planes, both casts, the matcher, the wide
search, the moments, the check, the beam model and the ray-cast update: each called
through ``icpmi.lib()`` with every device buffer exactly as large as include/icpmi.h states, inside the guarded arena of
tests/arena.py.  Per case (tests/buffer_ends_grid.py lists them, tests/buffer_ends.py runs them): under byte pattern 0x7F, then
under 0xFF in the same arena, no guard byte and no input byte may change; the outputs of the two runs must be the same
bits; and they must equal the NumPy restatement of the contract (or, where the suite has none, the same call on roomy
buffers surrounded by zeros).  Every case prints "guards intact, N bytes watched" or fails with the names of the buffers
and the offsets of the bytes that changed.  DESIGN.md ("Buffer ends") has the inventory of buffers, sizes and vector
widths, and what hand mutations the cases catch.

A read outside a buffer that never reaches a result — a load whose value is masked away — cannot be seen this way."""
import pytest

import buffer_ends as be
from buffer_ends_grid import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import icpmi
    return icpmi.lib()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_buffer_ends(case, L):
    be.run(case, L)


def test_a_flipped_guard_byte_is_named(L):
    """The instrument itself, on the device: after a clean run one guard byte next to an output is flipped with a torch
    operation, and check() must name that output and that byte."""
    import arena as ar
    b = be.run(next(c for c in CASES if c.id == "score_field[5x33]"), L)
    assert b.arena.check() == []
    r = b.arena.regions["field"]
    for at, where, rel in ((r.offset + r.nbytes, "after", r.nbytes), (r.offset - 1, "before", -1), (r.offset + r.nbytes + ar.GUARD - 1, "after", r.nbytes + ar.GUARD - 1)):
        b.arena.buf[at:at + 1].bitwise_xor_(0x01)
        assert b.arena.check() == [("field", where, [rel])]
        b.arena.buf[at:at + 1].bitwise_xor_(0x01)
    assert b.arena.check() == []
