"""Buffer ends of the particle filter — predict, weights, resample, estimate, the free index and the draw from it: each called
through ``icpmi.lib()`` with every device buffer exactly as large as include/icpmi.h states, inside the guarded arena of
tests/arena.py.  Per case (tests/buffer_ends_particles.py lists them, tests/buffer_ends.py runs them): under byte pattern 0x7F, then
under 0xFF in the same arena, no guard byte and no input byte may change; the outputs of the two runs must be the same
bits; and they must equal the NumPy restatement of the contract (or, where the suite has none, the same call on roomy
buffers surrounded by zeros).  Every case prints "guards intact, N bytes watched" or fails with the names of the buffers
and the offsets of the bytes that changed.  DESIGN.md ("Buffer ends") has the inventory of buffers, sizes and vector
widths, and what hand mutations the cases catch.

A read outside a buffer that never reaches a result — a load whose value is masked away — cannot be seen this way."""
import pytest

import buffer_ends as be
from buffer_ends_particles import CASES

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
