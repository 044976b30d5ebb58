"""Buffer ends of the appearance signatures — icpmi_history_signatures_add and icpmi_history_similar: each called through
``icpmi.lib()`` with the signature tables, the records, the score rows and the workspace exactly as large as include/icpmi.h
states, inside the guarded arena of tests/arena.py.  Per case (tests/buffer_ends_signatures.py lists them, tests/buffer_ends.py
runs them): under byte pattern 0x7F, then under 0xFF in the same arena, no guard byte and no input byte may change, the
signatures of the scans outside the added range must keep the pattern, the outputs of the two runs must be the same bits,
and they must equal the NumPy restatement (tests/signatures_ref.py).  Every case prints "guards intact, N bytes watched" or
fails with the names of the buffers and the offsets of the bytes that changed.  The CPU half — exact sizes, one byte less of
workspace refused — is in tests/test_signatures_cpu.py.

A read outside a buffer that never reaches a result — a load whose value is masked away — cannot be seen this way."""
import pytest

import buffer_ends as be
from buffer_ends_signatures import CASES

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
