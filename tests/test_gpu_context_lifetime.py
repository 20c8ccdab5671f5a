"""fi_destroy returns everything a context allocated on the device.

A context that has planned one batch holds three table heaps (fi_context.cpp
kHeapI / kHeapF / kHeapD: 4 + 0.5 + 1 GiB).  fi_destroy used to free every
other buffer and leave those: 5.5 GiB lost per closed context, which the
suite only met once it created enough contexts in one process to exhaust the
card (a 1 GiB hipMalloc then failed in an unrelated test)."""
import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, Op

pytestmark = pytest.mark.gpu

# 56 x 5.5 GiB = 308 GiB, more than the card's 288 GiB: the loop below cannot
# finish unless each closed context gave its heaps back
CYCLES = 56


def test_closed_contexts_give_their_table_heaps_back():
    src = np.full((32, 48, 3), 200, np.uint8)
    op = Op(24, 0, L.FI_OP_THUMBNAIL | L.FI_GEOM_SHRINK_ONLY, L.GRAVITY["Center"], 0)
    first = None
    for k in range(CYCLES):
        with Context(0) as c:
            outs, recs, rc = c.process([src], [op])
            assert rc == 0 and recs[0].status == 0, (k, L.lib().fi_last_error())
            first = outs[0] if first is None else first
            assert np.array_equal(outs[0], first)
    assert first.shape == (16, 24, 3) and (first == 200).all()
