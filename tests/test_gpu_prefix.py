"""The prefix-sum helpers of the stages that compact variable-length output (csrc/kr_dev_prefix.inc: rows, `dist` text, `place` text,
FASTQ records), run on plain numbers by kr_debug_prefix the way those stages run them -- a sum per block, one workgroup's scan of the
block sums, the exclusive scan inside every block -- and compared with numpy.cumsum, exactly.  The product tests never reach the
carry between rounds of 1024 block sums (above 1,048,576 reads for the rows and the `dist` text); the two large sizes here are the
first that do, one per block size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
CARRY = {64: 64 * 1024 + 1, 1024: 1024 * 1024 + 1}  # the first size whose block sums need a second round of 1024
CASES = [(n, b) for b in (64, 1024) for n in SIZES + [CARRY[b]]]


def values_for(n, width):
    """width 4: values <= 255 (the total of the largest case stays below 2^32); width 8: up to 2^32 - 1, with runs of the largest
    value at the start and the end, so that the sum of a single wave's items already passes 2^32"""
    rng = np.random.default_rng(1000 * width + n % 997)
    if width == 4:
        return rng.integers(0, 256, n, dtype=np.uint32)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v[:8] = v[-8:] = 0xFFFFFFFF
    return v


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("n,block", CASES)
def test_prefix_equals_numpy_cumsum(capi, n, block, width):
    v = values_for(n, width)
    incl = np.cumsum(v, dtype=np.uint64)
    prefix, total = capi.debug_prefix(v, block, width)
    assert total == int(incl[-1])
    assert np.array_equal(prefix, incl - v)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("block", [64, 1024])
def test_no_values_give_total_zero(capi, block, width):
    prefix, total = capi.debug_prefix(np.zeros(0, np.uint32), block, width)
    assert total == 0 and len(prefix) == 0
