"""CPU tests of the helpers the field-level GPU suites share (tests/field_suite.py) and of the one executor_multiplicity the fp64
restatements share (tests/theta_ref.py)."""
import numpy as np
import pytest

from field_suite import TOL, blockwise
from theta_ref import executor_multiplicity
from util import rel_err

BLOCKS = [("H", 4000), ("lambda_3", 3), ("K", 5997)]


def test_blockwise_sees_an_error_confined_to_a_small_block():
    """10,000 elements, the large blocks with values up to 1000, an error of 1e-3 in a block of three values of size 1 (a wrong lambda_s
    beside a K_l): one norm over the whole vector measures 1e-6 and passes at 1e-5; the block's own norm measures 1e-3."""
    rng = np.random.default_rng(3)
    ref = rng.uniform(-1000, 1000, 10000)
    ref[4000:4003] = [1.0, -0.5, 0.25]
    ref[0] = 1000.0
    x = ref.copy()
    x[4000:4003] += [1e-3, -1e-3, 1e-3]
    assert rel_err(x, ref) == pytest.approx(1e-6) and rel_err(x, ref) <= TOL
    err, name = blockwise(x, ref, BLOCKS)
    assert name == "lambda_3" and err == pytest.approx(1e-3) and err > TOL


def test_blockwise_refuses_blocks_that_do_not_cover_the_vector():
    ref = np.zeros(10000)
    with pytest.raises(AssertionError):
        blockwise(ref, ref, BLOCKS[:2])
    with pytest.raises(AssertionError):
        blockwise(ref, ref, BLOCKS + [("W", 1)])


def test_executor_multiplicity_matches_the_closed_forms():
    for k in range(1, 13):
        j = np.arange(1, k + 1)
        assert executor_multiplicity(0, k) == [1] * k
        assert executor_multiplicity(1, k) == list(j)
        assert executor_multiplicity(2, k) == list(j * (j + 1) // 2)
        assert executor_multiplicity(3, k) == list(j * (j + 1) * (j + 2) // 6)
