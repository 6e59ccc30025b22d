"""gpu_helpers.assert_same, the comparison the GPU tests rest on, checked on
the host: it passes on equal results and names the key of a get that differs
in its found flag or in its value alone.  (dev and host need a GPU.)"""
import numpy as np
import pytest

from gpu_helpers import U64, assert_same

PROBE = np.array([0x11, 0x2222, (1 << 64) - 2], dtype=U64)
VALS = np.array([7, 0, 9], dtype=U64)
FOUND = np.array([1, 0, 1], dtype=np.uint8)


def test_equal_results_pass():
    assert_same(PROBE, VALS, FOUND, VALS.copy(), FOUND.copy())
    assert_same(PROBE, VALS, FOUND, VALS.copy(), FOUND.copy(), "with a prefix")
    assert_same(PROBE[:0], VALS[:0], FOUND[:0], VALS[:0], FOUND[:0])


def test_a_found_flag_alone_fails():
    gf = FOUND.copy()
    gf[1] = 1
    with pytest.raises(AssertionError) as e:
        assert_same(PROBE, VALS, FOUND, VALS.copy(), gf)
    assert "key=0x2222" in str(e.value) and "1 gets differ" in str(e.value)
    assert "key=0x11 " not in str(e.value)


def test_a_value_alone_fails():
    gv = VALS.copy()
    gv[2] = 10
    with pytest.raises(AssertionError) as e:
        assert_same(PROBE, VALS, FOUND, gv, FOUND.copy(), "after the chunk")
    msg = str(e.value)
    assert msg.startswith("after the chunk: 1 gets differ")
    assert "key=0xfffffffffffffffe" in msg and "oracle=(1,9) gpu=(1,10)" in msg
