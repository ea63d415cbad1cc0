"""rt_testing_set_descent_hold at the C boundary (include/hrt_testing.h): its argument check, and that the threshold
stays off the drop-in surface (no rt_params field, no ABI bump). CPU only; the walk itself runs in
test_gpu_descent_hold.py."""
import re
from pathlib import Path

import pytest

import hrt
from hrt import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "hrt.h").read_text()
TESTING = (ROOT / "include" / "hrt_testing.h").read_text()


def test_null_renderer_is_rejected():
    L = hrt.lib()
    assert L.rt_testing_set_descent_hold(None, 12) == _lib.RT_ERR_ARG
    assert b"rt_testing_set_descent_hold" in L.rt_last_error()


def test_range_is_0_to_64():
    """The range is checked before the handle, so it shows without a device: 0..64 pass on to the handle check."""
    L = hrt.lib()
    for hold in (0, 1, 64):
        assert L.rt_testing_set_descent_hold(None, hold) == _lib.RT_ERR_ARG
        assert L.rt_last_error().endswith(b"null")
    for hold in (65, 256, 0xFFFFFFFF):
        assert L.rt_testing_set_descent_hold(None, hold) == _lib.RT_ERR_ARG
        assert b"0..64" in L.rt_last_error()


def test_threshold_is_not_part_of_the_drop_in_abi():
    assert "rt_testing_set_descent_hold" in TESTING and "descent_hold" not in HEADER
    assert "hold" not in {f[0] for f in _lib.RtParams._fields_}
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)u", HEADER).group(1)) == 7
