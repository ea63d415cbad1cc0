"""rt_check_uniform_guards at the C-ABI boundary (include/hrt.h): argument checks before the device, the loud failure
without a GPU, and the shape of the Python wrapper. CPU only; the check itself runs in test_gpu_uniform_guards.py."""
import ctypes as C
import re
from pathlib import Path

import pytest

import hrt
from hrt import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "hrt.h").read_text()


def _words():
    return (C.c_uint64 * (len(hrt.UGUARD_HELPERS) * len(hrt.UGUARD_COLUMNS)))()


def test_bad_arguments_are_rejected_before_the_device():
    L = hrt.lib()
    assert L.rt_check_uniform_guards(1, 0, None) == _lib.RT_ERR_ARG
    assert b"rt_check_uniform_guards" in L.rt_last_error()
    assert L.rt_check_uniform_guards(0, 0, _words()) == _lib.RT_ERR_ARG
    assert b"rt_check_uniform_guards" in L.rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        hrt.check_uniform_guards(0, 1)
    assert e.value.code == _lib.RT_ERR_ARG


def test_fails_loudly_without_gpu():
    if hrt.device_count() > 0:
        pytest.skip("a GPU is visible")
    out = _words()
    assert hrt.lib().rt_check_uniform_guards(4, 1, out) == _lib.RT_ERR_DEVICE
    assert hrt.lib().rt_last_error()
    assert not any(out)
    with pytest.raises(hrt.RtError) as e:
        hrt.check_uniform_guards(4, 1)
    assert e.value.code == _lib.RT_ERR_DEVICE and "no CPU fallback" in str(e.value)


def test_wrapper_is_six_helpers_by_ten_columns(monkeypatch):
    """The wrapper's names follow the header's sizes and order, and it lays out[helper * words + column] out as
    {helper: {column: count}} (checked on a stand-in entry point that fills the words with their indices)."""
    helpers = int(re.search(r"#define RT_UGUARD_HELPERS (\d+)u", HEADER).group(1))
    words = int(re.search(r"#define RT_UGUARD_WORDS (\d+)u", HEADER).group(1))
    assert (len(hrt.UGUARD_HELPERS), len(hrt.UGUARD_COLUMNS)) == (helpers, words) == (6, 10)
    assert len(set(hrt.UGUARD_HELPERS)) == 6 and len(set(hrt.UGUARD_COLUMNS)) == 10
    assert hrt.UGUARD_HELPERS == ("sqrt_exact_u", "normalize_exact_u", "candidate_t", "div_by_radius3_u",
                                  "div_by_len_rng_u", "div_cam_u")
    for name in hrt.UGUARD_HELPERS:  # the header's table names the same helpers
        assert name in HEADER

    seen = {}

    class StandIn:
        def rt_check_uniform_guards(self, n_waves, seed, out):
            seen["args"] = (n_waves, seed)
            for i in range(helpers * words):
                out[i] = 1000 + i
            return _lib.RT_OK

    monkeypatch.setattr(hrt, "lib", lambda: StandIn())
    got = hrt.check_uniform_guards(12, 0x1_0000_0005)
    assert seen["args"] == (12, 5)
    assert list(got) == list(hrt.UGUARD_HELPERS)
    for i, h in enumerate(hrt.UGUARD_HELPERS):
        assert list(got[h]) == list(hrt.UGUARD_COLUMNS)
        assert [got[h][c] for c in hrt.UGUARD_COLUMNS] == [1000 + i * words + j for j in range(words)]
