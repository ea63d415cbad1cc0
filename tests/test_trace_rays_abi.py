"""The radiance-query boundary (rt_trace_rays, rt_primary_rng) without a device: both entry points are bound with their
argument types, reject a null renderer before they touch a GPU, and the header declares them and documents the NULL-state
rule and the bytes written. CPU only."""
import ctypes as C
import re
from pathlib import Path

import hrt
from hrt import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "hrt.h").read_text()
TESTING = (ROOT / "include" / "hrt_testing.h").read_text()


def test_entry_points_are_bound():
    assert {"rt_trace_rays", "rt_primary_rng"} <= set(_lib.SIGNATURES)
    restype, argtypes = _lib.SIGNATURES["rt_trace_rays"]
    assert restype is C.c_int
    # renderer, origins, dirs, rng, seed, n, radiance, queries
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    restype, argtypes = _lib.SIGNATURES["rt_primary_rng"]
    assert restype is C.c_int
    # renderer, time, rng, n_rays
    assert argtypes == [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
    for name in ("trace_rays", "primary_rng", "trace_frame"):
        assert hasattr(hrt.Renderer, name), name


def test_null_renderer_is_rejected_before_the_device():
    L = hrt.lib()
    buf = (C.c_float * 24)()
    p = C.cast(buf, C.c_void_p)
    assert L.rt_trace_rays(None, p, p, p, 7, 1, p, p) == _lib.RT_ERR_ARG
    assert b"rt_trace_rays" in L.rt_last_error()
    assert L.rt_cast_rays(None, p, p, 1, p) == _lib.RT_ERR_ARG  # (another call's text in rt_last_error)
    assert L.rt_trace_rays(None, None, None, None, 0, 0, None, None) == _lib.RT_ERR_ARG
    assert b"rt_trace_rays" in L.rt_last_error()
    assert L.rt_primary_rng(None, 1000, p, 1) == _lib.RT_ERR_ARG
    assert b"rt_primary_rng" in L.rt_last_error()
    assert L.rt_cast_rays(None, p, p, 1, p) == _lib.RT_ERR_ARG
    assert L.rt_primary_rng(None, 1000, None, 0) == _lib.RT_ERR_ARG
    assert b"rt_primary_rng" in L.rt_last_error()


def _comment_before(prototype: str) -> str:
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*" + re.escape(prototype), HEADER, flags=re.S).group(1)
    return re.sub(r"\s+", " ", comment.replace("\n *", " "))


def test_header_declares_them_and_documents_the_state_rule():
    text = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_trace_rays(rt_renderer *r, const void *origins_dev, const void *dirs_dev, const void *rng_dev, "
            "uint32_t seed, uint32_t n, void *radiance_dev, void *queries_dev);") in text
    assert "int rt_primary_rng(rt_renderer *r, uint32_t time, void *rng_dev, size_t n_rays);" in text
    comment = _comment_before("int rt_trace_rays(")
    for words in ("(i + 1) * seed", "exactly 12", "exactly 4", "NULL", "0.0 + trace(ray)", "albedo * 0.7", "d.y",
                  "600-step cap", "|det| >= 1e-4", "bounces = 0", "RT_ERR_ARG", "no camera is needed"):
        assert words in comment, words
    comment = _comment_before("int rt_primary_rng(")
    for words in ("after make_ray", "local_rows x width", "RT_ERR_STATE"):
        assert words in comment, words
    # no struct changed: the ABI version stays, and the version comment tells callers to look for the symbols
    assert re.search(r"#define RT_ABI_VERSION 7u", HEADER)
    version_comment = HEADER[HEADER.index("#define RT_ABI_VERSION"):]
    version_comment = version_comment[:version_comment.index("*/")]
    assert "rt_trace_rays" in version_comment and "rt_primary_rng" in version_comment and "symbols" in version_comment


def test_forced_rays_per_lane_is_a_testing_entry_point():
    """k_radiance_rays' rays per lane is moved by a test-only call (no environment variable, not in the drop-in header)."""
    L = hrt.lib()
    assert "rt_testing_set_trace_rays_per_lane" in _lib.TESTING_SIGNATURES
    assert "rt_testing_set_trace_rays_per_lane" in TESTING and "rays_per_lane" not in HEADER
    assert L.rt_testing_set_trace_rays_per_lane(None, 4) == _lib.RT_ERR_ARG
    assert b"rt_testing_set_trace_rays_per_lane" in L.rt_last_error()
    assert L.rt_testing_set_trace_rays_per_lane(None, 65) == _lib.RT_ERR_ARG
    assert b"0..64" in L.rt_last_error()
    assert hasattr(hrt.Renderer, "set_trace_rays_per_lane")
