"""The occlusion-query boundary (rt_occluded) without a device: the entry point is bound with its six arguments, rejects a
null renderer before it touches a GPU, and the header declares it and documents the NULL tmax. CPU only."""
import ctypes as C
import re
from pathlib import Path

import hrt
from hrt import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "hrt.h").read_text()


def test_entry_point_is_bound():
    assert "rt_occluded" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["rt_occluded"]
    assert restype is C.c_int
    # renderer, origins, dirs, tmax, n, occluded
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert hasattr(hrt.Renderer, "occluded")


def test_null_renderer_is_rejected_before_the_device():
    L = hrt.lib()
    buf = (C.c_float * 24)()
    p = C.cast(buf, C.c_void_p)
    assert L.rt_occluded(None, p, p, p, 1, p) == _lib.RT_ERR_ARG
    assert b"rt_occluded" in L.rt_last_error()
    assert L.rt_cast_rays(None, p, p, 1, p) == _lib.RT_ERR_ARG  # (another call's text in rt_last_error)
    assert L.rt_occluded(None, None, None, None, 0, None) == _lib.RT_ERR_ARG
    assert b"rt_occluded" in L.rt_last_error()


def test_header_declares_it_and_documents_the_null_tmax():
    text = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_occluded(rt_renderer *r, const void *origins_dev, const void *dirs_dev, const void *tmax_dev, "
            "uint32_t n, void *occluded_dev);") in text
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int rt_occluded\(", HEADER, flags=re.S).group(1)
    comment = re.sub(r"\s+", " ", comment.replace("\n *", " "))
    assert re.search(r"NULL = RT_T_MISS for every ray", comment), comment
    for words in ("t < tmax", "tmax = 1", "|det| >= 1e-4", "NaN", "exactly n bytes"):
        assert words in comment, words
    # no struct changed: the ABI version stays, and the version comment tells callers to look for the symbol
    assert re.search(r"#define RT_ABI_VERSION 7u", HEADER)
    version_comment = HEADER[HEADER.index("#define RT_ABI_VERSION"):]
    version_comment = version_comment[:version_comment.index("*/")]
    assert "rt_occluded" in version_comment and "symbols" in version_comment
