"""The path-step boundary (rt_bounce_rays) without a device: the entry point is bound with its argument types, RtBounce
has the header's layout, a null renderer is rejected before the call touches a GPU, and the header declares the call and
documents the miss, order, `paths` and aliasing rules. CPU only."""
import ctypes as C
import re
from pathlib import Path

import hrt
from hrt import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "hrt.h").read_text()


def test_entry_point_is_bound():
    assert "rt_bounce_rays" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["rt_bounce_rays"]
    assert restype is C.c_int
    # renderer, io, n
    assert argtypes == [C.c_void_p, C.POINTER(_lib.RtBounce), C.c_uint32]
    for name in ("bounce_rays", "trace_wavefront"):
        assert hasattr(hrt.Renderer, name), name


def test_struct_layout_is_the_headers():
    assert C.sizeof(_lib.RtBounce) == 88
    # the header's field order: ten pointers, then paths and reserved
    struct = re.search(r"typedef struct rt_bounce \{(.*?)\} rt_bounce;", HEADER, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    declared = re.findall(r"\*?\s*(\w+)\s*[,;]", struct)
    assert declared == ["origins_dev", "dirs_dev", "rng_dev", "throughput_dev", "queries_dev", "hits_dev", "index_in_dev",
                        "count_in_dev", "index_out_dev", "count_out_dev", "paths", "reserved"]
    assert [f[0] for f in _lib.RtBounce._fields_] == declared
    for k, name in enumerate(declared[:10]):
        field = getattr(_lib.RtBounce, name)
        assert (field.offset, field.size) == (8 * k, 8), name
    assert (_lib.RtBounce.paths.offset, _lib.RtBounce.paths.size) == (80, 4)
    assert (_lib.RtBounce.reserved.offset, _lib.RtBounce.reserved.size) == (84, 4)


def test_null_renderer_is_rejected_before_the_device():
    L = hrt.lib()
    buf = (C.c_float * 24)()
    p = C.cast(buf, C.c_void_p).value
    io = _lib.RtBounce(p, p, p, None, None, None, None, None, None, None, 1, 0)
    assert L.rt_bounce_rays(None, C.byref(io), 1) == _lib.RT_ERR_ARG
    assert b"rt_bounce_rays" in L.rt_last_error()
    assert L.rt_cast_rays(None, p, p, 1, p) == _lib.RT_ERR_ARG  # (another call's text in rt_last_error)
    assert b"rt_bounce_rays" not in L.rt_last_error()
    assert L.rt_bounce_rays(None, None, 0) == _lib.RT_ERR_ARG
    assert b"rt_bounce_rays" in L.rt_last_error()


def _comment_before(prototype: str) -> str:
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*" + re.escape(prototype), HEADER, flags=re.S).group(1)
    return re.sub(r"\s+", " ", comment.replace("\n *", " "))


def test_header_declares_it_and_documents_the_contract():
    text = re.sub(r"\s+", " ", HEADER)
    assert "int rt_bounce_rays(rt_renderer *r, const rt_bounce *io, uint32_t n);" in text
    assert text.index("int rt_trace_rays(") < text.index("int rt_bounce_rays(")
    comment = _comment_before("int rt_bounce_rays(")
    for words in (
            "on a miss, origins[j], dirs[j], rng[j] and throughput[j] are left untouched, bit for bit",  # the miss rule
            "keep their relative order; the order between waves is unspecified",  # the order rule
            "an entry with j >= paths is skipped",  # the paths rule
            "index_out must not overlap index_in and count_out must not be count_in",  # the aliasing rule
            "Duplicate indices in index_in are the caller's error: the result is undefined",
            "no camera is needed", "BEFORE the scatter", "queries[j] += 1", "albedo.r * 0.7", "600-step cap",
            "|det| >= 1e-4", "rt_params.bounces is not read", "*count_out is set to 0", "nothing past them is written",
            "min(n, *count_in)", "n = 0 returns RT_OK", "RT_ERR_ARG", "reserved != 0"):
        assert words in comment, words
    # no struct changed: the ABI version stays, and the version comment tells callers to look for the symbol
    assert re.search(r"#define RT_ABI_VERSION 7u", HEADER)
    version_comment = HEADER[HEADER.index("#define RT_ABI_VERSION"):]
    version_comment = version_comment[:version_comment.index("*/")]
    assert "rt_bounce_rays" in version_comment and "symbols" in version_comment
