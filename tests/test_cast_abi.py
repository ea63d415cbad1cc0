"""The ray-query boundary (rt_cast_rays, rt_primary_rays, rt_hit) without a device: the numpy mirror of rt_hit has the
header struct's layout, the Python constants are the header's, and both entry points reject a null renderer before they
touch a GPU. CPU only."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import hrt
from hrt import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "hrt.h").read_text()
SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4}


def _header_hit_fields():
    """(name, offset, bytes) of every field of `typedef struct rt_hit {...} rt_hit;`, natural alignment."""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    body = re.search(r"typedef struct rt_hit \{(.*?)\} rt_hit;", text, flags=re.S).group(1)
    out, off = [], 0
    for typ, names in re.findall(r"(float|int32_t|uint32_t)\s+([\w\s,\[\]]+);", body):
        for name in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", name)
            size = SIZES[typ] * int(m.group(2) or 1)
            off = (off + SIZES[typ] - 1) // SIZES[typ] * SIZES[typ]
            out.append((m.group(1), off, size))
            off += size
    return out, off


def test_hit_dtype_mirrors_the_header_struct():
    fields, size = _header_hit_fields()
    assert [f[0] for f in fields] == ["t", "prim", "n", "flags", "material", "reserved"]
    assert size == 32 and hrt.HIT_DTYPE.itemsize == 32
    assert list(hrt.HIT_DTYPE.names) == [f[0] for f in fields]
    for name, off, nbytes in fields:
        dt, got_off = hrt.HIT_DTYPE.fields[name][:2]
        assert (got_off, dt.itemsize) == (off, nbytes), name
    assert hrt.HIT_DTYPE["t"] == np.dtype("<f4") and hrt.HIT_DTYPE["prim"] == np.dtype("<i4")
    assert hrt.HIT_DTYPE["n"].subdtype == (np.dtype("<f4"), (3,))
    for name in ("flags", "material", "reserved"):
        assert hrt.HIT_DTYPE[name] == np.dtype("<u4")


def test_constants_match_the_header():
    t_miss = re.search(r"#define RT_T_MISS\s+([0-9.e+]+)f", HEADER).group(1)
    assert np.float32(hrt.RT_T_MISS) == np.float32(float(t_miss))
    assert np.float32(hrt.RT_T_MISS).view(np.uint32) == 0x7F7FFFEE  # the WGSL 3.40282e+38, not FLT_MAX
    assert hrt.RT_HIT_FRONT == int(re.search(r"#define RT_HIT_FRONT\s+(\d+)u", HEADER).group(1)) == 1
    assert hrt.RT_HIT_TRIANGLE == int(re.search(r"#define RT_HIT_TRIANGLE\s+(\d+)u", HEADER).group(1)) == 2


def test_null_renderer_is_rejected_before_the_device():
    L = hrt.lib()
    buf = (C.c_float * 24)()
    p = C.cast(buf, C.c_void_p)
    assert L.rt_cast_rays(None, p, p, 1, p) == _lib.RT_ERR_ARG
    assert L.rt_cast_rays(None, None, None, 0, None) == _lib.RT_ERR_ARG
    assert L.rt_primary_rays(None, 1000, p, p, 1) == _lib.RT_ERR_ARG
    assert b"rt_primary_rays" in L.rt_last_error()


def test_both_entry_points_are_bound():
    assert {"rt_cast_rays", "rt_primary_rays"} <= set(_lib.SIGNATURES)
    assert _lib.SIGNATURES["rt_cast_rays"][0] is C.c_int and _lib.SIGNATURES["rt_primary_rays"][0] is C.c_int
