"""The regrouping boundary (rt_regroup_paths, rt_host_regroup_keys) without a device: both symbols are exported and
bound, RtRegroup has the header's layout and the constants the header's values, a null renderer is rejected before the
call touches a GPU, the header carries the contract, and the host key function agrees exactly with a numpy restatement of
its definition — on random rays in and around four boxes and on a hand-made list of edge cases. CPU only."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "hrt.h").read_text()

C3_BOX = ((-12.0, -0.5, -12.0), (12.0, 2.5, 12.0))
BOXES = {
    "unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "c3": C3_BOX,
    "thin": ((0.0, 0.0, -2.0), (1.0, 2.0 ** -60, 3.0)),  # y extent exactly 2^-60 in f32 (so that axis sits at 0)
    "huge": ((-(2.0 ** 59), 0.0, -1.0), (2.0 ** 59, 2.0 ** 60, 1.0)),  # x and y extents 2^60
}


def _box(name):
    lo, hi = (np.array(v, dtype=np.float32) for v in BOXES[name])
    return lo, hi


# ------------------------------------------------------------------------------------------------ the numpy restatement
def numpy_keys(o, d, lo, hi):
    """include/hrt.h, mode 1, word for word: inv = 128 / (hi - lo); f = (o - lo) * inv as two rounded f32 operations;
    q = !(f > 0) ? 0 : (f >= 128 ? 127 : (uint32_t)f); bit i of q_x, q_y, q_z to key bit 3 + 3i, 4 + 3i, 5 + 3i; the raw
    sign bits of d in bits 0, 1, 2."""
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(128.0) / (hi - lo)
        assert inv.dtype == np.float32
        e = o - lo[None, :]
        f = e * inv[None, :]
        assert e.dtype == np.float32 and f.dtype == np.float32
        q = np.zeros(f.shape, dtype=np.uint32)
        pos = f > 0  # (False for NaN)
        top = pos & (f >= 128)
        mid = pos & ~top
        q[top] = 127
        q[mid] = f[mid].astype(np.uint32)  # (0 < f < 128: the truncation is defined)
    key = d.view(np.uint32)[:, 0] >> 31 | (d.view(np.uint32)[:, 1] >> 31) << 1 | (d.view(np.uint32)[:, 2] >> 31) << 2
    key = key.astype(np.uint32)
    for i in range(7):
        for axis in range(3):
            key |= ((q[:, axis] >> i) & 1) << (3 + 3 * i + axis)
    return key.astype(np.uint32)


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def handmade_rays(lo, hi):
    """The edge cases, per axis (the other two axes sit mid-box) and all three axes at once: an origin exactly at lo and
    at hi, one ulp inside and outside each, far outside on both sides, +-inf, NaN, and a denormal distance from lo (when lo
    is 0, else the smallest step from lo); then directions +0, -0, NaN with either sign bit, +-inf on every axis."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    mid = (lo * np.float32(0.5) + hi * np.float32(0.5)).astype(np.float32)
    neg_nan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    pos_nan = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
    origins = []
    for k in range(3):
        values = [lo[k], hi[k], _ulp(lo[k], True), _ulp(hi[k], False), _ulp(lo[k], False), _ulp(hi[k], True),
                  np.float32(-3.0e38), np.float32(3.0e38), lo[k] - np.float32(1e6) * (hi[k] - lo[k]),
                  hi[k] + np.float32(1e6) * (hi[k] - lo[k]), np.float32(np.inf), np.float32(-np.inf), pos_nan, neg_nan,
                  lo[k] + np.float32(1e-45), lo[k] + np.float32(1e-40), np.float32(1e-45), np.float32(-1e-45)]
        for v in values:
            o = mid.copy()
            o[k] = v
            origins.append(o)
    for v in (lo, hi, np.full(3, np.inf), np.full(3, -np.inf), np.full(3, pos_nan), mid):
        origins.append(np.asarray(v, dtype=np.float32))
    origins = np.array(origins, dtype=np.float32)
    special = np.array([0.0, -0.0, pos_nan, neg_nan, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32)
    dirs = []
    for a in special:
        for b in special:
            dirs.append([a, b, special[(len(dirs) * 3 + 1) % len(special)]])
            dirs.append([special[(len(dirs) * 5 + 2) % len(special)], a, b])
    dirs = np.array(dirs, dtype=np.float32)
    # every origin with a cycling direction, then every direction at the box's middle
    o_all = np.concatenate([origins, np.repeat(mid[None, :], len(dirs), axis=0)])
    d_all = np.concatenate([dirs[np.arange(len(origins)) % len(dirs)], dirs])
    return np.ascontiguousarray(o_all), np.ascontiguousarray(d_all)


def random_rays(lo, hi, n=4096, seed=20):
    """n rays in and around the box: origins uniform over 1.5 box extents around its middle, Gaussian directions."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    o = (lo + (rng.random((n, 3)) * 1.5 - 0.25) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    return o, d


# ------------------------------------------------------------------------------------------------ binding and layout
def test_symbols_exist_and_are_bound():
    L = hrt.lib()
    for name in ("rt_regroup_paths", "rt_host_regroup_keys"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    restype, argtypes = _lib.SIGNATURES["rt_regroup_paths"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(_lib.RtRegroup), C.c_uint32]
    for name in ("regroup_paths", "trace_wavefront"):
        assert hasattr(hrt.Renderer, name), name
    assert callable(hrt.regroup_keys)


def _header_struct():
    body = re.search(r"typedef struct rt_regroup \{(.*?)\} rt_regroup;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []  # (name, size, alignment) in declaration order
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        base = "uint32_t" if "uint32_t" in decl else "float" if "float" in decl else "void"
        assert pointer or base != "void", decl
        names = re.sub(r"^(const\s+)?(void|uint32_t|float)\s*", "", decl)
        for name in names.split(","):
            name = name.strip().lstrip("*").strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            count = int(m.group(2)) if m else 1
            name = m.group(1) if m else name
            fields.append((name, (8 if pointer else 4) * count, 8 if pointer else 4))
    return fields


def test_struct_layout_is_the_headers():
    fields = _header_struct()
    assert [f[0] for f in fields] == ["origins_dev", "dirs_dev", "keys_dev", "index_in_dev", "count_in_dev",
                                      "index_out_dev", "keys_out_dev", "paths", "mode", "box_lo", "box_hi", "reserved",
                                      "pad"]
    assert [f[0] for f in _lib.RtRegroup._fields_] == [f[0] for f in fields]
    offset = 0
    for name, size, align in fields:  # the C layout rule: each field at the next multiple of its alignment
        offset = (offset + align - 1) // align * align
        field = getattr(_lib.RtRegroup, name)
        assert (field.offset, field.size) == (offset, size), name
        offset += size
    assert offset == 96 and offset % 8 == 0  # no tail padding left to the compiler
    assert C.sizeof(_lib.RtRegroup) == 96
    # the library pins the same size (a static_assert beside the call)
    src = (ROOT / "hello-raytracing_amd" / "csrc" / "renderer.cpp").read_text()
    assert re.search(r"static_assert\(sizeof\(rt_regroup\) == 96", src)
    assert "multiple of" in re.search(r"uint32_t pad;\s*/\*(.*?)\*/", HEADER, flags=re.S).group(1)


def test_constants_match_the_header():
    def define(name):
        return re.search(r"#define " + name + r"\s+(\S+)", HEADER).group(1)

    assert define("RT_REGROUP_CELL_OCTANT") == "1u" and _lib.REGROUP_CELL_OCTANT == 1 == hrt.REGROUP_CELL_OCTANT
    assert define("RT_REGROUP_KEYS") == "2u" and _lib.REGROUP_KEYS == 2 == hrt.REGROUP_KEYS
    assert define("RT_REGROUP_MAX_ENTRIES") == "(1u" and "(1u << 28)" in HEADER and _lib.REGROUP_MAX_ENTRIES == 1 << 28
    assert int(define("RT_REGROUP_TILE").rstrip("u")) == _lib.REGROUP_TILE == hrt.REGROUP_TILE
    assert _lib.REGROUP_TILE % 64 == 0


def test_null_renderer_is_rejected_before_the_device():
    L = hrt.lib()
    buf = (C.c_uint32 * 16)()
    p = C.cast(buf, C.c_void_p).value
    io = _lib.RtRegroup(None, None, p, None, None, p, None, 4, _lib.REGROUP_KEYS)
    assert L.rt_regroup_paths(None, C.byref(io), 4) == _lib.RT_ERR_ARG
    assert b"rt_regroup_paths" in L.rt_last_error()
    assert L.rt_regroup_paths(None, None, 0) == _lib.RT_ERR_ARG
    assert list(buf) == [0] * 16


def test_header_declares_them_and_documents_the_contract():
    text = re.sub(r"\s+", " ", HEADER)
    assert "int rt_regroup_paths(rt_renderer *r, const rt_regroup *io, uint32_t n);" in text
    assert ("int rt_host_regroup_keys(const float *origins, const float *dirs, uint32_t n, const float box_lo[3], "
            "const float box_hi[3], uint32_t *keys_out);") in text
    assert text.index("int rt_bounce_rays(") < text.index("int rt_regroup_paths(") < text.index("int rt_primary_rng(")
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int rt_regroup_paths\(", HEADER, flags=re.S).group(1)
    comment = re.sub(r"\s+", " ", comment.replace("\n *", " "))
    for words in ("live = min(n, *count_in)", "ascending key order", "the sort is stable", "bit for bit",
                  "Nothing is written at or past position live", "There is no count_out", "0x00FFFFFF", "0xFFFFFFFF",
                  "nothing is read through such an index", "Duplicate indices are not an error",
                  "inv_k = 128.0f / (box_hi[k] - box_lo[k])", "!(f > 0) ? 0 : (f >= 128 ? 127 : (uint32_t)f)",
                  "3 + 3i, 4 + 3i, 5 + 3i", "raw sign bits", ">= 2^-60", "index_out == index_in, the same pointer, is allowed",
                  "keys_out must not overlap any input", "4 u32 per entry", "rt_release_scratch", "n = 0 returns RT_OK",
                  "reserved != 0", "RT_REGROUP_MAX_ENTRIES", "no scene and no camera",
                  "no image, frame count, stats, raw counters or learnt cost order"):
        assert words in comment, words
    assert re.search(r"#define RT_ABI_VERSION 7u", HEADER)
    version_comment = HEADER[HEADER.index("#define RT_ABI_VERSION"):]
    version_comment = version_comment[:version_comment.index("*/")]
    assert "rt_regroup_paths" in version_comment and "symbols" in version_comment


# ------------------------------------------------------------------------------------------------ the host key function
@pytest.mark.parametrize("box", sorted(BOXES))
def test_host_keys_are_the_numpy_restatement(box):
    lo, hi = _box(box)
    if box == "thin":
        assert hi[1] - lo[1] == np.float32(2.0 ** -60)
    if box == "huge":
        assert hi[0] - lo[0] == np.float32(2.0 ** 60) and hi[1] - lo[1] == np.float32(2.0 ** 60)
    for what, (o, d) in (("random", random_rays(lo, hi)), ("handmade", handmade_rays(lo, hi))):
        got = hrt.regroup_keys(o, d, lo, hi)
        ref = numpy_keys(o, d, lo, hi)
        assert got.dtype == np.uint32 and got.shape == (len(o),)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (box, what, bad[:5].tolist(), [hex(int(x)) for x in got[bad[:5]]],
                               [hex(int(x)) for x in ref[bad[:5]]], o[bad[:5]].tolist())
        assert int(got.max()) <= 0x00FFFFFF
    # the random rays do exercise the key: many cells, all eight octants
    got = hrt.regroup_keys(*random_rays(lo, hi), lo, hi)
    assert len(np.unique(got >> 3)) > 500 and len(np.unique(got & 7)) == 8


def test_host_keys_by_hand():
    """A few keys worked out by hand on the unit cube (q = floor(128 x))."""
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    o = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [np.nan, np.inf, -np.inf], [1.0 / 128, 0.0, 0.0],
                  [0.0, 2.0 / 128, 0.0], [0.0, 0.0, 127.5 / 128]], dtype=np.float32)
    d = np.array([[1.0, -1.0, 1.0], [-0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0],
                  [1.0, 1.0, -np.inf]], dtype=np.float32)
    want = [0x2, 0xE00001, 0xFFFFF8, 0x492497, 1 << 3, 1 << 7,
            sum(1 << (5 + 3 * i) for i in range(7)) | 4]  # (the last: q_z = 127, d.z negative)
    assert [int(x) for x in hrt.regroup_keys(o, d, lo, hi)] == want
    assert hrt.regroup_keys(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), lo, hi).shape == (0,)


@pytest.mark.parametrize("lo, hi", [
    ((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)),  # hi == lo
    ((0.0, 0.0, 0.0), (1.0, 1.0, -1.0)),  # hi < lo
    ((np.nan, 0.0, 0.0), (1.0, 1.0, 1.0)),
    ((0.0, 0.0, 0.0), (1.0, np.nan, 1.0)),
    ((0.0, 0.0, 0.0), (np.inf, 1.0, 1.0)),
    ((-np.inf, 0.0, 0.0), (1.0, 1.0, 1.0)),
    ((-3.0e38, 0.0, 0.0), (3.0e38, 1.0, 1.0)),  # finite corners, infinite extent
    ((0.0, 0.0, 0.0), (1.0, 1.0, 2.0 ** -61)),  # below 2^-60
])
def test_bad_boxes_are_refused(lo, hi):
    o = np.zeros((2, 3), dtype=np.float32)
    out_before = hrt.lib().rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        hrt.regroup_keys(o, o, lo, hi)
    assert e.value.code == _lib.RT_ERR_ARG, out_before
    assert b"rt_host_regroup_keys" in hrt.lib().rt_last_error()
