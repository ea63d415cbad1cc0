"""rt_closest_points on the host (rt_host_closest_points, hrt.closest_points_host): the symbols and the record layout, the
function's exact answers on dyadic inputs, degenerate and non-finite triangles, the definition (the lexicographic minimum
of the per-triangle answers), the three properties DESIGN.md §7e argues (hull, no NaN from finite input, accuracy), the cap
rules and the argument errors. CPU only; tests/test_gpu_closest.py compares the device with this function byte for byte.

The host function was also run once as a stand-alone program (its own main over csrc/rt_closest.hpp: sizes 0 to 100,000,
degenerate, non-finite and 1e37-scaled triangles, every cap class) under AddressSanitizer and UndefinedBehaviorSanitizer:
clean (scripts/closest_sanitize.cpp)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_util as U

ROOT = Path(__file__).resolve().parents[1]
MISS = K.MISS
CASES = U.cpu_cases()


def host(tris, pts, cap=None):
    return hrt.closest_points_host(tris, np.asarray(pts, dtype=np.float32).reshape(-1, 3), cap)


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "hrt.h").read_text()
    testing = (ROOT / "include" / "hrt_testing.h").read_text()
    names = ("rt_closest_points", "rt_host_closest_points")
    tnames = ("rt_testing_set_closest_count", "rt_testing_get_closest_counts")
    L = hrt.lib()
    for name in names:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and getattr(L, name).restype is C.c_int
    for name in tnames:
        assert re.search(r"^int %s\(" % name, testing, re.M) and name not in header, name
        assert name in _lib.TESTING_SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert set(names + tnames) <= set(re.findall(r"\bT (rt_\w+)", out))
    # no struct of the ABI changed: the version stays, and its comment lists the two calls
    assert "RT_ABI_VERSION 7u" in header
    comment = header[header.index("#define RT_ABI_VERSION"):header.index("int rt_abi_version")]
    assert "rt_closest_points / rt_host_closest_points" in comment
    assert "spheres of the mixed\n * program are not part of the query" in header


def test_record_layout():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hrt.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct rt_closest \{(.*?)\} rt_closest;", header, flags=re.S).group(1)
    fields = [f.strip() for f in re.sub(r"\b(float|int32_t|uint32_t)\b", "", body).replace(";", ",").split(",") if f.strip()]
    assert fields == ["d2", "prim", "p[3]", "v", "w", "reserved"]
    d = hrt.CLOSEST_DTYPE
    assert d.itemsize == 32
    assert [(n, d.fields[n][1]) for n in d.names] == [("d2", 0), ("prim", 4), ("p", 8), ("v", 20), ("w", 24),
                                                      ("reserved", 28)]
    assert d.fields["prim"][0] == np.int32 and d.fields["p"][0].shape == (3,)


TRI = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], dtype=np.float32)
# point -> (d2, v, w, closest point): one per region of the triangle (0,0,0), (4,0,0), (0,4,0)
EXACT = [
    ((1, 1, 3), (9, 0.25, 0.25, (1, 1, 0))),        # the face
    ((-1, -2, 0), (5, 0, 0, (0, 0, 0))),            # vertex a
    ((6, -1, 2), (9, 1, 0, (4, 0, 0))),             # vertex b
    ((-1, 7, 0), (10, 0, 1, (0, 4, 0))),            # vertex c
    ((2, -3, 0), (9, 0.5, 0, (2, 0, 0))),           # edge ab
    ((-2, 1, 1), (5, 0, 0.25, (0, 1, 0))),          # edge ac
    ((4, 2, 0), (2, 0.75, 0.25, (3, 1, 0))),        # edge bc
]


@pytest.mark.parametrize("offset", [(0, 0, 0), (1024, -2048, 4096)])
def test_exact_cases(offset):
    off = np.array(offset, dtype=np.float32)
    tris = U.triangles_from_vertices(TRI + off)
    pts = np.array([p for p, _ in EXACT], dtype=np.float32) + off
    got = host(tris, pts)
    for rec, (p, (d2, v, w, cp)) in zip(got, EXACT):
        assert (rec["d2"], rec["prim"], rec["v"], rec["w"], rec["reserved"]) == (d2, 0, v, w, 0), (p, rec)
        assert rec["p"].tolist() == (np.array(cp, dtype=np.float32) + off).tolist(), (p, rec)


def test_degenerate_triangles():
    point = np.array([[[1, 2, 3]] * 3], dtype=np.float32)             # collapsed to a point
    b_is_a = np.array([[[0, 0, 0], [0, 0, 0], [0, 4, 0]]], dtype=np.float32)
    c_on_ab = np.array([[[0, 0, 0], [4, 0, 0], [2, 0, 0]]], dtype=np.float32)
    q = np.array([[1, 2, 7], [4, 6, 3], [1, 2, 3]], dtype=np.float32)
    got = host(U.triangles_from_vertices(point), q)
    assert got["d2"].tolist() == [16, 25, 0] and (got["prim"] == 0).all()
    assert (got["p"] == np.float32([1, 2, 3])).all() and not got["v"].any() and not got["w"].any()
    got = host(U.triangles_from_vertices(b_is_a), np.array([[3, 1, 0], [0, 6, 2], [-1, -1, 0]], dtype=np.float32))
    assert got["d2"].tolist() == [9, 8, 2] and got["p"].tolist() == [[0, 1, 0], [0, 4, 0], [0, 0, 0]]
    got = host(U.triangles_from_vertices(c_on_ab), np.array([[1, 3, 0], [6, 0, 1], [3, 0, -2]], dtype=np.float32))
    assert got["d2"].tolist() == [9, 5, 4] and got["p"].tolist() == [[1, 0, 0], [4, 0, 0], [3, 0, 0]]
    for g in (point, b_is_a, c_on_ab):  # no NaN anywhere, for far and near points alike
        r = host(U.triangles_from_vertices(g), K.query_points(U.triangles_from_vertices(g), 64, 5, nonfinite=0))
        assert np.isfinite(r["d2"]).all() and np.isfinite(r["p"]).all() and (r["prim"] == 0).all()


def lexicographic_minimum(tris, pts, cap=None):
    """The definition, with the host function called on one triangle at a time."""
    n = len(pts)
    best = np.zeros(n, dtype=hrt.CLOSEST_DTYPE)
    best["d2"], best["prim"] = MISS, -1
    for j in range(len(tris)):
        r = host(tris[j:j + 1], pts, cap)
        take = (r["prim"] == 0) & ((best["prim"] < 0) | (r["d2"] < best["d2"]))  # (ascending j: ties keep the earlier one)
        r["prim"][take] = j
        best[take] = r[take]
    return best


@pytest.mark.parametrize("name", list(CASES))
def test_whole_array_is_the_lexicographic_minimum(name):
    tris = CASES[name]()
    pts = K.query_points(tris, 32, 40 + len(tris))
    got = host(tris, pts)
    want = lexicographic_minimum(tris, pts)
    assert K.records_equal(got, want), K.first_difference(got, want)
    finite_pts = np.isfinite(pts).all(axis=1)
    assert (got["prim"][~finite_pts] == -1).all()
    if len(tris) and name != "random0":
        assert (got["prim"][finite_pts] >= 0).all()
    if name == "identical70":
        assert (got["prim"][finite_pts] == 0).all()
    if name == "cube":
        lo, hi = K.root_box(tris)
        centre = host(tris, (0.5 * (lo + hi)).astype(np.float32))
        each = np.array([host(tris[j:j + 1], (0.5 * (lo + hi)).astype(np.float32))["d2"][0] for j in range(len(tris))])
        ties = np.flatnonzero(each == each.min())
        assert len(ties) > 1 and centre["prim"][0] == ties[0]


def test_non_finite_triangle_never_answers():
    tris = CASES["nan1of9"]()
    pts = K.query_points(tris, 256, 3)
    got = host(tris, pts)
    assert 4 not in got["prim"].tolist()
    keep = np.array([0, 1, 2, 3, 5, 6, 7, 8])
    want = host(tris[keep], pts)
    hit = want["prim"] >= 0
    want["prim"][hit] = keep[want["prim"][hit]]
    assert K.records_equal(got, want), K.first_difference(got, want)
    alone = host(tris[4:5], pts)
    assert (alone["prim"] == -1).all() and (alone["d2"] == MISS).all()


def property_sets():
    suz = U.mesh_triangles("suzanne.obj")
    return {"suzanne": suz, "suzanne_moved": K.moved(suz, (1000, -2000, 3000)), "random1025": CASES["random1025"](),
            "planar": CASES["planar"]()}


@pytest.mark.parametrize("name", ["suzanne", "suzanne_moved", "random1025", "planar"])
def test_hull_recomputation_and_accuracy(name):
    """The largest observed shares of the bound (B_EDGE + B_PLANE kappa) u D (DESIGN.md §7e records them): suzanne 0.0207,
    suzanne_moved 0.0192, random1025 0.0245, planar 0.0291; the largest errors themselves are 1.32, 1.23, 1.57 and
    1.86 u D, so B_EDGE alone would have held here (the kappa term is what the derivation can prove for a thin triangle)."""
    tris = property_sets()[name]
    pts = K.query_points(tris, 2000, 17, nonfinite=0)
    r = host(tris, pts)
    assert (r["prim"] >= 0).all()
    v64, w64 = r["v"].astype(np.float64), r["w"].astype(np.float64)
    assert (r["v"] >= 0).all() and (r["w"] >= 0).all() and (v64 + w64 <= 1.0).all()  # (the f64 sum of two f32 is exact)
    a = tris["a"][r["prim"], :3]
    e1 = (tris["b"][r["prim"], :3] - a).astype(np.float32)
    e2 = (tris["c"][r["prim"], :3] - a).astype(np.float32)
    ve, we = (r["v"][:, None] * e1).astype(np.float32), (r["w"][:, None] * e2).astype(np.float32)
    p = (a + (ve + we).astype(np.float32)).astype(np.float32)
    assert p.tobytes() == np.ascontiguousarray(r["p"]).tobytes()
    v, finite = U.tri_f64(tris)
    assert finite.all()
    dist, prim, inside = K.closest_f64(pts, v)
    root = hrt.lbvh_build(tris)["root"].astype(np.float64)
    D = np.linalg.norm(pts.astype(np.float64) - root[:3], axis=1) + root[3]
    err = np.abs(np.sqrt(r["d2"].astype(np.float64)) - dist)
    bound = (K.B_EDGE + np.where(inside, K.B_PLANE * K.kappa(v)[prim], 0.0)) * K.U24 * D
    print(f"{name}: largest error {np.max(err / (K.U24 * D)):.3f} u D, largest share of the bound {np.max(err / bound):.4f}")
    assert (err <= bound).all()


def test_cap_rules():
    tris = CASES["suzanne"]()
    pts = K.query_points(tris, 64, 9, nonfinite=0)
    free = host(tris, pts)
    assert (free["prim"] >= 0).all() and K.records_equal(free, host(tris, pts, None))
    miss = np.zeros(len(pts), dtype=hrt.CLOSEST_DTYPE)
    miss["d2"], miss["prim"] = MISS, -1
    for cap in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        got = host(tris, pts, np.full(len(pts), cap, dtype=np.float32))
        assert K.records_equal(got, miss), cap
    for cap in (np.inf, float(np.finfo(np.float32).max), float(MISS)):
        assert K.records_equal(host(tris, pts, np.full(len(pts), cap, dtype=np.float32)), free), cap
    away = free["d2"] > 0
    assert away.sum() > 16
    at = host(tris, pts, free["d2"])  # exactly the unconstrained d2: that triangle does not count, nor a farther one
    assert (at["prim"][away] == -1).all()
    assert K.records_equal(host(tris, pts, K.next_up(free["d2"]))[away], free[away])  # the next f32 above it: the hit
    assert K.records_equal(host(tris, pts, 1e30), free)  # a Python float for every point
    mixed = K.cap_mix(free["d2"], 4)
    got = host(tris, pts, mixed)
    want = lexicographic_minimum(tris, pts, mixed)
    assert K.records_equal(got, want), K.first_difference(got, want)
    assert 0 < (got["prim"] >= 0).sum() < len(pts)


def test_non_finite_points_are_misses():
    tris = CASES["cube"]()
    bad = K.query_points(tris, 12, 1, nonfinite=12)
    assert not np.isfinite(bad).all(axis=1).any()
    got = host(tris, bad)
    assert (got["prim"] == -1).all() and (got["d2"] == MISS).all()
    assert not got["p"].any() and not got["v"].any() and not got["w"].any() and not got["reserved"].any()


def test_overflowing_distance_is_a_miss_not_a_nan():
    tris = U.triangles_from_vertices(TRI * np.float32(1e37))
    pts = np.array([[-3e38, -3e38, 3e38], [3e38, 0, 0], [0, 0, 0], [4e37, 0, 0]], dtype=np.float32)
    got = host(tris, pts)
    # (p - a overflows, or the squared distance does: +inf is below no cap; a point on a vertex is still found)
    assert got["prim"].tolist() == [-1, -1, 0, 0] and got["d2"].tolist()[2:] == [0, 0] and not np.isnan(got["d2"]).any()
    one = hrt.closest_points_host(tris, pts[:2], float("inf"))
    assert (one["prim"] == -1).all() and (one["d2"] == MISS).all()


def test_arguments():
    L = hrt.lib()
    tris = CASES["cube"]()
    pts = np.zeros((2, 3), dtype=np.float32)
    out = np.zeros(2, dtype=hrt.CLOSEST_DTYPE)
    pf = pts.ctypes.data_as(_lib._PF)
    assert L.rt_host_closest_points(tris.ctypes.data, len(tris), None, None, 0, None) == _lib.RT_OK  # n = 0
    assert L.rt_host_closest_points(None, 0, pf, None, 2, out.ctypes.data) == _lib.RT_OK  # no triangles: misses
    assert (out["prim"] == -1).all() and (out["d2"] == MISS).all()
    assert L.rt_host_closest_points(None, len(tris), pf, None, 2, out.ctypes.data) == _lib.RT_ERR_ARG
    assert b"rt_host_closest_points" in L.rt_last_error()
    assert L.rt_host_closest_points(tris.ctypes.data, len(tris), None, None, 2, out.ctypes.data) == _lib.RT_ERR_ARG
    assert L.rt_host_closest_points(tris.ctypes.data, len(tris), pf, None, 2, None) == _lib.RT_ERR_ARG
    assert L.rt_closest_points(None, None, None, 0, None) == _lib.RT_ERR_ARG  # a null renderer, before any device
    assert len(hrt.closest_points_host(tris, np.zeros((0, 3), dtype=np.float32))) == 0
    with pytest.raises(ValueError):
        hrt.closest_points_host(tris, pts, np.zeros(3, dtype=np.float32))
