"""rt_cast_rays_multi on the host (rt_host_cast_rays_multi; hrt.cast_rays_multi_host): the symbols and statuses, the answer
on a stack of dyadic squares where every t is exact, paging by cursor, the walk against the flat definition on every tree
maker, the containment the exactness argument rests on, t, u, v against a float64 restatement, and how often the slab
clause changes the accepted set. CPU only; tests/test_gpu_multihit.py compares the device with these functions byte for
byte.

Measured here: of the 4,600 study rays on Suzanne (3,600 pixel centres of the Suzanne camera, 1,000 of
multihit_util.mesh_rays) the accepted set with the slab clause differs from the set of the triangle test alone on 0
(0.00 %); the test asserts at most 1 %.

The host functions were also run once as a stand-alone program (scripts/multihit_sanitize.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: clean. Nothing loaded into Python was run under a sanitizer."""
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
import multihit_util as M

ROOT = Path(__file__).resolve().parents[1]
PF = _lib._PF
MISS = M.MISS
CASES = dict(U.cpu_cases(), ico_sphere=lambda: U.mesh_triangles("ico_sphere.obj"), chain=M.chain)


# ------------------------------------------------------------------------------------------------ symbols and statuses
def test_symbols_layout_and_header():
    L = hrt.lib()  # (the parent fails here: no such symbol)
    assert L.rt_cast_rays_multi.restype is C.c_int
    header = (ROOT / "include" / "hrt.h").read_text()
    testing = (ROOT / "include" / "hrt_testing.h").read_text()
    names = ("rt_cast_rays_multi", "rt_host_cast_rays_multi")
    tnames = ("rt_testing_set_multihit_count", "rt_testing_get_multihit_counts")
    for name in names:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and getattr(L, name).restype is C.c_int
    for name in tnames:
        assert re.search(r"^int %s\(" % name, testing, re.M) and name not in header, name
        assert name in _lib.TESTING_SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert set(names + tnames) <= set(re.findall(r"\bT (rt_\w+)", out))
    assert "RT_ABI_VERSION 7u" in header
    comment = header[header.index("#define RT_ABI_VERSION"):header.index("int rt_abi_version")]
    assert "rt_cast_rays_multi" in comment and "rt_host_cast_rays_multi" in comment
    assert re.search(r"typedef struct rt_multi_hit \{ float t; int32_t prim; float u, v; \} rt_multi_hit;", header)
    assert "#define RT_MULTI_HIT_MAX_K 16u" in header and hrt.MULTI_HIT_MAX_K == 16
    dt = hrt.MULTI_HIT_DTYPE
    assert dt.itemsize == 16 and [dt.fields[k][1] for k in ("t", "prim", "u", "v")] == [0, 4, 8, 12]


def tree_args(tris, tree):
    nodes, order = np.ascontiguousarray(tree["nodes"]), np.ascontiguousarray(tree["order"])
    root = np.ascontiguousarray(tree["root"], dtype=np.float32)
    keep = (tris, nodes, order, root)
    return keep, [tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes), order.ctypes.data_as(_lib._PU32), len(order),
                  int(tree["info"][3]), root.ctypes.data_as(PF)]


def test_statuses():
    L = hrt.lib()
    tris = U.mesh_triangles("suzanne.obj")
    tree = hrt.lbvh_build(tris)
    keep, a = tree_args(tris, tree)
    o, d = M.mesh_rays(tris, 32, 1)
    po, pd = o.ctypes.data_as(PF), d.ctypes.data_as(PF)
    hits, cnt = np.zeros((32, 16), dtype=hrt.MULTI_HIT_DTYPE), np.zeros(32, dtype=np.uint32)
    ph, pc = hits.ctypes.data, cnt.ctypes.data_as(_lib._PU32)
    call = L.rt_host_cast_rays_multi
    assert L.rt_cast_rays_multi(None, None, None, None, None, 4, 1, None, None) == _lib.RT_ERR_ARG
    assert call(*a, po, pd, None, None, 32, 16, ph, pc) == _lib.RT_OK
    assert call(*a, po, pd, None, None, 32, 16, ph, None) == _lib.RT_OK
    assert call(*a, po, pd, None, None, 32, 0, None, pc) == _lib.RT_OK
    assert call(*a, po, pd, None, None, 32, 17, ph, pc) == _lib.RT_ERR_ARG and b"RT_MULTI_HIT_MAX_K" in L.rt_last_error()
    assert call(*a, po, pd, None, None, 32, 0, ph, None) == _lib.RT_ERR_ARG and b"counts" in L.rt_last_error()
    assert call(*a, po, pd, None, None, 32, 4, None, pc) == _lib.RT_ERR_ARG
    assert call(*a, None, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a, po, None, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a, None, None, None, None, 0, 4, None, None) == _lib.RT_OK
    assert call(None, len(tris), *a[2:], po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(a[0], a[1], None, a[3], *a[4:], po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a[:4], None, a[5], *a[6:], po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a[:7], None, po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # the root is always read
    # bytes that are no tree over these triangles
    assert call(a[0], 5, *a[2:], po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # order entries past n_tris
    assert call(*a[:6], len(tree["nodes"]), a[7], po, pd, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # root past the slots
    bad = dict(tree, nodes=tree["nodes"].copy())
    bad["nodes"][0, 7] = bad["nodes"][0, 3]  # one child named twice
    with pytest.raises(hrt.RtError):
        M.records(tris, bad, o, d, 4)
    # the flat definition: no nodes, the root alone is read
    assert call(a[0], a[1], None, 0, None, 0, 0, a[7], po, pd, None, None, 32, 16, ph, pc) == _lib.RT_OK
    flat, fc = M.records(tris, tree, o, d, 16, counts=True, flat=True)
    assert hits.tobytes() == flat.tobytes() and (cnt == fc).all()


# ------------------------------------------------------------------------------------------------ the stack of squares
SQUARES = 9


@pytest.fixture(scope="module", params=["flat", "lbvh", "ploc"])
def squares(request):
    tris = M.stack_of_squares(SQUARES)
    tree = hrt.lbvh_build(tris, 1 if request.param == "ploc" else 0)
    return tris, tree, request.param == "flat"


def z_rays(xy):
    o = np.array([[x, y, 0.0] for x, y in xy], dtype=np.float32)
    return o, np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (len(o), 1))


def test_interior_and_diagonal_rays(squares):
    tris, tree, flat = squares
    m = SQUARES
    o, d = z_rays([(0.75, 0.25), (0.25, 0.75), (0.5, 0.5), (0.25, 0.25)])
    h, c = M.records(tris, tree, o, d, 16, counts=True, flat=flat)
    layers = np.arange(1, m + 1, dtype=np.float32)
    assert c.tolist() == [m, m, 2 * m, 2 * m]
    for i, first in ((0, 0), (1, 1)):  # through the interior of the lower / the upper triangle of every square
        assert h["t"][i, :m].view(np.uint32).tolist() == layers.view(np.uint32).tolist()
        assert h["prim"][i, :m].tolist() == list(range(first, 2 * m, 2))
        assert (h["t"][i, m:] == MISS).all() and (h["prim"][i, m:] == -1).all()
        assert not h["u"][i, m:].view(np.uint32).any() and not h["v"][i, m:].view(np.uint32).any()  # the miss record
    for i in (2, 3):  # through the shared diagonal: both triangles of every square, the smaller index first
        assert h["t"][i].tolist() == np.repeat(layers, 2)[:16].tolist()
        assert h["prim"][i].tolist() == list(range(16))
    assert h["u"][0, 0] == 0.5 and h["v"][0, 0] == 0.25  # a + u e1 + v e2 = (0.75, 0.25): u = 0.5, v = 0.25
    # k < count keeps the first k; k = 0 counts
    for k in (1, 3, 5):
        hk, ck = M.records(tris, tree, o, d, k, counts=True, flat=flat)
        M.same_records(hk, np.ascontiguousarray(h[:, :k]), f"k = {k}")
        assert (ck == c).all()
        M.same_records(M.records(tris, tree, o, d, k, flat=flat), hk, f"k = {k} without counts")
    h0, c0 = M.records(tris, tree, o, d, 0, counts=True, flat=flat)
    assert h0.shape == (4, 0) and (c0 == c).all()


def test_cap_and_near_limit(squares):
    tris, tree, flat = squares
    m = SQUARES
    o, d = z_rays([(0.75, 0.25)] * 12)
    up = np.nextafter(np.float32(3.0), np.float32(np.inf))
    caps = np.array([3.0, up, np.nan, 0.0, -0.0, -1.0, np.inf, np.finfo(np.float32).max, 0.5, 1.0, 1e-5, 2.5], dtype=np.float32)
    want = [2, 3, 0, 0, 0, 0, m, m, 0, 0, 0, 2]  # a hit at t == cap is excluded
    h, c = M.records(tris, tree, o, d, 16, tmax=caps, counts=True, flat=flat)
    assert c.tolist() == want
    assert ((h["prim"] >= 0).sum(axis=1) == np.minimum(want, 16)).all()
    # t below 1e-4 is excluded, 1e-4 itself is not: origins just below the first square
    lim = np.float32(1e-4)
    z = np.array([1.0 - 1e-5, 1.0 - 3e-4, 1.0], dtype=np.float32)
    o3, d3 = z_rays([(0.75, 0.25)] * 3)
    o3[:, 2] = z
    t0 = (np.float32(1.0) - z).astype(np.float32)
    h3, c3 = M.records(tris, tree, o3, d3, 2, counts=True, flat=flat)
    assert t0[0] < lim <= t0[1] and c3.tolist() == [m - 1, m, m - 1]
    assert h3["t"][1, 0] == t0[1] and h3["prim"][0, 0] == 2 and h3["prim"][2, 0] == 2
    # a scaled direction scales t: the cut at 1e-4 is on the computed t, not on a distance
    d3s = d3 * np.float32(4096.0)
    hs, _ = M.records(tris, tree, o3, d3s, 1, counts=True, flat=flat)
    assert hs["prim"][1, 0] == 2  # t = 3e-4 / 4096 < 1e-4: the first square is left out now


@pytest.mark.parametrize("k", [1, 3, 16])
def test_paging_reproduces_the_whole_list(squares, k):
    tris, tree, flat = squares
    o, d = z_rays([(0.75, 0.25), (0.5, 0.5), (0.25, 0.25), (2.0, 2.0), (0.25, 0.75)])
    whole = M.ragged(M.paged(lambda after: M.records(tris, tree, o, d, 16, after=after, flat=flat), len(o), 16))
    assert [len(w) for w in whole] == [SQUARES, 2 * SQUARES, 2 * SQUARES, 0, SQUARES]
    got = M.ragged(M.paged(lambda after: M.records(tris, tree, o, d, k, after=after, flat=flat), len(o), k))
    for a, b in zip(got, whole):
        assert a.tobytes() == b.tobytes()
    # a miss record as cursor yields nothing; the counts beyond a cursor are what is left
    miss = np.zeros(len(o), dtype=hrt.MULTI_HIT_DTYPE)
    miss["t"], miss["prim"] = MISS, -1
    h, c = M.records(tris, tree, o, d, k, after=miss, counts=True, flat=flat)
    assert (h["prim"] == -1).all() and not c.any()
    first = M.records(tris, tree, o, d, k, flat=flat)
    _, left = M.records(tris, tree, o, d, 0, after=np.ascontiguousarray(first[:, k - 1]), counts=True, flat=flat)
    assert left.tolist() == [max(len(w) - k, 0) for w in whole]


# ------------------------------------------------------------------------------------------------ the walk is the definition
def trees_of(tris):
    """(name, triangles the tree is over, tree): both builders, and each refitted to the moved triangles."""
    moved = K.moved(tris, (0.375, -1.25, 2.0))
    out = []
    for b in M.BUILDERS:
        out.append((f"builder{b}", tris, hrt.lbvh_build(tris, b)))
        out.append((f"builder{b}-refit", moved, hrt.lbvh_refit(tris, moved, b)))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_equals_the_flat_definition(name):
    tris = CASES[name]()
    overflowed = False
    for tag, t, tree in trees_of(tris):
        o, d = M.chain_rays() if name == "chain" and "refit" not in tag else M.mesh_rays(t, 200, 5)
        flat, fc = M.records(t, tree, o, d, 16, counts=True, flat=True)
        caps = M.cap_mix(flat["t"][:, 0], 3)
        cursor = np.ascontiguousarray(flat[:, 1])
        for kw in (dict(), dict(tmax=caps), dict(after=cursor), dict(tmax=caps, after=cursor)):
            want, wc = (flat, fc) if not kw else M.records(t, tree, o, d, 16, counts=True, flat=True, **kw)
            for k in (0, 1, 4, 16):
                got, gc = M.records(t, tree, o, d, k, counts=True, **kw)
                M.same_records(got, np.ascontiguousarray(want[:, :k]), f"{name} {tag} k = {k} {sorted(kw)} with counts")
                assert (gc == wc).all(), (name, tag, k, sorted(kw))
                if k:
                    M.same_records(M.records(t, tree, o, d, k, **kw), np.ascontiguousarray(want[:, :k]),
                                   f"{name} {tag} k = {k} {sorted(kw)}")
        if name == "chain" and tag == "builder1":
            assert int(tree["info"][4]) > 24 and fc.max() >= 16  # deeper than the stack, and rays that cross it all
            overflowed = True
    assert overflowed == (name == "chain")


@pytest.mark.parametrize("name", sorted(CASES))
def test_containment(name):
    """Every triangle's own box (the definition's) lies inside every ancestor's decoded fp16 box: LBVH, PLOC, and both
    after a refit. (The host SAH tree is read back from a renderer: tests/test_gpu_multihit.py.)"""
    tris = CASES[name]()
    finite = int(U.tri_f64(tris)[1].sum())
    for tag, t, tree in trees_of(tris):
        assert M.check_containment(t, tree) == finite, (name, tag)


# ------------------------------------------------------------------------------------------------ accuracy, and the slab clause
def test_t_u_v_against_f64_on_suzanne():
    tris, tree, o, d, _, _ = M.suzanne_study()
    o, d = o[:3600], d[:3600]  # the camera's rays (the others aim at vertices and edges, which the reference leaves out)
    h = M.records(tris, tree, o, d, 4)
    ray, rank = np.nonzero(h["prim"] >= 0)
    assert len(ray) > 2000
    t64, u64, v64, kept, bound, bu, bv = M.triangle_reference(o[ray], d[ray], tris[h["prim"][ray, rank]])
    t, u, v = (h[f][ray, rank].astype(np.float64) for f in ("t", "u", "v"))
    left_out = 1.0 - kept.mean()
    ratio = np.abs(t[kept] - t64[kept]) / bound[kept]
    ru, rv = np.abs(u[kept] - u64[kept]) / bu[kept], np.abs(v[kept] - v64[kept]) / bv[kept]
    print(f"left out {100 * left_out:.2f} %, largest |t - t64| / bound = {ratio.max():.4f}, u {ru.max():.4f}, v {rv.max():.4f} "
          f"over {int(kept.sum())}")
    assert left_out <= 0.05
    assert (ratio <= 1.0).all(), (ratio.max(), int((ratio > 1).sum()))
    assert (ru <= 1.0).all() and (rv <= 1.0).all(), (ru.max(), rv.max())
    assert (h["t"][ray, rank] >= np.float32(1e-4)).all()


def test_the_slab_clause_changes_few_rays():
    tris, tree, o, d, unchanged, with_slab = M.suzanne_study()
    changed = int((~unchanged).sum())
    hits = sum(len(w) for w in with_slab)
    print(f"slab clause: the accepted set differs on {changed} of {len(o)} rays ({100.0 * changed / len(o):.2f} %); "
          f"{hits} hits in all")
    assert hits > 5000
    assert changed <= 0.01 * len(o)
