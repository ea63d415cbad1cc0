"""rt_refit_triangles_device's host mirror (rt_host_lbvh_refit, hrt.lbvh_refit) and the tree cost (rt_host_lbvh_cost,
hrt.lbvh_cost): the symbols are there and bound; a refit with the unmoved array is the build, byte for byte; a refit with
moved triangles keeps the build's topology and gives boxes that contain the moved triangles; the cost is the documented
function of the tree's bytes. CPU only; tests/test_gpu_lbvh_refit.py compares the device refit with this one.

The two host functions were also run as a stand-alone program (its own main over csrc/rt_lbvh.hpp) under
AddressSanitizer and UndefinedBehaviorSanitizer (DESIGN.md §7d Refit has the inputs): clean."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

import lbvh_refit_util as R
import lbvh_util as U

ROOT = Path(__file__).resolve().parents[1]
SHAPES = R.shapes()
NEW = ("rt_refit_triangles_device", "rt_host_lbvh_refit", "rt_host_lbvh_cost", "rt_get_tri_tree_cost")


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "hrt.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    L = hrt.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes is not None
    m = re.search(r"#define RT_ABI_VERSION 7u /\*(.*?)\*/", header, re.S)
    assert m, "RT_ABI_VERSION stays 7 (no struct changed)"
    for name in NEW:
        assert name in m.group(1), name  # detected by their symbols: the comment says so
    assert callable(hrt.lbvh_refit) and callable(hrt.lbvh_cost)
    assert hasattr(hrt.Renderer, "refit_triangles_device") and hasattr(hrt.Renderer, "tri_tree_cost")
    # the renderer calls refuse what they can before they need a device
    cost = (C.c_uint64 * 4)()
    assert L.rt_refit_triangles_device(None, None, 0) == _lib.RT_ERR_ARG
    assert L.rt_get_tri_tree_cost(None, cost) == _lib.RT_ERR_ARG


@pytest.mark.parametrize("name", list(SHAPES))
def test_refit_with_the_unmoved_array_is_the_build(name):
    a = SHAPES[name]()
    U.same_tree(hrt.lbvh_refit(a, a), hrt.lbvh_build(a))
    U.same_tree(hrt.lbvh_refit(a, a.copy()), hrt.lbvh_build(a))


@pytest.mark.parametrize("kind", R.DEFORMATIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_refit_keeps_the_topology_and_bounds_the_moved_triangles(name, kind):
    a = SHAPES[name]()
    b = R.deform(a, kind)
    built, tree = hrt.lbvh_build(a), hrt.lbvh_refit(a, b)
    assert tree["order"].tobytes() == built["order"].tobytes()
    assert R.child_words(tree).tobytes() == R.child_words(built).tobytes()
    # slots no child word names are zero, every child's decoded box contains the f64 boxes of b's triangles beneath it,
    # info is consistent with the tree (lbvh_util.check_tree checks all of the format against b)
    U.check_tree(b, tree)
    assert tree["info"].tolist() == built["info"].tolist()  # node slots, leaves, finite, root word and the depth
    U.same_tree(tree, hrt.lbvh_refit(a, b.copy()))
    if kind == "translate" and int(tree["info"][2]):  # (the boxes are relative to the root centre, which has moved)
        assert abs(float(tree["root"][0]) - 1000.0) < 10.0 and abs(float(built["root"][0])) < 10.0
    if kind == "collapse" and int(tree["info"][2]):
        assert tree["root"][:3].tolist() == [0.5, -1.25, 2.0]


def test_walk_of_a_refitted_tree_finds_the_brute_force_triangle():
    """256 rays on Suzanne with every triangle displaced on its own: the walk of the refitted tree, culling with its
    boxes, finds the (t, index) minimum a loop over all moved triangles finds."""
    a = SHAPES["suzanne"]()
    b = R.deform(a, "scatter", amount=0.1)
    tree = hrt.lbvh_refit(a, b)
    v, finite = U.tri_f64(b)
    assert finite.all()
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    rng = np.random.default_rng(12)
    hits = 0
    for k in range(256):
        o = 0.5 * (lo + hi) + rng.normal(size=3) * 3.0 * (hi - lo).max()
        d = rng.uniform(lo, hi) - o
        d /= np.linalg.norm(d)
        if k % 16 == 0:
            d[k // 16 % 3] = 0.0  # axis-parallel rays too
        t = U.moller_trumbore(o, d, v)
        bt = t.min()
        bj = int(np.flatnonzero(t == bt)[0]) if np.isfinite(bt) else -1
        wt, wj = U.walk(o, d, v, tree)
        assert (wj, wt) == (bj, bt) or (bj < 0 and wj < 0), (k, wj, wt, bj, bt)
        hits += bj >= 0
    assert hits > 50  # (the rays do aim at the mesh; the scattered triangles leave gaps the whole mesh has not)


def test_finiteness_mismatch_and_capacities():
    L = hrt.lib()
    with_nan, without = U.nan_triangles(), U.random_triangles(9, 77)
    for topo, now in ((without, with_nan), (with_nan, without)):  # a NaN introduced, a NaN removed
        with pytest.raises(hrt.RtError) as e:
            hrt.lbvh_refit(topo, now)
        assert e.value.code == _lib.RT_ERR_ARG and "finite" in str(e.value)
    moved = with_nan.copy()
    moved["a"][4, 0] = np.inf  # not finite in another way: the same set
    assert int(hrt.lbvh_refit(with_nan, moved)["info"][2]) == 8
    with pytest.raises(ValueError):
        hrt.lbvh_refit(without, without[:8])
    info, root = (C.c_uint32 * 8)(), (C.c_float * 4)()
    t, b = without, R.deform(without, "jitter")
    pt, pb = t.ctypes.data, b.ctypes.data
    assert L.rt_host_lbvh_refit(pt, pb, 9, None, 0, None, 0, None, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(None, pb, 9, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, None, 9, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, pb, 1 << 26, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, pb, 9, None, 0, None, 0, info, root) == _lib.RT_OK  # sizes only
    assert list(info)[:3] == [8, 9, 9]
    nodes, order = np.zeros((8, 8), np.uint32), np.zeros(9, np.uint32)
    po = order.ctypes.data_as(_lib._PU32)
    assert L.rt_host_lbvh_refit(pt, pb, 9, nodes.ctypes.data, 7, po, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, pb, 9, nodes.ctypes.data, 8, po, 8, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, pb, 9, nodes.ctypes.data, 8, None, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit(pt, pb, 9, nodes.ctypes.data, 8, po, 9, info, root) == _lib.RT_OK
    assert nodes.tobytes() == hrt.lbvh_refit(t, b)["nodes"].tobytes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_cost_counts_and_formula(name):
    a = SHAPES[name]()
    for tree in (hrt.lbvh_build(a), hrt.lbvh_refit(a, R.deform(a, "scatter"))):
        cost = hrt.lbvh_cost(tree)
        assert cost.dtype == np.uint64 and cost.shape == (4,)
        nodes = tree["nodes"]
        if int(tree["info"][3]) & U.LEAF_BIT:
            assert cost.tolist() == [0, 0, 0, 0] and len(nodes) == 0  # a tree without nodes
            continue
        words = R.child_words(tree)[nodes[:, 3] != 0].ravel()
        leaves = words[(words & U.LEAF_BIT) != 0]
        assert int(cost[2]) == int((nodes[:, 3] != 0).sum()) and int(cost[3]) == int((leaves & 15).sum())
        assert int(cost[3]) == int(tree["info"][1])  # every leaf position is in one leaf
        assert cost.tolist() == R.numpy_cost(tree)
        again = {k: v.copy() for k, v in tree.items()}
        assert hrt.lbvh_cost(again).tolist() == cost.tolist()  # the same bytes in, the same cost out


def test_cost_of_a_scattered_refit_is_above_a_fresh_builds():
    """Suzanne, every triangle displaced by its own vector of sigma a quarter of the root extent: the refitted tree's
    boxes overlap far more than a build's over the same triangles (measured on the host: 8.3 x the SAH figure; 3.6 x at a
    tenth of the extent)."""
    a = SHAPES["suzanne"]()
    b = R.deform(a, "scatter", amount=0.25)
    refit, fresh = hrt.lbvh_cost(hrt.lbvh_refit(a, b)), hrt.lbvh_cost(hrt.lbvh_build(b))
    assert int(refit[0]) + int(refit[1]) > int(fresh[0]) + int(fresh[1])
    assert int(refit[3]) == int(fresh[3]) == len(a)
    L = hrt.lib()
    cost = (C.c_uint64 * 4)()
    nodes = hrt.lbvh_build(a)["nodes"]
    assert L.rt_host_lbvh_cost(nodes.ctypes.data, len(nodes), len(nodes), cost) == _lib.RT_ERR_ARG  # no such root node
    assert L.rt_host_lbvh_cost(nodes.ctypes.data, len(nodes), 0, None) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_cost(None, 0, U.LEAF_BIT | 3, cost) == _lib.RT_OK and list(cost) == [0, 0, 0, 0]
