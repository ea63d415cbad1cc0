"""rt_set_triangles_device's builder on the host (rt_host_lbvh_build, hrt.lbvh_build): the symbols are there and bound,
and the tree it makes is a valid tree of the documented format for every shape the builder has a special path for. CPU
only; tests/test_gpu_lbvh.py compares the device build with this one byte for byte.

The host builder was also run once as a stand-alone program (its own main over csrc/rt_lbvh.hpp, random, identical,
planar and non-finite triangles) under AddressSanitizer and UndefinedBehaviorSanitizer: clean."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

import lbvh_util as U

ROOT = Path(__file__).resolve().parents[1]
CASES = U.cpu_cases()


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "hrt.h").read_text()
    testing = (ROOT / "include" / "hrt_testing.h").read_text()
    for name in ("rt_set_triangles_device", "rt_host_lbvh_build"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r"^int rt_testing_get_tri_tree\(", testing, re.M)
    assert "rt_testing_get_tri_tree" in _lib.TESTING_SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    assert {"rt_set_triangles_device", "rt_host_lbvh_build", "rt_testing_get_tri_tree"} <= exported
    L = hrt.lib()
    assert L.rt_host_lbvh_build.argtypes is not None and L.rt_set_triangles_device.restype is C.c_int
    assert "RT_ABI_VERSION 7u" in header  # (no struct changed: the calls are detected by their symbols)
    assert callable(hrt.lbvh_build) and hasattr(hrt.Renderer, "set_triangles_device") and hasattr(hrt.Renderer, "tri_tree")


def test_arguments():
    L = hrt.lib()
    info, root = (C.c_uint32 * 8)(), (C.c_float * 4)()
    t = U.random_triangles(9, 5)
    assert L.rt_host_lbvh_build(t.ctypes.data, 9, None, 0, None, 0, None, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build(None, 9, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build(t.ctypes.data, 1 << 26, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build(t.ctypes.data, 9, None, 0, None, 0, info, root) == _lib.RT_OK  # sizes only
    assert list(info)[:3] == [8, 9, 9]
    nodes, order = np.zeros((8, 8), np.uint32), np.zeros(9, np.uint32)
    po = order.ctypes.data_as(_lib._PU32)
    assert L.rt_host_lbvh_build(t.ctypes.data, 9, nodes.ctypes.data, 7, po, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build(t.ctypes.data, 9, nodes.ctypes.data, 8, po, 8, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build(t.ctypes.data, 9, nodes.ctypes.data, 8, po, 9, info, root) == _lib.RT_OK
    # the renderer call refuses what it can before it needs a device
    assert L.rt_set_triangles_device(None, None, 0, None, 0) == _lib.RT_ERR_ARG
    # (m, 16) float32 rows are the same records
    U.same_tree(hrt.lbvh_build(t), hrt.lbvh_build(t.view(np.float32).reshape(-1, 16)))


@pytest.mark.parametrize("name", list(CASES))
def test_tree_is_valid(name):
    tris = CASES[name]()
    tree = hrt.lbvh_build(tris)
    U.check_tree(tris, tree)
    U.same_tree(tree, hrt.lbvh_build(tris.copy()))  # a pure function of the input
    m = len(tris)
    if name == "nan1of9":
        assert 4 not in tree["order"].tolist() and int(tree["info"][2]) == 8
    elif name.startswith("random") or name in ("identical70", "planar"):
        assert int(tree["info"][2]) == m
    if name == "identical70":  # all keys equal: the index tie-break alone shapes the tree, and it is balanced
        assert int(tree["info"][4]) <= 7
        assert tree["order"].tolist() == list(range(70))  # (the sort is stable)
    if name == "random0":
        assert int(tree["info"][3]) == U.LEAF_BIT and len(tree["order"]) == 0
    if name in ("random1", "random4"):
        assert int(tree["info"][3]) == (U.LEAF_BIT | m) and len(tree["nodes"]) == 0


def test_walk_finds_the_brute_force_triangle():
    """256 rays on Suzanne: a walk of the mirrored tree that culls with the stored boxes finds the triangle a loop over
    all triangles finds (the (t, index) lexicographic minimum, same arithmetic)."""
    tris = CASES["suzanne"]()
    tree = hrt.lbvh_build(tris)
    v, finite = U.tri_f64(tris)
    assert finite.all()
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    rng = np.random.default_rng(11)
    hits = 0
    for k in range(256):
        o = 0.5 * (lo + hi) + rng.normal(size=3) * 3.0 * (hi - lo).max()
        target = rng.uniform(lo, hi)
        d = target - o
        d /= np.linalg.norm(d)
        if k % 16 == 0:
            d[k // 16 % 3] = 0.0  # axis-parallel rays too
        t = U.moller_trumbore(o, d, v)
        bt = t.min()
        bj = int(np.flatnonzero(t == bt)[0]) if np.isfinite(bt) else -1
        wt, wj = U.walk(o, d, v, tree)
        assert (wj, wt) == (bj, bt) or (bj < 0 and wj < 0), (k, wj, wt, bj, bt)
        hits += bj >= 0
    assert hits > 100  # (the rays do aim at the mesh)
