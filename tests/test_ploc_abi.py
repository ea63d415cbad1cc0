"""The PLOC builder on the host (rt_host_lbvh_build_with / rt_host_lbvh_refit_with, hrt.lbvh_build(..., builder=1)): the
symbols are there and bound, builder 0 through the new calls is the old calls' bytes, and builder 1 makes a valid tree of
the documented format, by the documented rules, for every shape the builder has a special path for. CPU only;
tests/test_gpu_ploc.py compares the device build with this one byte for byte.

The host mirror was also run once as a stand-alone program (its own main over csrc/rt_lbvh.hpp: sizes 0 to 100,000,
identical, planar, non-finite, 1e37-scaled and subnormal triangles, and the chain) under AddressSanitizer and
UndefinedBehaviorSanitizer: clean."""
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
PLOC = 1
RADIUS = 8
RANDOM_SIZES = (0, 1, 4, 5, 6, 9, 17, 64, 65, 1023, 1024, 1025, 1026, 2049)


def chain_triangles(m: int = 230) -> np.ndarray:
    """Triangles (x, 0, 0), (x, 1, 0), (x, 0, 1) with x = 1e-37 * 2.1^i: every cluster's nearest neighbour is the one
    before it, so one pair merges per iteration until flat mode ends the build at 64 iterations."""
    x = (1e-37 * 2.1 ** np.arange(m, dtype=np.float64)).astype(np.float32)
    v = np.zeros((m, 3, 3), dtype=np.float32)
    v[:, :, 0] = x[:, None]
    v[:, 1, 1] = 1.0
    v[:, 2, 2] = 1.0
    return U.triangles_from_vertices(v)


def ploc_cases() -> dict:
    """name -> a function that makes the triangles; the GPU tests add lucy."""
    cases = {"cube": lambda: U.mesh_triangles("cube.obj"), "quad": lambda: U.mesh_triangles("quad.obj"),
             "suzanne": lambda: U.mesh_triangles("suzanne.obj")}
    for m in RANDOM_SIZES:
        cases[f"random{m}"] = lambda m=m: U.random_triangles(m, 3000 + m)
    cases["identical70"] = U.identical_triangles
    cases["planar"] = U.planar_triangles
    cases["nan1of9"] = U.nan_triangles
    cases["chain230"] = chain_triangles
    return cases


CASES = ploc_cases()


def check_ploc_tree(tris: np.ndarray, tree: dict) -> int:
    """U.check_tree (which knows info[5:] as zeros: it sees a copy without the two iteration counts) and what builder 1
    promises beyond the format. Returns the deepest leaf."""
    plain = dict(tree, info=tree["info"].copy())
    plain["info"][5:7] = 0
    U.check_tree(tris, plain)
    nodes, info = tree["nodes"], tree["info"]
    m = int(info[2])
    assert int(info[7]) == 0 and int(info[6]) <= int(info[5]) <= 64
    if m <= U.LEAF_MAX:
        assert list(info[5:]) == [0, 0, 0] and len(nodes) == 0
        return 0
    words = nodes[:, [3, 7]]
    assert len(nodes) == m - 1 and (words[:, 0] != 0).all()  # every slot is referenced
    leaf = (words & U.LEAF_BIT) != 0
    assert ((words[leaf] & 15) == 1).all() and int(leaf.sum()) == m  # one triangle per leaf
    ids = np.arange(m - 1, dtype=np.uint32)[:, None]
    assert (words[~leaf] > np.broadcast_to(ids, words.shape)[~leaf]).all()  # a child's id is above its parent's
    depth = np.zeros(m - 1, dtype=np.int64)  # of the node; children come after parents in id order
    deepest = 0
    for i in range(m - 1):
        for w in words[i].tolist():
            if w & U.LEAF_BIT:
                deepest = max(deepest, int(depth[i]) + 1)
            else:
                depth[w] = depth[i] + 1
    assert int(info[4]) == deepest
    return deepest


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "hrt.h").read_text()
    names = ("rt_set_triangles_device_with", "rt_host_lbvh_build_with", "rt_host_lbvh_refit_with", "rt_get_tri_tree_info")
    for name in names:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r"^#define RT_TREE_LBVH 0u", header, re.M) and re.search(r"^#define RT_TREE_PLOC 1u", header, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert set(names) <= set(re.findall(r"\bT (rt_\w+)", out))
    assert "RT_ABI_VERSION 7u" in header  # (no struct changed: the calls are detected by their symbols)
    assert hrt.lib().rt_get_tri_tree_info.restype is C.c_int


@pytest.mark.parametrize("name", list(U.cpu_cases()))
def test_builder_0_is_the_old_calls_bytes(name):
    a = U.cpu_cases()[name]()
    U.same_tree(hrt.lbvh_build(a, builder=0), hrt.lbvh_build(a))
    b = R.deform(a, "jitter")
    U.same_tree(hrt.lbvh_refit(a, b, builder=0), hrt.lbvh_refit(a, b))
    assert list(hrt.lbvh_build(a, builder=0)["info"][5:]) == [0, 0, 0]


@pytest.mark.parametrize("name", list(CASES))
def test_ploc_tree_is_valid(name):
    tris = CASES[name]()
    tree = hrt.lbvh_build(tris, builder=PLOC)
    check_ploc_tree(tris, tree)
    U.same_tree(hrt.lbvh_build(tris, builder=PLOC), tree)  # a second call: the same bytes
    m = int(tree["info"][2])
    if m <= U.LEAF_MAX:  # builder 0's tree, bytes included
        U.same_tree(tree, hrt.lbvh_build(tris))
    else:
        assert (tree["order"] == hrt.lbvh_build(tris)["order"]).all()  # up to the sort nothing changes
    if name == "nan1of9":
        assert m == 8 and 4 not in tree["order"].tolist()


def numpy_ploc_words(tris: np.ndarray, order: np.ndarray):
    """The iteration restated with plain loops: (child words per node id, iterations)."""
    v, _ = U.tri_f64(tris)
    v = v + 0.0  # (-0 -> +0)
    clusters = [(v[j].min(axis=0), v[j].max(axis=0), U.LEAF_BIT | p << 4 | 1) for p, j in enumerate(order.tolist())]
    m = len(clusters)
    words, nxt, t = {}, m - 1, 0
    while len(clusters) > 1:
        c = len(clusters)
        flat = t + int(np.ceil(np.log2(c))) >= 64
        nn = []
        for i in range(c):
            best = None
            for j in range(max(0, i - RADIUS), min(c - 1, i + RADIUS) + 1):
                if j == i:
                    continue
                e = np.maximum(clusters[i][1], clusters[j][1]) - np.minimum(clusters[i][0], clusters[j][0])
                d = 0.0 if flat else float((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0])
                if best is None or (d, i ^ j) < best[:2]:
                    best = (d, i ^ j, j)
            nn.append(best[2])
        lower = [i for i in range(c) if nn[nn[i]] == i and i < nn[i]]
        k = len(lower)
        assert k >= 1
        out = []
        for i in range(c):
            j = nn[i]
            if nn[j] == i and j < i:
                continue
            if nn[j] == i:
                node = nxt - k + lower.index(i)
                words[node] = (clusters[i][2], clusters[j][2])
                out.append((np.minimum(clusters[i][0], clusters[j][0]), np.maximum(clusters[i][1], clusters[j][1]), node))
            else:
                out.append(clusters[i])
        clusters, nxt, t = out, nxt - k, t + 1
    assert nxt == 0
    return words, t


@pytest.mark.parametrize("m", [5, 17, 65])
def test_numpy_restatement_gives_the_same_words(m):
    tris = U.random_triangles(m, 3000 + m)
    tree = hrt.lbvh_build(tris, builder=PLOC)
    words, t = numpy_ploc_words(tris, tree["order"])
    assert t == int(tree["info"][5]) and int(tree["info"][6]) == 0
    assert [list(words[i]) for i in range(m - 1)] == tree["nodes"][:, [3, 7]].tolist()


def test_chain_runs_into_flat_mode_and_identical_triangles_pair_up():
    chain = hrt.lbvh_build(chain_triangles(), builder=PLOC)
    assert int(chain["info"][5]) == 64 and int(chain["info"][6]) >= 1 and int(chain["info"][4]) == 64
    same = hrt.lbvh_build(U.identical_triangles(70), builder=PLOC)
    assert int(same["info"][5]) == 7 and int(same["info"][6]) == 0


def sah(tree: dict) -> float:
    c = hrt.lbvh_cost(tree)
    return (int(c[0]) + int(c[1])) / 65536


@pytest.mark.parametrize("asset, recorded", [("suzanne.obj", 9.95), ("lucy_lp_20.obj", 32.85),
                                             ("xyzrgb_dragon_lp_20.obj", 27.02)])
def test_ploc_tree_costs_less_than_the_lbvh(asset, recorded):
    """The SAH read-out of builder 1 is below builder 0's (DESIGN.md §7d records 9.95 / 32.85 / 27.02 against 20.38 /
    44.39 / 33.98: a pure function of the mesh, so the recorded figures are checked to the digits recorded)."""
    tris = U.mesh_triangles(asset)
    lbvh, ploc = hrt.lbvh_build(tris), hrt.lbvh_build(tris, builder=PLOC)
    print(asset, "SAH", sah(lbvh), sah(ploc), "depth", lbvh["info"][4], ploc["info"][4], "iterations", ploc["info"][5])
    assert sah(ploc) < sah(lbvh)
    assert round(sah(ploc), 2) == recorded
    assert hrt.lbvh_cost(ploc).tolist() == R.numpy_cost(ploc)


@pytest.mark.parametrize("name", ["suzanne", "random1025", "identical70", "nan1of9", "chain230", "random4"])
def test_refit_keeps_the_topology(name):
    a = CASES[name]()
    built = hrt.lbvh_build(a, builder=PLOC)
    U.same_tree(hrt.lbvh_refit(a, a, builder=PLOC), built)
    for kind in R.DEFORMATIONS:
        b = R.deform(a, kind)
        tree = hrt.lbvh_refit(a, b, builder=PLOC)
        assert (R.child_words(tree) == R.child_words(built)).all() and (tree["order"] == built["order"]).all()
        assert tree["info"][:4].tolist() == built["info"][:4].tolist()
        assert tree["info"][5:].tolist() == built["info"][5:].tolist()
        check_ploc_tree(b, tree)  # the boxes contain the moved triangles


def test_walk_finds_the_brute_force_triangle():
    """256 rays on Suzanne through the builder-1 tree, as tests/test_lbvh_abi.py does for builder 0."""
    tris = CASES["suzanne"]()
    tree = hrt.lbvh_build(tris, builder=PLOC)
    v, finite = U.tri_f64(tris)
    assert finite.all()
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    rng = np.random.default_rng(11)
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
    assert hits > 100  # (the rays do aim at the mesh)


def test_refusals():
    L = hrt.lib()
    tris = U.random_triangles(9, 1)
    info, root = (C.c_uint32 * 8)(), (C.c_float * 4)()
    p = tris.ctypes.data
    for builder in (2, 7, 0xFFFFFFFF):  # unknown builders
        assert L.rt_host_lbvh_build_with(p, 9, builder, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
        assert L.rt_host_lbvh_refit_with(p, p, 9, builder, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
        with pytest.raises(hrt.RtError):
            hrt.lbvh_build(tris, builder=builder)
    with pytest.raises(ValueError):
        hrt.lbvh_build(tris, builder=-1)
    # the capacity rules of rt_host_lbvh_build
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, None, 0, None, 0, info, root) == _lib.RT_OK
    assert list(info)[:4] == [8, 9, 9, 0]
    nodes, order = np.zeros((8, 8), np.uint32), np.zeros(9, np.uint32)
    po = order.ctypes.data_as(_lib._PU32)
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, nodes.ctypes.data, 7, po, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, nodes.ctypes.data, 8, po, 8, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, None, 8, po, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_refit_with(p, p, 9, PLOC, nodes.ctypes.data, 7, po, 9, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, nodes.ctypes.data, 8, po, 9, None, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build_with(None, 9, PLOC, None, 0, None, 0, info, root) == _lib.RT_ERR_ARG
    assert L.rt_host_lbvh_build_with(p, 9, PLOC, nodes.ctypes.data, 8, po, 9, info, root) == _lib.RT_OK
    assert nodes.tobytes() == hrt.lbvh_build(tris, builder=PLOC)["nodes"].tobytes()
    # a triangle finite in one array and not in the other, either way
    with pytest.raises(hrt.RtError) as e:
        hrt.lbvh_refit(tris, U.nan_triangles(), builder=PLOC)
    assert e.value.code == _lib.RT_ERR_ARG and "finite" in str(e.value)
    with pytest.raises(hrt.RtError):
        hrt.lbvh_refit(U.nan_triangles(), U.random_triangles(9, 77), builder=PLOC)
