"""The four tree queries' device entry points through what they share (the prelude that refuses a
renderer without a triangle tree, the tree fields of the launch arguments, the counter slot, the wave epilogue of the
counting kernels): rt_closest_points, rt_winding_numbers, rt_cast_rays_multi and rt_overlap_volumes (both kinds), on
cube.obj with device geometry and with the host SAH tree of tri_bvh = 1, and on quad.obj (no nodes), at n = 1, 63, 65 and
257 queries: a partial wave, one wave and a lane, more than one workgroup.

With counting on, counter word 0 is n (the inactive lanes of a partial wave add 0 through the shared epilogue) and the other
words are COUNTS, which commit 821176f gave for the same calls (its kernels added each word with code of their own); the
outputs are the host mirror's bytes. With counting off again the product kernel gives the same bytes and the counters read
back what the last counted call left. A renderer without a triangle tree is refused with the texts of 821176f."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import Material, Mesh, Tree, Vec3, _lib, read_asset

import closest_util as K
import lbvh_util as U
import multihit_util as M
import overlap_util as V
from test_gpu_lbvh import ONE_MATERIAL, on_device

pytestmark = pytest.mark.gpu

NS = (1, 63, 65, 257)
TREES = ("cube device", "cube tri_bvh", "quad device")
QUERIES = ("closest", "winding", "multihit", "overlap box", "overlap ball")
NO_SPHERE_TREE = "the sphere program has no triangle tree"
NO_TREE = "no triangle tree (device geometry or rt_params.tri_bvh = 1 has one)"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


_made = {}


def renderer(tree: str):
    """(renderer, its triangles), made once per tree."""
    if tree not in _made:
        asset = tree.split()[0] + ".obj"
        r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
        if tree.endswith("device"):
            tris = U.mesh_triangles(asset)
            r.set_triangles_device(on_device(r, tris), ONE_MATERIAL)
        else:
            t = Tree.from_mesh(Mesh.load_obj(read_asset(asset), Material.new_lambertian(Vec3(0.5, 0.5, 0.5))))
            t.build()
            view = t.view()
            tris = view[2].copy()
            r.write_bvh(*view)
            r.set_params(tri_bvh=1)
        _made[tree] = (r, tris)
    return _made[tree]


def run(query: str, r, tris, n: int):
    """One call of n queries drawn as the query's own util draws them: (device bytes, the host mirror's bytes)."""
    tree = r.tri_tree()
    if query == "closest":
        pts = np.ascontiguousarray(K.query_points(tris, NS[-1], 11)[:n])
        return r.closest_records(pts).cpu().numpy().tobytes(), hrt.closest_points_host(tris, pts).tobytes()
    if query == "winding":
        pts = np.ascontiguousarray(K.query_points(tris, NS[-1], 12)[:n])
        return r.winding_numbers(pts, 2.0).cpu().numpy().tobytes(), hrt.winding_numbers_host(tris, tree, pts, 2.0).tobytes()
    if query == "multihit":
        o, d = (np.ascontiguousarray(x[:n]) for x in M.mesh_rays(tris, NS[-1], 13))
        rec, cnt = r.cast_rays_multi_records(o, d, 4, counts=True)
        want, wc = M.records(tris, tree, o, d, 4, counts=True)
    else:
        kind = V.BOX if query == "overlap box" else V.BALL
        vol = np.ascontiguousarray(V.volumes_for(kind, tris, NS[-1], 14)[:n])
        rec, cnt = r.overlap_records(kind, vol, 4, counts=True)
        want, wc = V.records(tris, tree, kind, vol, 4, counts=True)
    return rec.cpu().numpy().tobytes() + cnt.cpu().numpy().tobytes(), want.tobytes() + wc.tobytes()


def counting(query: str, r):
    """(switch, read-out) of the query's counting instantiation."""
    name = query.split()[0]
    return getattr(r, f"set_{name}_count"), getattr(r, f"{name}_counts")


def counted(query: str, tree: str, n: int):
    """The counter words of one counted call, after its bytes are checked against the mirror."""
    r, tris = renderer(tree)
    switch, read = counting(query, r)
    switch(True)
    try:
        got, want = run(query, r, tris, n)
    finally:
        switch(False)
    assert got == want, (query, tree, n)
    return [int(x) for x in read()]


# (query, tree) -> the counter words after word 0, for n = 1, 63, 65, 257 (commit 821176f, MI355X)
COUNTS = {
    ("closest", "cube device"): [[12, 0, 0], [756, 0, 0], [780, 0, 0], [3084, 0, 6]],
    ("closest", "cube tri_bvh"): [[6, 0, 0], [582, 0, 0], [606, 0, 0], [2374, 0, 6]],
    ("closest", "quad device"): [[2, 0, 0], [126, 0, 0], [130, 0, 0], [514, 0, 6]],
    ("winding", "cube device"): [[12, 0, 0, 0], [756, 0, 0, 0], [780, 0, 0, 0], [2142, 145, 0, 6]],
    ("winding", "cube tri_bvh"): [[12, 0, 0, 0], [756, 0, 0, 0], [780, 0, 0, 0], [1744, 283, 0, 6]],
    ("winding", "quad device"): [[2, 0, 0, 0], [126, 0, 0, 0], [130, 0, 0, 0], [502, 0, 0, 6]],
    ("multihit", "cube device"): [[12, 6, 0], [756, 378, 0], [780, 390, 0], [3024, 1512, 0]],
    ("multihit", "cube tri_bvh"): [[8, 10, 0], [304, 630, 0], [316, 650, 0], [1204, 2520, 0]],
    ("multihit", "quad device"): [[2, 0, 0], [126, 0, 0], [130, 0, 0], [504, 0, 0]],
    ("overlap box", "cube device"): [[12, 6, 0], [744, 374, 0], [768, 386, 0], [2832, 1444, 0]],
    ("overlap box", "cube tri_bvh"): [[6, 10, 0], [350, 622, 0], [362, 642, 0], [1340, 2388, 0]],
    ("overlap box", "quad device"): [[2, 0, 0], [126, 0, 0], [130, 0, 0], [500, 0, 0]],
    ("overlap ball", "cube device"): [[12, 6, 0], [756, 378, 0], [780, 390, 0], [3012, 1506, 0]],
    ("overlap ball", "cube tri_bvh"): [[12, 10, 0], [756, 630, 0], [780, 650, 0], [3012, 2510, 0]],
    ("overlap ball", "quad device"): [[2, 0, 0], [126, 0, 0], [130, 0, 0], [502, 0, 0]],
}


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("query", QUERIES)
def test_counters_and_bytes(query, tree):
    for n, rest in zip(NS, COUNTS[query, tree]):
        words = counted(query, tree, n)
        assert words[0] == n and words[1:] == rest, (query, tree, n, words)
    # counting off again: the product instantiation, the same bytes, and the counters as the last counted call left them
    r, tris = renderer(tree)
    got, want = run(query, r, tris, NS[-1])
    assert got == want and [int(x) for x in counting(query, r)[1]()] == words


def test_renderers_without_a_triangle_tree_are_refused():
    import torch

    L = hrt.lib()
    sph, bare = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE), hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    heap = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)  # triangles in the reference's heap, tri_bvh = 0: no tree either
    t = Tree.from_mesh(Mesh.load_obj(read_asset("cube.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.5))))
    t.build()
    heap.write_bvh(*t.view())
    buf = torch.zeros((4096,), dtype=torch.int32, device=sph._torch_device())
    torch.cuda.synchronize(buf.device)
    p = C.c_void_p(buf.data_ptr())
    calls = {"rt_closest_points": lambda h: L.rt_closest_points(h, p, None, 8, p),
             "rt_winding_numbers": lambda h: L.rt_winding_numbers(h, p, 8, C.c_float(0.0), p),
             "rt_cast_rays_multi": lambda h: L.rt_cast_rays_multi(h, p, p, None, None, 8, 4, p, None),
             "rt_overlap_volumes": lambda h: L.rt_overlap_volumes(h, V.BOX, p, None, 8, 4, p, None)}
    for fn, call in calls.items():
        assert call(sph._h) == _lib.RT_ERR_ARG and L.rt_last_error().decode() == f"{fn}: {NO_SPHERE_TREE}"
        for r in (bare, heap):
            assert call(r._h) == _lib.RT_ERR_STATE and L.rt_last_error().decode() == f"{fn}: {NO_TREE}"
    sph.synchronize()
    assert not buf.cpu().numpy().any()  # nothing was written by a refused call
