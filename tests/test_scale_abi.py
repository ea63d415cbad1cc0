"""The host mirrors of the device tree (hrt.lbvh_build, lbvh_refit, lbvh_cost, cast_rays_multi_host) at a quarter of a
million and a million triangles, held against checks that share no code with them: the numpy reading of the tree format,
a brute-force ray test, the numpy cost, and the flat definition. tests/test_gpu_scale.py compares the device with these
mirrors byte for byte at the same sizes (tests/scale_util.py says why these sizes). CPU only."""
import numpy as np
import pytest

import hrt

import lbvh_refit_util as R
import lbvh_util as U
import multihit_util as M
import scale_util as S
import test_ploc_abi as A


def test_the_generator_makes_what_the_sizes_promise():
    v = S.bumpy_sphere_vertices(16, 8)
    assert v.shape == (256, 3, 3) and np.isfinite(v).all()
    # closed: every directed edge of a proper triangle has its opposite (the pole rows' zero-area triangles have none to give)
    edges = {}
    for t in v:
        p = [tuple(x.tolist()) for x in t]
        for a, b in ((p[0], p[1]), (p[1], p[2]), (p[2], p[0])):
            if a != b:
                edges[a, b] = edges.get((a, b), 0) + 1
    assert all(edges.get((b, a), 0) == c for (a, b), c in edges.items())
    # wound outward: the signed volume is positive and near a unit sphere's
    vol = float((v[:, 0].astype(np.float64) * np.cross(v[:, 1].astype(np.float64), v[:, 2].astype(np.float64))).sum() / 6.0)
    assert 3.0 < vol / S.RADIUS ** 3 < 5.0
    area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    assert (area == 0).sum() == 2 * 16  # one triangle of every quad of the two pole rows
    for name, (nu, nv, dup, bad) in S.SIZES.items():
        n, m = S.RECORDS[name], S.FINITE[name]
        assert 2 * nu * nv + dup == m and m + bad == n
        pos = S.bad_positions(n, bad)
        assert len(set(pos.tolist())) == bad and (bad == 0 or (pos.min() < n // 20 and n - n // 20 < pos.max() < n - 1))
    t = S.bumpy_sphere(16, 8, dup=3, bad=5)
    finite = U.tri_f64(t)[1]
    assert len(t) == 264 and (~finite).sum() == 5 and np.flatnonzero(~finite).tolist() == S.bad_positions(264, 5).tolist()
    assert t[finite][-3:].tobytes() == t[finite][:3].tobytes()
    assert S.bumpy_sphere(16, 8, dup=3, bad=5).tobytes() == t.tobytes()
    # the branches the sizes are for
    assert S.tiles(S.FINITE["EDGE_LO"], S.PLOC_TILE) == S.PLOC_SCAN_TILES
    assert S.tiles(S.FINITE["EDGE_HI"], S.PLOC_TILE) == S.PLOC_SCAN_TILES + 1
    assert S.FINITE["EDGE_HI"] != S.RECORDS["EDGE_HI"] and S.FINITE["BIG"] != S.RECORDS["BIG"]
    big = S.FINITE["BIG"]
    assert (big + 255) // 256 == 4097
    assert [S.turns(S.tiles(c, S.PLOC_TILE), S.PLOC_SCAN_TILES) for c in (big, (big + 1) // 2, (big + 3) // 4)] == [5, 3, 2]
    assert S.turns(S.tiles(S.RECORDS["BIG"], S.SORT_TILE), S.SORT_SCAN_TILES) == 5
    assert S.tiles(big, S.FIT_BLOCK) == 4097


def test_left_descents_overflow_is_the_restated_walks():
    """scale_util.left_descents_overflow against winding_util.walk_shape with beta = +inf, on trees small enough for the
    latter: the 120-triangle chain's PLOC tree overflows a stack of 24, Suzanne's trees do not, and shorter stacks find
    the threshold of each tree."""
    import closest_util as K
    import winding_util as W

    p = np.float32([0.1, 0.2, 0.3])
    seen = set()
    for tris, builder in ((K.chain_triangles(120), S.PLOC), (U.mesh_triangles("suzanne.obj"), 0),
                          (U.mesh_triangles("suzanne.obj"), S.PLOC)):
        tree = hrt.lbvh_build(tris, builder=builder)
        mom = hrt.tree_moments_host(tris, tree)
        for stack in (24, 12, 8, 4):
            want = W.walk_shape(tree, mom, p, W.INF, stack=stack)[0]
            assert S.left_descents_overflow(tree, stack) == want, (builder, stack)
            seen.add((stack, want))
    assert {(24, True), (24, False), (4, True)} <= seen


@pytest.mark.parametrize("builder", S.BUILDERS)
def test_edge_hi_tree_is_valid(builder):
    tris, tree = S.mesh("EDGE_HI"), S.mirror("EDGE_HI", builder)
    if builder == 0:
        U.check_tree(tris, tree)
    else:
        A.check_ploc_tree(tris, tree)
    U.same_tree(hrt.lbvh_build(tris, builder=builder), tree)  # a second call: the same bytes
    assert int(tree["info"][2]) == S.FINITE["EDGE_HI"] == 262145
    bad = S.bad_positions(len(tris), 23)
    assert len(bad) == 23 and not np.isin(bad, tree["order"]).any()
    assert (tree["order"] == S.mirror("EDGE_HI", 0)["order"]).all()  # up to the sort nothing differs


@pytest.mark.slow  # (about 25 s: the walk is Python, per node)
@pytest.mark.filterwarnings("ignore:All-NaN slice")  # (the NaN ray's slab test)
def test_edge_hi_walks_find_the_brute_force_triangle():
    """64 rays of multihit_util.mesh_rays through both trees, as tests/test_ploc_abi.py does on Suzanne; the degenerate
    rays among them have no hit by either."""
    tris = S.mesh("EDGE_HI")
    v, finite = U.tri_f64(tris)
    o, d = M.mesh_rays(tris, 64, 17)
    trees = [S.mirror("EDGE_HI", b) for b in S.BUILDERS]
    hits = 0
    for k in range(64):
        ok, dk = o[k].astype(np.float64), d[k].astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            t = U.moller_trumbore(ok, dk, v[finite])
        bt = t.min()
        bj = int(np.flatnonzero(finite)[np.flatnonzero(t == bt)[0]]) if np.isfinite(bt) else -1
        for tree in trees:
            with np.errstate(over="ignore", invalid="ignore"):
                wt, wj = U.walk(ok, dk, v, tree)
            assert (wj, wt) == (bj, bt) or (bj < 0 and wj < 0), (k, wj, wt, bj, bt)
        hits += bj >= 0
    assert hits > 20  # (the rays do aim at the mesh)


@pytest.mark.parametrize("builder", S.BUILDERS)
def test_big_builds_costs_and_refits(builder):
    tris, tree = S.mesh("BIG"), S.mirror("BIG", builder)
    info = tree["info"].tolist()
    assert info[2] == S.FINITE["BIG"] and info[0] == info[2] - 1 and len(tree["order"]) == info[2]
    U.same_tree(hrt.lbvh_build(tris, builder=builder), tree)
    assert hrt.lbvh_cost(tree).tolist() == R.numpy_cost(tree)
    U.same_tree(hrt.lbvh_refit(tris, tris, builder=builder), tree)
    assert 24 < info[4] <= 64
    if builder == S.PLOC:
        assert 3 <= info[5] <= 64
    print(f"BIG builder {builder}: depth {info[4]}, iterations {info[5]}, flat {info[6]}")


@pytest.mark.parametrize("builder", S.BUILDERS)
def test_big_multi_hit_walk_is_the_flat_definition(builder):
    tris, tree = S.mesh("BIG"), S.mirror("BIG", builder)
    o, d = M.mesh_rays(tris, 128, 23)
    walk, wc = M.records(tris, tree, o, d, 4, counts=True)
    flat, fc = M.records(tris, tree, o, d, 4, counts=True, flat=True)
    M.same_records(walk, flat, f"BIG builder {builder}")
    assert (wc == fc).all() and fc.max() >= 2 and (flat["prim"][:, 0] >= 0).sum() > 32
