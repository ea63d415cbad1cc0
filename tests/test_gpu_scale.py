"""The device tree builders, the refit, the moments and the point and ray queries at a quarter of a million and a million
triangles (tests/scale_util.py has the mesh and says why these sizes): the first tests to run the second and later turns
of k_ploc_scan, the third and later iterations of k_regroup_scan inside a build, fit, refit and moments grids of more
than 256 workgroups (4097: dispatched in several waves), and the stack fallback of the three queries on trees that are
deeper than 24 because the mesh is large, not because it is a chain. Everything is compared with the host mirrors that
tests/test_scale_abi.py pins: bits throughout; the two tolerances are existing ones (the f64 triangle test's bound of
tests/test_gpu_cast_rays.py, the 0.25 sanity bound of tests/test_gpu_winding.py)."""
import math

import numpy as np
import pytest

import hrt

import closest_util as K
import lbvh_util as U
import multihit_util as M
import scale_util as S
import test_gpu_cast_rays as CR
import test_gpu_closest as GC
import test_gpu_multihit as GM
import test_gpu_winding as GW
import winding_util as W
from test_gpu_lbvh import ONE_MATERIAL, on_device, primary_records

pytestmark = pytest.mark.gpu

PLOC = S.PLOC
STACK = 24
INF = W.INF
# The trees the queries run on: both builds of BIG, and the PLOC tree refitted to two moved meshes. "bend" keeps the surface
# closed: every check applies. "jitter" (the refit test's deformation) moves every vertex on its own by twenty times a
# triangle's size: a soup of a million large triangles whose boxes cull almost nothing, so the walks are long and the
# host mirror's too (fewer queries there). Its winding numbers are sums of a million terms of either sign, far outside
# [0, 1] (|w| up to 14.8 over these points, and beta = 2 up to 0.29 from the flat sum over 128 of them): the 0.25 sanity
# bound and the inside and outside points, which presume a surface, are for the other three; the bits are compared all
# the same.
TREES = {"lbvh": (0, None, 128), "ploc": (PLOC, None, 128), "ploc-bend": (PLOC, "bend", 128), "ploc-jitter": (PLOC, "jitter", 32)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def built(name, builder, w=16, h=16):
    r = hrt.Renderer(w, h, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, S.mesh(name)), ONE_MATERIAL, builder=builder)
    return r


def check_tree(r, want, builder):
    """Nodes, order, info and root; the info words; the cost."""
    U.same_tree(r.tri_tree(), want)
    assert r.tri_tree_info().tolist() == S.info_of(want, builder)
    assert r.tri_tree_cost().tolist() == hrt.lbvh_cost(want).tolist()


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def query_case(kind):
    """(renderer, triangles, mirror tree) of one of TREES, made once: the query tests share the four renderers."""
    def make():
        builder, how, _ = TREES[kind]
        r = built("BIG", builder)
        if how is None:
            return r, S.mesh("BIG"), S.mirror("BIG", builder)
        r.refit_triangles_device(on_device(r, S.moved("BIG", how)))
        check_tree(r, S.refitted("BIG", builder, how), builder)
        return r, S.moved("BIG", how), S.refitted("BIG", builder, how)
    return cached(("case", kind), make)


def mesh_key(kind):
    return TREES[kind][1]


def rays(kind):
    return cached(("rays", mesh_key(kind)), lambda: M.mesh_rays(query_case(kind)[1], TREES[kind][2], 23))


def points(kind):
    return cached(("points", mesh_key(kind)), lambda: K.query_points(query_case(kind)[1], TREES[kind][2], 29))


# ------------------------------------------------------------------------------------------------ tree identity
@pytest.mark.parametrize("builder", S.BUILDERS)
@pytest.mark.parametrize("name", list(S.SIZES))
def test_device_tree_is_the_mirrors(name, builder):
    want = S.mirror(name, builder)
    info = want["info"].tolist()
    print(f"{name} builder {builder}: depth {info[4]}, iterations {info[5]}, flat {info[6]}")
    assert info[2] == S.FINITE[name] and len(S.mesh(name)) == S.RECORDS[name]
    check_tree(built(name, builder), want, builder)
    if name == "BIG":
        assert (info[2] + 255) // 256 == 4097  # the first PLOC iteration's tiles, and the fit's workgroups
        if builder == 0:
            assert info[4] > STACK
        else:
            assert info[5] >= 3


def test_rebuilds_and_stale_scratch_on_one_renderer():
    """BIG with PLOC, BIG with LBVH, Suzanne with PLOC (in buffers that still hold the million-cluster lists, flags and tile
    counts), BIG with PLOC, and after rt_release_scratch (everything is allocated again) BIG with PLOC once more; the
    vertices of BIG are moved on the device between its builds."""
    import torch

    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    t = on_device(r, S.mesh("BIG")).view(torch.float32)  # (n, 16): a.xyzw, b.xyzw, c.xyzw, custom.xyz, material
    suzanne = U.mesh_triangles("suzanne.obj")
    step = 0

    def move(t):
        moved = t.clone()
        for v in (0, 4, 8):  # a shear and a wave along x, in f32 on the device (a NaN vertex stays NaN)
            moved[:, v] = t[:, v] * 1.25 + 0.3 * torch.sin(t[:, v + 1] * (2.0 + step))
            moved[:, v + 2] = t[:, v + 2] - 0.2 * t[:, v + 1]
        return moved

    r.set_triangles_device(t, ONE_MATERIAL, builder=PLOC)
    check_tree(r, S.mirror("BIG", PLOC), PLOC)
    for builder, what in ((0, "big"), (PLOC, "suzanne"), (PLOC, "big"), (PLOC, "released")):
        step += 1
        if what == "suzanne":
            r.set_triangles_device(on_device(r, suzanne), ONE_MATERIAL, builder=builder)
            check_tree(r, hrt.lbvh_build(suzanne, builder=builder), builder)
            continue
        if what == "released":
            r.release_scratch()
        t = move(t)
        r.set_triangles_device(t, ONE_MATERIAL, builder=builder)
        want = hrt.lbvh_build(t.cpu().numpy(), builder=builder)
        assert int(want["info"][2]) == S.FINITE["BIG"]
        check_tree(r, want, builder)


# ------------------------------------------------------------------------------------------------ refit, moments
@pytest.mark.parametrize("builder", S.BUILDERS)
def test_refit_is_the_mirrors(builder):
    r = built("BIG", builder)
    r.refit_triangles_device(on_device(r, S.moved("BIG")))
    check_tree(r, S.refitted("BIG", builder), builder)
    r.refit_triangles_device(on_device(r, S.mesh("BIG")))  # the unmoved array: the build's bytes
    check_tree(r, S.mirror("BIG", builder), builder)


@pytest.mark.parametrize("builder", S.BUILDERS)
def test_moments_are_the_host_mirrors(builder):
    a, b = S.mesh("BIG"), S.moved("BIG")
    r = built("BIG", builder)
    tree = S.mirror("BIG", builder)
    want = hrt.tree_moments_host(a, tree)
    got = r.tree_moments()
    assert got.shape == want.shape == (S.FINITE["BIG"] - 1, 16) and got.tobytes() == want.tobytes()
    r.refit_triangles_device(on_device(r, b))
    want = hrt.tree_moments_host(b, S.refitted("BIG", builder))
    assert r.tree_moments().tobytes() == want.tobytes() and want.tobytes() != got.tobytes()
    r.release_scratch()  # frees the moments; they are made again
    assert r.tree_moments().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ queries
@pytest.mark.parametrize("kind", ["lbvh", "ploc", "ploc-bend"])
def test_closest_points_are_the_flat_definitions(kind):
    """A fifth to a half of these ordinary points overflow the stack on these trees and test every triangle: a device call
    takes about 3 s, its slowest lane's time, whatever the number of points (DESIGN.md §7d Scale). The jittered tree is
    left to the other two queries: it overflows no differently here."""
    r, tris, _ = query_case(kind)
    pts = points(kind)
    want = cached(("closest", mesh_key(kind)), lambda: hrt.closest_points_host(tris, pts))
    GC.same(GC.records(r, pts), want)
    finite = np.isfinite(pts).all(axis=1)
    assert (want["prim"][finite] >= 0).all() and (want["prim"][~finite] == -1).all() and (want["d2"] == 0).sum() > len(pts) // 16
    rec, c = GC.counted(r, pts)
    GC.same(rec, want)
    print(f"closest points, {kind} (depth {r.tri_tree_info()[4]}): {c[2]} of {c[0]} queries overflowed the stack, "
          f"{c[3]} outside the walk's bound, {c[1] / c[0]:.0f} triangle tests per query")
    assert c[0] == len(pts)


@pytest.mark.parametrize("kind", list(TREES))
def test_multi_hit_records_are_the_mirrors(kind):
    r, tris, _ = query_case(kind)
    o, d = rays(kind)
    tree = r.tri_tree()
    flat, fc = cached(("multi", mesh_key(kind)), lambda: M.records(tris, tree, o, d, 16, counts=True, flat=True))
    assert fc.max() >= 2 and (flat["prim"][:, 0] >= 0).sum() > len(o) // 4
    for k in (1, 4, 16):
        walk, wc = M.records(tris, tree, o, d, k, counts=True)
        M.same_records(walk, np.ascontiguousarray(flat[:, :k]), f"{kind}: host walk, k = {k}")
        assert (wc == fc).all()
        got, gc = GM.device(r, o, d, k, counts=True)
        M.same_records(got, walk, f"{kind}: k = {k} with counts")
        assert (gc == fc).all()
        got, _ = GM.device(r, o, d, k)
        M.same_records(got, walk, f"{kind}: k = {k}")
    kw = dict(tmax=M.cap_mix(flat["t"][:, 0], 3), after=np.ascontiguousarray(flat[:, 1]))
    want, wc = M.records(tris, tree, o, d, 4, counts=True, flat=True, **kw)
    got, gc = GM.device(r, o, d, 4, counts=True, **kw)
    M.same_records(got, want, f"{kind}: caps and cursors")
    assert (gc == wc).all()
    rec, cnt, c = GM.counted(r, o, d, 4, counts=True)
    M.same_records(rec, np.ascontiguousarray(flat[:, :4]), f"{kind}: counted")
    print(f"multi-hit, {kind} (depth {r.tri_tree_info()[4]}): {c[3]} of {c[0]} queries overflowed the stack, "
          f"{c[1] / c[0]:.0f} triangle and {c[2] / c[0]:.0f} box tests per ray")
    assert (cnt == fc).all() and c[0] == len(o)


@pytest.mark.parametrize("kind", list(TREES))
def test_winding_numbers_are_the_mirrors(kind):
    r, tris, tree = query_case(kind)
    pts = points(kind)
    covered = np.isfinite(pts).all(axis=1)  # (the finite points are well inside D_MAX)
    flat = cached(("winding", mesh_key(kind)), lambda: hrt.winding_numbers_host(tris, None, pts))
    assert (flat[~covered].view(np.uint32) == W.QNAN).all() and np.isfinite(flat[covered]).all()
    mom = hrt.tree_moments_host(tris, tree)
    deep = S.left_descents_overflow(tree)
    surface = kind != "ploc-jitter"
    every = (pts, covered, flat)
    some = np.r_[0:26, len(pts) - 6:len(pts)]  # beta = +inf sums a million terms per point, on the host too: 32 of them
    for beta in (2.0, INF):
        pts, covered, flat = every if beta == 2.0 else tuple(x[some] for x in every)
        want = hrt.winding_numbers_host(tris, tree, pts, beta)
        W.same_bits(GW.device(r, pts, beta), want)
        print(f"winding numbers, {kind}, beta {beta}: largest |w - flat| = {np.abs(want - flat)[covered].max():.4f}, "
              f"largest |flat| = {np.abs(flat[covered]).max():.2f}")
        if surface:
            assert np.abs(want - flat)[covered].max() < 0.25
        w, c = GW.counted(r, pts, beta)
        W.same_bits(w, want)
        print(f"winding numbers, {kind} (depth {tree['info'][4]}), beta {beta}: {c[3]} of {c[0]} queries overflowed the "
              f"stack, {c[1] / c[0]:.0f} triangle and {c[2] / c[0]:.0f} dipole terms per query")
        assert c[0] == len(pts) and c[4] == (~covered).sum()
        if beta == INF:  # no child is far: every covered walk is the whole tree's, and overflows if the tree makes it
            assert c[3] == (int(covered.sum()) if deep else 0)
        elif surface:  # (the restated walk is Python, per node: the soup's boxes cull too little for it)
            assert c[3] == sum(W.walk_shape(tree, mom, p, beta)[0] for p in pts[covered])
    if surface:
        inside, outside = S.inside_outside_points()
        if TREES[kind][1] == "bend":
            inside, outside = S.bend(inside), S.bend(outside)
        wi, wo = GW.device(r, inside), GW.device(r, outside)
        W.same_bits(wi, hrt.winding_numbers_host(tris, tree, inside))
        W.same_bits(wo, hrt.winding_numbers_host(tris, tree, outside))
        assert (np.abs(wi) > 0.9).all() and (np.abs(wo) < 0.1).all()


def test_cast_rays_and_occluded_agree_through_both_trees():
    import torch

    (r0, tris, _), (r1, _, _) = query_case("lbvh"), query_case("ploc")
    o, d = rays("lbvh")
    hits = [r.cast_rays(o, d) for r in (r0, r1)]
    rec = [CR._records(h) for h in hits]
    assert rec[0].tobytes() == rec[1].tobytes()
    t = hits[0]["t"]
    scale = torch.where(torch.arange(len(t), device=t.device) % 2 == 0, 1.25, 0.75)
    tmax = torch.where(t < hrt.RT_T_MISS, t * scale, torch.full_like(t, 7.0))
    occ = [r.occluded(o, d, tmax).cpu().numpy() for r in (r0, r1)]
    assert occ[0].tobytes() == occ[1].tobytes() and occ[0].any() and not occ[0].all()
    t, prim = t.cpu().numpy(), hits[0]["prim"].cpu().numpy()
    m = prim >= 0
    assert m.sum() > len(o) // 4 and prim[m].max() < len(tris) and np.isfinite(U.tri_f64(tris[prim[m]])[0]).all()
    t64, kept, bound = CR.triangle_reference(o[m], d[m], tris[prim[m]])
    ratio = np.abs(t[m][kept].astype(np.float64) - t64[kept]) / bound[kept]
    print(f"cast_rays: {int(m.sum())} hits, {int(kept.sum())} kept, largest |t - t64| / bound = {ratio.max():.4f}")
    assert kept.sum() >= 8 and (ratio <= 1.0).all()


# ------------------------------------------------------------------------------------------------ draws
def test_draws_agree_through_both_trees():
    cam = hrt.Camera.new(hrt.Vec3(0.0, -2.5 * S.RADIUS, S.RADIUS), hrt.Vec3(0.0, 0.0, 0.0), 2.5 * S.RADIUS, 0.0, math.pi * 0.3)
    records, images = [], []
    for builder in S.BUILDERS:
        r = hrt.Renderer(64, 48, hrt.RT_MODE_TRIS)
        r.set_camera(cam)
        r.set_triangles_device(on_device(r, S.mesh("BIG")), ONE_MATERIAL, builder=builder)
        records.append(primary_records(r))
        r.draw_frames(2, 1000, 10)
        images.append(r.read_image().view(np.uint32))
    assert (records[0][:, 1] >= 0).sum() > 500 and records[0].tobytes() == records[1].tobytes()
    assert images[0].tobytes() == images[1].tobytes() and images[0].any()
