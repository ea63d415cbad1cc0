"""rt_winding_numbers on the GPU: the device bytes are the host mirror's (hrt.winding_numbers_host on the bytes of the tree
the renderer walks, read back with Renderer.tri_tree) through every tree the renderer can hold (device LBVH and PLOC,
refitted, the host SAH tree of tri_bvh = 1), through trees without nodes, the walk's stack overflow and the points it does
not cover; the device moments are rt_host_tree_moments' bytes; the counting instantiation shows dipoles at work; statuses;
nothing of a draw's state moves; and the signed distance composed from the two point queries. Bits only: no tolerance on
anything the device computes."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_refit_util as R
import lbvh_util as U
import test_gpu_cast_rays as CR
import winding_util as W
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device
from test_gpu_lbvh_refit import host_sah_renderer

pytestmark = pytest.mark.gpu

N = 512
INF = W.INF
BETAS = (0.0, 2.0, 3.0, INF)
CASES = dict(U.cpu_cases(), chain120=lambda: K.chain_triangles(120))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def tris_renderer(tris, builder=0, materials=ONE_MATERIAL):
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), materials, builder=builder)
    return r


def device(r, pts, beta=0.0) -> np.ndarray:
    return r.winding_numbers(pts, beta).cpu().numpy()


def check_all_betas(r, tris, pts):
    tree = r.tri_tree()
    for beta in BETAS:
        W.same_bits(device(r, pts, beta), hrt.winding_numbers_host(tris, tree, pts, beta))
    return tree


# ------------------------------------------------------------------------------------------------ equality with the mirror
@pytest.mark.parametrize("builder", W.BUILDERS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_bytes_are_the_mirrors(name, builder):
    tris = CASES[name]()
    pts = K.query_points(tris, N, 300 + len(tris))
    r = tris_renderer(tris, builder)
    tree = check_all_betas(r, tris, pts)
    U.same_tree(tree, hrt.lbvh_build(tris, builder))  # (the mirror's tree is the host builder's)
    bad = ~np.isfinite(pts).all(axis=1)
    w = device(r, pts)
    assert bad.sum() == 6 and (w[bad].view(np.uint32) == W.QNAN).all() and np.isfinite(w[~bad]).all()
    if name == "cube":
        assert w[~bad].max() > 0.99 and abs(w[~bad]).min() < 0.01


@pytest.mark.parametrize("scene", ["cube", "suzane", "mixed"])
def test_host_sah_tree_returns_the_mirrors_bytes(scene):
    sd = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}[scene](32, 24)
    tris = sd.bvh[2]
    r = host_sah_renderer(sd)
    assert int(r.tri_tree_info()[0]) == 0xFFFFFFFF
    pts = K.query_points(tris, N, 5)
    if scene == "mixed":  # points on and inside the spheres too: only triangles answer
        pts = np.ascontiguousarray(np.concatenate([pts, sd.spheres["center"].astype(np.float32)]))
        assert sd.mode == hrt.RT_MODE_MIXED and len(sd.spheres) > 4
    tree = check_all_betas(r, tris, pts)
    assert r.tree_moments().tobytes() == hrt.tree_moments_host(tris, tree).tobytes()
    ok = W.clear_of_surface(tris, pts)
    assert ok.sum() > 100 and np.abs(device(r, pts, INF)[ok] - W.winding_f64(tris, pts[ok])).max() < 1e-3


# ------------------------------------------------------------------------------------------------ moments, refit, scratch
@pytest.mark.parametrize("builder", W.BUILDERS)
def test_device_moments_are_the_host_mirrors(builder):
    for name in ("suzanne", "random1025", "identical70", "nan1of9", "chain120", "random4"):
        tris = CASES[name]()
        r = tris_renderer(tris, builder)
        tree = r.tri_tree()
        got, want = r.tree_moments(), hrt.tree_moments_host(tris, tree)
        assert got.shape == want.shape == (len(tree["nodes"]), 16), name
        assert got.tobytes() == want.tobytes(), name
    assert len(want) == 0  # (random4: a tree without nodes has no records)


@pytest.mark.parametrize("builder", W.BUILDERS)
@pytest.mark.parametrize("kind", ["translate", "jitter"])
def test_refit_makes_the_moments_again(kind, builder):
    a = W.mesh("suzanne")
    b = R.deform(a, kind)
    r = tris_renderer(a, builder)
    pts = K.query_points(b, N, 21)
    before = device(r, pts)
    old = r.tree_moments()
    r.refit_triangles_device(on_device(r, b))
    tree = r.tri_tree()
    U.same_tree(tree, hrt.lbvh_refit(a, b, builder))
    mom = r.tree_moments()
    assert mom.tobytes() == hrt.tree_moments_host(b, tree).tobytes() and mom.tobytes() != old.tobytes()
    for beta in BETAS:  # the query answers for the moved mesh
        W.same_bits(device(r, pts, beta), hrt.winding_numbers_host(b, tree, pts, beta))
    after = device(r, pts)
    assert after.tobytes() != before.tobytes()
    ok = W.clear_of_surface(b, pts)
    assert ok.sum() > 100 and np.abs(device(r, pts, INF)[ok] - W.winding_f64(b, pts[ok])).max() < 1e-3
    # rt_release_scratch frees the moments; the next query makes them again: the same bytes
    r.release_scratch()
    W.same_bits(device(r, pts), after)
    assert r.tree_moments().tobytes() == mom.tobytes()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_counts_write_exactly_4n_bytes(n):
    import torch

    tris = W.mesh("suzanne")
    pts = K.query_points(tris, N, 100 + len(tris))
    r = tris_renderer(tris)
    dev = r._torch_device()
    p = torch.from_numpy(pts[:n].copy()).to(dev)
    out = torch.full((n + 5,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    assert hrt.lib().rt_winding_numbers(r._h, C.c_void_p(p.data_ptr()), n, 0.0, C.c_void_p(out.data_ptr())) == _lib.RT_OK
    r.synchronize()
    got = out.cpu().numpy()
    W.same_bits(got[:n].view(np.float32), hrt.winding_numbers_host(tris, r.tri_tree(), pts[:n]))
    assert (got[n:] == 0x5A5A5A5A).all()


def test_every_tree_is_within_its_bound_of_the_brute_force():
    sd = CR.suzane_scene(16, 16)
    tris, mats = sd.bvh[2], sd.bvh[3]
    pts = W.accuracy_points(tris)
    ref = W.winding_f64(tris, pts)
    refitted = tris_renderer(R.deform(tris, "jitter"), 1, mats)
    refitted.refit_triangles_device(on_device(refitted, tris))  # another topology, these positions
    trees = {"lbvh": tris_renderer(tris, 0, mats), "ploc": tris_renderer(tris, 1, mats), "refitted": refitted,
             "host": host_sah_renderer(sd)}
    for name, r in trees.items():
        tree = r.tri_tree()
        for beta in (2.0, INF):
            w = device(r, pts, beta)
            W.same_bits(w, hrt.winding_numbers_host(tris, tree, pts, beta))
            if name in ("lbvh", "ploc"):  # (the bound was measured on these two trees)
                assert np.abs(w - ref).max() <= W.bound("suzanne", beta), (name, beta)
            assert np.abs(w - ref).max() < 0.25, (name, beta)


# ------------------------------------------------------------------------------------------------ counters
def counted(r, pts, beta):
    r.set_winding_count(True)
    w = device(r, pts, beta)
    c = [int(x) for x in r.winding_counts()]
    r.set_winding_count(False)
    return w, c


def test_counters_show_dipoles_at_work():
    tris = W.mesh("suzanne")
    m = len(tris)
    rng = np.random.default_rng(2)
    lo, hi = K.root_box(tris)
    pts = np.concatenate([W.accuracy_points(tris), W.accuracy_points(tris, 19)[:400]])
    pts = np.ascontiguousarray(np.concatenate([pts, 0.5 * (lo + hi) + rng.uniform(-0.75, 0.75, size=(800, 3)) * (hi - lo)]).astype(np.float32))
    assert len(pts) == 2000
    for builder in W.BUILDERS:
        r = tris_renderer(tris, builder)
        tree = r.tri_tree()
        assert r.winding_counts().tolist() == [0, 0, 0, 0, 0]
        w, c = counted(r, pts, 2.0)
        print(f"suzanne builder {builder} beta 2: {c[1] / c[0]:.1f} triangle and {c[2] / c[0]:.1f} dipole terms per query of {m}")
        W.same_bits(w, hrt.winding_numbers_host(tris, tree, pts, 2.0))
        assert c[0] == 2000 and c[2] > 0 and c[3] == 0 and c[4] == 0
        assert c[1] / c[0] < m / 4  # well under 979 (an always-exact kernel has m: this is no performance claim)
        w, c = counted(r, pts, INF)
        W.same_bits(w, hrt.winding_numbers_host(tris, tree, pts, INF))
        assert c == [2000, 2000 * m, 0, 0, 0]
        # non-finite points and points past the covered range: exactly they are uncovered, and only the finite ones sum
        odd = K.query_points(tris, 500, 9, nonfinite=12)
        odd[:5] = [[2e18, 0, 0], [0, -3e25, 1], [1e30, 1e30, 1e30], [3e38, -3e38, 3e38], [0, 0, 1.2e18]]
        w, c = counted(r, odd, 2.0)
        W.same_bits(w, hrt.winding_numbers_host(tris, tree, odd, 2.0))
        assert c[0] == 500 and c[4] == 17 and c[3] == 0 and c[1] >= 5 * m
        W.same_bits(device(r, pts, 2.0), hrt.winding_numbers_host(tris, tree, pts, 2.0))  # counting off again: same bytes


def test_a_deep_tree_overflows_the_stack_and_still_answers():
    tris = K.chain_triangles(120)
    r = tris_renderer(tris, 1)
    tree = r.tri_tree()
    assert int(r.tri_tree_info()[4]) > 24
    pts = W.chain_points()
    mom = hrt.tree_moments_host(tris, tree)
    for beta in (2.0, INF):
        over = sum(W.walk_shape(tree, mom, p, beta)[0] for p in pts)
        w, c = counted(r, pts, beta)
        print(f"chain120 beta {beta}: {c[3]} of {c[0]} queries overflowed the stack")
        W.same_bits(w, hrt.winding_numbers_host(tris, tree, pts, beta))
        assert c[0] == len(pts) and c[3] == over > 0 and c[4] == 0
    W.same_bits(w, hrt.winding_numbers_host(tris, None, pts))  # beta = inf: every query took the flat definition


# ------------------------------------------------------------------------------------------------ statuses and state
def test_statuses():
    import torch

    L = hrt.lib()
    tris = W.mesh("suzanne")
    pts = K.query_points(tris, N, 100 + len(tris))
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    dev = sph._torch_device()
    p = torch.from_numpy(pts[:64].copy()).to(dev)
    out = torch.zeros((80,), dtype=torch.int32, device=dev)
    pp, po = C.c_void_p(p.data_ptr()), C.c_void_p(out.data_ptr())
    torch.cuda.synchronize(dev)
    assert L.rt_winding_numbers(sph._h, pp, 64, 0.0, po) == _lib.RT_ERR_ARG
    assert b"sphere program" in L.rt_last_error()
    r = tris_renderer(tris)
    assert L.rt_winding_numbers(r._h, pp, 0, 0.0, po) == _lib.RT_OK  # n = 0, and null buffers with it
    assert L.rt_winding_numbers(r._h, None, 0, 0.0, None) == _lib.RT_OK
    for args in ((None, 64, 0.0, po), (pp, 64, 0.0, None),                       # null
                 (C.c_void_p(p.data_ptr() + 2), 32, 0.0, po),                    # misaligned points
                 (pp, 32, 0.0, C.c_void_p(out.data_ptr() + 1)),                  # misaligned w
                 (pp, 32, float("nan"), po), (pp, 32, -1.0, po), (pp, 32, 0.5, po), (pp, 32, -INF, po)):  # bad beta
        assert L.rt_winding_numbers(r._h, *args) == _lib.RT_ERR_ARG, args
        assert b"rt_winding_numbers" in L.rt_last_error()
    r.synchronize()
    assert not out.cpu().numpy().any()  # nothing was written by a refused call
    with pytest.raises(hrt.RtError) as e:
        r.winding_numbers(pts[:4], 0.25)
    assert e.value.code == _lib.RT_ERR_ARG and "winding_numbers" in str(e.value)
    assert L.rt_winding_numbers(r._h, C.c_void_p(p.data_ptr() + 4), 32, 1.0, C.c_void_p(out.data_ptr() + 4)) == _lib.RT_OK
    r.synchronize()
    W.same_bits(out.cpu().numpy()[1:33].view(np.float32), hrt.winding_numbers_host(tris, r.tri_tree(), pts[:64].reshape(-1)[1:97].reshape(-1, 3), 1.0))
    # no tree: tri_bvh = 0 and no device geometry
    sd = CR.suzane_scene(16, 16)
    h = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    assert L.rt_winding_numbers(h._h, pp, 64, 0.0, po) == _lib.RT_ERR_STATE
    h.write_bvh(*sd.bvh)
    assert L.rt_winding_numbers(h._h, pp, 64, 0.0, po) == _lib.RT_ERR_STATE
    assert b"no triangle tree" in L.rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        h.winding_numbers(pts[:4])
    assert e.value.code == _lib.RT_ERR_STATE
    h.set_params(tri_bvh=1)  # the host SAH tree is built by the query itself
    W.same_bits(device(h, pts), hrt.winding_numbers_host(sd.bvh[2], h.tri_tree(), pts))
    # rt_set_bvh leaves the device-geometry state, and the moments follow the tree that answers
    want = device(r, pts)
    r.write_bvh(*sd.bvh)
    with pytest.raises(hrt.RtError) as e:
        r.winding_numbers(pts[:4])
    assert e.value.code == _lib.RT_ERR_STATE
    r.set_params(tri_bvh=1)
    W.same_bits(device(r, pts), hrt.winding_numbers_host(sd.bvh[2], r.tri_tree(), pts))
    r.set_params(tri_bvh=0)
    # a failed build keeps the geometry, the tree and the moments that answer
    r.set_triangles_device(on_device(r, tris), ONE_MATERIAL, builder=1)
    good = device(r, pts)
    bad = R.deform(tris, "scatter")
    bad["material"][len(bad) // 2] = 1
    with pytest.raises(hrt.RtError):
        r.set_triangles_device(on_device(r, bad), ONE_MATERIAL, builder=1)
    W.same_bits(device(r, pts), good)
    W.same_bits(good, hrt.winding_numbers_host(tris, r.tri_tree(), pts))
    assert np.abs(good - want)[np.isfinite(want)].max() <= 2 * W.bound("suzanne", 2.0)


def test_draw_state_is_untouched():
    sd = CR.suzane_scene(48, 32)
    sd.bounces = 3
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    tris = sd.bvh[2]
    pts = K.query_points(tris, N, 31)
    r.draw_frames(2, 1000, 10)
    img, fc, st, raw, order = r.read_image(), r.frame_count, r.stats(), r.raw_counters(), r.tile_order()
    W.same_bits(device(r, pts), hrt.winding_numbers_host(tris, r.tri_tree(), pts))
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st) and r.raw_counters() == raw
    assert all((a == b).all() for a, b in zip(r.tile_order(), order))
    r.reset_frame_count()
    r.draw_frames(2, 1000, 10)
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and img.any()
    assert r.stats().queries == st.queries


# ------------------------------------------------------------------------------------------------ the signed distance
def test_signed_distance_on_the_ico_sphere():
    import torch

    tris = W.mesh("ico_sphere")
    lo, hi = K.root_box(tris)
    centre, radius = 0.5 * (lo + hi), 0.5 * float((hi - lo).min())
    rng = np.random.default_rng(8)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([centre[None], centre + d[:100] * 0.5 * radius, centre + d[100:] * 2.0 * radius]).astype(np.float32)
    inward = U.triangles_from_vertices(U.tri_f64(tris)[0][:, ::-1].astype(np.float32))
    for mesh in (tris, inward):  # |w|: a mesh wound inward works too
        r = tris_renderer(mesh, 1)
        sd = r.signed_distance(pts)
        dist, inside, w = sd["distance"].cpu().numpy(), sd["inside"].cpu().numpy(), sd["winding"].cpu().numpy()
        assert inside[:101].all() and not inside[101:].any()
        assert (dist[:101] < 0).all() and (dist[101:] > 0).all()
        assert np.sign(w[0]) == (1 if mesh is tris else -1) and abs(abs(w[0]) - 1) <= W.bound("ico_sphere", 2.0)
        cp = r.closest_points(pts)
        assert torch.equal(sd["distance"].abs(), torch.sqrt(cp["d2"])) and torch.equal(sd["d2"], cp["d2"])
        assert torch.equal(sd["prim"], cp["prim"]) and torch.equal(sd["point"], cp["point"])
        W.same_bits(w, hrt.winding_numbers_host(mesh, r.tri_tree(), pts))
        assert 0.7 * radius < -dist[0] <= radius * 1.001
