"""rt_refit_triangles_device on the GPU: the refitted device tree is the host mirror's (hrt.lbvh_refit), byte for byte;
every query and draw through it gives what a fresh rt_set_triangles_device and the host-built SAH tree give on the moved
triangles; the call's errors leave the renderer as it was; rt_get_tri_tree_cost is hrt.lbvh_cost of the tree read back.
No tolerance anywhere: every comparison is of bits."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import hrt
import scenes
from hrt import _lib

import lbvh_refit_util as R
import lbvh_util as U
import test_gpu_cast_rays as CR
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device, primary_records

pytestmark = pytest.mark.gpu

W, H = 64, 48
SHAPES = R.shapes()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def moved_scene(sd, tris):
    return dataclasses.replace(sd, bvh=(sd.bvh[0], sd.bvh[1], tris, sd.bvh[3]))


def host_sah_renderer(sd, **params):
    """The host's SAH tree over sd's triangles (the heap of sd.bvh is not read with tri_bvh = 1)."""
    r = scenes.make_renderer(sd)
    r.set_params(tri_bvh=1, **params)
    return r


# ------------------------------------------------------------------------------------------------ tree identity
@pytest.mark.parametrize("name", list(SHAPES))
def test_refitted_device_tree_is_the_mirrors(name):
    a = SHAPES[name]()
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    ta = on_device(r, a)
    for kind in R.DEFORMATIONS:
        b, c = R.deform(a, kind), R.deform(a, "jitter" if kind != "jitter" else "scatter", seed=5)
        r.set_triangles_device(ta, ONE_MATERIAL)
        r.refit_triangles_device(on_device(r, b))
        U.same_tree(r.tri_tree(), hrt.lbvh_refit(a, b))
        r.refit_triangles_device(on_device(r, c))
        U.same_tree(r.tri_tree(), hrt.lbvh_refit(a, c))
    r.refit_triangles_device(ta)  # the unmoved array: the build's bytes
    U.same_tree(r.tri_tree(), hrt.lbvh_build(a))


def test_refits_on_one_renderer_match_the_mirror():
    """lucy built once and refitted three times on one renderer, the vertices moved on the device in between: the fit's
    hand-offs (78 workgroups over all XCDs) with the buffers of the refit before still in the caches."""
    import torch

    tris = U.mesh_triangles("lucy_lp_20.obj")
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    t = on_device(r, tris).view(torch.float32)  # (m, 16): a.xyzw, b.xyzw, c.xyzw, custom.xyz, material
    r.set_triangles_device(t, ONE_MATERIAL)
    assert len(tris) > 19000 and int(r.tri_tree()["info"][0]) == len(tris) - 1
    for step in range(3):
        moved = t.clone()
        for v in (0, 4, 8):  # a shear and a wave along x, in f32 on the device
            moved[:, v] = t[:, v] * 1.25 + 0.3 * torch.sin(t[:, v + 1] * (2.0 + step))
            moved[:, v + 2] = t[:, v + 2] - 0.2 * t[:, v + 1]
        t = moved
        r.refit_triangles_device(t)
        U.same_tree(r.tri_tree(), hrt.lbvh_refit(tris, t.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ hits, queries, draws
HIT_SCENES = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}


def _queries(r, o, d, tmax, rng):
    import torch

    out = [r.occluded(o, d, tmax).cpu().numpy()]
    out += [x.cpu().numpy() for x in r.trace_rays(o, d, rng=rng, want_queries=True)]
    dev = r._torch_device()
    bo, bd, bs = o.clone(), d.clone(), rng.clone()
    tp = torch.ones((len(bo), 3), dtype=torch.float32, device=dev)
    q = torch.zeros((len(bo),), dtype=torch.int32, device=dev)
    hits = torch.zeros((len(bo), 8), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    r.bounce_rays(bo, bd, bs, throughput=tp, queries=q, hits=hits, count_out=count)
    return out + [x.cpu().numpy() for x in (bo, bd, bs, tp, q, hits, count)]


@pytest.mark.parametrize("name", list(HIT_SCENES))
def test_hits_queries_and_draws_equal_a_fresh_builds(name):
    import torch

    sd = HIT_SCENES[name](W, H)
    sd.bounces = 5
    b = R.deform(sd.bvh[2], "scatter", amount=0.05)
    sdb = moved_scene(sd, b)
    r = device_renderer(sd)
    before = primary_records(r)
    r.refit_triangles_device(on_device(r, b))
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(sd.bvh[2], b))
    fresh, host = device_renderer(sdb), host_sah_renderer(sdb)
    got = primary_records(r)
    assert (got != before).any() and (got[:, 1] >= 0).sum() > 100
    assert (got == primary_records(fresh)).all() and (got == primary_records(host)).all()
    o, d = host.primary_rays(1000)
    o, d = o.view(-1, 3).contiguous(), d.view(-1, 3).contiguous()
    t = host.cast_rays(o, d)["t"]
    scale = torch.where(torch.arange(len(t), device=t.device) % 2 == 0, 1.25, 0.75)
    tmax = torch.where(t < hrt.RT_T_MISS, t * scale, torch.full_like(t, 7.0))
    rng = host.primary_rng(1000).view(-1).contiguous()
    want = _queries(fresh, o, d, tmax, rng)
    for other in (_queries(r, o, d, tmax, rng), _queries(host, o, d, tmax, rng)):
        for x, y in zip(want, other):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert want[0].any() and not want[0].all()
    for schedule in (hrt.RT_SCHEDULE_TILES, hrt.RT_SCHEDULE_QUEUE):
        images = []
        for x in (r, fresh):
            x.set_params(schedule=schedule)
            x.reset_frame_count()
            x.draw_frames(2, 1000, 10)
            images.append(x.read_image().view(np.uint32))
            assert x.stats().schedule == schedule
        assert (images[0] == images[1]).all() and images[0].any()


# ------------------------------------------------------------------------------------------------ cost
def test_tri_tree_cost_is_the_hosts():
    sd = CR.suzane_scene(16, 16)
    r = device_renderer(sd)
    built = r.tri_tree_cost()
    assert built.tolist() == hrt.lbvh_cost(r.tri_tree()).tolist() == hrt.lbvh_cost(hrt.lbvh_build(sd.bvh[2])).tolist()
    b = R.deform(sd.bvh[2], "scatter")
    r.refit_triangles_device(on_device(r, b))
    refit = r.tri_tree_cost()
    assert refit.tolist() == hrt.lbvh_cost(hrt.lbvh_refit(sd.bvh[2], b)).tolist() == R.numpy_cost(r.tri_tree())
    assert int(refit[0]) + int(refit[1]) > int(built[0]) + int(built[1]) and refit[2:].tolist() == built[2:].tolist()
    host = scenes.make_renderer(sd)
    host.set_params(tri_bvh=1)  # the SAH tree is not built yet: the call builds it
    sah = host.tri_tree_cost()
    tree = host.tri_tree()
    assert sah.tolist() == hrt.lbvh_cost(tree).tolist() == R.numpy_cost(tree) and int(sah[3]) == len(sd.bvh[2])
    assert int(sah[0]) + int(sah[1]) > 0
    # a tree without nodes: four zeros; the sphere program has no tree
    small = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    small.set_triangles_device(on_device(small, U.random_triangles(4, 1)), ONE_MATERIAL)
    assert small.tri_tree_cost().tolist() == [0, 0, 0, 0]
    cost, sph = (C.c_uint64 * 4)(), hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    assert hrt.lib().rt_get_tri_tree_cost(sph._h, cost) == _lib.RT_ERR_ARG


# ------------------------------------------------------------------------------------------------ errors and state
def test_errors_keep_the_geometry():
    L = hrt.lib()
    sd = CR.suzane_scene(W, H)
    tris, mats = sd.bvh[2], sd.bvh[3]
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    assert L.rt_refit_triangles_device(sph._h, C.c_void_p(on_device(sph, tris).data_ptr()), len(tris)) == _lib.RT_ERR_ARG
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    want, tree = primary_records(r), r.tri_tree()
    b = R.deform(tris, "jitter")
    t = on_device(r, b)
    assert t.data_ptr() % 16 == 0

    def unchanged():
        U.same_tree(r.tri_tree(), tree)
        assert (primary_records(r) == want).all()

    for args in ((C.c_void_p(t.data_ptr()), len(tris) - 1),        # a wrong n_tris
                 (C.c_void_p(t.data_ptr()), len(tris) + 1),
                 (C.c_void_p(t.data_ptr() + 4), len(tris)),         # misaligned
                 (None, len(tris))):                                # null with n > 0
        assert L.rt_refit_triangles_device(r._h, *args) == _lib.RT_ERR_ARG, args[1:]
        unchanged()
    bad = b.copy()
    bad["material"][len(bad) // 2] = len(mats)  # one index out of range
    with pytest.raises(hrt.RtError) as e:
        r.refit_triangles_device(on_device(r, bad))
    assert e.value.code == _lib.RT_ERR_ARG and "material" in str(e.value)
    unchanged()
    nan = b.copy()
    nan["c"][[3, 500], 2] = np.nan  # two triangles leave the finite set
    with pytest.raises(hrt.RtError) as e:
        r.refit_triangles_device(on_device(r, nan))
    assert e.value.code == _lib.RT_ERR_ARG and "2 triangles" in str(e.value)
    unchanged()
    # the other direction: a tree built with a non-finite triangle, refitted with it finite
    with_nan = U.nan_triangles()
    r2 = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r2.set_triangles_device(on_device(r2, with_nan), ONE_MATERIAL)
    tree2 = r2.tri_tree()
    with pytest.raises(hrt.RtError) as e:
        r2.refit_triangles_device(on_device(r2, U.random_triangles(9, 77)))
    assert e.value.code == _lib.RT_ERR_ARG and "1 triangles" in str(e.value)
    U.same_tree(r2.tri_tree(), tree2)
    # and the refit still works after all of them
    r.refit_triangles_device(t)
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(tris, b))


def test_state_scratch_failed_build_and_untouched_state():
    L = hrt.lib()
    sd = CR.suzane_scene(W, H)
    a, mats = sd.bvh[2], sd.bvh[3]
    # RT_ERR_STATE before any build, and after rt_set_bvh has left the device-geometry state
    r = hrt.Renderer(W, H, hrt.RT_MODE_TRIS)
    ta = on_device(r, a)
    assert L.rt_refit_triangles_device(r._h, C.c_void_p(ta.data_ptr()), len(a)) == _lib.RT_ERR_STATE
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    # image, frame count and stats are not touched
    r.draw_frames(2, 1000, 10)
    img, fc, st = r.read_image(), r.frame_count, r.stats()
    b = R.deform(a, "jitter")
    r.refit_triangles_device(on_device(r, b))
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st)
    # after rt_release_scratch: staging, arrivals and boxes are allocated again; the links were the tree's
    r.release_scratch()
    c = R.deform(a, "scatter", seed=3)
    r.refit_triangles_device(on_device(r, c))
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(a, c))
    # a build that fails on a bad material (other positions, so another topology) leaves the live links alone
    a2 = a[::-1].copy()
    a2["material"][7] = len(mats)
    with pytest.raises(hrt.RtError) as e:
        r.set_triangles_device(on_device(r, a2), mats)
    assert e.value.code == _lib.RT_ERR_ARG and "material" in str(e.value)
    r.refit_triangles_device(on_device(r, b))
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(a, b))
    fresh = device_renderer(moved_scene(sd, b), schedule=hrt.RT_SCHEDULE_TILES)
    assert (primary_records(r) == primary_records(fresh)).all()
    r.write_bvh(*sd.bvh)
    assert L.rt_refit_triangles_device(r._h, C.c_void_p(ta.data_ptr()), len(a)) == _lib.RT_ERR_STATE
