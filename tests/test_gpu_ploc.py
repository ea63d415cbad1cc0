"""rt_set_triangles_device_with(RT_TREE_PLOC) on the GPU: the device tree is the host mirror's (hrt.lbvh_build(...,
builder=1)), byte for byte, through the one-workgroup tail and through the iterations that take their own launches; the
refit on it is the mirror's; every query and draw through it gives what builder 0's tree and the host-built SAH tree
give; errors leave the renderer as it was. No tolerance anywhere: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import _lib

import lbvh_refit_util as R
import lbvh_util as U
import test_gpu_cast_rays as CR
import test_ploc_abi as A
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device, primary_records
from test_gpu_lbvh_refit import _queries, host_sah_renderer

pytestmark = pytest.mark.gpu

W, H = 64, 48
PLOC = A.PLOC
TREE_CASES = dict(A.CASES, lucy=lambda: U.mesh_triangles("lucy_lp_20.obj"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def ploc_renderer(sd, **params):
    """device_renderer (builder 0), then the same triangles again with builder 1."""
    r = device_renderer(sd, **params)
    r.set_triangles_device(on_device(r, sd.bvh[2]), sd.bvh[3], builder=PLOC)
    return r


def info_of(tree: dict, builder: int) -> list:
    """rt_get_tri_tree_info's eight words from a mirror's info."""
    i = tree["info"].tolist()
    return [builder, i[0], i[2], i[3], i[4], i[5], i[6], 0]


# ------------------------------------------------------------------------------------------------ tree identity
@pytest.mark.parametrize("name", list(TREE_CASES))
def test_device_tree_is_the_mirrors(name):
    tris = TREE_CASES[name]()
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), ONE_MATERIAL, builder=PLOC)
    got, want = r.tri_tree(), hrt.lbvh_build(tris, builder=PLOC)
    U.same_tree(got, want)
    assert r.tri_tree_info().tolist() == info_of(want, PLOC)
    if name == "lucy":  # many workgroups, and several iterations before the tail
        assert len(tris) > 19000 and int(got["info"][0]) == len(tris) - 1 and int(got["info"][5]) > 30
    if name == "chain230":  # the fit at its 64-level limit, and flat iterations
        assert int(got["info"][4]) == 64 and int(got["info"][5]) == 64 and int(got["info"][6]) >= 1


def test_rebuilds_on_one_renderer_match_the_mirror():
    """lucy three times on one renderer, the vertices moved on the device in between: the cluster lists, flags and tile
    counts of the build before are still in the buffers and the caches."""
    import torch

    tris = TREE_CASES["lucy"]()
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    t = on_device(r, tris).view(torch.float32)  # (m, 16): a.xyzw, b.xyzw, c.xyzw, custom.xyz, material
    for step in range(3):
        r.set_triangles_device(t, ONE_MATERIAL, builder=PLOC)
        mirror = hrt.lbvh_build(t.cpu().numpy(), builder=PLOC)
        U.same_tree(r.tri_tree(), mirror)
        assert int(mirror["info"][2]) == len(tris)
        moved = t.clone()
        for v in (0, 4, 8):  # a shear and a wave along x, in f32 on the device
            moved[:, v] = t[:, v] * 1.25 + 0.3 * torch.sin(t[:, v + 1] * (2.0 + step))
            moved[:, v + 2] = t[:, v + 2] - 0.2 * t[:, v + 1]
        t = moved


@pytest.mark.parametrize("name", ["suzanne", "chain230"])
def test_refits_are_the_mirrors(name):
    """build(A, 1), refit(B), refit(C) leaves lbvh_refit(A, C, builder=1); the chain's fit climbs 64 levels."""
    a = TREE_CASES[name]()
    b, c = R.deform(a, "jitter"), R.deform(a, "scatter", seed=5)
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, a), ONE_MATERIAL, builder=PLOC)
    r.refit_triangles_device(on_device(r, b))
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(a, b, builder=PLOC))
    r.refit_triangles_device(on_device(r, c))
    want = hrt.lbvh_refit(a, c, builder=PLOC)
    U.same_tree(r.tri_tree(), want)
    assert r.tri_tree_info().tolist() == info_of(want, PLOC)
    r.refit_triangles_device(on_device(r, a))  # the unmoved array: the build's bytes
    U.same_tree(r.tri_tree(), hrt.lbvh_build(a, builder=PLOC))
    if name == "chain230":
        assert int(want["info"][4]) == 64


# ------------------------------------------------------------------------------------------------ hits, queries, draws
HIT_SCENES = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}


@pytest.mark.parametrize("name", list(HIT_SCENES))
def test_hits_queries_and_draws_equal_builder_0s_and_the_host_trees(name):
    import torch

    sd = HIT_SCENES[name](W, H)
    sd.bounces = 5
    r, lbvh, host = ploc_renderer(sd), device_renderer(sd), host_sah_renderer(sd)
    assert int(r.tri_tree_info()[0]) == PLOC and int(lbvh.tri_tree_info()[0]) == 0
    got = primary_records(r)
    assert (got[:, 1] >= 0).sum() > 100
    assert (got == primary_records(lbvh)).all() and (got == primary_records(host)).all()
    o, d = host.primary_rays(1000)
    o, d = o.view(-1, 3).contiguous(), d.view(-1, 3).contiguous()
    t = host.cast_rays(o, d)["t"]
    scale = torch.where(torch.arange(len(t), device=t.device) % 2 == 0, 1.25, 0.75)
    tmax = torch.where(t < hrt.RT_T_MISS, t * scale, torch.full_like(t, 7.0))
    rng = host.primary_rng(1000).view(-1).contiguous()
    want = _queries(r, o, d, tmax, rng)  # rt_occluded, rt_trace_rays, one rt_bounce_rays step
    for other in (_queries(lbvh, o, d, tmax, rng), _queries(host, o, d, tmax, rng)):
        for x, y in zip(want, other):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert want[0].any() and not want[0].all()
    for schedule in (hrt.RT_SCHEDULE_TILES, hrt.RT_SCHEDULE_QUEUE):
        images = []
        for x in (r, lbvh):
            x.set_params(schedule=schedule)
            x.reset_frame_count()
            x.draw_frames(2, 1000, 10)
            images.append(x.read_image().view(np.uint32))
            assert x.stats().schedule == schedule
        assert (images[0] == images[1]).all() and images[0].any()


def test_tri_tree_cost_is_the_hosts():
    sd = CR.suzane_scene(16, 16)
    r = ploc_renderer(sd)
    tree = r.tri_tree()
    cost = r.tri_tree_cost().tolist()
    assert cost == hrt.lbvh_cost(tree).tolist() == R.numpy_cost(tree)
    assert cost[2] == len(sd.bvh[2]) - 1 and cost[3] == len(sd.bvh[2])
    lbvh = hrt.lbvh_cost(hrt.lbvh_build(sd.bvh[2])).tolist()
    assert cost[0] + cost[1] < lbvh[0] + lbvh[1]


# ------------------------------------------------------------------------------------------------ errors and state
def test_errors_keep_the_geometry():
    L = hrt.lib()
    sd = CR.suzane_scene(W, H)
    tris, mats = sd.bvh[2], np.ascontiguousarray(sd.bvh[3], dtype=hrt.MATERIAL_DTYPE)
    pm, nm = mats.ctypes.data, len(mats)
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    ts = on_device(sph, tris)
    assert L.rt_set_triangles_device_with(sph._h, C.c_void_p(ts.data_ptr()), len(tris), pm, nm, PLOC) == _lib.RT_ERR_ARG
    info = (C.c_uint32 * 8)()
    assert L.rt_get_tri_tree_info(sph._h, info) == _lib.RT_ERR_ARG
    r = ploc_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    want, tree, winfo = primary_records(r), r.tri_tree(), r.tri_tree_info().tolist()
    other = R.deform(tris, "scatter")[::-1].copy()  # other positions: another topology, were it to be built
    t = on_device(r, other)
    p = C.c_void_p(t.data_ptr())

    def unchanged():
        U.same_tree(r.tri_tree(), tree)
        assert r.tri_tree_info().tolist() == winfo and (primary_records(r) == want).all()

    for args in ((p, len(tris), pm, nm, 2),                           # unknown builders
                 (p, len(tris), pm, nm, 0xFFFFFFFF),
                 (C.c_void_p(t.data_ptr() + 4), len(tris) - 1, pm, nm, PLOC),  # misaligned
                 (None, len(tris), pm, nm, PLOC),                     # null with n > 0
                 (p, len(tris), None, nm, PLOC),                      # null materials
                 (p, 1 << 26, pm, nm, PLOC)):                         # too many
        assert L.rt_set_triangles_device_with(r._h, *args) == _lib.RT_ERR_ARG, args[1:]
        unchanged()
    bad = other.copy()
    bad["material"][len(bad) // 2] = nm  # one index out of range: found on the device, after the sort
    with pytest.raises(hrt.RtError) as e:
        r.set_triangles_device(on_device(r, bad), mats, builder=PLOC)
    assert e.value.code == _lib.RT_ERR_ARG and "material" in str(e.value)
    unchanged()
    r.refit_triangles_device(on_device(r, R.deform(tris, "jitter")))  # the live links were not touched
    U.same_tree(r.tri_tree(), hrt.lbvh_refit(tris, R.deform(tris, "jitter"), builder=PLOC))


def test_builders_alternate_scratch_state_and_untouched_state():
    L = hrt.lib()
    sd = CR.suzane_scene(W, H)
    a, mats = sd.bvh[2], sd.bvh[3]
    info = (C.c_uint32 * 8)()
    r = hrt.Renderer(W, H, hrt.RT_MODE_TRIS)
    assert L.rt_get_tri_tree_info(r._h, info) == _lib.RT_ERR_STATE  # no triangle tree yet
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    ta = on_device(r, a)
    want = primary_records(r)
    # image, frame count and stats are not touched
    r.draw_frames(2, 1000, 10)
    img, fc, st = r.read_image(), r.frame_count, r.stats()
    r.set_triangles_device(ta, mats, builder=PLOC)
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st)
    ploc, lbvh = hrt.lbvh_build(a, builder=PLOC), hrt.lbvh_build(a)
    U.same_tree(r.tri_tree(), ploc)
    # builder 1, then 0, and back
    r.set_triangles_device(ta, mats, builder=0)
    U.same_tree(r.tri_tree(), lbvh)
    assert r.tri_tree_info().tolist() == info_of(lbvh, 0)
    r.set_triangles_device(ta, mats, builder=PLOC)
    U.same_tree(r.tri_tree(), ploc)
    # after rt_release_scratch everything the builder needs is allocated again
    r.release_scratch()
    r.set_triangles_device(ta, mats, builder=PLOC)
    U.same_tree(r.tri_tree(), ploc)
    assert r.tri_tree_info().tolist() == info_of(ploc, PLOC) and (primary_records(r) == want).all()
    r.release_scratch()  # (frees the builder's scratch and its pinned status block, not the tree)
    assert (primary_records(r) == want).all()
    # rt_set_bvh leaves the state: no tree with tri_bvh = 0, the host SAH tree with tri_bvh = 1
    r.write_bvh(*sd.bvh)
    assert L.rt_get_tri_tree_info(r._h, info) == _lib.RT_ERR_STATE
    r.set_params(tri_bvh=1)
    host = r.tri_tree_info().tolist()
    tree = r.tri_tree()
    assert host == [0xFFFFFFFF] + [int(tree["info"][k]) for k in (0, 2, 3, 4)] + [0, 0, 0]
    assert (primary_records(r) == want).all()
