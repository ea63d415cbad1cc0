"""rt_set_triangles_device on the GPU: the device-built tree is the host mirror's, byte for byte; every query and draw
through it gives what the host-built SAH tree gives (the hit contract of tri_bvh = 1 does not depend on the tree); the
call's errors leave the renderer as it was. No tolerance anywhere: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import hrt
import scenes
from hrt import _lib

import lbvh_util as U
import test_gpu_cast_rays as CR

pytestmark = pytest.mark.gpu

W, H = 64, 48
ONE_MATERIAL = np.array([hrt.Material.new_lambertian(hrt.Vec3(0.5, 0.5, 0.5))], dtype=hrt.MATERIAL_DTYPE).reshape(-1)
TREE_CASES = dict(U.cpu_cases(), lucy=lambda: U.mesh_triangles("lucy_lp_20.obj"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def on_device(r, tris: np.ndarray):
    import torch

    raw = np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64)
    return torch.from_numpy(raw.copy()).to(r._torch_device())


def device_renderer(sd, **params):
    """scenes.make_renderer with the triangles through rt_set_triangles_device instead of rt_set_bvh."""
    r = hrt.Renderer(sd.width, sd.height, sd.mode)
    kw = {"count_tests": 1}
    if sd.bounces is not None:
        kw["bounces"] = sd.bounces
    if sd.min_sphere_slots is not None:
        kw["min_sphere_slots"] = sd.min_sphere_slots
    kw.update(params)
    r.set_params(**kw)
    r.set_camera(sd.camera)
    if sd.mode != hrt.RT_MODE_TRIS:
        r.write_spheres(sd.spheres if sd.spheres is not None else hrt.spheres_array([]))
    r.set_triangles_device(on_device(r, sd.bvh[2]), sd.bvh[3])
    return r


def host_renderer(sd, **params):
    r = scenes.make_renderer(sd)
    r.set_params(**params)
    return r


def primary_records(r, time=1000):
    o, d = r.primary_rays(time)
    return CR._records(r.cast_rays(o.view(-1, 3), d.view(-1, 3)))


# ------------------------------------------------------------------------------------------------ tree identity
@pytest.mark.parametrize("name", list(TREE_CASES))
def test_device_tree_is_the_mirrors(name):
    tris = TREE_CASES[name]()
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), ONE_MATERIAL)
    got, want = r.tri_tree(), hrt.lbvh_build(tris)
    U.same_tree(got, want)
    if name == "lucy":
        assert len(tris) > 19000 and int(got["info"][0]) == len(tris) - 1


def test_rebuilds_on_one_renderer_match_the_mirror():
    """lucy three times on one renderer, the vertices moved on the device in between: the fit's hand-offs with the
    buffers of the build before still in the caches."""
    import torch

    tris = TREE_CASES["lucy"]()
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    t = on_device(r, tris).view(torch.float32)  # (m, 16): a.xyzw, b.xyzw, c.xyzw, custom.xyz, material
    for step in range(3):
        r.set_triangles_device(t, ONE_MATERIAL)
        mirror = hrt.lbvh_build(t.cpu().numpy())
        U.same_tree(r.tri_tree(), mirror)
        assert int(mirror["info"][2]) == len(tris)
        moved = t.clone()
        for v in (0, 4, 8):  # a shear and a wave along x, in f32 on the device
            moved[:, v] = t[:, v] * 1.25 + 0.3 * torch.sin(t[:, v + 1] * (2.0 + step))
            moved[:, v + 2] = t[:, v + 2] - 0.2 * t[:, v + 1]
        t = moved


def test_host_sah_tree_reads_back_in_the_same_format():
    sd = CR.suzane_scene(16, 16)
    tree = host_renderer(sd).tri_tree()
    v, finite = U.tri_f64(sd.bvh[2])
    assert finite.all() and sorted(tree["order"].tolist()) == list(range(len(v)))
    assert int(tree["info"][3]) == 0 and len(tree["nodes"]) == int(tree["info"][0]) > 100


# ------------------------------------------------------------------------------------------------ hits
HIT_SCENES = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed-simple": lambda w, h: CR.mixed_scene(w, h, 0),
              "mixed-defer": lambda w, h: CR.mixed_scene(w, h, 12), "mixed-bvh": lambda w, h: CR.mixed_scene(w, h, 60)}


@pytest.mark.parametrize("name", list(HIT_SCENES))
def test_hits_are_the_host_trees(name):
    sd = HIT_SCENES[name](W, H)
    want = primary_records(host_renderer(sd, tri_bvh=1))
    r = device_renderer(sd)
    assert r.params.tri_bvh == 0
    for tb in (0, 1):  # rt_params.tri_bvh does not matter with device geometry
        r.set_params(tri_bvh=tb)
        got = primary_records(r)
        bad = (got != want).any(axis=1)
        assert not bad.any(), (name, tb, np.argwhere(bad)[:8].ravel().tolist())
    assert (want[:, 1] >= 0).sum() > 100
    tri = (want[:, 5] & hrt.RT_HIT_TRIANGLE) != 0
    assert tri.any() and (want[tri, 1] < len(sd.bvh[2])).all()  # prim: the index into the caller's array


# ------------------------------------------------------------------------------------------------ other queries, draws
def test_occluded_trace_and_bounce_agree_with_the_host_tree():
    import torch

    sd = CR.mixed_scene(W, H, 12)
    sd.bounces = 5
    a, b = host_renderer(sd, tri_bvh=1), device_renderer(sd)
    o, d = a.primary_rays(1000)
    o, d = o.view(-1, 3).contiguous(), d.view(-1, 3).contiguous()
    t = a.cast_rays(o, d)["t"]
    # beyond the hit for even rays (occluded), short of it for odd ones; the rays that miss get a finite reach
    scale = torch.where(torch.arange(len(t), device=t.device) % 2 == 0, 1.25, 0.75)
    tmax = torch.where(t < hrt.RT_T_MISS, t * scale, torch.full_like(t, 7.0))
    occ = [r.occluded(o, d, tmax).cpu().numpy() for r in (a, b)]
    assert (occ[0] == occ[1]).all() and occ[0].any() and not occ[0].all()
    rng = a.primary_rng(1000).view(-1).contiguous()
    rad = [tuple(x.cpu().numpy() for x in r.trace_rays(o, d, rng=rng, want_queries=True)) for r in (a, b)]
    assert (rad[0][0].view(np.uint32) == rad[1][0].view(np.uint32)).all() and (rad[0][1] == rad[1][1]).all()
    assert rad[0][1].max() > 1
    state = []
    for r in (a, b):
        dev = r._torch_device()
        bo, bd, bs = o.clone(), d.clone(), rng.clone()
        tp = torch.ones((len(bo), 3), dtype=torch.float32, device=dev)
        q = torch.zeros((len(bo),), dtype=torch.int32, device=dev)
        hits = torch.zeros((len(bo), 8), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        r.bounce_rays(bo, bd, bs, throughput=tp, queries=q, hits=hits, count_out=count)
        state.append([x.cpu().numpy() for x in (bo, bd, bs, tp, q, hits, count)])
    for x, y in zip(*state):
        assert x.tobytes() == y.tobytes()
    assert 0 < int(state[0][6][0]) < len(o)


@pytest.mark.parametrize("schedule", [hrt.RT_SCHEDULE_TILES, hrt.RT_SCHEDULE_QUEUE])
@pytest.mark.parametrize("mode", ["tris", "mixed"])
def test_draws_match_the_uncapped_oracle(mode, schedule):
    if mode == "tris":
        suz = hrt.SceneTris.new_suzane(40, 24)
        sd = scenes.SceneDef("suzane", hrt.RT_MODE_TRIS, 40, 24, suz.camera, bvh=suz.tris_bvh.view(), frames=2)
    else:
        sd = scenes.config_c4(40, 24, 2)
    r = device_renderer(sd, schedule=schedule)
    r.draw_frames(sd.frames, 1000, 10)
    img, st = r.read_image(), r.stats()
    ref, q = scenes.oracle_render(sd, step_cap=0)
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert st.queries == q and st.schedule == schedule


def test_scene_tris_init_with_device_geometry():
    s = hrt.SceneTris.new_cube(W, H)
    s.init(device_geometry=True)
    s2 = hrt.SceneTris.new_cube(W, H)
    s2.init()
    s2.renderer.set_params(tri_bvh=1)
    assert (primary_records(s.renderer) == primary_records(s2.renderer)).all()


# ------------------------------------------------------------------------------------------------ update
def test_moved_mesh_hits_equal_a_fresh_renderers():
    import torch

    sd = CR.suzane_scene(W, H)
    r = device_renderer(sd)
    before = primary_records(r)
    t = on_device(r, sd.bvh[2]).view(torch.float32)
    moved = t.clone()
    for v in (0, 4, 8):
        moved[:, v] = t[:, v] + 0.4 * torch.cos(t[:, v + 1] * 3.0)
        moved[:, v + 1] = t[:, v + 1] * 0.8
    r.set_triangles_device(moved, sd.bvh[3])
    got = primary_records(r)
    assert (got != before).any()
    moved_np = moved.cpu().numpy().view(hrt.TRIANGLE_DTYPE).reshape(-1)
    fresh = device_renderer(scenes.SceneDef(sd.name, sd.mode, W, H, sd.camera, bvh=(sd.bvh[0], sd.bvh[1], moved_np, sd.bvh[3]),
                                            frames=1, bounces=1))
    assert (got == primary_records(fresh)).all()
    # and the host's SAH tree over the moved triangles (the heap is not read with tri_bvh = 1)
    host = hrt.Renderer(W, H, sd.mode)
    host.set_params(tri_bvh=1)
    host.set_camera(sd.camera)
    host.write_bvh(sd.bvh[0], sd.bvh[1], moved_np, sd.bvh[3])
    assert (got == primary_records(host)).all()


# ------------------------------------------------------------------------------------------------ errors and state
def test_errors_keep_the_geometry_and_set_bvh_leaves_the_state():
    L = hrt.lib()
    sd = CR.suzane_scene(W, H)
    tris, mats = sd.bvh[2], sd.bvh[3]
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    t_sph = on_device(sph, tris)
    assert L.rt_set_triangles_device(sph._h, C.c_void_p(t_sph.data_ptr()), len(tris), mats.ctypes.data,
                                     len(mats)) == _lib.RT_ERR_ARG
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    want = primary_records(r)
    tree = r.tri_tree()
    t = on_device(r, tris)
    assert t.data_ptr() % 16 == 0
    for args in ((C.c_void_p(t.data_ptr() + 4), len(tris) - 1, mats.ctypes.data, len(mats)),   # misaligned
                 (None, len(tris), mats.ctypes.data, len(mats)),                                  # null with n > 0
                 (C.c_void_p(t.data_ptr()), len(tris), None, len(mats)),                          # null materials
                 (C.c_void_p(t.data_ptr()), 1 << 26, mats.ctypes.data, len(mats)),
                 (C.c_void_p(t.data_ptr()), len(tris), mats.ctypes.data, 1 << 28)):
        assert L.rt_set_triangles_device(r._h, *args) == _lib.RT_ERR_ARG, args[1:]
    bad = tris.copy()
    bad["material"][len(bad) // 2] = len(mats)  # one index out of range
    with pytest.raises(hrt.RtError) as e:
        r.set_triangles_device(on_device(r, bad), mats)
    assert e.value.code == _lib.RT_ERR_ARG and "material" in str(e.value)
    U.same_tree(r.tri_tree(), tree)
    assert (primary_records(r) == want).all()  # the geometry before still answers
    # the call leaves image, frame count and stats alone
    r.draw_frames(2, 1000, 10)
    img, fc, st = r.read_image(), r.frame_count, r.stats()
    r.set_triangles_device(t, mats)
    st2 = r.stats()
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(st2) == bytes(st)
    # rt_release_scratch frees the build's scratch and staging (counted in device_bytes, which a draw reports), not the tree
    r.release_scratch()
    assert (primary_records(r) == want).all()
    r.draw_frames(1, 1020, 10)
    assert r.stats().device_bytes < st.device_bytes
    # rt_set_bvh gives the heap back: tri_bvh = 0 walks it again
    r.write_bvh(*sd.bvh)
    assert r.params.tri_bvh == 0
    ref = host_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    assert (primary_records(r) == primary_records(ref)).all()
    for x in (r, ref):
        x.reset_frame_count()
        x.draw_frames(1, 1000, 10)
    assert r.stats().kernel == ref.stats().kernel and b"k_render" in r.stats().kernel
    assert (r.read_image().view(np.uint32) == ref.read_image().view(np.uint32)).all()
    assert r.stats().node_tests == ref.stats().node_tests
