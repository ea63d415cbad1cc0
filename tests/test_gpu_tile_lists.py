"""k_trace_split<true, false, false, false> answers and shades a listed tile's primary rays when it makes their frame block
(csrc/rt_tile_lists.hpp, rt_kernels.hip trace_split BLOCKRES). Two things are pinned here:

  * the lists the device builds equal the host mirror's, byte for byte;
  * a draw with lists gives the oracle's image bits and query count, and so does the same draw with lists forced off;
  * the draw with lists resolved every block of every listed tile when it made it, and the draw without resolved none
    (rt_testing_get_tile_lists_resolved: the image and the counts cannot tell).

Every draw sets count_tests = 0, turns stealing off and asserts the kernel's full name.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from hrt.parallel import owned_rows, rank_params

pytestmark = pytest.mark.gpu

KERNEL = "k_trace_split<true, false, false, false>"
WALK = 0xFFFFFFFF
K = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _renderer(sd, mode, k=K, **params):
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, count_tests=0,
                 **{"fold": hrt.RT_FOLD_BUFFER, "steal": 1, **params})
    r.set_tile_lists(mode, k)
    return r


def _draw(sd, mode, k=K, **params):
    r = _renderer(sd, mode, k, **params)
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    assert st.kernel.decode() == KERNEL, (sd.name, st.kernel)
    _resolved(r, sd, mode)
    return r.read_image(), st, r


def _resolved(r, sd, mode, frames=None):
    """Every frame block of a listed tile is resolved when it is made (bounce cap >= 1, lists on); no other block is."""
    want = 0
    if mode == 2 and (sd.bounces is None or sd.bounces >= 1):
        want = int((r.tile_lists()[:, 0] != WALK).sum()) * (sd.frames if frames is None else frames)
    assert r.tile_lists_resolved() == want, (sd.name, mode, r.tile_lists_resolved(), want)


def _same(img, ref, what):
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)


def _both_vs_oracle(sd, k=K, rows=None, **params):
    """Lists on and forced off against the oracle; returns the renderer that drew with lists."""
    ref, q = scenes.oracle_render(sd) if rows is None else scenes.oracle_render(sd, rows=rows)
    out = None
    for mode in (2, 1):
        img, st, r = _draw(sd, mode, k, **params)
        n = ref.shape[0]
        _same(img[:n], ref, f"{sd.name} lists {'on' if mode == 2 else 'off'}")
        assert st.queries == q, (sd.name, mode, st.queries, q)
        out = out or (r, st)
    return out


def _with_params(cam, focal=None, blur=None):
    cam = cam.copy()
    prm = cam["params"].copy()
    if focal is not None:
        prm.reshape(-1)[0] = focal
    if blur is not None:
        prm.reshape(-1)[1] = blur
    cam["params"] = prm
    return cam


# ---- 1. the device lists equal the mirror's
@pytest.mark.parametrize("case", ["c3_160x90", "c3_1080p", "blur0", "blur20x", "ragged_70x45", "rank3of8", "focal0",
                                  "eye_inside", "straddling", "far_eye", "k3"])
def test_device_lists_equal_mirror(case):
    w, h, share, k = 160, 90, {}, K
    sd = scenes.config_c3(w, h, 1)
    cam, sph = sd.camera, sd.spheres
    if case == "c3_1080p":
        w, h = 1920, 1080
    elif case == "blur0":
        cam = _with_params(cam, blur=0.0)
    elif case == "blur20x":
        cam = _with_params(cam, blur=1.0)
    elif case == "ragged_70x45":
        w, h = 70, 45
    elif case == "rank3of8":
        w, h, share = 160, 96, rank_params(3, 8, 8)
    elif case == "focal0":
        cam = _with_params(cam, focal=0.0)
    elif case == "eye_inside":
        sph = hrt.spheres_array(_wall() + [Sphere.new_dielectric(Vec3(0.0, 0.0, 5.0), 0.5, 1.5)])
        cam = Camera.new(Vec3(0.0, 0.0, 5.1), Vec3(0.0, 0.0, -1.0), 6.0, 0.0, 0.5)
    elif case == "straddling":  # the eye just outside the surface, inside the padded ball with the lens radius
        sph = hrt.spheres_array(_wall() + [Sphere.new_dielectric(Vec3(0.0, 0.0, 5.0), 0.5, 1.5)])
        cam = Camera.new(Vec3(0.0, 0.0, 5.52), Vec3(0.0, 0.0, -1.0), 6.0, 0.05, 0.5)
    elif case == "far_eye":  # the f32 ray's error term, which grows with the eye's distance from the origin
        sph = hrt.spheres_array([Sphere.new_lambertian(Vec3(1.0e5 + 0.3 * (i % 8) - 1.2, 5.0e4 + 0.3 * (i // 8) - 0.6, -1.0),
                                                       0.1, Vec3(0.4, 0.5, 0.6)) for i in range(40)])
        cam = Camera.new(Vec3(1.0e5, 5.0e4, 5.0), Vec3(1.0e5, 5.0e4, -1.0), 6.0, 0.0, 0.5)
    elif case == "k3":
        k = 3
    sd = scenes.SceneDef(case, hrt.RT_MODE_SPHERE, w, h, cam, sph, frames=1, bounces=50, min_sphere_slots=0)
    r = _renderer(sd, 2, k, **share)
    dev = r.tile_lists()
    host = hrt.host_tile_lists(cam, w, h, sph, k=k, **share)
    assert dev.tobytes() == host.tobytes(), case
    if case in ("focal0", "eye_inside", "straddling"):
        assert (host[:, 0] == WALK).all()
    elif case == "c3_1080p":
        assert (host[:, 0] != WALK).mean() >= 0.95


# ---- 2. draws of the cover scene
@pytest.fixture(scope="module", params=[(64, 40), (70, 45)], ids=["64x40", "70x45"])
def cover33(request):
    w, h = request.param
    sd = scenes.config_c3(w, h, 33)
    return sd, scenes.oracle_render(sd)


@pytest.mark.parametrize("fold", [hrt.RT_FOLD_BUFFER, hrt.RT_FOLD_NEXT], ids=["accumulate", "fold_next"])
@pytest.mark.parametrize("budget_mb", [0, 1], ids=["one_launch", "budget_1mb"])
def test_cover_launches_vs_oracle(cover33, budget_mb, fold):
    sd, (ref, q) = cover33
    for mode in (2, 1):
        img, st, _ = _draw(sd, mode, fold=fold, job_frames=8, queue_budget_mb=budget_mb)
        what = f"{sd.width}x{sd.height} budget {budget_mb} fold {fold} lists {mode}"
        if budget_mb and sd.width == 70:  # 41,472 B a frame: 25 fit 1 MiB, so launches of whole jobs start at frames 0 and 24
            assert st.trace_launches == 2 and st.launch_frames == 24, (what, st.trace_launches, st.launch_frames)
        _same(img, ref, what)
        assert st.queries == q, what


def test_learning_launch_and_ordered_draw(cover33):
    sd, (ref, q) = cover33
    learnt = {}
    for mode in (2, 1):
        r = _renderer(sd, mode, job_frames=8, cost_order=2)
        r.draw_frames(sd.frames, 1000, 10)
        st = r.stats()
        assert st.ordered_launches == 0 and st.kernel.decode() == KERNEL, st.kernel
        _resolved(r, sd, mode)
        _same(r.read_image(), ref, f"learning draw lists {mode}")
        assert st.queries == q
        learnt[mode] = r.tile_order()
        r.reset_frame_count()
        r.draw_frames(sd.frames, 1000, 10)
        st = r.stats()
        assert st.ordered_launches == st.trace_launches == 1 and st.kernel.decode() == KERNEL
        _resolved(r, sd, mode)
        _same(r.read_image(), ref, f"ordered draw lists {mode}")
        assert st.queries == q
    # a tile is charged its primary queries whether they were answered at block time or walked
    np.testing.assert_array_equal(learnt[2][0], learnt[1][0])
    np.testing.assert_array_equal(learnt[2][1], learnt[1][1])
    # (a finished sample adds its bounces + 1: its queries, and one more for a path the bounce cap ended)
    assert q <= int(learnt[2][0].sum()) <= q + sd.width * sd.height * sd.frames


def test_rank_3_of_8():
    sd = scenes.config_c3(64, 72, 9)
    p = rank_params(3, 8, 8)
    rows = owned_rows(p["row0"], p["row_step"], sd.height, 8)
    _both_vs_oracle(sd, rows=(p["row0"], p["row_step"], len(rows), 8), **p)


# ---- 3. constructed scenes: camera at (0, 0, 5) looking down -z, a wall of small spheres far off to the sides
def _wall():
    """40 small spheres outside the view (x = +-30): they make the scene a tree, and no tile lists them."""
    return [Sphere.new_lambertian(Vec3(30.0 if i % 2 else -30.0, -4.0 + 0.4 * (i // 2), -3.0), 0.15, Vec3(0.4, 0.5, 0.6))
            for i in range(40)]


CAM = dict(eye=Vec3(0.0, 0.0, 5.0), at=Vec3(0.0, 0.0, -1.0), focal=6.0, blur=0.0, fov=0.5)


def _scene(name, extra, bounces=50, w=64, h=40, frames=3, cam=None):
    c = {**CAM, **(cam or {})}
    camera = Camera.new(c["eye"], c["at"], c["focal"], c["blur"], c["fov"])
    return scenes.SceneDef(name, hrt.RT_MODE_SPHERE, w, h, camera, hrt.spheres_array(_wall() + extra), frames=frames,
                           bounces=bounces, min_sphere_slots=0)


def _mat(i, c, rad):
    if i % 3 == 0:
        return Sphere.new_lambertian(c, rad, Vec3(0.8, 0.3 + 0.05 * i, 0.2))
    if i % 3 == 1:
        return Sphere.new_metal(c, rad, Vec3(0.7, 0.7, 0.5), 0.2)
    return Sphere.new_dielectric(c, rad, 1.5)


def _centre_tile(sd):
    lists = hrt.host_tile_lists(sd.camera, sd.width, sd.height, sd.spheres)
    tiles_w = (sd.width + 7) // 8
    return lists, lists[(sd.height // 16) * tiles_w + sd.width // 16]


def _aligned(n, nearest):
    """n spheres on the view axis, one behind the other; slot 40 + `nearest` is the one in front."""
    z = [2.0 - 0.9 * i for i in range(n)]
    if n:
        z[0], z[nearest] = z[nearest], z[0]
    return [_mat(i, Vec3(0.0, 0.0, z[i]), 0.3) for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, K, K + 1])
def test_list_lengths_last_listed_wins(n):
    """The centre tile's list holds the n aligned spheres (K + 1: the tile falls back to the walk), and the last listed one
    is the sphere in front, so the winner is found at the list's end."""
    sd = None
    for nearest in range(max(n, 1)):
        sd = _scene(f"aligned {n}", _aligned(n, nearest))
        lists, centre = _centre_tile(sd)
        if n in (0, K + 1):
            break
        slots = hrt.sphere_bvh_leaves(sd.spheres)["slots"]
        if slots[int(centre[int(centre[0])])] == 40 + nearest:
            break
    else:
        pytest.fail("no arrangement puts the front sphere last in the centre tile's list")
    assert centre[0] == (WALK if n == K + 1 else n), centre
    assert (lists[:, 0] == 0).any()  # all-sky tiles: their blocks yield no entry
    r, st = _both_vs_oracle(sd)
    assert r.tile_lists().tobytes() == lists.tobytes()


def test_coincident_spheres_lower_slot_wins():
    c = Vec3(0.0, 0.0, 1.0)
    extra = [Sphere.new_metal(c, 0.4, Vec3(0.9, 0.2, 0.2), 0.0), Sphere.new_lambertian(c, 0.4, Vec3(0.1, 0.9, 0.1)),
             Sphere.new_dielectric(c, 0.4, 1.5)]
    sd = _scene("coincident", extra)
    _, centre = _centre_tile(sd)
    assert centre[0] == 3, centre
    _both_vs_oracle(sd)


@pytest.mark.parametrize("material", ["lambert", "fuzzy_metal", "glass_outside", "glass_inside"])
def test_every_ray_of_a_tile_hits(material):
    c, rad = Vec3(0.0, 0.0, 2.5), 0.6
    if material == "lambert":
        extra = [Sphere.new_lambertian(c, rad, Vec3(0.8, 0.4, 0.2))]
    elif material == "fuzzy_metal":
        extra = [Sphere.new_metal(c, rad, Vec3(0.9, 0.6, 0.3), 0.3)]
    elif material == "glass_outside":
        extra = [Sphere.new_dielectric(c, rad, 1.5)]
    else:  # a bubble: the negative radius turns the normal, so the primary rays meet the glass from inside
        extra = [Sphere.new_dielectric(c, -rad, 1.5)]
    for w, h in ((64, 40), (70, 45)):
        sd = _scene(material, extra, w=w, h=h)
        _both_vs_oracle(sd)
        _both_vs_oracle(_scene(material + " cap 1", extra, bounces=1, w=w, h=h))


def test_camera_inside_a_glass_sphere_falls_back():
    extra = [Sphere.new_dielectric(Vec3(0.0, 0.0, 5.0), 0.5, 1.5), _mat(0, Vec3(0.0, 0.0, 1.0), 0.4)]
    sd = _scene("inside glass", extra, cam=dict(eye=Vec3(0.0, 0.0, 5.1)))
    lists, _ = _centre_tile(sd)
    assert (lists[:, 0] == WALK).all()
    _both_vs_oracle(sd)


@pytest.mark.parametrize("nlarge", [0, 14])
@pytest.mark.parametrize("bounces", [0, 1, 50])
def test_bounce_caps_and_large_lists(bounces, nlarge):
    extra = [_mat(i, Vec3(-1.2 + 0.35 * (i % 8), -0.6 + 0.4 * (i // 8), 1.0 - 0.5 * (i % 3)), 0.15) for i in range(24)]
    extra += [Sphere.new_lambertian(Vec3(-6.0 + 3.0 * (k % 5), -21.0 - 0.01 * k, 1.0 - 3.0 * (k // 5)), 20.0,
                                    Vec3(0.5, 0.5, 0.4 + 0.02 * k)) for k in range(nlarge)]
    sd = _scene(f"cap {bounces} large {nlarge}", extra, bounces=bounces)
    assert len(hrt.sphere_bvh_leaves(sd.spheres)["large"]) == nlarge
    _both_vs_oracle(sd)


def test_camera_change_rebuilds_the_lists():
    extra = [_mat(i, Vec3(-1.2 + 0.35 * (i % 8), -0.6 + 0.4 * (i // 8), 1.0 - 0.5 * (i % 3)), 0.15) for i in range(24)]
    sd1 = _scene("first view", extra)
    sd2 = _scene("second view", extra, cam=dict(eye=Vec3(2.0, 1.0, 5.0), at=Vec3(-0.5, 0.0, 0.0)))
    r = _renderer(sd1, 2)
    r.draw_frames(sd1.frames, 1000, 10)
    _same(r.read_image(), scenes.oracle_render(sd1)[0], "first view")
    lists1 = r.tile_lists()
    r.set_camera(sd2.camera)
    r.reset_frame_count()
    r.draw_frames(sd2.frames, 1000, 10)
    assert r.stats().kernel.decode() == KERNEL
    _resolved(r, sd2, 2)
    ref2, q2 = scenes.oracle_render(sd2)
    _same(r.read_image(), ref2, "second view, after the first")
    assert r.stats().queries == q2
    lists2 = r.tile_lists()
    assert lists2.tobytes() == hrt.host_tile_lists(sd2.camera, 64, 40, sd2.spheres).tobytes() != lists1.tobytes()
    img, st, _ = _draw(sd2, 2)
    _same(r.read_image(), img, "second view: a fresh renderer")
