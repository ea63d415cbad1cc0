"""k_trace_split<true, false, false, false> in 512-lane workgroups, walking the pre-rotated LDS node table (rt_kernels.hip
split_prerot / split_wg, prerot_node, bvh_walk_noovf<.., PREROT>).

The table holds every [min|max] fp16 pair of a node in both orders, and a lane reads the order with the near plane in the
low half at three byte offsets it forms from the signs of 1/d once per walk call — where box_hit_so rotates the pairs per
box step. The same halves reach the same FMAs, so every draw here must give the CPU oracle's image bits and query count.
Every draw turns stealing off and asserts the kernel's full name; the counting twin (<true, false, true, false>: 256
lanes, 32-B nodes, box_hit_so) must give the same image and queries where a case names it.

* every octant and the axis cases: a camera inside a shell of spheres (secondary rays leave in every octant), cameras whose
  primary rays have direction components of exactly +0 and -0 (checked on rt_primary_rays), and boxes as thin as the
  node packer makes them;
* the table's ends: a tree of exactly LNODE_CAP nodes and depth 8 (the last node's z group is read), a one-leaf tree, an
  empty tree (root word with count 0), and LNODE_CAP + 1 nodes, which must run <false, ..> as before;
* the workgroup: draws with fewer jobs than a workgroup has waves (8) and with one more, a rank's row share, two launches
  the second of which folds the first, a learning launch and the ordered draw after it, the tail split;
* rt_testing_get_tile_lists_resolved still equals listed tiles x frames.

A box that is exactly flat in fp16 — min and max the same half, where the two orders of a pair coincide — cannot be built
through the renderer: pack_bvh_hnodes steps every bound one f32 ulp outward and rounds it to fp16 away from the box, so
max > min strictly on every axis of every node. test_thinnest_boxes draws the nearest thing, spheres of radius 2^-14
whose boxes are one or two fp16 steps wide.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from hrt.parallel import owned_rows, rank_params
from test_gpu_lds_spheres import NODE_CAP, DEPTH_CAP, _full_table
from test_gpu_lds_spheres import _oracle as _lds_oracle

pytestmark = pytest.mark.gpu

KERNEL = "k_trace_split<true, false, false, false>"
TWIN = "k_trace_split<true, false, true, false>"
BEYOND = "k_trace_split<false, false, false, false>"
WALK = 0xFFFFFFFF
WG_WAVES = 8  # (split_wg / 64)
SIZES = {"64x40": (64, 40), "70x45": (70, 45)}  # whole and ragged 8x8 tiles
FRAMES = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


_ORACLE = {}


def _oracle(sd, **kw):
    key = (sd.name, sd.width, sd.height, sd.frames, tuple(sorted(kw.items())))
    if key not in _ORACLE:  # once per scene, shared and read-only
        img, q = scenes.oracle_render(sd, **kw)
        img.setflags(write=False)
        _ORACLE[key] = (img, q)
    return _ORACLE[key]


def _renderer(sd, count_tests=0, lists=None, **params):
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, steal=1, count_tests=count_tests, **params)
    if lists is not None:
        r.set_tile_lists(lists, 8)
    return r


def _draw(sd, kernel=KERNEL, count_tests=0, lists=None, **params):
    r = _renderer(sd, count_tests, lists, **params)
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    assert st.kernel.decode() == kernel, (sd.name, st.kernel)
    return r.read_image(), st, r


def _same(img, ref, what):
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)


def _vs_oracle(sd, ref, q, twin=False, **params):
    """The headline kernel against the oracle; with `twin` the counting kernel too: equal image, equal queries."""
    img, st, r = _draw(sd, **params)
    n = ref.shape[0]
    _same(img[:n], ref, sd.name)
    assert st.queries == q, (sd.name, st.queries, q)
    if twin:
        img_t, st_t, _ = _draw(sd, TWIN, count_tests=1, **params)
        _same(img_t, img, f"{sd.name}: counting twin")
        assert st_t.queries == st.queries, (sd.name, st_t.queries, st.queries)
    return img, st, r


def _ball(k, c, r):
    if k % 3 == 0:
        return Sphere.new_lambertian(Vec3(*c), r, Vec3(0.2 + 0.09 * (k % 8), 0.6, 0.9 - 0.1 * (k % 8)))
    if k % 3 == 1:
        return Sphere.new_metal(Vec3(*c), r, Vec3(0.8, 0.7, 0.3 + 0.05 * (k % 8)), 0.05 * (k % 4))
    return Sphere.new_dielectric(Vec3(*c), r, 1.5)


def _leaves(sd):
    return hrt.sphere_bvh_leaves(sd.spheres, sd.min_sphere_slots or 0)


# ---- every octant and the axis cases
def _shell(size):
    """The camera at the centre of a shell of 56 spheres, seven in each octant: a path's secondary rays leave its first hit
    towards spheres in every octant, so walks run with every combination of the three offsets."""
    rng = np.random.default_rng(20)
    balls = []
    for k in range(56):
        s = np.array([1.0 if k & 1 else -1.0, 1.0 if k & 2 else -1.0, 1.0 if k & 4 else -1.0])
        d = s * (0.15 + 0.85 * rng.random(3))
        c = d / np.linalg.norm(d) * (3.0 + 2.0 * rng.random())
        balls.append(_ball(k, [float(np.float32(v)) for v in c], 0.55))
    w, h = SIZES[size]
    cam = Camera.new(Vec3(0.0, 0.0, 0.0), Vec3(0.3, 0.2, -1.0), 1.0, 0.0, 1.6)
    return scenes.SceneDef(f"shell {size}", hrt.RT_MODE_SPHERE, w, h, cam, hrt.spheres_array(balls), frames=FRAMES,
                           bounces=50, min_sphere_slots=0)


@pytest.mark.parametrize("size", list(SIZES))
def test_camera_inside_a_shell_of_spheres(size):
    sd = _shell(size)
    B = _leaves(sd)
    assert 2 <= len(B["leaves"]) - 1 <= NODE_CAP and B["depth"] <= DEPTH_CAP
    _vs_oracle(sd, *_oracle(sd), twin=True)


def _zero_camera(kind):
    """Raw camera records without a right vector (test_gpu_uniform_guards' constructions): a primary ray's direction is
    (0 * ux) * k + (up * uy) * k + direction per component, so d.x — and with "axis", no up vector either, d.y — is a zero
    whose sign is -0 in the image quadrant where both products are -0 and the camera direction's zero is -0, else +0."""
    cam = np.zeros((), dtype=hrt.CAMERA_DTYPE)
    # (the direction is focus point - origin, (eye + vn * focal) - (eye + 0): -0 only as (-0 + -0) - (-0 + 0))
    cam["eye"] = (-0.0, -0.0 if kind == "axis" else 0.0, 3.0, 0.0)
    cam["direction"] = (-0.0, -0.0 if kind == "axis" else 0.0, -1.0, 0.0)
    if kind == "plane":
        cam["up"] = (0.0, 1.0, 0.0, 0.0)
    cam["params"] = (1.0, 0.0, 0.8, 0.0)
    return cam


def _zero_scene(kind, size):
    # the mirror at the axis sends the axis rays straight back: secondary rays with zero components too
    balls = [Sphere.new_metal(Vec3(0.0, 0.0, -4.0), 1.0, Vec3(0.8, 0.8, 0.8), 0.0)]
    balls += [_ball(k, (-3.5 + 1.0 * (k % 8), -1.5 + 1.5 * (k // 8), -5.0 + 0.5 * (k % 3)), 0.4) for k in range(24)
              if (k % 8, k // 8) not in ((3, 1), (4, 1))]
    balls.append(Sphere.new_lambertian(Vec3(0.0, -1003.0, -5.0), 1000.0, Vec3(0.5, 0.5, 0.5)))
    w, h = SIZES[size]
    return scenes.SceneDef(f"zero {kind} {size}", hrt.RT_MODE_SPHERE, w, h, _zero_camera(kind), hrt.spheres_array(balls),
                           frames=FRAMES, bounces=50, min_sphere_slots=0)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["axis", "plane"])
def test_direction_components_of_plus_and_minus_zero(kind, size):
    sd = _zero_scene(kind, size)
    assert len(_leaves(sd)["leaves"]) > 2  # a tree with box steps
    _vs_oracle(sd, *_oracle(sd), twin=True)


@pytest.mark.parametrize("kind", ["axis", "plane"])
def test_the_zero_cameras_make_zeros_of_both_signs(kind):
    r = _renderer(_zero_scene(kind, "64x40"))
    _, d = r.primary_rays(1000)
    bits = d.cpu().numpy().view(np.uint32)
    for axis in (0, 1) if kind == "axis" else (0,):
        assert set(np.unique(bits[..., axis]).tolist()) == {0x00000000, 0x80000000}, (kind, axis)
    assert (bits[..., 2] & 0x7FFFFFFF != 0).all()


def test_thinnest_boxes():
    """Spheres of radius 2^-14 between visible ones: their leaves' boxes are as thin as the packer makes a box (see above)."""
    sd = _shell("70x45")
    tiny = [Sphere.new_lambertian(Vec3(-1.0 + 0.25 * i, 0.1 * (i % 3) - 0.1, -2.0 - 0.125 * i), 2.0 ** -14, Vec3(0.9, 0.1, 0.1))
            for i in range(9)]
    sd.spheres = np.concatenate([sd.spheres, hrt.spheres_array(tiny)])
    sd.name = "shell 70x45 with tiny spheres"
    assert len(_leaves(sd)["leaves"]) - 1 <= NODE_CAP
    _vs_oracle(sd, *_oracle(sd), twin=True)


# ---- the table's ends
def test_tree_of_exactly_the_node_cap():
    sd = _full_table("70x45")
    B = _leaves(sd)
    assert len(B["leaves"]) - 1 == NODE_CAP and B["depth"] == DEPTH_CAP
    _vs_oracle(sd, *_lds_oracle("full_table", "70x45"), twin=True)


def test_one_node_more_keeps_the_global_nodes():
    sd = _full_table("64x40")
    more = [Sphere.new_lambertian(Vec3(13.5 + 0.08 * j, 0.2, 0.05 * j), 0.2, Vec3(0.5, 0.5, 0.5)) for j in range(4)]
    sd.spheres = np.concatenate([sd.spheres, hrt.spheres_array(more)])
    sd.name = "full_table and one cluster"
    assert len(_leaves(sd)["leaves"]) - 1 == NODE_CAP + 1
    _vs_oracle(sd, *_oracle(sd), kernel=BEYOND)


@pytest.mark.parametrize("tree", ["one_leaf", "empty"])
def test_trees_without_a_node(tree):
    balls = []
    if tree == "one_leaf":
        balls = [_ball(k, (-0.8 + 0.8 * k, 0.0, -4.0), 0.5) for k in range(3)]
        balls.append(Sphere.new_lambertian(Vec3(0.0, -1000.5, -4.0), 1000.0, Vec3(0.5, 0.5, 0.5)))
    cam = Camera.new(Vec3(0.0, 0.5, 0.0), Vec3(0.0, 0.0, -4.0), 4.0, 0.0, 0.9)
    sd = scenes.SceneDef(tree, hrt.RT_MODE_SPHERE, 70, 45, cam, hrt.spheres_array(balls), frames=FRAMES, bounces=50,
                         min_sphere_slots=0)
    B = _leaves(sd)
    assert B["leaves"] == ([(0, 3)] if tree == "one_leaf" else [(0, 0)]) and B["depth"] == 0, B
    _vs_oracle(sd, *_oracle(sd), twin=True)


# ---- the workgroup
# jobs = tiles x frames with one-frame jobs and no tail split: (width, height, frames); a workgroup has 8 waves
SHAPES = {1: (6, 5, 1), 7: (56, 8, 1), 8: (32, 13, 1), 9: (72, 8, 1)}


@pytest.mark.parametrize("jobs", sorted(SHAPES))
def test_fewer_jobs_than_a_workgroup_has_waves(jobs):
    w, h, frames = SHAPES[jobs]
    sd = scenes.config_c3(w, h, frames)
    sd.name = f"C3 {w}x{h}x{frames}: {jobs} jobs"
    assert ((w + 7) // 8) * ((h + 7) // 8) * frames == jobs and min(SHAPES) < WG_WAVES < max(SHAPES)
    img, st, _ = _vs_oracle(sd, *_oracle(sd), twin=True, job_frames=1, tail_split=1)
    assert st.trace_launches == 1


def test_rank_3_of_8_row_share():
    sd = scenes.config_c3(64, 72, 9)
    p = rank_params(3, 8, 8)
    rows = owned_rows(p["row0"], p["row_step"], sd.height, 8)
    ref, q = _oracle(sd, rows=(p["row0"], p["row_step"], len(rows), 8))
    _vs_oracle(sd, ref, q, twin=True, **p)


@pytest.fixture(scope="module")
def cover33():
    sd = scenes.config_c3(70, 45, 33)
    return sd, _oracle(sd)


def test_two_launches_folded_by_the_next(cover33):
    sd, (ref, q) = cover33
    # 41,472 B a frame: 25 fit 1 MiB, so launches of whole jobs start at frames 0 and 24
    img, st, _ = _vs_oracle(sd, ref, q, twin=True, fold=hrt.RT_FOLD_NEXT, job_frames=8, queue_budget_mb=1)
    assert st.trace_launches == 2 and st.launch_frames == 24 and st.fold_ring == 2, (st.trace_launches, st.launch_frames)


@pytest.mark.parametrize("count_tests", [0, 1], ids=["headline", "twin"])
def test_learning_launch_then_ordered_draw(cover33, count_tests):
    sd, (ref, q) = cover33
    kernel = TWIN if count_tests else KERNEL
    r = _renderer(sd, count_tests, job_frames=8, cost_order=2)
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    assert st.ordered_launches == 0 and st.kernel.decode() == kernel, st.kernel
    _same(r.read_image(), ref, "learning draw")
    assert st.queries == q
    r.reset_frame_count()
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    assert st.ordered_launches == st.trace_launches == 1 and st.kernel.decode() == kernel, st.kernel
    _same(r.read_image(), ref, "ordered draw")
    assert st.queries == q


@pytest.mark.parametrize("tail", [0, 2, 3])
def test_tail_split(tail):
    sd = scenes.config_c3(72, 40, 16)
    _vs_oracle(sd, *_oracle(sd), twin=True, tail_split=tail, job_frames=8)


# ---- the observable
@pytest.mark.parametrize("size", list(SIZES))
def test_listed_tiles_are_resolved_when_their_blocks_are_made(size):
    sd = scenes.config_c3(*SIZES[size], 5)
    ref, q = _oracle(sd)
    for mode in (2, 1):
        img, st, r = _vs_oracle(sd, ref, q, lists=mode)
        listed = int((r.tile_lists()[:, 0] != WALK).sum()) if mode == 2 else 0
        assert mode == 1 or listed > 0
        assert r.tile_lists_resolved() == (listed * sd.frames if mode == 2 else 0), (mode, r.tile_lists_resolved(), listed)
