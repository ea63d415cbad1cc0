"""The 16-bit walk stack of k_trace_split<LNODES> (rt_kernels.hip bvh_walk_noovf, the stack entry type SW; renderer.cpp's gate).

With the tree's nodes in LDS a child word is a node index below 192 or LEAF | first << 4 | count with first below 2048:
15 bits and the leaf bit, so a stack entry is 16 bits — the LDS copy of the nodes holds the words sign-extended from bit
15, the push stores the low half and the pop's sign-extending read gives the word back. Two scenes:

* the nested clusters of test_gpu_pop_forms.py: a full-depth tree, pops with all 8 entries in use;
* a 24 x 24 grid of equal small spheres over a ground sphere: 576 leaf spheres in 191 nodes of depth 8, the largest
  square grid the LDS-nodes gate admits (25 x 25 builds 206 nodes; the gate's 192 nodes hold 772 leaf spheres at most,
  and this builder's leaves average three). Its leaf words reach first = 572, bits 12 and 13 of the word, so an entry
  cut to 8 or to 12 bits returns wrong spheres.

Every draw — suspend_below 1 (never suspends) and 64 (after nearly every pop), descent hold 0 and 12, counted and not —
must give the oracle's image and query count, and the counting draws the box / sphere test counts of the hold-0 draw.
The 25 x 25 grid, beyond the gate, must run the kernel without LDS nodes (32-bit entries) and match the oracle too.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu

W, H, FRAMES = 44, 28, 3  # ragged 8x8 tiles
GRID_N = 24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _grid(n):
    """n x n spheres of radius 0.1, 0.25 apart (coordinates exact in binary), every material, over a ground sphere."""
    o = []
    for i in range(n):
        for j in range(n):
            c = Vec3(0.25 * (i - n // 2), 0.1, -2.0 - 0.25 * j)
            k = (i + 2 * j) % 3
            o.append(Sphere.new_lambertian(c, 0.1, Vec3(0.8, 0.2 + 0.025 * (j % 24), 0.2)) if k == 0 else
                     Sphere.new_metal(c, 0.1, Vec3(0.7, 0.7, 0.4 + 0.02 * (i % 24)), 0.1) if k == 1 else
                     Sphere.new_dielectric(c, 0.1, 1.5))
    o.append(Sphere.new_lambertian(Vec3(0.0, -1000.0, -5.0), 1000.0, Vec3(0.5, 0.5, 0.5)))
    cam = Camera.new(Vec3(0.5, 2.5, 2.0), Vec3(0.0, 0.0, -5.0), 7.0, 0.02, 0.9)
    return scenes.SceneDef(f"grid {n}", hrt.RT_MODE_SPHERE, W, H, cam, hrt.spheres_array(o), frames=FRAMES, bounces=50,
                           min_sphere_slots=0)


def _nested():
    sd = _random_scene("nested_clusters", 7)
    sd.width, sd.height, sd.frames = W, H, FRAMES
    return sd


SCENES = {"nested_clusters": _nested, "grid": lambda: _grid(GRID_N), "grid_beyond_gate": lambda: _grid(GRID_N + 1)}


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name, make in SCENES.items():
        sd = make()
        ref, q = scenes.oracle_render(sd)
        ref.setflags(write=False)
        out[name] = (sd, ref, q)
    return out


def _draw(sd, suspend_below, hold, count_tests):
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, suspend_below=suspend_below, steal=1, count_tests=count_tests)
    r.set_descent_hold(hold)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


@pytest.mark.parametrize("count_tests", [1, 0])
@pytest.mark.parametrize("suspend_below", [1, 64])
@pytest.mark.parametrize("scene", ["nested_clusters", "grid"])
def test_full_stack_and_wide_leaf_words(refs, scene, suspend_below, count_tests):
    sd, ref, q = refs[scene]
    if scene == "grid":
        assert GRID_N * GRID_N > 512  # leaf words with first >= 512: bit 13
    base = None
    for hold in (0, 12):
        img, st = _draw(sd, suspend_below, hold, count_tests)
        what = f"{scene} suspend_below {suspend_below} hold {hold} count_tests {count_tests}"
        assert st.kernel.decode().startswith("k_trace_split<true, "), (what, st.kernel)
        np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
        assert st.queries == q, what
        if count_tests:
            base = base or (st.box_tests, st.sphere_tests)
            assert base[0] > 0 and (st.box_tests, st.sphere_tests) == base, what


def test_tree_beyond_the_gate_keeps_32_bit_entries(refs):
    sd, ref, q = refs["grid_beyond_gate"]
    img, st = _draw(sd, 24, 12, 0)
    assert st.kernel.decode().startswith("k_trace_split<false, "), st.kernel
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert st.queries == q
