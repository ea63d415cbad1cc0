"""The large list of k_trace_split<LNODES> in LDS (rt_device.hpp LLARGE_CAP; rt_kernels.hip bvh_begin<.., LLDS>).

Spheres far larger than the scene's median radius are not put in the culling BVH: every query tests them first, from a
short list. The kernel that keeps the tree's nodes in LDS keeps that list's spheres there too (copied once per
workgroup) when it has at most LLARGE_CAP = 14 entries — what fits beside the nodes, the stacks and the frame block with
7 workgroups per CU; a longer list runs the kernel without LDS nodes, which reads the list from memory as before. Lists of
0, 1, 14, 15, 16 and 17 spheres cover the empty copy, a single entry, the full copy and the gate; the kernel is asserted
by name, and image and query count equal the CPU oracle's bit for bit.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3

pytestmark = pytest.mark.gpu

W, H, FRAMES = 40, 24, 2
LLARGE_CAP = 14  # rt_device.hpp


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _small():
    """48 spheres of radius 0.2 (the median: anything above 6.4 goes to the large list), every material."""
    o = []
    for i in range(8):
        for j in range(6):
            c = Vec3(-2.8 + 0.8 * i, 0.2, -2.0 - 0.9 * j)
            k = (i + 2 * j) % 3
            o.append(Sphere.new_lambertian(c, 0.2, Vec3(0.8, 0.3 + 0.1 * j, 0.2)) if k == 0 else
                     Sphere.new_metal(c, 0.2, Vec3(0.7, 0.7, 0.5 + 0.05 * i), 0.1) if k == 1 else
                     Sphere.new_dielectric(c, 0.2, 1.5))
    return o


def _big(k):
    """The k-th large sphere: radius 20, the tops side by side under the small ones (a bumpy ground), material by k."""
    c = Vec3(-6.0 + 3.0 * (k % 5), -20.0 - 0.01 * k, -1.0 - 3.0 * (k // 5))
    if k % 3 == 0:
        return Sphere.new_lambertian(c, 20.0, Vec3(0.5, 0.5, 0.2 + 0.04 * k))
    if k % 3 == 1:
        return Sphere.new_metal(c, 20.0, Vec3(0.6, 0.5 + 0.02 * k, 0.6), 0.05)
    return Sphere.new_dielectric(c, 20.0, 1.5)


def _scene(name, objs):
    cam = Camera.new(Vec3(0.0, 2.5, 3.0), Vec3(0.0, 0.0, -4.0), 7.0, 0.02, 0.9)
    return scenes.SceneDef(name, hrt.RT_MODE_SPHERE, W, H, cam, hrt.spheres_array(objs), frames=FRAMES, bounces=50,
                           min_sphere_slots=0)


def _draw(sd, variant=4, **params):
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=variant, **params)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


@pytest.mark.parametrize("nlarge", [0, 1, 14, 15, 16, 17])
def test_large_list_lengths_vs_oracle(nlarge):
    # the large spheres are spread through the slots, so their slots are not the list's indices
    small = _small()
    objs = list(small)
    for k in range(nlarge):
        objs.insert(min(len(objs), 3 * k + 1), _big(k))
    sd = _scene(f"nlarge {nlarge}", objs)
    ref, q = scenes.oracle_render(sd)
    base = None
    for count_tests in (1, 0):
        img, st = _draw(sd, count_tests=count_tests)
        what = f"nlarge {nlarge} count_tests {count_tests}"
        want = "k_trace_split<true, " if nlarge <= LLARGE_CAP else "k_trace_split<false, "
        assert st.kernel.decode().startswith(want), (what, st.kernel)
        np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
        assert st.queries == q, what
        if count_tests:
            base = st.sphere_tests
            assert base >= nlarge * q  # every covered query tests the whole list
    # the list is what the builder says: the same scene's exact scan of every slot tests more
    img1, st1 = _draw(sd, count_tests=1, variant=1)
    np.testing.assert_array_equal(img1.view(np.uint32), ref.view(np.uint32))
    assert st1.queries == q and st1.sphere_tests > base


def test_identical_large_spheres_take_the_lower_slot():
    """Two large spheres with the same centre and radius and different materials, beside a third: every t on them ties,
    and the begin phase's tie-break must keep the lower slot — in both slot orders."""
    c = Vec3(0.0, -20.0, -4.0)
    twins = [Sphere.new_metal(c, 20.0, Vec3(0.9, 0.6, 0.2), 0.0), Sphere.new_lambertian(c, 20.0, Vec3(0.2, 0.3, 0.9))]
    other = Sphere.new_dielectric(Vec3(9.0, -19.0, -9.0), 20.0, 1.5)
    imgs = []
    for order in (0, 1):
        a, b = twins[order], twins[1 - order]
        objs = _small()
        objs.insert(5, a)
        objs.insert(20, other)
        objs.append(b)
        sd = _scene(f"twins {order}", objs)
        ref, q = scenes.oracle_render(sd)
        img, st = _draw(sd)
        assert st.kernel.decode().startswith("k_trace_split<true, "), st.kernel
        np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=f"order {order}")
        assert st.queries == q
        imgs.append(img)
    assert not np.array_equal(imgs[0], imgs[1])  # the two materials differ, so the order of the twins shows
