"""Both fold modes of the sample queue through every kernel instantiation a draw can select (rt_kernels.hip fold_ring).

A sample's colour goes to the sample buffer (folded by k_accumulate, or by the next launch: rt_params.fold 1 / 3) or to
the fold ring (fold 2), and the sample-queue kernels are compiled once per mode: k_trace_split<LNODES, STEAL, COUNT, PACKET>
with and without LDS nodes, counting and stealing (sample buffer only), k_trace and k_trace_split_tris. rt_stats.kernel
names the four-parameter form in both modes and rt_stats.fold_ring the mode. Every draw must equal the CPU oracle bit
for bit, with its query count, and the box / sphere test counts must not depend on the fold.

Draws: the C3 scene cropped to 64 x 40 and to a ragged 70 x 45, 37 frames (one whole 32-frame job plus a short one) and
64 frames (whole jobs, the tail split on); the ring also with two slots (rt_testing_set_faults: jobs wait for a slot,
which runs slot_poll, job_account's completion and fold_session's slot returns); a 15-sphere large list (no LDS nodes);
the stealing kernel; a 3-sphere linear scan (k_trace) and the cube mesh in the mixed program (k_trace_split_tris).
"""
import dataclasses
import re

import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from test_gpu_large_list_lds import _big, _scene, _small

pytestmark = pytest.mark.gpu

FOLDS = {"buffer": (hrt.RT_FOLD_BUFFER, 0), "next": (hrt.RT_FOLD_NEXT, 2), "ring": (hrt.RT_FOLD_RING, 1)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


_REFS = {}


def _oracle(key, make):
    """(scene, oracle image, oracle queries) of a case, rendered once for the module and left unchanged."""
    if key not in _REFS:
        sd = make()
        ref, q = scenes.oracle_render(sd)
        ref.setflags(write=False)
        _REFS[key] = (sd, ref, q)
    return _REFS[key]


def _draw(sd, fold, ring_slots_max=0, **params):
    r = scenes.make_renderer(sd)
    if ring_slots_max:
        r.set_faults(ring_slots_max=ring_slots_max)
    if fold == "next":  # a budget of about 30 frames: two or more launches, each folded by the next
        params.setdefault("queue_budget_mb", 1)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, fold=FOLDS[fold][0], **params)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


def _check(img, st, ref, q, fold, kernel, what):
    assert st.fold_ring == FOLDS[fold][1], (what, st.fold_ring)
    assert st.kernel.decode() == kernel, (what, st.kernel)
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
    assert st.queries == q, what


@pytest.mark.parametrize("frames", [37, 64])
@pytest.mark.parametrize("size", [(64, 40), (70, 45)])
def test_split_kernel_folds_vs_oracle(size, frames):
    sd, ref, q = _oracle(("c3", size, frames), lambda: scenes.config_c3(size[0], size[1], frames))
    for count_tests in (1, 0):
        kernel = f"k_trace_split<true, false, {'true' if count_tests else 'false'}, false>"
        counts, ring_bytes = {}, {}
        for fold, slots in (("buffer", 0), ("next", 0), ("ring", 0), ("ring", 2)):
            what = f"{size} x {frames} count_tests {count_tests} fold {fold} slots {slots}"
            img, st = _draw(sd, fold, ring_slots_max=slots, variant=4, steal=1, count_tests=count_tests)
            _check(img, st, ref, q, fold, kernel, what)
            if fold == "next":
                assert st.trace_launches >= 2, (what, st.trace_launches)
            if fold == "ring":
                ring_bytes[slots] = st.fold_bytes
            counts[(fold, slots)] = (st.box_tests, st.sphere_tests)
        assert ring_bytes[2] < ring_bytes[0], ring_bytes  # (the two slots took: a smaller ring)
        if count_tests:
            assert counts["buffer", 0][0] > 0 and len(set(counts.values())) == 1, counts


def _large15():
    objs = list(_small())
    for k in range(15):
        objs.insert(min(len(objs), 3 * k + 1), _big(k))
    # (100 frames of 40 x 24: more colours than a 1 MiB budget holds, so fold 3 has two launches)
    return dataclasses.replace(_scene("nlarge 15", objs), frames=100)


@pytest.mark.parametrize("count_tests", [1, 0])
def test_split_kernel_without_lds_nodes(count_tests):
    """15 large spheres: one more than the LDS list holds, so the kernel reads nodes and list from memory."""
    sd, ref, q = _oracle("large15", _large15)
    kernel = f"k_trace_split<false, false, {'true' if count_tests else 'false'}, false>"
    counts = set()
    for fold, slots in (("buffer", 0), ("next", 0), ("ring", 0), ("ring", 2)):
        img, st = _draw(sd, fold, ring_slots_max=slots, variant=4, steal=1, count_tests=count_tests)
        _check(img, st, ref, q, fold, kernel, f"count_tests {count_tests} fold {fold} slots {slots}")
        counts.add((st.box_tests, st.sphere_tests))
    if count_tests:
        assert len(counts) == 1 and min(counts)[0] > 0, counts


@pytest.mark.parametrize("count_tests", [1, 0])
def test_stealing_kernel_with_the_sample_buffer(count_tests):
    sd, ref, q = _oracle(("c3", (70, 45), 37), lambda: scenes.config_c3(70, 45, 37))
    kernel = f"k_trace_split<true, true, {'true' if count_tests else 'false'}, false>"
    for fold in ("buffer", "next"):
        img, st = _draw(sd, fold, variant=4, steal=2, count_tests=count_tests)
        _check(img, st, ref, q, fold, kernel, f"steal count_tests {count_tests} fold {fold}")


def _three_spheres():
    objs = [Sphere.new_lambertian(Vec3(0.0, -100.5, -1.0), 100.0, Vec3(0.8, 0.8, 0.0)),
            Sphere.new_metal(Vec3(-0.6, 0.0, -1.2), 0.5, Vec3(0.8, 0.6, 0.2), 0.1),
            Sphere.new_dielectric(Vec3(0.6, 0.0, -1.0), 0.5, 1.5)]
    cam = Camera.new(Vec3(0.0, 0.5, 2.0), Vec3(0.0, 0.0, -1.0), 3.0, 0.02, 0.9)
    return scenes.SceneDef("three spheres", hrt.RT_MODE_SPHERE, 44, 28, cam, hrt.spheres_array(objs), frames=5, bounces=50,
                           min_sphere_slots=0)


def _cube_mixed():
    from hrt import Material, Mesh, Tree, read_asset
    t = Tree.from_mesh(Mesh.load_obj(read_asset("cube.obj"), Material.new_lambertian(Vec3(0.3, 0.4, 0.6))))
    t.build()
    ground = hrt.spheres_array([Sphere.new_lambertian(Vec3(0.0, -101.0, -4.5), 100.0, Vec3(0.5, 0.5, 0.6)),
                                Sphere.new_metal(Vec3(1.5, 0.0, -4.0), 0.6, Vec3(0.8, 0.8, 0.8), 0.0)])
    cam = Camera.new(Vec3(0.0, 2.2, 4.5), Vec3(0.0, 0.0, -4.5), 5.6, 0.0, 0.9)
    return scenes.SceneDef("cube mixed", hrt.RT_MODE_MIXED, 44, 28, cam, ground, bvh=t.view(), frames=5, bounces=50,
                           min_sphere_slots=0)


@pytest.mark.parametrize("case", ["k_trace", "k_trace_split_tris"])
def test_other_sample_queue_kernels_in_both_modes(case):
    """k_trace (the linear sphere scan) and k_trace_split_tris (the mixed program's heap walk): 44 x 28 x 5 frames."""
    sd, ref, q = _oracle(case, _three_spheres if case == "k_trace" else _cube_mixed)
    names = set()
    for fold, slots in (("buffer", 0), ("ring", 0), ("ring", 2)):
        img, st = _draw(sd, fold, ring_slots_max=slots, variant=1, steal=1)
        name = st.kernel.decode()
        _check(img, st, ref, q, fold, name, f"{case} fold {fold} slots {slots}")
        names.add(name)
    (name,) = names  # one name in both modes
    if case == "k_trace":
        assert name == "k_trace<0, 1, false>", name
    else:
        assert re.fullmatch(r"k_trace_split_tris<2, 1, \d, false>", name), name
