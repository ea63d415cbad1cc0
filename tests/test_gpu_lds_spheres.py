"""k_trace_split<true, false, false, false> at the bounds of its tree gate and with workgroups short of jobs (DESIGN.md §4
Round 11).

Round 11 built this kernel in 1024- and 512-lane workgroups with the tree's leaf spheres copied into LDS, measured both
against the parent and kept neither (the gain stayed under the project's bar; profiles/r11/). These are the tests that
change was held to; they hold for the kernel as it is — the round's kept change, the leaf's two pairs written out in place
of the pair loop, runs in every draw below — and for any later form of it. The counted kernel and the uncounted
one are separate instantiations with separate register budgets, so every scene is drawn by both, each asserted by name, and
compared with the oracle bit for bit and in its query count: the same spheres, the same arithmetic, the same order.

The scenes are test_gpu_leaf_loads' (leaves of every size with a candidate alone in an odd leaf's last position, the
last leaf odd under rays through the world origin, with and without a zero slot behind it, exact ties within and across
leaves, the coincident spheres, the C3 crop), the fullest trees the node gate admits (below), and the two-cover-scene tree
of test_gpu_kernels, which is past the gate and must run the kernel without LDS nodes. The workgroup-shape cases give a
launch 1, 3, 4, 5, 15, 16 and 17 jobs, one wave each: a lone workgroup most of whose waves never get a job, one with a
single such wave, full workgroups, and full ones beside a workgroup with a single busy wave (4 waves per workgroup today;
16 in the form Round 11 measured).

"cover_dense": a seeded search on the host (rtiow_spheres(42) plus the first k small spheres of rtiow_spheres(seed), seeds
1..12, k in steps of 4, kept while the tree has <= 192 nodes and depth <= 8) reaches 527 leaf spheres with seed 2, k = 44;
the depth bound, not the node bound, stops it. "full_table": 193 clusters of four spheres on a grid, a tree of exactly 192
nodes and depth 8 with 772 leaf spheres, the most a tree of 192 nodes can hold. test_fullest_trees_pass_the_gate checks
both structures through rt_testing_sphere_bvh_leaves, without a GPU.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Sphere, Vec3
from test_gpu_kernels import _deep_spheres
from test_gpu_leaf_loads import COUNTED, SCENES as LEAF_SCENES, SIZES, UNCOUNTED, _bvh
from test_gpu_leaf_loads import _oracle as _leaf_oracle

FRAMES = 3
SUSPENDS = (1, 24, 64)
HOLDS = (0, 12)
NODE_CAP, DEPTH_CAP, LARGE_CAP, MAX_LEAF = 192, 8, 14, 4  # (rt_device.hpp LNODE_CAP, LNODE_DEPTH, LLARGE_CAP, BVH_MAX_LEAF)
MOST = (NODE_CAP + 1) * MAX_LEAF  # (the most leaf spheres of a tree of NODE_CAP nodes: two children per node)
DEEP_COUNTED = "k_trace_split<false, false, true, false>"
DEEP_UNCOUNTED = "k_trace_split<false, false, false, false>"


def _cover(name, size, spheres):
    sd = scenes.config_c3(*SIZES[size], FRAMES)
    sd.name, sd.spheres, sd.bounces = f"{name} {size}", spheres, 8
    return sd


def _cover_dense(size):
    return _cover("cover_dense", size, np.concatenate([scenes.rtiow_spheres(42), scenes.rtiow_spheres(2)[1:-3][:44]]))


def _full_table(size):
    """The cover scene's ground and camera over a 16 x 12 grid of clusters of four spheres and one cluster beside it."""
    balls = [Sphere.new_lambertian(Vec3(0.0, -1000.0, 0.0), 1000.0, Vec3(0.5, 0.5, 0.5))]
    cells = [((a - 8) * 1.5, (b - 6) * 1.5) for a in range(16) for b in range(12)] + [(12.0, 0.0)]
    for n, (x, z) in enumerate(cells):
        for j in range(4):
            c = Vec3(x + 0.08 * j, 0.2, z + 0.05 * j)
            if (n + j) % 5 == 0:
                balls.append(Sphere.new_metal(c, 0.2, Vec3(0.8, 0.7, 0.6), 0.1))
            else:
                balls.append(Sphere.new_lambertian(c, 0.2, Vec3(0.2 + 0.15 * j, 0.5, 0.8 - 0.15 * j)))
    return _cover("full_table", size, hrt.spheres_array(balls))


def _deep(size):
    return _cover("deep", size, _deep_spheres())


LEAF = ("c3", "clusters", "last_leaf", "last_leaf_padded", "tie_same_leaf", "tie_two_leaves", "tie_two_leaves_swapped",
        "coincident")
OWN = {"cover_dense": _cover_dense, "full_table": _full_table, "deep": _deep}
CASES = [(s, z) for s in LEAF + tuple(OWN) for z in SIZES]
_ORACLE = {}


def _scene(scene, size):
    return OWN[scene](size) if scene in OWN else LEAF_SCENES[scene](size)


def _oracle_of(key, make):
    if key not in _ORACLE:  # once per scene, shared and read-only
        img, q = scenes.oracle_render(make())
        img.setflags(write=False)
        _ORACLE[key] = (img, q)
    return _ORACLE[key]


def _oracle(scene, size):
    if scene in OWN:
        return _oracle_of((scene, size), lambda: OWN[scene](size))
    return _leaf_oracle(scene, size)  # (test_gpu_leaf_loads' cache: one oracle run for both files)


def _gate(B):
    return len(B["leaves"]) - 1 <= NODE_CAP and B["depth"] <= DEPTH_CAP and len(B["large"]) <= LARGE_CAP


def test_fullest_trees_pass_the_gate():
    c3 = _bvh(scenes.config_c3(64, 40, 1))
    dense, full, deep = _bvh(_cover_dense("64x40")), _bvh(_full_table("64x40")), _bvh(_deep("64x40"))
    assert _gate(c3) and _gate(dense) and _gate(full) and not _gate(deep)
    assert len(c3["slots"]) < len(dense["slots"]) == 527 <= MOST
    assert dense["depth"] == DEPTH_CAP and {c for _, c in dense["leaves"]} == {2, 3, 4}
    # 193 leaves of four under 192 nodes (one leaf more would be a 193rd node)
    assert len(full["leaves"]) == NODE_CAP + 1 and {c for _, c in full["leaves"]} == {MAX_LEAF}
    assert len(full["slots"]) == MOST and full["depth"] == DEPTH_CAP and len(full["large"]) == 1
    assert len(deep["leaves"]) - 1 > NODE_CAP
    for B in (c3, dense, full):
        pos = 0
        for first, count in B["leaves"]:
            assert first == pos and 1 <= count <= MAX_LEAF
            pos += count
        assert pos == len(B["slots"])


def _draw(sd, hold=12, **params):
    r = scenes.make_renderer(sd)  # (count_tests = 1 unless params says otherwise)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, steal=1, **params)
    r.set_descent_hold(hold)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


@pytest.fixture(scope="module")
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


@pytest.mark.gpu
@pytest.mark.parametrize("scene,size", CASES)
def test_lds_spheres_draw_the_counted_kernels_and_the_oracles_bits(_need_gpu, scene, size):
    sd = _scene(scene, size)
    ref, q = _oracle(scene, size)
    counted, uncounted = (DEEP_COUNTED, DEEP_UNCOUNTED) if scene == "deep" else (COUNTED, UNCOUNTED)
    img_c, st_c = _draw(sd)
    assert st_c.kernel.decode() == counted, st_c.kernel
    img_u, st_u = _draw(sd, count_tests=0)
    assert st_u.kernel.decode() == uncounted, st_u.kernel
    np.testing.assert_array_equal(img_c.view(np.uint32), ref.view(np.uint32), err_msg=f"{sd.name} counted")
    np.testing.assert_array_equal(img_u.view(np.uint32), ref.view(np.uint32), err_msg=f"{sd.name} uncounted")
    np.testing.assert_array_equal(img_u.view(np.uint32), img_c.view(np.uint32), err_msg=f"{sd.name} uncounted / counted")
    assert st_c.queries == q and st_u.queries == q, (sd.name, st_c.queries, st_u.queries, q)
    assert st_c.sphere_tests > 0


# jobs = tiles x frames with one-frame jobs and no tail split: (width, height, frames)
SHAPES = {1: (6, 5, 1), 3: (20, 7, 1), 4: (13, 16, 1), 5: (40, 8, 1), 15: (40, 24, 1), 16: (32, 13, 2), 17: (133, 7, 1)}


def _shape_scene(jobs):
    w, h, frames = SHAPES[jobs]
    sd = scenes.config_c3(w, h, frames)
    sd.name = f"C3 {w}x{h}x{frames}: {jobs} jobs"
    assert ((w + 7) // 8) * ((h + 7) // 8) * frames == jobs
    return sd


@pytest.mark.gpu
@pytest.mark.parametrize("jobs", sorted(SHAPES))
def test_workgroups_with_idle_waves_end_and_draw_the_oracle(_need_gpu, jobs):
    sd = _shape_scene(jobs)
    ref, q = _oracle_of(("shape", jobs), lambda: _shape_scene(jobs))
    for sb in SUSPENDS:
        for hold in HOLDS:
            img, st = _draw(sd, hold, suspend_below=sb, count_tests=0, job_frames=1, tail_split=1)
            what = f"{sd.name} suspend_below {sb} hold {hold}"
            assert st.kernel.decode() == UNCOUNTED, (what, st.kernel)
            assert st.trace_launches == 1, what
            np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
            assert st.queries == q, what


@pytest.mark.gpu
def test_fold_by_next_launch_in_the_uncounted_kernel(_need_gpu):
    """Three trace launches (a 1 MiB budget: 40 frames of 96 x 64 in 14 + 14 + 12): the second and third fold the launch
    before them (fold_prev_tiles: wave 0 of the workgroups it picks). Against the fold after every launch, and the oracle."""
    sd = scenes.config_c3(96, 64, 40)
    out = {}
    for fold in (hrt.RT_FOLD_BUFFER, hrt.RT_FOLD_NEXT):
        out[fold] = _draw(sd, count_tests=0, queue_budget_mb=1, job_frames=4, fold=fold)
        st = out[fold][1]
        assert st.kernel.decode() == UNCOUNTED and st.trace_launches == 3, (st.kernel, st.trace_launches)
    assert out[hrt.RT_FOLD_BUFFER][1].fold_ring == 0 and out[hrt.RT_FOLD_NEXT][1].fold_ring == 2
    assert out[hrt.RT_FOLD_NEXT][1].launches == 4 and out[hrt.RT_FOLD_BUFFER][1].launches == 6
    a, b = out[hrt.RT_FOLD_BUFFER][0], out[hrt.RT_FOLD_NEXT][0]
    np.testing.assert_array_equal(b.view(np.uint32), a.view(np.uint32))
    assert out[hrt.RT_FOLD_NEXT][1].queries == out[hrt.RT_FOLD_BUFFER][1].queries
    ref, q = _oracle_of("fold", lambda: scenes.config_c3(96, 64, 40))
    np.testing.assert_array_equal(b.view(np.uint32), ref.view(np.uint32))
    assert out[hrt.RT_FOLD_NEXT][1].queries == q
