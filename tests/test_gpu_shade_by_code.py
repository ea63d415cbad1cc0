"""k_trace_split shades its winner by BVH code (KParams::code_aux: the sphere records in code order, no slot lookup).

The walk keeps its running winner as a code: the sphere's position in BVH order, or nleaf + its large-list index. The
shade phase reads the winner's centre, radius and material from a table in that order, and the dielectric arm's
constants from the same table; the rare full scan yields a slot, which indexes the slot-order records behind the
code-order ones. Ties are still broken by slot ("the lowest slot among equal t"). Every case below makes code order and
slot order disagree in its own way, and compares image and query count with the CPU oracle bit for bit, through the
counted and the uncounted (timed) instantiation, on whole and on ragged 8x8 tiles.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3

pytestmark = pytest.mark.gpu

SHAPES = ((64, 40), (70, 45))
FRAMES = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _material(k, c, rad):
    k %= 3
    if k == 0:
        return Sphere.new_lambertian(c, rad, Vec3(0.9, 0.3, 0.2))
    if k == 1:
        return Sphere.new_metal(c, rad, Vec3(0.3, 0.8, 0.5), 0.1)
    return Sphere.new_dielectric(c, rad, 1.5)


def _coincident_alternating(w, h):
    """64 coincident spheres, Lambert / metal / dielectric by slot: every t ties, slot 0's material must shade."""
    sph = hrt.spheres_array([_material(k, Vec3(0.0, 0.0, -3.0), 1.0) for k in range(64)])
    cam = Camera.new(Vec3(0.0, 0.5, 1.0), Vec3(0.0, 0.0, -3.0), 4.0, 0.0, 0.9)
    return scenes.SceneDef("coincident alternating", hrt.RT_MODE_SPHERE, w, h, cam, sph, frames=FRAMES, bounces=8,
                           min_sphere_slots=0)


def _reversed_row(w, h):
    """A row of spheres whose slots run against the builder's order: the builder sorts and bins by centre, ascending,
    and slot k sits at descending x (and, in the second row, descending z), so code c is roughly slot n - 1 - c. Every
    third sphere is glass: a wrong record shows as a wrong colour, a wrong normal or a wrong refraction."""
    o = []
    for k in range(48):
        o.append(_material(k, Vec3(4.7 - 0.2 * k, 0.0, -6.0), 0.1 + 0.002 * k))
    for k in range(48):
        o.append(_material(k + 1, Vec3(0.0, 0.35, -2.0 - 0.2 * (47 - k)), 0.1))
    o.append(Sphere.new_lambertian(Vec3(0.0, -1000.2, -6.0), 1000.0, Vec3(0.5, 0.5, 0.5)))
    cam = Camera.new(Vec3(0.0, 1.5, 2.0), Vec3(0.0, 0.0, -6.0), 8.0, 0.02, 0.9)
    return scenes.SceneDef("reversed row", hrt.RT_MODE_SPHERE, w, h, cam, hrt.spheres_array(o), frames=FRAMES,
                           bounces=50, min_sphere_slots=0)


def _cover(w, h):
    """The cover scene: the ground wins from the large list beside the small spheres' leaf winners."""
    return scenes.config_c3(w, h, FRAMES)


def _zero_radius_padding(w, h):
    """25 spheres in a 100-slot buffer (min_sphere_slots: zero-radius padding slots at the origin)."""
    sd = scenes.golden_scene("complex_scene", w, h)
    sd.frames = FRAMES
    return sd


def _full_scan_hits(w, h):
    """Focal length 2^60: the sphere program does not normalise d, so every primary ray's 2a lies beyond 2^100 (bvh_begin's
    uncovered rule) and its query is the exact full scan, whose winner is a slot; the bounces after it walk the tree."""
    sd = scenes.config_c3(w, h, FRAMES)
    sd.camera = Camera.new(Vec3(13.0, 2.0, 3.0), Vec3(0.0, 0.0, 0.0), 2.0 ** 60, 0.0, hrt.f32(20.0) * hrt.PI / hrt.f32(180.0))
    return sd


def _non_finite_origin(w, h):
    """An eye at x = +inf: every primary ray has a non-finite origin (the full scan, which accepts nothing)."""
    sd = scenes.config_c3(w, h, FRAMES)
    cam = sd.camera.copy()
    eye = cam["eye"].copy()
    eye[0] = np.inf
    cam["eye"] = eye
    cam["params"] = (cam["params"][0], 0.0, cam["params"][2], cam["params"][3])  # (no lens offset: inf - inf)
    sd.camera = cam
    return sd


CASES = {
    "coincident_alternating": _coincident_alternating,
    "reversed_row": _reversed_row,
    "large_list_winner": _cover,
    "zero_radius_padding": _zero_radius_padding,
    "full_scan_hits": _full_scan_hits,
    "non_finite_origin": _non_finite_origin,
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", sorted(CASES))
def test_shade_by_code_vs_oracle(case, shape):
    sd = CASES[case](*shape)
    ref, q = scenes.oracle_render(sd)
    for count_tests in (1, 0):
        r = scenes.make_renderer(sd)
        r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, count_tests=count_tests)
        r.draw_frames(sd.frames, 1000, 10)
        img, st = r.read_image(), r.stats()
        what = f"{case} {shape} count_tests {count_tests}"
        k = st.kernel.decode()
        assert k.startswith("k_trace_split<") and k.endswith(f"{'true' if count_tests else 'false'}, false>"), (what, k)
        np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
        assert st.queries == q, what


def test_full_scan_case_takes_the_fallback():
    """The forcing case does what it says: more exact sphere tests than the same scene with the cover camera."""
    w, h = SHAPES[0]
    tests = []
    for sd in (_cover(w, h), _full_scan_hits(w, h)):
        r = scenes.make_renderer(sd)
        r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, bounces=1)
        r.draw_frames(1, 1000, 10)
        st = r.stats()
        tests.append(st.sphere_tests / st.queries)
    assert tests[1] >= len(sd.spheres) > tests[0], tests  # every query of the second draw scans every slot
