"""The leaf step of k_trace_split<LNODES>'s culling walk without packets (bvh_walk_noovf<.., PAIR>).

The first pass over a leaf loads its spheres two at a time before one wait; the second position of an odd leaf's last
pair lies past the leaf's count and is excluded by the count, never by what was loaded (the next leaf's first sphere, or
zeros past the buffer's end). Every sphere is still tested with the same arithmetic and the candidates are still taken in
ascending order, so the image, the query count and the box / sphere test counts cannot change.

Each scene below is built for one way that could go wrong, and test_scenes_have_their_structure checks on the host alone
(the builder's leaves through rt_testing_sphere_bvh_leaves, and the candidates of the pixel-centre rays in float64) that
the scene has the leaf sizes and candidate counts it is meant to have. A primary ray is jittered by at most one pixel
around its centre (oracle/rt_oracle.c sample_pixel), so a count is taken as present only where a pixel and its eight
neighbours agree on it.

The builder's partitions are stable, so the positions of a leaf are in ascending slot order (asserted): an exact tie inside
one leaf is always met in slot order, and a tie whose BVH order runs against the slot order needs two leaves: the
"tie_same_leaf" and the two "tie_two_leaves" scenes.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from test_gpu_packet import _coincident
from test_gpu_uniform_guards import _camera as _raw_camera

SIZES = {"64x40": (64, 40), "70x45": (70, 45)}
FRAMES = 6
SUSPENDS = (1, 24, 64)
HOLDS = (0, 12)
COUNTED = "k_trace_split<true, false, true, false>"
UNCOUNTED = "k_trace_split<true, false, false, false>"
GROUND = Sphere.new_lambertian(Vec3(0.0, -101.5, -6.0), 100.0, Vec3(0.5, 0.5, 0.5))  # (the large list)


def _ball(k, c, r):
    if k % 3 == 2:
        return Sphere.new_metal(Vec3(*c), r, Vec3(0.8, 0.7, 0.3 + 0.05 * (k % 8)), 0.1)
    return Sphere.new_lambertian(Vec3(*c), r, Vec3(0.2 + 0.09 * (k % 8), 0.6, 0.9 - 0.1 * (k % 8)))


def _scene(name, size, cam, balls, **kw):
    w, h = SIZES[size]
    sph = hrt.spheres_array([_ball(k, c, r) for k, (c, r) in enumerate(balls)] + [GROUND])
    kw.setdefault("min_sphere_slots", 0)
    return scenes.SceneDef(f"{name} {size}", hrt.RT_MODE_SPHERE, w, h, cam, sph, frames=FRAMES, bounces=6, **kw)


def _front_camera(fov=0.9):
    return Camera.new(Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, -1.0), 1.0, 0.0, fov)


def _clusters(size):
    """Clusters of 1, 2, 3 and 4 overlapping spheres, far from each other: leaves of every size. In each cluster the
    spheres shift sideways, so pixels at its edge see only its last sphere (the odd leaf's last position)."""
    balls = []
    # (along x no run of neighbouring clusters has 4 spheres or fewer: the builder makes a leaf of any such subtree)
    for n, x0, y0 in ((3, -5.5, 0.0), (2, -2.2, 0.0), (4, 0.4, 0.0), (1, 6.0, 3.0)):
        balls += [((x0 + 0.8 * j, y0, -6.0), 0.8) for j in range(n)]
    return _scene("clusters", size, _front_camera(1.2), balls)


def _concentric(size):
    """Four concentric spheres in one leaf, radii out of order: pixels with 0, 1, 2, 3 and 4 candidates in that leaf."""
    balls = [((0.0, 0.0, -5.0), r) for r in (0.9, 1.7, 0.5, 1.3)]
    balls += [((-4.0, 2.0, -7.0), 0.6), ((4.0, 2.0, -7.0), 0.6), ((4.0, -1.0, -7.0), 0.6)]
    return _scene("concentric", size, _front_camera(1.0), balls)


def _loses(size):
    """A tree of two leaves. Leaf {0, 1, 2} holds the nearest hit of the centre rays (sphere 0, t = 2.7) and its box is
    entered first (t = 0.7); leaf {3, 4}'s box is entered before that hit (t = 2) and its sphere 3, hit at t = 3.34, is
    a first candidate that loses to the running best."""
    balls = [((0.0, 0.0, -3.0), 0.3), ((0.8, -0.5, -1.0), 0.3), ((-0.8, -0.5, -1.0), 0.3),
             ((0.0, 2.5, -5.0), 3.0), ((0.5, 4.5, -5.0), 0.5)]
    return _scene("loses", size, _front_camera(1.4), balls)


TIE_FILL = [((9.0, 6.0, -5.0), 1.0), ((-9.0, 6.0, -5.0), 1.0), ((-9.0, -6.0, -5.0), 1.0), ((9.0, -6.0, -5.0), 1.0)]


def _tie_same_leaf(size):
    """The "plane" camera (every primary ray has o = 0 and d.x = 0 exactly). For such a ray a sphere at (x, 0, -5) has
    b = 10 d.z and c = 25 + x^2 - r^2 exactly: spheres 0 and 1 (x = 0, -0.75; r = 1, 1.25: c = 24), in one leaf, tie on
    every primary ray, the pair's first position first."""
    return _scene("tie_same_leaf", size, _raw_camera("plane", 1.0),
                  [((0.0, 0.0, -5.0), 1.0), ((-0.75, 0.0, -5.0), 1.25)] + TIE_FILL)


def _tie_two_leaves(size, swap):
    """As _tie_same_leaf with x = 4, 0; r = 5, 3 (c = 16), in two leaves: the second leaf's first candidate ties with
    the running best of the first (three small spheres hidden at each one's centre fill the two leaves). The wide sphere's
    leaf is entered first. swap false: the wide sphere has the lower
    slot (the later candidate loses the tie; BVH order against slot order); true: the higher one (it wins the tie)."""
    pair = [((4.0, 0.0, -5.0), 5.0), ((0.0, 0.0, -5.0), 3.0)]
    return _scene("tie_two_leaves" + ("_swapped" if swap else ""), size, _raw_camera("plane", 1.0),
                  (pair[::-1] if swap else pair) + [((x, y, -5.0), 0.3) for x in (0.0, 4.0) for y in (-0.5, 0.0, 0.5)])


def _origin_camera():
    cam = _raw_camera("axis", 1.0)
    cam["eye"] = (0.0, 0.0, 3.0, 0.0)  # every primary ray is exactly (0, 0, 3) + t (0, 0, -1): through the world origin
    return cam


def _last_leaf(size, pad):
    """Rays through the world origin, and the sphere buffer's last leaf with an odd count: a position past that leaf's
    count, read past the buffer's end as zeros, would be a sphere of radius 0 at the origin, hit at t = 3 in front of
    sphere 0. `pad`: one zero slot after the spheres (min_sphere_slots), which is such a sphere and is hit."""
    balls = [((0.0, 0.0, -4.0), 1.0), ((-3.0, 0.5, -4.0), 0.8), ((-3.4, 0.5, -4.0), 0.8), ((3.0, 0.5, -4.0), 0.8),
             ((3.4, 0.5, -4.0), 0.8), ((3.8, 0.5, -4.0), 0.8), ((0.0, 3.0, -4.0), 0.7)]
    return _scene("last_leaf" + ("_padded" if pad else ""), size, _origin_camera(), balls,
                  min_sphere_slots=len(balls) + 2 if pad else 0)  # (the spheres, the ground, one zero slot)


def _guard_plane(size):
    """The guard-forcing "plane" scene of test_gpu_uniform_guards (the eye on a sphere: c == 0, a zero numerator) at a focal
    length of 2^-50, 2a beyond candidate_t's range: the root pass's slow arm."""
    from test_gpu_uniform_guards import FOCALS, _spheres
    w, h = SIZES[size]
    return scenes.SceneDef(f"guard_plane {size}", hrt.RT_MODE_SPHERE, w, h, _raw_camera("plane", FOCALS["2^-50"]),
                           hrt.spheres_array(_spheres()), frames=FRAMES, min_sphere_slots=0)


def _coincident_scene(size):
    sd = _coincident(FRAMES)
    sd.width, sd.height = SIZES[size]
    return sd


SCENES = {
    "clusters": _clusters,
    "concentric": _concentric,
    "loses": _loses,
    "tie_same_leaf": _tie_same_leaf,
    "tie_two_leaves": lambda size: _tie_two_leaves(size, False),
    "tie_two_leaves_swapped": lambda size: _tie_two_leaves(size, True),
    "coincident": _coincident_scene,  # every t ties, within and across leaves: the lowest slot wins
    "last_leaf": lambda size: _last_leaf(size, False),
    "last_leaf_padded": lambda size: _last_leaf(size, True),
    "guard_plane": _guard_plane,
    "c3": lambda size: scenes.config_c3(*SIZES[size], FRAMES),
}
CASES = [(s, z) for s in SCENES for z in SIZES]


# ---- the scenes' structure, on the host
def _bvh(sd):
    return hrt.sphere_bvh_leaves(sd.spheres, sd.min_sphere_slots or 0)


def _slot_geo(sd, slots):
    n = len(sd.spheres)
    c = np.array([sd.spheres["center"][s] if s < n else (0.0, 0.0, 0.0) for s in slots], dtype=np.float64).reshape(-1, 3)
    r = np.array([sd.spheres["radius"][s] if s < n else 0.0 for s in slots], dtype=np.float64)
    return c, r


def _centre_rays(sd):
    """make_ray (oracle/rt_oracle.c) at the pixel centres, blur 0, in float64: origin (3,), directions (H, W, 3)."""
    cam = sd.camera
    assert float(cam["params"][1]) == 0.0
    k = np.tan(float(cam["params"][2]) * 0.5)
    ux = (2.0 * (np.arange(sd.width) + 0.5) / (sd.width - 1.0) - 1.0) * (sd.width / sd.height)
    uy = -(2.0 * (np.arange(sd.height) + 0.5) / (sd.height - 1.0) - 1.0)
    right, up, dirn = (np.asarray(cam[f], dtype=np.float64) for f in ("right", "up", "direction"))
    v = right * (ux[None, :, None] * k) + up * (uy[:, None, None] * k) + dirn
    d = v / np.linalg.norm(v, axis=2, keepdims=True) * float(cam["params"][0])
    return np.asarray(cam["eye"], dtype=np.float64)[:3], d[:, :, :3]


def _terms(o, d, c, r):
    """b, disc and t of every ray against every sphere: (H, W, n) each."""
    oc = o - c
    a = np.sum(d * d, axis=2)[:, :, None]
    b = 2.0 * np.einsum("nk,hwk->hwn", oc, d)
    disc = b * b - 4.0 * a * (np.sum(oc * oc, axis=1) - r * r)
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2.0 * a)
    return b, disc, t


def _leaf_candidates(sd, leaf):
    """Per pixel-centre ray, the candidates (disc >= 0, b <= 0) among the leaf's positions: bool (H, W, count)."""
    B = _bvh(sd)
    first, count = leaf
    o, d = _centre_rays(sd)
    b, disc, _ = _terms(o, d, *_slot_geo(sd, B["slots"][first:first + count]))
    return (disc >= 0.0) & (b <= 0.0)


def _settled(a):
    """The values of the (H, W) array that a pixel and its eight neighbours share."""
    h, w = a.shape
    same = np.ones((h - 2, w - 2), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            same &= a[dy:dy + h - 2, dx:dx + w - 2] == a[1:-1, 1:-1]
    return set(np.unique(a[1:-1, 1:-1][same]).tolist())


def _box_entry(sd, o, d, slots):
    """Where each ray enters the box of the spheres (H, W); inf where it misses it."""
    c, r = _slot_geo(sd, slots)
    lo, hi = (c - r[:, None]).min(axis=0), (c + r[:, None]).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    t0, t1 = np.where(np.isnan(t0), -np.inf, t0), np.where(np.isnan(t1), np.inf, t1)
    enter = np.maximum(np.minimum(t0, t1).max(axis=2), 0.0)
    return np.where(enter <= np.maximum(t0, t1).min(axis=2), enter, np.inf)


def _leaf_of(B, slot):
    p = B["slots"].index(slot)
    return next(lf for lf in B["leaves"] if lf[0] <= p < lf[0] + lf[1])


def _leaf_slots(B, leaf):
    return B["slots"][leaf[0]:leaf[0] + leaf[1]]


@pytest.mark.parametrize("scene,size", CASES)
def test_scenes_have_their_structure(scene, size):
    sd = SCENES[scene](size)
    B = _bvh(sd)
    n = max(len(sd.spheres), sd.min_sphere_slots or 0)
    assert sorted(B["slots"] + B["large"]) == list(range(n))
    assert B["depth"] <= 8, "k_trace_split<LNODES> needs a tree of depth <= 8"
    pos = 0
    for first, count in B["leaves"]:
        assert first == pos and 1 <= count <= 4
        assert _leaf_slots(B, (first, count)) == sorted(_leaf_slots(B, (first, count))), "a leaf is in slot order"
        pos += count
    assert pos == len(B["slots"])
    sizes = {c for _, c in B["leaves"]}
    if scene == "clusters":
        assert B["large"] == [10]
        assert sizes == {1, 2, 3, 4}
        for first, count in B["leaves"]:
            if count % 2:  # the candidate in the last position of an odd leaf, alone
                cand = _leaf_candidates(sd, (first, count))
                only_last = cand[:, :, -1] & ~cand[:, :, :-1].any(axis=2)
                assert True in _settled(only_last), (first, count)
        four = next(lf for lf in B["leaves"] if lf[1] == 4)
        assert _settled(_leaf_candidates(sd, four).sum(axis=2)) == {0, 1, 2}
    elif scene == "concentric":
        leaf = _leaf_of(B, 0)
        assert _leaf_slots(B, leaf) == [0, 1, 2, 3]
        assert _settled(_leaf_candidates(sd, leaf).sum(axis=2)) == {0, 1, 2, 3, 4}
    elif scene == "loses":
        near, far = _leaf_of(B, 0), _leaf_of(B, 3)
        assert sorted(map(tuple, (_leaf_slots(B, lf) for lf in B["leaves"]))) == [(0, 1, 2), (3, 4)]
        o, d = _centre_rays(sd)
        b, disc, t = _terms(o, d, *_slot_geo(sd, [0, 1, 2, 3, 4]))
        cand = (disc >= 0.0) & (b <= 0.0)
        enter_near, enter_far = _box_entry(sd, o, d, _leaf_slots(B, near)), _box_entry(sd, o, d, _leaf_slots(B, far))
        # (the root's two children are these leaves: the walk takes the one entered first, then the other if it is
        # entered before the best hit so far)
        lost = (cand[:, :, 0] & cand[:, :, 3] & ~cand[:, :, 4] & (t[:, :, 0] < t[:, :, 3]) & (enter_near < enter_far)
                & (enter_far < t[:, :, 0]))
        assert True in _settled(lost)
    elif scene.startswith("tie_"):
        pair = (0, 1)
        l0, l1 = _leaf_of(B, 0), _leaf_of(B, 1)
        if scene == "tie_same_leaf":
            assert l0 == l1 and _leaf_slots(B, l0)[:2] == [0, 1]
        else:
            assert l0 != l1
            wide, other = (1, 0) if scene.endswith("swapped") else (0, 1)
            assert float(sd.spheres["radius"][wide]) == 5.0
            if wide == 0:
                assert l1[0] < l0[0], "slot 0 < 1, BVH order 1 before 0"
            o, d = _centre_rays(sd)
            first = _box_entry(sd, o, d, _leaf_slots(B, _leaf_of(B, wide)))
            second = _box_entry(sd, o, d, _leaf_slots(B, _leaf_of(B, other)))
            _, _, t = _terms(o, d, *_slot_geo(sd, [wide]))
            assert True in _settled((first < second) & (second < t[:, :, 0]))
        # the exact terms of a ray of the plane x = 0 from the origin, in float32 as the kernel forms them
        c = sd.spheres["center"].astype(np.float32)
        r2 = (sd.spheres["radius"] * sd.spheres["radius"]).astype(np.float32)
        cc = [np.float32(np.float32(c[s][2] * c[s][2]) + np.float32(c[s][0] * c[s][0])) - r2[s] for s in pair]
        assert cc[0] == cc[1] and c[0][2] == c[1][2] and c[0][1] == c[1][1] == 0.0
        o, d = _centre_rays(sd)
        assert np.all(o == 0.0) and np.all(d[:, :, 0] == 0.0)
        _, _, t = _terms(o, d, *_slot_geo(sd, [0, 1]))
        others = _terms(o, d, *_slot_geo(sd, list(range(2, len(sd.spheres)))))
        hit = np.where((others[1] >= 0.0) & (others[2] > 0.0), others[2], np.inf).min(axis=2)
        assert True in _settled((t[:, :, 0] > 0.0) & (t[:, :, 0] < hit))  # the tie is the nearest hit there
    elif scene == "coincident":
        assert len(B["leaves"]) > 8 and sizes == {4}
    elif scene.startswith("last_leaf"):
        last = B["leaves"][-1]
        assert last[1] % 2 == 1, B["leaves"]
        assert last[0] + last[1] == len(B["slots"])
        o, d = _centre_rays(sd)
        assert o.tolist() == [0.0, 0.0, 3.0] and np.all(d == np.array([0.0, 0.0, -1.0]))
        b, disc, t = _terms(o, d, np.zeros((1, 3)), np.zeros(1))  # a zero record: a candidate, hit at t = 3
        assert np.all(disc == 0.0) and np.all(b < 0.0) and np.all(t == 3.0)
        _, _, t0 = _terms(o, d, *_slot_geo(sd, [0]))
        assert np.all(t0 == 6.0)  # the nearest real sphere lies behind the origin
        pads = [s for s in B["slots"] if s >= len(sd.spheres)]
        assert len(pads) == (1 if scene.endswith("padded") else 0)
    elif scene == "guard_plane":
        assert 2.0 * float(sd.camera["params"][0]) ** 2 < 2.0 ** -60  # 2a of a primary ray
    ref, q = _oracle(scene, size)
    assert q > sd.width * sd.height * sd.frames  # (rays that hit: more than one query per sample)
    if not scene.startswith("last_leaf"):  # (their primary rays are all the same ray)
        assert len(np.unique(ref.view(np.uint32))) > 8


# ---- the kernels against the oracle
_ORACLE = {}


def _oracle(scene, size):
    if (scene, size) not in _ORACLE:  # once per scene and size, shared
        img, q = scenes.oracle_render(SCENES[scene](size))
        img.setflags(write=False)
        _ORACLE[scene, size] = (img, q)
    return _ORACLE[scene, size]


def _draw(sd, hold, **params):
    r = scenes.make_renderer(sd)  # (count_tests = 1)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, steal=1, **params)
    r.set_descent_hold(hold)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,size", CASES)
def test_leaf_step_draws_the_oracle_image_with_the_same_tests(scene, size):
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")
    sd = SCENES[scene](size)
    ref, q = _oracle(scene, size)
    base = None
    for sb in SUSPENDS:
        for hold in HOLDS:
            img, st = _draw(sd, hold, suspend_below=sb)
            what = f"{sd.name} suspend_below {sb} hold {hold}"
            assert st.kernel.decode() == COUNTED, (what, st.kernel)
            np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
            assert st.queries == q, what
            if base is None:
                base = (st.box_tests, st.sphere_tests)
                assert base[1] > 0 and (base[0] > 0) == (_bvh(sd)["depth"] > 0)  # (a one-leaf tree has no box)
            assert (st.box_tests, st.sphere_tests) == base, what
    img, st = _draw(sd, 12, count_tests=0)
    assert st.kernel.decode() == UNCOUNTED, st.kernel
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=f"{sd.name} uncounted")
    assert st.queries == q
