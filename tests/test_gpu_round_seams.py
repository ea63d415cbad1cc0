"""The seams of k_trace_split's round: what the sample-buffer kernels read and write around the walk.

A round's shading reads the winner's hit record (KParams::code_aux: the records in BVH-code order, the large list's
behind them, then every slot's again for the full-scan fallback) and its dielectric arm the record's three constants; a
finished sample's colour goes to its place in the launch's sample buffer, frame-major over the tile-padded pixels; and the
round takes the bounce cap, the large list's length and the buffer's address from the launch's constants. The cases below
pin each of these at its edges — the last record of each of the table's three parts, both faces of a glass winner, a
launch whose buffer passes 4 GiB, launches that start at different frames, a row share, a learning launch, the bounce caps
0, 1 and 50 — and compare image bits and query counts with the CPU oracle, through the counting and the uncounted
instantiation, on whole and on ragged 8x8 tiles.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3
from hrt.parallel import owned_rows, rank_params

pytestmark = pytest.mark.gpu

SHAPES = ((64, 40), (70, 45))
FRAMES = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


# ---- the scene: 48 small spheres (radius 0.2, the median) over `nlarge` spheres of radius 20 (the large list)
def _geometry(nlarge):
    """(centre, radius) per slot; the large spheres spread through the slots (their slots are not the list's indices)."""
    geo = [((-2.8 + 0.8 * i, 0.2, -2.0 - 0.9 * j), 0.2) for i in range(8) for j in range(6)]
    for k in range(nlarge):
        big = ((-6.0 + 3.0 * (k % 5), -20.0 - 0.01 * k, -1.0 - 3.0 * (k // 5)), 20.0)
        geo.insert(min(len(geo), 3 * k + 1), big)
    return geo


def _default_material(k, c, rad):
    if k % 3 == 0:
        return Sphere.new_lambertian(c, rad, Vec3(0.8, 0.3 + 0.01 * (k % 40), 0.2))
    if k % 3 == 1:
        return Sphere.new_metal(c, rad, Vec3(0.7, 0.7, 0.5 + 0.01 * (k % 40)), 0.1)
    return Sphere.new_dielectric(c, rad, 1.5)


MATERIALS = ("glass_outside", "glass_inside", "metal_fuzz")


def _objects(geo, target, material):
    """Every slot with its default material, the target slot with the case's."""
    o = []
    for k, (c, rad) in enumerate(geo):
        c = Vec3(*c)
        if k != target:
            o.append(_default_material(k, c, rad))
        elif material == "metal_fuzz":
            o.append(Sphere.new_metal(c, rad, Vec3(0.9, 0.6, 0.3), 0.3))
        else:
            o.append(Sphere.new_dielectric(c, rad, 1.7))  # (not the other glass spheres' index: its own constants)
    return o


def _camera(geo, target, material, focal=None):
    """Looks at the target from outside (most primary rays hit its front face), or from inside it (its back face)."""
    (cx, cy, cz), rad = geo[target]
    if rad > 1.0:  # a large sphere: its top, from above or from just under it
        eye = Vec3(cx, cy + rad - 1.0, cz) if material == "glass_inside" else Vec3(cx, cy + rad + 2.0, cz + 3.0)
        at = Vec3(cx, cy + rad + 0.2, cz - 1.0) if material == "glass_inside" else Vec3(cx, cy + rad, cz)
    else:
        eye = Vec3(cx, cy, cz + 0.25 * rad) if material == "glass_inside" else Vec3(cx, cy + 0.3, cz + 3.0 * rad + 0.4)
        at = Vec3(cx, cy, cz - rad) if material == "glass_inside" else Vec3(cx, cy, cz)
    dist = float(np.sqrt((eye.x - at.x) ** 2 + (eye.y - at.y) ** 2 + (eye.z - at.z) ** 2))
    return Camera.new(eye, at, dist if focal is None else focal, 0.0, 0.9)


def _target(part):
    """(large spheres, the target's slot, full scan) for a part of the record table, read off the builder's own tree."""
    nlarge = {"last_code": 1, "large_1": 1, "large_14": 14, "slot_record": 1}[part]
    geo = _geometry(nlarge)
    B = hrt.sphere_bvh_leaves(hrt.spheres_array(_objects(geo, -1, "")))
    assert len(B["large"]) == nlarge and len(B["slots"]) + nlarge == len(geo) >= 32, B
    if part == "last_code":
        return nlarge, B["slots"][-1], False      # code nleaf - 1
    if part == "slot_record":
        return nlarge, len(geo) - 1, True         # record nleaf + nlarge + nslots - 1: the table's last
    return nlarge, B["large"][-1], False          # code nleaf + nlarge - 1 (nlarge 1: nleaf + 0)


def _kernel(count_tests):
    """The kernel every draw of this file must run: LDS nodes, NOT stealing (small launches steal by default, and the
    stealing kernel has none of the code these tests are about), counting or not, no packets; the sample buffer."""
    return f"k_trace_split<true, false, {'true' if count_tests else 'false'}, false>"


def _draw(sd, count_tests, **params):
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, count_tests=count_tests,
                 **{"fold": hrt.RT_FOLD_BUFFER, "steal": 1, **params})
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    # (fold_ring: 0 the sample buffer, 2 two of them, each launch folded inside the next; 1 would be the fold ring)
    fold = 2 if st.trace_launches > 1 and params.get("fold") == hrt.RT_FOLD_NEXT else 0
    assert st.kernel.decode() == _kernel(count_tests) and st.fold_ring == fold, (sd.name, params, st.kernel, st.fold_ring)
    return r.read_image(), st, r


def _same(img, ref, what):
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)


# ---- 1. the record's range: the last record of each part of the table, as glass from both sides and as fuzzy metal
@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("part", ["last_code", "large_1", "large_14", "slot_record"])
def test_record_range_vs_oracle(part, material):
    nlarge, target, full_scan = _target(part)
    geo = _geometry(nlarge)
    sph = hrt.spheres_array(_objects(geo, target, material))
    # (the full scan's construction: focal length 2^60, every primary ray's 2a beyond 2^100 — test_gpu_shade_by_code.py)
    cam = _camera(geo, target, material, focal=2.0 ** 60 if full_scan else None)
    for w, h in SHAPES:
        sd = scenes.SceneDef(f"{part} {material}", hrt.RT_MODE_SPHERE, w, h, cam, sph, frames=FRAMES, bounces=50,
                             min_sphere_slots=0)
        ref, q = scenes.oracle_render(sd)
        tests = {}
        for count_tests in (1, 0):
            img, st, _ = _draw(sd, count_tests=count_tests)
            what = f"{sd.name} {w}x{h} count_tests {count_tests}"
            _same(img, ref, what)
            assert st.queries == q, what
            tests[count_tests] = st.sphere_tests
        if full_scan:  # the forcing does what it says: every primary query tests every slot
            assert tests[1] >= w * h * FRAMES * len(geo), (sd.name, tests)


def test_record_range_uncovered_eye():
    """An eye at x = +inf (the other full-scan construction: a scan that accepts nothing, so no record is read)."""
    nlarge, target, _ = _target("slot_record")
    geo = _geometry(nlarge)
    cam = _camera(geo, target, "glass_outside").copy()
    eye = cam["eye"].copy()
    eye[0] = np.inf
    cam["eye"] = eye
    sd = scenes.SceneDef("eye at +inf", hrt.RT_MODE_SPHERE, 70, 45, cam, hrt.spheres_array(_objects(geo, target, "glass_outside")),
                         frames=FRAMES, bounces=50, min_sphere_slots=0)
    ref, q = scenes.oracle_render(sd)
    for count_tests in (1, 0):
        img, st, _ = _draw(sd, count_tests=count_tests)
        _same(img, ref, f"{sd.name} count_tests {count_tests}")
        assert st.queries == q


# ---- 2. the sample's place in the launch's buffer
@pytest.fixture(scope="module")
def ragged33():
    """70 x 45 (ragged tiles) x 33 frames of the cover scene: with 8-frame jobs the last job of a tile holds one frame."""
    sd = scenes.config_c3(70, 45, 33)
    return sd, scenes.oracle_render(sd)


@pytest.mark.parametrize("fold", [hrt.RT_FOLD_BUFFER, hrt.RT_FOLD_NEXT], ids=["fold1", "fold3"])
@pytest.mark.parametrize("budget_mb", [0, 1], ids=["one_launch", "cut_launches"])
def test_sample_index_launches_vs_oracle(ragged33, budget_mb, fold):
    sd, (ref, q) = ragged33
    for count_tests in (1, 0):
        img, st, _ = _draw(sd, count_tests=count_tests, fold=fold, steal=1, job_frames=8, queue_budget_mb=budget_mb)
        what = f"budget {budget_mb} fold {fold} count_tests {count_tests}"
        if budget_mb:  # 54 tiles x 64 px x 12 B = 41,472 B a frame: 25 fit 1 MiB, so two launches, of whole jobs: 24 + 9
            assert st.trace_launches == 2 and st.launch_frames == 24, (what, st.trace_launches, st.launch_frames)
        else:
            assert st.trace_launches == 1 and st.launch_frames == 33, (what, st.trace_launches, st.launch_frames)
        _same(img, ref, what)
        assert st.queries == q, what


def test_sample_index_row_share_vs_oracle():
    """Rank 3 of 8 of a 64 x 72 image in 8-row blocks: one block, rows 24..31, global coordinates in the rays."""
    sd = scenes.config_c3(64, 72, 9)
    p = rank_params(3, 8, 8)
    rows = owned_rows(p["row0"], p["row_step"], sd.height, 8)
    assert list(rows) == list(range(24, 32))
    ref, q = scenes.oracle_render(sd, rows=(p["row0"], p["row_step"], len(rows), 8))
    for count_tests in (1, 0):
        img, st, _ = _draw(sd, count_tests=count_tests, steal=1, **p)
        _same(img[:len(rows)], ref, f"row share count_tests {count_tests}")
        assert st.queries == q


def test_sample_index_learning_launch(ragged33):
    """cost_order 2: the first draw's launch counts every finished sample's queries into its pixel's counter, the
    following draw deals every launch in the learnt order; the image is the oracle's both times."""
    sd, (ref, q) = ragged33
    for count_tests in (1, 0):
        r = scenes.make_renderer(sd)
        r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, fold=hrt.RT_FOLD_BUFFER, steal=1, job_frames=8, cost_order=2,
                     count_tests=count_tests)
        r.draw_frames(sd.frames, 1000, 10)
        st = r.stats()
        assert st.ordered_launches == 0 and st.trace_launches == 1 and st.kernel.decode() == _kernel(count_tests), st.kernel
        _same(r.read_image(), ref, f"learning draw count_tests {count_tests}")
        r.reset_frame_count()
        r.draw_frames(sd.frames, 1000, 10)
        st = r.stats()
        assert st.ordered_launches == st.trace_launches == 1, (st.ordered_launches, st.trace_launches)
        assert st.kernel.decode() == _kernel(count_tests), st.kernel
        _same(r.read_image(), ref, f"ordered draw count_tests {count_tests}")
        assert st.queries == q


# ---- 3. one launch whose sample buffer passes 4 GiB
def test_sample_buffer_past_4gib():
    """1920 x 1080 x 180 frames in one launch: 373 M samples, 4.48 GB of colours, so a sample's byte offset needs more
    than 32 bits although its index does not. Bounce cap 1 over 40 spheres: a few tens of ms of tracing."""
    import torch

    W, H, F = 1920, 1080, 180
    need = 2 * 4.5e9
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the device has {free / 1e9:.1f} GB free; the two draws need 2 x 4.5 GB")
    o = [Sphere.new_lambertian(Vec3(0.0, -100.5, -3.0), 100.0, Vec3(0.5, 0.5, 0.5))]
    for k in range(39):
        o.append(_default_material(k, Vec3(-3.0 + 0.5 * (k % 13), -0.2 + 0.5 * (k // 13), -3.0 - 0.3 * (k % 5)), 0.2))
    cam = Camera.new(Vec3(0.0, 0.5, 2.0), Vec3(0.0, 0.0, -3.0), 5.0, 0.02, 0.9)
    sd = scenes.SceneDef("past 4 GiB", hrt.RT_MODE_SPHERE, W, H, cam, hrt.spheres_array(o), frames=F, bounces=1,
                         min_sphere_slots=0)
    imgs = []
    for budget_mb, launches, frames in ((0, 1, 180), (2048, 3, 64)):
        r = scenes.make_renderer(sd)
        # (a budget alone would choose the fold ring; stealing and the job size fixed, not left to the device's CU count)
        r.set_params(count_tests=0, queue_budget_mb=budget_mb, fold=hrt.RT_FOLD_BUFFER, steal=1, job_frames=32)
        r.draw_frames(F, 1000, 10)
        st = r.stats()
        assert st.kernel.decode() == _kernel(0) and st.fold_ring == 0, (st.kernel, st.fold_ring)
        assert (st.trace_launches, st.launch_frames) == (launches, frames), (budget_mb, st.trace_launches, st.launch_frames)
        imgs.append((r.read_image(), st.queries))
        del r
    _same(imgs[0][0], imgs[1][0], "one launch against launches of 2 GiB")
    assert imgs[0][1] == imgs[1][1]
    ref, _ = scenes.oracle_render(sd, rows=(67, 135, 8))
    _same(imgs[0][0][67::135], ref, "8 rows against the oracle")


# ---- 4. the round's constants
@pytest.mark.parametrize("nlarge", [0, 14])
@pytest.mark.parametrize("bounces", [0, 1, 50])
def test_round_constants_vs_oracle(bounces, nlarge):
    geo = _geometry(nlarge)
    cam = Camera.new(Vec3(0.0, 2.5, 3.0), Vec3(0.0, 0.0, -4.0), 7.0, 0.02, 0.9)
    sd = scenes.SceneDef(f"bounces {bounces} nlarge {nlarge}", hrt.RT_MODE_SPHERE, 64, 40, cam,
                         hrt.spheres_array(_objects(geo, -1, "")), frames=FRAMES, bounces=bounces, min_sphere_slots=0)
    ref, q = scenes.oracle_render(sd)
    assert (q == 0) == (bounces == 0)
    for count_tests in (1, 0):
        img, st, _ = _draw(sd, count_tests=count_tests)
        what = f"{sd.name} count_tests {count_tests}"
        _same(img, ref, what)
        assert st.queries == q, what
        if count_tests and bounces:
            assert st.sphere_tests >= nlarge * q, what  # every covered query tests the whole large list
