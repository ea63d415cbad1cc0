"""rt_trace_rays / rt_primary_rng (Renderer.trace_rays, primary_rng, trace_frame): path-traced radiance for the caller's
rays.

Oracle identity. With frame_count 0 the accumulation weight is exactly 1, so the oracle's one-frame image from a zeroed
image is 0.0 + trace(primary ray) for every pixel: trace_frame(t) — rt_trace_rays on the rays of rt_primary_rays and the
states of rt_primary_rng — must give those bits on all three channels, and its queries must sum to the oracle's ray
count. No tolerance anywhere in this file: every comparison is of uint32 views.

Everything else is held against results the identity has pinned (the per-frame results, or the same call with the rule's
rays per lane), so a forced rays-per-lane, a permutation, a batch size or a neighbour's degenerate ray can change nothing.
"""
import ctypes as C

import numpy as np
import pytest

import hrt
import scenes
from hrt import PI, Camera, Material, Mesh, Sphere, Tree, Vec3, f32, read_asset

pytestmark = pytest.mark.gpu

SHAPES = ((70, 45), (64, 40))
TIMES = (1000, 1010)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _u32(t):
    """A float32 / int32 tensor or array as a uint32 numpy array on the host (bitwise comparisons, NaNs included)."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ scenes
def split_cube_bvh():
    """Every triangle of cube2.obj as a one-triangle mesh with a material of its own kind (Lambertian, metal, glass)."""
    whole = Tree.from_mesh(Mesh.load_obj(read_asset("cube2.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
    whole.build()
    tris = whole.view()[2]
    tree = Tree()
    for k, t in enumerate(tris):
        obj = "".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in t[v][:3]) for v in ("a", "b", "c")) + "f 1 2 3\n"
        x = (k + 1.0) / (len(tris) + 1.0)
        kind = (hrt.LAMBERTIAN, hrt.METAL, hrt.DIELECTRIC)[k % 3]
        mat = Material._make([0.05 + 0.9 * x, 0.95 - 0.9 * x, 0.5, 1.0], [(0.0, 0.1, 1.5)[k % 3]] * 3, kind)
        tree.add_mesh(Mesh.load_obj(obj.encode(), mat))
    tree.build()
    return tree.view()


def cube_scene(w, h):
    cam = Camera.new(Vec3(0.0, 2.2, 6.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.0, PI * f32(0.3))  # SceneTris::new_cube
    return scenes.SceneDef("split-cube", hrt.RT_MODE_TRIS, w, h, cam, bvh=split_cube_bvh(), frames=1, bounces=5)


def suzane_scene(w, h):
    sd = scenes._tris_scene("suzane", w, h, 1)
    sd.bounces = 5
    return sd


def _golden(name, slots=None):
    def build(w, h):
        sd = scenes.golden_scene(name, w, h)
        sd.frames, sd.bounces, sd.min_sphere_slots = 1, 10, slots
        return sd
    return build


# case -> (scene builder, the scene's own bounces, the rt_params.variant values to force (0 = by slot count))
# Sphere scans: the goldens hold 4 / 5 / 26 spheres in the reference's 100 slots (auto: the culling walk, 4) and every scan
# is forced on them; with min_sphere_slots = 0 the slot count itself selects the simple scan (metal: 4) and the deferred
# scan (complex: 26). C3 (484 spheres) selects the culling walk. C4 is mixed with the linear scan (1 sphere), C5 mixed with
# the culling walk.
CASES = {
    "complex_scene": (_golden("complex_scene"), 10, (0, 1, 3, 4)),
    "dielectric_materials": (_golden("dielectric_materials"), 10, (0, 1, 3, 4)),
    "metal_materials": (_golden("metal_materials"), 10, (0, 1, 3, 4)),
    "complex_scene-slots0": (_golden("complex_scene", 0), 10, (0,)),
    "metal_materials-slots0": (_golden("metal_materials", 0), 10, (0,)),
    "c3": (lambda w, h: scenes.config_c3(w, h, 1), 50, (0, 1, 3)),
    "split-cube": (cube_scene, 5, (0,)),
    "suzane": (suzane_scene, 5, (0,)),
    "c4": (lambda w, h: scenes.config_c4(w, h, 1), 50, (0,)),
    "c5": (lambda w, h: scenes.config_c5(w, h, 1), 50, (0,)),
}


def _bounce_set(own):
    return sorted({0, 1, own, 50})


@pytest.mark.parametrize("case", sorted(CASES))
def test_traced_frame_is_the_oracles_frame(case):
    build, own, variants = CASES[case]
    for w, h in SHAPES:
        sd = build(w, h)
        if case == "c3":
            assert len(sd.spheres) == 484
        r = scenes.make_renderer(sd)
        for time in TIMES:
            for b in _bounce_set(own):
                ref, rays = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=b)
                for v in variants:
                    what = f"{case} {w}x{h} time {time} bounces {b} variant {v}"
                    r.set_params(bounces=b, variant=v)
                    img, q = r.trace_frame(time, want_queries=True)
                    assert tuple(img.shape) == (h, w, 3) and tuple(q.shape) == (h, w), what
                    bad = (_u32(img) != ref.view(np.uint32)).any(axis=2)
                    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
                    q = q.cpu().numpy()
                    assert int(q.sum()) == rays, (what, int(q.sum()), rays)
                    assert q.min() >= 0 and q.max() <= b, (what, int(q.max()))
                    if b > 0:  # (a path asks at least once)
                        assert q.min() >= 1, what


@pytest.mark.parametrize("case", ["split-cube", "suzane", "c4", "c5"])
def test_traced_frame_with_the_sah_walk_is_the_drawn_frame(case):
    """tri_bvh = 1 has no oracle parity (the oracle walks the reference heap): the traced frame against the renderer's own
    one-frame tiles draw from a zeroed image at frame count 0, and the queries against its ray count."""
    build, own, _ = CASES[case]
    w, h = SHAPES[0]
    sd = build(w, h)
    r = scenes.make_renderer(sd)
    r.set_params(tri_bvh=1, schedule=hrt.RT_SCHEDULE_TILES)
    for time in TIMES:
        for b in _bounce_set(own):
            what = f"{case} time {time} bounces {b}"
            r.set_params(bounces=b)
            r.write_image(np.zeros((h, w, 3), np.float32))
            r.set_frame_count(0)
            r.draw_frames(1, time, 10)
            ref, rays = r.read_image(), r.stats().queries
            img, q = r.trace_frame(time, want_queries=True)
            bad = (_u32(img) != ref.view(np.uint32)).any(axis=2)
            assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            assert int(q.sum()) == rays and int(q.max()) <= b, what


# ------------------------------------------------------------------------------------------------ rays are just data
@pytest.fixture(scope="module")
def two_cameras():
    """complex_scene at 70 x 45 (10 bounces) seen by its own camera and by camera_position's, at both times: the rays,
    states, and the per-frame radiance and queries (the first renderer's frames are pinned by the oracle identity above;
    the second renderer holds the same spheres). 4 x 3150 = 12600 rays, not a multiple of 64."""
    w, h = SHAPES[0]
    sd = _golden("complex_scene")(w, h)
    other = _golden("complex_scene")(w, h)
    other.camera = scenes.golden_scene("camera_position", w, h).camera
    ra, rb = scenes.make_renderer(sd), scenes.make_renderer(other)
    o, d, s, rad, q = [], [], [], [], []
    for r in (ra, rb):
        for time in TIMES:
            po, pd = r.primary_rays(time)
            o.append(po.view(-1, 3))
            d.append(pd.view(-1, 3))
            s.append(r.primary_rng(time).view(-1))
            img, qq = r.trace_frame(time, want_queries=True)
            rad.append(_u32(img).reshape(-1, 3))
            q.append(qq.cpu().numpy().reshape(-1))
    import torch

    return ra, torch.cat(o), torch.cat(d), torch.cat(s), np.concatenate(rad), np.concatenate(q)


def test_a_permuted_batch_is_the_permuted_result(two_cameras):
    import torch

    r, o, d, s, rad, q = two_cameras
    n = o.shape[0]
    assert n == 4 * 70 * 45 and n % 64 != 0
    assert (q > 1).any() and len(np.unique(rad, axis=0)) > 1000
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(20261020))
    pd = perm.to(o.device)
    got, gq = r.trace_rays(o[pd].contiguous(), d[pd].contiguous(), rng=s[pd].contiguous(), want_queries=True)
    np.testing.assert_array_equal(_u32(got), rad[perm.numpy()])
    np.testing.assert_array_equal(gq.cpu().numpy(), q[perm.numpy()])
    # and without the queries buffer, numpy in
    got = r.trace_rays(o[pd].cpu().numpy(), d[pd].cpu().numpy(), rng=s[pd].cpu().numpy())
    np.testing.assert_array_equal(_u32(got), rad[perm.numpy()])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_ray_counts_and_sentinel(n, two_cameras):
    """The first n rays give the first n records, and the words after them are not written (radiance: 12 n bytes,
    queries: 4 n bytes), with and without the queries buffer."""
    import torch

    r, o, d, s, rad, q = two_cameras
    dev = o.device
    # (start inside the first frame: rays of both frames when n > 650)
    k0 = 2500
    to, td, ts = o[k0:k0 + n].contiguous(), d[k0:k0 + n].contiguous(), s[k0:k0 + n].contiguous()
    for with_q in (True, False):
        out = torch.full((n + 2, 3), SENTINEL, dtype=torch.int32, device=dev)
        oq = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rc = hrt.lib().rt_trace_rays(r._h, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), C.c_void_p(ts.data_ptr()),
                                     0, n, C.c_void_p(out.data_ptr()), C.c_void_p(oq.data_ptr()) if with_q else None)
        assert rc == 0, hrt.lib().rt_last_error()
        r.synchronize()
        got, gq = out.cpu().numpy(), oq.cpu().numpy()
        assert (got[n:] == SENTINEL).all(), got[n:]
        assert (gq[n if with_q else 0:] == SENTINEL).all()
        np.testing.assert_array_equal(got[:n].view(np.uint32), rad[k0:k0 + n])
        if with_q:
            np.testing.assert_array_equal(gq[:n], q[k0:k0 + n])
    got, gq = r.trace_rays(to, td, rng=ts, want_queries=True)  # the wrapper
    assert tuple(got.shape) == (n, 3) and tuple(gq.shape) == (n,)
    np.testing.assert_array_equal(_u32(got), rad[k0:k0 + n])


@pytest.mark.parametrize("n", [1000, 6300])
def test_every_rays_per_lane_gives_the_same_records(n, two_cameras):
    """The host's rule for k_radiance_rays' rays per lane only reaches R > 1 at batches of hundreds of thousands of rays, so
    R is forced (include/hrt_testing.h) over every value the rule can pick, and a few it cannot (3: not a power of two; 64:
    the largest), at a batch with a partial last wave (1000 = 15 x 64 + 40) and at two whole frames (6300): chunks that
    end inside a wave's 64 R rays, and whole waves past the end of the batch."""
    r, o, d, s, rad, q = two_cameras
    to, td, ts = o[:n].contiguous(), d[:n].contiguous(), s[:n].contiguous()
    try:
        for R in (1, 2, 3, 4, 8, 16, 64):
            r.set_trace_rays_per_lane(R)
            got, gq = r.trace_rays(to, td, rng=ts, want_queries=True)
            np.testing.assert_array_equal(_u32(got), rad[:n], err_msg=f"R {R}")
            np.testing.assert_array_equal(gq.cpu().numpy(), q[:n], err_msg=f"R {R}")
            got = r.trace_rays(to, td, seed=12345)  # the NULL-state rule indexes the ray, not the lane
            r.set_trace_rays_per_lane(0)
            want = r.trace_rays(to, td, seed=12345)
            np.testing.assert_array_equal(_u32(got), _u32(want), err_msg=f"R {R}")
    finally:
        r.set_trace_rays_per_lane(0)
    with pytest.raises(hrt.RtError):
        r.set_trace_rays_per_lane(65)


# ------------------------------------------------------------------------------------------------ the grid set
def _albedo(k, n):
    x = (k + 1.0) / (n + 1.0)
    return [0.05 + 0.9 * x, 0.95 - 0.9 * x, 0.1 + 0.8 * ((7 * k + 3) % (n + 1)) / (n + 1.0), 1.0]


def _material(k, n):
    kind = (hrt.LAMBERTIAN, hrt.METAL, hrt.DIELECTRIC)[k % 3]
    return Material._make(_albedo(k, n), [(0.0, 0.1, 1.5)[k % 3]] * 3, kind)


def grid_spheres():
    """The sphere set of test_gpu_cast_rays.py, rebuilt: 49 spheres at (1.5 i, 1.5 j, -6), i, j = -3 .. 3 in i-major
    order, radius 0.4 + 0.01 (k % 7), materials by k % 3, and a ground sphere of radius 1000 at (0, -1006, -6)."""
    c, r = [], []
    for i in range(-3, 4):
        for j in range(-3, 4):
            c.append((1.5 * i, 1.5 * j, -6.0))
            r.append(0.4 + 0.01 * (len(r) % 7))
    c.append((0.0, -1006.0, -6.0))
    r.append(1000.0)
    sp = hrt.spheres_array([Sphere._make(Vec3(*ck), rk, _material(k, len(c))) for k, (ck, rk) in enumerate(zip(c, r))])
    return sp["center"].astype(np.float64), sp["radius"].astype(np.float64), sp


def grid_scene(bounces):
    cam = Camera.new(Vec3(0.0, 0.0, 2.0), Vec3(0.0, 0.0, -6.0), 8.0, 0.1, 0.9)
    return scenes.SceneDef("grid-50", hrt.RT_MODE_SPHERE, 64, 40, cam, grid_spheres()[2], frames=1, bounces=bounces,
                           min_sphere_slots=0)


def grid_rays(n=4096):
    """The 4096-ray set of test_gpu_cast_rays.py, rebuilt (same generator, same seed): origins in front of the grid, each
    aimed near one of the 49 small spheres, |d| in [0.25, 4] x the distance."""
    c, r, _ = grid_spheres()
    rng = np.random.default_rng(20261019)
    o = np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(0, 2, n)], axis=1)
    tgt = rng.integers(0, 49, n)
    off = rng.uniform(-0.7, 0.7, (n, 3)) * r[tgt][:, None]
    o = o.astype(np.float32)
    d = ((c[tgt] + off - o) * rng.uniform(0.25, 4, (n, 1))).astype(np.float32)
    return o, d


@pytest.mark.parametrize("seed", [0, 1, 0x9E3779B9])
def test_null_state_is_index_plus_one_times_seed(seed):
    o, d = grid_rays()
    r = scenes.make_renderer(grid_scene(10))
    s = ((np.arange(len(o), dtype=np.uint64) + 1) * seed % (1 << 32)).astype(np.uint32)
    want, wq = r.trace_rays(o, d, rng=s, want_queries=True)
    got, gq = r.trace_rays(o, d, seed=seed, want_queries=True)
    np.testing.assert_array_equal(_u32(got), _u32(want))
    np.testing.assert_array_equal(gq.cpu().numpy(), wq.cpu().numpy())
    assert int(wq.max()) > 1
    if seed == 1:  # the state matters: another seed draws other paths
        other = r.trace_rays(o, d, seed=2)
        assert (_u32(other) != _u32(want)).any()


def test_one_bounce_agrees_with_cast_rays():
    """bounces = 1: one query per ray, and the radiance leaves the bounces = 0 sky colour exactly where cast_rays reports a
    hit: the red channel of the sky is 0.54 u + 0.54 t = 0.54 up to rounding whatever the unnormalised d makes of t (|t| is
    below 32 on this set, so within 0.54 +- 2^-17), and every albedo's red x 0.7 is below 1."""
    o, d = grid_rays()
    r = scenes.make_renderer(grid_scene(1))
    one, q = r.trace_rays(o, d, seed=7, want_queries=True)
    assert (q.cpu().numpy() == 1).all()
    hit = r.cast_rays(o, d)["prim"].cpu().numpy() >= 0
    r.set_params(bounces=0)
    sky, q0 = r.trace_rays(o, d, seed=7, want_queries=True)
    assert (q0.cpu().numpy() == 0).all()
    assert np.isfinite(sky.cpu().numpy()).all() and (np.abs(sky.cpu().numpy()[:, 0] - 0.54) <= 2.0 ** -17).all()
    assert (np.abs(d[:, 1]) < 62).all()  # (t = 0.5 d.y + 0.5)
    differs = (_u32(one) != _u32(sky)).any(axis=1)
    np.testing.assert_array_equal(differs, hit)
    assert 0.9 < hit.mean() < 1.0


@pytest.mark.parametrize("variant", [0, 1, 3])
def test_degenerate_rays_leave_their_neighbours_alone(variant):
    """Rays with d = 0, an origin at +inf and a NaN component, mixed into the grid set: the call returns and every other
    ray's radiance and queries are bitwise what they are without them. Nothing is asserted about the degenerate rays'
    own values.

    Why the call returns: k_radiance_rays' loop either ends the lane's path (a miss, or the bounce cap) or counts a bounce, so
    a ray costs at most `bounces` queries whatever its values. Each query is bounded whatever the floats compare to:
    scan_spheres / scan_spheres_deferred are loops over the nslots slots; bvh_walk_ovf (closest_hit's culling walk) visits
    a node only by descending from its parent or popping it once, pushes behind a `sp < STACK` check (an overflow only adds
    the exact full scan, bvh_end), and a leaf holds at most 15 spheres: at most one visit per node of the tree. scatter,
    sphere_record and the exact sqrt / division sequences behind them hold no loop. (Sphere program only: the set
    test_gpu_cast_rays.py feeds rt_cast_rays.)"""
    o, d = grid_rays()
    s = np.random.default_rng(5).integers(0, 1 << 32, len(o), dtype=np.uint64).astype(np.uint32)
    r = scenes.make_renderer(grid_scene(10))
    r.set_params(variant=variant)
    want, wq = r.trace_rays(o, d, rng=s, want_queries=True)
    eo = np.array([[0.0, 0.0, 1.0], [np.inf, 0.0, 1.0], [0.0, np.nan, 1.0], [0.5, 0.5, 1.0]], dtype=np.float32)
    ed = np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, -1.0], [0.1, 0.2, -1.0], [0.0, np.nan, -1.0]], dtype=np.float32)
    at = np.array([5, 70, 1000, 4095])  # (positions in the original set the degenerate rays are inserted before)
    o2, d2 = np.insert(o, at, eo, axis=0), np.insert(d, at, ed, axis=0)
    s2 = np.insert(s, at, np.array([1, 2, 3, 4], np.uint32))
    keep = np.ones(len(o2), bool)
    keep[at + np.arange(4)] = False
    assert (o2[keep] == o).all() and np.isnan(o2[~keep]).any() and np.isinf(o2[~keep]).any()
    got, gq = r.trace_rays(o2, d2, rng=s2, want_queries=True)
    np.testing.assert_array_equal(_u32(got)[keep], _u32(want))
    np.testing.assert_array_equal(gq.cpu().numpy()[keep], wq.cpu().numpy())
    assert int(gq.max()) <= 10


# ------------------------------------------------------------------------------------------------ isolation
def test_trace_rays_leaves_the_draw_state_alone():
    sd = scenes.config_c3(64, 40, 6)
    ref, q = scenes.oracle_render(sd)

    def three(r, t0):
        r.draw_frames(3, t0, 10)
        return r.stats().queries

    r, plain = scenes.make_renderer(sd), scenes.make_renderer(sd)
    for x in (r, plain):
        x.set_params(schedule=hrt.RT_SCHEDULE_QUEUE)
    q3 = three(r, 1000)
    assert three(plain, 1000) == q3

    def snapshot():
        st = r.stats()
        return r.read_image().tobytes(), bytes(st), tuple(r.raw_counters()), r.frame_count, st.ordered_launches

    before = snapshot()
    img, tq = r.trace_frame(1030, want_queries=True)
    o, d = grid_rays(512)
    r.trace_rays(o, d, seed=3)
    assert int(tq.max()) > 1
    assert snapshot() == before
    q6 = three(r, 1030)
    three(plain, 1030)
    np.testing.assert_array_equal(r.read_image().view(np.uint32), plain.read_image().view(np.uint32))
    np.testing.assert_array_equal(r.read_image().view(np.uint32), ref.view(np.uint32))
    assert r.stats().queries == plain.stats().queries == q6
    assert q3 + q6 == q and r.frame_count == 6
    assert r.stats().ordered_launches == plain.stats().ordered_launches


def test_partition_rows_are_the_full_frames_rows():
    from hrt.parallel import owned_rows

    w, h = SHAPES[0]
    for sd in (_golden("complex_scene")(w, h), suzane_scene(w, h)):
        full = scenes.make_renderer(sd)
        fs = full.primary_rng(1010).cpu().numpy()
        fimg, fq = full.trace_frame(1010, want_queries=True)
        part = scenes.make_renderer(sd)
        part.set_params(row0=1, row_step=3, row_block=2)
        rows = owned_rows(1, 3, h, 2)
        ps = part.primary_rng(1010)
        assert tuple(ps.shape) == (len(rows), w) and len(rows) == part.local_rows and str(ps.dtype) == "torch.int32"
        np.testing.assert_array_equal(ps.cpu().numpy(), fs[rows])
        pimg, pq = part.trace_frame(1010, want_queries=True)
        assert tuple(pimg.shape) == (len(rows), w, 3)
        np.testing.assert_array_equal(_u32(pimg), _u32(fimg)[rows])
        np.testing.assert_array_equal(pq.cpu().numpy(), fq.cpu().numpy()[rows])
        assert len(np.unique(fs)) > w * h // 2


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    import torch

    L = hrt.lib()
    E = hrt._lib
    r = hrt.Renderer(16, 8, hrt.RT_MODE_SPHERE)
    dev = torch.device("cuda", r.device()[0])
    buf = torch.zeros((16 * 8, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((16 * 8, 8), dtype=torch.float32, device=dev)
    p, po = buf.data_ptr(), out.data_ptr()
    V = C.c_void_p
    # the states before a camera is set
    assert L.rt_primary_rng(r._h, 1000, V(po), 16 * 8) == E.RT_ERR_STATE
    with pytest.raises(hrt.RtError) as e:
        r.primary_rng(1000)
    assert e.value.code == E.RT_ERR_STATE
    # a trace needs no camera; a null origins / dirs / radiance pointer with n > 0 is refused, n = 0 is not
    for args in ((None, V(p), V(po)), (V(p), None, V(po)), (V(p), V(p), None)):
        assert L.rt_trace_rays(r._h, args[0], args[1], V(p), 0, 4, args[2], None) == E.RT_ERR_ARG
        assert b"rt_trace_rays" in L.rt_last_error()
    assert L.rt_trace_rays(r._h, None, None, None, 0, 0, None, None) == E.RT_OK
    # every buffer 4-byte aligned
    for k in range(5):
        a = [p, p, p, po, po + 2048]
        a[k] += 2
        assert L.rt_trace_rays(r._h, V(a[0]), V(a[1]), V(a[2]), 0, 4, V(a[3]), V(a[4])) == E.RT_ERR_ARG, k
    assert L.rt_trace_rays(r._h, V(p + 4), V(p + 8), V(p + 12), 0, 4, V(po + 4), V(po + 2052)) == E.RT_OK
    assert L.rt_trace_rays(r._h, V(p), V(p), None, 9, 4, V(po), None) == E.RT_OK  # (an empty scene: 100 zero slots)
    r.synchronize()
    r.set_camera(scenes.default_sphere_camera())
    assert L.rt_primary_rng(r._h, 1000, V(po), 16 * 8 - 1) == E.RT_ERR_ARG  # a wrong n_rays
    assert L.rt_primary_rng(r._h, 1000, None, 16 * 8) == E.RT_ERR_ARG
    assert L.rt_primary_rng(r._h, 1000, V(po + 2), 16 * 8) == E.RT_ERR_ARG
    s = r.primary_rng(1000)
    assert tuple(s.shape) == (8, 16) and s.dtype == torch.int32
    assert tuple(r.trace_frame(1000).shape) == (8, 16, 3)
    # the Python layer: shapes, dtypes and devices
    z3 = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match=r"^trace_rays: origins "):  # (the method's own name, not cast_rays')
        r.trace_rays(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        r.trace_rays(z3, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        r.trace_rays(torch.zeros((4, 3), dtype=torch.float64, device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        r.trace_rays(torch.zeros((4, 3)), torch.zeros((4, 3)))  # host tensors: the wrong device
    with pytest.raises(ValueError):
        r.trace_rays(z3, z3, rng=np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        r.trace_rays(z3, z3, rng=np.zeros(5, np.uint32))
    with pytest.raises(ValueError):
        r.trace_rays(z3, z3, rng=torch.zeros(4, dtype=torch.int32))  # a host tensor
    with pytest.raises(ValueError):
        r.trace_rays(z3, z3, rng=torch.zeros(4, dtype=torch.float32, device=dev))
    assert tuple(r.trace_rays(z3, z3, rng=np.zeros(4, np.int32)).shape) == (4, 3)
