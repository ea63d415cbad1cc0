"""rt_occluded (Renderer.occluded): is anything in the way before tmax?

The contract is one sentence (include/hrt.h): byte i is 1 exactly when rt_cast_rays on the same renderer and the same ray
returns a hit with t < tmax[i], as an f32 comparison. So the reference throughout is the cast itself — pinned to the
oracle by test_gpu_cast_rays.py — and `expected = (prim >= 0) & (t < tmax)` in numpy float32, with no tolerance and no
rays left out. tmax = t bitwise (nothing occluded) and tmax = nextafter(t) (every hit occluded) together are the sharp
pair: a walk that computes t by another sequence than the cast, or accepts t == tmax, fails one of them.

The scene builders, ray sets and float64 sphere reference are test_gpu_cast_rays'.
"""
import ctypes as C

import numpy as np
import pytest

import hrt
import scenes
import test_gpu_cast_rays as cast

pytestmark = pytest.mark.gpu

T_MISS = np.float32(hrt.RT_T_MISS)
FACTORS = np.array([0.5, 0.999, 1.001, 2.0], np.float32)
SENTINEL = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


# ------------------------------------------------------------------------------------------------ helpers
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def occ_bytes(r, o, d, tmax=None, n=None, pad=16, offset=0):
    """The raw C call: (the n result bytes, the `pad` bytes after them), the buffer pre-filled with the sentinel and
    starting `offset` bytes into its allocation."""
    import torch

    dev = torch.device("cuda", r.device()[0])
    o, d = _np(o).astype(np.float32, copy=False), _np(d).astype(np.float32, copy=False)
    n = len(o) if n is None else n
    to = torch.from_numpy(np.ascontiguousarray(o[:n])).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(d[:n])).to(dev)
    tt = None if tmax is None else torch.from_numpy(np.ascontiguousarray(tmax[:n], dtype=np.float32)).to(dev)
    out = torch.full((offset + n + pad,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rc = hrt.lib().rt_occluded(r._h, C.c_void_p(to.data_ptr()) if n else None, C.c_void_p(td.data_ptr()) if n else None,
                               C.c_void_p(tt.data_ptr()) if tt is not None and n else None, n,
                               C.c_void_p(out.data_ptr() + offset))
    assert rc == 0, hrt.lib().rt_last_error()
    r.synchronize()
    got = out.cpu().numpy()
    assert (got[:offset] == SENTINEL).all()
    return got[offset:offset + n], got[offset + n:]


def occluded(r, o, d, tmax=None):
    """n bytes, each checked to be 0 or 1, with the bytes behind them untouched."""
    got, tail = occ_bytes(r, o, d, tmax)
    assert (tail == SENTINEL).all(), tail
    assert (got <= 1).all(), np.unique(got)
    return got.astype(bool)


def pattern_tmax(hit):
    """Pattern (d): t x {0.5, 0.999, 1.001, 2}[i % 4] (an f32 product) for a hit, a hashed value in [0.1, 50] for a miss."""
    t, prim = hit["t"], hit["prim"]
    i = np.arange(len(t))
    on_hit = np.where(prim >= 0, t, np.float32(1.0)) * FACTORS[i % 4]  # (a miss's RT_T_MISS x 2 would overflow)
    h = ((i.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    on_miss = (0.1 + 49.9 * h).astype(np.float32)
    return np.where(prim >= 0, on_hit, on_miss).astype(np.float32)


def expected(hit, tmax):
    return (hit["prim"] >= 0) & (hit["t"] < tmax)


def check_patterns(r, o, d, what, shares=False):
    """Patterns (a)-(d) on rays o, d against the renderer's own cast of them. Returns (cast, tmax of (d), result of (d))."""
    hit = cast._cpu(r.cast_rays(o, d))
    is_hit = hit["prim"] >= 0
    t = hit["t"]
    assert t.dtype == np.float32
    np.testing.assert_array_equal(occluded(r, o, d), is_hit, err_msg=f"{what}: (a) tmax NULL")
    assert not occluded(r, o, d, t).any(), f"{what}: (b) tmax = t"
    np.testing.assert_array_equal(occluded(r, o, d, np.nextafter(t, np.float32(np.inf))), is_hit,
                                  err_msg=f"{what}: (c) tmax = nextafter(t)")
    tm = pattern_tmax(hit)
    want = expected(hit, tm)
    got = occluded(r, o, d, tm)
    bad = got != want
    assert not bad.any(), (what, "(d)", int(bad.sum()), np.argwhere(bad)[:8].ravel().tolist())
    print(f"{what}: hits {is_hit.mean():.3f}, occluded under (d) {want.mean():.3f}")
    if shares:
        assert want.mean() >= 0.1 and (~want).mean() >= 0.1, (what, want.mean())
    return hit, tm, got


def primary(r, time=1000):
    return tuple(x.reshape(-1, 3) for x in r.primary_rays(time))


# ------------------------------------------------------------------------------------------------ 1. equals the cast
@pytest.mark.parametrize("case", sorted(cast.CASES))
def test_equals_the_cast_below_tmax(case):
    build, shapes, params, _, _ = cast.CASES[case]
    w, h = shapes[0]  # 70 x 45: 3150 rays, a multiple of neither 64 nor 256 (dragon-capped keeps its 64 x 48)
    r = scenes.make_renderer(build(w, h))
    r.set_params(**params)
    o, d = primary(r)
    assert len(o) == w * h
    check_patterns(r, o, d, case, shares=True)


# ------------------------------------------------------------------------------------------------ 2. beyond the first hit
@pytest.mark.parametrize("case", ["mixed-bvh-tribvh0", "mixed-bvh-tribvh1", "suzane-tribvh0", "suzane-tribvh1"])
def test_secondary_rays(case):
    """Rays leaving the first hits: incoherent, starting inside the scene's boxes, and in the mixed scene with a sphere
    and a triangle competing."""
    build, _, params, _, _ = cast.CASES[case]
    r = scenes.make_renderer(build(70, 45))
    r.set_params(**params)
    o, d = (_np(x) for x in primary(r))
    hit = cast._cpu(r.cast_rays(o, d))
    m = hit["prim"] >= 0
    assert m.sum() > 500
    p = (o[m] + hit["t"][m][:, None] * d[m] + np.float32(1e-3) * hit["normal"][m]).astype(np.float32)
    dirs = np.array([[0.3, 1.0, 0.2], [-0.6, 0.25, 0.7], [0.5, -0.4, -0.75]], np.float32)
    seen = 0
    for k, dk in enumerate(dirs):
        dd = np.broadcast_to(dk, p.shape).copy()
        _, _, got = check_patterns(r, p, dd, f"{case} direction {k}")
        seen += int(got.sum())
    assert seen > 50, seen  # (some of these rays are blocked: the test is not vacuous)


# ------------------------------------------------------------------------------------------------ 3. variants agree
@pytest.fixture(scope="module")
def grid_occluded():
    """The grid scene's 4096 + 4 rays: variant 1's cast, the pattern-(d) tmax from it, and the result per variant."""
    o, d = cast._grid_rays_with_degenerates()
    sd = cast.grid_scene(64, 40)
    hit1, tm, out = None, None, {}
    for v in (1, 3, 4):
        r = scenes.make_renderer(sd)
        r.set_params(variant=v)
        if v == 1:
            hit1 = cast._cpu(r.cast_rays(o, d))
            tm = pattern_tmax(hit1)
        out[v] = occluded(r, o, d, tm)
    return o, d, hit1, tm, out


def test_sphere_scan_variants_agree(grid_occluded):
    o, d, hit1, tm, out = grid_occluded
    want = expected(hit1, tm)
    assert len(want) == 4100 and 0.3 < want.mean() < 0.7
    for v in (1, 3, 4):
        bad = out[v] != want
        assert not bad.any(), (v, np.argwhere(bad)[:8].ravel().tolist())


def test_triangle_walks_agree_on_suzane():
    res = []
    for tb in (0, 1):
        r = scenes.make_renderer(cast.suzane_scene(70, 45))
        r.set_params(tri_bvh=tb)
        o, d = primary(r)
        if tb == 0:
            hit = cast._cpu(r.cast_rays(o, d))
            tm = pattern_tmax(hit)
        res.append(occluded(r, o, d, tm))
    np.testing.assert_array_equal(res[0], res[1])
    np.testing.assert_array_equal(res[0], expected(hit, tm))
    assert res[0].sum() > 250


# ------------------------------------------------------------------------------------------------ 4. float64 reference
def test_against_float64_sphere_reference():
    """tmax = f32(t64 x {0.5, 0.9, 1.1, 2.0}[i % 4]) with t64 the float64 near root: on the rays the reference keeps and
    that hit, occluded is `factor > 1` (the cast's t lies within 0.0052 of the distance between tmax and t64 — its
    derived bound, test_gpu_cast_rays — so the 10 % factors are never marginal); a kept miss is not occluded at all."""
    o, d = cast.grid_rays()
    win, t64, kept, _ = cast.sphere_reference(o, d)
    f = np.array([0.5, 0.9, 1.1, 2.0])[np.arange(len(o)) % 4]
    with np.errstate(over="ignore"):
        tm = (t64 * f).astype(np.float32)  # (a miss: +inf, "any hit at all")
    left_out = 1.0 - kept.mean()
    assert left_out <= 0.05, left_out
    for v in (1, 3, 4):
        r = scenes.make_renderer(cast.grid_scene(64, 40))
        r.set_params(variant=v)
        got = occluded(r, o, d, tm)
        k = kept & (win >= 0)
        print(f"variant {v}: left out {100 * left_out:.2f} %, hits {100 * (win >= 0).mean():.2f} %, "
              f"occluded {got[k].mean():.3f} of {int(k.sum())} kept hits")
        bad = k & (got != (f > 1.0))
        assert not bad.any(), (v, np.argwhere(bad)[:8].ravel().tolist())
        assert abs(got[k].mean() - 0.5) < 0.02
        none = occluded(r, o, d)
        assert not none[kept & (win < 0)].any()
        assert none[k].all()


# ------------------------------------------------------------------------------------------------ 5. degenerate tmax
DEGENERATE = np.array([np.nan, 0.0, -0.0, -1.0, 1e-45, 1e-30, hrt.RT_T_MISS, np.finfo(np.float32).max, np.inf], np.float32)


@pytest.mark.parametrize("name", ["grid", "suzane"])
def test_degenerate_tmax(name):
    sd = cast.grid_scene(70, 45) if name == "grid" else cast.suzane_scene(70, 45)
    r = scenes.make_renderer(sd)
    o, d = (_np(x) for x in primary(r))
    hit = cast._cpu(r.cast_rays(o, d))
    hits, misses = np.flatnonzero(hit["prim"] >= 0)[:96], np.flatnonzero(hit["prim"] < 0)[:96]
    assert len(hits) >= 32 and len(misses) >= 32, (len(hits), len(misses))
    block = np.concatenate([hits, misses])
    idx = np.tile(block, len(DEGENERATE))
    tm = np.repeat(DEGENERATE, len(block))
    assert DEGENERATE[4] > 0 and np.signbit(DEGENERATE[2])  # the smallest denormal is kept; -0 is a negative zero
    got = occluded(r, o[idx], d[idx], tm)
    with np.errstate(invalid="ignore"):
        want = (hit["prim"][idx] >= 0) & (hit["t"][idx] < np.fmin(tm, T_MISS)) & ~np.isnan(tm)
    bad = got != want
    assert not bad.any(), [(float(tm[k]), int(idx[k])) for k in np.flatnonzero(bad)[:8]]
    # by value: nothing below 1e-30 occludes, and the three "any hit" values give the hit mask
    per = got.reshape(len(DEGENERATE), len(block))
    assert not per[:6].any()
    for k in (6, 7, 8):
        np.testing.assert_array_equal(per[k], hit["prim"][block] >= 0)


# ------------------------------------------------------------------------------------------------ 6. tiny heaps
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8])
def test_tiny_heaps(k):
    """The triangle fans of test_gpu_parity.test_tiny_heaps_leaf_pairs_vs_oracle (n = 1, 2, 4, 8; the last leaf body
    inside or after a pair): the early exit beside the leaf-pair bookkeeping and the n == 1 case."""
    lines, faces = [], []
    for t in range(k):
        a = -1.2 + 0.3 * t
        lines += [f"v {a:.3f} -0.8 {-0.2 * t:.3f}", f"v {a + 1.1:.3f} -0.6 {-0.1 * t:.3f}", f"v {a + 0.4:.3f} 0.9 0.0"]
        faces.append(f"f {3 * t + 1} {3 * t + 2} {3 * t + 3}")
    obj = ("\n".join(lines + faces) + "\n").encode()
    tree = hrt.Tree.from_mesh(hrt.Mesh.load_obj(obj, hrt.Material.new_metal(hrt.Vec3(0.6, 0.5, 0.4), 0.3)))
    tree.build()
    sizes = tree.view()[0]
    assert sizes[1] == k and sizes[0] == (max(1, 1 << (k - 1).bit_length()) if k else 1)
    camera = hrt.Camera.new(hrt.Vec3(0.0, 0.2, 3.5), hrt.Vec3(0.0, 0.1, -3.0), 2.2, 0.0, hrt.PI * hrt.f32(0.3))
    sd = scenes.SceneDef(f"tiny{k}", hrt.RT_MODE_TRIS, 48, 32, camera, bvh=tree.view(), frames=1)
    for tb in (0, 1):
        r = scenes.make_renderer(sd)
        r.set_params(tri_bvh=tb)
        o, d = primary(r)
        hit, _, _ = check_patterns(r, o, d, f"{k} triangles, tri_bvh {tb}")
        assert (hit["prim"] >= 0).any() == (k > 0)


# ------------------------------------------------------------------------------------------------ 7. counts, sentinel
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_ray_counts_and_sentinel(n, grid_occluded):
    """The first n rays give the first n bytes of the 4100-ray result, exactly n bytes are written, and the output needs
    no alignment."""
    o, d, _, tm, out = grid_occluded
    r = scenes.make_renderer(cast.grid_scene(64, 40))
    for offset in (0, 1, 3):
        got, tail = occ_bytes(r, o, d, tm, n=n, pad=16, offset=offset)
        assert len(tail) == 16 and (tail == SENTINEL).all(), (offset, tail)
        np.testing.assert_array_equal(got, out[4][:n].astype(np.uint8), err_msg=f"offset {offset}")
    res = r.occluded(o[:n], d[:n], tm[:n])  # the wrapper, numpy in
    assert tuple(res.shape) == (n,)
    np.testing.assert_array_equal(res.cpu().numpy(), out[4][:n])


# ------------------------------------------------------------------------------------------------ 8. isolation
def test_occluded_leaves_the_draw_state_alone():
    sd = scenes.config_c3(64, 40, 6)
    ref, q = scenes.oracle_render(sd)
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE)
    r.draw_frames(3, 1000, 10)

    def snapshot():
        st = r.stats()
        return r.read_image().tobytes(), bytes(st), tuple(r.raw_counters()), r.frame_count

    before = snapshot()
    q3 = r.stats().queries
    o, d = primary(r, 1030)
    assert r.occluded(o, d).any()
    go, gd = cast.grid_rays(512)
    r.occluded(go, gd, 3.0)
    assert snapshot() == before
    r.draw_frames(3, 1030, 10)
    np.testing.assert_array_equal(r.read_image().view(np.uint32), ref.view(np.uint32))
    assert q3 + r.stats().queries == q and r.frame_count == 6


# ------------------------------------------------------------------------------------------------ 9. errors, wrapper
def test_errors_and_wrapper():
    import torch

    L = hrt.lib()
    r = hrt.Renderer(16, 8, hrt.RT_MODE_SPHERE)
    dev = torch.device("cuda", r.device()[0])
    buf = torch.zeros((128, 3), dtype=torch.float32, device=dev)
    tm = torch.ones((128,), dtype=torch.float32, device=dev)
    out = torch.zeros((128,), dtype=torch.uint8, device=dev)
    p, pt, po = C.c_void_p(buf.data_ptr()), C.c_void_p(tm.data_ptr()), C.c_void_p(out.data_ptr())
    for args in ((None, p, po), (p, None, po), (p, p, None)):
        assert L.rt_occluded(r._h, args[0], args[1], pt, 4, args[2]) == hrt._lib.RT_ERR_ARG
        assert b"rt_occluded" in L.rt_last_error()
    assert L.rt_occluded(r._h, p, p, C.c_void_p(tm.data_ptr() + 2), 4, po) == hrt._lib.RT_ERR_ARG  # tmax: 4-byte aligned
    assert L.rt_occluded(r._h, C.c_void_p(buf.data_ptr() + 2), p, pt, 4, po) == hrt._lib.RT_ERR_ARG
    assert L.rt_occluded(r._h, None, None, None, 0, None) == hrt._lib.RT_OK
    assert L.rt_occluded(r._h, p, p, None, 4, po) == hrt._lib.RT_OK  # NULL tmax; an empty scene: 100 zero slots
    assert L.rt_occluded(r._h, p, p, pt, 4, po) == hrt._lib.RT_OK
    r.synchronize()

    r = scenes.make_renderer(cast.grid_scene(64, 40))
    o, d = cast.grid_rays(300)
    hit = cast._cpu(r.cast_rays(o, d))
    res = r.occluded(o, d)
    assert res.dtype == torch.bool and tuple(res.shape) == (300,) and res.device == torch.device("cuda", r.device()[0])
    np.testing.assert_array_equal(res.cpu().numpy(), hit["prim"] >= 0)
    half = float(np.median(hit["t"]))
    np.testing.assert_array_equal(r.occluded(o, d, half).cpu().numpy(), hit["t"] < np.float32(half))  # a scalar tmax
    tt = torch.from_numpy(hit["t"]).to(res.device)
    assert not r.occluded(torch.from_numpy(o).to(res.device), torch.from_numpy(d).to(res.device), tt).any()
    with pytest.raises(ValueError):
        r.occluded(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        r.occluded(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        r.occluded(o, d, np.ones(299, np.float32))
    with pytest.raises(ValueError):
        r.occluded(o, d, np.ones((300, 2), np.float32))
    with pytest.raises(ValueError):
        r.occluded(o, d, torch.ones(300, dtype=torch.float64, device=res.device))
