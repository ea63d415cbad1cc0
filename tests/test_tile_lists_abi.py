"""The per-tile primary candidate lists (csrc/rt_tile_lists.hpp) without a GPU: the entry points, and soundness of the
host mirror.

Soundness is list >= what the walk could find: for every in-image pixel of a tile and every sampled frame, each leaf
sphere that is a sphere_candidate (disc >= 0 and b <= 0) of that pixel's primary ray is in the tile's list, or the tile
is marked "walk". The rays are made here, in f64, from the reference's make_ray and its PCG stream (a numpy restatement:
nothing of the rule under test is used), and by a second sampler that pushes the jitter and the lens sample to their
extremes, which no particular frame reaches.

scripts/tile_lists_sanitize.cpp is a stand-alone program over csrc/rt_tile_lists.hpp (random views, row shares and sphere
sets, with zero focal lengths, NaN and infinite camera values, zero radii and K = 0..8) for a host build with
-fsanitize=address,undefined; its build line is at its head.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import hrt
import scenes
from hrt import Camera, Sphere, Vec3, _lib
from hrt.parallel import owned_rows, rank_params

ROOT = Path(__file__).resolve().parents[1]
WALK = 0xFFFFFFFF
NAMES = ("rt_testing_set_tile_lists", "rt_testing_get_tile_lists", "rt_testing_get_tile_lists_resolved", "rt_host_tile_lists")


def test_symbols_declared_exported_bound():
    header = (ROOT / "include" / "hrt_testing.h").read_text()
    L = hrt.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.TESTING_SIGNATURES, name
        assert getattr(L, name).argtypes is not None, name
    n = C.c_size_t(0)
    assert L.rt_host_tile_lists(None, 8, 8, 0, 1, 1, None, 0, 0, 8, None, 0, C.byref(n)) == _lib.RT_ERR_ARG
    cam = np.ascontiguousarray(scenes.rtiow_camera()).tobytes()
    assert L.rt_host_tile_lists(cam, 8, 8, 0, 1, 1, None, 0, 0, 9, None, 0, C.byref(n)) == _lib.RT_ERR_ARG  # k > 8
    assert L.rt_host_tile_lists(cam, 0, 8, 0, 1, 1, None, 0, 0, 8, None, 0, C.byref(n)) == _lib.RT_ERR_ARG
    assert L.rt_host_tile_lists(cam, 20, 9, 0, 1, 1, None, 0, 0, 8, None, 0, C.byref(n)) == _lib.RT_OK
    assert n.value == 3 * 2 * 9
    assert L.rt_testing_set_tile_lists(None, 0, 8) == _lib.RT_ERR_ARG
    assert L.rt_testing_set_tile_lists(None, 3, 8) == _lib.RT_ERR_ARG


# ---- the reference's primary rays, restated (shader_sphere.wgsl make_ray and fs_main's prologue), f64
def _pcg(s):
    old = (s + np.uint32(747796405) + np.uint32(2891336453)).astype(np.uint32)
    word = (((old >> ((old >> np.uint32(28)) + np.uint32(4))) ^ old) * np.uint32(277803737)).astype(np.uint32)
    return ((word >> np.uint32(22)) ^ word).astype(np.uint32)


def _rng(s):
    s = _pcg(s)
    return s, s.astype(np.float32).astype(np.float64) * 2.0 ** -32


def _rays(cam, W, H, xs, ys, time=None, extreme=None, f32=False):
    """Origins and directions (n, 3) of the primary rays of pixels (xs, ys): of frame `time`, or with the jitter and the
    lens sample at corner `extreme` (0..15) of their ranges. f32: the focus point, the origin and the direction rounded
    to f32 at each step, as the kernels form them."""
    eye, dirv, up, right = (np.asarray(cam[k], dtype=np.float64).reshape(4) for k in ("eye", "direction", "up", "right"))
    focal, blur, fov = (float(v) for v in np.asarray(cam["params"]).reshape(4)[:3])
    n = len(xs)
    with np.errstate(over="ignore"):
        if extreme is None:
            s = ((xs.astype(np.uint32) * np.uint32(H) + ys.astype(np.uint32)) * np.uint32(time)).astype(np.uint32)
            s, r1 = _rng(s)
            s, r2 = _rng(s)
            l = np.sqrt(r1 * r1 + r2 * r2)
            j1, j2 = r1 / l, r2 / l
        else:
            j1 = np.full(n, float(extreme & 1))
            j2 = np.full(n, float((extreme >> 1) & 1))
        px, py = xs + 0.5 + j1, ys + 0.5 + j2
        ux = (2.0 * px / (np.float32(W) - np.float32(1.0)) - 1.0) * float(np.float32(W) / np.float32(H))
        uy = -(2.0 * py / (np.float32(H) - np.float32(1.0)) - 1.0)
        k = float(np.tan(np.float32(fov) * np.float32(0.5)))
        v = right[None, :] * (ux * k)[:, None] + up[None, :] * (uy * k)[:, None] + dirv[None, :]
        vn = v / np.sqrt((v * v).sum(axis=1))[:, None]  # (all four components: the reference normalises a vec4)
        f = eye[None, :3] + vn[:, :3] * focal
        if extreme is None:
            s, q1 = _rng(s)
            s, q2 = _rng(s)
            l = np.sqrt(q1 * q1 + q2 * q2)
            e1, e2 = q1 / l, q2 / l
            s, rr = _rng(s)
            rr = rr * blur
        else:
            # (the lens sample: none, or the full radius along +x, +y and the diagonal of its quadrant)
            a = (0.0, 0.0, 0.5 * np.pi, 0.25 * np.pi)[extreme >> 2]
            e1, e2 = np.full(n, np.cos(a)), np.full(n, np.sin(a))
            rr = np.full(n, blur if extreme >> 2 else 0.0)
        o = np.stack([eye[0] + e1 * rr, eye[1] + e2 * rr, np.full(n, eye[2])], axis=1)
        if f32:
            F = np.float32
            f = (eye[None, :3].astype(F) + (vn[:, :3].astype(F) * F(focal)).astype(F)).astype(F)
            lens = np.stack([(e1 * rr).astype(F), (e2 * rr).astype(F), np.zeros(n, dtype=F)], axis=1)
            o = (eye[None, :3].astype(F) + lens).astype(F)
            return o, (f - o).astype(F)
    return o, f - o


def _candidates(o, d, geo):
    """bool (rays, spheres): the reference's test that goes on to the root, in f64."""
    oc = o[:, None, :] - geo[None, :, :3]
    bd = (oc * d[:, None, :]).sum(axis=2)
    b = bd + bd
    c = (oc * oc).sum(axis=2) - geo[None, :, 3]
    a4 = 4.0 * (d * d).sum(axis=1)
    disc = b * b - a4[:, None] * c
    return (disc >= 0.0) & (b <= 0.0)


def _candidates32(o, d, geo):
    """The same test with the kernels' f32 steps (the sign of the fused discriminant is that of its exact value)."""
    F = np.float32
    g = geo.astype(F)

    def dot(a, b):
        return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)

    oc = (o[:, None, :] - g[None, :, :3]).astype(F)
    bd = dot(oc, np.broadcast_to(d[:, None, :], oc.shape)).astype(F)
    b = (bd + bd).astype(F)
    c = (dot(oc, oc).astype(F) - g[None, :, 3]).astype(F)
    a4 = (F(4.0) * dot(d, d).astype(F)).astype(F)
    a4c = (a4[:, None] * c).astype(F)
    disc = b.astype(np.float64) * b.astype(np.float64) - a4c.astype(np.float64)
    return (disc >= 0.0) & (b <= 0.0)


def _check(cam, W, H, spheres, *, row_share=None, tiles=None, frames=(0, 1, 7), k=8, expect_walk=None, min_list_frac=None,
           f32=False):
    p = dict(row0=0, row_step=1, row_block=1) if row_share is None else row_share
    rows = np.array(list(owned_rows(p["row0"], p["row_step"], H, p["row_block"])), dtype=np.int64)
    lists = hrt.host_tile_lists(cam, W, H, spheres, k=k, **p)
    tiles_w, tiles_h = (W + 7) // 8, (len(rows) + 7) // 8
    assert lists.shape == (tiles_w * tiles_h, 9)
    walk = lists[:, 0] == WALK
    assert (lists[~walk, 0] <= k).all()
    for row in lists[~walk]:
        n = int(row[0])
        assert (np.diff(row[1:1 + n].astype(np.int64)) > 0).all() and (row[1 + n:] == 0).all()
    if expect_walk is not None:
        assert walk.all() == expect_walk, walk.mean()
    if min_list_frac is not None:
        assert 1.0 - walk.mean() >= min_list_frac, walk.mean()
    B = hrt.sphere_bvh_leaves(spheres)
    slots = np.array(B["slots"], dtype=np.int64)
    geo = np.zeros((len(slots), 4))
    if len(slots):
        geo[:, :3] = np.asarray(spheres["center"], dtype=np.float64)[slots]
        geo[:, 3] = np.asarray(spheres["radius"], dtype=np.float32)[slots].astype(np.float64) ** 2
    todo = np.flatnonzero(~walk) if tiles is None else np.array([t for t in tiles if not walk[t]], dtype=np.int64)
    missing = 0
    for t in todo:
        tx, ty = t % tiles_w, t // tiles_w
        xs, kr = np.meshgrid(np.arange(tx * 8, min(tx * 8 + 8, W)), np.arange(ty * 8, min(ty * 8 + 8, len(rows))))
        xs, ys = xs.ravel().astype(np.int64), rows[kr.ravel()]
        listed = np.zeros(len(slots), dtype=bool)
        listed[lists[t, 1:1 + int(lists[t, 0])]] = True
        found = np.zeros(len(slots), dtype=bool)
        for f in frames:
            found |= _candidates(*_rays(cam, W, H, xs, ys, time=1000 + 10 * f), geo).any(axis=0)
        for e in range(16):
            found |= _candidates(*_rays(cam, W, H, xs, ys, extreme=e), geo).any(axis=0)
        if f32:  # what the kernels' own arithmetic accepts, on top of the exact rays
            for f in frames:
                found |= _candidates32(*_rays(cam, W, H, xs, ys, time=1000 + 10 * f, f32=True), geo).any(axis=0)
            for e in range(16):
                found |= _candidates32(*_rays(cam, W, H, xs, ys, extreme=e, f32=True), geo).any(axis=0)
        missing += int((found & ~listed).sum())
    assert missing == 0, f"{missing} candidate spheres missing from their tiles' lists"
    return lists


def _with_blur(cam, blur):
    cam = cam.copy()
    prm = cam["params"].copy()
    prm.reshape(-1)[1] = blur
    cam["params"] = prm
    return cam


C3_BLUR = 0.05


@pytest.mark.parametrize("blur", [0.0, C3_BLUR, 20 * C3_BLUR])
def test_sound_c3_160x90(blur):
    sd = scenes.config_c3(160, 90, 1)
    assert abs(float(np.asarray(sd.camera["params"]).reshape(-1)[1]) - C3_BLUR) < 1e-6
    lists = _check(_with_blur(sd.camera, blur), 160, 90, sd.spheres)
    if blur <= C3_BLUR:
        assert (lists[:, 0] != WALK).mean() > 0.5  # (not vacuous: most tiles keep a list)


@pytest.mark.parametrize("blur", [0.0, C3_BLUR, 20 * C3_BLUR])
def test_sound_c3_1080p_sampled_tiles(blur):
    sd = scenes.config_c3()
    tiles = np.random.default_rng(13).choice(240 * 135, size=160, replace=False)
    _check(_with_blur(sd.camera, blur), 1920, 1080, sd.spheres, tiles=tiles, frames=(0, 5),
           min_list_frac=0.95 if blur <= C3_BLUR else None)


def test_sound_ragged_70x45():
    sd = scenes.config_c3(70, 45, 1)
    _check(sd.camera, 70, 45, sd.spheres)


def test_sound_rank_3_of_8():
    sd = scenes.config_c3(160, 96, 1)
    for block in (8, 1):  # whole tiles of one row block, and interleaved rows: a tile then spans 8 x 8 image rows
        _check(sd.camera, 160, 96, sd.spheres, row_share=rank_params(3, 8, block))


def test_focal_length_zero_walks():
    sd = scenes.config_c3(64, 40, 1)
    cam = sd.camera.copy()
    prm = cam["params"].copy()
    prm.reshape(-1)[0] = 0.0
    cam["params"] = prm
    _check(cam, 64, 40, sd.spheres, expect_walk=True)


def _small_scene(extra):
    o = [Sphere.new_lambertian(Vec3(0.0, -1000.0, 0.0), 1000.0, Vec3(0.5, 0.5, 0.5))]
    for i in range(8):
        for j in range(5):
            o.append(Sphere.new_metal(Vec3(-2.8 + 0.8 * i, 0.2, -2.0 - 0.9 * j), 0.2, Vec3(0.7, 0.7, 0.5), 0.1))
    return hrt.spheres_array(o + extra)


def test_eye_inside_a_sphere_walks():
    sph = _small_scene([Sphere.new_dielectric(Vec3(0.0, 1.0, 3.0), 0.5, 1.5)])
    cam = Camera.new(Vec3(0.0, 1.0, 3.1), Vec3(0.0, 0.2, -3.0), 6.0, 0.0, 0.9)
    assert 41 in hrt.sphere_bvh_leaves(sph)["slots"]  # (a leaf sphere, not the large list)
    _check(cam, 64, 40, sph, expect_walk=True)


def test_sphere_straddling_the_eye_walks():
    """The eye just outside the sphere's surface, inside its padded ball with the lens radius."""
    sph = _small_scene([Sphere.new_dielectric(Vec3(0.0, 1.0, 3.0), 0.5, 1.5)])
    cam = Camera.new(Vec3(0.0, 1.0, 3.52), Vec3(0.0, 0.2, -3.0), 6.0, 0.05, 0.9)
    _check(cam, 64, 40, sph, expect_walk=True)
    # and from a clear distance the same scene keeps lists, which hold what its rays find
    cam = Camera.new(Vec3(0.0, 1.0, 5.0), Vec3(0.0, 0.2, -3.0), 6.0, 0.05, 0.9)
    lists = _check(cam, 64, 40, sph, expect_walk=False)
    assert (lists[:, 0] != WALK).any()


@pytest.mark.parametrize("fov", [0.1, 0.35])
@pytest.mark.parametrize("eye", [(3.0e4, 1.5e4, 5.0), (1.0e5, 5.0e4, 5.0)], ids=["3e4", "1e5"])
def test_sound_far_from_the_origin_f32(eye, fov):
    """The kernels form the ray in f32, so its error grows with the eye's distance from the origin: the lists must hold
    what the f32 ray and the f32 test accept, or the tile walks."""
    ex, ey, ez = eye
    o = [Sphere.new_lambertian(Vec3(ex, ey - 1000.0, ez), 990.0, Vec3(0.5, 0.5, 0.5))]
    for i in range(-7, 8):
        for j in range(-4, 5):
            z = ez - 6.0 - 0.37 * ((i * 5 + j * 3) % 7)
            o.append(Sphere.new_metal(Vec3(ex + 0.02 * fov * 10 * i * abs(ez - z), ey + 0.02 * fov * 10 * j * abs(ez - z), z),
                                      0.01 + 0.004 * ((i + j) % 5), Vec3(0.7, 0.7, 0.5), 0.1))
    sph = hrt.spheres_array(o)
    cam = Camera.new(Vec3(ex, ey, ez), Vec3(ex, ey, ez - 6.0), 6.0, 0.0, fov)
    tiles = np.random.default_rng(5).choice(240 * 135, size=120, replace=False)
    tiles = np.concatenate([tiles, 240 * 67 + np.arange(100, 140)])  # (and a run through the image's middle)
    lists = _check(cam, 1920, 1080, sph, tiles=tiles, frames=(0, 3), f32=True)
    assert lists.shape[0] == 240 * 135


def test_k_caps_the_lists():
    sd = scenes.config_c3(160, 90, 1)
    full = hrt.host_tile_lists(sd.camera, 160, 90, sd.spheres, k=8)
    for k in (0, 1, 3):
        capped = hrt.host_tile_lists(sd.camera, 160, 90, sd.spheres, k=k)
        over = (full[:, 0] == WALK) | (full[:, 0] > k)
        assert ((capped[:, 0] == WALK) == over).all()
        np.testing.assert_array_equal(capped[~over], full[~over])
