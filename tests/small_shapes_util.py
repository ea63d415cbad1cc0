"""What test_small_shapes_oracle.py (CPU) and test_gpu_small_shapes.py (GPU) share: the scenes and shapes of the draws
at degenerate image sizes, the two comparison rules, and the tile order's rule restated in numpy.

Shapes. REGULAR are images narrower or lower than an 8x8 tile, with fewer pixels than a wave, or with fewer tiles than
the sample queue has per-XCD job counters; ONE_WIDE have a width or height of 1, where make_ray's px / (W - 1) or
py / (H - 1) is 0 / 0: every primary ray is NaN, misses everything and leaves a NaN pixel after one query.

The order rule (rt_kernels.hip order_bucket, k_order_cut, k_order_count, k_order_blockscan, k_order_scatter):
  class(c) = 127 - min((bits(f32(c) + 1) >> 21) - 508, 127): floor(4 log2(c + 1)), the most expensive class first;
  cap = ntiles * 50 // 100; walking the classes upward the head takes whole classes while n + hist[b] <= cap and closes for
  good at the first class that does not fit; order[:nhead] holds the head's tiles by class, within a class by block of
  1024 tiles (inside one class and block the LDS atomics decide); order[nhead:] is every other tile, ascending.
"""
from __future__ import annotations

import functools

import numpy as np

import hrt
import scenes
from hrt import Camera, Material, Mesh, Sphere, Tree, Vec3, read_asset

REGULAR = [(2, 2), (7, 5), (8, 8), (9, 9), (15, 17), (65, 2), (2, 65)]
ONE_WIDE = [(1, 1), (1, 9), (9, 1), (64, 1)]
FRAMES = (1, 40)
PROGRAMS = {"sphere": hrt.RT_MODE_SPHERE, "mixed": hrt.RT_MODE_MIXED, "tris": hrt.RT_MODE_TRIS}

ORDER_CLASSES, ORDER_BLOCK, ORDER_HEAD_PCT = 128, 1024, 50
# the tile order's sizes: 1, 2, 3 and 54 tiles (one block), 1025 (two blocks) and 2050 (three blocks) tiles of a slit
ORDER_SHAPES = [(2, 2), (9, 2), (17, 2), (70, 45), (2, 8200), (2, 16400)]
SLITS = [(2, 8200), (2, 16400)]
ORDER_FRAMES = 8  # one job of job_frames = 8 per tile


def shape_id(shape) -> str:
    return f"{'onewide' if tuple(shape) in ONE_WIDE else 'regular'}-{shape[0]}x{shape[1]}"


def four_spheres():
    """The spheres of test_gpu_uniform_guards._spheres(): metal, glass, metal, the Lambertian ground."""
    return [Sphere.new_metal(Vec3(0.0, 0.0, -1.0), 1.0, Vec3(0.8, 0.8, 0.8), 0.0),
            Sphere.new_dielectric(Vec3(0.0, 0.0, -5.0), 1.0, 1.5),
            Sphere.new_metal(Vec3(0.0, 2.5, -5.0), 1.0, Vec3(0.8, 0.6, 0.2), 0.0),
            Sphere.new_lambertian(Vec3(0.0, -101.0, -5.0), 100.0, Vec3(0.5, 0.5, 0.5))]


def camera() -> np.ndarray:
    """An ordinary camera: above and beside the axis, outside every sphere, a small lens. A one-tile-wide slit of any
    height sees the sky, the three spheres and the ground with it."""
    return Camera.new(Vec3(0.5, 1.0, 4.0), Vec3(0.0, 0.5, -5.0), 5.0, 0.05, 0.8)


@functools.lru_cache(maxsize=None)
def _cube():
    tree = Tree.from_mesh(Mesh.load_obj(read_asset("cube.obj"), Material.new_lambertian(Vec3(0.3, 0.4, 0.6))))
    tree.build()
    return tree.view()


def scene(program: str, w: int, h: int, frames: int) -> scenes.SceneDef:
    """sphere: the four spheres. mixed / tris: cube.obj and the last three of them (the triangle program reads no
    sphere), as test_gpu_uniform_guards.test_forced_fallback_mixed_program builds them."""
    if program == "sphere":
        return scenes.SceneDef(f"sphere {w}x{h}x{frames}", hrt.RT_MODE_SPHERE, w, h, camera(),
                               hrt.spheres_array(four_spheres()), frames=frames, min_sphere_slots=0)
    return scenes.SceneDef(f"{program} {w}x{h}x{frames}", PROGRAMS[program], w, h, camera(),
                           hrt.spheres_array(four_spheres()[1:]), bvh=_cube(), frames=frames, min_sphere_slots=0)


@functools.lru_cache(maxsize=None)
def oracle(program: str, w: int, h: int, frames: int):
    """(image, queries, node_tests, tri_tests) of the CPU oracle, rendered once per scene, shape and frame count (the
    draw paths share it) and read-only."""
    from oracle import oracle as O
    img, q = scenes.oracle_render(scene(program, w, h, frames))
    img.setflags(write=False)
    return img, q, int(O.last_counts["node_tests"]), int(O.last_counts["tri_tests"])


def assert_bits(img: np.ndarray, ref: np.ndarray, what: str):
    """The regular shapes' rule: a finite reference, and its bits."""
    assert img.shape == ref.shape and img.dtype == ref.dtype == np.float32, (what, img.shape, ref.shape)
    assert np.isfinite(ref).all(), f"{what}: the reference has {int((~np.isfinite(ref)).sum())} non-finite channels"
    same = img.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), (f"{what}: {int((~same).sum())} of {same.size} channels differ, first at "
                        f"{np.argwhere(~same)[:4].tolist()}, max |d| {np.nanmax(np.abs(img - ref))}")


def assert_nan_rule(img: np.ndarray, ref: np.ndarray, what: str):
    """The rule of the ONE_WIDE shapes alone: the NaN masks are equal and every other channel has the reference's bits (an
    x86 host and the GPU may give a NaN another sign or payload)."""
    assert img.shape == ref.shape and img.dtype == ref.dtype == np.float32, (what, img.shape, ref.shape)
    nan = np.isnan(ref)
    assert (np.isnan(img) == nan).all(), f"{what}: NaN masks differ in {int((np.isnan(img) != nan).sum())} channels"
    same = (img.view(np.uint32) == ref.view(np.uint32)) | nan
    assert same.all(), f"{what}: {int((~same).sum())} non-NaN channels differ"


def assert_image(img: np.ndarray, ref: np.ndarray, shape, what: str):
    """assert_bits, or on the four one-wide shapes the NaN rule with the mask pinned to "everything"
    (test_small_shapes_oracle.py pins the same of the oracle)."""
    w, h = shape
    assert img.shape == (h, w, 3), (what, img.shape)
    if tuple(shape) in ONE_WIDE:
        assert np.isnan(ref).all(), f"{what}: the reference is not all NaN"
        assert np.isnan(img).all(), f"{what}: {int((~np.isnan(img)).sum())} channels are not NaN"
        assert_nan_rule(img, ref, what)
    else:
        assert_bits(img, ref, what)


# ------------------------------------------------------------------------------------------------- the tile order's rule
def order_class(sums) -> np.ndarray:
    f = np.asarray(sums, dtype=np.uint32).astype(np.float32) + np.float32(1.0)
    k = (f.view(np.uint32) >> np.uint32(21)).astype(np.int64) - 508
    return (ORDER_CLASSES - 1) - np.minimum(k, ORDER_CLASSES - 1)


def order_head(sums):
    """(class of every tile, cut: the head's classes are those below it, nhead)."""
    cls = order_class(sums)
    cap = len(cls) * ORDER_HEAD_PCT // 100
    hist = np.bincount(cls, minlength=ORDER_CLASSES)
    n = cut = 0
    for b in range(ORDER_CLASSES):
        if n + hist[b] > cap:
            break
        n += int(hist[b])
        cut = b + 1
    return cls, cut, n


def one_order(sums) -> np.ndarray:
    """One order the rule allows: ascending tiles inside a class and block too."""
    cls, cut, nhead = order_head(sums)
    t = np.arange(len(cls), dtype=np.uint32)
    head = t[cls < cut]
    head = head[np.argsort(cls[head], kind="stable")]
    return np.concatenate([head, t[cls >= cut]]).astype(np.uint32)


def check_order(sums, order) -> int:
    """Asserts `order` against the rule for `sums`; returns nhead."""
    sums, order = np.asarray(sums), np.asarray(order).astype(np.int64)
    n = len(sums)
    assert order.shape == (n,), (order.shape, n)
    assert np.array_equal(np.sort(order), np.arange(n)), "not a permutation of the tiles"
    cls, cut, nhead = order_head(sums)
    head, rest = order[:nhead], order[nhead:]
    assert np.array_equal(np.sort(head), np.flatnonzero(cls < cut)), "order[:nhead] is not the head's tiles"
    key = cls[head] * (1 << 32) + head // ORDER_BLOCK
    assert (np.diff(key) >= 0).all(), "the head is not sorted by class, then by block of 1024 tiles"
    assert np.array_equal(rest, np.flatnonzero(cls >= cut)), "order[nhead:] is not the other tiles, ascending"
    return nhead
