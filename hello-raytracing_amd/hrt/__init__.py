"""hrt — MI355X-native path tracer (drop-in for hucancode/hello-raytracing's per-pixel ray loop).

The compute path is lib/libhrt.so (HIP kernels for gfx950 behind the C-ABI of include/hrt.h); this
package is the host-side mirror of the reference's Rust scene API plus ctypes plumbing.
"""
from . import _lib
from ._lib import (REGROUP_CELL_OCTANT, REGROUP_KEYS, REGROUP_TILE, RtRegroup, RT_HIT_FRONT, RT_HIT_TRIANGLE, RT_T_MISS, UGUARD_COLUMNS, UGUARD_HELPERS, LIB_PATH, RT_FOLD_AUTO, RT_FOLD_BUFFER, RT_FOLD_NEXT, RT_FOLD_RING, RT_MODE_MIXED, RT_SCHEDULE_AUTO, RT_SCHEDULE_QUEUE, RT_SCHEDULE_TILES, RT_MODE_SPHERE, RT_MODE_TRIS, RtError, RtParams, RtStats,
                   lib)
from .scene import (CAMERA_DTYPE, CLOSEST_DTYPE, HIT_DTYPE, MULTI_HIT_DTYPE, MULTI_HIT_MAX_K, OVERLAP_HIT_DTYPE, OVERLAP_MAX_K, VOLUME_BOX, VOLUME_BALL, DIELECTRIC, LAMBERTIAN, MATERIAL_DTYPE, MAX_OBJECT_IN_SCENE, METAL,
                    NODE_DTYPE, PI, SPHERE_DTYPE, TRIANGLE_DTYPE, Camera, ComparisonError, Material, Mesh, OrbitCamera,
                    Renderer, SceneSphere, SceneTris, Sphere, Tree, Vec3, compare_ppm_images, f32,
                    closest_points_host, lbvh_build, lbvh_cost, lbvh_refit, ppm_from_image, read_asset, render_ppm, spheres_array,
                    tree_moments_host, winding_numbers_host, cast_rays_multi_host, overlap_volumes_host)


def device_count() -> int:
    """Visible HIP devices (0 on a CPU-only host). Does not create a context on the host side."""
    return int(lib().rt_device_count())


def check_uniform_guards(n_waves: int, seed: int) -> dict:
    """rt_check_uniform_guards (include/hrt.h): the GPU self-check of the wave-uniform range guards on n_waves waves,
    as {helper: {column: count}} for the six helpers (UGUARD_HELPERS) by ten columns (UGUARD_COLUMNS). Raises RtError
    without a gfx950 device or on bad arguments."""
    import ctypes as C

    out = (C.c_uint64 * (len(UGUARD_HELPERS) * len(UGUARD_COLUMNS)))()
    _lib.check(lib().rt_check_uniform_guards(int(n_waves), int(seed) & 0xFFFFFFFF, out), "rt_check_uniform_guards")
    w = len(UGUARD_COLUMNS)
    return {h: {c: int(out[i * w + j]) for j, c in enumerate(UGUARD_COLUMNS)} for i, h in enumerate(UGUARD_HELPERS)}


def regroup_keys(origins, dirs, lo, hi):
    """rt_host_regroup_keys (include/hrt.h): rt_regroup_paths' 24-bit cell-and-octant key of each of n rays, on the host
    (no device): (n, 3) float32 origins and directions and the box (lo, hi) the origins are quantised in -> (n,) uint32.
    Raises RtError for a bad box (an extent that is not finite or below 2^-60)."""
    import ctypes as C

    import numpy as np

    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"regroup_keys: {o.shape} origins for {d.shape} directions")
    blo = np.ascontiguousarray(lo, dtype=np.float32).reshape(3)
    bhi = np.ascontiguousarray(hi, dtype=np.float32).reshape(3)
    out = np.empty((o.shape[0],), dtype=np.uint32)
    pf = C.POINTER(C.c_float)
    _lib.check(lib().rt_host_regroup_keys(o.ctypes.data_as(pf), d.ctypes.data_as(pf), o.shape[0], blo.ctypes.data_as(pf),
                                          bhi.ctypes.data_as(pf), out.ctypes.data_as(C.POINTER(C.c_uint32))),
               "rt_host_regroup_keys")
    return out


def host_tile_lists(camera, width: int, height: int, spheres, *, row0: int = 0, row_step: int = 1, row_block: int = 1,
                    min_sphere_slots: int = 0, k: int = 8):
    """Test-only (include/hrt_testing.h rt_host_tile_lists, host only): the per-tile primary candidate lists the renderer
    builds on the device, uint32[tiles, 9]: the count (0xFFFFFFFF: the tile walks), then the BVH codes."""
    import ctypes as C

    import numpy as np

    cam = np.ascontiguousarray(camera).tobytes()
    sp = np.ascontiguousarray(spheres).tobytes()
    n = C.c_size_t(0)
    args = (cam, width, height, row0, row_step, row_block, sp, len(spheres), min_sphere_slots, k)
    _lib.check(lib().rt_host_tile_lists(*args, None, 0, C.byref(n)), "rt_host_tile_lists")
    words = np.zeros(n.value, dtype=np.uint32)
    if n.value:
        _lib.check(lib().rt_host_tile_lists(*args, words.ctypes.data_as(_lib._PU32), n.value, C.byref(n)),
                   "rt_host_tile_lists")
    return words.reshape(-1, 9)


def sphere_bvh_leaves(spheres, min_sphere_slots: int = 0) -> dict:
    """Test-only (include/hrt_testing.h rt_testing_sphere_bvh_leaves, host only): the culling BVH the renderer builds over
    `spheres` padded with zero slots to min_sphere_slots, as {"leaves": [(first, count), ...] in BVH order, "slots": the
    slot of every BVH position, "large": the large list's slots, "depth"}."""
    import ctypes as C

    import numpy as np

    n = max(len(spheres), int(min_sphere_slots))
    cr = np.zeros((n, 4), dtype=np.float32)
    if len(spheres):
        cr[:len(spheres), :3] = spheres["center"]
        cr[:len(spheres), 3] = spheres["radius"]
    crp = cr.ctypes.data_as(C.POINTER(C.c_float))
    counts = (C.c_uint32 * 4)()
    _lib.check(lib().rt_testing_sphere_bvh_leaves(crp, n, None, 0, None, 0, counts), "rt_testing_sphere_bvh_leaves")
    words, slots = (C.c_uint32 * max(counts[0], 1))(), (C.c_int32 * max(counts[1] + counts[2], 1))()
    _lib.check(lib().rt_testing_sphere_bvh_leaves(crp, n, words, len(words), slots, len(slots), counts),
               "rt_testing_sphere_bvh_leaves")
    return {"leaves": [(int(w) >> 4, int(w) & 15) for w in words[:counts[0]]], "slots": list(slots[:counts[1]]),
            "large": list(slots[counts[1]:counts[1] + counts[2]]), "depth": int(counts[3])}


__all__ = [
    "host_tile_lists",
    "HIT_DTYPE", "RT_HIT_FRONT", "RT_HIT_TRIANGLE", "RT_T_MISS",
    "LIB_PATH", "RT_FOLD_AUTO", "RT_FOLD_BUFFER", "RT_FOLD_NEXT", "RT_FOLD_RING", "RT_MODE_MIXED", "RT_SCHEDULE_AUTO", "RT_SCHEDULE_QUEUE", "RT_SCHEDULE_TILES", "RT_MODE_SPHERE", "RT_MODE_TRIS", "RtError", "RtParams", "RtStats", "lib",
    "CAMERA_DTYPE", "DIELECTRIC", "LAMBERTIAN", "MATERIAL_DTYPE", "MAX_OBJECT_IN_SCENE", "METAL", "NODE_DTYPE",
    "PI", "SPHERE_DTYPE", "TRIANGLE_DTYPE", "Camera", "ComparisonError", "Material", "Mesh", "OrbitCamera", "Renderer",
    "SceneSphere", "SceneTris", "Sphere", "Tree", "Vec3", "compare_ppm_images", "f32", "ppm_from_image",
    "read_asset", "render_ppm", "spheres_array", "device_count", "check_uniform_guards", "UGUARD_COLUMNS", "UGUARD_HELPERS",
    "sphere_bvh_leaves", "regroup_keys", "REGROUP_CELL_OCTANT", "REGROUP_KEYS", "REGROUP_TILE", "RtRegroup",
    "lbvh_build", "lbvh_refit", "lbvh_cost", "CLOSEST_DTYPE", "closest_points_host",
    "tree_moments_host", "winding_numbers_host",
    "MULTI_HIT_DTYPE", "MULTI_HIT_MAX_K", "cast_rays_multi_host",
    "OVERLAP_HIT_DTYPE", "OVERLAP_MAX_K", "VOLUME_BOX", "VOLUME_BALL", "overlap_volumes_host",
]
