"""TEST INFRASTRUCTURE ONLY — ctypes wrapper of oracle/build/liboracle.so (rt_oracle.c).

The CPU restatement of the reference's WGSL ray loop. Imported only by tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg, as the checker / timed CPU baseline — never by the product.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB = HERE / "build" / "liboracle.so"

MODE_SPHERE, MODE_TRIS, MODE_MIXED = 0, 1, 2
# step_cap of the walks that are not the reference's (tri_bvh = 1, the device trees): no cap, and a ray with a NaN or
# infinite component takes the triangle test over every triangle in index order (rt_oracle.c STEP_CAP_SAH, include/hrt.h)
STEP_CAP_SAH = 0xFFFFFFFF


class OParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "mode", "bounces", "ema_cap", "frame0", "time0",
                                          "dtime", "frames", "x0", "nx", "row0", "row_step", "nrows",
                                          "row_block", "step_cap")]


_libs: dict = {}

# rt_hit of include/hrt.h, the record of the per-ray entry points (restated here: the oracle does not import the product)
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("n", "<f4", (3,)), ("flags", "<u4"), ("material", "<u4"),
                      ("reserved", "<u4")])


def build() -> None:
    subprocess.run(["make", "-s", "-C", os.fspath(HERE)], check=True)


def lib(contract: int = 0) -> C.CDLL:
    """The oracle library; contract 1-5 = the float-contract study variants (rt_oracle.c ORACLE_CONTRACT)."""
    if contract not in _libs:
        path = LIB if contract == 0 else HERE / "build" / f"liboracle_c{contract}.so"
        if not path.exists() or (HERE / "rt_oracle.c").exists() and path.stat().st_mtime < (HERE / "rt_oracle.c").stat().st_mtime:
            subprocess.run(["make", "-s", "-C", os.fspath(HERE), "all" if contract == 0 else "contracts"], check=True)
        L = C.CDLL(os.fspath(path))
        L.oracle_render.restype = C.c_uint64
        L.oracle_render.argtypes = [C.POINTER(OParams), C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_uint64)]
        scene = [C.POINTER(OParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        tail = [C.c_int, C.POINTER(C.c_uint64)]
        L.oracle_cast_rays.restype = C.c_uint64
        L.oracle_cast_rays.argtypes = scene + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + tail
        L.oracle_trace_rays.restype = C.c_uint64
        L.oracle_trace_rays.argtypes = scene + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.c_void_p] + tail
        L.oracle_bounce_step.restype = C.c_uint64
        L.oracle_bounce_step.argtypes = scene + [C.c_uint32] + [C.c_void_p] * 6 + tail
        L.oracle_primary_rays.restype = None
        L.oracle_primary_rays.argtypes = [C.POINTER(OParams), C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_sizeof.restype = C.c_uint32
        L.oracle_sizeof.argtypes = [C.c_int]
        assert [L.oracle_sizeof(i) for i in range(7)] == [80, 32, 48, 32, 64, C.sizeof(OParams), HIT_DTYPE.itemsize]
        _libs[contract] = L
    return _libs[contract]


def _scene_args(mode: int, spheres, min_sphere_slots, bvh):
    """The scene as oracle_render takes it: (spheres pointer, nslots, sizes, nodes, triangles, materials pointers, and
    the arrays that must outlive the call)."""
    sph_ptr, nslots, keep = None, 0, []
    if mode != MODE_TRIS:
        sp = spheres if spheres is not None else np.zeros(0, dtype=np.uint8)
        n = len(sp)
        nslots = max(n, min_sphere_slots)
        buf = np.zeros(nslots * 48, dtype=np.uint8)
        if n:
            buf[: n * 48] = np.frombuffer(np.ascontiguousarray(sp).tobytes(), dtype=np.uint8)
        keep.append(buf)
        sph_ptr = buf.ctypes.data
    sizes_p = nodes_p = tris_p = mats_p = None
    if mode != MODE_SPHERE and bvh is not None:
        sizes, nodes, tris, mats = bvh
        sz = np.array(sizes, dtype=np.uint32)
        nodes, tris, mats = (np.ascontiguousarray(a) for a in (nodes, tris, mats))
        keep += [sz, nodes, tris, mats]
        sizes_p, nodes_p, tris_p, mats_p = sz.ctypes.data, nodes.ctypes.data, tris.ctypes.data, mats.ctypes.data
    elif mode != MODE_SPHERE:
        sz = np.zeros(2, dtype=np.uint32)
        keep.append(sz)
        sizes_p = sz.ctypes.data
    return sph_ptr, nslots, sizes_p, nodes_p, tris_p, mats_p, keep


def _threads(threads: int) -> int:
    if threads <= 0:  # explicit: importing torch can leave the OpenMP default at one thread
        threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, os.cpu_count() or 1)
    return threads


def _ray_call(mode, bounces, step_cap, spheres, min_sphere_slots, bvh):
    """(OParams, scene arguments, keep-alive list) of a per-ray call: defaults as render()."""
    if bounces is None:
        bounces = 10 if mode == MODE_SPHERE else 5
    if min_sphere_slots is None:
        min_sphere_slots = 100 if mode == MODE_SPHERE else 0
    p = OParams(0, 0, mode, bounces, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, step_cap)
    *scene, keep = _scene_args(mode, spheres, min_sphere_slots, bvh)
    return p, scene, keep


def _rays(origins, dirs):
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    assert o.ndim == 2 and o.shape[1] == 3 and o.shape == d.shape, (o.shape, d.shape)
    return o, d


def _counts(c) -> dict:
    return dict(rays=int(c[0]), node_tests=int(c[1]), tri_tests=int(c[2]), capped_walks=int(c[3]))


def cast_rays(origins, dirs, *, mode: int, spheres=None, min_sphere_slots: int | None = None, bvh=None,
              step_cap: int = 600, flat: bool = False, threads: int = 0, contract: int = 0):
    """oracle_cast_rays: what one bounce of trace() sees for each of the (n, 3) float32 rays, as HIT_DTYPE records
    (the bytes of rt_hit). flat: the triangle part is the triangle test over every triangle in index order, no tree.
    Returns (records, counts dict)."""
    o, d = _rays(origins, dirs)
    p, scene, keep = _ray_call(mode, 0, step_cap, spheres, min_sphere_slots, bvh)
    hits = np.zeros(len(o), dtype=HIT_DTYPE)
    c = (C.c_uint64 * 4)()
    lib(contract).oracle_cast_rays(C.byref(p), *scene, len(o), o.ctypes.data, d.ctypes.data, int(flat), hits.ctypes.data,
                                   _threads(threads), c)
    return hits, _counts(c)


def trace_rays(origins, dirs, *, mode: int, rng=None, seed: int = 0, bounces: int | None = None, spheres=None,
               min_sphere_slots: int | None = None, bvh=None, step_cap: int = 600, threads: int = 0, contract: int = 0):
    """oracle_trace_rays: 0.0 + trace(ray) for each ray from the given (n,) uint32 RNG states, or rng None and state
    (i + 1) * seed in u32. Returns (radiance (n, 3) float32, queries (n,) uint32, counts dict)."""
    o, d = _rays(origins, dirs)
    p, scene, keep = _ray_call(mode, bounces, step_cap, spheres, min_sphere_slots, bvh)
    s = None
    if rng is not None:
        s = np.ascontiguousarray(rng).view(np.uint32)
        assert s.shape == (len(o),), s.shape
    rad = np.zeros((len(o), 3), dtype=np.float32)
    q = np.zeros(len(o), dtype=np.uint32)
    c = (C.c_uint64 * 4)()
    lib(contract).oracle_trace_rays(C.byref(p), *scene, len(o), o.ctypes.data, d.ctypes.data,
                                    s.ctypes.data if s is not None else None, int(seed) & 0xFFFFFFFF, rad.ctypes.data,
                                    q.ctypes.data, _threads(threads), c)
    return rad, q, _counts(c)


def bounce_step(origins, dirs, rng, throughput, *, mode: int, spheres=None, min_sphere_slots: int | None = None,
                bvh=None, step_cap: int = 600, threads: int = 0, contract: int = 0):
    """oracle_bounce_step: one iteration of trace()'s loop. The inputs are left alone; returns the new
    (origins, dirs, rng, throughput), the HIT_DTYPE records of the rays before the scatter and the (n,) bool hit flags.
    A ray that misses keeps its state bit for bit."""
    o, d = (a.copy() for a in _rays(origins, dirs))
    s = np.ascontiguousarray(rng).view(np.uint32).copy()
    tp = np.ascontiguousarray(throughput, dtype=np.float32).copy()
    assert s.shape == (len(o),) and tp.shape == o.shape, (s.shape, tp.shape)
    p, scene, keep = _ray_call(mode, 0, step_cap, spheres, min_sphere_slots, bvh)
    hits = np.zeros(len(o), dtype=HIT_DTYPE)
    flags = np.zeros(len(o), dtype=np.uint8)
    c = (C.c_uint64 * 4)()
    lib(contract).oracle_bounce_step(C.byref(p), *scene, len(o), o.ctypes.data, d.ctypes.data, s.ctypes.data,
                                     tp.ctypes.data, hits.ctypes.data, flags.ctypes.data, _threads(threads), c)
    return o, d, s, tp, hits, flags != 0


def primary_rays(*, width: int, height: int, mode: int, camera: np.ndarray, time: int, rows=None, x0: int = 0,
                 nx: int | None = None, contract: int = 0):
    """oracle_primary_rays: the ray sample_pixel hands to trace() and the RNG state after make_ray, for the pixels
    render() would draw with the same rows / x0 / nx. Returns (origins, dirs (nrows, nx, 3) float32, rng (nrows, nx)
    uint32)."""
    row0, row_step, nrows, row_block = (tuple(rows) + (1,))[:4] if rows is not None else (0, 1, height, 1)
    nx = width - x0 if nx is None else nx
    p = OParams(width, height, mode, 0, 0, 0, 0, 0, 0, x0, nx, row0, row_step, nrows, row_block, 0)
    o = np.zeros((nrows, nx, 3), dtype=np.float32)
    d = np.zeros((nrows, nx, 3), dtype=np.float32)
    s = np.zeros((nrows, nx), dtype=np.uint32)
    lib(contract).oracle_primary_rays(C.byref(p), np.ascontiguousarray(camera).tobytes(), int(time) & 0xFFFFFFFF,
                                      o.ctypes.data, d.ctypes.data, s.ctypes.data)
    return o, d, s


def render(*, width: int, height: int, mode: int, camera: np.ndarray, frames: int, time0: int = 1000,
           dtime: int = 10, frame0: int = 0, bounces: int | None = None, ema_cap: int = 1000,
           spheres: np.ndarray | None = None, min_sphere_slots: int | None = None, bvh=None,
           rows=None, x0: int = 0, nx: int | None = None, image: np.ndarray | None = None,
           threads: int = 0, step_cap: int = 600, contract: int = 0):
    """Render `frames` frames (time0 + f*dtime, frame_count frame0 + f) of a scene.

    spheres: SPHERE_DTYPE array (zero slots appended up to min_sphere_slots, default 100 in sphere mode
    like the reference's 100-slot buffer); bvh: (sizes, nodes, triangles, materials) from Tree.view().
    rows: (row0, row_step, nrows[, row_block]) subset of rows (global coordinates), default all rows; with
    row_block b > 1 local row k is row0 + (k // b) * row_step * b + k % b (rt_params.row_block).
    step_cap: the reference walk's 600-step cap (shader_tris.wgsl:274); 0 = uncapped (only to check the
    opt-in SAH triangle walk, which has no cap); STEP_CAP_SAH = uncapped, with that walk's rule for non-finite rays.
    Returns (image[nrows, nx, 3] float32, queries).
    """
    if bounces is None:
        bounces = 10 if mode == MODE_SPHERE else 5
    if min_sphere_slots is None:
        min_sphere_slots = 100 if mode == MODE_SPHERE else 0
    row0, row_step, nrows, row_block = (tuple(rows) + (1,))[:4] if rows is not None else (0, 1, height, 1)
    nx = width - x0 if nx is None else nx
    p = OParams(width, height, mode, bounces, ema_cap, frame0, time0, dtime, frames, x0, nx, row0, row_step, nrows,
                row_block, step_cap)
    sph_ptr, nslots, sizes_p, nodes_p, tris_p, mats_p, keep = _scene_args(mode, spheres, min_sphere_slots, bvh)
    if image is None:
        image = np.zeros((nrows, nx, 3), dtype=np.float32)
    else:
        image = np.ascontiguousarray(image, dtype=np.float32).copy()
        assert image.shape == (nrows, nx, 3)
    cam = np.ascontiguousarray(camera).tobytes()
    if threads <= 0:  # explicit: importing torch can leave the OpenMP default at one thread
        threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, os.cpu_count() or 1)
    counts = (C.c_uint64 * 4)()
    q = lib(contract).oracle_render(C.byref(p), cam, sph_ptr, nslots, sizes_p, nodes_p, tris_p, mats_p,
                            image.ctypes.data, threads, counts)
    last_counts.update(rays=counts[0], node_tests=counts[1], tri_tests=counts[2], capped_walks=counts[3])
    return image, int(q)


# {rays, node_tests, tri_tests} of the last render() call (triangle-program work counters)
last_counts: dict = {}
