"""Python mirror of the reference's scene API (hucancode/hello-raytracing src/scene, src/geometry,
src/renderer.rs), over the C-ABI in include/hrt.h.

Names, argument meaning and call order follow the Rust code so that tests read like
tests/rendering_tests.rs:

    scene = SceneSphere.new(512, 512)            # SceneSphere::new(RenderOutput::Headless(512, 512))
    scene.objects.clear()
    scene.objects.append(Sphere.new_lambertian(Vec3(-2, 0, -5), 1.0, Vec3(0.8, 0.2, 0.2)))
    scene.init()                                  # Scene::init: set_camera + write_scene_data
    for i in range(frames):
        scene.set_time(1000 + i * 10); scene.draw()
    ppm = render_ppm(scene.renderer)

POD values are numpy structured scalars/arrays with the reference's #[repr(C)] layouts.
"""
from __future__ import annotations

import ctypes as C
import gzip
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import RT_MODE_MIXED, RT_MODE_SPHERE, RT_MODE_TRIS, RtParams, RtStats, check, lib

LAMBERTIAN, METAL, DIELECTRIC = 1, 2, 3  # src/scene/material.rs:4-6
MAX_OBJECT_IN_SCENE = 100  # src/scene/scene_sphere.rs:15
MAX_TRIS = 1_000_000  # src/scene/scene_tris.rs:11
MAX_MATS = 1000  # src/scene/scene_tris.rs:12
PI = np.float32(math.pi)  # std::f32::consts::PI

ASSETS = _lib.PKG_ROOT / "assets"

CAMERA_DTYPE = np.dtype([("eye", "<f4", 4), ("direction", "<f4", 4), ("up", "<f4", 4),
                         ("right", "<f4", 4), ("params", "<f4", 4)])
MATERIAL_DTYPE = np.dtype([("albedo", "<f4", 4), ("params", "<f4", 3), ("kind", "<u4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material", MATERIAL_DTYPE)])
NODE_DTYPE = np.dtype([("bound_min", "<f4", 4), ("bound_max", "<f4", 4)])
TRIANGLE_DTYPE = np.dtype([("a", "<f4", 4), ("b", "<f4", 4), ("c", "<f4", 4), ("custom", "<f4", 3),
                           ("material", "<u4")])
# rt_hit (include/hrt.h): one record of rt_cast_rays
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("n", "<f4", 3), ("flags", "<u4"), ("material", "<u4"),
                      ("reserved", "<u4")])
assert HIT_DTYPE.itemsize == 32
# rt_closest (include/hrt.h): one record of rt_closest_points
CLOSEST_DTYPE = np.dtype([("d2", "<f4"), ("prim", "<i4"), ("p", "<f4", 3), ("v", "<f4"), ("w", "<f4"),
                          ("reserved", "<u4")])
assert CLOSEST_DTYPE.itemsize == 32
# rt_multi_hit (include/hrt.h): one record of rt_cast_rays_multi
MULTI_HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")])
MULTI_HIT_MAX_K = 16
assert MULTI_HIT_DTYPE.itemsize == 16
# rt_overlap_hit (include/hrt.h): one record of rt_overlap_volumes; the kinds of volume and their floats per query
OVERLAP_HIT_DTYPE = np.dtype([("d2", "<f4"), ("prim", "<i4"), ("v", "<f4"), ("w", "<f4")])
OVERLAP_MAX_K = 16
VOLUME_BOX, VOLUME_BALL = 1, 2
_VOLUME_FLOATS = {VOLUME_BOX: 6, VOLUME_BALL: 4}
assert OVERLAP_HIT_DTYPE.itemsize == 16
assert CAMERA_DTYPE.itemsize == 80 and MATERIAL_DTYPE.itemsize == 32 and SPHERE_DTYPE.itemsize == 48
assert NODE_DTYPE.itemsize == 32 and TRIANGLE_DTYPE.itemsize == 64


def f32(x) -> np.float32:
    return np.float32(x)


def _ptr(t):
    """A torch tensor's device address for a void* argument or field; None (an optional buffer not given) is null."""
    return t.data_ptr() if t is not None else None


@dataclass(frozen=True)
class Vec3:
    x: float
    y: float
    z: float

    def arr(self) -> np.ndarray:
        return np.array([self.x, self.y, self.z], dtype=np.float32)


class Camera:
    """src/scene/camera.rs — 80-byte POD."""

    @staticmethod
    def new(from_: Vec3, to: Vec3, focal_length, focal_blur_amount, fov) -> np.ndarray:
        out = C.create_string_buffer(80)
        a, b = from_.arr(), to.arr()
        check(lib().rt_host_camera_new(a.ctypes.data_as(_lib._PF), b.ctypes.data_as(_lib._PF),
                                       float(f32(focal_length)), float(f32(focal_blur_amount)),
                                       float(f32(fov)), out), "Camera::new")
        return np.frombuffer(out.raw, dtype=CAMERA_DTYPE)[0].copy()


def _glam_normalize(v: np.ndarray) -> np.ndarray:
    """glam 0.24 Vec3::normalize: v * (1 / sqrt(x*x + y*y + z*z)), f32, no FMA."""
    d = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return v * (np.float32(1.0) / np.sqrt(d))


def _glam_cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]],
                    dtype=np.float32)


class OrbitCamera:
    """src/camera_controller.rs:5-129 — the interactive app's camera. Only `to_uniform` crosses the boundary:
    App re-uploads it every redraw through Scene::update_camera -> Renderer::update_camera_uniform
    (app.rs:138, mod.rs:52,93, renderer.rs:330-334), the same 80-byte binding as Camera but with w = 0 basis
    vectors, focal length 10 and no blur — the kernels' 4-component make_ray normalise then acts in 3-D."""

    def __init__(self, aspect_ratio: float, radius: float = 5.0, theta: float = 0.0, phi: float = math.pi / 4.0):
        self.target = np.zeros(3, dtype=np.float32)
        self.up = np.array([0.0, 1.0, 0.0], dtype=np.float32)
        self.fov = f32(math.radians(45.0))  # 45.0_f32.to_radians()
        self.aspect_ratio = f32(aspect_ratio)
        self.radius, self.theta, self.phi = f32(radius), f32(theta), f32(phi)
        self.update_position()

    def update_position(self) -> None:
        """camera_controller.rs:60-71 (f32 sin/cos; the host libm's, not pinned against Rust's)."""
        self.phi = f32(min(max(self.phi, f32(0.1)), f32(math.pi) - f32(0.1)))
        sp, cp = np.sin(self.phi, dtype=np.float32), np.cos(self.phi, dtype=np.float32)
        st, ct = np.sin(self.theta, dtype=np.float32), np.cos(self.theta, dtype=np.float32)
        x, y, z = self.radius * sp * ct, self.radius * cp, self.radius * sp * st
        self.position = self.target + np.array([x, y, z], dtype=np.float32)

    def build_view_matrix(self):
        """camera_controller.rs:107-113: forward, up, right."""
        forward = _glam_normalize(self.target - self.position)
        right = _glam_normalize(_glam_cross(forward, self.up))
        up = _glam_normalize(_glam_cross(right, forward))
        return forward, up, right

    def to_uniform(self) -> np.ndarray:
        """camera_controller.rs:116-129: CameraUniform {eye.w = 1, direction/up/right .w = 0, 10, 0, fov, 0}."""
        forward, up, right = self.build_view_matrix()
        u = np.zeros((), dtype=CAMERA_DTYPE)
        u["eye"] = np.append(self.position, np.float32(1.0))
        u["direction"] = np.append(forward, np.float32(0.0))
        u["up"] = np.append(up, np.float32(0.0))
        u["right"] = np.append(right, np.float32(0.0))
        u["params"] = np.array([10.0, 0.0, self.fov, 0.0], dtype=np.float32)
        return u


class Material:
    """src/scene/material.rs:17-37."""

    @staticmethod
    def _make(albedo, params, kind) -> np.ndarray:
        m = np.zeros((), dtype=MATERIAL_DTYPE)
        m["albedo"] = albedo
        m["params"] = params
        m["kind"] = kind
        return m

    @staticmethod
    def new_lambertian(albedo: Vec3) -> np.ndarray:
        return Material._make([albedo.x, albedo.y, albedo.z, 1.0], [0, 0, 0], LAMBERTIAN)

    @staticmethod
    def new_metal(albedo: Vec3, fuzzy) -> np.ndarray:
        return Material._make([albedo.x, albedo.y, albedo.z, 1.0], [fuzzy] * 3, METAL)

    @staticmethod
    def new_dielectric(ir) -> np.ndarray:
        return Material._make([1.0, 1.0, 1.0, 1.0], [ir] * 3, DIELECTRIC)


class Sphere:
    """src/scene/sphere.rs:14-37."""

    @staticmethod
    def _make(center: Vec3, radius, material) -> np.ndarray:
        s = np.zeros((), dtype=SPHERE_DTYPE)
        s["center"] = center.arr()
        s["radius"] = radius
        s["material"] = material
        return s

    @staticmethod
    def new_lambertian(center: Vec3, radius, color: Vec3) -> np.ndarray:
        return Sphere._make(center, radius, Material.new_lambertian(color))

    @staticmethod
    def new_metal(center: Vec3, radius, color: Vec3, fuzzy) -> np.ndarray:
        return Sphere._make(center, radius, Material.new_metal(color, fuzzy))

    @staticmethod
    def new_dielectric(center: Vec3, radius, ir) -> np.ndarray:
        return Sphere._make(center, radius, Material.new_dielectric(ir))


def spheres_array(objects) -> np.ndarray:
    arr = np.zeros(len(objects), dtype=SPHERE_DTYPE)
    for i, s in enumerate(objects):
        arr[i] = s
    return arr


# ----------------------------------------------------------------------------------------- meshes / BVH
def read_asset(name: str) -> bytes:
    """Bytes of an OBJ asset (stored gzip-compressed under hello-raytracing_amd/assets/)."""
    p = ASSETS / f"{name}.gz"
    if p.exists():
        return gzip.decompress(p.read_bytes())
    return (ASSETS / name).read_bytes()


class Mesh:
    """src/geometry/mesh.rs — Mesh::load_obj(source, material)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def load_obj(source: bytes, material: np.ndarray) -> "Mesh":
        h = C.c_void_p()
        mat = np.ascontiguousarray(material).tobytes()
        check(lib().rt_host_mesh_load_obj(source, len(source), mat, C.byref(h)), "Mesh::load_obj")
        return Mesh(h)

    def counts(self) -> tuple[int, int]:
        nv, ni = C.c_uint32(), C.c_uint32()
        check(lib().rt_host_mesh_counts(self._h, C.byref(nv), C.byref(ni)), "mesh_counts")
        return nv.value, ni.value

    def __del__(self):
        if getattr(self, "_h", None):
            lib().rt_host_mesh_destroy(self._h)
            self._h = None


class Tree:
    """src/scene/bvh/tree.rs — implicit-heap median-split BVH (Tree::from(mesh), add_mesh, build)."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().rt_host_tree_new(C.byref(h)), "Tree::new")
        self._h = h

    @staticmethod
    def from_mesh(mesh: Mesh) -> "Tree":
        t = Tree()
        t.add_mesh(mesh)
        return t

    def add_mesh(self, mesh: Mesh) -> None:
        check(lib().rt_host_tree_add_mesh(self._h, mesh._h), "Tree::add_mesh")

    def build(self, threads: int = 0) -> None:
        """tree.rs:36-72. threads 0 = all (capped at 16); the result does not depend on it."""
        if threads:
            check(lib().rt_host_tree_build_threads(self._h, threads), "Tree::build")
        else:
            check(lib().rt_host_tree_build(self._h), "Tree::build")

    def view(self):
        """(sizes[2], nodes, triangles, materials) as numpy copies."""
        sizes = (C.c_uint32 * 2)()
        pn, pt, pm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nn, nt, nm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().rt_host_tree_view(self._h, sizes, C.byref(pn), C.byref(nn), C.byref(pt), C.byref(nt),
                                      C.byref(pm), C.byref(nm)), "Tree::view")

        def grab(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(C.string_at(ptr.value, n * dt.itemsize), dtype=dt).copy()

        return ([sizes[0], sizes[1]], grab(pn, nn.value, NODE_DTYPE), grab(pt, nt.value, TRIANGLE_DTYPE),
                grab(pm, nm.value, MATERIAL_DTYPE))

    @property
    def sizes(self):
        return self.view()[0]

    def __del__(self):
        if getattr(self, "_h", None):
            lib().rt_host_tree_destroy(self._h)
            self._h = None


# ----------------------------------------------------------------------------------------- renderer
class Renderer:
    """src/renderer.rs Renderer (headless), backed by the HIP kernels. GPU required."""

    def __init__(self, width: int, height: int, mode: int):
        h = C.c_void_p()
        L = lib()
        _lib.check_single_hip_runtime()  # (torch may have been imported since libhrt.so was loaded)
        check(L.rt_create(width, height, mode, C.byref(h)), "Renderer::new")
        self._h = h
        self.mode = mode
        self.width = width
        self.height = height

    # --- protocol (renderer.rs:315-410)
    def set_camera(self, camera: np.ndarray) -> None:
        check(lib().rt_set_camera(self._h, np.ascontiguousarray(camera).tobytes()), "set_camera")

    def set_time(self, time: int) -> None:
        check(lib().rt_set_time(self._h, int(time) & 0xFFFFFFFF), "set_time")

    def set_frame_count(self, n: int) -> None:
        check(lib().rt_set_frame_count(self._h, n), "set_frame_count")

    def device(self) -> tuple:
        """(HIP ordinal, (PCI domain, bus, device)) of the GPU this renderer draws on (rt_get_device)."""
        o = C.c_int32()
        pci = (C.c_int32 * 3)()
        check(lib().rt_get_device(self._h, C.byref(o), pci), "rt_get_device")
        return o.value, tuple(pci)

    @property
    def frame_count(self) -> int:
        v = C.c_uint32()
        check(lib().rt_get_frame_count(self._h, C.byref(v)), "frame_count")
        return v.value

    def draw(self) -> None:
        check(lib().rt_draw(self._h), "draw")

    def draw_frames(self, count: int, time0: int, dtime: int) -> None:
        check(lib().rt_draw_frames(self._h, count, time0, dtime), "draw_frames")

    def reset_frame_count(self) -> None:
        check(lib().rt_reset_frame_count(self._h), "reset_frame_count")

    def resize(self, width: int, height: int) -> None:
        check(lib().rt_resize(self._h, width, height), "resize")
        self.width, self.height = max(1, width), max(1, height)

    def release_scratch(self) -> None:
        """Free the sample queue's colour-fold memory (include/hrt.h rt_release_scratch)."""
        check(lib().rt_release_scratch(self._h), "release_scratch")

    def synchronize(self) -> None:
        check(lib().rt_synchronize(self._h), "synchronize")

    # --- buffers (write_buffer, renderer.rs:350-353)
    def write_spheres(self, spheres: np.ndarray) -> None:
        spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        check(lib().rt_set_spheres(self._h, spheres.tobytes(), len(spheres)), "write_buffer(spheres)")

    def write_bvh(self, sizes, nodes: np.ndarray, triangles: np.ndarray, materials: np.ndarray) -> None:
        sz = (C.c_uint32 * 2)(int(sizes[0]), int(sizes[1]))
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        triangles = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE)
        materials = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE)
        check(lib().rt_set_bvh(self._h, sz, nodes.ctypes.data, len(nodes), triangles.ctypes.data, len(triangles),
                               materials.ctypes.data, len(materials)), "write_buffer(bvh)")

    def set_triangles_device(self, tris, materials: np.ndarray, builder: int = 0) -> None:
        """rt_set_triangles_device_with: triangles from a contiguous torch tensor on the renderer's device, (m, 16) float32
        or (m, 64) uint8 in the layout of TRIANGLE_DTYPE, with a tree built for them on the GPU; materials as in write_bvh
        (numpy). builder: 0 (RT_TREE_LBVH, the default: the fast Morton-order build) or 1 (RT_TREE_PLOC: a slower build of
        a tree that is cheaper to walk). The renderer then has device geometry: every draw and query walks that tree
        (include/hrt.h). Synchronises torch's current stream before the call; the call itself is synchronous."""
        stream = self._check_device_triangles(tris, "set_triangles_device")
        materials = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE)
        stream.synchronize()
        check(lib().rt_set_triangles_device_with(self._h, C.c_void_p(tris.data_ptr()), int(tris.shape[0]),
                                                 materials.ctypes.data, len(materials), _builder(builder)),
              "set_triangles_device")

    def _check_device_triangles(self, tris, where: str):
        """The tensor checks of set_triangles_device / refit_triangles_device; returns torch's current stream on the
        renderer's device, for the caller to synchronise."""
        import torch

        dev = self._torch_device()
        if not torch.is_tensor(tris):
            raise TypeError(f"{where}: tris must be a torch tensor on the renderer's device")
        if tris.device != dev:
            raise ValueError(f"{where}: tris is on {tris.device}, the renderer draws on {dev}")
        if not ((tris.dtype == torch.float32 and tris.ndim == 2 and tris.shape[1] == 16) or
                (tris.dtype == torch.uint8 and tris.ndim == 2 and tris.shape[1] == 64)):
            raise ValueError(f"{where}: tris must be (m, 16) float32 or (m, 64) uint8, got "
                             f"{tuple(tris.shape)} {tris.dtype}")
        if not tris.is_contiguous():
            raise ValueError(f"{where}: tris must be contiguous")
        return torch.cuda.current_stream(dev)

    def refit_triangles_device(self, tris) -> None:
        """rt_refit_triangles_device: the moved positions of the mesh of the last set_triangles_device (same tensor
        layout, same count), on that build's topology: only the triangle records and the boxes are made again. Hits are
        bit for bit a fresh build's; the tree gets slower as the mesh leaves the built pose (tri_tree_cost()).
        Synchronises torch's current stream before the call; the call itself is synchronous."""
        stream = self._check_device_triangles(tris, "refit_triangles_device")
        stream.synchronize()
        check(lib().rt_refit_triangles_device(self._h, C.c_void_p(tris.data_ptr()), int(tris.shape[0])),
              "refit_triangles_device")

    def tri_tree_cost(self) -> np.ndarray:
        """rt_get_tri_tree_cost: four uint64 of the triangle tree the renderer walks (device geometry, or tri_bvh = 1):
        q of node children, q x count of leaf children (q: box half-area over the root's, x 65536), referenced nodes,
        leaf entries. (cost[0] + cost[1]) / 65536 is the usual SAH figure; hrt.lbvh_cost is the same on the host."""
        cost = (C.c_uint64 * 4)()
        check(lib().rt_get_tri_tree_cost(self._h, cost), "tri_tree_cost")
        return np.array(list(cost), dtype=np.uint64)

    def tri_tree_info(self) -> np.ndarray:
        """rt_get_tri_tree_info: eight uint32 of the triangle tree the renderer walks: builder (0 LBVH, 1 PLOC,
        0xFFFFFFFF the host SAH tree of tri_bvh = 1), node slots, finite triangles, root word, depth, PLOC iterations,
        flat ones among them, 0. RtError without a triangle tree."""
        info = (C.c_uint32 * 8)()
        check(lib().rt_get_tri_tree_info(self._h, info), "tri_tree_info")
        return np.array(list(info), dtype=np.uint32)

    def tri_tree(self) -> dict:
        """Test-only (include/hrt_testing.h rt_testing_get_tri_tree): the triangle tree the renderer walks, read back, in
        the format of hrt.lbvh_build."""
        h = self._h
        return _tree_dict(lambda *a: lib().rt_testing_get_tri_tree(h, *a), "testing_get_tri_tree")

    # --- knobs beyond the reference (WGSL compile-time constants there)
    @property
    def params(self) -> RtParams:
        p = RtParams()
        check(lib().rt_get_params(self._h, C.byref(p)), "get_params")
        return p

    def set_params(self, **kw) -> None:
        p = self.params
        names = {f[0] for f in RtParams._fields_}
        for k, v in kw.items():
            if k not in names:  # (a ctypes Structure would silently take an unknown attribute)
                raise TypeError(f"set_params: rt_params has no field {k!r}")
            setattr(p, k, v)
        check(lib().rt_set_params(self._h, C.byref(p)), "set_params")

    def set_faults(self, ring_slots_max: int = 0, fail_alloc_above_mb: int = 0) -> None:
        """Test-only fault injection (include/hrt_testing.h rt_testing_set_faults)."""
        check(lib().rt_testing_set_faults(self._h, ring_slots_max, fail_alloc_above_mb), "testing_set_faults")

    def tile_order(self) -> tuple[np.ndarray, np.ndarray]:
        """Test-only: what cost-ordered dealing has learnt, (per-tile cost sums, tile order), uint32[tiles] each
        (include/hrt_testing.h rt_testing_get_tile_order)."""
        n = C.c_size_t(0)
        check(lib().rt_testing_get_tile_order(self._h, None, None, 0, C.byref(n)), "testing_get_tile_order")
        sums, order = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(lib().rt_testing_get_tile_order(self._h, sums.ctypes.data_as(_lib._PU32), order.ctypes.data_as(_lib._PU32),
                                                  n.value, C.byref(n)), "testing_get_tile_order")
        return sums, order

    def set_tile_lists(self, mode: int = 0, k: int = 8) -> None:
        """Test-only: the per-tile primary candidate lists of k_trace_split, 0 auto, 1 off, 2 on, and the entries a list
        may hold (include/hrt_testing.h rt_testing_set_tile_lists)."""
        check(lib().rt_testing_set_tile_lists(self._h, mode, k), "testing_set_tile_lists")

    def tile_lists_resolved(self) -> int:
        """Test-only: the frame blocks of the last draw whose primary rays were answered when the block was made
        (include/hrt_testing.h rt_testing_get_tile_lists_resolved)."""
        n = C.c_uint64(0)
        check(lib().rt_testing_get_tile_lists_resolved(self._h, C.byref(n)), "testing_get_tile_lists_resolved")
        return int(n.value)

    def tile_lists(self) -> np.ndarray:
        """Test-only: the lists for the renderer's camera, spheres, size and row share, uint32[tiles, 9]: the count
        (0xFFFFFFFF: the tile walks), then the BVH codes (include/hrt_testing.h rt_testing_get_tile_lists)."""
        n = C.c_size_t(0)
        check(lib().rt_testing_get_tile_lists(self._h, None, 0, C.byref(n)), "testing_get_tile_lists")
        words = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(lib().rt_testing_get_tile_lists(self._h, words.ctypes.data_as(_lib._PU32), n.value, C.byref(n)),
                  "testing_get_tile_lists")
        return words.reshape(-1, 9)

    def set_descent_hold(self, hold: int) -> None:
        """Test-only: the descent hold of k_trace_split (include/hrt_testing.h rt_testing_set_descent_hold)."""
        check(lib().rt_testing_set_descent_hold(self._h, hold), "testing_set_descent_hold")

    @property
    def local_rows(self) -> int:
        from .parallel import local_rows

        p = self.params
        return local_rows(p.row0, p.row_step, self.height, p.row_block)

    def read_image(self) -> np.ndarray:
        """copy_image_buffer (render_ppm.rs:7-36): (local_rows, width, 3) float32."""
        out = np.empty((self.local_rows, self.width, 3), dtype=np.float32)
        check(lib().rt_read_image(self._h, out.ctypes.data_as(_lib._PF), out.size), "read_image")
        return out

    def write_image(self, img: np.ndarray) -> None:
        img = np.ascontiguousarray(img, dtype=np.float32)
        check(lib().rt_write_image(self._h, img.ctypes.data_as(_lib._PF), img.size), "write_image")

    def copy_image_to_device(self, dst_ptr: int, n_floats: int) -> None:
        check(lib().rt_copy_image_to_device(self._h, C.c_void_p(dst_ptr), n_floats), "copy_image_to_device")

    # --- ray queries (include/hrt.h rt_cast_rays / rt_primary_rays; torch is imported on first use)
    def _torch_device(self):
        import torch

        return torch.device("cuda", self.device()[0])

    def _f32_on_device(self, who: str, what: str, x, shape: tuple, coerce: bool = False, verb: str = "is"):
        """A numpy array or tensor as a contiguous float32 tensor of `shape` on the renderer's device (numpy arrays are
        uploaded). shape: None for an extent that is free (printed as N). coerce: a numpy array of another dtype is
        converted, not refused. who, what, verb: the calling method and the argument, for the messages."""
        import torch

        dev = self._torch_device()
        if not torch.is_tensor(x):
            x = np.asarray(x)
            if not coerce and x.dtype != np.float32:
                raise ValueError(f"{who}: {what} must be float32, got {x.dtype}")
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        if x.dtype != torch.float32 or x.ndim != len(shape) or any(s not in (None, e) for s, e in zip(shape, x.shape)):
            want = ", ".join("N" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "")
            raise ValueError(f"{who}: {what} must be ({want}) float32, got {tuple(x.shape)} {x.dtype}")
        if x.device != dev:
            raise ValueError(f"{who}: {what} {verb} on {x.device}, the renderer draws on {dev}")
        return x.contiguous()

    def _rays_on_device(self, who: str, a, what: str):
        """(N, 3) float32 rays as a contiguous tensor on the renderer's device. who: the calling method, for the messages."""
        return self._f32_on_device(who, what, a, (None, 3), coerce=True)

    def _cursor(self, who: str, after, dtype, n: int):
        """The cursors of a paged query, or None: an (n, 4) int32 tensor on the renderer's device, or n numpy records of
        `dtype`, as a contiguous tensor there."""
        import torch

        if after is None:
            return None
        dev = self._torch_device()
        cur = after
        if not torch.is_tensor(cur):
            cur = np.ascontiguousarray(cur, dtype=dtype).reshape(-1)
            cur = torch.from_numpy(cur.view(np.int32).reshape(-1, 4)).to(dev)
        if cur.dtype != torch.int32 or tuple(cur.shape) != (n, 4):
            raise ValueError(f"{who}: after must be ({n}, 4) int32 records, got {tuple(cur.shape)} {cur.dtype}")
        if cur.device != dev:
            raise ValueError(f"{who}: after is on {cur.device}, the renderer draws on {dev}")
        return cur.contiguous()

    @staticmethod
    def _k_counts(who: str, k, kmax: int, counts: bool) -> int:
        """k of a k-nearest query, checked: 0 .. kmax, and 0 only with counts."""
        k = int(k)
        if not 0 <= k <= kmax:
            raise ValueError(f"{who}: k must be 0 .. {kmax}, got {k}")
        if k == 0 and not counts:
            raise ValueError(f"{who}: k = 0 needs counts = True")
        return k

    def _set_testing_count(self, name: str, on: bool) -> None:
        check(getattr(lib(), f"rt_testing_set_{name}_count")(self._h, 1 if on else 0), f"testing_set_{name}_count")

    def _testing_counts(self, name: str, words: int) -> np.ndarray:
        c = (C.c_uint64 * words)()
        check(getattr(lib(), f"rt_testing_get_{name}_counts")(self._h, c), f"testing_get_{name}_counts")
        return np.array(list(c), dtype=np.uint64)

    def _ragged_pages(self, cnt, K: int, page):
        """The paging loop of all_hits and all_overlaps. cnt: the (n,) counts of a counting call; page(rows, cursor): the
        (len(rows), K, 4) int32 records of one more call over the queries `rows`. Returns (offsets, four columns): the
        first cnt[i] records of query i at [offsets[i], offsets[i + 1]), columns 0, 2, 3 as float32, 1 as int32."""
        import torch

        dev = self._torch_device()
        n = int(cnt.shape[0])
        cnt = cnt.to(torch.int64)
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=offsets[1:])
        total = int(offsets[-1].item()) if n else 0
        out = torch.empty((total, 4), dtype=torch.int32, device=dev)
        rows = torch.nonzero(cnt > 0).reshape(-1)
        done = torch.zeros((n,), dtype=torch.int64, device=dev)
        cursor = None
        rank = torch.arange(K, device=dev, dtype=torch.int64)
        while rows.numel():
            rec = page(rows, cursor)
            left = (cnt[rows] - done[rows]).clamp(max=K)
            take = rank[None, :] < left[:, None]
            dst = (offsets[rows] + done[rows])[:, None] + rank[None, :]
            out[dst[take]] = rec[take]
            done[rows] += left
            more = done[rows] < cnt[rows]
            cursor = rec[more][:, K - 1, :].contiguous()
            rows = rows[more]
        f = out.view(torch.float32)
        return offsets, f[:, 0].clone(), out[:, 1].clone(), f[:, 2].clone(), f[:, 3].clone()

    def _ray_pair(self, who: str, origins, dirs):
        """The rays of one query, checked: (origins, dirs, N), both (N, 3) float32 on the renderer's device."""
        o, d = self._rays_on_device(who, origins, "origins"), self._rays_on_device(who, dirs, "dirs")
        if o.shape != d.shape:
            raise ValueError(f"{who}: {tuple(o.shape)} origins for {tuple(d.shape)} directions")
        n = int(o.shape[0])
        if n >= 1 << 32:
            raise ValueError(f"{who}: at most 2^32 - 1 rays per call")
        return o, d, n

    def _rng_states(self, who: str, rng, n: int):
        """The caller's (n,) int32 / uint32 RNG states as a contiguous int32 tensor on the renderer's device."""
        import torch

        dev = self._torch_device()
        s = rng
        if not torch.is_tensor(s):
            s = np.asarray(s)
            if s.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
                raise ValueError(f"{who}: rng must be int32 or uint32, got {s.dtype}")
            s = torch.from_numpy(np.ascontiguousarray(s).view(np.int32)).to(dev)
        if s.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or tuple(s.shape) != (n,):
            raise ValueError(f"{who}: rng must be ({n},) int32, got {tuple(s.shape)} {s.dtype}")
        if s.device != dev:
            raise ValueError(f"{who}: rng is on {s.device}, the renderer draws on {dev}")
        return s.contiguous()

    def _query(self, who: str, fn, *args) -> None:
        """One call of a ray query: torch's current stream on the renderer's device is synchronised before it (the
        caller's tensors are complete) and the renderer after it (so are the results)."""
        import torch

        torch.cuda.current_stream(self._torch_device()).synchronize()
        check(fn(self._h, *args), who)
        self.synchronize()

    def stream(self) -> int:
        """The renderer's HIP stream as an integer handle (rt_get_stream), e.g. for torch.cuda.ExternalStream."""
        s = C.c_void_p()
        check(lib().rt_get_stream(self._h, C.byref(s)), "rt_get_stream")
        return int(s.value or 0)

    def cast_rays(self, origins, dirs) -> dict:
        """rt_cast_rays: the closest hit of each ray, as one bounce of the renderer's program would find it. origins and
        dirs: (N, 3) float32, torch tensors on the renderer's device or numpy arrays. Returns torch tensors on that
        device: t (N,) float32 (RT_T_MISS for a miss), prim (N,) int32 (-1 for a miss), normal (N, 3) float32, and
        flags (RT_HIT_FRONT | RT_HIT_TRIANGLE) and material as (N,) int32. Synchronises torch's current stream before
        the call and the renderer after it."""
        import torch

        o, d, n = self._ray_pair("cast_rays", origins, dirs)
        hits = torch.empty((n, HIT_DTYPE.itemsize // 4), dtype=torch.int32, device=self._torch_device())
        self._query("cast_rays", lib().rt_cast_rays, _ptr(o), _ptr(d), n, _ptr(hits))
        f = hits.view(torch.float32)
        return {"t": f[:, 0].clone(), "prim": hits[:, 1].clone(), "normal": f[:, 2:5].clone(),
                "flags": hits[:, 5].clone(), "material": hits[:, 6].clone()}

    def occluded(self, origins, dirs, tmax=None):
        """rt_occluded: for each ray, whether cast_rays would return a hit with t < tmax (an f32 comparison; a hit at
        exactly tmax does not occlude). origins and dirs as cast_rays; tmax is None (any hit at all), a Python float
        for every ray, or an (N,) float32 numpy array or tensor on the renderer's device. A segment from a to b is
        origins = a, dirs = b - a, tmax = 1. Returns a torch.bool tensor (N,) on the renderer's device. Synchronises
        torch's current stream before the call and the renderer after it."""
        import torch

        o, d, n = self._ray_pair("occluded", origins, dirs)
        t = self._per_ray_f32("occluded", "tmax", tmax, n)
        out = torch.empty((n,), dtype=torch.uint8, device=self._torch_device())
        self._query("occluded", lib().rt_occluded, _ptr(o), _ptr(d), _ptr(t), n, _ptr(out))
        return out != 0

    def closest_records(self, points, max_dist2=None):
        """rt_closest_points, the raw records: an (N, 8) int32 tensor on the renderer's device, one 32-byte rt_closest
        per point (CLOSEST_DTYPE on the host). points: (N, 3) float32, a torch tensor on the renderer's device or a
        numpy array; max_dist2: None (however far), a Python float for every point, or an (N,) float32 numpy array or
        tensor on the renderer's device — the squared search radius. Synchronises torch's current stream before the
        call and the renderer after it."""
        import torch

        who = "closest_points"
        pts = self._rays_on_device(who, points, "points")
        n = int(pts.shape[0])
        if n >= 1 << 32:
            raise ValueError(f"{who}: at most 2^32 - 1 points per call")
        cap = self._per_ray_f32(who, "max_dist2", max_dist2, n)
        out = torch.empty((n, CLOSEST_DTYPE.itemsize // 4), dtype=torch.int32, device=self._torch_device())
        self._query(who, lib().rt_closest_points, _ptr(pts), _ptr(cap), n, _ptr(out))
        return out

    def closest_points(self, points, max_dist2=None) -> dict:
        """rt_closest_points: the nearest point of the renderer's triangles for each point (triangle and mixed programs,
        with device geometry or tri_bvh = 1; the spheres of the mixed program do not answer). Arguments as
        closest_records. Returns torch tensors on the renderer's device: d2 (N,) float32, the squared distance (RT_T_MISS
        for a miss: nothing nearer than max_dist2, or a non-finite point), prim (N,) int32 (-1 for a miss), point (N, 3)
        float32, and v, w (N,) float32, the weights of the triangle's b and c (a's is 1 - v - w)."""
        import torch

        rec = self.closest_records(points, max_dist2)
        f = rec.view(torch.float32)
        return {"d2": f[:, 0].clone(), "prim": rec[:, 1].clone(), "point": f[:, 2:5].clone(), "v": f[:, 5].clone(),
                "w": f[:, 6].clone()}

    def set_closest_count(self, on: bool) -> None:
        """Test-only: closest_points runs the counting instantiation of its kernel (include/hrt_testing.h
        rt_testing_set_closest_count)."""
        self._set_testing_count("closest", on)

    def closest_counts(self) -> np.ndarray:
        """Test-only: uint64[4] of the last counted closest_points call: queries, point-triangle tests, stack overflows,
        points outside the walk's error bound (include/hrt_testing.h rt_testing_get_closest_counts)."""
        return self._testing_counts("closest", 4)

    def _per_ray_f32(self, who: str, what: str, x, n: int):
        """An optional per-ray float: None, a Python float for every ray, or an (n,) float32 numpy array or tensor on the
        renderer's device, as a contiguous tensor there (or None)."""
        import torch

        if x is None:
            return None
        if isinstance(x, (int, float)):
            return torch.full((n,), float(x), dtype=torch.float32, device=self._torch_device())
        return self._f32_on_device(who, what, x, (n,))

    def cast_rays_multi_records(self, origins, dirs, k: int, tmax=None, after=None, counts: bool = False):
        """rt_cast_rays_multi, the raw records: an (N, k, 4) int32 tensor on the renderer's device, one 16-byte
        rt_multi_hit per ray and rank (MULTI_HIT_DTYPE on the host), and the (N,) int32 counts or None. origins, dirs,
        tmax as occluded; after: None, or the cursors as an (N, 4) int32 tensor on the renderer's device (one record per
        ray, e.g. records[:, -1]) or N MULTI_HIT_DTYPE numpy records. Synchronises torch's current stream before the call
        and the renderer after it."""
        import torch

        who = "cast_rays_multi"
        o, d, n = self._ray_pair(who, origins, dirs)
        k = self._k_counts(who, k, MULTI_HIT_MAX_K, counts)
        dev = self._torch_device()
        cap = self._per_ray_f32(who, "tmax", tmax, n)
        cur = self._cursor(who, after, MULTI_HIT_DTYPE, n)
        hits = torch.empty((n, k, 4), dtype=torch.int32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev) if counts else None
        self._query(who, lib().rt_cast_rays_multi, _ptr(o), _ptr(d), _ptr(cap), _ptr(cur), n, k, _ptr(hits) if k else None,
                    _ptr(cnt))
        return hits, cnt

    def cast_rays_multi(self, origins, dirs, k: int, tmax=None, after=None, counts: bool = False) -> dict:
        """rt_cast_rays_multi: the k nearest triangles each ray passes through, in (t, prim) order — two triangles at the
        same t are both listed — on the renderer's triangle tree (triangle and mixed programs, with device geometry or
        tri_bvh = 1; the spheres of the mixed program do not answer). k: 0 .. 16; tmax as occluded (hits at t >= tmax are
        left out); after: a cursor per ray, see cast_rays_multi_records — with each ray's last record of one call the next
        call returns the next k hits. Returns torch tensors on the renderer's device: t (N, k) float32 (RT_T_MISS for an
        unused rank), prim (N, k) int32 (-1 there), u, v (N, k) float32, records (N, k, 4) int32 (the raw records), and
        with counts = True count (N,) int32, the number of all hits under tmax and beyond the cursor, not capped by k."""
        import torch

        rec, cnt = self.cast_rays_multi_records(origins, dirs, k, tmax, after, counts)
        f = rec.view(torch.float32)
        out = {"t": f[:, :, 0].clone(), "prim": rec[:, :, 1].clone(), "u": f[:, :, 2].clone(), "v": f[:, :, 3].clone(),
               "records": rec}
        if counts:
            out["count"] = cnt
        return out

    def all_hits(self, origins, dirs, tmax=None):
        """Every hit of every ray, ragged: one counting call (k = 0), then pages of 16 by cursor over the rays that still
        have hits left. Returns (offsets, t, prim, u, v) on the renderer's device: offsets (N + 1,) int64, ray i's hits at
        [offsets[i], offsets[i + 1]) of t (float32), prim (int32), u, v (float32), in (t, prim) order."""
        who = "all_hits"
        o, d, n = self._ray_pair(who, origins, dirs)
        cap = self._per_ray_f32(who, "tmax", tmax, n)
        _, cnt = self.cast_rays_multi_records(o, d, 0, cap, None, True)
        K = MULTI_HIT_MAX_K
        return self._ragged_pages(cnt, K, lambda rays, cursor: self.cast_rays_multi_records(
            o[rays], d[rays], K, None if cap is None else cap[rays], cursor, False)[0])

    def set_multihit_count(self, on: bool) -> None:
        """Test-only: cast_rays_multi runs the counting instantiation of its kernel (include/hrt_testing.h
        rt_testing_set_multihit_count)."""
        self._set_testing_count("multihit", on)

    def multihit_counts(self) -> np.ndarray:
        """Test-only: uint64[4] of the last counted cast_rays_multi call: queries, triangle tests, box tests, stack
        overflows (include/hrt_testing.h rt_testing_get_multihit_counts)."""
        return self._testing_counts("multihit", 4)

    def overlap_records(self, kind: int, volumes, k: int, after=None, counts: bool = False):
        """rt_overlap_volumes, the raw records: an (N, k, 4) int32 tensor on the renderer's device, one 16-byte
        rt_overlap_hit per query and rank (OVERLAP_HIT_DTYPE on the host), and the (N,) int32 counts or None. kind:
        VOLUME_BOX (volumes (N, 6) float32: lo xyz, hi xyz) or VOLUME_BALL ((N, 4) float32: centre xyz, squared radius),
        a torch tensor on the renderer's device or a numpy array; after: None, or the cursors as an (N, 4) int32 tensor on
        the renderer's device (one record per query, e.g. records[:, -1]) or N OVERLAP_HIT_DTYPE numpy records.
        Synchronises torch's current stream before the call and the renderer after it."""
        import torch

        who = "overlap_volumes"
        if kind not in _VOLUME_FLOATS:
            raise ValueError(f"{who}: kind must be VOLUME_BOX or VOLUME_BALL, got {kind}")
        width = _VOLUME_FLOATS[kind]
        dev = self._torch_device()
        vol = self._f32_on_device(who, "volumes", volumes, (None, width), verb="are")
        n = int(vol.shape[0])
        if n >= 1 << 32:
            raise ValueError(f"{who}: at most 2^32 - 1 queries per call")
        k = self._k_counts(who, k, OVERLAP_MAX_K, counts)
        cur = self._cursor(who, after, OVERLAP_HIT_DTYPE, n)
        hits = torch.empty((n, k, 4), dtype=torch.int32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev) if counts else None
        self._query(who, lib().rt_overlap_volumes, kind, _ptr(vol), _ptr(cur), n, k, _ptr(hits) if k else None, _ptr(cnt))
        return hits, cnt

    def _overlap_dict(self, rec, cnt, counts: bool) -> dict:
        import torch

        f = rec.view(torch.float32)
        out = {"d2": f[:, :, 0].clone(), "prim": rec[:, :, 1].clone(), "v": f[:, :, 2].clone(), "w": f[:, :, 3].clone(),
               "records": rec}
        if counts:
            out["count"] = cnt
        return out

    def overlap_boxes(self, lo, hi, k: int, after=None, counts: bool = False) -> dict:
        """rt_overlap_volumes, RT_VOLUME_BOX: the triangles that touch each axis-aligned box [lo, hi] (touching counts),
        the k of smallest index, in index order, on the renderer's triangle tree (triangle and mixed programs, with device
        geometry or tri_bvh = 1; the spheres of the mixed program do not answer). lo, hi: (N, 3) float32, torch tensors on
        the renderer's device or numpy arrays; k: 0 .. 16; after: a cursor per box, see overlap_records. Returns torch
        tensors on the renderer's device: prim (N, k) int32 (-1 for an unused rank), d2 (N, k) float32 (0 for a hit,
        RT_T_MISS for an unused rank), v, w (N, k) float32 (0), records (N, k, 4) int32 (the raw records), and with
        counts = True count (N,) int32, the number of all such triangles beyond the cursor, not capped by k."""
        import torch

        lo_t = self._rays_on_device("overlap_boxes", lo, "lo")
        hi_t = self._rays_on_device("overlap_boxes", hi, "hi")
        if lo_t.shape != hi_t.shape:
            raise ValueError(f"overlap_boxes: {tuple(lo_t.shape)} lo for {tuple(hi_t.shape)} hi")
        rec, cnt = self.overlap_records(VOLUME_BOX, torch.cat([lo_t, hi_t], dim=1), k, after, counts)
        return self._overlap_dict(rec, cnt, counts)

    def nearest_triangles(self, points, k: int, max_dist2=None, after=None, counts: bool = False) -> dict:
        """rt_overlap_volumes, RT_VOLUME_BALL: the k nearest triangles of each point, in (d2, prim) order, on the
        renderer's triangle tree. points: (N, 3) float32; max_dist2 as closest_points (None: however far; a triangle at
        exactly max_dist2 does not count); after: a cursor per point, see overlap_records. Returns torch tensors on the
        renderer's device: d2 (N, k) float32 (RT_T_MISS for an unused rank), prim (N, k) int32 (-1 there), v, w (N, k)
        float32 (the weights of the triangle's b and c at its nearest point), records (N, k, 4) int32, and with counts =
        True count (N,) int32, the number of all triangles nearer than max_dist2 and beyond the cursor."""
        import torch

        who = "nearest_triangles"
        pts = self._rays_on_device(who, points, "points")
        n = int(pts.shape[0])
        cap = self._per_ray_f32(who, "max_dist2", max_dist2, n)
        if cap is None:
            cap = torch.full((n,), _lib.RT_T_MISS, dtype=torch.float32, device=pts.device)
        rec, cnt = self.overlap_records(VOLUME_BALL, torch.cat([pts, cap[:, None]], dim=1), k, after, counts)
        return self._overlap_dict(rec, cnt, counts)

    def all_overlaps(self, kind: int, volumes):
        """Every triangle of every volume, ragged: one counting call (k = 0), then pages of 16 by cursor over the queries
        that still have triangles left. Returns (offsets, d2, prim, v, w) on the renderer's device: offsets (N + 1,)
        int64, query i's triangles at [offsets[i], offsets[i + 1]) of d2 (float32), prim (int32), v, w (float32), in index
        order (boxes) or (d2, prim) order (balls)."""
        import torch

        dev = self._torch_device()
        vol = volumes if torch.is_tensor(volumes) else torch.from_numpy(np.ascontiguousarray(volumes)).to(dev)
        _, cnt = self.overlap_records(kind, vol, 0, None, True)
        K = OVERLAP_MAX_K
        return self._ragged_pages(cnt, K, lambda rows, cursor: self.overlap_records(kind, vol[rows], K, cursor, False)[0])

    def set_overlap_count(self, on: bool) -> None:
        """Test-only: overlap_records runs the counting instantiation of its kernel (include/hrt_testing.h
        rt_testing_set_overlap_count)."""
        self._set_testing_count("overlap", on)

    def overlap_counts(self) -> np.ndarray:
        """Test-only: uint64[4] of the last counted overlap_records call: queries, triangle tests, box tests, stack
        overflows (include/hrt_testing.h rt_testing_get_overlap_counts)."""
        return self._testing_counts("overlap", 4)

    def winding_numbers(self, points, beta: float = 0.0):
        """rt_winding_numbers: the generalized winding number of the renderer's triangles at each point (triangle and
        mixed programs, with device geometry or tri_bvh = 1; the spheres of the mixed program do not answer): 1 inside a
        closed mesh wound outward, 0 outside, in between where the mesh is open. points as closest_points; beta: the
        far-field factor (0 = the default 2.0, at least 1 otherwise, float("inf") sums every triangle exactly). Returns
        an (N,) float32 tensor on the renderer's device; a non-finite point gives NaN."""
        import torch

        who = "winding_numbers"
        pts = self._rays_on_device(who, points, "points")
        n = int(pts.shape[0])
        if n >= 1 << 32:
            raise ValueError(f"{who}: at most 2^32 - 1 points per call")
        out = torch.empty((n,), dtype=torch.float32, device=self._torch_device())
        self._query(who, lib().rt_winding_numbers, _ptr(pts), n, C.c_float(beta), _ptr(out))
        return out

    def signed_distance(self, points, beta: float = 0.0) -> dict:
        """closest_points and winding_numbers on the same points, composed with torch ops: the fields of closest_points,
        winding (the raw w), inside = |w| >= 0.5 (|w|, so that a mesh wound inward works too) and distance = sqrt(d2),
        negative where inside is true."""
        import torch

        pts = self._rays_on_device("signed_distance", points, "points")
        out = self.closest_points(pts)
        w = self.winding_numbers(pts, beta)
        inside = w.abs() >= 0.5
        dist = torch.sqrt(out["d2"])
        out.update(winding=w, inside=inside, distance=torch.where(inside, -dist, dist))
        return out

    def set_winding_count(self, on: bool) -> None:
        """Test-only: winding_numbers runs the counting instantiation of its kernel (include/hrt_testing.h
        rt_testing_set_winding_count)."""
        self._set_testing_count("winding", on)

    def winding_counts(self) -> np.ndarray:
        """Test-only: uint64[5] of the last counted winding_numbers call: queries, triangle terms, dipole terms, stack
        overflows, uncovered points (include/hrt_testing.h rt_testing_get_winding_counts)."""
        return self._testing_counts("winding", 5)

    def tree_moments(self) -> np.ndarray:
        """Test-only (include/hrt_testing.h rt_testing_get_tree_moments): the moments winding_numbers reads, (node slots,
        16) float32, made first if the tree changed since."""
        n = C.c_size_t(0)
        check(lib().rt_testing_get_tree_moments(self._h, None, 0, C.byref(n)), "testing_get_tree_moments")
        out = np.zeros((int(n.value), 16), dtype=np.float32)
        if out.size:
            check(lib().rt_testing_get_tree_moments(self._h, out.ctypes.data, len(out), C.byref(n)), "testing_get_tree_moments")
        return out

    def primary_rays(self, time: int):
        """rt_primary_rays: (origins, dirs), each (local_rows, width, 3) float32 on the renderer's device — the rays the
        frame drawn at `time` traces first for each of this renderer's pixels."""
        import torch

        dev = self._torch_device()
        shape = (self.local_rows, self.width, 3)
        o = torch.empty(shape, dtype=torch.float32, device=dev)
        d = torch.empty(shape, dtype=torch.float32, device=dev)
        self._query("primary_rays", lib().rt_primary_rays, int(time) & 0xFFFFFFFF, _ptr(o), _ptr(d), shape[0] * shape[1])
        return o, d

    def first_hit(self, time: int) -> dict:
        """The first hit behind each pixel sample of the frame drawn at `time` (depth, normal, primitive and material
        guide buffers): cast_rays on primary_rays, shaped (local_rows, width[, 3])."""
        o, d = self.primary_rays(time)
        hit = self.cast_rays(o.view(-1, 3), d.view(-1, 3))
        return {k: v.view(*o.shape[:2], *v.shape[1:]) for k, v in hit.items()}

    def trace_rays(self, origins, dirs, rng=None, seed: int = 0, want_queries: bool = False):
        """rt_trace_rays: the path-traced radiance of each ray, trace() of the renderer's program with rt_params.bounces
        bounces. origins and dirs as cast_rays; rng is None (ray i starts from the state (i + 1) * seed mod 2^32) or the
        (N,) int32 / uint32 states, a numpy array or a tensor on the renderer's device (int32 holds the same 32 bits).
        Returns (N, 3) float32 radiance on the renderer's device and, with want_queries, also the (N,) int32 number of
        closest-hit queries each path took. Synchronises torch's current stream before the call and the renderer after
        it."""
        import torch

        o, d, n = self._ray_pair("trace_rays", origins, dirs)
        dev = self._torch_device()
        s = self._rng_states("trace_rays", rng, n) if rng is not None else None
        rad = torch.empty((n, 3), dtype=torch.float32, device=dev)
        q = torch.empty((n,), dtype=torch.int32, device=dev) if want_queries else None
        self._query("trace_rays", lib().rt_trace_rays, _ptr(o), _ptr(d), _ptr(s), int(seed) & 0xFFFFFFFF, n, _ptr(rad), _ptr(q))
        return (rad, q) if want_queries else rad

    def primary_rng(self, time: int):
        """rt_primary_rng: (local_rows, width) int32 on the renderer's device — the RNG state fs_main holds after
        make_ray for each of this renderer's pixels in the frame drawn at `time` (the 32 bits of the u32 state)."""
        import torch

        dev = self._torch_device()
        shape = (self.local_rows, self.width)
        s = torch.empty(shape, dtype=torch.int32, device=dev)
        self._query("primary_rng", lib().rt_primary_rng, int(time) & 0xFFFFFFFF, _ptr(s), shape[0] * shape[1])
        return s

    def trace_frame(self, time: int, want_queries: bool = False):
        """The radiance of each pixel sample of the frame drawn at `time`: trace_rays on primary_rays and primary_rng,
        shaped (local_rows, width, 3) — bit for bit the image a one-frame draw at that time leaves from frame count 0.
        With want_queries also the (local_rows, width) queries. The counterpart of first_hit."""
        o, d = self.primary_rays(time)
        s = self.primary_rng(time)
        out = self.trace_rays(o.view(-1, 3), d.view(-1, 3), rng=s.view(-1), want_queries=want_queries)
        if want_queries:
            return out[0].view(*o.shape), out[1].view(*o.shape[:2])
        return out.view(*o.shape)

    def _bounce_buffer(self, t, name: str, shape, dtypes, optional: bool = False, who: str = "bounce_rays"):
        """A caller's state tensor of bounce_rays (or of `who`, for the messages), checked: it is used in place, so nothing
        is converted or copied."""
        import torch

        if t is None:
            if optional:
                return None
            raise ValueError(f"{who}: {name} is required")
        dev = self._torch_device()
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a torch tensor on {dev} (it is used in place)")
        if t.dtype not in dtypes or (shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError(f"{who}: {name} must be {tuple(shape) if shape is not None else '(n,)'} "
                             f"{dtypes[0]}, got {tuple(t.shape)} {t.dtype}")
        if t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, the renderer draws on {dev}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous (it is used in place)")
        return t

    def bounce_rays(self, origins, dirs, rng, throughput=None, queries=None, hits=None, index_in=None, count_in=None,
                    index_out=None, count_out=None, n=None) -> None:
        """rt_bounce_rays: one step of trace()'s loop, IN PLACE on the caller's torch tensors on the renderer's device.
        origins, dirs: (paths, 3) float32; rng: (paths,) int32 (the 32 bits of the u32 state); throughput: (paths, 3)
        float32; queries: (paths,) int32; hits: (paths, 8) int32 (the 32-byte rt_hit records, as cast_rays reads them);
        index_in: (n,) int32 path indices (None: path i is entry i, n = paths); count_in / count_out: (1,) int32;
        index_out: int32 with room for n entries. A path that hits gets its next ray, RNG state and throughput and is
        appended to index_out; a path that misses is left untouched (include/hrt.h rt_bounce has the whole contract).
        n (default: len(index_in), or paths) is the number of entries. Synchronises torch's current stream before the
        call and the renderer after it."""
        import torch

        i32 = (torch.int32, getattr(torch, "uint32", torch.int32))
        f32 = (torch.float32,)
        o = self._bounce_buffer(origins, "origins", None, f32)
        if o.ndim != 2 or o.shape[1] != 3:
            raise ValueError(f"bounce_rays: origins must be (paths, 3) float32, got {tuple(o.shape)}")
        paths = int(o.shape[0])
        if paths >= 1 << 32:
            raise ValueError("bounce_rays: at most 2^32 - 1 paths")
        d = self._bounce_buffer(dirs, "dirs", (paths, 3), f32)
        s = self._bounce_buffer(rng, "rng", (paths,), i32)
        tp = self._bounce_buffer(throughput, "throughput", (paths, 3), f32, optional=True)
        q = self._bounce_buffer(queries, "queries", (paths,), i32, optional=True)
        h = self._bounce_buffer(hits, "hits", (paths, HIT_DTYPE.itemsize // 4), i32, optional=True)
        ii = self._bounce_buffer(index_in, "index_in", None, i32, optional=True)
        if ii is not None and ii.ndim != 1:
            raise ValueError(f"bounce_rays: index_in must be (n,) int32, got {tuple(ii.shape)}")
        if n is None:
            n = int(ii.shape[0]) if ii is not None else paths
        n = int(n)
        if n < 0 or n >= 1 << 32 or (ii is not None and n > int(ii.shape[0])):
            raise ValueError(f"bounce_rays: n = {n} entries for an index_in of "
                             f"{int(ii.shape[0]) if ii is not None else paths}")
        ci = self._bounce_buffer(count_in, "count_in", (1,), i32, optional=True)
        io = self._bounce_buffer(index_out, "index_out", None, i32, optional=True)
        if io is not None and (io.ndim != 1 or int(io.shape[0]) < n):
            raise ValueError(f"bounce_rays: index_out must have room for {n} int32, got {tuple(io.shape)}")
        co = self._bounce_buffer(count_out, "count_out", (1,), i32, optional=True)
        b = _lib.RtBounce(_ptr(o), _ptr(d), _ptr(s), _ptr(tp), _ptr(q), _ptr(h), _ptr(ii), _ptr(ci), _ptr(io), _ptr(co), paths, 0)
        self._query("bounce_rays", lib().rt_bounce_rays, C.byref(b), n)

    def regroup_paths(self, index_out, origins=None, dirs=None, keys=None, box=None, index_in=None, count_in=None,
                      keys_out=None, n=None, paths=None) -> None:
        """rt_regroup_paths: sort a path index list by a coherence key, IN PLACE on the caller's torch tensors on the
        renderer's device (include/hrt.h rt_regroup has the whole contract). Exactly one of
          box=(lo, hi): the 24-bit cell-and-octant key of each path's ray, from origins and dirs ((paths, 3) float32) and
                        the box the origins are quantised in (hrt.regroup_keys gives the same keys on the host);
          keys:         (paths,) int32, the caller's own 32-bit keys, indexed by path.
        index_in: (n,) int32 path indices (None: entry i is path i); count_in: (1,) int32, only the first
        min(n, count_in) entries are sorted; index_out: int32 with room for n entries — index_in itself for a sort in
        place; keys_out: int32 with room for n, the key of each output entry. The sort is stable. n (default:
        len(index_in), or paths) is the number of entries; paths (default: the rows of origins or keys) the number of
        paths behind the indices. Synchronises torch's current stream before the call and the renderer after it."""
        import torch

        who = "regroup_paths"
        i32 = (torch.int32, getattr(torch, "uint32", torch.int32))
        f32 = (torch.float32,)
        if (box is None) == (keys is None):
            raise ValueError("regroup_paths: give exactly one of box=(lo, hi) (with origins and dirs) and keys")
        o = d = kk = None
        lo = hi = (0.0, 0.0, 0.0)
        if box is not None:
            lo, hi = (tuple(float(x) for x in b) for b in box)
            if len(lo) != 3 or len(hi) != 3:
                raise ValueError("regroup_paths: box must be ((x, y, z), (x, y, z))")
            o = self._bounce_buffer(origins, "origins", None, f32, who=who)
            if o.ndim != 2 or o.shape[1] != 3:
                raise ValueError(f"regroup_paths: origins must be (paths, 3) float32, got {tuple(o.shape)}")
            d = self._bounce_buffer(dirs, "dirs", tuple(o.shape), f32, who=who)
            rows = int(o.shape[0])
        else:
            kk = self._bounce_buffer(keys, "keys", None, i32, who=who)
            if kk.ndim != 1:
                raise ValueError(f"regroup_paths: keys must be (paths,) int32, got {tuple(kk.shape)}")
            rows = int(kk.shape[0])
        paths = rows if paths is None else int(paths)
        if paths < 0 or paths > rows:
            raise ValueError(f"regroup_paths: paths = {paths} for state arrays of {rows} rows")
        ii = self._bounce_buffer(index_in, "index_in", None, i32, optional=True, who=who)
        if ii is not None and ii.ndim != 1:
            raise ValueError(f"regroup_paths: index_in must be (n,) int32, got {tuple(ii.shape)}")
        if n is None:
            n = int(ii.shape[0]) if ii is not None else paths
        n = int(n)
        if n < 0 or n >= 1 << 32 or (ii is not None and n > int(ii.shape[0])):
            raise ValueError(f"regroup_paths: n = {n} entries for an index_in of "
                             f"{int(ii.shape[0]) if ii is not None else paths}")
        ci = self._bounce_buffer(count_in, "count_in", (1,), i32, optional=True, who=who)
        io = self._bounce_buffer(index_out, "index_out", None, i32, who=who)
        if io.ndim != 1 or int(io.shape[0]) < n:
            raise ValueError(f"regroup_paths: index_out must have room for {n} int32, got {tuple(io.shape)}")
        ko = self._bounce_buffer(keys_out, "keys_out", None, i32, optional=True, who=who)
        if ko is not None and (ko.ndim != 1 or int(ko.shape[0]) < n):
            raise ValueError(f"regroup_paths: keys_out must have room for {n} int32, got {tuple(ko.shape)}")
        g = _lib.RtRegroup(_ptr(o), _ptr(d), _ptr(kk), _ptr(ii), _ptr(ci), _ptr(io), _ptr(ko), paths,
                           _lib.REGROUP_CELL_OCTANT if box is not None else _lib.REGROUP_KEYS,
                           (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), 0, 0)
        self._query("regroup_paths", lib().rt_regroup_paths, C.byref(g), n)

    def trace_wavefront(self, origins, dirs, rng, bounces: int, want_queries: bool = False, regroup_box=None,
                        regroup_after=()):
        """The wavefront form of trace_rays: `bounces` bounce_rays steps on copies of the given rays and states, the
        survivors of each step handed to the next through two (index, count) pairs with no host read-back in between,
        then 0.0 + throughput * sky with the sky of the GIVEN rays' d.y. Bit for bit trace_rays' radiance (and queries)
        for rt_params.bounces = `bounces`. Returns (N, 3) float32 and, with want_queries, the (N,) int32 queries.
        regroup_box=(lo, hi) with regroup_after, the 1-based steps after which the survivors' list is regrouped in place
        (regroup_paths by the cell-and-octant key, index_out = index_in, the step's own count buffer): the order of the
        list changes, the result does not."""
        import torch

        o, d, n = self._ray_pair("trace_wavefront", origins, dirs)
        o, d = o.clone(), d.clone()
        dev = self._torch_device()
        s = self._rng_states("trace_wavefront", rng, n).clone()
        # the sky blend of trace()'s epilogue, one rounded f32 operation per operation of the kernels' expression
        t = d[:, 1] * 0.5 + 0.5
        u = 1.0 - t
        sky = torch.stack((0.54 * u + 0.54 * t, 0.86 * u + 0.7 * t, 0.92 * u + 0.98 * t), dim=1)
        att = torch.ones((n, 3), dtype=torch.float32, device=dev)
        q = torch.zeros((n,), dtype=torch.int32, device=dev) if want_queries else None
        index = [torch.empty((max(n, 1),), dtype=torch.int32, device=dev) for _ in range(2)]
        count = [torch.zeros((1,), dtype=torch.int32, device=dev) for _ in range(2)]
        regroup_after = frozenset(int(k) for k in regroup_after)
        if regroup_after and regroup_box is None:
            raise ValueError("trace_wavefront: regroup_after needs regroup_box=(lo, hi)")
        if n > 0:
            for k in range(int(bounces)):
                src, dst = (k + 1) & 1, k & 1
                self.bounce_rays(o, d, s, throughput=att, queries=q,
                                 index_in=index[src] if k else None, count_in=count[src] if k else None,
                                 index_out=index[dst], count_out=count[dst], n=n)
                if k + 1 in regroup_after:
                    self.regroup_paths(index[dst], origins=o, dirs=d, box=regroup_box, index_in=index[dst],
                                       count_in=count[dst], n=n)
        rad = 0.0 + att * sky
        return (rad, q) if want_queries else rad

    def set_trace_rays_per_lane(self, rays_per_lane: int) -> None:
        """Test-only: k_radiance_rays' rays per lane, 0 = the host's rule (include/hrt_testing.h)."""
        check(lib().rt_testing_set_trace_rays_per_lane(self._h, rays_per_lane), "testing_set_trace_rays_per_lane")

    def stats(self) -> RtStats:
        s = RtStats()
        check(lib().rt_get_stats(self._h, C.byref(s)), "get_stats")
        return s

    def raw_counters(self, n: int = 16) -> list:
        """Device counters of the last draw (include/hrt.h rt_get_raw_counters; slots 8-11 are
        region cycle sums in the diagnostic build)."""
        buf = (C.c_uint64 * n)()
        check(lib().rt_get_raw_counters(self._h, buf, n), "get_raw_counters")
        return list(buf)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _tree_dict(call, where: str) -> dict:
    """The two-call protocol of rt_host_lbvh_build / rt_testing_get_tri_tree (sizes, then the arrays)."""
    info, root = (C.c_uint32 * 8)(), (C.c_float * 4)()
    check(call(None, 0, None, 0, info, root), where)
    nodes = np.zeros((int(info[0]), 8), dtype=np.uint32)
    order = np.zeros((int(info[1]),), dtype=np.uint32)
    if nodes.size or order.size:
        check(call(nodes.ctypes.data if nodes.size else None, len(nodes),
                   order.ctypes.data_as(_lib._PU32) if order.size else None, len(order), info, root), where)
    return {"nodes": nodes, "order": order, "info": np.array(list(info), dtype=np.uint32),
            "root": np.array(list(root), dtype=np.float32)}


def _builder(builder) -> int:
    """A builder argument as the uint32 the library takes (which refuses the unknown ones)."""
    b = int(builder)
    if not 0 <= b <= 0xFFFFFFFF:
        raise ValueError(f"builder must be 0 (LBVH) or 1 (PLOC), got {builder!r}")
    return b


def lbvh_build(triangles: np.ndarray, builder: int = 0) -> dict:
    """rt_host_lbvh_build_with (include/hrt.h): rt_set_triangles_device's builders on the host, no device. triangles:
    TRIANGLE_DTYPE records (or (m, 16) float32); builder: 0 (LBVH) or 1 (PLOC). Returns nodes (slots, 8) uint32 — per
    child [min | max << 16] fp16 bounds per axis relative to the root centre, then the child word —, order (the finite
    triangles' indices in key order), info {node slots, leaf positions, finite triangles, root word, depth, PLOC's
    iterations, the flat ones among them, 0} and root (centre xyz, radius)."""
    t = np.ascontiguousarray(triangles)
    if t.dtype != TRIANGLE_DTYPE:
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 16)
    m, p, b = len(t), t.ctypes.data, _builder(builder)
    return _tree_dict(lambda *a: lib().rt_host_lbvh_build_with(p if m else None, m, b, *a), "rt_host_lbvh_build")


def _triangle_records(triangles: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(triangles)
    if t.dtype != TRIANGLE_DTYPE:
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 16)
    return t


def lbvh_refit(topology_triangles: np.ndarray, triangles: np.ndarray, builder: int = 0) -> dict:
    """rt_host_lbvh_refit_with (include/hrt.h): rt_refit_triangles_device on the host, no device. The tree has the
    topology lbvh_build(topology_triangles, builder) has and the boxes of triangles (the same count; a triangle finite in
    one array and not in the other is an RtError). The dict is lbvh_build's."""
    a, b = _triangle_records(topology_triangles), _triangle_records(triangles)
    if len(a) != len(b):
        raise ValueError(f"lbvh_refit: {len(a)} triangles for the topology, {len(b)} to fit")
    m, pa, pb, bld = len(a), a.ctypes.data, b.ctypes.data, _builder(builder)
    return _tree_dict(lambda *x: lib().rt_host_lbvh_refit_with(pa if m else None, pb if m else None, m, bld, *x),
                      "rt_host_lbvh_refit")


def lbvh_cost(tree: dict) -> np.ndarray:
    """rt_host_lbvh_cost (include/hrt.h): the four uint64 cost words of a tree dict (lbvh_build, lbvh_refit,
    Renderer.tri_tree): a pure function of the node bytes and the root word. Renderer.tri_tree_cost is the same on the
    device."""
    nodes = np.ascontiguousarray(tree["nodes"], dtype=np.uint32).reshape(-1, 8)
    cost = (C.c_uint64 * 4)()
    check(lib().rt_host_lbvh_cost(nodes.ctypes.data if len(nodes) else None, len(nodes), int(tree["info"][3]), cost),
          "rt_host_lbvh_cost")
    return np.array(list(cost), dtype=np.uint64)


def closest_points_host(triangles: np.ndarray, points: np.ndarray, max_dist2=None) -> np.ndarray:
    """rt_host_closest_points (include/hrt.h): the definition of Renderer.closest_points as a loop over every triangle, on
    the host, no device. triangles: TRIANGLE_DTYPE records (or (m, 16) float32); points: (n, 3) float32; max_dist2: None,
    a float for every point, or (n,) float32. Returns n CLOSEST_DTYPE records: the bytes the device writes."""
    t = _triangle_records(triangles)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n, m = len(p), len(t)
    cap = None
    if max_dist2 is not None:
        cap = (np.full((n,), max_dist2, dtype=np.float32) if isinstance(max_dist2, (int, float))
               else np.ascontiguousarray(max_dist2, dtype=np.float32))
        if cap.shape != (n,):
            raise ValueError(f"closest_points_host: max_dist2 must be ({n},) float32, got {cap.shape}")
    out = np.zeros((n,), dtype=CLOSEST_DTYPE)
    check(lib().rt_host_closest_points(t.ctypes.data if m else None, m, p.ctypes.data_as(_lib._PF) if n else None,
                                       cap.ctypes.data_as(_lib._PF) if cap is not None and n else None, n,
                                       out.ctypes.data if n else None), "rt_host_closest_points")
    return out


def _tree_args(triangles, tree, flat: bool = False):
    """(triangles, m, nodes, slots, order, n_order, root word, root) as the host mirrors take them; tree: a dict of
    lbvh_build / lbvh_refit / Renderer.tri_tree, or None for the flat definition without a root. flat: the flat definition
    with the tree's root (centre, radius): no nodes, no order, a leaf root word."""
    t = _triangle_records(triangles)
    m = len(t)
    nodes, order, word = np.zeros((0, 8), dtype=np.uint32), np.zeros((0,), dtype=np.uint32), 0x80000000
    root = np.zeros((4,), dtype=np.float32) if tree is None else np.ascontiguousarray(tree["root"], dtype=np.float32)
    if tree is not None and not flat:
        nodes = np.ascontiguousarray(tree["nodes"], dtype=np.uint32).reshape(-1, 8)
        order = np.ascontiguousarray(tree["order"], dtype=np.uint32)
        word = int(tree["info"][3])
    keep = (t, nodes, order, root)
    return keep, (t.ctypes.data if m else None, m, nodes.ctypes.data if len(nodes) else None, len(nodes),
                  order.ctypes.data_as(_lib._PU32) if len(order) else None, len(order), word, root.ctypes.data_as(_lib._PF))


def tree_moments_host(triangles: np.ndarray, tree: dict) -> np.ndarray:
    """rt_host_tree_moments (include/hrt.h): the moments of a tree dict's subtrees on the host, no device: (node slots, 16)
    float32, per child c xyz (relative to the root centre), N xyz, 0, 0. A tree without nodes gives no records."""
    keep, args = _tree_args(triangles, tree)
    out = np.zeros((len(keep[1]), 16), dtype=np.float32)
    check(lib().rt_host_tree_moments(*args, out.ctypes.data if out.size else None, len(out)), "rt_host_tree_moments")
    return out


def winding_numbers_host(triangles: np.ndarray, tree, points: np.ndarray, beta: float = 0.0) -> np.ndarray:
    """rt_host_winding_numbers (include/hrt.h): Renderer.winding_numbers on the host, no device, for the tree dict `tree`
    (the bytes the device writes for that tree), or the flat definition — every triangle, no dipoles — with tree = None.
    Returns (n,) float32."""
    keep, args = _tree_args(triangles, tree)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(p)
    out = np.zeros((n,), dtype=np.float32)
    check(lib().rt_host_winding_numbers(*args, p.ctypes.data_as(_lib._PF) if n else None, n, C.c_float(beta),
                                        out.ctypes.data_as(_lib._PF) if n else None), "rt_host_winding_numbers")
    return out


def cast_rays_multi_host(triangles: np.ndarray, tree: dict, origins: np.ndarray, dirs: np.ndarray, k: int, tmax=None,
                         after=None, counts: bool = False, flat: bool = False):
    """rt_host_cast_rays_multi (include/hrt.h): Renderer.cast_rays_multi on the host, no device, for the tree dict `tree`
    (lbvh_build / lbvh_refit / Renderer.tri_tree): the bytes the device writes for that tree. flat = True runs the flat
    definition instead, a loop over all triangles in index order; only the tree's root (centre, radius) is read then.
    tmax: None, a float for every ray, or (n,) float32; after: None or n MULTI_HIT_DTYPE records (t and prim are read).
    Returns (n, k) MULTI_HIT_DTYPE records, and with counts = True a pair of them and (n,) uint32 counts (k = 0 needs
    counts)."""
    keep, args = _tree_args(triangles, tree, flat)
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    n = len(o)
    if o.shape != d.shape:
        raise ValueError(f"cast_rays_multi_host: {o.shape} origins for {d.shape} directions")
    cap = None
    if tmax is not None:
        cap = (np.full((n,), tmax, dtype=np.float32) if isinstance(tmax, (int, float))
               else np.ascontiguousarray(tmax, dtype=np.float32))
        if cap.shape != (n,):
            raise ValueError(f"cast_rays_multi_host: tmax must be ({n},) float32, got {cap.shape}")
    cur = None
    if after is not None:
        cur = np.ascontiguousarray(after, dtype=MULTI_HIT_DTYPE)
        if cur.shape != (n,):
            raise ValueError(f"cast_rays_multi_host: after must be ({n},) records, got {cur.shape}")
    hits = np.zeros((n, k), dtype=MULTI_HIT_DTYPE)
    cnt = np.zeros((n,), dtype=np.uint32) if counts else None
    check(lib().rt_host_cast_rays_multi(*args, o.ctypes.data_as(_lib._PF) if n else None,
                                        d.ctypes.data_as(_lib._PF) if n else None,
                                        cap.ctypes.data_as(_lib._PF) if cap is not None and n else None,
                                        cur.ctypes.data if cur is not None and n else None, n, k,
                                        hits.ctypes.data if hits.size else None,
                                        cnt.ctypes.data_as(_lib._PU32) if cnt is not None else None),
          "rt_host_cast_rays_multi")
    return (hits, cnt) if counts else hits


def overlap_volumes_host(triangles: np.ndarray, tree: dict, kind: int, volumes: np.ndarray, k: int, after=None,
                         counts: bool = False, flat: bool = False):
    """rt_host_overlap_volumes (include/hrt.h): Renderer.overlap_records on the host, no device, for the tree dict `tree`
    (lbvh_build / lbvh_refit / Renderer.tri_tree): the bytes the device writes for that tree. flat = True runs the flat
    definition instead, a loop over all triangles in index order; only the tree's root (centre, radius) is read then.
    kind: VOLUME_BOX (volumes (n, 6) float32) or VOLUME_BALL ((n, 4) float32); after: None or n OVERLAP_HIT_DTYPE records
    (d2 and prim are read). Returns (n, k) OVERLAP_HIT_DTYPE records, and with counts = True a pair of them and (n,)
    uint32 counts (k = 0 needs counts)."""
    keep, args = _tree_args(triangles, tree, flat)
    width = _VOLUME_FLOATS.get(kind, 1)
    vol = np.ascontiguousarray(volumes, dtype=np.float32).reshape(-1, width)
    n = len(vol)
    cur = None
    if after is not None:
        cur = np.ascontiguousarray(after, dtype=OVERLAP_HIT_DTYPE)
        if cur.shape != (n,):
            raise ValueError(f"overlap_volumes_host: after must be ({n},) records, got {cur.shape}")
    hits = np.zeros((n, k), dtype=OVERLAP_HIT_DTYPE)
    cnt = np.zeros((n,), dtype=np.uint32) if counts else None
    check(lib().rt_host_overlap_volumes(*args, kind, vol.ctypes.data_as(_lib._PF) if n else None,
                                        cur.ctypes.data if cur is not None and n else None, n, k,
                                        hits.ctypes.data if hits.size else None,
                                        cnt.ctypes.data_as(_lib._PU32) if cnt is not None else None),
          "rt_host_overlap_volumes")
    return (hits, cnt) if counts else hits


def render_ppm(renderer: Renderer) -> str:
    """src/scene/render_ppm.rs:38-57 — blocking readback + ASCII P3."""
    return ppm_from_image(renderer.read_image(), renderer.width, renderer.height)


def ppm_from_image(img: np.ndarray, width: int, height: int) -> str:
    img = np.ascontiguousarray(img, dtype=np.float32)
    n = C.c_size_t()
    check(lib().rt_host_render_ppm(img.ctypes.data_as(_lib._PF), width, height, None, 0, C.byref(n)), "render_ppm")
    buf = C.create_string_buffer(n.value)
    check(lib().rt_host_render_ppm(img.ctypes.data_as(_lib._PF), width, height, buf, n.value, C.byref(n)),
          "render_ppm")
    return buf.raw[: n.value].decode()


class ComparisonError(Exception):
    """tests/rendering_tests.rs:77-82."""

    def __init__(self, kind: str, avg_diff: float | None = None):
        super().__init__(kind if avg_diff is None else f"{kind} {{ avg_diff: {avg_diff} }}")
        self.kind = kind
        self.avg_diff = avg_diff


def compare_ppm_images(img1: str, img2: str, tolerance_percent: float) -> float:
    """tests/rendering_tests.rs:84-131. Returns the mean |du8| in % of 255, raises ComparisonError."""
    a, b = img1.encode(), img2.encode()
    code, avg = C.c_int(), C.c_float(float("nan"))
    rc = lib().rt_host_compare_ppm(a, len(a), b, len(b), tolerance_percent, C.byref(code), C.byref(avg))
    if rc == _lib.RT_OK:
        return avg.value
    kinds = {1: "DifferentDimensions", 2: "PixelCountMismatch", 3: "ExcessiveDifference"}
    raise ComparisonError(kinds.get(code.value, f"status {rc}"), avg.value if code.value == 3 else None)


# ----------------------------------------------------------------------------------------- scenes
class SceneSphere:
    """src/scene/scene_sphere.rs + the Scene impl of src/scene/mod.rs:68-107."""

    def __init__(self, renderer: Renderer, camera: np.ndarray, objects: list):
        self.renderer = renderer
        self.camera = camera
        self.objects = objects

    @staticmethod
    def new(width: int, height: int) -> "SceneSphere":
        """SceneSphere::new (scene_sphere.rs:32-89). The random 'globe' uses thread_rng (non-deterministic);
        every reference test clears it, so the object list starts with the fixed base sphere only."""
        black = Vec3(0.06, 0.06, 0.1)
        camera = Camera.new(Vec3(0.0, 0.0, 3.5), Vec3(0.0, 0.0, 0.0), 3.5, 0.04, PI * f32(0.2))
        objects = [Sphere.new_lambertian(Vec3(0.0, 0.0, 0.0), 1.0, black)]
        return SceneSphere(Renderer(width, height, RT_MODE_SPHERE), camera, objects)

    @staticmethod
    def new_simple(width: int, height: int) -> "SceneSphere":
        """SceneSphere::new_simple (scene_sphere.rs:90-128)."""
        yellow, red = Vec3(0.98, 0.89, 0.69), Vec3(0.953, 0.545, 0.659)
        base, blue, black = Vec3(0.12, 0.12, 0.18), Vec3(0.54, 0.7, 0.98), Vec3(0.06, 0.06, 0.1)
        camera = Camera.new(Vec3(0.0, 0.2, 1.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.05, PI * f32(0.3))
        objects = [
            Sphere.new_lambertian(Vec3(0.0, -100.5, -1.0), 100.0, base),
            Sphere.new_dielectric(Vec3(-1.0, 0.0, -0.6), 0.5, 1.5),
            Sphere.new_lambertian(Vec3(0.0, 0.0, -1.0), 0.5, black),
            Sphere.new_metal(Vec3(1.0, 0.0, -1.0), 0.5, yellow, 0.1),
            Sphere.new_lambertian(Vec3(-0.7, -0.3, -0.1), 0.2, red),
            Sphere.new_metal(Vec3(-0.3, -0.4, -0.4), 0.1, blue, 0.9),
            Sphere.new_dielectric(Vec3(0.2, -0.38, -0.16), 0.12, 0.1),
        ]
        return SceneSphere(Renderer(width, height, RT_MODE_SPHERE), camera, objects)

    def write_scene_data(self) -> None:
        """scene_sphere.rs:24-31: truncated to the 100-sphere buffer like the reference."""
        self.renderer.write_spheres(spheres_array(self.objects[:MAX_OBJECT_IN_SCENE]))

    # Scene trait
    def init(self) -> None:
        self.renderer.set_camera(self.camera)
        self.write_scene_data()

    def draw(self) -> None:
        self.renderer.draw()

    def set_time(self, time: int) -> None:
        self.renderer.set_time(time)

    def resize(self, width: int, height: int) -> None:
        self.renderer.resize(width, height)

    def reset_frame_count(self) -> None:
        self.renderer.reset_frame_count()


class SceneTris:
    """src/scene/scene_tris.rs + the Scene impl of src/scene/mod.rs:27-66."""

    def __init__(self, renderer: Renderer, camera: np.ndarray, tris_bvh: Tree):
        self.renderer = renderer
        self.camera = camera
        self.tris_bvh = tris_bvh

    @staticmethod
    def build_suzane_tree() -> Tree:
        """The tree of SceneTris::new_suzane (scene_tris.rs:119-145), host-only."""
        tree = Tree.from_mesh(Mesh.load_obj(read_asset("suzanne.obj"), Material.new_lambertian(Vec3(0.3, 0.4, 0.6))))
        tree.add_mesh(Mesh.load_obj(read_asset("ico_sphere.obj"), Material.new_dielectric(0.2)))
        tree.add_mesh(Mesh.load_obj(read_asset("cube_s.obj"), Material.new_metal(Vec3(0.5, 0.5, 0.6), 0.2)))
        tree.add_mesh(Mesh.load_obj(read_asset("cube_m.obj"), Material.new_dielectric(0.1)))
        tree.add_mesh(Mesh.load_obj(read_asset("cube_l.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
        tree.build()
        return tree

    @staticmethod
    def suzane_camera() -> np.ndarray:
        return Camera.new(Vec3(0.0, 2.2, 4.5), Vec3(0.0, 0.0, -4.5), 5.6, 0.0, PI * f32(0.3))

    @staticmethod
    def new_suzane(width: int, height: int) -> "SceneTris":
        return SceneTris(Renderer(width, height, RT_MODE_TRIS), SceneTris.suzane_camera(),
                         SceneTris.build_suzane_tree())

    @staticmethod
    def _mesh_on_floor(asset: str, albedo: Vec3) -> Tree:
        tree = Tree.from_mesh(Mesh.load_obj(read_asset(asset), Material.new_lambertian(albedo)))
        tree.add_mesh(Mesh.load_obj(read_asset("floor.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
        tree.build()
        return tree

    @staticmethod
    def new_dragon(width: int, height: int) -> "SceneTris":
        """scene_tris.rs:67-92 (xyzrgb_dragon_lp_20.obj + floor.obj, 49,988 triangles)."""
        tree = SceneTris._mesh_on_floor("xyzrgb_dragon_lp_20.obj", Vec3(0.7, 0.7, 0.2))
        camera = Camera.new(Vec3(0.0, 2.0, 8.0), Vec3(0.0, 0.0, -8.0), 5.6, 0.0, PI * f32(0.3))
        return SceneTris(Renderer(width, height, RT_MODE_TRIS), camera, tree)

    @staticmethod
    def new_lucy(width: int, height: int) -> "SceneTris":
        """scene_tris.rs:93-118 (lucy_lp_20.obj + floor.obj)."""
        tree = SceneTris._mesh_on_floor("lucy_lp_20.obj", Vec3(0.4, 0.3, 0.6))
        camera = Camera.new(Vec3(0.0, 5.0, 6.0), Vec3(0.0, 0.0, -8.0), 5.6, 0.0, PI * f32(0.3))
        return SceneTris(Renderer(width, height, RT_MODE_TRIS), camera, tree)

    @staticmethod
    def new_cube(width: int, height: int) -> "SceneTris":
        """scene_tris.rs:160-180."""
        tree = Tree.from_mesh(Mesh.load_obj(read_asset("cube2.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
        tree.build()
        camera = Camera.new(Vec3(0.0, 2.2, 6.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.0, PI * f32(0.3))
        return SceneTris(Renderer(width, height, RT_MODE_TRIS), camera, tree)

    @staticmethod
    def new_quad(width: int, height: int) -> "SceneTris":
        """scene_tris.rs:181-201."""
        tree = Tree.from_mesh(Mesh.load_obj(read_asset("quad.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
        tree.build()
        camera = Camera.new(Vec3(0.0, 0.2, 3.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.0, PI * f32(0.3))
        return SceneTris(Renderer(width, height, RT_MODE_TRIS), camera, tree)

    def write_tree_data(self) -> None:
        """scene_tris.rs:21-44 (MAX_TRIS / MAX_MATS truncation as in the reference)."""
        sizes, nodes, tris, mats = self.tris_bvh.view()
        self.renderer.write_bvh(sizes, nodes[:MAX_TRIS], tris[:MAX_TRIS], mats[:MAX_MATS])

    def write_triangles_device(self) -> None:
        """The same triangles and materials through rt_set_triangles_device: uploaded as a torch tensor, the tree built on
        the GPU (no reference heap: the renderer walks the device tree, include/hrt.h)."""
        import torch

        _, _, tris, mats = self.tris_bvh.view()
        raw = np.ascontiguousarray(tris[:MAX_TRIS]).view(np.uint8).reshape(-1, 64)
        self.renderer.set_triangles_device(torch.from_numpy(raw.copy()).to(self.renderer._torch_device()),
                                           mats[:MAX_MATS])

    def init(self, device_geometry: bool = False) -> None:
        self.renderer.set_camera(self.camera)
        if device_geometry:
            self.write_triangles_device()
        else:
            self.write_tree_data()

    def draw(self) -> None:
        self.renderer.draw()

    def set_time(self, time: int) -> None:
        self.renderer.set_time(time)

    def resize(self, width: int, height: int) -> None:
        self.renderer.resize(width, height)

    def reset_frame_count(self) -> None:
        self.renderer.reset_frame_count()
