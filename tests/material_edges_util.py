"""What test_material_edges_oracle.py (CPU) and test_gpu_material_edges.py (GPU) share: the tables of edge values of
Material.kind, Material.params, Material.albedo and Sphere.radius, the scenes that show every table entry to primary rays,
and the oracle's renders of them (rendered once, read-only).

The reference's scatter (shader_sphere.wgsl:172-217, shader_tris.wgsl:222-267) switches on material.id: 1 Lambertian, 2 metal,
3 dielectric, and a default arm that is a copy of the dielectric one (shader_sphere.wgsl:199-215, shader_tris.wgsl:249-265),
so every u32 is a valid kind and every f32 a valid index of refraction, fuzz or albedo. The tables below are data; a table
is a MATERIAL_DTYPE array, and table entry i is sphere slot i (and triangle material i) of a scene.

Layouts. The table's spheres stand on a grid in the plane z = 0, facing a camera on the z axis whose field of view is
fitted to the grid; every fifth sphere (i % 5 == 3: the slot of IOR 2^50 among them) has a negative radius, which flips the
normal, so primary rays meet it "from inside" (front_face false). The ground (radius 100) is below the grid and is the one
large sphere of the culling BVH. The triangle scenes are Suzanne's reference tree with only its material array replaced and
triangles["material"] = index % len(table); the image is larger there, because a material owns only 979 / len(table)
triangles and needs 16 primary hits all the same (test_material_edges_oracle.py holds every scene to that).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import hrt
import scenes
import small_shapes_util as S
from hrt import Camera, Material, Sphere, Vec3

INF, NAN = float("inf"), float("nan")
_f = np.float32


def _next(x, to=INF):
    return float(np.nextafter(_f(x), _f(to)))


KINDS = [0, 3, 4, 5, 6, 7, 0x10001, 0x10002, 0x80000001, 0x80000002, 0xFFFFFFFF]
KIND_PARAMS = [1.5, 0.3]
MASKED_KINDS = [5, 6, 0x10001, 0x10002, 0x80000001, 0x80000002]  # their two low bits spell Lambertian or metal
IOR = [1.0, _next(1.0, 2.0), 0.5, 0.0, -0.0, -1.0, -1.5, 1e-40, 2.0 ** -60, 2.0 ** -51, 2.0 ** -50, 2.0 ** -49, 2.0 ** 49,
       2.0 ** 50, 2.0 ** 51, 2.0 ** 64, 1e20, 3e38, INF, -INF, NAN]
FUZZ = [0.0, 1.0, 1.5, 8.0, -0.5, -8.0, 2.0 ** 39, 2.0 ** 40, _next(2.0 ** 40), 2.0 ** 41, 2.0 ** 63, 2.0 ** 64, 1e30, INF, NAN,
        1e-40, 2.0 ** -41]
ALBEDO_FINITE = [(0.0, 0.0, 0.0), (1 / 0.7,) * 3, (2.0, 3.0, 4.0), (-1.0, 0.5, 0.5), (1e-40,) * 3, (1e30,) * 3]
ALBEDO_NONFINITE = [(INF, 0.5, 0.5), (0.5, NAN, 0.5), (0.5, 0.5, -INF)]
ALBEDO_KIND_PARAM = {1: 0.0, 2: 0.1, 3: 1.5}


def _table(rows) -> np.ndarray:
    t = np.zeros(len(rows), dtype=hrt.MATERIAL_DTYPE)
    for i, (albedo, param, kind) in enumerate(rows):
        t[i] = Material._make(list(albedo) + [1.0], [param] * 3, kind)
    t.setflags(write=False)
    return t


TABLES = {
    "kinds": _table([((0.8, 0.6, 0.4), p, k) for k in KINDS for p in KIND_PARAMS]),
    "ior": _table([((1.0, 1.0, 1.0), v, 3) for v in IOR]),
    "fuzz": _table([((0.8, 0.8, 0.8), v, 2) for v in FUZZ]),
    "albedo_finite": _table([(a, ALBEDO_KIND_PARAM[k], k) for k in (1, 2, 3) for a in ALBEDO_FINITE]),
    "albedo_nonfinite": _table([(a, ALBEDO_KIND_PARAM[k], k) for k in (1, 2, 3) for a in ALBEDO_NONFINITE]),
}
TABLES["all"] = np.concatenate([TABLES[k] for k in ("kinds", "ior", "fuzz", "albedo_finite", "albedo_nonfinite")])
TABLES["all"].setflags(write=False)
TABLE_NAMES = ["kinds", "ior", "fuzz", "albedo_finite", "albedo_nonfinite"]
FINITE_TABLES = ["kinds", "ior", "fuzz"]  # the oracle's images of these hold no NaN and no infinity
ALBEDO_TABLES = ["albedo_finite", "albedo_nonfinite"]
SLOT_IOR_2_50 = IOR.index(2.0 ** 50)  # 13: a negative-radius slot
SLOT_FUZZ_MINUS_8 = FUZZ.index(-8.0)

FRAMES, BOUNCES, TIME0 = 8, 50, 1000
SAH_FRAMES = 2  # frames of the draws held to the oracle with STEP_CAP_SAH (it is slow there)
STEP_CAP_SAH = 0xFFFFFFFF  # oracle.STEP_CAP_SAH: uncapped, and the rule of tri_bvh = 1 and the device trees for non-finite rays
MIN_HITS = 16  # primary rays at time 1000 whose first hit is a given table entry, in every scene
FEW = 11       # table spheres of sphere_few and mixed: 12 slots with the ground, the deferred scan
RADIUS = 0.45
# a 48 x 40 image is 30 tiles of 768 B a frame: a 1 MiB sample buffer holds 45 frames, so 100 frames are three launches
FOLD_FRAMES = 100


def table_size(name: str):
    """The image of a scene: about 48 x 40, and more where a table has more entries than such an image shows 16 pixels of."""
    return (96, 80) if name == "all" else (48, 40)


# ------------------------------------------------------------------------------------------------------ sphere layouts
def _grid(n: int, aspect: float):
    cols = max(1, math.ceil(math.sqrt(n * aspect)))
    rows = math.ceil(n / cols)
    return cols, rows


def _signed_radius(i: int, radius: float) -> float:
    return -radius if i % 5 == 3 else radius


def _grid_spheres(table, aspect: float):
    """The table's spheres, row by row from the bottom, and the ground under them; (spheres, cols, rows)."""
    cols, rows = _grid(len(table), aspect)
    o = []
    for i, m in enumerate(table):
        x, y = (i % cols) - (cols - 1) / 2, (i // cols) + 0.5
        o.append(Sphere._make(Vec3(x, y, 0.0), _signed_radius(i, RADIUS), m))
    o.append(Sphere.new_lambertian(Vec3(0.0, -100.05, 0.0), 100.0, Vec3(0.5, 0.5, 0.5)))
    return o, cols, rows


def _grid_camera(cols: int, rows: int, aspect: float) -> np.ndarray:
    dist = 8.0
    half = max(rows / 2, cols / 2 / aspect) * 1.04
    return Camera.new(Vec3(0.0, rows / 2, dist), Vec3(0.0, rows / 2, 0.0), dist, 0.02, 2.0 * math.atan(half / dist))


def _filler(count: int, cols: int, rows: int):
    """Ordinary spheres behind the grid, in its gaps."""
    o = []
    per = (cols + 1) * (rows + 1)
    for k in range(count):
        c = Vec3((k % (cols + 1)) - cols / 2, ((k // (cols + 1)) % (rows + 1)) + 0.0, -2.0 - 1.5 * (k // per))
        if k % 3 == 0:
            o.append(Sphere.new_lambertian(c, 0.3, Vec3(0.2 + 0.1 * (k % 7), 0.5, 0.8 - 0.1 * (k % 5))))
        elif k % 3 == 1:
            o.append(Sphere.new_metal(c, 0.3, Vec3(0.8, 0.7, 0.6), 0.05 * (k % 4)))
        else:
            o.append(Sphere.new_dielectric(c, 0.3, 1.5))
    return o


def _sphere_scene(name: str, table_name: str, n=None, filler=None) -> scenes.SceneDef:
    table = TABLES[table_name][:n]
    w, h = table_size(table_name)
    o, cols, rows = _grid_spheres(table, w / h)
    if filler == "bvh":
        o += _filler(max(64 - len(o), 6), cols, rows)
    sp = hrt.spheres_array(o)
    if filler == "deep":  # two seeded cover scenes, moved behind the grid: > 192 nodes, no LDS nodes
        deep = np.concatenate([scenes.rtiow_spheres(42), scenes.rtiow_spheres(7)])
        deep["center"][:, 2] -= np.float32(15.0)
        sp = np.concatenate([sp, deep])
    return scenes.SceneDef(f"{name}({table_name})", hrt.RT_MODE_SPHERE, w, h, _grid_camera(cols, rows, w / h), sp,
                           frames=FRAMES, bounces=BOUNCES, min_sphere_slots=0)


def sphere_bvh(table_name: str) -> scenes.SceneDef:
    """At least 64 slots: variant = 4 walks the culling BVH and k_trace_split runs."""
    return _sphere_scene("sphere_bvh", table_name, filler="bvh")


def deep(table_name: str) -> scenes.SceneDef:
    return _sphere_scene("deep", table_name, filler="deep")


def sphere_few(table_name: str) -> scenes.SceneDef:
    """The first 11 table spheres and the ground: 12 slots, the deferred scan."""
    return _sphere_scene("sphere_few", table_name, n=FEW)


# ---------------------------------------------------------------------------------------------------- triangle layouts
# suzanne.obj is the head (x +-1.37, y 0 .. 1.95, z +-0.85) on a floor of a few large triangles at y = -0.45. From 45 degrees
# above the front every material index of every table owns 16 pixels; the camera was searched for that over 108 directions.
TRI_SIZE = {"all": (192, 156)}
TRI_SIZE_DEFAULT = (64, 52)
TRI_TARGET = (0.0, 0.9, 0.0)
TRI_DIST = 4.0
_S45 = math.sqrt(0.5)
TRI_EYE = (0.0, TRI_TARGET[1] + TRI_DIST * _S45, TRI_DIST * _S45)
TRI_UP = (0.0, _S45, -_S45)  # the camera's up vector in the world


@functools.lru_cache(maxsize=None)
def _suzanne():
    sizes, nodes, tris, mats = scenes.suzanne_tree().view()
    return tuple(sizes), nodes.copy(), tris.copy()


def _tree(table) -> tuple:
    """Suzanne's tree with the table for its materials: nothing else changes, so the reference walk and its 600-step cap
    stay as they are."""
    sizes, nodes, tris = _suzanne()
    tris = tris.copy()
    tris["material"] = np.arange(len(tris), dtype=np.uint32) % np.uint32(len(table))
    return sizes, nodes, tris, np.array(table, dtype=hrt.MATERIAL_DTYPE)


def _tri_camera(half: float) -> np.ndarray:
    return Camera.new(Vec3(*TRI_EYE), Vec3(*TRI_TARGET), TRI_DIST, 0.01, 2.0 * math.atan(half / TRI_DIST))


def tris(table_name: str) -> scenes.SceneDef:
    w, h = TRI_SIZE.get(table_name, TRI_SIZE_DEFAULT)
    return scenes.SceneDef(f"tris({table_name})", hrt.RT_MODE_TRIS, w, h, _tri_camera(1.25), bvh=_tree(TABLES[table_name]),
                           frames=FRAMES, bounces=BOUNCES, min_sphere_slots=0)


def mixed(table_name: str, slots: int = FEW + 1) -> scenes.SceneDef:
    """The same tree over the first 11 spheres of the REVERSED table and the ground, so a sphere slot and a triangle
    material of one index differ: a scatter that reads the sphere's constants for a triangle hit, or the other way round,
    shades wrongly. The spheres stand in a column left and a column right of the head, in the plane through it that faces
    the camera. slots = 1 keeps only the ground (the simple scan); slots > 12 adds ordinary spheres behind the head
    (60: the culling BVH)."""
    table = TABLES[table_name]
    w, h = TRI_SIZE.get(table_name, TRI_SIZE_DEFAULT)
    rev = table[::-1][:FEW]
    o = []
    if slots > 1:
        for i, m in enumerate(rev):
            left = i < 6
            u = ((i - 2.5) if left else (i - 6 - 2.0)) * 0.5  # along the camera's up vector
            c = Vec3(-1.62 if left else 1.62, TRI_TARGET[1] + u * TRI_UP[1], u * TRI_UP[2])
            o.append(Sphere._make(c, _signed_radius(i, 0.22), m))
    o.append(Sphere.new_lambertian(Vec3(0.0, -100.6, 0.0), 100.0, Vec3(0.5, 0.5, 0.5)))
    for k in range(max(slots - len(o), 0)):
        c = Vec3((k % 8 - 3.5) * 0.7, 0.3 + (k // 8) * 0.6, -2.5)
        o.append(Sphere.new_metal(c, 0.25, Vec3(0.8, 0.7, 0.6), 0.1) if k % 2 else
                 Sphere.new_lambertian(c, 0.25, Vec3(0.3, 0.5, 0.7)))
    return scenes.SceneDef(f"mixed({table_name}, {slots})", hrt.RT_MODE_MIXED, w, h, _tri_camera(1.5), hrt.spheres_array(o),
                           bvh=_tree(table), frames=FRAMES, bounces=BOUNCES, min_sphere_slots=0)


# ------------------------------------------------------------------------------------------------------- the far wall
FAR_RADII = [2.0 ** 60, _next(2.0 ** 60)]  # either side of upload_spheres' rad_ok: 1 / radius, or the division


def far_wall() -> scenes.SceneDef:
    """small_shapes_util's four spheres and camera, and two metal spheres so large that the camera sees each as a wall: one
    of radius 2^60 with its centre 2^60 + 2^41 behind the scene, one of the next radius with its centre 2^60 + 2^39 to the
    right of it (an ulp is 2^37 there). Slots 4 and 5."""
    o = S.four_spheres()
    o.append(Sphere.new_metal(Vec3(0.0, 0.0, -(2.0 ** 60 + 2.0 ** 41)), FAR_RADII[0], Vec3(0.8, 0.8, 0.8), 0.0))
    o.append(Sphere.new_metal(Vec3(2.0 ** 60 + 2.0 ** 39, 0.0, 0.0), FAR_RADII[1], Vec3(0.8, 0.6, 0.2), 0.0))
    return scenes.SceneDef("far_wall", hrt.RT_MODE_SPHERE, 48, 40, S.camera(), hrt.spheres_array(o), frames=FRAMES,
                           bounces=BOUNCES, min_sphere_slots=0)


FAR_SLOTS = [4, 5]

BUILDERS = {"sphere_bvh": sphere_bvh, "deep": deep, "sphere_few": sphere_few, "tris": tris, "mixed": mixed}


@functools.lru_cache(maxsize=None)
def scene(builder: str, table_name: str = "all", **kw) -> scenes.SceneDef:
    """The scenes by name, built once; read-only by agreement (use dataclasses.replace for another frame count)."""
    return far_wall() if builder == "far_wall" else BUILDERS[builder](table_name, **kw)


def table_slots(builder: str, table_name: str):
    """(sphere slots that hold table entries, triangle material indices) of a scene."""
    n = len(TABLES[table_name])
    if builder in ("sphere_bvh", "deep"):
        return list(range(n)), []
    if builder == "sphere_few":
        return list(range(min(n, FEW))), []
    if builder == "tris":
        return [], list(range(n))
    if builder == "mixed":
        return list(range(min(n, FEW))), list(range(n))
    return FAR_SLOTS, []


@functools.lru_cache(maxsize=None)
def oracle(builder: str, table_name: str = "all", frames: int = FRAMES, step_cap: int = 600, **kw):
    """(image, queries) of the CPU oracle for a scene, rendered once and read-only."""
    import dataclasses

    sd = dataclasses.replace(scene(builder, table_name, **kw), frames=frames)
    img, q = scenes.oracle_render(sd, step_cap=step_cap)
    img.setflags(write=False)
    return img, q


@functools.lru_cache(maxsize=None)
def primary(builder: str, table_name: str = "all", **kw):
    """The oracle's primary rays at time 1000, flat: (origins (n, 3), dirs (n, 3), rng (n,)); read-only."""
    o, d, s = scenes.oracle_primary_rays(scene(builder, table_name, **kw), TIME0)
    out = (np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3)), np.ascontiguousarray(s.reshape(-1)))
    for a in out:
        a.setflags(write=False)
    return out


def first_hit_counts(builder: str, table_name: str = "all", **kw):
    """How many primary rays at time 1000 have each sphere slot, and each triangle material, as their first hit:
    (dict slot -> rays, dict material -> rays), from oracle_primary_rays and oracle_cast_rays."""
    sd = scene(builder, table_name, **kw)
    o, d, _ = primary(builder, table_name, **kw)
    rec, _ = scenes.oracle_cast_rays(sd, o, d)
    hit = rec["prim"] >= 0
    tri = hit & ((rec["flags"] & hrt.RT_HIT_TRIANGLE) != 0)
    sph = hit & ~tri
    slots = dict(zip(*(a.tolist() for a in np.unique(rec["prim"][sph], return_counts=True))))
    mats = dict(zip(*(a.tolist() for a in np.unique(rec["material"][tri], return_counts=True))))
    return slots, mats


def assert_image(img: np.ndarray, ref: np.ndarray, what: str):
    """small_shapes_util.assert_bits where the oracle's image is finite, and its NaN rule where it is not: equal NaN masks,
    and every other channel, +inf and -inf included, the reference's bits."""
    if np.isfinite(ref).all():
        S.assert_bits(img, ref, what)
    else:
        S.assert_nan_rule(img, ref, what)
