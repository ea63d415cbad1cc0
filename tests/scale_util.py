"""Shared by tests/test_scale_abi.py and tests/test_gpu_scale.py: a mesh generated at run time that is large enough for
the device tree builders' multi-turn and multi-wave paths, the three sizes that reach them, and per-module caches of the
meshes and of their host mirror trees (both builders, built and refitted). Nothing here is read from a file: device and
mirror consume the same array within one run.

The sizes (finite triangles m', records n):
  EDGE_LO  262,144 /   262,144  512 x 256 x 2: 1024 PLOC tiles of 256 clusters exactly, the last size whose tile counts
                                are scanned in one turn of k_ploc_scan (1024 tiles per turn)
  EDGE_HI  262,145 /   262,168  + 1 duplicate, + 23 non-finite: 1025 tiles, a second turn with one tile in it
  BIG    1,048,577 / 1,048,600  1024 x 512 x 2 + 1 duplicate, + 23 non-finite. A PLOC iteration keeps at least
                                ceil(c / 2) clusters, so the first three iterations have at least 1,048,577, 524,289 and
                                262,145 clusters: 4097, >= 2049 and >= 1025 tiles, which is 5, >= 3 and >= 2 turns of the
                                scan. The sort has 1025 tiles of 1024 keys: 5 iterations of k_regroup_scan (256 tiles
                                each). The fits and the moments climb have 4097 workgroups. Derived, not measured."""
from __future__ import annotations

import numpy as np

import hrt

import lbvh_refit_util as R
import lbvh_util as U

PLOC = 1
BUILDERS = (0, PLOC)
PLOC_TILE = 256           # clusters per tile of the PLOC kernels
PLOC_SCAN_TILES = 1024    # tile counts per turn of k_ploc_scan
SORT_TILE = 1024          # keys per tile of the regroup sort
SORT_SCAN_TILES = 256     # tiles per iteration of k_regroup_scan
FIT_BLOCK = 256           # nodes per workgroup of the bottom-up fits
# The triangle test refuses |e1 . (d x e2)| < 1e-4, an absolute figure (csrc/rt_kernels.hip tri_t, after the reference). A
# million triangles on a unit sphere have |e1 x e2| near 4e-5: no ray of unit length would ever hit one. At radius 8 it
# is 2.4e-3 around the equator, and only the few rings next to the poles stay unseen.
RADIUS = 8.0

# name -> (nu, nv, dup, bad)
SIZES = {"EDGE_LO": (512, 256, 0, 0), "EDGE_HI": (512, 256, 1, 23), "BIG": (1024, 512, 1, 23)}
FINITE = {"EDGE_LO": 262144, "EDGE_HI": 262145, "BIG": 1048577}
RECORDS = {"EDGE_LO": 262144, "EDGE_HI": 262168, "BIG": 1048600}


def bumpy_sphere_vertices(nu: int, nv: int) -> np.ndarray:
    """(2 nu nv, 3, 3) float32: a closed UV sphere wound outward, radius RADIUS (1 + 0.25 cos(6 theta)) along the polar angle
    theta, nu quads around by nv from pole to pole, two triangles each. Every ring is one set of f32 vertices that its
    quads share (the seam included), and the two pole rings are one point each: the quads of the pole rows keep both their
    triangles, one of them with two equal vertices (zero area, finite)."""
    theta = np.pi * np.arange(nv + 1, dtype=np.float64) / nv
    phi = 2.0 * np.pi * np.arange(nu, dtype=np.float64) / nu
    radius = RADIUS * (1.0 + 0.25 * np.cos(6.0 * theta))
    ring = radius * np.sin(theta)
    ring[0] = ring[nv] = 0.0  # (sin(pi) is not 0 in f64)
    p = np.empty((nv + 1, nu, 3), dtype=np.float64)
    p[:, :, 0] = ring[:, None] * np.cos(phi)[None, :]
    p[:, :, 1] = ring[:, None] * np.sin(phi)[None, :]
    p[:, :, 2] = (radius * np.cos(theta))[:, None]
    p = p.astype(np.float32)
    nxt = np.roll(np.arange(nu), -1)
    p00, p10, p01, p11 = p[:-1], p[:-1, nxt], p[1:], p[1:, nxt]
    v = np.empty((nv, nu, 2, 3, 3), dtype=np.float32)
    v[:, :, 0] = np.stack([p00, p01, p11], axis=2)  # (d theta) x (d theta + d phi): along the radius, outward
    v[:, :, 1] = np.stack([p00, p11, p10], axis=2)
    return v.reshape(-1, 3, 3)


def bad_positions(n: int, bad: int) -> np.ndarray:
    """Where the non-finite records of an n-record array sit: spread evenly through it, none in the last record."""
    return ((np.arange(bad, dtype=np.int64) * 2 + 1) * n // (2 * bad)) if bad else np.zeros(0, dtype=np.int64)


def bumpy_sphere(nu: int, nv: int, dup: int = 0, bad: int = 0) -> np.ndarray:
    """2 nu nv + dup + bad TRIANGLE_DTYPE records: the sphere's triangles in ring order, then copies of its first `dup`
    triangles (equal keys and boxes), with `bad` records of NaN vertices put in between at bad_positions(): the
    finite triangles keep their order, their indices do not."""
    v = bumpy_sphere_vertices(nu, nv)
    v = np.concatenate([v, v[:dup]])
    n = len(v) + bad
    out = np.full((n, 3, 3), np.nan, dtype=np.float32)
    keep = np.ones(n, dtype=bool)
    keep[bad_positions(n, bad)] = False
    out[keep] = v
    return U.triangles_from_vertices(out)


_MESH, _TREE, _REFIT = {}, {}, {}


def mesh(name: str) -> np.ndarray:
    """The records of one named size, made once. Do not write to them."""
    if name not in _MESH:
        t = bumpy_sphere(*SIZES[name])
        assert len(t) == RECORDS[name] and int(U.tri_f64(t)[1].sum()) == FINITE[name]
        t.flags.writeable = False
        _MESH[name] = t
    return _MESH[name]


def mirror(name: str, builder: int) -> dict:
    """hrt.lbvh_build of one named size, made once."""
    if (name, builder) not in _TREE:
        _TREE[name, builder] = hrt.lbvh_build(mesh(name), builder=builder)
    return _TREE[name, builder]


def bend(points: np.ndarray) -> np.ndarray:
    """(..., 3) float32 -> float32: x' = 1.25 x + 0.3 RADIUS sin(2 y / RADIUS), z' = z - 0.2 y, a shear and a wave. One to
    one on space, and a function of the f32 point alone: vertices that were equal stay equal, so a closed mesh stays
    closed and keeps its inside."""
    p = np.asarray(points, dtype=np.float32)
    out = p.copy()
    with np.errstate(invalid="ignore"):
        out[..., 0] = np.float32(1.25) * p[..., 0] + np.float32(0.3 * RADIUS) * np.sin(np.float32(2.0 / RADIUS) * p[..., 1])
        out[..., 2] = p[..., 2] - np.float32(0.2) * p[..., 1]
    return out


def moved(name: str, how: str = "jitter") -> np.ndarray:
    """The records of one named size moved, made once. "jitter": tests/lbvh_refit_util.py deform, every vertex on its own
    by 5 % of the extent, twenty times a triangle's size at BIG: a soup of large triangles, the worst a refit can be
    given. "bend": bend() of every vertex: the surface a user's deformation would leave, still closed."""
    if (name, how) not in _REFIT:
        a = mesh(name)
        if how == "jitter":
            b = R.deform(a, "jitter")
        else:
            b = a.copy()
            for k in "abc":
                b[k][:, :3] = bend(a[k][:, :3])
        assert (U.tri_f64(b)[1] == U.tri_f64(a)[1]).all()
        b.flags.writeable = False
        _REFIT[name, how] = b
    return _REFIT[name, how]


def refitted(name: str, builder: int, how: str = "jitter") -> dict:
    """hrt.lbvh_refit(mesh, moved mesh) of one named size, made once."""
    if (name, builder, how) not in _TREE:
        _TREE[name, builder, how] = hrt.lbvh_refit(mesh(name), moved(name, how), builder=builder)
    return _TREE[name, builder, how]


def tiles(count: int, tile: int) -> int:
    return (count + tile - 1) // tile


def turns(count: int, per_turn: int) -> int:
    return (count + per_turn - 1) // per_turn


def info_of(tree: dict, builder: int) -> list:
    """rt_get_tri_tree_info's eight words from a mirror's info."""
    i = tree["info"].tolist()
    return [builder, i[0], i[2], i[3], i[4], i[5], i[6], 0]


def left_descents_overflow(tree: dict, stack: int = 24) -> bool:
    """Whether a depth-first walk that takes every child (left first, the node's index pushed while its left child is
    descended: csrc/rt_winding.hpp's walk with beta = +inf, where no child is far) needs more than `stack` words: the
    stack holds the ancestors that were entered through their left child, so it overflows where a node with `stack` such
    ancestors has a node as its left child. A property of the child words alone, level by level in numpy."""
    nodes = tree["nodes"]
    root = int(tree["info"][3])
    if root & U.LEAF_BIT:
        return False
    front, lefts = np.array([root], dtype=np.int64), np.zeros(1, dtype=np.int64)
    while len(front):
        lw, rw = nodes[front, 3], nodes[front, 7]
        ln, rn = (lw & U.LEAF_BIT) == 0, (rw & U.LEAF_BIT) == 0
        if (lefts[ln] == stack).any():
            return True
        front = np.concatenate([lw[ln], rw[rn]]).astype(np.int64)
        lefts = np.concatenate([lefts[ln] + 1, lefts[rn]])
    return False


def inside_outside_points():
    """A few points well inside the sphere (its radius is at least 0.75 RADIUS everywhere) and a few well outside (at most
    1.25 RADIUS), float32."""
    rng = np.random.default_rng(41)
    d = rng.normal(size=(16, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = np.concatenate([np.zeros((1, 3)), d[:7] * 0.4 * RADIUS])
    outside = d[8:] * rng.uniform(2.0, 6.0, size=(8, 1)) * RADIUS
    return np.ascontiguousarray(inside.astype(np.float32)), np.ascontiguousarray(outside.astype(np.float32))
