"""Shared by tests/test_winding_abi.py and tests/test_gpu_winding.py: a float64 brute-force winding number (Van Oosterom
and Strackee's form over every triangle, numpy), the query-point generators, the decoded moments of a tree, and the
measured error bounds. The triangle sets come from tests/lbvh_util.py and tests/closest_util.py."""
from __future__ import annotations

import math

import numpy as np

import hrt

import closest_util as K
import lbvh_util as U

LEAF_BIT = 0x80000000
QNAN = 0x7FC00000
INF = float("inf")
BUILDERS = (0, 1)  # LBVH, PLOC
MESHES = ("cube", "ico_sphere", "suzanne")

# The largest |w - w_ref| of the host mirror against winding_f64 over accuracy_points(mesh), both builders, measured once
# (python tests/winding_util.py prints them); the tests assert four times these.
MEASURED = {
    "cube": {INF: 2.86e-6, 2.0: 3.23e-3, 3.0: 2.86e-6},
    "ico_sphere": {INF: 7.62e-7, 2.0: 1.45e-2, 3.0: 1.77e-3},
    "suzanne": {INF: 2.48e-5, 2.0: 4.05e-2, 3.0: 9.07e-3},
}
MARGIN = 4.0


def bound(mesh: str, beta: float) -> float:
    return MARGIN * MEASURED[mesh][beta]


_TRIS = {}


def mesh(name: str) -> np.ndarray:
    if name not in _TRIS:
        _TRIS[name] = U.mesh_triangles(name + ".obj")
    return _TRIS[name]


def winding_f64(tris: np.ndarray, points: np.ndarray, chunk: int = 64) -> np.ndarray:
    """(1 / 4 pi) sum of the signed solid angles of the finite triangles (the vertices the device keeps: a, a + e1, a + e2)
    in float64, every point against every triangle."""
    v, finite = U.tri_f64(tris)
    v = v[finite]
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(p))
    for s in range(0, len(p), chunk):
        x = v[None] - p[s:s + chunk, None, None, :]
        ln = np.linalg.norm(x, axis=-1)
        x0, x1, x2 = x[:, :, 0], x[:, :, 1], x[:, :, 2]
        num = (x0 * np.cross(x1, x2)).sum(-1)
        den = (ln[..., 0] * ln[..., 1] * ln[..., 2] + (x0 * x1).sum(-1) * ln[..., 2] + (x1 * x2).sum(-1) * ln[..., 0]
               + (x2 * x0).sum(-1) * ln[..., 1])
        out[s:s + chunk] = np.arctan2(num, den).sum(-1) / (2.0 * math.pi)
    return out


def accuracy_points(tris: np.ndarray, seed: int = 18) -> np.ndarray:
    """400 points uniform in 1.5 times the box and 400 within 1 % (of the box diagonal) of the surface, float32."""
    rng = np.random.default_rng(seed)
    v, finite = U.tri_f64(tris)
    v = v[finite]
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    box = 0.5 * (lo + hi) + rng.uniform(-0.75, 0.75, size=(400, 3)) * (hi - lo)
    wts = rng.dirichlet((1.0, 1.0, 1.0), size=400)
    on = (v[rng.integers(0, len(v), size=400)] * wts[:, :, None]).sum(1)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = on + d * rng.uniform(0.0, 0.01, size=(400, 1)) * np.linalg.norm(hi - lo)
    return np.ascontiguousarray(np.concatenate([box, near]).astype(np.float32))


_ACC = {}


def accuracy_case(name: str):
    """(triangles, points, f64 reference), made once per mesh."""
    if name not in _ACC:
        tris = mesh(name)
        pts = accuracy_points(tris)
        _ACC[name] = (tris, pts, winding_f64(tris, pts))
    return _ACC[name]


def scaled(tris: np.ndarray, factor: float) -> np.ndarray:
    """Every vertex times `factor`, rounded to f32."""
    out = tris.copy()
    with np.errstate(over="ignore"):
        for name in ("a", "b", "c"):
            out[name][:, :3] = (tris[name][:, :3].astype(np.float64) * factor).astype(np.float32)
    return out


def child_moments(mom: np.ndarray, node: int, side: int):
    """(c, N) of one child, float64."""
    r = mom[node, 8 * side:8 * side + 8].astype(np.float64)
    return r[0:3], r[3:6]


def child_box_rel(nodes: np.ndarray, node: int, side: int):
    """The decoded fp16 box of one child relative to the root centre, float64 (lo, hi)."""
    w = nodes[node, 4 * side:4 * side + 3].astype(np.uint32)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    hi = (w >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    return lo, hi


def same_bits(got: np.ndarray, want: np.ndarray) -> None:
    a, b = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert a.shape == b.shape, (a.shape, b.shape)
    rows = np.flatnonzero(a != b)
    assert not len(rows), f"{len(rows)} of {len(a)} differ; first at {rows[0]}: {got[rows[0]]!r} != {want[rows[0]]!r}"


def chain_points(n: int = 256, seed: int = 4) -> np.ndarray:
    """Points beside and inside the 120-triangle chain (tests/closest_util.py chain_triangles), float32."""
    rng = np.random.default_rng(seed)
    tris = K.chain_triangles(120)
    pts = np.concatenate([rng.uniform(-1.0, 1.0, size=(n // 2, 3)) - [3.0, 0.0, 0.0], K.query_points(tris, n - n // 2, 6, nonfinite=0)])
    return np.ascontiguousarray(pts.astype(np.float32))


def clear_of_surface(tris: np.ndarray, points: np.ndarray, fraction: float = 0.01) -> np.ndarray:
    """Which points are finite and further than `fraction` of the box diagonal from every triangle: there w is smooth, and
    an f32 answer can be held against the f64 one."""
    p = np.asarray(points, dtype=np.float64)
    ok = np.isfinite(p).all(axis=1)
    v, finite = U.tri_f64(tris)
    lo, hi = K.root_box(tris)
    dist = np.full(len(p), np.inf)
    dist[ok] = K.closest_f64(p[ok], v[finite])[0]
    return ok & (dist > fraction * np.linalg.norm(hi - lo))


def walk_shape(tree: dict, mom: np.ndarray, p, beta: float, stack: int = 24):
    """The control flow of csrc/rt_winding.hpp's walk for one covered point, restated: (overflowed, dipole terms, triangle
    terms before any overflow). The far-field test is the header's, operation for operation, in Python's f64."""
    nodes, root = tree["nodes"], tree["root"]
    q = [float(np.float32(np.float32(p[k]) - root[k])) for k in range(3)]
    beta2 = float(beta) * float(beta)
    node, side, pending, dip, tri = int(tree["info"][3]), 0, [], 0, 0
    assert not node & LEAF_BIT
    while True:
        lo, hi = child_box_rel(nodes, node, side)
        c, _ = child_moments(mom, node, side)
        dd = [(float(c[k]) - q[k]) ** 2 for k in range(3)]
        mm = [max(float(c[k]) - float(lo[k]), float(hi[k]) - float(c[k])) ** 2 for k in range(3)]
        L2, R2 = (dd[0] + dd[1]) + dd[2], (mm[0] + mm[1]) + mm[2]
        word = int(nodes[node, 4 * side + 3])
        with np.errstate(invalid="ignore"):
            far = bool(np.float64(L2) > np.float64(beta2) * np.float64(R2))
        if far:
            dip += 1
        elif word & LEAF_BIT:
            tri += word & 15
        else:
            if side == 0:
                if len(pending) == stack:
                    return True, dip, tri
                pending.append(node)
            node, side = word, 0
            continue
        if side == 0:
            side = 1
        elif pending:
            node, side = pending.pop(), 1
        else:
            return False, dip, tri


if __name__ == "__main__":  # the figures of MEASURED
    for name in MESHES:
        tris, pts, ref = accuracy_case(name)
        worst = {b: 0.0 for b in (INF, 2.0, 3.0)}
        worst[INF] = float(np.abs(hrt.winding_numbers_host(tris, None, pts) - ref).max())
        for builder in BUILDERS:
            tree = hrt.lbvh_build(tris, builder)
            for beta in worst:
                worst[beta] = max(worst[beta], float(np.abs(hrt.winding_numbers_host(tris, tree, pts, beta) - ref).max()))
        skipped = float((np.abs(ref - 0.5) < 0.25).mean())
        print(name, {k: f"{v:.3g}" for k, v in worst.items()}, f"w in [{ref.min():.3f}, {ref.max():.3f}]", f"skipped {skipped:.4f}")
