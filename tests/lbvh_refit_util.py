"""Shared by tests/test_lbvh_refit_abi.py and tests/test_gpu_lbvh_refit.py: the shapes and deformations the refit
(rt_refit_triangles_device, rt_host_lbvh_refit) is tried on, and a numpy reading of the tree cost (include/hrt.h
rt_host_lbvh_cost)."""
from __future__ import annotations

import numpy as np

import lbvh_util as U

RANDOM_SIZES = (0, 1, 4, 5, 6, 64, 65, 1025)
DEFORMATIONS = ("translate", "jitter", "scatter", "collapse")


def shapes() -> dict:
    """name -> a function that makes the triangles A the topology is built over."""
    cases = {"cube": lambda: U.mesh_triangles("cube.obj"), "quad": lambda: U.mesh_triangles("quad.obj"),
             "suzanne": lambda: U.mesh_triangles("suzanne.obj")}
    for m in RANDOM_SIZES:
        cases[f"random{m}"] = lambda m=m: U.random_triangles(m, 2000 + m)
    cases["identical70"] = U.identical_triangles
    cases["nan1of9"] = U.nan_triangles
    return cases


def deform(tris: np.ndarray, kind: str, seed: int = 0, amount: float = 0.25) -> np.ndarray:
    """The records with their finite triangles moved (a non-finite one keeps its bytes: the refit asks for the same set):
    translate  by (1000, -2000, 3000): the root centre moves and every box is packed again
    jitter     every vertex of every record on its own, sigma = 5 % of the largest root extent
    scatter    every triangle by its own vector, sigma = `amount` of the largest root extent: the spatial order is gone
    collapse   every vertex to one point"""
    out = tris.copy()
    v64, finite = U.tri_f64(tris)
    if not finite.any():
        return out
    v = np.stack([tris[k][:, :3] for k in "abc"], axis=1).astype(np.float32)
    ext = float((v64[finite].max(axis=(0, 1)) - v64[finite].min(axis=(0, 1))).max())
    ext = ext if ext > 0 else 1.0
    rng = np.random.default_rng(seed * 7919 + DEFORMATIONS.index(kind))
    if kind == "translate":
        nv = v + np.array([1000.0, -2000.0, 3000.0], np.float32)
    elif kind == "jitter":
        nv = v + rng.normal(scale=0.05 * ext, size=v.shape).astype(np.float32)
    elif kind == "scatter":
        nv = v + rng.normal(scale=amount * ext, size=(len(v), 1, 3)).astype(np.float32)
    else:
        nv = np.broadcast_to(np.array([0.5, -1.25, 2.0], np.float32), v.shape)
    for k, name in enumerate("abc"):
        out[name][finite, :3] = nv[finite, k]
    assert (U.tri_f64(out)[1] == finite).all()
    return out


def child_words(tree: dict) -> np.ndarray:
    return tree["nodes"][:, [3, 7]]


def numpy_cost(tree: dict) -> list:
    """The four cost words by the rule of include/hrt.h, in numpy f64 (IEEE, no FMA) and Python integers."""
    nodes, root = tree["nodes"], int(tree["info"][3])
    if root & U.LEAF_BIT:
        return [0, 0, 0, 0]

    def extent(lo, hi):
        with np.errstate(invalid="ignore"):
            e = hi - lo
        e = np.where(e > 0, e, 0.0)
        return np.minimum(e, 131008.0)

    def half_area(e):
        return (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2]) + e[..., 2] * e[..., 0]

    box = nodes.reshape(-1, 2, 4)[:, :, :3]  # (slot, child, axis)
    lo = (box & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    hi = (box >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    R = float(half_area(extent(lo[root].min(axis=0), hi[root].max(axis=0))))
    A = half_area(extent(lo, hi))  # (slot, child)
    cost = [0, 0, 0, 0]
    for slot in np.flatnonzero(nodes[:, 3] != 0):
        cost[2] += 1
        for c in range(2):
            q = min(int(A[slot, c] / R * 65536.0), 1 << 32) if R > 0 else 0
            w = int(nodes[slot, 4 * c + 3])
            if w & U.LEAF_BIT:
                cost[1] += q * (w & 15)
                cost[3] += w & 15
            else:
                cost[0] += q
    return cost
