"""Shared by tests/test_closest_abi.py and tests/test_gpu_closest.py: a float64 closest-point reference (Ericson's regions,
vectorised), the query-point and cap generators, and the chain of triangles that makes a PLOC tree 64 deep. The triangle
sets come from tests/lbvh_util.py (cpu_cases())."""
from __future__ import annotations

import numpy as np

import hrt

import lbvh_util as U

MISS = np.float32(hrt.RT_T_MISS)
U24 = 2.0 ** -24
# DESIGN.md §7e "Accuracy": |sqrt(d2) - true distance| <= (B_EDGE + B_PLANE * kappa) u D, kappa = |e1|^2 |e2|^2 / |e1 x e2|^2 of
# the nearest triangle (its term applies only when the nearest point is inside that triangle), D = |p - rc| + root radius.
B_EDGE, B_PLANE = 64.0, 96.0


def chain_triangles(m: int = 230) -> np.ndarray:
    """Triangles (x, 0, 0), (x, 1, 0), (x, 0, 1) with x = 1e-37 * 2.1^i (tests/test_ploc_abi.py's chain, restated): every
    cluster's nearest neighbour is the one before it, so PLOC merges one pair per iteration until flat mode ends the build:
    a tree 64 deep. m = 230 reaches x = 6e36; m = 120 ends at x = 21."""
    x = (1e-37 * 2.1 ** np.arange(m, dtype=np.float64)).astype(np.float32)
    v = np.zeros((m, 3, 3), dtype=np.float32)
    v[:, :, 0] = x[:, None]
    v[:, 1, 1] = 1.0
    v[:, 2, 2] = 1.0
    return U.triangles_from_vertices(v)


def moved(tris: np.ndarray, offset) -> np.ndarray:
    """The triangles with every vertex moved by `offset`, the sum rounded to f32 (what a caller would upload)."""
    out = tris.copy()
    off = np.asarray(offset, dtype=np.float32)
    for name in ("a", "b", "c"):
        out[name][:, :3] = (tris[name][:, :3] + off).astype(np.float32)
    return out


def closest_f64(points: np.ndarray, v: np.ndarray, chunk: int = 256):
    """Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5) in float64, every point against every
    triangle v (m, 3, 3): (distance (n,), index of a nearest triangle (n,), whether its nearest point is interior (n,))."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    ab, ac = b - a, c - a
    dist, prim, inside = np.empty(len(p)), np.empty(len(p), dtype=np.int64), np.empty(len(p), dtype=bool)
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None, :]
        ap, bp, cp = q - a, q - b, q - c
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide="ignore", invalid="ignore"):
            t_ab = d1 / (d1 - d3)
            t_ac = d2 / (d2 - d6)
            t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            den = 1.0 / (va + vb + vc)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        wv = np.select(conds, [zero, one, zero, t_ab, zero, 1.0 - t_bc], vb * den)
        ww = np.select(conds, [zero, zero, one, zero, t_ac, t_bc], vc * den)
        r = ap - (wv[..., None] * ab + ww[..., None] * ac)
        d = np.sqrt((r * r).sum(-1))
        j = np.argmin(d, axis=1)
        rows = np.arange(len(j))
        dist[s:s + chunk], prim[s:s + chunk] = d[rows, j], j
        inside[s:s + chunk] = ~np.any([cnd[rows, j] for cnd in conds], axis=0)
    return dist, prim, inside


def kappa(v: np.ndarray) -> np.ndarray:
    """|e1|^2 |e2|^2 / |e1 x e2|^2 per triangle (inf for a zero-area one)."""
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (e1 * e1).sum(1) * (e2 * e2).sum(1) / (n * n).sum(1)


def root_box(tris: np.ndarray):
    v, finite = U.tri_f64(tris)
    if not finite.any():
        return np.zeros(3), np.ones(3)
    return v[finite].min(axis=(0, 1)), v[finite].max(axis=(0, 1))


def query_points(tris: np.ndarray, n: int, seed: int, nonfinite: int = 6) -> np.ndarray:
    """n float32 points for one triangle set: vertices and centroids (d2 = 0, and ties between neighbours), near-surface
    jitter, uniform in three times the root box, 1,000 radii away, and `nonfinite` NaN and infinite points at the end."""
    rng = np.random.default_rng(seed)
    v, finite = U.tri_f64(tris)
    lo, hi = root_box(tris)
    centre, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3 * max(float(np.abs(hi - lo).max()), 1e-30))
    radius = 0.5 * float(np.linalg.norm(hi - lo)) or 1.0
    k = max((n - nonfinite) // 4, 1)
    parts = []
    if finite.any():
        vf = v[finite]
        j = rng.integers(0, len(vf), size=k)
        onmesh = np.where((np.arange(k) % 2 == 0)[:, None], vf[j, rng.integers(0, 3, size=k)], vf[j].mean(axis=1))
        wts = rng.dirichlet((1.0, 1.0, 1.0), size=k)
        surf = (vf[rng.integers(0, len(vf), size=k)] * wts[:, :, None]).sum(1)
        parts += [onmesh, surf + rng.normal(size=(k, 3)) * 0.01 * radius]
    else:
        parts += [rng.normal(size=(2 * k, 3))]
    parts.append(centre + (rng.uniform(-1.5, 1.5, size=(k, 3))) * ext)
    far = rng.normal(size=(max(n - nonfinite - 3 * k, 0), 3))
    far /= np.linalg.norm(far, axis=1, keepdims=True)
    parts.append(centre + far * 1000.0 * radius)
    with np.errstate(over="ignore"):
        pts = np.concatenate(parts).astype(np.float32)[:n - nonfinite]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 1],
                    [1, np.nan, np.inf]], dtype=np.float32)
    bad = np.tile(bad, (nonfinite // 6 + 1, 1))[:nonfinite]
    return np.ascontiguousarray(np.concatenate([pts, bad]).astype(np.float32))


def next_up(x: np.ndarray) -> np.ndarray:
    return np.nextafter(np.asarray(x, dtype=np.float32), np.float32(np.inf))


def cap_mix(d2_free: np.ndarray, seed: int) -> np.ndarray:
    """A maxd2 array that mixes every class of cap over the points: NaN, 0, -0, negative, +inf, above RT_T_MISS, exactly
    the unconstrained d2 (a miss), the next f32 above it (the hit), a fraction and a multiple of it, and a tiny radius."""
    rng = np.random.default_rng(seed)
    d = np.asarray(d2_free, dtype=np.float32)
    kind = rng.integers(0, 11, size=len(d))
    with np.errstate(over="ignore", invalid="ignore"):
        choices = [np.full_like(d, np.nan), np.zeros_like(d), np.full_like(d, -0.0), np.full_like(d, -1.0),
                   np.full_like(d, np.inf), np.full_like(d, np.finfo(np.float32).max), d, next_up(d),
                   d * np.float32(0.5), d * np.float32(4.0), np.full_like(d, 2.0 ** -20)]
    return np.ascontiguousarray(np.select([kind == k for k in range(11)], choices).astype(np.float32))


def records_equal(a: np.ndarray, b: np.ndarray) -> bool:
    """All 32 bytes of every record."""
    return a.dtype == b.dtype == hrt.CLOSEST_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(a: np.ndarray, b: np.ndarray) -> str:
    x = np.frombuffer(a.tobytes(), dtype=np.uint32).reshape(-1, 8)
    y = np.frombuffer(b.tobytes(), dtype=np.uint32).reshape(-1, 8)
    rows = np.flatnonzero((x != y).any(axis=1))
    if not len(rows):
        return "equal"
    i = int(rows[0])
    return f"{len(rows)} of {len(x)} records differ; first at {i}: {a[i]} != {b[i]}"
