"""Shared by tests/test_overlap_abi.py and tests/test_gpu_overlap.py: the boxes and balls rt_overlap_volumes is tried on,
the paging loop, and a float64 statement of the box kind's thirteen axes on the exact vertices (a, a + e1, a + e2). The
triangle sets come from tests/lbvh_util.py (cpu_cases()), tests/multihit_util.py (the chain, the stack of squares) and
tests/closest_util.py (the points)."""
from __future__ import annotations

import numpy as np

import hrt

import closest_util as K
import lbvh_util as U
import multihit_util as M

MISS = np.float32(hrt.RT_T_MISS)
BOX, BALL = hrt.VOLUME_BOX, hrt.VOLUME_BALL
KINDS = (BOX, BALL)
BUILDERS = (0, 1)  # LBVH, PLOC
# The band of the box kind against f64, relative to S: the issue's figure, eight times its estimate of 2^-21. DESIGN.md §7h
# derives (13 + 5 / sin(theta)) 2^-24 S + 1.5 * 2^-24 |c| (theta: the angle between e1 and e2; c: the box centre), which this
# band covers for triangles with theta >= 6 degrees and boxes with |c| <= 16 S. A mesh of slivers, or small boxes far from the
# origin, can disagree with f64 outside the band without the code being wrong: the band is no guarantee for arbitrary input.
BAND = 2.0 ** -18

BAD_BOXES = np.array([[0, 0, 0, -1, 1, 1], [0, 1, 0, 1, 0.5, 1], [np.nan, 0, 0, 1, 1, 1], [0, 0, 0, 1, np.nan, 1],
                      [-np.inf, -1, -1, 1, 1, 1], [-1, -1, -1, 1, 1, np.inf], [np.inf, np.inf, np.inf, np.inf, np.inf, np.inf],
                      [-3e38, -3e38, -3e38, 3e38, 3e38, 3e38], [-1e30, -1e30, -1e30, 1e30, 1e30, 1e30]], dtype=np.float32)
N_INVALID = 7  # of BAD_BOXES: inverted, NaN or infinite, which have no hits; the last two are huge and hold everything


def boxes_for(tris: np.ndarray, n: int, seed: int, bad: bool = True, points: bool = True) -> np.ndarray:
    """n float32 boxes (lo xyz, hi xyz) for one triangle set: centred at mesh vertices plus a jitter, half sizes
    log-uniform in 0.5 % to 50 % of the largest root extent, per axis; every eighth a point box at a vertex, a centroid or
    an edge midpoint (points = True: these touch their triangles exactly); with bad = True the last ones are BAD_BOXES."""
    rng = np.random.default_rng(seed)
    v, finite = U.tri_f64(tris)
    lo, hi = K.root_box(tris)
    ext = max(float((hi - lo).max()), 1e-30)
    k = n - (len(BAD_BOXES) if bad else 0)
    if finite.any():
        vf = v[finite]
        j = rng.integers(0, len(vf), size=k)
        centre = vf[j, rng.integers(0, 3, size=k)]
        onmesh = np.select([(np.arange(k) % 3 == 0)[:, None], (np.arange(k) % 3 == 1)[:, None]],
                           [centre, vf[j].mean(axis=1)], 0.5 * (vf[j, 0] + vf[j, 1]))
    else:
        centre = onmesh = rng.normal(size=(k, 3))
    half = ext * np.exp(rng.uniform(np.log(0.005), np.log(0.5), size=(k, 3)))
    centre = centre + rng.normal(size=(k, 3)) * 0.5 * half
    point = ((np.arange(k) % 8 == 3) & points)[:, None]
    with np.errstate(over="ignore"):
        b = np.concatenate([np.where(point, onmesh, centre - half), np.where(point, onmesh, centre + half)], axis=1).astype(np.float32)
    if bad:
        b = np.concatenate([b, BAD_BOXES])
    return np.ascontiguousarray(b)


def balls_for(tris: np.ndarray, n: int, seed: int, r2=None) -> np.ndarray:
    """n float32 balls (centre xyz, squared radius): closest_util.query_points with the radius column (default: RT_T_MISS,
    however far)."""
    p = K.query_points(tris, n, seed)
    col = np.full((n, 1), MISS, dtype=np.float32) if r2 is None else np.asarray(r2, dtype=np.float32).reshape(n, 1)
    return np.ascontiguousarray(np.concatenate([p, col], axis=1))


def volumes_for(kind: int, tris: np.ndarray, n: int, seed: int) -> np.ndarray:
    return boxes_for(tris, n, seed) if kind == BOX else balls_for(tris, n, seed)


def records(triangles, tree, kind, volumes, k, **kw):
    return hrt.overlap_volumes_host(triangles, tree, kind, volumes, k, **kw)


def same_records(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """All 16 bytes of every record."""
    assert got.dtype == want.dtype == hrt.OVERLAP_HIT_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    x = np.frombuffer(got.tobytes(), dtype=np.uint32).reshape(-1, 4)
    y = np.frombuffer(want.tobytes(), dtype=np.uint32).reshape(-1, 4)
    rows = np.flatnonzero((x != y).any(axis=1))
    i = int(rows[0])
    k = max(got.shape[1], 1) if got.ndim == 2 else 1
    raise AssertionError(f"{what}: {len(rows)} of {len(x)} records differ; first at query {i // k} rank {i % k}: "
                         f"{got.reshape(-1)[i]} != {want.reshape(-1)[i]}")


def miss_records(n: int) -> np.ndarray:
    m = np.zeros(n, dtype=hrt.OVERLAP_HIT_DTYPE)
    m["d2"], m["prim"] = MISS, -1
    return m


def paged(query, n: int, k: int, limit: int = 4096):
    """Every record of n queries by pages of k: query(after) -> (n, k) records; the cursor is each query's last record.
    Returns the list of pages up to and including the first page without a hit in its last rank."""
    pages, after = [], None
    for _ in range(limit):
        page = query(after)
        pages.append(page)
        if (page["prim"][:, k - 1] < 0).all():
            return pages
        after = np.ascontiguousarray(page[:, k - 1])
    raise AssertionError("paging did not end")


def ragged(pages):
    """Pages -> per query the (count, 4) uint32 words of its records."""
    allp = np.concatenate(pages, axis=1)
    out = []
    for row in allp:
        hit = row[row["prim"] >= 0]
        out.append(np.frombuffer(hit.tobytes(), dtype=np.uint32).reshape(-1, 4).copy())
    return out


def accepted_matrix(tris, tree, boxes, flat=True) -> np.ndarray:
    """(n, m) bool: which triangles the box kind accepts, from the paged k = 16 answer; the counts must agree."""
    n, m = len(boxes), len(tris)
    _, cnt = records(tris, tree, BOX, boxes, 0, counts=True, flat=flat)
    lists = ragged(paged(lambda after: records(tris, tree, BOX, boxes, 16, after=after, flat=flat), n, 16))
    out = np.zeros((n, m), dtype=bool)
    for i, w in enumerate(lists):
        assert len(w) == cnt[i], (i, len(w), int(cnt[i]))
        out[i, w[:, 1].astype(np.int64)] = True
    return out


def sat_f64(boxes: np.ndarray, tris: np.ndarray, chunk: int = 32):
    """The thirteen axes in float64 on the exact vertices and the exact box: per (box, triangle) pair
    sep  the largest signed gap over the non-zero axes, each divided by its axis length (> 0: separated; 0: touching),
    S    the largest |coordinate| of the three vertices relative to the box centre, and of the half extent,
    aabb whether the triangle's exact box and the query box share a point.
    A non-finite triangle has sep = +inf."""
    v, finite = U.tri_f64(tris)
    b = boxes.astype(np.float64)
    c, h = 0.5 * (b[:, :3] + b[:, 3:]), 0.5 * (b[:, 3:] - b[:, :3])
    e = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], axis=1)  # (m, 3, 3): f0, f1, f2
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[k], (len(v), 3)) for k in range(3)]
    axes += [np.cross(unit[k][None], e[:, i]) for i in range(3) for k in range(3)]
    axes.append(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    L = np.stack(axes, axis=1)  # (m, 13, 3)
    length = np.linalg.norm(L, axis=2)  # (m, 13)
    n, m = len(b), len(v)
    sep, S, aabb = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(0, n, chunk):
            rel = v[None] - c[s:s + chunk, None, None, :]  # (q, m, 3 vertices, 3)
            p = np.einsum("qmvx,max->qmav", rel, L)  # (q, m, 13, 3 vertices)
            r = np.einsum("qx,max->qma", h[s:s + chunk], np.abs(L))
            gap = np.maximum(p.min(axis=3) - r, -p.max(axis=3) - r) / length[None]
            gap = np.where(length[None] > 0.0, gap, -np.inf)
            sep[s:s + chunk] = gap.max(axis=2)
            S[s:s + chunk] = np.maximum(np.abs(rel).max(axis=(2, 3)), h[s:s + chunk].max(axis=1)[:, None])
            aabb[s:s + chunk] = (gap[:, :, :3] <= 0.0).all(axis=2)
    sep[:, ~finite] = np.inf
    aabb[:, ~finite] = False
    return sep, S, aabb
