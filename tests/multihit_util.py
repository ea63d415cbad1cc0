"""Shared by tests/test_multihit_abi.py and tests/test_gpu_multihit.py: the triangle sets and rays rt_cast_rays_multi is
tried on, the paging loop, numpy restatements of the definition's parts (a triangle's own box, the decoded node boxes, the
triangle test alone in f32 and in f64) and the containment check. The other triangle sets come from tests/lbvh_util.py
(cpu_cases()) and tests/closest_util.py (the chain)."""
from __future__ import annotations

import numpy as np

import hrt

import closest_util as K
import lbvh_util as U

MISS = np.float32(hrt.RT_T_MISS)
LEAF_BIT = 0x80000000
BUILDERS = (0, 1)  # LBVH, PLOC
T_MIN = np.float32(1e-4)
_F32 = np.float32


def stack_of_squares(m: int) -> np.ndarray:
    """m unit squares [0, 1]^2 at z = 1 .. m, two triangles each (2 i, 2 i + 1 at z = i + 1) sharing the diagonal x = y.
    Every coordinate is a small integer: every product and sum of the triangle test is exact."""
    v = []
    for z in range(1, m + 1):
        p = [(0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)]
        v += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    return U.triangles_from_vertices(np.array(v, dtype=np.float32))


def chain() -> np.ndarray:
    """The first 120 triangles of the PLOC chain (x up to 21: the 230-triangle chain's root box makes D overflow, and a
    ray with a non-finite D has no hits by definition)."""
    return K.chain_triangles(120)


def chain_rays(n: int = 96, seed: int = 9):
    """Rays along +x through the chain's triangles (y, z > 0, y + z < 1), some tilted, some from the far side."""
    rng = np.random.default_rng(seed)
    yz = rng.dirichlet((1.0, 1.0, 1.0), size=n)[:, :2]
    o = np.concatenate([np.full((n, 1), -1.0), yz], axis=1)
    d = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 2)) * 0.01], axis=1)
    back = np.arange(n) % 4 == 3
    o[back, 0], d[back, 0] = 30.0, -1.0
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d.astype(np.float32))


def camera_rays(cam: np.ndarray, w: int, h: int):
    """The rays through the pixel centres of a w x h image of `cam` (a CAMERA_DTYPE record): no jitter, no lens."""
    eye, dirv, up, right = (np.asarray(cam[k], dtype=np.float64).reshape(4)[:3] for k in ("eye", "direction", "up", "right"))
    fov = float(np.asarray(cam["params"]).reshape(4)[2])
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
    ux = (2.0 * xs.ravel() / w - 1.0) * (w / h) * np.tan(0.5 * fov)
    uy = -(2.0 * ys.ravel() / h - 1.0) * np.tan(0.5 * fov)
    d = right[None] * ux[:, None] + up[None] * uy[:, None] + dirv[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(eye[None], (len(d), 1))
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d.astype(np.float32))


BAD_RAYS = np.array([[[np.nan, 0, 0], [0, 0, 1]], [[0, 0, 0], [0, np.inf, 1]], [[0, -np.inf, 0], [0, 1, 0]],
                     [[0, 0, 0], [np.nan, np.nan, np.nan]], [[0, 0, 0], [0, 0, 0]], [[3e38, -3e38, 3e38], [1, 0, 0]],
                     [[0.1, 0.2, -50.0], [0, 0, 1]], [[0.1, -50.0, 0.3], [0, 1, 0]], [[-50.0, 0.2, 0.3], [1, 0, -0.0]],
                     [[0.1, 0.2, 0.3], [1e-31, -1e-31, 1]], [[0, 0, 0], [1e-20, 1e-20, 1e-20]],
                     [[0, 0, 0], [1e20, -1e20, 3e19]]], dtype=np.float32)


def mesh_rays(tris: np.ndarray, n: int, seed: int):
    """n float32 rays for one triangle set: from around three times the root box towards vertices, edge midpoints and
    centroids (ties between neighbours, u or v at 0 or 1) and towards random surface points, unnormalised lengths, some
    starting on the surface; then the degenerate ones (non-finite, zero, axis-parallel, tiny and huge directions)."""
    rng = np.random.default_rng(seed)
    v, finite = U.tri_f64(tris)
    lo, hi = K.root_box(tris)
    centre, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3 * max(float(np.abs(hi - lo).max()), 1e-30))
    k = n - len(BAD_RAYS)
    o = centre + rng.uniform(-1.5, 1.5, size=(k, 3)) * ext
    if finite.any():
        vf = v[finite]
        j = rng.integers(0, len(vf), size=k)
        kind = np.arange(k) % 4
        corner = vf[j, rng.integers(0, 3, size=k)]
        edge = 0.5 * (vf[j, 0] + vf[j, rng.integers(1, 3, size=k)])
        wts = rng.dirichlet((1.0, 1.0, 1.0), size=k)
        target = np.select([(kind == 0)[:, None], (kind == 1)[:, None], (kind == 2)[:, None]],
                           [corner, edge, vf[j].mean(axis=1)], (vf[j] * wts[:, :, None]).sum(1))
        on = np.arange(k) % 16 == 5  # these start on the surface: a hit at t near 0
        o[on] = (vf[rng.integers(0, len(vf), size=k)] * wts[:, :, None]).sum(1)[on]
    else:
        target = centre + rng.normal(size=(k, 3))
    d = (target - o) * rng.uniform(0.25, 4.0, size=(k, 1))
    with np.errstate(over="ignore"):
        o, d = o.astype(np.float32), d.astype(np.float32)
    return (np.ascontiguousarray(np.concatenate([o, BAD_RAYS[:, 0]])), np.ascontiguousarray(np.concatenate([d, BAD_RAYS[:, 1]])))


def cap_mix(t_first: np.ndarray, seed: int) -> np.ndarray:
    """A tmax array that mixes every class of rt_occluded's tmax over the rays: NaN, 0, -0, negative, +inf, FLT_MAX, exactly
    the first hit's t (that hit is left out), the next f32 above it (it is kept), a fraction and a multiple of it, tiny."""
    return K.cap_mix(t_first, seed)


def records(triangles, tree, o, d, k, **kw):
    return hrt.cast_rays_multi_host(triangles, tree, o, d, k, **kw)


def same_records(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """All 16 bytes of every record."""
    assert got.dtype == want.dtype == hrt.MULTI_HIT_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    x = np.frombuffer(got.tobytes(), dtype=np.uint32).reshape(-1, 4)
    y = np.frombuffer(want.tobytes(), dtype=np.uint32).reshape(-1, 4)
    rows = np.flatnonzero((x != y).any(axis=1))
    i = int(rows[0])
    k = max(got.shape[1], 1) if got.ndim == 2 else 1
    raise AssertionError(f"{what}: {len(rows)} of {len(x)} records differ; first at ray {i // k} rank {i % k}: "
                         f"{got.reshape(-1)[i]} != {want.reshape(-1)[i]}")


def paged(query, n: int, k: int, limit: int = 4096):
    """Every hit of n rays by pages of k: query(after) -> (n, k) records; the cursor is each ray's last record. Returns the
    list of pages up to and including the first page without a hit in its last rank."""
    pages, after = [], None
    for _ in range(limit):
        page = query(after)
        pages.append(page)
        if (page["prim"][:, k - 1] < 0).all():
            return pages
        after = np.ascontiguousarray(page[:, k - 1])
    raise AssertionError("paging did not end")


def ragged(pages):
    """Pages -> per ray the list of (t bits, prim, u bits, v bits) of its hits."""
    allp = np.concatenate(pages, axis=1)
    out = []
    for row in allp:
        hit = row[row["prim"] >= 0]
        out.append(np.frombuffer(hit.tobytes(), dtype=np.uint32).reshape(-1, 4).copy())
    return out


# ---- the definition's parts, restated
def f32_outward(x: np.ndarray, up: bool) -> np.ndarray:
    """rt_lbvh.hpp f32_outward: the f32 on that side of the f64 value, and one more ulp."""
    side = _F32(np.inf) if up else _F32(-np.inf)
    f = x.astype(np.float32)
    wrong = (f.astype(np.float64) < x) if up else (f.astype(np.float64) > x)
    f = np.where(wrong, np.nextafter(f, side), f).astype(np.float32)
    return np.nextafter(f, side).astype(np.float32)


def own_boxes(tris: np.ndarray, root: np.ndarray):
    """(lo, hi, finite): every triangle's own box relative to the root centre, f32, as the definition makes it."""
    v, finite = U.tri_f64(tris)
    v = v + 0.0  # (-0 -> +0)
    with np.errstate(invalid="ignore"):
        lo, hi = f32_outward(v.min(axis=1), False), f32_outward(v.max(axis=1), True)
    rc = root[:3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (lo.astype(np.float64) - rc).astype(np.float32), (hi.astype(np.float64) - rc).astype(np.float32), finite


def node_box(nodes: np.ndarray, node: int, side: int):
    w = nodes[node, 4 * side:4 * side + 3].astype(np.uint32)
    return ((w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32),
            (w >> 16).astype(np.uint16).view(np.float16).astype(np.float32))


def check_containment(tris: np.ndarray, tree: dict) -> int:
    """Every triangle's own box lies inside the decoded box of every one of its ancestors (the intersection of the
    ancestors' boxes is carried down). Returns the number of triangles checked."""
    nodes, order, root = tree["nodes"], tree["order"], tree["root"]
    lo, hi, finite = own_boxes(tris, root)
    inf = np.full(3, np.inf, dtype=np.float32)
    todo, checked = [(int(tree["info"][3]), -inf, inf)], 0
    while todo:
        word, alo, ahi = todo.pop()
        if word & LEAF_BIT:
            first, count = (word >> 4) & 0x07FFFFFF, word & 15
            for j in order[first:first + count].tolist():
                assert finite[j], j
                assert (lo[j] >= alo).all() and (hi[j] <= ahi).all(), (j, lo[j], hi[j], alo, ahi)
                checked += 1
            continue
        for side in range(2):
            blo, bhi = node_box(nodes, word, side)
            todo.append((int(nodes[word, 4 * side + 3]), np.maximum(alo, blo), np.minimum(ahi, bhi)))
    return checked


def _fma32(a, b, c):
    """fma in f32 through f64: the product is exact there; the sum is rounded twice, which differs from one rounding only
    on a tie of the second (about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _dot32(a, b):
    return _fma32(a[..., 2], b[..., 2], _fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(np.float32)))


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(np.float32)


def triangle_test_f32(o: np.ndarray, d: np.ndarray, tris: np.ndarray, chunk: int = 256):
    """The triangle test alone (rt_kernels.hip tri_t, numpy f32, no slab clause): (t (n, m) float32, accepted (n, m) bool)
    with accepted = the determinant, u and v tests and 1e-4 <= t < RT_T_MISS."""
    a = tris["a"][:, :3].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = (tris["b"][:, :3] - a).astype(np.float32), (tris["c"][:, :3] - a).astype(np.float32)
    n, m = len(o), len(a)
    T, OK = np.zeros((n, m), dtype=np.float32), np.zeros((n, m), dtype=bool)
    one = _F32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for s in range(0, n, chunk):
            oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
            dd = np.broadcast_to(dd, (dd.shape[0], m, 3))
            hh = _cross32(dd, e2[None])
            det = _dot32(np.broadcast_to(e1[None], hh.shape), hh)
            inv = (one / det).astype(np.float32)
            sv = (oo - a[None]).astype(np.float32)
            u = (inv * _dot32(sv, hh)).astype(np.float32)
            q = _cross32(sv, np.broadcast_to(e1[None], sv.shape))
            v = (inv * _dot32(dd, q)).astype(np.float32)
            t = (inv * _dot32(np.broadcast_to(e2[None], q.shape), q)).astype(np.float32)
            ok = ~(np.abs(det) < T_MIN) & ~((u < 0) | (u > 1)) & ~((v < 0) | ((u + v).astype(np.float32) > 1))
            ok &= (t >= T_MIN) & (t < MISS)
            T[s:s + chunk], OK[s:s + chunk] = t, ok
    return T, OK


def triangle_reference(o, d, tri):
    """Moller-Trumbore of ray k against triangle tri[k] in float64 (tests/test_gpu_cast_rays.py triangle_reference, with u
    and v): (t, u, v, kept mask, bound of t, of u, of v). The bound of t is that test's, 64 * 2^-24 |e1||e2|(|s| + t|d|) / |det|.
    u = s . (d x e2) / det and v = d . (s x e1) / det are quotients of the same kind: the numerator's rounding is a few
    2^-24 |s||d||e2| (|s||d||e1|), and the determinant's, a few 2^-24 |e1||e2||d|, enters times u (v) <= 1; with the same
    64: 64 * 2^-24 |d||e2|(|s| + |e1|) / |det| for u, 64 * 2^-24 |d||e1|(|s| + |e2|) / |det| for v."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    a, b, c = (tri[x][:, :3].astype(np.float64) for x in ("a", "b", "c"))
    e1, e2 = b - a, c - a
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    s = o - a
    u = (s * pv).sum(1) / det
    q = np.cross(s, e1)
    v = (d * q).sum(1) / det
    t = (e2 * q).sum(1) / det
    n1, n2, nd, ns = (np.linalg.norm(x, axis=1) for x in (e1, e2, d, s))
    kept = (np.abs(det) >= 1e-3 * n1 * n2 * nd) & (u >= 1e-3) & (v >= 1e-3) & (u + v <= 1.0 - 1e-3)
    bound = 64.0 * 2.0 ** -24 * n1 * n2 * (ns + t * nd) / np.abs(det)
    bu = 64.0 * 2.0 ** -24 * nd * n2 * (ns + n1) / np.abs(det)
    bv = 64.0 * 2.0 ** -24 * nd * n1 * (ns + n2) / np.abs(det)
    return t, u, v, kept, bound, bu, bv


# ---- the rays of the slab-clause study (tests/test_multihit_abi.py measures it; the GPU test reads `unchanged`)
_STUDY = {}


def suzanne_study():
    """Suzanne, its LBVH tree, the rays (80 x 45 pixel centres of SceneTris' Suzanne camera, then 1,000 of mesh_rays) and,
    per ray, whether the accepted set with the slab clause equals the set of the triangle test alone."""
    if "s" not in _STUDY:
        tris = U.mesh_triangles("suzanne.obj")
        tree = hrt.lbvh_build(tris, 0)
        co, cd = camera_rays(hrt.SceneTris.suzane_camera(), 80, 45)
        ro, rd = mesh_rays(tris, 1000, 19)
        o, d = np.concatenate([co, ro]), np.concatenate([cd, rd])
        t, ok = triangle_test_f32(o, d, tris)
        pages = paged(lambda after: records(tris, tree, o, d, 16, after=after, flat=True), len(o), 16)
        with_slab = ragged(pages)
        unchanged = np.zeros(len(o), dtype=bool)
        for i in range(len(o)):
            js = np.flatnonzero(ok[i])
            js = js[np.lexsort((js, t[i, js]))]
            unchanged[i] = (len(js) == len(with_slab[i]) and (with_slab[i][:, 1] == js).all()
                            and (with_slab[i][:, 0] == t[i, js].view(np.uint32)).all())
        _STUDY["s"] = (tris, tree, o, d, unchanged, with_slab)
    return _STUDY["s"]
