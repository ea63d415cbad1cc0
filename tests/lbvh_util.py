"""Shared by tests/test_lbvh_abi.py and tests/test_gpu_lbvh.py: the triangle sets the LBVH builder is tried on, and a
numpy reading of the tree format (include/hrt.h rt_host_lbvh_build) that checks a tree against its triangles."""
from __future__ import annotations

import numpy as np

import hrt
from hrt import Material, Mesh, Tree, Vec3, read_asset

LEAF_BIT = 0x80000000
LEAF_MAX = 4


def mesh_triangles(*assets: str) -> np.ndarray:
    """TRIANGLE_DTYPE records of OBJ assets (one Lambertian material each), as Tree.view() hands them out."""
    tree = None
    for a in assets:
        mesh = Mesh.load_obj(read_asset(a), Material.new_lambertian(Vec3(0.5, 0.5, 0.5)))
        if tree is None:
            tree = Tree.from_mesh(mesh)
        else:
            tree.add_mesh(mesh)
    tree.build()
    return tree.view()[2].copy()


def triangles_from_vertices(v: np.ndarray, material: int = 0) -> np.ndarray:
    """(m, 3, 3) float32 vertices -> TRIANGLE_DTYPE records."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3, 3)
    t = np.zeros((len(v),), dtype=hrt.TRIANGLE_DTYPE)
    for k, name in enumerate(("a", "b", "c")):
        t[name][:, :3] = v[:, k]
        t[name][:, 3] = 1.0
    t["custom"] = (0.0, 1.0, 0.0)
    t["material"] = material
    return t


def random_triangles(m: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4.0, 4.0, size=(m, 1, 3))
    return triangles_from_vertices(centre + rng.uniform(-0.3, 0.3, size=(m, 3, 3)))


def identical_triangles(m: int = 70) -> np.ndarray:
    return triangles_from_vertices(np.tile(np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]]]), (m, 1, 1)))


def planar_triangles(n: int = 10) -> np.ndarray:
    """A n x n grid of quads in the plane z = 0.25: one axis of the root box has no extent."""
    v = []
    for i in range(n):
        for j in range(n):
            p = [(i, j, 0.25), (i + 1, j, 0.25), (i + 1, j + 1, 0.25), (i, j + 1, 0.25)]
            v += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    return triangles_from_vertices(np.array(v, dtype=np.float32) * np.float32(0.37))


def nan_triangles() -> np.ndarray:
    t = random_triangles(9, 77)
    t["b"][4, 1] = np.nan
    return t


RANDOM_SIZES = (0, 1, 2, 3, 4, 5, 64, 65, 1025)


def cpu_cases() -> dict:
    """name -> a function that makes the triangles (meshes are loaded when asked for)."""
    cases = {"cube": lambda: mesh_triangles("cube.obj"), "quad": lambda: mesh_triangles("quad.obj"),
             "suzanne": lambda: mesh_triangles("suzanne.obj")}
    for m in RANDOM_SIZES:
        cases[f"random{m}"] = lambda m=m: random_triangles(m, 1000 + m)
    cases["identical70"] = identical_triangles
    cases["planar"] = planar_triangles
    cases["nan1of9"] = nan_triangles
    return cases


def tri_f64(tris: np.ndarray):
    """The vertices Moller-Trumbore sees, in f64: a, a + e1, a + e2 with e1 = b - a, e2 = c - a in f32; and which
    triangles are finite (every a, e1, e2 component)."""
    a = tris["a"][:, :3].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e1 = (tris["b"][:, :3] - a).astype(np.float32)
        e2 = (tris["c"][:, :3] - a).astype(np.float32)
    finite = np.isfinite(a).all(1) & np.isfinite(e1).all(1) & np.isfinite(e2).all(1)
    a64 = a.astype(np.float64)
    return np.stack([a64, a64 + e1.astype(np.float64), a64 + e2.astype(np.float64)], axis=1), finite


def child_box(word3: np.ndarray, root: np.ndarray):
    """The fp16 box of one child (three words [min | max << 16]) as absolute f64 (lo, hi) in long double."""
    w = np.asarray(word3, dtype=np.uint32)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.longdouble)
    hi = (w >> 16).astype(np.uint16).view(np.float16).astype(np.longdouble)
    rc = root[:3].astype(np.longdouble)
    return rc + lo, rc + hi


def check_tree(tris: np.ndarray, tree: dict) -> None:
    """Every structural property of the format, against the triangles."""
    v, finite = tri_f64(tris)
    nodes, order, info, root = tree["nodes"], tree["order"], tree["info"], tree["root"]
    m = int(finite.sum())
    assert int(info[2]) == m and int(info[1]) == m and len(order) == m
    assert len(nodes) == int(info[0]) == (m - 1 if m > LEAF_MAX else 0)
    assert list(info[5:]) == [0, 0, 0]
    root_word = int(info[3])
    assert root_word == ((LEAF_BIT | m) if m <= LEAF_MAX else 0)
    # the non-finite triangles are absent, every finite one is there once
    assert sorted(order.tolist()) == np.flatnonzero(finite).tolist()
    if m:
        lo, hi = v[finite].min(axis=(0, 1)), v[finite].max(axis=(0, 1))
        half = np.maximum(hi - root[:3].astype(np.float64), root[:3].astype(np.float64) - lo)
        assert float(root[3]) >= np.sqrt((half * half).sum())
    vl = v.astype(np.longdouble)
    seen_nodes, covered = set(), np.zeros(m, dtype=np.int64)
    max_depth = 0
    # (word, depth) -> the f64 box of the triangles beneath it; an explicit stack, children before parents
    boxes = {}
    stack = [(root_word, 0, False)]
    while stack:
        word, depth, done = stack.pop()
        if word & LEAF_BIT:
            first, count = (word >> 4) & 0x07FFFFFF, word & 15
            assert (1 <= count <= LEAF_MAX) or (m == 0 and count == 0), (first, count)
            assert first + count <= m
            covered[first:first + count] += 1
            max_depth = max(max_depth, depth)
            idx = order[first:first + count]
            if count:
                boxes[word] = (vl[idx].min(axis=(0, 1)), vl[idx].max(axis=(0, 1)))
            continue
        if not done:
            assert word < len(nodes) and word not in seen_nodes, word  # reachable once
            seen_nodes.add(word)
            stack.append((word, depth, True))
            stack.append((int(nodes[word, 3]), depth + 1, False))
            stack.append((int(nodes[word, 7]), depth + 1, False))
            continue
        sub = []
        for c in range(2):
            cw = int(nodes[word, 4 * c + 3])
            blo, bhi = child_box(nodes[word, 4 * c:4 * c + 3], root)
            tlo, thi = boxes[cw]
            assert (blo <= tlo).all() and (bhi >= thi).all(), (word, c)
            sub.append((tlo, thi))
        boxes[word] = (np.minimum(sub[0][0], sub[1][0]), np.maximum(sub[0][1], sub[1][1]))
    assert (covered == 1).all()
    assert int(info[4]) == max_depth
    unreferenced = np.ones(len(nodes), dtype=bool)
    unreferenced[list(seen_nodes)] = False
    assert not nodes[unreferenced].any()  # slots no child word names stay zero
    assert 0 not in {int(nodes[k, 3]) for k in seen_nodes} | {int(nodes[k, 7]) for k in seen_nodes}


def same_tree(a: dict, b: dict) -> None:
    for k in ("nodes", "order", "info", "root"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


def moller_trumbore(o: np.ndarray, d: np.ndarray, v: np.ndarray) -> np.ndarray:
    """t of one ray against triangles v (k, 3, 3) in f64, inf for a miss (t < 1e-4 or |det| < 1e-12 refused)."""
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    p = np.cross(d, e2)
    det = (e1 * p).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v[:, 0]
        u = (s * p).sum(1) * inv
        q = np.cross(s, e1)
        w = (q * d).sum(1) * inv
        t = (e2 * q).sum(1) * inv
        ok = (np.abs(det) >= 1e-12) & (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t >= 1e-4)
    return np.where(ok, t, np.inf)


def walk(o, d, v, tree):
    """Closest (t, triangle index) of one ray through the tree: slab tests on the decoded boxes themselves (they contain
    their triangles exactly; 1e-9 of the scale covers the f64 rounding of the test), the same Moller-Trumbore as the
    brute force at the leaves."""
    nodes, order, root = tree["nodes"], tree["order"], tree["root"]
    scale = float(root[3]) + float(np.abs(o).max()) + 1.0
    best, bj = np.inf, -1
    stack = [int(tree["info"][3])]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
    while stack:
        word = stack.pop()
        if word & LEAF_BIT:
            first, count = (word >> 4) & 0x07FFFFFF, word & 15
            idx = order[first:first + count]
            if count:
                t = moller_trumbore(o, d, v[idx])
                for tt, j in zip(t.tolist(), idx.tolist()):
                    if tt < best or (tt == best and j < bj):
                        best, bj = tt, j
            continue
        for c in range(2):
            lo, hi = child_box(nodes[word, 4 * c:4 * c + 3], root)
            lo, hi = lo.astype(np.float64) - 1e-9 * scale, hi.astype(np.float64) + 1e-9 * scale
            with np.errstate(invalid="ignore"):
                t0, t1 = (lo - o) * inv, (hi - o) * inv
            near, far = np.fmin(t0, t1), np.fmax(t0, t1)
            inside = (d != 0) | ((o >= lo) & (o <= hi))
            if inside.all() and np.nanmax(np.where(d != 0, near, -np.inf)) <= min(np.nanmin(np.where(d != 0, far, np.inf)), best):
                stack.append(int(nodes[word, 4 * c + 3]))
    return best, bj
