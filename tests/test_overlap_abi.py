"""rt_overlap_volumes on the host (rt_host_overlap_volumes; hrt.overlap_volumes_host): the symbols and statuses, the walk
against the flat definition on both builders and their refits, the box kind against a float64 statement of its thirteen
axes (inside a band, and exactly on dyadic cases), the ball kind against rt_closest_points' host definition, paging by
cursor, and the edges. CPU only; tests/test_gpu_overlap.py compares the device with these functions byte for byte.

Measured here: on 400 jittered boxes each against Suzanne (979 triangles, 391,600 pairs) and random1025
(410,000 pairs) the f32 flat answer and the f64 statement disagree on no pair; 2 and 0 pairs lie inside the band of
2^-18 S. With every eighth box a point of the mesh itself (sep = 0 up to the point's own rounding) 4 pairs of each mesh
disagree, all inside the band, the largest |sep| / S among them 5.5e-8 = 2^-24.1.

The host functions were also run once as a stand-alone program (scripts/overlap_sanitize.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: clean. Nothing loaded into Python was run under a sanitizer."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_util as U
import multihit_util as M
import overlap_util as V

ROOT = Path(__file__).resolve().parents[1]
PF = _lib._PF
MISS = V.MISS
BOX, BALL = V.BOX, V.BALL
CASES = dict(U.cpu_cases(), chain=M.chain)
N = 400


# ------------------------------------------------------------------------------------------------ symbols and statuses
def test_symbols_layout_and_header():
    L = hrt.lib()  # (the parent fails here: no such symbol)
    assert L.rt_overlap_volumes.restype is C.c_int
    header = (ROOT / "include" / "hrt.h").read_text()
    testing = (ROOT / "include" / "hrt_testing.h").read_text()
    names = ("rt_overlap_volumes", "rt_host_overlap_volumes")
    tnames = ("rt_testing_set_overlap_count", "rt_testing_get_overlap_counts")
    for name in names:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and getattr(L, name).restype is C.c_int
    for name in tnames:
        assert re.search(r"^int %s\(" % name, testing, re.M) and name not in header, name
        assert name in _lib.TESTING_SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert set(names + tnames) <= set(re.findall(r"\bT (rt_\w+)", out))
    assert "RT_ABI_VERSION 7u" in header
    comment = header[header.index("#define RT_ABI_VERSION"):header.index("int rt_abi_version")]
    assert "rt_overlap_volumes" in comment and "rt_host_overlap_volumes" in comment
    assert re.search(r"typedef struct rt_overlap_hit \{ float d2; int32_t prim; float v, w; \} rt_overlap_hit;", header)
    assert "#define RT_OVERLAP_MAX_K 16u" in header and hrt.OVERLAP_MAX_K == 16
    assert re.search(r"#define RT_VOLUME_BOX +1u", header) and re.search(r"#define RT_VOLUME_BALL +2u", header)
    assert (hrt.VOLUME_BOX, hrt.VOLUME_BALL) == (1, 2)
    dt = hrt.OVERLAP_HIT_DTYPE
    assert dt.itemsize == 16 and [dt.fields[k][1] for k in ("d2", "prim", "v", "w")] == [0, 4, 8, 12]


def tree_args(tris, tree):
    nodes, order = np.ascontiguousarray(tree["nodes"]), np.ascontiguousarray(tree["order"])
    root = np.ascontiguousarray(tree["root"], dtype=np.float32)
    keep = (tris, nodes, order, root)
    return keep, [tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes), order.ctypes.data_as(_lib._PU32), len(order),
                  int(tree["info"][3]), root.ctypes.data_as(PF)]


@pytest.mark.parametrize("kind", V.KINDS)
def test_statuses(kind):
    L = hrt.lib()
    tris = U.mesh_triangles("suzanne.obj")
    tree = hrt.lbvh_build(tris)
    keep, a = tree_args(tris, tree)
    vol = V.volumes_for(kind, tris, 32, 1)
    pv = vol.ctypes.data_as(PF)
    hits, cnt = np.zeros((32, 16), dtype=hrt.OVERLAP_HIT_DTYPE), np.zeros(32, dtype=np.uint32)
    ph, pc = hits.ctypes.data, cnt.ctypes.data_as(_lib._PU32)
    call = L.rt_host_overlap_volumes
    assert L.rt_overlap_volumes(None, kind, None, None, 4, 1, None, None) == _lib.RT_ERR_ARG
    assert call(*a, kind, pv, None, 32, 16, ph, pc) == _lib.RT_OK
    assert call(*a, kind, pv, None, 32, 16, ph, None) == _lib.RT_OK
    assert call(*a, kind, pv, None, 32, 0, None, pc) == _lib.RT_OK
    assert call(*a, kind, pv, None, 32, 17, ph, pc) == _lib.RT_ERR_ARG and b"RT_OVERLAP_MAX_K" in L.rt_last_error()
    assert call(*a, kind, pv, None, 0, 17, ph, pc) == _lib.RT_ERR_ARG  # for every n
    for unknown in (0, 3, 0xFFFFFFFF):
        assert call(*a, unknown, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG and b"kind" in L.rt_last_error()
    assert call(*a, kind, pv, None, 32, 0, ph, None) == _lib.RT_ERR_ARG and b"counts" in L.rt_last_error()
    assert call(*a, kind, pv, None, 32, 4, None, pc) == _lib.RT_ERR_ARG
    assert call(*a, kind, None, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a, kind, None, None, 0, 4, None, None) == _lib.RT_OK
    assert call(*a, kind, None, None, 0, 0, None, None) == _lib.RT_OK  # k = 0 without counts is refused with n > 0 only
    assert call(None, len(tris), *a[2:], kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(a[0], a[1], None, a[3], *a[4:], kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a[:4], None, a[5], *a[6:], kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG
    assert call(*a[:7], None, kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # the root is always read
    # bytes that are no tree over these triangles
    assert call(a[0], 5, *a[2:], kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # order entries past n_tris
    assert call(*a[:6], len(tree["nodes"]), a[7], kind, pv, None, 32, 4, ph, pc) == _lib.RT_ERR_ARG  # root past the slots
    bad = dict(tree, nodes=tree["nodes"].copy())
    bad["nodes"][0, 7] = bad["nodes"][0, 3]  # one child named twice
    with pytest.raises(hrt.RtError):
        V.records(tris, bad, kind, vol, 4)
    # the flat definition: no nodes, the root alone is read
    assert call(a[0], a[1], None, 0, None, 0, 0, a[7], kind, pv, None, 32, 16, ph, pc) == _lib.RT_OK
    flat, fc = V.records(tris, tree, kind, vol, 16, counts=True, flat=True)
    assert hits.tobytes() == flat.tobytes() and (cnt == fc).all()


# ------------------------------------------------------------------------------------------------ the walk is the definition
def trees_of(tris):
    """(name, triangles the tree is over, tree): both builders, and each refitted to the moved triangles."""
    moved = K.moved(tris, (0.375, -1.25, 2.0))
    out = []
    for b in V.BUILDERS:
        out.append((f"builder{b}", tris, hrt.lbvh_build(tris, b)))
        out.append((f"builder{b}-refit", moved, hrt.lbvh_refit(tris, moved, b)))
    return out


def check_order_and_fill(kind, rec, cnt, after=None):
    """What must hold of any answer: ascending without duplicates, beyond the cursor, miss records after the listed ones."""
    listed = np.minimum(cnt, rec.shape[1])
    rank = np.arange(rec.shape[1])[None, :]
    used = rank < listed[:, None]
    assert ((rec["prim"] >= 0) == used).all()
    unused = rec[~used]
    assert (unused["d2"] == MISS).all() and (unused["prim"] == -1).all()
    assert not unused["v"].view(np.uint32).any() and not unused["w"].view(np.uint32).any()
    d, p = rec["d2"], rec["prim"]
    if kind == BOX:
        assert (d[used] == 0).all() and not rec["v"][used].view(np.uint32).any() and not rec["w"][used].view(np.uint32).any()
    both = used[:, 1:]
    asc = (d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (p[:, :-1] < p[:, 1:]))
    assert asc[both].all()
    if after is not None:
        ad, ap = after["d2"][:, None], after["prim"][:, None]
        beyond = (ad < d) | ((ad == d) & (ap < p))
        assert beyond[used].all()


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_equals_the_flat_definition(name, kind):
    tris = CASES[name]()
    overflowed = False
    for tag, t, tree in trees_of(tris):
        vol = V.volumes_for(kind, t, N, 5)
        flat, fc = V.records(t, tree, kind, vol, 16, counts=True, flat=True)
        check_order_and_fill(kind, flat, fc)
        cursor = np.ascontiguousarray(flat[:, 1])  # a record of the query, or the miss record
        variants = [dict(), dict(after=cursor)]
        if kind == BALL:  # every class of cap on the radius column
            capped = vol.copy()
            capped[:, 3] = K.cap_mix(flat["d2"][:, 0], 3)
            variants += [dict(vol=capped), dict(vol=capped, after=cursor)]
        for kw in variants:
            kw = dict(kw)
            q = kw.pop("vol", vol)
            want, wc = V.records(t, tree, kind, q, 16, counts=True, flat=True, **kw)
            check_order_and_fill(kind, want, wc, kw.get("after"))
            for k in (0, 1, 4, 16):
                got, gc = V.records(t, tree, kind, q, k, counts=True, **kw)
                V.same_records(got, np.ascontiguousarray(want[:, :k]), f"{name} {tag} k = {k} {sorted(kw)} with counts")
                assert (gc == wc).all(), (name, tag, k, sorted(kw))
                if k:
                    V.same_records(V.records(t, tree, kind, q, k, **kw), np.ascontiguousarray(want[:, :k]),
                                   f"{name} {tag} k = {k} {sorted(kw)}")
        if name == "chain" and tag == "builder1":
            assert int(tree["info"][4]) > 24 and fc.max() >= 16  # deeper than the stack, and queries that hold it all
            overflowed = True
        if name in ("suzanne", "random1025", "planar") and "refit" not in tag:
            assert fc.max() >= 16 and (fc > 0).sum() > N // 4
    assert overflowed == (name == "chain")


# ------------------------------------------------------------------------------------------------ the box kind is the geometry
def compare_with_f64(name, tris, boxes):
    got = V.accepted_matrix(tris, hrt.lbvh_build(tris), boxes)
    sep, S, aabb = V.sat_f64(boxes, tris)
    want = sep <= 0.0
    in_band = np.abs(sep) < V.BAND * S
    differ = got != want
    worst = float((np.abs(sep) / S)[differ].max()) if differ.any() else 0.0
    edge_plane = aabb & ~want  # the boxes share a point and the f64 test separates: an edge or the plane axis did it
    print(f"{name}: {got.size} pairs, {int(aabb.sum())} with overlapping boxes, {int((in_band & aabb).sum())} of them in the band, "
          f"{int(edge_plane.sum())} separated by an edge or plane axis, {int(want.sum())} accepted, {int(differ.sum())} "
          f"disagreements, largest |sep| / S of one {worst:.3e} (band {V.BAND:.3e})")
    assert not (differ & ~in_band).any(), (int((differ & ~in_band).sum()), worst)
    return aabb, in_band, edge_plane, want


@pytest.mark.parametrize("name", ["suzanne", "random1025"])
def test_box_kind_against_f64_inside_a_band(name):
    """f32 flat answer == the f64 thirteen axes wherever |sep| >= 2^-18 S. Measured: on the 400 jittered boxes no pair
    disagrees on either mesh, and 2 (Suzanne) and 0 (random1025) pairs lie in the band. On boxes that are points of the mesh
    (vertices, centroids, edge midpoints: sep is 0 up to the rounding of the point) 4 pairs of each mesh disagree, the
    largest |sep| / S among them 5.5e-8 = 2^-24.1."""
    tris = CASES[name]()
    aabb, in_band, edge_plane, want = compare_with_f64(name, tris, V.boxes_for(tris, N, 11, bad=False, points=False))
    assert (in_band & aabb).sum() <= 1e-3 * aabb.sum()
    assert edge_plane.sum() >= 100
    assert want.sum() >= 1000
    compare_with_f64(name + ", with point boxes on the mesh", tris, V.boxes_for(tris, N, 11, bad=False))


def int_boxes():
    """Boxes with small integer or half bounds against the stack of squares ([0, 1]^2 at z = 1 .. 9)."""
    b = [[0, 0, 1, 1, 1, 1],            # the first square itself, flat
         [1, 0, 0.5, 2, 1, 2.5],        # touches squares 1 and 2 at the face x = 1: an edge of the lower, a corner of the upper
         [1, 1, 0, 2, 2, 3],            # touches at the corner (1, 1): both triangles of squares 1 to 3
         [-1, -1, 0, 0, 0, 9],          # the corner (0, 0) of every square
         [0, 1, 2, 1, 2, 2],            # the edge y = 1 of square 2: the upper triangle, and the lower one at (1, 1)
         [2, 0, 0, 3, 1, 9],            # misses by one unit in x
         [0, 0, 10, 1, 1, 11],          # misses by one unit in z
         [0.5, 0, 1.5, 1, 0.5, 2.5],    # the lower triangle of square 2 only... and the diagonal at (0.5, 0.5)
         [0, 0.5, 0.5, 0.5, 1, 1],      # square 1 from below, touching z = 1: the upper triangle, the diagonal at (0.5, 0.5)
         [0.5, 0.5, 3, 0.5, 0.5, 3],    # a point on the diagonal of square 3
         [0.25, 0.5, 4, 0.25, 0.5, 4],  # a point in the interior of the upper triangle of square 4
         [0.75, 0, 1, 1, 0.25, 9],      # a box in the lower triangles' corner, all nine squares
         [0, 0.75, 1, 0.25, 1, 9],      # the upper triangles' corner
         [0.5, 0, 0, 1.5, 0.5, 1]]      # touching the first square's plane from below, half outside
    return np.array(b, dtype=np.float32)


def test_exact_cases_on_the_stack_of_squares():
    tris = M.stack_of_squares(9)
    boxes = int_boxes()
    sep, _, _ = V.sat_f64(boxes, tris)
    want = sep <= 0.0  # touching (sep == 0) overlaps
    assert (sep == 0.0).sum() >= 20 and (sep == 1.0).sum() >= 2  # touching pairs, and misses by exactly one unit
    for b in (None, 0, 1):
        tree = hrt.lbvh_build(tris, b or 0)
        got = V.accepted_matrix(tris, tree, boxes, flat=b is None)
        assert (got == want).all(), np.argwhere(got != want)
    assert want[0].tolist() == [True, True] + [False] * 16
    assert want[1].tolist() == [True] * 4 + [False] * 14  # the upper triangles touch at the corner (1, 1)
    assert want[2].sum() == 6 and want[3].sum() == 18 and not want[5].any() and not want[6].any()
    assert np.flatnonzero(want[10]).tolist() == [7] and np.flatnonzero(want[9]).tolist() == [4, 5]


def test_exact_cases_on_the_planar_grid():
    """The grid's own coordinates are multiples of fl(0.37): exact touching is tried where the arithmetic is exact, at the
    faces x = 0 and y = 0, the corner at the origin and the plane z = Z (a box symmetric about 0 has c = 0 and h = Z)."""
    tris = U.planar_triangles()
    Z = float(tris["a"][0, 2])
    b = np.array([[-1, 0, -1, 0, 1, 1], [-1, -1, -1, 0, 0, 1], [0, -2, 0, 4, 0, 0.5], [-2, -2, -1, -1, -1, 1],
                  [0, 0, 0.5, 4, 4, 1], [0, 0, -Z, 1, 1, Z], [0, 0, -Z, 1, 1, 0], [0.5, 0.5, 0, 1.5, 1.5, 0.5],
                  [-1, -1, -Z, 0, 0, Z], [1, 1, 1, 2, 2, 2]], dtype=np.float32)
    sep, _, _ = V.sat_f64(b, tris)
    want = sep <= 0.0
    assert (sep == 0.0).sum() >= 10
    assert want[0].any() and want[1].sum() == 2 and want[2].any() and not want[3].any() and not want[4].any()
    assert want[5].any() and not want[6].any() and want[8].sum() == 2
    for bld in (None, 0, 1):
        got = V.accepted_matrix(tris, hrt.lbvh_build(tris, bld or 0), b, flat=bld is None)
        assert (got == want).all(), np.argwhere(got != want)


# ------------------------------------------------------------------------------------------------ the ball kind
def test_ball_record_0_is_closest_points():
    tris = U.mesh_triangles("suzanne.obj")
    tree = hrt.lbvh_build(tris)
    pts = K.query_points(tris, N, 4)
    free = hrt.closest_points_host(tris, pts)
    for caps in (None, K.cap_mix(free["d2"], 9)):
        want = hrt.closest_points_host(tris, pts, caps)
        vol = V.balls_for(tris, N, 4, caps)
        for flat in (True, False):
            got = V.records(tris, tree, BALL, vol, 1, flat=flat)[:, 0]
            for f in ("d2", "prim", "v", "w"):
                assert got[f].tobytes() == np.ascontiguousarray(want[f]).tobytes(), (f, flat)
    assert (want["prim"] < 0).sum() > N // 8 and (want["prim"] >= 0).sum() > N // 8  # the caps cut both ways


def test_ball_counts_are_the_triangles_below_the_cap():
    tris = U.random_triangles(64, 1064)
    tree = hrt.lbvh_build(tris)
    pts = K.query_points(tris, 100, 6)
    alone = np.stack([hrt.closest_points_host(tris[j:j + 1], pts)["d2"] for j in range(len(tris))], axis=1)  # (n, m)
    near = np.sort(alone, axis=1)[:, 5]  # the sixth smallest d2 of every point, as the cap: equality is excluded
    for caps, least in ((near, None), (K.cap_mix(near, 2), None), (np.full(100, 9.0, dtype=np.float32), 1)):
        caps = np.asarray(caps, dtype=np.float32)
        cap = np.where(caps > 0, np.minimum(caps, MISS), np.float32(0))  # (NaN: 0)
        want = (alone < cap[:, None]).sum(axis=1)
        vol = V.balls_for(tris, 100, 6, caps)
        for flat in (True, False):
            rec, cnt = V.records(tris, tree, BALL, vol, 16, counts=True, flat=flat)
            assert (cnt == want).all(), (flat, np.flatnonzero(cnt != want))
            j = np.argsort(np.where(alone < cap[:, None], alone, np.inf), axis=1, kind="stable")[:, :16]
            listed = np.minimum(want, 16)
            for i in range(100):
                assert rec["prim"][i, :listed[i]].tolist() == j[i, :listed[i]].tolist()
                assert rec["d2"][i, :listed[i]].tobytes() == alone[i, j[i, :listed[i]]].tobytes()
        if least:
            assert want.max() > 16
    fin = np.isfinite(pts).all(axis=1)
    assert (want[~fin] == 0).all() and (~fin).sum() == 6


# ------------------------------------------------------------------------------------------------ paging
@pytest.mark.parametrize("kind", V.KINDS)
def test_paging_continues_the_list(kind):
    tris = U.mesh_triangles("suzanne.obj")
    n = 60
    vol = V.boxes_for(tris, n, 13) if kind == BOX else V.balls_for(tris, n, 13, np.full(n, 0.05, dtype=np.float32))
    for tree, flat in ((hrt.lbvh_build(tris, 1), False), (hrt.lbvh_build(tris, 0), True)):
        _, cnt = V.records(tris, tree, kind, vol, 0, counts=True, flat=flat)
        assert cnt.max() > 40
        whole = V.ragged(V.paged(lambda after: V.records(tris, tree, kind, vol, 16, after=after, flat=flat), n, 16))
        got = V.ragged(V.paged(lambda after: V.records(tris, tree, kind, vol, 3, after=after, flat=flat), n, 3))
        for i, (a, b) in enumerate(zip(got, whole)):
            assert a.tobytes() == b.tobytes() and len(a) == cnt[i]
            key = a[:, 0].view(np.float32).astype(np.float64) * 2.0 ** 32 + a[:, 1]  # (d2, prim) as one ascending number
            assert (np.diff(a[:, 1].astype(np.int64)) != 0).all() and len(set(a[:, 1].tolist())) == len(a)
            assert (np.diff(a[:, 0].view(np.float32)) >= 0).all() and (kind == BALL or (np.diff(key) > 0).all())
        h, c = V.records(tris, tree, kind, vol, 3, after=V.miss_records(n), counts=True, flat=flat)
        assert (h["prim"] == -1).all() and (h["d2"] == MISS).all() and not c.any()
        first = V.records(tris, tree, kind, vol, 3, flat=flat)
        _, left = V.records(tris, tree, kind, vol, 0, after=np.ascontiguousarray(first[:, 2]), counts=True, flat=flat)
        assert left.tolist() == [max(len(w) - 3, 0) for w in whole]


# ------------------------------------------------------------------------------------------------ edges
def test_invalid_boxes_points_and_triangles():
    tris = U.mesh_triangles("suzanne.obj")
    tree = hrt.lbvh_build(tris)
    for flat in (True, False):
        rec, cnt = V.records(tris, tree, BOX, V.BAD_BOXES, 4, counts=True, flat=flat)
        assert not cnt[:V.N_INVALID].any() and (rec["prim"][:V.N_INVALID] == -1).all()
        assert (cnt[V.N_INVALID:] == len(tris)).all() and (rec["prim"][V.N_INVALID:] == [0, 1, 2, 3]).all()
    # a point box in a triangle's interior, and on a vertex
    v, _ = U.tri_f64(tris)
    j = 17
    inside = (v[j, 0] * 0.5 + v[j, 1] * 0.25 + v[j, 2] * 0.25).astype(np.float32)
    corner = tris["a"][j, :3]
    b = np.array([np.concatenate([inside, inside]), np.concatenate([corner, corner])], dtype=np.float32)
    sep, S, _ = V.sat_f64(b, tris)
    rec, cnt = V.records(tris, tree, BOX, b, 16, counts=True)
    for i in range(2):
        mine = set(rec["prim"][i, :cnt[i]].tolist())
        assert j in mine or abs(sep[i, j]) < V.BAND * S[i, j]
        assert mine >= set(np.flatnonzero(sep[i] <= -V.BAND * S[i]).tolist())
        assert mine <= set(np.flatnonzero(sep[i] < V.BAND * S[i]).tolist())
    assert j in set(rec["prim"][1, :cnt[1]].tolist()) and cnt[1] >= 3  # the vertex's fan
    # a non-finite triangle never answers, whatever the volume
    t = U.nan_triangles()
    tree = hrt.lbvh_build(t)
    huge = V.BAD_BOXES[V.N_INVALID:]
    balls = np.array([[0, 0, 0, np.inf], [1, 1, 1, 3e38]], dtype=np.float32)
    for flat in (True, False):
        for kind, vol in ((BOX, huge), (BALL, balls)):
            rec, cnt = V.records(t, tree, kind, vol, 16, counts=True, flat=flat)
            assert (cnt == 8).all() and sorted(rec["prim"][0, :8].tolist()) == [0, 1, 2, 3, 5, 6, 7, 8]
    # non-finite points
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, np.inf]], dtype=np.float32)
    rec, cnt = V.records(t, tree, BALL, bad, 2, counts=True)
    assert not cnt.any() and (rec["prim"] == -1).all()
