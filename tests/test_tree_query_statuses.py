"""What the five host mirrors of the tree queries accept and refuse (rt_host_closest_points, rt_host_tree_moments,
rt_host_winding_numbers, rt_host_cast_rays_multi, rt_host_overlap_volumes), call by call: one table over quad.obj (2
triangles: the root is a leaf word, there are no nodes) and cube.obj (12 triangles: the smallest asset with nodes at
LEAF_MAX = 4), 5 queries each. CPU only.

EXPECTED was recorded at commit 821176f, before the mirrors came to share one host tree, and is the
behaviour to keep: a refused call's status is RT_ERR_ARG and its message is the text after "<function>: "; an accepted
call's outputs are the bytes of the same mirror's flat definition. The mirrors do not refuse the same calls — the winding
mirrors take a null root without nodes, the other two never; rt_host_cast_rays_multi refuses k = 0 without counts for
every n, rt_host_overlap_volumes for n > 0 only — and the table says so line by line. rt_host_winding_numbers with nodes
is no flat sum (it adds in tree order): its five words on the cube, and the CRC of the cube's moments, are recorded
likewise."""
import zlib

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_util as U
import multihit_util as M
import overlap_util as V

N = 5
LEAF = 0x80000000
TREE = ("tris", "n_tris", "hnodes", "node_slots", "order", "n_order", "root_word", "root")
FLAT = dict(hnodes=None, node_slots=0, order=None, n_order=0, root_word=LEAF)
# function -> (argument names in call order, the output arguments, (pointer, its count) pairs nulled in turn)
MIRRORS = {
    "rt_host_closest_points": (("tris", "n_tris", "points", "maxd2", "n", "out"), ("out",),
                               (("tris", "n_tris"), ("points", "n"), ("maxd2", "n"), ("out", "n"))),
    "rt_host_tree_moments": (TREE + ("moments_out", "moment_cap"), ("moments_out",),
                             (("tris", "n_tris"), ("hnodes", "node_slots"), ("order", "n_order"), ("root", None),
                              ("moments_out", "moment_cap"))),
    "rt_host_winding_numbers": (TREE + ("points", "n", "beta", "w_out"), ("w_out",),
                                (("tris", "n_tris"), ("hnodes", "node_slots"), ("order", "n_order"), ("root", None),
                                 ("points", "n"), ("w_out", "n"))),
    "rt_host_cast_rays_multi": (TREE + ("origins", "dirs", "tmax", "after", "n", "k", "hits", "counts"), ("hits", "counts"),
                                (("tris", "n_tris"), ("hnodes", "node_slots"), ("order", "n_order"), ("root", None),
                                 ("origins", "n"), ("dirs", "n"), ("tmax", "n"), ("after", "n"), ("hits", "n"),
                                 ("counts", "n"))),
    "rt_host_overlap_volumes": (TREE + ("kind", "volumes", "after", "n", "k", "hits", "counts"), ("hits", "counts"),
                                (("tris", "n_tris"), ("hnodes", "node_slots"), ("order", "n_order"), ("root", None),
                                 ("volumes", "n"), ("after", "n"), ("hits", "n"), ("counts", "n"))),
}
ROWS = [(f, None) for f in MIRRORS if f != "rt_host_overlap_volumes"] + [("rt_host_overlap_volumes", k) for k in V.KINDS]
# the substrings other tests pin, by case
PINS = {"k = 17": "_MAX_K", "kind = 3": "kind", "k = 0 without counts, n = 5": "counts", "beta = 0.5": "beta",
        "moment_cap below node_slots": "moment_cap"}
MAX_K = {"rt_host_cast_rays_multi": "RT_MULTI_HIT_MAX_K", "rt_host_overlap_volumes": "RT_OVERLAP_MAX_K"}
# rt_host_winding_numbers on the cube's tree at beta = +inf, and the CRC-32 of rt_host_tree_moments' records there (821176f)
CUBE_WINDING_WORDS = [0x3E000000, 0x31E52EE1, 0xB0A2F983, 0xAF9BB738, 0x7FC00000]
CUBE_MOMENTS_CRC = 0x8365986F


def base_arguments(fn: str, kind, asset: str) -> dict:
    tris = U.mesh_triangles(asset)
    tree = hrt.lbvh_build(tris)
    nodes = np.ascontiguousarray(tree["nodes"], dtype=np.uint32).reshape(-1, 8)
    order = np.ascontiguousarray(tree["order"], dtype=np.uint32)
    neutral = np.zeros(N, dtype=hrt.MULTI_HIT_DTYPE)  # a cursor before every record: (0, -1)
    neutral["prim"] = -1
    o, d = M.mesh_rays(tris, N + len(M.BAD_RAYS), 3)
    points = K.query_points(tris, N, 1, nonfinite=1)
    balls = np.ascontiguousarray(np.concatenate([points, np.full((N, 1), 4.0, dtype=np.float32)], axis=1))
    b = dict(tris=tris, n_tris=len(tris), hnodes=nodes if len(nodes) else None, node_slots=len(nodes), order=order,
             n_order=len(order), root_word=int(tree["info"][3]), root=np.ascontiguousarray(tree["root"], dtype=np.float32),
             points=points, maxd2=np.full(N, 4.0, dtype=np.float32), n=N, beta=float("inf"),
             origins=np.ascontiguousarray(o[:N]), dirs=np.ascontiguousarray(d[:N]), tmax=np.full(N, 1e30, dtype=np.float32),
             after=neutral, k=4, kind=kind, moment_cap=len(nodes),
             volumes=V.boxes_for(tris, N, 1, bad=False) if kind == V.BOX else balls)
    return {a: b[a] for a in MIRRORS[fn][0] if a in b}


def cases(fn: str, b: dict):
    """(name, the arguments that differ from the well-formed call)."""
    yield "tree", {}
    if "hnodes" in b:
        yield "flat", FLAT
    for ptr, count in MIRRORS[fn][2]:
        if ptr != "hnodes":
            yield f"{ptr} null", {ptr: None}
        if count:
            yield f"{ptr} null, {count} = 0", {ptr: None, count: 0}
    if "hnodes" in b:
        some = b["hnodes"] if b["hnodes"] is not None else np.zeros((1, 8), dtype=np.uint32)
        yield "node_slots without nodes", dict(hnodes=None, node_slots=max(b["node_slots"], 1))
        yield "nodes without node_slots", dict(hnodes=some, node_slots=0)
        yield "root_word = node_slots", dict(root_word=b["node_slots"])
        yield "root_word = node_slots + 1", dict(root_word=b["node_slots"] + 1)
        yield "node_slots = 2^26", dict(hnodes=some, node_slots=1 << 26)  # refused before a byte of `some` is read
    if "k" in b:
        yield "k = 17", dict(k=17)
        yield "k = 0 without counts, n = 0", dict(k=0, hits=None, counts=None, n=0)
        yield "k = 0 without counts, n = 5", dict(k=0, hits=None, counts=None)
        yield "k = 0 with counts", dict(k=0, hits=None)
    if "kind" in b:
        yield "kind = 3", dict(kind=3)
    if "beta" in b:
        yield "beta = 0.5", dict(beta=0.5)
    if "moment_cap" in b:
        yield "moment_cap below node_slots", dict(moment_cap=max(b["node_slots"], 1) - 1)


def fresh_outputs(fn: str, v: dict) -> dict:
    """The output buffers of one call, filled with a pattern: what a call leaves alone compares equal."""
    shapes = {"out": (N, 8), "w_out": (N,), "hits": (N, 17, 4), "counts": (N,), "moments_out": (max(v.get("node_slots", 0), 1), 16)}
    return {a: np.full(shapes[a], 0xABABABAB, dtype=np.uint32) for a in MIRRORS[fn][1]}


def call(fn: str, v: dict):
    """One call with fresh output buffers where v holds one (an output given as None stays null): status, message, outputs."""
    outs = fresh_outputs(fn, v)
    args = []
    for name, ctype in zip(MIRRORS[fn][0], _lib.SIGNATURES[fn][1]):
        x = v[name] if name not in outs else outs[name] if v[name] is not None else None
        if isinstance(x, np.ndarray):
            x = x.ctypes.data if ctype is _lib._P else x.ctypes.data_as(ctype)
        args.append(x)
    L = hrt.lib()
    rc = getattr(L, fn)(*args)
    return rc, (L.rt_last_error() or b"").decode() if rc else "", outs


def observe(fn: str, kind, asset: str) -> dict:
    """case -> what the call answered: None when accepted, else the message after '<function>: '."""
    b = base_arguments(fn, kind, asset)
    seen = {}
    for name, change in cases(fn, b):
        v = dict(b, **change)
        for out in MIRRORS[fn][1]:
            v.setdefault(out, True)
        rc, msg, outs = call(fn, v)
        if rc == _lib.RT_OK:
            seen[name] = None
            check_outputs(fn, asset, name, v, outs)
            continue
        assert rc == _lib.RT_ERR_ARG and msg.startswith(fn + ": "), (fn, name, rc, msg)
        seen[name] = msg[len(fn) + 2:]
        pin = PINS.get(name)
        if pin:
            assert (MAX_K[fn] if pin == "_MAX_K" else pin) in msg, (fn, name, msg)
    return seen


def check_outputs(fn: str, asset: str, name: str, v: dict, outs: dict) -> None:
    """An accepted call's bytes are the flat definition's for the same queries."""
    if fn == "rt_host_closest_points":
        n = v["n"]
        tris = (v["tris"] if v["tris"] is not None else np.zeros(0, dtype=hrt.TRIANGLE_DTYPE))[:v["n_tris"]]
        want = hrt.closest_points_host(tris, v["points"][:n], None if v["maxd2"] is None else v["maxd2"][:n]) if n else None
        if n and v["out"] is not None:
            assert outs["out"][:n].tobytes() == want.tobytes(), (fn, asset, name)
        return
    walked = v["node_slots"] != 0
    if fn == "rt_host_tree_moments":
        if walked and v["moments_out"] is not None:
            assert asset == "cube.obj" and zlib.crc32(outs["moments_out"].tobytes()) == CUBE_MOMENTS_CRC, (fn, asset, name)
        return
    if fn == "rt_host_winding_numbers" and walked:
        if v["n"] and v["w_out"] is not None:
            assert asset == "cube.obj" and outs["w_out"].tolist() == CUBE_WINDING_WORDS, (fn, asset, name)
        return
    rc, msg, want = call(fn, dict(v, **FLAT))
    assert rc == _lib.RT_OK, (fn, asset, name, msg)
    for a in outs:
        assert outs[a].tobytes() == want[a].tobytes(), (fn, asset, name, a)


# function -> case -> the answer on (quad.obj, cube.obj), or one answer for both; None: accepted
EXPECTED = {
    "rt_host_closest_points": {
        "tree": None,
        "tris null": "null triangles",
        "tris null, n_tris = 0": None,
        "points null": "null points or out",
        "points null, n = 0": None,
        "maxd2 null": None,
        "maxd2 null, n = 0": None,
        "out null": "null points or out",
        "out null, n = 0": None,
    },
    "rt_host_tree_moments": {
        "tree": None,
        "flat": None,
        "tris null": "null triangles",
        "tris null, n_tris = 0": (None, "the nodes are not a tree over order and the triangles"),
        "hnodes null, node_slots = 0": None,
        "order null": "null order",
        "order null, n_order = 0": (None, "the nodes are not a tree over order and the triangles"),
        "root null": (None, "null nodes or root"),
        "moments_out null": (None, "null output"),
        "moments_out null, moment_cap = 0": (None, "moment_cap is below node_slots"),
        "node_slots without nodes": "null nodes or root",
        "nodes without node_slots": None,
        "root_word = node_slots": (None, "the root word names a node past node_slots"),
        "root_word = node_slots + 1": (None, "the root word names a node past node_slots"),
        "node_slots = 2^26": "2^26 or more node slots or positions",
        "moment_cap below node_slots": (None, "moment_cap is below node_slots"),
    },
    "rt_host_winding_numbers": {
        "tree": None,
        "flat": None,
        "tris null": "null triangles",
        "tris null, n_tris = 0": (None, "the nodes are not a tree over order and the triangles"),
        "hnodes null, node_slots = 0": None,
        "order null": "null order",
        "order null, n_order = 0": (None, "the nodes are not a tree over order and the triangles"),
        "root null": (None, "null nodes or root"),
        "points null": "null points or w_out",
        "points null, n = 0": None,
        "w_out null": "null points or w_out",
        "w_out null, n = 0": None,
        "node_slots without nodes": "null nodes or root",
        "nodes without node_slots": None,
        "root_word = node_slots": (None, "the root word names a node past node_slots"),
        "root_word = node_slots + 1": (None, "the root word names a node past node_slots"),
        "node_slots = 2^26": "2^26 or more node slots or positions",
        "beta = 0.5": "beta must be 0 (the default 2.0) or at least 1 (+inf: no dipoles)",
    },
    "rt_host_cast_rays_multi": {
        "tree": None,
        "flat": None,
        "tris null": "null triangles",
        "tris null, n_tris = 0": (None, "the nodes are not a tree over order and the triangles"),
        "hnodes null, node_slots = 0": None,
        "order null": (None, "null order"),
        "order null, n_order = 0": (None, "the nodes are not a tree over order and the triangles"),
        "root null": "null root",
        "origins null": "null rays or hits",
        "origins null, n = 0": None,
        "dirs null": "null rays or hits",
        "dirs null, n = 0": None,
        "tmax null": None,
        "tmax null, n = 0": None,
        "after null": None,
        "after null, n = 0": None,
        "hits null": "null rays or hits",
        "hits null, n = 0": None,
        "counts null": None,
        "counts null, n = 0": None,
        "node_slots without nodes": "nodes and node_slots disagree",
        "nodes without node_slots": "nodes and node_slots disagree",
        "root_word = node_slots": (None, "the nodes are not a tree over order and the triangles"),
        "root_word = node_slots + 1": (None, "the nodes are not a tree over order and the triangles"),
        "node_slots = 2^26": "2^26 or more node slots or positions",
        "k = 17": "k exceeds RT_MULTI_HIT_MAX_K",
        "k = 0 without counts, n = 0": "k = 0 needs counts",
        "k = 0 without counts, n = 5": "k = 0 needs counts",
        "k = 0 with counts": None,
    },
    "rt_host_overlap_volumes": {
        "tree": None,
        "flat": None,
        "tris null": "null triangles",
        "tris null, n_tris = 0": (None, "the nodes are not a tree over order and the triangles"),
        "hnodes null, node_slots = 0": None,
        "order null": (None, "null order"),
        "order null, n_order = 0": (None, "the nodes are not a tree over order and the triangles"),
        "root null": "null root",
        "volumes null": "null volumes or hits",
        "volumes null, n = 0": None,
        "after null": None,
        "after null, n = 0": None,
        "hits null": "null volumes or hits",
        "hits null, n = 0": None,
        "counts null": None,
        "counts null, n = 0": None,
        "node_slots without nodes": "nodes and node_slots disagree",
        "nodes without node_slots": "nodes and node_slots disagree",
        "root_word = node_slots": (None, "the nodes are not a tree over order and the triangles"),
        "root_word = node_slots + 1": (None, "the nodes are not a tree over order and the triangles"),
        "node_slots = 2^26": "2^26 or more node slots or positions",
        "k = 17": "k exceeds RT_OVERLAP_MAX_K",
        "k = 0 without counts, n = 0": None,
        "k = 0 without counts, n = 5": "k = 0 needs counts",
        "k = 0 with counts": None,
        "kind = 3": "unknown kind",
    },
}


@pytest.mark.parametrize("fn,kind", ROWS)
def test_statuses_of_the_host_mirrors(fn, kind):
    for col, asset in enumerate(("quad.obj", "cube.obj")):
        seen = observe(fn, kind, asset)
        want = {c: (a[col] if isinstance(a, tuple) else a) for c, a in EXPECTED[fn].items()}
        assert seen == want, {c: (seen.get(c), want.get(c)) for c in set(seen) | set(want) if seen.get(c) != want.get(c)}
