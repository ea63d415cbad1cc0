"""rt_winding_numbers on the host (rt_host_tree_moments, rt_host_winding_numbers; hrt.tree_moments_host,
hrt.winding_numbers_host): the symbols and statuses, the flat definition on known shapes, the written-out atan2 against
math.atan2, the moments, the accuracy of the tree walk against a float64 brute-force sum, tree independence, robustness
and the stack overflow. CPU only; tests/test_gpu_winding.py compares the device with these functions byte for byte.

Measured here (tests/winding_util.py MEASURED), largest |w - w_ref| over 800 points per mesh and both
builders: cube 2.86e-6 (beta = inf), 3.23e-3 (2), 2.86e-6 (3); ico_sphere 7.62e-7, 1.45e-2, 1.77e-3; Suzanne 2.48e-5,
4.05e-2, 9.07e-3. The tests assert four times these. atan2: largest error 2.73e-7, asserted 5.5e-7 (ATAN2_ERR).

The host functions were also run once as a stand-alone program (scripts/winding_sanitize.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: clean. Nothing loaded into Python was run under a sanitizer."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_util as U
import winding_util as W

ROOT = Path(__file__).resolve().parents[1]
INF = W.INF
CASES = dict(U.cpu_cases(), ico_sphere=lambda: W.mesh("ico_sphere"))
PF = _lib._PF


def flat(tris, pts):
    return hrt.winding_numbers_host(tris, None, np.asarray(pts, dtype=np.float32).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ symbols and statuses
def test_symbols_are_declared_exported_and_bound():
    L = hrt.lib()  # (the parent fails here: no such symbol)
    assert L.rt_winding_numbers.restype is C.c_int
    header = (ROOT / "include" / "hrt.h").read_text()
    testing = (ROOT / "include" / "hrt_testing.h").read_text()
    names = ("rt_winding_numbers", "rt_host_tree_moments", "rt_host_winding_numbers")
    tnames = ("rt_testing_set_winding_count", "rt_testing_get_winding_counts", "rt_testing_get_tree_moments",
              "rt_testing_winding_atan2")
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
    assert "rt_winding_numbers" in comment and "rt_host_tree_moments / rt_host_winding_numbers" in comment


def tree_args(tris, tree):
    nodes, order = np.ascontiguousarray(tree["nodes"]), np.ascontiguousarray(tree["order"])
    root = np.ascontiguousarray(tree["root"], dtype=np.float32)
    keep = (tris, nodes, order, root)
    return keep, [tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes), order.ctypes.data_as(_lib._PU32), len(order),
                  int(tree["info"][3]), root.ctypes.data_as(PF)]


def test_statuses_of_the_host_calls():
    L = hrt.lib()
    tris = W.mesh("suzanne")
    tree = hrt.lbvh_build(tris)
    keep, a = tree_args(tris, tree)
    pts = W.accuracy_points(tris)[:8]
    pp, out = pts.ctypes.data_as(PF), np.zeros(8, dtype=np.float32)
    po = out.ctypes.data_as(PF)
    assert L.rt_winding_numbers(None, None, 4, 0.0, None) == _lib.RT_ERR_ARG
    # beta classes
    for beta in (0.0, -0.0, 1.0, 2.0, 3.5, 1e30, INF):
        assert L.rt_host_winding_numbers(*a, pp, 8, beta, po) == _lib.RT_OK, beta
    for beta in (float("nan"), -1.0, -INF, 0.5, 1e-30, 0.99999994):
        assert L.rt_host_winding_numbers(*a, pp, 8, beta, po) == _lib.RT_ERR_ARG, beta
        assert b"beta" in L.rt_last_error()
    assert hrt.winding_numbers_host(tris, tree, pts, 0.0).tobytes() == hrt.winding_numbers_host(tris, tree, pts, 2.0).tobytes()
    # null pointers
    assert L.rt_host_winding_numbers(*a, None, 8, 0.0, po) == _lib.RT_ERR_ARG
    assert L.rt_host_winding_numbers(*a, pp, 8, 0.0, None) == _lib.RT_ERR_ARG
    assert L.rt_host_winding_numbers(*a, None, 0, 0.0, None) == _lib.RT_OK
    assert L.rt_host_winding_numbers(None, len(tris), *a[2:], pp, 8, 0.0, po) == _lib.RT_ERR_ARG
    assert L.rt_host_winding_numbers(a[0], a[1], None, a[3], *a[4:], pp, 8, 0.0, po) == _lib.RT_ERR_ARG
    assert L.rt_host_winding_numbers(*a[:4], None, a[5], *a[6:], pp, 8, 0.0, po) == _lib.RT_ERR_ARG
    assert L.rt_host_winding_numbers(*a[:7], None, pp, 8, 0.0, po) == _lib.RT_ERR_ARG
    # the flat definition: no nodes, and nothing else of the tree is read
    assert L.rt_host_winding_numbers(a[0], a[1], None, 0, None, 0, 0, None, pp, 8, 0.0, po) == _lib.RT_OK
    assert out.tobytes() == flat(tris, pts).tobytes()
    # the moments call's capacity rules
    slots = len(tree["nodes"])
    mom = np.zeros((slots + 1, 16), dtype=np.float32)
    assert L.rt_host_tree_moments(*a, mom.ctypes.data, slots - 1) == _lib.RT_ERR_ARG
    assert b"moment_cap" in L.rt_last_error()
    assert L.rt_host_tree_moments(*a, None, slots) == _lib.RT_ERR_ARG
    mom[:] = 7.0
    assert L.rt_host_tree_moments(*a, mom.ctypes.data, slots + 1) == _lib.RT_OK
    assert (mom[slots] == 7.0).all() and mom[:slots].tobytes() == hrt.tree_moments_host(tris, tree).tobytes()
    # bytes that are no tree over these triangles
    assert L.rt_host_tree_moments(a[0], 5, *a[2:], mom.ctypes.data, slots) == _lib.RT_ERR_ARG  # order entries past n_tris
    assert L.rt_host_tree_moments(*a[:6], slots, a[7], mom.ctypes.data, slots) == _lib.RT_ERR_ARG  # root past the slots
    bad = dict(tree, nodes=tree["nodes"].copy())
    bad["nodes"][0, 7] = bad["nodes"][0, 3]  # one child named twice
    with pytest.raises(hrt.RtError):
        hrt.tree_moments_host(tris, bad)
    with pytest.raises(hrt.RtError):
        hrt.winding_numbers_host(tris, bad, pts)


# ------------------------------------------------------------------------------------------------ the flat definition
@pytest.mark.parametrize("name", ["cube", "ico_sphere"])
def test_flat_is_one_inside_and_zero_far_outside(name):
    tris = W.mesh(name)
    lo, hi = K.root_box(tris)
    centre = 0.5 * (lo + hi)
    far = centre + np.array([[1000.0, 0, 0], [0, -300.0, 40.0], [1e6, 1e6, 1e6]]) * np.linalg.norm(hi - lo)
    w = flat(tris, np.concatenate([centre[None], far]))
    print(name, w)
    assert abs(float(w[0]) - 1.0) <= W.bound(name, INF)
    assert np.abs(w[1:]).max() <= W.bound(name, INF)


def test_one_triangle_on_its_axis_and_reversed():
    # the octant triangle seen from the origin, which lies on the axis through its centroid: Omega = 4 pi / 8
    v = np.array([[[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]], dtype=np.float32)
    tri, rev = U.triangles_from_vertices(v), U.triangles_from_vertices(v[:, ::-1])
    pts = np.array([[0, 0, 0], [0.1, 0.1, 0.1], [-2.0, -2.0, -2.0], [5.0, 5.0, 5.0]], dtype=np.float32)
    w, wr = flat(tri, pts), flat(rev, pts)
    print(w, wr)
    assert abs(float(w[0]) - 0.125) <= 4e-7  # (one atan2: ATAN2_ERR / 2 pi, and the f32 operands)
    # the regular pyramid's apex angle for the other axis points: Omega = 2 pi - 6 atan(...) by the f64 brute force
    assert np.abs(w - W.winding_f64(tri, pts)).max() <= 4e-7
    assert w[0] > 0 and w[1] > 0 and w[2] > 0 and w[3] < 0  # the far side sees it from behind
    assert np.abs(w + wr).max() <= 4e-7
    for s in (2.0 ** -100, 2.0 ** 100):  # scale invariance, exact for powers of two
        assert flat(W.scaled(tri, s), (pts.astype(np.float64) * s).astype(np.float32)).tobytes() == w.tobytes()


def test_points_on_the_surface_are_finite():
    for name in ("cube", "ico_sphere", "suzanne"):
        tris = W.mesh(name)
        v, _ = U.tri_f64(tris)
        on = np.concatenate([v[:, 0], 0.5 * (v[:, 0] + v[:, 1]), v.mean(axis=1)]).astype(np.float32)
        for tree in (None, hrt.lbvh_build(tris, 0), hrt.lbvh_build(tris, 1)):
            w = hrt.winding_numbers_host(tris, tree, on)
            assert np.isfinite(w).all() and np.abs(w).max() < 3.0


# ------------------------------------------------------------------------------------------------ atan2
def atan2(y, x):
    y, x = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(y)
    assert hrt.lib().rt_testing_winding_atan2(y.ctypes.data_as(PF), x.ctypes.data_as(PF), len(y), out.ctypes.data_as(PF)) == 0
    return out


def test_atan2_against_math_atan2():
    rng = np.random.default_rng(1)
    ang = np.concatenate([np.linspace(-math.pi, math.pi, 200001), rng.uniform(-math.pi, math.pi, 200000)])
    worst = 0.0

    def err(y, x):
        got = atan2(y, x)
        assert np.isfinite(got).all() and np.abs(got).max() <= np.float32(math.pi)
        return float(np.abs(got.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max())

    for _ in range(9):  # all quadrants, magnitudes 2^-20 .. 2^20
        r = 2.0 ** rng.uniform(-20, 20, size=len(ang))
        worst = max(worst, err((np.sin(ang) * r).astype(np.float32), (np.cos(ang) * r).astype(np.float32)))
    k = np.arange(-60, 61)
    for sy in (1.0, -1.0):  # ratios 2^-60 .. 2^60 either way, every sign: the axes' neighbourhoods
        for sx in (1.0, -1.0):
            for mant in (1.0, 1.3, 1.9):
                y, x = (sy * mant * 2.0 ** k).astype(np.float32), np.full(len(k), sx, dtype=np.float32)
                worst = max(worst, err(y, x), err(x, y))
    axes = np.array([1e-30, 1.0, 3e38], dtype=np.float32)  # the axes themselves
    for z in (0.0, -0.0):
        zz = np.full(3, z, dtype=np.float32)
        worst = max(worst, err(zz, axes), err(zz, -axes), err(axes, zz), err(-axes, zz))
    print(f"atan2_f32: largest error {worst:.3g}")
    assert worst <= 5.5e-7  # twice the largest error found (2.73e-7): rt_winding.hpp ATAN2_ERR


def test_atan2_special_cases_are_exact():
    pi, z = np.float32(3.14159265), np.float32(0.0)
    got = atan2([0.0, -0.0, 0.0, -0.0], [0.0, 0.0, -0.0, -0.0])
    assert got.view(np.uint32).tolist() == [0, 0, 0, 0]  # atan2(+-0, +-0) = +0
    got = atan2([0.0, -0.0, 0.0, -0.0], [-1.0, -1.0, -3e38, -1e-45])
    assert got.tolist() == [pi, -pi, pi, -pi]  # by the sign bit of the first argument
    assert atan2([0.0, -0.0], [2.0, 2.0]).view(np.uint32).tolist() == [0, 0x80000000]
    assert atan2([1.0, -1.0, 1.0, -1.0], [0.0, 0.0, -0.0, -0.0]).tolist() == [pi / 2, -pi / 2, pi / 2, -pi / 2]
    assert atan2([1.0, 1.0, -1.0, -1.0], [1.0, -1.0, 1.0, -1.0]).tolist() == [pi / 4, pi - pi / 4, -pi / 4, -(pi - pi / 4)]
    assert z == atan2([0.0], [0.0])[0]
    with np.errstate(invalid="ignore"):
        assert np.isfinite(atan2([np.inf, np.inf, 1.0, np.nan], [np.inf, 1.0, -np.inf, 1.0])).all()  # (never NaN)


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("builder", W.BUILDERS)
@pytest.mark.parametrize("name", list(CASES))
def test_moments(name, builder):
    tris = CASES[name]()
    tree = hrt.lbvh_build(tris, builder)
    mom = hrt.tree_moments_host(tris, tree)
    nodes, root_word = tree["nodes"], int(tree["info"][3])
    assert mom.shape == (len(nodes), 16) and mom.dtype == np.float32
    if root_word & W.LEAF_BIT:
        assert len(mom) == 0  # a tree without nodes gives no records
        return
    assert np.isfinite(mom).all() and not mom[:, [6, 7, 14, 15]].any()
    v, finite = U.tri_f64(tris)
    an = np.cross(v[finite][:, 1] - v[finite][:, 0], v[finite][:, 2] - v[finite][:, 0])
    (cl, nl), (cr, nr) = W.child_moments(mom, root_word, 0), W.child_moments(mom, root_word, 1)
    # each N is one f64 sum rounded to f32 once (half an ulp each); 1e-13: the f64 sums' own rounding
    tol = 2.0 ** -24 * (np.abs(nl) + np.abs(nr)) + 1e-13 * np.abs(an).sum(axis=0) + 1e-45
    assert (np.abs((nl + nr) - an.sum(axis=0)) <= tol).all(), (nl + nr, an.sum(axis=0))
    referenced = np.flatnonzero(nodes[:, 3] != 0)
    assert not mom[np.setdiff1d(np.arange(len(nodes)), referenced)].any()
    for node in referenced:
        for side in (0, 1):
            c, _ = W.child_moments(mom, int(node), side)
            lo, hi = W.child_box_rel(nodes, int(node), side)
            assert (lo <= c).all() and (c <= hi).all(), (node, side, lo, c, hi)


def test_zero_area_children_sit_at_the_box_centre():
    v = np.zeros((9, 3, 3), dtype=np.float32)  # nine zero-area triangles (segments) along x
    v[:, 0, 0], v[:, 1, 0], v[:, 2, 0] = np.arange(9), np.arange(9) + 0.5, np.arange(9) + 1.0
    tris = U.triangles_from_vertices(v)
    for builder in W.BUILDERS:
        tree = hrt.lbvh_build(tris, builder)
        mom = hrt.tree_moments_host(tris, tree)
        for node in np.flatnonzero(tree["nodes"][:, 3] != 0):
            for side in (0, 1):
                c, n = W.child_moments(mom, int(node), side)
                lo, hi = W.child_box_rel(tree["nodes"], int(node), side)
                assert not n.any() and (c == (0.5 * (lo + hi)).astype(np.float32)).all()
        pts = np.array([[4.0, 0, 0], [4.25, 0, 0], [3.0, 1.0, 2.0], [100.0, 0, 0]], dtype=np.float32)
        assert not hrt.winding_numbers_host(tris, tree, pts).any() and not flat(tris, pts).any()


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("builder", W.BUILDERS)
@pytest.mark.parametrize("name", W.MESHES)
def test_accuracy_against_the_f64_brute_force(name, builder):
    tris, pts, ref = W.accuracy_case(name)
    tree = hrt.lbvh_build(tris, builder)
    err = {}
    for beta in (INF, 2.0, 3.0):
        w = hrt.winding_numbers_host(tris, tree, pts, beta)
        err[beta] = float(np.abs(w - ref).max())
        print(f"{name} builder {builder} beta {beta}: largest |w - w_ref| = {err[beta]:.3g} (bound {W.bound(name, beta):.3g})")
        assert err[beta] <= W.bound(name, beta)  # (a), (b): four times the measured error
        assert W.bound(name, beta) < 0.25
        # (c) the sign, wherever the reference is not within 0.25 of one half
        clear = np.abs(ref - 0.5) >= 0.25
        assert (~clear).mean() <= 0.01
        assert ((w >= 0.5) == (ref >= 0.5))[clear].all()
    assert float(np.abs(flat(tris, pts) - ref).max()) <= W.bound(name, INF)
    _ERR[(name, builder)] = err


_ERR = {}


@pytest.mark.parametrize("name", W.MESHES)
def test_beta_3_is_more_accurate_than_beta_2(name):
    """The measured error of a mesh is the larger of its two trees' (W.MEASURED): at beta = 3 it is below the one at
    beta = 2. Per tree it is never above it; the cube's LBVH takes no dipole for any of the 800 points at either beta, so
    there both are the f32 figure of beta = inf, 2.86e-6."""
    for builder in W.BUILDERS:
        if (name, builder) not in _ERR:
            test_accuracy_against_the_f64_brute_force(name, builder)
        assert _ERR[(name, builder)][3.0] <= _ERR[(name, builder)][2.0]
    worst = {beta: max(_ERR[(name, b)][beta] for b in W.BUILDERS) for beta in (2.0, 3.0)}
    assert worst[3.0] < worst[2.0]
    assert W.MEASURED[name][3.0] < W.MEASURED[name][2.0]


@pytest.mark.parametrize("name", W.MESHES)
def test_trees_agree_within_their_bounds(name):
    tris, pts, ref = W.accuracy_case(name)
    f = flat(tris, pts).astype(np.float64)
    lbvh, ploc = hrt.lbvh_build(tris, 0), hrt.lbvh_build(tris, 1)
    for beta in (INF, 2.0, 3.0):
        a = hrt.winding_numbers_host(tris, lbvh, pts, beta).astype(np.float64)
        b = hrt.winding_numbers_host(tris, ploc, pts, beta).astype(np.float64)
        assert np.abs(a - b).max() <= 2 * W.bound(name, beta)
        assert np.abs(a - f).max() <= W.bound(name, beta) + W.bound(name, INF)
        assert np.abs(b - f).max() <= W.bound(name, beta) + W.bound(name, INF)


# ------------------------------------------------------------------------------------------------ robustness
@pytest.mark.parametrize("factor", [1e37, 1e-30])
def test_scaled_meshes(factor):
    base = W.mesh("ico_sphere")
    _, pts0, ref = W.accuracy_case("ico_sphere")
    tris = W.scaled(base, factor)
    with np.errstate(over="ignore"):
        pts = (pts0.astype(np.float64) * factor).astype(np.float32)
    assert np.isfinite(pts).all()
    ref = W.winding_f64(tris, pts)  # (of the scaled, rounded mesh)
    f = flat(tris, pts)
    assert np.isfinite(f).all() and np.abs(f - ref).max() <= W.bound("ico_sphere", INF)
    for builder in W.BUILDERS:
        tree = hrt.lbvh_build(tris, builder)
        assert len(tree["nodes"]) == 79
        for beta in (2.0, INF):  # the walk's range does not cover these points: the flat definition's bytes
            assert hrt.winding_numbers_host(tris, tree, pts, beta).tobytes() == f.tobytes()
        if factor < 1:  # covered points far from a tiny mesh: the moments underflow to nothing, as the true weight does
            away = np.array([[1.0, 0, 0], [0, -2.0, 0.5], [1e-6, 0, 0]], dtype=np.float32)
            w = hrt.winding_numbers_host(tris, tree, away, 2.0)
            assert np.isfinite(w).all() and np.abs(w).max() <= 1e-6


def test_degenerate_and_non_finite_input():
    tris = W.mesh("suzanne").copy()
    pts = K.query_points(tris, 512, 3, nonfinite=12)
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() == 12
    clean = flat(tris, pts)
    tris["b"][10, :3] = tris["a"][10, :3]            # zero-area: an edge
    tris["b"][11, :3] = tris["c"][11, :3] = tris["a"][11, :3]  # a point
    tris["c"][12, 1] = np.nan                         # a NaN vertex: contributes 0
    tris["a"][13, 0] = np.inf
    ok = tris.copy()
    ok["b"][12, :3] = ok["c"][12, :3] = ok["a"][12, :3]  # (the same mesh with those two as points: weight 0)
    ok["a"][13, :3] = 0.0
    ok["b"][13, :3] = ok["c"][13, :3] = 0.0
    want = flat(ok, pts)
    for tree in (None, hrt.lbvh_build(tris, 0), hrt.lbvh_build(tris, 1)):
        for beta in (2.0, INF):
            w = hrt.winding_numbers_host(tris, tree, pts, beta)
            assert (w[bad].view(np.uint32) == W.QNAN).all()  # the NaN pattern, exactly
            assert np.isfinite(w[~bad]).all()
            tol = 1e-4 if beta == INF else W.bound("suzanne", 2.0)
            assert np.abs(w[~bad] - want[~bad]).max() <= tol
    assert (clean[bad].view(np.uint32) == W.QNAN).all() and np.abs(clean[~bad] - want[~bad]).max() < 0.05
    # huge finite coordinates: a - p overflows f32, the triangle counts for nothing, nothing is NaN or infinite
    big = U.triangles_from_vertices(np.array([[[3e38, 0, 0], [3e38, 1e38, 0], [3e38, 0, 1e38]]], dtype=np.float32))
    w = flat(big, np.array([[-3e38, 0, 0], [3e38, 1e37, 1e37], [0, 0, 0]], dtype=np.float32))
    assert np.isfinite(w).all() and w[0] == 0


def test_uncovered_points_take_the_flat_definition():
    tris = W.mesh("suzanne")
    far = np.array([[2e18, 0, 0], [0, -3e25, 1.0], [1e30, 1e30, 1e30], [3e38, -3e38, 3e38]], dtype=np.float32)
    near = W.accuracy_points(tris)[:16]
    pts = np.ascontiguousarray(np.concatenate([far, near]))
    f = flat(tris, pts)
    for builder in W.BUILDERS:
        w = hrt.winding_numbers_host(tris, hrt.lbvh_build(tris, builder), pts, 2.0)
        assert w[:4].tobytes() == f[:4].tobytes() and np.isfinite(w).all()
        assert w[4:].tobytes() != f[4:].tobytes()  # (the covered ones took the walk)


# ------------------------------------------------------------------------------------------------ stack overflow
def test_overflowed_queries_return_the_flat_bytes():
    tris = K.chain_triangles(120)
    tree = hrt.lbvh_build(tris, 1)
    assert int(tree["info"][4]) == 60  # (the 230-triangle chain reaches 64, and lies outside the covered range)
    mom = hrt.tree_moments_host(tris, tree)
    pts = W.chain_points()
    f = flat(tris, pts)
    for beta in (2.0, INF):
        w = hrt.winding_numbers_host(tris, tree, pts, beta)
        over = np.array([W.walk_shape(tree, mom, p, beta)[0] for p in pts])
        print(f"chain120 beta {beta}: {over.sum()} of {len(pts)} queries overflow the stack")
        assert over.any()
        assert w[over].tobytes() == f[over].tobytes()
        assert np.isfinite(w).all() and np.abs(w - W.winding_f64(tris, pts)).max() < 0.25
    assert over.all()  # beta = inf: nothing is far, every query runs out of stack on the 60 levels
    lb = hrt.lbvh_build(tris, 0)  # the LBVH of the same chain is shallow: no query overflows
    assert int(lb["info"][4]) <= 24
    ml = hrt.tree_moments_host(tris, lb)
    assert not any(W.walk_shape(lb, ml, p, 2.0)[0] for p in pts[::8])
