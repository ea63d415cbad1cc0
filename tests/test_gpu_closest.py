"""rt_closest_points on the GPU: the device records are the host definition's (hrt.closest_points_host), all 32 bytes,
through every tree the renderer can hold (device LBVH and PLOC, refitted, the host SAH tree of tri_bvh = 1), through trees
without nodes, the walk's stack overflow and the points its error bound does not cover; the counting instantiation shows
that the walk culls; statuses; and nothing of a draw's state moves. No tolerance anywhere: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_refit_util as R
import lbvh_util as U
import test_gpu_cast_rays as CR
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device
from test_gpu_lbvh_refit import host_sah_renderer

pytestmark = pytest.mark.gpu

N = 2000
PLOC = 1
STACK = 24
CASES = dict(U.cpu_cases(), chain230=K.chain_triangles, chain120=lambda: K.chain_triangles(120))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


_MIRROR = {}


def mirror(name):
    """(triangles, points, caps, host records without caps, host records with them), made once per case."""
    if name not in _MIRROR:
        tris = CASES[name]() if name in CASES else U.mesh_triangles(name)
        pts = K.query_points(tris, N, 100 + len(tris))
        free = hrt.closest_points_host(tris, pts)
        caps = K.cap_mix(free["d2"], 7)
        _MIRROR[name] = (tris, pts, caps, free, hrt.closest_points_host(tris, pts, caps))
    return _MIRROR[name]


def records(r, pts, caps=None) -> np.ndarray:
    return r.closest_records(pts, caps).cpu().numpy().view(hrt.CLOSEST_DTYPE).reshape(-1)


def tris_renderer(tris, builder=0, materials=ONE_MATERIAL):
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), materials, builder=builder)
    return r


def same(got, want):
    assert K.records_equal(got, want), K.first_difference(got, want)


# ------------------------------------------------------------------------------------------------ equality with the mirror
@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("name", list(CASES))
def test_device_records_are_the_mirrors(name, builder):
    tris, pts, caps, free, capped = mirror(name)
    r = tris_renderer(tris, builder)
    same(records(r, pts), free)
    same(records(r, pts, caps), capped)
    if name in ("suzanne", "random1025", "planar"):
        finite = np.isfinite(pts).all(axis=1)
        assert (free["prim"][finite] >= 0).all() and (free["prim"][~finite] == -1).all()
        assert 0 < (capped["prim"] >= 0).sum() < finite.sum()
        assert (free["d2"] == 0).sum() > 100  # the vertices and centroids
    d = r.closest_points(pts[:64], 1e30)  # the dict, and a float for every point
    assert d["d2"].cpu().numpy().tobytes() == free["d2"][:64].tobytes()
    assert d["prim"].cpu().numpy().tolist() == free["prim"][:64].tolist()
    assert d["point"].cpu().numpy().tobytes() == np.ascontiguousarray(free["p"][:64]).tobytes()
    assert d["v"].cpu().numpy().tobytes() == free["v"][:64].tobytes()
    assert d["w"].cpu().numpy().tobytes() == free["w"][:64].tobytes()


@pytest.mark.parametrize("scene", ["cube", "suzane", "mixed"])
def test_host_sah_tree_answers_the_same(scene):
    sd = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}[scene](32, 24)
    tris = sd.bvh[2]
    r = host_sah_renderer(sd)
    assert int(r.tri_tree_info()[0]) == 0xFFFFFFFF
    pts = K.query_points(tris, N, 5)
    if scene == "mixed":  # points on and inside the spheres too: only triangles answer
        pts = np.ascontiguousarray(np.concatenate([pts, sd.spheres["center"].astype(np.float32)]))
        assert sd.mode == hrt.RT_MODE_MIXED and len(sd.spheres) > 4
    free = hrt.closest_points_host(tris, pts)
    caps = K.cap_mix(free["d2"], 3)
    same(records(r, pts), free)
    same(records(r, pts, caps), hrt.closest_points_host(tris, pts, caps))
    assert (free["prim"][np.isfinite(pts).all(axis=1)] >= 0).all() and free["prim"].max() < len(tris)


@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("kind", ["translate", "jitter"])
def test_refitted_tree_answers_for_the_moved_mesh(kind, builder):
    a = U.mesh_triangles("suzanne.obj")
    b = R.deform(a, kind)
    r = tris_renderer(a, builder)
    r.refit_triangles_device(on_device(r, b))
    pts = K.query_points(b, N, 21)
    free = hrt.closest_points_host(b, pts)
    caps = K.cap_mix(free["d2"], 8)
    same(records(r, pts), free)
    same(records(r, pts, caps), hrt.closest_points_host(b, pts, caps))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_counts_write_exactly_n_records(n):
    import torch

    tris, pts, caps, free, capped = mirror("suzanne")
    r = tris_renderer(tris)
    dev = r._torch_device()
    p = torch.from_numpy(pts[:n].copy()).to(dev)
    out = torch.full((n + 3, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    assert hrt.lib().rt_closest_points(r._h, C.c_void_p(p.data_ptr()), None, n, C.c_void_p(out.data_ptr())) == _lib.RT_OK
    r.synchronize()
    got = out.cpu().numpy()
    same(got[:n].view(hrt.CLOSEST_DTYPE).reshape(-1), free[:n])
    assert (got[n:] == 0x5A5A5A5A).all()


def test_every_tree_gives_the_same_records():
    sd = CR.suzane_scene(16, 16)
    tris, mats = sd.bvh[2], sd.bvh[3]
    pts = K.query_points(tris, N, 12)
    free = hrt.closest_points_host(tris, pts)
    caps = K.cap_mix(free["d2"], 13)
    capped = hrt.closest_points_host(tris, pts, caps)
    refitted = tris_renderer(R.deform(tris, "jitter"), PLOC, mats)
    refitted.refit_triangles_device(on_device(refitted, tris))  # another topology, these positions
    trees = {"lbvh": tris_renderer(tris, 0, mats), "ploc": tris_renderer(tris, PLOC, mats), "refitted": refitted,
             "host": host_sah_renderer(sd)}
    assert [int(t.tri_tree_info()[0]) for t in trees.values()] == [0, 1, 1, 0xFFFFFFFF]
    for name, r in trees.items():
        assert K.records_equal(records(r, pts), free), name
        assert K.records_equal(records(r, pts, caps), capped), name


# ------------------------------------------------------------------------------------------------ counters
def counted(r, pts, caps=None):
    r.set_closest_count(True)
    rec = records(r, pts, caps)
    c = [int(x) for x in r.closest_counts()]
    r.set_closest_count(False)
    return rec, c


def test_counters_show_a_culling_walk():
    tris = U.mesh_triangles("suzanne.obj")
    m = len(tris)
    v, _ = U.tri_f64(tris)
    rng = np.random.default_rng(2)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=N)
    near = ((v[rng.integers(0, m, size=N)] * w[:, :, None]).sum(1) + rng.normal(size=(N, 3)) * 0.01).astype(np.float32)
    for builder in (0, PLOC):
        r = tris_renderer(tris, builder)
        assert r.closest_counts().tolist() == [0, 0, 0, 0]
        rec, c = counted(r, near)
        print(f"suzanne builder {builder}: {c[1] / c[0]:.1f} triangle tests per query of {m}, depth {r.tri_tree_info()[4]}")
        same(rec, hrt.closest_points_host(tris, near))
        assert c[0] == N and c[3] == 0
        assert c[1] / c[0] < m / 4  # (an always-brute-force kernel has m: this is no performance claim)
        # non-finite points take the loop over all triangles, and only they
        pts = K.query_points(tris, 512, 9, nonfinite=12)
        rec, c = counted(r, pts)
        same(rec, hrt.closest_points_host(tris, pts))
        assert c[0] == 512 and c[3] == 12 and c[1] >= 12 * m
        # a tiny search radius far away: nothing is tested, everything misses
        far = pts[np.isfinite(pts).all(axis=1)][-100:]
        assert np.linalg.norm(far, axis=1).min() > 100
        rec, c = counted(r, far, 2.0 ** -20)
        assert c[0] == len(far) and c[1] * 100 <= c[0] and c[3] == 0
        assert (rec["prim"] == -1).all() and (rec["d2"] == K.MISS).all()
        assert K.records_equal(records(r, near), hrt.closest_points_host(tris, near))  # counting off again: same records


def test_a_deep_tree_overflows_the_stack_and_still_answers():
    """The 120-triangle chain ends at x = 21, inside the walk's bound: its PLOC tree is 64 deep, and a point left of it finds
    the deep child nearer at every level, so the stack of 24 overflows. The 230-triangle chain reaches x = 6e36, where
    D = |p - rc| + radius is past the bound's range for every point: all of them take the loop, none the walk."""
    tris = K.chain_triangles(120)
    r = tris_renderer(tris, PLOC)
    assert int(r.tri_tree_info()[4]) > STACK
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-1.0, 1.0, size=(256, 3)) - [3.0, 0.0, 0.0], K.query_points(tris, 256, 6, nonfinite=0)])
    pts = np.ascontiguousarray(pts.astype(np.float32))
    rec, c = counted(r, pts)
    print(f"chain120: {c[2]} of {c[0]} queries overflowed the stack")
    same(rec, hrt.closest_points_host(tris, pts))
    assert c[0] == len(pts) and c[2] > 0 and c[3] == 0
    big = K.chain_triangles(230)
    r = tris_renderer(big, PLOC)
    assert int(r.tri_tree_info()[4]) == 64
    rec, c = counted(r, pts)
    same(rec, hrt.closest_points_host(big, pts))
    assert c == [len(pts), len(pts) * 230, 0, len(pts)]


# ------------------------------------------------------------------------------------------------ statuses and state
def test_statuses():
    import torch

    L = hrt.lib()
    tris, pts, caps, free, capped = mirror("suzanne")
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    dev = sph._torch_device()
    p = torch.from_numpy(pts[:64].copy()).to(dev)
    out = torch.zeros((65, 8), dtype=torch.int32, device=dev)
    pp, po = C.c_void_p(p.data_ptr()), C.c_void_p(out.data_ptr())
    torch.cuda.synchronize(dev)
    assert L.rt_closest_points(sph._h, pp, None, 64, po) == _lib.RT_ERR_ARG
    assert b"sphere program" in L.rt_last_error()
    r = tris_renderer(tris)
    assert L.rt_closest_points(r._h, pp, None, 0, po) == _lib.RT_OK  # n = 0, and null buffers with it
    assert L.rt_closest_points(r._h, None, None, 0, None) == _lib.RT_OK
    for args in ((None, None, 64, po), (pp, None, 64, None),                       # null
                 (C.c_void_p(p.data_ptr() + 2), None, 32, po),                     # misaligned points
                 (pp, C.c_void_p(p.data_ptr() + 1), 32, po),                       # misaligned maxd2
                 (pp, None, 32, C.c_void_p(out.data_ptr() + 8))):                  # out not 16-byte aligned
        assert L.rt_closest_points(r._h, *args) == _lib.RT_ERR_ARG, args
        assert b"rt_closest_points" in L.rt_last_error()
    r.synchronize()
    assert not out.cpu().numpy().any()  # nothing was written by a refused call
    with pytest.raises(ValueError):
        r.closest_points(pts[:4], np.zeros(5, dtype=np.float32))
    # no tree: tri_bvh = 0 and no device geometry
    sd = CR.suzane_scene(16, 16)
    h = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    assert L.rt_closest_points(h._h, pp, None, 64, po) == _lib.RT_ERR_STATE
    h.write_bvh(*sd.bvh)
    assert L.rt_closest_points(h._h, pp, None, 64, po) == _lib.RT_ERR_STATE
    assert b"no triangle tree" in L.rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        h.closest_points(pts[:4])
    assert e.value.code == _lib.RT_ERR_STATE and "closest_points" in str(e.value)
    h.set_params(tri_bvh=1)  # the host SAH tree is built by the query itself
    same(records(h, pts), hrt.closest_points_host(sd.bvh[2], pts))
    # rt_set_bvh leaves the device-geometry state
    want = records(r, pts)
    same(want, free)
    r.write_bvh(*sd.bvh)
    with pytest.raises(hrt.RtError) as e:
        r.closest_points(pts[:4])
    assert e.value.code == _lib.RT_ERR_STATE
    r.set_params(tri_bvh=1)
    same(records(r, pts), hrt.closest_points_host(sd.bvh[2], pts))
    r.set_params(tri_bvh=0)
    # a failed build keeps the geometry that answers
    r.set_triangles_device(on_device(r, tris), ONE_MATERIAL, builder=PLOC)
    bad = R.deform(tris, "scatter")
    bad["material"][len(bad) // 2] = 1
    with pytest.raises(hrt.RtError):
        r.set_triangles_device(on_device(r, bad), ONE_MATERIAL, builder=PLOC)
    same(records(r, pts, caps), capped)
    r.release_scratch()
    same(records(r, pts), free)


def test_draw_state_is_untouched():
    sd = CR.suzane_scene(48, 32)
    sd.bounces = 3
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    tris = sd.bvh[2]
    pts = K.query_points(tris, 512, 31)
    r.draw_frames(2, 1000, 10)
    img, fc, st, raw = r.read_image(), r.frame_count, r.stats(), r.raw_counters()
    same(records(r, pts), hrt.closest_points_host(tris, pts))
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st) and r.raw_counters() == raw
    r.reset_frame_count()
    r.draw_frames(2, 1000, 10)
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and img.any()
    assert r.stats().queries == st.queries
