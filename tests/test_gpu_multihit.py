"""rt_cast_rays_multi on the GPU: the device records and counts are the host mirror's (hrt.cast_rays_multi_host on the tree
read back from the renderer, and the flat definition), all 16 bytes, through every tree the renderer can hold (device LBVH
and PLOC, refitted, the host SAH tree of tri_bvh = 1), for k = 0, 1, 4, 16, with and without counts, caps of every class
and cursors; exactly n k records and n counts are written; record 0 is rt_cast_rays' hit; the counting instantiation shows
the stack overflow and the culling; statuses; and nothing of a draw's state moves. No tolerance anywhere: every
comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import _lib

import lbvh_refit_util as R
import lbvh_util as U
import multihit_util as M
import test_gpu_cast_rays as CR
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device
from test_gpu_lbvh_refit import host_sah_renderer

pytestmark = pytest.mark.gpu

N = 400
PLOC = 1
KS = (0, 1, 4, 16)
CASES = dict(U.cpu_cases(), chain=M.chain)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def tris_renderer(tris, builder=0, materials=ONE_MATERIAL):
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), materials, builder=builder)
    return r


def device(r, o, d, k, tmax=None, after=None, counts=False):
    """(records (n, k), counts or None) of one device call, on the host."""
    rec, cnt = r.cast_rays_multi_records(o, d, k, tmax, after, counts)
    rec = rec.cpu().numpy().reshape(len(o), k, 4).view(hrt.MULTI_HIT_DTYPE).reshape(len(o), k)
    return rec, (cnt.cpu().numpy().view(np.uint32) if cnt is not None else None)


def check_against_mirror(r, tris, o, d, what, ks=KS):
    """Every k, with and without counts, free, with a cap array of every class, with cursors and with both: the device
    returns the bytes of the walk on its own tree, which are the flat definition's."""
    tree = r.tri_tree()
    flat, fc = M.records(tris, tree, o, d, 16, counts=True, flat=True)
    caps = M.cap_mix(flat["t"][:, 0], 3)
    cursor = np.ascontiguousarray(flat[:, 1])
    for kw in (dict(), dict(tmax=caps), dict(after=cursor), dict(tmax=caps, after=cursor)):
        want, wc = (flat, fc) if not kw else M.records(tris, tree, o, d, 16, counts=True, flat=True, **kw)
        for k in ks:
            walk, walk_c = M.records(tris, tree, o, d, k, counts=True, **kw)
            M.same_records(walk, np.ascontiguousarray(want[:, :k]), f"{what}: host walk, k = {k} {sorted(kw)}")
            got, gc = device(r, o, d, k, counts=True, **kw)
            M.same_records(got, walk, f"{what}: k = {k} {sorted(kw)} with counts")
            assert (gc == wc).all() and (walk_c == wc).all(), (what, k, sorted(kw))
            if k:
                got, _ = device(r, o, d, k, **kw)
                M.same_records(got, walk, f"{what}: k = {k} {sorted(kw)}")
    return flat, fc


# ------------------------------------------------------------------------------------------------ equality with the mirror
@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("name", list(CASES))
def test_device_records_are_the_mirrors(name, builder):
    tris = CASES[name]()
    o, d = M.chain_rays() if name == "chain" else M.mesh_rays(tris, N, 100 + len(tris))
    r = tris_renderer(tris, builder)
    flat, fc = check_against_mirror(r, tris, o, d, f"{name} builder {builder}")
    if name in ("suzanne", "random1025", "planar", "chain"):
        assert fc.max() >= 2 and (flat["prim"][:, 0] >= 0).sum() > len(o) // 4
    res = r.cast_rays_multi(o[:64], d[:64], 4, tmax=1e30, counts=True)  # the dict, and a float for every ray
    want, wc = M.records(tris, r.tri_tree(), o[:64], d[:64], 4, tmax=1e30, counts=True)
    for f in ("t", "prim", "u", "v"):
        assert res[f].cpu().numpy().tobytes() == np.ascontiguousarray(want[f]).tobytes(), f
    assert (res["count"].cpu().numpy() == wc).all()


@pytest.mark.parametrize("scene", ["cube", "suzane", "mixed"])
def test_host_sah_tree_answers_the_same(scene):
    sd = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}[scene](32, 24)
    tris = sd.bvh[2]
    r = host_sah_renderer(sd)
    assert int(r.tri_tree_info()[0]) == 0xFFFFFFFF
    o, d = M.mesh_rays(tris, N, 5)
    if scene == "mixed":  # rays at the spheres too: only triangles answer
        c = sd.spheres["center"].astype(np.float32)
        o = np.ascontiguousarray(np.concatenate([o, np.zeros_like(c) + np.float32([0.0, 1.0, 6.0])]))
        d = np.ascontiguousarray(np.concatenate([d, c - np.float32([0.0, 1.0, 6.0])]))
        assert sd.mode == hrt.RT_MODE_MIXED and len(sd.spheres) > 4
    flat, fc = check_against_mirror(r, tris, o, d, scene)
    assert flat["prim"].max() < len(tris) and fc.max() >= 2
    assert M.check_containment(tris, r.tri_tree()) == int(U.tri_f64(tris)[1].sum())  # the third tree maker


@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("kind", ["translate", "jitter"])
def test_refitted_tree_answers_for_the_moved_mesh(kind, builder):
    a = U.mesh_triangles("suzanne.obj")
    b = R.deform(a, kind)
    r = tris_renderer(a, builder)
    r.refit_triangles_device(on_device(r, b))
    o, d = M.mesh_rays(b, N, 21)
    check_against_mirror(r, b, o, d, f"refit {kind} builder {builder}", ks=(0, 4, 16))
    assert M.check_containment(b, r.tri_tree()) == len(b)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_counts_write_exactly_n_records(n):
    import torch

    tris = U.mesh_triangles("suzanne.obj")
    o, d = M.mesh_rays(tris, 300, 8)
    o, d = o[:n].copy(), d[:n].copy()
    r = tris_renderer(tris)
    want, wc = M.records(tris, r.tri_tree(), o, d, 3, counts=True)
    dev = r._torch_device()
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    k = 3
    hits = torch.full((n * k + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    cnt = torch.full((n + 3,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    P = C.c_void_p
    assert hrt.lib().rt_cast_rays_multi(r._h, P(to.data_ptr()), P(td.data_ptr()), None, None, n, k, P(hits.data_ptr()),
                                        P(cnt.data_ptr())) == _lib.RT_OK
    r.synchronize()
    got, gc = hits.cpu().numpy(), cnt.cpu().numpy()
    M.same_records(got[:n * k].view(hrt.MULTI_HIT_DTYPE).reshape(n, k), want, f"n = {n}")
    assert (got[n * k:] == 0x5A5A5A5A).all()
    assert (gc[:n].view(np.uint32) == wc).all() and (gc[n:] == 0x5A5A5A5A).all()


def test_record_0_is_cast_rays_hit_and_all_hits_pages():
    """On the rays where the slab clause changes nothing (tests/test_multihit_abi.py measures how many: all of them) record 0
    of k = 1 is rt_cast_rays' (t, prim); every ray is compared with the host mirror. all_hits returns the paged lists.
    The four rays of the study with a NaN or infinite component are where the two calls' contracts part (include/hrt.h):
    rt_cast_rays_multi gives them no hits, rt_cast_rays the reference's answer, a hit with t = NaN or a miss; there the
    multi-hit record is the miss record and rt_cast_rays' own answer is test_gpu_ray_queries_oracle.py's business."""
    tris, tree, o, d, unchanged, with_slab = M.suzanne_study()
    finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    assert (~finite).sum() == 4 and unchanged[~finite].all()
    for builder in (0, PLOC):
        r = tris_renderer(tris, builder)
        got, _ = device(r, o, d, 1)
        M.same_records(got, M.records(tris, r.tri_tree(), o, d, 1), f"builder {builder}")
        M.same_records(got, M.records(tris, tree, o, d, 1, flat=True), f"builder {builder}, flat")
        hit = r.cast_rays(o, d)
        t, prim = hit["t"].cpu().numpy(), hit["prim"].cpu().numpy()
        assert unchanged.sum() > 0.99 * len(o)
        same = unchanged & finite
        assert (prim[same] == got["prim"][same, 0]).all()
        assert t[same].tobytes() == np.ascontiguousarray(got["t"][same, 0]).tobytes()
        assert (got["prim"][~finite, 0] == -1).all() and (got["t"][~finite, 0] == np.float32(hrt.RT_T_MISS)).all()
        assert ((prim[~finite] >= 0) | (t[~finite] == np.float32(hrt.RT_T_MISS))).all()
    offsets, t, prim, u, v = (x.cpu().numpy() for x in r.all_hits(o, d))
    assert offsets[0] == 0 and (np.diff(offsets) == [len(w) for w in with_slab]).all()
    want = np.concatenate(with_slab)
    got = np.stack([t.view(np.uint32), prim.view(np.uint32), u.view(np.uint32), v.view(np.uint32)], axis=1)
    assert got.tobytes() == want.tobytes()
    assert np.diff(offsets).max() <= 16  # (Suzanne: one page; the chain below needs several)
    ch = M.chain()
    rc = tris_renderer(ch, PLOC)
    co, cd = M.chain_rays()
    offsets, t, prim, u, v = (x.cpu().numpy() for x in rc.all_hits(co, cd, tmax=25.0))
    pages = M.ragged(M.paged(lambda after: M.records(ch, rc.tri_tree(), co, cd, 5, tmax=25.0, after=after), len(co), 5))
    assert (np.diff(offsets) == [len(w) for w in pages]).all() and np.diff(offsets).max() > 32
    got = np.stack([t.view(np.uint32), prim.view(np.uint32), u.view(np.uint32), v.view(np.uint32)], axis=1)
    assert got.tobytes() == np.concatenate(pages).tobytes()


# ------------------------------------------------------------------------------------------------ counters
def counted(r, o, d, k, counts=False, **kw):
    r.set_multihit_count(True)
    rec, cnt = device(r, o, d, k, counts=counts, **kw)
    c = [int(x) for x in r.multihit_counts()]
    r.set_multihit_count(False)
    return rec, cnt, c


def test_counters_show_the_overflow_and_the_culling():
    ch = M.chain()
    r = tris_renderer(ch, PLOC)
    assert int(r.tri_tree_info()[4]) > 24
    assert r.multihit_counts().tolist() == [0, 0, 0, 0]
    o, d = M.chain_rays()
    rec, cnt, c = counted(r, o, d, 16, counts=True)
    print(f"chain: {c[3]} of {c[0]} queries overflowed the stack")
    want, wc = M.records(ch, r.tri_tree(), o, d, 16, counts=True, flat=True)
    M.same_records(rec, want, "chain, counted")
    assert (cnt == wc).all() and c[0] == len(o) and c[3] > 0  # and the counts did not double
    tris = U.mesh_triangles("suzanne.obj")
    o, d = M.camera_rays(hrt.SceneTris.suzane_camera(), 64, 36)
    for builder in (0, PLOC):
        r = tris_renderer(tris, builder)
        rec1, _, culled = counted(r, o, d, 1)
        rec1c, _, everything = counted(r, o, d, 1, counts=True)
        M.same_records(rec1, rec1c, f"builder {builder}")
        print(f"suzanne builder {builder}: {culled[1] / culled[0]:.1f} triangle tests and {culled[2] / culled[0]:.1f} box tests "
              f"per ray with culling, {everything[1] / everything[0]:.1f} and {everything[2] / everything[0]:.1f} without")
        assert culled[0] == everything[0] == len(o) and culled[3] == everything[3] == 0
        assert culled[1] < everything[1] and culled[2] < everything[2]
        assert everything[1] / everything[0] < len(tris) / 4  # (an always-flat kernel has m: this is no performance claim)
        got, _ = device(r, o, d, 1)
        M.same_records(got, rec1, "counting off again")


# ------------------------------------------------------------------------------------------------ statuses and state
def test_statuses():
    import torch

    L = hrt.lib()
    P = C.c_void_p
    tris = U.mesh_triangles("suzanne.obj")
    o, d = M.mesh_rays(tris, 64, 2)
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    dev = sph._torch_device()
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hits = torch.zeros((64 * 16 + 1, 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros((65,), dtype=torch.int32, device=dev)
    po, pd, ph, pc = P(to.data_ptr()), P(td.data_ptr()), P(hits.data_ptr()), P(cnt.data_ptr())
    torch.cuda.synchronize(dev)
    assert L.rt_cast_rays_multi(sph._h, po, pd, None, None, 64, 4, ph, pc) == _lib.RT_ERR_ARG
    assert b"sphere program" in L.rt_last_error()
    r = tris_renderer(tris)
    assert L.rt_cast_rays_multi(r._h, po, pd, None, None, 0, 4, ph, pc) == _lib.RT_OK  # n = 0, and null buffers with it
    assert L.rt_cast_rays_multi(r._h, None, None, None, None, 0, 4, None, None) == _lib.RT_OK
    assert L.rt_cast_rays_multi(r._h, po, pd, None, None, 0, 17, ph, pc) == _lib.RT_ERR_ARG
    off = lambda p, b: P(p.value + b)
    for args in ((po, pd, None, None, 64, 17, ph, pc),               # k past RT_MULTI_HIT_MAX_K
                 (po, pd, None, None, 64, 0, ph, None),              # k = 0 without counts
                 (po, pd, None, None, 64, 4, None, pc),              # k > 0 without hits
                 (None, pd, None, None, 64, 4, ph, pc), (po, None, None, None, 64, 4, ph, pc),  # null rays
                 (off(po, 2), pd, None, None, 32, 4, ph, pc), (po, off(pd, 1), None, None, 32, 4, ph, pc),
                 (po, pd, off(po, 3), None, 32, 4, ph, pc),          # misaligned tmax
                 (po, pd, None, off(ph, 2), 32, 4, ph, pc),          # misaligned cursors
                 (po, pd, None, None, 32, 4, off(ph, 8), pc),        # hits not 16-byte aligned
                 (po, pd, None, None, 32, 4, ph, off(pc, 2))):       # misaligned counts
        assert L.rt_cast_rays_multi(r._h, *args) == _lib.RT_ERR_ARG, args
        assert b"rt_cast_rays_multi" in L.rt_last_error()
    r.synchronize()
    assert not hits.cpu().numpy().any() and not cnt.cpu().numpy().any()  # nothing was written by a refused call
    assert L.rt_cast_rays_multi(r._h, po, pd, None, off(ph, 4), 32, 4, ph, pc) == _lib.RT_OK  # cursors: 4-byte aligned
    with pytest.raises(ValueError):
        r.cast_rays_multi(o[:4], d[:4], 17)
    with pytest.raises(ValueError):
        r.cast_rays_multi(o[:4], d[:4], 0)
    with pytest.raises(ValueError):
        r.cast_rays_multi(o[:4], d[:4], 2, tmax=np.zeros(5, dtype=np.float32))
    # no tree: tri_bvh = 0 and no device geometry
    sd = CR.suzane_scene(16, 16)
    h = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    assert L.rt_cast_rays_multi(h._h, po, pd, None, None, 64, 4, ph, pc) == _lib.RT_ERR_STATE
    h.write_bvh(*sd.bvh)
    assert L.rt_cast_rays_multi(h._h, po, pd, None, None, 64, 4, ph, pc) == _lib.RT_ERR_STATE
    assert b"no triangle tree" in L.rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        h.cast_rays_multi(o[:4], d[:4], 2)
    assert e.value.code == _lib.RT_ERR_STATE and "cast_rays_multi" in str(e.value)
    h.set_params(tri_bvh=1)  # the host SAH tree is built by the query itself
    got, gc = device(h, o, d, 4, counts=True)
    want, wc = M.records(sd.bvh[2], h.tri_tree(), o, d, 4, counts=True, flat=True)
    M.same_records(got, want, "host SAH tree built by the query")
    assert (gc == wc).all()


def test_draw_state_is_untouched():
    sd = CR.suzane_scene(48, 32)
    sd.bounces = 3
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    tris = sd.bvh[2]
    o, d = M.mesh_rays(tris, 256, 31)
    r.draw_frames(2, 1000, 10)
    img, fc, st, raw = r.read_image(), r.frame_count, r.stats(), r.raw_counters()
    got, gc = device(r, o, d, 4, counts=True)
    want, wc = M.records(tris, r.tri_tree(), o, d, 4, counts=True, flat=True)
    M.same_records(got, want, "after a draw")
    assert (gc == wc).all()
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st) and r.raw_counters() == raw
    r.reset_frame_count()
    r.draw_frames(2, 1000, 10)
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and img.any()
    assert r.stats().queries == st.queries
