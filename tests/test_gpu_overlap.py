"""rt_overlap_volumes on the GPU: the device records and counts are the host mirror's (hrt.overlap_volumes_host on the tree
read back from the renderer, and the flat definition), all 16 bytes, for both kinds of volume, through every tree the
renderer can hold (device LBVH and PLOC, refitted, the host SAH tree of tri_bvh = 1), for k = 0, 1, 4, 16, with and
without counts, with cursors; exactly n k records and n counts are written; the ball kind's first record is
rt_closest_points'; the counting instantiation shows the stack overflow and the culling; statuses; and nothing of a
draw's state moves. No tolerance anywhere: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import hrt
from hrt import _lib

import closest_util as K
import lbvh_refit_util as R
import lbvh_util as U
import multihit_util as M
import overlap_util as V
import test_gpu_cast_rays as CR
from test_gpu_lbvh import ONE_MATERIAL, device_renderer, on_device
from test_gpu_lbvh_refit import host_sah_renderer

pytestmark = pytest.mark.gpu

N = 400
PLOC = 1
KS = (0, 1, 4, 16)
BOX, BALL = V.BOX, V.BALL
CASES = dict(U.cpu_cases(), chain=M.chain)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def tris_renderer(tris, builder=0, materials=ONE_MATERIAL):
    r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    r.set_triangles_device(on_device(r, tris), materials, builder=builder)
    return r


def device(r, kind, vol, k, after=None, counts=False):
    """(records (n, k), counts or None) of one device call, on the host."""
    rec, cnt = r.overlap_records(kind, vol, k, after, counts)
    rec = rec.cpu().numpy().reshape(len(vol), k, 4).view(hrt.OVERLAP_HIT_DTYPE).reshape(len(vol), k)
    return rec, (cnt.cpu().numpy().view(np.uint32) if cnt is not None else None)


def check_against_mirror(r, tris, kind, vol, what, ks=KS):
    """Every k, with and without counts, free and with cursors (the ball kind also with a radius column of every class of
    cap): the device returns the bytes of the walk on its own tree, which are the flat definition's."""
    tree = r.tri_tree()
    flat, fc = V.records(tris, tree, kind, vol, 16, counts=True, flat=True)
    cursor = np.ascontiguousarray(flat[:, 1])
    variants = [(vol, dict()), (vol, dict(after=cursor))]
    if kind == BALL:
        capped = vol.copy()
        capped[:, 3] = K.cap_mix(flat["d2"][:, 0], 3)
        variants += [(capped, dict()), (capped, dict(after=cursor))]
    for q, kw in variants:
        want, wc = V.records(tris, tree, kind, q, 16, counts=True, flat=True, **kw)
        for k in ks:
            walk, walk_c = V.records(tris, tree, kind, q, k, counts=True, **kw)
            V.same_records(walk, np.ascontiguousarray(want[:, :k]), f"{what}: host walk, k = {k} {sorted(kw)}")
            got, gc = device(r, kind, q, k, counts=True, **kw)
            V.same_records(got, walk, f"{what}: k = {k} {sorted(kw)} with counts")
            assert (gc == wc).all() and (walk_c == wc).all(), (what, k, sorted(kw))
            if k:
                got, _ = device(r, kind, q, k, **kw)
                V.same_records(got, walk, f"{what}: k = {k} {sorted(kw)}")
    return flat, fc


# ------------------------------------------------------------------------------------------------ equality with the mirror
@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("name", list(CASES))
def test_device_records_are_the_mirrors(name, builder, kind):
    tris = CASES[name]()
    vol = V.volumes_for(kind, tris, N, 100 + len(tris))
    r = tris_renderer(tris, builder)
    flat, fc = check_against_mirror(r, tris, kind, vol, f"{name} builder {builder} kind {kind}")
    if name in ("suzanne", "random1025", "planar"):
        assert fc.max() >= 16 and (flat["prim"][:, 0] >= 0).sum() > len(vol) // 4
    if kind == BOX:  # the dicts
        res = r.overlap_boxes(vol[:64, :3], vol[:64, 3:], 4, counts=True)
        want, wc = V.records(tris, r.tri_tree(), BOX, vol[:64], 4, counts=True)
    else:
        res = r.nearest_triangles(vol[:64, :3], 4, max_dist2=2.5, counts=True)
        q = vol[:64].copy()
        q[:, 3] = 2.5
        want, wc = V.records(tris, r.tri_tree(), BALL, q, 4, counts=True)
    for f in ("d2", "prim", "v", "w"):
        assert res[f].cpu().numpy().tobytes() == np.ascontiguousarray(want[f]).tobytes(), f
    assert (res["count"].cpu().numpy() == wc).all()


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("scene", ["cube", "suzane", "mixed"])
def test_host_sah_tree_answers_the_same(scene, kind):
    sd = {"cube": CR.cube_scene, "suzane": CR.suzane_scene, "mixed": lambda w, h: CR.mixed_scene(w, h, 12)}[scene](32, 24)
    tris = sd.bvh[2]
    r = host_sah_renderer(sd)
    assert int(r.tri_tree_info()[0]) == 0xFFFFFFFF
    vol = V.volumes_for(kind, tris, N, 5)
    if scene == "mixed":  # volumes at the spheres too: only triangles answer
        c = sd.spheres["center"][:, :3].astype(np.float32)
        rad = np.float32(0.5)
        extra = (np.concatenate([c - rad, c + rad], axis=1) if kind == BOX
                 else np.concatenate([c, np.full((len(c), 1), 0.25, dtype=np.float32)], axis=1))
        vol = np.ascontiguousarray(np.concatenate([vol, extra.astype(np.float32)]))
        assert sd.mode == hrt.RT_MODE_MIXED and len(sd.spheres) > 4
    flat, fc = check_against_mirror(r, tris, kind, vol, f"{scene} kind {kind}")
    assert flat["prim"].max() < len(tris) and fc.max() >= 2
    assert M.check_containment(tris, r.tri_tree()) == int(U.tri_f64(tris)[1].sum())  # the third tree maker


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("builder", [0, PLOC])
@pytest.mark.parametrize("move", ["translate", "jitter"])
def test_refitted_tree_answers_for_the_moved_mesh(move, builder, kind):
    a = U.mesh_triangles("suzanne.obj")
    b = R.deform(a, move)
    r = tris_renderer(a, builder)
    r.refit_triangles_device(on_device(r, b))
    vol = V.volumes_for(kind, b, N, 21)
    check_against_mirror(r, b, kind, vol, f"refit {move} builder {builder} kind {kind}")
    assert M.check_containment(b, r.tri_tree()) == len(b)


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_counts_write_exactly_n_records(n, kind):
    import torch

    tris = U.mesh_triangles("suzanne.obj")
    vol = np.ascontiguousarray(V.volumes_for(kind, tris, 300, 8)[:n])
    r = tris_renderer(tris)
    k = 3
    want, wc = V.records(tris, r.tri_tree(), kind, vol, k, counts=True)
    dev = r._torch_device()
    tv = torch.from_numpy(vol).to(dev)
    hits = torch.full((n * k + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    cnt = torch.full((n + 3,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    P = C.c_void_p
    assert hrt.lib().rt_overlap_volumes(r._h, kind, P(tv.data_ptr()), None, n, k, P(hits.data_ptr()),
                                        P(cnt.data_ptr())) == _lib.RT_OK
    r.synchronize()
    got, gc = hits.cpu().numpy(), cnt.cpu().numpy()
    V.same_records(got[:n * k].view(hrt.OVERLAP_HIT_DTYPE).reshape(n, k), want, f"n = {n}")
    assert (got[n * k:] == 0x5A5A5A5A).all()
    assert (gc[:n].view(np.uint32) == wc).all() and (gc[n:] == 0x5A5A5A5A).all()


def test_ball_record_0_is_closest_points_and_all_overlaps_pages():
    tris = U.mesh_triangles("suzanne.obj")
    pts = K.query_points(tris, N, 4)
    caps = K.cap_mix(hrt.closest_points_host(tris, pts)["d2"], 9)
    for builder in (0, PLOC):
        r = tris_renderer(tris, builder)
        for cap in (None, caps):
            near = r.closest_records(pts, cap).cpu().numpy().view(hrt.CLOSEST_DTYPE).reshape(-1)
            got, _ = device(r, BALL, V.balls_for(tris, N, 4, cap), 1)
            for f in ("d2", "prim", "v", "w"):
                assert got[f][:, 0].tobytes() == np.ascontiguousarray(near[f]).tobytes(), (f, builder)
    # the ragged lists are the paged host lists
    for kind, vol in ((BOX, V.boxes_for(tris, 60, 13)), (BALL, V.balls_for(tris, 60, 13, np.full(60, 0.05, dtype=np.float32)))):
        offsets, d2, prim, v, w = (x.cpu().numpy() for x in r.all_overlaps(kind, vol))
        pages = V.ragged(V.paged(lambda after: V.records(tris, r.tri_tree(), kind, vol, 5, after=after), len(vol), 5))
        assert (np.diff(offsets) == [len(p) for p in pages]).all() and np.diff(offsets).max() > 32
        got = np.stack([d2.view(np.uint32), prim.view(np.uint32), v.view(np.uint32), w.view(np.uint32)], axis=1)
        assert got.tobytes() == np.concatenate(pages).tobytes()


# ------------------------------------------------------------------------------------------------ counters
def counted(r, kind, vol, k, counts=False, **kw):
    r.set_overlap_count(True)
    rec, cnt = device(r, kind, vol, k, counts=counts, **kw)
    c = [int(x) for x in r.overlap_counts()]
    r.set_overlap_count(False)
    return rec, cnt, c


def test_counters_show_the_overflow_and_the_culling():
    ch = M.chain()
    r = tris_renderer(ch, PLOC)
    assert int(r.tri_tree_info()[4]) > 24
    assert r.overlap_counts().tolist() == [0, 0, 0, 0]
    for kind in V.KINDS:
        vol = V.volumes_for(kind, ch, N, 7)
        rec, cnt, c = counted(r, kind, vol, 16, counts=True)
        print(f"chain kind {kind}: {c[3]} of {c[0]} queries overflowed the stack")
        want, wc = V.records(ch, r.tri_tree(), kind, vol, 16, counts=True, flat=True)
        V.same_records(rec, want, f"chain, counted, kind {kind}")
        assert (cnt == wc).all() and c[0] == len(vol) and c[3] > 0  # and the counts did not double
    tris = U.mesh_triangles("suzanne.obj")
    m = len(tris)
    for builder in (0, PLOC):
        r = tris_renderer(tris, builder)
        # small boxes: 0.5 % to 2 % of the extent
        big = V.boxes_for(tris, N, 3, bad=False)
        c0, h0 = 0.5 * (big[:, :3] + big[:, 3:]), 0.5 * (big[:, 3:] - big[:, :3])
        small = np.ascontiguousarray(np.concatenate([c0 - 0.04 * h0, c0 + 0.04 * h0], axis=1).astype(np.float32))
        rec, cnt, c = counted(r, BOX, small, 4, counts=True)
        V.same_records(rec, device(r, BOX, small, 4)[0], f"builder {builder}: counted and product, boxes")
        print(f"suzanne builder {builder}, small boxes: {c[1] / c[0]:.1f} triangle tests and {c[2] / c[0]:.1f} box tests per query")
        assert c[0] == N and c[3] == 0 and c[1] / c[0] < m / 8
        balls = np.ascontiguousarray(V.balls_for(tris, N, 4)[:290])  # (on and near the mesh and around it: not the far ones)
        rec1, _, culled = counted(r, BALL, balls, 1)
        rec1c, _, everything = counted(r, BALL, balls, 1, counts=True)
        V.same_records(rec1, rec1c, f"builder {builder}: with and without counts")
        print(f"suzanne builder {builder}, balls k = 1: {culled[1] / culled[0]:.1f} triangle tests per query culling by the list, "
              f"{everything[1] / everything[0]:.1f} counting all")
        assert culled[0] == everything[0] == len(balls) and culled[3] == 0
        assert culled[1] < everything[1] and culled[1] / culled[0] < m / 4
        V.same_records(device(r, BALL, balls, 1)[0], rec1, "counting off again")


# ------------------------------------------------------------------------------------------------ statuses and state
def test_statuses():
    import torch

    L = hrt.lib()
    P = C.c_void_p
    tris = U.mesh_triangles("suzanne.obj")
    vol = V.boxes_for(tris, 64, 2)
    sph = hrt.Renderer(16, 16, hrt.RT_MODE_SPHERE)
    dev = sph._torch_device()
    tv = torch.from_numpy(vol).to(dev)
    hits = torch.zeros((64 * 16 + 1, 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros((65,), dtype=torch.int32, device=dev)
    pv, ph, pc = P(tv.data_ptr()), P(hits.data_ptr()), P(cnt.data_ptr())
    torch.cuda.synchronize(dev)
    call = L.rt_overlap_volumes
    for kind in V.KINDS:
        assert call(sph._h, kind, pv, None, 64, 4, ph, pc) == _lib.RT_ERR_ARG
        assert b"sphere program" in L.rt_last_error()
    r = tris_renderer(tris)
    assert call(r._h, BOX, pv, None, 0, 4, ph, pc) == _lib.RT_OK  # n = 0, and null buffers with it
    assert call(r._h, BALL, None, None, 0, 4, None, None) == _lib.RT_OK
    assert call(sph._h, BOX, None, None, 0, 4, None, None) == _lib.RT_OK  # whatever the program
    assert call(r._h, BOX, pv, None, 0, 17, ph, pc) == _lib.RT_ERR_ARG
    assert call(r._h, 0, pv, None, 0, 4, ph, pc) == _lib.RT_ERR_ARG
    off = lambda p, b: P(p.value + b)
    for args in ((BOX, pv, None, 64, 17, ph, pc),                # k past RT_OVERLAP_MAX_K
                 (0, pv, None, 64, 4, ph, pc), (3, pv, None, 64, 4, ph, pc),  # unknown kinds
                 (BOX, pv, None, 64, 0, ph, None),               # k = 0 without counts
                 (BALL, pv, None, 64, 4, None, pc),              # k > 0 without hits
                 (BOX, None, None, 64, 4, ph, pc),               # null volumes
                 (BOX, off(pv, 2), None, 32, 4, ph, pc),         # misaligned volumes
                 (BALL, pv, off(ph, 2), 32, 4, ph, pc),          # misaligned cursors
                 (BOX, pv, None, 32, 4, off(ph, 8), pc),         # hits not 16-byte aligned
                 (BOX, pv, None, 32, 4, ph, off(pc, 2))):        # misaligned counts
        assert call(r._h, *args) == _lib.RT_ERR_ARG, args
        assert b"rt_overlap_volumes" in L.rt_last_error()
    r.synchronize()
    assert not hits.cpu().numpy().any() and not cnt.cpu().numpy().any()  # nothing was written by a refused call
    assert call(r._h, BOX, pv, off(ph, 4), 32, 4, ph, pc) == _lib.RT_OK  # cursors: 4-byte aligned
    assert call(r._h, BALL, off(pv, 4), None, 32, 4, ph, pc) == _lib.RT_OK  # volumes: 4-byte aligned
    r.synchronize()
    with pytest.raises(ValueError):
        r.overlap_records(BOX, vol[:4], 17)
    with pytest.raises(ValueError):
        r.overlap_records(BOX, vol[:4], 0)
    with pytest.raises(ValueError):
        r.overlap_records(BALL, vol[:4], 2)  # six floats per query for a ball
    with pytest.raises(ValueError):
        r.overlap_records(5, vol[:4], 2)
    # no tree: tri_bvh = 0 and no device geometry
    sd = CR.suzane_scene(16, 16)
    h = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
    assert call(h._h, BOX, pv, None, 64, 4, ph, pc) == _lib.RT_ERR_STATE
    h.write_bvh(*sd.bvh)
    assert call(h._h, BOX, pv, None, 64, 4, ph, pc) == _lib.RT_ERR_STATE
    assert b"no triangle tree" in L.rt_last_error()
    with pytest.raises(hrt.RtError) as e:
        h.overlap_records(BOX, vol[:4], 2)
    assert e.value.code == _lib.RT_ERR_STATE and "overlap_volumes" in str(e.value)
    h.set_params(tri_bvh=1)  # the host SAH tree is built by the query itself
    vol = V.boxes_for(sd.bvh[2], 64, 2)
    got, gc = device(h, BOX, vol, 4, counts=True)
    want, wc = V.records(sd.bvh[2], h.tri_tree(), BOX, vol, 4, counts=True, flat=True)
    V.same_records(got, want, "host SAH tree built by the query")
    assert (gc == wc).all()


def test_draw_state_is_untouched():
    sd = CR.suzane_scene(48, 32)
    sd.bounces = 3
    r = device_renderer(sd, schedule=hrt.RT_SCHEDULE_TILES)
    tris = sd.bvh[2]
    r.draw_frames(2, 1000, 10)
    img, fc, st, raw = r.read_image(), r.frame_count, r.stats(), r.raw_counters()
    for kind in V.KINDS:
        vol = V.volumes_for(kind, tris, 256, 31)
        got, gc = device(r, kind, vol, 4, counts=True)
        want, wc = V.records(tris, r.tri_tree(), kind, vol, 4, counts=True, flat=True)
        V.same_records(got, want, f"after a draw, kind {kind}")
        assert (gc == wc).all()
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and r.frame_count == fc == 2
    assert bytes(r.stats()) == bytes(st) and r.raw_counters() == raw
    r.reset_frame_count()
    r.draw_frames(2, 1000, 10)
    assert (r.read_image().view(np.uint32) == img.view(np.uint32)).all() and img.any()
    assert r.stats().queries == st.queries
