"""The draw kernels at degenerate image shapes against the oracle (small_shapes_util.py; the CPU side is
test_small_shapes_oracle.py).

Images narrower or lower than one 8x8 tile, with fewer pixels than a wave, with fewer tiles than the sample queue has
per-XCD job counters, and one pixel wide or high. renderer.cpp's launch_frames branches on the tile count in many places
(auto stealing, halved jobs, the tail split's tail_from = njobs - min(njobs, 64 CUs): every job dealt in parts, per-XCD
queues dead on the first take, the fold ring's slots by ntiles x nchunks, fold_prev_tiles in 1 of 64 waves, a tile order
with a head cap of ntiles / 2 = 0), and all of them end at or near their limits at 1 to 4 tiles.

Every case asserts the kernel it ran (rt_stats.kernel), the oracle's image and its query count. On the REGULAR shapes the
oracle's image is finite and the comparison is of uint32 views. On the four ONE_WIDE shapes every primary ray is NaN
(0 / 0 in make_ray); there the NaN masks must be equal, the mask is "everything", and queries = W H frames: a NaN ray
takes one query through k_render, k_trace, k_trace_split (walked, stolen, resolved at block time or not) and
k_trace_split_tris, and every such draw finishes. Case ids start with "regular" or "onewide".
"""
import numpy as np
import pytest

import hrt
import scenes
import small_shapes_util as U

pytestmark = pytest.mark.gpu

WALK = 0xFFFFFFFF
SPLIT = dict(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4)
QUEUES = dict(SPLIT, steal=1, fold=hrt.RT_FOLD_BUFFER)  # per-XCD queues, the tail split, tile lists
# path -> (rt_params, the kernel's name or its prefix, rt_stats.fold_ring)
PATHS = {
    "1_k_render": (dict(schedule=hrt.RT_SCHEDULE_TILES), "k_render<", 0),
    "2_k_trace": (dict(schedule=hrt.RT_SCHEDULE_QUEUE, variant=1), "k_trace<", 0),
    "3_steal": (dict(SPLIT, count_tests=0), "k_trace_split<true, true, false, false>", 0),
    "4_queues": (dict(QUEUES, count_tests=0), "k_trace_split<true, false, false, false>", 0),
    "5_ring": (dict(SPLIT, count_tests=0, fold=hrt.RT_FOLD_RING), "k_trace_split<true, false, false, false>", 1),
    "6_count": (dict(QUEUES, count_tests=1), "k_trace_split<true, false, true, false>", 0),
}
ALL_SHAPES = U.REGULAR + U.ONE_WIDE
SOME_SHAPES = U.REGULAR + [(1, 1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _kernel_is(st, kernel, what):
    name = st.kernel.decode()
    assert (name == kernel if kernel.endswith(">") else name.startswith(kernel)), (what, name, kernel)


def _check(r, program, shape, frames, kernel, what, fold_ring=None, counts=False):
    """The renderer's image, queries (and test counts) and kernel against the oracle of (program, shape, frames)."""
    w, h = shape
    ref, q, nodes, tris = U.oracle(program, w, h, frames)
    img, st = r.read_image(), r.stats()
    print(f"{what}: kernel {st.kernel.decode()} launches {st.launches} trace {st.trace_launches} fold_ring {st.fold_ring} "
          f"ordered {st.ordered_launches} queries {st.queries} (oracle {q}) nan {int(np.isnan(img).sum())}")
    _kernel_is(st, kernel, what)
    if fold_ring is not None:
        assert st.fold_ring == fold_ring, (what, st.fold_ring)
    U.assert_image(img, ref, shape, what)
    assert st.queries == q, (what, st.queries, q)
    assert st.samples == w * h * frames, (what, st.samples)
    if tuple(shape) in U.ONE_WIDE:
        assert q == w * h * frames, (what, q)
    if counts:
        assert (st.node_tests, st.tri_tests) == (nodes, tris), (what, st.node_tests, st.tri_tests, nodes, tris)
    return st


def _draw(program, shape, frames, params, kernel, what, **kw):
    sd = U.scene(program, *shape, frames)
    r = scenes.make_renderer(sd)
    r.set_params(**params)
    r.draw_frames(frames, 1000, 10)
    return r, _check(r, program, shape, frames, kernel, what, **kw)


def _lists_resolved(r, shape, frames, what):
    """Path 4 draws with the tile lists: every frame block of a listed tile was resolved when it was made, and a one-wide
    view is refused (every tile walks)."""
    lists = r.tile_lists()
    assert lists.shape[0] == ((shape[0] + 7) // 8) * ((shape[1] + 7) // 8), (what, lists.shape)
    if tuple(shape) in U.ONE_WIDE:
        assert (lists[:, 0] == WALK).all(), (what, lists[:, 0])
    assert r.tile_lists_resolved() == int((lists[:, 0] != WALK).sum()) * frames, (what, r.tile_lists_resolved(), lists[:, 0])


def _cases(paths, shapes):
    return [pytest.param(p, s, f, id=f"{U.shape_id(s)}-{p}-{f}f") for s in shapes for p in paths for f in U.FRAMES]


# ---- paths 1 to 6: the sphere program
@pytest.mark.parametrize("path, shape, frames",
                         _cases(["1_k_render", "3_steal", "4_queues"], ALL_SHAPES) +
                         _cases(["2_k_trace", "5_ring", "6_count"], SOME_SHAPES))
def test_sphere_program(path, shape, frames):
    params, kernel, fold_ring = PATHS[path]
    what = f"{path} {shape[0]}x{shape[1]} x{frames}"
    r, st = _draw("sphere", shape, frames, params, kernel, what, fold_ring=fold_ring)
    if path == "4_queues":
        _lists_resolved(r, shape, frames, what)


@pytest.mark.parametrize("tail_split", [2, 3])
@pytest.mark.parametrize("job_frames", [4, 8])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=U.shape_id)
def test_queues_job_sizes_and_tail_parts(shape, job_frames, tail_split):
    """Path 4 at 40 frames in jobs of 4 and 8 frames, their tails dealt in quarters and eighths (eighths of a 4-frame job
    do not exist: that launch deals whole jobs)."""
    params, kernel, fold_ring = PATHS["4_queues"]
    what = f"4_queues {shape[0]}x{shape[1]} job_frames {job_frames} tail_split {tail_split}"
    r, st = _draw("sphere", shape, 40, dict(params, job_frames=job_frames, tail_split=tail_split), kernel, what,
                  fold_ring=fold_ring)
    _lists_resolved(r, shape, 40, what)


# ---- path 7: the mixed and triangle programs
@pytest.mark.parametrize("program, shape, frames",
                         [pytest.param(p, s, f, id=f"{U.shape_id(s)}-{p}-{f}f")
                          for s in SOME_SHAPES for p in ("mixed", "tris") for f in U.FRAMES])
def test_mixed_and_triangle_programs(program, shape, frames):
    for schedule, kernel in ((hrt.RT_SCHEDULE_TILES, "k_render<"), (hrt.RT_SCHEDULE_QUEUE, "k_trace_split_tris<")):
        _draw(program, shape, frames, dict(schedule=schedule, variant=1), kernel,
              f"{program} {shape[0]}x{shape[1]} x{frames} schedule {schedule}", counts=True)


# ---- path 8: several launches over few tiles
@pytest.mark.parametrize("fold", [hrt.RT_FOLD_NEXT, hrt.RT_FOLD_BUFFER], ids=["fold_next", "fold_buffer"])
@pytest.mark.parametrize("shape, frames", [((2, 2), 2800), ((9, 9), 700)], ids=["regular-2x2-2800f", "regular-9x9-700f"])
def test_several_launches_over_few_tiles(shape, frames, fold):
    """One frame of one tile is 768 B of colours, so a 1 MiB buffer holds 1365 frames of 2x2 (one tile) and 341 frames of
    9x9 (four): three balanced launches each, the second and third folding the one before in 1 of 64 waves of a launch
    that has only a few."""
    params, kernel, _ = PATHS["4_queues"]
    what = f"{shape[0]}x{shape[1]} x{frames} fold {fold}"
    r, st = _draw("sphere", shape, frames, dict(params, fold=fold, queue_budget_mb=1), kernel, what,
                  fold_ring=2 if fold == hrt.RT_FOLD_NEXT else 0)
    assert st.trace_launches == 3 and st.launch_frames * 3 >= frames > st.launch_frames * 2, (what, st.trace_launches,
                                                                                              st.launch_frames)
    assert st.launches == (st.trace_launches + 1 if fold == hrt.RT_FOLD_NEXT else 2 * st.trace_launches), (what, st.launches)


# ---- path 9: the wavefront route
@pytest.mark.parametrize("shape", [(2, 2), (7, 5), (9, 9)], ids=U.shape_id)
def test_wavefront_route_equals_the_drawn_frame(shape):
    """rt_primary_rays and rt_primary_rng, then rt_trace_rays, as test_gpu_trace_rays.py: the one-frame image and its
    queries, the oracle's and the draw's."""
    w, h = shape
    sd = U.scene("sphere", w, h, 1)
    r = scenes.make_renderer(sd)
    o, d = r.primary_rays(1000)
    s = r.primary_rng(1000)
    assert tuple(o.shape) == tuple(d.shape) == (h, w, 3) and tuple(s.shape) == (h, w)
    rad, q = r.trace_rays(o.view(-1, 3), d.view(-1, 3), rng=s.view(-1), want_queries=True)
    rad = rad.view(h, w, 3).cpu().numpy()
    ref, rays, _, _ = U.oracle("sphere", w, h, 1)
    U.assert_bits(rad, ref, f"trace_rays {w}x{h}")
    assert int(q.sum().item()) == rays
    r.set_params(**PATHS["4_queues"][0])
    r.draw_frames(1, 1000, 10)
    st = _check(r, "sphere", shape, 1, PATHS["4_queues"][1], f"draw {w}x{h}")
    U.assert_bits(rad, r.read_image(), f"trace_rays against the draw {w}x{h}")


# ---- one renderer through a chain of resizes
CHAIN = [(1, 1), (9, 9), (2, 2), (65, 2), (16, 8), (8, 16), (64, 40)]


def test_resize_chain():
    """64x40 -> 1x1 -> 9x9 -> 2x2 -> 65x2 -> 16x8 -> 8x16 (the same two tiles in another grid) -> 64x40 with path 4's
    parameters: after every resize a 5-frame draw (it learns the tile order and builds the lists of the new view), then
    the same draw again from frame 0, which deals in the learnt order and finds the lists built."""
    params, kernel, fold_ring = PATHS["4_queues"]
    frames = 5
    r = scenes.make_renderer(U.scene("sphere", 64, 40, frames))
    r.set_params(**params)
    tiles_before = 0
    for k, shape in enumerate([(64, 40)] + CHAIN):
        if k:
            r.resize(*shape)
            assert r.frame_count == 0
        ntiles = ((shape[0] + 7) // 8) * ((shape[1] + 7) // 8)
        for again in (0, 1):
            if again:
                r.reset_frame_count()
            r.draw_frames(frames, 1000, 10)
            what = f"resize {k} to {shape[0]}x{shape[1]} draw {again}"
            st = _check(r, "sphere", shape, frames, kernel, what, fold_ring=fold_ring)
            # (a learning draw deals in the order it holds when that is a permutation of as many tiles: 16x8's at 8x16)
            assert st.ordered_launches == (1 if again or ntiles == tiles_before else 0), (what, st.ordered_launches)
            _lists_resolved(r, shape, frames, what)
            sums, order = r.tile_order()
            assert len(sums) == ntiles
            U.check_order(sums, order)
        tiles_before = ntiles


# ---- the tile order against its rule
@pytest.mark.parametrize("shape", U.ORDER_SHAPES, ids=lambda s: f"regular-{s[0]}x{s[1]}")
def test_tile_order_follows_its_rule(shape):
    """cost_order = 2: the first draw learns, the second deals in that order; both give the oracle's image. The order read
    back is the rule's (small_shapes_util.check_order) at 1, 2, 3 and 54 tiles and over two and three blocks of 1024."""
    w, h = shape
    frames = U.ORDER_FRAMES
    ntiles = ((w + 7) // 8) * ((h + 7) // 8)
    r = scenes.make_renderer(U.scene("sphere", w, h, frames))
    r.set_params(**dict(PATHS["4_queues"][0], cost_order=2, job_frames=8))
    kernel = PATHS["4_queues"][1]
    for again in (0, 1):
        if again:
            r.reset_frame_count()
        r.draw_frames(frames, 1000, 10)
        st = _check(r, "sphere", shape, frames, kernel, f"order {w}x{h} draw {again}", fold_ring=0)
        assert st.ordered_launches == again and st.trace_launches == 1, (st.ordered_launches, st.trace_launches)
        sums, order = r.tile_order()
        assert len(sums) == len(order) == ntiles
        nhead = U.check_order(sums, order)
        if again == 0:
            learnt = (sums, order)
        else:  # the ordered draw did not learn again
            assert np.array_equal(sums, learnt[0]) and np.array_equal(order, learnt[1])
    # a finished sample adds its queries, and one more if the bounce cap ended its path
    q = U.oracle("sphere", w, h, frames)[1]
    assert q <= int(sums.astype(np.int64).sum()) <= q + w * h * frames, (q, int(sums.sum()))
    print(f"order {w}x{h}: {ntiles} tiles, nhead {nhead}, classes {sorted(set(U.order_class(sums).tolist()))}")
    if ntiles < 2:
        assert nhead == 0
    if tuple(shape) in U.SLITS:  # the seams are crossed: a head sorted by class and block, and a tail
        assert len(set(U.order_class(sums).tolist())) >= 3
        assert 0 < nhead < ntiles
