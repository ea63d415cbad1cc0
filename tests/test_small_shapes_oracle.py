"""The CPU side of test_gpu_small_shapes.py: what the oracle gives at the degenerate image shapes, and the numpy
restatement of the tile order's rule on hand-made sums (small_shapes_util.py).

At a width or height of 1 make_ray divides 0 by W - 1 = 0 or H - 1 = 0: the primary ray is NaN, no intersection test
passes, the sky colour of a NaN direction is NaN, and the sample ends after its one query. That is the contract the GPU
draws are held to, so it is pinned here: all NaN, queries = W H frames, in every program. At the regular shapes no
channel is non-finite, so the GPU comparison there is of bits with no NaN rule.
"""
import numpy as np
import pytest

import hrt
import scenes
import small_shapes_util as U


def test_scene_is_the_uniform_guards_spheres():
    import test_gpu_uniform_guards as G
    assert hrt.spheres_array(U.four_spheres()).tobytes() == hrt.spheres_array(G._spheres()).tobytes()


@pytest.mark.parametrize("program", list(U.PROGRAMS))
@pytest.mark.parametrize("shape", U.ONE_WIDE, ids=U.shape_id)
def test_one_wide_shapes_are_all_nan_with_one_query_per_sample(shape, program):
    w, h = shape
    for frames in U.FRAMES:
        img, q, nodes, tris = U.oracle(program, w, h, frames)
        assert img.shape == (h, w, 3)
        assert np.isnan(img).all(), (shape, frames, img)
        assert q == w * h * frames, (shape, frames, q)
        if program != "sphere":  # a NaN ray fails the root box: one node test a query, no triangle
            assert (nodes, tris) == (q, 0), (shape, frames, nodes, tris)


@pytest.mark.parametrize("program", list(U.PROGRAMS))
@pytest.mark.parametrize("shape", U.REGULAR, ids=U.shape_id)
def test_regular_shapes_are_finite(shape, program):
    w, h = shape
    for frames in U.FRAMES:
        img, q, _, _ = U.oracle(program, w, h, frames)
        assert img.shape == (h, w, 3)
        assert np.isfinite(img).all(), (shape, frames)
        assert q >= w * h * frames
        if program == "sphere":  # some path bounces: the draws are not all sky
            assert q > w * h * frames, (shape, frames, q)


def test_nan_rule_is_not_the_bits_rule():
    """The two comparison rules on hand-made images: the NaN rule passes another NaN's bits and nothing else; the bits
    rule refuses a NaN reference outright."""
    ref = np.array([[[1.0, np.nan, 0.5]]], dtype=np.float32)
    other = ref.copy()
    other.view(np.uint32)[0, 0, 1] ^= 0x80000001  # another sign and payload
    assert np.isnan(other[0, 0, 1])
    U.assert_nan_rule(other, ref, "another NaN")
    with pytest.raises(AssertionError):
        U.assert_bits(other, ref, "a NaN reference")
    for bad in (np.array([[[1.0, 2.0, 0.5]]], np.float32), np.array([[[np.nan, np.nan, 0.5]]], np.float32),
                np.array([[[1.0, np.nan, np.nextafter(np.float32(0.5), np.float32(1.0))]]], np.float32)):
        with pytest.raises(AssertionError):
            U.assert_nan_rule(bad, ref, "a wrong image")
    fin = np.array([[[1.0, 0.25, -0.0]]], dtype=np.float32)
    U.assert_bits(fin.copy(), fin, "equal")
    with pytest.raises(AssertionError):
        U.assert_bits(np.array([[[1.0, 0.25, 0.0]]], np.float32), fin, "the sign of zero")
    with pytest.raises(AssertionError):  # all NaN is required at a one-wide shape, of the image and of the reference
        U.assert_image(np.array([[[np.nan, np.nan, 1.0]]], np.float32), np.full((1, 1, 3), np.nan, np.float32), (1, 1), "")
    with pytest.raises(AssertionError):
        U.assert_image(np.full((2, 2, 3), np.nan, np.float32), np.full((2, 2, 3), np.nan, np.float32), (2, 2), "")


# ------------------------------------------------------------------------------------------------- the tile order's rule
def test_order_classes():
    c = U.order_class([0, 1, 2, 3, 4, 6, 7, 2 ** 24, 2 ** 32 - 1])
    # floor(4 log2(c + 1)): 0, 4, 6 (log2 3 = 1.58), 8, 9 (log2 5 = 2.32), 11 (log2 7 = 2.81), 12, 96, 127 (2^32: clamped)
    assert (127 - c).tolist() == [0, 4, 6, 8, 9, 11, 12, 96, 127]


def test_order_rule_empty_head():
    # one tile: cap = 0; three tiles of three classes: cap = 1 and the head is the one most expensive tile
    cls, cut, nhead = U.order_head([77])
    assert nhead == 0 and cut == cls[0]  # (the empty classes before the tile's fit; its own does not)
    assert U.one_order([77]).tolist() == [0] and U.check_order([77], [0]) == 0
    # two tiles of one class: cap = 1 < 2
    assert U.check_order([50, 50], [0, 1]) == 0
    with pytest.raises(AssertionError):
        U.check_order([50, 50], [1, 0])  # the tail is ascending
    assert U.one_order([5, 900, 60]).tolist() == [1, 0, 2] and U.check_order([5, 900, 60], [1, 0, 2]) == 1


def test_order_rule_everything_in_one_class():
    sums = np.full(2050, 1000, dtype=np.uint32)
    sums[::7] += 5  # (the same class: 4 log2 1001 = 39.87, 4 log2 1006 = 39.90)
    assert len(set(U.order_class(sums).tolist())) == 1
    order = U.one_order(sums)
    assert order.tolist() == list(range(2050)) and U.check_order(sums, order) == 0
    with pytest.raises(AssertionError):
        U.check_order(sums, order[::-1])


def test_order_rule_class_straddling_the_cap():
    # 10 tiles, cap 5: 2 in the most expensive class, 4 in the next (2 + 4 > 5: the head closes for good), then a class
    # of 1 that would have fit, and 3 cheap ones
    sums = np.array([10, 4000, 300, 300, 10, 300, 4000, 60, 300, 10], dtype=np.uint32)
    cls, cut, nhead = U.order_head(sums)
    assert nhead == 2 and cut == cls[2] and len(set(cls.tolist())) == 4  # (the empty classes in between still fit)
    assert U.check_order(sums, [1, 6, 0, 2, 3, 4, 5, 7, 8, 9]) == 2
    assert U.check_order(sums, [6, 1, 0, 2, 3, 4, 5, 7, 8, 9]) == 2  # one class, one block: either way round
    for wrong in ([1, 6, 7, 0, 2, 3, 4, 5, 8, 9],   # the class of 1 after the closed one
                  [1, 2, 0, 6, 3, 4, 5, 7, 8, 9],   # a tile of the straddling class in the head
                  [1, 6, 0, 2, 3, 4, 5, 7, 9, 8],   # the tail out of order
                  [1, 6, 0, 2, 3, 4, 5, 7, 8, 8]):  # not a permutation
        with pytest.raises(AssertionError):
            U.check_order(sums, wrong)
    # a head of two classes over two blocks: class first, then block; inside a class and block any order
    sums = np.full(2050, 10, dtype=np.uint32)
    sums[[5, 1030, 2049]] = 300
    sums[[7, 1500]] = 4000
    assert U.check_order(sums, U.one_order(sums)) == 5
    tail = [t for t in range(2050) if t not in (5, 7, 1030, 1500, 2049)]
    assert U.check_order(sums, [7, 1500, 5, 1030, 2049] + tail) == 5
    for wrong in ([1500, 7, 5, 1030, 2049], [7, 1500, 1030, 5, 2049], [5, 7, 1500, 1030, 2049]):
        with pytest.raises(AssertionError):
            U.check_order(sums, wrong + tail)


@pytest.mark.parametrize("shape", U.SLITS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_slits_cross_the_order_seams(shape):
    """The tall slits of the GPU order test, beforehand: the queries of every 16th tile (windowed oracle calls; a tile's
    learnt sum is its queries plus one for each path the bounce cap ended) fall into at least three classes, and the most
    expensive class alone holds fewer than half of them, so 0 < nhead < ntiles there."""
    w, h = shape
    sd = U.scene("sphere", w, h, U.ORDER_FRAMES)
    tiles = list(range(0, h // 8, 16))
    q = [scenes.oracle_render(sd, rows=(8 * t, 1, 8), threads=1)[1] for t in tiles]
    cls, cut, nhead = U.order_head(q)
    assert len(set(cls.tolist())) >= 3, sorted(set(cls.tolist()))
    assert 0 < nhead < len(tiles), (nhead, len(tiles))
