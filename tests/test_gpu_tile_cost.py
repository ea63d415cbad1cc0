"""What a learning launch of cost-ordered dealing learns (rt_params.cost_order; include/hrt_testing.h
rt_testing_get_tile_order).

A finished sample adds its bounces + 1 to its pixel's counter, and the tiles are ordered by the sums. The sums do not
depend on which kernel traced the samples or in which order, so the sample-buffer kernel without stealing — which finds
the pixel from the sample's index in the launch's buffer — must learn what the stealing kernel learns, which carries
the pixel itself: tile for tile, on ragged tiles, whole images and a rank's row share, in one launch and in several.
"""
import numpy as np
import pytest

import hrt
import scenes
from hrt.parallel import rank_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _learn(sd, steal, count_tests, **params):
    r = scenes.make_renderer(sd)
    # cost_order 3: every launch learns, so the sums are the last launch's (the counters are cleared when they are summed)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, fold=hrt.RT_FOLD_BUFFER, steal=steal, job_frames=8, cost_order=3,
                 count_tests=count_tests, **params)
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    want = f"k_trace_split<true, {'true' if steal == 2 else 'false'}, {'true' if count_tests else 'false'}, false>"
    assert st.kernel.decode() == want and st.fold_ring == 0, (st.kernel, st.fold_ring)
    sums, order = r.tile_order()
    return sums, order, st, r.read_image()


@pytest.mark.parametrize("case", ["one_launch", "two_launches", "row_share"])
def test_learnt_costs_do_not_depend_on_the_kernel(case):
    sd = scenes.config_c3(70, 45, 33) if case != "row_share" else scenes.config_c3(64, 72, 9)
    params = {"two_launches": {"queue_budget_mb": 1}, "row_share": rank_params(3, 8, 8)}.get(case, {})
    tiles = ((sd.width + 7) // 8) * ((45 + 7) // 8 if case != "row_share" else 1)
    ref = _learn(sd, 2, 1, **params)  # the stealing kernel: the pixel carried from the deal to the store
    assert len(ref[0]) == tiles and sorted(ref[1]) == list(range(tiles))
    # every sample adds at least 1: a tile's sum is at least its pixels in the image x the last launch's frames
    frames = {"two_launches": 9}.get(case, sd.frames)
    ys = 8 if case == "row_share" else sd.height
    inside = np.array([min(8, sd.width - 8 * (t % ((sd.width + 7) // 8))) * min(8, ys - 8 * (t // ((sd.width + 7) // 8)))
                       for t in range(tiles)])
    assert (ref[0] >= inside * frames).all() and (ref[0] <= inside * frames * 51).all()
    for count_tests in (1, 0):
        got = _learn(sd, 1, count_tests, **params)
        np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{case} sums, count_tests {count_tests}")
        np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{case} order, count_tests {count_tests}")
        np.testing.assert_array_equal(got[3].view(np.uint32), ref[3].view(np.uint32))
        assert got[2].queries == ref[2].queries
