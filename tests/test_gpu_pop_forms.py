"""The pop of k_trace_split's culling walk as selects (rt_kernels.hip bvh_walk_noovf<.., HOLD>, its pop).

After a leaf or a miss a lane pops its next node: the entry below the top of its LDS stack is read by every lane — entry
0 for an empty stack, its value discarded — and the new node, the new depth and "finished" are selects; a lane the
descent hold keeps at an internal node keeps both. The nested-clusters scene builds a full-depth tree (pops at depth 8)
of leaves with several candidates; suspend_below 1 never suspends, so every pop down to the last one at depth 0 happens
inside one call, and 64 suspends after nearly every pop, so popped and held nodes pass through the saved query state.
Same visits for every hold: the oracle's image and query count, and the box / sphere test counts of the hold-0 draw.
"""
import numpy as np
import pytest

import hrt
import scenes
from test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


@pytest.fixture(scope="module")
def chain():
    sd = _random_scene("nested_clusters", 7)
    sd.width, sd.height, sd.frames = 44, 28, 3  # ragged 8x8 tiles
    ref, q = scenes.oracle_render(sd)
    ref.setflags(write=False)
    return sd, ref, q


@pytest.mark.parametrize("count_tests", [1, 0])
@pytest.mark.parametrize("suspend_below", [1, 64])
def test_pops_at_depth_zero_and_full_depth(chain, suspend_below, count_tests):
    sd, ref, q = chain
    base = None
    for hold in (0, 2, 12, 64):
        r = scenes.make_renderer(sd)
        r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, variant=4, suspend_below=suspend_below, steal=1,
                     count_tests=count_tests)
        r.set_descent_hold(hold)
        r.draw_frames(sd.frames, 1000, 10)
        img, st = r.read_image(), r.stats()
        what = f"suspend_below {suspend_below} hold {hold} count_tests {count_tests}"
        want = f"k_trace_split<true, false, {'true' if count_tests else 'false'}, false>"
        assert st.kernel.decode() == want, (what, st.kernel)
        assert st.suspend_below == suspend_below
        np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
        assert st.queries == q, what
        if count_tests:
            base = base or (st.box_tests, st.sphere_tests)
            assert base[0] > 0 and (st.box_tests, st.sphere_tests) == base, what
