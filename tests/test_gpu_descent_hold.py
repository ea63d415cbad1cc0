"""The descent hold of k_trace_split's culling walk (bvh_walk_noovf<.., HOLD>).

After a box step that fewer than `hold` lanes of a wave would follow with another one, while other walking lanes wait
at a leaf or a miss, the wave leaves the descent loop; the stragglers keep their internal node, do not pop, and take their
next step in the next outer iteration beside the lanes that did pop. Every lane takes exactly the steps it took before,
in the same order, so for every hold and every suspend threshold the image and the query count must equal the oracle's
bit for bit, and the box / sphere test counts must equal the hold-0 draw's ("same per-lane visits"). The thresholds
cover the edges of both checks: hold 1 (a hold no count is below), 2 (the smallest that acts), 64 (every step with a
waiting lane is held); suspend_below 1 (never suspended: held lanes only ever resume inside one call) and 64 (suspended
after nearly every pop: held internal nodes go through Q.node and bvh_walk_noovf's entry).
"""
import numpy as np
import pytest

import hrt
import scenes
from test_gpu_packet import _coincident
from test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu

HOLDS = (0, 1, 2, 12, 32, 64)
SUSPENDS = (1, 16, 24, 64)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _c3_zero_bounces():
    sd = scenes.config_c3(64, 40, 4)
    sd.bounces = 0
    return sd


CASES = {
    "c3_whole_tiles": lambda: scenes.config_c3(64, 40, 4),
    "c3_ragged_tiles": lambda: scenes.config_c3(60, 36, 4),
    "c3_zero_bounces": _c3_zero_bounces,
    "coincident": _coincident,                                   # every t ties: the lowest slot wins
    "nested_clusters": lambda: _random_scene("nested_clusters", 7),  # a full-depth LDS tree, several candidates per leaf
}
_ORACLE = {}


def _oracle(case):
    if case not in _ORACLE:  # computed once per scene, shared by every test below
        _ORACLE[case] = scenes.oracle_render(CASES[case]())
    return _ORACLE[case]


def _draw(sd, hold, **params):
    r = scenes.make_renderer(sd)  # (count_tests = 1)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE, **params)
    if hold is not None:
        r.set_descent_hold(hold)
    r.draw_frames(sd.frames, 1000, 10)
    return r.read_image(), r.stats()


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_hold_and_suspend_threshold_walks_the_same_visits(case):
    sd = CASES[case]()
    ref, q = _oracle(case)
    base = None
    for sb in SUSPENDS:
        for hold in HOLDS:
            img, st = _draw(sd, hold, variant=4, suspend_below=sb, steal=1)  # (small launches steal by default)
            what = f"{case} hold {hold} suspend_below {sb}"
            # the kernel with the hold: LDS nodes, no stealing, counting, no packet
            assert st.kernel.decode().startswith("k_trace_split<true, false, true, false>"), (what, st.kernel)
            assert st.suspend_below == sb
            np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=what)
            assert st.queries == q, what
            if base is None:
                assert hold == 0
                base = (st.box_tests, st.sphere_tests)
                if sd.bounces != 0:
                    assert base[0] > 0 and base[1] > 0
            assert (st.box_tests, st.sphere_tests) == base, what


def test_default_hold_and_the_uncounted_kernel():
    """The renderer's own default (setter not called) through the timed, uncounted instantiation."""
    sd = scenes.config_c3(60, 36, 4)
    ref, q = _oracle("c3_ragged_tiles")
    img, st = _draw(sd, None, variant=4, count_tests=0, steal=1)
    assert st.kernel.decode().startswith("k_trace_split<true, false, false, false>"), st.kernel
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert st.queries == q


@pytest.mark.parametrize("hold", [2, 12, 64])
def test_hold_in_the_stealing_kernel(hold):
    sd = scenes.config_c3(60, 36, 4)
    ref, q = _oracle("c3_ragged_tiles")
    img0, st0 = _draw(sd, 0, variant=4, steal=2)
    img, st = _draw(sd, hold, variant=4, steal=2)
    assert st.kernel.decode().startswith("k_trace_split<true, true, true, false>"), st.kernel
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32), err_msg=f"steal, hold {hold}")
    assert st.queries == q == st0.queries
    assert (st.box_tests, st.sphere_tests) == (st0.box_tests, st0.sphere_tests)


def test_setter_range_on_a_renderer():
    r = hrt.Renderer(8, 8, hrt.RT_MODE_SPHERE)
    for hold in (0, 64):
        r.set_descent_hold(hold)
    with pytest.raises(hrt.RtError) as e:
        r.set_descent_hold(65)
    assert "0..64" in str(e.value)


def test_k_trace_draws_the_same_image():
    """The linear scan in k_trace (no culling walk, so no hold) against the held walk: same image, same queries."""
    sd = scenes.config_c3(60, 36, 4)
    img1, st1 = _draw(sd, 12, variant=1)
    img4, st4 = _draw(sd, 12, variant=4, steal=1)
    assert st1.kernel.decode().startswith("k_trace<") and st4.kernel.decode().startswith("k_trace_split<true")
    np.testing.assert_array_equal(img1.view(np.uint32), img4.view(np.uint32))
    assert st1.queries == st4.queries == _oracle("c3_ragged_tiles")[1]
