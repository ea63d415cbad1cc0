"""rt_regroup_paths (Renderer.regroup_paths, trace_wavefront's regroup_after): a path index list sorted on the device by
a coherence key, stably, with the live count left on the device.

The contract fixes the result bit for bit, so every comparison here is of integer arrays against a numpy model
(np.argsort(kind="stable") of the entries' keys), with no tolerance: the caller's keys (mode 2) at the sizes where the
kernels change shape (a wave, a round, a tile, several tiles, more tiles than one iteration of the scan), indirection with
duplicate and out-of-range indices, every kind of count_in, the cell-and-octant key (mode 1) against the host function,
the sort in place, and the wavefront loop with regrouping against the traced frame.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hrt
import scenes
from hrt import _lib
from test_regroup_abi import BOXES, C3_BOX, handmade_rays, random_rays

pytestmark = pytest.mark.gpu

T = hrt.REGROUP_TILE
SENTINEL = 0x5A5A5A5A
TAIL = 7  # sentinel words kept after position n of each output
# 300,000 entries are 293 tiles of 1024: k_regroup_scan takes 256 tiles per iteration of its loop, so it runs two
# iterations (the second one partial, with the carry of the first); every smaller size here runs one.
N_TWO_SCAN_ITERATIONS = 300_000
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, N_TWO_SCAN_ITERATIONS)
assert N_TWO_SCAN_ITERATIONS > 256 * T


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


@pytest.fixture(scope="module")
def bare():
    """A renderer with no scene and no camera: regrouping needs neither."""
    return hrt.Renderer(8, 8, hrt.RT_MODE_SPHERE)


def _dev(r):
    return torch.device("cuda", r.device()[0])


def _up(r, a):
    """A uint32 / float32 numpy array as an int32 / float32 tensor on the renderer's device."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(_dev(r))


def _down(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _sentinels(r, n):
    return torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=_dev(r))


def model(entry_keys, idx, live):
    """The contract: the first `live` entries in ascending key order, equal keys in input order."""
    order = np.argsort(entry_keys[:live], kind="stable")
    return idx[:live][order], entry_keys[:live][order]


def key_sets(n, rng):
    i = np.arange(n, dtype=np.uint64)
    sets = {
        "equal": np.full(n, 0x01020304, dtype=np.uint32),
        "sorted": (i * 7 + 3).astype(np.uint32),
        "descending": (np.uint64(0xFFFFFFF0) - i * 11).astype(np.uint32),
        "random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        "top-byte": (rng.integers(0, 256, n, dtype=np.uint64) << 24 | 0x00ABCDEF).astype(np.uint32),
        "bottom-byte": (rng.integers(0, 256, n, dtype=np.uint64) | 0x12345600).astype(np.uint32),
        "alternating": np.where(i % 2 == 0, 0x80000001, 0x7FFFFFFE).astype(np.uint32),
        "extremes": rng.choice(np.array([0, 0xFFFFFFFF, 0x00FFFFFF, 1, 0xFFFFFFFE], dtype=np.uint32), n),
    }
    if n >= 2:
        sets["extremes"][0], sets["extremes"][-1] = 0xFFFFFFFF, 0
    return sets


def check_outputs(what, out_idx, out_keys, want_idx, want_keys, live):
    got_idx, got_keys = _down(out_idx), _down(out_keys)
    bad = np.flatnonzero(got_idx[:live] != want_idx)
    assert bad.size == 0, (what, "index_out", bad[:5].tolist(), got_idx[bad[:5]].tolist(), want_idx[bad[:5]].tolist())
    bad = np.flatnonzero(got_keys[:live] != want_keys)
    assert bad.size == 0, (what, "keys_out", bad[:5].tolist())
    assert (got_idx[live:] == SENTINEL).all(), (what, "index_out written at or past live")
    assert (got_keys[live:] == SENTINEL).all(), (what, "keys_out written at or past live")


# ------------------------------------------------------------------------------------------------ mode 2: the sort
@pytest.mark.parametrize("n", SIZES)
def test_caller_keys_sort_as_the_stable_argsort(bare, n):
    rng = np.random.default_rng(n)
    for name, keys in key_sets(n, rng).items():
        idx = np.arange(n, dtype=np.uint32)
        out_idx, out_keys = _sentinels(bare, n), _sentinels(bare, n)
        bare.regroup_paths(out_idx, keys=_up(bare, keys), keys_out=out_keys, n=n)
        want_idx, want_keys = model(keys, idx, n)
        check_outputs(f"n {n} keys {name}", out_idx, out_keys, want_idx, want_keys, n)
        if name == "equal":  # the stability check: the output is the input order
            assert (_down(out_idx)[:n] == idx).all()


def test_without_keys_out(bare):
    n = 3 * T + 17
    keys = np.random.default_rng(5).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    out_idx = _sentinels(bare, n)
    bare.regroup_paths(out_idx, keys=_up(bare, keys), n=n)
    assert (_down(out_idx)[:n] == model(keys, np.arange(n, dtype=np.uint32), n)[0]).all()
    assert (_down(out_idx)[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ indirection
@pytest.mark.parametrize("n", (65, 3 * T + 17))
def test_indirection_duplicates_and_indices_past_paths(bare, n):
    """index_in is a random permutation with a duplicate index and entries >= paths; those sort last with the all-ones key
    and nothing is read through them: `paths` is the whole allocation of the keys tensor, so keys[j] for j >= paths would
    lie outside it."""
    rng = np.random.default_rng(n + 1)
    paths = n
    keys = rng.integers(0, 1 << 32, paths, dtype=np.uint64).astype(np.uint32)
    keys[rng.integers(0, paths, 8)] = 0xFFFFFFFF  # real paths with the largest key: they tie with the out-of-range entries
    idx = rng.permutation(paths).astype(np.uint32)
    idx[3] = idx[40]  # a duplicate
    idx[[1, n // 2, n - 1]] = [paths, 0xFFFFFFFF, paths + 12345]  # entries >= paths, the first one just past the end
    keys_t = _up(bare, keys)
    assert keys_t.untyped_storage().nbytes() == 4 * paths  # `paths` ends at the end of the tensor's allocation
    entry_keys = np.where(idx < paths, keys[np.minimum(idx, paths - 1)], np.uint32(0xFFFFFFFF)).astype(np.uint32)
    out_idx, out_keys = _sentinels(bare, n), _sentinels(bare, n)
    bare.regroup_paths(out_idx, keys=keys_t, index_in=_up(bare, idx), keys_out=out_keys, n=n)
    want_idx, want_keys = model(entry_keys, idx, n)
    check_outputs(f"indirection n {n}", out_idx, out_keys, want_idx, want_keys, n)
    assert (want_keys[-3:] == 0xFFFFFFFF).all()
    # the keys tensor was only read
    assert (_down(keys_t) == keys).all()


# ------------------------------------------------------------------------------------------------ count_in
@pytest.mark.parametrize("n", (257, 3 * T + 17))
def test_count_in_limits_the_sort(bare, n):
    rng = np.random.default_rng(n + 2)
    keys = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint32)  # (ties as well)
    idx = rng.permutation(n).astype(np.uint32)
    keys_t, idx_t = _up(bare, keys), _up(bare, idx)
    for count in (0, 1, 64, n - 1, n, n + 1000):
        live = min(n, count)
        count_t = torch.tensor([count], dtype=torch.int32, device=_dev(bare))
        out_idx, out_keys = _sentinels(bare, n), _sentinels(bare, n)
        bare.regroup_paths(out_idx, keys=keys_t, index_in=idx_t, count_in=count_t, keys_out=out_keys, n=n)
        want_idx, want_keys = model(keys[idx], idx, live)
        check_outputs(f"n {n} count_in {count}", out_idx, out_keys, want_idx, want_keys, live)
        assert int(count_t.item()) == count  # the count buffer is only read
        if count == 0:
            assert (_down(out_idx) == SENTINEL).all() and (_down(out_keys) == SENTINEL).all()
    assert (_down(idx_t) == idx).all()


# ------------------------------------------------------------------------------------------------ mode 1: the key
@pytest.mark.parametrize("box", sorted(BOXES))
def test_cell_octant_keys_are_the_hosts(bare, box):
    lo, hi = (np.array(v, dtype=np.float32) for v in BOXES[box])
    for what, (o, d) in (("handmade", handmade_rays(lo, hi)), ("random", random_rays(lo, hi))):
        n = len(o)
        host = hrt.regroup_keys(o, d, lo, hi)
        out_idx, out_keys = _sentinels(bare, n), _sentinels(bare, n)
        o_t, d_t = _up(bare, o), _up(bare, d)
        bare.regroup_paths(out_idx, origins=o_t, dirs=d_t, box=(lo, hi), keys_out=out_keys, n=n)
        want_idx, want_keys = model(host, np.arange(n, dtype=np.uint32), n)
        check_outputs(f"box {box} {what}", out_idx, out_keys, want_idx, want_keys, n)
        assert (_down(o_t) == o.view(np.uint32)).all() and (_down(d_t) == d.view(np.uint32)).all()
    # an index >= paths takes the largest 24-bit key
    idx = np.array([2, n, 0, 0xFFFFFFFF, 1], dtype=np.uint32)
    out_idx, out_keys = _sentinels(bare, 5), _sentinels(bare, 5)
    bare.regroup_paths(out_idx, origins=o_t, dirs=d_t, box=(lo, hi), index_in=_up(bare, idx), keys_out=out_keys, n=5)
    entry_keys = np.where(idx < n, host[np.minimum(idx, n - 1)], np.uint32(0x00FFFFFF)).astype(np.uint32)
    check_outputs(f"box {box} past paths", out_idx, out_keys, *model(entry_keys, idx, 5), 5)


# ------------------------------------------------------------------------------------------------ in place
@pytest.mark.parametrize("n", (64, T + 1, 3 * T + 17))
def test_in_place_is_the_same_sort(bare, n):
    rng = np.random.default_rng(n + 3)
    keys = rng.integers(0, 1 << 10, n, dtype=np.uint64).astype(np.uint32)
    idx = rng.permutation(n).astype(np.uint32)
    keys_t = _up(bare, keys)
    separate = _sentinels(bare, n)
    bare.regroup_paths(separate, keys=keys_t, index_in=_up(bare, idx), n=n)
    both = _sentinels(bare, n)
    both[:n] = _up(bare, idx)
    count_t = torch.tensor([n - 5], dtype=torch.int32, device=_dev(bare))
    bare.regroup_paths(both, keys=keys_t, index_in=both, n=n)
    assert (_down(both) == _down(separate)).all()
    assert (_down(both)[:n] == model(keys[idx], idx, n)[0]).all()
    # with a count: the entries past it stay where they were
    both[:n] = _up(bare, idx)
    bare.regroup_paths(both, keys=keys_t, index_in=both, count_in=count_t, n=n)
    got = _down(both)
    assert (got[:n - 5] == model(keys[idx], idx, n - 5)[0]).all() and (got[n - 5:n] == idx[n - 5:]).all()
    assert (got[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the wavefront loop
def _sphere_extent(sd):
    """The scene's own extent: the bounds of its spheres, the ground spheres (radius >= 100) left out."""
    s = sd.spheres[sd.spheres["radius"] < 100.0]
    c, rad = s["center"].astype(np.float64), s["radius"].astype(np.float64)[:, None]
    return tuple((c - rad).min(axis=0)), tuple((c + rad).max(axis=0))


def _mesh_extent(sd):
    """The scene's own extent: the bounds of its triangles' vertices."""
    tris = sd.bvh[2]
    v = np.concatenate([tris[k][:, :3] for k in ("a", "b", "c")]).astype(np.float64)
    return tuple(v.min(axis=0)), tuple(v.max(axis=0))


def _suzane(w, h):
    sd = scenes._tris_scene("suzane", w, h, 1)
    sd.bounces = 5
    return sd


def _complex(w, h):
    sd = scenes.golden_scene("complex_scene", w, h)
    sd.frames, sd.bounces = 1, 10
    return sd


# case -> (scene builder, the scene's own bounces, its box)
LOOP_CASES = {
    "complex_scene": (_complex, 10, _sphere_extent),
    "c3": (lambda w, h: scenes.config_c3(w, h, 1), 50, lambda sd: C3_BOX),
    "suzane": (_suzane, 5, _mesh_extent),
}


@pytest.mark.parametrize("case", sorted(LOOP_CASES))
def test_wavefront_with_regrouping_is_the_traced_frame(case):
    """A lost or doubled index, or a count that moved, shows as a wrong radiance or query count."""
    build, bounces, box_of = LOOP_CASES[case]
    for w, h in ((70, 45), (64, 40)):
        sd = build(w, h)
        box = box_of(sd)
        r = scenes.make_renderer(sd)
        r.set_params(bounces=bounces)
        o, d = r.primary_rays(1000)
        s = r.primary_rng(1000)
        ref, rq = r.trace_frame(1000, want_queries=True)
        for after in ((1,), tuple(range(1, bounces + 1))):
            what = f"{case} {w}x{h} regroup after {after[:3]}.."
            got, gq = r.trace_wavefront(o.view(-1, 3), d.view(-1, 3), s.view(-1), bounces, want_queries=True,
                                        regroup_box=box, regroup_after=after)
            bad = (_down(got) != _down(ref).reshape(-1, 3)).any(axis=1)
            assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            np.testing.assert_array_equal(gq.cpu().numpy(), rq.cpu().numpy().reshape(-1), err_msg=what)


def test_after_a_real_bounce_step():
    """The step's index_out keeps no order between waves, so: the same set, keys_out non-decreasing, and keys_out[k] the
    host key of path index_out[k]'s ray after the step."""
    sd = scenes.config_c3(70, 45, 1)
    r = scenes.make_renderer(sd)
    o, d = (t.view(-1, 3).clone() for t in r.primary_rays(1000))
    s = r.primary_rng(1000).view(-1).clone()
    n = int(o.shape[0])
    dev = _dev(r)
    index, count = _sentinels(r, n), torch.zeros((1,), dtype=torch.int32, device=dev)
    r.bounce_rays(o, d, s, index_out=index, count_out=count, n=n)
    live = int(count.item())
    assert 64 < live < n
    out_idx, out_keys = _sentinels(r, n), _sentinels(r, n)
    r.regroup_paths(out_idx, origins=o, dirs=d, box=C3_BOX, index_in=index, count_in=count, keys_out=out_keys, n=n)
    got_idx, got_keys = _down(out_idx), _down(out_keys)
    assert (np.sort(got_idx[:live]) == np.sort(_down(index)[:live])).all()
    assert (np.diff(got_keys[:live].astype(np.int64)) >= 0).all()
    host = hrt.regroup_keys(o.cpu().numpy(), d.cpu().numpy(), *C3_BOX)
    assert (got_keys[:live] == host[got_idx[:live]]).all()
    assert len(np.unique(got_keys[:live])) > 50  # (the survivors do spread over many cells)
    assert (got_idx[live:] == SENTINEL).all() and (got_keys[live:] == SENTINEL).all()
    assert int(count.item()) == live


# ------------------------------------------------------------------------------------------------ isolation
def test_a_regroup_leaves_the_draw_state_alone():
    """A draw before and after a regroup leaves the image of two draws without it; frame count, stats (but the times and
    the device memory held, which now includes the sort's scratch) and raw counters are those of the plain pair."""
    sd = scenes.config_c3(64, 40, 1)
    results = []
    for regroup in (False, True):
        r = scenes.make_renderer(sd)
        r.set_time(1000)
        r.draw()
        if regroup:
            n = 3 * T + 17
            keys = np.random.default_rng(9).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            out_idx = _sentinels(r, n)
            r.regroup_paths(out_idx, keys=_up(r, keys), n=n)
            assert (_down(out_idx)[:n] == model(keys, np.arange(n, dtype=np.uint32), n)[0]).all()
        r.set_time(1010)
        r.draw()
        img = r.read_image()
        st = r.stats()
        fields = {f[0]: getattr(st, f[0]) for f in _lib.RtStats._fields_
                  if f[0] not in ("kernel_ms", "trace_ms", "device_bytes")}
        results.append((img.view(np.uint32), r.frame_count, fields, r.raw_counters()))
    (img_a, fc_a, st_a, raw_a), (img_b, fc_b, st_b, raw_b) = results
    assert (img_a == img_b).all()
    assert fc_a == fc_b == 2
    assert st_a == st_b
    assert raw_a == raw_b


# ------------------------------------------------------------------------------------------------ errors
def _io(r, n, **kw):
    """A valid mode 2 call's struct over real device buffers, with fields replaced."""
    dev = _dev(r)
    bufs = {name: torch.zeros((max(n, 1) + 4,), dtype=torch.int32, device=dev) for name in ("keys", "index_in", "out", "ko")}
    rays = torch.zeros((max(n, 1) + 4, 3), dtype=torch.float32, device=dev)
    io = _lib.RtRegroup(rays.data_ptr(), rays.data_ptr(), bufs["keys"].data_ptr(), bufs["index_in"].data_ptr(), None,
                        bufs["out"].data_ptr(), bufs["ko"].data_ptr(), n, _lib.REGROUP_KEYS,
                        (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), 0, 0)
    for k, v in kw.items():
        setattr(io, k, v)
    return io, (bufs, rays)


def test_argument_errors(bare):
    L, h, n = hrt.lib(), bare._h, 100
    torch.cuda.synchronize()
    io, keep = _io(bare, n)
    assert L.rt_regroup_paths(h, C.byref(io), n) == _lib.RT_OK  # the struct the cases below spoil is valid
    assert L.rt_regroup_paths(h, None, n) == _lib.RT_ERR_ARG  # a null io
    cell = _lib.REGROUP_CELL_OCTANT
    nan, inf = float("nan"), float("inf")
    cases = {
        "null index_out": dict(index_out_dev=None),
        "null origins in mode 1": dict(mode=cell, origins_dev=None),
        "null dirs in mode 1": dict(mode=cell, dirs_dev=None),
        "null keys in mode 2": dict(keys_dev=None),
        "mode 0": dict(mode=0),
        "mode 3": dict(mode=3),
        "reserved": dict(reserved=1),
        "misaligned keys": dict(keys_dev=io.keys_dev + 2),
        "misaligned origins": dict(mode=cell, origins_dev=io.origins_dev + 1),
        "misaligned dirs": dict(mode=cell, dirs_dev=io.dirs_dev + 2),
        "misaligned index_in": dict(index_in_dev=io.index_in_dev + 1),
        "misaligned count_in": dict(count_in_dev=io.index_in_dev + 3),
        "misaligned index_out": dict(index_out_dev=io.index_out_dev + 2),
        "misaligned keys_out": dict(keys_out_dev=io.keys_out_dev + 1),
        "n above paths without index_in": dict(index_in_dev=None, paths=n - 1),
        "box hi == lo": dict(mode=cell, box_hi=(C.c_float * 3)(1, 0, 1)),
        "box hi < lo": dict(mode=cell, box_hi=(C.c_float * 3)(1, 1, -1)),
        "box NaN": dict(mode=cell, box_lo=(C.c_float * 3)(nan, 0, 0)),
        "box infinite": dict(mode=cell, box_hi=(C.c_float * 3)(1, inf, 1)),
    }
    for what, fields in cases.items():
        bad, keep2 = _io(bare, n)
        for k in ("origins_dev", "dirs_dev", "keys_dev", "index_in_dev", "index_out_dev", "keys_out_dev"):
            setattr(bad, k, getattr(io, k))
        for k, v in fields.items():
            setattr(bad, k, v)
        assert L.rt_regroup_paths(h, C.byref(bad), n) == _lib.RT_ERR_ARG, what
        assert b"rt_regroup_paths" in L.rt_last_error(), what
    # more than RT_REGROUP_MAX_ENTRIES entries: refused before anything is allocated or launched
    big, keep3 = _io(bare, n, paths=0xFFFFFFFF)
    assert L.rt_regroup_paths(h, C.byref(big), _lib.REGROUP_MAX_ENTRIES + 1) == _lib.RT_ERR_ARG
    # the same good struct in mode 1, and n = 0 with anything at all
    good, keep4 = _io(bare, n, mode=cell)
    assert L.rt_regroup_paths(h, C.byref(good), n) == _lib.RT_OK
    assert L.rt_regroup_paths(h, C.byref(bad), 0) == _lib.RT_OK
    assert L.rt_regroup_paths(h, None, 0) == _lib.RT_OK
    bare.synchronize()
    # a buffer the mode does not read may be NULL
    io2, keep5 = _io(bare, n, origins_dev=None, dirs_dev=None)
    assert L.rt_regroup_paths(h, C.byref(io2), n) == _lib.RT_OK
    io3, keep6 = _io(bare, n, mode=cell, keys_dev=None)
    assert L.rt_regroup_paths(h, C.byref(io3), n) == _lib.RT_OK
    bare.synchronize()
    # the Python layer: exactly one of box and keys
    out = _sentinels(bare, 4)
    with pytest.raises(ValueError):
        bare.regroup_paths(out, n=4)
    with pytest.raises(ValueError):
        bare.regroup_paths(out, keys=out, box=BOXES["unit"], origins=keep[1], dirs=keep[1], n=4)


# ------------------------------------------------------------------------------------------------ scratch
def test_after_release_scratch_the_same_result_again():
    r = hrt.Renderer(8, 8, hrt.RT_MODE_SPHERE)
    n = 3 * T + 17
    keys = np.random.default_rng(11).integers(0, 1 << 20, n, dtype=np.uint64).astype(np.uint32)
    want = model(keys, np.arange(n, dtype=np.uint32), n)
    keys_t = _up(r, keys)
    for attempt in range(3):
        out_idx, out_keys = _sentinels(r, n), _sentinels(r, n)
        r.regroup_paths(out_idx, keys=keys_t, keys_out=out_keys, n=n)
        check_outputs(f"attempt {attempt}", out_idx, out_keys, *want, n)
        r.release_scratch()
    r.release_scratch()  # (twice in a row, and before close)
    r.close()
