"""rt_bounce_rays (Renderer.bounce_rays, trace_wavefront): one step of trace()'s loop on path state the caller keeps in
device memory, with the surviving paths compacted into an index list.

Identity. Iterating the step `bounces` times from a frame's primary rays and RNG states, then throughput * sky, must be
bit for bit what rt_trace_rays gives for those rays (trace_frame), radiance and queries; three cases are also held
directly against the CPU oracle's one-frame image and ray count, so the pin does not rest on rt_trace_rays alone.

Everything else — one step against rt_cast_rays, the compaction, ragged and partial batches, inactive leading lanes,
indirection, optional buffers, isolation — is held against results the identity has pinned. No tolerance anywhere in this
file: every comparison is of uint32 views.
"""
import ctypes as C

import numpy as np
import pytest

import hrt
import scenes
from hrt import PI, Camera, Material, Mesh, Sphere, Tree, Vec3, f32, read_asset

pytestmark = pytest.mark.gpu

SHAPES = ((70, 45), (64, 40))  # 3150 rays: a ragged last wave; 2560: whole waves and whole workgroups
TIMES = (1000, 1010)
SENTINEL = 0x5A5A5A5A
ONE = 0x3F800000  # 1.0f


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _u32(t):
    """A float32 / int32 tensor or array as a uint32 numpy array on the host (bitwise comparisons, NaNs included)."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ scenes
# (the builders of test_gpu_trace_rays.py, restated)
def split_cube_bvh():
    """Every triangle of cube2.obj as a one-triangle mesh with a material of its own kind (Lambertian, metal, glass)."""
    whole = Tree.from_mesh(Mesh.load_obj(read_asset("cube2.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
    whole.build()
    tris = whole.view()[2]
    tree = Tree()
    for k, t in enumerate(tris):
        obj = "".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in t[v][:3]) for v in ("a", "b", "c")) + "f 1 2 3\n"
        x = (k + 1.0) / (len(tris) + 1.0)
        kind = (hrt.LAMBERTIAN, hrt.METAL, hrt.DIELECTRIC)[k % 3]
        mat = Material._make([0.05 + 0.9 * x, 0.95 - 0.9 * x, 0.5, 1.0], [(0.0, 0.1, 1.5)[k % 3]] * 3, kind)
        tree.add_mesh(Mesh.load_obj(obj.encode(), mat))
    tree.build()
    return tree.view()


def cube_scene(w, h):
    cam = Camera.new(Vec3(0.0, 2.2, 6.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.0, PI * f32(0.3))  # SceneTris::new_cube
    return scenes.SceneDef("split-cube", hrt.RT_MODE_TRIS, w, h, cam, bvh=split_cube_bvh(), frames=1, bounces=5)


def suzane_scene(w, h):
    sd = scenes._tris_scene("suzane", w, h, 1)
    sd.bounces = 5
    return sd


def _golden(name, slots=None):
    def build(w, h):
        sd = scenes.golden_scene(name, w, h)
        sd.frames, sd.bounces, sd.min_sphere_slots = 1, 10, slots
        return sd
    return build


# case -> (scene builder, the scene's own bounces, the rt_params.variant values to force (0 = by slot count))
CASES = {
    "complex_scene": (_golden("complex_scene"), 10, (0, 1, 3, 4)),
    "dielectric_materials": (_golden("dielectric_materials"), 10, (0, 1, 3, 4)),
    "metal_materials": (_golden("metal_materials"), 10, (0, 1, 3, 4)),
    "complex_scene-slots0": (_golden("complex_scene", 0), 10, (0,)),
    "c3": (lambda w, h: scenes.config_c3(w, h, 1), 50, (0,)),
    "split-cube": (cube_scene, 5, (0,)),
    "suzane": (suzane_scene, 5, (0,)),
    "c4": (lambda w, h: scenes.config_c4(w, h, 1), 50, (0,)),
    "c5": (lambda w, h: scenes.config_c5(w, h, 1), 50, (0,)),
}


def _bounce_set(own):
    return sorted({0, 1, own, 50})


def _frame_state(r, time):
    """The primary rays and RNG states of the frame at `time`, flat."""
    o, d = r.primary_rays(time)
    return o.view(-1, 3), d.view(-1, 3), r.primary_rng(time).view(-1)


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("case", sorted(CASES))
def test_wavefront_is_the_traced_frame(case):
    build, own, variants = CASES[case]
    for w, h in SHAPES:
        r = scenes.make_renderer(build(w, h))
        for time in TIMES:
            o, d, s = _frame_state(r, time)
            for b in _bounce_set(own):
                for v in variants:
                    what = f"{case} {w}x{h} time {time} bounces {b} variant {v}"
                    r.set_params(bounces=b, variant=v)
                    ref, rq = r.trace_frame(time, want_queries=True)
                    r.set_params(bounces=3)  # (the step does not read rt_params.bounces)
                    got, gq = r.trace_wavefront(o, d, s, b, want_queries=True)
                    assert tuple(got.shape) == (w * h, 3) and tuple(gq.shape) == (w * h,), what
                    bad = (_u32(got) != _u32(ref).reshape(-1, 3)).any(axis=1)
                    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
                    np.testing.assert_array_equal(gq.cpu().numpy(), rq.cpu().numpy().reshape(-1), err_msg=what)
                    if b > 0:
                        assert int(gq.min()) >= 1 and int(gq.max()) <= b, what
            # the inputs were cloned
            o2, d2, s2 = _frame_state(r, time)
            assert (_u32(o) == _u32(o2)).all() and (_u32(d) == _u32(d2)).all() and (_u32(s) == _u32(s2)).all()


@pytest.mark.parametrize("case", ["dielectric_materials", "c3", "c4"])
def test_wavefront_is_the_oracles_frame(case):
    """Directly against the CPU oracle: with frame_count 0 its one-frame image is 0.0 + trace(primary ray)."""
    build, own, _ = CASES[case]
    w, h = SHAPES[0]
    sd = build(w, h)
    r = scenes.make_renderer(sd)
    for time in TIMES:
        o, d, s = _frame_state(r, time)
        for b in _bounce_set(own):
            what = f"{case} time {time} bounces {b}"
            ref, rays = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=b)
            got, gq = r.trace_wavefront(o, d, s, b, want_queries=True)
            bad = (_u32(got).reshape(h, w, 3) != ref.view(np.uint32)).any(axis=2)
            assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            assert int(gq.sum()) == rays, (what, int(gq.sum()), rays)


@pytest.mark.parametrize("case", ["split-cube", "c4"])
def test_wavefront_with_the_sah_walk_is_the_traced_frame(case):
    build, own, _ = CASES[case]
    for w, h in SHAPES:
        r = scenes.make_renderer(build(w, h))
        r.set_params(tri_bvh=1)
        for time in TIMES:
            o, d, s = _frame_state(r, time)
            for b in _bounce_set(own):
                what = f"{case} {w}x{h} time {time} bounces {b}"
                r.set_params(bounces=b)
                ref, rq = r.trace_frame(time, want_queries=True)
                got, gq = r.trace_wavefront(o, d, s, b, want_queries=True)
                np.testing.assert_array_equal(_u32(got), _u32(ref).reshape(-1, 3), err_msg=what)
                np.testing.assert_array_equal(gq.cpu().numpy(), rq.cpu().numpy().reshape(-1), err_msg=what)


# ------------------------------------------------------------------------------------------------ path state with sentinels
class Paths:
    """Path state for `paths` rays in tensors of paths + extra rows; the rows past the paths hold SENTINEL in every word,
    throughput starts at 1, queries at 0 and the hit records at SENTINEL."""

    NAMES = ("O", "D", "S", "T", "Q", "H")

    def __init__(self, o, d, s, extra=0):
        import torch

        n, dev = int(o.shape[0]), o.device
        self.n, self.dev, self.rows = n, dev, n + extra

        def filled(cols, src=None, value=None):
            t = torch.full((self.rows, cols) if cols else (self.rows,), SENTINEL, dtype=torch.int32, device=dev)
            if src is not None:
                t[:n] = src.contiguous().view(torch.int32)
            elif value is not None:
                t[:n] = value
            return t

        self.O, self.D, self.S = filled(3, o), filled(3, d), filled(0, s)
        self.T, self.Q, self.H = filled(3, value=ONE), filled(0, value=0), filled(8)

    def step(self, r, paths=None, throughput=True, queries=True, hits=True, **kw):
        import torch

        p = self.n if paths is None else paths
        F = torch.float32
        r.bounce_rays(self.O[:p].view(F), self.D[:p].view(F), self.S[:p],
                      throughput=self.T[:p].view(F) if throughput else None, queries=self.Q[:p] if queries else None,
                      hits=self.H[:p] if hits else None, **kw)
        return self

    def snap(self):
        return {k: _u32(getattr(self, k)).copy() for k in self.NAMES}


def _ints(dev, n, value=SENTINEL):
    import torch

    return torch.full((n,), value, dtype=torch.int32, device=dev)


def _expect(before, after, processed):
    """The state in which exactly the rows `processed` (a bool mask over all rows) took the step."""
    out = {}
    for k in Paths.NAMES:
        m = processed if before[k].ndim == 1 else processed[:, None]
        out[k] = np.where(m, after[k], before[k])
    return out


def _same(got, want, what, names=Paths.NAMES):
    for k in names:
        bad = got[k] != want[k]
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.fixture(scope="module", params=["complex_scene", "c4"])
def frame(request):
    """One 70 x 45 frame's rays and states, the cast's records for them, and the state before and after one whole step
    (the identity above pins what the step does to it; the cast pins the records)."""
    build, own, _ = CASES[request.param]
    w, h = SHAPES[0]
    r = scenes.make_renderer(build(w, h))
    o, d, s = _frame_state(r, 1000)
    cast = {k: v.cpu().numpy() for k, v in r.cast_rays(o, d).items()}
    hit = cast["prim"] >= 0
    assert hit.any() and (~hit).any(), request.param
    p = Paths(o, d, s)
    before = p.snap()
    after = p.step(r).snap()
    return {"r": r, "o": o, "d": d, "s": s, "cast": cast, "hit": hit, "before": before, "after": after, "n": w * h,
            "name": request.param}


# ------------------------------------------------------------------------------------------------ one step against the cast
def test_one_step_against_the_cast(frame):
    import torch

    r, n, hit, cast = frame["r"], frame["n"], frame["hit"], frame["cast"]
    p = Paths(frame["o"], frame["d"], frame["s"], extra=8)
    before = p.snap()
    index, count = _ints(p.dev, n + 8), _ints(p.dev, 1)
    p.step(r, paths=n, index_out=index, count_out=count)
    got = p.snap()
    # the records: rt_cast_rays of the rays before the scatter, field for field
    H = got["H"][:n]
    np.testing.assert_array_equal(H[:, 0], cast["t"].view(np.uint32))
    np.testing.assert_array_equal(H[:, 1].view(np.int32), cast["prim"])
    np.testing.assert_array_equal(H[:, 2:5], cast["normal"].view(np.uint32))
    np.testing.assert_array_equal(H[:, 5].view(np.int32), cast["flags"])
    np.testing.assert_array_equal(H[:, 6].view(np.int32), cast["material"])
    assert (H[:, 7] == 0).all()
    assert (H[~hit, 0] == np.float32(hrt.RT_T_MISS).view(np.uint32)).all()
    # the survivors are exactly the hits; the rest of index_out is untouched
    c = int(count.cpu()[0])
    idx = index.cpu().numpy()
    assert c == int(hit.sum())
    np.testing.assert_array_equal(np.sort(idx[:c]), np.flatnonzero(hit))
    assert (idx[c:].view(np.uint32) == SENTINEL).all()
    # a miss leaves the path alone bit for bit; a hit moved it; every path asked once; rows past the paths untouched
    for k in ("O", "D", "S", "T"):
        assert (got[k][:n][~hit] == before[k][:n][~hit]).all(), k
    assert (got["O"][:n][hit] != before["O"][:n][hit]).any(axis=1).all()
    assert (got["S"][:n][hit] != before["S"][:n][hit]).any()  # (not all: glass may reflect without a draw)
    assert (got["Q"][:n] == 1).all()
    for k in Paths.NAMES:
        assert (got[k][n:] == SENTINEL).all(), k
    _same({k: v[:n] for k, v in got.items()}, frame["after"], "one step")
    # the scattered state is the one trace() continues from: a second step over the survivors, then the sky, is
    # rt_trace_rays with bounces = 2
    count2 = _ints(p.dev, 1)
    p.step(r, paths=n, index_in=index, count_in=count, count_out=count2, n=n)
    assert 0 < int(count2.cpu()[0]) <= c
    F = torch.float32
    t = frame["d"][:, 1] * 0.5 + 0.5
    u = 1.0 - t
    sky = torch.stack((0.54 * u + 0.54 * t, 0.86 * u + 0.7 * t, 0.92 * u + 0.98 * t), dim=1)
    rad = 0.0 + p.T[:n].view(F) * sky
    r.set_params(bounces=2)
    want, wq = r.trace_rays(frame["o"], frame["d"], rng=frame["s"], want_queries=True)
    np.testing.assert_array_equal(_u32(rad), _u32(want))
    np.testing.assert_array_equal(p.Q[:n].cpu().numpy(), wq.cpu().numpy())
    assert (_u32(p.Q[:n]) == 1 + hit).all()


# ------------------------------------------------------------------------------------------------ compaction
def _albedo(k, n):
    x = (k + 1.0) / (n + 1.0)
    return [0.05 + 0.9 * x, 0.95 - 0.9 * x, 0.1 + 0.8 * ((7 * k + 3) % (n + 1)) / (n + 1.0), 1.0]


def _material(k, n):
    kind = (hrt.LAMBERTIAN, hrt.METAL, hrt.DIELECTRIC)[k % 3]
    return Material._make(_albedo(k, n), [(0.0, 0.1, 1.5)[k % 3]] * 3, kind)


def grid_scene():
    """49 spheres at (1.5 i, 1.5 j, -6), i, j = -3 .. 3, radius 0.4 + 0.01 (k % 7), materials by k % 3 (no ground)."""
    c = [(1.5 * i, 1.5 * j, -6.0) for i in range(-3, 4) for j in range(-3, 4)]
    sp = hrt.spheres_array([Sphere._make(Vec3(*ck), 0.4 + 0.01 * (k % 7), _material(k, len(c))) for k, ck in enumerate(c)])
    cam = Camera.new(Vec3(0.0, 0.0, 2.0), Vec3(0.0, 0.0, -6.0), 8.0, 0.1, 0.9)
    sd = scenes.SceneDef("grid-49", hrt.RT_MODE_SPHERE, 64, 40, cam, sp, frames=1, bounces=10, min_sphere_slots=0)
    return sd, np.array(c, np.float64)


def wave_batch():
    """293 rays from in front of the grid: wave 0 aimed at sphere centres (all 64 hit), wave 1 aimed away from the grid
    (none hits), wave 2 alternating, wave 3 hits except its lanes 0-4, wave 4 (37 lanes, ragged) alternating in threes."""
    _, c = grid_scene()
    n = 4 * 64 + 37
    i = np.arange(n)
    wave, lane = i // 64, i % 64
    aim = np.select([wave == 0, wave == 1, wave == 2, wave == 3], [True, False, lane % 2 == 1, lane >= 5], (lane // 3) % 2 == 0)
    o = np.stack([0.01 * (i % 17) - 0.08, 0.01 * (i % 13) - 0.06, 2.0 + 0.001 * i], axis=1).astype(np.float32)
    d = np.where(aim[:, None], c[i % 49] - o, np.array([0.3, 0.2, 1.0]) + 0.001 * (i % 7)[:, None]).astype(np.float32)
    return o, d, aim


def test_compaction_of_full_empty_and_mixed_waves():
    import torch

    sd, _ = grid_scene()
    r = scenes.make_renderer(sd)
    dev = torch.device("cuda", r.device()[0])
    o, d, aim = wave_batch()
    n = len(o)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    ts = torch.arange(1, n + 1, dtype=torch.int32, device=dev) * 7919
    hit = r.cast_rays(to, td)["prim"].cpu().numpy() >= 0
    np.testing.assert_array_equal(hit, aim)  # (the batch is what it says: a full wave, an empty one, mixed ones)
    assert hit[:64].all() and not hit[64:128].any()
    index, count = _ints(dev, n + 8), _ints(dev, 1)
    p = Paths(to, td, ts).step(r, index_out=index, count_out=count)
    c, idx = int(count.cpu()[0]), index.cpu().numpy()
    assert c == int(hit.sum())
    np.testing.assert_array_equal(np.sort(idx[:c]), np.flatnonzero(hit))
    assert (idx[c:].view(np.uint32) == SENTINEL).all() and len(idx) == n + 8
    for w in range(5):  # the entries of one wave keep their order
        mine = idx[:c][idx[:c] // 64 == w]
        assert (np.diff(mine) > 0).all(), (w, mine)
    assert (_u32(p.Q) == 1).all()
    # count_out without index_out only counts, and changes nothing else
    count2 = _ints(dev, 1)
    q = Paths(to, td, ts).step(r, count_out=count2)
    assert int(count2.cpu()[0]) == c
    _same(q.snap(), p.snap(), "count only")
    # neither: the step alone
    _same(Paths(to, td, ts).step(r).snap(), p.snap(), "no compaction")


# ------------------------------------------------------------------------------------------------ ragged and partial
def _mixed_start(frame, n):
    """Where a batch of n rays starts: 30 rays before the frame's first hit (lane 0 a miss), n rays fitting."""
    return max(0, min(int(np.flatnonzero(frame["hit"])[0]) - 30, frame["n"] - n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_ragged_batches_and_count_in(n, frame):
    """n paths of the frame (from 30 rays before its first hit: misses lead, hits follow), processed up to min(n, *count_in): the
    processed paths end as in the whole frame's step, everything else — the entries past the count, the rows past the
    paths, index_out past the survivors — keeps its bits."""
    r, k0 = frame["r"], _mixed_start(frame, n)
    sl = slice(k0, k0 + n)
    o, d, s = frame["o"][sl], frame["d"][sl], frame["s"][sl]
    hit = frame["hit"][sl]
    after = {k: v[sl] for k, v in frame["after"].items()}
    for cin in (None, 0, 1, 64, n - 1, n, n + 5):
        m = n if cin is None else min(n, cin)
        what = f"{frame['name']} n {n} count_in {cin}"
        p = Paths(o, d, s, extra=8)
        before = p.snap()
        index, count = _ints(p.dev, n + 8), _ints(p.dev, 1)
        kw = {} if cin is None else {"count_in": _ints(p.dev, 1, cin)}
        p.step(r, paths=n, index_out=index, count_out=count, **kw)
        processed = np.arange(n + 8) < m
        want = _expect(before, {k: np.concatenate([v, before[k][n:]]) for k, v in after.items()}, processed)
        _same(p.snap(), want, what)
        c, idx = int(count.cpu()[0]), index.cpu().numpy()
        assert c == int(hit[:m].sum()), what
        np.testing.assert_array_equal(np.sort(idx[:c]), np.flatnonzero(hit[:m]), err_msg=what)
        assert (idx[c:].view(np.uint32) == SENTINEL).all(), what


def test_inactive_leading_lanes(frame):
    """Lanes 0-9 of every wave hold an index at or above `paths` (the tensors have rows there, so nothing can go out of
    bounds): those entries are skipped, their rows keep their bits, and the wave's leader is found among the live lanes —
    the survivors and the count are exact."""
    import torch

    r, n = frame["r"], 1024
    k0 = _mixed_start(frame, n)
    sl = slice(k0, k0 + n)
    hit = frame["hit"][sl]
    after = {k: v[sl] for k, v in frame["after"].items()}
    p = Paths(frame["o"][sl], frame["d"][sl], frame["s"][sl], extra=64)
    before = p.snap()
    i = np.arange(n)
    dead = i % 64 < 10
    index_in = np.where(dead, n + i % 64, i).astype(np.int32)
    index_in[5] = -1  # (0xFFFFFFFF: the largest u32, skipped as well)
    index, count = _ints(p.dev, n + 8), _ints(p.dev, 1)
    p.step(r, paths=n, index_in=torch.from_numpy(index_in).to(p.dev), index_out=index, count_out=count)
    processed = np.concatenate([~dead, np.zeros(64, bool)])
    want = _expect(before, {k: np.concatenate([v, before[k][n:]]) for k, v in after.items()}, processed)
    _same(p.snap(), want, "inactive lanes")
    c, idx = int(count.cpu()[0]), index.cpu().numpy()
    assert c == int((hit & ~dead).sum()) and 0 < c < n
    np.testing.assert_array_equal(np.sort(idx[:c]), np.flatnonzero(hit & ~dead))
    assert (idx[c:].view(np.uint32) == SENTINEL).all()
    # a wave whose only live lanes miss, and one with no live lane at all, forward nothing and count nothing
    n = frame["n"]
    miss = np.flatnonzero(~frame["hit"])[:54]  # (the whole frame's misses: up to 54 of them in lanes 10 and up)
    assert len(miss) > 0
    index_in = np.full(128, n + 1)
    index_in[:10] = n + 3
    index_in[10:10 + len(miss)] = miss
    p2 = Paths(frame["o"], frame["d"], frame["s"], extra=64)
    before = p2.snap()
    index, count = _ints(p2.dev, 128 + 8), _ints(p2.dev, 1)
    p2.step(r, paths=n, index_in=torch.from_numpy(index_in.astype(np.int32)).to(p2.dev), index_out=index, count_out=count)
    assert int(count.cpu()[0]) == 0 and (_u32(index) == SENTINEL).all()
    processed = np.zeros(n + 64, bool)
    processed[miss] = True
    after = {k: np.concatenate([v, before[k][n:]]) for k, v in frame["after"].items()}
    _same(p2.snap(), _expect(before, after, processed), "missing waves")


# ------------------------------------------------------------------------------------------------ indirection
def test_a_permutation_as_index_in(frame):
    import torch

    r, n = frame["r"], frame["n"]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(20261020)).to(torch.int32)
    p = Paths(frame["o"], frame["d"], frame["s"])
    index, count = _ints(p.dev, n), _ints(p.dev, 1)
    p.step(r, index_in=perm.to(p.dev), index_out=index, count_out=count)
    _same(p.snap(), frame["after"], "permuted")
    c = int(count.cpu()[0])
    np.testing.assert_array_equal(np.sort(index.cpu().numpy()[:c]), np.flatnonzero(frame["hit"]))
    # survivors in the order the permutation presented them, wave by wave
    pn, idx = perm.numpy(), index.cpu().numpy()[:c]
    pos = np.empty(n, np.int64)
    pos[pn] = np.arange(n)
    for w in range((n + 63) // 64):
        mine = pos[idx][pos[idx] // 64 == w]
        assert (np.diff(mine) > 0).all(), w


@pytest.mark.parametrize("case", ["complex_scene", "c4"])
def test_chaining_by_hand_is_count_in_chaining(case):
    """The survivors handed on with the count read back on the host (n = count, index_in = the survivors) against
    trace_wavefront's loop (every step launched for the first n, the count read on the device)."""
    import torch

    build, own, _ = CASES[case]
    w, h = SHAPES[0]
    r = scenes.make_renderer(build(w, h))
    o, d, s = _frame_state(r, 1010)
    n, F = w * h, torch.float32
    want, wq = r.trace_wavefront(o, d, s, own, want_queries=True)
    p = Paths(o, d, s)
    index, count = None, n
    counts = []
    for _ in range(own):
        if count == 0:
            break
        out, cnt = _ints(p.dev, count), _ints(p.dev, 1)
        p.step(r, index_in=index, index_out=out, count_out=cnt)
        count = int(cnt.cpu()[0])
        index = out[:count].contiguous()
        counts.append(count)
    assert counts[0] > 0 and all(a >= b for a, b in zip(counts, counts[1:])), counts
    t = d[:, 1] * 0.5 + 0.5
    u = 1.0 - t
    sky = torch.stack((0.54 * u + 0.54 * t, 0.86 * u + 0.7 * t, 0.92 * u + 0.98 * t), dim=1)
    np.testing.assert_array_equal(_u32(0.0 + p.T.view(F) * sky), _u32(want))
    np.testing.assert_array_equal(_u32(p.Q), _u32(wq))


# ------------------------------------------------------------------------------------------------ optional buffers
@pytest.mark.parametrize("without", ["throughput", "queries", "hits"])
def test_optional_buffers(without, frame):
    r, n = frame["r"], frame["n"]
    p = Paths(frame["o"], frame["d"], frame["s"])
    before = p.snap()
    index, count = _ints(p.dev, n), _ints(p.dev, 1)
    p.step(r, index_out=index, count_out=count, **{without: False})
    got = p.snap()
    left = {"throughput": "T", "queries": "Q", "hits": "H"}[without]
    assert (got[left] == before[left]).all()
    _same(got, frame["after"], f"without {without}", [k for k in Paths.NAMES if k != left])
    c = int(count.cpu()[0])
    np.testing.assert_array_equal(np.sort(index.cpu().numpy()[:c]), np.flatnonzero(frame["hit"]))


# ------------------------------------------------------------------------------------------------ isolation
def test_bounce_rays_leaves_the_draw_state_alone():
    sd = scenes.config_c3(64, 40, 6)
    ref, q = scenes.oracle_render(sd)

    def three(r, t0):
        r.draw_frames(3, t0, 10)
        return r.stats().queries

    r, plain = scenes.make_renderer(sd), scenes.make_renderer(sd)
    for x in (r, plain):
        x.set_params(schedule=hrt.RT_SCHEDULE_QUEUE)
    q3 = three(r, 1000)
    assert three(plain, 1000) == q3

    def snapshot():
        st = r.stats()
        return r.read_image().tobytes(), bytes(st), tuple(r.raw_counters()), r.frame_count, st.ordered_launches

    before = snapshot()
    o, d, s = _frame_state(r, 1030)
    p = Paths(o, d, s)
    index, count = _ints(p.dev, p.n), _ints(p.dev, 1)
    p.step(r, index_out=index, count_out=count)
    assert 0 < int(count.cpu()[0]) < p.n
    _, wq = r.trace_wavefront(o, d, s, 50, want_queries=True)
    assert int(wq.max()) > 1
    assert snapshot() == before
    q6 = three(r, 1030)
    three(plain, 1030)
    np.testing.assert_array_equal(r.read_image().view(np.uint32), plain.read_image().view(np.uint32))
    np.testing.assert_array_equal(r.read_image().view(np.uint32), ref.view(np.uint32))
    assert r.stats().queries == plain.stats().queries == q6
    assert q3 + q6 == q and r.frame_count == 6
    assert r.stats().ordered_launches == plain.stats().ordered_launches


def test_partition_rows_are_the_full_frames_rows():
    from hrt.parallel import owned_rows

    w, h = SHAPES[0]
    for sd in (_golden("complex_scene")(w, h), suzane_scene(w, h)):
        full = scenes.make_renderer(sd)
        fimg, fq = full.trace_wavefront(*_frame_state(full, 1010), sd.bounces, want_queries=True)
        part = scenes.make_renderer(sd)
        part.set_params(row0=1, row_step=3, row_block=2)
        rows = owned_rows(1, 3, h, 2)
        pimg, pq = part.trace_wavefront(*_frame_state(part, 1010), sd.bounces, want_queries=True)
        assert tuple(pimg.shape) == (len(rows) * w, 3)
        np.testing.assert_array_equal(_u32(pimg).reshape(len(rows), w, 3), _u32(fimg).reshape(h, w, 3)[rows])
        np.testing.assert_array_equal(_u32(pq).reshape(len(rows), w), _u32(fq).reshape(h, w)[rows])


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    import torch

    L = hrt.lib()
    E = hrt._lib
    r = hrt.Renderer(16, 8, hrt.RT_MODE_SPHERE)  # (no camera, no spheres: 100 zero slots; the step needs neither)
    dev = torch.device("cuda", r.device()[0])
    buf = torch.zeros((4096,), dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    buf[2048:2064] = torch.arange(16, dtype=torch.int32, device=dev)  # index_in: distinct paths (8 and up are skipped)
    buf[2304] = 16  # count_in
    torch.cuda.synchronize(dev)
    state = dict(origins_dev=p, dirs_dev=p + 1024, rng_dev=p + 2048, throughput_dev=p + 3072, queries_dev=p + 4096,
                 hits_dev=p + 5120, index_in_dev=p + 8192, count_in_dev=p + 9216, index_out_dev=p + 10240,
                 count_out_dev=p + 11264, paths=8, reserved=0)

    def call(n=8, **change):
        io = E.RtBounce(**{**state, **change})
        rc = L.rt_bounce_rays(r._h, C.byref(io), n)
        if rc:
            assert b"rt_bounce_rays" in L.rt_last_error()
        return rc

    assert call() == E.RT_OK
    assert L.rt_bounce_rays(r._h, None, 0) == E.RT_OK  # n = 0: nothing is looked at
    assert L.rt_bounce_rays(r._h, None, 8) == E.RT_ERR_ARG
    for name in ("origins_dev", "dirs_dev", "rng_dev"):
        assert call(**{name: None}) == E.RT_ERR_ARG, name
    for name in ("throughput_dev", "queries_dev", "hits_dev", "index_in_dev", "count_in_dev"):
        assert call(**{name: None}) == E.RT_OK, name
    assert call(index_out_dev=None) == E.RT_OK
    assert call(index_out_dev=None, count_out_dev=None) == E.RT_OK
    assert call(count_out_dev=None) == E.RT_ERR_ARG  # index_out without count_out
    assert call(n=9, index_in_dev=None) == E.RT_ERR_ARG  # n > paths without index_in
    assert call(n=9) == E.RT_OK  # (with index_in, n may exceed paths)
    assert call(reserved=1) == E.RT_ERR_ARG
    assert call(count_out_dev=state["count_in_dev"]) == E.RT_ERR_ARG
    for name in [k for k in state if k.endswith("_dev")]:
        assert call(**{name: state[name] + 2}) == E.RT_ERR_ARG, name
    assert call(hits_dev=state["hits_dev"] + 8) == E.RT_ERR_ARG  # 16-byte aligned
    assert call(origins_dev=p + 4, dirs_dev=p + 1028) == E.RT_OK
    r.synchronize()
    # the Python layer: tensors on the renderer's device, used in place
    z3 = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    zs = torch.zeros((4,), dtype=torch.int32, device=dev)
    one = torch.zeros((1,), dtype=torch.int32, device=dev)
    r.bounce_rays(z3, z3.clone(), zs)
    with pytest.raises(ValueError):
        r.bounce_rays(np.zeros((4, 3), np.float32), z3, zs)  # numpy: not in place
    with pytest.raises(ValueError):
        r.bounce_rays(z3, torch.zeros((5, 3), dtype=torch.float32, device=dev), zs)
    with pytest.raises(ValueError):
        r.bounce_rays(z3, z3, zs.to(torch.float32))
    with pytest.raises(ValueError):
        r.bounce_rays(z3.cpu(), z3.cpu(), zs.cpu())
    with pytest.raises(ValueError):
        r.bounce_rays(z3, z3, zs, throughput=torch.zeros((4, 4), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        r.bounce_rays(z3, z3, zs, hits=torch.zeros((4, 4), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        r.bounce_rays(z3, z3, zs, index_out=torch.zeros((3,), dtype=torch.int32, device=dev), count_out=one)
    with pytest.raises(ValueError):
        r.bounce_rays(torch.zeros((8, 3), dtype=torch.float32, device=dev)[::2], z3, zs)  # not contiguous
    with pytest.raises(hrt.RtError) as e:
        r.bounce_rays(z3, z3.clone(), zs, index_out=zs.clone())  # index_out without count_out
    assert e.value.code == E.RT_ERR_ARG
    with pytest.raises(ValueError):
        r.trace_wavefront(z3, z3, zs.to(torch.float32), 2)
    assert tuple(r.trace_wavefront(z3, z3, zs, 2).shape) == (4, 3)
