"""rt_cast_rays, rt_occluded, rt_trace_rays, rt_bounce_rays, rt_primary_rays and rt_primary_rng against the CPU oracle's
per-ray entry points (oracle_cast_rays, oracle_trace_rays, oracle_bounce_step, oracle_primary_rays), on the rays of
ray_sets.py: axis-parallel, on the surface, inside, of every length, far away, grazing, non-finite and plain, 4099 per
scene, in an interleaved and in a blocked layout. include/hrt.h promises "exactly what one bounce of trace() would see for
that ray"; here that is checked for rays no camera makes.

Comparison rule, everywhere: uint32 views; a NaN equals a NaN whatever its sign or payload ((p - c) / 0 on a padding slot
makes them); nothing else has a tolerance and no ray is left out. The walks that are not the reference's (tri_bvh = 1 and
the device trees) are held to oracle_cast_rays(flat=True): t by bits, a miss a miss, and prim one of the triangles whose
flat t has the winner's bits, with n, flags and material those of the reported prim.

Figures (test_oracle_rays.py prints them from the oracle alone; 4099 rays per scene, share of hits in classes a .. h):
  grid          53.4 77.7 74.3 65.5 59.7 69.0  0.0 65.9      grid-100: f 77.1, 62 rays hit a padding slot
  coincident    52.4 77.9 73.7 66.7 66.0 71.3  0.0 66.9
  rtiow         53.2 80.6 74.1 56.6 56.7 84.6  0.0 60.6
  cube          41.3 67.6 78.1 19.7 38.1 64.6 22.3 51.9
  suzane        65.4 79.1 84.8 25.0 42.5 74.9 40.3 66.5      92 walks cut by the 600-step cap
  dragon        66.2 80.4 82.4 26.4 42.9 76.5 36.4 66.5      347 walks cut by the cap
  mixed-simple  67.0 84.6 75.1 47.3 64.4 85.6 34.2 71.3      70 cut;  mixed-defer 53 cut;  mixed-bvh 48 cut
  heap1 .. 3    a 42-44, b 55-64, c 57-68, d 62-65, e 64-65, f 55-58, g 17-57, h 63-65
Measured on an MI355X (the figures the other-walk tests print): on the 3,675 rays with finite components every walk agrees
with the flat test on every record, and every record is the lowest index of its tie; triangle hits with more than one
triangle at the winner's t: cube 0.90 % of 1,884, Suzanne 0.27 % of 2,211 (host SAH, LBVH and PLOC trees alike),
mixed-simple 0.28 % of 2,114, mixed-defer 0.45 % of 1,120, mixed-bvh 0.55 % of 1,095, the planar sheet 5.80 % of 931.
On the 424 rays with a NaN or infinite component the flat test reports t = NaN for 379 (cube), 424 (Suzanne), 422 - 423
(mixed) and 326 (planar) rays; the walks missed all of those before walk_sah answered non-finite rays by the reference's rule.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import closest_util
import hrt
import lbvh_util
import ray_sets
import scenes
import test_gpu_cast_rays as cast
from hrt.parallel import local_rows

pytestmark = pytest.mark.gpu

LAYOUTS = ("interleaved", "blocked")
SENTINEL = 0x5A5A5A5A
FLOAT_WORDS = np.array([True, False, True, True, True, False, False, False])  # of the 8 words of an rt_hit


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


# ------------------------------------------------------------------------------------------------ configurations
# name -> (ray-set scene, rt_params, triangles only): the parity paths, whose definition the oracle is
PARITY = {}
for _v in (1, 3, 4):
    for _slots, _scene in ((0, "grid"), (100, "grid-100")):
        PARITY[f"sphere-v{_v}-slots{_slots}"] = (_scene, dict(variant=_v), False)
    PARITY[f"coincident-v{_v}"] = ("coincident", dict(variant=_v), False)
for _name in ("cube", "suzane", "mixed-simple", "mixed-defer", "mixed-bvh"):
    PARITY[f"{_name}-tribvh0"] = (_name, dict(tri_bvh=0), False)
PARITY["dragon-capped"] = ("dragon", dict(tri_bvh=0), False)
PARITY["rtiow-484"] = ("rtiow", {}, False)
for _k in (1, 2, 3):
    PARITY[f"heap{_k}-mixed"] = (f"heap{_k}", dict(tri_bvh=0), False)
    PARITY[f"heap{_k}-tris"] = (f"heap{_k}", dict(tri_bvh=0), True)  # the same rays, the triangles alone


@functools.lru_cache(maxsize=None)
def _scene(scene, tris_only=False):
    sd, rays = ray_sets.scene_and_rays(scene)
    if tris_only:
        sd = dataclasses.replace(sd, mode=hrt.RT_MODE_TRIS, spheres=None)
    return sd, rays


def _layout(rays, layout):
    if layout == "interleaved":
        o, d, _ = rays.interleaved()
    else:
        o, d, _, _ = rays.blocked()
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _renderer(name):
    scene, params, tris_only = PARITY[name]
    sd, rays = _scene(scene, tris_only)
    r = scenes.make_renderer(sd)
    r.set_params(**params)
    return sd, rays, r


@functools.lru_cache(maxsize=None)
def _oracle_cast(scene, tris_only, layout):
    """The oracle's records of a scene's rays, once per module; read only."""
    sd, rays = _scene(scene, tris_only)
    o, d = _layout(rays, layout)
    rec, _ = scenes.oracle_cast_rays(sd, o, d, step_cap=ray_sets.STEP_CAP)
    rec.flags.writeable = False
    return rec


def _states(n, seed=7):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ comparison
def _is_nan(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def _differs(a, b, is_float=True):
    """Elementwise on the uint32 views: different bits, unless both are NaNs. is_float: True, False, or a mask of the
    words that hold floats."""
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    assert ua.shape == ub.shape, (ua.shape, ub.shape)
    return (ua != ub) & ~(_is_nan(ua) & _is_nan(ub) & is_float)


def _words(rec):
    """HIT_DTYPE records (or an (n, 8) int32 buffer) as (n, 8) uint32."""
    return np.frombuffer(np.ascontiguousarray(rec).tobytes(), dtype=np.uint32).reshape(-1, 8)


def _record_differs(got, want):
    return _differs(_words(got), _words(want), FLOAT_WORDS[None, :]).any(axis=1)


def _assert_records(got, want, what):
    bad = _record_differs(got, want)
    if bad.any():
        g, w = _words(got), _words(want)
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {len(g)} records differ; first at {i}: device {g[i].tolist()} "
                    f"(t {g[i, :1].view(np.float32)[0]!r}), oracle {w[i].tolist()} (t {w[i, :1].view(np.float32)[0]!r})")


def _assert_same(got, want, what, is_float=True):
    bad = _differs(got, want, is_float)
    if bad.any():
        rows = np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1))
        i = int(rows[0])
        pytest.fail(f"{what}: {len(rows)} of {len(bad)} rows differ; first at {i}: device {np.asarray(got)[i]!r}, "
                    f"oracle {np.asarray(want)[i]!r}")


def _cast_raw(r, o, d):
    """rt_cast_rays through the C ABI into a buffer of sentinels with one record to spare: all 8 words of n records."""
    import torch

    dev = r._torch_device()
    n = len(o)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hits = torch.full((n + 1, 8), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = hrt.lib().rt_cast_rays(r._h, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), n, C.c_void_p(hits.data_ptr()))
    assert rc == 0, hrt.lib().rt_last_error()
    r.synchronize()
    got = hits.cpu().numpy()
    assert (got[n] == SENTINEL).all()
    return got[:n]


# ------------------------------------------------------------------------------------------------ the parity paths
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(PARITY))
def test_cast_rays_records_are_the_oracles(name, layout):
    sd, rays, r = _renderer(name)
    o, d = _layout(rays, layout)
    want = _oracle_cast(*PARITY[name][::2], layout)
    _assert_records(_cast_raw(r, o, d), want, f"{name} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(PARITY))
def test_occluded_is_the_oracles_hit_before_tmax(name, layout):
    """tmax mixes NaN, 0, -0, negative, +inf, FLT_MAX, exactly the oracle's t (not occluded), the next f32 above it
    (occluded), fractions and multiples of it and a tiny value."""
    sd, rays, r = _renderer(name)
    o, d = _layout(rays, layout)
    rec = _oracle_cast(*PARITY[name][::2], layout)
    tmax = closest_util.cap_mix(rec["t"], 20261021)
    with np.errstate(invalid="ignore"):
        want = (rec["prim"] >= 0) & (rec["t"] < tmax)
        any_hit = (rec["prim"] >= 0) & (rec["t"] < np.float32(hrt.RT_T_MISS))
    exact = (tmax.view(np.uint32) == rec["t"].view(np.uint32)) & (rec["prim"] >= 0)
    assert exact.sum() > 50 and not want[exact].any() and want.any()
    got = r.occluded(o, d, tmax).cpu().numpy()
    bad = got != want
    assert not bad.any(), (name, layout, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    got = r.occluded(o, d).cpu().numpy()
    bad = got != any_hit
    assert not bad.any(), (name, layout, "no tmax", int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(PARITY))
def test_trace_rays_is_the_oracles_trace(name, layout):
    """The scene's own bounce cap (10 sphere, 5 triangle and mixed); given states, then NULL with seeds 1 and 0x9E3779B9."""
    sd, rays, r = _renderer(name)
    o, d = _layout(rays, layout)
    for rng, seed in ((_states(len(o)), 0), (None, 1), (None, 0x9E3779B9)):
        what = f"{name} {layout} " + ("given states" if rng is not None else f"seed {seed:#x}")
        rad, q, _ = scenes.oracle_trace_rays(sd, o, d, rng=rng, seed=seed, step_cap=ray_sets.STEP_CAP)
        got, gq = r.trace_rays(o, d, rng=rng, seed=seed, want_queries=True)
        _assert_same(got.cpu().numpy(), rad, what + " radiance")
        _assert_same(gq.cpu().numpy(), q, what + " queries", is_float=False)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(PARITY))
def test_three_bounce_steps_are_the_oracles(name, layout):
    """Three chained rt_bounce_rays steps through two (index, count) pairs against three oracle_bounce_step calls on the
    surviving paths: origins, dirs, rng, throughput, queries, the hit records of the processed paths (the others keep
    their sentinel) and the forwarded indices as sets."""
    import torch

    sd, rays, r = _renderer(name)
    o, d = _layout(rays, layout)
    n = len(o)
    dev = r._torch_device()
    co, cd, cs, ct = o.copy(), d.copy(), _states(n, 11), np.ones_like(o)
    cq = np.zeros(n, np.uint32)
    O, D = torch.from_numpy(co.copy()).to(dev), torch.from_numpy(cd.copy()).to(dev)
    S = torch.from_numpy(cs.view(np.int32).copy()).to(dev)
    T = torch.ones((n, 3), dtype=torch.float32, device=dev)
    Q = torch.zeros((n,), dtype=torch.int32, device=dev)
    H = torch.empty((n, 8), dtype=torch.int32, device=dev)
    idx = [torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    cnt = [torch.zeros((1,), dtype=torch.int32, device=dev) for _ in range(2)]
    live = np.arange(n)
    for step in range(3):
        what = f"{name} {layout} step {step + 1}"
        H.fill_(SENTINEL)
        kw = dict(index_in=idx[(step - 1) % 2], count_in=cnt[(step - 1) % 2]) if step else {}
        r.bounce_rays(O, D, S, throughput=T, queries=Q, hits=H, index_out=idx[step % 2], count_out=cnt[step % 2], **kw)
        no, nd, ns, nt, rec, hit = scenes.oracle_bounce_step(sd, co[live], cd[live], cs[live], ct[live],
                                                             step_cap=ray_sets.STEP_CAP)
        co[live], cd[live], cs[live], ct[live] = no, nd, ns, nt
        cq[live] += 1
        h = H.cpu().numpy()
        _assert_records(h[live], rec, what + " hit records")
        untouched = np.ones(n, bool)
        untouched[live] = False
        assert (h[untouched] == SENTINEL).all(), what
        _assert_same(O.cpu().numpy(), co, what + " origins")
        _assert_same(D.cpu().numpy(), cd, what + " dirs")
        _assert_same(T.cpu().numpy(), ct, what + " throughput")
        _assert_same(S.cpu().numpy(), cs, what + " rng", is_float=False)
        _assert_same(Q.cpu().numpy(), cq, what + " queries", is_float=False)
        count = int(cnt[step % 2].item())
        forwarded = np.sort(idx[step % 2].cpu().numpy()[:count])
        live = live[hit]
        assert count == len(live) and np.array_equal(forwarded, live), (what, count, len(live))
        assert step or len(live) > n // 20, what  # (a twentieth of the paths at least go on)


# ------------------------------------------------------------------------------------------------ primary rays
PRIMARY_SCENES = {"grid": cast.grid_scene, "suzane": cast.suzane_scene, "mixed": lambda w, h: cast.mixed_scene(w, h, 12)}
PRIMARY_TIMES = (0, 1, 1000, 0x7FFFFFFF, 0xFFFFFFFF)


@pytest.mark.parametrize("name", sorted(PRIMARY_SCENES))
def test_primary_rays_and_states_are_the_oracles(name):
    """The seed (x * H + y) * time wraps in u32; the whole image, and the blocked row share of rank 1 of 3."""
    for w, h in ((70, 45), (33, 17)):
        sd = PRIMARY_SCENES[name](w, h)
        for rows in (None, (1, 3, local_rows(1, 3, h, 2), 2)):
            r = scenes.make_renderer(sd)
            if rows is not None:
                r.set_params(row0=rows[0], row_step=rows[1], row_block=rows[3])
                assert r.local_rows == rows[2]
            for time in PRIMARY_TIMES:
                what = f"{name} {w}x{h} rows {rows} time {time:#x}"
                wo, wd, ws = scenes.oracle_primary_rays(sd, time, rows=rows)
                go, gd = (x.cpu().numpy() for x in r.primary_rays(time))
                gs = r.primary_rng(time).cpu().numpy()
                assert go.shape == wo.shape and gs.shape == ws.shape, what
                _assert_same(go.reshape(-1, 3), wo.reshape(-1, 3), what + " origins")
                _assert_same(gd.reshape(-1, 3), wd.reshape(-1, 3), what + " dirs")
                _assert_same(gs.reshape(-1), ws.reshape(-1), what + " rng", is_float=False)


# ------------------------------------------------------------------------------------------------ the other walks
def _planar_scene():
    tris = lbvh_util.planar_triangles()
    mats = np.array([hrt.Material.new_lambertian(hrt.Vec3(0.5, 0.5, 0.5))], dtype=hrt.MATERIAL_DTYPE).reshape(-1)
    nodes = np.zeros(1, dtype=hrt.NODE_DTYPE)
    cam = cast.grid_scene(8, 8).camera
    return scenes.SceneDef("planar", hrt.RT_MODE_TRIS, 64, 40, cam, bvh=((1, len(tris)), nodes, tris, mats))


@functools.lru_cache(maxsize=None)
def _other_scene(scene):
    """(SceneDef, RaySet): a ray-set scene, or the planar sheet with rays made for it by the same generator (it has no
    heap, and rays that start on its one plane cannot hit it again, so it is not among ray_sets.SCENES)."""
    if scene != "planar":
        return ray_sets.scene_and_rays(scene)
    sd = _planar_scene()

    def first_hit(o, d):
        rec, _ = scenes.oracle_cast_rays(sd, o, d, flat=True)
        t = rec["t"].astype(np.float64)[:, None]
        return rec["prim"] >= 0, (o + t * d).astype(np.float32), d  # (seed origins only: any point near the sheet will do)

    return sd, ray_sets.make_rays(None, sd.bvh[2], None, first_hit)


OTHER = {f"{s}-tribvh1": (s, "sah") for s in ("cube", "suzane", "mixed-simple", "mixed-defer", "mixed-bvh")}
for _s in ("suzane", "planar"):
    OTHER[f"{_s}-lbvh"] = (_s, 0)
    OTHER[f"{_s}-ploc"] = (_s, 1)


def _other_renderer(sd, how):
    if how == "sah":
        r = scenes.make_renderer(sd)
        r.set_params(tri_bvh=1)
        return r
    from test_gpu_lbvh import device_renderer, on_device

    r = device_renderer(sd)
    if how == 1:
        r.set_triangles_device(on_device(r, sd.bvh[2]), sd.bvh[3], builder=1)
    return r


def _check_other_walk(name, layout, finite):
    """The rays of the set with only finite components (finite) or the others, cast by the walk and held to the flat test.
    The flat test in index order keeps the lowest index among triangles of equal t and in reverse order the highest, so a
    device record equal to either is in the tie set; any other is checked against the flat test of the one triangle it
    names. Prints the share of triangle hits with more than one triangle at the winner's t."""
    scene, how = OTHER[name]
    sd, rays = _other_scene(scene)
    o, d = _layout(rays, layout)
    sel = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    sel = np.flatnonzero(sel if finite else ~sel)
    got = _cast_raw(_other_renderer(sd, how), o, d)[sel]  # (the whole set in one launch, as a caller would)
    o, d = np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])
    sizes, nodes, tris, mats = sd.bvh
    m = len(tris)
    fwd, _ = scenes.oracle_cast_rays(sd, o, d, flat=True)
    rsd = dataclasses.replace(sd, bvh=(sizes, nodes, np.ascontiguousarray(tris[::-1]), mats))
    rev, _ = scenes.oracle_cast_rays(rsd, o, d, flat=True)
    rtri = (rev["prim"] >= 0) & ((rev["flags"] & hrt.RT_HIT_TRIANGLE) != 0)
    rev["prim"][rtri] = m - 1 - rev["prim"][rtri]
    g, f = _words(got), _words(fwd)
    what = f"{name} {layout} {'finite' if finite else 'non-finite'} rays"
    thit = (fwd["prim"] >= 0) & ((fwd["flags"] & hrt.RT_HIT_TRIANGLE) != 0)
    ties = thit & (fwd["prim"] != rev["prim"])
    bad_t = _differs(g[:, 0], f[:, 0])
    bad_miss = (g[:, 1].view(np.int32) < 0) != (fwd["prim"] < 0)
    rest = np.flatnonzero(_record_differs(got, fwd) & _record_differs(got, rev) & ~bad_t & ~bad_miss)
    print(f"{what}: {len(sel)} rays, {int(thit.sum())} triangle hits of the flat test ({int(np.isnan(fwd['t']).sum())} with "
          f"t = NaN), {100.0 * ties.sum() / max(int(thit.sum()), 1):.2f} % with more than one triangle at the winner's t; "
          f"t differs on {int(bad_t.sum())}, hit or miss on {int(bad_miss.sum())}, {len(rest)} records are neither end of "
          f"their tie")
    assert not bad_t.any(), (what, "t", int(bad_t.sum()), sel[bad_t][:8].tolist())
    assert not bad_miss.any(), (what, "hit or miss", int(bad_miss.sum()), sel[bad_miss][:8].tolist())
    for i in rest:  # neither the lowest nor the highest index of a tie: the triangle the record names, alone
        p = int(g[i, 1].view(np.int32))
        assert (g[i, 5] & hrt.RT_HIT_TRIANGLE) and 0 <= p < m, (what, int(sel[i]), g[i].tolist())
        one = dataclasses.replace(sd, mode=hrt.RT_MODE_TRIS, spheres=None, bvh=((1, 1), nodes[:1], tris[p:p + 1], mats))
        rec, _ = scenes.oracle_cast_rays(one, o[i:i + 1], d[i:i + 1], flat=True)
        rec["prim"][rec["prim"] >= 0] = p
        _assert_records(got[i:i + 1], rec, f"{what} ray {int(sel[i])} against triangle {p} alone")
    return int(thit.sum())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(OTHER))
def test_other_walks_find_what_the_flat_test_finds(name, layout):
    """Every ray of the set whose six components are finite (3,675 of 4,099: all but class g's non-finite ones)."""
    assert _check_other_walk(name, layout, finite=True) > 400


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(OTHER))
def test_other_walks_on_non_finite_rays(name, layout):
    """The rays with a NaN or an infinite component, by the same rule: the flat test keeps the reference's
    `t < EPSILON || t >= hit.t` rejection, which accepts a NaN t, so it reports a hit with t = NaN for most of these rays
    (379 to 424 of 424 on the meshes, 326 on the planar sheet), and the last such triangle in index order is the record's."""
    _check_other_walk(name, layout, finite=False)
