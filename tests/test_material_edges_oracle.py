"""The CPU side of test_gpu_material_edges.py: what the oracle gives for the edge materials of material_edges_util.py, pinned
so that the GPU tests cannot pass while testing nothing.

Coverage: in every scene every table entry is the first hit of at least 16 primary rays at time 1000. The default arm: a
kind outside 1 .. 3 shades as kind 3 with the same param (shader_sphere.wgsl:199-215 and shader_tris.wgsl:249-265 are copies
of the dielectric arms at :183-198 and :233-248), also where its low bits spell 1 or 2. Finiteness: a NaN secondary ray
misses everything and the sample ends as att * sky(primary), so kind, index of refraction, fuzz and radius alone leave every
channel finite and the GPU tests compare plain bits there; only albedo makes a pixel non-finite.

Figures of the scenes as committed (8 frames; share of channels NaN / +inf / -inf):
                      sphere_bvh        deep              sphere_few        tris              mixed
  albedo_finite       0.28 4.29 0.02    0.23 3.94 0       0.10 0.43 0.03    0.55 3.14 0.19    1.40 7.96 0.34
  albedo_nonfinite    12.2 9.74 5.40    11.2 8.96 4.58    11.1 8.82 4.50    20.6 13.7 19.5    24.4 14.9 17.2
  all                 2.11 2.08 0.79    2.23 2.19 0.92    0 0 0             6.71 4.21 1.72    13.1 12.6 3.71
Fewest primary rays on a table entry: sphere_bvh and deep 35 (kinds, ior), 47 (fuzz, albedo_finite), 79 (albedo_nonfinite),
42 (all); sphere_few 79 (330 in all); tris 33, 36, 33, 32, 76 and 31 (all); mixed 45 on a sphere (426 in all) and 19, 22, 27,
24, 57 and 19 (all) on a triangle material; the far wall 307.
"""
import numpy as np
import pytest

import hrt
import scenes
import material_edges_util as M
from hrt import Material, Sphere, Vec3

SCENES = [(b, t) for b in M.BUILDERS for t in M.TABLE_NAMES + ["all"]] + [("mixed-1", "all"), ("mixed-60", "all")]
PROGRAM_BUILDERS = ["sphere_bvh", "deep", "sphere_few", "tris", "mixed"]  # all three programs


def _scene_args(builder):
    if builder.startswith("mixed-"):
        return "mixed", dict(slots=int(builder[6:]))
    return builder, {}


@pytest.mark.parametrize("builder, table", SCENES + [("far_wall", "all")], ids=lambda x: str(x))
def test_every_table_entry_is_the_first_hit_of_16_primary_rays(builder, table):
    b, kw = _scene_args(builder)
    slots, mats = M.first_hit_counts(b, table, **kw)
    want_slots, want_mats = M.table_slots(b, table)
    if kw.get("slots") == 1:
        want_slots = []  # (only the ground is left)
    low = {i: slots.get(i, 0) for i in want_slots if slots.get(i, 0) < M.MIN_HITS}
    assert not low, f"{builder}({table}): sphere slots with fewer than {M.MIN_HITS} primary rays: {low}"
    low = {i: mats.get(i, 0) for i in want_mats if mats.get(i, 0) < M.MIN_HITS}
    assert not low, f"{builder}({table}): triangle materials with fewer than {M.MIN_HITS} primary rays: {low}"
    print(f"{builder}({table}): fewest rays on a slot {min([slots[i] for i in want_slots], default=None)}, "
          f"on a triangle material {min([mats[i] for i in want_mats], default=None)}")


def test_scene_sizes_select_the_scans():
    """64 slots or more for the culling BVH, more than 192 nodes' worth for the deep tree, 12 slots for the deferred scan,
    1 for the simple one, 60 for the mixed program's BVH; mixed holds the reversed table."""
    for t in M.TABLE_NAMES + ["all"]:
        assert len(M.scene("sphere_bvh", t).spheres) >= 64
        assert len(M.scene("deep", t).spheres) > 900
        n = min(len(M.TABLES[t]), M.FEW)
        assert len(M.scene("sphere_few", t).spheres) == n + 1
        mx = M.scene("mixed", t)
        assert len(mx.spheres) == M.FEW + 1  # (a table of 9 is filled up with ordinary spheres)
        assert mx.spheres["material"][:n].tobytes() == M.TABLES[t][::-1][:n].tobytes()
        assert mx.bvh[3].tobytes() == M.TABLES[t].tobytes()
        sizes, nodes, tris, _ = scenes.suzanne_tree().view()
        assert tuple(mx.bvh[0]) == tuple(sizes) and mx.bvh[1].tobytes() == nodes.tobytes()
        assert (mx.bvh[2]["material"] == np.arange(len(tris)) % len(M.TABLES[t])).all()
        for f in ("a", "b", "c", "custom"):
            assert mx.bvh[2][f].tobytes() == tris[f].tobytes()
    assert len(M.scene("mixed", "all", slots=1).spheres) == 1 and len(M.scene("mixed", "all", slots=60).spheres) == 60
    for sd in (M.scene("sphere_bvh", "ior"), M.scene("mixed", "ior")):  # every fifth sphere, IOR 2^50 among them
        r = sd.spheres["radius"][:M.FEW]
        assert (r[3::5] < 0).all() and (np.delete(r, np.s_[3::5]) > 0).all()
    assert M.SLOT_IOR_2_50 % 5 == 3 and M.scene("sphere_bvh", "ior").spheres["radius"][M.SLOT_IOR_2_50] < 0


# ------------------------------------------------------------------------------------------------------ the default arm
def _one_sphere(kind, param, mode):
    """A sphere of the given material alone in front of a bundle of rays (sphere program), or one triangle of it."""
    m = Material._make([0.8, 0.6, 0.4, 1.0], [param] * 3, kind)
    if mode == hrt.RT_MODE_SPHERE:
        return scenes.SceneDef("one", mode, 8, 8, None, hrt.spheres_array([Sphere._make(Vec3(0.0, 0.0, 0.0), 1.0, m)]),
                               min_sphere_slots=0)
    tri = np.zeros(1, dtype=hrt.TRIANGLE_DTYPE)
    tri["a"], tri["b"], tri["c"] = [-3.0, -3.0, 0.0, 1.0], [3.0, -3.0, 0.0, 1.0], [0.0, 3.0, 0.0, 1.0]
    tri["custom"] = [0.0, 0.0, 1.0]
    return scenes.SceneDef("one", mode, 8, 8, None, bvh=((1, 1), np.zeros(1, dtype=hrt.NODE_DTYPE), tri,
                                                          np.array([m], dtype=hrt.MATERIAL_DTYPE)))


def _bundle(n=512):
    g = np.random.default_rng(20261021)
    o = np.stack([g.uniform(-0.45, 0.45, n), g.uniform(-0.45, 0.45, n), np.full(n, 4.0)], axis=1).astype(np.float32)
    d = np.stack([g.uniform(-0.1, 0.1, n), g.uniform(-0.1, 0.1, n), np.full(n, -1.5)], axis=1).astype(np.float32)
    o[::2, 2], d[::2, 2] = -4.0, 1.5  # (half of them from behind: the triangle's other face)
    s = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return o, d, s, np.ones_like(o)


def _step(kind, param, mode):
    out = scenes.oracle_bounce_step(_one_sphere(kind, param, mode), *_bundle())
    assert out[5].all()  # every ray of the bundle hits
    return [np.ascontiguousarray(a).view(np.uint8) if a.dtype != bool else a for a in out]


@pytest.mark.parametrize("mode", [hrt.RT_MODE_SPHERE, hrt.RT_MODE_TRIS], ids=["sphere", "tris"])
@pytest.mark.parametrize("kind", M.KINDS, ids=hex)
def test_every_other_kind_shades_as_the_dielectric(kind, mode):
    for param in M.KIND_PARAMS:
        got, want = _step(kind, param, mode), _step(3, param, mode)
        for a, b, name in zip(got, want, ("origins", "dirs", "rng", "throughput", "records", "hit")):
            assert np.array_equal(a, b), f"kind {kind:#x} param {param}: {name} differ from kind 3's"
        if kind in M.MASKED_KINDS:
            low = _step(kind & 3, param, mode)
            assert kind & 3 in (1, 2)
            assert not np.array_equal(got[1], low[1]), f"kind {kind:#x} param {param}: the directions of kind {kind & 3}"
            assert not np.array_equal(got[2], low[2]), f"kind {kind:#x} param {param}: the RNG states of kind {kind & 3}"


# ----------------------------------------------------------------------------------------------------------- finiteness
@pytest.mark.parametrize("builder", PROGRAM_BUILDERS)
@pytest.mark.parametrize("table", M.FINITE_TABLES)
def test_kind_ior_and_fuzz_leave_every_channel_finite(table, builder):
    img, q = M.oracle(builder, table)
    sd = M.scene(builder, table)
    assert img.shape == (sd.height, sd.width, 3)
    assert np.isfinite(img).all(), (builder, table, int((~np.isfinite(img)).sum()))
    assert q > sd.width * sd.height * sd.frames  # (some path bounces)


def test_the_far_wall_is_finite():
    img, q = M.oracle("far_wall")
    assert np.isfinite(img).all(), int((~np.isfinite(img)).sum())
    r = M.scene("far_wall").spheres["radius"][M.FAR_SLOTS]
    assert r[0] == np.float32(2.0 ** 60) and r[1] == np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf))


@pytest.mark.parametrize("builder", PROGRAM_BUILDERS)
@pytest.mark.parametrize("table", M.ALBEDO_TABLES)
def test_albedo_scenes_hold_every_class_and_few_nans(table, builder):
    """NaN channels are at most a quarter; +inf and NaN channels exist in every albedo scene, and -inf channels wherever
    the -inf albedo is (with finite albedos a -inf needs the -1 sphere and two overflowing bounces in one path: some
    layouts show a few such channels, the deep one none in 8 frames)."""
    img, _ = M.oracle(builder, table)
    nan, pinf, ninf = int(np.isnan(img).sum()), int(np.isposinf(img).sum()), int(np.isneginf(img).sum())
    print(f"{builder}({table}): NaN {nan} +inf {pinf} -inf {ninf} of {img.size} channels")
    assert 4 * nan <= img.size, (builder, table, nan, img.size)
    assert nan >= 1 and pinf >= 1, (builder, table, nan, pinf)
    if table == "albedo_nonfinite":
        assert ninf >= 1, (builder, table, ninf)


@pytest.mark.parametrize("table", M.ALBEDO_TABLES)
def test_the_fold_draws_meet_every_class(table):
    """The draws of test_gpu_material_edges.test_folds_of_non_finite_samples: sphere_bvh at FOLD_FRAMES frames."""
    img, _ = M.oracle("sphere_bvh", table, frames=M.FOLD_FRAMES)
    nan, pinf, ninf = int(np.isnan(img).sum()), int(np.isposinf(img).sum()), int(np.isneginf(img).sum())
    print(f"sphere_bvh({table}) x{M.FOLD_FRAMES}: NaN {nan} +inf {pinf} -inf {ninf} of {img.size} channels")
    assert nan >= 1 and pinf >= 1 and ninf >= 1, (table, nan, pinf, ninf)
    assert 4 * nan <= img.size


@pytest.mark.parametrize("builder", ["tris", "mixed"])
def test_the_other_walks_rule_for_non_finite_rays_matters_only_where_such_rays_are(builder):
    """tri_bvh = 1 and the device trees answer a ray with a NaN or infinite component by the triangle test over every
    triangle in index order (include/hrt.h); the heap walk fails an all-NaN ray at the root box. The kinds table makes no
    such ray: the uncapped oracle is the same with and without the rule. All tables at once make many (fuzz NaN and
    infinity, IOR NaN): each then meets a triangle with t = NaN at every bounce until the cap."""
    from oracle import oracle as O

    assert M.STEP_CAP_SAH == O.STEP_CAP_SAH
    a, qa = M.oracle(builder, "kinds", step_cap=0)
    b, qb = M.oracle(builder, "kinds", step_cap=M.STEP_CAP_SAH)
    assert a.tobytes() == b.tobytes() and qa == qb
    a, qa = M.oracle(builder, "all", frames=M.SAH_FRAMES, step_cap=0)
    b, qb = M.oracle(builder, "all", frames=M.SAH_FRAMES, step_cap=M.STEP_CAP_SAH)
    assert (np.isnan(a) == np.isnan(b)).all()
    differ = int(((a.view(np.uint32) != b.view(np.uint32)) & ~np.isnan(a)).sum())
    print(f"{builder}(all): queries {qa} uncapped, {qb} with the rule; {differ} channels differ")
    assert qb > qa and differ > 0


# ----------------------------------------------------------------------------------------------------------- long paths
def _first_hits(builder, table):
    sd = M.scene(builder, table)
    o, d, s = M.primary(builder, table)
    rec, _ = scenes.oracle_cast_rays(sd, o, d)
    return sd, o, d, s, rec


def test_ior_2_50_from_inside_reflects_and_some_path_runs_to_the_bounce_cap():
    """Slot 13 has a negative radius: front_face is false, ir stays 2^50 and ir * sin_theta > 1 for every primary ray, so
    each is reflected. intersect_sphere (shader_sphere.wgsl:136-155) returns the near root alone and turns the normal
    against the ray, so the reflected ray leaves the sphere (d . n > 0) and cannot meet it again: -b - sqrt(disc) < 0. These
    samples end after 2 to 5 queries; no layout makes total reflection last inside a sphere of this reference. The paths
    that do use all 50 queries are stuck ones: IOR 1 refracts straight on, and where rounding leaves the new origin
    outside the sphere (c > 0) the near root is a tiny positive t and the same hit repeats until the cap."""
    sd, o, d, s, rec = _first_hits("sphere_bvh", "ior")
    on = rec["prim"] == M.SLOT_IOR_2_50
    assert on.sum() >= M.MIN_HITS and not (rec["flags"][on] & hrt.RT_HIT_FRONT).any()
    no, nd, _, _, rec1, hit = scenes.oracle_bounce_step(sd, o[on], d[on], s[on], np.ones_like(o[on]))
    assert hit.all() and ((nd * rec1["n"]).sum(axis=1) > 0).all()
    rec2, _ = scenes.oracle_cast_rays(sd, no, nd)
    assert (rec2["prim"] != M.SLOT_IOR_2_50).all()
    _, q, _ = scenes.oracle_trace_rays(sd, o, d, rng=s)
    capped = q == M.BOUNCES
    print(f"IOR 2^50 from inside: {int(on.sum())} primary rays, queries {np.bincount(q[on]).nonzero()[0].tolist()}; "
          f"{int(capped.sum())} samples of the scene use all {M.BOUNCES} queries, first hits {sorted(set(rec['prim'][capped].tolist()))}")
    assert capped.any()


def test_fuzz_minus_8_sends_the_ray_into_the_sphere_it_left():
    """After the first bounce on the fuzz -8 sphere some rays point into it (d . n < 0); their second query starts on that
    sphere and does not hit it (the near root is behind the origin)."""
    sd, o, d, s, rec = _first_hits("sphere_bvh", "fuzz")
    on = rec["prim"] == M.SLOT_FUZZ_MINUS_8
    assert on.sum() >= M.MIN_HITS
    no, nd, _, _, rec1, hit = scenes.oracle_bounce_step(sd, o[on], d[on], s[on], np.ones_like(o[on]))
    assert hit.all() and (rec1["prim"] == M.SLOT_FUZZ_MINUS_8).all()
    inward = (nd * rec1["n"]).sum(axis=1) < 0
    rec2, _ = scenes.oracle_cast_rays(sd, no, nd)
    left = inward & (rec2["prim"] != M.SLOT_FUZZ_MINUS_8)
    _, q, _ = scenes.oracle_trace_rays(sd, o[on], d[on], rng=s[on])
    print(f"fuzz -8: {int(on.sum())} primary rays, {int(inward.sum())} scattered inward, {int(left.sum())} of them miss the "
          f"sphere they start on; queries {np.bincount(q).nonzero()[0].tolist()}")
    assert left.any()
    assert (q[left] >= 2).all()
