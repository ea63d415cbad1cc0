"""The oracle's per-ray entry points (oracle_cast_rays, oracle_trace_rays, oracle_bounce_step, oracle_primary_rays)
pinned, bit for bit, to the path the goldens pin (oracle_render), and the conditions the ray sets of ray_sets.py must meet,
asserted from the oracle alone. No GPU.

The per-ray functions call the same static functions oracle_render calls; these tests show that the export added nothing
of its own: a frame put together from them is the frame oracle_render draws, queries included.
"""
import dataclasses

import numpy as np
import pytest

import hrt
import ray_sets
import scenes
import test_gpu_cast_rays as cast
from hrt.parallel import local_rows

SHAPES = ((33, 17), (70, 45))
TIMES = (1000, 1010)
SCENES = {
    "grid": lambda w, h: cast.grid_scene(w, h),
    "grid-100": lambda w, h: cast.grid_scene(w, h, 100),
    "cube": cast.cube_scene,
    "suzane": cast.suzane_scene,
    "mixed": lambda w, h: cast.mixed_scene(w, h, 12),
}


def _scene(name, w, h):
    """The scene with the reference's own bounce cap (10 sphere / 5 triangle and mixed) in place of the builders' 1."""
    return dataclasses.replace(SCENES[name](w, h), bounces=None)


def _bounces(sd):
    return 10 if sd.mode == hrt.RT_MODE_SPHERE else 5


def _partitions(h):
    """All rows, and the blocked share of rank 1 of 3 with blocks of 2 rows."""
    return (None, (1, 3, local_rows(1, 3, h, 2), 2))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sky(d):
    """trace()'s sky term from the primary direction, in f32 as the oracle evaluates it (no fused operation)."""
    one, half = np.float32(1.0), np.float32(0.5)
    tt = d[:, 1] * half + half
    lo, hi = np.array([0.54, 0.86, 0.92], np.float32), np.array([0.54, 0.7, 0.98], np.float32)
    return hi[None, :] * tt[:, None] + lo[None, :] * (one - tt)[:, None]


def _records_u32(rec):
    return np.frombuffer(rec.tobytes(), dtype=np.uint32).reshape(-1, 8)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_frame_from_the_per_ray_functions_is_oracle_renders_frame(name):
    for w, h in SHAPES:
        sd = _scene(name, w, h)
        for rows in _partitions(h):
            for time in TIMES:
                what = f"{name} {w}x{h} rows {rows} time {time}"
                img, q = scenes.oracle_render(sd, frames=1, frame0=0, time0=time, rows=rows)
                o, d, s = scenes.oracle_primary_rays(sd, time, rows=rows)
                assert o.shape == img.shape and s.shape == img.shape[:2], what
                o, d, s = o.reshape(-1, 3), d.reshape(-1, 3), s.reshape(-1)
                # 1. trace_rays on the primary rays and states
                rad, qs, counts = scenes.oracle_trace_rays(sd, o, d, rng=s)
                assert np.array_equal(_u32(rad), _u32(img.reshape(-1, 3))), what
                assert int(qs.sum()) == q == counts["rays"], what
                assert qs.max() <= _bounces(sd) and (qs >= 1).all(), what
                # 2. bounce_step iterated: throughput * sky, and step 1's records are cast_rays'
                co, cd, cs = o.copy(), d.copy(), s.copy()
                tp = np.ones_like(o)
                queries = np.zeros(len(o), np.uint32)
                live = np.arange(len(o))
                for step in range(_bounces(sd)):
                    if not len(live):
                        break
                    no, nd, ns, ntp, rec, hit = scenes.oracle_bounce_step(sd, co[live], cd[live], cs[live], tp[live])
                    if step == 0:
                        first, _ = scenes.oracle_cast_rays(sd, o, d)
                        assert rec.tobytes() == first.tobytes(), what
                    miss = ~hit
                    for new, old in ((no, co), (nd, cd), (ntp, tp)):  # a miss leaves the state alone
                        assert np.array_equal(_u32(new[miss]), _u32(old[live][miss])), what
                    assert np.array_equal(ns[miss], cs[live][miss]), what
                    assert ((rec["prim"] >= 0) == hit).all(), what
                    co[live], cd[live], cs[live], tp[live] = no, nd, ns, ntp
                    queries[live] += 1
                    live = live[hit]
                zero = np.float32(0.0)
                assert np.array_equal(_u32(zero + tp * _sky(d)), _u32(rad)), what
                assert np.array_equal(queries, qs), what


@pytest.mark.parametrize("name", sorted(SCENES))
def test_cast_rays_on_primary_rays_satisfies_the_albedo_identity(name):
    """img1 = (albedo * 0.7) * img0 on a hit and img0 on a miss, with the albedo of the primitive the record names: the
    identity test_gpu_cast_rays.py holds the device's first_hit to."""
    for w, h in SHAPES:
        sd = SCENES[name](w, h)
        cast._assert_albedos_distinct(sd)
        sph_al, tri_al = cast._albedo_tables(sd)
        for time in TIMES:
            what = f"{name} {w}x{h} time {time}"
            img0, _ = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=0)
            img1, _ = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=1)
            o, d, _ = scenes.oracle_primary_rays(sd, time)
            rec, _ = scenes.oracle_cast_rays(sd, o.reshape(-1, 3), d.reshape(-1, 3))
            rec = rec.reshape(h, w)
            miss = rec["prim"] < 0
            is_tri = (rec["flags"] & hrt.RT_HIT_TRIANGLE) != 0
            assert (~miss).any() and not (miss & is_tri).any(), what
            assert (rec["t"][miss] == np.float32(hrt.RT_T_MISS)).all(), what
            for k in ("n", "flags", "material", "reserved"):
                assert not rec[k][miss].any(), (what, k)
            al = np.ones((h, w, 3), np.float32)
            s_hit, t_hit = ~miss & ~is_tri, ~miss & is_tri
            al[s_hit] = sph_al[rec["prim"][s_hit]]
            al[t_hit] = tri_al[rec["prim"][t_hit]]
            want = np.where(miss[..., None], img0, (al * np.float32(0.7)) * img0)
            assert np.array_equal(_u32(want), _u32(img1)), what
            assert (rec["material"][s_hit] == rec["prim"][s_hit]).all(), what
            if t_hit.any():
                assert (rec["material"][t_hit] == sd.bvh[2]["material"][rec["prim"][t_hit]]).all(), what


def test_flat_is_the_uncapped_walk_on_suzannes_primary_rays():
    """No walk drops anything there: the capped walk, the uncapped walk and the test of every triangle agree."""
    sd = cast.suzane_scene(70, 45)
    o, d, _ = scenes.oracle_primary_rays(sd, 1000)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    flat, cf = scenes.oracle_cast_rays(sd, o, d, flat=True)
    walk, cw = scenes.oracle_cast_rays(sd, o, d, step_cap=0)
    capped, cc = scenes.oracle_cast_rays(sd, o, d)
    assert flat.tobytes() == walk.tobytes() == capped.tobytes()
    assert cf["tri_tests"] == len(o) * int(sd.bvh[0][1]) > cw["tri_tests"] > 0
    assert cw["capped_walks"] == 0 and (flat["prim"] >= 0).sum() > 500


def test_null_states_are_the_seed_product_in_u32():
    sd = _scene("grid", 33, 17)
    o, d, _ = scenes.oracle_primary_rays(sd, 1000)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    for seed in (1, 0x9E3779B9):
        s = ((np.arange(len(o), dtype=np.uint64) + 1) * seed & 0xFFFFFFFF).astype(np.uint32)
        a = scenes.oracle_trace_rays(sd, o, d, rng=s)
        b = scenes.oracle_trace_rays(sd, o, d, rng=None, seed=seed)
        assert np.array_equal(_u32(a[0]), _u32(b[0])) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the ray sets
@pytest.mark.parametrize("name", sorted(ray_sets.SCENES))
def test_ray_set_conditions(name):
    """What the issue asks of the ray sets, from the oracle alone; prints the share of hits in every class."""
    sd, rays = ray_sets.scene_and_rays(name)
    o, d, label = rays.interleaved()
    assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (len(label), 3)
    assert 64 * 64 < len(o) < 65 * 64 and len(o) % 64 != 0, len(o)
    ob, db, lb, perm = rays.blocked()
    assert np.array_equal(_u32(ob), _u32(o[perm])) and np.array_equal(_u32(db), _u32(d[perm]))
    assert sorted(perm.tolist()) == list(range(len(o)))
    # blocked: the full waves up to the last of each class hold one class each
    full = lb[: len(lb) // 64 * 64].reshape(-1, 64)
    uniform = (full == full[:, :1]).all(axis=1)
    assert uniform.sum() >= len(full) - len(ray_sets.CLASSES), (int(uniform.sum()), len(full))
    for c in ray_sets.CLASSES:
        assert uniform[full[:, 0] == c].any(), c
    # interleaved: every full wave mixes classes
    fi = label[: len(label) // 64 * 64].reshape(-1, 64)
    assert all(len(set(row.tolist())) >= 4 for row in fi)

    rec, counts = scenes.oracle_cast_rays(sd, o, d, step_cap=ray_sets.STEP_CAP)
    hit = rec["prim"] >= 0
    shares = {}
    for c in ray_sets.CLASSES:
        m = label == c
        assert m.sum() >= 64, (c, int(m.sum()))
        shares[c] = float(hit[m].mean())
    print(f"{name}: {len(o)} rays, hit share by class " + ", ".join(f"{c} {100 * v:.1f} %" for c, v in shares.items())
          + f"; capped walks {counts['capped_walks']}")
    for c, v in shares.items():
        if c != "g":
            assert 0.10 <= v <= 0.90, (name, c, v)
    if sd.mode == hrt.RT_MODE_SPHERE:
        for k in ray_sets.LENGTH_EXPONENTS:
            m = rays.length_exponent == k
            assert m.any() and hit[m].any(), (name, k)
    if name == "dragon":
        assert counts["capped_walks"] > 0
    if sd.mode != hrt.RT_MODE_TRIS and (sd.min_sphere_slots or 0) == 100:
        pad = hit & ((rec["flags"] & hrt.RT_HIT_TRIANGLE) == 0) & (rec["prim"] >= len(sd.spheres))
        print(f"{name}: {int(pad.sum())} rays hit a padding slot")
        assert pad.any()


def test_ray_sets_are_seeded():
    a = ray_sets.scene_and_rays("grid")[1].interleaved()
    b = ray_sets.scene_and_rays("grid")[1].interleaved()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
