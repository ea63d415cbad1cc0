"""rt_cast_rays / rt_primary_rays (Renderer.cast_rays, primary_rays, first_hit): closest-hit queries for the caller's
rays and the first hit behind each pixel sample.

Oracle identity. With frame_count 0 the accumulation weight is exactly 1, so a one-frame oracle image with bounces = 0
is the sky colour of each primary ray (img0) and with bounces = 1 it is img0 for a miss and (f32(albedo) * f32(0.7)) *
img0 for a hit: plain f32 products numpy repeats bit for bit. Every primitive carries its own albedo (asserted distinct
after the multiply), so img1 pins hit / miss and the identity of the primitive behind every pixel, and first_hit must
reproduce it on all three channels as uint32.

The cube scene: cube2.obj holds three boxes, 36 triangles (not 12); all 36 become one-triangle meshes with a material
each, so every triangle's identity is pinned.

Measured on an MI355X (the figures the tests print before they assert):
  sphere t against float64: 1.46 % of the 4096 rays left out, 99.61 % hit; largest |t - t64| / bound = 0.0332 over the
  4024 kept hits (a plain-f32 numpy evaluation of the same formula: 0.0424)
  triangle t against float64 Moller-Trumbore: suzane 0.32 % left out, largest ratio 0.0197 over 2517 hits; cube 0.74 %
  left out, 0.0154 over 1215
"""
import ctypes as C

import numpy as np
import pytest

import hrt
import scenes
from hrt import PI, Camera, Material, Mesh, Sphere, Tree, Vec3, f32, read_asset

pytestmark = pytest.mark.gpu

SHAPES = ((70, 45), (64, 40))
TIMES = (1000, 1010)
T_MISS = np.float32(hrt.RT_T_MISS)
U24 = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


# ------------------------------------------------------------------------------------------------ scenes
def _albedo(k, n):
    """Albedo k of n, all three channels distinct from every other k's (and from 0 and 1)."""
    x = (k + 1.0) / (n + 1.0)
    return [0.05 + 0.9 * x, 0.95 - 0.9 * x, 0.1 + 0.8 * ((7 * k + 3) % (n + 1)) / (n + 1.0), 1.0]


def _material(k, n):
    """Own albedo through Material._make whatever the kind: Lambertian, metal (fuzz 0.1), dielectric (1.5) by k % 3."""
    kind = (hrt.LAMBERTIAN, hrt.METAL, hrt.DIELECTRIC)[k % 3]
    return Material._make(_albedo(k, n), [(0.0, 0.1, 1.5)[k % 3]] * 3, kind)


def _recolour_bvh(bvh, first=0, total=None):
    sizes, nodes, tris, mats = bvh
    mats = mats.copy()
    total = len(mats) if total is None else total
    for k in range(len(mats)):
        mats[k] = _material(first + k, total)
    return (sizes, nodes, tris, mats)


def grid_spheres():
    """49 spheres at (1.5 i, 1.5 j, -6), i, j = -3 .. 3 in i-major order, radius 0.4 + 0.01 (k % 7), and a ground sphere
    of radius 1000 at (0, -1006, -6): (centres float64 (50, 3), radii float64 (50,), SPHERE_DTYPE array)."""
    c, r = [], []
    for i in range(-3, 4):
        for j in range(-3, 4):
            c.append((1.5 * i, 1.5 * j, -6.0))
            r.append(0.4 + 0.01 * (len(r) % 7))
    c.append((0.0, -1006.0, -6.0))
    r.append(1000.0)
    sp = hrt.spheres_array([Sphere._make(Vec3(*ck), rk, _material(k, len(c))) for k, (ck, rk) in enumerate(zip(c, r))])
    return sp["center"].astype(np.float64), sp["radius"].astype(np.float64), sp


def grid_scene(w, h, min_sphere_slots=0):
    cam = Camera.new(Vec3(0.0, 0.0, 2.0), Vec3(0.0, 0.0, -6.0), 8.0, 0.1, 0.9)
    return scenes.SceneDef("grid-50", hrt.RT_MODE_SPHERE, w, h, cam, grid_spheres()[2], frames=1, bounces=1,
                           min_sphere_slots=min_sphere_slots)


def grid_rays(n=4096):
    """The 4096-ray set: origins in front of the grid, each aimed near one of the 49 small spheres, |d| in
    [0.25, 4] x the distance (the sphere program does not normalise d). float32 (n, 3) origins and directions."""
    c, r, _ = grid_spheres()
    rng = np.random.default_rng(20261019)
    o = np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(0, 2, n)], axis=1)
    tgt = rng.integers(0, 49, n)
    off = rng.uniform(-0.7, 0.7, (n, 3)) * r[tgt][:, None]
    o = o.astype(np.float32)
    d = ((c[tgt] + off - o) * rng.uniform(0.25, 4, (n, 1))).astype(np.float32)
    return o, d


def split_cube_bvh():
    """Every triangle of cube2.obj as a one-triangle mesh with its own material."""
    whole = Tree.from_mesh(Mesh.load_obj(read_asset("cube2.obj"), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
    whole.build()
    tris = whole.view()[2]
    tree = Tree()
    for k, t in enumerate(tris):
        obj = "".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in t[v][:3]) for v in ("a", "b", "c")) + "f 1 2 3\n"
        tree.add_mesh(Mesh.load_obj(obj.encode(), _material(k, len(tris))))
    tree.build()
    return tree.view()


def cube_scene(w, h):
    cam = Camera.new(Vec3(0.0, 2.2, 6.5), Vec3(0.0, 0.1, -3.0), 2.2, 0.0, PI * f32(0.3))  # SceneTris::new_cube
    return scenes.SceneDef("split-cube", hrt.RT_MODE_TRIS, w, h, cam, bvh=split_cube_bvh(), frames=1, bounces=1)


def suzane_scene(w, h):
    bvh = _recolour_bvh(hrt.SceneTris.build_suzane_tree().view())
    return scenes.SceneDef("new_suzane", hrt.RT_MODE_TRIS, w, h, hrt.SceneTris.suzane_camera(), bvh=bvh, frames=1,
                           bounces=1)


def dragon_scene(w, h):
    sd = scenes._tris_scene("dragon", w, h, 1)
    sd.bvh = _recolour_bvh(sd.bvh)
    sd.bounces = 1
    return sd


def mixed_scene(w, h, extra):
    """C4, plus rtiow_spheres()[1:extra] (12 slots: the deferred scan; 60: the culling BVH), every primitive recoloured."""
    sd = scenes.config_c4(w, h, 1)
    if extra:
        sd.spheres = np.concatenate([sd.spheres, scenes.rtiow_spheres()[1:extra]])
    total = len(sd.spheres) + len(sd.bvh[3])
    sd.spheres = sd.spheres.copy()
    for k in range(len(sd.spheres)):
        sd.spheres[k]["material"] = _material(k, total)
    sd.bvh = _recolour_bvh(sd.bvh, first=len(sd.spheres), total=total)
    sd.bounces = 1
    return sd


# case -> (scene builder, shapes, rt_params, the oracle's step cap, the sphere scan the case is there for)
CASES = {}
for _v in (1, 3, 4):
    for _slots in (0, 100):
        CASES[f"sphere-v{_v}-slots{_slots}"] = (lambda w, h, s=_slots: grid_scene(w, h, s), SHAPES,
                                                dict(variant=_v), 600, _v)
for _tb in (0, 1):
    CASES[f"cube-tribvh{_tb}"] = (cube_scene, SHAPES, dict(tri_bvh=_tb), 0 if _tb else 600, 1)
    CASES[f"suzane-tribvh{_tb}"] = (suzane_scene, SHAPES, dict(tri_bvh=_tb), 0 if _tb else 600, 1)
    CASES[f"mixed-simple-tribvh{_tb}"] = (lambda w, h: mixed_scene(w, h, 0), SHAPES, dict(tri_bvh=_tb),
                                          0 if _tb else 600, 1)
    CASES[f"mixed-defer-tribvh{_tb}"] = (lambda w, h: mixed_scene(w, h, 12), SHAPES, dict(tri_bvh=_tb),
                                         0 if _tb else 600, 3)
    CASES[f"mixed-bvh-tribvh{_tb}"] = (lambda w, h: mixed_scene(w, h, 60), SHAPES, dict(tri_bvh=_tb),
                                       0 if _tb else 600, 4)
CASES["dragon-capped"] = (dragon_scene, ((64, 48),), dict(tri_bvh=0), 600, 1)


def _albedo_tables(sd):
    """(sphere albedos by slot, zero-filled padding slots included; triangle albedos by triangle index), float32 rgb."""
    sph = np.zeros((0, 3), np.float32)
    if sd.mode != hrt.RT_MODE_TRIS:
        n = len(sd.spheres)
        sph = np.zeros((max(n, sd.min_sphere_slots or 0), 3), np.float32)
        sph[:n] = sd.spheres["material"]["albedo"][:, :3]
    tri = np.zeros((0, 3), np.float32)
    if sd.mode != hrt.RT_MODE_SPHERE:
        tris, mats = sd.bvh[2], sd.bvh[3]
        tri = mats["albedo"][tris["material"]][:, :3].astype(np.float32)
    return sph, tri


def _assert_albedos_distinct(sd):
    """al * 0.7f pairwise distinct over the scene's materials (red channel): the image pins the primitive's material."""
    reds = []
    if sd.mode != hrt.RT_MODE_TRIS:
        reds += list(sd.spheres["material"]["albedo"][:, 0])
    if sd.mode != hrt.RT_MODE_SPHERE:
        reds += list(sd.bvh[3]["albedo"][:, 0])
    att = np.asarray(reds, np.float32) * np.float32(0.7)
    assert len(np.unique(att)) == len(att) and (att > 0).all(), sd.name


def _cpu(hit):
    return {k: v.cpu().numpy() for k, v in hit.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_first_hit_is_the_oracles_first_hit(case):
    build, shapes, params, step_cap, scan = CASES[case]
    for w, h in shapes:
        sd = build(w, h)
        _assert_albedos_distinct(sd)
        sph_al, tri_al = _albedo_tables(sd)
        r = scenes.make_renderer(sd)
        r.set_params(**params)
        if sd.mode != hrt.RT_MODE_TRIS and "variant" not in params:  # (the scan the slot count selects: the case's)
            want = 4 if len(sd.spheres) >= 32 else 3 if len(sd.spheres) > 8 else 1
            assert want == scan, (case, len(sd.spheres))
        for time in TIMES:
            what = f"{case} {w}x{h} time {time}"
            img0, _ = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=0, step_cap=step_cap)
            img1, _ = scenes.oracle_render(sd, frames=1, time0=time, frame0=0, bounces=1, step_cap=step_cap)
            hit = _cpu(r.first_hit(time))
            assert hit["t"].shape == (h, w) and hit["normal"].shape == (h, w, 3), what
            miss = hit["prim"] < 0
            is_tri = (hit["flags"] & hrt.RT_HIT_TRIANGLE) != 0
            assert not (miss & is_tri).any(), what
            assert (hit["t"][miss] == T_MISS).all() and (hit["t"][~miss] < T_MISS).all(), what
            for k in ("normal", "flags", "material"):
                assert not hit[k][miss].any(), (what, k)
            al = np.ones((h, w, 3), np.float32)
            s_hit, t_hit = ~miss & ~is_tri, ~miss & is_tri
            if sd.mode == hrt.RT_MODE_TRIS:
                assert not s_hit.any(), what
            if sd.mode == hrt.RT_MODE_SPHERE:
                assert not t_hit.any(), what
            assert (hit["prim"][s_hit] < len(sph_al)).all() and (hit["prim"][t_hit] < len(tri_al)).all(), what
            al[s_hit] = sph_al[hit["prim"][s_hit]]
            al[t_hit] = tri_al[hit["prim"][t_hit]]
            want = np.where(miss[..., None], img0, (al * np.float32(0.7)) * img0)
            bad = (want.view(np.uint32) != img1.view(np.uint32)).any(axis=2)
            assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            # material: the sphere's slot, or the triangle's material index
            assert (hit["material"][s_hit] == hit["prim"][s_hit]).all(), what
            if t_hit.any():
                assert (hit["material"][t_hit] == sd.bvh[2]["material"][hit["prim"][t_hit]]).all(), what
            assert (~miss).any(), what


# ------------------------------------------------------------------------------------------------ variants agree
def _records(hit):
    """The dict's fields side by side as int32 words (N, 7): bitwise comparison, NaNs included."""
    h = _cpu(hit)
    return np.concatenate([h["t"].view(np.int32)[:, None], h["prim"][:, None], h["normal"].view(np.int32),
                           h["flags"][:, None], h["material"][:, None]], axis=1)


def _grid_rays_with_degenerates():
    o, d = grid_rays()
    c, r, _ = grid_spheres()
    eo = np.array([[0.0, 0.0, 1.0],            # d = 0
                   [np.inf, 0.0, 1.0],         # an origin at +inf
                   c[24] + [0.1, 0.0, 0.0],    # inside small sphere 24 (the near root is behind the origin)
                   [0.0, -50.0, -6.0]],        # inside the ground sphere
                  dtype=np.float32)
    ed = np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, -1.0], [0.3, -0.5, -1.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    return np.concatenate([o, eo]), np.concatenate([d, ed])


@pytest.fixture(scope="module")
def grid_cast():
    """The 4096-ray cast of the grid scene (+ 4 degenerate rays) by variants 1, 3 and 4: {variant: records}, and the
    variant-4 dict on the host."""
    o, d = _grid_rays_with_degenerates()
    sd = grid_scene(64, 40)
    out, hit4 = {}, None
    for v in (1, 3, 4):
        r = scenes.make_renderer(sd)
        r.set_params(variant=v)
        hit = r.cast_rays(o, d)
        out[v] = _records(hit)
        if v == 4:
            hit4 = _cpu(hit)
    return o, d, out, hit4


def test_sphere_scan_variants_agree_bitwise(grid_cast):
    o, d, rec, _ = grid_cast
    assert rec[1].shape == (len(o), 7)
    for v in (3, 4):  # variant 1 is the literal linear scan
        bad = (rec[v] != rec[1]).any(axis=1)
        assert not bad.any(), (v, np.argwhere(bad)[:8].ravel().tolist())
    # the degenerate rays: d = 0 and the infinite origin miss; a ray from inside a sphere does not see that sphere (near
    # root only): the one inside sphere 24 goes on to the ground, the one inside the ground sphere leaves it unseen
    tail = rec[1][len(o) - 4:]
    assert (tail[[0, 1, 3], 1] == -1).all() and tail[2, 1] == 49, tail


def test_triangle_walks_agree_on_suzane():
    """tri_bvh 0 and 1 give bitwise-equal records on Suzanne's primary rays (no walk is capped there)."""
    sd = suzane_scene(70, 45)
    rec = []
    for tb in (0, 1):
        r = scenes.make_renderer(sd)
        r.set_params(tri_bvh=tb)
        rec.append(_records({k: v.reshape(70 * 45, *v.shape[2:]) for k, v in r.first_hit(1000).items()}))
    bad = (rec[0] != rec[1]).any(axis=1)
    assert not bad.any(), np.argwhere(bad)[:8].ravel().tolist()
    assert (rec[0][:, 1] >= 0).sum() > 500


# ------------------------------------------------------------------------------------------------ float64 references
def sphere_reference(o, d):
    """The near-root formula in float64 over all 50 spheres: (winner or -1, t64, kept mask, bound, h, D of the winner)."""
    c, r, _ = grid_spheres()
    o, d = o.astype(np.float64), d.astype(np.float64)
    oc = o[:, None, :] - c[None, :, :]                      # (N, 50, 3)
    a = (d * d).sum(1)[:, None]
    b = 2.0 * (oc * d[:, None, :]).sum(2)
    D2 = (oc * oc).sum(2)
    cc = D2 - r[None, :] ** 2
    disc = b * b - 4.0 * a * cc
    with np.errstate(invalid="ignore"):
        t = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), -1.0)
    acc = np.where(t > 0, t, np.inf)
    win = acc.argmin(1)
    t64 = acc.min(1)
    hit = np.isfinite(t64)
    # the impact parameter of every sphere: distance from its centre to the ray's line
    h = np.sqrt(np.maximum(D2 - (b / 2.0) ** 2 / a, 0.0))
    near_graze = (np.abs(h - r[None, :]) < 0.02).any(1)
    near_surface = (np.abs(np.sqrt(D2) - r[None, :]) < 0.02).any(1)
    two = np.sort(acc, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):  # (inf - inf where nothing is accepted)
        close_pair = hit & np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] < 1e-3 * two[:, 0])
    kept = ~(near_graze | near_surface | close_pair)
    k = np.arange(len(o))
    hw, Dw, rw = h[k, win], np.sqrt(D2[k, win]), r[win]
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = 64.0 * U24 * Dw ** 2 / (np.sqrt(a[:, 0]) * np.sqrt(np.maximum(rw ** 2 - hw ** 2, 0.0)))
    return np.where(hit, win, -1), t64, kept, bound


def test_sphere_t_and_normal_against_float64(grid_cast):
    """t within 64 * 2^-24 * D^2 / (|d| sqrt(r^2 - h^2)) of the float64 near root (first-order rounding of b^2 carried
    through the root, ~16x margin; derived, not measured), the same winner, n = +-(p - c) / r facing against d, and the
    front flag by the sign of d . (p - c)."""
    o, d, _, hit = grid_cast
    n = 4096
    o, d = o[:n], d[:n]
    hit = {k: v[:n] for k, v in hit.items()}
    win, t64, kept, bound = sphere_reference(o, d)
    c, r, _ = grid_spheres()
    left_out = 1.0 - kept.mean()
    print(f"left out {100 * left_out:.2f} %, hits {100 * (win >= 0).mean():.2f} %")
    assert left_out <= 0.05
    assert (win >= 0).mean() > 0.9
    assert (hit["prim"][kept] == win[kept]).all(), np.argwhere(kept & (hit["prim"] != win))[:8].ravel().tolist()
    k = kept & (win >= 0)
    ratio = np.abs(hit["t"][k].astype(np.float64) - t64[k]) / bound[k]
    print(f"largest |t - t64| / bound = {ratio.max():.4f} over {int(k.sum())} rays")
    assert (ratio <= 1.0).all(), (ratio.max(), int((ratio > 1).sum()))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    p = o64[k] + t64[k][:, None] * d64[k]
    nref = (p - c[win[k]]) / r[win[k]][:, None]
    front = (d64[k] * nref).sum(1) < 0
    nref = np.where(front[:, None], nref, -nref)
    assert np.abs(hit["normal"][k] - nref).max() <= 1e-4
    assert ((hit["normal"][k].astype(np.float64) * d64[k]).sum(1) < 0).all()
    assert (((hit["flags"][k] & hrt.RT_HIT_FRONT) != 0) == front).all()
    assert ((hit["flags"][k] & hrt.RT_HIT_TRIANGLE) == 0).all()
    assert (hit["material"][k] == win[k]).all()


def triangle_reference(o, d, tri):
    """Moller-Trumbore of ray k against triangle tri[k] in float64: (t, kept mask, bound)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    a, b, c = (tri[v][:, :3].astype(np.float64) for v in ("a", "b", "c"))
    e1, e2 = b - a, c - a
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    s = o - a
    u = (s * pv).sum(1) / det
    q = np.cross(s, e1)
    v = (d * q).sum(1) / det
    t = (e2 * q).sum(1) / det
    n1, n2, nd, ns = (np.linalg.norm(x, axis=1) for x in (e1, e2, d, s))
    kept = (np.abs(det) >= 1e-3 * n1 * n2 * nd) & (u >= 1e-3) & (v >= 1e-3) & (u + v <= 1.0 - 1e-3)
    bound = 64.0 * U24 * n1 * n2 * (ns + t * nd) / np.abs(det)
    return t, kept, bound


@pytest.mark.parametrize("name", ["suzane", "cube"])
def test_triangle_t_normal_and_material(name):
    """The record of the returned triangle: its stored normal bitwise, its material, and t within
    64 * 2^-24 |e1||e2|(|s| + t|d|) / |det| of a float64 Moller-Trumbore test of that triangle (closest-ness is the
    oracle-identity cases' business)."""
    w, h = 70, 45
    sd = suzane_scene(w, h) if name == "suzane" else cube_scene(w, h)
    tris = sd.bvh[2]
    r = scenes.make_renderer(sd)
    o, d = (x.cpu().numpy().reshape(-1, 3) for x in r.primary_rays(1000))
    hit = {k: v.reshape(w * h, *v.shape[2:]) for k, v in _cpu(r.first_hit(1000)).items()}
    m = hit["prim"] >= 0
    assert m.sum() > 300 and ((hit["flags"][m] & hrt.RT_HIT_TRIANGLE) != 0).all()
    tri = tris[hit["prim"][m]]
    np.testing.assert_array_equal(hit["normal"][m].view(np.uint32), tri["custom"].view(np.uint32))
    assert (hit["material"][m] == tri["material"]).all()
    front = (tri["custom"].astype(np.float64) * d[m].astype(np.float64)).sum(1) > 0  # (tri_record: dot(n, d) > 0)
    assert (((hit["flags"][m] & hrt.RT_HIT_FRONT) != 0) == front).all()
    t64, kept, bound = triangle_reference(o[m], d[m], tri)
    left_out = 1.0 - kept.mean()
    ratio = np.abs(hit["t"][m][kept].astype(np.float64) - t64[kept]) / bound[kept]
    print(f"{name}: left out {100 * left_out:.2f} %, largest |t - t64| / bound = {ratio.max():.4f} over {int(kept.sum())}")
    assert left_out <= 0.05
    assert (hit["t"][m][kept] >= np.float32(1e-4)).all()
    assert (ratio <= 1.0).all(), (ratio.max(), int((ratio > 1).sum()))


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_ray_counts_and_sentinel(n, grid_cast):
    """The first n rays give the first n records of the 4096-ray cast, and the record after them is not written."""
    import torch

    o, d, rec, _ = grid_cast
    r = scenes.make_renderer(grid_scene(64, 40))
    dev = torch.device("cuda", r.device()[0])
    to = torch.from_numpy(o[:n].copy()).to(dev)
    td = torch.from_numpy(d[:n].copy()).to(dev)
    hits = torch.full((n + 1, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = hrt.lib().rt_cast_rays(r._h, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), n, C.c_void_p(hits.data_ptr()))
    assert rc == 0, hrt.lib().rt_last_error()
    r.synchronize()
    got = hits.cpu().numpy()
    assert (got[n] == 0x5A5A5A5A).all(), got[n]
    assert (got[:n, 7] == 0).all()  # reserved
    np.testing.assert_array_equal(got[:n, :7], rec[4][:n])
    hit = r.cast_rays(o[:n], d[:n])  # the wrapper, numpy in
    assert hit["t"].shape == (n,) and hit["normal"].shape == (n, 3)
    np.testing.assert_array_equal(_records(hit), rec[4][:n])


# ------------------------------------------------------------------------------------------------ isolation
def test_queries_leave_the_draw_state_alone():
    sd = scenes.config_c3(64, 40, 6)
    ref, q = scenes.oracle_render(sd)
    r = scenes.make_renderer(sd)
    r.set_params(schedule=hrt.RT_SCHEDULE_QUEUE)
    r.draw_frames(3, 1000, 10)

    def snapshot():
        st = r.stats()
        return r.read_image().tobytes(), bytes(st), tuple(r.raw_counters()), r.frame_count

    before = snapshot()
    q3 = r.stats().queries
    hit = r.first_hit(1030)
    o, d = grid_rays(512)
    r.cast_rays(o, d)
    assert (hit["prim"] >= 0).any()
    assert snapshot() == before
    r.draw_frames(3, 1030, 10)
    img = r.read_image()
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert q3 + r.stats().queries == q and r.frame_count == 6


# ------------------------------------------------------------------------------------------------ partition
def test_partition_primary_rays_are_the_full_images_rows():
    from hrt.parallel import owned_rows

    w, h = 70, 45
    for sd in (grid_scene(w, h), suzane_scene(w, h)):
        full = scenes.make_renderer(sd)
        fo, fd = (x.cpu().numpy() for x in full.primary_rays(1010))
        part = scenes.make_renderer(sd)
        part.set_params(row0=1, row_step=3, row_block=2)
        rows = owned_rows(1, 3, h, 2)
        po, pd = (x.cpu().numpy() for x in part.primary_rays(1010))
        assert po.shape == (len(rows), w, 3) and len(rows) == part.local_rows
        np.testing.assert_array_equal(po.view(np.uint32), fo[rows].view(np.uint32))
        np.testing.assert_array_equal(pd.view(np.uint32), fd[rows].view(np.uint32))
        hit = part.first_hit(1010)
        assert hit["t"].shape == (len(rows), w)
        np.testing.assert_array_equal(_cpu(hit)["prim"], _cpu(full.first_hit(1010))["prim"][rows])


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    import torch

    L = hrt.lib()
    r = hrt.Renderer(16, 8, hrt.RT_MODE_SPHERE)
    dev = torch.device("cuda", r.device()[0])
    buf = torch.zeros((16 * 8, 8), dtype=torch.float32, device=dev)
    hits = torch.zeros((16 * 8, 8), dtype=torch.float32, device=dev)
    p, ph = C.c_void_p(buf.data_ptr()), C.c_void_p(hits.data_ptr())
    # primary rays before a camera is set
    assert L.rt_primary_rays(r._h, 1000, p, p, 16 * 8) == hrt._lib.RT_ERR_STATE
    with pytest.raises(hrt.RtError) as e:
        r.primary_rays(1000)
    assert e.value.code == hrt._lib.RT_ERR_STATE
    # a cast needs no camera; a null pointer with n > 0 is refused, n = 0 is not
    for args in ((None, p, ph), (p, None, ph), (p, p, None)):
        assert L.rt_cast_rays(r._h, *args[:2], 4, args[2]) == hrt._lib.RT_ERR_ARG
    assert L.rt_cast_rays(r._h, None, None, 0, None) == hrt._lib.RT_OK
    assert L.rt_cast_rays(r._h, p, p, 4, C.c_void_p(hits.data_ptr() + 8)) == hrt._lib.RT_ERR_ARG  # hits: 16-B aligned
    assert L.rt_cast_rays(r._h, p, p, 4, ph) == hrt._lib.RT_OK  # (an empty scene: 100 zero slots)
    r.synchronize()
    r.set_camera(scenes.default_sphere_camera())
    assert L.rt_primary_rays(r._h, 1000, p, p, 16 * 8 - 1) == hrt._lib.RT_ERR_ARG  # a wrong n_rays
    assert L.rt_primary_rays(r._h, 1000, None, p, 16 * 8) == hrt._lib.RT_ERR_ARG
    o, d = r.primary_rays(1000)
    assert o.shape == (8, 16, 3) and torch.isfinite(d).all()
    with pytest.raises(ValueError):
        r.cast_rays(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        r.cast_rays(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32))
