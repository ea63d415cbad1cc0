"""Every shading path against the oracle at the edges of Material.kind, Material.params, Material.albedo and Sphere.radius
(material_edges_util.py has the tables and scenes; test_material_edges_oracle.py pins, on the CPU, that every table entry is
seen by primary rays, what the default arm is and which scenes are finite).

The kernels restate the reference's scatter in several places: five record loads fold Material.kind into two bits of
Hit::id (id == 1 || id == 2 ? id : 0), the dielectric arm reads 1 / param and two r0^2 values the HOST computed
(renderer.cpp dielectric_consts) from SphereAux or MatDev depending on the program and on h.id & 4, and the metal arm and
refract run range-guarded exact-math helpers whose arguments the material parameters alone can push out of range. Every
assertion here is against the oracle: its bits where its image is finite (kind, index of refraction, fuzz, the far wall),
and where albedo makes it non-finite, equal NaN masks and the oracle's bits in every other channel, +-inf included. Queries
equal the oracle's count everywhere.
"""
import dataclasses
import functools

import numpy as np
import pytest

import hrt
import kernel_cases
import material_edges_util as M
import scenes
import test_gpu_ray_queries_oracle as Q
from test_gpu_small_shapes import PATHS, _kernel_is

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")


def _draw(sd, params, frames=None):
    r = scenes.make_renderer(sd)
    r.set_params(**params)
    r.draw_frames(sd.frames if frames is None else frames, M.TIME0, 10)
    return r


def _check(r, ref, q, what, kernel=None):
    img, st = r.read_image(), r.stats()
    print(f"{what}: kernel {st.kernel.decode()} launches {st.launches} trace {st.trace_launches} fold_ring {st.fold_ring} "
          f"queries {st.queries} (oracle {q}) NaN {int(np.isnan(img).sum())} (oracle {int(np.isnan(ref).sum())}) "
          f"differing channels {int(((img.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(img) & np.isnan(ref))).sum())}")
    if kernel is not None:
        _kernel_is(st, kernel, what)
    M.assert_image(img, ref, what)
    assert st.queries == q, (what, st.queries, q)
    return st


# ---- a. every draw kernel shades the edge materials
ROLE_SCENES = {"c3": ("sphere_bvh", {}), "deep": ("deep", {}), "tris": ("tris", {}), "c4": ("mixed", dict(slots=1)),
               "defer": ("mixed", {}), "bvh": ("mixed", dict(slots=60))}
# the deferred scan of the sphere program, which no role above draws: k_trace and k_render over 12 slots
FEW_CASES = [dict(schedule=hrt.RT_SCHEDULE_QUEUE, variant=v, steal=1) for v in (1, 3)] + \
            [dict(schedule=hrt.RT_SCHEDULE_TILES, variant=v) for v in (1, 3)] + [dict(schedule=hrt.RT_SCHEDULE_TILES)]


def test_every_instantiation_shades_the_edge_materials():
    """kernel_cases.param_cases(), the dictionaries of test_gpu_kernels.test_every_instantiation_is_reached, each on the scene
    of its role that holds every table at once. The kernels these draws report are the whole set in the code object, which
    is the set that test reaches: no instantiation is left shading only demo materials. tri_bvh = 1 is held to the uncapped
    oracle with that walk's rule for non-finite rays (M.STEP_CAP_SAH): the edge materials make such rays, the demo ones none."""
    want = kernel_cases.library_kernels()
    assert len(want) >= 30, want
    seen = {}
    cases = [(ROLE_SCENES[role], params) for role, params in kernel_cases.param_cases()]
    cases += [(("sphere_few", {}), params) for params in FEW_CASES]
    for (builder, kw), params in cases:
        sd = M.scene(builder, "all", **kw)
        # (2 frames under the rule: a NaN ray costs the oracle every triangle at each of its 50 bounces)
        frames = M.SAH_FRAMES if params.get("tri_bvh") else sd.frames
        ref, q = M.oracle(builder, "all", frames=frames, step_cap=M.STEP_CAP_SAH if params.get("tri_bvh") else 600, **kw)
        r = _draw(sd, params, frames)
        st = _check(r, ref, q, f"{sd.name} {params}")
        seen.setdefault(st.kernel.decode(), (sd.name, params))
    missing, extra = want - set(seen), set(seen) - want
    assert not missing, f"instantiations no edge-material draw reaches: {sorted(missing)}"
    assert not extra, f"kernels reported but not in the library: {sorted(extra)}"


# ---- b. per table, on the default paths
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("table", M.TABLE_NAMES)
def test_sphere_program_per_table(table, path):
    params, kernel, fold_ring = PATHS[path]
    sd = M.scene("sphere_bvh", table)
    ref, q = M.oracle("sphere_bvh", table)
    st = _check(_draw(sd, params), ref, q, f"sphere_bvh({table}) {path}", kernel)
    assert st.fold_ring == fold_ring, (table, path, st.fold_ring)
    assert st.samples == sd.width * sd.height * sd.frames


@pytest.mark.parametrize("schedule, kernel", [(hrt.RT_SCHEDULE_QUEUE, "k_trace_split_tris<"), (hrt.RT_SCHEDULE_TILES, "k_render<")],
                         ids=["queue", "tiles"])
@pytest.mark.parametrize("builder", ["tris", "mixed"])
@pytest.mark.parametrize("table", M.TABLE_NAMES)
def test_triangle_and_mixed_programs_per_table(table, builder, schedule, kernel):
    sd = M.scene(builder, table)
    ref, q = M.oracle(builder, table)
    _check(_draw(sd, dict(schedule=schedule)), ref, q, f"{builder}({table}) schedule {schedule}", kernel)


# ---- c. folds of non-finite samples
# (the ring's launches are not sized by the budget but hold 48 jobs a tile: jobs of one frame make 100 frames three launches)
FOLDS = {"fold_buffer": (hrt.RT_FOLD_BUFFER, 0, {}), "fold_next": (hrt.RT_FOLD_NEXT, 2, {}),
         "fold_ring": (hrt.RT_FOLD_RING, 1, dict(job_frames=1))}


@pytest.mark.parametrize("fold", sorted(FOLDS))
@pytest.mark.parametrize("table", M.ALBEDO_TABLES)
def test_folds_of_non_finite_samples(table, fold):
    """100 frames of a 48 x 40 image under a 1 MiB budget: three launches (a frame is 30 tiles of 768 B), the second and
    third folding +inf, -inf and NaN samples onto sums that hold them already (inf - inf, 0 x inf). The NaN rule holds the
    ring, the sample buffer and the next-launch fold to the same classes: a NaN where the oracle has one, and the bits of
    +inf or -inf where it has those."""
    mode, fold_ring, more = FOLDS[fold]
    sd = dataclasses.replace(M.scene("sphere_bvh", table), frames=M.FOLD_FRAMES)
    ref, q = M.oracle("sphere_bvh", table, frames=M.FOLD_FRAMES)
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()
    params = dict(PATHS["4_queues"][0], fold=mode, queue_budget_mb=1, **more)
    st = _check(_draw(sd, params), ref, q, f"sphere_bvh({table}) x{sd.frames} {fold}", "k_trace_split<")
    assert st.fold_ring == fold_ring, (fold, st.fold_ring)
    assert st.trace_launches == 3, (fold, st.trace_launches, st.launch_frames)


@pytest.mark.parametrize("table", M.ALBEDO_TABLES)
def test_draw_frames_and_per_frame_draws_of_non_finite_samples(table):
    """The same 100 frames by one draw_frames call and by 100 draw calls (k_accumulate's running mean frame by frame)."""
    sd = dataclasses.replace(M.scene("sphere_bvh", table), frames=M.FOLD_FRAMES)
    ref, q = M.oracle("sphere_bvh", table, frames=M.FOLD_FRAMES)
    _check(_draw(sd, {}), ref, q, f"sphere_bvh({table}) x{sd.frames} draw_frames")
    r = scenes.make_renderer(sd)
    for i in range(sd.frames):
        r.set_time(M.TIME0 + 10 * i)
        r.draw()
    img = r.read_image()
    M.assert_image(img, ref, f"sphere_bvh({table}) x{sd.frames} per-frame draws")


# ---- d. the far wall
@pytest.mark.parametrize("path", ["1_k_render", "2_k_trace", "4_queues"])
def test_far_wall(path):
    """Metal spheres of radius 2^60 and the next f32, either side of upload_spheres' rad_ok: the normal is (p - c) * (1 / r)
    below and the division sequence above."""
    params, kernel, _ = PATHS[path]
    ref, q = M.oracle("far_wall")
    assert np.isfinite(ref).all()
    # (6 slots: path 4's variant 4 draws them with k_trace_split all the same)
    _check(_draw(M.scene("far_wall"), params), ref, q, f"far_wall {path}", kernel.split("<")[0] + "<")


# ---- e. ray queries
QUERY_SCENES = ["sphere_bvh", "tris", "mixed"]


@functools.lru_cache(maxsize=None)
def _rays(builder):
    o, d, s = (a.copy() for a in M.primary(builder, "all"))  # (writable: torch.from_numpy wants that)
    return M.scene(builder, "all"), o, d, s


@pytest.mark.parametrize("builder", QUERY_SCENES)
def test_cast_rays_records(builder):
    sd, o, d, _ = _rays(builder)
    want, _ = scenes.oracle_cast_rays(sd, o, d)
    Q._assert_records(Q._cast_raw(scenes.make_renderer(sd), o, d), want, f"{sd.name} cast_rays")


@pytest.mark.parametrize("builder", QUERY_SCENES)
def test_trace_rays_radiance_and_queries(builder):
    sd, o, d, s = _rays(builder)
    rad, q, _ = scenes.oracle_trace_rays(sd, o, d, rng=s)
    got, gq = scenes.make_renderer(sd).trace_rays(o, d, rng=s, want_queries=True)
    Q._assert_same(got.cpu().numpy(), rad, f"{sd.name} trace_rays radiance")
    Q._assert_same(gq.cpu().numpy(), q, f"{sd.name} trace_rays queries", is_float=False)
    ref1, q1 = M.oracle(builder, "all", frames=1)  # the primary rays' radiance is the one-frame image
    Q._assert_same(got.cpu().numpy(), ref1.reshape(-1, 3), f"{sd.name} trace_rays against the one-frame render")
    assert int(q.sum()) == q1


@pytest.mark.parametrize("builder", QUERY_SCENES)
def test_three_bounce_steps(builder):
    """As test_gpu_ray_queries_oracle.test_three_bounce_steps_are_the_oracles, from the primary rays: origins, directions,
    RNG states, throughput (infinite and NaN after an albedo slot), queries, hit records, and the compacted count and
    index set after rays whose direction became NaN or zero (fuzz 2^64 normalises to 0)."""
    import torch

    sd, o, d, s = _rays(builder)
    r = scenes.make_renderer(sd)
    n = len(o)
    dev = r._torch_device()
    co, cd, cs, ct = o.copy(), d.copy(), s.copy(), np.ones_like(o)
    cq = np.zeros(n, np.uint32)
    O, D = torch.from_numpy(co.copy()).to(dev), torch.from_numpy(cd.copy()).to(dev)
    S = torch.from_numpy(cs.view(np.int32).copy()).to(dev)
    T = torch.ones((n, 3), dtype=torch.float32, device=dev)
    NQ = torch.zeros((n,), dtype=torch.int32, device=dev)
    H = torch.empty((n, 8), dtype=torch.int32, device=dev)
    idx = [torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    cnt = [torch.zeros((1,), dtype=torch.int32, device=dev) for _ in range(2)]
    live = np.arange(n)
    for step in range(3):
        what = f"{sd.name} step {step + 1}"
        H.fill_(Q.SENTINEL)
        kw = dict(index_in=idx[(step - 1) % 2], count_in=cnt[(step - 1) % 2]) if step else {}
        r.bounce_rays(O, D, S, throughput=T, queries=NQ, hits=H, index_out=idx[step % 2], count_out=cnt[step % 2], **kw)
        no, nd, ns, nt, rec, hit = scenes.oracle_bounce_step(sd, co[live], cd[live], cs[live], ct[live])
        co[live], cd[live], cs[live], ct[live] = no, nd, ns, nt
        cq[live] += 1
        h = H.cpu().numpy()
        Q._assert_records(h[live], rec, what + " hit records")
        untouched = np.ones(n, bool)
        untouched[live] = False
        assert (h[untouched] == Q.SENTINEL).all(), what
        Q._assert_same(O.cpu().numpy(), co, what + " origins")
        Q._assert_same(D.cpu().numpy(), cd, what + " dirs")
        Q._assert_same(T.cpu().numpy(), ct, what + " throughput")
        Q._assert_same(S.cpu().numpy(), cs, what + " rng", is_float=False)
        Q._assert_same(NQ.cpu().numpy(), cq, what + " queries", is_float=False)
        count = int(cnt[step % 2].item())
        forwarded = np.sort(idx[step % 2].cpu().numpy()[:count])
        live = live[hit]
        nonfinite = int((~np.isfinite(cd[live])).any(axis=1).sum())
        zero = int((cd[live] == 0).all(axis=1).sum())
        print(f"{what}: {count} paths go on (oracle {len(live)}), {nonfinite} with a non-finite and {zero} with a zero "
              f"direction, {int((~np.isfinite(ct[live])).any(axis=1).sum())} with a non-finite throughput")
        assert count == len(live) and np.array_equal(forwarded, live), (what, count, len(live))
        assert len(live) > n // 20, what


@pytest.mark.parametrize("builder", QUERY_SCENES)
def test_wavefront_with_regrouping_is_the_drawn_frame(builder):
    """50 bounce_rays steps with rt_regroup_paths after the first, and after every step: the oracle's one-frame image and
    per-ray queries (as test_gpu_regroup.test_wavefront_with_regrouping_is_the_traced_frame, held to the oracle)."""
    sd, o, d, s = _rays(builder)
    ref1, q1 = M.oracle(builder, "all", frames=1)
    _, q, _ = scenes.oracle_trace_rays(sd, o, d, rng=s)
    r = scenes.make_renderer(sd)
    box = ((-8.0, -2.0, -8.0), (8.0, 8.0, 8.0))
    for after in ((1,), tuple(range(1, M.BOUNCES + 1))):
        what = f"{sd.name} wavefront, regroup after {after[:3]}.."
        got, gq = r.trace_wavefront(o, d, s, M.BOUNCES, want_queries=True, regroup_box=box, regroup_after=after)
        Q._assert_same(got.cpu().numpy(), ref1.reshape(-1, 3), what + " radiance")
        Q._assert_same(gq.cpu().numpy(), q, what + " queries", is_float=False)
    assert int(q.sum()) == q1


# ---- f. device geometry
@pytest.mark.parametrize("builder_id", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("builder", ["tris", "mixed"])
@pytest.mark.parametrize("table", ["kinds", "all"])
def test_device_geometry_shades_the_edge_materials(table, builder, builder_id):
    """rt_set_triangles_device is pack_materials' second caller: the edge materials through it, drawn with tri_bvh = 1,
    against the uncapped oracle. The kinds make no non-finite ray and are held to step_cap = 0 as it is. All tables at once
    do (a NaN fuzz or index of refraction gives a NaN direction), and include/hrt.h answers such
    a ray, on a device tree and with tri_bvh = 1, by the triangle test over every triangle in index order, where the heap
    walk misses an all-NaN ray at the root box: the uncapped oracle with that rule (M.STEP_CAP_SAH). Measured on an
    MI355X at 8 frames: against plain step_cap = 0 the draws of all tables differ in 6958 (tris) and 4912 (mixed) channels
    and take 1466723 and 1445696 queries for the oracle's 770460 and 908229; the oracle with the rule gives exactly those
    differences and counts. 2 frames here: a NaN ray costs the oracle every triangle at each of its 50 bounces."""
    from test_gpu_lbvh import device_renderer, on_device

    sd = M.scene(builder, table)
    frames = sd.frames if table == "kinds" else M.SAH_FRAMES
    ref, q = M.oracle(builder, table, frames=frames, step_cap=0 if table == "kinds" else M.STEP_CAP_SAH)
    r = device_renderer(sd, tri_bvh=1)
    if builder_id:
        r.set_triangles_device(on_device(r, sd.bvh[2]), sd.bvh[3], builder=builder_id)
    r.draw_frames(frames, M.TIME0, 10)
    _check(r, ref, q, f"{sd.name} device tree {builder_id}")
