"""Rate of rt_cast_rays on the C3 cover scene's primary rays against the draw that traces the same rays.

Three figures for the closest-hit query, each in rays/s, on one GPU:
  cast_pixel_order   the width x height primary rays of the frame at time 1000, cast in pixel order (ray i = pixel i)
  cast_permuted      the same rays in a fixed random permutation (no two neighbouring lanes share a pixel neighbourhood)
  draw_bounces1      a one-frame bounces = 1 draw on the tiles schedule (k_render: one query per pixel, no ray read, no
                     record written), from rt_stats.trace_ms — the same on any commit that has the tiles schedule

Four more on the same primary rays, for rt_occluded (1 B out per ray instead of 32), timed the same way in the same
alternating windows:
  occluded_any_pixel_order  tmax NULL (any hit at all), rays in pixel order: the figure to hold against cast_pixel_order
  occluded_any_permuted     tmax NULL, the permutation of cast_permuted
  occluded_half_t           tmax = 0.5 x the cast's t: nothing is occluded, so this prices the walk culled by tmax
  occluded_shadow           from each primary hit point, 1e-3 along the returned normal, towards one fixed direction,
                            tmax NULL (one ray per primary hit, in pixel order)
Each carries its bytes per ray (24 B in, + 4 B with a tmax, 1 B out). Outside the timed part every occlusion result is
compared with `cast t < tmax` of the same rays, ray for ray; a difference makes the script exit non-zero.

The casts are timed with device events on the renderer's own stream (rt_get_stream): `--casts` back-to-back calls per
window, `--windows` windows after `--warmup` untimed ones, the two orders alternating window by window; the draw is
timed per draw by the library's events, `--draws` draws after the warm-up. Medians are reported with min and max. A cast
reads 24 B and writes 32 B per ray; the JSON line carries the implied bytes/s beside each rate.

    python scripts/bench_cast.py [--width 1920 --height 1080] [--casts 200] [--windows 9] [--draws 60]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import hrt  # noqa: E402
import scenes  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--casts", type=int, default=200, help="casts per timed window")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=60)
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_cast: no GPU visible (there is no CPU fallback)")
    import torch

    sd = scenes.config_c3(a.width, a.height, 1)
    r = scenes.make_renderer(sd)
    r.set_params(count_tests=0, bounces=1, schedule=hrt.RT_SCHEDULE_TILES)
    dev = torch.device("cuda", r.device()[0])
    n = a.width * a.height
    o, d = (x.view(-1, 3) for x in r.primary_rays(1000))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(20261019)).to(dev)
    rays = {"cast_pixel_order": (o, d), "cast_permuted": (o[perm].contiguous(), d[perm].contiguous())}
    hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
    # the occlusion queries' rays and bounds (name -> origins, directions, tmax or None), from the pixel-order cast
    pix = r.cast_rays(o, d)
    hit = pix["prim"] >= 0
    so = (o[hit] + pix["t"][hit][:, None] * d[hit] + 1e-3 * pix["normal"][hit]).contiguous()
    sdir = torch.tensor([0.4, 1.0, 0.3], dtype=torch.float32, device=dev).expand(so.shape).contiguous()
    occ_rays = {"occluded_any_pixel_order": (o, d, None), "occluded_any_permuted": (*rays["cast_permuted"], None),
                "occluded_half_t": (o, d, (pix["t"] * 0.5).contiguous()), "occluded_shadow": (so, sdir, None)}
    occ = torch.empty((n,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(r.stream(), device=dev)
    L = hrt.lib()

    def call(name):
        if name in rays:
            ro, rd = rays[name]
            hrt._lib.check(L.rt_cast_rays(r._h, C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()), n,
                                          C.c_void_p(hits.data_ptr())), "rt_cast_rays")
        else:
            ro, rd, tm = occ_rays[name]
            hrt._lib.check(L.rt_occluded(r._h, C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()),
                                         C.c_void_p(tm.data_ptr()) if tm is not None else None, ro.shape[0],
                                         C.c_void_p(occ.data_ptr())), "rt_occluded")

    def window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.casts):
            call(name)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.casts  # ms per cast

    names = list(rays) + list(occ_rays)
    ms = {k: [] for k in names}
    for w in range(a.warmup + a.windows):
        for name in names:
            t = window(name)
            if w >= a.warmup:
                ms[name].append(t)
    # every occlusion result is `cast t < tmax` of the same rays, ray for ray (an absent tmax: RT_T_MISS)
    occ_same, occ_fraction = {}, {}
    for name, (ro, rd, tm) in occ_rays.items():
        ref = pix if ro is o else r.cast_rays(ro, rd)
        bound = tm if tm is not None else torch.full_like(ref["t"], hrt.RT_T_MISS)
        got = r.occluded(ro, rd, tm)
        occ_same[name] = bool((got == ((ref["prim"] >= 0) & (ref["t"] < bound))).all())
        occ_fraction[name] = float(got.float().mean())
    # the permuted cast finds the same hits, ray for ray
    per = r.cast_rays(*rays["cast_permuted"])
    same = all(bool((per[k] == pix[k][perm]).all()) for k in ("prim", "flags", "material")) and \
        bool((per["t"].view(torch.int32) == pix["t"][perm].view(torch.int32)).all())
    hit_fraction = float((pix["prim"] >= 0).float().mean())

    draw_ms, queries = [], 0
    for k in range(a.warmup + a.draws):
        r.draw_frames(1, 1000, 10)
        st = r.stats()
        if k >= a.warmup:
            draw_ms.append(st.trace_ms)
            queries = st.queries
    kernel = st.kernel.decode()

    def rate(rays_per, times):
        med = statistics.median(times)
        return {"rays_per_s": rays_per / (med * 1e-3), "ms_median": med, "ms_min": min(times), "ms_max": max(times),
                "samples": len(times)}

    out = {"scene": sd.name, "width": a.width, "height": a.height, "rays": n, "hit_fraction": hit_fraction,
           "permuted_equals_pixel_order": same, "casts_per_window": a.casts, "draw_kernel": kernel,
           "draw_queries": int(queries), "occluded_equals_cast": all(occ_same.values())}
    for name in rays:
        out[name] = rate(n, ms[name])
        out[name]["bytes_per_s"] = out[name]["rays_per_s"] * 56.0
    for name, (ro, _, tm) in occ_rays.items():
        out[name] = rate(int(ro.shape[0]), ms[name])
        out[name].update(rays=int(ro.shape[0]), bytes_per_ray=25 if tm is None else 29, equals_cast=occ_same[name],
                         occluded_fraction=occ_fraction[name])
        out[name]["bytes_per_s"] = out[name]["rays_per_s"] * out[name]["bytes_per_ray"]
    out["draw_bounces1"] = rate(queries, draw_ms)
    print(json.dumps(out))
    return 0 if same and all(occ_same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
