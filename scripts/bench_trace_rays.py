"""Rate of rt_trace_rays on the C3 cover scene's primary rays against the one-frame draw that traces the same paths.

The workload is the C3 scene at 1920x1080 with its 50 bounces and the primary rays and RNG states of time 1000
(rt_primary_rays, rt_primary_rng), so every figure traces the same paths:
  trace_pixel_order  rt_trace_rays on the rays in pixel order (ray i = pixel i)
  trace_permuted     the same rays and states in bench_cast.py's fixed permutation
  draw_one_frame     a one-frame draw on the tiles schedule (k_render: no ray read, no radiance written, a wave per 8x8
                     tile), from rt_stats.trace_ms — the yardstick, and the same on any commit with the tiles schedule
Each is given in paths/s (rays traced per second) and rays/s (closest-hit queries per second: the draw's ray count, which
the traced paths' queries must sum to). A traced ray reads 28 B (origin, direction, state) and writes 12 B, 16 B with the
queries (--queries); the JSON line carries bytes per ray and the ratio to draw_one_frame.

`--rays-per-lane` lists the values of k_radiance_rays' R to time (include/hrt_testing.h rt_testing_set_trace_rays_per_lane;
0 = the host's rule); all of them are timed in the same process, window by window in turn, with device events on the
renderer's own stream: `--calls` back-to-back calls per window, `--windows` windows after `--warmup` untimed ones. The
draw is timed per draw by the library's events. Medians are reported with min and max.

Outside the timed part, for every R and both orders, the traced frame must equal the drawn frame (one frame from a zeroed
image at frame count 0) bit for bit and the queries must sum to the draw's ray count, or the script exits non-zero.

    python scripts/bench_trace_rays.py [--width 1920 --height 1080] [--rays-per-lane 0,1,2,4,8,16] [--calls 20]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import hrt  # noqa: E402
import scenes  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays-per-lane", default="0,1,2,4,8,16", help="values of R to time, 0 = the host's rule")
    ap.add_argument("--calls", type=int, default=20, help="rt_trace_rays calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=40)
    ap.add_argument("--queries", action="store_true", help="time the calls with a queries buffer (16 B out per ray)")
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_trace_rays: no GPU visible (there is no CPU fallback)")
    import torch

    sd = scenes.config_c3(a.width, a.height, 1)
    r = scenes.make_renderer(sd)
    r.set_params(count_tests=0, schedule=hrt.RT_SCHEDULE_TILES)
    dev = torch.device("cuda", r.device()[0])
    n = a.width * a.height
    o, d = (x.view(-1, 3) for x in r.primary_rays(1000))
    s = r.primary_rng(1000).view(-1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(20261019)).to(dev)
    rays = {"trace_pixel_order": (o, d, s),
            "trace_permuted": (o[perm].contiguous(), d[perm].contiguous(), s[perm].contiguous())}
    rad = torch.empty((n, 3), dtype=torch.float32, device=dev)
    qbuf = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(r.stream(), device=dev)
    L = hrt.lib()
    Rs = [int(x) for x in a.rays_per_lane.split(",")]

    def call(name):
        ro, rd, rs = rays[name]
        hrt._lib.check(L.rt_trace_rays(r._h, C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()),
                                       C.c_void_p(rs.data_ptr()), 0, n, C.c_void_p(rad.data_ptr()),
                                       C.c_void_p(qbuf.data_ptr()) if a.queries else None), "rt_trace_rays")

    def window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            call(name)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls  # ms per call

    ms = {(R, name): [] for R in Rs for name in rays}
    for w in range(a.warmup + a.windows):
        for R in Rs:
            r.set_trace_rays_per_lane(R)
            for name in rays:
                t = window(name)
                if w >= a.warmup:
                    ms[(R, name)].append(t)

    # the yardstick, and the frame every traced result must reproduce
    draw_ms, queries = [], 0
    for k in range(a.warmup + a.draws):
        r.write_image(np.zeros((a.height, a.width, 3), np.float32))
        r.set_frame_count(0)
        r.draw_frames(1, 1000, 10)
        st = r.stats()
        if k >= a.warmup:
            draw_ms.append(st.trace_ms)
            queries = int(st.queries)
    kernel = st.kernel.decode()
    frame = torch.from_numpy(r.read_image()).view(-1, 3).view(torch.int32)
    same = {}
    for R in Rs:
        r.set_trace_rays_per_lane(R)
        for name, (ro, rd, rs) in rays.items():
            got, q = r.trace_rays(ro, rd, rng=rs, want_queries=True)
            want = frame if name == "trace_pixel_order" else frame[perm.cpu()]
            same[f"{name}@R{R}"] = bool((got.cpu().view(torch.int32) == want).all()) and int(q.sum()) == queries
    r.set_trace_rays_per_lane(0)

    def rate(times):
        med = statistics.median(times)
        return {"paths_per_s": n / (med * 1e-3), "rays_per_s": queries / (med * 1e-3), "ms_median": med,
                "ms_min": min(times), "ms_max": max(times), "samples": len(times)}

    out = {"scene": sd.name, "width": a.width, "height": a.height, "paths": n, "bounces": sd.bounces, "queries": queries,
           "queries_per_path": queries / n, "calls_per_window": a.calls, "draw_kernel": kernel,
           "bytes_per_ray": 28 + (16 if a.queries else 12), "traced_equals_drawn": all(same.values()),
           "draw_one_frame": rate(draw_ms), "rays_per_lane": {}}
    base = out["draw_one_frame"]["ms_median"]
    for R in Rs:
        row = {}
        for name in rays:
            row[name] = rate(ms[(R, name)])
            row[name]["ratio_to_draw"] = base / row[name]["ms_median"]
            row[name]["equals_drawn"] = same[f"{name}@R{R}"]
        out["rays_per_lane"][str(R)] = row
    print(json.dumps(out))
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
