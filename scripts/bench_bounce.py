"""Cost of the wavefront path loop (rt_bounce_rays step by step) against the megakernel (rt_trace_rays) on the same paths.

The workload is the C3 scene at 1920x1080 with its 50 bounces and the primary rays and RNG states of time 1000
(rt_primary_rays, rt_primary_rng), so every figure traces the same paths:
  wavefront_loop  `bounces` rt_bounce_rays steps with throughput, two (index, count) pairs and count_in chaining — every
                  step launched for all n entries, no host read-back — timed from the first step to the last
  trace_rays      one rt_trace_rays call on the same rays and states, in the same windows (the megakernel)
  step1           the first step alone (all n paths, throughput, index_out and count_out, no hits) ...
  step1_plain     ... the same without index_out and count_out (no ballot, no atomic, no index store) ...
  cast_rays       ... beside rt_cast_rays on the same rays (the same query; 32-B records instead of the scatter)
  steps           per step: ms and the number of entries it processed (the survivors of the step before)
All times are device events on the renderer's own stream; the state is reset (copies on that stream) outside the timed
part. `--windows` windows after `--warmup` untimed ones; medians with min and max. The per-step figures come from loops
of their own, with an event between every two steps.

Outside the timed part the loop's throughput * sky must equal rt_trace_rays' radiance bit for bit, or the script exits
non-zero.

    python scripts/bench_bounce.py [--width 1920 --height 1080] [--windows 9] [--queries]
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
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", action="store_true", help="the steps and rt_trace_rays also count queries per path")
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_bounce: no GPU visible (there is no CPU fallback)")
    import torch

    sd = scenes.config_c3(a.width, a.height, 1)
    r = scenes.make_renderer(sd)
    r.set_params(count_tests=0)
    bounces = sd.bounces
    dev = torch.device("cuda", r.device()[0])
    n = a.width * a.height
    o0, d0 = (x.view(-1, 3) for x in r.primary_rays(1000))
    s0 = r.primary_rng(1000).view(-1)
    i32, f32 = torch.int32, torch.float32
    o, d, s = torch.empty_like(o0), torch.empty_like(d0), torch.empty_like(s0)
    att = torch.empty((n, 3), dtype=f32, device=dev)
    q = torch.empty((n,), dtype=i32, device=dev)
    index = [torch.empty((n,), dtype=i32, device=dev) for _ in range(2)]
    count = [torch.zeros((1,), dtype=i32, device=dev) for _ in range(2)]
    counts = torch.zeros((bounces,), dtype=i32, device=dev)
    rad = torch.empty((n, 3), dtype=f32, device=dev)
    qbuf = torch.empty((n,), dtype=i32, device=dev)
    hits = torch.empty((n, 8), dtype=i32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(r.stream(), device=dev)
    L, E = hrt.lib(), hrt._lib

    def ptr(t):
        return t.data_ptr() if t is not None else None

    def reset():
        with torch.cuda.stream(stream):
            o.copy_(o0)
            d.copy_(d0)
            s.copy_(s0)
            att.fill_(1.0)
            q.zero_()

    def step(k, compact=True):
        src, dst = (k + 1) & 1, k & 1
        io = E.RtBounce(ptr(o), ptr(d), ptr(s), ptr(att), ptr(q) if a.queries else None, None,
                        ptr(index[src]) if k else None, ptr(count[src]) if k else None,
                        ptr(index[dst]) if compact else None, ptr(count[dst]) if compact else None, n, 0)
        E.check(L.rt_bounce_rays(r._h, C.byref(io), n), "rt_bounce_rays")
        return dst

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def timed(fn):
        e0 = event()
        fn()
        e1 = event()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def loop():
        for k in range(bounces):
            step(k)

    def trace():
        E.check(L.rt_trace_rays(r._h, C.c_void_p(o0.data_ptr()), C.c_void_p(d0.data_ptr()), C.c_void_p(s0.data_ptr()), 0, n,
                                C.c_void_p(rad.data_ptr()), C.c_void_p(qbuf.data_ptr()) if a.queries else None),
                "rt_trace_rays")

    def cast():
        E.check(L.rt_cast_rays(r._h, C.c_void_p(o0.data_ptr()), C.c_void_p(d0.data_ptr()), n, C.c_void_p(hits.data_ptr())),
                "rt_cast_rays")

    def per_step():
        ev = [event()]
        for k in range(bounces):
            dst = step(k)
            with torch.cuda.stream(stream):
                counts[k].copy_(count[dst][0])
            ev.append(event())
        ev[-1].synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(bounces)]

    ms = {"wavefront_loop": [], "trace_rays": [], "step1": [], "step1_plain": [], "cast_rays": []}
    step_ms = []
    for w in range(a.warmup + a.windows):
        t = {}
        reset()
        t["wavefront_loop"] = timed(loop)
        t["trace_rays"] = timed(trace)
        reset()
        t["step1"] = timed(lambda: step(0))
        t["cast_rays"] = timed(cast)
        reset()
        t["step1_plain"] = timed(lambda: step(0, compact=False))
        reset()
        per = per_step()  # (the event and the count copy between the steps are in each step's figure)
        if w >= a.warmup:
            for k, v in t.items():
                ms[k].append(v)
            step_ms.append(per)
    survivors = counts.cpu().tolist()

    # the loop's result against the megakernel's
    r.set_params(bounces=bounces)
    reset()
    loop()
    r.synchronize()
    t = d0[:, 1] * 0.5 + 0.5
    u = 1.0 - t
    sky = torch.stack((0.54 * u + 0.54 * t, 0.86 * u + 0.7 * t, 0.92 * u + 0.98 * t), dim=1)
    got = 0.0 + att * sky
    want, wq = r.trace_rays(o0, d0, rng=s0, want_queries=True)
    same = bool((got.view(i32) == want.view(i32)).all())
    if a.queries:
        same = same and bool((q == wq).all())
    queries = int(wq.sum())

    def stat(times):
        return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "samples": len(times)}

    out = {"scene": sd.name, "width": a.width, "height": a.height, "paths": n, "bounces": bounces, "queries": queries,
           "with_queries": bool(a.queries), "wavefront_equals_trace_rays": same}
    for k, v in ms.items():
        out[k] = stat(v)
    out["wavefront_over_trace_rays"] = out["wavefront_loop"]["ms_median"] / out["trace_rays"]["ms_median"]
    out["step1_over_cast_rays"] = out["step1"]["ms_median"] / out["cast_rays"]["ms_median"]
    entries = [n] + survivors[:-1]
    out["steps"] = [{"step": k + 1, "entries": entries[k], "survivors": survivors[k],
                     "ms_median": statistics.median(x[k] for x in step_ms), "ms_min": min(x[k] for x in step_ms),
                     "ms_max": max(x[k] for x in step_ms)} for k in range(bounces)]
    out["steps_ms_sum"] = sum(x["ms_median"] for x in out["steps"])
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
