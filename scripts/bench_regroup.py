"""Does regrouping pay? The wavefront path loop (rt_bounce_rays step by step) with rt_regroup_paths between steps, against
the plain loop, on the same paths.

The workload is bench_bounce.py's: the C3 scene at 1920x1080 with its 50 bounces and the primary rays and RNG states of
time 1000. The box of the cell-and-octant key is lo = (-12, -0.5, -12), hi = (12, 2.5, 12): the grid of small spheres
and the three big ones, not the r = 1000 ground. Figures, all from this one process, the variants interleaved in the same
windows:
  loop_plain        the plain loop (bench_bounce.py's wavefront_loop, measured again here)
  loop_regroup_1    the loop with a regroup (in place, mode 1) after step 1 only
  loop_regroup_1_3  ... after each of steps 1 to 3
  loop_regroup_all  ... after every step
  at_step           for steps 1, 2, 3, 5, 10, 20, on the entries that step processes in the plain loop (arrival order):
                    rt_regroup_paths alone in mode 1 and in mode 2 (the paths' RNG states as keys: 32 arbitrary bits),
                    into a separate list so the state stays put, beside the rt_bounce_rays step itself
  step2             step 2 alone on the arrival-order list of step 1's survivors, and on the same list regrouped
All times are device events on the renderer's own stream; state is reset or restored (copies on that stream) outside
the timed part. `--windows` windows after `--warmup` untimed ones; medians with min and max.

Outside the timed part every loop's throughput * sky must equal rt_trace_rays' radiance bit for bit, or the script exits
non-zero.

    python scripts/bench_regroup.py [--width 1920 --height 1080] [--windows 9]
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

BOX = ((-12.0, -0.5, -12.0), (12.0, 2.5, 12.0))
AT_STEPS = (1, 2, 3, 5, 10, 20)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_regroup: no GPU visible (there is no CPU fallback)")
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
    saved = [torch.empty_like(x) for x in (o, d, s, att)]  # the state after step 1 (step2)
    index = [torch.empty((n,), dtype=i32, device=dev) for _ in range(2)]
    count = [torch.zeros((1,), dtype=i32, device=dev) for _ in range(2)]
    side_index = torch.empty((n,), dtype=i32, device=dev)  # a regroup's output when the loop's own list must stay
    entries_seen = torch.zeros((bounces + 1,), dtype=i32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(r.stream(), device=dev)
    L, E = hrt.lib(), hrt._lib
    lo, hi = ((C.c_float * 3)(*v) for v in BOX)

    def ptr(t):
        return t.data_ptr() if t is not None else None

    def reset():
        with torch.cuda.stream(stream):
            o.copy_(o0)
            d.copy_(d0)
            s.copy_(s0)
            att.fill_(1.0)

    def step(k, index_in=None):
        """Step k (0-based) of the loop; index_in replaces the list the step before left."""
        src, dst = (k + 1) & 1, k & 1
        if index_in is None and k:
            index_in = index[src]
        io = E.RtBounce(ptr(o), ptr(d), ptr(s), ptr(att), None, None, ptr(index_in), ptr(count[src]) if k else None,
                        ptr(index[dst]), ptr(count[dst]), n, 0)
        E.check(L.rt_bounce_rays(r._h, C.byref(io), n), "rt_bounce_rays")
        return dst

    def regroup(index_in, count_in, index_out, mode=E.REGROUP_CELL_OCTANT):
        g = E.RtRegroup(ptr(o), ptr(d), ptr(s), ptr(index_in), ptr(count_in), ptr(index_out), None, n, mode, lo, hi, 0, 0)
        E.check(L.rt_regroup_paths(r._h, C.byref(g), n), "rt_regroup_paths")

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

    def loop(after=()):
        for k in range(bounces):
            dst = step(k)
            if k + 1 in after:
                regroup(index[dst], count[dst], index[dst])

    VARIANTS = {"loop_plain": (), "loop_regroup_1": (1,), "loop_regroup_1_3": (1, 2, 3),
                "loop_regroup_all": tuple(range(1, bounces + 1))}

    def at_steps():
        """One plain loop; before each step of AT_STEPS, on that step's entries: regroup mode 1, regroup mode 2, then
        the step itself, each between two events."""
        out = {}
        for k in range(bounces):
            src = (k + 1) & 1
            if k + 1 in AT_STEPS:
                ii, ci = (index[src], count[src]) if k else (None, None)
                with torch.cuda.stream(stream):
                    if k:
                        entries_seen[k + 1].copy_(count[src][0])
                    else:
                        entries_seen[1].fill_(n)
                ev = [event()]
                regroup(ii, ci, side_index, E.REGROUP_CELL_OCTANT)
                ev.append(event())
                regroup(ii, ci, side_index, E.REGROUP_KEYS)
                ev.append(event())
                step(k)
                ev.append(event())
                out[k + 1] = ev
            else:
                step(k)
        r.synchronize()
        return {k: [ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for k, ev in out.items()}

    def step2(regrouped):
        """Step 2 alone, from the saved state after step 1, on the arrival-order list or on the regrouped one."""
        with torch.cuda.stream(stream):
            for x, y in zip((o, d, s, att), saved):
                x.copy_(y)
        ii = index[0]
        if regrouped:
            regroup(index[0], count[0], side_index)
            ii = side_index
        return timed(lambda: step(1, index_in=ii))

    ms = {k: [] for k in VARIANTS}
    ms.update({"step2_arrival": [], "step2_regrouped": []})
    at = {k: [] for k in AT_STEPS if k <= bounces}
    for w in range(a.warmup + a.windows):
        t = {}
        for name, after in VARIANTS.items():
            reset()
            t[name] = timed(lambda: loop(after))
        reset()
        per = at_steps()
        reset()
        step(0)
        with torch.cuda.stream(stream):
            for x, y in zip((o, d, s, att), saved):
                y.copy_(x)
        t["step2_arrival"] = step2(False)
        t["step2_regrouped"] = step2(True)
        if w >= a.warmup:
            for k, v in t.items():
                ms[k].append(v)
            for k, v in per.items():
                at[k].append(v)
    entries = entries_seen.cpu().tolist()

    # every loop's result against the megakernel's
    r.set_params(bounces=bounces)
    want = r.trace_rays(o0, d0, rng=s0)
    t = d0[:, 1] * 0.5 + 0.5
    u = 1.0 - t
    sky = torch.stack((0.54 * u + 0.54 * t, 0.86 * u + 0.7 * t, 0.92 * u + 0.98 * t), dim=1)
    same = {}
    for name, after in VARIANTS.items():
        reset()
        loop(after)
        r.synchronize()
        got = 0.0 + att * sky
        same[name] = bool((got.view(i32) == want.view(i32)).all())

    def stat(times):
        return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "samples": len(times)}

    out = {"scene": sd.name, "width": a.width, "height": a.height, "paths": n, "bounces": bounces,
           "box": BOX, "tile": E.REGROUP_TILE, "loops_equal_trace_rays": same}
    for k, v in ms.items():
        out[k] = stat(v)
    for k in VARIANTS:
        out[k]["over_plain"] = out[k]["ms_median"] / out["loop_plain"]["ms_median"]
    out["step2_regrouped_over_arrival"] = out["step2_regrouped"]["ms_median"] / out["step2_arrival"]["ms_median"]
    out["at_step"] = [{"step": k, "entries": entries[k],
                       "regroup_cell_octant": stat([x[0] for x in v]), "regroup_keys": stat([x[1] for x in v]),
                       "bounce_step": stat([x[2] for x in v])} for k, v in sorted(at.items())]
    print(json.dumps(out))
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
