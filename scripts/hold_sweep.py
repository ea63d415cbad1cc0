"""Sweep of the descent hold (include/hrt_testing.h rt_testing_set_descent_hold) against suspend_below on a bench
config, one process, the settings interleaved round by round (same box, same clocks). Per setting and round: one
warm-up draw (the sample queue learns its cost order), then `--steps` timed draws with count_tests 0; the figure is
the kernels' event time (rt_stats.kernel_ms), the rate is queries over it.

    python scripts/hold_sweep.py [--config c3] [--hold 0 6 8 12 16 24] [--suspend 16 20 24] [--rounds 2]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c3", choices=["c3", "c5"])
ap.add_argument("--hold", type=int, nargs="+", default=[0, 6, 8, 12, 16, 24])
ap.add_argument("--suspend", type=int, nargs="+", default=[16, 20, 24])
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--frames", type=int, default=None)
ap.add_argument("--width", type=int, default=None)
ap.add_argument("--height", type=int, default=None)
a = ap.parse_args()
sd = scenes.CONFIGS[a.config]()
sd.frames = a.frames or sd.frames
sd.width, sd.height = a.width or sd.width, a.height or sd.height
res = {}
for rnd in range(a.rounds):
    for sb in a.suspend:
        for hold in a.hold:
            r = scenes.make_renderer(sd)
            r.set_params(suspend_below=sb, count_tests=0)
            r.set_descent_hold(hold)
            r.draw_frames(sd.frames, 1000, 10)
            for _ in range(a.steps):
                r.draw_frames(sd.frames, 1000, 10)
                st = r.stats()
                res.setdefault((sb, hold), []).append((st.kernel_ms, st.queries / st.kernel_ms / 1e6))
            ms, gr = res[(sb, hold)][-1]
            print(f"round {rnd} suspend_below {sb:2d} hold {hold:2d}: {ms:8.2f} ms {gr:7.3f} Grays/s  {st.kernel.decode()}",
                  flush=True)
            del r
print("\nsuspend_below hold  mean_ms  min_ms  max_ms  mean_Grays/s  vs hold 0 of the same suspend_below")
for sb in a.suspend:
    base = statistics.mean(m for m, _ in res[(sb, a.hold[0])])
    for hold in a.hold:
        ms = [m for m, _ in res[(sb, hold)]]
        gr = statistics.mean(g for _, g in res[(sb, hold)])
        print(f"{sb:13d} {hold:4d} {statistics.mean(ms):8.2f} {min(ms):7.2f} {max(ms):7.2f} {gr:13.3f}  "
              f"{100.0 * (base / statistics.mean(ms) - 1.0):+6.2f} %")
