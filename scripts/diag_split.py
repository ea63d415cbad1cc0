"""Lane utilisation of k_trace_split's walk and shading phases (diagnostic build counters 5-14).

Run on the GPU box after `make -C hello-raytracing_amd diag`:
    HRT_LIB=lib/libhrt_diag.so python scripts/diag_split.py [--suspend 0 8 16 32] [--hold 0 12]
(--hold: the descent hold, include/hrt_testing.h; default: the renderer's own)
With --leaf, after `make -C hello-raytracing_amd diag HIPEXTRA=-DHRT_LEAFSTAT` (from a clean build directory): the
iterations of the leaf step's first pass and the runs and iterations of its root pass, beside the wave model's figures
(scripts/studies/wave_run.py).
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--suspend", type=int, nargs="+", default=[1, 8, 16, 24, 32, 48])
ap.add_argument("--hold", type=int, nargs="+", default=[None])
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--count-tests", type=int, default=None,
                help="rt_params.count_tests; 0: the uncounted kernel, which answers listed tiles' primary rays when it makes "
                     "their frame block (the box and sphere test figures are then 0; rounds and shade lanes hold)")
ap.add_argument("--steal", type=int, default=None,
                help="rt_params.steal (1: off — a launch that steals runs the stealing kernel, which walks its primary rays)")
ap.add_argument("--leaf", action="store_true",
                help="the library was built with -DHRT_LEAFSTAT too: the leaf step's first-pass and root-pass counts")
a = ap.parse_args()
sd = scenes.config_c3(1920, 1080, a.frames)
for sb, hold in ((sb, hold) for sb in a.suspend for hold in a.hold):
    r = scenes.make_renderer(sd)
    r.set_params(variant=4, schedule=2, suspend_below=sb, **({} if a.count_tests is None else {"count_tests": a.count_tests}), **({} if a.steal is None else {"steal": a.steal}))
    if hold is not None:
        r.set_descent_hold(hold)
    r.draw_frames(sd.frames, 1000, 10)
    st = r.stats()
    c = r.raw_counters()
    if a.leaf:
        lbox, wbox, lleaf, wleaf, lpass1, wpass1, lrun, wrun, lroot, wroot = c[5:15]
        q64 = st.queries / 64.0
        print(f"suspend_below {sb:2d} hold {'default' if hold is None else hold}: {st.trace_ms:8.1f} ms  per 64 queries: "
              f"wave leaf steps {wleaf / q64:.3f} ({lleaf / max(wleaf, 1):.1f} lanes)  first-pass iterations "
              f"{wpass1 / q64:.3f} ({lpass1 / max(wpass1, 1):.1f} lanes, {wpass1 / max(wleaf, 1):.2f} per leaf step)  "
              f"root-pass runs {wrun / q64:.3f} ({lrun / max(wrun, 1):.1f} lanes)  root iterations {wroot / q64:.3f} "
              f"({lroot / max(wroot, 1):.1f} lanes)   [model, wave_run.py --hold 12: leaf steps 2.216, at most 3.74 spheres "
              f"per leaf step, runs 1.98 (13.4 lanes), iterations 2.55]", flush=True)
        continue
    lbox, wbox, lleaf, wleaf, rounds, lshade, wshade, lwalk, wwalk, lentry = c[5:15]
    print(f"suspend_below {sb:2d} hold {'default' if hold is None else hold}: {st.trace_ms:8.1f} ms  box-step util {lbox / max(64 * wbox, 1):.3f}  "
          f"leaf-step util {lleaf / max(64 * wleaf, 1):.3f}  box steps/query {lbox / st.queries:.2f} "
          f"wave box steps/query {64 * wbox / st.queries:.2f}  leaf {lleaf / st.queries:.2f}/{64 * wleaf / st.queries:.2f}  "
          f"rounds/query/64 {64 * rounds / st.queries:.3f}  shading lanes/round {lshade / max(wshade, 1):.1f}  "
          f"walking lanes per walk iteration {lwalk / max(wwalk, 1):.1f}  lanes entering the walk per round "
          f"{lentry / max(rounds, 1):.1f}", flush=True)
