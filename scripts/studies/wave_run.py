"""Driver of scripts/studies/wave_sim.cpp (round-7 study: the wave-lockstep model of k_trace_split).

usage: python scripts/studies/wave_run.py [--config c3] [--waves 40] [--jobs 6] [--suspend 24] [--hold 0 8 12 ...]
       python scripts/studies/wave_run.py --hold 12 --cand-hold 0/0 8/1 12/1 16/2 24/4 64/2   
       python scripts/studies/wave_run.py --hold 12 --block-time 0 1            
       python scripts/studies/wave_run.py --calibrate      (suspend_below 24, hold 0 against the GPU's diagnostic counters)
Builds the simulator with g++ into a temporary directory, writes the scene beside it and prints the simulator's counts
per setting; with several settings, a table of the wave's box steps, lanes per box step and the modelled issue cost.
--block-time 1 answers and shades a listed tile's primary rays when their block is made; the lists' lengths are
rt_host_tile_lists's (the built library's host mirror, no GPU).
--calibrate compares six figures with scripts/diag_split.py's committed counters (profiles/r05/diag_c/diag_split_c3.log,
the suspend_below 24 line) and fails when one is off by more than 5 %.
"""
import argparse
import json
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import numpy as np  # noqa: E402
import scenes  # noqa: E402

DIAG_LOG = ROOT / "profiles" / "r05" / "diag_c" / "diag_split_c3.log"

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c3")
ap.add_argument("--waves", type=int, default=40)
ap.add_argument("--jobs", type=int, default=6)
ap.add_argument("--job-frames", type=int, default=32)
ap.add_argument("--suspend", type=int, nargs="+", default=[24])
ap.add_argument("--hold", type=int, nargs="+", default=[0])
ap.add_argument("--cand-hold", nargs="+", default=["0/0"], metavar="CHOLD/CWAIT",
                help="the candidate hold priced in round 10 (0/0 = none): the root pass waits for CHOLD lanes with a "
                     "candidate, at most CWAIT iterations")
ap.add_argument("--block-time", type=int, nargs="+", default=[0], choices=[0, 1],
                help="1: primary rays of listed tiles answered and shaded when their block is made (round 13)")
ap.add_argument("--calibrate", action="store_true")
a = ap.parse_args()
if a.calibrate:
    a.suspend, a.hold, a.cand_hold, a.block_time = [24], [0], ["0/0"], [0]

sd = scenes.CONFIGS[a.config]()
assert sd.bvh is None, "the model is of the sphere program"
cam = np.ascontiguousarray(sd.camera).tobytes()
sph = np.ascontiguousarray(sd.spheres).tobytes()
assert len(cam) == 80 and len(sph) % 48 == 0
rows = []
with tempfile.TemporaryDirectory() as tmp:
    exe, scene = Path(tmp) / "wave_sim", Path(tmp) / "scene.bin"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-I", str(ROOT / "hello-raytracing_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "scripts" / "studies" / "wave_sim.cpp"),
                    str(ROOT / "hello-raytracing_amd" / "csrc" / "host" / "sphere_bvh.cpp")], check=True)
    scene.write_bytes(cam + struct.pack("<I", len(sph) // 48) + sph)
    lens = Path(tmp) / "tile_list_lengths.bin"
    if 1 in a.block_time:
        import hrt  # noqa: E402

        lists = hrt.host_tile_lists(sd.camera, sd.width, sd.height, sd.spheres)
        lens.write_bytes(np.ascontiguousarray(lists[:, 0], dtype=np.uint32).tobytes())
        listed = lists[lists[:, 0] != 0xFFFFFFFF, 0]
        print(f"tile lists (rt_host_tile_lists): {len(lists)} tiles, {len(lists) - len(listed)} walk, mean length "
              f"{listed.mean():.3f}, max {listed.max()}\n")
    for sb in a.suspend:
        for hold in a.hold:
            for ch in a.cand_hold:
                for bt in a.block_time:
                    chold, cwait = ch.split("/")
                    out = subprocess.run([str(exe), str(scene), str(sd.width), str(sd.height), str(sd.bounces or 50),
                                          str(a.waves), str(a.jobs), str(sb), str(hold), str(a.job_frames), chold, cwait,
                                          str(bt), str(lens)], capture_output=True, text=True, check=True).stdout
                    print(out.split("\nJSON ", 1)[0] + "\n")
                    rows.append(json.loads(out.split("\nJSON ", 1)[1]))

if len(rows) > 1:
    base = rows[0]
    print("suspend_below hold chold/cwait block  rounds / 64 q  wave box steps / 64 q  lanes / box step  root runs / 64 q  lanes / run  "
          "issue cost / query  vs the first row")
    for r in rows:
        ch = f"{r['chold']}/{r['cwait']}"
        print(f"{r['suspend_below']:13d} {r['hold']:4d} {ch:>11s} {r['blocktime']:5d} {r['rounds_per_64q']:14.3f} "
              f"{r['wave_box_per_64q']:22.2f} {r['box_lanes']:17.1f} "
              f"{r['root_runs_per_64q']:16.2f} {r['root_lanes']:11.1f} "
              f"{r['cost_per_query']:19.3f} {100.0 * (r['cost_per_query'] / base['cost_per_query'] - 1.0):+15.1f} %")

if a.calibrate:
    line = next(ln for ln in DIAG_LOG.read_text().splitlines() if ln.startswith("suspend_below 24"))

    def num(pat):
        return float(re.search(pat, line).group(1))

    box_util, leaf_util = num(r"box-step util ([\d.]+)"), num(r"leaf-step util ([\d.]+)")
    gpu = {"walk_lanes": num(r"walking lanes per walk iteration ([\d.]+)"), "box_lanes": 64.0 * box_util,
           "leaf_lanes": 64.0 * leaf_util, "shade_lanes": num(r"shading lanes/round ([\d.]+)"),
           "wave_box_per_64q": num(r"wave box steps/query ([\d.]+)"), "lane_box_per_q": num(r"box steps/query ([\d.]+)")}
    names = {"walk_lanes": "walking lanes per walk iteration", "box_lanes": "lanes per box step",
             "leaf_lanes": "lanes per leaf step", "shade_lanes": "shading lanes per round",
             "wave_box_per_64q": "wave box steps per 64 queries", "lane_box_per_q": "lane box steps per query"}
    r, bad = rows[0], []
    print(f"calibration against {DIAG_LOG.relative_to(ROOT)} (suspend_below 24, no hold)")
    print(f"{'':34s} {'model':>8s} {'GPU diag':>9s} {'off':>7s}")
    for k, name in names.items():
        off = r[k] / gpu[k] - 1.0
        print(f"{name:34s} {r[k]:8.2f} {gpu[k]:9.2f} {100.0 * off:+6.1f} %")
        if abs(off) > 0.05:
            bad.append(name)
    print(f"phase shares (model): refill {r['share_refill']:.3f} begin {r['share_begin']:.3f} walk {r['share_walk']:.3f} "
          f"shade {r['share_shade']:.3f}   (measured phase split, DESIGN.md §4 Round 6: 0.116 0.118 0.583 0.183)")
    if bad:
        sys.exit("calibration off by more than 5 %: " + ", ".join(bad))
