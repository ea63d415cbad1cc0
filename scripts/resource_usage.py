"""Compiler resource usage of every product kernel of the eight device translation units (rt_kernels.hip, rt_regroup.hip, rt_lbvh.hip, rt_ploc.hip, rt_closest.hip, rt_winding.hip, rt_multihit.hip, rt_overlap.hip) (VGPRs, AGPRs, SGPRs, spills, scratch, LDS, occupancy), from
hipcc -Rpass-analysis=kernel-resource-usage with the product flags (hello-raytracing_amd/Makefile).

usage: python scripts/resource_usage.py [extra hipcc flags ...] > profiles/rNN/resource_usage.txt
"""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "--cuda-device-only", "-c"]
KEYS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vgpr_spill"),
        ("SGPRs Spill", "sgpr_spill"), (r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds"),
        (r"Occupancy \[waves/SIMD\]", "waves")]


def main() -> int:
    # one translation unit after the other: rt_kernels.hip's rows first, as before; then rt_regroup.hip's, rt_lbvh.hip's, rt_ploc.hip's, rt_closest.hip's, rt_winding.hip's, rt_multihit.hip's and rt_overlap.hip's
    csrc = ROOT / "hello-raytracing_amd" / "csrc"
    out, cmds = "", []
    for src in (csrc / "rt_kernels.hip", csrc / "rt_regroup.hip", csrc / "rt_lbvh.hip", csrc / "rt_ploc.hip",
                csrc / "rt_closest.hip", csrc / "rt_winding.hip", csrc / "rt_multihit.hip", csrc / "rt_overlap.hip"):
        cmd = ["/opt/rocm/bin/hipcc", *FLAGS, *sys.argv[1:], str(src), "-o", "/tmp/hrt_ru.o",
               "-Rpass-analysis=kernel-resource-usage"]
        out += subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        cmds.append(cmd)
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            sym = m.group(1)
            dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            cur = {"kernel": dem.split("(")[0].replace("void ", "")}
            rows.append(cur)
            continue
        for key, short in KEYS:
            m = re.search(r"\b" + key + r": (\d+)", line)
            if m and cur is not None and short not in cur:
                cur[short] = int(m.group(1))
    cols = ["kernel"] + [s for _, s in KEYS]
    for cmd in cmds:
        print("# " + " ".join(cmd[:-1]))
    print("\t".join(cols))
    for r in rows:
        print("\t".join(str(r.get(c, "")) for c in cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
