"""What test_gpu_kernels.py and test_gpu_material_edges.py share: the rt_params dictionaries that between them select every
kernel instantiation in lib/libhrt.so, by the role of the scene each is drawn on, and the set of instantiations read from
the code object.

Roles: "c3" a sphere scene whose culling BVH fits the LDS nodes, "deep" one of more than 192 nodes, "tris" the triangle
program, and the mixed program over 1 sphere ("c4": the simple scan), 12 ("defer": the deferred scan) and 60 ("bvh": the
culling BVH).
"""
import re
import subprocess
from pathlib import Path

import hrt

LIB = Path(__file__).resolve().parents[1] / "hello-raytracing_amd" / "lib" / "libhrt.so"
ROLES = ("c3", "deep", "tris", "c4", "defer", "bvh")


def library_kernels() -> set:
    """Demangled names of the ray-tracing kernels in the code object (their kernel-descriptor symbols)."""
    data = LIB.read_bytes()
    syms = sorted({m.decode() for m in re.findall(rb"_Z[0-9A-Za-z_]*k_(?:trace|render)[0-9A-Za-z_]*\.kd", data)})
    out = subprocess.run(["c++filt"], input="\n".join(s[:-3] for s in syms), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return {re.sub(r"^void ", "", s.split("(")[0]) for s in out if s.strip()}


def param_cases():
    """[(role, rt_params dictionary)]: one draw each."""
    Q, T = hrt.RT_SCHEDULE_QUEUE, hrt.RT_SCHEDULE_TILES
    cases = []
    for role in ("c3", "deep"):
        for steal in (1, 2):
            for count in (0, 1):
                for packet in ((1, 2) if role == "c3" else (0,)):  # (the packet walk needs the LDS nodes: not the deep tree)
                    cases.append((role, dict(schedule=Q, steal=steal, count_tests=count, packet=packet)))
    for v in (1, 3):
        cases.append(("c3", dict(schedule=Q, variant=v, steal=1)))
    for v in (1, 3, 4):
        cases.append(("c3", dict(schedule=T, variant=v)))
    for role in ("tris", "c4", "defer", "bvh"):
        for heap_lds in (1, 2):
            for steal in (1, 2):
                cases.append((role, dict(schedule=Q, heap_lds=heap_lds, steal=steal)))
        for tri_bvh in (0, 1):
            cases.append((role, dict(schedule=T, tri_bvh=tri_bvh)))
        cases.append((role, dict(schedule=Q, tri_bvh=1)))
    return cases
