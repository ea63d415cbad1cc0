"""What a deforming mesh pays per step with rt_refit_triangles_device instead of rt_set_triangles_device, and what its
rays pay afterwards, on Suzanne (979 triangles), lucy_lp_20 (19,917) and xyzrgb_dragon_lp_20 (49,976), each mesh alone in
the triangle program (the meshes and cameras of scripts/bench_lbvh.py).

Per mesh, on one GPU:
  rebuild_ms, refit_ms   wall time of one rt_set_triangles_device and of one rt_refit_triangles_device call (host clock;
                         both calls are synchronous) on the SAME renderer and the same triangles, already in a torch
                         tensor on the device: `--builds` windows alternating between the two after `--warmup` untimed ones
  per deformation (applied to the undeformed mesh, in f32 on the device):
    smooth   a twist about the y axis, a quarter turn over the mesh height
    rough    every triangle displaced by its own vector of length a tenth of the largest root extent
    cast_refit_ms, cast_rebuilt_ms   rt_cast_rays on the width x height primary rays of the frame at time 1000 through
                         the tree built for the undeformed mesh and refitted, and through a tree built for the deformed
                         mesh (two renderers): device events on each renderer's stream, `--casts` back-to-back calls per
                         window, `--windows` windows alternating between the two after `--warmup` untimed ones
    cost_refit, cost_rebuilt         rt_get_tri_tree_cost of both trees beside them; sah = (cost[0] + cost[1]) / 65536
  cost_lbvh, cost_host_sah            the cost of the LBVH and of the host's binned-SAH tree for the undeformed mesh
Medians with min and max. Outside the timed part the two casts are compared record for record (the hit contract does not
depend on the tree); a difference makes the script exit non-zero. One JSON line.

    python scripts/bench_refit.py [--width 1920 --height 1080] [--builds 20] [--casts 20] [--windows 7]
"""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests", ROOT / "scripts"):
    sys.path.insert(0, str(p))
import numpy as np  # noqa: E402

import hrt  # noqa: E402
from hrt import Material, Mesh, Tree, Vec3, read_asset  # noqa: E402
from bench_lbvh import MESHES, spread  # noqa: E402


def cost_dict(cost) -> dict:
    c = [int(x) for x in cost]
    return {"words": c, "sah": (c[0] + c[1]) / 65536.0}


def deformed(t, kind: str):
    """t: (m, 16) float32 on the device (a.xyzw, b.xyzw, c.xyzw, custom.xyz, material); a moved copy."""
    import torch

    out = t.clone()
    pos = torch.stack([t[:, 0:3], t[:, 4:7], t[:, 8:11]], dim=1)  # (m, 3, 3)
    lo, hi = pos.amin(dim=(0, 1)), pos.amax(dim=(0, 1))
    if kind == "smooth":
        angle = (pos[..., 1] - lo[1]) / (hi[1] - lo[1]) * (0.5 * math.pi)
        cx, cz = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[2] + hi[2])
        x, z = pos[..., 0] - cx, pos[..., 2] - cz
        moved = torch.stack([cx + x * torch.cos(angle) + z * torch.sin(angle), pos[..., 1],
                             cz - x * torch.sin(angle) + z * torch.cos(angle)], dim=-1)
    else:
        g = torch.Generator(device=t.device)
        g.manual_seed(20261020)
        v = torch.randn((len(t), 1, 3), generator=g, device=t.device, dtype=torch.float32)
        v = v / v.norm(dim=-1, keepdim=True) * (0.1 * float((hi - lo).max()))
        moved = pos + v
    for k, c in enumerate((0, 4, 8)):
        out[:, c:c + 3] = moved[:, k]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--casts", type=int, default=20, help="casts per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--meshes", default=",".join(MESHES))
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_refit: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    n = a.width * a.height
    out = {"width": a.width, "height": a.height, "rays": n, "library": str(hrt.LIB_PATH.name), "meshes": {}}
    ok = True
    for name in a.meshes.split(","):
        asset, camera = MESHES[name]
        tree = Tree.from_mesh(Mesh.load_obj(read_asset(asset), Material.new_lambertian(Vec3(0.5, 0.5, 0.6))))
        tree.build()
        sizes, nodes, tris, mats = tree.view()
        res = {"triangles": int(len(tris))}

        def renderer():
            r = hrt.Renderer(a.width, a.height, hrt.RT_MODE_TRIS)
            r.set_params(count_tests=0)
            r.set_camera(camera())
            return r

        ra, rb = renderer(), renderer()  # ra: built for the undeformed mesh and refitted; rb: built for each deformed mesh
        dev = torch.device("cuda", ra.device()[0])
        t0_dev = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).copy()).to(dev).view(torch.float32)
        torch.cuda.synchronize(dev)
        ptr, m = C.c_void_p(t0_dev.data_ptr()), len(tris)
        # ---- refit against rebuild, alternating, on one renderer
        ra.set_triangles_device(t0_dev, mats)
        ms = {"rebuild_ms": [], "refit_ms": []}
        for k in range(a.warmup + a.builds):
            t0 = time.perf_counter()
            hrt._lib.check(L.rt_set_triangles_device(ra._h, ptr, m, mats.ctypes.data, len(mats)), "rt_set_triangles_device")
            t1 = time.perf_counter()
            hrt._lib.check(L.rt_refit_triangles_device(ra._h, ptr, m), "rt_refit_triangles_device")
            t2 = time.perf_counter()
            if k >= a.warmup:
                ms["rebuild_ms"].append((t1 - t0) * 1e3)
                ms["refit_ms"].append((t2 - t1) * 1e3)
        res.update({k: spread(v) for k, v in ms.items()})
        res["refit_over_rebuild"] = res["refit_ms"]["median"] / res["rebuild_ms"]["median"]
        # ---- tree quality without a ray: the LBVH and the host's SAH tree of the undeformed mesh
        res["cost_lbvh"] = cost_dict(ra.tri_tree_cost())
        rh = renderer()
        rh.set_params(tri_bvh=1)
        rh.write_bvh(sizes, nodes, tris, mats)
        res["cost_host_sah"] = cost_dict(rh.tri_tree_cost())
        del rh
        # ---- the casts after two deformations
        o, d = (x.view(-1, 3).contiguous() for x in ra.primary_rays(1000))
        renderers = {"refit": ra, "rebuilt": rb}
        hits = {k: torch.empty((n, 8), dtype=torch.int32, device=dev) for k in renderers}
        streams = {k: torch.cuda.ExternalStream(r.stream(), device=dev) for k, r in renderers.items()}
        for kind in ("smooth", "rough"):
            moved = deformed(t0_dev, kind)
            ra.set_triangles_device(t0_dev, mats)
            ra.refit_triangles_device(moved)
            rb.set_triangles_device(moved, mats)
            part = {f"cost_{k}": cost_dict(r.tri_tree_cost()) for k, r in renderers.items()}
            cast_ms = {k: [] for k in renderers}
            for w in range(a.warmup + a.windows):
                for k, r in renderers.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(streams[k])
                    for _ in range(a.casts):
                        hrt._lib.check(L.rt_cast_rays(r._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), n,
                                                      C.c_void_p(hits[k].data_ptr())), "rt_cast_rays")
                    e1.record(streams[k])
                    e1.synchronize()
                    if w >= a.warmup:
                        cast_ms[k].append(e0.elapsed_time(e1) / a.casts)
            for k in renderers:
                part[f"cast_{k}_ms"] = spread(cast_ms[k])
            part["hit_fraction"] = float((hits["refit"][:, 1] >= 0).float().mean())
            part["casts_equal"] = bool((hits["refit"] == hits["rebuilt"]).all())
            part["cast_refit_over_rebuilt"] = part["cast_refit_ms"]["median"] / part["cast_rebuilt_ms"]["median"]
            part["cost_refit_over_rebuilt"] = part["cost_refit"]["sah"] / part["cost_rebuilt"]["sah"]
            ok = ok and part["casts_equal"]
            res[kind] = part
        out["meshes"][name] = res
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
