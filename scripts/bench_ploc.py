"""What the PLOC builder (rt_set_triangles_device_with, RT_TREE_PLOC) costs to build and saves per ray against the LBVH
(RT_TREE_LBVH) and the host's binned-SAH tree (rt_set_bvh with tri_bvh = 1), on Suzanne (979 triangles), lucy_lp_20
(19,917) and xyzrgb_dragon_lp_20 (49,976), each mesh alone in the triangle program (the meshes and cameras of
scripts/bench_lbvh.py).

Per mesh, on one GPU:
  build_lbvh_ms, build_ploc_ms   wall time of one rt_set_triangles_device_with call per builder (host clock; the call is
                         synchronous) on the SAME renderer and the same triangles, already in a torch tensor on the
                         device: `--builds` calls each, alternating, after `--warmup` untimed ones
  build_host_ms          wall time of rt_set_bvh plus the first rt_get_tri_tree_cost (which builds and uploads the SAH
                         tree) on a renderer with tri_bvh = 1: `--host-builds` calls
  tree                   per tree (host_sah, lbvh, ploc): the cost words, sah = (cost[0] + cost[1]) / 65536, the depth and,
                         for ploc, the iterations run and the flat ones among them (rt_get_tri_tree_info)
  cast_*_ms              rt_cast_rays on the width x height primary rays of the frame at time 1000 through each of the three
                         trees (three renderers): device events on each renderer's stream, `--casts` back-to-back calls per
                         window, `--windows` windows alternating between the three after `--warmup` untimed ones
  refit                  the same casts after scripts/bench_refit.py's smooth deformation, refitted, on an LBVH and on a
                         PLOC tree built for the undeformed mesh, with both costs
Medians with min and max. Outside the timed part every pair of casts is compared record for record (the hit contract does
not depend on the tree); a difference makes the script exit non-zero. One JSON line.

    python scripts/bench_ploc.py [--width 1920 --height 1080] [--builds 20] [--casts 20] [--windows 7]
"""
import argparse
import ctypes as C
import json
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
from bench_refit import cost_dict, deformed  # noqa: E402

LBVH, PLOC = 0, 1


def tree_dict(r) -> dict:
    info = [int(x) for x in r.tri_tree_info()]
    return dict(cost_dict(r.tri_tree_cost()), depth=info[4], iterations=info[5], flat=info[6], node_slots=info[1])


def timed_casts(L, renderers, o, d, hits, streams, n, a) -> dict:
    import torch

    ms = {k: [] for k in renderers}
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
                ms[k].append(e0.elapsed_time(e1) / a.casts)
    return {f"cast_{k}_ms": spread(v) for k, v in ms.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--host-builds", type=int, default=3)
    ap.add_argument("--casts", type=int, default=20, help="casts per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--meshes", default=",".join(MESHES))
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_ploc: no GPU visible (there is no CPU fallback)")
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

        rs = {"host_sah": renderer(), "lbvh": renderer(), "ploc": renderer()}
        dev = torch.device("cuda", rs["lbvh"].device()[0])
        t_dev = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).copy()).to(dev).view(torch.float32)
        torch.cuda.synchronize(dev)
        ptr, m = C.c_void_p(t_dev.data_ptr()), len(tris)
        # ---- the two device builds, alternating, on one renderer
        ms = {"build_lbvh_ms": [], "build_ploc_ms": []}
        for k in range(a.warmup + a.builds):
            for key, b in (("build_lbvh_ms", LBVH), ("build_ploc_ms", PLOC)):
                t0 = time.perf_counter()
                hrt._lib.check(L.rt_set_triangles_device_with(rs["ploc"]._h, ptr, m, mats.ctypes.data, len(mats), b),
                               "rt_set_triangles_device_with")
                if k >= a.warmup:
                    ms[key].append((time.perf_counter() - t0) * 1e3)
        # ---- the host path: rt_set_bvh and the SAH tree's build and upload
        rs["host_sah"].set_params(tri_bvh=1)
        ms["build_host_ms"] = []
        for _ in range(a.host_builds):
            t0 = time.perf_counter()
            rs["host_sah"].write_bvh(sizes, nodes, tris, mats)
            rs["host_sah"].tri_tree_cost()
            ms["build_host_ms"].append((time.perf_counter() - t0) * 1e3)
        res.update({k: spread(v) for k, v in ms.items()})
        res["ploc_over_lbvh_build"] = res["build_ploc_ms"]["median"] / res["build_lbvh_ms"]["median"]
        res["host_over_ploc_build"] = res["build_host_ms"]["median"] / res["build_ploc_ms"]["median"]
        # ---- the three trees and the casts through them
        rs["lbvh"].set_triangles_device(t_dev, mats, builder=LBVH)
        rs["ploc"].set_triangles_device(t_dev, mats, builder=PLOC)
        res["tree"] = {k: tree_dict(r) for k, r in rs.items()}
        o, d = (x.view(-1, 3).contiguous() for x in rs["lbvh"].primary_rays(1000))
        hits = {k: torch.empty((n, 8), dtype=torch.int32, device=dev) for k in rs}
        streams = {k: torch.cuda.ExternalStream(r.stream(), device=dev) for k, r in rs.items()}
        res.update(timed_casts(L, rs, o, d, hits, streams, n, a))
        res["hit_fraction"] = float((hits["lbvh"][:, 1] >= 0).float().mean())
        res["casts_equal"] = bool((hits["ploc"] == hits["lbvh"]).all() and (hits["ploc"] == hits["host_sah"]).all())
        res["cast_ploc_over_lbvh"] = res["cast_ploc_ms"]["median"] / res["cast_lbvh_ms"]["median"]
        res["cast_ploc_over_host_sah"] = res["cast_ploc_ms"]["median"] / res["cast_host_sah_ms"]["median"]
        res["cast_lbvh_over_host_sah"] = res["cast_lbvh_ms"]["median"] / res["cast_host_sah_ms"]["median"]
        ok = ok and res["casts_equal"]
        # ---- after a refit: the smooth deformation on both device trees
        two = {k: rs[k] for k in ("lbvh", "ploc")}
        moved = deformed(t_dev, "smooth")
        for r in two.values():
            r.refit_triangles_device(moved)
        part = {"tree": {k: tree_dict(r) for k, r in two.items()}}
        part.update(timed_casts(L, two, o, d, hits, streams, n, a))
        part["casts_equal"] = bool((hits["ploc"] == hits["lbvh"]).all())
        part["cast_ploc_over_lbvh"] = part["cast_ploc_ms"]["median"] / part["cast_lbvh_ms"]["median"]
        ok = ok and part["casts_equal"]
        res["refit"] = part
        out["meshes"][name] = res
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
