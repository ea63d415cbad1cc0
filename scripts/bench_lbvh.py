"""What a moving mesh pays per step, and what its rays pay afterwards: rt_set_triangles_device (triangles in device
memory, LBVH built on the GPU) against the host path (Tree.build + rt_set_bvh + the first tri_bvh = 1 query, which
builds and uploads the binned-SAH tree), on Suzanne (979 triangles), lucy_lp_20 (19,917) and xyzrgb_dragon_lp_20
(49,976), each mesh alone in the triangle program.

Per mesh, on one GPU:
  device_build_ms   wall time of one rt_set_triangles_device call (host clock; the call is synchronous), the triangles
                    already in a torch tensor on the device; `--builds` calls on one renderer after `--warmup` untimed ones
  host_path_ms      wall time of Tree.build, of rt_set_bvh (Tree.view + Renderer.write_bvh) and of the first tri_bvh = 1
                    cast of the 1080p primary rays (host clock around a synchronising call), `--host-builds` times, a fresh
                    Tree each time; first_query_ms minus the steady cast below is the SAH build and upload
  cast_*_ms         rt_cast_rays on the width x height primary rays of the frame at time 1000 through the host's SAH tree
                    and through the device's LBVH: device events on each renderer's stream, `--casts` back-to-back calls per
                    window, `--windows` windows alternating between the two trees after `--warmup` untimed ones
  trees             node slots, depth and largest leaf of both trees (rt_testing_get_tri_tree)
Medians with min and max. Outside the timed part the two casts are compared record for record (the hit contract does not
depend on the tree); a difference makes the script exit non-zero. One JSON line.

The builder's leaf size is a compile-time constant. `make -C hello-raytracing_amd leaf1` builds lib/libhrt_leaf1.so with
one triangle per leaf; `HRT_LIB=lib/libhrt_leaf1.so python scripts/bench_lbvh.py --device-only` gives its build and cast
times (the JSON line carries the leaf size it found in the tree).

    python scripts/bench_lbvh.py [--width 1920 --height 1080] [--builds 20] [--host-builds 3] [--casts 20] [--windows 7]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import numpy as np  # noqa: E402

import hrt  # noqa: E402
from hrt import PI, Camera, Material, Mesh, Tree, Vec3, f32, read_asset  # noqa: E402

MESHES = {
    "suzanne": ("suzanne.obj", lambda: hrt.SceneTris.suzane_camera()),
    "lucy_lp_20": ("lucy_lp_20.obj", lambda: Camera.new(Vec3(0.0, 5.0, 6.0), Vec3(0.0, 0.0, -8.0), 5.6, 0.0, PI * f32(0.3))),
    "xyzrgb_dragon_lp_20": ("xyzrgb_dragon_lp_20.obj",
                            lambda: Camera.new(Vec3(0.0, 2.0, 8.0), Vec3(0.0, 0.0, -8.0), 5.6, 0.0, PI * f32(0.3))),
}


def spread(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "samples": len(times)}


def tree_shape(r):
    t = r.tri_tree()
    words = np.concatenate([t["nodes"][:, 3], t["nodes"][:, 7], t["info"][3:4]])
    leaves = words[(words & 0x80000000) != 0]
    return {"node_slots": int(t["info"][0]), "depth": int(t["info"][4]), "leaves": int(len(leaves)),
            "max_leaf": int((leaves & 15).max()) if len(leaves) else 0}


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
    ap.add_argument("--device-only", action="store_true", help="no host path (a comparison library)")
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_lbvh: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    n = a.width * a.height
    out = {"width": a.width, "height": a.height, "rays": n, "library": str(hrt.LIB_PATH.name), "meshes": {}}
    ok = True
    for name in a.meshes.split(","):
        asset, camera = MESHES[name]
        material = Material.new_lambertian(Vec3(0.5, 0.5, 0.6))
        mesh = Mesh.load_obj(read_asset(asset), material)

        def host_tree():
            t = Tree.from_mesh(mesh)
            t.build()
            return t

        sizes, nodes, tris, mats = host_tree().view()
        res = {"triangles": int(len(tris))}
        # ---- the device path
        rd = hrt.Renderer(a.width, a.height, hrt.RT_MODE_TRIS)
        rd.set_params(count_tests=0)
        rd.set_camera(camera())
        dev = torch.device("cuda", rd.device()[0])
        t_dev = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        ms = []
        for k in range(a.warmup + a.builds):
            t0 = time.perf_counter()
            hrt._lib.check(L.rt_set_triangles_device(rd._h, C.c_void_p(t_dev.data_ptr()), len(tris), mats.ctypes.data,
                                                     len(mats)), "rt_set_triangles_device")
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        res["device_build_ms"] = spread(ms)
        res["trees"] = {"device": tree_shape(rd)}
        o, d = (x.view(-1, 3).contiguous() for x in rd.primary_rays(1000))
        renderers = {"device": rd}
        # ---- the host path
        if not a.device_only:
            rh = hrt.Renderer(a.width, a.height, hrt.RT_MODE_TRIS)
            rh.set_params(count_tests=0, tri_bvh=1)
            rh.set_camera(camera())
            parts = {"tree_build_ms": [], "set_bvh_ms": [], "first_query_ms": [], "host_path_ms": []}
            hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
            for k in range(a.host_builds):
                t0 = time.perf_counter()
                tree = host_tree()
                t1 = time.perf_counter()
                rh.write_bvh(*tree.view())
                t2 = time.perf_counter()
                hrt._lib.check(L.rt_cast_rays(rh._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), n,
                                              C.c_void_p(hits.data_ptr())), "rt_cast_rays")
                rh.synchronize()
                t3 = time.perf_counter()
                for key, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                    parts[key].append(v * 1e3)
            res.update({k: spread(v) for k, v in parts.items()})
            res["trees"]["host"] = tree_shape(rh)
            renderers["host"] = rh
        # ---- the casts, alternating
        hits = {k: torch.empty((n, 8), dtype=torch.int32, device=dev) for k in renderers}
        streams = {k: torch.cuda.ExternalStream(r.stream(), device=dev) for k, r in renderers.items()}
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
            res[f"cast_{k}_ms"] = spread(cast_ms[k])
        res["hit_fraction"] = float((hits["device"][:, 1] >= 0).float().mean())
        if "host" in renderers:
            res["casts_equal"] = bool((hits["device"] == hits["host"]).all())
            ok = ok and res["casts_equal"]
            res["sah_build_and_upload_ms"] = res["first_query_ms"]["median"] - res["cast_host_ms"]["median"]
            res["build_speedup"] = res["host_path_ms"]["median"] / res["device_build_ms"]["median"]
            res["cast_device_over_host"] = res["cast_device_ms"]["median"] / res["cast_host_ms"]["median"]
        out["meshes"][name] = res
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
