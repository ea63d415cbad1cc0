"""Rate of rt_winding_numbers beside rt_closest_points on the same points and tree, for three meshes and the three trees a
renderer can hold.

Per mesh (Suzanne, lucy, the dragon) the two point sets are scripts/bench_closest.py's: a camera looks at the root box from
1.1 radii away, and its width x height primary rays give
  surface   the hit points of rt_cast_rays on those rays, taken round and round until there are as many as rays, each
            moved off the surface by its own normal-distributed 1 % of the root radius
  volume    uniform in twice the root box
Per tree (RT_TREE_LBVH, RT_TREE_PLOC, the host SAH tree of tri_bvh = 1) and per set, rt_winding_numbers at beta = 2 and
beta = 3 and rt_closest_points (the yardstick) run on all the points, and rt_winding_numbers at beta = +inf — every
triangle for every point — on the first `--exact-points` of them. Timed with device events on the renderer's own stream
(rt_get_stream): `--calls` back-to-back calls per window, `--windows` windows after `--warmup` untimed ones, the calls
alternating window by window. Medians are reported with min and max, as points per second. A winding query reads 12 B and
writes 4 B per point. One more call per set and beta runs the counting instantiation (include/hrt_testing.h) for the
triangle and dipole terms per query; the first 512 answers of each are compared with the host mirror on the tree read back
(rt_testing_get_tri_tree) outside the timed part, and the beta = 2 and 3 answers with the beta = +inf ones on the exact
points (the largest difference is reported); a byte that differs from the mirror makes the script exit non-zero. The
first call's time, which makes the moments, is reported per tree.

    python scripts/bench_winding.py [--width 1920 --height 1080] [--calls 10] [--windows 5] > profiles/rNN/bench_winding.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import hrt  # noqa: E402
from hrt import Camera, Material, Mesh, Tree, Vec3, read_asset  # noqa: E402

MESHES = {"suzanne": "suzanne.obj", "lucy": "lucy_lp_20.obj", "dragon": "xyzrgb_dragon_lp_20.obj"}
TREES = ("lbvh", "ploc", "host_sah")
BETAS = {"beta2": 2.0, "beta3": 3.0, "exact": float("inf")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--exact-points", type=int, default=4096, help="points of the beta = +inf runs")
    ap.add_argument("--meshes", default=",".join(MESHES))
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_winding: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    out = {"width": a.width, "height": a.height, "calls_per_window": a.calls, "windows": a.windows,
           "exact_points": a.exact_points, "results": []}
    ok = True
    for mesh_name in a.meshes.split(","):
        tree = Tree.from_mesh(Mesh.load_obj(read_asset(MESHES[mesh_name]), Material.new_lambertian(Vec3(0.5, 0.5, 0.5))))
        tree.build()
        view = tree.view()
        tris = view[2].copy()
        v = np.stack([tris[k][:, :3] for k in ("a", "b", "c")], axis=1).astype(np.float64)
        lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
        centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
        eye = centre + np.array([0.0, 0.15, 1.1]) * radius
        cam = Camera.new(Vec3(*eye.tolist()), Vec3(*centre.tolist()), 1.1 * radius, 0.0, hrt.PI * hrt.f32(0.3))
        for tree_name in TREES:
            r = hrt.Renderer(a.width, a.height, hrt.RT_MODE_TRIS)
            r.set_params(count_tests=0)
            r.set_camera(cam)
            dev = torch.device("cuda", r.device()[0])
            if tree_name == "host_sah":
                r.write_bvh(*view)
                r.set_params(tri_bvh=1)
            else:
                raw = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).copy()).to(dev)
                r.set_triangles_device(raw, view[3], builder=TREES.index(tree_name))
            o, d = (x.view(-1, 3).contiguous() for x in r.primary_rays(1000))
            n = int(o.shape[0])
            ne = min(a.exact_points, n)
            hit = r.cast_rays(o, d)
            mask = hit["prim"] >= 0
            gen = torch.Generator().manual_seed(20261021)
            jitter = (torch.randn((n, 3), generator=gen) * (0.01 * radius)).to(dev)
            on = o[mask] + hit["t"][mask][:, None] * d[mask]
            surface = (on[torch.arange(n, device=dev) % on.shape[0]] + jitter).contiguous()
            box = torch.rand((n, 3), generator=gen, dtype=torch.float64) * 2.0 - 1.0
            volume = (torch.from_numpy(centre) + box * torch.from_numpy(hi - lo)).to(torch.float32).to(dev).contiguous()
            sets = {"surface": surface, "volume": volume}
            rec = torch.empty((n, 8), dtype=torch.int32, device=dev)
            w = torch.empty((n,), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r.winding_numbers(surface[:64])  # the first call makes the moments
            first_ms = (time.perf_counter() - t0) * 1e3
            stream = torch.cuda.ExternalStream(r.stream(), device=dev)

            def call(name):
                s, what = name.split("/")
                p = sets[s]
                if what == "closest":
                    hrt._lib.check(L.rt_closest_points(r._h, C.c_void_p(p.data_ptr()), None, n, C.c_void_p(rec.data_ptr())),
                                   "rt_closest_points")
                else:
                    hrt._lib.check(L.rt_winding_numbers(r._h, C.c_void_p(p.data_ptr()), ne if what == "exact" else n,
                                                        BETAS[what], C.c_void_p(w.data_ptr())), "rt_winding_numbers")

            def window(name):
                calls = 1 if name.endswith("/exact") else a.calls
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    call(name)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / calls  # ms per call

            names = [f"{s}/{what}" for s in sets for what in ("beta2", "beta3", "exact", "closest")]
            ms = {k: [] for k in names}
            for k in range(a.warmup + a.windows):
                for name in names:
                    t = window(name)
                    if k >= a.warmup:
                        ms[name].append(t)
            info = r.tri_tree_info()
            row = {"mesh": mesh_name, "triangles": int(len(tris)), "tree": tree_name, "depth": int(info[4]),
                   "node_slots": int(info[1]), "first_call_ms": first_ms}
            tree_back = r.tri_tree()
            for s, p in sets.items():
                row[s] = {}
                exact = None
                for what in ("exact", "beta2", "beta3", "closest"):
                    name = f"{s}/{what}"
                    count = ne if what == "exact" else n
                    med = statistics.median(ms[name])
                    cell = {"count": count, "per_s": count / (med * 1e-3), "ms_median": med, "ms_min": min(ms[name]),
                            "ms_max": max(ms[name]), "samples": len(ms[name])}
                    if what != "closest":
                        r.set_winding_count(True)
                        got = r.winding_numbers(p[:count], BETAS[what])
                        c = [int(x) for x in r.winding_counts()]
                        r.set_winding_count(False)
                        cell.update(triangle_terms_per_query=c[1] / max(c[0], 1), dipole_terms_per_query=c[2] / max(c[0], 1),
                                    stack_overflows=c[3], uncovered=c[4])
                        head = p[:512].cpu().numpy()
                        same = got[:512].cpu().numpy().tobytes() == hrt.winding_numbers_host(tris, tree_back, head, BETAS[what]).tobytes()
                        cell["equals_host_mirror"] = same
                        ok = ok and same
                        if what == "exact":
                            exact = got
                        else:
                            cell["max_abs_diff_to_exact"] = float((got[:ne] - exact).abs().max())
                    row[s][what] = cell
            out["results"].append(row)
            r.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
