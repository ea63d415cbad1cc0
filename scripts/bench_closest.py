"""Rate of rt_closest_points beside rt_cast_rays on the same tree, for three meshes and the three trees a renderer can hold.

Per mesh (Suzanne, lucy, the dragon) a camera looks at the root box from 1.1 radii away; its width x height primary rays
are the yardstick's rays (rt_cast_rays), and give the first of two sets of as many points as rays:
  surface   the hit points of that cast, taken round and round until there are as many as rays, each moved off the
            surface by its own normal-distributed 1 % of the root radius
  volume    uniform in twice the root box
Per tree (RT_TREE_LBVH, RT_TREE_PLOC, the host SAH tree of tri_bvh = 1) the two point sets and the cast are timed with
device events on the renderer's own stream (rt_get_stream): `--calls` back-to-back calls per window, `--windows` windows
after `--warmup` untimed ones, the three alternating window by window. Medians are reported with min and max, as points
(rays) per second. A query reads 12 B and writes 32 B per point. One more call per set runs the counting instantiation
(include/hrt_testing.h) for the triangle tests per query, and the first 512 records of each set are compared with the host
definition outside the timed part; a difference makes the script exit non-zero.

    python scripts/bench_closest.py [--width 1920 --height 1080] [--calls 20] [--windows 7] > profiles/rNN/bench_closest.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "hello-raytracing_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import hrt  # noqa: E402
from hrt import Camera, Material, Mesh, Tree, Vec3, read_asset  # noqa: E402

MESHES = {"suzanne": "suzanne.obj", "lucy": "lucy_lp_20.obj", "dragon": "xyzrgb_dragon_lp_20.obj"}
TREES = ("lbvh", "ploc", "host_sah")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_closest: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    out = {"width": a.width, "height": a.height, "calls_per_window": a.calls, "windows": a.windows, "results": []}
    ok = True
    for mesh_name, asset in MESHES.items():
        tree = Tree.from_mesh(Mesh.load_obj(read_asset(asset), Material.new_lambertian(Vec3(0.5, 0.5, 0.5))))
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
            hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            stream = torch.cuda.ExternalStream(r.stream(), device=dev)

            def call(name):
                if name == "cast":
                    hrt._lib.check(L.rt_cast_rays(r._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), n,
                                                  C.c_void_p(hits.data_ptr())), "rt_cast_rays")
                else:
                    p = sets[name]
                    hrt._lib.check(L.rt_closest_points(r._h, C.c_void_p(p.data_ptr()), None, int(p.shape[0]),
                                                       C.c_void_p(rec.data_ptr())), "rt_closest_points")

            def window(name):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    call(name)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / a.calls  # ms per call

            names = ["surface", "volume", "cast"]
            ms = {k: [] for k in names}
            for w in range(a.warmup + a.windows):
                for name in names:
                    t = window(name)
                    if w >= a.warmup:
                        ms[name].append(t)
            row = {"mesh": mesh_name, "triangles": int(len(tris)), "tree": tree_name,
                   "depth": int(r.tri_tree_info()[4]), "hit_fraction": float(mask.float().mean())}
            for name in names:
                count = n if name == "cast" else int(sets[name].shape[0])
                med = statistics.median(ms[name])
                row[name] = {"count": count, "per_s": count / (med * 1e-3), "ms_median": med, "ms_min": min(ms[name]),
                             "ms_max": max(ms[name]), "samples": len(ms[name])}
            for name, p in sets.items():
                r.set_closest_count(True)
                got = r.closest_records(p)
                c = [int(x) for x in r.closest_counts()]
                r.set_closest_count(False)
                row[name].update(tests_per_query=c[1] / max(c[0], 1), stack_overflows=c[2], uncovered=c[3])
                head = p[:512].cpu().numpy()
                want = hrt.closest_points_host(tris, head)
                same = got[:512].cpu().numpy().tobytes() == want.tobytes()
                row[name]["equals_host_definition"] = same
                ok = ok and same
            out["results"].append(row)
            r.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
