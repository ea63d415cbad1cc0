"""Rate of rt_cast_rays_multi beside rt_cast_rays on the same rays and tree, for three meshes and the three trees a renderer
can hold.

Per mesh (Suzanne, lucy, the dragon) a camera looks at the root box from 1.1 radii away (scripts/bench_closest.py's), and
its width x height primary rays are the rays. Per tree (RT_TREE_LBVH, RT_TREE_PLOC, the host SAH tree of tri_bvh = 1):
rt_cast_rays_multi with k = 1, 4 and 16 without counts, k = 0 with counts (counts only), and rt_cast_rays (the yardstick)
run on all the rays. Timed with device events on the renderer's own stream (rt_get_stream): `--calls` back-to-back calls
per window, `--windows` windows after `--warmup` untimed ones, the calls alternating window by window. Medians are
reported with min and max, as rays per second. Renderer.all_hits (a counting call, then pages of 16 with host-side
bookkeeping in torch) is timed by the host clock around the whole call, synchronised, `--windows` times. One more call
per k runs the counting instantiation (include/hrt_testing.h) for the triangle and box tests per ray; the first 512 rays'
records of each k are compared with the host mirror on the tree read back (rt_testing_get_tri_tree) outside the timed
part; a byte that differs from the mirror makes the script exit non-zero.

    python scripts/bench_multihit.py [--width 1920 --height 1080] [--calls 10] [--windows 5] > profiles/rNN/bench_multihit.json
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
KS = {"k1": (1, False), "k4": (4, False), "k16": (16, False), "count": (0, True)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--meshes", default=",".join(MESHES))
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_multihit: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    P = C.c_void_p
    out = {"width": a.width, "height": a.height, "calls_per_window": a.calls, "windows": a.windows, "results": []}
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
            hits = torch.empty((n * 16, 4), dtype=torch.int32, device=dev)
            cnt = torch.empty((n,), dtype=torch.int32, device=dev)
            rec = torch.empty((n, 8), dtype=torch.int32, device=dev)
            r.cast_rays_multi(o[:64], d[:64], 1)  # (a host SAH tree is built by the first query)
            stream = torch.cuda.ExternalStream(r.stream(), device=dev)
            po, pd = P(o.data_ptr()), P(d.data_ptr())

            def call(name):
                if name == "cast_rays":
                    hrt._lib.check(L.rt_cast_rays(r._h, po, pd, n, P(rec.data_ptr())), "rt_cast_rays")
                    return
                k, counts = KS[name]
                hrt._lib.check(L.rt_cast_rays_multi(r._h, po, pd, None, None, n, k, P(hits.data_ptr()) if k else None,
                                                    P(cnt.data_ptr()) if counts else None), "rt_cast_rays_multi")

            def window(name):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    call(name)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / a.calls  # ms per call

            names = list(KS) + ["cast_rays"]
            ms = {k: [] for k in names}
            for w in range(a.warmup + a.windows):
                for name in names:
                    t = window(name)
                    if w >= a.warmup:
                        ms[name].append(t)
            all_ms, total_hits, most = [], 0, 0
            for w in range(a.warmup + a.windows):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                offsets = r.all_hits(o, d)[0]
                torch.cuda.synchronize(dev)
                if w >= a.warmup:
                    all_ms.append((time.perf_counter() - t0) * 1e3)
                total_hits, most = int(offsets[-1].item()), int((offsets[1:] - offsets[:-1]).max().item())
            info = r.tri_tree_info()
            row = {"mesh": mesh_name, "triangles": int(len(tris)), "tree": tree_name, "depth": int(info[4]), "rays": n,
                   "hits_in_all": total_hits, "most_hits_on_a_ray": most}
            tree_back = r.tri_tree()
            head_o, head_d = o[:512].cpu().numpy(), d[:512].cpu().numpy()
            for name in names:
                med = statistics.median(ms[name])
                cell = {"rays_per_s": n / (med * 1e-3), "ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]),
                        "samples": len(ms[name])}
                if name != "cast_rays":
                    k, counts = KS[name]
                    r.set_multihit_count(True)
                    got, gc = r.cast_rays_multi_records(o, d, k, None, None, counts)
                    c = [int(x) for x in r.multihit_counts()]
                    r.set_multihit_count(False)
                    cell.update(triangle_tests_per_ray=c[1] / max(c[0], 1), box_tests_per_ray=c[2] / max(c[0], 1),
                                stack_overflows=c[3])
                    want = hrt.cast_rays_multi_host(tris, tree_back, head_o, head_d, k, counts=counts)
                    if counts:
                        same = (gc[:512].cpu().numpy().view(np.uint32) == want[1]).all()
                    else:
                        same = got[:512].cpu().numpy().tobytes() == want.tobytes()
                    cell["equals_host_mirror"] = bool(same)
                    ok = ok and bool(same)
                row[name] = cell
            med = statistics.median(all_ms)
            row["all_hits"] = {"rays_per_s": n / (med * 1e-3), "ms_median": med, "ms_min": min(all_ms), "ms_max": max(all_ms),
                               "samples": len(all_ms), "timed_with": "host clock, synchronised"}
            out["results"].append(row)
            r.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
