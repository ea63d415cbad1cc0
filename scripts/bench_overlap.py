"""Rate of rt_overlap_volumes, both kinds, beside rt_closest_points on the same points and tree, for two meshes.

Per mesh (Suzanne, the dragon) on the device LBVH tree, `--queries` (2^20) query positions: random points of the surface
moved by a normal jitter of 2 % of the largest root extent. Boxes are cubes centred there with a side of 1 %, 5 % and 25 %
of that extent, each at k = 0 with counts, k = 4 and k = 16; balls are the same points without a radius cap at k = 1, 8 and
16; rt_closest_points runs on the same points beside the ball k = 1 figure. Timed with device events on the renderer's own
stream (rt_get_stream): back-to-back calls per window, as many as fill `--window-s` seconds (1.0) by the first call's time,
`--windows` windows after `--warmup` untimed ones, the cases alternating window by window. Medians are reported with min
and max, as queries per second. One more call per case runs the counting instantiation (include/hrt_testing.h) for the
triangle and box tests per query; the first 512 queries' records of each case are compared with the host mirror on the
tree read back outside the timed part; a byte that differs from the mirror makes the script exit non-zero.

    python scripts/bench_overlap.py [--queries 1048576] [--window-s 1.0] [--windows 5] > profiles/rNN/bench_overlap.json
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
from hrt import Material, Mesh, Tree, Vec3, read_asset  # noqa: E402

MESHES = {"suzanne": "suzanne.obj", "dragon": "xyzrgb_dragon_lp_20.obj"}
BOX_SIDES = (0.01, 0.05, 0.25)
BOX_KS = {"count": (0, True), "k4": (4, False), "k16": (16, False)}
BALL_KS = {"k1": (1, False), "k8": (8, False), "k16": (16, False)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--window-s", type=float, default=1.0, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--meshes", default=",".join(MESHES))
    a = ap.parse_args()
    if hrt.device_count() == 0:
        raise SystemExit("bench_overlap: no GPU visible (there is no CPU fallback)")
    import torch

    L = hrt.lib()
    P = C.c_void_p
    n = a.queries
    out = {"queries": n, "window_s": a.window_s, "windows": a.windows, "results": []}
    ok = True
    for mesh_name in a.meshes.split(","):
        tree = Tree.from_mesh(Mesh.load_obj(read_asset(MESHES[mesh_name]), Material.new_lambertian(Vec3(0.5, 0.5, 0.5))))
        tree.build()
        view = tree.view()
        tris = view[2].copy()
        v = np.stack([tris[k][:, :3] for k in ("a", "b", "c")], axis=1).astype(np.float64)
        lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
        ext = float((hi - lo).max())
        rng = np.random.default_rng(7)
        j = rng.integers(0, len(v), size=n)
        wts = rng.dirichlet((1.0, 1.0, 1.0), size=n)
        pts = ((v[j] * wts[:, :, None]).sum(axis=1) + rng.normal(size=(n, 3)) * 0.02 * ext).astype(np.float32)
        r = hrt.Renderer(16, 16, hrt.RT_MODE_TRIS)
        r.set_params(count_tests=0)
        dev = torch.device("cuda", r.device()[0])
        raw = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).copy()).to(dev)
        r.set_triangles_device(raw, view[3], builder=0)
        tp = torch.from_numpy(pts).to(dev)
        vols = {}
        for side in BOX_SIDES:
            half = np.float32(0.5 * side * ext)
            vols[f"box{int(round(100 * side))}"] = (hrt.VOLUME_BOX, torch.cat([tp - half, tp + half], dim=1).contiguous())
        vols["ball"] = (hrt.VOLUME_BALL, torch.cat([tp, torch.full((n, 1), hrt.RT_T_MISS, dtype=torch.float32, device=dev)],
                                                   dim=1).contiguous())
        hits = torch.empty((n * 16, 4), dtype=torch.int32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev)
        rec = torch.empty((n, 8), dtype=torch.int32, device=dev)
        stream = torch.cuda.ExternalStream(r.stream(), device=dev)
        cases = [(f"{vn}_{kn}", vn, k, c) for vn in vols if vn != "ball" for kn, (k, c) in BOX_KS.items()]
        cases += [(f"ball_{kn}", "ball", k, c) for kn, (k, c) in BALL_KS.items()] + [("closest_points", None, 0, False)]

        def call(case):
            _, vn, k, counts = case
            if vn is None:
                hrt._lib.check(L.rt_closest_points(r._h, P(tp.data_ptr()), None, n, P(rec.data_ptr())), "rt_closest_points")
                return
            kind, vol = vols[vn]
            hrt._lib.check(L.rt_overlap_volumes(r._h, kind, P(vol.data_ptr()), None, n, k, P(hits.data_ptr()) if k else None,
                                                P(cnt.data_ptr()) if counts else None), "rt_overlap_volumes")

        def window(case, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                call(case)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls  # ms per call

        calls = {}
        for case in cases:  # two untimed calls each; the second one's time settles the number of calls per window
            call(case)  # (the first launch of an instantiation loads it)
            r.synchronize()
            t0 = time.perf_counter()
            call(case)
            r.synchronize()
            calls[case[0]] = max(1, min(4096, int(np.ceil(a.window_s / max(time.perf_counter() - t0, 1e-6)))))
            print(f"{mesh_name} {case[0]}: {1e3 * (time.perf_counter() - t0):.1f} ms for one call", file=sys.stderr, flush=True)
        ms = {c[0]: [] for c in cases}
        for w in range(a.warmup + a.windows):
            for case in cases:
                t = window(case, calls[case[0]])
                if w >= a.warmup:
                    ms[case[0]].append(t)
        info = r.tri_tree_info()
        row = {"mesh": mesh_name, "triangles": int(len(tris)), "tree": "lbvh", "depth": int(info[4]), "queries": n,
               "extent": ext}
        tree_back = r.tri_tree()
        for case in cases:
            name, vn, k, counts = case
            med = statistics.median(ms[name])
            cell = {"queries_per_s": n / (med * 1e-3), "ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]),
                    "samples": len(ms[name]), "calls_per_window": calls[name]}
            if vn is not None:
                kind, vol = vols[vn]
                r.set_overlap_count(True)
                got, gc = r.overlap_records(kind, vol, k, None, counts)
                c = [int(x) for x in r.overlap_counts()]
                r.set_overlap_count(False)
                cell.update(triangle_tests_per_query=c[1] / max(c[0], 1), box_tests_per_query=c[2] / max(c[0], 1),
                            stack_overflows=c[3])
                if counts:
                    cell["triangles_per_query"] = float(gc.to(torch.float64).mean().item())
                want = hrt.overlap_volumes_host(tris, tree_back, kind, vol[:512].cpu().numpy(), k, counts=counts)
                if counts:
                    same = (gc[:512].cpu().numpy().view(np.uint32) == want[1]).all()
                else:
                    same = got[:512].cpu().numpy().tobytes() == want.tobytes()
                cell["equals_host_mirror"] = bool(same)
                ok = ok and bool(same)
            row[name] = cell
        out["results"].append(row)
        r.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
